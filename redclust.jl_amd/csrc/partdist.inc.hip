// Partition distances: everything the Binder loss, the VI and the information distance between each of L labellings and each
// of m posterior samples need, as exact integers, on the device — the rectangle L×m that credible balls and exact expected
// losses are made of (rc_loss_matrix is the square m×m, in f64).  DESIGN.md §8 "Partition distances"; the contract is in
// include/redclust_hip.h.  Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, the holders,
// select_device and cluster_order of hostutil.inc.hip, and visearch::gtable — the one fixed-point table of the library).
//
// For labelling c and sample z with contingency table N_kl = #{j : c_j = k, z_j = l} the kernel returns
//   P = Σ_kl N_kl²   and   T = Σ_kl Phiq(N_kl),   Phiq(x) = Σ_{y<x} Gq[y];
// the marginals (Σ n_k², Σ Phiq(n_k), K of every labelling and of every sample) are summed on the host.
//
// Host: every labelling and sample is compacted to dense u16 ids, and every sample's points are sorted by cluster
// (cluster_order, the routine predict uses): ord[s][t] = point index, bit 15 set on the last point of its cluster.
//
// k_partdist: one workgroup of WPB waves per (sample, block of WPB labellings), one wave per labelling.  The sample's order
// is staged in LDS once per workgroup.  A wave walks it 64 positions at a time and stops each step at the first end-of-
// cluster mark (a ballot), so a step never spans two of the sample's clusters.  Every lane adds 1 to the wave's histogram
// cell of its point's labelling id with a returning atomic: the old count c is how many points of this (k, l) cell came
// before, so N² grows by 2c + 1 and Phiq(N) by Gq[c] — both sums need no pass over the cells, and their order of arrival
// does not matter because every cell sees the counts 0, 1, …, N − 1 exactly once.  At a cluster's end the wave walks the
// cluster again and stores zeros, which leaves the histogram ready for the next cluster, the next work item and (the global
// one) the next launch.  c never exceeds the largest cluster of the sample, so only that many entries of Gq are ever read:
// when they fit GQ_LDS_BYTES for every sample of a chunk the workgroup copies them to LDS (GQLDS), else — a sample with one
// huge cluster, or RC_PARTDIST_GQ_GLOBAL=1 — the table is read from global memory through the caches.
// Histogram: u32[KLDS] per wave in LDS for labellings of at most KLDS = 1024 clusters; labellings with more (or all, with
// RC_PARTDIST_HIST_GLOBAL=1) run in a second pass whose histograms are in global memory, one u32[n] per resident wave —
// that pass's grid is capped and its workgroups loop over the work items.  The integers are the same either way.

namespace partdist {

constexpr int64_t LMAX = 65536;
constexpr int WPB = 8, TPB = WPB * 64;          // labellings (waves) per workgroup
constexpr int KLDS = 1024;                      // cells of a wave's LDS histogram
constexpr size_t WORKSPACE = (size_t)1 << 30;   // device bytes of one chunk: half for the samples' orders, half for what scales with labellings
constexpr int GLOBAL_GRID_MAX = 1024;           // workgroups of the global-histogram pass
constexpr size_t GQ_LDS_BYTES = 16 * 1024;      // the most of Gq a workgroup copies to LDS (2048 entries)

struct Args {
    const unsigned short *ord;      // [mc][npad]
    const unsigned short *lab;      // [Lc][n] dense ids
    const long long *Gq;            // [n]
    unsigned *hist;                 // HGLOBAL: [gridDim.x·WPB][hstride], zero between launches
    long long *sq, *phi;            // [Lc][mc], either may be null
    int n, npad, mc, Lc, hstride;
    int gcap;                       // GQLDS: entries of Gq copied to LDS (even; above every count the chunk's samples can reach)
    long long items;                // mc · ceil(Lc / WPB); item = block·mc + sample
};

template <bool HGLOBAL> __device__ __forceinline__ void zero_cell(unsigned *p)
{
    if (HGLOBAL) atomicExch(p, 0u);             // through the same path as the adds
    else *p = 0u;
}

// dynamic LDS: the order u16[npad] | GQLDS: Gq i64[gcap] | !HGLOBAL: the histograms u32[WPB][KLDS]
template <bool HGLOBAL, bool GQLDS>
__global__ __launch_bounds__(TPB) void k_partdist(const Args A)
{
    extern __shared__ __align__(16) unsigned char pd_lds[];
    unsigned short *ord = reinterpret_cast<unsigned short *>(pd_lds);
    const int n = A.n, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned *h;
    if constexpr (HGLOBAL) {
        h = A.hist + ((size_t)blockIdx.x * WPB + wave) * (size_t)A.hstride;
    } else {
        h = reinterpret_cast<unsigned *>(pd_lds + (size_t)A.npad * 2 + (GQLDS ? (size_t)A.gcap * 8 : 0)) + wave * KLDS;
        for (int k = lane; k < KLDS; k += 64) h[k] = 0u;
    }
    const long long *Gq;
    if constexpr (GQLDS) {
        long long *g = reinterpret_cast<long long *>(pd_lds + (size_t)A.npad * 2);
        for (int x = threadIdx.x; x < A.gcap; x += TPB) g[x] = A.Gq[x];       // read behind the first barrier below
        Gq = g;
    } else {
        Gq = A.Gq;
    }
    for (long long item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int s = (int)(item % A.mc), l = (int)(item / A.mc) * WPB + wave;
        const uint4 *src = reinterpret_cast<const uint4 *>(A.ord + (size_t)s * A.npad);
        for (int j = threadIdx.x; j < A.npad / 8; j += TPB) reinterpret_cast<uint4 *>(ord)[j] = src[j];
        __syncthreads();
        if (l < A.Lc) {
            const unsigned short *__restrict__ lab = A.lab + (size_t)l * n;
            unsigned long long P = 0, T = 0;
            int a = 0, pos = 0;                                      // the current cluster's first position, the next position
            while (pos < n) {
                const int i = pos + lane;
                const unsigned e = i < n ? ord[i] : 0u;
                // position n − 1 carries a mark, so a step that reaches the end of the order stops there at the latest
                const unsigned long long ends = __ballot((e & 0x8000u) != 0u);
                const int f = ends ? __ffsll(ends) - 1 : 63;         // the step's last lane
                const bool act = lane <= f;
                unsigned id = 0;
                if (act) {
                    id = lab[e & 0x7FFFu];
                    const unsigned c = atomicAdd(h + id, 1u);
                    P += 2ull * c + 1ull;
                    T += (unsigned long long)Gq[c];
                }
                if (ends) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    for (int k = a + lane; k < pos; k += 64) zero_cell<HGLOBAL>(h + lab[ord[k] & 0x7FFFu]);
                    if (act) zero_cell<HGLOBAL>(h + id);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    a = pos + f + 1;
                }
                pos += f + 1;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                P += __shfl_xor(P, off);
                T += __shfl_xor(T, off);
            }
            if (lane == 0) {
                const size_t o = (size_t)l * A.mc + s;
                if (A.sq) A.sq[o] = (long long)P;
                if (A.phi) A.phi[o] = (long long)T;
            }
        }
        __syncthreads();                                             // the next item replaces the order
    }
}

// The marginals of one row: Σ n_k², Σ Phiq(n_k), K.  cnt: n + 1 zeros, left zeroed; id: n + 1 scratch.
static void marginals(const int64_t *z, int64_t n, const int64_t *Phi, std::vector<int> &cnt, std::vector<int> &id, int64_t *marg)
{
    int64_t sq = 0, ph = 0;
    marg[2] = compact_labels(z, n, cnt, id, [&](int, int64_t, int sz) { sq += (int64_t)sz * sz; ph += Phi[(size_t)sz]; });
    marg[0] = sq; marg[1] = ph;
}

// One pass: the labellings idx[0..count) (rows of `labels`) against every sample, with the LDS or the global histograms.
struct Pass {
    const char *who;
    int64_t n, m, npad;
    const int64_t *samples, *labels;
    const long long *d_Gq;
    int64_t *sq_out, *phi_out;
    size_t workspace;
    bool gq_global;
};

static int32_t run_pass(const Pass &p, const std::vector<int64_t> &idx, bool hglobal, double &ms_acc)
{
    const int64_t n = p.n, m = p.m, npad = p.npad, count = (int64_t)idx.size();
    if (!count || (!p.sq_out && !p.phi_out)) return RC_OK;
    // Chunks.  Samples: their orders take half the workspace.  Labellings: ids (2n bytes) and two outputs per sample of the chunk.
    const int64_t mc = std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(p.workspace / 2 / (2 * (size_t)npad))));
    const size_t per_lab = 2 * (size_t)n + 16 * (size_t)mc;
    const int64_t Lc = std::max<int64_t>(1, std::min<int64_t>(count, (int64_t)(p.workspace / 2 / per_lab)));
    const long long max_items = (long long)mc * ((Lc + WPB - 1) / WPB);
    // the global histograms: one u32[n] per resident wave, within a quarter of the workspace (one workgroup at the least)
    const int grid_global = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(GLOBAL_GRID_MAX, max_items),
                                                                           (long long)(p.workspace / 4 / ((size_t)WPB * 4 * (size_t)n))));
    std::vector<unsigned short> h_ord, h_lab;
    std::vector<long long> h_sq, h_phi;
    std::vector<int> cnt, slot_of_label, pos, id;
    try {
        h_ord.assign((size_t)mc * npad, 0); h_lab.resize((size_t)Lc * n);
        if (p.sq_out) h_sq.resize((size_t)Lc * mc);
        if (p.phi_out) h_phi.resize((size_t)Lc * mc);
        cnt.assign((size_t)n + 1, 0); slot_of_label.assign((size_t)n + 1, 0); pos.assign((size_t)n, 0); id.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for a chunk of %lld samples and %lld labellings", p.who, (long long)mc, (long long)Lc); }

    DeviceBuffers B;
    unsigned short *d_ord, *d_lab; unsigned *d_hist = nullptr; long long *d_sq = nullptr, *d_phi = nullptr;
    HIPCHK(nullptr, B.alloc(d_ord, h_ord.size()));
    HIPCHK(nullptr, B.alloc(d_lab, h_lab.size()));
    if (p.sq_out) HIPCHK(nullptr, B.alloc(d_sq, (size_t)Lc * mc));
    if (p.phi_out) HIPCHK(nullptr, B.alloc(d_phi, (size_t)Lc * mc));
    if (hglobal) {
        HIPCHK(nullptr, B.alloc(d_hist, (size_t)grid_global * WPB * (size_t)n));
        HIPCHK(nullptr, hipMemset(d_hist, 0, (size_t)grid_global * WPB * (size_t)n * sizeof(unsigned)));   // once: the kernel leaves zeros behind
    }
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());

    for (int64_t s0 = 0; s0 < m; s0 += mc) {
        const int64_t ms = std::min(mc, m - s0);
        int cmax = 0;                                                         // the chunk's largest cluster
        for (int64_t s = 0; s < ms; ++s) {
            unsigned short *o = h_ord.data() + (size_t)s * npad;
            const int K = cluster_order(p.samples + (size_t)(s0 + s) * n, n, cnt, slot_of_label, pos,
                                        [&](int, int64_t, int sz) { cmax = std::max(cmax, sz); },
                                        [&](int at, int64_t j, int) { o[at] = (unsigned short)j; });
            for (int t = 0; t < K; ++t) o[pos[(size_t)t] - 1] |= 0x8000u;     // the last point of every cluster
        }
        HIPCHK(nullptr, hipMemcpy(d_ord, h_ord.data(), (size_t)ms * npad * sizeof(unsigned short), hipMemcpyHostToDevice));
        // counts reach cmax − 1 at the most, so Gq[0 .. cmax) is all the chunk reads (cmax <= n entries exist)
        const int gcap = (int)std::min<int64_t>(n, (cmax + 1) / 2 * 2);
        const bool gqlds = !p.gq_global && (size_t)gcap * 8 <= GQ_LDS_BYTES;
        const size_t lds = (size_t)npad * 2 + (gqlds ? (size_t)gcap * 8 : 0) + (hglobal ? 0 : (size_t)WPB * KLDS * sizeof(unsigned));
        auto kern = hglobal ? (gqlds ? k_partdist<true, true> : k_partdist<true, false>) : (gqlds ? k_partdist<false, true> : k_partdist<false, false>);
        HIPCHK(nullptr, set_dynamic_lds(kern, lds));
        for (int64_t l0 = 0; l0 < count; l0 += Lc) {
            const int64_t nl = std::min(Lc, count - l0);
            for (int64_t l = 0; l < nl; ++l) {
                const int64_t *z = p.labels + (size_t)idx[(size_t)(l0 + l)] * n;
                compact_labels(z, n, cnt, id, [](int, int64_t, int) {});
                dense_ids(z, n, id, h_lab.data() + (size_t)l * n);
            }
            HIPCHK(nullptr, hipMemcpy(d_lab, h_lab.data(), (size_t)nl * n * sizeof(unsigned short), hipMemcpyHostToDevice));
            Args a{};
            a.ord = d_ord; a.lab = d_lab; a.Gq = p.d_Gq; a.hist = d_hist; a.sq = d_sq; a.phi = d_phi;
            a.n = (int)n; a.npad = (int)npad; a.mc = (int)ms; a.Lc = (int)nl; a.hstride = (int)n; a.gcap = gqlds ? gcap : 0;
            a.items = (long long)ms * ((nl + WPB - 1) / WPB);
            const unsigned grid = (unsigned)(hglobal ? std::min<long long>(grid_global, a.items) : a.items);
            HIPCHK(nullptr, ev.begin(0));
            kern<<<grid, TPB, lds, 0>>>(a);
            HIPCHK(nullptr, ev.end(0));
            HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
            // device [nl][ms] into the caller's [L][m]
            for (int pass = 0; pass < 2; ++pass) {
                int64_t *dst = pass ? p.phi_out : p.sq_out;
                if (!dst) continue;
                long long *h = pass ? h_phi.data() : h_sq.data();
                HIPCHK(nullptr, hipMemcpy(h, pass ? d_phi : d_sq, (size_t)nl * ms * sizeof(long long), hipMemcpyDeviceToHost));
                for (int64_t l = 0; l < nl; ++l)
                    memcpy(dst + (size_t)idx[(size_t)(l0 + l)] * m + s0, h + (size_t)l * ms, (size_t)ms * sizeof(int64_t));
            }
        }
    }
    return RC_OK;
}

}  // namespace partdist

extern "C" int32_t rc_partition_distances(int32_t device, const int64_t *samples, int64_t m, int64_t n, int64_t L, const int64_t *labels,
                                          int64_t *sq_out, int64_t *phi_out, int64_t *lab_marg, int64_t *smp_marg, double *kernel_ms)
{
    using namespace partdist;
    const char *who = "rc_partition_distances";
    if (!samples || !labels) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (m < 1 || n < 1 || L < 1) return fail(nullptr, RC_ERR_ARG, "%s: need m >= 1, n >= 1 and L >= 1 (got m=%lld n=%lld L=%lld)", who, (long long)m, (long long)n, (long long)L);
    int32_t rc = check_label_shape(nullptr, who, n, "points", m, "m");   // u16 point indices with bit 15 free for the end-of-cluster mark
    if (rc != RC_OK) return rc;
    if (L > LMAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: L = %lld exceeds %lld labellings per call", who, (long long)L, (long long)LMAX);
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(nullptr, who, "labelling", labels, L, n);
    if (rc != RC_OK) return rc;

    std::vector<int64_t> Gq, Phi, lmarg, idx_lds, idx_global;
    std::vector<int> cnt, id;
    try {
        Gq.resize((size_t)n); Phi.resize((size_t)n + 1); lmarg.resize((size_t)L * 3);
        cnt.assign((size_t)n + 1, 0); id.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    visearch::gtable(n, Gq.data());
    Phi[0] = 0;
    for (int64_t x = 0; x < n; ++x) Phi[(size_t)x + 1] = Phi[(size_t)x] + Gq[(size_t)x];
    const bool force_global = env_flag("RC_PARTDIST_HIST_GLOBAL");          // tests: the global histograms at every cluster count
    for (int64_t l = 0; l < L; ++l) {
        marginals(labels + (size_t)l * n, n, Phi.data(), cnt, id, lmarg.data() + (size_t)l * 3);
        (force_global || lmarg[(size_t)l * 3 + 2] > KLDS ? idx_global : idx_lds).push_back(l);
    }
    if (lab_marg) memcpy(lab_marg, lmarg.data(), lmarg.size() * sizeof(int64_t));
    if (smp_marg)
        for (int64_t s = 0; s < m; ++s) marginals(samples + (size_t)s * n, n, Phi.data(), cnt, id, smp_marg + (size_t)s * 3);
    if (kernel_ms) *kernel_ms = 0.0;
    if (!sq_out && !phi_out) return RC_OK;

    rc = select_device(who, device);
    if (rc != RC_OK) return rc;
    const size_t workspace = env_workspace_kib("RC_PARTDIST_WORKSPACE_KIB", WORKSPACE);
    DeviceBuffers B;
    long long *d_Gq;
    HIPCHK(nullptr, B.alloc(d_Gq, (size_t)n));
    HIPCHK(nullptr, hipMemcpy(d_Gq, Gq.data(), (size_t)n * sizeof(long long), hipMemcpyHostToDevice));
    const Pass p{who, n, m, (n + 7) / 8 * 8, samples, labels, d_Gq, sq_out, phi_out, workspace,
                 env_flag("RC_PARTDIST_GQ_GLOBAL")};                        // tests: the table from global memory for every chunk
    double ms_acc = 0.0;
    rc = run_pass(p, idx_lds, false, ms_acc);
    if (rc != RC_OK) return rc;
    rc = run_pass(p, idx_global, true, ms_acc);
    if (rc != RC_OK) return rc;
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

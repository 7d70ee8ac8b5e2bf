// The slab driver: per-cluster sums of rows against many labellings at once, the machine under predict (predict.inc.hip), the
// joint predict (predictjoint.inc.hip), the scoring of labellings (score.inc.hip) and the cluster profiles (profile.inc.hip).
// DESIGN.md §8 "The slab driver".  Included at the end of redclust_hip.hip ahead of those four (same translation unit: shares
// fail(), HIPCHK, View, make_view, the holders and set_dynamic_lds of hostutil.inc.hip, cluster_order of labels.inc.hpp and
// slab_plan of slabplan.inc.hpp).
//
// A labelling is a row of n labels in 1..n: a posterior sample for the predicts, any partition for the other two.  A row is n
// interleaved (Dq, Lq) pairs of fixed-point integers, 16 bytes per point: a new observation's distances to the training points
// (the predicts, quantised on the host) or a row of a context's matrices in the caller's order (score and profiles, gathered on
// the device by their staging kernels).  The slab is sums[row][slot] = Σ_{j in slot} (Dq, Lq)[row][j], exact int64, for every
// slot of every labelling of a chunk; what is done with it is the caller's consumer kernel.
//
// An entry point: checks the matrix of labellings (check_label_shape, check_label_rows of hostutil.inc.hip), counts every
// labelling's clusters (count_clusters of labels.inc.hpp), cuts the labellings into chunks that fit its workspace (slab_plan)
// and, per chunk, builds the sorted orders (Orders::build, Orders::upload) and sends the rows through k_predict_sums
// (Orders::launch_sums) to its consumer; run_rows is that last step for the rows of a context.
//
// Host, per labelling (Orders::build): the labels are compacted to slots 0..K-1 in ascending label order and the points are
// sorted by slot (counting sort).  The sorted order is stored transposed, perm[j][s] (u16: point index, bit 15 set on the last
// point of its slot), so 64 lanes that own 64 consecutive labellings read 128 contiguous bytes per step.  On request the dense
// slot of every point, rslot[s][i], is filled in the same pass.
//
// k_predict_sums (the rows·labellings·n integer adds): one workgroup per row.  The row is staged in LDS, so one 128-bit LDS
// gather fetches both addends; rows beyond the LDS (n > 10240) or the entry point's RC_*_ROWS_GLOBAL=1 gather from global memory
// instead — the same integers.  A lane owns (labelling, part of the sorted order), adds into two int64 registers and at every
// slot boundary flushes them to the (row, labelling, slot) sums: a plain store when a labelling is one part (at least TPB1
// labellings, padded to 64, in the chunk), 64-bit integer atomic adds into zeros when the workgroup has more lanes than
// labellings and cuts every labelling into parts (exact in any order).

namespace slab {

constexpr size_t WORKSPACE = (size_t)1 << 30;   // device bytes per chunk that scale with the number of rows
constexpr size_t PERM_BYTES = (size_t)1 << 29;  // ... and the most the sorted orders of one chunk of labellings take
constexpr int64_t KMAX = 4096;                  // clusters of one labelling where a consumer keeps per-cluster state in LDS

}  // namespace slab

namespace prd {

constexpr int TPB1 = 1024;
constexpr int64_t LDS_ROW_MAX_N = 160 * 1024 / 16;

template <bool ATOMIC> __device__ __forceinline__ void flush(ll2 *o, long long sd, long long sl)
{
    if (ATOMIC) {
        atomicAdd((u64 *)o, (u64)sd);
        atomicAdd((u64 *)o + 1, (u64)sl);
    } else {
        ll2 v; v.x = sd; v.y = sl;
        *o = v;
    }
}

// The walk of one row (in LDS or global memory) through the sorted orders of ms labellings: perm: [n][ms_pad]; koff: [ms] first
// slot of every labelling; startslot: [parts][ms_pad] slot of a part's first position (ATOMIC only); out: the row's [ktot] sums.
template <bool ATOMIC>
__device__ __forceinline__ void walk_sums(const ll2 *__restrict__ row, int n, const unsigned short *__restrict__ perm, int ms, int ms_pad, int parts,
                                          const int *__restrict__ startslot, const long long *__restrict__ koff, ll2 *__restrict__ out)
{
    for (int w = threadIdx.x; w < ms_pad * parts; w += blockDim.x) {
        const int part = w / ms_pad, s = w - part * ms_pad;
        if (s >= ms) continue;
        const int j0 = (int)((long long)part * n / parts), j1 = (int)((long long)(part + 1) * n / parts);
        ll2 *o = out + koff[s] + (ATOMIC ? startslot[w] : 0);
        const unsigned short *pp = perm + (size_t)j0 * (size_t)ms_pad + s;
        long long sd = 0, sl = 0;
        unsigned e = 0x8000u;
        // Batches of NB steps: the NB entries of the sorted order are requested one batch ahead and the NB row gathers are
        // issued together, so a lane waits once per batch for either memory, not once per step — a flush is a branch, and
        // across a branch the compiler keeps no load in flight.  (The prefetch past the part's end re-reads its last entry.)
        constexpr int NB = 8;
        unsigned en[NB];
        int j = j0;
        if (j + NB <= j1) {
#pragma unroll
            for (int u = 0; u < NB; ++u) en[u] = pp[(size_t)u * ms_pad];
        }
        for (; j + NB <= j1; j += NB) {
            unsigned ec[NB];
            ll2 v[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) ec[u] = en[u];
#pragma unroll
            for (int u = 0; u < NB; ++u) en[u] = pp[(size_t)(min(j + NB + u, j1 - 1) - j) * ms_pad];
#pragma unroll
            for (int u = 0; u < NB; ++u) v[u] = row[ec[u] & 0x7FFFu];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                sd += v[u].x; sl += v[u].y;
                if (ec[u] & 0x8000u) { flush<ATOMIC>(o, sd, sl); ++o; sd = 0; sl = 0; }
            }
            e = ec[NB - 1];
            pp += (size_t)NB * ms_pad;
        }
        for (; j < j1; ++j, pp += ms_pad) {
            e = *pp;
            const ll2 v = row[e & 0x7FFFu];
            sd += v.x; sl += v.y;
            if (e & 0x8000u) { flush<ATOMIC>(o, sd, sl); ++o; sd = 0; sl = 0; }
        }
        if (ATOMIC && !(e & 0x8000u)) flush<ATOMIC>(o, sd, sl);   // the part ends inside a slot
    }
}

// rows: [points][n] (Dq, Lq); sums: [points][ktot]; the rest as walk_sums.  Grid: one block per point.
template <bool LDSROW, bool ATOMIC>
__global__ __launch_bounds__(TPB1) void k_predict_sums(const ll2 *__restrict__ rows, int n, const unsigned short *__restrict__ perm, int ms, int ms_pad,
                                                       int parts, const int *__restrict__ startslot, const long long *__restrict__ koff, long long ktot,
                                                       ll2 *__restrict__ sums)
{
    extern __shared__ __align__(16) unsigned char prd_lds[];
    const ll2 *grow = rows + (size_t)blockIdx.x * (size_t)n;
    const ll2 *row = grow;
    if (LDSROW) {
        ll2 *l = reinterpret_cast<ll2 *>(prd_lds);
        for (int j = threadIdx.x; j < n; j += blockDim.x) l[j] = grow[j];
        __syncthreads();
        row = l;
    }
    walk_sums<ATOMIC>(row, n, perm, ms, ms_pad, parts, startslot, koff, sums + (size_t)blockIdx.x * (size_t)ktot);
}

// The sorted orders of a chunk of labellings on the host and the device, and the launch of k_predict_sums over them.
struct Orders {
    int64_t n = 0, ms = 0;
    int ms_pad = 0, parts = 1;
    long long ktot = 0;
    std::vector<unsigned short> perm, rslot; // [n][ms_pad]; [ms][n] dense slot of every point, if asked for
    std::vector<int> startslot, Ks;         // [parts][ms_pad]; [ms]
    std::vector<long long> koff;            // [ms]
    std::vector<int2> szlab;                // [ktot] (size, label)
    unsigned short *d_perm = nullptr, *d_rslot = nullptr; int *d_startslot = nullptr, *d_K = nullptr; long long *d_koff = nullptr; int2 *d_szlab = nullptr;

    // labellings s0 .. s0 + ms - 1 of the matrix of rows of n, K: the cluster counts of all its rows; slots: fill rslot;
    // slot(s, at, label, size) once per slot of labelling s, `at` its index among the ktot slots.  false: no host memory.
    template <typename Slot>
    bool build(const int64_t *labels, int64_t n_, const int *K, int64_t s0, int64_t ms_, bool slots, Slot slot)
    {
        n = n_; ms = ms_;
        ms_pad = (int)((ms + 63) / 64 * 64);
        parts = ms_pad >= TPB1 ? 1 : (int)std::min<int64_t>(TPB1 / ms_pad, n);
        std::vector<int> partat, cnt, slot_of_label, pos;
        ktot = 0;
        try {
            perm.assign((size_t)n * ms_pad, 0);
            if (slots) rslot.resize((size_t)ms * n);
            startslot.assign((size_t)parts * ms_pad, 0);
            partat.assign((size_t)n, -1);
            cnt.assign((size_t)n + 1, 0); slot_of_label.assign((size_t)n + 1, 0); pos.assign((size_t)n, 0);
            koff.resize((size_t)ms); Ks.resize((size_t)ms);
            for (int64_t s = 0; s < ms; ++s) ktot += K[s0 + s];
            szlab.resize((size_t)ktot);
        } catch (const std::bad_alloc &) { return false; }
        for (int p = 0; p < parts; ++p) partat[(size_t)((long long)p * n / parts)] = p;
        long long k0 = 0;
        for (int64_t s = 0; s < ms; ++s) {
            const int64_t *z = labels + (size_t)(s0 + s) * n;
            unsigned short *rs = slots ? rslot.data() + (size_t)s * n : nullptr;
            const int Ks_ = cluster_order(z, n, cnt, slot_of_label, pos,
                [&](int t, int64_t l, int sz) {
                    szlab[(size_t)(k0 + t)] = make_int2(sz, (int)l);
                    slot(s, k0 + t, l, sz);
                },
                [&](int at_, int64_t j, int t) {
                    perm[(size_t)at_ * ms_pad + s] = (unsigned short)j;
                    if (rs) rs[j] = (unsigned short)t;
                    if (partat[(size_t)at_] >= 0) startslot[(size_t)partat[(size_t)at_] * ms_pad + s] = t;
                });
            koff[(size_t)s] = k0; Ks[(size_t)s] = Ks_;
            // after the fill pos[t] is one past slot t's last position: mark those
            for (int t = 0; t < Ks_; ++t) perm[(size_t)(pos[(size_t)t] - 1) * ms_pad + s] |= 0x8000u;
            k0 += Ks_;
        }
        return true;
    }

    hipError_t upload(DeviceBuffers &B)
    {
        hipError_t e;
        if ((e = B.alloc(d_perm, perm.size())) != hipSuccess) return e;
        if ((e = B.alloc(d_startslot, startslot.size())) != hipSuccess) return e;
        if ((e = B.alloc(d_K, (size_t)ms)) != hipSuccess) return e;
        if ((e = B.alloc(d_koff, (size_t)ms)) != hipSuccess) return e;
        if ((e = B.alloc(d_szlab, (size_t)ktot)) != hipSuccess) return e;
        if ((e = hipMemcpy(d_perm, perm.data(), perm.size() * sizeof(unsigned short), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(d_startslot, startslot.data(), startslot.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(d_K, Ks.data(), (size_t)ms * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(d_koff, koff.data(), (size_t)ms * sizeof(long long), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = hipMemcpy(d_szlab, szlab.data(), (size_t)ktot * sizeof(int2), hipMemcpyHostToDevice)) != hipSuccess) return e;
        if (rslot.empty()) return hipSuccess;
        if ((e = B.alloc(d_rslot, rslot.size())) != hipSuccess) return e;
        return hipMemcpy(d_rslot, rslot.data(), rslot.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
    }

    // the [np][ktot] sums of np rows ([np][n] (Dq, Lq)) on stream 0; rows_global: gather from global memory at any n
    hipError_t launch_sums(const ll2 *d_rows, int64_t np, bool rows_global, ll2 *d_sums) const
    {
        const bool ldsrow = !rows_global && n <= LDS_ROW_MAX_N;
        const size_t lds = ldsrow ? (size_t)n * sizeof(ll2) : 0;
        auto kern = ldsrow ? (parts > 1 ? k_predict_sums<true, true> : k_predict_sums<true, false>)
                           : (parts > 1 ? k_predict_sums<false, true> : k_predict_sums<false, false>);
        hipError_t e = set_dynamic_lds(kern, lds);
        if (e != hipSuccess) return e;
        if (parts > 1 && (e = hipMemsetAsync(d_sums, 0, (size_t)np * ktot * sizeof(ll2), 0)) != hipSuccess) return e;   // the parts add into zeros
        kern<<<(unsigned)np, TPB1, lds, 0>>>(d_rows, (int)n, d_perm, (int)ms, ms_pad, parts, d_startslot, d_koff, ktot, d_sums);
        return hipGetLastError();
    }
};

}  // namespace prd

namespace slab {

// The uploaded labellings of O against every row of context c, the rows in chunks of at most qc.  Per chunk of np rows from
// i0: stage<<<np, tpb_stage>>>(view, i0, rows) gathers them in the caller's order (k_score_rows, k_profile_rows),
// k_predict_sums fills their [np][O.ktot] slab and consume(sums, i0, np) launches the caller's kernel on it, all on stream 0.
// The rows and the slab are B's.  ms_acc: device milliseconds, added to.
template <typename Consume>
static int32_t run_rows(rc_ctx *c, const prd::Orders &O, DeviceBuffers &B, int64_t qc, bool rows_global, void (*stage)(View, int, ll2 *),
                        int tpb_stage, Consume consume, double &ms_acc)
{
    const int64_t n = O.n;
    ll2 *d_rows, *d_sums;
    HIPCHK(c, B.alloc(d_rows, (size_t)qc * n));
    HIPCHK(c, B.alloc(d_sums, (size_t)qc * O.ktot));
    const View V = make_view(c);
    TimingEvents ev;
    HIPCHK(c, ev.create());
    for (int64_t i0 = 0; i0 < n; i0 += qc) {
        const int64_t np = std::min(qc, n - i0);
        HIPCHK(c, ev.begin(0));
        stage<<<(unsigned)np, tpb_stage, 0, 0>>>(V, (int)i0, d_rows);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, O.launch_sums(d_rows, np, rows_global, d_sums));
        consume(d_sums, i0, np);
        HIPCHK(c, ev.end(0));
        HIPCHK(c, ev.elapsed_ms(ms_acc));
    }
    return RC_OK;
}

}  // namespace slab

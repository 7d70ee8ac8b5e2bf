// Relabelling: every posterior sample renamed onto a pivot labelling (a point estimate) by the matching of its clusters to the
// pivot's that maximises the number of points on which the two agree, and, per point, how often it lands in each of the pivot's
// clusters — pivot relabelling (ECR with a fixed pivot) in exact integers, on the device.  DESIGN.md §8 "Relabelling"; the
// contract is in include/redclust_hip.h.  Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK,
// the holders and select_device of hostutil.inc.hip, and compact_row / check_rows of partdist.inc.hip).
//
// Host: the pivot and every sample are compacted to dense u16 ids in ascending label order (compact_row).
//
// k_relabel: one workgroup of TPB threads per sample (the grid is capped, workgroups loop), three phases.
//   1. Table.  T[r][c], r over the side with fewer clusters (the pivot on a tie), c over the other: R rows of `stride` 16-bit
//      cells (n <= 32767, so a cell fits 15 bits), two cells per dword.  All threads walk the n points and add 1 << 16·(cell & 1)
//      to the cell's dword with a non-returning atomic: the low half never carries into the high half.  The table is in LDS
//      behind the assignment's vectors when both fit LDS_BUDGET, else (or with RC_RELABEL_TABLE_GLOBAL=1) in a slab of global
//      memory that belongs to the resident workgroup, written and read with device-scope atomics only.
//   2. Assignment, by wave 0.  Shortest augmenting paths with potentials on cost = −T, rows inserted in ascending id.  Lane x
//      owns the columns j ≡ x (mod 64): it alone reads and writes minv[j], way[j], used[j], v[j].  A step's next column is the
//      wave minimum of the key minv[j]·2^32 + j over the unused columns, so among equal reduced costs the smallest column id
//      wins by the order of the keys.  Potentials, minv, way, used and the matching p are in LDS.  With the table in the slab
//      a lane loads all its cells of the scanned row before it uses the first, so a step waits for global memory once.
//   3. Rename and count.  All threads write labels[s][j] and add 1 to counts[j][k] (global atomics: integer adds commute).
// There is no floating point in the kernel.

namespace relabel {

constexpr int64_t NMAX = 32767;                 // a cell of the table fits 15 bits
constexpr int KMAX = 1024;                      // clusters of the pivot and of every sample
constexpr int TPB = 256;                        // four waves: one per SIMD, up to eight workgroups per CU
constexpr size_t LDS_BUDGET = 128 * 1024;       // vectors and table of one workgroup (the CU has 160 KiB)
constexpr size_t WORKSPACE = (size_t)1 << 30;   // device bytes of one chunk of samples
constexpr int GRID_MAX = 2048;                  // workgroups with the table in LDS
constexpr int GLOBAL_GRID_MAX = 256;            // workgroups with the table in a global slab
constexpr int INF = 0x3fffffff;
constexpr int NVEC = 6;                         // u, v, minv, p, way, used
constexpr int CPL = KMAX / 64 + 1;              // columns 0..KMAX that a lane of the assignment's wave owns at the most

struct Args {
    const unsigned short *piv;      // [n] dense ids of the pivot
    const unsigned short *zid;      // [mc][n] dense ids of the samples
    const int *Ks;                  // [mc]
    const int *names;               // [Kp] the pivot's label of dense id k
    unsigned *slab;                 // TGLOBAL: [gridDim.x][slab_dwords]
    long long *labels;              // [mc][n] or null
    long long *maps;                // [mc][W] or null
    long long *overlap;             // [mc]
    unsigned *counts;               // [n][Kp + 1], accumulated
    size_t slab_dwords;
    int n, mc, Kp, W;
    int vw;                         // ints per vector: above every column count of the chunk, a multiple of 4
};

template <bool TGLOBAL> __device__ __forceinline__ void zero_dword(unsigned *q)
{
    // The slab is zeroed, added to and read (read_cell) with relaxed device-scope atomic operations only, with a workgroup barrier
    // between the three.  That is enough because the vector memory operations of one workgroup — one CU, not in threadgroup-split
    // mode — reach L2 in the order they were issued and none of them is served by the CU's vector cache.  A plain load in
    // read_cell could meet a stale cache line left by the previous sample; in threadgroup-split mode the barriers would need
    // device-scope release / acquire fences.
    if (TGLOBAL) __hip_atomic_store(q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *q = 0u;
}

template <bool TGLOBAL> __device__ __forceinline__ void add_cell(unsigned *tab, int e)
{
    (void)__hip_atomic_fetch_add(tab + (e >> 1), 1u << ((e & 1) * 16), __ATOMIC_RELAXED,
                                 TGLOBAL ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP);
}

template <bool TGLOBAL> __device__ __forceinline__ int read_cell(const unsigned *tab, int e)
{
    if (TGLOBAL) return (int)((__hip_atomic_load(tab + (e >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> ((e & 1) * 16)) & 0xFFFFu);
    return (int)reinterpret_cast<const unsigned short *>(tab)[e];
}

// what one lane wrote to LDS is visible to the other lanes of its wave behind this
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// dynamic LDS: int u[vw] | v[vw] | minv[vw] | p[vw] | way[vw] | used[vw] | !TGLOBAL: the table
template <bool TGLOBAL>
__global__ __launch_bounds__(TPB) void k_relabel(const Args A)
{
    extern __shared__ __align__(16) unsigned char rl_lds[];
    int *u = reinterpret_cast<int *>(rl_lds), *v = u + A.vw, *minv = v + A.vw, *p = minv + A.vw, *way = p + A.vw, *used = way + A.vw;
    unsigned *tab;
    if constexpr (TGLOBAL) tab = A.slab + (size_t)blockIdx.x * A.slab_dwords;
    else tab = reinterpret_cast<unsigned *>(used + A.vw);
    const int n = A.n, Kp = A.Kp, tid = threadIdx.x, lane = tid & 63;
    for (int s = blockIdx.x; s < A.mc; s += gridDim.x) {
        const int Ks = A.Ks[s];
        const bool prow = Kp <= Ks;                                  // the pivot's clusters are the rows
        const int R = prow ? Kp : Ks, Cc = prow ? Ks : Kp, stride = (Cc + 1) & ~1;
        const unsigned short *__restrict__ zs = A.zid + (size_t)s * n;

        // 1. the table
        for (int i = tid; i < R * stride / 2; i += TPB) zero_dword<TGLOBAL>(tab + i);
        for (int i = tid; i <= Cc; i += TPB) { u[i] = 0; v[i] = 0; p[i] = 0; }
        __syncthreads();
        for (int j = tid; j < n; j += TPB) {
            const int c = A.piv[j], z = zs[j];
            add_cell<TGLOBAL>(tab, prow ? c * stride + z : z * stride + c);
        }
        __syncthreads();

        // 2. the assignment: rows 1..R, columns 1..Cc, column 0 the root of every path; p[j] the row of column j (0: free)
        if (tid < 64) {
            for (int i = 1; i <= R; ++i) {
                for (int j = lane; j <= Cc; j += 64) { minv[j] = INF; used[j] = 0; }
                if (lane == 0) p[0] = i;
                wave_sync();
                int j0 = 0;
                do {
                    if (lane == (j0 & 63)) used[j0] = 1;
                    const int i0 = p[j0], ui = u[i0], e0 = (i0 - 1) * stride - 1;
                    long long best = 0x7fffffffffffffffLL;
                    auto scan = [&](int j, int cell) {
                        const int cur = -cell - ui - v[j];
                        int mv = minv[j];
                        if (cur < mv) { mv = cur; minv[j] = cur; way[j] = j0; }
                        const long long key = (long long)mv * 4294967296LL + j;
                        best = key < best ? key : best;
                    };
                    if constexpr (TGLOBAL) {
                        // the lane's cells of the row first, all loads in flight at once (a clamped column: always inside the row)
                        int cell[CPL];
#pragma unroll
                        for (int t = 0; t < CPL; ++t) cell[t] = read_cell<true>(tab, e0 + min(max(lane + 64 * t, 1), Cc));
#pragma unroll
                        for (int t = 0; t < CPL; ++t) {
                            const int j = lane + 64 * t;
                            if (j >= 1 && j <= Cc && !used[j]) scan(j, cell[t]);
                        }
                    } else {
                        for (int j = lane; j <= Cc; j += 64) {
                            if (j == 0 || used[j]) continue;
                            scan(j, read_cell<false>(tab, e0 + j));
                        }
                    }
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        const long long o = __shfl_xor(best, off);
                        best = o < best ? o : best;
                    }
                    const int delta = (int)(best >> 32), j1 = (int)(best & 0xffffffffLL);
                    for (int j = lane; j <= Cc; j += 64) {
                        if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                        else minv[j] -= delta;
                    }
                    wave_sync();
                    j0 = j1;
                } while (p[j0] != 0);
                do {                                                 // every column of the path is written once, before it is read
                    const int j1 = way[j0], r = p[j1];
                    if (lane == 0) p[j0] = r;
                    j0 = j1;
                } while (j0);
                wave_sync();
            }
            // kcol[l] (in minv): the pivot's dense id + 1 that the sample's cluster l goes to, 0 = unmatched; the matched overlap
            // (every l is written: the columns are the sample's clusters, or every row is matched)
            long long ov = 0;
            for (int j = 1 + lane; j <= Cc; j += 64) {
                const int r = p[j];
                if (r) ov += read_cell<TGLOBAL>(tab, (r - 1) * stride + j - 1);
                if (prow) minv[j - 1] = r;
                else if (r) minv[r - 1] = j;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) ov += __shfl_xor(ov, off);
            if (lane == 0) A.overlap[s] = ov;
        }
        __syncthreads();

        // 3. rename and count
        const int *kcol = minv;
        if (A.maps)
            for (int t = tid; t < A.W; t += TPB) {
                long long to = -1;
                if (t < Ks) { const int k = kcol[t]; to = k ? A.names[k - 1] : 0; }
                A.maps[(size_t)s * A.W + t] = to;
            }
        for (int j = tid; j < n; j += TPB) {
            const int k = kcol[zs[j]];
            if (A.labels) A.labels[(size_t)s * n + j] = k ? A.names[k - 1] : 0;
            (void)__hip_atomic_fetch_add(A.counts + (size_t)j * (Kp + 1) + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();                                             // the next sample replaces the vectors and the table
    }
}

// bytes of one sample's table and its column count, given the two cluster counts
static inline size_t table_bytes(int Kp, int Ks, int &cols)
{
    const int R = Kp <= Ks ? Kp : Ks;
    cols = Kp <= Ks ? Ks : Kp;
    return (size_t)R * (size_t)((cols + 1) & ~1) * 2;
}

}  // namespace relabel

extern "C" int32_t rc_relabel(int32_t device, const int64_t *samples, int64_t m, int64_t n, const int64_t *pivot, int64_t Kp_in,
                              int64_t *labels_out, int64_t *maps_out, int64_t maps_width, int64_t *overlap_out, void *counts_out,
                              double *kernel_ms)
{
    using namespace relabel;
    const char *who = "rc_relabel";
    if (!samples || !pivot || !overlap_out || !counts_out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (m < 1 || n < 1) return fail(nullptr, RC_ERR_ARG, "%s: need m >= 1 and n >= 1 (got m=%lld n=%lld)", who, (long long)m, (long long)n);
    if (n > NMAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %lld points whose counts fit 15 bits", who, (long long)n, (long long)NMAX);
    if (m >= ((int64_t)1 << 31)) return fail(nullptr, RC_ERR_CAPACITY, "%s: m = %lld is not below 2^31", who, (long long)m);
    int32_t rc = check_label_rows(nullptr, who, "pivot", pivot, 1, n);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;

    std::vector<int> cnt, id, Ks, names;
    std::vector<unsigned short> h_piv;
    try {
        cnt.assign((size_t)n + 1, 0); id.assign((size_t)n + 1, 0); Ks.resize((size_t)m); h_piv.resize((size_t)n);
    } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    const auto no_slot = [](int, int64_t, int) {};                    // only the ids and the cluster counts are wanted here
    const int64_t Kp = compact_labels(pivot, n, cnt, id, no_slot);
    dense_ids(pivot, n, id, h_piv.data());
    if (Kp > KMAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: the pivot has %lld clusters, more than %d", who, (long long)Kp, KMAX);
    names.assign((size_t)Kp, 0);
    for (int64_t j = 0; j < n; ++j) names[h_piv[(size_t)j]] = (int)pivot[j];
    const size_t workspace = env_workspace_kib("RC_RELABEL_WORKSPACE_KIB", WORKSPACE);
    // The samples are compacted here for their cluster counts, which the capacity checks need before any device work.  Their
    // dense ids are kept for the chunks when all of them fit a workspace's worth of host memory, else made again per chunk.
    const bool keep_ids = 2 * (size_t)m * (size_t)n <= workspace;
    std::vector<unsigned short> h_zid;
    if (keep_ids) {
        try { h_zid.resize((size_t)m * n); } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for the ids of %lld samples", who, (long long)m); }
    }
    int64_t W = 0;
    size_t slab_bytes = 0;                                            // the largest table of the call
    for (int64_t s = 0; s < m; ++s) {
        const int K = compact_labels(samples + (size_t)s * n, n, cnt, id, no_slot);
        if (keep_ids) dense_ids(samples + (size_t)s * n, n, id, h_zid.data() + (size_t)s * n);
        if (K > KMAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: sample %lld has %lld clusters, more than %d", who, (long long)s + 1, (long long)K, KMAX);
        Ks[(size_t)s] = K;
        W = std::max<int64_t>(W, K);
        int cols;
        slab_bytes = std::max(slab_bytes, table_bytes((int)Kp, K, cols));
    }
    if (Kp_in != Kp) return fail(nullptr, RC_ERR_ARG, "%s: the pivot has %lld clusters, not %lld (counts is n x (K_p + 1))", who, (long long)Kp, (long long)Kp_in);
    if (maps_out && maps_width < W) return fail(nullptr, RC_ERR_ARG, "%s: maps is %lld wide, the largest sample has %lld clusters", who, (long long)maps_width, (long long)W);
    if (kernel_ms) *kernel_ms = 0.0;

    rc = select_device(who, device);
    if (rc != RC_OK) return rc;
    const bool force_global = env_flag("RC_RELABEL_TABLE_GLOBAL");          // tests: the table in the global slab at every size
    const int64_t Wd = maps_out ? maps_width : 0;
    const size_t per_sample = 2 * (size_t)n + sizeof(int) + sizeof(long long) + (labels_out ? 8 * (size_t)n : 0) + 8 * (size_t)Wd;
    const int64_t mc = std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(workspace / per_sample)));
    // the slabs: one table per resident workgroup, within a quarter of the workspace (one workgroup at the least)
    const size_t slab_dwords = (slab_bytes + 15) / 16 * 4;
    const int grid_global = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(GLOBAL_GRID_MAX, mc),
                                                                           (long long)(workspace / 4 / (slab_dwords * 4))));
    if (!keep_ids) {
        try { h_zid.resize((size_t)mc * n); } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for a chunk of %lld samples", who, (long long)mc); }
    }

    DeviceBuffers B;
    unsigned short *d_piv, *d_zid; int *d_Ks, *d_names; unsigned *d_counts, *d_slab = nullptr;
    long long *d_labels = nullptr, *d_maps = nullptr, *d_overlap;
    const size_t ncounts = (size_t)n * (size_t)(Kp + 1);
    HIPCHK(nullptr, B.alloc(d_piv, (size_t)n));
    HIPCHK(nullptr, B.alloc(d_names, (size_t)Kp));
    HIPCHK(nullptr, B.alloc(d_counts, ncounts));
    HIPCHK(nullptr, B.alloc(d_zid, (size_t)mc * n));
    HIPCHK(nullptr, B.alloc(d_Ks, (size_t)mc));
    HIPCHK(nullptr, B.alloc(d_overlap, (size_t)mc));
    if (labels_out) HIPCHK(nullptr, B.alloc(d_labels, (size_t)mc * n));
    if (maps_out) HIPCHK(nullptr, B.alloc(d_maps, (size_t)mc * Wd));
    HIPCHK(nullptr, hipMemcpy(d_piv, h_piv.data(), (size_t)n * sizeof(unsigned short), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_names, names.data(), (size_t)Kp * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemset(d_counts, 0, ncounts * sizeof(unsigned)));
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());

    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < m; s0 += mc) {
        const int64_t ms = std::min(mc, m - s0);
        size_t tab = 0;
        int cmax = 0;
        for (int64_t s = 0; s < ms; ++s) {
            if (!keep_ids) {
                compact_labels(samples + (size_t)(s0 + s) * n, n, cnt, id, no_slot);
                dense_ids(samples + (size_t)(s0 + s) * n, n, id, h_zid.data() + (size_t)s * n);
            }
            int cols;
            tab = std::max(tab, table_bytes((int)Kp, Ks[(size_t)(s0 + s)], cols));
            cmax = std::max(cmax, cols);
        }
        const int vw = (cmax + 1 + 3) / 4 * 4;
        const size_t vec_bytes = (size_t)NVEC * vw * sizeof(int);
        const bool tglobal = force_global || vec_bytes + tab > LDS_BUDGET;
        const size_t lds = vec_bytes + (tglobal ? 0 : tab);
        if (tglobal && !d_slab) HIPCHK(nullptr, B.alloc(d_slab, (size_t)grid_global * slab_dwords));
        HIPCHK(nullptr, hipMemcpy(d_zid, h_zid.data() + (keep_ids ? (size_t)s0 * n : 0), (size_t)ms * n * sizeof(unsigned short), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_Ks, Ks.data() + s0, (size_t)ms * sizeof(int), hipMemcpyHostToDevice));
        auto kern = tglobal ? k_relabel<true> : k_relabel<false>;
        HIPCHK(nullptr, set_dynamic_lds(kern, lds));
        Args a{};
        a.piv = d_piv; a.zid = d_zid; a.Ks = d_Ks; a.names = d_names; a.slab = d_slab; a.labels = d_labels; a.maps = d_maps;
        a.overlap = d_overlap; a.counts = d_counts; a.slab_dwords = slab_dwords;
        a.n = (int)n; a.mc = (int)ms; a.Kp = (int)Kp; a.W = (int)Wd; a.vw = vw;
        const unsigned grid = (unsigned)std::min<int64_t>(tglobal ? grid_global : GRID_MAX, ms);
        HIPCHK(nullptr, ev.begin(0));
        kern<<<grid, TPB, lds, 0>>>(a);
        HIPCHK(nullptr, ev.end(0));
        HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
        HIPCHK(nullptr, hipMemcpy(overlap_out + s0, d_overlap, (size_t)ms * sizeof(long long), hipMemcpyDeviceToHost));
        if (labels_out) HIPCHK(nullptr, hipMemcpy(labels_out + (size_t)s0 * n, d_labels, (size_t)ms * n * sizeof(long long), hipMemcpyDeviceToHost));
        if (maps_out) HIPCHK(nullptr, hipMemcpy(maps_out + (size_t)s0 * Wd, d_maps, (size_t)ms * Wd * sizeof(long long), hipMemcpyDeviceToHost));
    }
    HIPCHK(nullptr, hipMemcpy(counts_out, d_counts, ncounts * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

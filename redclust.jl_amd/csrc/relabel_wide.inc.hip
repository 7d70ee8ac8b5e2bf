// Relabelling onto pivots and samples of up to 4096 clusters: rc_relabel's definition, outputs and tie rule (relabel.inc.hip;
// DESIGN.md §8 "Relabelling", "Wide relabelling") with the contingency table kept sparse.  Two labellings of n points share at most
// n non-zero cells however many clusters they have, so a workgroup needs O(n + K) memory per sample where k_relabel's dense table
// needs O(K²), and the assignment's column scan is the work of sixteen waves, not of one.  Included from redclust_hip.hip after
// relabel.inc.hip: the host side is relabel::run with this file's launcher.
//
// k_relabel_wide: one workgroup of 1024 threads per sample (the grid is capped at one workgroup per CU, workgroups loop).
//   1. Sparse table.  Rows are the side with fewer clusters (the pivot on a tie), as in k_relabel.  A histogram of the points' row
//      ids in LDS, an exclusive scan (rowptr), and every point's column id scattered into its row's segment of `seg`, a u16[n]
//      slab of global memory that belongs to the resident workgroup.  Then wave w takes the rows w, w + 16, …: it adds the row's
//      segment into a dense u16 row of its own in LDS, and walks the segment again taking each cell out with a returning AND: the
//      lane that finds the cell non-zero owns its count and appends the packed word (column + 1) << 15 | count to the row's
//      entries in `csr`, a second slab, u32[n].  A row's distinct columns are no more than its points, so its entries fit the
//      place of its segment, and the AND has cleared the cell for the next row.
//      The order of a row's entries is whatever the lanes make it: nothing reads it (a step stores every entry of a row before
//      any is used).  rowptr and the rows' entry counts are u16 in LDS (offsets <= n <= 32767).
//   2. Assignment, by all threads.  Thread t owns the columns 1 + t + 1024·k, k < 4, and keeps their minv, v, way and used bits in
//      registers; u (by row), the matching p and two dense u16 row buffers are in LDS.  A step: the threads that hold the scanned
//      row's entries (four at the most each) store the counts into the step's row buffer | barrier | every thread scans its unused
//      columns, the minimum of the keys minv·2^32 + j is taken in the wave by DPP and two shuffles, sixteen partials go to LDS |
//      barrier | every thread takes the minimum of the partials, puts delta on its columns and on the rows of its used columns
//      (distinct rows: plain LDS read-modify-writes), and takes the row's entries out of the buffer again.  The next step uses the
//      other buffer, so its stores cannot meet this step's clears.  After a row's last step way goes to LDS, a barrier, and thread 0
//      flips the path while the others store the next row.
//   3. Rename and count, as k_relabel's phase 3; the overlap is the number of points whose renamed label is the pivot's.
// The slabs are written and read with relaxed device-scope atomic stores and loads only, workgroup barriers (or, within a wave,
// program order) between them: relabel.inc.hip's argument for its slab (zero_dword).  There is no floating point.

namespace relabel_wide {

constexpr int KMAX = 4096;                      // clusters of the pivot and of every sample
constexpr int TPB = 1024;                       // sixteen waves, four per SIMD: 128 VGPRs at the most
constexpr int NWAVE = TPB / 64;
constexpr int CPT = KMAX / TPB;                 // columns per thread
constexpr int GRID_MAX = 256;                   // one workgroup per CU
constexpr int INF = relabel::INF;
constexpr int CNT_BITS = 15;                    // a packed entry: (column + 1) << 15 | count, count <= n <= 32767

// The LDS carve, in bytes from the start of dynamic LDS.  cw: the u16 / i32 elements per vector, above every column count of the
// chunk (rows + 1 <= columns + 1 <= cw), a multiple of 8.
//   rowptr u16[cw] | rownnz u16[cw] | part i64[16] | overlay
// The overlay is, while the table is built, hist i32[cw] (then the rows' cursors) and after the scatter sixteen waves' dense rows
// u16[cw]; in the assignment u i32[cw] | p u16[cw] | way u16[cw] | kcol u16[cw] | rowbuf u16[2][cw] (14·cw bytes, inside).
// 36·cw + 128 bytes: 147 872 at 4096 columns (cw = 4104), of the CU's 163 840; n does not enter.
__host__ __device__ constexpr int carve_width(int cols) { return (cols + 1 + 7) & ~7; }
__host__ __device__ constexpr size_t overlay_offset(int cw) { return 4 * (size_t)cw + 8 * NWAVE; }
__host__ __device__ constexpr size_t lds_bytes(int cw) { return overlay_offset(cw) + (size_t)NWAVE * 2 * cw; }
static_assert(lds_bytes(carve_width(KMAX)) <= 160 * 1024 - 64, "the carve and the static counter must fit the CU's LDS at 4096 columns");

struct Args {
    const unsigned short *piv;      // [n] dense ids of the pivot
    const unsigned short *zid;      // [mc][n] dense ids of the samples
    const int *Ks;                  // [mc]
    const int *names;               // [Kp] the pivot's label of dense id k
    unsigned short *seg;            // [gridDim.x][slab]: the points' column ids by row
    unsigned *csr;                  // [gridDim.x][slab]: the rows' packed entries
    long long *labels;              // [mc][n] or null
    long long *maps;                // [mc][W] or null
    long long *overlap;             // [mc]
    unsigned *counts;               // [n][Kp + 1], accumulated
    size_t slab;                    // elements of one workgroup's slab: n rounded up
    int n, mc, Kp, W, cw;
};

template <typename T> __device__ __forceinline__ void slab_store(T *q, T x) { __hip_atomic_store(q, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T> __device__ __forceinline__ T slab_load(const T *q) { return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the other 64-bit value of a DPP control that moves lanes within a row of 16
template <int CTRL> __device__ __forceinline__ long long dpp64(long long x)
{
    const int lo = (int)x, hi = (int)(x >> 32);
    const unsigned l = (unsigned)__builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    const int h = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return (long long)(((unsigned long long)(unsigned)h << 32) | l);
}

// the minimum over the lane's row of 16, in every lane of it: the neighbour, the other pair (quad_perm), the other quad
// (row_half_mirror), the other half (row_mirror)
__device__ __forceinline__ long long row_min(long long x)
{
    long long o = dpp64<0xB1>(x); x = o < x ? o : x;
    o = dpp64<0x4E>(x); x = o < x ? o : x;
    o = dpp64<0x141>(x); x = o < x ? o : x;
    o = dpp64<0x140>(x); x = o < x ? o : x;
    return x;
}

__device__ __forceinline__ long long wave_min(long long x)
{
    x = row_min(x);
    long long o = __shfl_xor(x, 16); x = o < x ? o : x;
    o = __shfl_xor(x, 32);
    return o < x ? o : x;
}

__global__ __launch_bounds__(TPB) void k_relabel_wide(const Args A)
{
    extern __shared__ __align__(16) unsigned char rw_lds[];
    __shared__ int ovl;                                              // the sample's overlap
    const int cw = A.cw, n = A.n, Kp = A.Kp, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned short *rowptr = reinterpret_cast<unsigned short *>(rw_lds), *rownnz = rowptr + cw;
    long long *part = reinterpret_cast<long long *>(rw_lds + 4 * (size_t)cw);
    unsigned char *ov = rw_lds + overlay_offset(cw);
    int *hist = reinterpret_cast<int *>(ov);
    unsigned *wrow = reinterpret_cast<unsigned *>(ov + (size_t)wave * 2 * cw);                 // the wave's dense row, two cells a dword
    int *u = reinterpret_cast<int *>(ov);
    unsigned short *p = reinterpret_cast<unsigned short *>(ov + 4 * (size_t)cw), *way = p + cw, *kcol = way + cw, *rowbuf = kcol + cw;
    unsigned short *seg = A.seg + (size_t)blockIdx.x * A.slab;
    unsigned *csr = A.csr + (size_t)blockIdx.x * A.slab;

    for (int s = blockIdx.x; s < A.mc; s += gridDim.x) {
        const int Ks = A.Ks[s];
        const bool prow = Kp <= Ks;                                  // the pivot's clusters are the rows
        const int R = prow ? Kp : Ks, Cc = prow ? Ks : Kp;
        const unsigned short *__restrict__ zs = A.zid + (size_t)s * n;

        // 1. the sparse table: histogram of the rows
        for (int i = tid; i < R; i += TPB) hist[i] = 0;
        if (tid == 0) { ovl = 0; rowptr[R] = (unsigned short)n; }
        __syncthreads();
        for (int j = tid; j < n; j += TPB)
            (void)__hip_atomic_fetch_add(hist + (prow ? A.piv[j] : zs[j]), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        {   // exclusive scan: thread t has the rows 4t .. 4t + 3 (R <= 4096), its wave the inclusive scan of the threads' sums
            int h[CPT], sum = 0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) { const int r = CPT * tid + k; h[k] = r < R ? hist[r] : 0; sum += h[k]; }
            int inc = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(inc, off); if (lane >= off) inc += o; }
            int *wsum = reinterpret_cast<int *>(part);
            if (lane == 63) wsum[wave] = inc;
            __syncthreads();
            int at = inc - sum;
            for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int r = CPT * tid + k;
                if (r < R) { rowptr[r] = (unsigned short)at; hist[r] = at; }        // the row's cursor of the scatter
                at += h[k];
            }
        }
        __syncthreads();
        for (int j = tid; j < n; j += TPB) {
            const int c = A.piv[j], z = zs[j];
            const int at = __hip_atomic_fetch_add(hist + (prow ? c : z), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            slab_store(seg + at, (unsigned short)(prow ? z : c));
        }
        __syncthreads();
        for (int i = tid; i < NWAVE * cw / 2; i += TPB) reinterpret_cast<unsigned *>(ov)[i] = 0u;   // the waves' dense rows
        __syncthreads();
        for (int r = wave; r < R; r += NWAVE) {
            const int e0 = rowptr[r], e1 = rowptr[r + 1];
            for (int e = e0 + lane; e < e1; e += 64) {
                const int c = slab_load(seg + e);
                (void)__hip_atomic_fetch_add(wrow + (c >> 1), 1u << ((c & 1) * 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            relabel::wave_sync();
            int nnz = 0;
            for (int e = e0; e < e1; e += 64) {                      // (uniform in the wave: the ballot)
                unsigned cnt = 0;
                int c = 0;
                if (e + lane < e1) {
                    c = slab_load(seg + e + lane);
                    const int sh = (c & 1) * 16;
                    cnt = (__hip_atomic_fetch_and(wrow + (c >> 1), ~(0xFFFFu << sh), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> sh) & 0xFFFFu;
                }
                const unsigned long long owners = __ballot(cnt != 0);
                if (cnt) slab_store(csr + e0 + nnz + __popcll(owners & ((1ull << lane) - 1)), ((unsigned)(c + 1) << CNT_BITS) | cnt);
                nnz += __popcll(owners);
            }
            if (lane == 0) rownnz[r] = (unsigned short)nnz;
            relabel::wave_sync();
        }
        __syncthreads();                                             // the dense rows are zero again; the overlay changes hands
        for (int i = tid; i <= Cc; i += TPB) { u[i] = 0; p[i] = 0; kcol[i] = 0; rowbuf[i] = 0; rowbuf[cw + i] = 0; }
        __syncthreads();

        // 2. the assignment: rows 1..R, columns 1..Cc, column 0 the root of every path (its row is the inserted row i, kept in no
        //    array); p[j] the row of column j (0: free).  Two barriers a step: between the row's stores and the scan that reads
        //    them, and between the partial minima and their readers.
        int v[CPT], minv[CPT], wayr[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) { v[k] = 0; wayr[k] = 0; }
        int par = 0;
        for (int i = 1; i <= R; ++i) {
            unsigned used = 0;
#pragma unroll
            for (int k = 0; k < CPT; ++k) minv[k] = INF;
            int j0 = 0, i0 = i;
            do {
                unsigned short *rb = rowbuf + par * cw;
                const int e0 = rowptr[i0 - 1], ne = rownnz[i0 - 1];  // ne <= Cc <= 4096: four entries a thread at the most
                unsigned ent[CPT];
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    const int e = tid + k * TPB;
                    ent[k] = e < ne ? slab_load(csr + e0 + e) : 0u;
                    if (e < ne) rb[ent[k] >> CNT_BITS] = (unsigned short)(ent[k] & ((1u << CNT_BITS) - 1));
                }
                __syncthreads();
                if (j0 && ((j0 - 1) & (TPB - 1)) == tid) used |= 1u << ((j0 - 1) / TPB);
                const int ui = u[i0];
                long long best = 0x7fffffffffffffffLL;
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    const int j = 1 + tid + k * TPB;
                    if (j <= Cc && !((used >> k) & 1u)) {
                        const int cur = -(int)rb[j] - ui - v[k];
                        if (cur < minv[k]) { minv[k] = cur; wayr[k] = j0; }
                        const long long key = (long long)minv[k] * 4294967296LL + j;
                        best = key < best ? key : best;
                    }
                }
                best = wave_min(best);
                if (lane == 0) part[wave] = best;
                __syncthreads();
                best = row_min(part[lane & (NWAVE - 1)]);
                const int delta = (int)(best >> 32), j1 = (int)(best & 0xffffffffLL);
#pragma unroll
                for (int k = 0; k < CPT; ++k) {
                    const int j = 1 + tid + k * TPB;
                    if ((used >> k) & 1u) { u[p[j]] += delta; v[k] -= delta; }
                    else if (j <= Cc) minv[k] -= delta;
                }
                if (tid == 0) u[i] += delta;                         // column 0
#pragma unroll
                for (int k = 0; k < CPT; ++k)
                    if (tid + k * TPB < ne) rb[ent[k] >> CNT_BITS] = 0;
                par ^= 1;
                j0 = j1;
                i0 = p[j0];
            } while (i0 != 0);
#pragma unroll
            for (int k = 0; k < CPT; ++k) {
                const int j = 1 + tid + k * TPB;
                if (j <= Cc) way[j] = (unsigned short)wayr[k];
            }
            __syncthreads();                                         // the last step's u[p[j]] are done; way is there
            if (tid == 0)
                do {                                                 // the next row's first barrier stands before p's next reader
                    const int j1 = way[j0];
                    p[j0] = j1 ? p[j1] : (unsigned short)i;
                    j0 = j1;
                } while (j0);
        }
        __syncthreads();
        // kcol[l]: the pivot's dense id + 1 that the sample's cluster l goes to, 0 = unmatched (every l is written: the columns
        // are the sample's clusters, or every row is matched)
        for (int j = 1 + tid; j <= Cc; j += TPB) {
            const int r = p[j];
            if (prow) kcol[j - 1] = (unsigned short)r;
            else if (r) kcol[r - 1] = (unsigned short)j;
        }
        __syncthreads();

        // 3. rename and count
        if (A.maps)
            for (int t = tid; t < A.W; t += TPB) {
                long long to = -1;
                if (t < Ks) { const int k = kcol[t]; to = k ? A.names[k - 1] : 0; }
                A.maps[(size_t)s * A.W + t] = to;
            }
        int agree = 0;
        for (int j = tid; j < n; j += TPB) {
            const int k = kcol[zs[j]];
            agree += k == A.piv[j] + 1;
            if (A.labels) A.labels[(size_t)s * n + j] = k ? A.names[k - 1] : 0;
            (void)__hip_atomic_fetch_add(A.counts + (size_t)j * (Kp + 1) + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) agree += __shfl_xor(agree, off);
        if (lane == 0) (void)__hip_atomic_fetch_add(&ovl, agree, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();                                             // the next sample replaces the overlay
        if (tid == 0) A.overlap[s] = ovl;
    }
}

// k_relabel_wide's launches for relabel::run
struct Launch {
    size_t slab = 0;
    int grid = 1;
    unsigned short *d_seg = nullptr;
    unsigned *d_csr = nullptr;

    void prepare(int64_t n, int, const std::vector<int> &, int64_t mc, size_t workspace)
    {
        // the slabs: 6 bytes a point per resident workgroup, within a quarter of the workspace (one workgroup at the least)
        slab = ((size_t)n + 7) & ~(size_t)7;
        grid = (int)std::max<long long>(1, std::min<long long>(std::min<long long>(GRID_MAX, mc), (long long)(workspace / 4 / (slab * 6))));
    }

    int32_t launch(DeviceBuffers &B, TimingEvents &ev, const relabel::Chunk &c)
    {
        int cmax = 0;
        for (int s = 0; s < c.ms; ++s) cmax = std::max(cmax, std::max(c.Kp, c.h_Ks[s]));
        const int cw = carve_width(cmax);
        const size_t lds = lds_bytes(cw);
        if (!d_seg) {
            HIPCHK(nullptr, B.alloc(d_seg, (size_t)grid * slab));
            HIPCHK(nullptr, B.alloc(d_csr, (size_t)grid * slab));
        }
        HIPCHK(nullptr, set_dynamic_lds(k_relabel_wide, lds));
        Args a{};
        a.piv = c.piv; a.zid = c.zid; a.Ks = c.Ks; a.names = c.names; a.seg = d_seg; a.csr = d_csr; a.labels = c.labels; a.maps = c.maps;
        a.overlap = c.overlap; a.counts = c.counts; a.slab = slab;
        a.n = c.n; a.mc = c.ms; a.Kp = c.Kp; a.W = c.W; a.cw = cw;
        HIPCHK(nullptr, ev.begin(0));
        k_relabel_wide<<<(unsigned)std::min<int64_t>(grid, c.ms), TPB, lds, 0>>>(a);
        HIPCHK(nullptr, ev.end(0));
        return RC_OK;
    }
};

}  // namespace relabel_wide

extern "C" int32_t rc_relabel_wide(int32_t device, const int64_t *samples, int64_t m, int64_t n, const int64_t *pivot, int64_t Kp_in,
                                   int64_t *labels_out, int64_t *maps_out, int64_t maps_width, int64_t *overlap_out, void *counts_out,
                                   double *kernel_ms)
{
    return relabel::run("rc_relabel_wide", relabel_wide::KMAX, relabel_wide::Launch{}, device, samples, m, n, pivot, Kp_in, labels_out,
                        maps_out, maps_width, overlap_out, counts_out, kernel_ms);
}

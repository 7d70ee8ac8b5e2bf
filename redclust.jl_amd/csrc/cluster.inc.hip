// What the two batched clusterings on the device — k-medoids (kmedoids.inc.hip) and k-means (kmeans.inc.hip) — share: the
// workgroup geometry and run flags, the wave / block reductions, the integer weighted draw, the grouping of an assignment,
// the per-k within / between split, and the host side of a scan over k (checks, workspace, rounds, status, errors).
// Included at the end of redclust_hip.hip before both (same translation unit: shares fail(), HIPCHK, rc_ctx, rc_qlog,
// wb_finish).
//
// A scan runs k = kmax, kmax-1, ..., kmin in chunks: slot s of a chunk runs k = khi - s (the largest k is dispatched
// first), one workgroup per slot; a finished run's workgroup exits at once, and the host reads the count of active runs
// every RC_CLUSTER_POLL rounds — no round trip per k and none per iteration.

#define RC_CLUSTER_T 256                    // threads per workgroup
#define RC_CLUSTER_NW (RC_CLUSTER_T / 64)   // waves per workgroup
#define RC_CLUSTER_POLL 4                   // rounds between two reads of the active-run counter
#define RC_CLUSTER_WS_BYTES ((size_t)512 << 20)   // bound of a chunk's workspace (k-medoids at n = 32768 fits)
#define RC_CLUSTER_DONE 1                   // run flags; each clustering's own error bits start at 4
#define RC_CLUSTER_CONV 2

namespace clu {

// floor(u · W / 2^53), exactly
__device__ __forceinline__ u64 scale53(u64 u, u64 W) { return __umul64hi(u << 11, W); }

__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ long long wave_incl_scan(long long v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ long long block_sum(long long v, long long *red /* [RC_CLUSTER_NW] */)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int w = 0; w < RC_CLUSTER_NW; ++w) s += red[w];
    __syncthreads();
    return s;
}

// The contiguous range lo..hi-1 of the points 0..n-1 that the calling thread's wave owns in a weighted draw.  A kernel that
// writes the weights through the same ranges (lanes striding by 64) needs no barrier between its writes and the draw.
__device__ __forceinline__ void wave_range(int n, int &lo, int &hi)
{
    const int seg = (n + RC_CLUSTER_NW - 1) / RC_CLUSTER_NW;
    lo = min(n, (int)(threadIdx.x >> 6) * seg);
    hi = min(n, lo + seg);
}

// One weighted draw over the points 0..n-1 with integer weights q_j = weight(j) >= 0: W = Σ q_j, the first index whose
// inclusive prefix sum exceeds floor(u · W / 2^53); -1 when W == 0.  Each wave owns its wave_range (lanes stride through
// it, so the prefix sums follow the point order).  Called by every thread of the block; the same answer in
// each.  red: [RC_CLUSTER_NW] and pick: one int, both in LDS and free again on return.
template <typename F>
__device__ int draw_weighted(F weight, int n, u64 u, long long *red, int *pick)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int lo, hi;
    wave_range(n, lo, hi);
    if (threadIdx.x == 0) *pick = -1;
    long long v = 0;
    for (int j = lo + lane; j < hi; j += 64) v += weight(j);
    v = wave_sum(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    long long W = 0, excl = 0;
#pragma unroll
    for (int q = 0; q < RC_CLUSTER_NW; ++q) { if (q < wid) excl += red[q]; W += red[q]; }
    int p = -1;
    if (W > 0) {   // uniform over the block
        const u64 thr = scale53(u, (u64)W);   // 0 <= thr < W
        if ((u64)excl <= thr && thr < (u64)(excl + red[wid])) {   // exactly one wave's range holds the pick
            long long base = excl;
            for (int j0 = lo; j0 < hi; j0 += 64) {
                const int j = j0 + lane;
                const long long incl = wave_incl_scan(j < hi ? weight(j) : 0ll, lane) + base;
                const u64 hit = __ballot(j < hi && (u64)incl > thr);
                if (hit) {
                    if (lane == 0) *pick = j0 + __ffsll((unsigned long long)hit) - 1;
                    break;
                }
                base = __shfl(incl, 63);
            }
        }
        __syncthreads();
        p = *pick;
    }
    __syncthreads();   // red and pick are free again
    return p;
}

// Offsets of k groups of sizes cnt: an exclusive scan, each thread owning a contiguous run of groups; off[g] and the scatter
// cursor cur[g] get group g's offset.  Returns whether some group is empty (the same answer in every thread).  Called by
// every thread of the block after a barrier behind the last write of cnt and *flag = 0; off / cur are visible after the
// caller's next barrier.  wtot: [RC_CLUSTER_NW] and flag: one int, both in LDS.
__device__ bool group_offsets(const int *cnt, int k, int *off, int *cur, int *wtot, int *flag)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int per = (k + RC_CLUSTER_T - 1) / RC_CLUSTER_T, g0 = min(k, (int)threadIdx.x * per), g1 = min(k, g0 + per);
    int local = 0, my_empty = 0;
    for (int g = g0; g < g1; ++g) { local += cnt[g]; my_empty |= cnt[g] == 0; }
    if (my_empty) *flag = 1;
    int incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int x = __shfl_up(incl, d);
        if (lane >= d) incl += x;
    }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    const bool empty = *flag != 0;
    int run = incl - local;
    for (int q = 0; q < wid; ++q) run += wtot[q];
    for (int g = g0; g < g1; ++g) { off[g] = run; cur[g] = run; run += cnt[g]; }
    return empty;
}

// The groups of assignment a (k labels): sizes cnt, offsets off (off[k] = n), scatter cursors cur and the members grouped by
// label (their order inside a group depends on timing: every use of it is order-free).  Returns whether some group is empty.
// Called by every thread of the block; wtot: [RC_CLUSTER_NW] and flag: one int, both in LDS.
__device__ bool group_points(const int *a, int n, int k, int *cnt, int *off, int *cur, int *mem, int *wtot, int *flag)
{
    if (threadIdx.x == 0) *flag = 0;
    for (int g = threadIdx.x; g < k; g += RC_CLUSTER_T) cnt[g] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += RC_CLUSTER_T) atomicAdd(&cnt[a[j]], 1);
    __syncthreads();
    const bool empty = group_offsets(cnt, k, off, cur, wtot, flag);
    if (threadIdx.x == 0) off[k] = n;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += RC_CLUSTER_T) mem[atomicAdd(&cur[a[j]], 1)] = j;
    __syncthreads();
    return empty;
}

// The head of both clusterings' workspaces (C slots): all the split reads of a chunk, and its own two arrays
struct Groups {
    int n, ld;             // ld: leading dimension of the context's D
    int khi;               // k of slot 0; slot s runs k = khi - s
    int kstride;           // per-slot stride of the k-sized arrays (>= khi + 1)
    int *assign;           // [C][n] 0-based label of every point
    int *members;          // [C][n] points grouped by label
    int *cnt, *off, *cur;  // [C][kstride] group sizes, offsets into members, scatter cursors
    // per-k split (the _scan_split entries only; null otherwise)
    unsigned long long *acc;  // [C + 2][4]: within sums of slot s (D hi, D lo, logD hi, logD lo: RC_LO_BITS halves as
                              // k_blocksums); row C the upper triangle's totals, row C + 1 (logD's diagonal hi, lo, 0, 0)
    long long *pairs;         // [C] within pairs: Σ_g n_g (n_g - 1) / 2
};

// ---- The per-k split of rc_kmedoids_scan_split / rc_kmeans_scan_split: Σ D and Σ logD over the pairs i < j of one group
// under each slot's final assignment, in exact integers.  logD entries as the block sums take them: rc_qlog of Dq when the
// context derives logD (L == null), otherwise the stored fixed-point logD in the caller's order (Lq_src).  Row sums fit int64
// (quant_exponent); sums over rows go through (hi, lo) halves as in k_blocksums.

__device__ __forceinline__ void acc_add(long long v, long long &hi, long long &lo)
{
    hi += v >> RC_LO_BITS;
    lo += v & (((long long)1 << RC_LO_BITS) - 1);
}

template <typename T>
__device__ __forceinline__ void pair_add(const T *__restrict__ D, const T *__restrict__ L, size_t e, int eD, double sL,
                                         const double2 *__restrict__ tab, long long &sd, long long &sl)
{
    const long long d = (long long)D[e];
    sd += d;
    sl += L ? (long long)L[e] : rc_qlog(d, eD, sL, tab);
}

// the groups of every slot's final assignment (members / cnt of the last round predate its reassignment) and the count of
// within pairs
__global__ __launch_bounds__(RC_CLUSTER_T) void k_split_group(Groups w)
{
    __shared__ long long red[RC_CLUSTER_NW];
    __shared__ int wtot[RC_CLUSTER_NW];
    __shared__ int flag;
    const int slot = blockIdx.x, k = w.khi - slot, n = w.n;
    const size_t ko = (size_t)slot * w.kstride;
    int *cnt = w.cnt + ko;
    (void)group_points(w.assign + (size_t)slot * n, n, k, cnt, w.off + ko, w.cur + ko, w.members + (size_t)slot * n, wtot, &flag);
    long long v = 0;   // (an empty group — a run that ended on a degenerate reassignment — contributes nothing)
    for (int g = threadIdx.x; g < k; g += RC_CLUSTER_T) v += (long long)cnt[g] * (cnt[g] - 1) / 2;
    v = block_sum(v, red);
    if (threadIdx.x == 0) w.pairs[slot] = v;
}

// blockIdx.y = slot; each wave owns 64 consecutive member positions.  A lane whose group has at most 64 members sums its row
// against the group's later positions on its own; the rows of larger groups go through the whole wave one at a time — as
// k-medoids' medoid update does, a group above n/16 streams the row's tail masked by the labels (pairs i < j by point index),
// a smaller one gathers its later members' columns (pairs by member position).  Within a group every row takes the same path,
// so each unordered pair is summed exactly once.
template <typename T>
__global__ __launch_bounds__(RC_CLUSTER_T) void k_split_pairs(const T *__restrict__ D, const T *__restrict__ L, Groups w, int eD,
                                                              double sL, const double2 *__restrict__ tab)
{
    const int slot = blockIdx.y, n = w.n, ld = w.ld;
    const int lane = threadIdx.x & 63, q0 = ((int)blockIdx.x * RC_CLUSTER_NW + (threadIdx.x >> 6)) * 64;
    if (q0 >= n) return;   // (whole waves; no block-level synchronisation follows)
    const int *a = w.assign + (size_t)slot * n, *mem = w.members + (size_t)slot * n;
    const size_t ko = (size_t)slot * w.kstride;
    const int *cnt = w.cnt + ko, *off = w.off + ko;
    const int q = q0 + lane;
    int i = 0, g = 0, s = 0, o = 0;
    if (q < n) { i = mem[q]; g = a[i]; s = cnt[g]; o = off[g]; }
    long long dh = 0, dl = 0, lh = 0, ll = 0;
    if (q < n && s <= 64) {
        long long sd = 0, sl = 0;
        for (int x = q + 1; x < o + s; ++x) pair_add(D, L, (size_t)i * ld + mem[x], eD, sL, tab, sd, sl);
        acc_add(sd, dh, dl);
        acc_add(sl, lh, ll);
    }
    for (u64 big = __ballot(q < n && s > 64); big; big &= big - 1) {
        const int b = __ffsll((unsigned long long)big) - 1;
        const int bi = __shfl(i, b), bg = __shfl(g, b), bs = __shfl(s, b), bo = __shfl(o, b), bq = q0 + b;
        const size_t row = (size_t)bi * ld;
        long long sd = 0, sl = 0;
        if ((long long)bs * 16 > n) {
            for (int j = bi + 1 + lane; j < n; j += 64)
                if (a[j] == bg) pair_add(D, L, row + j, eD, sL, tab, sd, sl);
        } else {
            for (int x = bq + 1 + lane; x < bo + bs; x += 64) pair_add(D, L, row + mem[x], eD, sL, tab, sd, sl);
        }
        sd = wave_sum(sd);
        sl = wave_sum(sl);
        if (lane == 0) { acc_add(sd, dh, dl); acc_add(sl, lh, ll); }
    }
    dh = wave_sum(dh); dl = wave_sum(dl); lh = wave_sum(lh); ll = wave_sum(ll);
    if (lane == 0) {
        unsigned long long *acc = w.acc + (size_t)slot * 4;
        atomicAdd(&acc[0], (unsigned long long)dh);
        atomicAdd(&acc[1], (unsigned long long)dl);
        atomicAdd(&acc[2], (unsigned long long)lh);
        atomicAdd(&acc[3], (unsigned long long)ll);
    }
}

// Σ_{i<j} D and Σ_{i<j} logD over the whole upper triangle and Σ_i logD[i][i] (zero unless the caller's logD has a diagonal):
// the between sums follow as total - within.  One wave per row.
template <typename T>
__global__ __launch_bounds__(RC_CLUSTER_T) void k_split_total(const T *__restrict__ D, const T *__restrict__ L, int n, int ld,
                                                              int eD, double sL, const double2 *__restrict__ tab,
                                                              unsigned long long *tot /* [8] */)
{
    const int lane = threadIdx.x & 63, i = (int)blockIdx.x * RC_CLUSTER_NW + (threadIdx.x >> 6);
    if (i >= n) return;
    const size_t row = (size_t)i * ld;
    long long sd = 0, sl = 0;
    for (int j = i + 1 + lane; j < n; j += 64) pair_add(D, L, row + j, eD, sL, tab, sd, sl);
    sd = wave_sum(sd);
    sl = wave_sum(sl);
    if (lane == 0) {
        long long h[6] = {0, 0, 0, 0, 0, 0};
        acc_add(sd, h[0], h[1]);
        acc_add(sl, h[2], h[3]);
        acc_add(L ? (long long)L[row + i] : 0ll, h[4], h[5]);
        for (int t = 0; t < 6; ++t) atomicAdd(&tot[t], (unsigned long long)h[t]);
    }
}

// ---- The host side of a scan

static int32_t check_ctx(rc_ctx *c, const char *who)
{
    if (!c) return fail(c, RC_ERR_ARG, "%s: NULL ctx", who);
    if (c->broken) return fail(c, RC_ERR_STATE, "%s: the context is void after a failed capacity growth", who);
    return RC_OK;
}

// bad: the code of a k range, maxiter or tol out of range (RC_ERR_ARG for k-medoids, RC_ERR_DOMAIN for k-means)
static int32_t check_range(rc_ctx *c, const char *who, int32_t bad, bool outputs, int64_t kmin, int64_t kmax, int64_t maxiter,
                           double tol)
{
    if (!outputs) return fail(c, RC_ERR_ARG, "%s: NULL output", who);
    const int64_t n = c->n;
    if (kmin < 1 || kmax < kmin || kmax > n)
        return fail(c, bad, "%s: need 1 <= k <= n (got %lld..%lld, n = %lld)", who, (long long)kmin, (long long)kmax, (long long)n);
    if (maxiter < 0 || maxiter > (1 << 24)) return fail(c, bad, "%s: maxiter must be in 0..2^24", who);
    if (!(tol >= 0.0)) return fail(c, bad, "%s: tol must be >= 0", who);
    return RC_OK;
}

// One device allocation carved into 16-byte aligned arrays; freed on scope exit.
struct Workspace {
    char *base = nullptr, *p = nullptr;
    size_t bytes = 0;
    Workspace() = default;
    Workspace(const Workspace &) = delete;
    ~Workspace() { if (base) (void)hipFree(base); }
    hipError_t alloc(size_t b) { bytes = b; const hipError_t e = hipMalloc(&base, b); p = base; return e; }
    template <typename T> T *take(size_t count)
    {
        T *q = (T *)p;
        p += (count * sizeof(T) + 15) & ~(size_t)15;
        return q;
    }
    bool overflow() const { return (size_t)(p - base) > bytes; }   // (checked once, after the last take, before any use)
};

// f(D): D is the context's fixed-point matrix in the caller's point order, typed by its storage (const long long * or
// const int *): kernels templated on the entry type deduce it
template <typename F>
static void by_bits(const rc_ctx *c, F &&f)
{
    if (c->bits == 64) f((const long long *)c->Dq_src);
    else f((const int *)c->Dq_src);
}

// A chunk's rounds 0..rounds-1 after its seeding: launch(r) enqueues round r; every RC_CLUSTER_POLL rounds the host reads
// the count of runs still active after the last one and stops at 0.
template <typename F>
static hipError_t run_rounds(hipStream_t s, int64_t rounds, const unsigned *active, F &&launch)
{
    hipError_t e = hipGetLastError();   // the seeding's launch
    for (int64_t r = 0; r < rounds && e == hipSuccess;) {
        const int64_t r1 = std::min<int64_t>(rounds, r + RC_CLUSTER_POLL);
        for (; r < r1 && e == hipSuccess; ++r) {
            launch(r);
            e = hipGetLastError();
        }
        unsigned act = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&act, active + (r - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess || act == 0) break;
    }
    return e;
}

// a chunk's per-slot status on the host; Cost: the device's type of a slot's cost (8 bytes)
template <typename Cost>
struct Status {
    std::vector<Cost> cost;
    std::vector<int> iter, flags;
    unsigned err = 0;   // OR of the error bits of every chunk so far
    explicit Status(int64_t C) : cost((size_t)C), iter((size_t)C), flags((size_t)C) {}
    hipError_t read(hipStream_t s, int cnt, const Cost *d_cost, const int *d_iter, const int *d_flags, const unsigned *d_err)
    {
        unsigned ce = 0;
        hipError_t e = hipMemcpyAsync(cost.data(), d_cost, (size_t)cnt * sizeof(Cost), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(iter.data(), d_iter, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(flags.data(), d_flags, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&ce, d_err, sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) err |= ce;
        return e;
    }
};

// The within / between split of a scan: carve() with the workspace, begin() once (the upper triangle's totals), chunk() after
// each chunk's last round, before the next chunk's seeding overwrites the assignments.
struct Split {
    const void *L = nullptr;   // the stored logD (null: derived from Dq)
    double sL = 0;
    unsigned long long tot[8] = {};
    std::vector<unsigned long long> acc;
    std::vector<long long> pairs;

    static constexpr size_t PER_SLOT = 40, FIXED = 64 + 2 * 16;   // workspace bytes: acc and pairs; the totals and alignment
    void carve(Workspace &ws, Groups &g, int64_t C)
    {
        g.acc = ws.take<unsigned long long>((size_t)(C + 2) * 4);
        g.pairs = ws.take<long long>((size_t)C);
        acc.resize((size_t)C * 4);
        pairs.resize((size_t)C);
    }
    hipError_t begin(const rc_ctx *c, hipStream_t s, const Groups &g, int64_t C)
    {
        L = c->derived ? nullptr : c->Lq_src;
        sL = std::ldexp(1.0, c->eL);
        unsigned long long *d_tot = g.acc + (size_t)C * 4;
        const unsigned nb = (unsigned)((g.n + RC_CLUSTER_NW - 1) / RC_CLUSTER_NW);
        hipError_t e = hipMemsetAsync(d_tot, 0, 64, s);
        if (e != hipSuccess) return e;
        by_bits(c, [&](auto *D) { k_split_total<<<nb, RC_CLUSTER_T, 0, s>>>(D, (decltype(D))L, g.n, g.ld, c->eD, sL, c->ltab, d_tot); });
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(tot, d_tot, 64, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return e;
    }
    // slots 0..cnt-1 run k = g.khi, g.khi - 1, ...: out[k - kmin]
    hipError_t chunk(const rc_ctx *c, hipStream_t s, const Groups &g, int cnt, int64_t kmin, rc_wb_stats *out)
    {
        hipError_t e = hipMemsetAsync(g.acc, 0, (size_t)cnt * 32, s);
        if (e != hipSuccess) return e;
        k_split_group<<<cnt, RC_CLUSTER_T, 0, s>>>(g);
        // (slots on y: a chunk has fewer than 65536 of them — k-means caps them; k-medoids would need per_slot < 8 KB, i.e.
        // n < 512 >= kmax)
        const dim3 grid((unsigned)((g.n + 64 * RC_CLUSTER_NW - 1) / (64 * RC_CLUSTER_NW)), (unsigned)cnt);
        by_bits(c, [&](auto *D) { k_split_pairs<<<grid, RC_CLUSTER_T, 0, s>>>(D, (decltype(D))L, g, c->eD, sL, c->ltab); });
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(acc.data(), g.acc, (size_t)cnt * 32, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(pairs.data(), g.pairs, (size_t)cnt * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        auto join = [](const unsigned long long *h) {   // (hi, lo) halves -> exact integer
            return (__int128)(long long)h[0] * ((__int128)1 << RC_LO_BITS) + (__int128)(long long)h[1];
        };
        const __int128 uD = join(tot), uL = join(tot + 2), dgL = join(tot + 4);
        const long long all_pairs = (long long)g.n * (g.n - 1) / 2;
        for (int q = 0; q < cnt; ++q) {
            const __int128 wD = join(&acc[(size_t)q * 4]), wL = join(&acc[(size_t)q * 4 + 2]);
            const long long pA = pairs[(size_t)q];
            wb_finish(c, pA, all_pairs - pA, 2 * wD, 2 * wL + dgL, uD - wD, uL - wL, &out[g.khi - q - kmin]);
        }
        return hipSuccess;
    }
};

// the scan's HIP status as the entry point's return code
static int32_t hip_result(rc_ctx *c, const char *who, hipError_t e)
{
    return e == hipSuccess ? RC_OK : fail(c, (e == hipErrorOutOfMemory) ? RC_ERR_OOM : RC_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
}

}  // namespace clu

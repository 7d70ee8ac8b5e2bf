// Batched exact k-medoids on the device: Clustering.jl's kmedoids(D, k; maxiter, tol) with :kmpp seeding, which
// RedClust's fitprior (src/prior.jl:22-128 of the reference) runs for every k of a range and runsampler
// (src/mcmc.jl:516-527) runs once for its starting labels.  Algorithm as restated in DESIGN.md §8.
// Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, rc_ctx).
//
// Exactness: everything works on the context's fixed-point matrix in the caller's point order (Dq_src, int64 or int32
// entries, value = q·2^-eD).  Sums are int64, comparisons are integer comparisons with explicit tie rules, and the
// weighted draws of the seeding use integers only, so a run is a pure function of (D, k, seed): independent of the
// launch geometry, of which other k run beside it and of wave timing.
//
//   * one workgroup per k (slot s of a chunk runs k = khi - s: the largest k is dispatched first);
//   * k_kmed_seed: the k-1 weighted draws of k-medoids++ and the initial assignment, one launch per chunk;
//   * k_kmed_round: one iteration (groups -> medoids -> reassignment -> convergence) of every run still active, one
//     launch per round; a converged run's workgroup exits at once.  The host reads the count of active runs every
//     RC_KMED_POLL rounds — no round trip per k and none per iteration;
//   * the per-k workspace is sized for a chunk of k values bounded by RC_KMED_WS_BYTES (n = 32768 fits).

#define RC_KMED_T 256                   // threads per workgroup
#define RC_KMED_NW (RC_KMED_T / 64)     // waves per workgroup
#define RC_KMED_TAG 0x4B4D4544u         // "KMED": domain tag of the seeding stream, XORed into the high key word
#define RC_KMED_POLL 4                  // rounds between two reads of the active-run counter
#define RC_KMED_WS_BYTES ((size_t)512 << 20)
#define RC_KMED_DONE 1
#define RC_KMED_CONV 2
#define RC_KMED_ERR_EMPTY 4             // a group lost all its points (possible only with a nonzero diagonal entry)
#define RC_KMED_ERR_WEIGHT 8            // every remaining seeding weight is zero (distances that quantise to 0)

namespace kmed {

struct Ws {
    int n, ld;
    int khi;               // k of slot 0; slot s runs k = khi - s
    int kstride;           // per-slot stride of the k-sized arrays (>= khi + 1)
    int *assign;           // [C][n] 0-based medoid index of every point
    int *members;          // [C][n] points grouped by medoid
    long long *wcost;      // [C][n] min cost (seeding) / cost of each candidate medoid (medoid update)
    int *cnt, *off, *cur;  // [C][kstride] group sizes, offsets into members, scatter cursors
    int *med, *bestj;      // [C][kstride] medoids (0-based point indices), best candidate per group
    long long *bestc;      // [C][kstride] smallest candidate cost per group
    long long *tcost;      // [C]
    int *iter, *flags;     // [C]
    unsigned *active;      // [maxiter + 1] runs still active after round r
    unsigned *err;         // OR of the RC_KMED_ERR_* bits of every slot
    // per-k split (rc_kmedoids_scan_split only; null otherwise)
    unsigned long long *acc;  // [C + 2][4]: within sums of slot s (D hi, D lo, logD hi, logD lo: RC_LO_BITS halves as
                              // k_blocksums); row C the upper triangle's totals, row C + 1 (logD's diagonal hi, lo, 0, 0)
    long long *pairs;         // [C] within pairs: Σ_g n_g (n_g - 1) / 2
};

// Philox4x32-10, key (seed_lo, seed_hi ^ "KMED"), counter (step, k, 0, 0): 53 random bits
__device__ __forceinline__ u64 u53(u64 seed, unsigned k, unsigned step)
{
    unsigned c0 = step, c1 = k, c2 = 0, c3 = 0, k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ RC_KMED_TAG;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * (u64)c0, p1 = (u64)0xCD9E8D57u * (u64)c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (((u64)c0 << 32) | c1) >> 11;
}

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

__device__ __forceinline__ long long block_sum(long long v, long long *red /* [RC_KMED_NW] */)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_sum(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int w = 0; w < RC_KMED_NW; ++w) s += red[w];
    __syncthreads();
    return s;
}

// Every point to its nearest medoid, ties to the first medoid in medoid order (strict <); returns the total cost.
template <typename T>
__device__ long long assign_all(const T *__restrict__ D, int n, int ld, const int *med, int k, int *a, long long *red)
{
    long long sum = 0;
    for (int j = threadIdx.x; j < n; j += RC_KMED_T) {
        long long best = (long long)D[(size_t)med[0] * ld + j];
        int bi = 0, i = 1;
        for (; i + 8 <= k; i += 8) {   // eight independent row loads in flight, then the comparisons in medoid order
            long long c[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) c[u] = (long long)D[(size_t)med[i + u] * ld + j];
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c[u] < best) { best = c[u]; bi = i + u; }
        }
        for (; i < k; ++i) {
            const long long c = (long long)D[(size_t)med[i] * ld + j];
            if (c < best) { best = c; bi = i; }
        }
        a[j] = bi;
        sum += best;
    }
    return block_sum(sum, red);
}

// The groups of assignment a (k medoids): sizes cnt, offsets off (exclusive scan over the k sizes, each thread owning a
// contiguous run of groups; off[k] = n), scatter cursors cur and the members grouped by medoid (their order inside a group
// depends on timing: every use of it is order-free).  Returns whether some group is empty (the same answer in every thread).
// Called by every thread of the block; wtot: [RC_KMED_NW] and flag: one int, both in LDS.
__device__ bool group_points(const int *a, int n, int k, int *cnt, int *off, int *cur, int *mem, int *wtot, int *flag)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (threadIdx.x == 0) *flag = 0;
    for (int g = threadIdx.x; g < k; g += RC_KMED_T) cnt[g] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += RC_KMED_T) atomicAdd(&cnt[a[j]], 1);
    __syncthreads();
    const int per = (k + RC_KMED_T - 1) / RC_KMED_T, g0 = min(k, (int)threadIdx.x * per), g1 = min(k, g0 + per);
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
    if (threadIdx.x == 0) off[k] = n;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += RC_KMED_T) mem[atomicAdd(&cur[a[j]], 1)] = j;
    __syncthreads();
    return empty;
}

// k-medoids++ by costs (Clustering.jl initseeds_by_costs!, :kmpp) and the initial assignment.
template <typename T>
__global__ __launch_bounds__(RC_KMED_T) void k_kmed_seed(const T *__restrict__ D, Ws w, u64 seed, int maxiter)
{
    __shared__ long long red[RC_KMED_NW];
    __shared__ int pick;
    const int slot = blockIdx.x, k = w.khi - slot, n = w.n, ld = w.ld;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int *a = w.assign + (size_t)slot * n;
    long long *mc = w.wcost + (size_t)slot * n;
    int *med = w.med + (size_t)slot * w.kstride;
    // each wave owns a contiguous range of points (lanes stride through it: coalesced row reads, and the prefix sums of
    // the draw follow the point order)
    const int seg = (n + RC_KMED_NW - 1) / RC_KMED_NW, lo = min(n, wid * seg), hi = min(n, lo + seg);
    int p = (int)scale53(u53(seed, (unsigned)k, 0), (u64)n);   // first medoid uniform on 0..n-1
    if (threadIdx.x == 0) med[0] = p;
    for (int j = lo + lane; j < hi; j += 64) mc[j] = (j == p) ? 0 : (long long)D[(size_t)p * ld + j];
    unsigned err = 0;
    for (int s = 1; s < k; ++s) {
        if (threadIdx.x == 0) pick = -1;
        long long v = 0;
        for (int j = lo + lane; j < hi; j += 64) v += mc[j];
        v = wave_sum(v);
        if (lane == 0) red[wid] = v;
        __syncthreads();
        long long W = 0, excl = 0;
#pragma unroll
        for (int q = 0; q < RC_KMED_NW; ++q) { if (q < wid) excl += red[q]; W += red[q]; }
        if (W <= 0) { err = RC_KMED_ERR_WEIGHT; break; }   // uniform over the block
        const u64 thr = scale53(u53(seed, (unsigned)k, (unsigned)s), (u64)W);   // 0 <= thr < W
        // the first point whose inclusive prefix sum exceeds thr: exactly one wave's range holds it
        if ((u64)excl <= thr && thr < (u64)(excl + red[wid])) {
            long long base = excl;
            for (int j0 = lo; j0 < hi; j0 += 64) {
                const int j = j0 + lane;
                const long long incl = wave_incl_scan(j < hi ? mc[j] : 0, lane) + base;
                const u64 hit = __ballot(j < hi && (u64)incl > thr);
                if (hit) {
                    if (lane == 0) pick = j0 + __ffsll((unsigned long long)hit) - 1;
                    break;
                }
                base = __shfl(incl, 63);
            }
        }
        __syncthreads();
        p = pick;
        if (p < 0 || p >= n) { err = RC_KMED_ERR_WEIGHT; break; }   // (cannot happen: thr < W; uniform over the block)
        if (threadIdx.x == 0) med[s] = p;
        for (int j = lo + lane; j < hi; j += 64) {
            const long long d = (long long)D[(size_t)p * ld + j];
            mc[j] = (j == p) ? 0 : min(mc[j], d);
        }
        __syncthreads();
    }
    if (err) {
        if (threadIdx.x == 0) { w.flags[slot] = RC_KMED_DONE | err; w.iter[slot] = 0; w.tcost[slot] = 0; atomicOr(w.err, err); }
        return;
    }
    const long long tc = assign_all(D, n, ld, med, k, a, red);
    if (threadIdx.x == 0) {
        w.tcost[slot] = tc;
        w.iter[slot] = 0;
        w.flags[slot] = maxiter <= 0 ? RC_KMED_DONE : 0;
    }
}

// One iteration of Clustering.jl's _kmedoids! loop for every run of the chunk that is still active.
template <typename T>
__global__ __launch_bounds__(RC_KMED_T) void k_kmed_round(const T *__restrict__ D, Ws w, int maxiter, double tol, double qs,
                                                          int round)
{
    __shared__ long long red[RC_KMED_NW];
    __shared__ int wtot[RC_KMED_NW];
    __shared__ int empty;
    const int slot = blockIdx.x;
    if (w.flags[slot] & RC_KMED_DONE) return;
    const int k = w.khi - slot, n = w.n, ld = w.ld;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int *a = w.assign + (size_t)slot * n, *mem = w.members + (size_t)slot * n;
    long long *wc = w.wcost + (size_t)slot * n;
    const size_t ko = (size_t)slot * w.kstride;
    int *cnt = w.cnt + ko, *off = w.off + ko, *cur = w.cur + ko, *med = w.med + ko, *bestj = w.bestj + ko;
    long long *bestc = w.bestc + ko;
    const int t = w.iter[slot] + 1;
    for (int g = threadIdx.x; g < k; g += RC_KMED_T) { bestc[g] = 0x7fffffffffffffffll; bestj[g] = 0x7fffffff; }
    if (group_points(a, n, k, cnt, off, cur, mem, wtot, &empty)) {
        // Clustering.jl asserts here; only a nonzero diagonal entry can get a medoid out of its own group
        if (threadIdx.x == 0) { w.flags[slot] = RC_KMED_DONE | RC_KMED_ERR_EMPTY; atomicOr(w.err, (unsigned)RC_KMED_ERR_EMPTY); }
        return;
    }
    // medoid update: candidate j of group g costs sum_{h in g} D[j, h] (row j: D is symmetric).  One wave per candidate;
    // a large group streams row j masked by the labels, a small one gathers its members' columns
    for (int q = wid; q < n; q += RC_KMED_NW) {
        const int j = mem[q], g = a[j], s = cnt[g];
        long long v = 0;
        if (s > 1) {
            const T *row = D + (size_t)j * ld;
            if ((long long)s * 16 > n) {
                for (int h = lane; h < n; h += 64) v += (a[h] == g) ? (long long)row[h] : 0;
            } else {
                const int lo = off[g];
                for (int x = lo + lane; x < lo + s; x += 64) v += (long long)row[mem[x]];
            }
            v = wave_sum(v);
        }
        if (lane == 0) { wc[q] = v; atomicMin(&bestc[g], v); }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n; q += RC_KMED_T) {   // ties to the lowest point index
        const int j = mem[q], g = a[j];
        if (wc[q] == bestc[g]) atomicMin(&bestj[g], j);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < k; g += RC_KMED_T) med[g] = bestj[g];
    __syncthreads();
    const long long tc = assign_all(D, n, ld, med, k, a, red);
    if (threadIdx.x == 0) {
        const long long prev = w.tcost[slot];
        const long long dq = tc >= prev ? tc - prev : prev - tc;
        const bool conv = (double)dq * qs < tol;   // |tcost - tcost_prev| < tol in units of D
        const bool done = conv || t >= maxiter;
        w.tcost[slot] = tc;
        w.iter[slot] = t;
        w.flags[slot] = (conv ? RC_KMED_CONV : 0) | (done ? RC_KMED_DONE : 0);
        if (!done) atomicAdd(&w.active[round], 1u);
    }
}

// ---- The per-k split of rc_kmedoids_scan_split: Σ D and Σ logD over the pairs i < j of one group under each slot's final
// assignment, in exact integers.  logD entries as the block sums take them: rc_qlog of Dq when the context derives logD
// (L == null), otherwise the stored fixed-point logD in the caller's order (Lq_src).  Row sums fit int64 (quant_exponent);
// sums over rows go through (hi, lo) halves as in k_blocksums.

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
__global__ __launch_bounds__(RC_KMED_T) void k_kmed_split_group(Ws w)
{
    __shared__ long long red[RC_KMED_NW];
    __shared__ int wtot[RC_KMED_NW];
    __shared__ int flag;
    const int slot = blockIdx.x, k = w.khi - slot, n = w.n;
    const size_t ko = (size_t)slot * w.kstride;
    int *cnt = w.cnt + ko;
    (void)group_points(w.assign + (size_t)slot * n, n, k, cnt, w.off + ko, w.cur + ko, w.members + (size_t)slot * n, wtot, &flag);
    long long v = 0;   // (an empty group — a run that ended on a degenerate reassignment — contributes nothing)
    for (int g = threadIdx.x; g < k; g += RC_KMED_T) v += (long long)cnt[g] * (cnt[g] - 1) / 2;
    v = block_sum(v, red);
    if (threadIdx.x == 0) w.pairs[slot] = v;
}

// blockIdx.y = slot; each wave owns 64 consecutive member positions.  A lane whose group has at most 64 members sums its row
// against the group's later positions on its own; the rows of larger groups go through the whole wave one at a time — as the
// medoid update does, a group above n/16 streams the row's tail masked by the labels (pairs i < j by point index), a smaller
// one gathers its later members' columns (pairs by member position).  Within a group every row takes the same path, so each
// unordered pair is summed exactly once.
template <typename T>
__global__ __launch_bounds__(RC_KMED_T) void k_kmed_split_pairs(const T *__restrict__ D, const T *__restrict__ L, Ws w, int eD,
                                                                double sL, const double2 *__restrict__ tab)
{
    const int slot = blockIdx.y, n = w.n, ld = w.ld;
    const int lane = threadIdx.x & 63, q0 = ((int)blockIdx.x * RC_KMED_NW + (threadIdx.x >> 6)) * 64;
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
__global__ __launch_bounds__(RC_KMED_T) void k_kmed_split_total(const T *__restrict__ D, const T *__restrict__ L, int n, int ld,
                                                                int eD, double sL, const double2 *__restrict__ tab,
                                                                unsigned long long *tot /* [8] */)
{
    const int lane = threadIdx.x & 63, i = (int)blockIdx.x * RC_KMED_NW + (threadIdx.x >> 6);
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

}  // namespace kmed

// Runs k = kmax, kmax-1, ..., kmin in chunks; per-k results into totalcost / iterations / converged[k - kmin].  With
// assignments / medoids non-null (kmin == kmax) the single run's labels and medoids (1-based) as well; with split non-null
// the within / between split of every k's final assignment into split[k - kmin].
static int32_t kmed_run(rc_ctx *c, const char *who, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                        double *totalcost, int64_t *iterations, uint8_t *converged, int64_t *assignments, int64_t *medoids,
                        rc_wb_stats *split)
{
    if (!c) return fail(c, RC_ERR_ARG, "%s: NULL ctx", who);
    if (c->broken) return fail(c, RC_ERR_STATE, "%s: the context is void after a failed capacity growth", who);
    if (!totalcost || !iterations || !converged) return fail(c, RC_ERR_ARG, "%s: NULL output", who);
    const int64_t n = c->n;
    if (kmin < 1 || kmax < kmin || kmax > n)
        return fail(c, RC_ERR_ARG, "%s: need 1 <= k <= n (got %lld..%lld, n = %lld)", who, (long long)kmin, (long long)kmax, (long long)n);
    if (maxiter < 0 || maxiter > (1 << 24)) return fail(c, RC_ERR_ARG, "%s: maxiter must be in 0..2^24", who);
    if (!(tol >= 0.0)) return fail(c, RC_ERR_ARG, "%s: tol must be >= 0", who);
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t kstride = (size_t)kmax + 1;
    const size_t per_slot = (size_t)n * 16 + kstride * 28 + 16 + (split ? 40 : 0);
    const int64_t R = kmax - kmin + 1;
    const int64_t C = std::max<int64_t>(1, std::min<int64_t>(R, (int64_t)(RC_KMED_WS_BYTES / per_slot)));
    char *base = nullptr;
    const size_t bytes = (size_t)C * per_slot + (size_t)(maxiter + 2) * sizeof(unsigned) + 16 * 16   // + alignment of the 14 arrays
                         + (split ? 64 + 2 * 16 : 0);                                                  // + the split's totals, 2 arrays
    HIPCHK(c, hipMalloc(&base, bytes));
    kmed::Ws w{};
    {
        char *p = base;
        auto take = [&](size_t b) { char *q = p; p += (b + 15) & ~(size_t)15; return q; };
        w.wcost = (long long *)take((size_t)C * n * 8);
        w.bestc = (long long *)take((size_t)C * kstride * 8);
        w.tcost = (long long *)take((size_t)C * 8);
        w.assign = (int *)take((size_t)C * n * 4);
        w.members = (int *)take((size_t)C * n * 4);
        w.cnt = (int *)take((size_t)C * kstride * 4);
        w.off = (int *)take((size_t)C * kstride * 4);
        w.cur = (int *)take((size_t)C * kstride * 4);
        w.med = (int *)take((size_t)C * kstride * 4);
        w.bestj = (int *)take((size_t)C * kstride * 4);
        w.iter = (int *)take((size_t)C * 4);
        w.flags = (int *)take((size_t)C * 4);
        w.err = (unsigned *)take(4);
        w.active = (unsigned *)take((size_t)(maxiter + 1) * 4);
        if (split) {
            w.acc = (unsigned long long *)take((size_t)(C + 2) * 32);
            w.pairs = (long long *)take((size_t)C * 8);
        }
        if ((size_t)(p - base) > bytes) { (void)hipFree(base); return fail(c, RC_ERR_HIP, "%s: workspace layout", who); }
    }
    w.n = (int)n; w.ld = c->ld; w.kstride = (int)kstride;
    const double qs = std::ldexp(1.0, -c->eD);
    hipStream_t s = c->sA;
    std::vector<long long> h_tc((size_t)C);
    std::vector<int> h_it((size_t)C), h_fl((size_t)C);
    hipError_t e = hipSuccess;
    unsigned h_err = 0;
    // the split: logD entries as the block sums take them (derived: rc_qlog of Dq; stored: Lq_src, the caller's order)
    const void *Lsrc = c->derived ? nullptr : c->Lq_src;
    const double sL = std::ldexp(1.0, c->eL);
    unsigned long long h_tot[8] = {};
    std::vector<unsigned long long> h_acc;
    std::vector<long long> h_pairs;
    if (split) {
        h_acc.resize((size_t)C * 4);
        h_pairs.resize((size_t)C);
        unsigned long long *tot = w.acc + (size_t)C * 4;
        const unsigned nb = (unsigned)((n + RC_KMED_NW - 1) / RC_KMED_NW);
        e = hipMemsetAsync(tot, 0, 64, s);
        if (e == hipSuccess) {
            if (c->bits == 64) kmed::k_kmed_split_total<long long><<<nb, RC_KMED_T, 0, s>>>((const long long *)c->Dq_src, (const long long *)Lsrc, (int)n, c->ld, c->eD, sL, c->ltab, tot);
            else kmed::k_kmed_split_total<int><<<nb, RC_KMED_T, 0, s>>>((const int *)c->Dq_src, (const int *)Lsrc, (int)n, c->ld, c->eD, sL, c->ltab, tot);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h_tot, tot, 64, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    auto join = [](const unsigned long long *h) {   // (hi, lo) halves -> exact integer
        return (__int128)(long long)h[0] * ((__int128)1 << RC_LO_BITS) + (__int128)(long long)h[1];
    };
    for (int64_t khi = kmax; khi >= kmin && e == hipSuccess; khi -= C) {
        const int cnt = (int)std::min<int64_t>(C, khi - kmin + 1);
        w.khi = (int)khi;
        e = hipMemsetAsync(w.err, 0, sizeof(unsigned), s);
        if (e == hipSuccess) e = hipMemsetAsync(w.active, 0, (size_t)(maxiter + 1) * sizeof(unsigned), s);
        if (e != hipSuccess) break;
        if (c->bits == 64) kmed::k_kmed_seed<long long><<<cnt, RC_KMED_T, 0, s>>>((const long long *)c->Dq_src, w, seed, (int)maxiter);
        else kmed::k_kmed_seed<int><<<cnt, RC_KMED_T, 0, s>>>((const int *)c->Dq_src, w, seed, (int)maxiter);
        e = hipGetLastError();
        for (int64_t r = 0; r < maxiter && e == hipSuccess;) {
            const int64_t r1 = std::min<int64_t>(maxiter, r + RC_KMED_POLL);
            for (; r < r1 && e == hipSuccess; ++r) {
                if (c->bits == 64) kmed::k_kmed_round<long long><<<cnt, RC_KMED_T, 0, s>>>((const long long *)c->Dq_src, w, (int)maxiter, tol, qs, (int)r);
                else kmed::k_kmed_round<int><<<cnt, RC_KMED_T, 0, s>>>((const int *)c->Dq_src, w, (int)maxiter, tol, qs, (int)r);
                e = hipGetLastError();
            }
            unsigned act = 0;
            if (e == hipSuccess) e = hipMemcpyAsync(&act, w.active + (r - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess || act == 0) break;
        }
        unsigned ce = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(h_tc.data(), w.tcost, (size_t)cnt * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_it.data(), w.iter, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_fl.data(), w.flags, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&ce, w.err, sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) break;
        h_err |= ce;
        if (h_err) break;
        for (int q = 0; q < cnt; ++q) {
            const int64_t i = khi - q - kmin;
            totalcost[i] = std::ldexp((double)h_tc[(size_t)q], -c->eD);
            iterations[i] = h_it[(size_t)q];
            converged[i] = (h_fl[(size_t)q] & RC_KMED_CONV) ? 1 : 0;
        }
        if (split) {   // (before the next chunk's seeding overwrites the assignments)
            e = hipMemsetAsync(w.acc, 0, (size_t)cnt * 32, s);
            if (e != hipSuccess) break;
            kmed::k_kmed_split_group<<<cnt, RC_KMED_T, 0, s>>>(w);
            // (slots on y: a chunk has fewer than 65536 of them — more would need per_slot < 8 KB, i.e. n < 512 >= kmax)
            const dim3 grid((unsigned)((n + 64 * RC_KMED_NW - 1) / (64 * RC_KMED_NW)), (unsigned)cnt);
            if (c->bits == 64) kmed::k_kmed_split_pairs<long long><<<grid, RC_KMED_T, 0, s>>>((const long long *)c->Dq_src, (const long long *)Lsrc, w, c->eD, sL, c->ltab);
            else kmed::k_kmed_split_pairs<int><<<grid, RC_KMED_T, 0, s>>>((const int *)c->Dq_src, (const int *)Lsrc, w, c->eD, sL, c->ltab);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(h_acc.data(), w.acc, (size_t)cnt * 32, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(h_pairs.data(), w.pairs, (size_t)cnt * 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) break;
            const __int128 uD = join(h_tot), uL = join(h_tot + 2), dgL = join(h_tot + 4);
            const long long all_pairs = (long long)n * (n - 1) / 2;
            for (int q = 0; q < cnt; ++q) {
                const __int128 wD = join(&h_acc[(size_t)q * 4]), wL = join(&h_acc[(size_t)q * 4 + 2]);
                const long long pA = h_pairs[(size_t)q];
                wb_finish(c, pA, all_pairs - pA, 2 * wD, 2 * wL + dgL, uD - wD, uL - wL, &split[khi - q - kmin]);
            }
        }
        if (assignments || medoids) {   // single run: slot 0
            std::vector<int> ha((size_t)n), hm((size_t)kmax);
            e = hipMemcpyAsync(ha.data(), w.assign, (size_t)n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(hm.data(), w.med, (size_t)kmax * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) break;
            if (assignments) for (int64_t j = 0; j < n; ++j) assignments[j] = (int64_t)ha[(size_t)j] + 1;
            if (medoids) for (int64_t g = 0; g < kmax; ++g) medoids[g] = (int64_t)hm[(size_t)g] + 1;
        }
    }
    (void)hipFree(base);
    if (e != hipSuccess) return fail(c, (e == hipErrorOutOfMemory) ? RC_ERR_OOM : RC_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    if (h_err & RC_KMED_ERR_EMPTY)
        return fail(c, RC_ERR_DOMAIN, "%s: a k-medoids group became empty (a point is closer to another medoid than to itself: D has a "
                                      "nonzero diagonal entry)", who);
    if (h_err & RC_KMED_ERR_WEIGHT)
        return fail(c, RC_ERR_DOMAIN, "%s: k-medoids++ seeding found every remaining weight zero (distances that are zero in the "
                                      "stored fixed point: duplicate points?)", who);
    return RC_OK;
}

extern "C" int32_t rc_kmedoids(rc_ctx *c, int64_t k, int64_t maxiter, double tol, uint64_t seed, int64_t *assignments,
                               int64_t *medoids, double *totalcost, int64_t *iterations, uint8_t *converged)
{
    if (!assignments || !medoids) return fail(c, RC_ERR_ARG, "rc_kmedoids: NULL output");
    return kmed_run(c, "rc_kmedoids", k, k, maxiter, tol, seed, totalcost, iterations, converged, assignments, medoids, nullptr);
}

extern "C" int32_t rc_kmedoids_scan(rc_ctx *c, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                                    double *totalcost, int64_t *iterations, uint8_t *converged)
{
    return kmed_run(c, "rc_kmedoids_scan", kmin, kmax, maxiter, tol, seed, totalcost, iterations, converged, nullptr, nullptr, nullptr);
}

extern "C" int32_t rc_kmedoids_scan_split(rc_ctx *c, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                                          double *totalcost, int64_t *iterations, uint8_t *converged, rc_wb_stats *split)
{
    if (!split) return fail(c, RC_ERR_ARG, "rc_kmedoids_scan_split: NULL output");
    return kmed_run(c, "rc_kmedoids_scan_split", kmin, kmax, maxiter, tol, seed, totalcost, iterations, converged, nullptr, nullptr,
                    split);
}

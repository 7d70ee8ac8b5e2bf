// Batched exact k-means on the device: Clustering.jl's kmeans(X, k; maxiter, tol) with :kmpp seeding, which RedClust's
// fitprior / fitprior2 (src/prior.jl:22-128, :151-277 of the reference) run with algo = "k-means" for every k of a range.
// Algorithm as restated in DESIGN.md §8 "k-means (built)".  Included at the end of redclust_hip.hip (same translation
// unit: shares fail(), HIPCHK, rc_ctx, wb_finish and the split kernels of kmedoids.inc.hip).
//
// Exactness: a run is a pure function of (points, k, seed | init) that NumPy reproduces bit for bit (tests/kmeans_ref.py):
//   * squared distances are Σ_c (x_c - m_c)² over ascending c — a subtraction, a multiplication and an addition in f64,
//     never contracted into an fma (every function below that forms one carries fp contract(off));
//   * a centre is the sum of its members in ascending point index, then one division by the count;
//   * the objective is summed in one fixed order (256 strided partials, then a halving tree);
//   * the weighted draws (seeding, repicking an empty group) use integers only: floor(w · 2^s), s fixed per context.
// Nothing depends on the launch geometry, on the tile sizes or on which other k share the launch.
//
//   * slot s of a chunk runs k = khi - s (the largest k first); a finished run's blocks exit at once;
//   * k_kmn_seed (one block per slot): the k weighted draws of k-means++, or the caller's init;
//   * k_kmn_assign (point tiles × slots): every point to its nearest centre — the n·k·dim hot loop.  A thread keeps its
//     point's coordinates in registers and reads centre tiles from LDS (broadcast reads), four centres in flight;
//   * k_kmn_step (one block per slot): the objective and the convergence test of the assignment just made, then — for a
//     run that goes on — the ordered centre update and the repicking of empty groups;
//   * the host reads the count of active runs every RC_KMN_POLL rounds.

#define RC_KMN_T 256
#define RC_KMN_NW (RC_KMN_T / 64)
#define RC_KMN_TAG 0x4B4D4E53u          // "KMNS": domain tag of the draw stream, XORed into the high key word
#define RC_KMN_POLL 4
#define RC_KMN_WS_BYTES ((size_t)512 << 20)
#define RC_KMN_LDS 4096                 // doubles of a centre tile (32 KiB)
#define RC_KMN_DONE 1
#define RC_KMN_CONV 2
#define RC_KMN_ERR_WEIGHT 8             // every weight of a draw is zero (duplicate points)

namespace kmn {

struct Ws {
    int n, dim;
    int khi;               // k of slot 0; slot s runs k = khi - s
    int kstride;           // per-slot stride of the k-sized arrays (>= khi + 1)
    size_t cstride;        // per-slot stride of the centres (kstride · dim)
    const double *X, *XT;  // the points, n×dim and dim×n
    int shift;             // s of the integer draws: weights are floor(w · 2^s)
    int *assign;           // [C][n] 0-based centre of every point
    int *members;          // [C][n] points grouped by centre, ascending inside a group
    double *costs;         // [C][n] squared distance to the own centre (seeding: to the nearest seed)
    double *cen;           // [C][cstride]
    int *cnt, *off, *cur;  // [C][kstride]
    double *objv;          // [C]
    int *iter, *flags, *ndraw;   // [C]; ndraw: draws made so far (the next draw's stream index)
    unsigned *active;      // [maxiter + 2] runs still active after round r
    unsigned *err;
};

// Philox4x32-10, key (seed_lo, seed_hi ^ "KMNS"), counter (draw, k, 0, 0): 53 random bits
__device__ __forceinline__ u64 u53(u64 seed, unsigned k, unsigned draw)
{
    unsigned c0 = draw, c1 = k, c2 = 0, c3 = 0, k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32) ^ RC_KMN_TAG;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u64 p0 = (u64)0xD2511F53u * (u64)c0, p1 = (u64)0xCD9E8D57u * (u64)c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (((u64)c0 << 32) | c1) >> 11;
}

// ‖x_i - x_p‖² over ascending coordinates
__device__ __forceinline__ double dist_pp(const double *__restrict__ X, const double *__restrict__ XT, int n, int dim, int i, int p)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    const double *xp = X + (size_t)p * dim;
    for (int c = 0; c < dim; ++c) {
        const double d = XT[(size_t)c * n + i] - xp[c];
        acc = acc + d * d;
    }
    return acc;
}

// One weighted draw over w[0..n): weights q_j = floor(ldexp(w_j, shift)) as integers, W = Σ q_j, the first index whose inclusive
// prefix sum exceeds floor(u · W / 2^53).  -1 when W == 0.  Called by every thread of the block; the same answer in each.
__device__ int draw_weighted(const double *w, int n, int shift, u64 u, long long *red /* [RC_KMN_NW] */, int *pick)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int seg = (n + RC_KMN_NW - 1) / RC_KMN_NW, lo = min(n, wid * seg), hi = min(n, lo + seg);
    if (threadIdx.x == 0) *pick = -1;
    long long v = 0;
    for (int j = lo + lane; j < hi; j += 64) v += (long long)ldexp(w[j], shift);
    v = kmed::wave_sum(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    long long W = 0, excl = 0;
#pragma unroll
    for (int q = 0; q < RC_KMN_NW; ++q) { if (q < wid) excl += red[q]; W += red[q]; }
    int p = -1;
    if (W > 0) {   // uniform over the block
        const u64 thr = kmed::scale53(u, (u64)W);   // 0 <= thr < W
        if ((u64)excl <= thr && thr < (u64)(excl + red[wid])) {   // exactly one wave's range holds the pick
            long long base = excl;
            for (int j0 = lo; j0 < hi; j0 += 64) {
                const int j = j0 + lane;
                const long long incl = kmed::wave_incl_scan(j < hi ? (long long)ldexp(w[j], shift) : 0, lane) + base;
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

__device__ __forceinline__ void run_failed(const Ws &w, int slot, unsigned err)
{
    if (threadIdx.x == 0) { w.flags[slot] = RC_KMN_DONE | (int)err; atomicOr(w.err, err); }
}

// Seeding: k-means++ by costs (Clustering.jl initseeds!, :kmpp), or the caller's init (0-based point indices).
__global__ __launch_bounds__(RC_KMN_T) void k_kmn_seed(Ws w, u64 seed, const int *__restrict__ init)
{
    __shared__ long long red[RC_KMN_NW];
    __shared__ int pick;
    const int slot = blockIdx.x, k = w.khi - slot, n = w.n, dim = w.dim;
    double *cen = w.cen + (size_t)slot * w.cstride, *mc = w.costs + (size_t)slot * n;
    int *cnt = w.cnt + (size_t)slot * w.kstride;
    for (int g = threadIdx.x; g < k; g += RC_KMN_T) cnt[g] = 0;
    if (threadIdx.x == 0) { w.iter[slot] = 0; w.flags[slot] = 0; w.objv[slot] = 0.0; w.ndraw[slot] = init ? 0 : k; }
    if (init) {
        for (size_t e = threadIdx.x; e < (size_t)k * dim; e += RC_KMN_T) {
            const size_t g = e / (size_t)dim, c = e - g * (size_t)dim;
            cen[e] = w.X[(size_t)init[g] * dim + c];
        }
        return;
    }
    int p = (int)kmed::scale53(u53(seed, (unsigned)k, 0), (u64)n);   // the first centre: uniform on 0..n-1
    for (int c = threadIdx.x; c < dim; c += RC_KMN_T) cen[c] = w.X[(size_t)p * dim + c];
    for (int j = threadIdx.x; j < n; j += RC_KMN_T) mc[j] = (j == p) ? 0.0 : dist_pp(w.X, w.XT, n, dim, j, p);
    __syncthreads();
    for (int s = 1; s < k; ++s) {
        p = draw_weighted(mc, n, w.shift, u53(seed, (unsigned)k, (unsigned)s), red, &pick);
        if (p < 0 || p >= n) { run_failed(w, slot, RC_KMN_ERR_WEIGHT); return; }   // uniform over the block
        for (int c = threadIdx.x; c < dim; c += RC_KMN_T) cen[(size_t)s * dim + c] = w.X[(size_t)p * dim + c];
        for (int j = threadIdx.x; j < n; j += RC_KMN_T) {
            const double d = dist_pp(w.X, w.XT, n, dim, j, p), m = mc[j];
            mc[j] = (j == p) ? 0.0 : (d < m ? d : m);
        }
        __syncthreads();
    }
}

// Every point to its nearest centre, ties to the lowest centre index (strict <, centres visited in ascending order whatever
// the tile size).  blockIdx.y = slot, blockIdx.x = a tile of RC_KMN_T points.  DIMR > 0: dim <= DIMR, the point's
// coordinates live in registers and centre tiles (rows padded with zeros to DIMR: a zero term leaves the sum as it is) in
// LDS; DIMR == 0: any dim, everything from memory.
template <int DIMR>
__global__ __launch_bounds__(RC_KMN_T) void k_kmn_assign(Ws w)
{
#pragma clang fp contract(off)
    const int slot = blockIdx.y;
    if (w.flags[slot] & RC_KMN_DONE) return;
    const int k = w.khi - slot, n = w.n, dim = w.dim;
    const int i = (int)blockIdx.x * RC_KMN_T + (int)threadIdx.x;
    const bool valid = i < n;
    const double *cen = w.cen + (size_t)slot * w.cstride;
    double best = INFINITY;
    int bi = 0;
    if constexpr (DIMR > 0) {
        __shared__ double sm[RC_KMN_LDS];
        constexpr int TJ = RC_KMN_LDS / DIMR;
        double x[DIMR];
#pragma unroll
        for (int c = 0; c < DIMR; ++c) x[c] = (valid && c < dim) ? w.XT[(size_t)c * n + i] : 0.0;
        for (int j0 = 0; j0 < k; j0 += TJ) {
            const int tj = min(TJ, k - j0);
            __syncthreads();
            for (int e = threadIdx.x; e < tj * DIMR; e += RC_KMN_T) {
                const int jj = e / DIMR, c = e - jj * DIMR;
                sm[e] = (c < dim) ? cen[(size_t)(j0 + jj) * dim + c] : 0.0;
            }
            __syncthreads();
            int jj = 0;
            for (; jj + 4 <= tj; jj += 4) {
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                const double *m = sm + jj * DIMR;
#pragma unroll
                for (int c = 0; c < DIMR; ++c) {
                    const double d0 = x[c] - m[c], d1 = x[c] - m[DIMR + c], d2 = x[c] - m[2 * DIMR + c], d3 = x[c] - m[3 * DIMR + c];
                    a0 = a0 + d0 * d0; a1 = a1 + d1 * d1; a2 = a2 + d2 * d2; a3 = a3 + d3 * d3;
                }
                if (a0 < best) { best = a0; bi = j0 + jj; }
                if (a1 < best) { best = a1; bi = j0 + jj + 1; }
                if (a2 < best) { best = a2; bi = j0 + jj + 2; }
                if (a3 < best) { best = a3; bi = j0 + jj + 3; }
            }
            for (; jj < tj; ++jj) {
                double a0 = 0.0;
                const double *m = sm + jj * DIMR;
#pragma unroll
                for (int c = 0; c < DIMR; ++c) {
                    const double d0 = x[c] - m[c];
                    a0 = a0 + d0 * d0;
                }
                if (a0 < best) { best = a0; bi = j0 + jj; }
            }
        }
    } else {
        if (valid)
            for (int j = 0; j < k; ++j) {
                const double *m = cen + (size_t)j * dim;
                double a0 = 0.0;
                for (int c = 0; c < dim; ++c) {
                    const double d0 = w.XT[(size_t)c * n + i] - m[c];
                    a0 = a0 + d0 * d0;
                }
                if (a0 < best) { best = a0; bi = j; }
            }
    }
    if (valid) {
        w.assign[(size_t)slot * n + i] = bi;
        w.costs[(size_t)slot * n + i] = best;
        atomicAdd(&w.cnt[(size_t)slot * w.kstride + bi], 1);
    }
}

// After an assignment: its objective and Clustering.jl's convergence test; for a run that goes on, iteration t + 1's centre
// update (update_centers!) and the repicking of empty groups (repick_unused_centers).  The reassignment is the next launch.
__global__ __launch_bounds__(RC_KMN_T) void k_kmn_step(Ws w, u64 seed, int maxiter, double tol, int round)
{
#pragma clang fp contract(off)
    __shared__ double part[RC_KMN_T];
    __shared__ long long red[RC_KMN_NW];
    __shared__ int wtot[RC_KMN_NW];
    __shared__ int s_empty, s_done, pick;
    const int slot = blockIdx.x;
    if (w.flags[slot] & RC_KMN_DONE) return;
    const int k = w.khi - slot, n = w.n, dim = w.dim;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int *a = w.assign + (size_t)slot * n, *mem = w.members + (size_t)slot * n;
    double *costs = w.costs + (size_t)slot * n, *cen = w.cen + (size_t)slot * w.cstride;
    const size_t ko = (size_t)slot * w.kstride;
    int *cnt = w.cnt + ko, *off = w.off + ko, *cur = w.cur + ko;
    // objv: partial[t] = costs[t] + costs[t + 256] + ..., then p[i] += p[i + h] for h = 128 .. 1
    double ps = 0.0;
    for (int j = tid; j < n; j += RC_KMN_T) ps = ps + costs[j];
    part[tid] = ps;
    __syncthreads();
    for (int h = RC_KMN_T / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] = part[tid] + part[tid + h];
        __syncthreads();
    }
    if (tid == 0) {
        const double objv = part[0], prev = w.objv[slot];
        const int t = w.iter[slot];
        bool conv = false;
        if (t > 0) {
            const double change = objv - prev;
            if (change > tol) { /* the reference warns that the objective went up, and goes on */ }
            else if (k == 1 || fabs(change) < tol) conv = true;
        }
        const bool done = conv || t >= maxiter;
        w.objv[slot] = objv;
        if (done) w.flags[slot] = RC_KMN_DONE | (conv ? RC_KMN_CONV : 0);
        else { w.iter[slot] = t + 1; atomicAdd(&w.active[round], 1u); }
        s_done = done ? 1 : 0;
        s_empty = 0;
    }
    __syncthreads();
    if (s_done) return;   // (the counts of the final assignment stay as they are)
    // offsets of the groups: an exclusive scan over the k sizes, each thread owning a contiguous run of groups
    const int per = (k + RC_KMN_T - 1) / RC_KMN_T, g0 = min(k, tid * per), g1 = min(k, g0 + per);
    int local = 0, my_empty = 0;
    for (int g = g0; g < g1; ++g) { local += cnt[g]; my_empty |= cnt[g] == 0; }
    if (my_empty) s_empty = 1;
    int incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int x = __shfl_up(incl, d);
        if (lane >= d) incl += x;
    }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    const bool empty = s_empty != 0;
    int run = incl - local;
    for (int q = 0; q < wid; ++q) run += wtot[q];
    for (int g = g0; g < g1; ++g) { off[g] = run; cur[g] = run; run += cnt[g]; }
    __syncthreads();
    // members in ascending point index inside every group: one wave walks the points in order, 64 at a time; the lanes
    // that share a label take consecutive places (one atomic per distinct label of the 64)
    if (wid == 0) {
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane, g = (j < n) ? a[j] : -1;
            u64 todo = __ballot(j < n);
            while (todo) {
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const int gl = __shfl(g, leader);
                const u64 m = __ballot(g == gl);
                int base = 0;
                if (lane == leader) base = atomicAdd(&cur[gl], __popcll(m));
                base = __shfl(base, leader);
                if (g == gl) mem[base + __popcll(m & (((u64)1 << lane) - 1))] = j;
                todo &= ~m;
            }
        }
    }
    __syncthreads();
    // centre = (sum of the members in ascending point index, starting from the first member) / count
    for (size_t e = tid; e < (size_t)k * dim; e += RC_KMN_T) {
        const size_t g = e / (size_t)dim, c = e - g * (size_t)dim;
        const int s = cnt[g];
        if (s > 0) {
            const int *mg = mem + off[g];
            double sum = w.X[(size_t)mg[0] * dim + c];
            for (int x = 1; x < s; ++x) sum = sum + w.X[(size_t)mg[x] * dim + c];
            cen[e] = sum / (double)s;
        }
    }
    __syncthreads();
    if (empty) {   // w = copy(costs) (the costs are recomputed by the reassignment); every empty group in ascending index
        int nd = w.ndraw[slot];
        for (int g = 0; g < k; ++g) {
            if (cnt[g] != 0) continue;   // uniform over the block
            const int p = draw_weighted(costs, n, w.shift, u53(seed, (unsigned)k, (unsigned)nd), red, &pick);
            ++nd;
            if (p < 0 || p >= n) { run_failed(w, slot, RC_KMN_ERR_WEIGHT); return; }
            for (int c = tid; c < dim; c += RC_KMN_T) cen[(size_t)g * dim + c] = w.X[(size_t)p * dim + c];
            for (int j = tid; j < n; j += RC_KMN_T) {
                const double d = dist_pp(w.X, w.XT, n, dim, j, p);
                if (d < costs[j]) costs[j] = d;
            }
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0) w.ndraw[slot] = nd;
    }
    for (int g = tid; g < k; g += RC_KMN_T) cnt[g] = 0;   // the reassignment counts afresh
}

}  // namespace kmn

static void kmn_launch_assign(const kmn::Ws &w, dim3 grid, hipStream_t s)
{
    const int d = w.dim;
    if (d <= 4) kmn::k_kmn_assign<4><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 8) kmn::k_kmn_assign<8><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 16) kmn::k_kmn_assign<16><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 24) kmn::k_kmn_assign<24><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 32) kmn::k_kmn_assign<32><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 40) kmn::k_kmn_assign<40><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 48) kmn::k_kmn_assign<48><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 56) kmn::k_kmn_assign<56><<<grid, RC_KMN_T, 0, s>>>(w);
    else if (d <= 64) kmn::k_kmn_assign<64><<<grid, RC_KMN_T, 0, s>>>(w);
    else kmn::k_kmn_assign<0><<<grid, RC_KMN_T, 0, s>>>(w);
}

// Runs k = kmax, kmax-1, ..., kmin in chunks of at most slots_per_chunk (0 = as many as the workspace bound allows); per-k
// results into totalcost / iterations / converged[k - kmin].  A single run (kmin == kmax) also returns whichever of
// assignments / centers / costs / counts is non-null; with split non-null the within / between split of every k's final
// assignment goes into split[k - kmin].
static int32_t kmn_run(rc_ctx *c, const char *who, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                       int64_t slots_per_chunk, const int64_t *init, double *totalcost, int64_t *iterations, uint8_t *converged,
                       int64_t *assignments, double *centers, double *costs, int64_t *counts, rc_wb_stats *split)
{
    if (!c) return fail(c, RC_ERR_ARG, "%s: NULL ctx", who);
    if (c->broken) return fail(c, RC_ERR_STATE, "%s: the context is void after a failed capacity growth", who);
    if (!c->pts || c->dim < 1)
        return fail(c, RC_ERR_STATE, "%s: k-means needs the observations: this context was created from a dissimilarity matrix "
                                     "(use rc_create_from_points)", who);
    if (!totalcost || !iterations || !converged) return fail(c, RC_ERR_ARG, "%s: NULL output", who);
    const int64_t n = c->n, dim = c->dim;
    if (kmin < 1 || kmax < kmin || kmax > n)
        return fail(c, RC_ERR_DOMAIN, "%s: need 1 <= k <= n (got %lld..%lld, n = %lld)", who, (long long)kmin, (long long)kmax, (long long)n);
    if (maxiter < 0 || maxiter > (1 << 24)) return fail(c, RC_ERR_DOMAIN, "%s: maxiter must be in 0..2^24", who);
    if (!(tol >= 0.0)) return fail(c, RC_ERR_DOMAIN, "%s: tol must be >= 0", who);
    if (slots_per_chunk < 0) return fail(c, RC_ERR_ARG, "%s: slots_per_chunk must be >= 0", who);
    std::vector<int> h_init;
    if (init) {
        std::vector<char> seen((size_t)n, 0);
        h_init.resize((size_t)kmax);
        for (int64_t g = 0; g < kmax; ++g) {
            if (init[g] < 1 || init[g] > n)
                return fail(c, RC_ERR_ARG, "%s: init[%lld] = %lld is outside 1..%lld", who, (long long)g, (long long)init[g], (long long)n);
            if (seen[(size_t)(init[g] - 1)])
                return fail(c, RC_ERR_ARG, "%s: init names point %lld twice", who, (long long)init[g]);
            seen[(size_t)(init[g] - 1)] = 1;
            h_init[(size_t)g] = (int)(init[g] - 1);
        }
    }
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t kstride = (size_t)kmax + 1, cstride = kstride * (size_t)dim;
    const size_t per_slot = (size_t)n * 16 + cstride * 8 + kstride * 12 + 8 + 12 + (split ? 40 : 0);
    if (per_slot > RC_KMN_WS_BYTES)
        return fail(c, RC_ERR_OOM, "%s: one run's workspace (n = %lld, dim = %lld, k = %lld: %zu bytes) exceeds the bound of %zu bytes",
                    who, (long long)n, (long long)dim, (long long)kmax, per_slot, (size_t)RC_KMN_WS_BYTES);
    const int64_t R = kmax - kmin + 1;
    int64_t C = std::max<int64_t>(1, std::min<int64_t>(R, (int64_t)(RC_KMN_WS_BYTES / per_slot)));
    C = std::min<int64_t>(C, 65535);   // slots ride on a grid's y
    if (slots_per_chunk > 0) C = std::min<int64_t>(C, slots_per_chunk);
    char *base = nullptr;
    const size_t bytes = (size_t)C * per_slot + (size_t)(maxiter + 2) * sizeof(unsigned) + 16 * 16 + (size_t)kmax * sizeof(int)
                         + (split ? 64 + 2 * 16 : 0);
    HIPCHK(c, hipMalloc(&base, bytes));
    kmn::Ws w{};
    kmed::Ws kw{};
    int *d_init = nullptr;
    {
        char *p = base;
        auto take = [&](size_t b) { char *q = p; p += (b + 15) & ~(size_t)15; return q; };
        w.costs = (double *)take((size_t)C * n * 8);
        w.cen = (double *)take((size_t)C * cstride * 8);
        w.objv = (double *)take((size_t)C * 8);
        w.assign = (int *)take((size_t)C * n * 4);
        w.members = (int *)take((size_t)C * n * 4);
        w.cnt = (int *)take((size_t)C * kstride * 4);
        w.off = (int *)take((size_t)C * kstride * 4);
        w.cur = (int *)take((size_t)C * kstride * 4);
        w.iter = (int *)take((size_t)C * 4);
        w.flags = (int *)take((size_t)C * 4);
        w.ndraw = (int *)take((size_t)C * 4);
        w.err = (unsigned *)take(4);
        w.active = (unsigned *)take((size_t)(maxiter + 2) * 4);
        if (init) d_init = (int *)take((size_t)kmax * 4);
        if (split) {
            kw.acc = (unsigned long long *)take((size_t)(C + 2) * 32);
            kw.pairs = (long long *)take((size_t)C * 8);
        }
        if ((size_t)(p - base) > bytes) { (void)hipFree(base); return fail(c, RC_ERR_HIP, "%s: workspace layout", who); }
    }
    w.n = (int)n; w.dim = (int)dim; w.kstride = (int)kstride; w.cstride = cstride;
    w.X = c->pts; w.XT = c->ptsT; w.shift = c->km_shift;
    kw.n = (int)n; kw.ld = c->ld; kw.kstride = (int)kstride;
    kw.assign = w.assign; kw.members = w.members; kw.cnt = w.cnt; kw.off = w.off; kw.cur = w.cur;
    hipStream_t s = c->sA;
    std::vector<double> h_tc((size_t)C);
    std::vector<int> h_it((size_t)C), h_fl((size_t)C);
    hipError_t e = hipSuccess;
    unsigned h_err = 0;
    if (init) e = hipMemcpyAsync(d_init, h_init.data(), (size_t)kmax * 4, hipMemcpyHostToDevice, s);
    const void *Lsrc = c->derived ? nullptr : c->Lq_src;
    const double sL = std::ldexp(1.0, c->eL);
    unsigned long long h_tot[8] = {};
    std::vector<unsigned long long> h_acc;
    std::vector<long long> h_pairs;
    if (split && e == hipSuccess) {
        h_acc.resize((size_t)C * 4);
        h_pairs.resize((size_t)C);
        unsigned long long *tot = kw.acc + (size_t)C * 4;
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
    const unsigned tiles = (unsigned)((n + RC_KMN_T - 1) / RC_KMN_T);
    for (int64_t khi = kmax; khi >= kmin && e == hipSuccess; khi -= C) {
        const int cnt = (int)std::min<int64_t>(C, khi - kmin + 1);
        w.khi = (int)khi;
        kw.khi = (int)khi;
        e = hipMemsetAsync(w.err, 0, sizeof(unsigned), s);
        if (e == hipSuccess) e = hipMemsetAsync(w.active, 0, (size_t)(maxiter + 2) * sizeof(unsigned), s);
        if (e != hipSuccess) break;
        kmn::k_kmn_seed<<<cnt, RC_KMN_T, 0, s>>>(w, seed, d_init);
        e = hipGetLastError();
        // round r: the assignment under the centres of iteration r (r = 0: the seeds), then its test and the next update;
        // a run whose t reaches maxiter ends in round maxiter at the latest
        for (int64_t r = 0; r <= maxiter && e == hipSuccess;) {
            const int64_t r1 = std::min<int64_t>(maxiter + 1, r + RC_KMN_POLL);
            for (; r < r1 && e == hipSuccess; ++r) {
                kmn_launch_assign(w, dim3(tiles, (unsigned)cnt), s);
                kmn::k_kmn_step<<<cnt, RC_KMN_T, 0, s>>>(w, seed, (int)maxiter, tol, (int)r);
                e = hipGetLastError();
            }
            unsigned act = 0;
            if (e == hipSuccess) e = hipMemcpyAsync(&act, w.active + (r - 1), sizeof(unsigned), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess || act == 0) break;
        }
        unsigned ce = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(h_tc.data(), w.objv, (size_t)cnt * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_it.data(), w.iter, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_fl.data(), w.flags, (size_t)cnt * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&ce, w.err, sizeof(unsigned), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) break;
        h_err |= ce;
        if (h_err) break;
        for (int q = 0; q < cnt; ++q) {
            const int64_t i = khi - q - kmin;
            totalcost[i] = h_tc[(size_t)q];
            iterations[i] = h_it[(size_t)q];
            converged[i] = (h_fl[(size_t)q] & RC_KMN_CONV) ? 1 : 0;
        }
        if (assignments || centers || costs || counts) {   // single run: slot 0 (before the split regroups the points)
            std::vector<int> ha((size_t)n), hc((size_t)kmax);
            e = hipMemcpyAsync(ha.data(), w.assign, (size_t)n * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), w.cnt, (size_t)kmax * 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && centers) e = hipMemcpyAsync(centers, w.cen, (size_t)kmax * dim * 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess && costs) e = hipMemcpyAsync(costs, w.costs, (size_t)n * 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) break;
            if (assignments) for (int64_t j = 0; j < n; ++j) assignments[j] = (int64_t)ha[(size_t)j] + 1;
            if (counts) for (int64_t g = 0; g < kmax; ++g) counts[g] = (int64_t)hc[(size_t)g];
        }
        if (split) {   // (before the next chunk's seeding overwrites the assignments)
            e = hipMemsetAsync(kw.acc, 0, (size_t)cnt * 32, s);
            if (e != hipSuccess) break;
            kmed::k_kmed_split_group<<<cnt, RC_KMED_T, 0, s>>>(kw);
            const dim3 grid((unsigned)((n + 64 * RC_KMED_NW - 1) / (64 * RC_KMED_NW)), (unsigned)cnt);
            if (c->bits == 64) kmed::k_kmed_split_pairs<long long><<<grid, RC_KMED_T, 0, s>>>((const long long *)c->Dq_src, (const long long *)Lsrc, kw, c->eD, sL, c->ltab);
            else kmed::k_kmed_split_pairs<int><<<grid, RC_KMED_T, 0, s>>>((const int *)c->Dq_src, (const int *)Lsrc, kw, c->eD, sL, c->ltab);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(h_acc.data(), kw.acc, (size_t)cnt * 32, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(h_pairs.data(), kw.pairs, (size_t)cnt * 8, hipMemcpyDeviceToHost, s);
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
    }
    (void)hipFree(base);
    if (e != hipSuccess) return fail(c, (e == hipErrorOutOfMemory) ? RC_ERR_OOM : RC_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    if (h_err & RC_KMN_ERR_WEIGHT)
        return fail(c, RC_ERR_DOMAIN, "%s: a weighted draw (k-means++ seeding or the repicking of an empty group) found every weight "
                                      "zero: fewer distinct points than k (duplicate observations?)", who);
    return RC_OK;
}

extern "C" int32_t rc_kmeans(rc_ctx *c, int64_t k, int64_t maxiter, double tol, uint64_t seed, const int64_t *init_or_null,
                             int64_t *assignments, double *centers, double *costs, int64_t *counts, double *totalcost,
                             int64_t *iterations, uint8_t *converged)
{
    if (!assignments || !centers || !costs || !counts) return fail(c, RC_ERR_ARG, "rc_kmeans: NULL output");
    return kmn_run(c, "rc_kmeans", k, k, maxiter, tol, seed, 0, init_or_null, totalcost, iterations, converged, assignments, centers,
                   costs, counts, nullptr);
}

extern "C" int32_t rc_kmeans_scan(rc_ctx *c, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                                  int64_t slots_per_chunk, double *totalcost, int64_t *iterations, uint8_t *converged)
{
    return kmn_run(c, "rc_kmeans_scan", kmin, kmax, maxiter, tol, seed, slots_per_chunk, nullptr, totalcost, iterations, converged,
                   nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int32_t rc_kmeans_scan_split(rc_ctx *c, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                                        int64_t slots_per_chunk, double *totalcost, int64_t *iterations, uint8_t *converged,
                                        rc_wb_stats *split)
{
    if (!split) return fail(c, RC_ERR_ARG, "rc_kmeans_scan_split: NULL output");
    return kmn_run(c, "rc_kmeans_scan_split", kmin, kmax, maxiter, tol, seed, slots_per_chunk, nullptr, totalcost, iterations,
                   converged, nullptr, nullptr, nullptr, nullptr, split);
}

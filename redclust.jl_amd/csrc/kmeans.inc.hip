// Batched exact k-means on the device: Clustering.jl's kmeans(X, k; maxiter, tol) with :kmpp seeding, which RedClust's
// fitprior / fitprior2 (src/prior.jl:22-128, :151-277 of the reference) run with algo = "k-means" for every k of a range.
// Algorithm as restated in DESIGN.md §8 "k-means (built)".  Included at the end of redclust_hip.hip after cluster.inc.hip (same
// translation unit: shares fail(), HIPCHK, rc_ctx, rc_philox and everything in namespace clu: the geometry, the reductions,
// the weighted draw, the group offsets, the split and the host side of a scan).
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
//     run that goes on — the ordered centre update and the repicking of empty groups.

#define RC_KMN_LDS 4096                 // doubles of a centre tile (32 KiB)
#define RC_KMN_ERR_WEIGHT 8             // every weight of a draw is zero (duplicate points)

namespace kmn {

using namespace clu;

struct Ws : Groups {       // (labels: 0-based centres; members ascending inside a group)
    int dim;
    size_t cstride;        // per-slot stride of the centres (kstride · dim)
    const double *X, *XT;  // the points, n×dim and dim×n
    int shift;             // s of the integer draws: weights are floor(w · 2^s)
    double *costs;         // [C][n] squared distance to the own centre (seeding: to the nearest seed)
    double *cen;           // [C][cstride]
    double *objv;          // [C]
    int *iter, *flags, *ndraw;   // [C]; ndraw: draws made so far (the next draw's stream index)
    unsigned *active;      // [maxiter + 2] runs still active after round r
    unsigned *err;
};

// the draw stream: 53 random bits of draw `draw` of run k
__device__ __forceinline__ u64 u53(u64 seed, unsigned k, unsigned draw)
{
    return rc_bits53(rc_philox(draw, k, 0, 0, (unsigned)seed, (unsigned)(seed >> 32) ^ RC_KMN_TAG));
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

// One weighted draw over w[0..n) with the integer weights q_j = floor(ldexp(w_j, shift)); -1 when every q_j is zero
__device__ int draw_costs(const double *w, int n, int shift, u64 u, long long *red /* [RC_CLUSTER_NW] */, int *pick)
{
    return draw_weighted([w, shift](int j) { return (long long)ldexp(w[j], shift); }, n, u, red, pick);
}

__device__ __forceinline__ void run_failed(const Ws &w, int slot, unsigned err)
{
    if (threadIdx.x == 0) { w.flags[slot] = RC_CLUSTER_DONE | (int)err; atomicOr(w.err, err); }
}

// Seeding: k-means++ by costs (Clustering.jl initseeds!, :kmpp), or the caller's init (0-based point indices).
__global__ __launch_bounds__(RC_CLUSTER_T) void k_kmn_seed(Ws w, u64 seed, const int *__restrict__ init)
{
    __shared__ long long red[RC_CLUSTER_NW];
    __shared__ int pick;
    const int slot = blockIdx.x, k = w.khi - slot, n = w.n, dim = w.dim;
    double *cen = w.cen + (size_t)slot * w.cstride, *mc = w.costs + (size_t)slot * n;
    int *cnt = w.cnt + (size_t)slot * w.kstride;
    for (int g = threadIdx.x; g < k; g += RC_CLUSTER_T) cnt[g] = 0;
    if (threadIdx.x == 0) { w.iter[slot] = 0; w.flags[slot] = 0; w.objv[slot] = 0.0; w.ndraw[slot] = init ? 0 : k; }
    if (init) {
        for (size_t e = threadIdx.x; e < (size_t)k * dim; e += RC_CLUSTER_T) {
            const size_t g = e / (size_t)dim, c = e - g * (size_t)dim;
            cen[e] = w.X[(size_t)init[g] * dim + c];
        }
        return;
    }
    int p = (int)scale53(u53(seed, (unsigned)k, 0), (u64)n);   // the first centre: uniform on 0..n-1
    for (int c = threadIdx.x; c < dim; c += RC_CLUSTER_T) cen[c] = w.X[(size_t)p * dim + c];
    for (int j = threadIdx.x; j < n; j += RC_CLUSTER_T) mc[j] = (j == p) ? 0.0 : dist_pp(w.X, w.XT, n, dim, j, p);
    __syncthreads();
    for (int s = 1; s < k; ++s) {
        p = draw_costs(mc, n, w.shift, u53(seed, (unsigned)k, (unsigned)s), red, &pick);
        if (p < 0 || p >= n) { run_failed(w, slot, RC_KMN_ERR_WEIGHT); return; }   // uniform over the block
        for (int c = threadIdx.x; c < dim; c += RC_CLUSTER_T) cen[(size_t)s * dim + c] = w.X[(size_t)p * dim + c];
        for (int j = threadIdx.x; j < n; j += RC_CLUSTER_T) {
            const double d = dist_pp(w.X, w.XT, n, dim, j, p), m = mc[j];
            mc[j] = (j == p) ? 0.0 : (d < m ? d : m);
        }
        __syncthreads();
    }
}

// Every point to its nearest centre, ties to the lowest centre index (strict <, centres visited in ascending order whatever
// the tile size).  blockIdx.y = slot, blockIdx.x = a tile of RC_CLUSTER_T points.  DIMR > 0: dim <= DIMR, the point's
// coordinates live in registers and centre tiles (rows padded with zeros to DIMR: a zero term leaves the sum as it is) in
// LDS; DIMR == 0: any dim, everything from memory.
template <int DIMR>
__global__ __launch_bounds__(RC_CLUSTER_T) void k_kmn_assign(Ws w)
{
#pragma clang fp contract(off)
    const int slot = blockIdx.y;
    if (w.flags[slot] & RC_CLUSTER_DONE) return;
    const int k = w.khi - slot, n = w.n, dim = w.dim;
    const int i = (int)blockIdx.x * RC_CLUSTER_T + (int)threadIdx.x;
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
            for (int e = threadIdx.x; e < tj * DIMR; e += RC_CLUSTER_T) {
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
__global__ __launch_bounds__(RC_CLUSTER_T) void k_kmn_step(Ws w, u64 seed, int maxiter, double tol, int round)
{
#pragma clang fp contract(off)
    __shared__ double part[RC_CLUSTER_T];
    __shared__ long long red[RC_CLUSTER_NW];
    __shared__ int wtot[RC_CLUSTER_NW];
    __shared__ int s_empty, s_done, pick;
    const int slot = blockIdx.x;
    if (w.flags[slot] & RC_CLUSTER_DONE) return;
    const int k = w.khi - slot, n = w.n, dim = w.dim;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int *a = w.assign + (size_t)slot * n, *mem = w.members + (size_t)slot * n;
    double *costs = w.costs + (size_t)slot * n, *cen = w.cen + (size_t)slot * w.cstride;
    const size_t ko = (size_t)slot * w.kstride;
    int *cnt = w.cnt + ko, *off = w.off + ko, *cur = w.cur + ko;
    // objv: partial[t] = costs[t] + costs[t + 256] + ..., then p[i] += p[i + h] for h = 128 .. 1
    double ps = 0.0;
    for (int j = tid; j < n; j += RC_CLUSTER_T) ps = ps + costs[j];
    part[tid] = ps;
    __syncthreads();
    for (int h = RC_CLUSTER_T / 2; h > 0; h >>= 1) {
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
        if (done) w.flags[slot] = RC_CLUSTER_DONE | (conv ? RC_CLUSTER_CONV : 0);
        else { w.iter[slot] = t + 1; atomicAdd(&w.active[round], 1u); }
        s_done = done ? 1 : 0;
        s_empty = 0;
    }
    __syncthreads();
    if (s_done) return;   // (the counts of the final assignment stay as they are)
    const bool empty = group_offsets(cnt, k, off, cur, wtot, &s_empty);
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
    for (size_t e = tid; e < (size_t)k * dim; e += RC_CLUSTER_T) {
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
            const int p = draw_costs(costs, n, w.shift, u53(seed, (unsigned)k, (unsigned)nd), red, &pick);
            ++nd;
            if (p < 0 || p >= n) { run_failed(w, slot, RC_KMN_ERR_WEIGHT); return; }
            for (int c = tid; c < dim; c += RC_CLUSTER_T) cen[(size_t)g * dim + c] = w.X[(size_t)p * dim + c];
            for (int j = tid; j < n; j += RC_CLUSTER_T) {
                const double d = dist_pp(w.X, w.XT, n, dim, j, p);
                if (d < costs[j]) costs[j] = d;
            }
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0) w.ndraw[slot] = nd;
    }
    for (int g = tid; g < k; g += RC_CLUSTER_T) cnt[g] = 0;   // the reassignment counts afresh
}

}  // namespace kmn

static void kmn_launch_assign(const kmn::Ws &w, dim3 grid, hipStream_t s)
{
    const int d = w.dim;
    if (d <= 4) kmn::k_kmn_assign<4><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 8) kmn::k_kmn_assign<8><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 16) kmn::k_kmn_assign<16><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 24) kmn::k_kmn_assign<24><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 32) kmn::k_kmn_assign<32><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 40) kmn::k_kmn_assign<40><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 48) kmn::k_kmn_assign<48><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 56) kmn::k_kmn_assign<56><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else if (d <= 64) kmn::k_kmn_assign<64><<<grid, RC_CLUSTER_T, 0, s>>>(w);
    else kmn::k_kmn_assign<0><<<grid, RC_CLUSTER_T, 0, s>>>(w);
}

// Runs k = kmax, kmax-1, ..., kmin in chunks of at most slots_per_chunk (0 = as many as the workspace bound allows); per-k
// results into totalcost / iterations / converged[k - kmin].  A single run (kmin == kmax) also returns whichever of
// assignments / centers / costs / counts is non-null; with split non-null the within / between split of every k's final
// assignment goes into split[k - kmin].
static int32_t kmn_run(rc_ctx *c, const char *who, int64_t kmin, int64_t kmax, int64_t maxiter, double tol, uint64_t seed,
                       int64_t slots_per_chunk, const int64_t *init, double *totalcost, int64_t *iterations, uint8_t *converged,
                       int64_t *assignments, double *centers, double *costs, int64_t *counts, rc_wb_stats *split)
{
    int32_t rc = clu::check_ctx(c, who);
    if (rc != RC_OK) return rc;
    if (!c->pts || c->dim < 1)
        return fail(c, RC_ERR_STATE, "%s: k-means needs the observations: this context was created from a dissimilarity matrix "
                                     "(use rc_create_from_points)", who);
    rc = clu::check_range(c, who, RC_ERR_DOMAIN, totalcost && iterations && converged, kmin, kmax, maxiter, tol);
    if (rc != RC_OK) return rc;
    const int64_t n = c->n, dim = c->dim;
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
    const size_t per_slot = (size_t)n * 16 + cstride * 8 + kstride * 12 + 8 + 12 + (split ? clu::Split::PER_SLOT : 0);
    if (per_slot > RC_CLUSTER_WS_BYTES)
        return fail(c, RC_ERR_OOM, "%s: one run's workspace (n = %lld, dim = %lld, k = %lld: %zu bytes) exceeds the bound of %zu bytes",
                    who, (long long)n, (long long)dim, (long long)kmax, per_slot, (size_t)RC_CLUSTER_WS_BYTES);
    int64_t C = std::max<int64_t>(1, std::min<int64_t>(kmax - kmin + 1, (int64_t)(RC_CLUSTER_WS_BYTES / per_slot)));
    C = std::min<int64_t>(C, 65535);   // slots ride on a grid's y
    if (slots_per_chunk > 0) C = std::min<int64_t>(C, slots_per_chunk);
    clu::Workspace ws;
    HIPCHK(c, ws.alloc((size_t)C * per_slot + (size_t)(maxiter + 2) * sizeof(unsigned) + 16 * 16 + (size_t)kmax * sizeof(int)
                       + (split ? clu::Split::FIXED : 0)));
    kmn::Ws w{};
    clu::Split sp;
    int *d_init = nullptr;
    w.costs = ws.take<double>((size_t)C * n);
    w.cen = ws.take<double>((size_t)C * cstride);
    w.objv = ws.take<double>((size_t)C);
    w.assign = ws.take<int>((size_t)C * n);
    w.members = ws.take<int>((size_t)C * n);
    w.cnt = ws.take<int>((size_t)C * kstride);
    w.off = ws.take<int>((size_t)C * kstride);
    w.cur = ws.take<int>((size_t)C * kstride);
    w.iter = ws.take<int>((size_t)C);
    w.flags = ws.take<int>((size_t)C);
    w.ndraw = ws.take<int>((size_t)C);
    w.err = ws.take<unsigned>(1);
    w.active = ws.take<unsigned>((size_t)(maxiter + 2));
    if (init) d_init = ws.take<int>((size_t)kmax);
    if (split) sp.carve(ws, w, C);
    if (ws.overflow()) return fail(c, RC_ERR_HIP, "%s: workspace layout", who);
    w.n = (int)n; w.ld = c->ld; w.dim = (int)dim; w.kstride = (int)kstride; w.cstride = cstride;
    w.X = c->pts; w.XT = c->ptsT; w.shift = c->km_shift;
    hipStream_t s = c->sA;
    clu::Status<double> st(C);
    hipError_t e = hipSuccess;
    if (init) e = hipMemcpyAsync(d_init, h_init.data(), (size_t)kmax * 4, hipMemcpyHostToDevice, s);
    if (split && e == hipSuccess) e = sp.begin(c, s, w, C);
    const unsigned tiles = (unsigned)((n + RC_CLUSTER_T - 1) / RC_CLUSTER_T);
    for (int64_t khi = kmax; khi >= kmin && e == hipSuccess; khi -= C) {
        const int cnt = (int)std::min<int64_t>(C, khi - kmin + 1);
        w.khi = (int)khi;
        e = hipMemsetAsync(w.err, 0, sizeof(unsigned), s);
        if (e == hipSuccess) e = hipMemsetAsync(w.active, 0, (size_t)(maxiter + 2) * sizeof(unsigned), s);
        if (e != hipSuccess) break;
        kmn::k_kmn_seed<<<cnt, RC_CLUSTER_T, 0, s>>>(w, seed, d_init);
        // round r: the assignment under the centres of iteration r (r = 0: the seeds), then its test and the next update;
        // a run whose t reaches maxiter ends in round maxiter at the latest
        e = clu::run_rounds(s, maxiter + 1, w.active, [&](int64_t r) {
            kmn_launch_assign(w, dim3(tiles, (unsigned)cnt), s);
            kmn::k_kmn_step<<<cnt, RC_CLUSTER_T, 0, s>>>(w, seed, (int)maxiter, tol, (int)r);
        });
        if (e == hipSuccess) e = st.read(s, cnt, w.objv, w.iter, w.flags, w.err);
        if (e != hipSuccess || st.err) break;
        for (int q = 0; q < cnt; ++q) {
            const int64_t i = khi - q - kmin;
            totalcost[i] = st.cost[(size_t)q];
            iterations[i] = st.iter[(size_t)q];
            converged[i] = (st.flags[(size_t)q] & RC_CLUSTER_CONV) ? 1 : 0;
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
        if (split) {
            e = sp.chunk(c, s, w, cnt, kmin, split);
            if (e != hipSuccess) break;
        }
    }
    rc = clu::hip_result(c, who, e);
    if (rc != RC_OK) return rc;
    if (st.err & RC_KMN_ERR_WEIGHT)
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

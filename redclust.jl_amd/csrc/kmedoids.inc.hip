// Batched exact k-medoids on the device: Clustering.jl's kmedoids(D, k; maxiter, tol) with :kmpp seeding, which
// RedClust's fitprior (src/prior.jl:22-128 of the reference) runs for every k of a range and runsampler
// (src/mcmc.jl:516-527) runs once for its starting labels.  Algorithm as restated in DESIGN.md §8.
// Included at the end of redclust_hip.hip after cluster.inc.hip (same translation unit: shares fail(), HIPCHK, rc_ctx,
// rc_philox and everything in namespace clu: the geometry, the reductions, the weighted draw, the grouping, the split and
// the host side of a scan).
//
// Exactness: everything works on the context's fixed-point matrix in the caller's point order (Dq_src, int64 or int32
// entries, value = q·2^-eD).  Sums are int64, comparisons are integer comparisons with explicit tie rules, and the
// weighted draws of the seeding use integers only, so a run is a pure function of (D, k, seed): independent of the
// launch geometry, of which other k run beside it and of wave timing.
//
//   * one workgroup per k (slot s of a chunk runs k = khi - s: the largest k is dispatched first);
//   * k_kmed_seed: the k-1 weighted draws of k-medoids++ and the initial assignment, one launch per chunk;
//   * k_kmed_round: one iteration (groups -> medoids -> reassignment -> convergence) of every run still active, one
//     launch per round; a converged run's workgroup exits at once;
//   * the per-k workspace is sized for a chunk of k values bounded by RC_CLUSTER_WS_BYTES (n = 32768 fits).

#define RC_KMED_ERR_EMPTY 4             // a group lost all its points (possible only with a nonzero diagonal entry)
#define RC_KMED_ERR_WEIGHT 8            // every remaining seeding weight is zero (distances that quantise to 0)

namespace kmed {

using namespace clu;

struct Ws : Groups {       // (labels: 0-based medoid indices)
    long long *wcost;      // [C][n] min cost (seeding) / cost of each candidate medoid (medoid update)
    int *med, *bestj;      // [C][kstride] medoids (0-based point indices), best candidate per group
    long long *bestc;      // [C][kstride] smallest candidate cost per group
    long long *tcost;      // [C]
    int *iter, *flags;     // [C]
    unsigned *active;      // [maxiter + 1] runs still active after round r
    unsigned *err;         // OR of the RC_KMED_ERR_* bits of every slot
};

// the seeding stream: 53 random bits of draw `step` of run k
__device__ __forceinline__ u64 u53(u64 seed, unsigned k, unsigned step)
{
    return rc_bits53(rc_philox(step, k, 0, 0, (unsigned)seed, (unsigned)(seed >> 32) ^ RC_KMED_TAG));
}

// Every point to its nearest medoid, ties to the first medoid in medoid order (strict <); returns the total cost.
template <typename T>
__device__ long long assign_all(const T *__restrict__ D, int n, int ld, const int *med, int k, int *a, long long *red)
{
    long long sum = 0;
    for (int j = threadIdx.x; j < n; j += RC_CLUSTER_T) {
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

// k-medoids++ by costs (Clustering.jl initseeds_by_costs!, :kmpp) and the initial assignment.
template <typename T>
__global__ __launch_bounds__(RC_CLUSTER_T) void k_kmed_seed(const T *__restrict__ D, Ws w, u64 seed, int maxiter)
{
    __shared__ long long red[RC_CLUSTER_NW];
    __shared__ int pick;
    const int slot = blockIdx.x, k = w.khi - slot, n = w.n, ld = w.ld;
    const int lane = threadIdx.x & 63;
    int *a = w.assign + (size_t)slot * n;
    long long *mc = w.wcost + (size_t)slot * n;
    int *med = w.med + (size_t)slot * w.kstride;
    // each wave keeps the weights of the range the draw reads from it (lanes stride through it: coalesced row reads)
    int lo, hi;
    wave_range(n, lo, hi);
    int p = (int)scale53(u53(seed, (unsigned)k, 0), (u64)n);   // first medoid uniform on 0..n-1
    if (threadIdx.x == 0) med[0] = p;
    for (int j = lo + lane; j < hi; j += 64) mc[j] = (j == p) ? 0 : (long long)D[(size_t)p * ld + j];
    unsigned err = 0;
    for (int s = 1; s < k; ++s) {
        p = draw_weighted([mc](int j) { return mc[j]; }, n, u53(seed, (unsigned)k, (unsigned)s), red, &pick);
        if (p < 0 || p >= n) { err = RC_KMED_ERR_WEIGHT; break; }   // every weight zero; uniform over the block
        if (threadIdx.x == 0) med[s] = p;
        for (int j = lo + lane; j < hi; j += 64) {
            const long long d = (long long)D[(size_t)p * ld + j];
            mc[j] = (j == p) ? 0 : min(mc[j], d);
        }
        __syncthreads();
    }
    if (err) {
        if (threadIdx.x == 0) { w.flags[slot] = RC_CLUSTER_DONE | err; w.iter[slot] = 0; w.tcost[slot] = 0; atomicOr(w.err, err); }
        return;
    }
    const long long tc = assign_all(D, n, ld, med, k, a, red);
    if (threadIdx.x == 0) {
        w.tcost[slot] = tc;
        w.iter[slot] = 0;
        w.flags[slot] = maxiter <= 0 ? RC_CLUSTER_DONE : 0;
    }
}

// One iteration of Clustering.jl's _kmedoids! loop for every run of the chunk that is still active.
template <typename T>
__global__ __launch_bounds__(RC_CLUSTER_T) void k_kmed_round(const T *__restrict__ D, Ws w, int maxiter, double tol, double qs,
                                                             int round)
{
    __shared__ long long red[RC_CLUSTER_NW];
    __shared__ int wtot[RC_CLUSTER_NW];
    __shared__ int empty;
    const int slot = blockIdx.x;
    if (w.flags[slot] & RC_CLUSTER_DONE) return;
    const int k = w.khi - slot, n = w.n, ld = w.ld;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int *a = w.assign + (size_t)slot * n, *mem = w.members + (size_t)slot * n;
    long long *wc = w.wcost + (size_t)slot * n;
    const size_t ko = (size_t)slot * w.kstride;
    int *cnt = w.cnt + ko, *off = w.off + ko, *cur = w.cur + ko, *med = w.med + ko, *bestj = w.bestj + ko;
    long long *bestc = w.bestc + ko;
    const int t = w.iter[slot] + 1;
    for (int g = threadIdx.x; g < k; g += RC_CLUSTER_T) { bestc[g] = 0x7fffffffffffffffll; bestj[g] = 0x7fffffff; }
    if (group_points(a, n, k, cnt, off, cur, mem, wtot, &empty)) {
        // Clustering.jl asserts here; only a nonzero diagonal entry can get a medoid out of its own group
        if (threadIdx.x == 0) { w.flags[slot] = RC_CLUSTER_DONE | RC_KMED_ERR_EMPTY; atomicOr(w.err, (unsigned)RC_KMED_ERR_EMPTY); }
        return;
    }
    // medoid update: candidate j of group g costs sum_{h in g} D[j, h] (row j: D is symmetric).  One wave per candidate;
    // a large group streams row j masked by the labels, a small one gathers its members' columns
    for (int q = wid; q < n; q += RC_CLUSTER_NW) {
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
    for (int q = threadIdx.x; q < n; q += RC_CLUSTER_T) {   // ties to the lowest point index
        const int j = mem[q], g = a[j];
        if (wc[q] == bestc[g]) atomicMin(&bestj[g], j);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < k; g += RC_CLUSTER_T) med[g] = bestj[g];
    __syncthreads();
    const long long tc = assign_all(D, n, ld, med, k, a, red);
    if (threadIdx.x == 0) {
        const long long prev = w.tcost[slot];
        const long long dq = tc >= prev ? tc - prev : prev - tc;
        const bool conv = (double)dq * qs < tol;   // |tcost - tcost_prev| < tol in units of D
        const bool done = conv || t >= maxiter;
        w.tcost[slot] = tc;
        w.iter[slot] = t;
        w.flags[slot] = (conv ? RC_CLUSTER_CONV : 0) | (done ? RC_CLUSTER_DONE : 0);
        if (!done) atomicAdd(&w.active[round], 1u);
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
    int32_t rc = clu::check_ctx(c, who);
    if (rc == RC_OK) rc = clu::check_range(c, who, RC_ERR_ARG, totalcost && iterations && converged, kmin, kmax, maxiter, tol);
    if (rc != RC_OK) return rc;
    const int64_t n = c->n;
    HIPCHK(c, hipSetDevice(c->dev));
    const size_t kstride = (size_t)kmax + 1;
    const size_t per_slot = (size_t)n * 16 + kstride * 28 + 16 + (split ? clu::Split::PER_SLOT : 0);
    const int64_t C = std::max<int64_t>(1, std::min<int64_t>(kmax - kmin + 1, (int64_t)(RC_CLUSTER_WS_BYTES / per_slot)));
    clu::Workspace ws;
    HIPCHK(c, ws.alloc((size_t)C * per_slot + (size_t)(maxiter + 2) * sizeof(unsigned) + 16 * 16   // + alignment of the 14 arrays
                       + (split ? clu::Split::FIXED : 0)));
    kmed::Ws w{};
    clu::Split sp;
    w.wcost = ws.take<long long>((size_t)C * n);
    w.bestc = ws.take<long long>((size_t)C * kstride);
    w.tcost = ws.take<long long>((size_t)C);
    w.assign = ws.take<int>((size_t)C * n);
    w.members = ws.take<int>((size_t)C * n);
    w.cnt = ws.take<int>((size_t)C * kstride);
    w.off = ws.take<int>((size_t)C * kstride);
    w.cur = ws.take<int>((size_t)C * kstride);
    w.med = ws.take<int>((size_t)C * kstride);
    w.bestj = ws.take<int>((size_t)C * kstride);
    w.iter = ws.take<int>((size_t)C);
    w.flags = ws.take<int>((size_t)C);
    w.err = ws.take<unsigned>(1);
    w.active = ws.take<unsigned>((size_t)(maxiter + 1));
    if (split) sp.carve(ws, w, C);
    if (ws.overflow()) return fail(c, RC_ERR_HIP, "%s: workspace layout", who);
    w.n = (int)n; w.ld = c->ld; w.kstride = (int)kstride;
    const double qs = std::ldexp(1.0, -c->eD);
    hipStream_t s = c->sA;
    clu::Status<long long> st(C);
    hipError_t e = split ? sp.begin(c, s, w, C) : hipSuccess;
    for (int64_t khi = kmax; khi >= kmin && e == hipSuccess; khi -= C) {
        const int cnt = (int)std::min<int64_t>(C, khi - kmin + 1);
        w.khi = (int)khi;
        e = hipMemsetAsync(w.err, 0, sizeof(unsigned), s);
        if (e == hipSuccess) e = hipMemsetAsync(w.active, 0, (size_t)(maxiter + 1) * sizeof(unsigned), s);
        if (e != hipSuccess) break;
        clu::by_bits(c, [&](auto *D) { kmed::k_kmed_seed<<<cnt, RC_CLUSTER_T, 0, s>>>(D, w, seed, (int)maxiter); });
        e = clu::run_rounds(s, maxiter, w.active, [&](int64_t r) {
            clu::by_bits(c, [&](auto *D) { kmed::k_kmed_round<<<cnt, RC_CLUSTER_T, 0, s>>>(D, w, (int)maxiter, tol, qs, (int)r); });
        });
        if (e == hipSuccess) e = st.read(s, cnt, w.tcost, w.iter, w.flags, w.err);
        if (e != hipSuccess || st.err) break;
        for (int q = 0; q < cnt; ++q) {
            const int64_t i = khi - q - kmin;
            totalcost[i] = std::ldexp((double)st.cost[(size_t)q], -c->eD);
            iterations[i] = st.iter[(size_t)q];
            converged[i] = (st.flags[(size_t)q] & RC_CLUSTER_CONV) ? 1 : 0;
        }
        if (split) {
            e = sp.chunk(c, s, w, cnt, kmin, split);
            if (e != hipSuccess) break;
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
    rc = clu::hip_result(c, who, e);
    if (rc != RC_OK) return rc;
    if (st.err & RC_KMED_ERR_EMPTY)
        return fail(c, RC_ERR_DOMAIN, "%s: a k-medoids group became empty (a point is closer to another medoid than to itself: D has a "
                                      "nonzero diagonal entry)", who);
    if (st.err & RC_KMED_ERR_WEIGHT)
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

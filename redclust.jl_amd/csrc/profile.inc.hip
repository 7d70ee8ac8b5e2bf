// Cluster profiles: what dissimilarity-based clustering describes its clusters by — the medoid of every cluster, and for every
// point the sum of its distances within its own cluster and its neighbour cluster, the best alternative to its own — for each
// of L given labellings against a context's staged fixed-point D, without touching its state.  The silhouette width
// (Rousseeuw 1987) is host arithmetic on these integers.  DESIGN.md §8 "Cluster profiles"; the contract is in
// include/redclust_hip.h.
// Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, View, sync_and_check, the holders,
// checks and switches of hostutil.inc.hip, clu::check_ctx and slab.inc.hip).
//
// Definitions.  Dq is the integer matrix, D = Dq·2^-eD, caller's point order; the diagonal entry Dq[i][i] never counts.  A
// labelling's K clusters are listed in ascending label order, slots 0..K−1 of sizes n_k; A(i) is the slot of point i.
//   within[i]  = Σ_{j in A(i), j != i} Dq[i][j]
//   S_t(i)     = Σ_{j in t} Dq[i][j] for t != A(i); the neighbour of i is the t of minimum mean S_t(i)/n_t, means compared
//                exactly — S_t·n_u against S_u·n_t in 128 bits — and ties to the lower slot (the smaller label)
//   nearest[i] = S_t(i) of the neighbour, neighbour[i] its label; both 0 when K = 1
//   medoid of cluster k: its member of minimum within, ties to the smallest point index.
// Everything is an exact integer, so every output is a pure function of (Dq, labelling) whatever the batch and the chunking.
//
// The sums S come out of the slab driver (slab.inc.hip): the context's rows, in the caller's order, are its rows, with the dense
// slot of every point, rslot[s][i], from its sorted orders; RC_PROFILE_WORKSPACE_KIB and RC_PROFILE_ROWS_GLOBAL are its switches
// for this entry point.
// k_profile_rows (its staging kernel): one workgroup per row of a chunk of rows.  Row i of the caller's order is gathered through
// View.pi into (Dq, 0) pairs with a 0 at j = i: the diagonal drops out here, no logarithm is ever computed and the second half of
// every sum stays zero.
// k_profile_points (its consumer): one wave per (row of the chunk, labelling).  Lanes stride over the labelling's slots, each
// keeps its best (S, n_t, slot) under the exact comparison, a wave reduction with the same comparison finishes; lane 0 stores.
// k_profile_medoids: after all rows of a chunk of labellings, one workgroup per labelling.  Two passes of LDS atomic minima
// per cluster — on within, then on the point index among the points that attain it: exact in any order of arrival.

namespace prf {

constexpr int TPB_ROWS = 256, TPB_POINTS = 256, TPB_MEDOIDS = 256;   // (slab::KMAX clusters: 12 B of LDS each in the medoid pass)

// rows[b][j] = (Dq[row0 + b][j], 0), caller's order, 0 on the diagonal.  Grid: one block per row of the chunk.
__global__ __launch_bounds__(TPB_ROWS) void k_profile_rows(View V, int row0, ll2 *__restrict__ rows)
{
    const int n = V.n, i = row0 + blockIdx.x, u = V.pi[i];
    ll2 *dst = rows + (size_t)blockIdx.x * (size_t)n;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const size_t e = (size_t)u * V.ld + V.pi[j];
        ll2 v;
        v.x = (V.bits == 64) ? ((const long long *)V.Dq)[e] : (long long)((const int *)V.Dq)[e];
        if (j == i) v.x = 0;
        v.y = 0;
        dst[j] = v;
    }
}

// a candidate neighbour: the sum S to a cluster of nt points in slot t (t < 0: none; it loses to every candidate)
struct Cand { long long S; int nt, t; };

// x's mean is below y's, or equal with the lower slot: S_x·n_y against S_y·n_x, exact
__device__ __forceinline__ bool closer(const Cand &x, const Cand &y)
{
    if (x.t < 0) return false;
    if (y.t < 0) return true;
    const __int128 l = (__int128)x.S * y.nt, r = (__int128)y.S * x.nt;
    return l < r || (l == r && x.t < y.t);
}

struct PointArgs {
    const ll2 *sums;                 // [np][ktot] the slab of this chunk of rows
    long long ktot;
    int np, row0, n, ms;
    const unsigned short *rslot;     // [ms][n] dense slot of every point
    const long long *koff;           // [ms] first slab column of every labelling
    const int *K;                    // [ms]
    const int2 *szlab;               // [ktot] (size, label)
    long long *within;               // [ms][n]
    long long *nearest, *neighbour;  // [ms][n] or both null
};

// Grid: one wave per (row of the chunk, labelling), the labellings of a row adjacent.
__global__ __launch_bounds__(TPB_POINTS) void k_profile_points(const PointArgs a)
{
    const long long pair = (long long)blockIdx.x * (TPB_POINTS / 64) + (threadIdx.x >> 6);
    if (pair >= (long long)a.np * a.ms) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(pair / a.ms), s = (int)(pair - (long long)b * a.ms);
    const int K = a.K[s];
    const long long k0 = a.koff[s];
    const ll2 *S = a.sums + (size_t)b * (size_t)a.ktot + k0;
    const size_t o = (size_t)s * (size_t)a.n + (size_t)(a.row0 + b);
    const int own = a.rslot[o];
    if (!a.nearest) {                                   // medoids only: the own-slot entry is all that is needed
        if (lane == 0) a.within[o] = S[own].x;
        return;
    }
    Cand best{0, 0, -1};
    for (int t = lane; t < K; t += 64) {
        if (t == own) continue;
        const Cand c{S[t].x, a.szlab[k0 + t].x, t};
        if (closer(c, best)) best = c;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Cand c;
        c.S = __shfl_xor(best.S, off); c.nt = __shfl_xor(best.nt, off); c.t = __shfl_xor(best.t, off);
        if (closer(c, best)) best = c;
    }
    if (lane == 0) {
        a.within[o] = S[own].x;
        a.nearest[o] = best.t < 0 ? 0 : best.S;
        a.neighbour[o] = best.t < 0 ? 0 : (long long)a.szlab[k0 + best.t].y;
    }
}

// the order of int64 in unsigned keys, for the unsigned LDS minimum
__device__ __forceinline__ u64 min_key(long long v) { return (u64)v ^ 0x8000000000000000ull; }

// within, rslot: [ms][n]; medoid, medoid_within: [ktot].  Grid: one block per labelling.  Dynamic LDS: (largest K of the
// chunk) × (8 + 4) bytes.
__global__ __launch_bounds__(TPB_MEDOIDS) void k_profile_medoids(const long long *__restrict__ within, const unsigned short *__restrict__ rslot, int n,
                                                                 const long long *__restrict__ koff, const int *__restrict__ Ks, int Kmax,
                                                                 long long *__restrict__ medoid, long long *__restrict__ medoid_within)
{
    extern __shared__ __align__(16) unsigned char prf_lds[];
    u64 *best = reinterpret_cast<u64 *>(prf_lds);                 // [Kmax] least within of the cluster, as a key
    unsigned *who = reinterpret_cast<unsigned *>(best + Kmax);    // [Kmax] smallest index that attains it
    const int s = blockIdx.x, K = Ks[s];
    const long long *w = within + (size_t)s * (size_t)n;
    const unsigned short *rs = rslot + (size_t)s * (size_t)n;
    for (int k = threadIdx.x; k < K; k += blockDim.x) { best[k] = ~0ull; who[k] = 0xFFFFFFFFu; }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) atomicMin(&best[rs[i]], min_key(w[i]));
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int k = rs[i];
        if (min_key(w[i]) == best[k]) atomicMin(&who[k], (unsigned)i);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        medoid[koff[s] + k] = (long long)who[k] + 1;
        medoid_within[koff[s] + k] = (long long)(best[k] ^ 0x8000000000000000ull);
    }
}

// what the caller passed, after the checks
struct Call {
    rc_ctx *c;
    int64_t n, L;
    const int64_t *labels;
    int64_t *medoids_out, *medoid_within_out, *within_out, *nearest_out, *neighbour_out;
    const int *K;                    // [L]
    const int64_t *moff;             // [L + 1] first medoid of every labelling in medoids_out
    bool rows_global;
};

// labellings s0 .. s0 + ms - 1 against every row, the rows in chunks of at most qc.  ms_acc: device milliseconds, added to.
static int32_t run_labellings(const char *who, const Call &a, int64_t s0, int64_t ms, int64_t qc, double &ms_acc)
{
    rc_ctx *c = a.c;
    const int64_t n = a.n;
    const bool want_points = a.nearest_out || a.neighbour_out;
    prd::Orders O;
    if (!O.build(a.labels, n, a.K, s0, ms, true, [](int64_t, long long, int64_t, int) {}))
        return fail(c, RC_ERR_OOM, "%s: no host memory for the sorted orders of %lld labellings", who, (long long)ms);
    const long long ktot = O.ktot;
    const int Kmax = *std::max_element(O.Ks.begin(), O.Ks.end());

    DeviceBuffers B;
    long long *d_within, *d_nearest = nullptr, *d_neighbour = nullptr, *d_medoid, *d_medoid_within;
    HIPCHK(c, O.upload(B));
    HIPCHK(c, B.alloc(d_within, (size_t)ms * n));
    if (want_points) {
        HIPCHK(c, B.alloc(d_nearest, (size_t)ms * n));
        HIPCHK(c, B.alloc(d_neighbour, (size_t)ms * n));
    }
    HIPCHK(c, B.alloc(d_medoid, (size_t)ktot));
    HIPCHK(c, B.alloc(d_medoid_within, (size_t)ktot));

    const int32_t rc = slab::run_rows(c, O, B, qc, a.rows_global, k_profile_rows, TPB_ROWS, [&](const ll2 *d_sums, int64_t i0, int64_t np) {
        PointArgs p{};
        p.sums = d_sums; p.ktot = ktot; p.np = (int)np; p.row0 = (int)i0; p.n = (int)n; p.ms = (int)ms; p.rslot = O.d_rslot;
        p.koff = O.d_koff; p.K = O.d_K; p.szlab = O.d_szlab; p.within = d_within; p.nearest = d_nearest; p.neighbour = d_neighbour;
        k_profile_points<<<(unsigned)(((size_t)np * ms + TPB_POINTS / 64 - 1) / (TPB_POINTS / 64)), TPB_POINTS, 0, 0>>>(p);
    }, ms_acc);
    if (rc != RC_OK) return rc;
    const size_t lds_medoids = (size_t)Kmax * (sizeof(u64) + sizeof(unsigned));
    TimingEvents ev;
    HIPCHK(c, ev.create());
    HIPCHK(c, ev.begin(0));
    k_profile_medoids<<<(unsigned)ms, TPB_MEDOIDS, lds_medoids, 0>>>(d_within, O.d_rslot, (int)n, O.d_koff, O.d_K, Kmax, d_medoid, d_medoid_within);
    HIPCHK(c, ev.end(0));
    HIPCHK(c, ev.elapsed_ms(ms_acc));

    // the device's [ms][n] and [ktot] are the caller's rows s0 .. s0 + ms - 1 and medoids moff[s0] ..
    const size_t pts = (size_t)ms * n * sizeof(int64_t), at = (size_t)s0 * n, med = (size_t)ktot * sizeof(int64_t);
    if (a.within_out) HIPCHK(c, hipMemcpy(a.within_out + at, d_within, pts, hipMemcpyDeviceToHost));
    if (a.nearest_out) HIPCHK(c, hipMemcpy(a.nearest_out + at, d_nearest, pts, hipMemcpyDeviceToHost));
    if (a.neighbour_out) HIPCHK(c, hipMemcpy(a.neighbour_out + at, d_neighbour, pts, hipMemcpyDeviceToHost));
    if (a.medoids_out) HIPCHK(c, hipMemcpy(a.medoids_out + a.moff[s0], d_medoid, med, hipMemcpyDeviceToHost));
    if (a.medoid_within_out) HIPCHK(c, hipMemcpy(a.medoid_within_out + a.moff[s0], d_medoid_within, med, hipMemcpyDeviceToHost));
    return RC_OK;
}

}  // namespace prf

extern "C" int32_t rc_cluster_profiles(rc_ctx *c, int64_t L, const int64_t *labels, int64_t *K_out, int64_t *medoids_out,
                                       int64_t *medoid_within_out, int64_t medoids_len, int64_t *within_out, int64_t *nearest_out,
                                       int64_t *neighbour_out, int32_t *eD_out, double *kernel_ms)
{
    const char *who = "rc_cluster_profiles";
    int32_t rc = clu::check_ctx(c, who);
    if (rc != RC_OK) return rc;
    if (!labels) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    if (L < 1) return fail(c, RC_ERR_ARG, "%s: need L >= 1 (got %lld)", who, (long long)L);
    const int64_t n = c->n;
    rc = check_label_shape(c, who, n, "points", L, "L");
    if (rc != RC_OK) return rc;
    rc = check_label_rows(c, who, "labelling", labels, L, n);
    if (rc != RC_OK) return rc;
    std::vector<int> K, seen;
    std::vector<int64_t> moff;
    try { K.assign((size_t)L, 0); seen.assign((size_t)n + 1, -1); moff.assign((size_t)L + 1, 0); }
    catch (const std::bad_alloc &) { return fail(c, RC_ERR_OOM, "%s: no host memory", who); }
    const int64_t over = count_clusters(labels, L, n, slab::KMAX, seen, K.data());
    if (over < L) return fail(c, RC_ERR_CAPACITY, "%s: labelling %lld has %d clusters, more than the %lld whose minima fit the workgroup's LDS", who, (long long)over + 1, K[(size_t)over], (long long)slab::KMAX);
    for (int64_t s = 0; s < L; ++s) moff[(size_t)s + 1] = moff[(size_t)s] + K[(size_t)s];
    const bool want_medoids = medoids_out || medoid_within_out;
    if (medoids_len != (want_medoids ? moff[(size_t)L] : 0))
        return fail(c, RC_ERR_ARG, "%s: medoids_len = %lld, the labellings have %lld clusters%s", who, (long long)medoids_len, (long long)moff[(size_t)L],
                    want_medoids ? "" : " (and the medoid outputs are NULL: pass 0)");
    HIPCHK(c, hipSetDevice(c->dev));
    rc = sync_and_check(c, true);
    if (rc != RC_OK) return rc;
    if (c->sC) HIPCHK(c, hipStreamSynchronize(c->sC));
    const prf::Call a{c, n, L, labels, medoids_out, medoid_within_out, within_out, nearest_out, neighbour_out, K.data(), moff.data(),
                      env_flag("RC_PROFILE_ROWS_GLOBAL")};                       // tests: gather from the rows in global memory at small n
    // Chunks.  Device bytes per row for a run of labellings: the staged row and its slots' sums.  Labellings are taken while 512
    // rows (or all n) of them fit the workspace, their sorted orders fit theirs and their per-point results half the workspace;
    // the rows then go in chunks of what fits.
    const size_t workspace = env_workspace_kib("RC_PROFILE_WORKSPACE_KIB", slab::WORKSPACE);
    const int64_t ms_cap = slab_ms_cap(slab::PERM_BYTES, 4, n);
    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < L;) {
        const SlabChunk ch = slab_plan(s0, K.data(), L, ms_cap, 16 * (size_t)n, 0, n, std::min<int64_t>(n, 512), workspace,
                                       [n](size_t k) { return 24 * (size_t)n + 16 * k; }, workspace / 2);
        rc = prf::run_labellings(who, a, s0, ch.ms, ch.qc, ms_acc);
        if (rc != RC_OK) return rc;
        s0 += ch.ms;
    }
    if (K_out) for (int64_t s = 0; s < L; ++s) K_out[s] = K[(size_t)s];
    if (eD_out) *eD_out = c->eD;
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

// Predict from points: rc_predict for new observations given by their coordinates, with the distances, their logarithms, the
// quantisation and the per-cluster summary of the draws on the device.  DESIGN.md §8 "Predict from points"; the contract is in
// include/redclust_hip.h.  Included at the end of redclust_hip.hip after predict.inc.hip (same translation unit: shares
// prd::Call and prd::Run — everything of rc_predict after "the chunk's rows are on the device" — k_transpose_points, rc_flog,
// flog_table, quant_exponent_hd, slab_plan and the holders, checks and switches of hostutil.inc.hip).
//
// k_points_dist: a block takes R new points, whose coordinates it stages in LDS a tile of DT coordinates at a time, and a strip
// of 256 training points, one per thread.  A thread keeps R accumulators and walks the coordinates in ascending order: one
// coalesced load of the training coordinate (the training points are transposed to dim×n once per call), R LDS-broadcast
// reads, and per (new point, training point, coordinate) one subtraction and one explicit fma — the chain of the contract, never
// reassociated and never split across threads.  A correctly rounded square root finishes the distance; the row's largest
// distance is folded with integer atomic maxima on the bit patterns (positive doubles order as their bits), and a squared
// distance that is 0, subnormal or not finite lowers the call's "first bad pair" word to its row-major index (atomic minimum).
// The kernel is a template over the metric (metric.inc.hip: met::step per coordinate, met::finish and met::bad at the end; the
// norms of the two angular metrics come from met::k_metric_prep, which has also centred both point sets for CORRELATION); the
// EUCLIDEAN instantiation is the kernel described above, operation for operation.
//
// k_points_rows: one block per new point: rc_flog of the row (twice: once for the largest |log|, once to quantise — cheaper
// than a round trip through memory), the exponents by quant_exponent_hd, the (Dq, Lq) row and the scales 2^-eD, 2^-eL where
// rc_predict's host loop writes them.

namespace pp {

constexpr int TPB = 256;    // threads of both kernels: a strip of training points / the lanes over a row
constexpr int R = 8;        // new points per block of k_points_dist
constexpr int DT = 256;     // coordinates per LDS tile (R·DT·8 = 16 KiB)
constexpr u64 NO_PAIR = ~(u64)0;
constexpr int64_t DIM_MAX = (int64_t)1 << 20;

// XT: [dim][n]; Y: [np][dim]; dist: [np][n]; maxd: [np] bit patterns, zero before the launch; firstbad: min over the bad pairs
// of pair0 + i·n + j; nX: [n], nY: [np] the norms (angular metrics, else unused).  Grid: (groups of R new points, strips of TPB
// training points).
template <int M>
__global__ __launch_bounds__(TPB) void k_points_dist(const double *__restrict__ XT, int n, int dim, const double *__restrict__ Y, int np, u64 pair0,
                                                     double *__restrict__ dist, u64 *__restrict__ maxd, u64 *__restrict__ firstbad,
                                                     const double *__restrict__ nX, const double *__restrict__ nY)
{
    __shared__ double ys[DT * R];
    const int ib = blockIdx.x * R;
    const int nr = min(R, np - ib);
    const int j = blockIdx.y * TPB + threadIdx.x;
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    for (int k0 = 0; k0 < dim; k0 += DT) {
        const int dt = min(DT, dim - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < R * dt; e += TPB) {
            const int r = e / dt, kk = e - r * dt;
            ys[kk * R + r] = r < nr ? Y[(size_t)(ib + r) * (size_t)dim + (size_t)(k0 + kk)] : 0.0;
        }
        __syncthreads();
        if (j < n) {
            const double *xp = XT + (size_t)k0 * (size_t)n + j;
#pragma unroll 4
            for (int kk = 0; kk < dt; ++kk) {
                const double x = xp[(size_t)kk * (size_t)n];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = met::step<M>(acc[r], ys[kk * R + r], x);
            }
        }
    }
    const double nx = (met::angular(M) && j < n) ? nX[j] : 1.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        u64 bits = 0;
        if (j < n && r < nr) {
            double s;
            const double d = met::finish<M>(acc[r], met::angular(M) ? nY[ib + r] : 1.0, nx, s);
            dist[(size_t)(ib + r) * (size_t)n + j] = d;
            if (!met::bad<M>(acc[r], d, s)) bits = (u64)__double_as_longlong(d);
            else atomicMin(firstbad, pair0 + (u64)(ib + r) * (u64)n + (u64)j);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const u64 o = __shfl_xor(bits, off);
            bits = o > bits ? o : bits;
        }
        if ((threadIdx.x & 63) == 0 && bits) atomicMax(&maxd[ib + r], bits);
    }
}

// dist: [np][n]; maxd: [np]; rows: [np][n] (Dq, Lq); logs: [np][n] or null; scD, scL, eD, eL: [np].  Grid: one block per new point.
__global__ __launch_bounds__(TPB) void k_points_rows(const double *__restrict__ dist, int n, const u64 *__restrict__ maxd, const double2 *__restrict__ flt,
                                                     ll2 *__restrict__ rows, double *__restrict__ logs, double *__restrict__ scD, double *__restrict__ scL,
                                                     int *__restrict__ eD_out, int *__restrict__ eL_out)
{
    __shared__ double red[TPB / 64];
    const int i = blockIdx.x;
    const double *d = dist + (size_t)i * (size_t)n;
    double lm = 0.0;
    for (int j = threadIdx.x; j < n; j += TPB) lm = fmax(lm, fabs(rc_flog(d[j], flt)));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lm = fmax(lm, __shfl_xor(lm, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lm;
    __syncthreads();
    lm = red[0];
#pragma unroll
    for (int w = 1; w < TPB / 64; ++w) lm = fmax(lm, red[w]);
    const int eD = quant_exponent_hd(n, __longlong_as_double((long long)maxd[i]), 64), eL = quant_exponent_hd(n, lm, 64);
    ll2 *row = rows + (size_t)i * (size_t)n;
    for (int j = threadIdx.x; j < n; j += TPB) {
        const double x = d[j], l = rc_flog(x, flt);
        ll2 v;
        v.x = __double2ll_rn(ldexp(x, eD));
        v.y = __double2ll_rn(ldexp(l, eL));
        row[j] = v;
        if (logs) logs[(size_t)i * (size_t)n + j] = l;
    }
    if (threadIdx.x == 0) {
        scD[i] = ldexp(1.0, -eD); scL[i] = ldexp(1.0, -eL);
        eD_out[i] = eD; eL_out[i] = eL;
    }
}

// what rc_predict_points adds to prd::Call
struct Points {
    int64_t dim;
    const double *points, *new_points;      // host: n×dim, q×dim
    const double *d_XT;                     // device: dim×n (centred for CORRELATION)
    u64 *d_firstbad;
    double *dist_out, *log_out;             // host q×n or null
    int32_t *eD_out, *eL_out;               // host q or null
    int32_t metric;
    const double *d_nX;                     // device: the training points' norms (angular metrics, else null)
};

// the q×n (here np×n) distances of one chunk in the call's metric
static void launch_dist(int32_t metric, const double *d_XT, int64_t n, int64_t dim, const double *d_Y, int64_t np, u64 pair0, double *d_dist, u64 *d_maxd,
                        u64 *d_firstbad, const double *d_nX, const double *d_nY)
{
    const dim3 grid((unsigned)((np + R - 1) / R), (unsigned)((n + TPB - 1) / TPB));
#define RC_POINTS_DIST(M) k_points_dist<M><<<grid, TPB, 0, 0>>>(d_XT, (int)n, (int)dim, d_Y, (int)np, pair0, d_dist, d_maxd, d_firstbad, d_nX, d_nY)
    switch (metric) {
    case RC_METRIC_EUCLIDEAN:   RC_POINTS_DIST(RC_METRIC_EUCLIDEAN); break;
    case RC_METRIC_SQEUCLIDEAN: RC_POINTS_DIST(RC_METRIC_SQEUCLIDEAN); break;
    case RC_METRIC_CITYBLOCK:   RC_POINTS_DIST(RC_METRIC_CITYBLOCK); break;
    case RC_METRIC_CHEBYSHEV:   RC_POINTS_DIST(RC_METRIC_CHEBYSHEV); break;
    case RC_METRIC_COSINE:      RC_POINTS_DIST(RC_METRIC_COSINE); break;
    default:                    RC_POINTS_DIST(RC_METRIC_CORRELATION); break;
    }
#undef RC_POINTS_DIST
}

// a point's coordinates as the angular metrics see them (centred for CORRELATION) and their norm, in the header's arithmetic
static double host_prepared(int32_t metric, const double *x, int64_t dim, std::vector<double> &out)
{
    double mu = 0.0;
    if (metric == RC_METRIC_CORRELATION) {
        double sum = 0.0;
        for (int64_t k = 0; k < dim; ++k) sum += x[k];
        mu = sum / (double)dim;
    }
    double nn = 0.0;
    out.resize((size_t)dim);
    for (int64_t k = 0; k < dim; ++k) {
        const double v = metric == RC_METRIC_CORRELATION ? x[k] - mu : x[k];
        out[(size_t)k] = v;
        nn = std::fma(v, v, nn);
    }
    return std::sqrt(nn);
}

// the library's error for the first bad pair (row-major, 0-based index into q×n): it names the pair, the metric and the cause
static int32_t bad_pair(const char *who, const prd::Call &c, const Points &pt, u64 pair)
{
    const int64_t i = (int64_t)(pair / (u64)c.n), j = (int64_t)(pair % (u64)c.n);
    const double *y = pt.new_points + (size_t)i * pt.dim, *x = pt.points + (size_t)j * pt.dim;
    const char *name = met::NAMES[pt.metric];
    const long long i1 = (long long)i + 1, j1 = (long long)j + 1;
    bool same = true;
    for (int64_t k = 0; k < pt.dim; ++k) same = same && y[k] == x[k];
    if (met::angular(pt.metric)) {
        std::vector<double> yc, xc;
        const double ny = host_prepared(pt.metric, y, pt.dim, yc), nx = host_prepared(pt.metric, x, pt.dim, xc);
        const char *flat = pt.metric == RC_METRIC_COSINE ? "is the zero vector" : "has constant coordinates";
        if (ny == 0.0) return fail(nullptr, RC_ERR_DOMAIN, "%s: new point %lld %s: its %s distance is undefined", who, i1, flat, name);
        if (nx == 0.0) return fail(nullptr, RC_ERR_DOMAIN, "%s: training point %lld %s: its %s distance is undefined (met at new point %lld)", who, j1, flat, name, i1);
        const double s = ny * nx;
        if (!met::positive_normal(s))
            return fail(nullptr, RC_ERR_DOMAIN, "%s: the product of the norms of new point %lld and training point %lld is %g (metric %s): the coordinates' scale %s it",
                        who, i1, j1, s, name, s < 1.0 ? "underflows" : "overflows");
        if (same) return fail(nullptr, RC_ERR_DOMAIN, "%s: new point %lld coincides with training point %lld (metric %s): the distances must be positive", who, i1, j1, name);
        return fail(nullptr, RC_ERR_DOMAIN, "%s: new point %lld is parallel to training point %lld: their %s distance is 0 to within the rounding of the norms, and the distances must be positive", who, i1, j1, name);
    }
    if (same) return fail(nullptr, RC_ERR_DOMAIN, "%s: new point %lld coincides with training point %lld (metric %s): the distances must be positive", who, i1, j1, name);
    double acc = 0.0;
    for (int64_t k = 0; k < pt.dim; ++k) {
        const double t = y[k] - x[k];
        acc = pt.metric == RC_METRIC_CITYBLOCK ? acc + std::fabs(t) : pt.metric == RC_METRIC_CHEBYSHEV ? std::fmax(acc, std::fabs(t)) : std::fma(t, t, acc);
    }
    const bool squared = pt.metric == RC_METRIC_EUCLIDEAN || pt.metric == RC_METRIC_SQEUCLIDEAN;
    return fail(nullptr, RC_ERR_DOMAIN, "%s: the %s distance of new point %lld to training point %lld is %g (metric %s): the coordinates' scale %s %s",
                who, squared ? "squared" : name, i1, j1, acc, name, acc < 1.0 ? "underflows" : "overflows", squared ? "the square" : "it");
}

// samples s0 .. s0 + ms - 1 against every new point, the points in chunks of at most qc whose rows are filled on the device.
static int32_t run_samples(const char *who, const prd::Call &c, const Points &pt, int64_t s0, int64_t ms, int64_t qc, double &ms_acc)
{
    const int64_t n = c.n, dim = pt.dim;
    prd::Run run;
    int32_t rc = run.begin(who, c, s0, ms, qc);
    if (rc != RC_OK) return rc;
    DeviceBuffers B;
    double *d_Y, *d_dist, *d_log = nullptr; u64 *d_maxd; int *d_eD, *d_eL;
    HIPCHK(nullptr, B.alloc(d_Y, (size_t)qc * dim));
    HIPCHK(nullptr, B.alloc(d_dist, (size_t)qc * n));
    if (pt.log_out) HIPCHK(nullptr, B.alloc(d_log, (size_t)qc * n));
    HIPCHK(nullptr, B.alloc(d_maxd, (size_t)qc));
    HIPCHK(nullptr, B.alloc(d_eD, (size_t)qc));
    HIPCHK(nullptr, B.alloc(d_eL, (size_t)qc));
    double *d_nY = nullptr;
    if (met::angular(pt.metric)) HIPCHK(nullptr, B.alloc(d_nY, (size_t)qc));
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());
    for (int64_t i0 = 0; i0 < c.q; i0 += qc) {
        const int64_t np = std::min(qc, c.q - i0);
        HIPCHK(nullptr, hipMemcpy(d_Y, pt.new_points + (size_t)i0 * dim, (size_t)np * dim * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemsetAsync(d_maxd, 0, (size_t)np * sizeof(u64), 0));
        HIPCHK(nullptr, ev.begin(0));
        met::launch_prep(pt.metric, d_Y, np, dim, d_nY, 0);
        launch_dist(pt.metric, pt.d_XT, n, dim, d_Y, np, (u64)i0 * (u64)n, d_dist, d_maxd, pt.d_firstbad, pt.d_nX, d_nY);
        k_points_rows<<<(unsigned)np, TPB, 0, 0>>>(d_dist, (int)n, d_maxd, c.d_flt, run.d_rows, d_log, run.d_scD, run.d_scL, d_eD, d_eL);
        HIPCHK(nullptr, ev.end(0));
        HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
        u64 firstbad = NO_PAIR;
        HIPCHK(nullptr, hipMemcpy(&firstbad, pt.d_firstbad, sizeof(u64), hipMemcpyDeviceToHost));
        if (firstbad != NO_PAIR) return bad_pair(who, c, pt, firstbad);
        if (pt.dist_out) HIPCHK(nullptr, hipMemcpy(pt.dist_out + (size_t)i0 * n, d_dist, (size_t)np * n * sizeof(double), hipMemcpyDeviceToHost));
        if (pt.log_out) HIPCHK(nullptr, hipMemcpy(pt.log_out + (size_t)i0 * n, d_log, (size_t)np * n * sizeof(double), hipMemcpyDeviceToHost));
        if (pt.eD_out) HIPCHK(nullptr, hipMemcpy(pt.eD_out + i0, d_eD, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
        if (pt.eL_out) HIPCHK(nullptr, hipMemcpy(pt.eL_out + i0, d_eL, (size_t)np * sizeof(int), hipMemcpyDeviceToHost));
        rc = run.finish(c, i0, np, ms_acc);
        if (rc != RC_OK) return rc;
    }
    return RC_OK;
}

// The training points on the device as k_points_dist reads them: uploaded, through the metric's pre-pass (d_nX: their norms,
// null unless the metric is angular) and transposed to dim×n (d_XT); both are owned by B.
static int32_t stage_training(int32_t metric, const double *points, int64_t n, int64_t dim, DeviceBuffers &B, double *&d_XT, double *&d_nX)
{
    DeviceBuffers T;                            // the points as given, until they are transposed
    double *d_X;
    d_nX = nullptr;
    HIPCHK(nullptr, T.alloc(d_X, (size_t)n * dim));
    HIPCHK(nullptr, B.alloc(d_XT, (size_t)n * dim));
    if (met::angular(metric)) HIPCHK(nullptr, B.alloc(d_nX, (size_t)n));
    HIPCHK(nullptr, hipMemcpy(d_X, points, (size_t)n * dim * sizeof(double), hipMemcpyHostToDevice));
    met::launch_prep(metric, d_X, n, dim, d_nX, 0);
    k_transpose_points<<<(unsigned)std::min<size_t>(((size_t)n * (size_t)dim + 255) / 256, 65535), 256, 0, 0>>>(d_X, (int)n, (int)dim, d_XT);
    HIPCHK(nullptr, hipGetLastError());
    HIPCHK(nullptr, hipStreamSynchronize(0));
    return RC_OK;
}

// the first coordinate of n×dim points and q×dim new points (null: none) that is not finite: the library's error
static int32_t check_finite(const char *who, const double *points, int64_t n, const double *new_points, int64_t q, int64_t dim)
{
    for (int pass = 0; pass < (new_points ? 2 : 1); ++pass) {
        const double *x = pass ? new_points : points;
        const int64_t rows = pass ? q : n;
        for (size_t e = 0; e < (size_t)rows * (size_t)dim; ++e)
            if (!(std::fabs(x[e]) <= 1.79769313486231570e308))
                return fail(nullptr, RC_ERR_DOMAIN, "%s: coordinate %lld of %s %lld is not finite", who, (long long)(e % (size_t)dim) + 1, pass ? "new point" : "training point", (long long)(e / (size_t)dim) + 1);
    }
    return RC_OK;
}

}  // namespace pp

static int32_t predict_points_impl(const char *who, int32_t metric, int32_t device, int64_t n, int64_t dim, const double *points, int64_t q, const double *new_points, int64_t m,
                                   const int64_t *samples, const double *r, const double *p, const rc_params *params, uint64_t seed,
                                   uint64_t sample_offset, uint64_t point_offset, int64_t *labels_out, int64_t *map_out, const int64_t *maps,
                                   int64_t maps_width, const int64_t *pivot_labels, int64_t Kp, void *counts_out, void *mapcounts_out, int64_t Kmax,
                                   double *scores_out, int64_t *sums_out, double *dist_out, double *log_out, int32_t *eD_out, int32_t *eL_out,
                                   double *kernel_ms)
{
    if (!points || !new_points || !samples || !r || !p || !params) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (!labels_out && !map_out && !counts_out && !mapcounts_out) return fail(nullptr, RC_ERR_ARG, "%s: one of labels_out, map_out, counts_out and mapcounts_out must be given", who);
    if (n < 1 || q < 1 || m < 1) return fail(nullptr, RC_ERR_ARG, "%s: need n >= 1, q >= 1 and m >= 1 (got n=%lld q=%lld m=%lld)", who, (long long)n, (long long)q, (long long)m);
    int32_t rc = check_label_shape(nullptr, who, n, "training points", m, "m");
    if (rc != RC_OK) return rc;
    if (dim < 1 || dim > pp::DIM_MAX) return fail(nullptr, RC_ERR_ARG, "%s: dim = %lld outside 1..%lld", who, (long long)dim, (long long)pp::DIM_MAX);
    rc = met::check_metric(nullptr, who, metric, dim);
    if (rc != RC_OK) return rc;
    const bool want_counts = counts_out || mapcounts_out;
    if (want_counts && (!maps || !pivot_labels)) return fail(nullptr, RC_ERR_ARG, "%s: the counts need maps and pivot_labels", who);
    rc = check_params(nullptr, who, params);
    if (rc != RC_OK) return rc;
    rc = check_r_p(nullptr, who, "sample", m, r, p);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    const bool want_tab = scores_out || sums_out;
    std::vector<int> K, seen;
    std::vector<double> A;
    try { K.assign((size_t)m, 0); seen.assign((size_t)n + 1, -1); A.resize((size_t)n + 1); }
    catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    const int64_t over = count_clusters(samples, m, n, want_tab ? Kmax : n, seen, K.data());
    if (over < m) return fail(nullptr, RC_ERR_ARG, "%s: sample %lld has %d clusters, Kmax = %lld", who, (long long)over + 1, K[(size_t)over], (long long)Kmax);
    if (want_counts) {
        if (Kp < 1 || Kp > n) return fail(nullptr, RC_ERR_ARG, "%s: Kp = %lld outside 1..n", who, (long long)Kp);
        for (int64_t k = 0; k < Kp; ++k)
            if (pivot_labels[k] < 1 || pivot_labels[k] > n || (k > 0 && pivot_labels[k] <= pivot_labels[k - 1]))
                return fail(nullptr, RC_ERR_ARG, "%s: pivot_labels must be strictly ascending in 1..n (entry %lld)", who, (long long)k + 1);
        for (int64_t s = 0; s < m; ++s) {
            if (maps_width < K[(size_t)s]) return fail(nullptr, RC_ERR_ARG, "%s: maps_width = %lld is below the %d clusters of sample %lld", who, (long long)maps_width, K[(size_t)s], (long long)s + 1);
            for (int64_t t = 0; t < maps_width; ++t) {
                const int64_t to = maps[(size_t)s * maps_width + t];
                if (to == 0 || (to == -1 && t >= K[(size_t)s]) || std::binary_search(pivot_labels, pivot_labels + Kp, to)) continue;
                return fail(nullptr, RC_ERR_ARG, "%s: maps[%lld][%lld] = %lld is neither 0 nor a pivot label", who, (long long)s + 1, (long long)t + 1, (long long)to);
            }
        }
    }
    rc = pp::check_finite(who, points, n, new_points, q, dim);
    if (rc != RC_OK) return rc;
    rc = select_device(who, device);
    if (rc != RC_OK) return rc;
    size_table(params, n, A.data());
    DeviceBuffers B;
    double2 *d_flt;
    {
        double2 ft[128];
        flog_table(ft);
        HIPCHK(nullptr, B.alloc(d_flt, 128));
        HIPCHK(nullptr, hipMemcpy(d_flt, ft, sizeof(ft), hipMemcpyHostToDevice));
    }
    double *d_XT, *d_nX;
    u64 *d_firstbad;
    rc = pp::stage_training(metric, points, n, dim, B, d_XT, d_nX);
    if (rc != RC_OK) return rc;
    HIPCHK(nullptr, B.alloc(d_firstbad, 1));
    HIPCHK(nullptr, hipMemset(d_firstbad, 0xFF, sizeof(u64)));
    prd::Call c{n, q, m, want_tab ? Kmax : 0, nullptr, nullptr, samples, r, p, params, seed, sample_offset, point_offset,
                labels_out, map_out, sums_out, scores_out, nullptr, nullptr, K.data(), A.data(), d_flt, env_flag("RC_PREDICT_ROWS_GLOBAL")};
    const size_t ncols = (size_t)Kp + 1;
    if (want_counts) { c.maps = maps; c.maps_width = maps_width; c.pivot = pivot_labels; c.Kp = Kp; }
    if (counts_out) {
        HIPCHK(nullptr, B.alloc(c.d_counts, (size_t)q * ncols));
        HIPCHK(nullptr, hipMemset(c.d_counts, 0, (size_t)q * ncols * sizeof(unsigned)));
    }
    if (mapcounts_out) {
        HIPCHK(nullptr, B.alloc(c.d_mapcounts, (size_t)q * ncols));
        HIPCHK(nullptr, hipMemset(c.d_mapcounts, 0, (size_t)q * ncols * sizeof(unsigned)));
    }
    const pp::Points pt{dim, points, new_points, d_XT, d_firstbad, dist_out, log_out, eD_out, eL_out, metric, d_nX};
    // Chunks: rc_predict's plan with, per new point, its coordinates, its f64 distances and, when asked for, its logarithms
    // beside its row.
    const size_t workspace = env_workspace_kib("RC_PREDICT_WORKSPACE_KIB", slab::WORKSPACE);
    const size_t per_sample = 16 + (scores_out ? 8 * ((size_t)c.Kmax + 1) : 0) + (sums_out ? 16 * (size_t)c.Kmax : 0);
    const size_t fixed = 16 * (size_t)n + 8 * (size_t)n + (log_out ? 8 * (size_t)n : 0) + 8 * (size_t)dim;
    const int64_t ms_cap = slab_ms_cap(slab::PERM_BYTES, 2, n);
    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < m;) {
        const SlabChunk ch = slab_plan(s0, K.data(), m, ms_cap, fixed, per_sample, q, std::min<int64_t>(q, 512), workspace);
        rc = pp::run_samples(who, c, pt, s0, ch.ms, ch.qc, ms_acc);
        if (rc != RC_OK) return rc;
        s0 += ch.ms;
    }
    if (counts_out) HIPCHK(nullptr, hipMemcpy(counts_out, c.d_counts, (size_t)q * ncols * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (mapcounts_out) HIPCHK(nullptr, hipMemcpy(mapcounts_out, c.d_mapcounts, (size_t)q * ncols * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

extern "C" int32_t rc_predict_points(int32_t device, int64_t n, int64_t dim, const double *points, int64_t q, const double *new_points, int64_t m,
                                     const int64_t *samples, const double *r, const double *p, const rc_params *params, uint64_t seed,
                                     uint64_t sample_offset, uint64_t point_offset, int64_t *labels_out, int64_t *map_out, const int64_t *maps,
                                     int64_t maps_width, const int64_t *pivot_labels, int64_t Kp, void *counts_out, void *mapcounts_out, int64_t Kmax,
                                     double *scores_out, int64_t *sums_out, double *dist_out, double *log_out, int32_t *eD_out, int32_t *eL_out,
                                     double *kernel_ms)
{
    return predict_points_impl("rc_predict_points", RC_METRIC_EUCLIDEAN, device, n, dim, points, q, new_points, m, samples, r, p, params, seed, sample_offset,
                               point_offset, labels_out, map_out, maps, maps_width, pivot_labels, Kp, counts_out, mapcounts_out, Kmax, scores_out,
                               sums_out, dist_out, log_out, eD_out, eL_out, kernel_ms);
}

extern "C" int32_t rc_predict_points_metric(int32_t metric, int32_t device, int64_t n, int64_t dim, const double *points, int64_t q, const double *new_points,
                                            int64_t m, const int64_t *samples, const double *r, const double *p, const rc_params *params, uint64_t seed,
                                            uint64_t sample_offset, uint64_t point_offset, int64_t *labels_out, int64_t *map_out, const int64_t *maps,
                                            int64_t maps_width, const int64_t *pivot_labels, int64_t Kp, void *counts_out, void *mapcounts_out,
                                            int64_t Kmax, double *scores_out, int64_t *sums_out, double *dist_out, double *log_out, int32_t *eD_out,
                                            int32_t *eL_out, double *kernel_ms)
{
    return predict_points_impl("rc_predict_points_metric", metric, device, n, dim, points, q, new_points, m, samples, r, p, params, seed, sample_offset,
                               point_offset, labels_out, map_out, maps, maps_width, pivot_labels, Kp, counts_out, mapcounts_out, Kmax, scores_out,
                               sums_out, dist_out, log_out, eD_out, eL_out, kernel_ms);
}

// Metrics from coordinates: the arithmetic of a pair in each RC_METRIC_* (include/redclust_hip.h states it, DESIGN.md §8
// "Metrics from coordinates"), the per-point pre-pass of the two angular metrics and the symmetric n×n kernel.  Included at
// the end of redclust_hip.hip after hostutil.inc.hip and before predictpoints.inc.hip, whose k_points_dist<M> computes the
// q×n form with the same step and finish (same translation unit).
//
// k_metric_prep: one thread per point walks its coordinates: the sum and the centred copy (CORRELATION), then the squared
// norm by explicit fma and its correctly rounded root.  n·dim work beside the n²·dim of the pairs: left simple.
//
// k_pairwise_metric<M>: k_pairwise's geometry — 64×64 pairs per 256-thread block, 4×4 per thread, the coordinates staged
// through LDS 16 at a time, the lower block triangle only — with two changes the stores asked for, since they bound the
// kernel: a thread's four columns are 16 apart (a wave's store of one (u, v) covers 16 consecutive doubles of four rows, and
// its LDS reads of the column tile are conflict-free), and the mirrored tile goes through LDS so that it, too, is written
// along rows (64 consecutive doubles per wave) instead of down columns.  A pair's chain stays inside one thread, ascending;
// coordinates past dim are staged as 0 on both sides, which leaves every accumulator as it is (t = 0: fma(0, 0, acc) = acc,
// acc + 0 = acc, max(acc, 0) = acc for acc >= +0; a dot product is never −0 under round-to-nearest, and fma(0, 0, dot) = dot).

namespace met {

constexpr int COUNT = 6;
static const char *const NAMES[COUNT] = {"euclidean", "sqeuclidean", "cityblock", "chebyshev", "cosine", "correlation"};
constexpr bool angular(int M) { return M == RC_METRIC_COSINE || M == RC_METRIC_CORRELATION; }
constexpr double DBL_MIN_NORMAL = 2.2250738585072014e-308, DBL_MAX_FINITE = 1.79769313486231570e308;
// What the angular arithmetic can return for a point against itself or against its multiple by a power of two: the root's rounding
// enters norm·norm twice and the product rounds once, so s is within (3·2^-53 + O(2^-106))·nn of nn; the quotient rounds once
// more and c >= 1 − 4·2^-53.  A d at or below this floor is the arithmetic's zero (measured on random vectors: 0 in three
// coincident pairs of four, 2^-53 or 2^-52 in the fourth).
constexpr double ANGULAR_FLOOR = 4.440892098500626e-16;     // 2^-51

// one coordinate of the chain
template <int M> __host__ __device__ __forceinline__ double step(double acc, double y, double x)
{
    if constexpr (angular(M)) return fma(y, x, acc);
    else {
        const double t = y - x;
        if constexpr (M == RC_METRIC_EUCLIDEAN || M == RC_METRIC_SQEUCLIDEAN) return fma(t, t, acc);
        else if constexpr (M == RC_METRIC_CITYBLOCK) return acc + fabs(t);      // a sum of two values: nothing to contract
        else return fmax(acc, fabs(t));
    }
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double rn_sqrt(double a) { return __dsqrt_rn(a); }
__device__ __forceinline__ double rn_div(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double rn_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double rn_sub(double a, double b) { return __dsub_rn(a, b); }
#else
static inline double rn_sqrt(double a) { return std::sqrt(a); }
static inline double rn_div(double a, double b) { return a / b; }
static inline double rn_mul(double a, double b) { return a * b; }
static inline double rn_sub(double a, double b) { return a - b; }
#endif

// the distance from the finished accumulator; s: the product of the norms (angular metrics; 1 otherwise)
template <int M> __host__ __device__ __forceinline__ double finish(double acc, double ny, double nx, double &s)
{
    s = 1.0;
    if constexpr (M == RC_METRIC_EUCLIDEAN) return rn_sqrt(acc);
    else if constexpr (angular(M)) {
        s = rn_mul(ny, nx);
        const double c = rn_div(acc, s);
        return fmax(rn_sub(1.0, c), 0.0);
    } else return acc;
}

__host__ __device__ __forceinline__ bool positive_normal(double a) { return a >= DBL_MIN_NORMAL && a <= DBL_MAX_FINITE; }

// the bad-pair rule of the header (acc: the finished accumulator, d and s from finish)
template <int M> __host__ __device__ __forceinline__ bool bad(double acc, double d, double s)
{
    if constexpr (M == RC_METRIC_EUCLIDEAN) return !positive_normal(acc);
    else if constexpr (angular(M)) return !(d > ANGULAR_FLOOR && d <= DBL_MAX_FINITE) || !positive_normal(s);
    else return !positive_normal(d);
}

// src, dst: [rows][dim] (dst may be src, or null when CENTRE is false: nothing to write); nrm: [rows]
template <bool CENTRE> __global__ __launch_bounds__(256) void k_metric_prep(const double *src, int rows, int dim, double *dst, double *__restrict__ nrm)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const double *x = src + (size_t)i * (size_t)dim;
    double mu = 0.0;
    if (CENTRE) {
        double sum = 0.0;
        for (int k = 0; k < dim; ++k) sum = __dadd_rn(sum, x[k]);
        mu = __ddiv_rn(sum, (double)dim);
    }
    double nn = 0.0;
    for (int k = 0; k < dim; ++k) {
        double v = x[k];
        if (CENTRE) {
            v = __dsub_rn(v, mu);
            dst[(size_t)i * (size_t)dim + k] = v;
        }
        nn = fma(v, v, nn);
    }
    nrm[i] = __dsqrt_rn(nn);
}

constexpr int PT = 64;          // pairs per block side
constexpr int KT = 16;          // coordinates per LDS tile
constexpr int PLD = PT + 1;     // padded row of both LDS uses

// pts: [n][dim] (centred already for CORRELATION); nrm: [n] (angular metrics, else unused); D: [n][n].  Grid: (nt, nt) blocks
// of 256 threads, nt = ceil(n / 64); blocks above the diagonal return at once.
template <int M> __global__ __launch_bounds__(256) void k_pairwise_metric(const double *__restrict__ pts, const double *__restrict__ nrm, int n, int dim,
                                                                         double *__restrict__ D)
{
    const int tj = blockIdx.x, ti = blockIdx.y;
    if (ti < tj) return;
    __shared__ double sh[PT * PLD];                 // the two coordinate tiles, then the tile to mirror
    double *A = sh, *B = sh + KT * PLD;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int k0 = 0; k0 < dim; k0 += KT) {
        for (int e = threadIdx.x; e < KT * PT; e += 256) {
            const int kk = e & (KT - 1), r = e >> 4;
            const int gi = ti * PT + r, gj = tj * PT + r, k = k0 + kk;
            A[kk * PLD + r] = (gi < n && k < dim) ? pts[(size_t)gi * (size_t)dim + k] : 0.0;
            B[kk * PLD + r] = (gj < n && k < dim) ? pts[(size_t)gj * (size_t)dim + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KT; ++kk) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = A[kk * PLD + ty * 4 + u]; b[u] = B[kk * PLD + tx + 16 * u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = step<M>(acc[u][v], a[u], b[v]);
        }
        __syncthreads();
    }
    double na[4], nb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int i = ti * PT + ty * 4 + u, j = tj * PT + tx + 16 * u;
        na[u] = (angular(M) && i < n) ? nrm[i] : 1.0;
        nb[u] = (angular(M) && j < n) ? nrm[j] : 1.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int il = ty * 4 + u, jl = tx + 16 * v;
            const int i = ti * PT + il, j = tj * PT + jl;
            double s;
            const double d = (i == j) ? 0.0 : finish<M>(acc[u][v], na[u], nb[v], s);
            if (i < n && j < n) D[(size_t)i * (size_t)n + j] = d;
            sh[jl * PLD + il] = d;                  // every thread is past the last tile's barrier
        }
    if (ti == tj) return;                           // a diagonal block computed both triangles itself
    __syncthreads();
    const int c = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < PT; r += 4) {
        const int j = tj * PT + r, i = ti * PT + c;
        if (i < n && j < n) D[(size_t)j * (size_t)n + i] = sh[r * PLD + c];
    }
}

static bool known(int32_t metric) { return metric >= 0 && metric < COUNT; }

// The argument errors every entry point with a metric shares
static int32_t check_metric(rc_ctx *c, const char *who, int32_t metric, int64_t dim)
{
    if (!known(metric)) return fail(c, RC_ERR_ARG, "%s: unknown metric %d (RC_METRIC_* are 0..%d)", who, metric, COUNT - 1);
    if (metric == RC_METRIC_CORRELATION && dim < 2) return fail(c, RC_ERR_ARG, "%s: the correlation metric needs dim >= 2 (got %lld)", who, (long long)dim);
    return RC_OK;
}

// The pre-pass of a set of points on the device, in place: norms (angular metrics) and centring (CORRELATION).  d_nrm: [rows],
// may be null for the other metrics.
static void launch_prep(int32_t metric, double *d_pts, int64_t rows, int64_t dim, double *d_nrm, hipStream_t st)
{
    const unsigned blocks = (unsigned)((rows + 255) / 256);
    if (metric == RC_METRIC_COSINE) k_metric_prep<false><<<blocks, 256, 0, st>>>(d_pts, (int)rows, (int)dim, nullptr, d_nrm);
    else if (metric == RC_METRIC_CORRELATION) k_metric_prep<true><<<blocks, 256, 0, st>>>(d_pts, (int)rows, (int)dim, d_pts, d_nrm);
}

// D = the symmetric matrix of the n points d_pts (n×dim, already through launch_prep) on stream st
static void launch_pairwise(int32_t metric, const double *d_pts, const double *d_nrm, int64_t n, int64_t dim, double *d_D, hipStream_t st)
{
    const unsigned nt = (unsigned)((n + PT - 1) / PT);
    const dim3 grid(nt, nt);
    switch (metric) {
    case RC_METRIC_EUCLIDEAN:   k_pairwise_metric<RC_METRIC_EUCLIDEAN><<<grid, 256, 0, st>>>(d_pts, d_nrm, (int)n, (int)dim, d_D); break;
    case RC_METRIC_SQEUCLIDEAN: k_pairwise_metric<RC_METRIC_SQEUCLIDEAN><<<grid, 256, 0, st>>>(d_pts, d_nrm, (int)n, (int)dim, d_D); break;
    case RC_METRIC_CITYBLOCK:   k_pairwise_metric<RC_METRIC_CITYBLOCK><<<grid, 256, 0, st>>>(d_pts, d_nrm, (int)n, (int)dim, d_D); break;
    case RC_METRIC_CHEBYSHEV:   k_pairwise_metric<RC_METRIC_CHEBYSHEV><<<grid, 256, 0, st>>>(d_pts, d_nrm, (int)n, (int)dim, d_D); break;
    case RC_METRIC_COSINE:      k_pairwise_metric<RC_METRIC_COSINE><<<grid, 256, 0, st>>>(d_pts, d_nrm, (int)n, (int)dim, d_D); break;
    default:                    k_pairwise_metric<RC_METRIC_CORRELATION><<<grid, 256, 0, st>>>(d_pts, d_nrm, (int)n, (int)dim, d_D); break;
    }
}

}  // namespace met

// create_impl's one call for a context in a metric (declared before it): d_pts is its staging copy of the points, which
// CORRELATION would centre, so the pre-pass works on a copy of its own; the buffers go back once the stream has run them.
static hipError_t metric_matrix_for_context(int32_t metric, const double *d_pts, int64_t n, int64_t dim, double *d_D, hipStream_t st)
{
    double *d_own = nullptr, *d_nrm = nullptr;
    const double *src = d_pts;
    hipError_t e = hipSuccess;
    if (met::angular(metric)) {
        e = hipMalloc(&d_nrm, (size_t)n * sizeof(double));
        if (e == hipSuccess && metric == RC_METRIC_CORRELATION) {
            e = hipMalloc(&d_own, (size_t)n * (size_t)dim * sizeof(double));
            if (e == hipSuccess) e = hipMemcpyAsync(d_own, d_pts, (size_t)n * (size_t)dim * sizeof(double), hipMemcpyDeviceToDevice, st);
            src = d_own;
        }
        if (e == hipSuccess) met::launch_prep(metric, d_own ? d_own : const_cast<double *>(d_pts), n, dim, d_nrm, st);   // COSINE writes the norms only
    }
    if (e == hipSuccess) {
        met::launch_pairwise(metric, src, d_nrm, n, dim, d_D, st);
        e = hipGetLastError();
    }
    if (d_own || d_nrm) {
        const hipError_t es = hipStreamSynchronize(st);
        if (e == hipSuccess) e = es;
    }
    if (d_own) (void)hipFree(d_own);
    if (d_nrm) (void)hipFree(d_nrm);
    return e;
}

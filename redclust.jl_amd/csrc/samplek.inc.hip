// sampleK (src/prior.jl:316-338 of the reference): draws of K from its prior predictive, the Gumbel-max draw over the n
// log-probabilities of every sample done on the device.  fitprior2 calls it with max(10^4, 100 n) samples, which is
// 6.7·10^9 scores at n = 8192 (two lgamma each).  Algorithm and streams as restated in DESIGN.md §8.
// Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, rc_philox and the holders of
// hostutil.inc.hip).
//
// The host draws r_i ~ Gamma(η, 1/σ) and p_i ~ Beta(u, v); the device scores K = 1..n of sample i as the reference does,
//     lp[K] = (r·K)·log(1-p) + (n-K)·log(p) - log(n-K) - logbeta(r·K, n-K)   (K < n),   lp[n] = r·n·log(1-p),
// with logbeta(a, b) = lgamma(a) + lgamma(b) - lgamma(a + b) in f64 (lgamma(n-K), log(n-K) tabulated once per call; no
// contraction into fma), adds Gumbel noise -log(-log u_K) (f64 log) and keeps the first maximum.  u_K: Philox4x32-10 keyed
// (seed_lo, seed_hi ^ "SMPK"), counter (K, i_lo, i_hi, 0), u = (52 bits + 0.5)·2^-52.  Sample i is a pure function of
// (n, r_i, p_i, seed, i): the launch geometry and the split into launches do not enter.
//
// A row without a score above -inf (p = 1: every lp is -inf; or NaN from r = 0 with p = 1) returns K = 1, the limit of the
// draw as p -> 1 (and what the reference's argmax returns on that row).  K and the loop index are int32: n <= 2^30.

#define RC_SK_T 256                      // threads per workgroup: one wave per sample
#define RC_SK_MAX_N (1 << 30)
#define RC_SK_SCORES_PER_LAUNCH ((int64_t)1 << 30)   // ~10 ms of scores per launch by the op count (<< 100 ms)

namespace samplek {

__device__ __forceinline__ double uniform(u64 seed, unsigned K, u64 i)
{
    return rc_unit52(rc_philox(K, (unsigned)i, (unsigned)(i >> 32), 0, (unsigned)seed, (unsigned)(seed >> 32) ^ RC_SK_TAG));
}

// sample s of the launch is sample i0 + s of the call; lg[K] = lgamma(n-K), lnk[K] = log(n-K) for K = 1..n-1
__global__ __launch_bounds__(RC_SK_T) void k_samplek(int n, int m, const double *__restrict__ r, const double *__restrict__ p,
                                                     const double *__restrict__ lg, const double *__restrict__ lnk, u64 seed,
                                                     u64 i0, long long *__restrict__ K_out)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * (RC_SK_T / 64) + (int)(threadIdx.x >> 6);
    if (s >= m) return;
    const double rs = r[s], ps = p[s];
    const double l1p = log(1.0 - ps), lp = log(ps);
    const u64 i = i0 + (u64)s;
    double best = -INFINITY;
    int bk = 0x7fffffff;
    for (int K = 1 + lane; K <= n; K += 64) {   // ascending K per lane: strict > keeps the first maximum
        const double a = rs * (double)K;
        double v;
        if (K < n) {
            const double b = (double)(n - K);
            const double logbeta = (lgamma(a) + lg[K]) - lgamma(a + b);
            v = ((a * l1p + b * lp) - lnk[K]) - logbeta;
        } else {
            v = a * l1p;
        }
        const double sc = -log(-log(uniform(seed, (unsigned)K, i))) + v;
        if (sc > best) { best = sc; bk = K; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // wave argmax; ties to the smaller K
        const double ob = __shfl_xor(best, o);
        const int ok = __shfl_xor(bk, o);
        if (ob > best || (ob == best && ok < bk)) { best = ob; bk = ok; }
    }
    if (lane == 0) K_out[s] = (bk == 0x7fffffff) ? 1 : bk;
}

}  // namespace samplek

extern "C" int32_t rc_sample_k(int32_t device, int64_t n, int64_t m, const double *r, const double *p, uint64_t seed,
                               int64_t *K_out, double *kernel_ms)
{
    if (!r || !p || !K_out) return fail(nullptr, RC_ERR_ARG, "rc_sample_k: NULL argument");
    if (n < 1 || n > RC_SK_MAX_N) return fail(nullptr, RC_ERR_ARG, "rc_sample_k: n must be in 1..2^30 (got %lld)", (long long)n);
    if (m < 1) return fail(nullptr, RC_ERR_ARG, "rc_sample_k: need m >= 1 samples (got %lld)", (long long)m);
    int32_t rc = select_device("rc_sample_k", device);
    if (rc != RC_OK) return rc;
    std::vector<double> lg((size_t)n), lnk((size_t)n);
    for (int64_t K = 1; K < n; ++K) {
        lg[(size_t)K] = std::lgamma((double)(n - K));
        lnk[(size_t)K] = std::log((double)(n - K));
    }
    // samples per launch: ~RC_SK_SCORES_PER_LAUNCH scores, a whole number of workgroups
    const int64_t per = RC_SK_T / 64;
    const int64_t mb = std::min<int64_t>(m, std::max<int64_t>(per, std::min<int64_t>((int64_t)1 << 20, RC_SK_SCORES_PER_LAUNCH / n) / per * per));
    DeviceBuffers B;
    TimingEvents ev;
    double *d_r, *d_p, *d_lg, *d_lnk;
    long long *d_K;
    HIPCHK(nullptr, B.alloc(d_r, (size_t)mb));
    HIPCHK(nullptr, B.alloc(d_p, (size_t)mb));
    HIPCHK(nullptr, B.alloc(d_K, (size_t)mb));
    HIPCHK(nullptr, B.alloc(d_lg, (size_t)n));
    HIPCHK(nullptr, B.alloc(d_lnk, (size_t)n));
    HIPCHK(nullptr, hipMemcpy(d_lg, lg.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_lnk, lnk.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIPCHK(nullptr, ev.create());
    double ms_total = 0;
    for (int64_t i0 = 0; i0 < m; i0 += mb) {
        const int cnt = (int)std::min<int64_t>(mb, m - i0);
        HIPCHK(nullptr, hipMemcpy(d_r, r + i0, (size_t)cnt * 8, hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_p, p + i0, (size_t)cnt * 8, hipMemcpyHostToDevice));
        HIPCHK(nullptr, ev.begin(0));
        samplek::k_samplek<<<(unsigned)((cnt + per - 1) / per), RC_SK_T, 0, 0>>>((int)n, cnt, d_r, d_p, d_lg, d_lnk, seed, (u64)i0, d_K);
        HIPCHK(nullptr, ev.end(0));
        HIPCHK(nullptr, ev.elapsed_ms(ms_total));
        HIPCHK(nullptr, hipMemcpy(K_out + i0, d_K, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    }
    if (kernel_ms) *kernel_ms = ms_total;
    return RC_OK;
}

// Predict: allocate observations that were not in the fit to the clusters of every posterior sample, on the device.  Under
// one sample the allocation of a new observation is the Gibbs full conditional (src/mcmc.jl:192-252) of an (n+1)-th point
// whose own cluster is empty: the stable score of DESIGN.md §4 on the sums of the new point's distances to the n training
// points, grouped by the sample's labels, and a Gumbel-max draw.  New points are conditionally independent given a sample, so
// every (sample, new point) pair is its own problem.  DESIGN.md §8 "Predict"; the contract is in include/redclust_hip.h.
// Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, check_params, size_table, flog_table,
// quant_exponent, rc_philox, rc_flog / rc_flog1p / rc_gumbel, the holders, checks and select_device of hostutil.inc.hip).
//
// Fixed point, per new point: its row of D and its row of logD are quantised with exponents of their own (quant_exponent on
// the row), so a point's result does not depend on which other points share the call.  Every sum is an exact int64.
//
// The sums are the slab driver's (slab.inc.hip): the samples are its labellings, the new points' rows, quantised here on the
// host, its rows; RC_PREDICT_WORKSPACE_KIB and RC_PREDICT_ROWS_GLOBAL are its switches for this entry point.  Everything of a
// score that depends only on (sample, slot) — A[size] + (log p + log(size - 1 + r)) — and the new cluster's score are computed
// on the host, once, instead of once per new point; k_predict_sums does no scoring either: at a slot boundary it would run one
// lane at a time.
//
// k_predict_draw: one wave per (sample, new point), one lane per candidate: score, Philox, noise; then a wave
// argmax whose key (value, then smaller label, the new cluster last) gives the tie rule whatever the reduction order.
//
// prd::Run holds a chunk of samples on the device and does everything that follows once a chunk of new points has its rows
// there; rc_predict fills them from the host (run_samples below), rc_predict_points on the device (predictpoints.inc.hip),
// which also asks for k_draw_counts, the per-cluster summary of the draws.

namespace prd {

constexpr int TPB2 = 256;
constexpr unsigned TAG = 0x50524544u;           // "PRED": key (seed_lo, seed_hi ^ TAG), counter (label, point, sample_lo, sample_hi)
constexpr unsigned KEY_NEW = 0x7FFFFFFFu, KEY_NONE = 0xFFFFFFFFu;

struct DrawArgs {
    int ms, npts, Kmax;                     // Kmax: columns of the optional outputs (0 when neither is asked for)
    long long ktot;
    const ll2 *sums;                        // [npts][ktot]
    const long long *koff;                  // [ms]
    const int *K;                           // [ms]
    const int2 *szlab;                      // [ktot] (size, label)
    const double *base;                     // [ktot] A[size] + (log p + log(size - 1 + r))
    const double *newscore;                 // [ms] log(K + 1) + r·log(1 - p), or -inf when no new cluster is offered
    const double *scD, *scL;                // [npts] 2^-eD, 2^-eL
    const double2 *flt;
    double alpha, beta, zeta, gamma, delta1, delta2, cL;
    int repulsion;
    unsigned k0, k1;
    u64 sample0, point0;                    // counters of sample 0 and point 0 of this launch
    long long *labels, *map;                // [ms][npts]
    double *scores;                         // [ms][npts][Kmax + 1] or null
    long long *sums_out;                    // [ms][npts][Kmax][2] or null
};

__device__ __forceinline__ bool better(double v, unsigned key, double bv, unsigned bkey)
{
    return key != KEY_NONE && (bkey == KEY_NONE || v > bv || (v == bv && key < bkey));
}

__global__ __launch_bounds__(TPB2) void k_predict_draw(const DrawArgs a)
{
    const long long pair = (long long)blockIdx.x * (TPB2 / 64) + (threadIdx.x >> 6);
    if (pair >= (long long)a.ms * a.npts) return;
    const int lane = threadIdx.x & 63;
    const int i = (int)(pair / a.ms), s = (int)(pair - (long long)i * a.ms);
    const int K = a.K[s];
    const long long k0 = a.koff[s];
    const ll2 *S = a.sums + (size_t)i * (size_t)a.ktot + k0;
    const double scD = a.scD[i], scL = a.scL[i], vnew = a.newscore[s];
    const u64 sc = a.sample0 + (u64)s;
    const unsigned pc = (unsigned)(a.point0 + (u64)i), s_lo = (unsigned)sc, s_hi = (unsigned)(sc >> 32);
    const size_t o = (size_t)s * a.npts + i;
    double bv = 0.0, bm = 0.0;
    unsigned bvk = KEY_NONE, bmk = KEY_NONE;
    const int T = a.Kmax > K ? a.Kmax : K;          // columns K..Kmax-1 of the optional outputs are filled by the same loop
    for (int t = lane; t <= T; t += 64) {
        double v;
        unsigned key;
        if (t < K) {
            const ll2 x = S[t];
            const int2 zl = a.szlab[k0 + t];
            const double sz = (double)zl.x;
            const double SDr = (double)x.x * scD, SLr = (double)x.y * scL;
            double lik = a.cL * SLr - (a.alpha + a.delta1 * sz) * rc_flog1p(SDr / a.beta, a.flt);
            if (a.repulsion) lik += (a.zeta + a.delta2 * sz) * rc_flog1p(SDr / a.gamma, a.flt);
            v = a.base[k0 + t] + lik;
            key = (unsigned)zl.y;
            if (a.scores) a.scores[o * (size_t)(a.Kmax + 1) + t] = v;
            if (a.sums_out) { a.sums_out[(o * (size_t)a.Kmax + t) * 2] = x.x; a.sums_out[(o * (size_t)a.Kmax + t) * 2 + 1] = x.y; }
        } else if (t < T) {
            if (a.scores) a.scores[o * (size_t)(a.Kmax + 1) + t] = __longlong_as_double(0x7FF8000000000000ll);
            if (a.sums_out) { a.sums_out[(o * (size_t)a.Kmax + t) * 2] = 0; a.sums_out[(o * (size_t)a.Kmax + t) * 2 + 1] = 0; }
            continue;
        } else {
            if (a.scores) a.scores[o * (size_t)(a.Kmax + 1) + a.Kmax] = vnew;
            if (!(vnew > -1.79769313486231570e308)) continue;       // not offered
            v = vnew;
            key = KEY_NEW;
        }
        if (better(v, key, bm, bmk)) { bm = v; bmk = key; }
        const double g = v + rc_gumbel(rc_unit52(rc_philox(key == KEY_NEW ? 0u : key, pc, s_lo, s_hi, a.k0, a.k1)), a.flt);
        if (better(g, key, bv, bvk)) { bv = g; bvk = key; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(bv, off), om = __shfl_xor(bm, off);
        const unsigned ovk = __shfl_xor(bvk, off), omk = __shfl_xor(bmk, off);
        if (better(ov, ovk, bv, bvk)) { bv = ov; bvk = ovk; }
        if (better(om, omk, bm, bmk)) { bm = om; bmk = omk; }
    }
    if (lane == 0) {
        a.labels[o] = bvk == KEY_NEW ? 0 : (long long)bvk;
        a.map[o] = bmk == KEY_NEW ? 0 : (long long)bmk;
    }
}

// what the caller passed, after the checks
struct Call {
    int64_t n, q, m, Kmax;
    const double *Dnew, *logDnew;    // rc_predict's host rows (null for rc_predict_points, whose rows are filled on the device)
    const int64_t *samples;
    const double *r, *p;
    const rc_params *P;
    uint64_t seed, sample_offset, point_offset;
    int64_t *labels_out, *map_out, *sums_out;
    double *scores_out;
    const int *eD, *eL;              // [q]
    const int *K;                    // [m]
    const double *A;                 // [n + 1]
    const double2 *d_flt;
    bool rows_global;
    // the per-cluster summary of rc_predict_points (predictpoints.inc.hip): maps [m][maps_width], the Kp pivot labels
    // ascending, and the device [q][Kp + 1] counts of the whole call that the draws (the arg-maxes) are added to
    const int64_t *maps = nullptr, *pivot = nullptr;
    int64_t maps_width = 0, Kp = 0;
    unsigned *d_counts = nullptr, *d_mapcounts = nullptr;
};

// counts[point0 + i][col] += the samples s whose label of new point i sits in a slot of column col: labels [ms][npts] as
// k_predict_draw wrote them (0: column 0), a sample's slots in ascending label order, colslot [ktot] the column of every slot.
// One block per new point, the histogram in LDS (Kp + 1 counters); the launches of one stream follow each other, so the
// block adds to its own row of the counts without atomics.
__global__ __launch_bounds__(TPB2) void k_draw_counts(const long long *__restrict__ labels, int ms, int npts, const long long *__restrict__ koff,
                                                         const int *__restrict__ K, const int2 *__restrict__ szlab, const int *__restrict__ colslot,
                                                         int ncols, unsigned *__restrict__ counts)
{
    extern __shared__ unsigned prd_hist[];
    const int i = blockIdx.x;
    for (int k = threadIdx.x; k < ncols; k += TPB2) prd_hist[k] = 0;
    __syncthreads();
    for (int s = threadIdx.x; s < ms; s += TPB2) {
        const int l = (int)labels[(size_t)s * npts + i];
        int col = 0;
        if (l > 0) {
            const long long k0 = koff[s];
            int lo = 0, hi = K[s] - 1;              // the label is one of the sample's: the search ends on it
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (szlab[k0 + mid].y < l) lo = mid + 1; else hi = mid;
            }
            col = colslot[k0 + lo];
        }
        atomicAdd(&prd_hist[col], 1u);
    }
    __syncthreads();
    unsigned *row = counts + (size_t)i * (size_t)ncols;
    for (int k = threadIdx.x; k < ncols; k += TPB2) {
        const unsigned h = prd_hist[k];
        if (h) row[k] += h;
    }
}

// A chunk of samples s0 .. s0 + ms - 1 on the device — their sorted orders, the host's part of their scores, the buffers of at
// most qc new points — and everything that follows once the (Dq, Lq) rows and the scales of a chunk of new points are in
// d_rows, d_scD and d_scL: rc_predict fills them from the host, rc_predict_points on the device.
struct Run {
    Orders O;
    DeviceBuffers B;
    TimingEvents ev;
    int64_t s0 = 0, ms = 0;
    int Kcols = 0;
    long long ktot = 0;
    double *d_base = nullptr, *d_newscore = nullptr, *d_scD = nullptr, *d_scL = nullptr, *d_scores = nullptr;
    ll2 *d_rows = nullptr, *d_sums = nullptr;
    long long *d_labels = nullptr, *d_map = nullptr, *d_sums_out = nullptr;
    int *d_colslot = nullptr;
    std::vector<long long> h_lab, h_tab;
    std::vector<double> h_sc;

    int32_t begin(const char *who, const Call &c, int64_t s0_, int64_t ms_, int64_t qc)
    {
        s0 = s0_; ms = ms_;
        const int64_t n = c.n;
        const bool want_tab = c.scores_out || c.sums_out;
        Kcols = want_tab ? (int)c.Kmax : 0;
        std::vector<double> base, newscore;
        std::vector<int> colslot;
        bool ok = true;
        try {
            long long kt = 0;
            for (int64_t s = 0; s < ms; ++s) kt += c.K[s0 + s];
            base.resize((size_t)kt); newscore.resize((size_t)ms);
            if (c.d_counts || c.d_mapcounts) colslot.resize((size_t)kt);
        } catch (const std::bad_alloc &) { ok = false; }
        ok = ok && O.build(c.samples, n, c.K, s0, ms, false, [&](int64_t s, long long at, int64_t, int sz) {
            base[(size_t)at] = c.A[sz] + (std::log(c.p[s0 + s]) + std::log((double)sz - 1.0 + c.r[s0 + s]));
        });
        if (!ok) return fail(nullptr, RC_ERR_OOM, "%s: no host memory for the sorted orders of %lld samples", who, (long long)ms);
        ktot = O.ktot;
        for (int64_t s = 0; s < ms; ++s) {
            const double r = c.r[s0 + s], p = c.p[s0 + s];
            const int K = O.Ks[(size_t)s];
            newscore[(size_t)s] = (c.P->maxK == 0 || K < c.P->maxK) ? std::log((double)(K + 1)) + r * std::log(1 - p) : -INFINITY;
            if (colslot.empty()) continue;
            for (int t = 0; t < K; ++t) {           // checked by the entry point: 0 or a pivot label
                const int64_t to = c.maps[(size_t)(s0 + s) * c.maps_width + t];
                colslot[(size_t)(O.koff[(size_t)s] + t)] = to > 0 ? (int)(std::lower_bound(c.pivot, c.pivot + c.Kp, to) - c.pivot) + 1 : 0;
            }
        }

        HIPCHK(nullptr, O.upload(B));
        HIPCHK(nullptr, B.alloc(d_base, (size_t)ktot));
        HIPCHK(nullptr, B.alloc(d_newscore, (size_t)ms));
        HIPCHK(nullptr, B.alloc(d_scD, (size_t)qc));
        HIPCHK(nullptr, B.alloc(d_scL, (size_t)qc));
        HIPCHK(nullptr, B.alloc(d_rows, (size_t)qc * n));
        HIPCHK(nullptr, B.alloc(d_sums, (size_t)qc * ktot));
        HIPCHK(nullptr, B.alloc(d_labels, (size_t)qc * ms));
        HIPCHK(nullptr, B.alloc(d_map, (size_t)qc * ms));
        if (c.scores_out) HIPCHK(nullptr, B.alloc(d_scores, (size_t)qc * ms * (Kcols + 1)));
        if (c.sums_out) HIPCHK(nullptr, B.alloc(d_sums_out, (size_t)qc * ms * std::max(Kcols, 1) * 2));
        HIPCHK(nullptr, hipMemcpy(d_base, base.data(), (size_t)ktot * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_newscore, newscore.data(), (size_t)ms * sizeof(double), hipMemcpyHostToDevice));
        if (!colslot.empty()) {
            HIPCHK(nullptr, B.alloc(d_colslot, (size_t)ktot));
            HIPCHK(nullptr, hipMemcpy(d_colslot, colslot.data(), (size_t)ktot * sizeof(int), hipMemcpyHostToDevice));
        }
        try {
            if (c.labels_out || c.map_out) h_lab.resize((size_t)qc * ms);
            if (c.scores_out) h_sc.resize((size_t)qc * ms * (Kcols + 1));
            if (c.sums_out) h_tab.resize((size_t)qc * ms * std::max(Kcols, 1) * 2);
        } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for a chunk of %lld new points", who, (long long)qc); }
        HIPCHK(nullptr, ev.create());
        return RC_OK;
    }

    // new points i0 .. i0 + np - 1, their rows and scales on the device: sums, draws, the outputs.  ms_acc: device milliseconds, added to.
    int32_t finish(const Call &c, int64_t i0, int64_t np, double &ms_acc)
    {
        const rc_params &P = *c.P;
        DrawArgs a{};
        a.ms = (int)ms; a.npts = (int)np; a.Kmax = Kcols; a.ktot = ktot; a.sums = d_sums; a.koff = O.d_koff; a.K = O.d_K; a.szlab = O.d_szlab;
        a.base = d_base; a.newscore = d_newscore; a.scD = d_scD; a.scL = d_scL; a.flt = c.d_flt;
        a.alpha = P.alpha; a.beta = P.beta; a.zeta = P.zeta; a.gamma = P.gamma; a.delta1 = P.delta1; a.delta2 = P.delta2;
        a.cL = (P.delta1 - 1.0) - (P.repulsion ? (P.delta2 - 1.0) : 0.0);
        a.repulsion = P.repulsion ? 1 : 0;
        a.k0 = (unsigned)c.seed; a.k1 = (unsigned)(c.seed >> 32) ^ TAG;
        a.sample0 = c.sample_offset + (uint64_t)s0; a.point0 = c.point_offset + (uint64_t)i0;
        a.labels = d_labels; a.map = d_map; a.scores = d_scores; a.sums_out = d_sums_out;
        HIPCHK(nullptr, ev.begin(0));
        HIPCHK(nullptr, O.launch_sums(d_rows, np, c.rows_global, d_sums));
        k_predict_draw<<<(unsigned)(((size_t)np * ms + TPB2 / 64 - 1) / (TPB2 / 64)), TPB2, 0, 0>>>(a);
        for (int pass = 0; pass < 2; ++pass) {
            unsigned *cnt = pass ? c.d_mapcounts : c.d_counts;
            if (!cnt) continue;
            const int ncols = (int)c.Kp + 1;
            const size_t lds = (size_t)ncols * sizeof(unsigned);
            HIPCHK(nullptr, set_dynamic_lds(k_draw_counts, lds));
            k_draw_counts<<<(unsigned)np, TPB2, lds, 0>>>(pass ? d_map : d_labels, (int)ms, (int)np, O.d_koff, O.d_K, O.d_szlab, d_colslot, ncols,
                                                             cnt + (size_t)i0 * (size_t)ncols);
        }
        HIPCHK(nullptr, ev.end(0));
        HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
        // device [ms][np][..] into the caller's [m][q][..]
        for (int pass = 0; pass < 2; ++pass) {
            int64_t *dst = pass ? c.map_out : c.labels_out;
            if (!dst) continue;
            HIPCHK(nullptr, hipMemcpy(h_lab.data(), pass ? d_map : d_labels, (size_t)np * ms * sizeof(long long), hipMemcpyDeviceToHost));
            for (int64_t s = 0; s < ms; ++s) memcpy(dst + (size_t)(s0 + s) * c.q + i0, h_lab.data() + (size_t)s * np, (size_t)np * sizeof(int64_t));
        }
        if (c.scores_out) {
            const size_t w = (size_t)Kcols + 1;
            HIPCHK(nullptr, hipMemcpy(h_sc.data(), d_scores, (size_t)np * ms * w * sizeof(double), hipMemcpyDeviceToHost));
            for (int64_t s = 0; s < ms; ++s) memcpy(c.scores_out + ((size_t)(s0 + s) * c.q + i0) * w, h_sc.data() + (size_t)s * np * w, (size_t)np * w * sizeof(double));
        }
        if (c.sums_out && Kcols > 0) {
            const size_t w = (size_t)Kcols * 2;
            HIPCHK(nullptr, hipMemcpy(h_tab.data(), d_sums_out, (size_t)np * ms * w * sizeof(long long), hipMemcpyDeviceToHost));
            for (int64_t s = 0; s < ms; ++s) memcpy(c.sums_out + ((size_t)(s0 + s) * c.q + i0) * w, h_tab.data() + (size_t)s * np * w, (size_t)np * w * sizeof(int64_t));
        }
        return RC_OK;
    }
};

// rc_predict: samples s0 .. s0 + ms - 1 against every new point, the points in chunks of at most qc whose rows are quantised
// here on the host.  ms_acc: device milliseconds, added to.
static int32_t run_samples(const char *who, const Call &c, int64_t s0, int64_t ms, int64_t qc, double &ms_acc)
{
    const int64_t n = c.n;
    Run R;
    int32_t rc = R.begin(who, c, s0, ms, qc);
    if (rc != RC_OK) return rc;
    std::vector<ll2> rows;
    std::vector<double> scD, scL;
    try { rows.resize((size_t)qc * n); scD.resize((size_t)qc); scL.resize((size_t)qc); }
    catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for a chunk of %lld new points", who, (long long)qc); }
    for (int64_t i0 = 0; i0 < c.q; i0 += qc) {
        const int64_t np = std::min(qc, c.q - i0);
        for (int64_t i = 0; i < np; ++i) {
            const double *x = c.Dnew + (size_t)(i0 + i) * n, *lx = c.logDnew ? c.logDnew + (size_t)(i0 + i) * n : nullptr;
            const int eD = c.eD[i0 + i], eL = c.eL[i0 + i];
            ll2 *dst = rows.data() + (size_t)i * n;
            for (int64_t j = 0; j < n; ++j) {
                dst[j].x = std::llrint(std::ldexp(x[j], eD));
                dst[j].y = std::llrint(std::ldexp(lx ? lx[j] : std::log(x[j]), eL));
            }
            scD[(size_t)i] = std::ldexp(1.0, -eD); scL[(size_t)i] = std::ldexp(1.0, -eL);
        }
        HIPCHK(nullptr, hipMemcpy(R.d_rows, rows.data(), (size_t)np * n * sizeof(ll2), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(R.d_scD, scD.data(), (size_t)np * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(R.d_scL, scL.data(), (size_t)np * sizeof(double), hipMemcpyHostToDevice));
        rc = R.finish(c, i0, np, ms_acc);
        if (rc != RC_OK) return rc;
    }
    return RC_OK;
}

}  // namespace prd

extern "C" int32_t rc_predict(int32_t device, int64_t n, int64_t q, const double *Dnew, const double *logDnew_or_null, int64_t m,
                              const int64_t *samples, const double *r, const double *p, const rc_params *params, uint64_t seed,
                              uint64_t sample_offset, uint64_t point_offset, int64_t *labels_out, int64_t *map_out, int64_t Kmax,
                              double *scores_out, int64_t *sums_out, int32_t *eD_out, int32_t *eL_out, double *kernel_ms)
{
    const char *who = "rc_predict";
    if (!Dnew || !samples || !r || !p || !params || !labels_out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (n < 1 || q < 1 || m < 1) return fail(nullptr, RC_ERR_ARG, "%s: need n >= 1, q >= 1 and m >= 1 (got n=%lld q=%lld m=%lld)", who, (long long)n, (long long)q, (long long)m);
    int32_t rc = check_label_shape(nullptr, who, n, "training points", m, "m");
    if (rc != RC_OK) return rc;
    rc = check_params(nullptr, who, params);
    if (rc != RC_OK) return rc;
    rc = check_r_p(nullptr, who, "sample", m, r, p);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    const bool want_tab = scores_out || sums_out;
    std::vector<int> K, eD, eL, seen;
    std::vector<double> A;
    try { K.assign((size_t)m, 0); eD.resize((size_t)q); eL.resize((size_t)q); seen.assign((size_t)n + 1, -1); A.resize((size_t)n + 1); }
    catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    const int64_t over = count_clusters(samples, m, n, want_tab ? Kmax : n, seen, K.data());
    if (over < m) return fail(nullptr, RC_ERR_ARG, "%s: sample %lld has %d clusters, Kmax = %lld", who, (long long)over + 1, K[(size_t)over], (long long)Kmax);
    for (int64_t i = 0; i < q; ++i) {
        const double *x = Dnew + (size_t)i * n, *lx = logDnew_or_null ? logDnew_or_null + (size_t)i * n : nullptr;
        double lo = INFINITY, hi = 0.0, lmax = 0.0;
        for (int64_t j = 0; j < n; ++j) {
            if (!(x[j] > 0.0 && x[j] <= 1.79769313486231570e308))
                return fail(nullptr, RC_ERR_DOMAIN, "%s: Dnew[%lld][%lld] = %g is not a positive finite distance", who, (long long)i + 1, (long long)j + 1, x[j]);
            lo = std::min(lo, x[j]); hi = std::max(hi, x[j]);
            if (lx) {
                if (!(std::fabs(lx[j]) <= 1.79769313486231570e308)) return fail(nullptr, RC_ERR_DOMAIN, "%s: logDnew[%lld][%lld] is not finite", who, (long long)i + 1, (long long)j + 1);
                lmax = std::max(lmax, std::fabs(lx[j]));
            }
        }
        if (!lx) lmax = std::max(std::fabs(std::log(lo)), std::fabs(std::log(hi)));   // log is monotone: the row's largest |log|
        eD[(size_t)i] = quant_exponent(n, hi, 64);
        eL[(size_t)i] = quant_exponent(n, lmax, 64);
        if (eD_out) eD_out[i] = eD[(size_t)i];
        if (eL_out) eL_out[i] = eL[(size_t)i];
    }
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
    prd::Call c{n, q, m, want_tab ? Kmax : 0, Dnew, logDnew_or_null, samples, r, p, params, seed, sample_offset, point_offset,
                labels_out, map_out, sums_out, scores_out, eD.data(), eL.data(), K.data(), A.data(), d_flt,
                env_flag("RC_PREDICT_ROWS_GLOBAL")};                       // tests: gather from the rows in global memory at small n
    // Chunks.  Device bytes per new point for a run of samples: its row, and per sample its slots' sums, two labels and the
    // optional columns.  Samples are taken while 512 points (or all q) of them fit the workspace and their sorted orders fit
    // theirs; the points then go in chunks of what fits.
    const size_t workspace = env_workspace_kib("RC_PREDICT_WORKSPACE_KIB", slab::WORKSPACE);
    const size_t per_sample = 16 + (scores_out ? 8 * ((size_t)c.Kmax + 1) : 0) + (sums_out ? 16 * (size_t)c.Kmax : 0);
    const int64_t ms_cap = slab_ms_cap(slab::PERM_BYTES, 2, n);
    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < m;) {
        const SlabChunk ch = slab_plan(s0, K.data(), m, ms_cap, 16 * (size_t)n, per_sample, q, std::min<int64_t>(q, 512), workspace);
        rc = prd::run_samples(who, c, s0, ch.ms, ch.qc, ms_acc);
        if (rc != RC_OK) return rc;
        s0 += ch.ms;
    }
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

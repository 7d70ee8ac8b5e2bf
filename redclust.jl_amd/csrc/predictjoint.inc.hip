// Joint predict: allocate q new observations to the clusters of every posterior sample so that they may form clusters with each
// other.  One sample (training labels z, r, p) is one independent problem whose state is z, which never changes, and the labels
// y_1..y_q of the new points, which start unallocated.  A visit of new point i is the Gibbs full conditional (src/mcmc.jl:192-252)
// of point n+i of the (n+q)-point problem in which the unallocated points do not exist; pass 0 visits 1..q in order (sequential
// allocation), `sweeps` further passes visit them again (Gibbs on the new labels given the training labels).  DESIGN.md §8
// "Joint predict"; the contract is in include/redclust_hip.h.  Included at the end of redclust_hip.hip after slab.inc.hip, whose
// sorted orders and k_predict_sums give the base sums (the samples are its labellings, the new points' training parts its rows,
// all q together; RC_PREDICT_WORKSPACE_KIB and RC_PREDICT_ROWS_GLOBAL are its switches here too), and after predict.inc.hip,
// whose tie rule (prd::better) it uses.
//
// Fixed point: new point i's row is the n entries of Dnew[i] followed by the q entries of Dnn[i] (the diagonal entry counts as
// 0), quantised with one exponent of its own for n + q addends; its logarithms likewise.  Every sum is an exact int64.
//
// Slots of a sample: 0..K-1 its training clusters in ascending label order, K..K+q-1 the clusters that new points may open;
// slot K+a carries the a-th smallest label of 1..n+q that the training labels do not use, so "the lowest label without a member"
// is the lowest new slot without a member.  The training part of every (new point, sample, slot) sum comes from k_predict_sums
// (the base sums); the new points' part is added up again at every visit, because it changes with every visit.
//
// k_joint (one 256-thread workgroup per sample, its state in LDS: per slot two int64 accumulators, a size and a label, and per
// new point its slot).  A visit of point i at visit index v:
//   A  the threads stride over the allocated new points j != i and add (Dq, Lq) of row i's new part into slot y_j's accumulators
//      with 64-bit integer LDS atomics: exact whatever the order.  Barrier.
//   B  the threads stride over the slots; a slot with members beside i forms base sum + accumulator, clears the accumulator, and
//      evaluates score, Philox and Gumbel noise; a new slot without members is a candidate for the lowest free one.  Wave argmax
//      (and min) by xor-shuffles, the four partials through LDS.  Barrier.
//   C  every thread combines the partials and adds the new-cluster candidate, so all know the winner's slot; thread 0 commits
//      sizes, y_i, K, the high-water mark of the new slots, moves and the labels; the thread that scored the winner writes its
//      sums.
// The next visit reads sizes, K and y_i only behind its first barrier, and in phase A takes the slot of the point just
// committed from its registers, so two barriers per visit suffice.

namespace prdj {

constexpr int TPB = 256, NWAVE = TPB / 64;
constexpr int64_t SLOT_MAX = 4096;              // slots of a sample (K_s + q): 24 B each in LDS
constexpr unsigned TAG = 0x5052444Au;           // "PRDJ": key (seed_lo, seed_hi ^ TAG), counter (label, visit, sample_lo, sample_hi)
constexpr unsigned KEY_NEW = prd::KEY_NEW, KEY_NONE = prd::KEY_NONE;
constexpr unsigned NO_SLOT = 0xFFFFFFFFu;

struct Args {
    int q, S;                               // S: slots the LDS is carved for (the chunk's largest K_s + q)
    long long sweeps, ktot;
    const ll2 *base;                        // [q][ktot] training part of every sum
    const ll2 *rown;                        // [q][q] (Dq, Lq) of new point i against new point j, 0 on the diagonal
    const long long *koff;                  // [ms]
    const int *K;                           // [ms]
    const int2 *szlab;                      // [ktot] (size, label) of the training clusters
    const int *freelab;                     // [ms][q] the labels new clusters take, ascending
    const double *A;                        // [n + q + 1]
    const double *r, *logp, *log1mp;        // [ms]
    const double *scD, *scL;                // [q] 2^-eD, 2^-eL
    const double2 *flt;
    double alpha, beta, zeta, gamma, delta1, delta2, cL;
    int repulsion;
    long long maxK;
    unsigned k0, k1;
    u64 sample0;                            // counter of sample 0 of this launch
    long long *labels, *first;              // [ms][q]; first may be null
    long long *Kout;                        // [ms]
    long long *moves;                       // [ms][sweeps + 1] or null
    long long *sums_out;                    // [ms][q][2] or null
};

__global__ __launch_bounds__(TPB) void k_joint(const Args a)
{
    extern __shared__ __align__(16) unsigned char prdj_lds[];
    __shared__ double p_v[NWAVE];
    __shared__ unsigned p_key[NWAVE], p_slot[NWAVE], p_free[NWAVE];
    __shared__ int s_K, s_hw;                                   // live clusters; new slots used so far (high-water mark)
    ll2 *acc = reinterpret_cast<ll2 *>(prdj_lds);               // [S]
    int *sz = reinterpret_cast<int *>(acc + a.S);               // [S]
    int *lab = sz + a.S;                                        // [S]
    int *y = lab + a.S;                                         // [q] slot of every new point, -1: unallocated

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = blockIdx.x, q = a.q;
    const int K0 = a.K[s];
    const long long k0 = a.koff[s];
    const int *fl = a.freelab + (size_t)s * q;
    for (int t = tid; t < K0 + q; t += TPB) {
        ll2 z; z.x = 0; z.y = 0;
        acc[t] = z;
        if (t < K0) { const int2 zl = a.szlab[k0 + t]; sz[t] = zl.x; lab[t] = zl.y; }
        else { sz[t] = 0; lab[t] = fl[t - K0]; }
    }
    for (int j = tid; j < q; j += TPB) y[j] = -1;
    if (tid == 0) { s_K = K0; s_hw = 0; }
    const double r = a.r[s], logp = a.logp[s], log1mp = a.log1mp[s];
    const u64 sc = a.sample0 + (u64)s;
    const unsigned s_lo = (unsigned)sc, s_hi = (unsigned)(sc >> 32);
    long long *labels = a.labels + (size_t)s * q;
    long long moved = 0;                                        // thread 0's count of the pass
    int iprev = -1;
    unsigned wprev = NO_SLOT;
    __syncthreads();

    for (long long pass = 0; pass <= a.sweeps; ++pass) {
        for (int i = 0; i < q; ++i) {
            const unsigned vis = (unsigned)pass * (unsigned)q + (unsigned)i;
            const ll2 *B = a.base + (size_t)i * (size_t)a.ktot + k0;
            const ll2 *R = a.rown + (size_t)i * q;
            // the first base sum of this thread is requested ahead of phase A's row reads
            ll2 b0; b0.x = 0; b0.y = 0;
            if (tid < K0) b0 = B[tid];
            // ---- A
            for (int j = tid; j < q; j += TPB) {
                if (j == i) continue;
                const int yj = j == iprev ? (int)wprev : y[j];
                if (yj < 0) continue;
                const ll2 x = R[j];
                u64 *o = reinterpret_cast<u64 *>(acc + yj);
                atomicAdd(o, (u64)x.x);
                atomicAdd(o + 1, (u64)x.y);
            }
            __syncthreads();
            // ---- B
            const int yi = y[i];
            const int Kc = s_K, hw = s_hw;
            const int Ki = Kc - ((yi >= 0 && sz[yi] == 1) ? 1 : 0);
            const int lim = K0 + min(q, hw + 1);
            const double scD = a.scD[i], scL = a.scL[i];
            double bv = 0.0;
            unsigned bkey = KEY_NONE, bslot = NO_SLOT, minfree = NO_SLOT;
            long long bsd = 0, bsl = 0;
            for (int t = tid; t < lim; t += TPB) {
                const int e = sz[t] - (t == yi ? 1 : 0);
                if (e <= 0) { minfree = min(minfree, (unsigned)t); continue; }      // (a training slot never gets here)
                ll2 x = acc[t];
                if (x.x | x.y) { ll2 z; z.x = 0; z.y = 0; acc[t] = z; }
                if (t < K0) { const ll2 b = t == tid ? b0 : B[t]; x.x += b.x; x.y += b.y; }
                const double szd = (double)e;
                const double SDr = (double)x.x * scD, SLr = (double)x.y * scL;
                double lik = a.cL * SLr - (a.alpha + a.delta1 * szd) * rc_flog1p(SDr / a.beta, a.flt);
                if (a.repulsion) lik += (a.zeta + a.delta2 * szd) * rc_flog1p(SDr / a.gamma, a.flt);
                const double v = (a.A[e] + (logp + rc_flog(szd - 1.0 + r, a.flt))) + lik;
                const unsigned key = (unsigned)lab[t];
                const double g = v + rc_gumbel(rc_unit52(rc_philox(key, vis, s_lo, s_hi, a.k0, a.k1)), a.flt);
                if (prd::better(g, key, bv, bkey)) { bv = g; bkey = key; bslot = (unsigned)t; bsd = x.x; bsl = x.y; }
            }
            const unsigned mykey = bkey;
            double wv = bv;
            unsigned wkey = bkey, wslot = bslot;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double ov = __shfl_xor(wv, off);
                const unsigned ok = __shfl_xor(wkey, off), os = __shfl_xor(wslot, off);
                if (prd::better(ov, ok, wv, wkey)) { wv = ov; wkey = ok; wslot = os; }
                minfree = min(minfree, (unsigned)__shfl_xor((int)minfree, off));
            }
            if (lane == 0) { p_v[wave] = wv; p_key[wave] = wkey; p_slot[wave] = wslot; p_free[wave] = minfree; }
            __syncthreads();
            // ---- C
            wv = p_v[0]; wkey = p_key[0]; wslot = p_slot[0]; minfree = p_free[0];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) {
                if (prd::better(p_v[w], p_key[w], wv, wkey)) { wv = p_v[w]; wkey = p_key[w]; wslot = p_slot[w]; }
                minfree = min(minfree, p_free[w]);
            }
            if (a.maxK == 0 || Ki < a.maxK) {
                // i's removal always leaves a new slot without members among the first min(q, hw + 1)
                const double v = rc_flog((double)(Ki + 1), a.flt) + r * log1mp;
                const double g = v + rc_gumbel(rc_unit52(rc_philox(0u, vis, s_lo, s_hi, a.k0, a.k1)), a.flt);
                if (prd::better(g, KEY_NEW, wv, wkey)) { wv = g; wkey = KEY_NEW; wslot = minfree; }
            }
            if (a.sums_out) {
                long long *o = a.sums_out + ((size_t)s * q + i) * 2;
                if (wkey == KEY_NEW) { if (tid == 0) { o[0] = 0; o[1] = 0; } }
                else if (mykey == wkey) { o[0] = bsd; o[1] = bsl; }
            }
            if (tid == 0) {
                const int w = (int)wslot;
                if (w != yi) {
                    ++moved;
                    if (yi >= 0) sz[yi] -= 1;
                    sz[w] += 1;
                    y[i] = w;
                    s_K = Ki + (wkey == KEY_NEW ? 1 : 0);
                    if (w - K0 + 1 > hw) s_hw = w - K0 + 1;
                }
                const long long name = (long long)lab[w];
                labels[i] = name;
                if (pass == 0 && a.first) a.first[(size_t)s * q + i] = name;
            }
            iprev = i; wprev = wslot;
        }
        if (tid == 0) {
            if (a.moves) a.moves[(size_t)s * (size_t)(a.sweeps + 1) + (size_t)pass] = moved;
            moved = 0;
        }
    }
    if (tid == 0) a.Kout[s] = (long long)s_K;
}

constexpr size_t lds_bytes(int64_t S, int64_t q) { return (size_t)S * 24 + (size_t)q * 4; }

}  // namespace prdj

extern "C" int32_t rc_predict_joint(int32_t device, int64_t n, int64_t q, const double *Dnew, const double *Dnn, const double *logDnew_or_null,
                                    const double *logDnn_or_null, int64_t m, const int64_t *samples, const double *r, const double *p,
                                    const rc_params *params, int64_t sweeps, uint64_t seed, uint64_t sample_offset, int64_t *labels_out,
                                    int64_t *first_out, int64_t *K_out, int64_t *moves_out, int64_t *sums_out, int32_t *eD_out,
                                    int32_t *eL_out, double *kernel_ms)
{
    const char *who = "rc_predict_joint";
    if (!Dnew || !Dnn || !samples || !r || !p || !params || !labels_out || !K_out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if ((logDnew_or_null == nullptr) != (logDnn_or_null == nullptr)) return fail(nullptr, RC_ERR_ARG, "%s: give logDnew and logDnn together or neither", who);
    if (n < 1 || q < 1 || m < 1) return fail(nullptr, RC_ERR_ARG, "%s: need n >= 1, q >= 1 and m >= 1 (got n=%lld q=%lld m=%lld)", who, (long long)n, (long long)q, (long long)m);
    if (sweeps < 0) return fail(nullptr, RC_ERR_ARG, "%s: sweeps must be >= 0 (got %lld)", who, (long long)sweeps);
    int32_t rc = check_label_shape(nullptr, who, n, "training points", m, "m");
    if (rc != RC_OK) return rc;
    if (q >= prdj::SLOT_MAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: q = %lld new points and a cluster do not fit the %lld slots of a sample; call in blocks", who, (long long)q, (long long)prdj::SLOT_MAX);
    if (sweeps >= (((int64_t)1 << 32) - 1) / q) return fail(nullptr, RC_ERR_ARG, "%s: (sweeps + 1)·q = (%lld + 1)·%lld is not below 2^32", who, (long long)sweeps, (long long)q);
    rc = check_params(nullptr, who, params);
    if (rc != RC_OK) return rc;
    rc = check_r_p(nullptr, who, "sample", m, r, p, true);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    const int64_t N = n + q;
    std::vector<int> K, eD, eL, seen;
    std::vector<double> A, scD, scL;
    std::vector<ll2> rowt, rown;
    try { K.assign((size_t)m, 0); seen.assign((size_t)n + 1, -1); }
    catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    const int64_t over = count_clusters(samples, m, n, prdj::SLOT_MAX - q, seen, K.data());
    if (over < m)
        return fail(nullptr, RC_ERR_CAPACITY, "%s: sample %lld has %d clusters; with q = %lld new points that exceeds the %lld slots of a sample; call in blocks", who, (long long)over + 1, K[(size_t)over], (long long)q, (long long)prdj::SLOT_MAX);
    try {
        eD.resize((size_t)q); eL.resize((size_t)q); A.resize((size_t)N + 1); scD.resize((size_t)q); scL.resize((size_t)q);
        rowt.resize((size_t)q * n); rown.resize((size_t)q * q);
    } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    // the checks of both distance blocks, the exponents of every extended row
    for (int64_t i = 0; i < q; ++i) {
        double lo = INFINITY, hi = 0.0, lmax = 0.0;
        for (int64_t j = 0; j < N; ++j) {
            const bool tr = j < n;
            if (!tr && j - n == i) continue;                                       // the diagonal entry is ignored
            const size_t at = tr ? (size_t)i * n + j : (size_t)i * q + (j - n);
            const double x = tr ? Dnew[at] : Dnn[at];
            if (!(x > 0.0 && x <= 1.79769313486231570e308))
                return fail(nullptr, RC_ERR_DOMAIN, "%s: %s[%lld][%lld] = %g is not a positive finite distance", who, tr ? "Dnew" : "Dnn", (long long)i + 1, (long long)(tr ? j : j - n) + 1, x);
            if (!tr && x != Dnn[(size_t)(j - n) * q + i])
                return fail(nullptr, RC_ERR_DOMAIN, "%s: Dnn is not symmetric at [%lld][%lld]", who, (long long)i + 1, (long long)(j - n) + 1);
            lo = std::min(lo, x); hi = std::max(hi, x);
            if (logDnew_or_null) {
                const double lx = tr ? logDnew_or_null[at] : logDnn_or_null[at];
                if (!(std::fabs(lx) <= 1.79769313486231570e308))
                    return fail(nullptr, RC_ERR_DOMAIN, "%s: %s[%lld][%lld] is not finite", who, tr ? "logDnew" : "logDnn", (long long)i + 1, (long long)(tr ? j : j - n) + 1);
                lmax = std::max(lmax, std::fabs(lx));
            }
        }
        if (!logDnew_or_null) lmax = std::max(std::fabs(std::log(lo)), std::fabs(std::log(hi)));   // log is monotone: the row's largest |log|
        eD[(size_t)i] = quant_exponent(N, hi, 64);
        eL[(size_t)i] = quant_exponent(N, lmax, 64);
        if (eD_out) eD_out[i] = eD[(size_t)i];
        if (eL_out) eL_out[i] = eL[(size_t)i];
    }
    rc = select_device(who, device);
    if (rc != RC_OK) return rc;

    for (int64_t i = 0; i < q; ++i) {
        const int d = eD[(size_t)i], l = eL[(size_t)i];
        for (int64_t j = 0; j < n; ++j) {
            const size_t at = (size_t)i * n + j;
            rowt[at].x = std::llrint(std::ldexp(Dnew[at], d));
            rowt[at].y = std::llrint(std::ldexp(logDnew_or_null ? logDnew_or_null[at] : std::log(Dnew[at]), l));
        }
        for (int64_t j = 0; j < q; ++j) {
            const size_t at = (size_t)i * q + j;
            rown[at].x = j == i ? 0 : std::llrint(std::ldexp(Dnn[at], d));
            rown[at].y = j == i ? 0 : std::llrint(std::ldexp(logDnn_or_null ? logDnn_or_null[at] : std::log(Dnn[at]), l));
        }
        scD[(size_t)i] = std::ldexp(1.0, -d); scL[(size_t)i] = std::ldexp(1.0, -l);
    }
    size_table(params, N, A.data());

    DeviceBuffers B;
    double2 *d_flt; double *d_A, *d_scD, *d_scL; ll2 *d_rowt, *d_rown;
    {
        double2 ft[128];
        flog_table(ft);
        HIPCHK(nullptr, B.alloc(d_flt, 128));
        HIPCHK(nullptr, hipMemcpy(d_flt, ft, sizeof(ft), hipMemcpyHostToDevice));
    }
    HIPCHK(nullptr, B.alloc(d_A, A.size()));
    HIPCHK(nullptr, B.alloc(d_scD, (size_t)q));
    HIPCHK(nullptr, B.alloc(d_scL, (size_t)q));
    HIPCHK(nullptr, B.alloc(d_rowt, rowt.size()));
    HIPCHK(nullptr, B.alloc(d_rown, rown.size()));
    HIPCHK(nullptr, hipMemcpy(d_A, A.data(), A.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_scD, scD.data(), (size_t)q * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_scL, scL.data(), (size_t)q * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_rowt, rowt.data(), rowt.size() * sizeof(ll2), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_rown, rown.data(), rown.size() * sizeof(ll2), hipMemcpyHostToDevice));

    // Chunks of samples: the base sums of a chunk, q·16·ΣK_s bytes, fit the workspace (one sample always goes), and its sorted
    // orders fit theirs.  The new points of a call always travel together.
    const size_t workspace = env_workspace_kib("RC_PREDICT_WORKSPACE_KIB", slab::WORKSPACE);
    const int64_t ms_cap = slab_ms_cap(slab::PERM_BYTES, 2, n);
    const bool rows_global = env_flag("RC_PREDICT_ROWS_GLOBAL");
    const size_t nm = (size_t)sweeps + 1;
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());
    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < m;) {
        const int64_t ms = slab_plan(s0, K.data(), m, ms_cap, 0, 0, q, q, workspace).ms;   // no row of its own, q rows at once
        const int64_t Smax = *std::max_element(K.begin() + s0, K.begin() + s0 + ms) + q;
        prd::Orders O;
        std::vector<int> freelab;
        std::vector<double> logp, log1mp;
        bool ok = true;
        try { freelab.resize((size_t)ms * q); logp.resize((size_t)ms); log1mp.resize((size_t)ms); seen.assign((size_t)N + 2, 0); }
        catch (const std::bad_alloc &) { ok = false; }
        ok = ok && O.build(samples, n, K.data(), s0, ms, false, [](int64_t, long long, int64_t, int) {});
        if (!ok) return fail(nullptr, RC_ERR_OOM, "%s: no host memory for the sorted orders of %lld samples", who, (long long)ms);
        for (int64_t s = 0; s < ms; ++s) {
            // the q smallest labels of 1..n+q that sample s does not use, ascending
            const int64_t *z = samples + (size_t)(s0 + s) * n;
            for (int64_t j = 0; j < n; ++j) seen[(size_t)z[j]] = (int)s + 1;
            int64_t got = 0;
            for (int64_t l = 1; l <= N && got < q; ++l)
                if (seen[(size_t)l] != (int)s + 1) freelab[(size_t)s * q + got++] = (int)l;
            logp[(size_t)s] = std::log(p[s0 + s]);
            log1mp[(size_t)s] = std::log(1 - p[s0 + s]);
        }
        DeviceBuffers C;
        int *d_free; double *d_r, *d_logp, *d_log1mp; ll2 *d_base;
        long long *d_labels, *d_first = nullptr, *d_Kout, *d_moves = nullptr, *d_sums = nullptr;
        HIPCHK(nullptr, O.upload(C));
        HIPCHK(nullptr, C.alloc(d_free, freelab.size()));
        HIPCHK(nullptr, C.alloc(d_r, (size_t)ms));
        HIPCHK(nullptr, C.alloc(d_logp, (size_t)ms));
        HIPCHK(nullptr, C.alloc(d_log1mp, (size_t)ms));
        HIPCHK(nullptr, C.alloc(d_base, (size_t)q * O.ktot));
        HIPCHK(nullptr, C.alloc(d_labels, (size_t)ms * q));
        HIPCHK(nullptr, C.alloc(d_Kout, (size_t)ms));
        if (first_out) HIPCHK(nullptr, C.alloc(d_first, (size_t)ms * q));
        if (moves_out) HIPCHK(nullptr, C.alloc(d_moves, (size_t)ms * nm));
        if (sums_out) HIPCHK(nullptr, C.alloc(d_sums, (size_t)ms * q * 2));
        HIPCHK(nullptr, hipMemcpy(d_free, freelab.data(), freelab.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_r, r + s0, (size_t)ms * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_logp, logp.data(), (size_t)ms * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_log1mp, log1mp.data(), (size_t)ms * sizeof(double), hipMemcpyHostToDevice));

        prdj::Args a{};
        a.q = (int)q; a.sweeps = sweeps; a.S = (int)Smax; a.ktot = O.ktot;
        a.base = d_base; a.rown = d_rown; a.koff = O.d_koff; a.K = O.d_K; a.szlab = O.d_szlab; a.freelab = d_free; a.A = d_A;
        a.r = d_r; a.logp = d_logp; a.log1mp = d_log1mp; a.scD = d_scD; a.scL = d_scL; a.flt = d_flt;
        const rc_params &P = *params;
        a.alpha = P.alpha; a.beta = P.beta; a.zeta = P.zeta; a.gamma = P.gamma; a.delta1 = P.delta1; a.delta2 = P.delta2;
        a.cL = (P.delta1 - 1.0) - (P.repulsion ? (P.delta2 - 1.0) : 0.0);
        a.repulsion = P.repulsion ? 1 : 0;
        a.maxK = P.maxK;
        a.k0 = (unsigned)seed; a.k1 = (unsigned)(seed >> 32) ^ prdj::TAG;
        a.sample0 = sample_offset + (uint64_t)s0;
        a.labels = d_labels; a.first = d_first; a.Kout = d_Kout; a.moves = d_moves; a.sums_out = d_sums;
        const size_t lds = prdj::lds_bytes(Smax, q);
        HIPCHK(nullptr, set_dynamic_lds(prdj::k_joint, lds));
        HIPCHK(nullptr, ev.begin(0));
        HIPCHK(nullptr, O.launch_sums(d_rowt, q, rows_global, d_base));
        prdj::k_joint<<<(unsigned)ms, prdj::TPB, lds, 0>>>(a);
        HIPCHK(nullptr, ev.end(0));
        HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
        HIPCHK(nullptr, hipMemcpy(labels_out + (size_t)s0 * q, d_labels, (size_t)ms * q * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCHK(nullptr, hipMemcpy(K_out + s0, d_Kout, (size_t)ms * sizeof(long long), hipMemcpyDeviceToHost));
        if (first_out) HIPCHK(nullptr, hipMemcpy(first_out + (size_t)s0 * q, d_first, (size_t)ms * q * sizeof(long long), hipMemcpyDeviceToHost));
        if (moves_out) HIPCHK(nullptr, hipMemcpy(moves_out + (size_t)s0 * nm, d_moves, (size_t)ms * nm * sizeof(long long), hipMemcpyDeviceToHost));
        if (sums_out) HIPCHK(nullptr, hipMemcpy(sums_out + (size_t)s0 * q * 2, d_sums, (size_t)ms * q * 2 * sizeof(long long), hipMemcpyDeviceToHost));
        s0 += ms;
    }
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

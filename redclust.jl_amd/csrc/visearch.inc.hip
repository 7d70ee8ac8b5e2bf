// The host side of the exact searches (rc_vi_search, rc_id_search, rc_vi_search_groups): the launch, the fixed-point table, the
// checks, the staging of the samples and the runs, the results.  The kernels and their arguments are visearch_kernel.inc.hip's,
// included in front of this file.  Same translation unit as redclust_hip.hip: shares fail(), HIPCHK, the error buffer; the
// holders, check_label_rows, check_lds_capacity and select_device of hostutil.inc.hip; and from greedy.inc.hip the shared
// argument checks, the staging of the runs and the result loop.

namespace visearch {

template <int LOSS, bool GROUPED = false>
static hipError_t launch(int PQ, int nruns, size_t lds, const Args &A)
{
#define VIS_LAUNCH(QQ)                                                                                                    \
    do {                                                                                                                  \
        void (*kernel)(Args) = GROUPED ? k_vigroups<QQ> : k_visearch<QQ, LOSS>;                                           \
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   \
        if (e != hipSuccess) return e;                                                                                    \
        kernel<<<nruns, TPB, lds, 0>>>(A);                                                                                \
    } while (0)
    if (PQ == 0) VIS_LAUNCH(0);
    else if (PQ == 1) VIS_LAUNCH(1);
    else VIS_LAUNCH(STAGE_Q);
#undef VIS_LAUNCH
    return hipGetLastError();
}

static void gtable(int64_t n, int64_t *out)
{
    out[0] = 0;
    for (int64_t x = 1; x < n; ++x) {
        const double d = (double)x;
        out[x] = (int64_t)std::llrint(std::ldexp(std::log(d + 1.0) + d * std::log1p(1.0 / d), 32));
    }
}

// the label-staging depth for the largest sample count any run of the launch sums over
static int stage_depth(int64_t m) { return m <= TPB ? 1 : (m <= (int64_t)TPB * STAGE_Q ? STAGE_Q : 0); }

// What run and run_groups do alike on the host: the tables Gq and Φq, one sample's relabelling, one run's staging, the upload
struct Host {
    const int64_t n;
    std::vector<int64_t> Gq, Phi;
    std::vector<int> map, cnt;

    explicit Host(int64_t n_) : n(n_), Gq((size_t)n_), Phi((size_t)n_ + 1), map((size_t)n_ + 1), cnt((size_t)n_ + 1)
    {
        gtable(n, Gq.data());
        Phi[0] = 0;
        for (int64_t x = 0; x < n; ++x) Phi[(size_t)x + 1] = Phi[(size_t)x] + Gq[(size_t)x];
    }
    // one sample (labels 1..n, checked) re-labelled to 0..L−1 by first appearance into out[j·stride]; returns Σ_l Φq(n^s_l)
    long long take_sample(const int64_t *sample, unsigned short *out, size_t stride, int &L)
    {
        std::fill(map.begin(), map.end(), 0);
        std::fill(cnt.begin(), cnt.end(), 0);
        L = 0;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t l = sample[j];
            if (!map[(size_t)l]) map[(size_t)l] = ++L;
            out[(size_t)j * stride] = (unsigned short)(map[(size_t)l] - 1);
            cnt[(size_t)map[(size_t)l]]++;
        }
        long long bq = 0;
        for (int l = 1; l <= L; ++l) bq += Phi[(size_t)cnt[(size_t)l]];
        return bq;
    }
    // run r into S: its labels in 0..n compacted to slots 1..K0 by first appearance (K0 <= Kcap), its order a permutation of
    // 1..n; Aq = Σ_k Φq(n_k) of the start
    int32_t take_run(greedy::Staging &S, const char *who, int r, const int64_t *init, const int32_t *order, int Kcap, long long &Aq)
    {
        int64_t row, at;
        if (find_bad_label(init + (size_t)r * n, 1, n, 0, &row, &at))
            return fail(nullptr, RC_ERR_ARG, "%s: label %lld of run %d outside 0..n", who, (long long)init[(size_t)r * n + at], r + 1);
        std::fill(map.begin(), map.end(), 0);
        int K = 0;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t l = init[(size_t)r * n + j];
            if (l && !map[(size_t)l]) map[(size_t)l] = ++K;
        }
        if (K > Kcap) return fail(nullptr, RC_ERR_ARG, "%s: run %d starts with %d clusters, more than the slot cap %d", who, r + 1, K, Kcap);
        unsigned short *szr = S.sz_row(r);
        for (int64_t j = 0; j < n; ++j) {
            const int slot = map[(size_t)init[(size_t)r * n + j]];      // map[0] = 0
            S.init_row(r)[j] = (unsigned short)slot;
            if (slot) szr[slot]++;
        }
        S.K[(size_t)r] = K;
        Aq = 0;
        for (int k = 1; k <= K; ++k) Aq += Phi[(size_t)szr[k]];
        return S.take_order(nullptr, who, r, order);
    }
    // the device copies of the tables, the transposed samples and the staged runs, and table_elems zeroed contingency cells, into A
    hipError_t upload(DeviceBuffers &B, greedy::Staging &S, const std::vector<unsigned short> &h_SL, size_t table_elems, Args &A)
    {
        long long *d_G = nullptr, *d_Phi = nullptr; unsigned short *d_SL = nullptr, *d_N = nullptr;
        hipError_t e = B.alloc(d_G, Gq.size());
        if (e == hipSuccess) e = B.alloc(d_Phi, Phi.size());
        if (e == hipSuccess) e = B.alloc(d_SL, h_SL.size());
        if (e == hipSuccess) e = B.alloc(d_N, table_elems);
        if (e == hipSuccess) e = hipMemcpy(d_G, Gq.data(), Gq.size() * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_Phi, Phi.data(), Phi.size() * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_SL, h_SL.data(), h_SL.size() * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(d_N, 0, table_elems * 2);
        if (e == hipSuccess) e = S.upload(B, 0, sizeof(RunOut));
        A.Gq = d_G; A.Phi = d_Phi; A.SL = d_SL; A.N = d_N; A.init = S.d_init; A.sz0 = S.d_sz; A.K0 = S.d_K; A.order = S.d_order;
        A.labels = S.d_labels; A.out = (RunOut *)S.d_out;
        return e;
    }
};

// The host side of rc_vi_search (loss = LOSS_VI) and rc_id_search (LOSS_ID): the same arguments, checks, staging and results
static int32_t run(int loss, const char *who, int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t nruns,
                   const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out_,
                   int32_t *best, double *kernel_ms)
{
    rc_psm_run_t *runs_out = (rc_psm_run_t *)runs_out_;
    if (!samples) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    int32_t rc = greedy::check_args(nullptr, who, m, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    // the capacity in n and m·n before anything is read
    rc = check_lds_capacity(nullptr, who, n);
    if (rc != RC_OK) return rc;
    if (m > MN_MAX / n) return fail(nullptr, RC_ERR_CAPACITY, "%s: m*n exceeds 2^26 = %lld (m=%lld n=%lld)", who, MN_MAX, (long long)m, (long long)n);

    // ---- the samples: labels 1..n, re-labelled per sample to 0..L_s-1 by first appearance, transposed to [i][s]
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    std::vector<unsigned short> h_SL((size_t)n * m);
    Host H(n);
    int Lmax = 0;
    __int128 constant = 0;                                              // Σ_s Σ_l Φq(n^s_l)
    std::vector<long long> Bs(loss == LOSS_ID ? (size_t)m : 0);         // ID: the same sum per sample (Bq_s)
    for (int64_t s = 0; s < m; ++s) {
        int L;
        const long long bq = H.take_sample(samples + (size_t)s * n, h_SL.data() + s, (size_t)m, L);
        constant += bq;
        if (loss == LOSS_ID) Bs[(size_t)s] = bq;
        Lmax = std::max(Lmax, L);
    }
    // ---- the slot cap: always positive
    const int64_t Kcap64 = std::min<int64_t>(maxK > 0 ? maxK : Lmax, n);
    if (Kcap64 > KCAP_MAX)
        return fail(nullptr, RC_ERR_CAPACITY, "%s: the slot cap %lld (maxK, or the largest cluster count among the samples) exceeds %d", who,
                    (long long)Kcap64, KCAP_MAX);
    const int Kcap = (int)Kcap64, kpad = (Kcap + VEC - 1) / VEC * VEC;
    const size_t table_elems = (size_t)m * Lmax * kpad;
    if ((double)table_elems * 2.0 * nruns > (double)TABLE_BUDGET)
        return fail(nullptr, RC_ERR_CAPACITY, "%s: the contingency tables (runs x m x Lmax x Kcap4 x 2 B = %d x %lld x %d x %d x 2, Kcap4 = the slot cap rounded up to 4) exceed the budget of %llu MiB",
                    who, nruns, (long long)m, Lmax, kpad, (unsigned long long)(TABLE_BUDGET >> 20));

    // ---- the runs: labels in 0..n compacted to slots 1..K0 by first appearance, orders permutations of 1..n
    greedy::Staging S(nruns, n, (size_t)Kcap + 2);
    std::vector<long long> h_Aq((size_t)nruns, 0);                      // ID: Σ_k Φq(n_k) of the start
    for (int r = 0; r < nruns; ++r) {
        rc = H.take_run(S, who, r, init, order, Kcap, h_Aq[(size_t)r]);  // (per run: an earlier run's other errors come first)
        if (rc != RC_OK) return rc;
    }

    rc = select_device(who, device);
    if (rc != RC_OK) return rc;

    DeviceBuffers B;
    Args A{};
    HIPCHK(nullptr, H.upload(B, S, h_SL, table_elems * (size_t)nruns, A));
    A.n = (int)n; A.m = (int)m; A.Lmax = Lmax; A.kpad = kpad; A.Kcap = Kcap; A.maxsweeps = maxsweeps;
    const int PQ = stage_depth(m);
    size_t lds = Carve((int)n, kpad, Kcap, PQ).total;
    if (loss == LOSS_ID) {
        // F's table: the Bq_s ascending and their prefix sums; in LDS behind Aq where that fits, else read from global memory
        std::sort(Bs.begin(), Bs.end());
        std::vector<long long> Pre((size_t)m + 1, 0);
        for (int64_t s = 0; s < m; ++s) Pre[(size_t)s + 1] = Pre[(size_t)s] + Bs[(size_t)s];
        long long *d_Bs, *d_Pre, *d_Aq;
        HIPCHK(nullptr, B.alloc(d_Bs, Bs.size()));
        HIPCHK(nullptr, B.alloc(d_Pre, Pre.size()));
        HIPCHK(nullptr, B.alloc(d_Aq, h_Aq.size()));
        HIPCHK(nullptr, hipMemcpy(d_Bs, Bs.data(), Bs.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_Pre, Pre.data(), Pre.size() * 8, hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_Aq, h_Aq.data(), h_Aq.size() * 8, hipMemcpyHostToDevice));
        A.Bs = d_Bs; A.Pre = d_Pre; A.Aq0 = d_Aq;
        while ((1ll << A.nbits) < m + 1) ++A.nbits;                     // p(x) is in 0..m
        const bool force_global = env_flag("RC_ID_TABLE_GLOBAL");       // tests: force the global-memory table at small m
        A.tab_lds = (!force_global && lds + 16 * ((size_t)m + 1) <= LDS_MAX) ? 1 : 0;
        lds += A.tab_lds ? 16 * ((size_t)m + 1) : 16;
    }
    HIPCHK(nullptr, S.begin(0));
    HIPCHK(nullptr, loss == LOSS_ID ? launch<LOSS_ID>(PQ, nruns, lds, A) : launch<LOSS_VI>(PQ, nruns, lds, A));
    std::vector<RunOut> h_out;
    HIPCHK(nullptr, S.collect(0, h_out, kernel_ms));

    // ---- results: the losses; the best run is the first of minimal Q
    const double scale = std::ldexp((double)n * (double)m, 32);
    greedy::results(S, h_out, labels_out, runs_out, best, [&](const RunOut &o, rc_psm_run_t &R, const int *, int) {
        R.loss_num = o.Q;
        R.loss = (double)((__int128)o.Q + (loss == LOSS_ID ? (__int128)0 : constant)) / scale;
        return R.loss_num;
    });
    return RC_OK;
}

// The host side of rc_vi_search_groups: run's checks, per group where run's are per call, one staging, one upload and one launch
// of the grouped instantiation.  Run r is rc_vi_search's run on samples[group == run_group[r]].
static int32_t run_groups(int32_t device, const int64_t *samples, int64_t m, int64_t n, const int32_t *group, int32_t ngroups, int32_t nruns,
                          const int32_t *run_group, const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps,
                          int64_t *labels_out, void *runs_out_, int32_t *best, double *kernel_ms)
{
    const char *who = "rc_vi_search_groups";
    rc_psm_run_t *runs_out = (rc_psm_run_t *)runs_out_;
    if (!samples || !group || !run_group) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    int32_t rc = greedy::check_args(nullptr, who, m, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    if (ngroups < 1) return fail(nullptr, RC_ERR_ARG, "%s: need ngroups >= 1 (got %d)", who, ngroups);
    // the capacity in n and m·n before anything is read
    rc = check_lds_capacity(nullptr, who, n, m);
    if (rc != RC_OK) return rc;

    // ---- the groups: their sizes, and where each sample goes in its group's block
    std::vector<int64_t> mg((size_t)ngroups, 0), first((size_t)ngroups + 1, 0);   // first[g]: the samples in groups below g
    std::vector<int64_t> at((size_t)m);                                           // a sample's index within its group
    for (int64_t s = 0; s < m; ++s) {
        const int32_t g = group[(size_t)s];
        if (g < -1 || g >= ngroups) return fail(nullptr, RC_ERR_ARG, "%s: group %d of sample %lld outside -1..ngroups-1", who, g, (long long)s + 1);
        if (g >= 0) at[(size_t)s] = mg[(size_t)g]++;
    }
    std::vector<char> searched((size_t)ngroups, 0);
    for (int r = 0; r < nruns; ++r) {
        const int32_t g = run_group[r];
        if (g < 0 || g >= ngroups) return fail(nullptr, RC_ERR_ARG, "%s: group %d of run %d outside 0..ngroups-1", who, g, r + 1);
        if (!mg[(size_t)g]) return fail(nullptr, RC_ERR_ARG, "%s: run %d searches group %d, which has no samples", who, r + 1, g);
        searched[(size_t)g] = 1;
    }
    for (int g = 0; g < ngroups; ++g) {
        if (mg[(size_t)g] > MN_MAX / n)
            return fail(nullptr, RC_ERR_CAPACITY, "%s: m*n of group %d exceeds 2^26 = %lld (m=%lld n=%lld)", who, g, MN_MAX, (long long)mg[(size_t)g], (long long)n);
        first[(size_t)g + 1] = first[(size_t)g] + mg[(size_t)g];
    }

    // ---- the samples, group by group: block g is n × m_g, a sample's labels as in run
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    std::vector<unsigned short> h_SL((size_t)n * (size_t)std::max<int64_t>(first[(size_t)ngroups], 1));
    Host H(n);
    std::vector<int> Lmax((size_t)ngroups, 0);
    std::vector<__int128> constant((size_t)ngroups, 0);                           // Σ_s Σ_l Φq(n^s_l) over the group
    for (int64_t s = 0; s < m; ++s) {
        const int32_t g = group[(size_t)s];
        if (g < 0) continue;
        int L;
        constant[(size_t)g] += H.take_sample(samples + (size_t)s * n, h_SL.data() + (size_t)n * first[(size_t)g] + at[(size_t)s], (size_t)mg[(size_t)g], L);
        Lmax[(size_t)g] = std::max(Lmax[(size_t)g], L);
    }
    // ---- the slot caps of the groups that are searched, always positive; the launch's geometry from the largest
    std::vector<int> Kcap((size_t)ngroups, 0);
    int Kcap_max = 0, Lmax_max = 0;
    int64_t m_max = 0;
    for (int g = 0; g < ngroups; ++g) {
        if (!searched[(size_t)g]) continue;
        const int64_t K64 = std::min<int64_t>(maxK > 0 ? maxK : Lmax[(size_t)g], n);
        if (K64 > KCAP_MAX)
            return fail(nullptr, RC_ERR_CAPACITY, "%s: the slot cap %lld of group %d (maxK, or the largest cluster count among its samples) exceeds %d", who,
                        (long long)K64, g, KCAP_MAX);
        Kcap[(size_t)g] = (int)K64;
        Kcap_max = std::max(Kcap_max, (int)K64);
        Lmax_max = std::max(Lmax_max, Lmax[(size_t)g]);
        m_max = std::max(m_max, mg[(size_t)g]);
    }
    const int kpad = (Kcap_max + VEC - 1) / VEC * VEC;
    std::vector<GroupRun> h_runs((size_t)nruns);
    double table_elems = 0.0;                                                     // every term < 2^26 · 1024: exact in f64
    for (int r = 0; r < nruns; ++r) {
        const size_t g = (size_t)run_group[r];
        GroupRun &gr = h_runs[(size_t)r];
        gr.sl = (unsigned long long)n * (unsigned long long)first[g];
        gr.tab = (unsigned long long)table_elems;
        gr.m = (int)mg[g]; gr.Lmax = Lmax[g]; gr.Kcap = Kcap[g]; gr.pad_ = 0;
        table_elems += (double)mg[g] * Lmax[g] * kpad;
        if (table_elems * 2.0 > (double)TABLE_BUDGET)
            return fail(nullptr, RC_ERR_CAPACITY, "%s: the contingency tables (2 B x Kcap4 x the sum over the runs of m_g x Lmax_g; Kcap4 = %d, the largest slot cap rounded up to 4) exceed the budget of %llu MiB at run %d",
                        who, kpad, (unsigned long long)(TABLE_BUDGET >> 20), r + 1);
    }

    // ---- the runs, each against its own group's cap
    greedy::Staging S(nruns, n, (size_t)Kcap_max + 2);
    for (int r = 0; r < nruns; ++r) {
        long long Aq;
        rc = H.take_run(S, who, r, init, order, h_runs[(size_t)r].Kcap, Aq);
        if (rc != RC_OK) return rc;
    }

    rc = select_device(who, device);
    if (rc != RC_OK) return rc;

    DeviceBuffers B;
    Args A{};
    HIPCHK(nullptr, H.upload(B, S, h_SL, (size_t)table_elems, A));
    GroupRun *d_runs;
    HIPCHK(nullptr, B.alloc(d_runs, h_runs.size()));
    HIPCHK(nullptr, hipMemcpy(d_runs, h_runs.data(), h_runs.size() * sizeof(GroupRun), hipMemcpyHostToDevice));
    A.runs = d_runs;
    A.n = (int)n; A.m = (int)m_max; A.Lmax = Lmax_max; A.kpad = kpad; A.Kcap = Kcap_max; A.maxsweeps = maxsweeps;
    const int PQ = stage_depth(m_max);
    const size_t lds = Carve((int)n, kpad, Kcap_max, PQ).total;
    HIPCHK(nullptr, S.begin(0));
    HIPCHK(nullptr, (launch<LOSS_VI, true>(PQ, nruns, lds, A)));
    std::vector<RunOut> h_out;
    HIPCHK(nullptr, S.collect(0, h_out, kernel_ms));

    // ---- results: a run's loss with its group's constant and m; per group the first run of minimal Q
    int32_t any;
    greedy::results(S, h_out, labels_out, runs_out, &any, [&](const RunOut &o, rc_psm_run_t &R, const int *, int) {
        const size_t g = (size_t)run_group[&R - runs_out];
        R.loss_num = o.Q;
        R.loss = (double)((__int128)o.Q + constant[g]) / std::ldexp((double)n * (double)mg[g], 32);
        return R.loss_num;
    });
    std::fill(best, best + ngroups, -1);
    for (int r = 0; r < nruns; ++r) {
        int32_t &b = best[run_group[r]];
        if (b < 0 || runs_out[r].loss_num < runs_out[b].loss_num) b = r;
    }
    return RC_OK;
}

}  // namespace visearch

extern "C" int32_t rc_vi_search_groups(int32_t device, const int64_t *samples, int64_t m, int64_t n, const int32_t *group, int32_t ngroups,
                                       int32_t nruns, const int32_t *run_group, const int64_t *init, const int32_t *order, int32_t maxK,
                                       int32_t maxsweeps, int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms)
{
    return visearch::run_groups(device, samples, m, n, group, ngroups, nruns, run_group, init, order, maxK, maxsweeps, labels_out, runs_out,
                                best, kernel_ms);
}

extern "C" int32_t rc_vi_gtable(int64_t n, int64_t *out)
{
    if (!out) return fail(nullptr, RC_ERR_ARG, "rc_vi_gtable: NULL argument");
    if (n < 1) return fail(nullptr, RC_ERR_ARG, "rc_vi_gtable: need n >= 1 (got %lld)", (long long)n);
    visearch::gtable(n, out);
    return RC_OK;
}

extern "C" int32_t rc_vi_search(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t nruns, const int64_t *init,
                                const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                int32_t *best, double *kernel_ms)
{
    return visearch::run(visearch::LOSS_VI, "rc_vi_search", device, samples, m, n, nruns, init, order, maxK, maxsweeps, labels_out,
                         runs_out, best, kernel_ms);
}

extern "C" int32_t rc_id_search(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t nruns, const int64_t *init,
                                const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                int32_t *best, double *kernel_ms)
{
    return visearch::run(visearch::LOSS_ID, "rc_id_search", device, samples, m, n, nruns, init, order, maxK, maxsweeps, labels_out,
                         runs_out, best, kernel_ms);
}

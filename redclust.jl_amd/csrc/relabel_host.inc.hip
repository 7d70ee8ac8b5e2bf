// The host side that rc_relabel (relabel.inc.hip) and rc_relabel_wide (relabel_wide.inc.hip) share.  Included from
// redclust_hip.hip before both: each gives run() its cluster cap and its launcher.

namespace relabel {

constexpr int64_t NMAX = 32767;                 // a cell of the table fits 15 bits
constexpr size_t WORKSPACE = (size_t)1 << 30;   // device bytes of one chunk of samples

// What a chunk's launch is given: the device arrays of the chunk (ms samples) and the host's cluster counts of its samples.
struct Chunk {
    const unsigned short *piv, *zid;
    const int *Ks, *names;
    long long *labels, *maps, *overlap;
    unsigned *counts;
    const int *h_Ks;                // host: [ms]
    int n, ms, Kp, W;
};

// The host side of rc_relabel and rc_relabel_wide: the checks, the dense ids, the chunks over the workspace, the copies and the
// timing.  kmax: the clusters a pivot or a sample may have; L: prepare() once and launch() per chunk
// (relabel::Launch, relabel_wide::Launch).
template <typename L>
static int32_t run(const char *who, int kmax, L &&launcher, int32_t device, const int64_t *samples, int64_t m, int64_t n, const int64_t *pivot,
                   int64_t Kp_in, int64_t *labels_out, int64_t *maps_out, int64_t maps_width, int64_t *overlap_out, void *counts_out,
                   double *kernel_ms)
{
    if (!samples || !pivot || !overlap_out || !counts_out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (m < 1 || n < 1) return fail(nullptr, RC_ERR_ARG, "%s: need m >= 1 and n >= 1 (got m=%lld n=%lld)", who, (long long)m, (long long)n);
    if (n > NMAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %lld points whose counts fit 15 bits", who, (long long)n, (long long)NMAX);
    if (m >= ((int64_t)1 << 31)) return fail(nullptr, RC_ERR_CAPACITY, "%s: m = %lld is not below 2^31", who, (long long)m);
    int32_t rc = check_label_rows(nullptr, who, "pivot", pivot, 1, n);
    if (rc != RC_OK) return rc;
    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;

    std::vector<int> cnt, id, Ks, names;
    std::vector<unsigned short> h_piv;
    try {
        cnt.assign((size_t)n + 1, 0); id.assign((size_t)n + 1, 0); Ks.resize((size_t)m); h_piv.resize((size_t)n);
    } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory", who); }
    const auto no_slot = [](int, int64_t, int) {};                    // only the ids and the cluster counts are wanted here
    const int64_t Kp = compact_labels(pivot, n, cnt, id, no_slot);
    dense_ids(pivot, n, id, h_piv.data());
    if (Kp > kmax) return fail(nullptr, RC_ERR_CAPACITY, "%s: the pivot has %lld clusters, more than %d", who, (long long)Kp, kmax);
    names.assign((size_t)Kp, 0);
    for (int64_t j = 0; j < n; ++j) names[h_piv[(size_t)j]] = (int)pivot[j];
    const size_t workspace = env_workspace_kib("RC_RELABEL_WORKSPACE_KIB", WORKSPACE);
    // The samples are compacted here for their cluster counts, which the capacity checks need before any device work.  Their
    // dense ids are kept for the chunks when all of them fit a workspace's worth of host memory, else made again per chunk.
    const bool keep_ids = 2 * (size_t)m * (size_t)n <= workspace;
    std::vector<unsigned short> h_zid;
    if (keep_ids) {
        try { h_zid.resize((size_t)m * n); } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for the ids of %lld samples", who, (long long)m); }
    }
    int64_t W = 0;
    for (int64_t s = 0; s < m; ++s) {
        const int K = compact_labels(samples + (size_t)s * n, n, cnt, id, no_slot);
        if (keep_ids) dense_ids(samples + (size_t)s * n, n, id, h_zid.data() + (size_t)s * n);
        if (K > kmax) return fail(nullptr, RC_ERR_CAPACITY, "%s: sample %lld has %lld clusters, more than %d", who, (long long)s + 1, (long long)K, kmax);
        Ks[(size_t)s] = K;
        W = std::max<int64_t>(W, K);
    }
    if (Kp_in != Kp) return fail(nullptr, RC_ERR_ARG, "%s: the pivot has %lld clusters, not %lld (counts is n x (K_p + 1))", who, (long long)Kp, (long long)Kp_in);
    if (maps_out && maps_width < W) return fail(nullptr, RC_ERR_ARG, "%s: maps is %lld wide, the largest sample has %lld clusters", who, (long long)maps_width, (long long)W);
    if (kernel_ms) *kernel_ms = 0.0;

    rc = select_device(who, device);
    if (rc != RC_OK) return rc;
    const int64_t Wd = maps_out ? maps_width : 0;
    const size_t per_sample = 2 * (size_t)n + sizeof(int) + sizeof(long long) + (labels_out ? 8 * (size_t)n : 0) + 8 * (size_t)Wd;
    const int64_t mc = std::max<int64_t>(1, std::min<int64_t>(m, (int64_t)(workspace / per_sample)));
    launcher.prepare(n, (int)Kp, Ks, mc, workspace);
    if (!keep_ids) {
        try { h_zid.resize((size_t)mc * n); } catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for a chunk of %lld samples", who, (long long)mc); }
    }

    DeviceBuffers B;
    unsigned short *d_piv, *d_zid; int *d_Ks, *d_names; unsigned *d_counts;
    long long *d_labels = nullptr, *d_maps = nullptr, *d_overlap;
    const size_t ncounts = (size_t)n * (size_t)(Kp + 1);
    HIPCHK(nullptr, B.alloc(d_piv, (size_t)n));
    HIPCHK(nullptr, B.alloc(d_names, (size_t)Kp));
    HIPCHK(nullptr, B.alloc(d_counts, ncounts));
    HIPCHK(nullptr, B.alloc(d_zid, (size_t)mc * n));
    HIPCHK(nullptr, B.alloc(d_Ks, (size_t)mc));
    HIPCHK(nullptr, B.alloc(d_overlap, (size_t)mc));
    if (labels_out) HIPCHK(nullptr, B.alloc(d_labels, (size_t)mc * n));
    if (maps_out) HIPCHK(nullptr, B.alloc(d_maps, (size_t)mc * Wd));
    HIPCHK(nullptr, hipMemcpy(d_piv, h_piv.data(), (size_t)n * sizeof(unsigned short), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_names, names.data(), (size_t)Kp * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemset(d_counts, 0, ncounts * sizeof(unsigned)));
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());

    double ms_acc = 0.0;
    for (int64_t s0 = 0; s0 < m; s0 += mc) {
        const int64_t ms = std::min(mc, m - s0);
        for (int64_t s = 0; s < ms && !keep_ids; ++s) {
            compact_labels(samples + (size_t)(s0 + s) * n, n, cnt, id, no_slot);
            dense_ids(samples + (size_t)(s0 + s) * n, n, id, h_zid.data() + (size_t)s * n);
        }
        HIPCHK(nullptr, hipMemcpy(d_zid, h_zid.data() + (keep_ids ? (size_t)s0 * n : 0), (size_t)ms * n * sizeof(unsigned short), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(d_Ks, Ks.data() + s0, (size_t)ms * sizeof(int), hipMemcpyHostToDevice));
        Chunk c{};
        c.piv = d_piv; c.zid = d_zid; c.Ks = d_Ks; c.names = d_names; c.labels = d_labels; c.maps = d_maps; c.overlap = d_overlap;
        c.counts = d_counts; c.h_Ks = Ks.data() + s0; c.n = (int)n; c.ms = (int)ms; c.Kp = (int)Kp; c.W = (int)Wd;
        rc = launcher.launch(B, ev, c);
        if (rc != RC_OK) return rc;
        HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
        HIPCHK(nullptr, hipMemcpy(overlap_out + s0, d_overlap, (size_t)ms * sizeof(long long), hipMemcpyDeviceToHost));
        if (labels_out) HIPCHK(nullptr, hipMemcpy(labels_out + (size_t)s0 * n, d_labels, (size_t)ms * n * sizeof(long long), hipMemcpyDeviceToHost));
        if (maps_out) HIPCHK(nullptr, hipMemcpy(maps_out + (size_t)s0 * Wd, d_maps, (size_t)ms * Wd * sizeof(long long), hipMemcpyDeviceToHost));
    }
    HIPCHK(nullptr, hipMemcpy(counts_out, d_counts, ncounts * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

}  // namespace relabel

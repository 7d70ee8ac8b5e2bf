// The entry points that hand a metric to the kernels of metric.inc.hip and predictpoints.inc.hip without a prediction behind
// them: rc_pairwise (the raw distances) and rc_create_from_points_metric (a context whose D is in the metric).  Included at
// the end of redclust_hip.hip after predictpoints.inc.hip (same translation unit).  Contract: include/redclust_hip.h.

extern "C" int32_t rc_pairwise(int32_t device, int32_t metric, int64_t n, int64_t dim, const double *points, int64_t q, const double *new_points,
                               double *out, double *kernel_ms)
{
    const char *who = "rc_pairwise";
    if (!points || !out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (n < 1 || n > ((int64_t)1 << 24)) return fail(nullptr, RC_ERR_ARG, "%s: n = %lld outside 1..2^24", who, (long long)n);
    if (new_points && q < 1) return fail(nullptr, RC_ERR_ARG, "%s: need q >= 1 with new points (got %lld)", who, (long long)q);
    if (dim < 1 || dim > pp::DIM_MAX) return fail(nullptr, RC_ERR_ARG, "%s: dim = %lld outside 1..%lld", who, (long long)dim, (long long)pp::DIM_MAX);
    int32_t rc = met::check_metric(nullptr, who, metric, dim);
    if (rc != RC_OK) return rc;
    rc = pp::check_finite(who, points, n, new_points, q, dim);
    if (rc != RC_OK) return rc;
    rc = select_device(who, device);
    if (rc != RC_OK) return rc;
    DeviceBuffers B;
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());
    double ms_acc = 0.0;
    if (!new_points) {
        double *d_X, *d_D, *d_nrm = nullptr;
        HIPCHK(nullptr, B.alloc(d_D, (size_t)n * (size_t)n));
        HIPCHK(nullptr, B.alloc(d_X, (size_t)n * (size_t)dim));
        if (met::angular(metric)) HIPCHK(nullptr, B.alloc(d_nrm, (size_t)n));
        HIPCHK(nullptr, hipMemcpy(d_X, points, (size_t)n * (size_t)dim * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, ev.begin(0));
        met::launch_prep(metric, d_X, n, dim, d_nrm, 0);
        met::launch_pairwise(metric, d_X, d_nrm, n, dim, d_D, 0);
        HIPCHK(nullptr, ev.end(0));
        HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
        HIPCHK(nullptr, hipMemcpy(out, d_D, (size_t)n * (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        double *d_XT, *d_nX, *d_Y, *d_dist, *d_nY = nullptr;
        u64 *d_maxd, *d_firstbad;                   // the kernel's fold of the row maxima and its bad-pair word: written, never read here
        rc = pp::stage_training(metric, points, n, dim, B, d_XT, d_nX);
        if (rc != RC_OK) return rc;
        // a new point costs its row of distances, its coordinates and two words
        const size_t workspace = env_workspace_kib("RC_PREDICT_WORKSPACE_KIB", slab::WORKSPACE);
        int64_t qc = (int64_t)std::min<size_t>((size_t)q, std::max<size_t>(1, workspace / (8 * ((size_t)n + (size_t)dim + 2))));
        if (qc > pp::R) qc -= qc % pp::R;
        qc = std::min<int64_t>(qc, (int64_t)65535 * pp::R);
        HIPCHK(nullptr, B.alloc(d_Y, (size_t)qc * (size_t)dim));
        HIPCHK(nullptr, B.alloc(d_dist, (size_t)qc * (size_t)n));
        HIPCHK(nullptr, B.alloc(d_maxd, (size_t)qc));
        HIPCHK(nullptr, B.alloc(d_firstbad, 1));
        if (met::angular(metric)) HIPCHK(nullptr, B.alloc(d_nY, (size_t)qc));
        for (int64_t i0 = 0; i0 < q; i0 += qc) {
            const int64_t np = std::min(qc, q - i0);
            HIPCHK(nullptr, hipMemcpy(d_Y, new_points + (size_t)i0 * dim, (size_t)np * dim * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(nullptr, hipMemsetAsync(d_maxd, 0, (size_t)np * sizeof(u64), 0));
            HIPCHK(nullptr, hipMemsetAsync(d_firstbad, 0xFF, sizeof(u64), 0));
            HIPCHK(nullptr, ev.begin(0));
            met::launch_prep(metric, d_Y, np, dim, d_nY, 0);
            pp::launch_dist(metric, d_XT, n, dim, d_Y, np, 0, d_dist, d_maxd, d_firstbad, d_nX, d_nY);
            HIPCHK(nullptr, ev.end(0));
            HIPCHK(nullptr, ev.elapsed_ms(ms_acc));
            HIPCHK(nullptr, hipMemcpy(out + (size_t)i0 * n, d_dist, (size_t)np * n * sizeof(double), hipMemcpyDeviceToHost));
        }
    }
    if (kernel_ms) *kernel_ms = ms_acc;
    return RC_OK;
}

extern "C" int32_t rc_create_from_points_metric(int64_t n, int64_t dim, const double *points, int32_t metric, int32_t storage_bits,
                                                int32_t device_id, int64_t kcap, rc_ctx **out)
{
    const char *who = "rc_create_from_points_metric";
    if (!out) return fail(nullptr, RC_ERR_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!points) return fail(nullptr, RC_ERR_ARG, "%s: points is NULL", who);
    if (dim < 1 || dim > (1 << 20)) return fail(nullptr, RC_ERR_ARG, "%s: dim must be in 1..2^20", who);
    int32_t rc = met::check_metric(nullptr, who, metric, dim);
    if (rc != RC_OK) return rc;
    if (n >= 1) rc = pp::check_finite(who, points, n, nullptr, 0, dim);     // max(acc, |t|) would swallow a NaN; n < 1 is alloc_ctx's error
    if (rc != RC_OK) return rc;
    rc_ctx *c = nullptr;
    rc = alloc_ctx(n, storage_bits, device_id, kcap, &c);
    if (rc != RC_OK) return rc;
    rc = create_impl(c, n, nullptr, nullptr, points, dim, metric);
    if (rc == RC_OK) rc = finish_create(c);
    if (rc != RC_OK) {
        snprintf(g_err, sizeof(g_err), "%s", c->err);
        if (c->registered) { res_unregister(c); c->registered = false; }
        free_all(c);
        return rc;
    }
    *out = c;
    return RC_OK;
}

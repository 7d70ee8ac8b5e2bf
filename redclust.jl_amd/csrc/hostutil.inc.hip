// Host utilities of the entry points that own their device memory for one call (most of them take a device number and no
// context): a holder of device buffers, a pair of timing events, the checks of a label matrix, of its shape and of its rows' r
// and p, the tests' environment switches, the dynamic-LDS attribute, the device selection; and what the consumers of a
// co-clustering count matrix share: the n that fits a workgroup's LDS, the capacity check and the device check of the matrix (k_check_counts, check_counts) — how the matrix
// gets onto the device is cnt:: in samplecounts.inc.hip, not here.  Included at the end of redclust_hip.hip after
// labels.inc.hpp and before every other include (same translation unit: shares fail() and HIPCHK — HIPCHK(nullptr, call)
// reports into the thread's error buffer).  Both holders release on scope exit, so a HIPCHK may return from anywhere.

struct DeviceBuffers {
    std::vector<void *> owned;
    DeviceBuffers() = default;
    DeviceBuffers(const DeviceBuffers &) = delete;
    ~DeviceBuffers() { for (void *q : owned) (void)hipFree(q); }
    // count elements of T into out (null on failure)
    template <typename T> hipError_t alloc(T *&out, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e == hipSuccess) owned.push_back(q);
        out = (T *)q;
        return e;
    }
};

struct TimingEvents {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    TimingEvents() = default;
    TimingEvents(const TimingEvents &) = delete;
    ~TimingEvents()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    hipError_t create()
    {
        const hipError_t e = hipEventCreate(&e0);
        return e == hipSuccess ? hipEventCreate(&e1) : e;
    }
    // begin(st); the launches; end(st): the launches' error, else e1 behind them; elapsed_ms(acc): wait for e1, add e0 → e1 to acc
    hipError_t begin(hipStream_t st) { return hipEventRecord(e0, st); }
    hipError_t end(hipStream_t st)
    {
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? hipEventRecord(e1, st) : e;
    }
    hipError_t elapsed_ms(double &acc)
    {
        float t = 0;
        hipError_t e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        if (e == hipSuccess) acc += t;
        return e;
    }
};

// The library's error for the first label of `count` rows (each `what`, e.g. "sample") outside 1..n (labels.inc.hpp finds it)
static int32_t check_label_rows(rc_ctx *c, const char *who, const char *what, const int64_t *rows, int64_t count, int64_t n)
{
    int64_t r, j;
    if (!find_bad_label(rows, count, n, 1, &r, &j)) return RC_OK;
    return fail(c, RC_ERR_ARG, "%s: label %lld of %s %lld at position %lld outside 1..n", who, (long long)rows[(size_t)r * n + j], what,
                (long long)r + 1, (long long)j + 1);
}

// The shape of a matrix of label rows whose point indices are kept in u16 with bit 15 free for a mark and whose entries are
// indexed in 31 bits: n <= INDEX15_NMAX and rows·n < 2^31.  points: what the n are in the message ("points", "training
// points"); sym: the letter the rows go by there ("m", "L").
constexpr int64_t INDEX15_NMAX = 32767;
static int32_t check_label_shape(rc_ctx *c, const char *who, int64_t n, const char *points, int64_t rows, const char *sym)
{
    if (n > INDEX15_NMAX) return fail(c, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %lld %s whose indices fit 15 bits", who, (long long)n, (long long)INDEX15_NMAX, points);
    if (rows >= ((int64_t)1 << 31) / n + (((int64_t)1 << 31) % n != 0)) return fail(c, RC_ERR_CAPACITY, "%s: %s·n = %lld·%lld is not below 2^31", who, sym, (long long)rows, (long long)n);
    return RC_OK;
}

// r positive and finite (normal: and no subnormal) and p in (0, 1) for each of `count` rows (each `what`); a null r or p passes
static int32_t check_r_p(rc_ctx *c, const char *who, const char *what, int64_t count, const double *r, const double *p, bool normal = false)
{
    for (int64_t s = 0; s < count; ++s) {
        if (r && !(r[s] <= 1.79769313486231570e308 && (normal ? r[s] >= 2.2250738585072014e-308 : r[s] > 0)))
            return fail(c, RC_ERR_ARG, "%s: r of %s %lld must be %s", who, what, (long long)s + 1, normal ? "a positive, normal and finite number" : "positive and finite");
        if (p && !(p[s] > 0 && p[s] < 1)) return fail(c, RC_ERR_ARG, "%s: p of %s %lld must lie in (0, 1)", who, what, (long long)s + 1);
    }
    return RC_OK;
}

// The switches the tests set in the environment, read per call: an integer (0 when unset), a flag, and a workspace in KiB that
// shrinks the default (chunks at small shapes, the same results) and never exceeds it.
static long long env_int(const char *name)
{
    const char *e = std::getenv(name);
    return e ? atoll(e) : 0;
}
static bool env_flag(const char *name) { return env_int(name) != 0; }
static size_t env_workspace_kib(const char *name, size_t default_bytes)
{
    const long long v = env_int(name);
    return v > 0 ? std::min(default_bytes, (size_t)v << 10) : default_bytes;
}

// kernels that use more dynamic LDS than the 64 KiB every kernel may have must ask for it before the launch
template <typename Kernel> static hipError_t set_dynamic_lds(Kernel kernel, size_t bytes)
{
    return bytes > 64 * 1024 ? hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) : hipSuccess;
}

static int32_t select_device(const char *who, int32_t device)
{
    int ndev = 0;
    HIPCHK(nullptr, hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(nullptr, RC_ERR_ARG, "%s: device %d not available (%d visible)", who, device, ndev);
    HIPCHK(nullptr, hipSetDevice(device));
    return RC_OK;
}

// ---- what the consumers of a co-clustering count matrix share (the searches, hclust, the expected loss)

// One workgroup keeps a state per point in LDS (the searches of greedy.inc.hip, hclust), and where that state holds sums of
// a row of counts (m >= 1 given) they are kept in 32 bits: RC_ERR_CAPACITY beyond (n >= 1)
constexpr int LDS_NMAX = 8192;
static int32_t check_lds_capacity(rc_ctx *c, const char *who, int64_t n, int64_t m = 0)
{
    if (n > LDS_NMAX) return fail(c, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %d points whose state fits the workgroup's LDS", who, (long long)n, LDS_NMAX);
    if (m > 0x7FFFFFFFll / n) return fail(c, RC_ERR_CAPACITY, "%s: m*n does not fit 31 bits (m=%lld n=%lld)", who, (long long)m, (long long)n);
    return RC_OK;
}

// counts must be symmetric with diagonal m and no entry above m; flag bits: 1 diagonal, 2 symmetry, 4 range
__global__ __launch_bounds__(256) void k_check_counts(const unsigned *__restrict__ C, long long ld, int n, unsigned m, unsigned *flag)
{
    const int i = blockIdx.y;
    unsigned bad = 0;
    for (int j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
        const unsigned v = C[(size_t)i * ld + j];
        if (j == i) { if (v != m) bad |= 1u; }
        else if (j > i && v != C[(size_t)j * ld + i]) bad |= 2u;
        if (v > m) bad |= 4u;
    }
    if (bad) atomicOr(flag, bad);
}

// k_check_counts on the device counts (n × ld), with its flags turned into RC_ERR_ARG messages that start with `who`
static int32_t check_counts(rc_ctx *c, hipStream_t st, const char *who, const unsigned *dC, int64_t ld, int64_t m, int64_t n)
{
    DeviceBuffers B;
    unsigned *d_flag;
    HIPCHK(c, B.alloc(d_flag, 1));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
    k_check_counts<<<dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8), (unsigned)n), 256, 0, st>>>(dC, ld, (int)n, (unsigned)m, d_flag);
    HIPCHK(c, hipGetLastError());
    unsigned flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (flag & 1u) return fail(c, RC_ERR_ARG, "%s: the diagonal of the counts is not m = %lld everywhere", who, (long long)m);
    if (flag & 2u) return fail(c, RC_ERR_ARG, "%s: the counts are not symmetric", who);
    if (flag & 4u) return fail(c, RC_ERR_ARG, "%s: a count exceeds m = %lld", who, (long long)m);
    return RC_OK;
}

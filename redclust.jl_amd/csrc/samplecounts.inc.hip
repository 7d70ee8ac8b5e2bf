// Co-clustering counts from samples on the device: counts[i][j] = #{s : samples[s][i] == samples[s][j]} for an m×n label
// matrix that is already there — a stored MCMCResult, several merged chains, another sampler's draws — without the matrix
// ever reaching the host.  A live chain builds the same counts as it goes
// (k_snapshot / k_cocluster_batch, 32 samples per read-modify-write pass over the matrix); here all m samples are present, so
// every count is computed once from zero in registers and stored once.  DESIGN.md §8 "Counts from samples".
// Below the kernel, cnt:: — the one place where the counts of a consumer (the search, the dendrogram, the expected loss) reach
// the device, whichever of the three forms the caller has them in: cnt::acquire owns the staging of a host matrix, the call of
// sc::build for a consumer, and the flush-and-check sequence of a live context; cnt::with is the order of checks of all
// eight entry points.  DESIGN.md §8 "One counts source".
// Included at the end of redclust_hip.hip ahead of its consumers pointsearch.inc.hip and hclust.inc.hip (same translation
// unit: shares fail(), HIPCHK, rc_ctx, flush_counts, sync_and_check; the holders, check_label_rows and select_device of
// hostutil.inc.hip).
//
// Geometry.  The matrix is cut into TI × TJ = 128 × 128 tiles; a 256-thread workgroup computes one tile on or above the
// diagonal and stores it to both triangles.  A thread owns 8 × 8 counts (64 u32 registers): rows h·64 + ty·4 + 0..3 and columns
// g·64 + tx·4 + 0..3 (h, g = 0, 1).  A wave is an 8 (ty) × 8 (tx) patch of threads, so a store instruction of the tile as
// computed writes, for each of 8 rows, 8 lanes × 16 B = one whole 128-byte line, and so does a store instruction of the
// mirrored tile (there the 8 lanes of a line differ in ty): neither triangle is a strided scatter and nothing is transposed
// through LDS.
// Labels are u16, sample-major with leading dimension ldn (n rounded up to a multiple of TJ), padded with 0xFFFE.  Per
// sample a thread reads its 8 column labels from that array (two 8-byte loads, 64 contiguous bytes per row of the patch) and its
// 8 row labels from LDS, where the tile's row labels are staged SC = 32 samples at a time (8 KiB) with rows beyond n set to
// 0xFFFF: a pad never equals a label (<= 32767) and a row pad never equals a column pad, so pad entries count zero — which is
// what the columns n..ld-1 of the matrix must hold for the search.

namespace sc {

constexpr int TI = 128, TJ = 128;     // tile
constexpr int SC = 32;                // samples per staged chunk of row labels
constexpr int TPB = 256;
constexpr int64_t NMAX = 32767;       // the chain's limit: u16 values above it are free for the two pads
constexpr unsigned PAD_COL = 0xFFFEu;

// a staged row pad is the column pad with its lowest bit set (0xFFFF), in both halves of a packed pair
__device__ inline unsigned row_pads(unsigned x)
{
    return x | ((x & 0xFFFFu) == PAD_COL ? 1u : 0u) | ((x >> 16) == PAD_COL ? 0x10000u : 0u);
}

// One row of the thread's 8 × 8 patch for one sample: acc[R][c] += (row label == column label c).  The labels stay packed two
// per register and are compared as 16-bit halves (SDWA); a comparison's mask goes to its own SGPR pair and is added as a carry.
// gfx950 needs two wait states between a vector instruction that writes an SGPR and one that reads it: eight comparisons,
// then the eight additions, keeps seven instructions between each pair, where the compiler left alone alternates them and
// pads every pair with s_nop.
#define SC_ROW(R, ROWREG, SEL)                                                                                          \
    asm("v_cmp_eq_u32_sdwa %[m0], %[r], %[ca] src0_sel:" SEL " src1_sel:WORD_0\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m1], %[r], %[ca] src0_sel:" SEL " src1_sel:WORD_1\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m2], %[r], %[cb] src0_sel:" SEL " src1_sel:WORD_0\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m3], %[r], %[cb] src0_sel:" SEL " src1_sel:WORD_1\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m4], %[r], %[cc] src0_sel:" SEL " src1_sel:WORD_0\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m5], %[r], %[cc] src0_sel:" SEL " src1_sel:WORD_1\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m6], %[r], %[cd] src0_sel:" SEL " src1_sel:WORD_0\n\t"                                    \
        "v_cmp_eq_u32_sdwa %[m7], %[r], %[cd] src0_sel:" SEL " src1_sel:WORD_1\n\t"                                    \
        "v_addc_co_u32_e64 %[a0], %[m0], 0, %[a0], %[m0]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a1], %[m1], 0, %[a1], %[m1]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a2], %[m2], 0, %[a2], %[m2]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a3], %[m3], 0, %[a3], %[m3]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a4], %[m4], 0, %[a4], %[m4]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a5], %[m5], 0, %[a5], %[m5]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a6], %[m6], 0, %[a6], %[m6]\n\t"                                                          \
        "v_addc_co_u32_e64 %[a7], %[m7], 0, %[a7], %[m7]"                                                                \
        : [a0] "+v"(acc[R][0]), [a1] "+v"(acc[R][1]), [a2] "+v"(acc[R][2]), [a3] "+v"(acc[R][3]), [a4] "+v"(acc[R][4]),   \
          [a5] "+v"(acc[R][5]), [a6] "+v"(acc[R][6]), [a7] "+v"(acc[R][7]), [m0] "=&s"(msk[0]), [m1] "=&s"(msk[1]),       \
          [m2] "=&s"(msk[2]), [m3] "=&s"(msk[3]), [m4] "=&s"(msk[4]), [m5] "=&s"(msk[5]), [m6] "=&s"(msk[6]),             \
          [m7] "=&s"(msk[7])                                                                                            \
        : [r] "v"(ROWREG), [ca] "v"(c0.x), [cb] "v"(c0.y), [cc] "v"(c1.x), [cd] "v"(c1.y))

__global__ __launch_bounds__(TPB) void k_sample_counts(const unsigned short *__restrict__ S, int m, int n, size_t ldn,
                                                      unsigned *__restrict__ C, size_t ld)
{
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                                   // tiles below the diagonal are written by their mirror images
    __shared__ __align__(16) unsigned short rows[SC][TI];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ty = (wave >> 1) * 8 + (lane >> 3), tx = (wave & 1) * 8 + (lane & 7);
    const int i0 = bi * TI, j0 = bj * TJ;

    unsigned acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = 0u;

    const unsigned short *__restrict__ colp = S + j0 + tx * 4;
    uint2 n0 = *reinterpret_cast<const uint2 *>(colp), n1 = *reinterpret_cast<const uint2 *>(colp + 64);   // sample 0
    unsigned long long msk[8];
    for (int s0 = 0; s0 < m; s0 += SC) {
        const int cnt = min(SC, m - s0);
        __syncthreads();                                   // the previous chunk has been read
        // 16 threads per sample, 8 row labels (16 bytes) each; ldn covers the whole tile, so every read is in bounds
        for (int q = tid; q < cnt * (TI / 8); q += TPB) {
            const int t = q >> 4, r = (q & 15) * 8;
            uint4 v = *reinterpret_cast<const uint4 *>(S + (size_t)(s0 + t) * ldn + i0 + r);
            v.x = row_pads(v.x); v.y = row_pads(v.y); v.z = row_pads(v.z); v.w = row_pads(v.w);
            *reinterpret_cast<uint4 *>(&rows[t][r]) = v;
        }
        __syncthreads();
        for (int t = 0; t < cnt; ++t) {
            const uint2 c0 = n0, c1 = n1;
            {   // the next sample's column labels (the last sample again at the very end: always in bounds)
                const unsigned short *cp = colp + (size_t)min(s0 + t + 1, m - 1) * ldn;
                n0 = *reinterpret_cast<const uint2 *>(cp); n1 = *reinterpret_cast<const uint2 *>(cp + 64);
            }
            __builtin_amdgcn_sched_barrier(0);             // keep those loads in front of the sample's 128 instructions
            const uint2 r0 = *reinterpret_cast<const uint2 *>(&rows[t][ty * 4]), r1 = *reinterpret_cast<const uint2 *>(&rows[t][64 + ty * 4]);
            SC_ROW(0, r0.x, "WORD_0"); SC_ROW(1, r0.x, "WORD_1"); SC_ROW(2, r0.y, "WORD_0"); SC_ROW(3, r0.y, "WORD_1");
            SC_ROW(4, r1.x, "WORD_0"); SC_ROW(5, r1.x, "WORD_1"); SC_ROW(6, r1.y, "WORD_0"); SC_ROW(7, r1.y, "WORD_1");
        }
    }
#undef SC_ROW

    // the tile as computed: rows below n, 16-byte column groups below ld (ld is a multiple of 4; pad columns hold zero)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int row = i0 + (r >> 2) * 64 + ty * 4 + (r & 3);
        if (row >= n) continue;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const size_t col = (size_t)j0 + g * 64 + tx * 4;
            if (col < ld) *reinterpret_cast<uint4 *>(C + (size_t)row * ld + col) = make_uint4(acc[r][g * 4], acc[r][g * 4 + 1], acc[r][g * 4 + 2], acc[r][g * 4 + 3]);
        }
    }
    if (bj == bi) return;
    // its mirror image: row = the thread's column, 16-byte groups along the thread's rows
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int row = j0 + (c >> 2) * 64 + tx * 4 + (c & 3);
        if (row >= n) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const size_t col = (size_t)i0 + h * 64 + ty * 4;
            if (col < ld) *reinterpret_cast<uint4 *>(C + (size_t)row * ld + col) = make_uint4(acc[h * 4][c], acc[h * 4 + 1][c], acc[h * 4 + 2][c], acc[h * 4 + 3][c]);
        }
    }
}

// Labels 1..n narrowed to u16, sample-major with leading dimension ldn, pads 0xFFFE.  Host only.
static int32_t narrow(const char *who, const int64_t *samples, int64_t m, int64_t n, size_t ldn, std::vector<unsigned short> &out)
{
    const int32_t rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    try { out.assign((size_t)m * ldn, (unsigned short)PAD_COL); }
    catch (const std::bad_alloc &) { return fail(nullptr, RC_ERR_OOM, "%s: no host memory for the %lld x %zu 16-bit labels", who, (long long)m, ldn); }
    for (int64_t s = 0; s < m; ++s)
        for (int64_t j = 0; j < n; ++j) out[(size_t)s * ldn + j] = (unsigned short)samples[(size_t)s * n + j];
    return RC_OK;
}

// The counts of the samples in device memory: n × ld uint32 in d_counts, owned by B (every entry written, pad columns zero).
// The device is selected; work goes to the null stream.  ms (may be NULL): device time of the kernel.
static int32_t build(const char *who, const int64_t *samples, int64_t m, int64_t n, int64_t ld, DeviceBuffers &B,
                     unsigned *&d_counts, double *ms)
{
    const size_t ldn = (size_t)(n + TJ - 1) / TJ * TJ;
    std::vector<unsigned short> h_S;
    int32_t rc = narrow(who, samples, m, n, ldn, h_S);
    if (rc != RC_OK) return rc;
    unsigned short *d_S;
    HIPCHK(nullptr, B.alloc(d_counts, (size_t)n * (size_t)ld));
    HIPCHK(nullptr, B.alloc(d_S, h_S.size()));
    HIPCHK(nullptr, hipMemcpy(d_S, h_S.data(), h_S.size() * 2, hipMemcpyHostToDevice));
    const unsigned nt = (unsigned)(ldn / TJ);
    TimingEvents ev;
    HIPCHK(nullptr, ev.create());
    HIPCHK(nullptr, ev.begin(0));
    k_sample_counts<<<dim3(nt, nt), TPB, 0, 0>>>(d_S, (int)m, (int)n, ldn, d_counts, (size_t)ld);
    HIPCHK(nullptr, ev.end(0));
    double t = 0.0;
    HIPCHK(nullptr, ev.elapsed_ms(t));
    if (ms) *ms = t;
    return RC_OK;
}

}  // namespace sc

// ---- One counts source for the consumers of the matrix: the search (pointsearch.inc.hip), the dendrogram and the expected
// loss (hclust.inc.hip).  DESIGN.md §8 "One counts source".
namespace cnt {

// Where the n × n counts of m samples come from: a host matrix or the samples themselves, for `device`, or a live context
struct Source {
    enum Kind { HOST, SAMPLES, CTX } kind;
    int32_t device;
    const void *host;                                      // HOST: n × n uint32; SAMPLES: m × n int64 labels 1..n
    int64_t m, n;
    double *counts_ms;                                     // SAMPLES (may be NULL): device time of k_sample_counts
    rc_ctx *c;                                             // CTX
};
static Source host_counts(int32_t device, const void *counts, int64_t m, int64_t n) { return {Source::HOST, device, counts, m, n, nullptr, nullptr}; }
static Source samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, double *counts_ms)
{
    return {Source::SAMPLES, device, samples, m, n, counts_ms, nullptr};
}
static Source context(rc_ctx *c, int64_t numsamples) { return {Source::CTX, 0, nullptr, numsamples, c ? c->n : 0, nullptr, c}; }

// The counts on the device: n × ld at d (ld a multiple of 4, pad columns zero for the device forms), read in place.  Errors go
// to c and work to st: the context and its stream sA, or null and null — the thread's buffer, the null stream — for the
// device forms, whose staged matrix B owns.
struct OnDevice {
    DeviceBuffers B;
    const unsigned *d = nullptr;
    int64_t ld = 0;
    rc_ctx *c = nullptr;
    hipStream_t st = nullptr;
};

// Selects the source's device and puts its counts there.  A context's counts are flushed, checked to hold a sample, and then
// read where they are, at leading dimension ldc: nothing of the context is written.
static int32_t acquire(const char *who, const Source &s, OnDevice &D)
{
    if (s.kind == Source::CTX) {
        rc_ctx *c = s.c;
        HIPCHK(c, hipSetDevice(c->dev));
        unsigned d0 = 0;                                   // the first diagonal entry: the number of recorded samples
        if (c->counts) {
            int32_t rc = flush_counts(c);
            if (rc != RC_OK) return rc;
            rc = sync_and_check(c);
            if (rc != RC_OK) return rc;
            HIPCHK(c, hipMemcpy(&d0, c->counts, sizeof(unsigned), hipMemcpyDeviceToHost));
        }
        if (d0 == 0) return fail(c, RC_ERR_STATE, "%s: no sample has been recorded", who);
        D.d = c->counts; D.ld = c->ldc; D.c = c; D.st = c->sA;
        return RC_OK;
    }
    int32_t rc = select_device(who, s.device);
    if (rc != RC_OK) return rc;
    const int64_t n = s.n, ld = (n + 3) / 4 * 4;
    unsigned *d;
    if (s.kind == Source::SAMPLES) {
        rc = sc::build(who, (const int64_t *)s.host, s.m, n, ld, D.B, d, s.counts_ms);
        if (rc != RC_OK) return rc;
    } else {
        HIPCHK(nullptr, D.B.alloc(d, (size_t)n * ld));
        if (ld != n) HIPCHK(nullptr, hipMemset(d, 0, (size_t)n * ld * sizeof(unsigned)));
        HIPCHK(nullptr, hipMemcpy2D(d, (size_t)ld * sizeof(unsigned), s.host, (size_t)n * sizeof(unsigned), (size_t)n * sizeof(unsigned), (size_t)n,
                                    hipMemcpyHostToDevice));
    }
    D.d = d; D.ld = ld;
    return RC_OK;
}

// A consumer's entry point in the order every form keeps: the source is there; check(c, m, n), the consumer's own argument
// checks; acquire; run(c, st, d, ld, m, n), which begins with its own checks and check_counts.
template <typename Check, typename Run> static int32_t with(const char *who, const Source &s, Check check, Run run)
{
    if (s.kind == Source::CTX ? !s.c : !s.host) return fail(s.c, RC_ERR_ARG, s.kind == Source::CTX ? "%s: NULL ctx" : "%s: NULL argument", who);
    int32_t rc = check(s.c, s.m, s.n);
    if (rc != RC_OK) return rc;
    OnDevice D;
    rc = acquire(who, s, D);
    if (rc != RC_OK) return rc;
    return run(D.c, D.st, D.d, D.ld, s.m, s.n);
}

}  // namespace cnt

extern "C" int32_t rc_samples_counts(int32_t device, const int64_t *samples, int64_t m, int64_t n, void *counts_out, double *kernel_ms)
{
    const char *who = "rc_samples_counts";
    if (!samples || !counts_out) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (m < 1 || n < 1) return fail(nullptr, RC_ERR_ARG, "%s: need m >= 1 and n >= 1 (got m=%lld n=%lld)", who, (long long)m, (long long)n);
    if (n > sc::NMAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %lld points whose labels fit 16 bits beside the pads", who, (long long)n, (long long)sc::NMAX);
    if (m > 0x7FFFFFFFll) return fail(nullptr, RC_ERR_CAPACITY, "%s: m = %lld exceeds the 2^31 - 1 samples a 32-bit count holds", who, (long long)m);
    int32_t rc = select_device(who, device);
    if (rc != RC_OK) return rc;
    const int64_t ld = (n + 3) / 4 * 4;
    DeviceBuffers B;
    unsigned *d_counts;
    rc = sc::build(who, samples, m, n, ld, B, d_counts, kernel_ms);
    if (rc != RC_OK) return rc;
    HIPCHK(nullptr, hipMemcpy2D(counts_out, (size_t)n * sizeof(unsigned), d_counts, (size_t)ld * sizeof(unsigned), (size_t)n * sizeof(unsigned), (size_t)n,
                      hipMemcpyDeviceToHost));
    return RC_OK;
}

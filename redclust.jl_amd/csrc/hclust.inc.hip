// Hierarchical point estimates on the device: agglomerative clustering of the posterior co-clustering counts C (n×n
// uint32, C_ii = m) — Medvedovic's method, mcclust's minbinder / mcclust.ext's minVI with method = "avg" / "comp" — and the
// expected loss of a batch of given labellings under the same counts.  DESIGN.md §8 "Hierarchical point estimates".
// Included at the end of redclust_hip.hip behind samplecounts.inc.hip (same translation unit: shares fail(), HIPCHK, rc_ctx;
// the holders, check_counts, check_lds_capacity and LDS_NMAX of hostutil.inc.hip; greedy::shfl_xor_u64; cnt:: of
// samplecounts.inc.hip, which puts the counts of every entry point here on the device: nothing below stages a matrix or
// touches a context's counts).
//
// Linkage.  Clusters are named by their smallest member.  Per pair of active clusters a < b: S_ab = Σ_{i∈a, j∈b} C_ij (u64)
// and, for the two extreme linkages, M_ab = min (complete) or max (single) of C_ij over the pair (u32).  The similarity of a
// pair is the fraction S_ab / (|a|·|b|) (average) or M_ab / 1; fractions are compared by cross-multiplication in 128 bits
// (cmp_frac; with denominator 1 that is the comparison of the counts themselves), so a run is a pure integer function of
// (C, m, linkage).  A step merges the pair
// of largest similarity — ties: smallest a, then smallest b — b into a: S_ac += S_bc, M_ac = min / max(M_ac, M_bc).
//
// One job = one workgroup of 1024 threads, persistent over its n − 1 steps.  S and M are full symmetric n×n matrices in
// global memory, written and re-read by this one workgroup across __syncthreads().  Per active row r the LDS holds its best
// partner among the larger names (val = the partner's S or M, part = its name) and the cluster size:
//   val u64[n], part u16[n], sz u16[n], list u16[n]  — 14 bytes per point, 112 KiB at n = 8192.
// A step:  (A) block-wide argmax over the row caches;  (B) the thread that owns column c adds row b into row a and mirrors
// the entry into column a, then repairs row c's cache — the new (c, a) entry is compared with the cached one; a row whose
// cached partner was a or b goes on the rescan list; row a's new cache is a second block-wide argmax over the new entries;
// (C) one wave per listed row rescans it.
// Three barriers per step.  k_hclust_init (one workgroup per row) copies C into S and M and finds every row's first partner.
//
// Expected loss of given labellings: k_eloss returns T_i = Σ_{j: c_j = c_i} C_ij (u32) for every labelling and point; a
// workgroup stages up to EG labellings in LDS and reads each of its rows of C once for all of them.  The host finishes
// both criteria from T and the cluster sizes, so the device returns integers only.

namespace hcl {

constexpr int TPB = 1024;
constexpr int NWAVE = TPB / 64;
constexpr unsigned NONE = 0xFFFFu;       // no active larger name
constexpr int U = 4;                     // columns a thread (row update) or lane (rescan) keeps in flight
constexpr int EG = 8;                    // labellings per LDS group of k_eloss: 8 × 16 KiB at n = 8192
constexpr int64_t LMAX = 65536;          // labellings per call

struct Merge { int a, b, size; unsigned M; long long S; };   // rc_hclust_merge_t
static_assert(sizeof(Merge) == sizeof(rc_hclust_merge_t), "Merge mirrors rc_hclust_merge_t");

struct Args {
    unsigned long long *S;               // n × n
    unsigned *M;                         // n × n (null for average)
    const unsigned long long *val0;      // first row caches, from k_hclust_init
    const unsigned short *part0;
    const unsigned long long *tot;       // Σ_{i<j} C_ij
    Merge *merges;                       // n − 1 out
    long long *bnum;                     // n out
    int n;
    unsigned m;
};

// The sign of x/xd − y/yd, by x·yd against y·xd in 128 bits: S ≤ m·n²/4 < 2^42 times a size product < 2^24 passes 2^64 only
// near n = 8192 with m ≥ 65536, which no test reaches — so there is no 64-bit path beside this one.
__device__ inline int cmp_frac(unsigned long long x, unsigned xd, unsigned long long y, unsigned yd)
{
    const unsigned long long lh = __umul64hi(x, (unsigned long long)yd), ll = x * yd;
    const unsigned long long rh = __umul64hi(y, (unsigned long long)xd), rl = y * xd;
    if (lh != rh) return lh > rh ? 1 : -1;
    return ll > rl ? 1 : (ll < rl ? -1 : 0);
}

// a candidate pair: similarity num/den and the name the tie rule looks at (~0u: none; it loses every tie)
struct Cand { unsigned long long num; unsigned den, idx; };

// LINK: complete and single compare M_ab itself — every denominator is 1 — so only average pays for the products
template <int LINK>
__device__ inline bool better(const Cand &x, const Cand &y)
{
    const int c = LINK ? (int)(x.num > y.num) - (int)(x.num < y.num) : cmp_frac(x.num, x.den, y.num, y.den);
    return c > 0 || (c == 0 && x.idx < y.idx);
}

template <int LINK>
__device__ inline Cand wave_best(Cand v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const Cand o{greedy::shfl_xor_u64(v.num, off), (unsigned)__shfl_xor((int)v.den, off), (unsigned)__shfl_xor((int)v.idx, off)};
        if (better<LINK>(o, v)) v = o;
    }
    return v;
}

// the best of the NWAVE per-wave candidates a workgroup left in LDS, in every lane
template <int LINK>
__device__ inline Cand block_best(const unsigned long long *num, const unsigned *den, const unsigned *idx, int lane)
{
    const int w = lane & (NWAVE - 1);
    Cand v{num[w], den[w], idx[w]};
#pragma unroll
    for (int off = NWAVE / 2; off > 0; off >>= 1) {
        const Cand o{greedy::shfl_xor_u64(v.num, off), (unsigned)__shfl_xor((int)v.den, off), (unsigned)__shfl_xor((int)v.idx, off)};
        if (better<LINK>(o, v)) v = o;
    }
    return v;
}

// Σ_{i<j} C_ij: one workgroup per row, integer atomics
__global__ __launch_bounds__(256) void k_triu_sum(const unsigned *__restrict__ C, size_t ldc, int n, unsigned long long *tot)
{
    __shared__ unsigned long long part[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    unsigned long long s = 0;
    for (int c = r + 1 + tid; c < n; c += 256) s += C[(size_t)r * ldc + c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += greedy::shfl_xor_u64(s, off);
    if ((tid & 63) == 0) part[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd(tot, s);
    }
}

// Row r of S (and M) from C, and the row's first cache: the largest C_rc over c > r, the smallest such c (all sizes are 1,
// so counts are compared whatever the linkage)
template <int LINK>
__global__ __launch_bounds__(256) void k_hclust_init(const unsigned *__restrict__ C, size_t ldc, int n, unsigned long long *S,
                                                     unsigned *M, unsigned long long *val0, unsigned short *part0)
{
    __shared__ unsigned long long r_num[4];
    __shared__ unsigned r_idx[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    Cand best{0ull, 1u, ~0u};
    for (int c = tid; c < n; c += 256) {
        const unsigned v = C[(size_t)r * ldc + c];
        S[(size_t)r * n + c] = v;
        if (LINK) M[(size_t)r * n + c] = v;
        const Cand x{v, 1u, (unsigned)c};
        if (c > r && better<1>(x, best)) best = x;
    }
    best = wave_best<1>(best);
    if ((tid & 63) == 0) { r_num[tid >> 6] = best.num; r_idx[tid >> 6] = best.idx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            const Cand x{r_num[w], 1u, r_idx[w]};
            if (better<1>(x, best)) best = x;
        }
        val0[r] = best.num;
        part0[r] = (unsigned short)(best.idx == ~0u ? NONE : best.idx);
    }
}

template <int LINK>
__global__ __launch_bounds__(TPB) void k_hclust(Args A)
{
    extern __shared__ unsigned long long hcl_lds[];
    __shared__ unsigned long long r_num[NWAVE];
    __shared__ unsigned r_den[NWAVE], r_idx[NWAVE];
    __shared__ unsigned long long a_num[NWAVE];                        // row a's new cache, per wave
    __shared__ unsigned a_den[NWAVE], a_idx[NWAVE];
    __shared__ unsigned n_list;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n;
    const size_t ld = (size_t)n;
    unsigned long long *S = A.S;
    unsigned *M = A.M;

    unsigned long long *val = hcl_lds;
    unsigned short *part = reinterpret_cast<unsigned short *>(val + n);
    unsigned short *sz = part + n;
    unsigned short *list = sz + n;

    for (int r = tid; r < n; r += TPB) { val[r] = A.val0[r]; part[r] = A.part0[r]; sz[r] = 1; }
    long long num = (long long)*A.tot;                                 // the Binder numerator of the current partition (thread 0's)
    if (tid == 0) A.bnum[0] = num;
    __syncthreads();

    for (int t = 1; t < n; ++t) {
        // (A) the closest pair: every active row offers its cached partner
        Cand best{0ull, 1u, ~0u};
        for (int r = tid; r < n; r += TPB) {
            const unsigned p = part[r], s = sz[r];
            if (!s || p == NONE) continue;
            const Cand x{val[r], LINK ? 1u : s * (unsigned)sz[p], (unsigned)r};
            if (better<LINK>(x, best)) best = x;
        }
        best = wave_best<LINK>(best);
        if (lane == 0) { r_num[wave] = best.num; r_den[wave] = best.den; r_idx[wave] = best.idx; }
        if (tid == 0) n_list = 0;
        __syncthreads();
        best = block_best<LINK>(r_num, r_den, r_idx, lane);
        if (best.idx == ~0u) break;                                     // (uniform; cannot happen while two clusters are active)
        const int a = (int)best.idx, b = (int)part[a];
        const unsigned szA = sz[a], szB = sz[b], newsz = szA + szB;
        if (tid == 0) {
            const unsigned long long Sab = LINK ? S[(size_t)a * ld + b] : best.num;
            num += (long long)((unsigned long long)szA * szB * A.m) - 2ll * (long long)Sab;
            A.merges[t - 1] = Merge{a + 1, b + 1, (int)newsz, LINK ? (unsigned)best.num : 0u, (long long)Sab};
            A.bnum[t] = num;
        }
        // (B) row b into row a, mirrored into column a; the owner of column c repairs row c's cache.  Row a changes in
        // every entry: its new cache is the best of the new entries at the larger names, which are in registers here
        Cand ra{0ull, 1u, ~0u};
        for (int c0 = tid; c0 < n; c0 += U * TPB) {
            // U columns per thread at a time: all their loads are issued before the first store
            unsigned long long sa[U], sb[U];
            unsigned xa[U], xb[U], scs[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * TPB;
                scs[u] = (c < n && c != a && c != b) ? (unsigned)sz[c] : 0u;
                if (!scs[u]) continue;
                sa[u] = S[(size_t)a * ld + c];
                sb[u] = S[(size_t)b * ld + c];
                if (LINK) { xa[u] = M[(size_t)a * ld + c]; xb[u] = M[(size_t)b * ld + c]; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * TPB;
                const unsigned sc_ = scs[u];
                if (!sc_) continue;
                const unsigned long long s = sa[u] + sb[u];
                S[(size_t)a * ld + c] = s;
                S[(size_t)c * ld + a] = s;
                unsigned long long v = s;
                if (LINK) {
                    const unsigned mm = LINK == RC_HCLUST_COMPLETE ? min(xa[u], xb[u]) : max(xa[u], xb[u]);
                    M[(size_t)a * ld + c] = mm;
                    M[(size_t)c * ld + a] = mm;
                    v = mm;
                }
                if (c > a) {
                    const Cand x{v, LINK ? 1u : newsz * sc_, (unsigned)c};
                    if (better<LINK>(x, ra)) ra = x;
                }
                if (c > b) continue;                                    // row c holds larger names only: neither a nor b
                const unsigned p = part[c];
                if (p == (unsigned)b || p == (unsigned)a) {
                    list[atomicAdd(&n_list, 1u)] = (unsigned short)c;   // its cached entry is gone (b) or has changed (a)
                } else if (c < a) {
                    const Cand x{v, LINK ? 1u : sc_ * newsz, (unsigned)a}, cur{val[c], LINK ? 1u : sc_ * (unsigned)sz[p], p};
                    if (better<LINK>(x, cur)) { val[c] = v; part[c] = (unsigned short)a; }
                }
            }
        }
        ra = wave_best<LINK>(ra);
        if (lane == 0) { a_num[wave] = ra.num; a_den[wave] = ra.den; a_idx[wave] = ra.idx; }
        __syncthreads();
        // (C) rescans, one wave per listed row; sz[a] and sz[b] are being rewritten, so their new values come from registers
        if (tid == 0) { sz[a] = (unsigned short)newsz; sz[b] = 0; }
        if (wave == NWAVE - 1) {
            ra = block_best<LINK>(a_num, a_den, a_idx, lane);
            if (lane == 0) { val[a] = ra.num; part[a] = (unsigned short)(ra.idx == ~0u ? NONE : ra.idx); }
        }
        const unsigned cnt = n_list;
        for (unsigned q = wave; q < cnt; q += NWAVE) {
            const int r = list[q];
            const unsigned szr = sz[r];                                   // (a listed row is neither a nor b)
            Cand bc{0ull, 1u, ~0u};
            for (int c0 = r + 1 + lane; c0 < n; c0 += U * 64) {
                unsigned long long v[U];
                unsigned szc[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int c = c0 + u * 64;
                    szc[u] = c < n ? (c == a ? newsz : (c == b ? 0u : (unsigned)sz[c])) : 0u;
                    if (szc[u]) v[u] = LINK ? (unsigned long long)M[(size_t)r * ld + c] : S[(size_t)r * ld + c];
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!szc[u]) continue;
                    const Cand x{v[u], LINK ? 1u : szr * szc[u], (unsigned)(c0 + u * 64)};
                    if (better<LINK>(x, bc)) bc = x;
                }
            }
            bc = wave_best<LINK>(bc);
            if (lane == 0) { val[r] = bc.num; part[r] = (unsigned short)(bc.idx == ~0u ? NONE : bc.idx); }
        }
        __syncthreads();
    }
}

// T[l][i] = Σ_{j: lab_l[j] = lab_l[i]} C_ij for labellings l of one group of EG; one wave per row i
__global__ __launch_bounds__(TPB) void k_eloss(const unsigned *__restrict__ C, size_t ldc, int n, const unsigned short *__restrict__ labs,
                                               int L, unsigned *__restrict__ T)
{
    extern __shared__ unsigned short el_lab[];                          // G × n
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = blockIdx.y * EG, G = min(EG, L - g0);
    for (int k = tid; k < G * n; k += TPB) el_lab[k] = labs[(size_t)g0 * n + k];
    __syncthreads();
    for (int i = blockIdx.x * NWAVE + wave; i < n; i += gridDim.x * NWAVE) {
        unsigned li[EG], acc[EG];
#pragma unroll
        for (int g = 0; g < EG; ++g) { li[g] = g < G ? (unsigned)el_lab[g * n + i] : 0u; acc[g] = 0; }
        for (int j = lane; j < n; j += 64) {
            const unsigned v = C[(size_t)i * ldc + j];
#pragma unroll
            for (int g = 0; g < EG; ++g)
                if (g < G && el_lab[g * n + j] == li[g]) acc[g] += v;
        }
#pragma unroll
        for (int g = 0; g < EG; ++g) {
            unsigned s = acc[g];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += (unsigned)__shfl_xor((int)s, off);
            if (lane == 0 && g < G) T[(size_t)(g0 + g) * n + i] = s;
        }
    }
}

// ---- host side

static int32_t check_capacity(rc_ctx *c, const char *who, int64_t m, int64_t n)
{
    if (m < 1 || n < 1) return fail(c, RC_ERR_ARG, "%s: need m >= 1 and n >= 1 (got m=%lld n=%lld)", who, (long long)m, (long long)n);
    return check_lds_capacity(c, who, n, m);
}

// The partition after the first n − K merges as labels 1..K in sortlabels order: names are smallest members, so a cluster's
// rank among the names is the order of its first appearance.  A parent is always a smaller name than its child, so one
// ascending pass resolves every chain.  false: the merges are not a valid sequence.
static bool cut_labels(const Merge *mg, int64_t n, int64_t K, std::vector<int> &work, int64_t *out64, unsigned short *out16)
{
    work.resize((size_t)n);
    int *parent = work.data();
    for (int64_t i = 0; i < n; ++i) parent[i] = (int)i;
    for (int64_t t = 0; t < n - K; ++t) {
        const int64_t a = (int64_t)mg[t].a - 1, b = (int64_t)mg[t].b - 1;
        if (a < 0 || b <= a || b >= n || parent[a] != a || parent[b] != b) return false;
        parent[b] = (int)a;
    }
    int next = 0;
    for (int64_t i = 0; i < n; ++i) {
        // roots take the next rank (stored as −rank); members copy their parent's, which is resolved already
        const int v = parent[i] == (int)i ? -(++next) : parent[parent[i]];
        parent[i] = v;
        if (out64) out64[i] = -v;
        if (out16) out16[i] = (unsigned short)(-v);
    }
    return true;
}

// T of L labellings (slots 1..n as u16, L × n) under the device counts; ms: device time of the kernel, added to *ms
static int32_t eloss_T(rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ldc, int64_t n, const std::vector<unsigned short> &labs,
                       int64_t L, std::vector<unsigned> &T, double &ms)
{
    DeviceBuffers B;
    unsigned short *d_lab;
    unsigned *d_T;
    HIPCHK(c, B.alloc(d_lab, labs.size()));
    HIPCHK(c, B.alloc(d_T, labs.size()));
    HIPCHK(c, hipMemcpyAsync(d_lab, labs.data(), labs.size() * 2, hipMemcpyHostToDevice, st));
    const size_t lds = (size_t)std::min<int64_t>(EG, L) * (size_t)n * 2;
    HIPCHK(c, hipFuncSetAttribute((const void *)k_eloss, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    TimingEvents ev;
    HIPCHK(c, ev.create());
    HIPCHK(c, ev.begin(st));
    k_eloss<<<dim3((unsigned)std::min<int64_t>((n + NWAVE - 1) / NWAVE, 256), (unsigned)((L + EG - 1) / EG)), TPB, lds, st>>>(
        dC, (size_t)ldc, (int)n, d_lab, (int)L, d_T);
    HIPCHK(c, ev.end(st));
    T.resize(labs.size());
    HIPCHK(c, hipMemcpyAsync(T.data(), d_T, T.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, ev.elapsed_ms(ms));
    return RC_OK;
}

// Σ_{i<j} C_ij of the device counts
static int32_t triu_sum(rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ldc, int64_t n, unsigned long long *d_tot)
{
    HIPCHK(c, hipMemsetAsync(d_tot, 0, sizeof(unsigned long long), st));
    k_triu_sum<<<(unsigned)n, 256, 0, st>>>(dC, (size_t)ldc, (int)n, d_tot);
    HIPCHK(c, hipGetLastError());
    return RC_OK;
}

// The two criteria of one labelling from its T (redclust_hip.h): cnt is scratch of n + 1 entries
static void finish(int32_t loss, const unsigned short *lab, const unsigned *T, int64_t n, int64_t m, long long tot, std::vector<long long> &cnt,
                   double *loss_out, int64_t *num_out)
{
    std::fill(cnt.begin(), cnt.end(), 0ll);
    for (int64_t i = 0; i < n; ++i) cnt[lab[i]]++;
    if (loss == RC_PSM_VILB) {
        double f = 0.0;
        for (int64_t i = 0; i < n; ++i) f += std::log((double)cnt[lab[i]]) - 2.0 * std::log((double)T[i]);
        *loss_out = f / (double)n + 2.0 * std::log((double)m);
        if (num_out) *num_out = 0;
        return;
    }
    long long same = 0, twice = 0;
    for (int64_t k = 0; k <= n; ++k) same += cnt[(size_t)k] * (cnt[(size_t)k] - 1) / 2;
    for (int64_t i = 0; i < n; ++i) twice += (long long)T[i] - m;
    const long long num = tot + same * m - twice, pairs = n * (n - 1) / 2;
    *loss_out = pairs ? (double)num / (double)(m * pairs) : 0.0;
    if (num_out) *num_out = num;
}

template <int LINK>
static hipError_t launch(const unsigned *dC, int64_t ldc, size_t lds, hipStream_t st, unsigned long long *d_val0, unsigned short *d_part0,
                         const Args &A)
{
    hipError_t e = hipFuncSetAttribute((const void *)k_hclust<LINK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    k_hclust_init<LINK><<<(unsigned)A.n, 256, 0, st>>>(dC, (size_t)ldc, A.n, A.S, A.M, d_val0, d_part0);
    k_hclust<LINK><<<1, TPB, lds, st>>>(A);
    return hipGetLastError();
}

static int32_t check_args(rc_ctx *c, const char *who, int64_t m, int64_t n, int32_t linkage, const void *merges_out, const int64_t *binder_num,
                          int32_t maxcut, const double *vilb)
{
    if (!merges_out || !binder_num) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    if (linkage != RC_HCLUST_AVERAGE && linkage != RC_HCLUST_COMPLETE && linkage != RC_HCLUST_SINGLE)
        return fail(c, RC_ERR_ARG, "%s: invalid linkage specifier %d", who, linkage);
    const int32_t rc = check_capacity(c, who, m, n);
    if (rc != RC_OK) return rc;
    if (maxcut < 0 || maxcut > n || (maxcut > 0 && !vilb)) return fail(c, RC_ERR_ARG, "%s: need 0 <= maxcut <= n and vilb with maxcut > 0 (got %d)", who, maxcut);
    return RC_OK;
}

// Everything behind the three entry points.  dC: the device counts (n × ldc), read in place.
static int32_t run(rc_ctx *c, hipStream_t st, const char *who, const unsigned *dC, int64_t ldc, int64_t m, int64_t n, int32_t linkage,
                   rc_hclust_merge_t *merges_out, int64_t *binder_num, int32_t maxcut, double *vilb, double *kernel_ms)
{
    int32_t rc = check_counts(c, st, who, dC, ldc, m, n);
    if (rc != RC_OK) return rc;
    DeviceBuffers B;
    Args A{};
    unsigned long long *d_val0, *d_tot;
    unsigned short *d_part0;
    HIPCHK(c, B.alloc(A.S, (size_t)n * n));
    if (linkage != RC_HCLUST_AVERAGE) HIPCHK(c, B.alloc(A.M, (size_t)n * n));
    HIPCHK(c, B.alloc(d_val0, (size_t)n));
    HIPCHK(c, B.alloc(d_part0, (size_t)n));
    HIPCHK(c, B.alloc(d_tot, 1));
    HIPCHK(c, B.alloc(A.merges, (size_t)n));                            // (n − 1 used)
    HIPCHK(c, B.alloc(A.bnum, (size_t)n));
    HIPCHK(c, hipMemsetAsync(A.merges, 0, (size_t)n * sizeof(Merge), st));
    A.val0 = d_val0; A.part0 = d_part0; A.tot = d_tot; A.n = (int)n; A.m = (unsigned)m;
    const size_t lds = ((size_t)n * 14 + 15) / 16 * 16;
    TimingEvents ev;
    HIPCHK(c, ev.create());
    HIPCHK(c, ev.begin(st));
    rc = triu_sum(c, st, dC, ldc, n, d_tot);
    if (rc != RC_OK) return rc;
    const hipError_t le = linkage == RC_HCLUST_AVERAGE    ? launch<RC_HCLUST_AVERAGE>(dC, ldc, lds, st, d_val0, d_part0, A)
                          : linkage == RC_HCLUST_COMPLETE ? launch<RC_HCLUST_COMPLETE>(dC, ldc, lds, st, d_val0, d_part0, A)
                                                          : launch<RC_HCLUST_SINGLE>(dC, ldc, lds, st, d_val0, d_part0, A);
    if (le != hipSuccess) return fail(c, RC_ERR_HIP, "%s: launch failed: %s", who, hipGetErrorString(le));
    HIPCHK(c, ev.end(st));
    std::vector<Merge> h_mg((size_t)n);
    long long tot = 0;
    if (n > 1) HIPCHK(c, hipMemcpyAsync(h_mg.data(), A.merges, (size_t)(n - 1) * sizeof(Merge), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(binder_num, A.bnum, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(&tot, d_tot, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    double ms = 0.0;
    HIPCHK(c, ev.elapsed_ms(ms));
    for (int64_t t = 0; t + 1 < n; ++t)                                 // (the buffer was zeroed: a step the kernel did not take)
        if (h_mg[(size_t)t].a == 0) return fail(c, RC_ERR_STATE, "%s: the kernel stopped before merge %lld of %lld", who, (long long)t + 1, (long long)n - 1);
    std::memcpy(merges_out, h_mg.data(), (size_t)(n - 1) * sizeof(Merge));

    if (maxcut > 0) {
        // the cuts K = 1..maxcut, derived on the host by un-merging, evaluated by k_eloss
        std::vector<unsigned short> labs((size_t)maxcut * n);
        std::vector<int> work;
        for (int64_t K = 1; K <= maxcut; ++K)
            if (!cut_labels(h_mg.data(), n, K, work, nullptr, labs.data() + (size_t)(K - 1) * n))
                return fail(c, RC_ERR_STATE, "%s: the kernel returned an invalid merge sequence", who);
        std::vector<unsigned> T;
        rc = eloss_T(c, st, dC, ldc, n, labs, maxcut, T, ms);
        if (rc != RC_OK) return rc;
        std::vector<long long> cnt((size_t)n + 1);
        for (int64_t K = 1; K <= maxcut; ++K)
            finish(RC_PSM_VILB, labs.data() + (size_t)(K - 1) * n, T.data() + (size_t)(K - 1) * n, n, m, tot, cnt, vilb + (K - 1), nullptr);
    }
    if (kernel_ms) *kernel_ms = ms;
    return RC_OK;
}

// rc_psm_expected_loss and its context form behind their argument checks
static int32_t run_eloss(rc_ctx *c, hipStream_t st, const char *who, const unsigned *dC, int64_t ldc, int64_t m, int64_t n, int32_t loss,
                         int64_t L, const int64_t *labels, double *loss_out, int64_t *num_out, double *kernel_ms)
{
    int32_t rc = check_label_rows(c, who, "labelling", labels, L, n);
    if (rc != RC_OK) return rc;
    std::vector<unsigned short> labs(labels, labels + (size_t)L * n);  // narrowed: 1..n fits 16 bits (check_capacity)
    rc = check_counts(c, st, who, dC, ldc, m, n);
    if (rc != RC_OK) return rc;
    DeviceBuffers B;
    unsigned long long *d_tot;
    HIPCHK(c, B.alloc(d_tot, 1));
    rc = triu_sum(c, st, dC, ldc, n, d_tot);
    if (rc != RC_OK) return rc;
    std::vector<unsigned> T;
    double ms = 0.0;
    rc = eloss_T(c, st, dC, ldc, n, labs, L, T, ms);
    if (rc != RC_OK) return rc;
    long long tot = 0;
    HIPCHK(c, hipMemcpy(&tot, d_tot, sizeof(long long), hipMemcpyDeviceToHost));
    std::vector<long long> cnt((size_t)n + 1);
    for (int64_t l = 0; l < L; ++l)
        finish(loss, labs.data() + (size_t)l * n, T.data() + (size_t)l * n, n, m, tot, cnt, loss_out + l, num_out + l);
    if (kernel_ms) *kernel_ms = ms;
    return RC_OK;
}

static int32_t check_eloss_args(rc_ctx *c, const char *who, int64_t m, int64_t n, int32_t loss, int64_t L, const int64_t *labels,
                                const double *loss_out, const int64_t *num_out)
{
    if (!labels || !loss_out || !num_out) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    if (loss != RC_PSM_BINDER && loss != RC_PSM_VILB) return fail(c, RC_ERR_ARG, "%s: invalid loss specifier %d", who, loss);
    if (L < 1) return fail(c, RC_ERR_ARG, "%s: need at least one labelling (got %lld)", who, (long long)L);
    const int32_t rc = check_capacity(c, who, m, n);
    if (rc != RC_OK) return rc;
    if (L > LMAX) return fail(c, RC_ERR_CAPACITY, "%s: %lld labellings exceed the %lld of one call", who, (long long)L, (long long)LMAX);
    return RC_OK;
}

// The entry points of both consumers: cnt::with puts the counts of src on the device between the argument checks and the run
static int32_t dendrogram(const char *who, const cnt::Source &src, int32_t linkage, void *merges_out, int64_t *binder_num, int32_t maxcut,
                          double *vilb, double *kernel_ms)
{
    return cnt::with(
        who, src, [&](rc_ctx *c, int64_t m, int64_t n) { return check_args(c, who, m, n, linkage, merges_out, binder_num, maxcut, vilb); },
        [&](rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ldc, int64_t m, int64_t n) {
            return run(c, st, who, dC, ldc, m, n, linkage, (rc_hclust_merge_t *)merges_out, binder_num, maxcut, vilb, kernel_ms);
        });
}

static int32_t expected_loss(const char *who, const cnt::Source &src, int32_t loss, int64_t L, const int64_t *labels, double *loss_out,
                             int64_t *num_out, double *kernel_ms)
{
    return cnt::with(
        who, src, [&](rc_ctx *c, int64_t m, int64_t n) { return check_eloss_args(c, who, m, n, loss, L, labels, loss_out, num_out); },
        [&](rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ldc, int64_t m, int64_t n) {
            return run_eloss(c, st, who, dC, ldc, m, n, loss, L, labels, loss_out, num_out, kernel_ms);
        });
}

}  // namespace hcl

extern "C" int32_t rc_hclust(int32_t device, const void *counts, int64_t m, int64_t n, int32_t linkage, void *merges_out,
                             int64_t *binder_num, int32_t maxcut, double *vilb, double *kernel_ms)
{
    return hcl::dendrogram("rc_hclust", cnt::host_counts(device, counts, m, n), linkage, merges_out, binder_num, maxcut, vilb, kernel_ms);
}

extern "C" int32_t rc_hclust_samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t linkage, void *merges_out,
                                     int64_t *binder_num, int32_t maxcut, double *vilb, double *kernel_ms, double *counts_ms)
{
    return hcl::dendrogram("rc_hclust_samples", cnt::samples(device, samples, m, n, counts_ms), linkage, merges_out, binder_num, maxcut, vilb,
                           kernel_ms);
}

extern "C" int32_t rc_hclust_ctx(rc_ctx *c, int64_t numsamples, int32_t linkage, void *merges_out, int64_t *binder_num, int32_t maxcut,
                                 double *vilb, double *kernel_ms)
{
    return hcl::dendrogram("rc_hclust_ctx", cnt::context(c, numsamples), linkage, merges_out, binder_num, maxcut, vilb, kernel_ms);
}

extern "C" int32_t rc_hclust_cut(const void *merges, int64_t n, int64_t K, int64_t *labels_out)
{
    const char *who = "rc_hclust_cut";
    if (!labels_out || (!merges && n > 1)) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    if (n < 1 || n > LDS_NMAX || K < 1 || K > n) return fail(nullptr, RC_ERR_ARG, "%s: need 1 <= K <= n <= %d (got K=%lld n=%lld)", who, LDS_NMAX, (long long)K, (long long)n);
    std::vector<int> work;
    if (!hcl::cut_labels((const hcl::Merge *)merges, n, K, work, labels_out, nullptr))
        return fail(nullptr, RC_ERR_ARG, "%s: the merges are not a sequence of merges of active clusters a < b", who);
    return RC_OK;
}

extern "C" int32_t rc_psm_expected_loss(int32_t device, const void *counts, int64_t m, int64_t n, int32_t loss, int64_t L,
                                        const int64_t *labels, double *loss_out, int64_t *num_out, double *kernel_ms)
{
    return hcl::expected_loss("rc_psm_expected_loss", cnt::host_counts(device, counts, m, n), loss, L, labels, loss_out, num_out, kernel_ms);
}

extern "C" int32_t rc_psm_expected_loss_ctx(rc_ctx *c, int64_t numsamples, int32_t loss, int64_t L, const int64_t *labels,
                                            double *loss_out, int64_t *num_out, double *kernel_ms)
{
    return hcl::expected_loss("rc_psm_expected_loss_ctx", cnt::context(c, numsamples), loss, L, labels, loss_out, num_out, kernel_ms);
}

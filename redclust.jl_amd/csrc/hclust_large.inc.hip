// The hierarchical point estimates of hclust.inc.hip for n <= 32767 (DESIGN.md §8 "Hierarchical point estimates, large n"): the
// device side of rc_hclust_large* and rc_psm_expected_loss_large*.  Included behind hclust.inc.hip (same translation unit and
// namespace: Args, Merge, Cand, better, wave_best, block_best, k_hclust_init, k_triu_sum and the whole host side are that file's;
// its run() and eloss_T() call launch_large and launch_eloss_large below when an entry point asks for the large kernels).
//
// The definition of a run — similarity, tie rule, merge records, Binder curve — is k_hclust's, and so are the one persistent
// workgroup of 1024 threads, the full symmetric S (u64) and M (u32) in global memory, and steps (B) and (C).  A step picks the
// largest candidate of a total order (the fraction, then the row), so how the maximum is reduced does not matter: a run returns
// k_hclust's bytes.  What pins k_hclust to n <= 8192 is its 14 bytes per point of LDS; here a point keeps 4:
//
// LDS (dynamic; npad = n rounded up to whole blocks of BLK = 32 rows, nb = npad / 32 <= 1024):
//   part u16[npad]   the cached partner of a row            65 536 B at n = 32767
//   sz   u16[npad]   cluster sizes, 0 = not active          65 536 B
//   rescan u32[nb]   one bit per row whose cache is gone     4 096 B
//   dirty  u8[nb]    blocks whose best must be found again   1 024 B      total 136 192 B (+ 512 B static reduction scratch)
//
// val, the cached best value of every row (u64, 262 KB), lives in global memory: k_hclust_init's output array, kept up by this
// one workgroup across __syncthreads() like S and M.  So that step (A) is no 262 KB read in front of every merge there is a
// second level: thread k keeps the best candidate of block k — rows 32k..32k+31 — in REGISTERS (value, denominator, row: it is
// the block's only reader and only writer, so no LDS is spent on it), and (A) is the wave and workgroup argmax over those
// 1024 candidates.  A row's candidate changes only when the row is a or b, is rescanned, or is repaired in (B); each of these
// marks the row's block dirty, and at the top of the next step the owner of a dirty block reads its 32 values (256 contiguous
// bytes, four batches of four 16-byte loads; partners and sizes come from LDS as 16-byte reads) and finds its best again.
//
// (B) as k_hclust: the owner of column c (up to 32 columns a thread, U at a time, every load of a batch issued before its first
// store) adds row b into row a, mirrors the entry into column a and repairs row c's cache; the cached value of row c it
// compares with is one more coalesced load of the batch, issued only for c < a.  A row whose partner was a or b sets its bit in
// rescan[] (LDS atomicOr) instead of joining a list.  (C): lane l of wave w owns mask word 16·l + w — neighbouring blocks go
// to different waves — reads and clears it, and the wave walks the set bits of its 64 words by ballot, one row at a time,
// rescanning it as k_hclust does.  Three barriers per step, no communication outside the workgroup.
//
// S and M stay full symmetric matrices (8.6 GB + 4.3 GB at n = 32767): row c is read whole in (B) when c later becomes a or b,
// so the mirrored entries are read, and an upper triangle would turn the n scattered 8-byte stores of a step into as many
// scattered loads in front of the adds.  What the mirror costs is those n stores per step, 4× k_hclust's at n = 8192.
//
// k_eloss_large<EGT> is k_eloss with EGT labellings per LDS group: 8 up to n = 8192, 4 up to 16384, 2 up to 32767 (128 KiB).
// RC_ELOSS_GROUP (read at every call) lowers the group size for the tests; T is an integer sum, so every size gives k_eloss's.

namespace hcl {

constexpr int BLK = 32;                  // rows per block of the second level: one mask word, one thread

struct ArgsL {
    Args a;                              // k_hclust's; val0 is not used
    unsigned long long *val;             // the row caches' values: k_hclust_init's output, whole blocks allocated
};

struct CarveL {
    int nb;
    size_t part, sz, rescan, dirty, total;
    __host__ __device__ explicit CarveL(int n)
    {
        nb = (n + BLK - 1) / BLK;
        part = 0;
        sz = part + 2 * (size_t)nb * BLK;
        rescan = sz + 2 * (size_t)nb * BLK;
        dirty = rescan + 4 * (size_t)nb;
        total = (dirty + (size_t)nb + 15) / 16 * 16;
    }
};

__device__ inline unsigned u16_at(const uint4 &q, int i)
{
    const unsigned w = (i >> 1) == 0 ? q.x : (i >> 1) == 1 ? q.y : (i >> 1) == 2 ? q.z : q.w;
    return (i & 1) ? w >> 16 : w & 0xFFFFu;
}

// the best candidate among rows 32k..32k+31: what step (A) of k_hclust offers for them
template <int LINK>
__device__ inline Cand block_scan(const unsigned long long *val, const unsigned short *part, const unsigned short *sz, int k)
{
    Cand best{0ull, 1u, ~0u};
    const int r0 = k * BLK;
#pragma unroll
    for (int h = 0; h < BLK; h += 8) {
        ulonglong2 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = reinterpret_cast<const ulonglong2 *>(val + r0 + h)[i];
        const uint4 p4 = *reinterpret_cast<const uint4 *>(part + r0 + h), s4 = *reinterpret_cast<const uint4 *>(sz + r0 + h);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned p = u16_at(p4, i), s = u16_at(s4, i);
            if (!s || p == NONE) continue;                              // (the pad rows of the last block have size 0)
            const Cand x{(i & 1) ? v[i >> 1].y : v[i >> 1].x, LINK ? 1u : s * (unsigned)sz[p], (unsigned)(r0 + h + i)};
            if (better<LINK>(x, best)) best = x;
        }
    }
    return best;
}

template <int LINK>
__global__ __launch_bounds__(TPB) void k_hclust_large(ArgsL AL)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char hcll_lds[];
    __shared__ unsigned long long r_num[NWAVE];
    __shared__ unsigned r_den[NWAVE], r_idx[NWAVE];
    __shared__ unsigned long long a_num[NWAVE];                        // row a's new cache, per wave
    __shared__ unsigned a_den[NWAVE], a_idx[NWAVE];

    const Args &A = AL.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n;
    const size_t ld = (size_t)n;
    unsigned long long *S = A.S;
    unsigned *M = A.M;
    unsigned long long *val = AL.val;

    const CarveL cv(n);
    const int nb = cv.nb, npad = nb * BLK;
    unsigned short *part = reinterpret_cast<unsigned short *>(hcll_lds + cv.part);
    unsigned short *sz = reinterpret_cast<unsigned short *>(hcll_lds + cv.sz);
    unsigned *rescan = reinterpret_cast<unsigned *>(hcll_lds + cv.rescan);
    unsigned char *dirty = hcll_lds + cv.dirty;

    for (int r = tid; r < npad; r += TPB) {
        part[r] = r < n ? A.part0[r] : (unsigned short)NONE;
        sz[r] = r < n ? 1 : 0;
    }
    for (int k = tid; k < nb; k += TPB) { rescan[k] = 0; dirty[k] = 1; }
    long long num = (long long)*A.tot;                                 // the Binder numerator of the current partition (thread 0's)
    if (tid == 0) A.bnum[0] = num;
    Cand blk{0ull, 1u, ~0u};                                           // the best of block tid, kept up by this thread alone
    __syncthreads();

    for (int t = 1; t < n; ++t) {
        // (A) the closest pair: every block offers its best row; a dirty block finds it again first
        if (tid < nb && dirty[tid]) {
            dirty[tid] = 0;
            blk = block_scan<LINK>(val, part, sz, tid);
        }
        Cand best = wave_best<LINK>(blk);
        if (lane == 0) { r_num[wave] = best.num; r_den[wave] = best.den; r_idx[wave] = best.idx; }
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
        // (B) row b into row a, mirrored into column a; the owner of column c repairs row c's cache
        Cand ra{0ull, 1u, ~0u};
        for (int c0 = tid; c0 < n; c0 += U * TPB) {
            unsigned long long sa[U], sb[U], vc[U];
            unsigned xa[U], xb[U], scs[U], pc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + u * TPB;
                scs[u] = (c < n && c != a && c != b) ? (unsigned)sz[c] : 0u;
                if (!scs[u]) continue;
                sa[u] = S[(size_t)a * ld + c];
                sb[u] = S[(size_t)b * ld + c];
                if (LINK) { xa[u] = M[(size_t)a * ld + c]; xb[u] = M[(size_t)b * ld + c]; }
                pc[u] = c < b ? (unsigned)part[c] : NONE;
                if (c < a && pc[u] != (unsigned)a && pc[u] != (unsigned)b) vc[u] = val[c];
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
                const unsigned p = pc[u];
                if (p == (unsigned)b || p == (unsigned)a) {
                    atomicOr(&rescan[c >> 5], 1u << (c & 31));          // its cached entry is gone (b) or has changed (a)
                    dirty[c >> 5] = 1;
                } else if (c < a) {
                    const Cand x{v, LINK ? 1u : sc_ * newsz, (unsigned)a}, cur{vc[u], LINK ? 1u : sc_ * (unsigned)sz[p], p};
                    if (better<LINK>(x, cur)) { val[c] = v; part[c] = (unsigned short)a; dirty[c >> 5] = 1; }
                }
            }
        }
        ra = wave_best<LINK>(ra);
        if (lane == 0) { a_num[wave] = ra.num; a_den[wave] = ra.den; a_idx[wave] = ra.idx; }
        __syncthreads();
        // (C) rescans; sz[a] and sz[b] are being rewritten, so their new values come from registers
        if (tid == 0) { sz[a] = (unsigned short)newsz; sz[b] = 0; dirty[a >> 5] = 1; dirty[b >> 5] = 1; }
        if (wave == NWAVE - 1) {
            ra = block_best<LINK>(a_num, a_den, a_idx, lane);
            if (lane == 0) { val[a] = ra.num; part[a] = (unsigned short)(ra.idx == ~0u ? NONE : ra.idx); }
        }
        const int j = lane * NWAVE + wave;                              // this lane's mask word: read and cleared by it alone
        const unsigned word = j < nb ? rescan[j] : 0u;
        if (word) rescan[j] = 0;
        for (unsigned long long nz = __ballot(word != 0); nz; nz &= nz - 1) {
            const int src = __ffsll((long long)nz) - 1;
            const int rbase = (src * NWAVE + wave) * BLK;
            for (unsigned wd = (unsigned)__shfl((int)word, src); wd; wd &= wd - 1) {
                const int r = rbase + __ffs((int)wd) - 1;
                const unsigned szr = sz[r];                               // (a marked row is neither a nor b)
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
        }
        __syncthreads();
    }
}

// T[l][i] = Σ_{j: lab_l[j] = lab_l[i]} C_ij for the labellings l of one group of EGT (blockIdx.x); one wave per row i
template <int EGT>
__global__ __launch_bounds__(TPB) void k_eloss_large(const unsigned *__restrict__ C, size_t ldc, int n, const unsigned short *__restrict__ labs,
                                                     int L, unsigned *__restrict__ T)
{
    extern __shared__ unsigned short ell_lab[];                         // G × n
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = blockIdx.x * EGT, G = min(EGT, L - g0);
    for (int k = tid; k < G * n; k += TPB) ell_lab[k] = labs[(size_t)g0 * n + k];
    __syncthreads();
    for (int i = blockIdx.y * NWAVE + wave; i < n; i += gridDim.y * NWAVE) {
        unsigned li[EGT], acc[EGT];
#pragma unroll
        for (int g = 0; g < EGT; ++g) { li[g] = g < G ? (unsigned)ell_lab[g * n + i] : 0u; acc[g] = 0; }
        for (int j = lane; j < n; j += 64) {
            const unsigned v = C[(size_t)i * ldc + j];
#pragma unroll
            for (int g = 0; g < EGT; ++g)
                if (g < G && ell_lab[g * n + j] == li[g]) acc[g] += v;
        }
#pragma unroll
        for (int g = 0; g < EGT; ++g) {
            unsigned s = acc[g];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += (unsigned)__shfl_xor((int)s, off);
            if (lane == 0 && g < G) T[(size_t)(g0 + g) * n + i] = s;
        }
    }
}

// ---- host side: the two launches hclust.inc.hip's run() and eloss_T() make for the large entry points

template <int LINK>
static hipError_t launch_large_as(const unsigned *dC, int64_t ldc, hipStream_t st, unsigned long long *d_val, unsigned short *d_part0, const Args &A)
{
    const size_t lds = CarveL(A.n).total;
    const hipError_t e = set_dynamic_lds(k_hclust_large<LINK>, lds);
    if (e != hipSuccess) return e;
    k_hclust_init<LINK><<<(unsigned)A.n, 256, 0, st>>>(dC, (size_t)ldc, A.n, A.S, A.M, d_val, d_part0);
    k_hclust_large<LINK><<<1, TPB, lds, st>>>(ArgsL{A, d_val});
    return hipGetLastError();
}

static hipError_t launch_large(int32_t linkage, const unsigned *dC, int64_t ldc, hipStream_t st, unsigned long long *d_val, unsigned short *d_part0,
                               const Args &A)
{
    return linkage == RC_HCLUST_AVERAGE    ? launch_large_as<RC_HCLUST_AVERAGE>(dC, ldc, st, d_val, d_part0, A)
           : linkage == RC_HCLUST_COMPLETE ? launch_large_as<RC_HCLUST_COMPLETE>(dC, ldc, st, d_val, d_part0, A)
                                           : launch_large_as<RC_HCLUST_SINGLE>(dC, ldc, st, d_val, d_part0, A);
}

template <int EGT>
static hipError_t launch_eloss_as(hipStream_t st, const unsigned *dC, int64_t ldc, int64_t n, const unsigned short *d_lab, int64_t L, unsigned *d_T)
{
    const size_t lds = (size_t)std::min<int64_t>(EGT, L) * (size_t)n * 2;
    const hipError_t e = set_dynamic_lds(k_eloss_large<EGT>, lds);
    if (e != hipSuccess) return e;
    k_eloss_large<EGT><<<dim3((unsigned)((L + EGT - 1) / EGT), (unsigned)std::min<int64_t>((n + NWAVE - 1) / NWAVE, 256)), TPB, lds, st>>>(
        dC, (size_t)ldc, (int)n, d_lab, (int)L, d_T);
    return hipGetLastError();
}

// The group size: the power of two whose labellings fit 128 KiB — 8, 4 or 2 — or, for the tests, the largest power of two that
// is neither above it nor above RC_ELOSS_GROUP.
static hipError_t launch_eloss_large(hipStream_t st, const unsigned *dC, int64_t ldc, int64_t n, const unsigned short *d_lab, int64_t L, unsigned *d_T)
{
    int eg = n <= 8192 ? 8 : n <= 16384 ? 4 : 2;
    if (const long long v = env_int("RC_ELOSS_GROUP"); v >= 1)
        while (eg > v) eg >>= 1;
    return eg == 8   ? launch_eloss_as<8>(st, dC, ldc, n, d_lab, L, d_T)
           : eg == 4 ? launch_eloss_as<4>(st, dC, ldc, n, d_lab, L, d_T)
           : eg == 2 ? launch_eloss_as<2>(st, dC, ldc, n, d_lab, L, d_T)
                     : launch_eloss_as<1>(st, dC, ldc, n, d_lab, L, d_T);
}

}  // namespace hcl

extern "C" int32_t rc_hclust_large(int32_t device, const void *counts, int64_t m, int64_t n, int32_t linkage, void *merges_out,
                                   int64_t *binder_num, int32_t maxcut, double *vilb, double *kernel_ms)
{
    return hcl::dendrogram("rc_hclust_large", cnt::host_counts(device, counts, m, n), linkage, merges_out, binder_num, maxcut, vilb, kernel_ms,
                           true);
}

extern "C" int32_t rc_hclust_large_samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t linkage, void *merges_out,
                                           int64_t *binder_num, int32_t maxcut, double *vilb, double *kernel_ms, double *counts_ms)
{
    return hcl::dendrogram("rc_hclust_large_samples", cnt::samples(device, samples, m, n, counts_ms), linkage, merges_out, binder_num, maxcut,
                           vilb, kernel_ms, true);
}

extern "C" int32_t rc_hclust_large_ctx(rc_ctx *c, int64_t numsamples, int32_t linkage, void *merges_out, int64_t *binder_num, int32_t maxcut,
                                       double *vilb, double *kernel_ms)
{
    return hcl::dendrogram("rc_hclust_large_ctx", cnt::context(c, numsamples), linkage, merges_out, binder_num, maxcut, vilb, kernel_ms, true);
}

extern "C" int32_t rc_hclust_cut_large(const void *merges, int64_t n, int64_t K, int64_t *labels_out)
{
    return hcl::cut("rc_hclust_cut_large", hcl::LARGE_NMAX, merges, n, K, labels_out);
}

extern "C" int32_t rc_psm_expected_loss_large(int32_t device, const void *counts, int64_t m, int64_t n, int32_t loss, int64_t L,
                                              const int64_t *labels, double *loss_out, int64_t *num_out, double *kernel_ms)
{
    return hcl::expected_loss("rc_psm_expected_loss_large", cnt::host_counts(device, counts, m, n), loss, L, labels, loss_out, num_out,
                              kernel_ms, true);
}

extern "C" int32_t rc_psm_expected_loss_large_ctx(rc_ctx *c, int64_t numsamples, int32_t loss, int64_t L, const int64_t *labels,
                                                  double *loss_out, int64_t *num_out, double *kernel_ms)
{
    return hcl::expected_loss("rc_psm_expected_loss_large_ctx", cnt::context(c, numsamples), loss, L, labels, loss_out, num_out, kernel_ms, true);
}

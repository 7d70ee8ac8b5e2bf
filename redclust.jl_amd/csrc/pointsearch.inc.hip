// Point-estimate search on the device: a greedy search over ALL partitions for the clustering of minimum expected loss
// under the posterior co-clustering counts C (n×n uint32, C_ii = m = number of samples) — the step the reference's
// docs/src/index.md §"Point estimation" sends its users to R's SALSO for; getpointestimate(method = "MPEL")
// (src/pointestimate.jl:49-58 of the reference) only ever looks at the clusterings the chain visited.
// Included at the end of redclust_hip.hip (same translation unit: shares fail(), HIPCHK, rc_ctx, the error buffer and the
// holders of hostutil.inc.hip).
//
// Criterion (DESIGN.md §8 "Point-estimate search"):
//   Binder   num(c) = Σ_{i<j} C_ij + Σ_{i<j, c_i=c_j} (m − 2·C_ij)                 loss = num / (m·n(n−1)/2)   exact integers
//   VI bound f(c)   = Σ_i [log n_{c_i} − 2·log T_i],  T_i = Σ_{j: c_j=c_i} C_ij      loss = f/n + 2·log m
//
// One run = one workgroup of 1024 threads, persistent over its sweeps; nruns workgroups per launch.  A step visits one
// point i (the order is fixed in advance), takes it out of its cluster, reduces row i of C into per-cluster sums with
// integer LDS atomics, scores every candidate cluster, takes the argmin across the group and puts i there.  Two
// barriers per step.  Row order[t+1] is loaded into registers before step t's barriers — the only long latency.
//
// State in LDS (n ≤ 8192; RC_ERR_CAPACITY beyond):
//   lab  u16[n]     slot of every point, 0 = unallocated (slots are the caller's labels 1..n)
//   sz   u16[n+2]   members of every slot
//   T    u32[n]     VI only: T_j above (m·n < 2^31 is checked)
//   S    u32[W]     accumulator: S_ik = Σ_{j∈k, j≠i} C_ij
//   L    u64[W]     VI only: Σ_{j∈k} log((T_j + C_ij)/T_j) in units of 2^-40 — each term is rounded once to that quantum and
//                   added with an integer atomic, so the sum does not depend on the order the lanes arrive in
// W = n + 1 slots when that fits the 160 KiB (always for Binder; VI up to n = 8104); otherwise the occupied slot range
// 1..hi is covered in passes of W slots (VI, n > 8104, and only while a slot above W is or has been in use).
//
// Ties: lower score first; among equal scores the point's own slot (it does not move), then the lowest slot.  A new
// cluster takes the slot the point just emptied if it emptied one, else the lowest free slot.

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace psm {

constexpr int TPB = 1024;
constexpr int NWAVE = TPB / 64;
constexpr int NMAX = 8192;
constexpr double QUANT = 1099511627776.0;            // 2^40
constexpr size_t LDS_BUDGET = 160 * 1024 - 1024;     // dynamic part; the static reduction scratch is below 1 KiB

struct RunOut {
    long long tot, same, moves;   // Binder: Σ_{i<j} C_ij and Σ_{i<j, same cluster} C_ij of the final labelling
    double f;                     // VI: f(c)
    int sweeps, converged, K, pad_;
};

struct Args {
    const unsigned *C;            // n × ld counts
    long long ld;
    const unsigned short *init;   // nruns × n slots, 0 = unallocated
    const unsigned short *sz0;    // nruns × (n + 2) slot sizes of init
    const int *K0, *hi0;          // clusters / highest used slot of init
    const int *order;             // nruns × n, 0-based
    unsigned short *labels;       // nruns × n out (slots)
    RunOut *out;
    int n, W, maxK, maxsweeps;
    unsigned m;
};

// (score, priority) pairs compare lexicographically; scores are mapped to u64 so that one reduction serves both losses
__device__ inline unsigned long long key_i64(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }
__device__ inline unsigned long long key_f64(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);   // (−0 + 0 = +0)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct Cand { unsigned long long sc; unsigned pr, slot, S; };

__device__ inline bool better(unsigned long long sc, unsigned pr, const Cand &b) { return sc < b.sc || (sc == b.sc && pr < b.pr); }

__device__ inline unsigned long long shfl_xor_u64(unsigned long long v, int off)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

template <int Q>
__device__ inline void load_row(const unsigned *__restrict__ row, int n, int tid, unsigned (&r)[Q])
{
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = tid + q * TPB;
        r[q] = (j < n) ? row[j] : 0u;
    }
}

// counts must be symmetric with diagonal m and no entry above m; flag bits: 1 diagonal, 2 symmetry, 4 range
__global__ __launch_bounds__(256) void k_check(const unsigned *__restrict__ C, long long ld, int n, unsigned m, unsigned *flag)
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

// k_check on the device counts (n × ld), with its flags turned into RC_ERR_ARG messages that start with `who`
static int32_t check_counts(rc_ctx *c, hipStream_t st, const char *who, const unsigned *dC, int64_t ld, int64_t m, int64_t n)
{
    DeviceBuffers B;
    unsigned *d_flag;
    HIPCHK(c, B.alloc(d_flag, 1));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, sizeof(unsigned), st));
    k_check<<<dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8), (unsigned)n), 256, 0, st>>>(dC, ld, (int)n, (unsigned)m, d_flag);
    HIPCHK(c, hipGetLastError());
    unsigned flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (flag & 1u) return fail(c, RC_ERR_ARG, "%s: the diagonal of the counts is not m = %lld everywhere", who, (long long)m);
    if (flag & 2u) return fail(c, RC_ERR_ARG, "%s: the counts are not symmetric", who);
    if (flag & 4u) return fail(c, RC_ERR_ARG, "%s: a count exceeds m = %lld", who, (long long)m);
    return RC_OK;
}

template <int LOSS, int Q>
__global__ __launch_bounds__(TPB) void k_search(Args A)
{
    constexpr bool VI = LOSS == RC_PSM_VILB;
    extern __shared__ unsigned long long psm_lds[];
    __shared__ unsigned long long r_sc[NWAVE];
    __shared__ unsigned r_pr[NWAVE], r_slot[NWAVE], r_S[NWAVE], r_free[NWAVE];
    __shared__ double r_f[NWAVE];
    __shared__ unsigned long long r_a[NWAVE], r_b[NWAVE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, W = A.W, run = blockIdx.x;
    const unsigned m = A.m;
    const unsigned *__restrict__ C = A.C;
    const size_t ld = (size_t)A.ld;

    // carve the dynamic LDS: 8-byte items first
    unsigned long long *L = psm_lds;
    unsigned *S = reinterpret_cast<unsigned *>(L + (VI ? W : 0));
    unsigned *T = S + W;
    unsigned short *sz = reinterpret_cast<unsigned short *>(T + (VI ? n : 0));
    unsigned short *lab = sz + (n + 2);

    for (int k = tid; k < W; k += TPB) { S[k] = 0; if (VI) L[k] = 0; }
    for (int k = tid; k < n + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (n + 2) + k];
    for (int j = tid; j < n; j += TPB) lab[j] = A.init[(size_t)run * n + j];
    __syncthreads();
    if (VI) {
        // T_j of the starting labels: one wave per allocated row
        for (int j = wave; j < n; j += NWAVE) {
            const unsigned l = lab[j];
            if (!l) continue;                                           // wave-uniform
            unsigned s = 0;
            for (int c = lane; c < n; c += 64)
                if (lab[c] == l) s += C[(size_t)j * ld + c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += (unsigned)__shfl_xor((int)s, off);
            if (lane == 0) T[j] = s;
        }
        __syncthreads();
    }

    const int *__restrict__ ord = A.order + (size_t)run * n;
    int K = A.K0[run], hi = A.hi0[run];
    int i = ord[0], i1 = ord[n > 1 ? 1 : 0];
    int iprev = -1;
    unsigned wprev = 0;
    unsigned cur[Q], nxt[Q];
    load_row<Q>(C + (size_t)i * ld, n, tid, cur);
    long long moves = 0;
    int sweeps = 0, converged = 0;
    const double dnew = VI ? -2.0 * log((double)m) : 0.0;
    const unsigned long long key_new = VI ? key_f64(dnew) : key_i64(0);

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            // the next row: issued now, consumed in the next step
            const int inext = i1;
            {
                int t2 = t + 2;
                if (t2 >= n) t2 -= n;
                if (t2 >= n) t2 -= n;
                i1 = ord[t2];
            }
            load_row<Q>(C + (size_t)inext * ld, n, tid, nxt);

            // lab[i] was written by another thread without a barrier in between only if i is the previous point (n = 1)
            const unsigned a = (i == iprev) ? wprev : (unsigned)lab[i];
            const int scan_hi = min(hi + 1, n);                          // slots above hi are free; hi + 1 is the lowest of them
            Cand best{~0ull, ~0u, 0u, 0u};
            unsigned minfree = ~0u;
            unsigned emptied = 0;
            for (int base = 0, pass = 0; base < scan_hi; base += W, ++pass) {
                // phase A: row i into the per-slot accumulators of this window; the first pass also takes i out of T
                if (pass) __syncthreads();
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int j = tid + q * TPB;
                    if (j >= n || j == i) continue;
                    const unsigned l = lab[j];
                    if (!l) continue;
                    const unsigned c = cur[q];
                    unsigned Tj = 0;
                    if (VI) {
                        Tj = T[j];
                        if (pass == 0 && l == a) { Tj -= c; T[j] = Tj; }
                    }
                    const unsigned idx = l - 1u - (unsigned)base;
                    if (idx < (unsigned)W && c) {
                        atomicAdd(&S[idx], c);
                        if (VI) atomicAdd(&L[idx], __double2ull_rn(log1p((double)c / (double)Tj) * QUANT));
                    }
                }
                __syncthreads();
                // phase B: score the slots of this window (and clear their accumulators)
                emptied = (a && sz[a] == 1) ? 1u : 0u;
                const int kend = min(base + W, scan_hi);
                for (int k = base + 1 + tid; k <= kend; k += TPB) {
                    const int nk = (int)sz[k] - ((unsigned)k == a ? 1 : 0);
                    if (nk <= 0) { minfree = min(minfree, (unsigned)k); continue; }
                    const int idx = k - 1 - base;
                    const unsigned s = S[idx];
                    S[idx] = 0;
                    unsigned long long sc;
                    if (VI) {
                        const double ls = (double)L[idx] * (1.0 / QUANT);
                        L[idx] = 0;
                        const double d = (double)(nk + 1) * log((double)(nk + 1)) - (double)nk * log((double)nk) - 2.0 * ls -
                                         2.0 * log((double)s + (double)m);
                        sc = key_f64(d);
                    } else {
                        sc = key_i64((long long)m * nk - 2ll * (long long)s);
                    }
                    const unsigned pr = ((unsigned)k == a) ? 0u : (unsigned)k;
                    if (better(sc, pr, best)) best = Cand{sc, pr, (unsigned)k, s};
                }
            }
            // argmin across the group
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long osc = shfl_xor_u64(best.sc, off);
                const unsigned opr = (unsigned)__shfl_xor((int)best.pr, off), oslot = (unsigned)__shfl_xor((int)best.slot, off);
                const unsigned oS = (unsigned)__shfl_xor((int)best.S, off);
                if (better(osc, opr, best)) best = Cand{osc, opr, oslot, oS};
                minfree = min(minfree, (unsigned)__shfl_xor((int)minfree, off));
            }
            if (lane == 0) { r_sc[wave] = best.sc; r_pr[wave] = best.pr; r_slot[wave] = best.slot; r_S[wave] = best.S; r_free[wave] = minfree; }
            __syncthreads();
            best = Cand{r_sc[0], r_pr[0], r_slot[0], r_S[0]};
            minfree = r_free[0];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) {
                if (better(r_sc[w], r_pr[w], best)) best = Cand{r_sc[w], r_pr[w], r_slot[w], r_S[w]};
                minfree = min(minfree, r_free[w]);
            }
            // the new-cluster candidate
            const int Know = K - (int)emptied;
            unsigned isnew = 0;
            if (A.maxK == 0 || Know < A.maxK) {
                const unsigned slot = emptied ? a : minfree;
                const unsigned pr = emptied ? 0u : minfree;
                if (better(key_new, pr, best)) { best = Cand{key_new, pr, slot, 0u}; isnew = 1; }
            }
            const unsigned w = best.slot;
            // phase C: put i into w.  Per-point entries are written by the thread that owns them, sz by the owner of i;
            // the next step reads sz only behind its first barrier
            if (VI) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int j = tid + q * TPB;
                    if (j < n && j != i && lab[j] == w) T[j] += cur[q];
                }
            }
            if (tid == (i & (TPB - 1))) {
                lab[i] = (unsigned short)w;
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
                if (VI) T[i] = best.S + m;
            }
            moved += (a == 0 || w != a) ? 1 : 0;
            K = Know + (int)isnew;
            hi = max(hi, (int)w);
            iprev = i; wprev = w;
            i = inext;
#pragma unroll
            for (int q = 0; q < Q; ++q) cur[q] = nxt[q];
        }
        ++sweeps;
        moves += moved;
        if (!moved) { converged = 1; break; }
        if (sweeps >= A.maxsweeps) break;
    }
    __syncthreads();

    for (int j = tid; j < n; j += TPB) A.labels[(size_t)run * n + j] = lab[j];
    double f = 0.0;
    unsigned long long tot = 0, same = 0;
    if (VI) {
        // f in one fixed order: per thread ascending j, xor tree over the wave, waves in ascending order
        for (int j = tid; j < n; j += TPB) {
            const unsigned l = lab[j];
            if (l) f += log((double)sz[l]) - 2.0 * log((double)T[j]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) f += __shfl_xor(f, off);
        if (lane == 0) r_f[wave] = f;
    } else {
        // the Binder numerator's two sums over the upper triangle: one wave per row, 16-byte loads (ld is a multiple of 4)
        for (int r = wave; r < n; r += NWAVE) {
            const unsigned lr = lab[r];
            const uint4 *row = reinterpret_cast<const uint4 *>(C + (size_t)r * ld);
            for (int j = (((r + 1) >> 8) << 8) + 4 * lane; j < n; j += 256) {
                const uint4 v = row[j >> 2];
                const unsigned x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int jj = j + e;
                    if (jj > r && jj < n) {
                        tot += x[e];
                        if (lab[jj] == lr) same += x[e];
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { tot += shfl_xor_u64(tot, off); same += shfl_xor_u64(same, off); }
        if (lane == 0) { r_a[wave] = tot; r_b[wave] = same; }
    }
    __syncthreads();
    if (tid == 0) {
        RunOut o{};
        if (VI) {
            double s = 0.0;
            for (int w = 0; w < NWAVE; ++w) s += r_f[w];
            o.f = s;
        } else {
            unsigned long long ta = 0, tb = 0;
            for (int w = 0; w < NWAVE; ++w) { ta += r_a[w]; tb += r_b[w]; }
            o.tot = (long long)ta; o.same = (long long)tb;
        }
        o.moves = moves; o.sweeps = sweeps; o.converged = converged; o.K = K;
        A.out[run] = o;
    }
}

template <int LOSS>
static hipError_t launch(int Q, int nruns, size_t lds, hipStream_t st, const Args &A)
{
#define PSM_LAUNCH(QQ)                                                                                                    \
    do {                                                                                                                  \
        hipError_t e = hipFuncSetAttribute((const void *)k_search<LOSS, QQ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                                    \
        k_search<LOSS, QQ><<<nruns, TPB, lds, st>>>(A);                                                                   \
    } while (0)
    if (Q <= 1) PSM_LAUNCH(1);
    else if (Q <= 2) PSM_LAUNCH(2);
    else if (Q <= 4) PSM_LAUNCH(4);
    else PSM_LAUNCH(8);
#undef PSM_LAUNCH
    return hipGetLastError();
}

// Everything behind the two entry points.  c may be NULL (errors then go to the thread's buffer); dC is the device
// count matrix (n × ld, ld a multiple of 4, rows 16-byte aligned), read in place.
static int32_t run(rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ld, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                   const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                   rc_psm_run_t *runs_out, int32_t *best, double *kernel_ms)
{
    // ---- the caller's runs: labels in 0..n, orders permutations of 1..n, cluster counts within maxK
    std::vector<unsigned short> h_init((size_t)nruns * n), h_sz((size_t)nruns * (n + 2), 0);
    std::vector<int> h_K((size_t)nruns), h_hi((size_t)nruns), h_ord((size_t)nruns * n);
    std::vector<char> seen((size_t)n);
    for (int r = 0; r < nruns; ++r) {
        unsigned short *szr = h_sz.data() + (size_t)r * (n + 2);
        int K = 0, hi = 0;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t l = init[(size_t)r * n + j];
            if (l < 0 || l > n) return fail(c, RC_ERR_ARG, "point search: label %lld of run %d outside 0..n", (long long)l, r + 1);
            h_init[(size_t)r * n + j] = (unsigned short)l;
            if (l) { if (szr[l]++ == 0) ++K; hi = std::max(hi, (int)l); }
        }
        if (maxK > 0 && K > maxK) return fail(c, RC_ERR_ARG, "point search: run %d starts with %d clusters, more than maxK = %d", r + 1, K, maxK);
        h_K[(size_t)r] = K; h_hi[(size_t)r] = hi;
        std::fill(seen.begin(), seen.end(), 0);
        for (int64_t t = 0; t < n; ++t) {
            const int32_t o = order[(size_t)r * n + t];
            if (o < 1 || o > n || seen[(size_t)o - 1]) return fail(c, RC_ERR_ARG, "point search: the order of run %d is not a permutation of 1..n", r + 1);
            seen[(size_t)o - 1] = 1;
            h_ord[(size_t)r * n + t] = o - 1;
        }
    }
    // ---- the counts: symmetric, diagonal m, nothing above m
    const int32_t crc = check_counts(c, st, "point search", dC, ld, m, n);
    if (crc != RC_OK) return crc;
    DeviceBuffers B;

    // ---- geometry
    const bool vi = loss == RC_PSM_VILB;
    const size_t fixed = (vi ? 4 * (size_t)n : 0) + 2 * (size_t)(n + 2) + 2 * (size_t)n + 16;
    const size_t per_slot = vi ? 12 : 4;
    int64_t W = std::min<int64_t>(n + 1, (int64_t)((LDS_BUDGET - fixed) / per_slot));
    if (const long long v = env_int("RC_PSM_WINDOW"); v >= 1 && v < W) W = v;   // tests: force the windowed passes at small n
    const size_t lds = (fixed + per_slot * (size_t)W + 15) / 16 * 16;

    unsigned short *d_init, *d_sz, *d_lab; int *d_K, *d_hi, *d_ord; RunOut *d_out;
    HIPCHK(c, B.alloc(d_init, h_init.size()));
    HIPCHK(c, B.alloc(d_sz, h_sz.size()));
    HIPCHK(c, B.alloc(d_K, h_K.size()));
    HIPCHK(c, B.alloc(d_hi, h_hi.size()));
    HIPCHK(c, B.alloc(d_ord, h_ord.size()));
    HIPCHK(c, B.alloc(d_lab, h_init.size()));
    HIPCHK(c, B.alloc(d_out, (size_t)nruns));
    HIPCHK(c, hipMemcpyAsync(d_init, h_init.data(), h_init.size() * 2, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_sz, h_sz.data(), h_sz.size() * 2, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_K, h_K.data(), h_K.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_hi, h_hi.data(), h_hi.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(d_ord, h_ord.data(), h_ord.size() * 4, hipMemcpyHostToDevice, st));

    Args A{};
    A.C = dC; A.ld = ld; A.init = d_init; A.sz0 = d_sz; A.K0 = d_K; A.hi0 = d_hi; A.order = d_ord; A.labels = d_lab; A.out = d_out;
    A.n = (int)n; A.W = (int)W; A.maxK = maxK; A.maxsweeps = maxsweeps; A.m = (unsigned)m;
    TimingEvents ev;
    HIPCHK(c, ev.create());
    HIPCHK(c, ev.begin(st));
    const int Q = (int)((n + TPB - 1) / TPB);
    const hipError_t le = vi ? launch<RC_PSM_VILB>(Q, nruns, lds, st, A) : launch<RC_PSM_BINDER>(Q, nruns, lds, st, A);
    if (le != hipSuccess) return fail(c, RC_ERR_HIP, "point search: launch failed: %s", hipGetErrorString(le));
    HIPCHK(c, ev.end(st));
    std::vector<unsigned short> h_lab(h_init.size());
    std::vector<RunOut> h_out((size_t)nruns);
    HIPCHK(c, hipMemcpyAsync(h_lab.data(), d_lab, h_lab.size() * 2, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_out.data(), d_out, h_out.size() * sizeof(RunOut), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    double ms = 0.0;
    HIPCHK(c, ev.elapsed_ms(ms));
    if (kernel_ms) *kernel_ms = ms;

    // ---- results: sortlabels (utils.jl:69-74), the losses, the first minimum
    const long long pairs = (long long)n * (n - 1) / 2;
    std::vector<int> map((size_t)n + 1), cnt((size_t)n + 1);
    int b = 0;
    for (int r = 0; r < nruns; ++r) {
        std::fill(map.begin(), map.end(), 0);
        std::fill(cnt.begin(), cnt.end(), 0);
        int next = 0;
        for (int64_t j = 0; j < n; ++j) {
            const unsigned short l = h_lab[(size_t)r * n + j];
            if (!map[l]) map[l] = ++next;
            labels_out[(size_t)r * n + j] = map[l];
            cnt[(size_t)map[l]]++;
        }
        const RunOut &o = h_out[(size_t)r];
        rc_psm_run_t &R = runs_out[r];
        R.sweeps = o.sweeps; R.converged = o.converged; R.moves = o.moves; R.K = o.K;
        if (vi) {
            R.loss_num = 0;
            R.loss = o.f / (double)n + 2.0 * std::log((double)m);
        } else {
            long long within = 0;
            for (int k = 1; k <= next; ++k) within += (long long)cnt[(size_t)k] * (cnt[(size_t)k] - 1) / 2;
            R.loss_num = o.tot + (long long)m * within - 2 * o.same;
            R.loss = pairs ? (double)R.loss_num / (double)((long long)m * pairs) : 0.0;
        }
        if (R.loss < runs_out[b].loss) b = r;
    }
    *best = b;
    return RC_OK;
}

static int32_t check_args(rc_ctx *c, const char *who, int64_t m, int64_t n, int32_t loss, int32_t nruns, const int64_t *init,
                          const int32_t *order, int32_t maxK, int32_t maxsweeps, const int64_t *labels_out, const void *runs_out,
                          const int32_t *best)
{
    if (!init || !order || !labels_out || !runs_out || !best) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    if (m < 1 || n < 1 || nruns < 1) return fail(c, RC_ERR_ARG, "%s: need m >= 1, n >= 1 and nruns >= 1 (got m=%lld n=%lld nruns=%d)", who, (long long)m, (long long)n, nruns);
    if (maxsweeps < 1 || maxK < 0) return fail(c, RC_ERR_ARG, "%s: need maxsweeps >= 1 and maxK >= 0 (got %d, %d)", who, maxsweeps, maxK);
    if (loss != RC_PSM_BINDER && loss != RC_PSM_VILB) return fail(c, RC_ERR_ARG, "%s: invalid loss specifier %d", who, loss);
    if (n > NMAX) return fail(c, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %d points whose state fits the workgroup's LDS", who, (long long)n, NMAX);
    if (m > 0x7FFFFFFFll / n) return fail(c, RC_ERR_CAPACITY, "%s: m*n does not fit 31 bits (m=%lld n=%lld)", who, (long long)m, (long long)n);
    return RC_OK;
}

}  // namespace psm

extern "C" int32_t rc_psm_search(int32_t device, const void *counts, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                                 const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                                 void *runs_out, int32_t *best, double *kernel_ms)
{
    if (!counts) return fail(nullptr, RC_ERR_ARG, "rc_psm_search: NULL argument");
    int32_t rc = psm::check_args(nullptr, "rc_psm_search", m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    rc = select_device("rc_psm_search", device);
    if (rc != RC_OK) return rc;
    const int64_t ld = (n + 3) / 4 * 4;
    DeviceBuffers B;
    unsigned *d_C;
    HIPCHK(nullptr, B.alloc(d_C, (size_t)n * ld));
    if (ld != n) HIPCHK(nullptr, hipMemset(d_C, 0, (size_t)n * ld * sizeof(unsigned)));
    HIPCHK(nullptr, hipMemcpy2D(d_C, (size_t)ld * sizeof(unsigned), counts, (size_t)n * sizeof(unsigned), (size_t)n * sizeof(unsigned), (size_t)n,
                      hipMemcpyHostToDevice));
    return psm::run(nullptr, nullptr, d_C, ld, m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out,
                    (rc_psm_run_t *)runs_out, best, kernel_ms);
}

extern "C" int32_t rc_psm_search_ctx(rc_ctx *c, int64_t numsamples, int32_t loss, int32_t nruns, const int64_t *init,
                                     const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                                     rc_psm_run_t *runs_out, int32_t *best, double *kernel_ms)
{
    if (!c) return fail(c, RC_ERR_ARG, "rc_psm_search_ctx: NULL ctx");
    int32_t rc = psm::check_args(c, "rc_psm_search_ctx", numsamples, c->n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    HIPCHK(c, hipSetDevice(c->dev));
    if (!c->counts) return fail(c, RC_ERR_STATE, "rc_psm_search_ctx: no sample has been recorded");
    rc = flush_counts(c);
    if (rc != RC_OK) return rc;
    rc = sync_and_check(c);
    if (rc != RC_OK) return rc;
    unsigned d0 = 0;
    HIPCHK(c, hipMemcpy(&d0, c->counts, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (d0 == 0) return fail(c, RC_ERR_STATE, "rc_psm_search_ctx: no sample has been recorded");
    // the count matrix is read in place (caller's point order, leading dimension ldc); nothing of the context is written
    return psm::run(c, c->sA, c->counts, c->ldc, numsamples, c->n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best,
                    kernel_ms);
}

// Point-estimate search on the device: a greedy search over ALL partitions for the clustering of minimum expected loss
// under the posterior co-clustering counts C (n×n uint32, C_ii = m = number of samples) — the step the reference's
// docs/src/index.md §"Point estimation" sends its users to R's SALSO for; getpointestimate(method = "MPEL")
// (src/pointestimate.jl:49-58 of the reference) only ever looks at the clusterings the chain visited.
// Included at the end of redclust_hip.hip behind samplecounts.inc.hip (same translation unit: shares fail(), HIPCHK, rc_ctx,
// the error buffer, the holders and the count-matrix checks of hostutil.inc.hip; cnt:: of samplecounts.inc.hip, which puts
// the counts of all three entry points — host counts, samples, a live context — on the device; and from greedy.inc.hip
// everything of the search that does not depend on the criterion: the order walk, the keys and the group argmin, the
// new-cluster candidate, and on the host the shared argument checks, the staging of the runs and the result loop).  What is
// here: the two scores and their state.
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
// Ties: greedy.inc.hip.
//
// PEAR (DESIGN.md §8 "PEAR search"; rc_pear_search*) is a third, internal instantiation of the same kernel: the criterion is
// the fraction num/den of include/redclust_hip.h, maximised.  Phase A is Binder's; besides S it sums row i over the point's own
// cluster (S_ia, one LDS word per step parity), which turns the run's X into X₀.  Phase B scores slot k as the pair (num_k, den_k)
// of (X₀ + S_ik, A₀ + n_k); the argmax is greedy::group_argmax.  X, A (of the current labelling) and P sit in front of S in LDS:
// X and A are written in phase C by the thread that writes sz and read behind the next step's first barrier; P = Σ_{i<j} C_ij
// and the X of the start come from one pass over the matrix before the first step, the reported X and P from one after the last.

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace psm {

using greedy::TPB, greedy::NWAVE, greedy::Cand, greedy::better, greedy::key_i64, greedy::key_f64, greedy::shfl_xor_u64;
constexpr double QUANT = 1099511627776.0;            // 2^40
constexpr size_t LDS_BUDGET = 160 * 1024 - 1024;     // dynamic part; the static reduction scratch is below 1 KiB
constexpr int LOSS_PEAR = 2;                         // k_search's third criterion; not a loss specifier of rc_psm_search
constexpr size_t PEAR_HEAD = 4;                      // u64 words in front of S: X, A, P and the two S_ia accumulators

struct RunOut {
    long long tot, same, moves;   // Binder, PEAR: Σ_{i<j} C_ij and Σ_{i<j, same cluster} C_ij of the final labelling
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

template <int Q>
__device__ inline void load_row(const unsigned *__restrict__ row, int n, int tid, unsigned (&r)[Q])
{
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int j = tid + q * TPB;
        r[q] = (j < n) ? row[j] : 0u;
    }
}

// This wave's share of Σ_{i<j} C_ij (tot) and Σ_{i<j, same cluster} C_ij (same) over the upper triangle: one wave per row,
// 16-byte loads (ld is a multiple of 4).  ZEROS: lab may hold 0 (unallocated: a cluster of its own)
template <bool ZEROS>
__device__ inline void upper_sums(const unsigned *__restrict__ C, size_t ld, int n, const unsigned short *lab, int lane, int wave,
                                  unsigned long long &tot, unsigned long long &same)
{
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
                    if (lab[jj] == lr && (!ZEROS || lr)) same += x[e];
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { tot += shfl_xor_u64(tot, off); same += shfl_xor_u64(same, off); }
}

template <int LOSS, int Q>
__global__ __launch_bounds__(TPB) void k_search(Args A)
{
    constexpr bool VI = LOSS == RC_PSM_VILB, PEAR = LOSS == LOSS_PEAR;
    extern __shared__ unsigned long long psm_lds[];
    __shared__ unsigned long long r_sc[NWAVE];
    __shared__ unsigned r_pr[NWAVE], r_slot[NWAVE], r_S[NWAVE], r_free[NWAVE];
    __shared__ double r_f[NWAVE];
    __shared__ unsigned long long r_a[NWAVE], r_b[NWAVE];
    __shared__ long long r_num[NWAVE], r_den[NWAVE];                     // PEAR's partials (not allocated where unused)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, W = A.W, run = blockIdx.x;
    const unsigned m = A.m;
    const unsigned *__restrict__ C = A.C;
    const size_t ld = (size_t)A.ld;

    // carve the dynamic LDS: 8-byte items first
    unsigned long long *L = psm_lds;
    long long *XA = reinterpret_cast<long long *>(psm_lds);              // PEAR: X, A, P
    unsigned *Sa = reinterpret_cast<unsigned *>(psm_lds + 3);            // PEAR: S_ia of the even and the odd steps
    unsigned *S = reinterpret_cast<unsigned *>(L + (VI ? (size_t)W : PEAR ? PEAR_HEAD : 0));
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

    long long Pall = 0;
    const long long Tall = (long long)n * (n - 1) / 2;
    if (PEAR) {
        // P, and X and A of the starting labels
        unsigned long long tot = 0, same = 0, within = 0;
        upper_sums<true>(C, ld, n, lab, lane, wave, tot, same);
        for (int k = 1 + tid; k <= n; k += TPB) within += (unsigned long long)sz[k] * (sz[k] - 1u) / 2u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) within += shfl_xor_u64(within, off);
        if (lane == 0) { r_a[wave] = tot; r_b[wave] = same; r_sc[wave] = within; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long ta = 0, tb = 0, tc = 0;
            for (int w = 0; w < NWAVE; ++w) { ta += r_a[w]; tb += r_b[w]; tc += r_sc[w]; }
            XA[0] = (long long)tb; XA[1] = (long long)tc; XA[2] = (long long)ta;
            Sa[0] = Sa[1] = 0;
        }
        __syncthreads();
        Pall = XA[2];
    }

    const greedy::Partials red{r_sc, r_pr, r_slot, r_free, r_S};
    greedy::Visit v(A.order + (size_t)run * n, n);
    int K = A.K0[run], hi = A.hi0[run];
    int par = 0;                                                         // PEAR: which S_ia accumulator this step adds to
    unsigned cur[Q], nxt[Q];
    load_row<Q>(C + (size_t)v.i * ld, n, tid, cur);
    long long moves = 0;
    int sweeps = 0, converged = 0;
    const double dnew = VI ? -2.0 * log((double)m) : 0.0;
    const unsigned long long key_new = VI ? key_f64(dnew) : key_i64(0);

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            // the next row: issued now, consumed in the next step
            const int i = v.i, inext = v.ahead(t);
            load_row<Q>(C + (size_t)inext * ld, n, tid, nxt);

            const unsigned a = v.slot_of(lab);
            const int scan_hi = min(hi + 1, n);                          // slots above hi are free; hi + 1 is the lowest of them
            Cand best{~0ull, ~0u, 0u, 0u};
            greedy::FCand fbest = greedy::FCAND_NONE;
            long long X0 = 0, A0 = 0;                                    // PEAR: X and A with i out
            unsigned minfree = ~0u;
            unsigned emptied = 0;
            for (int base = 0, pass = 0; base < scan_hi; base += W, ++pass) {
                // phase A: row i into the per-slot accumulators of this window; the first pass also takes i out of T
                if (pass) __syncthreads();
                unsigned sa = 0;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int j = tid + q * TPB;
                    if (j >= n || j == i) continue;
                    const unsigned l = lab[j];
                    if (!l) continue;
                    const unsigned c = cur[q];
                    if (PEAR && l == a) sa += c;
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
                if (PEAR && pass == 0 && sa) atomicAdd(&Sa[par], sa);
                __syncthreads();
                // phase B: score the slots of this window (and clear their accumulators)
                emptied = (a && sz[a] == 1) ? 1u : 0u;
                if (PEAR && pass == 0) {
                    X0 = XA[0] - (long long)Sa[par];
                    A0 = XA[1] - (a ? (long long)sz[a] - 1 : 0ll);
                }
                const int kend = min(base + W, scan_hi);
                for (int k = base + 1 + tid; k <= kend; k += TPB) {
                    const int nk = (int)sz[k] - ((unsigned)k == a ? 1 : 0);
                    if (nk <= 0) { minfree = min(minfree, (unsigned)k); continue; }
                    const int idx = k - 1 - base;
                    const unsigned s = S[idx];
                    S[idx] = 0;
                    const unsigned pr = ((unsigned)k == a) ? 0u : (unsigned)k;
                    if constexpr (PEAR) {
                        // (num_k, den_k) of X = X₀ + S_ik, A = A₀ + n_k: below 2^63 in magnitude while m·T² < 2^62
                        const long long Xk = X0 + (long long)s, Ak = A0 + nk;
                        const greedy::FCand cand = greedy::fraction(2 * (Tall * Xk - Ak * Pall), Tall * ((long long)m * Ak + Pall) - 2 * Ak * Pall,
                                                                    pr, (unsigned)k, s);
                        if (greedy::fbetter(cand, fbest)) fbest = cand;
                        continue;
                    }
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
                    if (better(sc, pr, best)) best = Cand{sc, pr, (unsigned)k, s};
                }
            }
            // argmin across the group (the second barrier; only VI's phase C needs the winner's S), then the new-cluster candidate
            if constexpr (PEAR) greedy::group_argmax(fbest, minfree, greedy::FPartials{r_num, r_den, r_pr, r_slot, r_free, r_S}, lane, wave);
            else greedy::group_argmin<VI>(best, minfree, red, lane, wave);
            const int Know = K - (int)emptied;
            unsigned isnew = 0;
            if (A.maxK == 0 || Know < A.maxK)
                isnew = PEAR ? greedy::offer_new(fbest, 2 * (Tall * X0 - A0 * Pall), Tall * ((long long)m * A0 + Pall) - 2 * A0 * Pall, emptied, a, minfree)
                             : greedy::offer_new(best, key_new, emptied, a, minfree);
            const unsigned w = PEAR ? fbest.slot : best.slot;
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
                if (PEAR) { XA[0] = X0 + (long long)fbest.S; XA[1] = A0 + (long long)sz[w]; Sa[par] = 0; }
                sz[w] = (unsigned short)(sz[w] + 1);
                if (VI) T[i] = best.S + m;
            }
            moved += v.moved_to(a, w, inext);
            K = Know + (int)isnew;
            hi = max(hi, (int)w);
            par ^= 1;
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
        // the two sums of the Binder numerator and of PEAR's X and P, from the matrix
        upper_sums<false>(C, ld, n, lab, lane, wave, tot, same);
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

// PEAR(c) = num/den from X, A, P (include/redclust_hip.h), 0/1 where den = 0; a < b: a is the larger fraction
struct Fraction {
    long long num, den;
    bool operator<(const Fraction &o) const { return (__int128)num * o.den > (__int128)o.num * den; }
};
static Fraction pear_fraction(long long X, long long A, long long P, long long m, long long T)
{
    const long long den = T * (m * A + P) - 2 * A * P;
    return den ? Fraction{2 * (T * X - A * P), den} : Fraction{0, 1};
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

// Everything behind the three entry points.  c may be NULL (errors then go to the thread's buffer); dC is the device
// count matrix (n × ld, ld a multiple of 4, rows 16-byte aligned), read in place.
// loss: RC_PSM_BINDER, RC_PSM_VILB (runs_out: rc_psm_run_t[nruns]) or LOSS_PEAR (runs_out: rc_pear_run_t[nruns]).
static int32_t run(rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ld, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                   const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                   void *runs_out, int32_t *best, double *kernel_ms)
{
    // ---- the caller's runs: labels in 0..n, orders permutations of 1..n, cluster counts within maxK
    // (the slots are the caller's labels; hi: the highest one in use)
    greedy::Staging S(nruns, n, (size_t)n + 2);
    std::vector<int> h_hi((size_t)nruns);
    for (int r = 0; r < nruns; ++r) {
        unsigned short *szr = S.sz_row(r);
        int K = 0, hi = 0;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t l = init[(size_t)r * n + j];
            if (l < 0 || l > n) return fail(c, RC_ERR_ARG, "point search: label %lld of run %d outside 0..n", (long long)l, r + 1);
            S.init_row(r)[j] = (unsigned short)l;
            if (l) { if (szr[l]++ == 0) ++K; hi = std::max(hi, (int)l); }
        }
        if (maxK > 0 && K > maxK) return fail(c, RC_ERR_ARG, "point search: run %d starts with %d clusters, more than maxK = %d", r + 1, K, maxK);
        S.K[(size_t)r] = K; h_hi[(size_t)r] = hi;
        const int32_t orc = S.take_order(c, "point search", r, order);
        if (orc != RC_OK) return orc;
    }
    // ---- the counts: symmetric, diagonal m, nothing above m
    const int32_t crc = check_counts(c, st, "point search", dC, ld, m, n);
    if (crc != RC_OK) return crc;
    DeviceBuffers B;

    // ---- geometry
    const bool vi = loss == RC_PSM_VILB, pear = loss == LOSS_PEAR;
    const size_t fixed = (vi ? 4 * (size_t)n : 0) + (pear ? 8 * PEAR_HEAD : 0) + 2 * (size_t)(n + 2) + 2 * (size_t)n + 16;
    const size_t per_slot = vi ? 12 : 4;
    int64_t W = std::min<int64_t>(n + 1, (int64_t)((LDS_BUDGET - fixed) / per_slot));
    if (const long long v = env_int("RC_PSM_WINDOW"); v >= 1 && v < W) W = v;   // tests: force the windowed passes at small n
    const size_t lds = (fixed + per_slot * (size_t)W + 15) / 16 * 16;

    int *d_hi;
    HIPCHK(c, S.upload(B, st, sizeof(RunOut)));
    HIPCHK(c, B.alloc(d_hi, h_hi.size()));
    HIPCHK(c, hipMemcpyAsync(d_hi, h_hi.data(), h_hi.size() * 4, hipMemcpyHostToDevice, st));

    Args A{};
    A.C = dC; A.ld = ld; A.init = S.d_init; A.sz0 = S.d_sz; A.K0 = S.d_K; A.hi0 = d_hi; A.order = S.d_order; A.labels = S.d_labels;
    A.out = (RunOut *)S.d_out; A.n = (int)n; A.W = (int)W; A.maxK = maxK; A.maxsweeps = maxsweeps; A.m = (unsigned)m;
    HIPCHK(c, S.begin(st));
    const int Q = (int)((n + TPB - 1) / TPB);
    const hipError_t le = vi ? launch<RC_PSM_VILB>(Q, nruns, lds, st, A) : pear ? launch<LOSS_PEAR>(Q, nruns, lds, st, A)
                                                                                : launch<RC_PSM_BINDER>(Q, nruns, lds, st, A);
    if (le != hipSuccess) return fail(c, RC_ERR_HIP, "point search: launch failed: %s", hipGetErrorString(le));
    std::vector<RunOut> h_out;
    HIPCHK(c, S.collect(st, h_out, kernel_ms));

    const long long pairs = (long long)n * (n - 1) / 2;
    if (pear) {
        // ---- results: num and den from the epilogue's X (same) and P (tot) and the final sizes; the best run is the first of
        // maximal fraction, compared as the kernel compares
        greedy::results(S, h_out, labels_out, (rc_pear_run_t *)runs_out, best, [&](const RunOut &o, rc_pear_run_t &R, const int *cnt, int K) {
            long long within = 0;
            for (int k = 1; k <= K; ++k) within += (long long)cnt[k] * (cnt[k] - 1) / 2;
            const Fraction f = pear_fraction(o.same, within, o.tot, m, pairs);
            R.num = f.num; R.den = f.den;
            R.pear = (double)f.num / (double)f.den;
            return f;
        });
        return RC_OK;
    }
    // ---- results: the losses; the best run is the first of minimal loss
    greedy::results(S, h_out, labels_out, (rc_psm_run_t *)runs_out, best, [&](const RunOut &o, rc_psm_run_t &R, const int *cnt, int K) {
        if (vi) {
            R.loss_num = 0;
            R.loss = o.f / (double)n + 2.0 * std::log((double)m);
        } else {
            long long within = 0;
            for (int k = 1; k <= K; ++k) within += (long long)cnt[k] * (cnt[k] - 1) / 2;
            R.loss_num = o.tot + (long long)m * within - 2 * o.same;
            R.loss = pairs ? (double)R.loss_num / (double)((long long)m * pairs) : 0.0;
        }
        return R.loss;
    });
    return RC_OK;
}

// greedy::check_args, then what the counts' entry points check besides, in this order
static int32_t check_args(rc_ctx *c, const char *who, int64_t m, int64_t n, int32_t loss, int32_t nruns, const int64_t *init,
                          const int32_t *order, int32_t maxK, int32_t maxsweeps, const int64_t *labels_out, const void *runs_out,
                          const int32_t *best)
{
    const int32_t rc = greedy::check_args(c, who, m, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    if (loss != RC_PSM_BINDER && loss != RC_PSM_VILB) return fail(c, RC_ERR_ARG, "%s: invalid loss specifier %d", who, loss);
    return check_lds_capacity(c, who, n, m);
}


// The three entry points: cnt::with puts the counts of src on the device between check_args and run
static int32_t search(const char *who, const cnt::Source &src, int32_t loss, int32_t nruns, const int64_t *init, const int32_t *order,
                      int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms)
{
    return cnt::with(
        who, src,
        [&](rc_ctx *c, int64_t m, int64_t n) { return check_args(c, who, m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best); },
        [&](rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ld, int64_t m, int64_t n) {
            return run(c, st, dC, ld, m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best, kernel_ms);
        });
}

// rc_pear_search*: rc_psm_search*'s checks in their order without the loss specifier, then PEAR's own capacity — m·T² < 2^62,
// T = n(n−1)/2, keeps |num| and den below 2^63
static int32_t pear_search(const char *who, const cnt::Source &src, int32_t nruns, const int64_t *init, const int32_t *order, int32_t maxK,
                           int32_t maxsweeps, int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms)
{
    return cnt::with(
        who, src,
        [&](rc_ctx *c, int64_t m, int64_t n) {
            int32_t rc = greedy::check_args(c, who, m, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
            if (rc == RC_OK) rc = check_lds_capacity(c, who, n, m);
            if (rc != RC_OK) return rc;
            const long long T = (long long)n * (n - 1) / 2;
            if ((__int128)m * T * T >= ((__int128)1 << 62))
                return fail(c, RC_ERR_CAPACITY, "%s: m*T^2 does not fit 62 bits, T = n(n-1)/2 (m=%lld n=%lld)", who, (long long)m, (long long)n);
            return (int32_t)RC_OK;
        },
        [&](rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ld, int64_t m, int64_t n) {
            return run(c, st, dC, ld, m, n, LOSS_PEAR, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best, kernel_ms);
        });
}

}  // namespace psm

extern "C" int32_t rc_pear_search(int32_t device, const void *counts, int64_t m, int64_t n, int32_t nruns, const int64_t *init,
                                  const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                  int32_t *best, double *kernel_ms)
{
    return psm::pear_search("rc_pear_search", cnt::host_counts(device, counts, m, n), nruns, init, order, maxK, maxsweeps, labels_out, runs_out,
                            best, kernel_ms);
}

extern "C" int32_t rc_pear_search_samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t nruns, const int64_t *init,
                                          const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                          int32_t *best, double *kernel_ms, double *counts_ms)
{
    return psm::pear_search("rc_pear_search_samples", cnt::samples(device, samples, m, n, counts_ms), nruns, init, order, maxK, maxsweeps,
                            labels_out, runs_out, best, kernel_ms);
}

extern "C" int32_t rc_pear_search_ctx(rc_ctx *c, int64_t numsamples, int32_t nruns, const int64_t *init, const int32_t *order,
                                      int32_t maxK, int32_t maxsweeps, int64_t *labels_out, rc_pear_run_t *runs_out, int32_t *best,
                                      double *kernel_ms)
{
    return psm::pear_search("rc_pear_search_ctx", cnt::context(c, numsamples), nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best,
                            kernel_ms);
}

extern "C" int32_t rc_psm_search(int32_t device, const void *counts, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                                 const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                                 void *runs_out, int32_t *best, double *kernel_ms)
{
    return psm::search("rc_psm_search", cnt::host_counts(device, counts, m, n), loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out,
                       best, kernel_ms);
}

extern "C" int32_t rc_psm_search_samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                                         const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps,
                                         int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms, double *counts_ms)
{
    return psm::search("rc_psm_search_samples", cnt::samples(device, samples, m, n, counts_ms), loss, nruns, init, order, maxK, maxsweeps,
                       labels_out, runs_out, best, kernel_ms);
}

extern "C" int32_t rc_psm_search_ctx(rc_ctx *c, int64_t numsamples, int32_t loss, int32_t nruns, const int64_t *init,
                                     const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                                     rc_psm_run_t *runs_out, int32_t *best, double *kernel_ms)
{
    return psm::search("rc_psm_search_ctx", cnt::context(c, numsamples), loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best,
                       kernel_ms);
}

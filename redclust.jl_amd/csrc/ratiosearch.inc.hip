// Ratio-loss search on the device (rc_ratio_search; DESIGN.md §8 "Ratio-loss search"): the greedy search of greedy.inc.hip for the
// three criteria that are a mean over the samples of a RATIO whose numerator and denominator both move with the candidate —
// omARI (the reference's fourth MPEL loss: the mean of 1 − ARI(c, sample)), NVI and NID (SALSO's normalised VI and normalised
// information distance).  Included behind visearch.inc.hip: the tables, their layout, the thread geometry, the carve and the host
// preparation (visearch::Host) are the exact searches'; k_visearch and its siblings are not touched.
//
// Per sample s one running integer and one constant, with rc_vi_gtable's Gq / Φq and C2(x) = x(x−1)/2:
//   entropic (NVI, NID):  T_s = Σ_kl Φq(N^s_kl),  A = Σ_k Φq(n_k),  B_s = Σ_l Φq(n^s_l),  C = Φq(n)
//       NVI: num = A + B_s − 2T_s, den = C − T_s           NID: num = max(A, B_s) − T_s, den = C − min(A, B_s)
//   omARI:  T_s = Σ_kl C2(N^s_kl),  A = Σ_k C2(n_k),  B_s = Σ_l C2(n^s_l),  C = C2(n)
//       num = C·(A + B_s − 2T_s), den = C·(A + B_s) − 2·A·B_s
//   term_s = 0 where den = 0, else llrint(__ddiv_rn((double)num, (double)den)·2^40);   Q(c) = Σ_s term_s (an i64, order-free).
// Every num and den is below 2^53 at n <= 8192, so the conversions are exact and the division is the correctly rounded one of
// two exact doubles: NumPy's float64 division gives the same bits.  Putting a point into slot k adds δ(N^s[l_s(i)][k]) to T_s and
// δ(n_k) to A, δ = Gq (entropic) or the identity (omARI: x more pairs).
//
// The step has k_visearch's phases and one barrier more.  T[s] and A are kept WITH THE VISITED POINT OUT:
//   (A) thread (r, c) reads, for each of its samples, the 8-byte row piece, T_s and B_s, forms the four candidate states
//       (T_s + δ(N), A + δ(n_k)) and adds their four terms — four independent f64 divisions in flight — into registers, then into
//       the per-slot LDS accumulators (64-bit atomics).  Column 0 also adds term_s of the state itself: the base, once per step.
//   barrier; (B) thread k − 1 scores slot k as acc_k − base; argmin (greedy's keys; its barrier); the new cluster scores 0;
//   (C) the tables as in k_visearch; the put-in T_s += δ(N^s[l][w]) by the owner of slot w's column and the take-out of the NEXT
//       point T_s −= δ(N^s[l'][a'] − 1) by the owner of its slot's column: two different threads, hence 64-bit LDS atomics
//       (PQ = 0: device-memory atomics) — integer adds commute; thread 0 keeps A, lab and sz.
//   barrier: what (C) added to T_s came from up to two threads that are not its readers, and every thread of a table row reads T_s
//       in the next (A); the workgroup barrier is the fence (LDS: it orders the ds atomics; PQ = 0: T is read with device-scope
//       atomic loads, which meet the atomics in L2).  This is the third barrier; two would need one writer AND one reader per scalar.
// T lives in LDS while the labels are staged there (PQ > 0: m <= 4096, 8·1024·PQ bytes behind the carve), else in device memory
// per run; B_s is copied to LDS behind it where 8·m more bytes fit (b_lds), else read from device memory (one address per row of
// threads: one request).

namespace ratiosearch {

using greedy::TPB, greedy::NWAVE, greedy::Cand, greedy::key_i64;
using visearch::VEC, visearch::Carve, visearch::RunOut, visearch::up16;
constexpr int OMARI = 0, NVI = 1, NID = 2;            // RC_RATIO_*
constexpr long long M_MAX = 1ll << 21;                // term_s <= 2·2^40, so Q <= m·2^41 <= 2^62

struct Args {
    visearch::Args a;             // Gq, Phi, SL, N, the runs: what visearch::Host uploads
    long long *T;                 // PQ = 0: nruns × m running integers
    const long long *B;           // m: the samples' constants, in sample order
    long long Cn;                 // Φq(n) or C2(n)
    int b_lds;                    // B is copied to LDS behind T
};

template <int LOSS> __device__ inline long long delta(const long long *Gq, unsigned x) { return LOSS == OMARI ? (long long)x : Gq[x]; }

// one sample's term at the state (T, A): int64 state, one correctly rounded division, 2^-40 fixed point
template <int LOSS> __device__ inline unsigned long long term(long long T, long long A, long long B, long long Cn)
{
    long long num, den;
    if (LOSS == NVI) { num = A + B - 2 * T; den = Cn - T; }
    else if (LOSS == NID) { num = max(A, B) - T; den = Cn - min(A, B); }
    else { num = Cn * (A + B - 2 * T); den = Cn * (A + B) - 2 * A * B; }
    const double q = __ddiv_rn((double)num, (double)(den ? den : 1));
    return den ? (unsigned long long)llrint(q * 0x1p40) : 0ull;
}

// T_s in LDS (PQ > 0) or in device memory, where its readers must not meet a stale line of the vector cache
template <int PQ> __device__ inline long long load_T(const long long *T, int s)
{
    return PQ ? T[s] : __hip_atomic_load(T + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <int PQ> __device__ inline void store_T(long long *T, int s, long long v)
{
    if (PQ) T[s] = v;
    else __hip_atomic_store(T + s, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void add_T(long long *T, int s, long long d)
{
    if (d) atomicAdd(reinterpret_cast<unsigned long long *>(T + s), (unsigned long long)d);
}

template <int PQ, int LOSS>
__global__ __launch_bounds__(TPB) void k_ratiosearch(Args RA)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    const visearch::Args &A = RA.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, m = A.m, kpad = A.kpad, Kcap = A.Kcap, Lmax = A.Lmax, run = blockIdx.x;
    const long long Cn = RA.Cn;

    const Carve cv(n, kpad, Kcap, PQ);
    long long *Gq = reinterpret_cast<long long *>(rs_lds + cv.gq);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(rs_lds + cv.acc);
    unsigned long long *r_sc = reinterpret_cast<unsigned long long *>(rs_lds + cv.red);
    unsigned long long *r_q = r_sc + NWAVE;
    unsigned *r_pr = reinterpret_cast<unsigned *>(r_q + NWAVE), *r_slot = r_pr + NWAVE, *r_free = r_slot + NWAVE;
    unsigned short *sz = reinterpret_cast<unsigned short *>(rs_lds + cv.sz);
    unsigned short *lab = reinterpret_cast<unsigned short *>(rs_lds + cv.lab);
    unsigned short *stage = reinterpret_cast<unsigned short *>(rs_lds + cv.stage);    // [2][TPB·PQ]
    long long *scal = reinterpret_cast<long long *>(rs_lds + cv.total);               // [0] A with the point out, [1] the base
    unsigned long long *base = reinterpret_cast<unsigned long long *>(scal + 1);
    long long *T_l = scal + 2;                                                        // PQ > 0: T[TPB·PQ]; then B[m] if b_lds
    long long *T = PQ ? T_l : RA.T + (size_t)run * m;
    const long long *Bc = RA.b_lds ? T_l + (size_t)TPB * PQ : RA.B;

    const unsigned short *__restrict__ SL = A.SL;
    unsigned short *Nrun = A.N + (size_t)run * m * Lmax * kpad;
    const size_t lstride = (size_t)Lmax * kpad;

    for (int x = tid; x < n; x += TPB) Gq[x] = A.Gq[x];
    for (int k = tid; k < kpad; k += TPB) acc[k] = 0;
    for (int k = tid; k < Kcap + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (Kcap + 2) + k];
    for (int j = tid; j < n; j += TPB) lab[j] = A.init[(size_t)run * n + j];
    if (RA.b_lds)
        for (int s = tid; s < m; s += TPB) T_l[(size_t)TPB * PQ + s] = RA.B[s];
    __syncthreads();
    int K = A.K0[run];
    // the tables of the starting labels and their T_s: one thread per sample (the only pass in which a thread writes table
    // elements it does not own; the barrier below orders it before everything else)
    for (int s = tid; s < m; s += TPB) {
        long long Ts = 0;
        if (K) {
            unsigned short *Ns = Nrun + (size_t)s * lstride;
            for (int j = 0; j < n; ++j) {
                const unsigned l = lab[j];
                if (l) {
                    unsigned short *p = Ns + (size_t)SL[(size_t)j * m + s] * kpad + (l - 1);
                    const unsigned x = *p;
                    Ts += delta<LOSS>(Gq, x);
                    *p = (unsigned short)(x + 1u);
                }
            }
        }
        store_T<PQ>(T, s, Ts);
    }

    const int G = kpad / VEC, R = TPB / G;
    const int r = tid / G, c = tid - r * G;
    const bool active = r < R;
    const greedy::Partials red{r_sc, r_pr, r_slot, r_free, nullptr};
    greedy::Visit v(A.order + (size_t)run * n, n);
    int buf = 0;
    if (PQ) {
#pragma unroll
        for (int q = 0; q < PQ; ++q) {
            const int s = tid + q * TPB;
            if (s < m) stage[s] = SL[(size_t)v.i * m + s];
        }
    }
    if (tid == 0) {
        // A of the start without the first point: Σ_k Σ_{y < n_k} δ(y), at most n terms
        long long Aq = 0;
        const unsigned a0 = lab[v.i];
        for (int k = 1; k <= Kcap; ++k) {
            const unsigned nk = sz[k] - (k == (int)a0 ? 1u : 0u);
            for (unsigned y = 0; y < nk; ++y) Aq += delta<LOSS>(Gq, y);
        }
        scal[0] = Aq;
        *base = 0;
    }
    __syncthreads();
    {
        // the first point out of T_s (PQ = 0: the plain stores above are the same thread's only where G = 1; the barrier orders them)
        const unsigned a0 = lab[v.i];
        if (active && a0 && (int)(a0 - 1u) / VEC == c) {
            const unsigned short *cur0 = PQ ? stage : SL + (size_t)v.i * m;
            for (int s = r; s < m; s += R)
                add_T(T, s, -delta<LOSS>(Gq, Nrun[(size_t)s * lstride + (size_t)cur0[s] * kpad + (a0 - 1u)] - 1u));
        }
    }
    __syncthreads();

    long long moves = 0;
    int sweeps = 0, converged = 0;
    const unsigned long long key_new = key_i64(0);

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            const int i = v.i, inext = v.ahead(t);
            unsigned short nxt[PQ ? PQ : 1];
            if (PQ) {
#pragma unroll
                for (int q = 0; q < PQ; ++q) {
                    const int s = tid + q * TPB;
                    nxt[q] = (s < m) ? SL[(size_t)inext * m + s] : (unsigned short)0;
                }
            }
            const unsigned short *cur = PQ ? stage + (size_t)buf * TPB * PQ : SL + (size_t)i * m;
            const unsigned a = v.slot_of(lab);
            const long long A0 = scal[0];

            // phase A: Σ_s term_s(T_s + δ(N^s[l_s(i)][k]), A0 + δ(n_k)) for this thread's four slots over its samples
            if (active) {
                const int ka = (int)a - 1 - c * VEC;
                const unsigned short *Nc = Nrun + (size_t)c * VEC;
                long long Ak[VEC];
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const int k = c * VEC + e + 1;
                    const unsigned nk = k <= Kcap ? (unsigned)sz[k] - (ka == e ? 1u : 0u) : 0u;
                    Ak[e] = A0 + delta<LOSS>(Gq, nk);
                }
                unsigned long long part[VEC] = {0, 0, 0, 0}, bpart = 0;
                for (int s = r; s < m; s += R) {
                    const uint2 w2 = *reinterpret_cast<const uint2 *>(Nc + (size_t)s * lstride + (size_t)cur[s] * kpad);
                    const long long Ts = load_T<PQ>(T, s), Bs = Bc[s];
                    const unsigned x[VEC] = {(w2.x & 0xFFFFu) - (ka == 0 ? 1u : 0u), (w2.x >> 16) - (ka == 1 ? 1u : 0u),
                                             (w2.y & 0xFFFFu) - (ka == 2 ? 1u : 0u), (w2.y >> 16) - (ka == 3 ? 1u : 0u)};
#pragma unroll
                    for (int e = 0; e < VEC; ++e) part[e] += term<LOSS>(Ts + delta<LOSS>(Gq, x[e]), Ak[e], Bs, Cn);
                    if (c == 0) bpart += term<LOSS>(Ts, A0, Bs, Cn);
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (part[e]) atomicAdd(&acc[c * VEC + e], part[e]);
                if (bpart) atomicAdd(base, bpart);
            }
            __syncthreads();

            // phase B: thread k − 1 scores slot k against the base (and clears its accumulator)
            if (PQ) {
#pragma unroll
                for (int q = 0; q < PQ; ++q) {
                    const int s = tid + q * TPB;
                    if (s < m) stage[(size_t)(buf ^ 1) * TPB * PQ + s] = nxt[q];
                }
            }
            const unsigned emptied = (a && sz[a] == 1) ? 1u : 0u;
            Cand best{~0ull, ~0u, 0u, 0u};
            unsigned minfree = ~0u;
            if (tid < kpad) {
                const unsigned k = (unsigned)tid + 1u;
                const long long sc = (long long)(acc[tid] - *base);
                acc[tid] = 0;
                if (k <= (unsigned)Kcap) {
                    const int nk = (int)sz[k] - (k == a ? 1 : 0);
                    if (nk <= 0) minfree = k;
                    else best = Cand{key_i64(sc), (k == a) ? 0u : k, k, 0u};
                }
            }
            greedy::group_argmin<false>(best, minfree, red, lane, wave);
            const int Know = K - (int)emptied;
            const unsigned isnew = Know < Kcap ? greedy::offer_new(best, key_new, emptied, a, minfree) : 0u;
            const unsigned w = best.slot;

            // phase C: i into w, the next point out.  Table elements by their owners as in k_visearch; T_s by atomics
            const unsigned an = (inext == i) ? w : (unsigned)lab[inext];
            if (active) {
                const bool da = a && (int)(a - 1u) / VEC == c, dw = (int)(w - 1u) / VEC == c, dn = an && (int)(an - 1u) / VEC == c;
                if ((da && a != w) || dw || dn) {
                    const unsigned short *nx = PQ ? stage + (size_t)(buf ^ 1) * TPB * PQ : SL + (size_t)inext * m;
                    for (int s = r; s < m; s += R) {
                        unsigned short *row = Nrun + (size_t)s * lstride + (size_t)cur[s] * kpad;
                        long long d = 0;
                        if (a != w) {
                            if (da) row[a - 1u] = (unsigned short)(row[a - 1u] - 1u);
                            if (dw) {
                                const unsigned x = row[w - 1u];
                                d = delta<LOSS>(Gq, x);
                                row[w - 1u] = (unsigned short)(x + 1u);
                            }
                        } else if (dw)
                            d = delta<LOSS>(Gq, row[w - 1u] - 1u);                    // back where it was
                        if (dn) d -= delta<LOSS>(Gq, Nrun[(size_t)s * lstride + (size_t)nx[s] * kpad + (an - 1u)] - 1u);
                        add_T(T, s, d);
                    }
                }
            }
            if (tid == 0) {
                long long Aq = A0 + delta<LOSS>(Gq, (unsigned)sz[w] - (w == a ? 1u : 0u));
                lab[i] = (unsigned short)w;
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
                if (an) Aq -= delta<LOSS>(Gq, (unsigned)sz[an] - 1u);
                scal[0] = Aq;
                *base = 0;
            }
            moved += v.moved_to(a, w, inext);
            K = Know + (int)isnew;
            buf ^= 1;
            __syncthreads();                                      // the third barrier: T_s, A, sz and lab before their readers
        }
        ++sweeps;
        moves += moved;
        if (!moved) { converged = 1; break; }
        if (sweeps >= A.maxsweeps) break;
    }

    // the pending point back in, then Q = Σ_s term_s of the state the run kept
    {
        const unsigned a = v.slot_of(lab);
        const unsigned short *cur = PQ ? stage + (size_t)buf * TPB * PQ : SL + (size_t)v.i * m;
        if (active && a && (int)(a - 1u) / VEC == c)
            for (int s = r; s < m; s += R)
                add_T(T, s, delta<LOSS>(Gq, Nrun[(size_t)s * lstride + (size_t)cur[s] * kpad + (a - 1u)] - 1u));
        if (tid == 0 && a) scal[0] += delta<LOSS>(Gq, (unsigned)sz[a] - 1u);
    }
    for (int j = tid; j < n; j += TPB) A.labels[(size_t)run * n + j] = lab[j];
    __syncthreads();
    unsigned long long q = 0;
    for (int s = tid; s < m; s += TPB) q += term<LOSS>(load_T<PQ>(T, s), scal[0], Bc[s], Cn);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += greedy::shfl_xor_u64(q, off);
    if (lane == 0) r_q[wave] = q;
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < NWAVE; ++w) s += r_q[w];
        RunOut o{};
        o.Q = (long long)s; o.moves = moves; o.sweeps = sweeps; o.converged = converged; o.K = K;
        A.out[run] = o;
    }
}

template <int LOSS>
static hipError_t launch(int PQ, int nruns, size_t lds, const Args &A)
{
#define RS_LAUNCH(QQ)                                                                                                     \
    do {                                                                                                                  \
        void (*kernel)(Args) = k_ratiosearch<QQ, LOSS>;                                                                   \
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);   \
        if (e != hipSuccess) return e;                                                                                    \
        kernel<<<nruns, TPB, lds, 0>>>(A);                                                                                \
    } while (0)
    if (PQ == 0) RS_LAUNCH(0);
    else if (PQ == 1) RS_LAUNCH(1);
    else RS_LAUNCH(visearch::STAGE_Q);
#undef RS_LAUNCH
    return hipGetLastError();
}

// The host side of rc_ratio_search: visearch::run's checks in its order, its preparation (visearch::Host) and its results
static int32_t run(const char *who, int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                   const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out_,
                   int32_t *best, double *kernel_ms)
{
    using namespace visearch;
    rc_psm_run_t *runs_out = (rc_psm_run_t *)runs_out_;
    if (!samples) return fail(nullptr, RC_ERR_ARG, "%s: NULL argument", who);
    int32_t rc = greedy::check_args(nullptr, who, m, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    if (loss != OMARI && loss != NVI && loss != NID)
        return fail(nullptr, RC_ERR_ARG, "%s: loss must be RC_RATIO_OMARI, RC_RATIO_NVI or RC_RATIO_NID (got %d)", who, loss);
    rc = check_lds_capacity(nullptr, who, n);
    if (rc != RC_OK) return rc;
    if (m > MN_MAX / n) return fail(nullptr, RC_ERR_CAPACITY, "%s: m*n exceeds 2^26 = %lld (m=%lld n=%lld)", who, MN_MAX, (long long)m, (long long)n);
    if (m > M_MAX) return fail(nullptr, RC_ERR_CAPACITY, "%s: m = %lld exceeds the 2^21 = %lld samples whose terms of up to 2^41 sum below 2^63", who, (long long)m, M_MAX);

    rc = check_label_rows(nullptr, who, "sample", samples, m, n);
    if (rc != RC_OK) return rc;
    std::vector<unsigned short> h_SL((size_t)n * m);
    Host H(n);
    int Lmax = 0;
    std::vector<long long> Bs((size_t)m);
    for (int64_t s = 0; s < m; ++s) {
        int L;
        Bs[(size_t)s] = H.take_sample(samples + (size_t)s * n, h_SL.data() + s, (size_t)m, L);
        if (loss == OMARI) {
            long long pairs = 0;
            for (int l = 1; l <= L; ++l) pairs += (long long)H.cnt[(size_t)l] * (H.cnt[(size_t)l] - 1) / 2;
            Bs[(size_t)s] = pairs;
        }
        Lmax = std::max(Lmax, L);
    }
    const int64_t Kcap64 = std::min<int64_t>(maxK > 0 ? maxK : Lmax, n);
    if (Kcap64 > KCAP_MAX)
        return fail(nullptr, RC_ERR_CAPACITY, "%s: the slot cap %lld (maxK, or the largest cluster count among the samples) exceeds %d", who,
                    (long long)Kcap64, KCAP_MAX);
    const int Kcap = (int)Kcap64, kpad = (Kcap + VEC - 1) / VEC * VEC;
    const size_t table_elems = (size_t)m * Lmax * kpad;
    if ((double)table_elems * 2.0 * nruns > (double)TABLE_BUDGET)
        return fail(nullptr, RC_ERR_CAPACITY, "%s: the contingency tables (runs x m x Lmax x Kcap4 x 2 B = %d x %lld x %d x %d x 2, Kcap4 = the slot cap rounded up to 4) exceed the budget of %llu MiB",
                    who, nruns, (long long)m, Lmax, kpad, (unsigned long long)(TABLE_BUDGET >> 20));

    greedy::Staging S(nruns, n, (size_t)Kcap + 2);
    for (int r = 0; r < nruns; ++r) {
        long long Aq;
        rc = H.take_run(S, who, r, init, order, Kcap, Aq);
        if (rc != RC_OK) return rc;
    }
    rc = select_device(who, device);
    if (rc != RC_OK) return rc;

    DeviceBuffers B;
    Args A{};
    HIPCHK(nullptr, H.upload(B, S, h_SL, table_elems * (size_t)nruns, A.a));
    A.a.n = (int)n; A.a.m = (int)m; A.a.Lmax = Lmax; A.a.kpad = kpad; A.a.Kcap = Kcap; A.a.maxsweeps = maxsweeps;
    A.Cn = loss == OMARI ? (long long)n * (n - 1) / 2 : (long long)H.Phi[(size_t)n];
    const int PQ = stage_depth(m);
    long long *d_B, *d_T = nullptr;
    HIPCHK(nullptr, B.alloc(d_B, Bs.size()));
    HIPCHK(nullptr, hipMemcpy(d_B, Bs.data(), Bs.size() * 8, hipMemcpyHostToDevice));
    if (!PQ) {                                                          // every entry is written before it is read
        HIPCHK(nullptr, B.alloc(d_T, (size_t)nruns * m));
    }
    A.B = d_B; A.T = d_T;
    size_t lds = Carve((int)n, kpad, Kcap, PQ).total + 16 + 8 * (size_t)TPB * PQ;
    A.b_lds = lds + 8 * (size_t)m <= LDS_MAX ? 1 : 0;
    if (A.b_lds) lds += 8 * (size_t)m;
    HIPCHK(nullptr, S.begin(0));
    HIPCHK(nullptr, loss == OMARI ? launch<OMARI>(PQ, nruns, lds, A) : loss == NVI ? launch<NVI>(PQ, nruns, lds, A) : launch<NID>(PQ, nruns, lds, A));
    std::vector<RunOut> h_out;
    HIPCHK(nullptr, S.collect(0, h_out, kernel_ms));

    const double scale = std::ldexp((double)m, 40);
    greedy::results(S, h_out, labels_out, runs_out, best, [&](const RunOut &o, rc_psm_run_t &R, const int *, int) {
        R.loss_num = o.Q;
        R.loss = (double)o.Q / scale;
        return R.loss_num;
    });
    return RC_OK;
}

}  // namespace ratiosearch

extern "C" int32_t rc_ratio_search(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t loss, int32_t nruns, const int64_t *init,
                                   const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                   int32_t *best, double *kernel_ms)
{
    return ratiosearch::run("rc_ratio_search", device, samples, m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best,
                            kernel_ms);
}

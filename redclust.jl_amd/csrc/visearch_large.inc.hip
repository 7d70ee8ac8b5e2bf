// The exact expected VI search of visearch_kernel.inc.hip for n <= 32767 (DESIGN.md §8 "Exact expected VI search, large n"): the
// device side of rc_vi_search_large, rc_vi_search_groups_large and rc_id_search_large.  Included behind visearch_kernel.inc.hip THREE
// times: plainly it defines the declarations and k_vilarge<PQ>; with VISL_GROUPED defined, from the same text, k_vilarge_groups<PQ>;
// with VISL_ID defined, k_idlarge<PQ> (below, "ID").  GROUPED and ID are constants folded at the top of the kernel, not template
// parameters: the names and the instructions of the first two do not depend on the third being there.
//
// The criterion (LOSS_VI), a run, the tie rules, maxK, the moves / sweeps / converged bookkeeping, the final Q from Φq, the 1024
// threads of one persistent workgroup per run, the (r, c) ownership of the table cells, the two barriers of a step and the LDS
// double buffer of the next point's sample labels are k_visearch's, and a run returns k_visearch's bytes.  What pins k_visearch to
// n <= 8192 is its carve — Gq i64[n+1] and lab u16[n] — and neither is here in that form:
//
// Labels.  A step needs one label: the visited point's.  The run's labels live in its row of the `labels` output in global memory,
// which the kernel copies the start into; from then on thread 0 is the row's only reader and only writer.  At the top of a step
// thread 0 loads the NEXT point's slot (its own earlier stores are the only ones to that row, so program order is all it needs),
// and publishes it in pub[2] behind the first barrier, as the stage buffer is; every thread reads it at the top of the next step.
// The load is in flight over phase A.  Only with n = 1 is the next point the one being moved; Visit's (iprev, wprev) covers that.
//
// Split Gq.  LDS holds the low words, lo u32[n+1] (128 KiB at n = 32767); the high word of Gq[x] is hi(x) of gqsplit.inc.hpp,
// from the at most 11 thresholds the host reads off the table and passes by value: the 16-entry octave table oct[] is built from
// them in the prologue, and a cell costs one ds_read of lo, one of oct (16 addresses: conflict-free) and a compare.  Phase A sums
// the low words in 64 bits and the high counts in 32 (a thread adds at most m <= 2^26 cells of hi <= 11) and combines them into
// the integer k_visearch forms before the LDS atomic.  Φq, needed once at the end, is read from global memory.
//
// LDS (dynamic, 16-byte offsets): lo u32[n+1], acc u64[kpad], the reduction partials, sz u16[Kcap+2], the label double buffer
// u16[2][1024·PQ]: 158 160 B at n = 32767, Kcap = 1024, PQ = 4; static: oct u32[32] and pub u32[2].
//
// ID (k_idlarge<PQ>, rc_id_search_large; DESIGN.md §8 "Exact expected ID search, large n"): the step above with k_visearch<LOSS_ID>'s
// additions.  Phase B scores slot k as F(A0 + Gq[n_k]) − F(A0) − acc_k, Gq[·] from gq_at (there is no i64 table in LDS), A0 = Aq
// without the visited point; thread 0 keeps Aq (LDS, behind the carve) up to date in phase C under sz's discipline; the final Q is
// F(Aq) − Σ Φq(N).  F(x) = x·p(x) + Pre[m] − Pre[p(x)], p(x) = #{t : Bs[t] <= x}, needs the sorted Bs i64[m] and Pre i64[m+1]:
//   whole (A.tab_lds)  both in LDS behind Aq, 16·(m+1) B with it, where that fits beside the carve and the static LDS — every
//                      m <= 1024 at any n; id_F2 as it stands.
//   fenced             otherwise (at n = 32767, m = 2048, PQ = 4, Kcap = 1024 the carve leaves 5 520 B): LDS holds Aq (16 B) and the
//                      fence Fn[t] = Bs[(t+1)·2^s − 1], t < m >> s, s = AL.fshift the smallest shift for which it fits (the host's
//                      choice); the search for p(x) does its first nbits − s trips on the fence and its last s on Bs in global
//                      memory, then reads Pre[p] there: id_F2_fenced.  p(x), and so every byte of a run, is the same either way.

namespace visearch {

#if !defined(VISL_GROUPED) && !defined(VISL_ID)
struct ArgsL {
    Args a;                       // k_visearch's: LOSS_VI's part of it (and runs, grouped), all of LOSS_ID's for k_idlarge
    GqSplit split;                // the thresholds of a.Gq
    int fshift;                   // k_idlarge with a.tab_lds = 0: the fence keeps every 2^fshift-th entry of Bs (behind everything
                                  // else: the other kernels' arguments stay where they were)
};

constexpr size_t STATIC_L = 144;                      // oct u32[32] and pub u32[2] as the compiler lays them out, beside the dynamic LDS

struct CarveL {
    size_t lo, acc, red, sz, stage, total;
    __host__ __device__ CarveL(int n, int kpad, int Kcap, int PQ)
    {
        lo = 0;
        acc = lo + up16(4 * (size_t)(n + 1));
        red = acc + up16(8 * (size_t)kpad);
        sz = red + up16((size_t)NWAVE * (8 + 8 + 4 + 4 + 4));
        stage = sz + up16(2 * (size_t)(Kcap + 2));
        total = stage + up16(2 * 2 * (size_t)TPB * PQ);
    }
};

// where x's octave entry sits in oct[32]: 31 − bitlength(x), 16..31 for x <= 32767 (2x + 1 is never 0)
__device__ inline int oct_index(unsigned x) { return __builtin_clz(2u * x + 1u); }

__device__ inline void add_cell(unsigned x, const unsigned *lo, const unsigned *oct, unsigned long long &sum, unsigned &cnt)
{
    const unsigned e = oct[oct_index(x)];
    sum += lo[x];
    cnt += (e & 15u) + (x >= (e >> 4) ? 1u : 0u);
}

__device__ inline long long gq_at(unsigned x, const unsigned *lo, const unsigned *oct)
{
    unsigned long long sum = 0;
    unsigned cnt = 0;
    add_cell(x, lo, oct, sum, cnt);
    return (long long)(sum + ((unsigned long long)cnt << 32));
}

__device__ inline void add_row_l(const uint2 v, int ka, const unsigned *lo, const unsigned *oct, unsigned long long (&sum)[VEC], unsigned (&cnt)[VEC])
{
    // ka: where the visited point's own slot sits in this thread's four, if it does — the point itself is out
    add_cell((v.x & 0xFFFFu) - (ka == 0 ? 1u : 0u), lo, oct, sum[0], cnt[0]);
    add_cell((v.x >> 16) - (ka == 1 ? 1u : 0u), lo, oct, sum[1], cnt[1]);
    add_cell((v.y & 0xFFFFu) - (ka == 2 ? 1u : 0u), lo, oct, sum[2], cnt[2]);
    add_cell((v.y >> 16) - (ka == 3 ? 1u : 0u), lo, oct, sum[3], cnt[3]);
}

// ID, fenced placement: (F(x0), F(x1)) − Pre[m] as id_F2 finds them — the same trips, the same p — with the first nbits − sh trips
// on the fence Fn[t] = Bs[(t + 1)·2^sh − 1] in LDS (a probe at q = p + 2^b, b >= sh, is a multiple of 2^sh) and the last sh trips on
// Bs itself, within the 2^sh − 1 entries behind p; mfl = m rounded down to a multiple of 2^sh, so q <= m exactly when q <= mfl, and
// while a trip is left on the fence 2^sh <= 2^(nbits−1) <= m: the fence is not empty.  Pre[m] is left out: it cancels in a step
__device__ inline void id_F2_fenced(const long long *Fn, const long long *__restrict__ Bs, const long long *__restrict__ Pre, int m, int nbits,
                                    int sh, long long x0, long long x1, long long &F0, long long &F1)
{
    const int mfl = (m >> sh) << sh;
    int p0 = 0, p1 = 0;
    for (int b = nbits - 1; b >= sh; --b) {
        const int q0 = p0 + (1 << b), q1 = p1 + (1 << b);
        const long long b0 = Fn[(min(q0, mfl) >> sh) - 1], b1 = Fn[(min(q1, mfl) >> sh) - 1];
        if (q0 <= m && b0 <= x0) p0 = q0;
        if (q1 <= m && b1 <= x1) p1 = q1;
    }
    for (int b = min(sh, nbits) - 1; b >= 0; --b) {
        const int q0 = p0 + (1 << b), q1 = p1 + (1 << b);
        const long long b0 = Bs[min(q0, m) - 1], b1 = Bs[min(q1, m) - 1];
        if (q0 <= m && b0 <= x0) p0 = q0;
        if (q1 <= m && b1 <= x1) p1 = q1;
    }
    F0 = x0 * p0 - Pre[p0];
    F1 = x1 * p1 - Pre[p1];
}

#endif
#if defined(VISL_GROUPED)
template <int PQ>
__global__ __launch_bounds__(TPB) void k_vilarge_groups(ArgsL AL)
{
    constexpr bool GROUPED = true, ID = false;
#elif defined(VISL_ID)
template <int PQ>
__global__ __launch_bounds__(TPB) void k_idlarge(ArgsL AL)
{
    constexpr bool GROUPED = false, ID = true;
#else
template <int PQ>
__global__ __launch_bounds__(TPB) void k_vilarge(ArgsL AL)
{
    constexpr bool GROUPED = false, ID = false;
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char visl_lds[];
    __shared__ unsigned oct[32], pub[2];
    const Args &A = AL.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, kpad = A.kpad, run = blockIdx.x;
    GroupRun g{};
    if (GROUPED) g = A.runs[run];
    const int m = GROUPED ? g.m : A.m, Lmax = GROUPED ? g.Lmax : A.Lmax, Kcap = GROUPED ? g.Kcap : A.Kcap;
    const int Kstride = GROUPED ? A.Kcap : Kcap;                      // the launch's largest cap: the carve and sz0's rows

    const CarveL cv(n, kpad, Kstride, PQ);
    unsigned *lo = reinterpret_cast<unsigned *>(visl_lds + cv.lo);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(visl_lds + cv.acc);
    unsigned long long *r_sc = reinterpret_cast<unsigned long long *>(visl_lds + cv.red);
    unsigned long long *r_q = r_sc + NWAVE;
    unsigned *r_pr = reinterpret_cast<unsigned *>(r_q + NWAVE), *r_slot = r_pr + NWAVE, *r_free = r_slot + NWAVE;
    unsigned short *sz = reinterpret_cast<unsigned short *>(visl_lds + cv.sz);
    unsigned short *stage = reinterpret_cast<unsigned short *>(visl_lds + cv.stage);  // [2][TPB·PQ]
    // ID, behind the carve: Aq, then Bs[m] and Pre[m + 1] (whole), or at 16 bytes the fence i64[m >> fshift] (fenced)
    long long *Aq = nullptr, *Bs_l = nullptr, *Pre_l = nullptr, *Fn = nullptr;
    if (ID) {
        Aq = reinterpret_cast<long long *>(visl_lds + cv.total);
        Bs_l = Aq + 1; Pre_l = Bs_l + A.m; Fn = Aq + 2;
    }

    const unsigned short *__restrict__ SL = GROUPED ? A.SL + g.sl : A.SL;
    unsigned short *Nrun = GROUPED ? A.N + g.tab : A.N + (size_t)run * m * Lmax * kpad;
    const size_t lstride = (size_t)Lmax * kpad;                       // elements per sample
    const unsigned short *__restrict__ start = A.init + (size_t)run * n;
    unsigned short *lab = A.labels + (size_t)run * n;                 // global: thread 0's from the first barrier on

    for (int x = tid; x < n; x += TPB) lo[x] = (unsigned)(unsigned long long)A.Gq[x];
    if (tid == 0) lo[n] = 0;
    if (tid >= 16 && tid < 32) oct[tid] = octave_entry(AL.split, 31 - tid);
    for (int k = tid; k < kpad; k += TPB) acc[k] = 0;
    for (int k = tid; k < Kcap + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (Kstride + 2) + k];
    for (int j = tid; j < n; j += TPB) lab[j] = start[j];
    if (ID) {
        if (tid == 0) Aq[0] = A.Aq0[run];
        if (A.tab_lds) {
            for (int s = tid; s < m; s += TPB) Bs_l[s] = A.Bs[s];
            for (int s = tid; s <= m; s += TPB) Pre_l[s] = A.Pre[s];
        } else {
            for (int t = tid; t < (m >> AL.fshift); t += TPB) Fn[t] = A.Bs[((t + 1) << AL.fshift) - 1];
        }
    }
    __syncthreads();
    int K = A.K0[run];
    if (K) {
        // the tables of the starting labels: one thread per sample (the only pass in which a thread writes elements
        // it does not own; the barrier below orders it before everything else)
        for (int s = tid; s < m; s += TPB) {
            unsigned short *Ns = Nrun + (size_t)s * lstride;
            for (int j = 0; j < n; ++j) {
                const unsigned l = start[j];
                if (l) Ns[(size_t)SL[(size_t)j * m + s] * kpad + (l - 1)] += 1;
            }
        }
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
    if (tid == 0) pub[0] = start[v.i];
    __syncthreads();

    long long moves = 0;
    int sweeps = 0, converged = 0;
    const unsigned long long key_new = key_i64(0);

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            // the next point's sample labels and (thread 0) its slot: issued now, parked in LDS behind the first barrier
            const int i = v.i, inext = v.ahead(t);
            unsigned short nxt[PQ ? PQ : 1];
            if (PQ) {
#pragma unroll
                for (int q = 0; q < PQ; ++q) {
                    const int s = tid + q * TPB;
                    nxt[q] = (s < m) ? SL[(size_t)inext * m + s] : (unsigned short)0;
                }
            }
            unsigned anext = 0;
            if (tid == 0) anext = lab[inext];
            const unsigned short *cur = PQ ? stage + (size_t)buf * TPB * PQ : SL + (size_t)i * m;

            // the slot i is in: published a step ago, unless i is the point that step moved (n = 1)
            const unsigned a = (i == v.iprev) ? v.wprev : pub[buf];

            // phase A: Σ_s Gq[N^s[l_s(i)][k]] for this thread's four slots over its samples, low words and high counts apart
            if (active) {
                const int ka = (int)a - 1 - c * VEC;
                const unsigned short *Nc = Nrun + (size_t)c * VEC;
                unsigned long long sum[VEC] = {0, 0, 0, 0};
                unsigned cnt[VEC] = {0, 0, 0, 0};
                int s = r;
                for (; s + 3 * R < m; s += 4 * R) {
                    const unsigned l0 = cur[s], l1 = cur[s + R], l2 = cur[s + 2 * R], l3 = cur[s + 3 * R];
                    const uint2 v0 = *reinterpret_cast<const uint2 *>(Nc + (size_t)s * lstride + (size_t)l0 * kpad);
                    const uint2 v1 = *reinterpret_cast<const uint2 *>(Nc + (size_t)(s + R) * lstride + (size_t)l1 * kpad);
                    const uint2 v2 = *reinterpret_cast<const uint2 *>(Nc + (size_t)(s + 2 * R) * lstride + (size_t)l2 * kpad);
                    const uint2 v3 = *reinterpret_cast<const uint2 *>(Nc + (size_t)(s + 3 * R) * lstride + (size_t)l3 * kpad);
                    add_row_l(v0, ka, lo, oct, sum, cnt); add_row_l(v1, ka, lo, oct, sum, cnt);
                    add_row_l(v2, ka, lo, oct, sum, cnt); add_row_l(v3, ka, lo, oct, sum, cnt);
                }
                for (; s < m; s += R) {
                    const unsigned l0 = cur[s];
                    add_row_l(*reinterpret_cast<const uint2 *>(Nc + (size_t)s * lstride + (size_t)l0 * kpad), ka, lo, oct, sum, cnt);
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const unsigned long long part = sum[e] + ((unsigned long long)cnt[e] << 32);
                    if (part) atomicAdd(&acc[c * VEC + e], part);
                }
            }
            __syncthreads();

            // phase B: score the slots (and clear their accumulators); thread k − 1 owns slot k
            if (PQ) {
#pragma unroll
                for (int q = 0; q < PQ; ++q) {
                    const int s = tid + q * TPB;
                    if (s < m) stage[(size_t)(buf ^ 1) * TPB * PQ + s] = nxt[q];
                }
            }
            if (tid == 0) pub[buf ^ 1] = anext;
            const unsigned emptied = (a && sz[a] == 1) ? 1u : 0u;
            Cand best{~0ull, ~0u, 0u, 0u};
            unsigned minfree = ~0u;
            if (tid < kpad) {
                const unsigned k = (unsigned)tid + 1u;
                const long long sum = (long long)acc[tid];
                acc[tid] = 0;
                if (k <= (unsigned)Kcap) {
                    const int nk = (int)sz[k] - (k == a ? 1 : 0);
                    long long idsc = 0;
                    if (ID) {
                        // F(A0 + Gq[n_k]) − F(A0) − acc_k; an empty slot runs the search too (nk = 0) and drops the result
                        const long long A0 = Aq[0] - (a ? gq_at((unsigned)sz[a] - 1u, lo, oct) : 0ll);
                        const long long A1 = A0 + gq_at((unsigned)nk, lo, oct);
                        long long F0, F1;
                        if (A.tab_lds) id_F2(Bs_l, Pre_l, m, A.nbits, A0, A1, F0, F1);
                        else id_F2_fenced(Fn, A.Bs, A.Pre, m, A.nbits, AL.fshift, A0, A1, F0, F1);
                        idsc = F1 - F0 - sum;
                    }
                    if (nk <= 0) minfree = k;
                    else best = Cand{key_i64(ID ? idsc : (long long)m * gq_at((unsigned)nk, lo, oct) - 2 * sum), (k == a) ? 0u : k, k, 0u};
                }
            }
            // argmin across the group (the second barrier), then the new-cluster candidate: while the cluster count is below
            // the cap there is a free slot in 1..Kcap
            greedy::group_argmin<false>(best, minfree, red, lane, wave);
            const int Know = K - (int)emptied;
            const unsigned isnew = Know < Kcap ? greedy::offer_new(best, key_new, emptied, a, minfree) : 0u;
            const unsigned w = best.slot;

            // phase C: put i into w.  A table element is touched only by the thread that reads it in phase A; sz is read by
            // the other threads only behind the next step's first barrier, the labels by none
            if (a != w && active) {
                const bool da = a && (int)(a - 1u) / VEC == c, dw = (int)(w - 1u) / VEC == c;
                if (da || dw) {
                    for (int s = r; s < m; s += R) {
                        unsigned short *row = Nrun + (size_t)s * lstride + (size_t)cur[s] * kpad;
                        if (da) row[a - 1u] = (unsigned short)(row[a - 1u] - 1u);
                        if (dw) row[w - 1u] = (unsigned short)(row[w - 1u] + 1u);
                    }
                }
            }
            if (tid == 0) {
                lab[i] = (unsigned short)w;
                if (ID && a != w) Aq[0] += gq_at(sz[w], lo, oct) - (a ? gq_at((unsigned)sz[a] - 1u, lo, oct) : 0ll);
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
            }
            moved += v.moved_to(a, w, inext);
            K = Know + (int)isnew;
            buf ^= 1;
        }
        ++sweeps;
        moves += moved;
        if (!moved) { converged = 1; break; }
        if (sweeps >= A.maxsweeps) break;
    }
    __syncthreads();

    // Q of the final labelling from the tables, with Φq (global memory: most cells are small, and the pass runs once)
    const long long *__restrict__ Phi = A.Phi;
    unsigned long long q = 0;
    if (ID) {
        if (tid == 0) {
            long long F0, F1;
            if (A.tab_lds) id_F2(Bs_l, Pre_l, m, A.nbits, Aq[0], Aq[0], F0, F1);
            else { id_F2_fenced(Fn, A.Bs, A.Pre, m, A.nbits, AL.fshift, Aq[0], Aq[0], F0, F1); F0 += A.Pre[m]; }
            q = (unsigned long long)F0;
        }
    } else if (tid < Kcap) q = (unsigned long long)((long long)m * Phi[sz[tid + 1]]);
    {
        unsigned long long t2 = 0;
        const uint2 *N2 = reinterpret_cast<const uint2 *>(Nrun);
        const size_t cells = (size_t)m * lstride / VEC;
        for (size_t x = tid; x < cells; x += TPB) {
            const uint2 c4 = N2[x];
            t2 += (unsigned long long)Phi[c4.x & 0xFFFFu] + (unsigned long long)Phi[c4.x >> 16] +
                  (unsigned long long)Phi[c4.y & 0xFFFFu] + (unsigned long long)Phi[c4.y >> 16];
        }
        q -= (ID ? 1 : 2) * t2;
    }
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

}  // namespace visearch

// Exact posterior expected VI search on the device: the greedy search of greedy.inc.hip (the mechanism and tie rules
// pointsearch.inc.hip has) for the criterion SALSO calls "VI" proper — the mean over the m samples of VI(c, sample) —
// instead of Wade & Ghahramani's lower bound.  This file is the device side — the kernel, its arguments and its LDS carve;
// the host side is visearch.inc.hip.  Included at the end of redclust_hip.hip behind greedy.inc.hip (the order walk, the
// sortable keys and the group argmin, the new-cluster candidate) TWICE: plainly it defines the declarations and
// k_visearch<PQ, LOSS>; with VIS_GROUPED defined, from the same text, k_vigroups<PQ> (below, "Grouped").  What is here: the
// two scores and their tables.
//
// Criterion (DESIGN.md §8 "Exact expected VI search"), φ(x) = x·log x:
//   n·m·E[VI](c) = m·Σ_k φ(n_k) + Σ_s Σ_l φ(n^s_l) − 2·Σ_s Σ_{k,l} φ(N^s_kl),   N^s_kl = #{j : c_j = k, c^s_j = l}
// in fixed point: Gq[x] = llrint((φ(x+1) − φ(x))·2^32), Φq(x) = Σ_{y<x} Gq[y], and the search minimises the integer
//   Q(c) = m·Σ_k Φq(n_k) − 2·Σ_s Σ_kl Φq(N^s_kl).
// With point i out of its cluster, putting it into k changes Q by exactly  Δ_k = m·Gq[n_k] − 2·Σ_s Gq[N^s[l_s(i)][k]]
// (Δ_new = 0), so a run is a pure integer function of its inputs and every accepted move lowers Q strictly.
//
// One run = one workgroup of 1024 threads, persistent over its sweeps; nruns workgroups per launch.
// Global memory, per run: the contingency tables u16 N[s][l][kpad] (kpad = Kcap rounded up to 4; a point's m rows
// N[s][l_s(i)][·] are each contiguous over k).  Shared by the runs: the samples, re-labelled per sample to 0..L_s−1 and
// transposed to SL[i][s], so the m labels of the visited point are contiguous.
// A table row is covered by G = kpad/4 threads of 8 bytes (4 slots) each; thread (r, c) = (tid / G, tid % G) takes the
// samples r, r + R, … (R = 1024 / G rows per pass) and the slots 4c..4c+3 of each.  Every table element is only ever
// read (phase A) and written (phase C) by that one thread, so the tables need no barrier of their own.
// A step: (A) each thread adds Gq[N] of its slots over its samples into four registers, then into the per-slot LDS
// accumulators with 64-bit integer atomics (order-free); barrier; (B) thread k − 1 scores slot k, argmin by greedy's
// sortable keys; barrier; (C) every thread reads the 16 partials, adds the new-cluster candidate; lab / sz are written
// by thread 0, N[s][l][a] −= 1 and N[s][l][w] += 1 by the owners of those slots (nothing when a = w).  Two barriers per
// step.  The next point's m sample labels are loaded into registers at the top of a step and parked in the other half
// of an LDS double buffer behind the first barrier (m ≤ 4096; beyond that they are read from global memory in place).
//
// LDS (dynamic, carved at 16-byte offsets): Gq i64[n+1] (64 KiB at n = 8192; Φq at the end), acc u64[kpad], the
// reduction partials, sz u16[Kcap+2], lab u16[n], the label double buffer u16[2][1024·PQ]: 109 024 B at the largest sizes.
//
// The same kernel searches the posterior expected information distance (LOSS = LOSS_ID, rc_id_search; DESIGN.md §8 "Exact
// expected ID search"):  n·m·E[ID](c) = F(A(c)) − Σ_s Σ_kl φ(N^s_kl),  A(c) = Σ_k φ(n_k),  F(x) = Σ_s max(x, B_s),
// B_s = Σ_l φ(n^s_l).  In fixed point Q_ID(c) = Σ_s max(Aq(c), Bq_s) − Σ_s Σ_kl Φq(N^s_kl), and with Bs the Bq_s sorted
// ascending, Pre their prefix sums and p(x) = #{t : Bs[t] <= x}:  F(x) = x·p(x) + Pre[m] − Pre[p(x)].  Phase A is the VI
// search's; phase B scores slot k as F(A₀ + Gq[n_k]) − F(A₀) − acc_k, A₀ = Aq without the visited point; thread 0 keeps Aq
// (LDS) up to date in phase C under sz's discipline.  Behind the carve above: Aq, then Bs i64[m] and Pre i64[m+1] — 16·(m+1)
// bytes with Aq — when that fits the 160 KiB, else 16 bytes for Aq and the two tables are read from global memory.
//
// Grouped (k_vigroups<PQ>: the same text with the compile-time constant GROUPED = true, LOSS_VI only; rc_vi_search_groups;
// DESIGN.md §8 "Several-partition summary"): every run sums over its own group of the samples.  The host lays the transposed
// samples out group by group (block g is n × m_g) and a run reads its sample count, the offsets of its group's block and of
// its tables, its largest L_s and its slot cap from its GroupRun; kpad, G, R, PQ and the carve stay the launch's, sized by the
// largest cap and the largest group (a run with fewer samples than R rows has idle rows, slots above a run's cap are never
// scored).  k_visearch takes none of these branches.
// One text, two kernels of different names: a call through a shared device function changes the compiler's register
// allocation of k_visearch, a constant folded at the top of the kernel does not — the six k_visearch kernels compile to the
// instructions they had before the grouped one existed.

namespace visearch {

#ifndef VIS_GROUPED
using greedy::TPB, greedy::NWAVE, greedy::Cand, greedy::key_i64;
constexpr int KCAP_MAX = 1024;                        // one slot per thread in phase B
constexpr int VEC = 4;                                // slots per thread in a table row (8 bytes)
constexpr long long MN_MAX = 1ll << 26;               // |Q| <= 2·m·n·log(n)·2^32 < 2^63
constexpr size_t TABLE_BUDGET = (size_t)4 << 30;      // bytes of contingency tables, all runs together
constexpr int STAGE_Q = 4;                            // labels of the next point staged in LDS while m <= 1024·STAGE_Q
constexpr size_t LDS_MAX = 160 * 1024;                // of a gfx950 CU, all of which one workgroup may take
constexpr int LOSS_VI = 0, LOSS_ID = 1;

struct RunOut {
    long long Q, moves;
    int sweeps, converged, K, pad_;
};

// GROUPED: what a run reads of its own group (rc_vi_search_groups): the group's samples, where its block of SL starts, where the
// run's tables start (both in elements), the group's largest L_s and its slot cap
struct GroupRun {
    unsigned long long sl, tab;
    int m, Lmax, Kcap, pad_;
};

struct Args {
    const long long *Gq;          // n entries
    const long long *Phi;         // n + 1 entries
    const unsigned short *SL;     // n × m per-sample labels, 0-based
    unsigned short *N;            // nruns × m × Lmax × kpad, zeroed
    const unsigned short *init;   // nruns × n slots, 0 = unallocated
    const unsigned short *sz0;    // nruns × (Kcap + 2) slot sizes of init
    const int *K0;                // clusters of init
    const int *order;             // nruns × n, 0-based
    unsigned short *labels;       // nruns × n out (slots)
    RunOut *out;
    int n, m, Lmax, kpad, Kcap, maxsweeps;
    // LOSS_ID only
    const long long *Bs;          // m: the samples' Σ_l Φq(n^s_l), ascending
    const long long *Pre;         // m + 1: Pre[p] = Σ_{t<p} Bs[t]
    const long long *Aq0;         // nruns: Σ_k Φq(n_k) of init
    int nbits;                    // trip count of the search for p(x): ceil(log2(m + 1))
    int tab_lds;                  // Bs and Pre are copied to LDS behind Aq
    // GROUPED only (behind everything else: the other instantiations' arguments stay where they were).  m, Lmax, Kcap above are
    // then the largest of any run — what PQ, the carve and the stride of sz0 are sized by — and SL holds the groups' blocks, n × m_g each
    const GroupRun *runs;         // nruns
};

__host__ __device__ inline size_t up16(size_t x) { return (x + 15) / 16 * 16; }

struct Carve {
    size_t gq, acc, red, sz, lab, stage, total;
    __host__ __device__ Carve(int n, int kpad, int Kcap, int PQ)
    {
        gq = 0;
        acc = gq + up16(8 * (size_t)(n + 1));
        red = acc + up16(8 * (size_t)kpad);
        sz = red + up16((size_t)NWAVE * (8 + 8 + 4 + 4 + 4));
        lab = sz + up16(2 * (size_t)(Kcap + 2));
        stage = lab + up16(2 * (size_t)n);
        total = stage + up16(2 * 2 * (size_t)TPB * PQ);
    }
};

// ID: (F(x0), F(x1)) from the sorted table, both searches in one loop of nbits trips (the same for every thread)
template <typename P>
__device__ inline void id_F2(P Bs, P Pre, int m, int nbits, long long x0, long long x1, long long &F0, long long &F1)
{
    int p0 = 0, p1 = 0;
    for (int b = nbits - 1; b >= 0; --b) {
        const int q0 = p0 + (1 << b), q1 = p1 + (1 << b);
        const long long b0 = Bs[min(q0, m) - 1], b1 = Bs[min(q1, m) - 1];
        if (q0 <= m && b0 <= x0) p0 = q0;
        if (q1 <= m && b1 <= x1) p1 = q1;
    }
    const long long tot = Pre[m];
    F0 = x0 * p0 + tot - Pre[p0];
    F1 = x1 * p1 + tot - Pre[p1];
}

__device__ inline void add_row(const uint2 v, int ka, const long long *Gq, long long (&acc)[VEC])
{
    // ka: where the visited point's own slot sits in this thread's four, if it does — the point itself is out
    const unsigned x0 = (v.x & 0xFFFFu) - (ka == 0 ? 1u : 0u), x1 = (v.x >> 16) - (ka == 1 ? 1u : 0u);
    const unsigned x2 = (v.y & 0xFFFFu) - (ka == 2 ? 1u : 0u), x3 = (v.y >> 16) - (ka == 3 ? 1u : 0u);
    acc[0] += Gq[x0]; acc[1] += Gq[x1]; acc[2] += Gq[x2]; acc[3] += Gq[x3];
}

#endif
#ifdef VIS_GROUPED
template <int PQ>
__global__ __launch_bounds__(TPB) void k_vigroups(Args A)
{
    constexpr int LOSS = LOSS_VI;
    constexpr bool GROUPED = true;
#else
template <int PQ, int LOSS>
__global__ __launch_bounds__(TPB) void k_visearch(Args A)
{
    constexpr bool GROUPED = false;
#endif
    static_assert(!GROUPED || LOSS == LOSS_VI, "only the VI criterion is grouped");
    extern __shared__ __attribute__((aligned(16))) unsigned char vis_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, kpad = A.kpad, run = blockIdx.x;
    GroupRun g{};
    if (GROUPED) g = A.runs[run];
    const int m = GROUPED ? g.m : A.m, Lmax = GROUPED ? g.Lmax : A.Lmax, Kcap = GROUPED ? g.Kcap : A.Kcap;
    const int Kstride = GROUPED ? A.Kcap : Kcap;                      // the launch's largest cap: the carve and sz0's rows

    const Carve cv(n, kpad, Kstride, PQ);
    long long *Gq = reinterpret_cast<long long *>(vis_lds + cv.gq);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(vis_lds + cv.acc);
    unsigned long long *r_sc = reinterpret_cast<unsigned long long *>(vis_lds + cv.red);
    unsigned long long *r_q = r_sc + NWAVE;
    unsigned *r_pr = reinterpret_cast<unsigned *>(r_q + NWAVE), *r_slot = r_pr + NWAVE, *r_free = r_slot + NWAVE;
    unsigned short *sz = reinterpret_cast<unsigned short *>(vis_lds + cv.sz);
    unsigned short *lab = reinterpret_cast<unsigned short *>(vis_lds + cv.lab);
    unsigned short *stage = reinterpret_cast<unsigned short *>(vis_lds + cv.stage);   // [2][TPB·PQ]
    long long *Aq = reinterpret_cast<long long *>(vis_lds + cv.total);                // ID: Aq, Bs[m], Pre[m + 1]
    long long *Bs_l = Aq + 1, *Pre_l = Bs_l + m;

    const unsigned short *__restrict__ SL = GROUPED ? A.SL + g.sl : A.SL;
    unsigned short *Nrun = GROUPED ? A.N + g.tab : A.N + (size_t)run * m * Lmax * kpad;
    const size_t lstride = (size_t)Lmax * kpad;                       // elements per sample

    for (int x = tid; x < n; x += TPB) Gq[x] = A.Gq[x];
    for (int k = tid; k < kpad; k += TPB) acc[k] = 0;
    for (int k = tid; k < Kcap + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (Kstride + 2) + k];
    for (int j = tid; j < n; j += TPB) lab[j] = A.init[(size_t)run * n + j];
    if (LOSS == LOSS_ID) {
        if (tid == 0) Aq[0] = A.Aq0[run];
        if (A.tab_lds) {
            for (int s = tid; s < m; s += TPB) Bs_l[s] = A.Bs[s];
            for (int s = tid; s <= m; s += TPB) Pre_l[s] = A.Pre[s];
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
                const unsigned l = lab[j];
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
    __syncthreads();

    long long moves = 0;
    int sweeps = 0, converged = 0;
    const unsigned long long key_new = key_i64(0);

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            // the next point's sample labels: issued now, parked in LDS behind the first barrier
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

            // phase A: Σ_s Gq[N^s[l_s(i)][k]] for this thread's four slots over its samples
            if (active) {
                const int ka = (int)a - 1 - c * VEC;
                const unsigned short *Nc = Nrun + (size_t)c * VEC;
                long long part[VEC] = {0, 0, 0, 0};
                int s = r;
                for (; s + 3 * R < m; s += 4 * R) {
                    const unsigned l0 = cur[s], l1 = cur[s + R], l2 = cur[s + 2 * R], l3 = cur[s + 3 * R];
                    const uint2 v0 = *reinterpret_cast<const uint2 *>(Nc + (size_t)s * lstride + (size_t)l0 * kpad);
                    const uint2 v1 = *reinterpret_cast<const uint2 *>(Nc + (size_t)(s + R) * lstride + (size_t)l1 * kpad);
                    const uint2 v2 = *reinterpret_cast<const uint2 *>(Nc + (size_t)(s + 2 * R) * lstride + (size_t)l2 * kpad);
                    const uint2 v3 = *reinterpret_cast<const uint2 *>(Nc + (size_t)(s + 3 * R) * lstride + (size_t)l3 * kpad);
                    add_row(v0, ka, Gq, part); add_row(v1, ka, Gq, part); add_row(v2, ka, Gq, part); add_row(v3, ka, Gq, part);
                }
                for (; s < m; s += R) {
                    const unsigned l0 = cur[s];
                    add_row(*reinterpret_cast<const uint2 *>(Nc + (size_t)s * lstride + (size_t)l0 * kpad), ka, Gq, part);
                }
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (part[e]) atomicAdd(&acc[c * VEC + e], (unsigned long long)part[e]);
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
                    if (LOSS == LOSS_ID) {
                        // F(A0 + Gq[n_k]) − F(A0) − acc_k; an empty slot runs the search too (nk = 0) and drops the result
                        const long long A0 = Aq[0] - (a ? Gq[sz[a] - 1] : 0ll);
                        long long F0, F1;
                        if (A.tab_lds) id_F2(Bs_l, Pre_l, m, A.nbits, A0, A0 + Gq[nk], F0, F1);
                        else id_F2(A.Bs, A.Pre, m, A.nbits, A0, A0 + Gq[nk], F0, F1);
                        idsc = F1 - F0 - sum;
                    }
                    if (nk <= 0) minfree = k;
                    else best = Cand{key_i64(LOSS == LOSS_ID ? idsc : (long long)m * Gq[nk] - 2 * sum), (k == a) ? 0u : k, k, 0u};
                }
            }
            // argmin across the group (the second barrier), then the new-cluster candidate: while the cluster count is below
            // the cap there is a free slot in 1..Kcap
            greedy::group_argmin<false>(best, minfree, red, lane, wave);
            const int Know = K - (int)emptied;
            const unsigned isnew = Know < Kcap ? greedy::offer_new(best, key_new, emptied, a, minfree) : 0u;
            const unsigned w = best.slot;

            // phase C: put i into w.  A table element is touched only by the thread that reads it in phase A; lab and sz
            // are read by the other threads only behind the next step's first barrier
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
                if (LOSS == LOSS_ID && a != w) Aq[0] += Gq[sz[w]] - (a ? Gq[sz[a] - 1] : 0ll);
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

    // Q of the final labelling from the tables, with Φq in place of Gq
    for (int j = tid; j < n; j += TPB) A.labels[(size_t)run * n + j] = lab[j];
    for (int x = tid; x <= n; x += TPB) Gq[x] = A.Phi[x];
    __syncthreads();
    unsigned long long q = 0;
    if (LOSS == LOSS_ID) {
        if (tid == 0) {
            long long F0, F1;
            if (A.tab_lds) id_F2(Bs_l, Pre_l, m, A.nbits, Aq[0], Aq[0], F0, F1);
            else id_F2(A.Bs, A.Pre, m, A.nbits, Aq[0], Aq[0], F0, F1);
            q = (unsigned long long)F0;
        }
    } else if (tid < Kcap) q = (unsigned long long)((long long)m * Gq[sz[tid + 1]]);
    {
        unsigned long long t2 = 0;
        const uint2 *N2 = reinterpret_cast<const uint2 *>(Nrun);
        const size_t cnt = (size_t)m * lstride / VEC;
        for (size_t x = tid; x < cnt; x += TPB) {
            const uint2 v = N2[x];
            t2 += (unsigned long long)Gq[v.x & 0xFFFFu] + (unsigned long long)Gq[v.x >> 16] +
                  (unsigned long long)Gq[v.y & 0xFFFFu] + (unsigned long long)Gq[v.y >> 16];
        }
        q -= (LOSS == LOSS_ID ? 1 : 2) * t2;
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

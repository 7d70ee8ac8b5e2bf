// MAP search on the device: the greedy search of greedy.inc.hip (the mechanism and tie rules pointsearch.inc.hip and
// visearch.inc.hip have) for the labelling of maximum log-posterior loglik + logprior (src/mcmc.jl:1-78) under a context's
// matrices — the quantity mapestimate and getpointestimate rank by.  DESIGN.md §8 "MAP search"; the contract is in
// include/redclust_hip.h.  Included at the end of redclust_hip.hip behind score.inc.hip (same translation unit: shares fail(),
// HIPCHK, View, make_view, rc_load_L, sync_and_check, check_params, the holders and checks of hostutil.inc.hip, the order
// walk, the sortable keys, the group argmin, the new-cluster candidate and the staging of greedy.inc.hip, and scr::score_valid
// of score.inc.hip, which recomputes everything that is reported; lgamma_pos and log1p_lean of mapmath.inc.hpp).
//
// Criterion.  The sufficient statistics of a labelling are its cluster sizes and the K×K block sums of D and logD,
// B_X[k][t] = Σ_{i in k} Σ_{j in t} Xq[i][j] (rc_score_labellings' blocks: D's stored diagonal travels with its point into
// B_D[k][k], logD's is 0; D is symmetric, so B[k][t] = B[t][k] and both are kept).  With P_k = n_k(n_k−1)/2,
//   within(k)     = (δ1−1)·B_L[k][k]/2 − P_k·lgΓ(δ1) + lgΓ(α+δ1·P_k) − lgΓ(α) − δ1·P_k·log β − (α+δ1·P_k)·log1p(B_D[k][k]/(2β))
//   between(k, t) = (δ2−1)·B_L[k][t] − n_k·n_t·lgΓ(δ2) + lgΓ(ζ+δ2·n_k·n_t) − lgΓ(ζ) − δ2·n_k·n_t·log γ − (ζ+δ2·n_k·n_t)·log1p(B_D[k][t]/γ)
// (the regrouping of ll_within_term / ll_between_term, hostmodel.inc.hpp, in f64), between counted only with repulsion.
//
// One visit of point i, taken out of its slot a.  (A) row i is reduced into exact per-slot sums over j != i, s_t = Σ_{j in t}
// Dq[i][j] and l_t for Lq, with 64-bit integer LDS atomics (order-free); barrier.  (B) every occupied slot k is scored,
//   Δ_k   = within(k ∪ i) − within(k) + Σ_{t != k} [between(k ∪ i, t) − between(k, t)] + log(n_k+1) − log n_k + log(n_k+r−1) + log p
//   Δ_new = within({i}) + Σ_t between({i}, t) + log(K+1) + r·log(1−p)
// where adding i to k changes B_D[k][k] by 2·s_k + Dq[i][i] and B_D[k][t] by s_t (B_L alike, no diagonal), and the blocks of a
// with i out are the stored ones less the same terms.  Candidate 0 is the new cluster, candidate k >= 1 slot k.  With repulsion
// a wave owns a candidate (wave, wave + 8, …): its lanes take the items t = lane, lane + 64, … in that order — t = k the
// candidate's own within difference, any other occupied t a between difference — and an xor tree adds the 64 partials, so Δ_k
// is a fixed function of the run's state whatever else shares the launch.  Without repulsion a thread takes the candidates tid,
// tid + 512, … and there is no K² loop.  Argmin of (−Δ, priority) by greedy's keys (the second barrier), then the new-cluster
// candidate.
// (C) if i moved, thread t adds to and takes from the cells (a, t), (t, a), (w, t), (t, w) the row sums the move is made of —
// O(K), every cell by one thread, never a block reduced again; thread 0 writes lab and sz.
//
// State.  LDS: lab u16[n], sz u16[Kcap+2], two generations of the (s, l) accumulators u64[2][2][Kcap+1] (a visit clears the
// other generation behind its first barrier), the partials of the argmin.  Global memory, per run: Kcap² cells of four int64,
// (D_hi, D_lo, L_hi, L_lo) with value = hi·2^24 + lo as rc_score_labellings carries a block — every row sum enters as its two
// halves, so a block beyond 63 bits cannot overflow.  One workgroup writes and re-reads its cells across barriers (as k_hclust
// its matrices).  The cells of the starting labels are built by the same row pass, one point after the other, before the sweeps.
//
// What is exact: the row sums, the blocks, and therefore the state a decision is taken on.  What is floating point: Δ (f64,
// lgamma_pos and log1p_lean of mapmath.inc.hpp), which decides moves only; nothing the kernel computes in floating point is reported.

namespace mapsearch {

using greedy::NWAVE, greedy::Cand, greedy::key_f64;
// 512 threads: the f64 lgamma and log1p beside the cell arithmetic need more than the 128 VGPRs that 1024 threads leave a lane,
// and 8 waves (two per SIMD) may have 256.  group_argmin merges greedy's 16 partials: the upper 8 are set once to "no candidate".
constexpr int TPB = 512, WAVES = TPB / 64;
constexpr int KCAP_MAX = 1024;                         // Kcap² cells per run
constexpr size_t CELL_BUDGET = (size_t)1 << 30;        // bytes of block cells per launch: more runs go in several launches
constexpr long long LO_MASK = ((long long)1 << RC_LO_BITS) - 1;

struct RunOut {
    long long moves;
    int sweeps, converged, K, capped;
};

// the likelihood's constants in f64
struct Consts { double d1, d2, al, be, ze, ga, lgd1, lgd2, lb, lg, scD, scL; };

struct Args {
    Consts C;
    const unsigned short *init;   // nruns × n slots, 0 = unallocated
    const unsigned short *sz0;    // nruns × (Kcap + 2) slot sizes of init
    const int *K0;                // clusters of init
    const int *order;             // nruns × n, 0-based
    const double *r, *p;          // nruns
    unsigned short *labels;       // nruns × n out (slots)
    RunOut *out;
    long long *cells;             // (runs of this launch) × Kcap × Kcap × 4, zeroed
    int n, Kcap, maxsweeps, run0, implicit_cap;
};

__host__ __device__ inline size_t up16(size_t x) { return (x + 15) / 16 * 16; }

struct Carve {
    size_t acc, red, sz, lab, total;
    __host__ __device__ Carve(int n, int Kcap)
    {
        acc = 0;
        red = acc + up16(4 * 8 * (size_t)(Kcap + 1));
        sz = red + up16((size_t)NWAVE * (8 + 4 + 4 + 4) + 8);
        lab = sz + up16(2 * (size_t)(Kcap + 2));
        total = lab + up16(2 * (size_t)n);
    }
};

struct Cell { long long dh, dl, lh, ll; };

__device__ inline Cell cell_load(const long long *q)
{
    const ll2 a = *reinterpret_cast<const ll2 *>(q), b = *reinterpret_cast<const ll2 *>(q + 2);
    return Cell{a.x, a.y, b.x, b.y};
}
__device__ inline void cell_store(long long *q, const Cell &c)
{
    ll2 a, b;
    a.x = c.dh; a.y = c.dl; b.x = c.lh; b.y = c.ll;
    *reinterpret_cast<ll2 *>(q) = a; *reinterpret_cast<ll2 *>(q + 2) = b;
}
// sign times the row sums (d, l) as their halves
__device__ inline void cell_add(Cell &c, long long d, long long l, long long sign)
{
    c.dh += sign * (d >> RC_LO_BITS); c.dl += sign * (d & LO_MASK);
    c.lh += sign * (l >> RC_LO_BITS); c.ll += sign * (l & LO_MASK);
}
// the value of a pair of halves, rounded once
__device__ inline double halves_f64(long long hi, long long lo) { return (double)hi * (double)((long long)1 << RC_LO_BITS) + (double)lo; }

// within and between are one form: (d−1)·bl − pairs·lgΓ(d) + lgΓ(a0 + d·pairs) − d·pairs·log(base) − (a0 + d·pairs)·log1p(bd/base),
// with (d, a0, base) = (δ1, α, β) and the block halved for within, (δ2, ζ, γ) for between; the constant −lgΓ(a0) is left out:
// only differences of two terms of one kind are ever taken.  One function and one call of it in the kernel (k_mapsearch, phase B).
struct TermC { double d, a0, lgd, lbase, base, fD, fL; };
__device__ inline double term(const TermC &T, double pairs, double bd, double bl)
{
    const double a = T.a0 + T.d * pairs;
    return (T.d - 1.0) * bl - pairs * T.lgd + lgamma_pos(a) - T.d * pairs * T.lbase - a * log1p_lean(bd / T.base);
}

__device__ inline double xor_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += __longlong_as_double((long long)greedy::shfl_xor_u64((unsigned long long)__double_as_longlong(v), off));
    return v;
}

// Row i of the matrices (caller's order, through V.pi) into the per-slot accumulators: every allocated j != i, its slot taken
// from lab — the previous visit's point from the registers, its lab entry may not have landed yet
__device__ inline void row_sums(const View &V, int i, int n, const unsigned short *lab, int iprev, unsigned wprev, u64 *accS, u64 *accL, int tid)
{
    const int u = V.pi[i];
    for (int j = tid; j < n; j += TPB) {
        const unsigned slot = (j == iprev) ? wprev : (unsigned)lab[j];
        if (j == i || slot == 0) continue;
        const int x = V.pi[j];
        const size_t e = (size_t)u * V.ld + x;
        const long long d = (V.bits == 64) ? ((const long long *)V.Dq)[e] : (long long)((const int *)V.Dq)[e];
        const long long l = rc_load_L(V, u, x, d);
        atomicAdd(&accS[slot], (u64)d);
        atomicAdd(&accL[slot], (u64)l);
    }
}

template <bool REP>
__global__ __launch_bounds__(TPB) void k_mapsearch(View V, Args A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char map_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, Kcap = A.Kcap, run = A.run0 + blockIdx.x;
    const Consts C = A.C;

    const Carve cv(n, Kcap);
    u64 *acc = reinterpret_cast<u64 *>(map_lds + cv.acc);                 // [generation][S, L][Kcap + 1]
    unsigned long long *r_sc = reinterpret_cast<unsigned long long *>(map_lds + cv.red);
    double *r_new = reinterpret_cast<double *>(r_sc + NWAVE);
    unsigned *r_pr = reinterpret_cast<unsigned *>(r_new + 1), *r_slot = r_pr + NWAVE, *r_free = r_slot + NWAVE;
    unsigned short *sz = reinterpret_cast<unsigned short *>(map_lds + cv.sz);
    unsigned short *lab = reinterpret_cast<unsigned short *>(map_lds + cv.lab);
    long long *cells = A.cells + (size_t)blockIdx.x * Kcap * Kcap * 4;
    const auto cell = [&](unsigned k, unsigned t) { return cells + ((size_t)(k - 1u) * Kcap + (t - 1u)) * 4; };
    const int astride = Kcap + 1;

    for (int k = tid; k < 4 * astride; k += TPB) acc[k] = 0;
    if (tid >= WAVES && tid < NWAVE) { r_sc[tid] = ~0ull; r_pr[tid] = ~0u; r_slot[tid] = 0u; r_free[tid] = ~0u; }
    for (int k = tid; k < Kcap + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (Kcap + 2) + k];
    for (int j = tid; j < n; j += TPB) lab[j] = A.init[(size_t)run * n + j];
    __syncthreads();
    int K = A.K0[run];
    unsigned hi = (unsigned)K;                                            // the highest slot ever occupied
    const double rr = A.r[run], logp = log(A.p[run]), rlog1mp = rr * log1p_lean(-A.p[run]);
    const TermC TW{C.d1, C.al, C.lgd1, C.lb, C.be, 0.5 * C.scD, 0.5 * C.scL};
    const TermC TB{C.d2, C.ze, C.lgd2, C.lg, C.ga, C.scD, C.scL};

    // the cells of the starting labels: row i of B is the sum of its points' row sums
    if (K) {
        u64 *accS = acc, *accL = acc + astride;
        for (int i = 0; i < n; ++i) {
            const unsigned a = lab[i];
            if (!a) continue;
            row_sums(V, i, n, lab, -1, 0u, accS, accL, tid);
            __syncthreads();
            for (unsigned t = (unsigned)tid + 1u; t <= hi; t += TPB) {
                long long d = (long long)accS[t];
                const long long l = (long long)accL[t];
                accS[t] = 0; accL[t] = 0;
                Cell c = cell_load(cell(a, t));
                cell_add(c, d, l, 1);
                if (t == a) {
                    const size_t e = (size_t)V.pi[i] * V.ld + V.pi[i];
                    d = (V.bits == 64) ? ((const long long *)V.Dq)[e] : (long long)((const int *)V.Dq)[e];
                    cell_add(c, d, 0, 1);
                }
                cell_store(cell(a, t), c);
            }
            __syncthreads();
        }
    }

    const greedy::Partials red{r_sc, r_pr, r_slot, r_free, nullptr};
    greedy::Visit v(A.order + (size_t)run * n, n);
    long long moves = 0;
    int sweeps = 0, converged = 0, capped = 0, gen = 0;

    for (;;) {
        int moved = 0;
        for (int t_ = 0; t_ < n; ++t_) {
            const int i = v.i, inext = v.ahead(t_);
            const unsigned a = v.slot_of(lab);
            u64 *accS = acc + (size_t)gen * 2 * astride, *accL = accS + astride;
            u64 *other = acc + (size_t)(gen ^ 1) * 2 * astride;
            const size_t ediag = (size_t)V.pi[i] * V.ld + V.pi[i];
            const long long dii = (V.bits == 64) ? ((const long long *)V.Dq)[ediag] : (long long)((const int *)V.Dq)[ediag];

            // phase A: the row sums
            row_sums(V, i, n, lab, v.iprev, v.wprev, accS, accL, tid);
            __syncthreads();

            // phase B: the scores; the other generation of the accumulators is cleared for the next visit
            for (int k = tid; k < 2 * astride; k += TPB) other[k] = 0;
            const unsigned emptied = (a && sz[a] == 1) ? 1u : 0u;
            const int Know = K - (int)emptied;
            const bool offered = Know < Kcap;
            Cand best{~0ull, ~0u, 0u, 0u};
            unsigned minfree = ~0u;

            // The change of one term when i joins candidate c (nk members with i out, row sums sk, lk; c = 0: the new cluster,
            // nk = 0): t = c is the candidate's own within term, any other t its between term with the occupied slot t.  Old and
            // new value come from the same call in a loop of two trips.
            const auto item = [&](unsigned c, unsigned t, int nk, long long sk, long long lk) {
                const bool own = t == c;
                const int nt = own ? nk : (int)sz[t] - (t == a ? 1 : 0);
                const long long st = own ? sk : (long long)accS[t], lt = own ? lk : (long long)accL[t];
                Cell q{0, 0, 0, 0};
                if (c) {
                    q = cell_load(cell(c, t));
                    if (c == a) cell_add(q, st, lt, own ? -2 : -1);
                    if (c == a && own) cell_add(q, dii, 0, -1);
                    if (t == a && !own) cell_add(q, sk, lk, -1);
                }
                Cell q1 = q;
                cell_add(q1, st, lt, own ? 2 : 1);
                if (own) cell_add(q1, dii, 0, 1);
                const double pairs0 = own ? 0.5 * (double)nk * (double)(nk - 1) : (double)nk * (double)nt;
                const double pairs1 = pairs0 + (double)nt;
                const TermC T = own ? TW : TB;
                double d = 0.0;
#pragma nounroll
                for (int e = 0; e < 2; ++e) {
                    const double val = term(T, e ? pairs1 : pairs0, halves_f64(e ? q1.dh : q.dh, e ? q1.dl : q.dl) * T.fD,
                                            halves_f64(e ? q1.lh : q.lh, e ? q1.ll : q.ll) * T.fL);
                    d = e ? d + val : -val;
                }
                return d;
            };
            // candidate c's Δ from the sum of its items: the prior's terms; the new cluster's goes to r_new, a slot's into best
            const auto finish = [&](unsigned c, int nk, double sum, bool writer) {
                if (!c) {
                    if (writer) r_new[0] = sum + log((double)(Know + 1)) + rlog1mp;
                    return;
                }
                const double delta = sum + (log((double)(nk + 1)) - log((double)nk) + log((double)nk + rr - 1.0) + logp);
                const unsigned long long key = key_f64(-delta);
                const unsigned pr = (c == a) ? 0u : c;
                if (greedy::better(key, pr, best)) best = Cand{key, pr, c, 0u};
            };

            // candidate 0 is the new cluster, candidate k >= 1 slot k.  With repulsion a wave takes a candidate and its lanes the
            // items t = lane, lane + 64, … in that order, an xor tree adds the partials; without, a thread takes a candidate
            const unsigned cstep = REP ? (unsigned)WAVES : (unsigned)TPB;
            for (unsigned c = REP ? (unsigned)wave : (unsigned)tid; c <= hi; c += cstep) {
                const int nk = c ? (int)sz[c] - (c == a ? 1 : 0) : 0;
                if (c && nk <= 0) { minfree = min(minfree, c); continue; }
                if (!c && !offered) continue;
                const long long sk = c ? (long long)accS[c] : 0ll, lk = c ? (long long)accL[c] : 0ll;
                if (REP) {
                    double part = 0.0;
                    for (unsigned t = (unsigned)lane; t <= hi; t += 64u) {
                        if (t != c && (t == 0u || (int)sz[t] - (t == a ? 1 : 0) <= 0)) continue;
                        part += item(c, t, nk, sk, lk);
                    }
                    finish(c, nk, xor_sum(part), lane == 0);
                } else {
                    finish(c, nk, item(c, c, nk, sk, lk), true);
                }
            }
            if (hi < (unsigned)Kcap) minfree = min(minfree, hi + 1u);
            // argmin across the group (the second barrier), then the new-cluster candidate: while the cluster count is below
            // the cap there is a free slot in 1..Kcap
            greedy::group_argmin<false>(best, minfree, red, lane, wave);
            unsigned isnew = 0u;
            if (offered) isnew = greedy::offer_new(best, key_f64(-r_new[0]), emptied, a, minfree);
            else if (A.implicit_cap) ++capped;
            const unsigned w = best.slot;

            // phase C: put i into w.  Cell (x, y) changes by −[x = a]·s_y − [y = a]·s_x + [x = w]·s_y + [y = w]·s_x and D's diagonal
            // entry on (a, a) and (w, w).  Thread t owns the cells (a, t) and (w, t) and, for t outside {a, w}, (t, a) and (t, w).
            if (a != w) {
                if (w > hi) hi = w;
                const long long sa = a ? (long long)accS[a] : 0ll, la = a ? (long long)accL[a] : 0ll;
                const long long sw = (long long)accS[w], lw = (long long)accL[w];
                for (unsigned t = (unsigned)tid + 1u; t <= hi; t += TPB) {
                    const long long st = (long long)accS[t], lt = (long long)accL[t];
                    if (a) {
                        Cell c = cell_load(cell(a, t));
                        cell_add(c, st, lt, -1);
                        if (t == a) { cell_add(c, sa, la, -1); cell_add(c, dii, 0, -1); }
                        if (t == w) cell_add(c, sa, la, 1);
                        cell_store(cell(a, t), c);
                    }
                    {
                        Cell c = cell_load(cell(w, t));
                        cell_add(c, st, lt, 1);
                        if (t == w) { cell_add(c, sw, lw, 1); cell_add(c, dii, 0, 1); }
                        if (a && t == a) cell_add(c, sw, lw, -1);
                        cell_store(cell(w, t), c);
                    }
                    if (t != a && t != w) {
                        if (a) {
                            Cell c = cell_load(cell(t, a));
                            cell_add(c, st, lt, -1);
                            cell_store(cell(t, a), c);
                        }
                        Cell c = cell_load(cell(t, w));
                        cell_add(c, st, lt, 1);
                        cell_store(cell(t, w), c);
                    }
                }
            }
            if (tid == 0) {
                lab[i] = (unsigned short)w;
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
            }
            moved += v.moved_to(a, w, inext);
            K = Know + (int)isnew;
            gen ^= 1;
        }
        ++sweeps;
        moves += moved;
        if (!moved) { converged = 1; break; }
        if (sweeps >= A.maxsweeps) break;
    }
    __syncthreads();

    for (int j = tid; j < n; j += TPB) A.labels[(size_t)run * n + j] = lab[j];
    if (tid == 0) {
        RunOut o{};
        o.moves = moves; o.sweeps = sweeps; o.converged = converged; o.K = K; o.capped = capped;
        A.out[run] = o;
    }
}

static hipError_t launch(bool rep, int runs, size_t lds, const View &V, const Args &A)
{
    hipError_t e = rep ? set_dynamic_lds(k_mapsearch<true>, lds) : set_dynamic_lds(k_mapsearch<false>, lds);
    if (e != hipSuccess) return e;
    if (rep) k_mapsearch<true><<<runs, TPB, lds, 0>>>(V, A);
    else k_mapsearch<false><<<runs, TPB, lds, 0>>>(V, A);
    return hipGetLastError();
}

}  // namespace mapsearch

extern "C" int32_t rc_map_search(rc_ctx *c, int32_t nruns, const int64_t *init, const int32_t *order, const double *r, const double *p,
                                 const rc_params *params, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out_,
                                 int64_t *blocks_out, int64_t *slots_out, int32_t *best, double *kernel_ms)
{
    using namespace mapsearch;
    const char *who = "rc_map_search";
    rc_map_run_t *runs_out = (rc_map_run_t *)runs_out_;
    int32_t rc = clu::check_ctx(c, who);
    if (rc != RC_OK) return rc;
    if (!r || !p) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    const int64_t n = c->n;
    rc = greedy::check_args(c, who, 1, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    // ---- the runs, staged as they are checked, run by run (an earlier run's errors come first): labels in 0..n compacted to
    // slots by first appearance, orders permutations of 1..n.  Nothing is uploaded before the last check has passed.  The
    // sizes are staged for at most KCAP_MAX slots: a start of more clusters is refused below.
    const int64_t Kcap64 = maxK > 0 ? maxK : std::min<int64_t>(n, KCAP_MAX);
    const size_t sz_stride = (size_t)std::min<int64_t>(Kcap64, KCAP_MAX) + 2;
    std::unique_ptr<greedy::Staging> staged;
    std::vector<int> map, start_at;
    std::vector<RunOut> h_out;
    try {
        staged.reset(new greedy::Staging(nruns, n, sz_stride));
        map.assign((size_t)n + 1, 0); start_at.assign((size_t)nruns, -1); h_out.reserve((size_t)nruns);
    } catch (const std::bad_alloc &) { return fail(c, RC_ERR_OOM, "%s: no host memory", who); }
    greedy::Staging &S = *staged;
    for (int q = 0; q < nruns; ++q) {
        int64_t row, at;
        if (find_bad_label(init + (size_t)q * n, 1, n, 0, &row, &at))
            return fail(c, RC_ERR_ARG, "%s: label %lld of run %d outside 0..n", who, (long long)init[(size_t)q * n + at], q + 1);
        rc = S.take_order(c, who, q, order);
        if (rc != RC_OK) return rc;
        std::fill(map.begin(), map.end(), 0);
        int K = 0;
        unsigned short *szr = S.sz_row(q);
        for (int64_t j = 0; j < n; ++j) {
            const int64_t l = init[(size_t)q * n + j];
            if (l && !map[(size_t)l]) map[(size_t)l] = ++K;
            const int slot = map[(size_t)l];                            // map[0] = 0
            S.init_row(q)[j] = (unsigned short)slot;
            if (slot && (size_t)slot + 2 <= sz_stride) szr[slot]++;
        }
        S.K[(size_t)q] = K;
    }
    rc = check_r_p(c, who, "run", nruns, r, p);
    if (rc != RC_OK) return rc;
    if (params) {
        rc = check_params(c, who, params);
        if (rc != RC_OK) return rc;
    } else if (!c->have_params) return fail(c, RC_ERR_STATE, "%s: params is NULL and the context has no parameters set", who);
    const rc_params P = params ? *params : c->P;
    // ---- the capacities
    rc = check_lds_capacity(c, who, n);
    if (rc != RC_OK) return rc;
    rc = check_label_shape(c, who, n, "points", 2 * (int64_t)nruns, "2·nruns");   // the final labellings and the starts are scored in one batch
    if (rc != RC_OK) return rc;
    if (Kcap64 > KCAP_MAX) return fail(c, RC_ERR_CAPACITY, "%s: the slot cap %lld (maxK) exceeds %d", who, (long long)Kcap64, KCAP_MAX);
    const int Kcap = (int)Kcap64;
    for (int q = 0; q < nruns; ++q)
        if (S.K[(size_t)q] > Kcap) return fail(c, RC_ERR_ARG, "%s: run %d starts with %d clusters, more than the slot cap %d", who, q + 1, S.K[(size_t)q], Kcap);

    HIPCHK(c, hipSetDevice(c->dev));
    rc = sync_and_check(c, true);
    if (rc != RC_OK) return rc;
    if (c->sC) HIPCHK(c, hipStreamSynchronize(c->sC));

    const size_t cell_elems = (size_t)Kcap * Kcap * 4;
    const int per_launch = (int)std::max<size_t>(1, std::min<size_t>((size_t)nruns, CELL_BUDGET / (cell_elems * sizeof(long long))));
    DeviceBuffers B;
    double *d_r, *d_p; long long *d_cells;
    HIPCHK(c, B.alloc(d_r, (size_t)nruns));
    HIPCHK(c, B.alloc(d_p, (size_t)nruns));
    HIPCHK(c, B.alloc(d_cells, cell_elems * (size_t)per_launch));
    HIPCHK(c, hipMemcpy(d_r, r, (size_t)nruns * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_p, p, (size_t)nruns * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, S.upload(B, 0, sizeof(RunOut)));

    Args A{};
    A.C = Consts{P.delta1, P.delta2, P.alpha, P.beta, P.zeta, P.gamma, std::lgamma(P.delta1), std::lgamma(P.delta2), std::log(P.beta), std::log(P.gamma),
                 std::ldexp(1.0, -c->eD), std::ldexp(1.0, -c->eL)};
    A.init = S.d_init; A.sz0 = S.d_sz; A.K0 = S.d_K; A.order = S.d_order; A.r = d_r; A.p = d_p; A.labels = S.d_labels; A.out = (RunOut *)S.d_out;
    A.cells = d_cells; A.n = (int)n; A.Kcap = Kcap; A.maxsweeps = maxsweeps; A.implicit_cap = maxK > 0 ? 0 : 1;
    const size_t lds = Carve((int)n, Kcap).total;
    const View V = make_view(c);
    // the events sit around each launch alone: neither the zeroing of the cells nor the copy of blocks_out is in kernel_ms
    TimingEvents ev;
    HIPCHK(c, ev.create());
    double ms_acc = 0.0;
    for (int q0 = 0; q0 < nruns; q0 += per_launch) {
        const int runs = std::min(per_launch, nruns - q0);
        A.run0 = q0;
        HIPCHK(c, hipMemsetAsync(d_cells, 0, cell_elems * (size_t)runs * sizeof(long long), 0));
        HIPCHK(c, ev.begin(0));
        HIPCHK(c, launch(P.repulsion != 0, runs, lds, V, A));
        HIPCHK(c, ev.end(0));
        HIPCHK(c, ev.elapsed_ms(ms_acc));
        if (blocks_out) HIPCHK(c, hipMemcpyAsync(blocks_out + (size_t)q0 * cell_elems, d_cells, cell_elems * (size_t)runs * sizeof(long long), hipMemcpyDeviceToHost, 0));
    }
    HIPCHK(c, S.begin(0));
    HIPCHK(c, S.collect(0, h_out, nullptr));                            // the final slots and the records
    if (kernel_ms) *kernel_ms = ms_acc;

    // ---- results: sortlabels of the final slots; everything reported comes from the exact scoring path, the final labellings
    // and the fully allocated starts in one batch
    std::vector<int64_t> rows;
    std::vector<double> rs, ps, ll, lp;
    try {
        rows.reserve((size_t)2 * nruns * n);
        rows.resize((size_t)nruns * n);
        for (int q = 0; q < nruns; ++q) {
            std::fill(map.begin(), map.end(), 0);
            int next = 0;
            for (int64_t j = 0; j < n; ++j) {
                const unsigned short l = S.labels[(size_t)q * n + j];
                if (!map[l]) map[l] = ++next;
                rows[(size_t)q * n + j] = labels_out[(size_t)q * n + j] = map[l];
                if (slots_out) slots_out[(size_t)q * n + j] = l;
            }
            rs.push_back(r[q]); ps.push_back(p[q]);
        }
        for (int q = 0; q < nruns; ++q) {
            const int64_t *z = init + (size_t)q * n;
            if (std::find(z, z + n, (int64_t)0) != z + n) continue;
            start_at[(size_t)q] = (int)rs.size();
            rows.insert(rows.end(), z, z + n);
            rs.push_back(r[q]); ps.push_back(p[q]);
        }
        ll.resize(rs.size()); lp.resize(rs.size());
    } catch (const std::bad_alloc &) { return fail(c, RC_ERR_OOM, "%s: no host memory", who); }
    rc = scr::score_valid(c, who, (int64_t)rs.size(), rows.data(), rs.data(), ps.data(), P, ll.data(), lp.data(), nullptr, nullptr, 0, nullptr);
    if (rc != RC_OK) return rc;
    int b = 0;
    for (int q = 0; q < nruns; ++q) {
        const RunOut &o = h_out[(size_t)q];
        rc_map_run_t &R = runs_out[q];
        R.loglik = ll[(size_t)q]; R.logprior = lp[(size_t)q]; R.logposterior = ll[(size_t)q] + lp[(size_t)q];
        const int s = start_at[(size_t)q];
        R.start_logposterior = s < 0 ? std::numeric_limits<double>::quiet_NaN() : ll[(size_t)s] + lp[(size_t)s];
        R.sweeps = o.sweeps; R.converged = o.converged; R.K = o.K; R.capped = o.capped; R.moves = o.moves;
        if (R.logposterior > runs_out[b].logposterior) b = q;
    }
    *best = b;
    return RC_OK;
}

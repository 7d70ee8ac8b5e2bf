// MAP search for n up to 32767: k_map_large<BITS, STORED, REP> and k_map_cells<BITS, STORED>, behind rc_map_search_large.
// DESIGN.md §8 "MAP search, large n"; the contract is rc_map_search's (include/redclust_hip.h).  Included at the end of
// redclust_hip.hip behind mapsearch.inc.hip: the criterion, the visit order, the tie rules, the slots, the cell layout, Args,
// Carve, the cell arithmetic, term and the host body are that file's.  What is this file's own is how a row gets into the
// per-slot sums, and where the cells of the starting labels are built.
//
// Internal order.  The run's slots live in LDS indexed by the context's internal index x = V.pi[j] (labx, padded with slot 0 to
// a multiple of 4; filled once, written back through pi at the end), so a visit of point i reads row u = pi[i] contiguously in
// x and gathers nothing.  A thread takes a chunk of 16 bytes per load — four adjacent columns with 32-bit storage, two with
// 64-bit, a second load of Lq where the log is stored — and the chunk's slots from one aligned LDS read.  Rows are 16-byte
// aligned (ld is a multiple of 1024) and ld >= the padded width, so no load needs a bounds branch: a padded column's slot is 0
// and the "unallocated" rule skips it, column u is skipped as j == i was, the previous visit's point is forwarded from
// registers.  Adjacent columns of a chunk with equal slots are added in registers and issue one pair of LDS atomics: the
// internal layout is cluster-contiguous for the context's own state, so labellings near it collapse most chunks, and the sums
// are exact integers, so any grouping gives the same accumulators.
//
// Prefetch.  The first PF chunks per thread of the next visit's row (u' = pi[inext], known a visit ahead from Visit::ahead)
// are loaded behind phase A's barrier, stay in registers across phases B and C and are consumed by the next phase A; the rest
// of a row is loaded four chunks at a time.  PF = 2 where the log is stored (two 16-byte loads per chunk), 4 where it is
// derived: 16 VGPRs either way.
//
// Phases B and C are k_mapsearch's text (a second copy, so that k_mapsearch compiles to the instructions it had): the same
// term, halves_f64, key_f64, group_argmin and offer_new in the same order, so a run is the same function of its inputs.
//
// k_map_cells builds the cells of the starting labels on the whole device, before k_map_large on the same stream: a workgroup
// takes CELL_ROWS internal rows of one run, reduces each with the row pass above into LDS per-slot sums, and adds them to the
// run's cells (a, t) with 64-bit global atomics on the four halves — every row sum as its two halves, as cell_add does, D's
// diagonal entry into (a, a).  Sums of halves are exact in any order, so the cells are the bytes k_mapsearch's serial build gives.

namespace mapsearch {

constexpr int CELL_ROWS = 32;                          // rows of one workgroup of k_map_cells
constexpr int LOAD_AHEAD = 4;                          // chunks a thread has in flight behind the prefetched ones

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32_alias __attribute__((may_alias));
typedef unsigned long long u64_alias __attribute__((may_alias));

template <int BITS> struct RowT;
template <> struct RowT<32> { typedef i32x4 vec; static constexpr int C = 4; };
template <> struct RowT<64> { typedef ll2 vec; static constexpr int C = 2; };

__host__ __device__ inline int pad4(int n) { return (n + 3) / 4 * 4; }
constexpr int prefetch_chunks(bool stored) { return stored ? 2 : 4; }

// C adjacent columns of one row: D and, where it is stored, the log
template <int BITS, bool STORED> struct Chunk { typename RowT<BITS>::vec d, l; };

template <int BITS, bool STORED>
__device__ inline Chunk<BITS, STORED> chunk_load(const View &V, int u, int q)
{
    typedef typename RowT<BITS>::vec vec;
    const size_t e = (size_t)u * (size_t)(V.ld / RowT<BITS>::C) + (size_t)q;
    Chunk<BITS, STORED> c;
    c.d = reinterpret_cast<const vec *>(V.Dq)[e];
    c.l = STORED ? reinterpret_cast<const vec *>(V.Lq)[e] : c.d;
    return c;
}

__device__ inline void slot_add(unsigned slot, long long d, long long l, u64 *accS, u64 *accL)
{
    if (!slot) return;
    atomicAdd(&accS[slot], (u64)d);
    atomicAdd(&accL[slot], (u64)l);
}

// chunk q of row u into the per-slot accumulators: runs of equal slots are summed in registers first
template <int BITS, bool STORED>
__device__ inline void chunk_add(const View &V, const Chunk<BITS, STORED> &c, int u, int q, const unsigned short *labx, int xprev, unsigned wprev,
                                 u64 *accS, u64 *accL)
{
    constexpr int C = RowT<BITS>::C;
    const int x0 = q * C;
    unsigned s[C];
    if constexpr (C == 4) {
        const unsigned long long w = *reinterpret_cast<const u64_alias *>(labx + x0);
        s[0] = (unsigned)w & 0xFFFFu; s[1] = ((unsigned)w >> 16) & 0xFFFFu; s[2] = (unsigned)(w >> 32) & 0xFFFFu; s[3] = (unsigned)(w >> 48);
    } else {
        const unsigned w = *reinterpret_cast<const u32_alias *>(labx + x0);
        s[0] = w & 0xFFFFu; s[1] = w >> 16;
    }
    unsigned cur = 0;
    long long d = 0, l = 0;
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const int x = x0 + k;
        unsigned slot = (x == xprev) ? wprev : s[k];
        if (x == u) slot = 0;
        if (slot != cur) {
            slot_add(cur, d, l, accS, accL);
            cur = slot; d = 0; l = 0;
        }
        if (slot) {
            const long long dk = (long long)c.d[k];
            d += dk;
            l += STORED ? (long long)c.l[k] : rc_qlog(dk, V.qeD, V.qsL, V.ltab);
        }
    }
    slot_add(cur, d, l, accS, accL);
}

// the chunks first, first + TPB, … below nq of row u, LOAD_AHEAD loads in flight
template <int BITS, bool STORED>
__device__ inline void row_rest(const View &V, int u, int first, int nq, const unsigned short *labx, int xprev, unsigned wprev, u64 *accS, u64 *accL)
{
    for (int q = first; q < nq; q += LOAD_AHEAD * TPB) {
        Chunk<BITS, STORED> c[LOAD_AHEAD];
#pragma unroll
        for (int f = 0; f < LOAD_AHEAD; ++f)
            if (q + f * TPB < nq) c[f] = chunk_load<BITS, STORED>(V, u, q + f * TPB);
#pragma unroll
        for (int f = 0; f < LOAD_AHEAD; ++f)
            if (q + f * TPB < nq) chunk_add<BITS, STORED>(V, c[f], u, q + f * TPB, labx, xprev, wprev, accS, accL);
    }
}

// labx[pi[j]] = the run's starting slot of j, the padding slot 0
__device__ inline void fill_labx(const View &V, const unsigned short *init, int n, unsigned short *labx, int tid)
{
    for (int j = tid; j < n; j += TPB) labx[V.pi[j]] = init[j];
    for (int x = n + tid; x < pad4(n); x += TPB) labx[x] = 0;
}

__device__ inline long long diag_load(const View &V, int u)
{
    const size_t e = (size_t)u * V.ld + u;
    return (V.bits == 64) ? ((const long long *)V.Dq)[e] : (long long)((const int *)V.Dq)[e];
}

// The cells of the starting labels.  Grid: (blocks of CELL_ROWS internal rows) × (the runs of the launch that start with
// clusters: runlist holds their numbers).  LDS: the (s, l) accumulators u64[2][Kcap + 1], then labx.
template <int BITS, bool STORED>
__global__ __launch_bounds__(TPB) void k_map_cells(View V, Args A, const int *runlist)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char map_lds[];
    const int tid = threadIdx.x;
    const int n = A.n, Kcap = A.Kcap, run = runlist[blockIdx.y];
    const int astride = Kcap + 1, nq = pad4(n) / RowT<BITS>::C;
    u64 *accS = reinterpret_cast<u64 *>(map_lds), *accL = accS + astride;
    unsigned short *labx = reinterpret_cast<unsigned short *>(map_lds + up16(2 * 8 * (size_t)astride));
    long long *cells = A.cells + (size_t)(run - A.run0) * Kcap * Kcap * 4;
    const unsigned hi = (unsigned)A.K0[run];

    for (int k = tid; k < 2 * astride; k += TPB) accS[k] = 0;
    fill_labx(V, A.init + (size_t)run * n, n, labx, tid);
    __syncthreads();

    const int xend = min(n, ((int)blockIdx.x + 1) * CELL_ROWS);
    for (int x = (int)blockIdx.x * CELL_ROWS; x < xend; ++x) {
        const unsigned a = labx[x];
        if (!a) continue;
        row_rest<BITS, STORED>(V, x, tid, nq, labx, -1, 0u, accS, accL);
        __syncthreads();
        for (unsigned t = (unsigned)tid + 1u; t <= hi; t += TPB) {
            const long long d = (long long)accS[t], l = (long long)accL[t];
            accS[t] = 0; accL[t] = 0;
            Cell c{0, 0, 0, 0};
            cell_add(c, d, l, 1);
            if (t == a) cell_add(c, diag_load(V, x), 0, 1);
            u64 *q = reinterpret_cast<u64 *>(cells + ((size_t)(a - 1u) * Kcap + (t - 1u)) * 4);
            if (c.dh) atomicAdd(q + 0, (u64)c.dh);
            if (c.dl) atomicAdd(q + 1, (u64)c.dl);
            if (c.lh) atomicAdd(q + 2, (u64)c.lh);
            if (c.ll) atomicAdd(q + 3, (u64)c.ll);
        }
        __syncthreads();
    }
}

template <int BITS, bool STORED, bool REP>
__global__ __launch_bounds__(TPB) void k_map_large(View V, Args A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char map_lds[];
    constexpr int PF = prefetch_chunks(STORED);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, Kcap = A.Kcap, run = A.run0 + blockIdx.x;
    const int nq = pad4(n) / RowT<BITS>::C;
    const Consts C = A.C;

    const Carve cv(pad4(n), Kcap);
    u64 *acc = reinterpret_cast<u64 *>(map_lds + cv.acc);                 // [generation][S, L][Kcap + 1]
    unsigned long long *r_sc = reinterpret_cast<unsigned long long *>(map_lds + cv.red);
    double *r_new = reinterpret_cast<double *>(r_sc + NWAVE);
    unsigned *r_pr = reinterpret_cast<unsigned *>(r_new + 1), *r_slot = r_pr + NWAVE, *r_free = r_slot + NWAVE;
    unsigned short *sz = reinterpret_cast<unsigned short *>(map_lds + cv.sz);
    unsigned short *labx = reinterpret_cast<unsigned short *>(map_lds + cv.lab);
    long long *cells = A.cells + (size_t)blockIdx.x * Kcap * Kcap * 4;
    const auto cell = [&](unsigned k, unsigned t) { return cells + ((size_t)(k - 1u) * Kcap + (t - 1u)) * 4; };
    const int astride = Kcap + 1;

    for (int k = tid; k < 4 * astride; k += TPB) acc[k] = 0;
    if (tid >= WAVES && tid < NWAVE) { r_sc[tid] = ~0ull; r_pr[tid] = ~0u; r_slot[tid] = 0u; r_free[tid] = ~0u; }
    for (int k = tid; k < Kcap + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (Kcap + 2) + k];
    fill_labx(V, A.init + (size_t)run * n, n, labx, tid);
    __syncthreads();
    int K = A.K0[run];
    unsigned hi = (unsigned)K;                                            // the highest slot ever occupied
    const double rr = A.r[run], logp = log(A.p[run]), rlog1mp = rr * log1p_lean(-A.p[run]);
    const TermC TW{C.d1, C.al, C.lgd1, C.lb, C.be, 0.5 * C.scD, 0.5 * C.scL};
    const TermC TB{C.d2, C.ze, C.lgd2, C.lg, C.ga, C.scD, C.scL};

    const greedy::Partials red{r_sc, r_pr, r_slot, r_free, nullptr};
    greedy::Visit v(A.order + (size_t)run * n, n);
    long long moves = 0;
    int sweeps = 0, converged = 0, capped = 0, gen = 0;
    int u = V.pi[v.i], uprev = -1;                                        // the visit's and the previous visit's internal index

    // the leading chunks of the first visit's row
    Chunk<BITS, STORED> pre[PF];
#pragma unroll
    for (int f = 0; f < PF; ++f) {
        pre[f] = Chunk<BITS, STORED>{};
        if (tid + f * TPB < nq) pre[f] = chunk_load<BITS, STORED>(V, u, tid + f * TPB);
    }

    for (;;) {
        int moved = 0;
        for (int t_ = 0; t_ < n; ++t_) {
            const int inext = v.ahead(t_);
            const int unext = V.pi[inext];
            const unsigned a = (u == uprev) ? v.wprev : (unsigned)labx[u];
            u64 *accS = acc + (size_t)gen * 2 * astride, *accL = accS + astride;
            u64 *other = acc + (size_t)(gen ^ 1) * 2 * astride;
            const long long dii = diag_load(V, u);

            // phase A: the row sums, the prefetched chunks first
#pragma unroll
            for (int f = 0; f < PF; ++f)
                if (tid + f * TPB < nq) chunk_add<BITS, STORED>(V, pre[f], u, tid + f * TPB, labx, uprev, v.wprev, accS, accL);
            row_rest<BITS, STORED>(V, u, tid + PF * TPB, nq, labx, uprev, v.wprev, accS, accL);
            __syncthreads();

            // the leading chunks of the next visit's row: in flight during phases B and C
#pragma unroll
            for (int f = 0; f < PF; ++f)
                if (tid + f * TPB < nq) pre[f] = chunk_load<BITS, STORED>(V, unext, tid + f * TPB);

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
                labx[u] = (unsigned short)w;
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
            }
            moved += v.moved_to(a, w, inext);
            uprev = u; u = unext;
            K = Know + (int)isnew;
            gen ^= 1;
        }
        ++sweeps;
        moves += moved;
        if (!moved) { converged = 1; break; }
        if (sweeps >= A.maxsweeps) break;
    }
    __syncthreads();

    for (int j = tid; j < n; j += TPB) A.labels[(size_t)run * n + j] = labx[V.pi[j]];
    if (tid == 0) {
        RunOut o{};
        o.moves = moves; o.sweeps = sweeps; o.converged = converged; o.K = K; o.capped = capped;
        A.out[run] = o;
    }
}

static size_t lds_large(int n, int Kcap) { return Carve(pad4(n), Kcap).total; }

template <int BITS, bool STORED>
static hipError_t launch_large_as(bool rep, int runs, const View &V, const Args &A, const int *runlist, int ncells)
{
    const size_t lds = lds_large(A.n, A.Kcap), lds_cells = up16(2 * 8 * (size_t)(A.Kcap + 1)) + up16(2 * (size_t)pad4(A.n));
    hipError_t e = set_dynamic_lds(k_map_cells<BITS, STORED>, lds_cells);
    if (e == hipSuccess) e = rep ? set_dynamic_lds(k_map_large<BITS, STORED, true>, lds) : set_dynamic_lds(k_map_large<BITS, STORED, false>, lds);
    if (e != hipSuccess) return e;
    if (ncells) k_map_cells<BITS, STORED><<<dim3((unsigned)((A.n + CELL_ROWS - 1) / CELL_ROWS), (unsigned)ncells), TPB, lds_cells, 0>>>(V, A, runlist);
    if (rep) k_map_large<BITS, STORED, true><<<runs, TPB, lds, 0>>>(V, A);
    else k_map_large<BITS, STORED, false><<<runs, TPB, lds, 0>>>(V, A);
    return hipGetLastError();
}

// the cells of the ncells runs of the launch that start with clusters (runlist: their numbers, on the device), then the sweeps
static hipError_t launch_large(bool rep, int runs, const View &V, const Args &A, const int *runlist, int ncells)
{
    const bool stored = V.Lq != nullptr;
    if (V.bits == 32) return stored ? launch_large_as<32, true>(rep, runs, V, A, runlist, ncells) : hipErrorInvalidValue;   // a derived log is 64-bit
    return stored ? launch_large_as<64, true>(rep, runs, V, A, runlist, ncells) : launch_large_as<64, false>(rep, runs, V, A, runlist, ncells);
}

}  // namespace mapsearch

extern "C" int32_t rc_map_search_large(rc_ctx *c, int32_t nruns, const int64_t *init, const int32_t *order, const double *r, const double *p,
                                       const rc_params *params, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                       int64_t *blocks_out, int64_t *slots_out, int32_t *best, double *kernel_ms)
{
    return mapsearch::search("rc_map_search_large", true, c, nruns, init, order, r, p, params, maxK, maxsweeps, labels_out, runs_out, blocks_out,
                             slots_out, best, kernel_ms);
}

// Point-estimate search for n beyond the 8192 points whose whole state fits one workgroup's LDS: rc_psm_search_large*, the
// Binder and VI-bound searches of pointsearch.inc.hip for n <= 32767 (DESIGN.md §8 "Point-estimate search, large n").
// Included at the end of redclust_hip.hip behind pointsearch.inc.hip (same translation unit: psm::'s arguments, record, staging
// and losses; greedy::'s walk, keys, argmin and new-cluster candidate; cnt:: for the three input forms).
//
// Criterion, run semantics, ties and arithmetic are k_search's, unchanged: a Binder run is the same exact integer function of its
// arguments, a VI run rounds every log term once to 2^-40 and adds integers, so for n <= 8192 both kernels give the same bits.
// What n forces to differ:
//
//   LDS      lab u16[n4] (n4 = n rounded up to 4, pad slots 0) and sz u16[n+2] stay; what is left of psm::LDS_BUDGET is the
//            accumulator window, S u32[W] (+ L u64[W] for VI): W ≈ 7.9k slots for Binder and ≈ 2.6k for VI at n = 32767.  The
//            occupied slot range 1..hi is always covered in passes of W slots (from empty labels hi = K: one pass).
//   T        VI's T u32 moves to global memory, n4 words per run.  OWNERSHIP: T[j] is read and written only by the thread that
//            owns column j, thread (j / 4) mod 1024 — phase A's "take i out", phase C's "put i in", and T[i] itself, which the
//            owner of column i sets in phase C.  So the loop needs no fence beyond its barriers.  Other threads touch T twice,
//            each time behind a barrier: one wave per allocated row computes the start's T, and the epilogue reads it.
//   rows     a thread owns the four adjacent columns 4·(tid + q·1024) … +3, q < Q4 = ⌈n/4096⌉ ∈ {1, 2, 4, 8}: a row of C is read
//            with 16-byte loads (ld is a multiple of 4, rows are 16-byte aligned), lab with one 8-byte LDS read per quad, T with
//            one 16-byte global read per quad.  Columns >= n are masked (a context's pad columns are not guaranteed zero).
//            Entries of a quad that share a label are combined in registers, so equal neighbours cost one LDS atomic.
//   prefetch the first PF quads of row order[t+1] are issued before step t's barriers and kept in registers; the other Q4 − PF
//            quads of a row are streamed from memory where its own step uses them.  Two whole rows are 64 VGPRs at Q4 = 8, and
//            a lane of a 1024-thread workgroup may own 128: PF is the largest part with which an instantiation compiles
//            without scratch — Binder 1, 2, 4, 2 and VI 1, 2, 1, 1 quads at Q4 = 1, 2, 4, 8 (VI's f64 log1p needs the rest).

namespace psm_large {

using greedy::TPB, greedy::NWAVE, greedy::Cand, greedy::better, greedy::key_i64, greedy::key_f64;
using psm::QUANT, psm::LDS_BUDGET, psm::RunOut;
constexpr int NMAX = 32767;

struct Args {
    psm::Args a;                  // W: the accumulator window
    unsigned *T;                  // VI: nruns × n4 workspace
    int n4;
};

// quad q of a row: columns 4·(tid + q·TPB) … +3, those at or beyond n as 0
__device__ inline uint4 load_quad(const unsigned *__restrict__ row, int n, int tid, int q)
{
    const int j0 = 4 * (tid + q * TPB);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (j0 < n) {
        v = *reinterpret_cast<const uint4 *>(row + j0);
        if (j0 + 1 >= n) v.y = 0u;
        if (j0 + 2 >= n) v.z = 0u;
        if (j0 + 3 >= n) v.w = 0u;
    }
    return v;
}

template <int LOSS, int Q4, int PF>
__global__ __launch_bounds__(TPB) void k_search_large(Args AA)
{
    constexpr bool VI = LOSS == RC_PSM_VILB;
    static_assert(PF >= 1 && PF <= Q4, "the prefetched part is a leading part of the row");
    constexpr int UNROLL_E = VI ? 1 : 4, UNROLL_Q = VI ? 1 : (Q4 > PF ? Q4 - PF : 1);   // phase A's loops, see there
    extern __shared__ unsigned long long psml_lds[];
    __shared__ unsigned long long r_sc[NWAVE];
    __shared__ unsigned r_pr[NWAVE], r_slot[NWAVE], r_S[NWAVE], r_free[NWAVE];
    __shared__ double r_f[NWAVE];
    __shared__ unsigned long long r_a[NWAVE], r_b[NWAVE];

    const psm::Args &A = AA.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, n4 = AA.n4, W = A.W, run = blockIdx.x;
    const unsigned m = A.m;
    const unsigned *__restrict__ C = A.C;
    const size_t ld = (size_t)A.ld;

    // carve the dynamic LDS so that lab sits on an 8-byte boundary whatever W is: L u64[W] | lab u16[n4] | S u32[W] | sz u16[n+2]
    unsigned long long *L = psml_lds;
    unsigned short *lab = reinterpret_cast<unsigned short *>(L + (VI ? (size_t)W : 0));
    unsigned *S = reinterpret_cast<unsigned *>(lab + n4);
    unsigned short *sz = reinterpret_cast<unsigned short *>(S + W);
    unsigned *T = VI ? AA.T + (size_t)run * n4 : nullptr;
    uint4 *T4 = reinterpret_cast<uint4 *>(T);

    for (int k = tid; k < W; k += TPB) { S[k] = 0; if (VI) L[k] = 0; }
    for (int k = tid; k < n + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (n + 2) + k];
    for (int j = tid; j < n4; j += TPB) lab[j] = (j < n) ? A.init[(size_t)run * n + j] : (unsigned short)0;
    if (VI)
        for (int g = tid; g < n4 / 4; g += TPB) T4[g] = make_uint4(0u, 0u, 0u, 0u);
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

    const greedy::Partials red{r_sc, r_pr, r_slot, r_free, r_S};
    greedy::Visit v(A.order + (size_t)run * n, n);
    int K = A.K0[run], hi = A.hi0[run];
    uint4 cur[PF], nxt[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) nxt[q] = load_quad(C + (size_t)v.i * ld, n, tid, q);
    long long moves = 0;
    int sweeps = 0, converged = 0;
    const double dnew = VI ? -2.0 * log((double)m) : 0.0;
    const unsigned long long key_new = VI ? key_f64(dnew) : key_i64(0);

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            // this row's leading part was prefetched; the next row's is issued now, to be consumed in the next step.  The rest
            // of this row is streamed where it is used
            const int i = v.i, inext = v.ahead(t);
            const unsigned *__restrict__ rowi = C + (size_t)i * ld;
#pragma unroll
            for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
#pragma unroll
            for (int q = 0; q < PF; ++q) nxt[q] = load_quad(C + (size_t)inext * ld, n, tid, q);

            const unsigned a = v.slot_of(lab);
            const int scan_hi = min(hi + 1, n);                          // slots above hi are free; hi + 1 is the lowest of them
            Cand best{~0ull, ~0u, 0u, 0u};
            unsigned minfree = ~0u;
            unsigned emptied = 0;
            for (int base = 0, pass = 0; base < scan_hi; base += W, ++pass) {
                // phase A: row i into the per-slot accumulators of this window; the first pass also takes i out of T
                if (pass) __syncthreads();
                // One quad.  Its four entries rotate through the .x lanes, so the loop over them needs no indexed registers:
                // VI keeps it rolled — one copy of the f64 log1p, or the kernel does not fit its 128 VGPRs — Binder unrolls it.
                // Runs of equal labels within the quad are summed in registers: one atomic per run
                const auto quad = [&](int q, uint4 cq) {
                    const int j0 = 4 * (tid + q * TPB);
                    if (j0 >= n) return;
                    const uint2 lw = *reinterpret_cast<const uint2 *>(lab + j0);
                    unsigned long long ls = ((unsigned long long)lw.y << 32) | lw.x;   // pad slots hold 0
                    uint4 tq = VI ? T4[j0 >> 2] : make_uint4(1u, 1u, 1u, 1u);
                    bool changed = false;
                    unsigned pidx = ~0u, ps = 0;
                    unsigned long long pl = 0;
#pragma unroll UNROLL_E
                    for (int e = 0; e < 4; ++e) {
                        const unsigned l = (j0 + e == i) ? 0u : (unsigned)(ls & 0xFFFFu);   // i itself is out
                        const unsigned c = cq.x;
                        unsigned Tj = tq.x;
                        if (VI && pass == 0 && l && l == a && c) { Tj -= c; tq.x = Tj; changed = true; }
                        const unsigned idx = l - 1u - (unsigned)base;   // l = 0 wraps beyond every W
                        if (idx < (unsigned)W && c) {
                            if (idx != pidx) {
                                if (ps) { atomicAdd(&S[pidx], ps); if (VI) atomicAdd(&L[pidx], pl); }
                                pidx = idx; ps = 0; pl = 0;
                            }
                            ps += c;
                            if (VI) pl += __double2ull_rn(log1p((double)c / (double)Tj) * QUANT);
                        }
                        ls >>= 16;
                        cq = make_uint4(cq.y, cq.z, cq.w, cq.x);
                        if (VI) tq = make_uint4(tq.y, tq.z, tq.w, tq.x);
                    }
                    if (ps) { atomicAdd(&S[pidx], ps); if (VI) atomicAdd(&L[pidx], pl); }
                    if (VI && changed) T4[j0 >> 2] = tq;                 // four rotations: back in place
                };
#pragma unroll
                for (int q = 0; q < PF; ++q) quad(q, cur[q]);
#pragma unroll UNROLL_Q
                for (int q = PF; q < Q4; ++q) quad(q, load_quad(rowi, n, tid, q));
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
                    const unsigned pr = ((unsigned)k == a) ? 0u : (unsigned)k;
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
            greedy::group_argmin<VI>(best, minfree, red, lane, wave);
            const int Know = K - (int)emptied;
            unsigned isnew = 0;
            if (A.maxK == 0 || Know < A.maxK) isnew = greedy::offer_new(best, key_new, emptied, a, minfree);
            const unsigned w = best.slot;
            // phase C: put i into w.  Per-point entries — lab, T, and T[i] with them — are written by the thread that owns the
            // column, sz by the owner of i; the next step reads sz only behind its first barrier
            if (VI) {
                const auto put = [&](int q, uint4 cq) {
                    const int j0 = 4 * (tid + q * TPB);
                    if (j0 >= n) return;
                    const uint2 lw = *reinterpret_cast<const uint2 *>(lab + j0);
                    const unsigned l[4] = {lw.x & 0xFFFFu, lw.x >> 16, lw.y & 0xFFFFu, lw.y >> 16};
                    const unsigned c[4] = {cq.x, cq.y, cq.z, cq.w};
                    bool hit = (unsigned)(i - j0) < 4u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) hit |= (l[e] == w && c[e]);
                    if (!hit) return;
                    const uint4 tq = T4[j0 >> 2];
                    unsigned Tj[4] = {tq.x, tq.y, tq.z, tq.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (j0 + e == i) Tj[e] = best.S + m;
                        else if (l[e] == w) Tj[e] += c[e];               // (pad columns: c = 0)
                    }
                    T4[j0 >> 2] = make_uint4(Tj[0], Tj[1], Tj[2], Tj[3]);
                };
#pragma unroll
                for (int q = 0; q < PF; ++q) put(q, cur[q]);
#pragma unroll 1
                for (int q = PF; q < Q4; ++q) put(q, load_quad(rowi, n, tid, q));
            }
            if (tid == ((i >> 2) & (TPB - 1))) {
                lab[i] = (unsigned short)w;
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
            }
            moved += v.moved_to(a, w, inext);
            K = Know + (int)isnew;
            hi = max(hi, (int)w);
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
        // f in k_search's order: per thread ascending j = tid + q·1024, xor tree over the wave, waves in ascending order
        for (int j = tid; j < n; j += TPB) {
            const unsigned l = lab[j];
            if (l) f += log((double)sz[l]) - 2.0 * log((double)T[j]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) f += __shfl_xor(f, off);
        if (lane == 0) r_f[wave] = f;
    } else {
        psm::upper_sums<false>(C, ld, n, lab, lane, wave, tot, same);
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
static hipError_t launch(int Q4, int nruns, size_t lds, hipStream_t st, const Args &A)
{
    constexpr bool VI = LOSS == RC_PSM_VILB;
#define PSML_LAUNCH(QQ, PP)                                                                                               \
    do {                                                                                                                  \
        hipError_t e = hipFuncSetAttribute((const void *)k_search_large<LOSS, QQ, PP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                                    \
        k_search_large<LOSS, QQ, PP><<<nruns, TPB, lds, st>>>(A);                                                         \
    } while (0)
    if (Q4 <= 1) PSML_LAUNCH(1, 1);
    else if (Q4 <= 2) PSML_LAUNCH(2, 2);
    else if (Q4 <= 4) PSML_LAUNCH(4, (VI ? 1 : 4));
    else PSML_LAUNCH(8, (VI ? 1 : 2));
#undef PSML_LAUNCH
    return hipGetLastError();
}

// ---- PEAR (rc_pear_search_large*; DESIGN.md §8 "PEAR search, large n"): k_search<LOSS_PEAR>'s criterion in this file's layout, as
// a kernel of its own.  Rows, the quad loop with its runs of equal labels, the window passes and the prefetch are Binder's above.
// PEAR's own parts:
//   head     X, A, P as u64 words and the two S_ia accumulators in front of lab: head u64[4] | lab u16[n4] | S u32[W] | sz u16[n+2].
//   S_ia     the row's sum over the point's own cluster, which turns the run's X into X₀, is summed in pass 0 only (slot a may lie
//            outside the window of any one pass): per thread in a register, over the wave by shuffles, one LDS atomic per wave into
//            the accumulator of the step's parity — the owner of i clears it in phase C while the other threads are already
//            adding to the other one.
//   score    slot k stands for the state (X₀ + S_ik, A₀ + n_k), a greedy::WCand; num and den (up to 75 bits each) are rebuilt from
//            it where two candidates are compared, exactly, in widefrac.inc.hpp — m·T² need not fit anything.  The best candidate
//            stays in registers across the window passes; X₀, A₀, P and the group's winner are wave-uniform and sit in scalar
//            registers, so the merge of the waves' partials and the new-cluster comparison cost no vector work.
//   P, X     one upper_sums pass before the first step (P and the start's X), one after the last (the reported X and P).
// PF is the largest leading part with which an instantiation compiles without scratch and within 128 VGPRs: 1, 2, 4, 3 quads at
// Q4 = 1, 2, 4, 8 (85, 97, 124, 123 VGPRs).  UNROLL_Q: how many of the streamed quads are loaded at a time — all of them, but two
// at Q4 = 8, where the uniform state's scalar registers (100 are in use) already overflow into vector ones.
template <int Q4, int PF, int UNROLL_Q = (Q4 > PF ? Q4 - PF : 1)>
__global__ __launch_bounds__(TPB) void k_pear_large(Args AA)
{
    static_assert(PF >= 1 && PF <= Q4, "the prefetched part is a leading part of the row");
    extern __shared__ unsigned long long pearl_lds[];
    __shared__ unsigned long long r_X[NWAVE], r_a[NWAVE], r_b[NWAVE];
    __shared__ unsigned r_A[NWAVE], r_pr[NWAVE], r_slot[NWAVE], r_free[NWAVE];

    const psm::Args &A = AA.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.n, n4 = AA.n4, W = A.W, run = blockIdx.x;
    const unsigned *__restrict__ C = A.C;
    const size_t ld = (size_t)A.ld;

    unsigned long long *XA = pearl_lds;                                  // X, A, P
    unsigned *Sa = reinterpret_cast<unsigned *>(XA + 3);                 // S_ia of the even and the odd steps
    unsigned short *lab = reinterpret_cast<unsigned short *>(XA + psm::PEAR_HEAD);
    unsigned *S = reinterpret_cast<unsigned *>(lab + n4);
    unsigned short *sz = reinterpret_cast<unsigned short *>(S + W);

    for (int k = tid; k < W; k += TPB) S[k] = 0;
    for (int k = tid; k < n + 2; k += TPB) sz[k] = A.sz0[(size_t)run * (n + 2) + k];
    for (int j = tid; j < n4; j += TPB) lab[j] = (j < n) ? A.init[(size_t)run * n + j] : (unsigned short)0;
    __syncthreads();
    {
        // P, and X and A of the starting labels
        unsigned long long tot = 0, same = 0, within = 0;
        psm::upper_sums<true>(C, ld, n, lab, lane, wave, tot, same);
        for (int k = 1 + tid; k <= n; k += TPB) within += (unsigned long long)sz[k] * (sz[k] - 1u) / 2u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) within += greedy::shfl_xor_u64(within, off);
        if (lane == 0) { r_a[wave] = tot; r_b[wave] = same; r_X[wave] = within; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long ta = 0, tb = 0, tc = 0;
            for (int w = 0; w < NWAVE; ++w) { ta += r_a[w]; tb += r_b[w]; tc += r_X[w]; }
            XA[0] = tb; XA[1] = tc; XA[2] = ta;
            Sa[0] = Sa[1] = 0;
        }
        __syncthreads();
    }
    const widefrac::Step step = widefrac::make_step((long long)n * (n - 1) / 2, (long long)A.m, (long long)greedy::uniform(XA[2]));

    const greedy::WPartials red{r_X, r_A, r_pr, r_slot, r_free};
    greedy::Visit v(A.order + (size_t)run * n, n);
    int K = A.K0[run], hi = A.hi0[run];
    int par = 0;
    uint4 cur[PF], nxt[PF];
#pragma unroll
    for (int q = 0; q < PF; ++q) nxt[q] = load_quad(C + (size_t)v.i * ld, n, tid, q);
    long long moves = 0;
    int sweeps = 0, converged = 0;

    for (;;) {
        int moved = 0;
        for (int t = 0; t < n; ++t) {
            const int i = v.i, inext = v.ahead(t);
            const unsigned *__restrict__ rowi = C + (size_t)i * ld;
#pragma unroll
            for (int q = 0; q < PF; ++q) cur[q] = nxt[q];
#pragma unroll
            for (int q = 0; q < PF; ++q) nxt[q] = load_quad(C + (size_t)inext * ld, n, tid, q);

            const unsigned a = greedy::uniform(v.slot_of(lab));
            const int scan_hi = min(hi + 1, n);
            greedy::WCand best = greedy::WCAND_NONE;
            unsigned long long X0 = 0;                                   // X and A with i out
            unsigned A0 = 0;
            unsigned minfree = ~0u;
            unsigned emptied = 0;
            for (int base = 0, pass = 0; base < scan_hi; base += W, ++pass) {
                // phase A: row i into the per-slot accumulators of this window; the first pass also sums it over i's own cluster
                if (pass) __syncthreads();
                unsigned sa = 0;
                const auto quad = [&](int q, uint4 cq) {
                    const int j0 = 4 * (tid + q * TPB);
                    if (j0 >= n) return;
                    const uint2 lw = *reinterpret_cast<const uint2 *>(lab + j0);
                    unsigned long long ls = ((unsigned long long)lw.y << 32) | lw.x;   // pad slots hold 0
                    unsigned pidx = ~0u, ps = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned l = (j0 + e == i) ? 0u : (unsigned)(ls & 0xFFFFu);   // i itself is out
                        const unsigned c = cq.x;
                        if (pass == 0 && a && l == a) sa += c;
                        const unsigned idx = l - 1u - (unsigned)base;   // l = 0 wraps beyond every W
                        if (idx < (unsigned)W && c) {
                            if (idx != pidx) {
                                if (ps) atomicAdd(&S[pidx], ps);
                                pidx = idx; ps = 0;
                            }
                            ps += c;
                        }
                        ls >>= 16;
                        cq = make_uint4(cq.y, cq.z, cq.w, cq.x);
                    }
                    if (ps) atomicAdd(&S[pidx], ps);
                };
#pragma unroll
                for (int q = 0; q < PF; ++q) quad(q, cur[q]);
#pragma unroll UNROLL_Q
                for (int q = PF; q < Q4; ++q) quad(q, load_quad(rowi, n, tid, q));
                if (pass == 0 && a) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) sa += (unsigned)__shfl_xor((int)sa, off);
                    if (lane == 0 && sa) atomicAdd(&Sa[par], sa);
                }
                __syncthreads();
                // phase B: score the slots of this window (and clear their accumulators)
                emptied = (a && sz[a] == 1) ? 1u : 0u;
                if (pass == 0) {
                    X0 = greedy::uniform(XA[0]) - greedy::uniform(Sa[par]);
                    A0 = greedy::uniform((unsigned)XA[1]) - (a ? greedy::uniform((unsigned)sz[a]) - 1u : 0u);
                }
                const int kend = min(base + W, scan_hi);
                for (int k = base + 1 + tid; k <= kend; k += TPB) {
                    const int nk = (int)sz[k] - ((unsigned)k == a ? 1 : 0);
                    if (nk <= 0) { minfree = min(minfree, (unsigned)k); continue; }
                    const int idx = k - 1 - base;
                    const unsigned s = S[idx];
                    S[idx] = 0;
                    const greedy::WCand cand{X0 + s, A0 + (unsigned)nk, ((unsigned)k == a) ? 0u : (unsigned)k, (unsigned)k};
                    if (greedy::fbetter(step, cand, best)) best = cand;
                }
            }
            // argmax across the group (the second barrier), then the new cluster: the state without the point
            greedy::group_argmax(step, best, minfree, red, lane, wave);
            const int Know = K - (int)emptied;
            unsigned isnew = 0;
            if (A.maxK == 0 || Know < A.maxK) isnew = greedy::offer_new(step, best, X0, A0, emptied, a, minfree);
            const unsigned w = best.slot;
            // phase C: put i into w — lab by the thread that owns the column, and sz, X, A and the used S_ia accumulator with it; the
            // next step reads them only behind its first barrier
            if (tid == ((i >> 2) & (TPB - 1))) {
                lab[i] = (unsigned short)w;
                if (a) sz[a] = (unsigned short)(sz[a] - 1);
                sz[w] = (unsigned short)(sz[w] + 1);
                XA[0] = best.X; XA[1] = best.A; Sa[par] = 0;
            }
            moved += v.moved_to(a, w, inext);
            K = Know + (int)isnew;
            hi = max(hi, (int)w);
            par ^= 1;
        }
        ++sweeps;
        moves += moved;
        if (!moved) { converged = 1; break; }
        if (sweeps >= A.maxsweeps) break;
    }
    __syncthreads();

    for (int j = tid; j < n; j += TPB) A.labels[(size_t)run * n + j] = lab[j];
    unsigned long long tot = 0, same = 0;
    psm::upper_sums<false>(C, ld, n, lab, lane, wave, tot, same);
    if (lane == 0) { r_a[wave] = tot; r_b[wave] = same; }
    __syncthreads();
    if (tid == 0) {
        RunOut o{};
        unsigned long long ta = 0, tb = 0;
        for (int w = 0; w < NWAVE; ++w) { ta += r_a[w]; tb += r_b[w]; }
        o.tot = (long long)ta; o.same = (long long)tb;
        o.moves = moves; o.sweeps = sweeps; o.converged = converged; o.K = K;
        A.out[run] = o;
    }
}

static hipError_t launch_pear(int Q4, int nruns, size_t lds, hipStream_t st, const Args &A)
{
#define PEARL_LAUNCH(...)                                                                                                 \
    do {                                                                                                                  \
        hipError_t e = hipFuncSetAttribute((const void *)k_pear_large<__VA_ARGS__>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        if (e != hipSuccess) return e;                                                                                    \
        k_pear_large<__VA_ARGS__><<<nruns, TPB, lds, st>>>(A);                                                            \
    } while (0)
    if (Q4 <= 1) PEARL_LAUNCH(1, 1);
    else if (Q4 <= 2) PEARL_LAUNCH(2, 2);
    else if (Q4 <= 4) PEARL_LAUNCH(4, 4);
    else PEARL_LAUNCH(8, 3, 2);                                          // (8, 4) spills however few of the other quads are in flight
#undef PEARL_LAUNCH
    return hipGetLastError();
}

// A run's fraction for greedy::results; a < b: a is the larger fraction
struct WideKey {
    widefrac::Frac f;
    bool operator<(const WideKey &o) const { return widefrac::compare(f, o.f) > 0; }
};

// psm::run for the large kernel: the same staging, counts check and results around another geometry and launch
static int32_t run(rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ld, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                   const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                   void *runs_out, int32_t *best, double *kernel_ms)
{
    greedy::Staging S(nruns, n, (size_t)n + 2);
    std::vector<int> h_hi((size_t)nruns);
    const int32_t src = psm::stage_runs(c, S, h_hi, n, nruns, init, order, maxK);
    if (src != RC_OK) return src;
    const int32_t crc = check_counts(c, st, "point search", dC, ld, m, n);
    if (crc != RC_OK) return crc;
    DeviceBuffers B;

    // ---- geometry: lab and sz fixed, the rest of the budget is the window
    const bool vi = loss == RC_PSM_VILB, pear = loss == psm::LOSS_PEAR;
    const int64_t n4 = (n + 3) / 4 * 4;
    const size_t fixed = 2 * (size_t)n4 + 2 * (size_t)(n + 2) + 16 + (pear ? 8 * psm::PEAR_HEAD : 0);
    const size_t per_slot = vi ? 12 : 4;
    int64_t W = std::min<int64_t>(n + 1, (int64_t)((LDS_BUDGET - fixed) / per_slot));
    if (const long long v = env_int("RC_PSM_WINDOW"); v >= 1 && v < W) W = v;   // tests: force many passes at small n
    const size_t lds = (fixed + per_slot * (size_t)W + 15) / 16 * 16;

    int *d_hi;
    unsigned *d_T = nullptr;
    HIPCHK(c, S.upload(B, st, sizeof(RunOut)));
    HIPCHK(c, B.alloc(d_hi, h_hi.size()));
    HIPCHK(c, hipMemcpyAsync(d_hi, h_hi.data(), h_hi.size() * 4, hipMemcpyHostToDevice, st));
    if (vi) HIPCHK(c, B.alloc(d_T, (size_t)nruns * (size_t)n4));

    Args A{};
    A.a.C = dC; A.a.ld = ld; A.a.init = S.d_init; A.a.sz0 = S.d_sz; A.a.K0 = S.d_K; A.a.hi0 = d_hi; A.a.order = S.d_order;
    A.a.labels = S.d_labels; A.a.out = (RunOut *)S.d_out; A.a.n = (int)n; A.a.W = (int)W; A.a.maxK = maxK; A.a.maxsweeps = maxsweeps;
    A.a.m = (unsigned)m; A.T = d_T; A.n4 = (int)n4;
    HIPCHK(c, S.begin(st));
    const int Q4 = (int)((n4 / 4 + TPB - 1) / TPB);
    const hipError_t le = vi ? launch<RC_PSM_VILB>(Q4, nruns, lds, st, A) : pear ? launch_pear(Q4, nruns, lds, st, A)
                                                                                 : launch<RC_PSM_BINDER>(Q4, nruns, lds, st, A);
    if (le != hipSuccess) return fail(c, RC_ERR_HIP, "point search: launch failed: %s", hipGetErrorString(le));
    std::vector<RunOut> h_out;
    HIPCHK(c, S.collect(st, h_out, kernel_ms));
    if (pear) {
        // num and den from the epilogue's X (same) and P (tot) and the final sizes; the best run is the first of maximal fraction,
        // compared as the kernel compares
        const long long pairs = (long long)n * (n - 1) / 2;
        greedy::results(S, h_out, labels_out, (rc_pear_large_run_t *)runs_out, best, [&](const RunOut &o, rc_pear_large_run_t &R, const int *cnt, int K) {
            long long within = 0;
            for (int k = 1; k <= K; ++k) within += (long long)cnt[k] * (cnt[k] - 1) / 2;
            const widefrac::Frac f = widefrac::fraction(widefrac::make_step(pairs, m, o.tot), (unsigned long long)o.same, (unsigned)within);
            R.num_hi = (int64_t)(f.num >> 64); R.num_lo = (uint64_t)f.num;
            R.den_hi = (int64_t)(f.den >> 64); R.den_lo = (uint64_t)f.den;
            R.X = o.same; R.A = within; R.P = o.tot;
            R.pear = (double)f.num / (double)f.den;
            return WideKey{f};
        });
        return RC_OK;
    }
    greedy::results(S, h_out, labels_out, (rc_psm_run_t *)runs_out, best, psm::Losses{vi, m, n});
    return RC_OK;
}

// rc_psm_search's checks in its order, with this kernel's capacity in place of the LDS one (loss LOSS_PEAR: rc_pear_search_large*,
// which have no loss specifier)
static int32_t check_args(rc_ctx *c, const char *who, int64_t m, int64_t n, int32_t loss, int32_t nruns, const int64_t *init,
                          const int32_t *order, int32_t maxK, int32_t maxsweeps, const int64_t *labels_out, const void *runs_out,
                          const int32_t *best, bool pear = false)
{
    const int32_t rc = greedy::check_args(c, who, m, n, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best);
    if (rc != RC_OK) return rc;
    if (!pear && loss != RC_PSM_BINDER && loss != RC_PSM_VILB) return fail(c, RC_ERR_ARG, "%s: invalid loss specifier %d", who, loss);
    if (n > NMAX) return fail(c, RC_ERR_CAPACITY, "%s: n = %lld exceeds the %d points whose slots fit 16 bits and the workgroup's LDS", who, (long long)n, NMAX);
    if (m > 0x7FFFFFFFll / n) return fail(c, RC_ERR_CAPACITY, "%s: m*n does not fit 31 bits (m=%lld n=%lld)", who, (long long)m, (long long)n);
    return RC_OK;
}

static int32_t search(const char *who, const cnt::Source &src, int32_t loss, int32_t nruns, const int64_t *init, const int32_t *order,
                      int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms, bool pear = false)
{
    return cnt::with(
        who, src,
        [&](rc_ctx *c, int64_t m, int64_t n) { return check_args(c, who, m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best, pear); },
        [&](rc_ctx *c, hipStream_t st, const unsigned *dC, int64_t ld, int64_t m, int64_t n) {
            return run(c, st, dC, ld, m, n, loss, nruns, init, order, maxK, maxsweeps, labels_out, runs_out, best, kernel_ms);
        });
}

}  // namespace psm_large

extern "C" int32_t rc_psm_search_large(int32_t device, const void *counts, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                                       const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                                       void *runs_out, int32_t *best, double *kernel_ms)
{
    return psm_large::search("rc_psm_search_large", cnt::host_counts(device, counts, m, n), loss, nruns, init, order, maxK, maxsweeps,
                             labels_out, runs_out, best, kernel_ms);
}

extern "C" int32_t rc_psm_search_large_samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t loss, int32_t nruns,
                                               const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps,
                                               int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms, double *counts_ms)
{
    return psm_large::search("rc_psm_search_large_samples", cnt::samples(device, samples, m, n, counts_ms), loss, nruns, init, order, maxK,
                             maxsweeps, labels_out, runs_out, best, kernel_ms);
}

extern "C" int32_t rc_psm_search_large_ctx(rc_ctx *c, int64_t numsamples, int32_t loss, int32_t nruns, const int64_t *init,
                                           const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out,
                                           void *runs_out, int32_t *best, double *kernel_ms)
{
    return psm_large::search("rc_psm_search_large_ctx", cnt::context(c, numsamples), loss, nruns, init, order, maxK, maxsweeps, labels_out,
                             runs_out, best, kernel_ms);
}

extern "C" int32_t rc_pear_search_large(int32_t device, const void *counts, int64_t m, int64_t n, int32_t nruns, const int64_t *init,
                                        const int32_t *order, int32_t maxK, int32_t maxsweeps, int64_t *labels_out, void *runs_out,
                                        int32_t *best, double *kernel_ms)
{
    return psm_large::search("rc_pear_search_large", cnt::host_counts(device, counts, m, n), psm::LOSS_PEAR, nruns, init, order, maxK, maxsweeps,
                             labels_out, runs_out, best, kernel_ms, true);
}

extern "C" int32_t rc_pear_search_large_samples(int32_t device, const int64_t *samples, int64_t m, int64_t n, int32_t nruns,
                                                const int64_t *init, const int32_t *order, int32_t maxK, int32_t maxsweeps,
                                                int64_t *labels_out, void *runs_out, int32_t *best, double *kernel_ms, double *counts_ms)
{
    return psm_large::search("rc_pear_search_large_samples", cnt::samples(device, samples, m, n, counts_ms), psm::LOSS_PEAR, nruns, init, order,
                             maxK, maxsweeps, labels_out, runs_out, best, kernel_ms, true);
}

extern "C" int32_t rc_pear_search_large_ctx(rc_ctx *c, int64_t numsamples, int32_t nruns, const int64_t *init, const int32_t *order,
                                            int32_t maxK, int32_t maxsweeps, int64_t *labels_out, rc_pear_large_run_t *runs_out,
                                            int32_t *best, double *kernel_ms)
{
    return psm_large::search("rc_pear_search_large_ctx", cnt::context(c, numsamples), psm::LOSS_PEAR, nruns, init, order, maxK, maxsweeps,
                             labels_out, runs_out, best, kernel_ms, true);
}

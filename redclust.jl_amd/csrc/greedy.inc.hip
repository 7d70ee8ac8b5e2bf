// The greedy search over all partitions that the criteria share — Binder / the VI bound / PEAR on the co-clustering counts
// (pointsearch.inc.hip, k_search) and the exact expected VI / ID on the samples' contingency tables (visearch.inc.hip,
// k_visearch): what is the same whatever the score.  DESIGN.md §8 "Point-estimate search", "One run".
// Included at the end of redclust_hip.hip in front of pointsearch.inc.hip (same translation unit: shares fail(), HIPCHK and
// the holders of hostutil.inc.hip).
//
// A run is one workgroup of TPB threads walking a fixed visiting order.  A step takes point i out of its slot a, scores every
// occupied slot (the criterion's phases A and B), takes the argmin of (score, priority) across the group, considers a new
// cluster, and puts i into the winner (the criterion's phase C); the run ends after a sweep that moves nothing or maxsweeps.
// Ties: lower score first; among equal scores the point's own slot (priority 0: it does not move), then the lowest slot.  A
// new cluster takes the slot the point just emptied if it emptied one (priority 0 again), else the lowest free slot.

namespace greedy {

constexpr int TPB = 1024;
constexpr int NWAVE = TPB / 64;

// (score, priority) pairs compare lexicographically; scores are mapped to u64 so that one reduction serves every criterion
__device__ inline unsigned long long key_i64(long long v) { return (unsigned long long)v ^ 0x8000000000000000ull; }
__device__ inline unsigned long long key_f64(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v + 0.0);   // (−0 + 0 = +0)
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct Cand { unsigned long long sc; unsigned pr, slot, S; };   // S: a payload that travels with the winner (k_search's S_ik)

__device__ inline bool better(unsigned long long sc, unsigned pr, const Cand &b) { return sc < b.sc || (sc == b.sc && pr < b.pr); }

__device__ inline unsigned long long shfl_xor_u64(unsigned long long v, int off)
{
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, off), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

// The walk along one run's order: the point of this step, the one after it, and where the previous point went
struct Visit {
    const int *__restrict__ ord;
    int n, i, i1, iprev;
    unsigned wprev;
    __device__ Visit(const int *order, int n_) : ord(order), n(n_), i(order[0]), i1(order[n_ > 1 ? 1 : 0]), iprev(-1), wprev(0) {}
    // step t's successor; the index of the one after that is fetched now, so that its load is never waited for (n may be 1)
    __device__ int ahead(int t)
    {
        const int inext = i1;
        int t2 = t + 2;
        if (t2 >= n) t2 -= n;
        if (t2 >= n) t2 -= n;
        i1 = ord[t2];
        return inext;
    }
    // the slot i is in: lab[i] was written by another thread without a barrier in between only if i is the previous point (n = 1)
    __device__ unsigned slot_of(const unsigned short *lab) const { return (i == iprev) ? wprev : (unsigned)lab[i]; }
    // i went to w; on to inext.  1 when the partition changed (an unallocated point always)
    __device__ int moved_to(unsigned a, unsigned w, int inext)
    {
        iprev = i; wprev = w;
        i = inext;
        return (a == 0 || w != a) ? 1 : 0;
    }
};

// where the NWAVE per-wave partials of the argmin live in LDS (S only when the payload travels)
struct Partials { unsigned long long *sc; unsigned *pr, *slot, *free, *S; };

// The argmin of the threads' candidates across the group, and the lowest free slot any thread saw, in every thread: xor
// tree over the wave, the partials through LDS, one barrier, a 16-way merge.  WITH_S: Cand::S travels with its candidate
// (otherwise it comes back 0 and costs neither shuffles nor LDS).
template <bool WITH_S>
__device__ inline void group_argmin(Cand &best, unsigned &minfree, const Partials &P, int lane, int wave)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long osc = shfl_xor_u64(best.sc, off);
        const unsigned opr = (unsigned)__shfl_xor((int)best.pr, off), oslot = (unsigned)__shfl_xor((int)best.slot, off);
        const unsigned oS = WITH_S ? (unsigned)__shfl_xor((int)best.S, off) : 0u;
        if (better(osc, opr, best)) best = Cand{osc, opr, oslot, oS};
        minfree = min(minfree, (unsigned)__shfl_xor((int)minfree, off));
    }
    if (lane == 0) { P.sc[wave] = best.sc; P.pr[wave] = best.pr; P.slot[wave] = best.slot; P.free[wave] = minfree; }
    if (WITH_S && lane == 0) P.S[wave] = best.S;
    __syncthreads();
    best = Cand{P.sc[0], P.pr[0], P.slot[0], WITH_S ? P.S[0] : 0u};
    minfree = P.free[0];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) {
        if (better(P.sc[w], P.pr[w], best)) best = Cand{P.sc[w], P.pr[w], P.slot[w], WITH_S ? P.S[w] : 0u};
        minfree = min(minfree, P.free[w]);
    }
}

// The new-cluster candidate (score key_new) against the group's best: 1 when it wins, and best is then the new cluster
__device__ inline unsigned offer_new(Cand &best, unsigned long long key_new, unsigned emptied, unsigned a, unsigned minfree)
{
    const unsigned slot = emptied ? a : minfree, pr = emptied ? 0u : minfree;
    if (!better(key_new, pr, best)) return 0u;
    best = Cand{key_new, pr, slot, 0u};
    return 1u;
}

// ---- a criterion that is a fraction and is maximised (k_search's PEAR, DESIGN.md §8 "PEAR search"): the same ties and the same
// reduction, on (num, den) pairs compared exactly by cross-multiplication in 128 bits

// den > 0 for a candidate (a fraction whose den is 0 is stored as 0/1); den = 0 marks "no candidate yet", which loses to any
struct FCand { long long num, den; unsigned pr, slot, S; };
constexpr FCand FCAND_NONE{0, 0, ~0u, 0u, 0u};

__device__ inline FCand fraction(long long num, long long den, unsigned pr, unsigned slot, unsigned S)
{
    return den ? FCand{num, den, pr, slot, S} : FCand{0, 1, pr, slot, S};
}

// x before b: the larger fraction, then the lower priority (|num|, den < 2^63, so the products fit)
__device__ inline bool fbetter(const FCand &x, const FCand &b)
{
    if (!x.den) return false;
    if (!b.den) return true;
    const __int128 l = (__int128)x.num * b.den, r = (__int128)b.num * x.den;
    return l > r || (l == r && x.pr < b.pr);
}

__device__ inline long long shfl_xor_i64(long long v, int off) { return (long long)shfl_xor_u64((unsigned long long)v, off); }

struct FPartials { long long *num, *den; unsigned *pr, *slot, *free, *S; };

// group_argmin's shape for fractions: the argmax of the threads' candidates and the lowest free slot, in every thread
__device__ inline void group_argmax(FCand &best, unsigned &minfree, const FPartials &P, int lane, int wave)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const FCand o{shfl_xor_i64(best.num, off), shfl_xor_i64(best.den, off), (unsigned)__shfl_xor((int)best.pr, off),
                      (unsigned)__shfl_xor((int)best.slot, off), (unsigned)__shfl_xor((int)best.S, off)};
        if (fbetter(o, best)) best = o;
        minfree = min(minfree, (unsigned)__shfl_xor((int)minfree, off));
    }
    if (lane == 0) {
        P.num[wave] = best.num; P.den[wave] = best.den; P.pr[wave] = best.pr; P.slot[wave] = best.slot; P.S[wave] = best.S;
        P.free[wave] = minfree;
    }
    __syncthreads();
    best = FCand{P.num[0], P.den[0], P.pr[0], P.slot[0], P.S[0]};
    minfree = P.free[0];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) {
        const FCand o{P.num[w], P.den[w], P.pr[w], P.slot[w], P.S[w]};
        if (fbetter(o, best)) best = o;
        minfree = min(minfree, P.free[w]);
    }
}

// offer_new for fractions: the new cluster's fraction num/den against the group's best
__device__ inline unsigned offer_new(FCand &best, long long num, long long den, unsigned emptied, unsigned a, unsigned minfree)
{
    const FCand c = fraction(num, den, emptied ? 0u : minfree, emptied ? a : minfree, 0u);
    if (!fbetter(c, best)) return 0u;
    best = c;
    return 1u;
}

// ---- host side

// What the entry points check first and alike (rc_psm_search, _ctx, _samples, rc_vi_search, rc_id_search, rc_pear_search*); each goes on
// with its own checks in its own order (the loss specifier, the capacities, the samples)
static int32_t check_args(rc_ctx *c, const char *who, int64_t m, int64_t n, int32_t nruns, const int64_t *init, const int32_t *order,
                          int32_t maxK, int32_t maxsweeps, const int64_t *labels_out, const void *runs_out, const int32_t *best)
{
    if (!init || !order || !labels_out || !runs_out || !best) return fail(c, RC_ERR_ARG, "%s: NULL argument", who);
    if (m < 1 || n < 1 || nruns < 1) return fail(c, RC_ERR_ARG, "%s: need m >= 1, n >= 1 and nruns >= 1 (got m=%lld n=%lld nruns=%d)", who, (long long)m, (long long)n, nruns);
    if (maxsweeps < 1 || maxK < 0) return fail(c, RC_ERR_ARG, "%s: need maxsweeps >= 1 and maxK >= 0 (got %d, %d)", who, maxsweeps, maxK);
    return RC_OK;
}

// One run's staging on the host and the device: the starting slots and their sizes (sz_stride entries per run), the
// cluster count, the order, and what comes back — the final slots and one RunOut of the kernel.  The criterion turns the
// caller's init into slots its own way (init_row / sz_row / K); everything else is here.
struct Staging {
    const int64_t n;
    const int nruns;
    const size_t sz_stride;
    std::vector<unsigned short> init, sz, labels;
    std::vector<int> K, order;
    std::vector<char> seen;
    unsigned short *d_init = nullptr, *d_sz = nullptr, *d_labels = nullptr;
    int *d_K = nullptr, *d_order = nullptr;
    void *d_out = nullptr;
    TimingEvents ev;

    Staging(int nruns_, int64_t n_, size_t sz_stride_)
        : n(n_), nruns(nruns_), sz_stride(sz_stride_), init((size_t)nruns_ * n_), sz((size_t)nruns_ * sz_stride_, 0), labels(init.size()),
          K((size_t)nruns_), order((size_t)nruns_ * n_), seen((size_t)n_) {}
    unsigned short *init_row(int r) { return init.data() + (size_t)r * n; }
    unsigned short *sz_row(int r) { return sz.data() + (size_t)r * sz_stride; }

    // run r's order, a permutation of 1..n, to 0-based ints; the error's text starts with `who`
    int32_t take_order(rc_ctx *c, const char *who, int r, const int32_t *all_orders)
    {
        std::fill(seen.begin(), seen.end(), 0);
        for (int64_t t = 0; t < n; ++t) {
            const int32_t o = all_orders[(size_t)r * n + t];
            if (o < 1 || o > n || seen[(size_t)o - 1]) return fail(c, RC_ERR_ARG, "%s: the order of run %d is not a permutation of 1..n", who, r + 1);
            seen[(size_t)o - 1] = 1;
            order[(size_t)r * n + t] = o - 1;
        }
        return RC_OK;
    }
    // device copies of the four inputs and room for the two outputs (out_bytes per run), owned by B
    hipError_t upload(DeviceBuffers &B, hipStream_t st, size_t out_bytes)
    {
        const auto put = [&](auto *&d, const auto &h) {
            const hipError_t e = B.alloc(d, h.size());
            return e == hipSuccess ? hipMemcpyAsync(d, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice, st) : e;
        };
        unsigned char *out = nullptr;
        hipError_t e = put(d_init, init);
        if (e == hipSuccess) e = put(d_sz, sz);
        if (e == hipSuccess) e = put(d_K, K);
        if (e == hipSuccess) e = put(d_order, order);
        if (e == hipSuccess) e = B.alloc(d_labels, labels.size());
        if (e == hipSuccess) e = B.alloc(out, (size_t)nruns * out_bytes);
        d_out = out;
        return e;
    }
    // around the launch: begin(st); the kernel; collect(st, …): its error, the final slots and the records, its device time
    hipError_t begin(hipStream_t st) { const hipError_t e = ev.create(); return e == hipSuccess ? ev.begin(st) : e; }
    template <typename RunOut> hipError_t collect(hipStream_t st, std::vector<RunOut> &out, double *kernel_ms)
    {
        out.resize((size_t)nruns);
        hipError_t e = ev.end(st);
        if (e == hipSuccess) e = hipMemcpyAsync(labels.data(), d_labels, labels.size() * 2, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(RunOut), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        double ms = 0.0;
        if (e == hipSuccess) e = ev.elapsed_ms(ms);
        if (e == hipSuccess && kernel_ms) *kernel_ms = ms;
        return e;
    }
};

// The results of the runs: sortlabels (utils.jl:69-74) of the final slots into labels_out, the runs' records (rc_psm_run_t, or
// rc_pear_run_t for the PEAR search), and in *best the first run of minimal key.  loss(o, R, cnt, K) sets R's criterion fields
// from the kernel's record o — cnt[1..K] are the sizes of the sorted clusters — and returns the key the runs are compared by
// with <: a number that is minimised, or a type whose < says "better".
template <typename RunOut, typename Run, typename Loss>
static void results(const Staging &S, const std::vector<RunOut> &out, int64_t *labels_out, Run *runs_out, int32_t *best, Loss loss)
{
    const int64_t n = S.n;
    std::vector<int> map((size_t)n + 1), cnt((size_t)n + 1);
    decltype(loss(out[0], runs_out[0], cnt.data(), 0)) least{};
    int b = 0;
    for (int r = 0; r < S.nruns; ++r) {
        std::fill(map.begin(), map.end(), 0);
        std::fill(cnt.begin(), cnt.end(), 0);
        int next = 0;
        for (int64_t j = 0; j < n; ++j) {
            const unsigned short l = S.labels[(size_t)r * n + j];
            if (!map[l]) map[l] = ++next;
            labels_out[(size_t)r * n + j] = map[l];
            cnt[(size_t)map[l]]++;
        }
        const RunOut &o = out[(size_t)r];
        Run &R = runs_out[r];
        R.sweeps = o.sweeps; R.converged = o.converged; R.moves = o.moves; R.K = o.K;
        const auto key = loss(o, R, cnt.data(), next);
        if (r == 0 || key < least) { b = r; least = key; }
    }
    *best = b;
}

}  // namespace greedy

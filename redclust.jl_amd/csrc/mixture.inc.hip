// generatemixture's oracle co-clustering matrix (src/utils.jl:130-143 of the reference) on the device.  Derivation, order
// and exactness contract as in DESIGN.md §8.  Included at the end of redclust_hip.hip (same translation unit: shares fail(),
// HIPCHK and the holders of hostutil.inc.hip).
//
// The centres are radius·e_j, so every factor of w_j·pdf(MvNormal(c_j, σ²I), x_i) but exp(radius·x_ij/σ²) is common to
// all j and cancels in the normalisation: with b_ij = radius·x_ij/σ² (j < K only),
//     P_t[i][j] = softmax_j(log w_tj + b_ij)   (row maximum subtracted),     oracle = (1/T)·Σ_t P_t P_tᵀ = (1/T)·QᵀQ,
// where Q[l][i], l = t·K4 + j, holds every P_t (K4 = K rounded up to a multiple of 4, rows j >= K and columns i >= n zero).
//
// A chunk of whole iterations at a time, k_mix_q writes Q and k_mix_syrk adds QᵀQ to the running sum S on the upper block
// triangle of 128 × 128 tiles with v_mfma_f64_16x16x4_f64: a tile loads its part of S into the accumulators, runs every
// 4-step of the chunk in ascending l (K4 % 4 == 0: a 4-step never straddles two iterations) and stores the sum back.  Every
// entry is therefore summed in one fixed order whatever the chunking.  k_mix_finish divides by T once (utils.jl:142) and
// mirrors the upper triangle, so the result is exactly symmetric.  No BLAS on this path.

#define RC_MIX_TILE 128                              // tile edge of the product: 4 waves of 64 × 64
#define RC_MIX_MAX_N (1 << 16)                       // S is npad² f64 on the device: 32 GiB at the bound
#define RC_MIX_CHUNK_BYTES ((int64_t)1 << 30)        // Q workspace of the automatic plan

namespace mixture {

typedef double d4 __attribute__((ext_vector_type(4)));

// Q rows of chunk iterations t = 0..iters-1: thread (i, t); B: K × npad, logw: iters × K (log of the weights, -inf for 0)
__global__ __launch_bounds__(256) void k_mix_q(int npad, int n, int K, int K4, int iters, const double *__restrict__ B,
                                               const double *__restrict__ logw, double *__restrict__ Q)
{
#pragma clang fp contract(off)
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= npad) return;
    for (int t = (int)blockIdx.y; t < iters; t += (int)gridDim.y) {
        double *q = Q + (size_t)t * K4 * npad + i;
        const double *lw = logw + (size_t)t * K;
        int j0 = 0;
        if (i < n) {
            double m = -INFINITY;
            for (int j = 0; j < K; ++j) m = fmax(m, lw[j] + B[(size_t)j * npad + i]);
            double s = 0.0;
            for (int j = 0; j < K; ++j) s += exp((lw[j] + B[(size_t)j * npad + i]) - m);
            for (int j = 0; j < K; ++j) q[(size_t)j * npad] = exp((lw[j] + B[(size_t)j * npad + i]) - m) / s;
            j0 = K;
        }
        for (int j = j0; j < K4; ++j) q[(size_t)j * npad] = 0.0;
    }
}

// S[I][J] += Σ_{l < L} Q[l][I]·Q[l][J] for the tile (tiles[2b], tiles[2b+1]) of the upper block triangle.  Wave w covers
// rows 64·(w>>1) and columns 64·(w&1) of the tile as 4 × 4 blocks of 16 × 16.  Operand of 16x16x4: lane holds
// A[i = lane&15][k = lane>>4] and B[k = lane>>4][j = lane&15]; result: acc[r] is row (lane>>4) + 4r, column lane&15.
__global__ __launch_bounds__(256) void k_mix_syrk(int npad, int L, const int *__restrict__ tiles, const double *__restrict__ Q,
                                                  double *__restrict__ S)
{
    const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
    const int i0 = tiles[2 * blockIdx.x] * RC_MIX_TILE + 64 * (w >> 1), j0 = tiles[2 * blockIdx.x + 1] * RC_MIX_TILE + 64 * (w & 1);
    const int r16 = lane & 15, kq = lane >> 4;
    d4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[a][c][r] = S[(size_t)(i0 + 16 * a + kq + 4 * r) * npad + j0 + 16 * c + r16];
    const double *qa = Q + (size_t)kq * npad + i0 + r16, *qb = Q + (size_t)kq * npad + j0 + r16;
    const size_t step = (size_t)4 * npad;
    double fa[4], fb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) { fa[a] = qa[16 * a]; fb[a] = qb[16 * a]; }
#pragma unroll 2
    for (int l = 0; l < L; l += 4) {
        if (l + 4 < L) { qa += step; qb += step; }   // the last step reloads its own rows: no branch around the loads
        double na[4], nb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) { na[a] = qa[16 * a]; nb[a] = qb[16 * a]; }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[c], acc[a][c], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 4; ++a) { fa[a] = na[a]; fb[a] = nb[a]; }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                S[(size_t)(i0 + 16 * a + kq + 4 * r) * npad + j0 + 16 * c + r16] = acc[a][c][r];
}

// In place on S: for the 32 × 32 block (bi, bj), bi <= bj, write v = S[i][j] / T to [i][j] and [j][i] (i <= j).  Block
// (bx, by) with by > bx only; 32 × 8 threads.
__global__ __launch_bounds__(256) void k_mix_finish(int npad, double T, double *__restrict__ S)
{
    const int bi = (int)blockIdx.y, bj = (int)blockIdx.x;
    if (bi > bj) return;
    __shared__ double t[32][33];
    const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
    const size_t r0 = (size_t)bi * 32, c0 = (size_t)bj * 32;
    for (int y = ty; y < 32; y += 8) t[y][tx] = S[(r0 + y) * npad + c0 + tx] / T;
    __syncthreads();
    if (bi == bj) {
        for (int y = ty; y < 32; y += 8) S[(r0 + y) * npad + c0 + tx] = (y <= tx) ? t[y][tx] : t[tx][y];
    } else {
        for (int y = ty; y < 32; y += 8) {
            S[(r0 + y) * npad + c0 + tx] = t[y][tx];
            S[(c0 + y) * npad + r0 + tx] = t[tx][y];
        }
    }
}

}  // namespace mixture

extern "C" int32_t rc_oracle_coclustering(int32_t device, int64_t n, int64_t dim, const double *points, int64_t K, double radius,
                                          double sigma, int64_t numiters, const double *weights, int64_t iters_per_chunk,
                                          double *out, double *kernel_ms)
{
    if (!points || !weights || !out) return fail(nullptr, RC_ERR_ARG, "rc_oracle_coclustering: NULL argument");
    if (n < 1 || n > RC_MIX_MAX_N) return fail(nullptr, RC_ERR_ARG, "rc_oracle_coclustering: n must be in 1..2^16 (got %lld)", (long long)n);
    if (K < 1 || K > dim) return fail(nullptr, RC_ERR_ARG, "rc_oracle_coclustering: K must be in 1..dim (K = %lld, dim = %lld)", (long long)K, (long long)dim);
    if (!(sigma > 0) || !std::isfinite(sigma) || !(radius > 0) || !std::isfinite(radius))
        return fail(nullptr, RC_ERR_ARG, "rc_oracle_coclustering: radius and sigma must be positive and finite");
    if (numiters < 1) return fail(nullptr, RC_ERR_ARG, "rc_oracle_coclustering: numiters must be >= 1 (got %lld)", (long long)numiters);
    if (iters_per_chunk < 0) return fail(nullptr, RC_ERR_ARG, "rc_oracle_coclustering: iters_per_chunk must be >= 0 (0 = automatic)");
    const int npad = (int)((n + RC_MIX_TILE - 1) / RC_MIX_TILE * RC_MIX_TILE), K4 = (int)((K + 3) / 4 * 4);
    // b (K × npad, zero padded) and log w, checked on the host
    std::vector<double> B((size_t)K * npad, 0.0), logw((size_t)numiters * K);
    const double scale = radius / (sigma * sigma);
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t d = 0; d < dim; ++d)
            if (!std::isfinite(points[i * dim + d])) return fail(nullptr, RC_ERR_DOMAIN, "rc_oracle_coclustering: points must be finite (point %lld)", (long long)i);
        for (int64_t j = 0; j < K; ++j) {
            const double b = scale * points[i * dim + j];
            if (!std::isfinite(b)) return fail(nullptr, RC_ERR_DOMAIN, "rc_oracle_coclustering: radius·x/σ² is not finite (point %lld)", (long long)i);
            B[(size_t)j * npad + i] = b;
        }
    }
    for (int64_t t = 0; t < numiters; ++t) {
        bool pos = false;
        for (int64_t j = 0; j < K; ++j) {
            const double v = weights[t * K + j];
            if (!std::isfinite(v) || v < 0) return fail(nullptr, RC_ERR_DOMAIN, "rc_oracle_coclustering: weights must be finite and non-negative (row %lld)", (long long)t);
            pos |= v > 0;
            logw[(size_t)t * K + j] = (v > 0) ? std::log(v) : -INFINITY;
        }
        if (!pos) return fail(nullptr, RC_ERR_DOMAIN, "rc_oracle_coclustering: weight row %lld has no positive entry", (long long)t);
    }
    // iterations per chunk: a Q of about RC_MIX_CHUNK_BYTES, or the caller's count
    const int64_t per_iter = (int64_t)K4 * npad * 8;
    const int64_t ipc = std::min<int64_t>(numiters, iters_per_chunk > 0 ? iters_per_chunk : std::max<int64_t>(1, RC_MIX_CHUNK_BYTES / per_iter));
    const int nb = npad / RC_MIX_TILE;
    std::vector<int> tiles;
    for (int bi = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj) { tiles.push_back(bi); tiles.push_back(bj); }
    int32_t rc = select_device("rc_oracle_coclustering", device);
    if (rc != RC_OK) return rc;
    DeviceBuffers bufs;
    TimingEvents ev;
    double *d_B, *d_lw, *d_Q, *d_S;
    int *d_tiles;
    HIPCHK(nullptr, bufs.alloc(d_B, B.size()));
    HIPCHK(nullptr, bufs.alloc(d_lw, logw.size()));
    HIPCHK(nullptr, bufs.alloc(d_Q, (size_t)(ipc * per_iter) / 8));
    HIPCHK(nullptr, bufs.alloc(d_S, (size_t)npad * npad));
    HIPCHK(nullptr, bufs.alloc(d_tiles, tiles.size()));
    HIPCHK(nullptr, hipMemcpy(d_B, B.data(), B.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_lw, logw.data(), logw.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(d_tiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemset(d_S, 0, (size_t)npad * npad * 8));
    HIPCHK(nullptr, ev.create());
    HIPCHK(nullptr, ev.begin(0));
    for (int64_t t0 = 0; t0 < numiters; t0 += ipc) {
        const int it = (int)std::min<int64_t>(ipc, numiters - t0);
        mixture::k_mix_q<<<dim3((unsigned)((npad + 255) / 256), (unsigned)std::min(it, 65535)), 256, 0, 0>>>(
            npad, (int)n, (int)K, K4, it, d_B, d_lw + (size_t)t0 * K, d_Q);
        HIPCHK(nullptr, hipGetLastError());
        mixture::k_mix_syrk<<<(unsigned)(tiles.size() / 2), 256, 0, 0>>>(npad, it * K4, d_tiles, d_Q, d_S);
        HIPCHK(nullptr, hipGetLastError());
    }
    mixture::k_mix_finish<<<dim3((unsigned)(npad / 32), (unsigned)(npad / 32)), 256, 0, 0>>>(npad, (double)numiters, d_S);
    HIPCHK(nullptr, ev.end(0));
    double ms = 0.0;
    HIPCHK(nullptr, ev.elapsed_ms(ms));
    HIPCHK(nullptr, hipMemcpy2D(out, (size_t)n * 8, d_S, (size_t)npad * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost));
    if (kernel_ms) *kernel_ms = ms;
    return RC_OK;
}

// gfx950 kernels and host driver of the MBAR Gram pass: with the weight matrix of M = n_state + n_extra columns over N samples
//     W[n][k]           = exp(f_k - u_k(n) - D_n)          k < n_state   (u_k, D_n as in kernels_mbar.hip; mbar_energy of mbar_device.h)
//     W[n][n_state + j] = exp(log_extra[j][n])             a host-supplied log-column, -inf = weight 0
// it returns G = W^T W (M x M) and the column sums c_k = sum_n W[n][k].  G and the sample counts give the asymptotic covariance of the
// free energies (Shirts & Chodera 2008, eq. D8/D9); G and c give the Hessian diag(N_k c_k) - N G N of the MBAR objective.  W is never held
// whole: it is generated in slabs of R consecutive samples into a workspace, column-major (Wt[k][r], so that a lane per sample stores
// coalesced and a tile load reads 256-byte runs), and each slab is folded into G before the next is made.
//   - k_mbar_gram_slab: one lane owns one sample of the slab (its values, E_n and D_n in registers) and walks the states ascending,
//     staged in LDS tiles of UPK_MBAR_STATE_TILE exactly as k_mbar_denominator does; each exponential is computed once per slab.  Rows
//     past the last sample (the slab is rounded up to the row granule) are written as 0.
//   - k_mbar_gram_extra: the explicit columns of the slab, and zeros in the padding columns M .. Mp (Mp = M rounded up to the tile).
//   - k_mbar_gram_tile: one workgroup (4 waves) owns one 64 x 64 tile (ti <= tj) of G for the whole slab.  It walks the slab in chunks
//     of 32 rows: the two 64-column panels go through LDS (stride 34 doubles per column: the MFMA operand reads of a half-wave then
//     touch every bank once -- by the address arithmetic, no counter run backs it), and each wave keeps a 32 x 32 quarter of the tile as 2 x 2 accumulators of v_mfma_f64_16x16x4_f64
//     (A[i][k] = Wt[ti 64 + i][k], B[k][j] = Wt[tj 64 + j][k]: lane l holds i or j = l & 15, k = l >> 4; D: column l & 15, row
//     (l >> 4) + 4 reg).  The accumulators start from G (0 for the first slab) and return to it, so every element is summed by one lane
//     in ascending sample order through one instruction sequence: two calls give the same bits.  No atomics.
//     Where the upper triangle has too few tiles to fill the device (M < 2048), the chunks of a slab are cut into P = gram_parts(M)
//     consecutive ranges and workgroup (tile, p) accumulates range p into a partial matrix of its own, partial[p] (Mp x Mp, at the
//     front of the workspace); k_mbar_gram_reduce then adds the partials in ascending p.  P depends on M alone, so the order is fixed.
//   - k_mbar_gram_mirror: G[row][col] = G[col][row] for row > col, after the last slab: G is bitwise symmetric.
//   - k_mbar_gram_colsum / _colsum_extra: c_k by the free-energy pass's shape (a workgroup per UPK_MBAR_FE_TILE columns, lane t takes
//     samples t, t + 256, ... ascending, block_sum).  It needs no workspace and is the whole of a call with G == NULL.
// upk_mbar_gram_solve is the host side of upside_hip_mbar_gram: every refusal returns before any device call.
#include "mbar_device.h"

using namespace up;
using namespace up::mbar;

#define GRAM_TILE UPK_MBAR_GRAM_TILE
#define GRAM_CHUNK UPK_MBAR_GRAM_GRANULE
#define GRAM_LDS_STRIDE (GRAM_CHUNK + 2)
static_assert(GRAM_TILE == 64 && GRAM_CHUNK == 32 && MBAR_BLOCK == 256, "k_mbar_gram_tile is written for 4 waves, 64 x 64 tiles and 32-row chunks");

namespace {

typedef double gram_acc_t __attribute__((ext_vector_type(4)));

inline int gram_padded(int m) { return (m + GRAM_TILE - 1) / GRAM_TILE * GRAM_TILE; }
// the ranges a slab is cut into: 1 where the upper triangle alone has 512 tiles or more, else enough for about 1024 workgroups, at most 64
inline int gram_parts(int m) {
    const int nt = gram_padded(m) / GRAM_TILE, pairs = nt * (nt + 1) / 2;
    if (pairs >= 512) return 1;
    return 1024 / pairs < 64 ? 1024 / pairs : 64;
}
inline size_t gram_partial_bytes(int m) { const int p = gram_parts(m); return p > 1 ? (size_t)p * gram_padded(m) * gram_padded(m) * sizeof(double) : 0; }

// the exponent of a parametric entry in the order of its definition, (f_k - beta_k e) - D_n, every operation rounded on its own: with
// reduced energies of 1e5 and more the three terms cancel, and a fused multiply-add would round differently from the definition
__device__ __forceinline__ double gram_exponent(double f, double beta, double e, double dn) {
#pragma clang fp contract(off)
    const double u = beta * e;
    return (f - u) - dn;
}

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_slab(upk_mbar_states_t S, upk_mbar_samples_t X, const double* __restrict__ denom,
                                                                const double* __restrict__ f, long long n0, int rows_pad, long long R,
                                                                double* __restrict__ Wt) {
    constexpr int W = mbar_state_doubles<D>();
    __shared__ double tile[MBAR_TILE * W];
    const int tid = threadIdx.x;
    const long long r = (long long)blockIdx.x * MBAR_BLOCK + tid;
    const long long n_raw = n0 + r;
    const long long n = n_raw < X.n ? n_raw : X.n - 1;      // (a lane past the end repeats the last sample and stores 0 or nothing)
    double v[D ? D : 1], E;
    mbar_load_sample<D>(X, n, v, E);
    const double dn = denom[n];
    for (int k0 = 0; k0 < S.n_state; k0 += MBAR_TILE) {
        const int nt = mbar_stage_tile<D>(S, k0, f, tile);
        if (r < rows_pad)
            for (int l = 0; l < nt; ++l) {
                const double* __restrict__ st = tile + l * W;
                const double w = exp(gram_exponent(st[0], st[1], mbar_energy<D>(v, E, st, S), dn));
                Wt[(size_t)(k0 + l) * R + r] = n_raw < X.n ? w : 0.;
            }
    }
}

// columns n_state .. Mp of the slab: blockIdx.y = column - n_state
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_extra(long long n, int n_state, int n_extra, const double* __restrict__ log_extra,
                                                                 long long n0, int rows_pad, long long R, double* __restrict__ Wt) {
    const long long r = (long long)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    const int j = blockIdx.y;
    if (r >= rows_pad) return;
    double w = 0.;
    if (j < n_extra && n0 + r < n) w = exp(log_extra[(size_t)j * n + n0 + r]);
    Wt[(size_t)(n_state + j) * R + r] = w;
}

// grid (tile of the upper triangle, part).  C: the accumulators' home, G itself (m = M) or the partials (m = Mp, a matrix per part).
// The tiles are numbered along one grid axis, not laid out as a square grid whose lower half returns at once: measured, the idle
// workgroups of such a grid leave the working ones unevenly spread over the device (13.1 against 6.9 ms at M = 1024, N = 2^18).
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_tile(const double* __restrict__ Wt, long long R, int n_chunk, int m, int n_tile,
                                                                int first, double* __restrict__ C) {
    __shared__ double As[GRAM_TILE * GRAM_LDS_STRIDE];
    __shared__ double Bs[GRAM_TILE * GRAM_LDS_STRIDE];
    // blockIdx.x counts the tiles of the upper triangle row by row: (0, 0), (0, 1), ..., (1, 1), ...; at most n_tile <= 128 scalar steps
    int ti = 0, rest = blockIdx.x;
    while (rest >= n_tile - ti) { rest -= n_tile - ti; ++ti; }
    const int tj = ti + rest;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int li = lane & 15, lk = lane >> 4;
    const double* __restrict__ Bp = ti == tj ? As : Bs;
    double* __restrict__ G = C + (size_t)blockIdx.y * m * m;
    const int c_begin = (int)((long long)blockIdx.y * n_chunk / gridDim.y), c_end = (int)((long long)(blockIdx.y + 1) * n_chunk / gridDim.y);

    gram_acc_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = ti * GRAM_TILE + wr + a * 16 + lk + 4 * q, col = tj * GRAM_TILE + wc + b * 16 + li;
                acc[a][b][q] = (!first && row < m && col < m) ? G[(size_t)row * m + col] : 0.;
            }

    for (int c = c_begin; c < c_end; ++c) {
        __syncthreads();      // (the previous chunk has been read)
#pragma unroll
        for (int i = 0; i < GRAM_TILE * GRAM_CHUNK / MBAR_BLOCK; ++i) {
            const int e = tid + i * MBAR_BLOCK, col = e / GRAM_CHUNK, r = e - col * GRAM_CHUNK;
            As[col * GRAM_LDS_STRIDE + r] = Wt[(size_t)(ti * GRAM_TILE + col) * R + (size_t)c * GRAM_CHUNK + r];
            if (ti != tj) Bs[col * GRAM_LDS_STRIDE + r] = Wt[(size_t)(tj * GRAM_TILE + col) * R + (size_t)c * GRAM_CHUNK + r];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < GRAM_CHUNK; kk += 4) {
            const double a0 = As[(wr + li) * GRAM_LDS_STRIDE + kk + lk], a1 = As[(wr + 16 + li) * GRAM_LDS_STRIDE + kk + lk];
            const double b0 = Bp[(wc + li) * GRAM_LDS_STRIDE + kk + lk], b1 = Bp[(wc + 16 + li) * GRAM_LDS_STRIDE + kk + lk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }

#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = ti * GRAM_TILE + wr + a * 16 + lk + 4 * q, col = tj * GRAM_TILE + wc + b * 16 + li;
                if (row < m && col < m) G[(size_t)row * m + col] = acc[a][b][q];
            }
}

// G[row][col] = partial[0][row][col] + partial[1][row][col] + ... in ascending order, over the tiles of the upper triangle
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_reduce(const double* __restrict__ partial, int n_part, int mp, int m, double* __restrict__ G) {
    const size_t i = (size_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (i >= (size_t)m * m) return;
    const size_t row = i / m, col = i - row * m;
    if (row / GRAM_TILE > col / GRAM_TILE) return;
    double s = 0.;
    for (int p = 0; p < n_part; ++p) s += partial[((size_t)p * mp + row) * mp + col];
    G[i] = s;
}

__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_mirror(int m, double* __restrict__ G) {
    const size_t i = (size_t)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (i >= (size_t)m * m) return;
    const size_t row = i / m, col = i - row * m;
    if (row > col) G[i] = G[col * m + row];
}

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_colsum(upk_mbar_states_t S, upk_mbar_samples_t X, const double* __restrict__ denom,
                                                                  const double* __restrict__ f, double* __restrict__ colsum) {
    constexpr int W = mbar_state_doubles<D>();
    __shared__ double st[MBAR_FE][W];
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    const int tid = threadIdx.x, k0 = blockIdx.x * MBAR_FE;
    mbar_stage_fe<D, true>(S, k0, f, st);
    __syncthreads();
    double s[MBAR_FE];
#pragma unroll
    for (int l = 0; l < MBAR_FE; ++l) s[l] = 0.;
    for (long long n = tid; n < X.n; n += MBAR_BLOCK) {
        double v[D ? D : 1], E;
        mbar_load_sample<D>(X, n, v, E);
        const double dn = denom[n];
#pragma unroll
        for (int l = 0; l < MBAR_FE; ++l) s[l] += exp(gram_exponent(st[l][0], st[l][1], mbar_energy<D>(v, E, st[l], S), dn));
    }
    block_sum<MBAR_FE>(s, part);
    if (tid == 0) {
#pragma unroll
        for (int l = 0; l < MBAR_FE; ++l) if (k0 + l < S.n_state) colsum[k0 + l] = s[l];
    }
}

__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_gram_colsum_extra(long long n, int n_state, const double* __restrict__ log_extra,
                                                                        double* __restrict__ colsum) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    const int j = blockIdx.x;
    double s[1] = {0.};
    for (long long i = threadIdx.x; i < n; i += MBAR_BLOCK) s[0] += exp(log_extra[(size_t)j * n + i]);
    block_sum<1>(s, part);
    if (threadIdx.x == 0) colsum[n_state + j] = s[0];
}

}  // namespace

extern "C" int upk_mbar_gram_tile(void) { return GRAM_TILE; }
extern "C" size_t upk_mbar_gram_partial_bytes(int m) { return m < 1 || m > UPK_MBAR_GRAM_MAX_COLUMNS ? 0 : gram_partial_bytes(m); }
extern "C" long long upk_mbar_gram_rows(int m, size_t workspace_bytes) {
    if (m < 1 || m > UPK_MBAR_GRAM_MAX_COLUMNS) return 0;
    if (workspace_bytes < gram_partial_bytes(m)) return 0;
    const size_t rows = (workspace_bytes - gram_partial_bytes(m)) / ((size_t)gram_padded(m) * sizeof(double)) / GRAM_CHUNK * GRAM_CHUNK;
    return (long long)(rows < ((size_t)1 << 30) ? rows : ((size_t)1 << 30));
}

extern "C" int upk_mbar_gram(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* denom, const double* f,
                             int n_extra, const double* log_extra, double* G, double* colsum, void* workspace, size_t workspace_bytes) {
    if (!launch_args_ok(S, X) || !denom || !f || !colsum || n_extra < 0 || (n_extra > 0 && !log_extra) ||
        S->n_state > UPK_MBAR_GRAM_MAX_COLUMNS - n_extra) return 9404;
    const int m = S->n_state + n_extra, mp = gram_padded(m);
    const long long R = G ? upk_mbar_gram_rows(m, workspace ? workspace_bytes : 0) : 0;
    if (G && R < GRAM_CHUNK) return 9405;
    hipStream_t st = (hipStream_t)stream;
    MBAR_DISPATCH(k_mbar_gram_colsum, (unsigned)((S->n_state + MBAR_FE - 1) / MBAR_FE), *S, *X, denom, f, colsum)
    if (n_extra) hipLaunchKernelGGL(k_mbar_gram_colsum_extra, dim3(n_extra), dim3(MBAR_BLOCK), 0, st, X->n, S->n_state, log_extra, colsum);
    if (!G) return launch_status();
    const int n_part = gram_parts(m);
    double* partial = (double*)workspace;
    double* Wt = (double*)((char*)workspace + gram_partial_bytes(m));
    const int n_tile = mp / GRAM_TILE;
    for (long long n0 = 0; n0 < X->n; n0 += R) {
        const long long rows = X->n - n0 < R ? X->n - n0 : R;
        const int rows_pad = (int)((rows + GRAM_CHUNK - 1) / GRAM_CHUNK * GRAM_CHUNK);      // <= R, a multiple of the granule
        const unsigned row_blocks = sample_blocks(rows_pad);
        MBAR_DISPATCH(k_mbar_gram_slab, row_blocks, *S, *X, denom, f, n0, rows_pad, R, Wt)
        if (mp > S->n_state)
            hipLaunchKernelGGL(k_mbar_gram_extra, dim3(row_blocks, mp - S->n_state), dim3(MBAR_BLOCK), 0, st, X->n, S->n_state, n_extra, log_extra, n0,
                               rows_pad, R, Wt);
        if (n_part > 1)
            hipLaunchKernelGGL(k_mbar_gram_tile, dim3(n_tile * (n_tile + 1) / 2, n_part), dim3(MBAR_BLOCK), 0, st, Wt, R, rows_pad / GRAM_CHUNK, mp, n_tile,
                               n0 == 0 ? 1 : 0, partial);
        else
            hipLaunchKernelGGL(k_mbar_gram_tile, dim3(n_tile * (n_tile + 1) / 2), dim3(MBAR_BLOCK), 0, st, Wt, R, rows_pad / GRAM_CHUNK, m, n_tile,
                               n0 == 0 ? 1 : 0, G);
        const int rc = launch_status();
        if (rc) return rc;
    }
    if (n_part > 1)
        hipLaunchKernelGGL(k_mbar_gram_reduce, dim3((unsigned)(((size_t)m * m + MBAR_BLOCK - 1) / MBAR_BLOCK)), dim3(MBAR_BLOCK), 0, st, partial, n_part, mp, m, G);
    hipLaunchKernelGGL(k_mbar_gram_mirror, dim3((unsigned)(((size_t)m * m + MBAR_BLOCK - 1) / MBAR_BLOCK)), dim3(MBAR_BLOCK), 0, st, m, G);
    return launch_status();
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
namespace {

// the slab length of the public entry: a function of M alone, never of free memory, so the returned bits do not depend on the
// machine's state.  At most UPK_MBAR_GRAM_MAX_WORKSPACE bytes and at most 2^16 rows.
size_t gram_public_workspace(int m) {
    long long rows = upk_mbar_gram_rows(m, UPK_MBAR_GRAM_MAX_WORKSPACE);
    if (rows > 65536) rows = 65536;
    return gram_partial_bytes(m) + (size_t)rows * gram_padded(m) * sizeof(double);
}

// every refusal of upside_hip_mbar_gram; nothing here touches the device
void gram_check(const upk_mbar_gram_problem_t& P) {
    size_t at = 0;
    if (P.n_extra < 0) MBAR_REFUSE("mbar_gram: n_extra = %d is negative", P.n_extra);
    if (P.n_state < 1) MBAR_REFUSE("mbar_gram: n_state = %d, at least one state is needed", P.n_state);
    if (P.n_state > UPK_MBAR_GRAM_MAX_COLUMNS - P.n_extra)
        MBAR_REFUSE("mbar_gram: n_state + n_extra = %d + %d columns, at most %d are supported", P.n_state, P.n_extra, UPK_MBAR_GRAM_MAX_COLUMNS);
    if (!P.colsum) MBAR_REFUSE("mbar_gram: colsum must be given");
    if (!P.f) MBAR_REFUSE("mbar_gram: f must be given");
    if (P.n_extra > 0 && !P.log_extra) MBAR_REFUSE("mbar_gram: log_extra must be given when n_extra > 0");
    // the samples and the states: the refusals of upside_hip_mbar, one statement of them
    upk_mbar_problem_t Q = as_mbar_problem(P);
    Q.tol = 0.; Q.max_iter = 1; Q.f = const_cast<double*>(P.f);
    mbar_check(Q);
    if (!all_finite(P.f, (size_t)P.n_state, &at)) MBAR_REFUSE("mbar_gram: f[%zu] is not finite", at);
    const size_t N = (size_t)P.n_sample;
    for (size_t j = 0; j < (size_t)P.n_extra; ++j)
        for (size_t n = 0; n < N; ++n) {
            const double x = P.log_extra[j * N + n];
            if (std::isnan(x) || x == INFINITY) MBAR_REFUSE("mbar_gram: log_extra: column %zu, sample %zu is %s (-inf is weight 0)", j, n, std::isnan(x) ? "not a number" : "+inf");
        }
}

void gram_run(const upk_mbar_gram_problem_t& P) {
    gram_check(P);
    StagedProblem staged(P);
    const upk_mbar_states_t& S = staged.S; const upk_mbar_samples_t& X = staged.X; Stream& st = staged.st;
    const int K = P.n_state, M = K + P.n_extra;
    const size_t N = (size_t)P.n_sample;
    DeviceBuffer a, f_dev, denom, extra, G, colsum, work;
    std::vector<double> av(K);
    log_counts_plus_f(log_sample_counts(P.n_k, K), P.f, av.data());
    a.upload(st.s, av.data(), K * sizeof(double), "copy of f");
    f_dev.upload(st.s, P.f, K * sizeof(double), "copy of f");
    if (P.n_extra) extra.upload(st.s, P.log_extra, (size_t)P.n_extra * N * sizeof(double), "copy of log_extra");
    denom.alloc(N * sizeof(double), "denominators"); colsum.alloc(M * sizeof(double), "colsum");
    const size_t work_bytes = P.G ? gram_public_workspace(M) : 0;
    if (P.G) { G.alloc((size_t)M * M * sizeof(double), "G"); work.alloc(work_bytes, "workspace"); }

    upk_ok(upk_mbar_denominator(st.s, &S, &X, a.as<double>(), denom.as<double>()), "denominator pass");
    upk_ok(upk_mbar_gram(st.s, &S, &X, denom.as<double>(), f_dev.as<double>(), P.n_extra, extra.as<double>(), G.as<double>(), colsum.as<double>(),
                         work.p, work_bytes), "Gram pass");
    if (P.G) hip_ok(hipMemcpyAsync(P.G, G.p, (size_t)M * M * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of G");
    hip_ok(hipMemcpyAsync(P.colsum, colsum.p, M * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of colsum");
    if (P.denominators) hip_ok(hipMemcpyAsync(P.denominators, denom.p, N * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of D");
    hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
}

}  // namespace

extern "C" int upk_mbar_gram_solve(const upk_mbar_gram_problem_t* P, char* message, int message_len) {
    return guarded_entry("mbar_gram", message, message_len, [&] {
        if (!P) MBAR_REFUSE("mbar_gram: no problem given");
        gram_run(*P);
    });
}

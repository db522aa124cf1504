// gfx950 kernels and host drivers of the metadynamics analysis (upside_hip_metad_bias, upside_hip_metad_grid; include/upside_engine_c.h
// states the definitions): with the hills h of a list in deposit order, centres s_h, weights w_h, widths sigma and periods,
//     e_h(x) = exp(-1/2 sum_c wrap_c(x_c - s_hc)^2 / sigma_c^2),   V_m(x) = sum_{h < m} w_h e_h(x),
// the bias V_{n_visible}(x) at points, the bias on a product grid at the last of a list of checkpoints, and at every checkpoint the
// log-sum-exps ln sum_g exp(scale V(g)) that the reweighting offset c(t) is made of.  Everything is fp64, there are no atomics, and
// every sum has ONE order, ascending in hills.
//   - met_accumulate: the direct sum.  A lane owns a point and walks the hills, staged by the workgroup in LDS tiles of 256 (centres
//     and weight widened to double: broadcast reads), as far as the largest prefix among the workgroup's points.
//   - k_metad_bias: a workgroup per 256 consecutive points of one list.
//   - k_metad_grid_direct: the same over the grid points of a list, for the hills between two checkpoints, starting from V.
//   - the factorised sum, d >= 2 with at least UPK_METAD_MIN_FACTORISED rows and columns.  The grid is a matrix, rows = axis 0
//     (d = 2) or axes 0 x 1 (d = 3, 4), columns = the rest, and the hills between two checkpoints enter as V += A^T B with
//     A[h][row] = exp(-1/2 z^2 of the row dimensions), B[h][col] = w_h exp(-1/2 z^2 of the column dimensions): H (rows + cols)
//     exponentials instead of H rows cols.  A and B are made in SLABS of Rs hills (k_metad_panel: a lane per hill, a workgroup per
//     256 hills and 16 rows or columns; column-major, At[row][r], so that lanes store coalesced and a tile load reads 256-byte runs)
//     and each slab is folded into V before the next is made.
//   - k_metad_tile: one workgroup (4 waves) owns one 64 x 64 tile of V of one list for the slab.  As k_mbar_gram_tile: chunks of 32
//     hills, the two panels through LDS at a stride of 34 doubles per row, each wave a 32 x 32 quarter as 2 x 2 accumulators of
//     v_mfma_f64_16x16x4_f64 (A: lane l holds row l & 15, k = l >> 4; B: column l & 15, k = l >> 4; D: column l & 15, row (l >> 4) +
//     4 reg).  The accumulators start from V and return to it: every element is summed by one lane, ascending in hills.  Where a grid
//     has fewer than 256 tiles, the n_chunk chunks of a slab are cut into min(P, n_chunk) ranges, P = met_parts(rows, cols);
//     workgroup (tile, p) sums range p into a partial matrix of its own and k_metad_reduce adds the partials to V in ascending p (a
//     slab of one chunk, or P = 1, goes straight into V).  Rs and P depend on the grid's shape alone, a list's slabs and their cut on
//     its own checkpoints alone: a list's bits depend on nothing else in the call.  What is ALLOCATED per list (the stride of a slab in
//     the panels, the number of partial matrices) follows the longest segment of the call, so that many lists with short segments
//     share a chunk; that moves addresses, not arithmetic.
//   - k_metad_lse_range / _sum / _finish: per list the largest and smallest V over pieces of 16384 grid points, then
//     sum_g exp(scale V(g) - M) per piece with M = scale x (largest V for scale > 0, else smallest V) -- rounding is monotone, so this
//     is the exact maximum of the rounded products -- then the pieces ascending and M + log(sum).
// Lists are processed in chunks whose workspace stays below UPK_METAD_WORKSPACE; a chunk's launches index the lists of the chunk, and
// nothing a list computes depends on the chunk.  upk_metad_bias_solve and upk_metad_grid_solve are the host sides: every refusal
// returns before any device call.
#include "mbar_device.h"
#include <chrono>

using namespace up;
using namespace up::mbar;

#define MET_BLOCK CV_BLOCK
#define MET_HILL_TILE 256
#define MET_TILE 64
#define MET_CHUNK 32
#define MET_LDS_STRIDE (MET_CHUNK + 2)
#define MET_PANEL_ROWS 16
#define MET_PIECE 16384
#define MET_MAX_SLAB 2048
#define MET_PANEL_BYTES ((size_t)16 << 20)
static_assert(MET_BLOCK == 256 && MET_TILE == 64 && MET_CHUNK == 32, "k_metad_tile is written for 4 waves, 64 x 64 tiles and chunks of 32 hills");
static_assert(UPK_METAD_MAX_SCALES <= CV_MAX_SUMS, "block_sum holds CV_MAX_SUMS totals");
static_assert(MET_TILE % MET_PANEL_ROWS == 0 && MET_MAX_SLAB % MET_CHUNK == 0, "a panel workgroup lies in A or in B; a slab is whole chunks");

namespace {

typedef double met_acc_t __attribute__((ext_vector_type(4)));

// the hills of all lists on the device
struct MetadDev {
    double inv_sigma[UPK_METAD_MAX_DIM], period[UPK_METAD_MAX_DIM];
    const long long* hill_start;      // [n_list + 1]
    const float* centers;             // [hills][d]
    const float* weights;             // [hills]
};

// the grid and the checkpoints on the device
struct MetadGridDev {
    int n_axis[UPK_METAD_MAX_DIM], axis_off[UPK_METAD_MAX_DIM];
    int G, rows, cols, n_checkpoint;
    const double* axes;               // concatenated
    const long long* checkpoints;     // [n_list][n_checkpoint]
};

// ((x - s) wrapped to the nearest image / sigma)^2 in dimension c
__device__ __forceinline__ double met_z2(const MetadDev& M, int c, double x, double s) {
    double dx = x - s;
    const double P = M.period[c];
    if (P > 0.) dx = dx - P * rint(dx / P);
    const double z = dx * M.inv_sigma[c];
    return z * z;
}

// acc + the hills first .. first + n_mine - 1, ascending, at the point x of this lane; n_max >= n_mine is the same for the whole workgroup
template <int D>
__device__ __forceinline__ double met_accumulate(const MetadDev& M, long long first, int n_max, int n_mine, const double (&x)[D], double acc,
                                                 double* __restrict__ tile) {
    const int tid = threadIdx.x;
    for (int k0 = 0; k0 < n_max; k0 += MET_HILL_TILE) {
        const int nt = min(MET_HILL_TILE, n_max - k0);
        __syncthreads();      // (the previous tile has been read)
        for (int i = tid; i < nt * (D + 1); i += MET_BLOCK) {
            const int l = i / (D + 1), j = i - l * (D + 1);
            const size_t h = (size_t)(first + k0 + l);
            tile[i] = j < D ? (double)M.centers[h * D + j] : (double)M.weights[h];
        }
        __syncthreads();
        const int lim = min(nt, n_mine - k0);
        for (int l = 0; l < lim; ++l) {
            const double* __restrict__ st = tile + l * (D + 1);
            double q = 0.;
#pragma unroll
            for (int c = 0; c < D; ++c) q += met_z2(M, c, x[c], st[c]);
            acc += st[D] * exp(-0.5 * q);
        }
    }
    return acc;
}

// grid: the blocks of 256 consecutive points of one list, numbered by the host (block_list, block_first)
template <int D>
__global__ void __launch_bounds__(MET_BLOCK) k_metad_bias(MetadDev M, const int* __restrict__ block_list, const long long* __restrict__ block_first,
                                                           const long long* __restrict__ point_start, const double* __restrict__ points,
                                                           const long long* __restrict__ n_visible, double* __restrict__ V) {
    __shared__ double tile[MET_HILL_TILE * (D + 1)];
    __shared__ int wave_max[CV_WAVES];
    const int l = block_list[blockIdx.x], tid = threadIdx.x;
    const long long p_end = point_start[l + 1], p_raw = block_first[blockIdx.x] + tid;
    const bool live = p_raw < p_end;
    const long long p = live ? p_raw : p_end - 1;      // (a lane past the end repeats the last point, sums nothing and stores nothing)
    const long long h0 = M.hill_start[l];
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = points[(size_t)p * D + c];
    const int m = live ? (n_visible ? (int)n_visible[p] : (int)(M.hill_start[l + 1] - h0)) : 0;
    int w = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w = max(w, __shfl_xor(w, o, 64));
    if ((tid & 63) == 0) wave_max[tid >> 6] = w;
    __syncthreads();
    int n_max = wave_max[0];
#pragma unroll
    for (int i = 1; i < CV_WAVES; ++i) n_max = max(n_max, wave_max[i]);
    const double v = met_accumulate<D>(M, h0, n_max, m, x, 0., tile);
    if (live) V[p_raw] = v;
}

// the hills of list l between checkpoint j - 1 (0 for j = 0) and checkpoint j: the first, counted within the list, and their number
__device__ __forceinline__ void met_segment(const MetadGridDev& Gd, int l, int j, long long& first, long long& n) {
    const long long* __restrict__ ck = Gd.checkpoints + (size_t)l * Gd.n_checkpoint;
    first = j ? ck[j - 1] : 0;
    n = ck[j] - first;
}
// of that segment, slab `slab` of at most Rs hills
__device__ __forceinline__ int met_slab(const MetadGridDev& Gd, int l, int j, int slab, int Rs, long long& first) {
    long long n;
    met_segment(Gd, l, j, first, n);
    first += (long long)slab * Rs;
    n -= (long long)slab * Rs;
    return (int)(n < Rs ? (n > 0 ? n : 0) : Rs);
}

// grid: list of the chunk x blocks of 256 grid points.  V[list of the chunk][G] += the hills of the list's segment j
template <int D>
__global__ void __launch_bounds__(MET_BLOCK) k_metad_grid_direct(MetadDev M, MetadGridDev Gd, int l0, int j, double* __restrict__ V) {
    __shared__ double tile[MET_HILL_TILE * (D + 1)];
    const int n_gb = (Gd.G + MET_BLOCK - 1) / MET_BLOCK;
    const int ll = blockIdx.x / n_gb, gb = blockIdx.x - ll * n_gb, l = l0 + ll;
    long long first, n;
    met_segment(Gd, l, j, first, n);
    if (n <= 0) return;
    const int g_raw = gb * MET_BLOCK + threadIdx.x;
    const bool live = g_raw < Gd.G;
    const int g = live ? g_raw : Gd.G - 1;
    double x[D];
    int rest = g;
#pragma unroll
    for (int c = D - 1; c >= 0; --c) { const int i = rest % Gd.n_axis[c]; rest /= Gd.n_axis[c]; x[c] = Gd.axes[Gd.axis_off[c] + i]; }
    double* __restrict__ out = V + (size_t)ll * Gd.G;
    const double v = met_accumulate<D>(M, M.hill_start[l] + first, (int)n, (int)n, x, out[g], tile);
    if (live) out[g] = v;
}

// grid (list of the chunk x blocks of 256 hills of the slab, 16 panel rows: first the Rp rows of A, then the Cp rows of B).  Rows past
// the grid's and hills past the slab's (up to the next whole chunk) are written as 0
template <int D>
__global__ void __launch_bounds__(MET_BLOCK) k_metad_panel(MetadDev M, MetadGridDev Gd, int l0, int j, int slab, int Rs, int ldp, int Rp, int Cp,
                                                            size_t per_list, double* __restrict__ panel) {
    constexpr int NR = D == 2 ? 1 : 2;      // the dimensions of a row; the other D - NR are a column's
    const int n_hb = (ldp + MET_BLOCK - 1) / MET_BLOCK;
    const int ll = blockIdx.x / n_hb, hb = blockIdx.x - ll * n_hb, l = l0 + ll;
    long long first;
    const int n = met_slab(Gd, l, j, slab, Rs, first);
    if (n <= 0) return;
    const int rows_pad = (n + MET_CHUNK - 1) / MET_CHUNK * MET_CHUNK;
    const int r = hb * MET_BLOCK + threadIdx.x;
    if (r >= rows_pad) return;
    const bool live = r < n;
    const size_t h = (size_t)(M.hill_start[l] + first + (live ? r : 0));
    double s[D];
#pragma unroll
    for (int c = 0; c < D; ++c) s[c] = (double)M.centers[h * D + c];
    const double w = (double)M.weights[h];
    double* __restrict__ At = panel + (size_t)ll * per_list;
    double* __restrict__ Bt = At + (size_t)Rp * ldp;
#pragma unroll 4
    for (int q = 0; q < MET_PANEL_ROWS; ++q) {
        const int rho = blockIdx.y * MET_PANEL_ROWS + q;
        if (rho < Rp) {
            double v = 0.;
            if (live && rho < Gd.rows) {
                double z;
                if constexpr (NR == 1) z = met_z2(M, 0, Gd.axes[rho], s[0]);
                else {
                    const int i0 = rho / Gd.n_axis[1], i1 = rho - i0 * Gd.n_axis[1];
                    z = met_z2(M, 0, Gd.axes[i0], s[0]) + met_z2(M, 1, Gd.axes[Gd.axis_off[1] + i1], s[1]);
                }
                v = exp(-0.5 * z);
            }
            At[(size_t)rho * ldp + r] = v;
        } else {
            const int kap = rho - Rp;
            double v = 0.;
            if (live && kap < Gd.cols) {
                double z;
                if constexpr (D - NR == 1) z = met_z2(M, D - 1, Gd.axes[Gd.axis_off[D - 1] + kap], s[D - 1]);
                else {
                    const int i2 = kap / Gd.n_axis[3], i3 = kap - i2 * Gd.n_axis[3];
                    z = met_z2(M, 2, Gd.axes[Gd.axis_off[2] + i2], s[2 < D ? 2 : 0]) + met_z2(M, 3, Gd.axes[Gd.axis_off[3] + i3], s[3 < D ? 3 : 0]);
                }
                v = w * exp(-0.5 * z);
            }
            Bt[(size_t)kap * ldp + r] = v;
        }
    }
}

// grid (list of the chunk x tiles, part).  A slab of n_chunk chunks is cut into parts = min(n_part, n_chunk) ranges (its own length
// decides, nothing else in the call).  parts == 1: the accumulators start from V and return to it.  parts > 1: part p sums its range
// of chunks from 0 into partial[list][p] (Rp x Cp; part_alloc of them are allocated per list)
__global__ void __launch_bounds__(MET_BLOCK) k_metad_tile(MetadGridDev Gd, int l0, int j, int slab, int Rs, int ldp, int Rp, int Cp, int n_part, int part_alloc, size_t per_list,
                                                           const double* __restrict__ panel, double* __restrict__ V, double* __restrict__ partial) {
    __shared__ double As[MET_TILE * MET_LDS_STRIDE];
    __shared__ double Bs[MET_TILE * MET_LDS_STRIDE];
    const int n_tc = Cp / MET_TILE, n_tile = (Rp / MET_TILE) * n_tc;
    const int ll = blockIdx.x / n_tile, t = blockIdx.x - ll * n_tile, tr = t / n_tc, tc = t - tr * n_tc, l = l0 + ll, p = blockIdx.y;
    long long first;
    const int n = met_slab(Gd, l, j, slab, Rs, first);
    if (n <= 0) return;
    const int n_chunk = (n + MET_CHUNK - 1) / MET_CHUNK;
    const int parts = n_part < n_chunk ? n_part : n_chunk;
    if (p >= parts) return;
    const int c_begin = p * n_chunk / parts, c_end = (p + 1) * n_chunk / parts;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const int li = lane & 15, lk = lane >> 4;
    const double* __restrict__ At = panel + (size_t)ll * per_list;
    const double* __restrict__ Bt = At + (size_t)Rp * ldp;
    const bool direct = parts == 1;
    double* __restrict__ C = direct ? V + (size_t)ll * Gd.G : partial + ((size_t)ll * part_alloc + p) * Rp * Cp;
    const int row_lim = direct ? Gd.rows : Rp, col_lim = direct ? Gd.cols : Cp, ld = col_lim;

    met_acc_t acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = tr * MET_TILE + wr + a * 16 + lk + 4 * q, col = tc * MET_TILE + wc + b * 16 + li;
                acc[a][b][q] = (direct && row < row_lim && col < col_lim) ? C[(size_t)row * ld + col] : 0.;
            }

    for (int c = c_begin; c < c_end; ++c) {
        __syncthreads();      // (the previous chunk has been read)
#pragma unroll
        for (int i = 0; i < MET_TILE * MET_CHUNK / MET_BLOCK; ++i) {
            const int e = tid + i * MET_BLOCK, col = e / MET_CHUNK, r = e - col * MET_CHUNK;
            As[col * MET_LDS_STRIDE + r] = At[(size_t)(tr * MET_TILE + col) * ldp + (size_t)c * MET_CHUNK + r];
            Bs[col * MET_LDS_STRIDE + r] = Bt[(size_t)(tc * MET_TILE + col) * ldp + (size_t)c * MET_CHUNK + r];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MET_CHUNK; kk += 4) {
            const double a0 = As[(wr + li) * MET_LDS_STRIDE + kk + lk], a1 = As[(wr + 16 + li) * MET_LDS_STRIDE + kk + lk];
            const double b0 = Bs[(wc + li) * MET_LDS_STRIDE + kk + lk], b1 = Bs[(wc + 16 + li) * MET_LDS_STRIDE + kk + lk];
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
                const int row = tr * MET_TILE + wr + a * 16 + lk + 4 * q, col = tc * MET_TILE + wc + b * 16 + li;
                if (row < row_lim && col < col_lim) C[(size_t)row * ld + col] = acc[a][b][q];
            }
}

// grid: list of the chunk x blocks of 256 grid points.  V = (((V + partial[0]) + partial[1]) + ...) over the parts of the list's slab `slab`,
// where it has one and that was cut
__global__ void __launch_bounds__(MET_BLOCK) k_metad_reduce(MetadGridDev Gd, int l0, int j, int slab, int Rs, int Rp, int Cp, int n_part, int part_alloc,
                                                             const double* __restrict__ partial, double* __restrict__ V) {
    const int n_gb = (Gd.G + MET_BLOCK - 1) / MET_BLOCK;
    const int ll = blockIdx.x / n_gb, gb = blockIdx.x - ll * n_gb;
    long long first;
    const int n_chunk = (met_slab(Gd, l0 + ll, j, slab, Rs, first) + MET_CHUNK - 1) / MET_CHUNK;
    const int parts = n_part < n_chunk ? n_part : n_chunk;
    if (parts <= 1) return;
    const int g = gb * MET_BLOCK + threadIdx.x;
    if (g >= Gd.G) return;
    const int row = g / Gd.cols, col = g - row * Gd.cols;
    double s = V[(size_t)ll * Gd.G + g];
    for (int p = 0; p < parts; ++p) s += partial[(((size_t)ll * part_alloc + p) * Rp + row) * Cp + col];
    V[(size_t)ll * Gd.G + g] = s;
}

// grid: list of the chunk x pieces.  range[list][piece] = (largest V, smallest V) of the piece
__global__ void __launch_bounds__(MET_BLOCK) k_metad_lse_range(int G, int n_piece, const double* __restrict__ V, double* __restrict__ range) {
    __shared__ double part[CV_WAVES][2];
    const int ll = blockIdx.x / n_piece, piece = blockIdx.x - ll * n_piece, tid = threadIdx.x;
    const double* __restrict__ v = V + (size_t)ll * G;
    const int g_end = min(G, (piece + 1) * MET_PIECE);
    double hi = -INFINITY, lo = INFINITY;
    for (int g = piece * MET_PIECE + tid; g < g_end; g += MET_BLOCK) { hi = fmax(hi, v[g]); lo = fmin(lo, v[g]); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { hi = fmax(hi, __shfl_xor(hi, o, 64)); lo = fmin(lo, __shfl_xor(lo, o, 64)); }
    if ((tid & 63) == 0) { part[tid >> 6][0] = hi; part[tid >> 6][1] = lo; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < CV_WAVES; ++w) { hi = fmax(hi, part[w][0]); lo = fmin(lo, part[w][1]); }
        range[2 * (size_t)blockIdx.x] = hi; range[2 * (size_t)blockIdx.x + 1] = lo;
    }
}

struct MetadScales { int n; double s[UPK_METAD_MAX_SCALES]; };

// the largest of scale V(g) over the list's grid: the rounded product is monotone in V
__device__ __forceinline__ void met_lse_maxima(const MetadScales& Sc, int n_piece, const double* __restrict__ range, double (&m)[UPK_METAD_MAX_SCALES]) {
    double hi = range[0], lo = range[1];
    for (int p = 1; p < n_piece; ++p) { hi = fmax(hi, range[2 * p]); lo = fmin(lo, range[2 * p + 1]); }
#pragma unroll
    for (int q = 0; q < UPK_METAD_MAX_SCALES; ++q) m[q] = q < Sc.n ? Sc.s[q] * (Sc.s[q] > 0. ? hi : lo) : 0.;
}
// scale v - m, each operation rounded on its own: the largest term is exactly 0
__device__ __forceinline__ double met_lse_term(double scale, double v, double m) {
#pragma clang fp contract(off)
    const double u = scale * v;
    return u - m;
}

// grid: list of the chunk x pieces.  psum[list][piece][q] = sum over the piece of exp(scale_q V - M_q); lane t adds t, t + 256, ...
__global__ void __launch_bounds__(MET_BLOCK) k_metad_lse_sum(int G, int n_piece, MetadScales Sc, const double* __restrict__ V, const double* __restrict__ range,
                                                              double* __restrict__ psum) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    const int ll = blockIdx.x / n_piece, piece = blockIdx.x - ll * n_piece, tid = threadIdx.x;
    const double* __restrict__ v = V + (size_t)ll * G;
    double m[UPK_METAD_MAX_SCALES], s[UPK_METAD_MAX_SCALES];
    met_lse_maxima(Sc, n_piece, range + 2 * (size_t)ll * n_piece, m);
#pragma unroll
    for (int q = 0; q < UPK_METAD_MAX_SCALES; ++q) s[q] = 0.;
    const int g_end = min(G, (piece + 1) * MET_PIECE);
    for (int g = piece * MET_PIECE + tid; g < g_end; g += MET_BLOCK) {
        const double x = v[g];
#pragma unroll
        for (int q = 0; q < UPK_METAD_MAX_SCALES; ++q) if (q < Sc.n) s[q] += exp(met_lse_term(Sc.s[q], x, m[q]));
    }
    block_sum<UPK_METAD_MAX_SCALES>(s, part);
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < UPK_METAD_MAX_SCALES; ++q) psum[(size_t)blockIdx.x * UPK_METAD_MAX_SCALES + q] = s[q];
    }
}

// a lane per (list of the chunk, scale): the pieces ascending, then lse[l0 + list][j][q] = M + log(sum)
__global__ void __launch_bounds__(MET_BLOCK) k_metad_lse_finish(int n_lists, int l0, int j, int n_checkpoint, int n_piece, MetadScales Sc,
                                                                 const double* __restrict__ range, const double* __restrict__ psum, double* __restrict__ lse) {
    const int i = blockIdx.x * MET_BLOCK + threadIdx.x;
    const int ll = i / UPK_METAD_MAX_SCALES, q = i - ll * UPK_METAD_MAX_SCALES;
    if (ll >= n_lists || q >= Sc.n) return;
    double m[UPK_METAD_MAX_SCALES];
    met_lse_maxima(Sc, n_piece, range + 2 * (size_t)ll * n_piece, m);
    double mq = 0., sum = 0.;
#pragma unroll
    for (int k = 0; k < UPK_METAD_MAX_SCALES; ++k) if (k == q) mq = m[k];
    for (int p = 0; p < n_piece; ++p) sum += psum[((size_t)ll * n_piece + p) * UPK_METAD_MAX_SCALES + q];
    lse[((size_t)(l0 + ll) * n_checkpoint + j) * Sc.n + q] = mq + log(sum);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

inline int met_padded(int n) { return (n + MET_TILE - 1) / MET_TILE * MET_TILE; }
// the hills of a slab: as many as keep both panels of a list within MET_PANEL_BYTES, whole chunks, 32 .. 2048: a function of the shape
inline int met_slab_hills(int rows, int cols) {
    const size_t fit = MET_PANEL_BYTES / (((size_t)met_padded(rows) + met_padded(cols)) * sizeof(double)) / MET_CHUNK * MET_CHUNK;
    return (int)(fit < MET_CHUNK ? MET_CHUNK : fit > MET_MAX_SLAB ? MET_MAX_SLAB : fit);
}
// the ranges a slab's chunks are cut into: 1 where the grid has 256 tiles or more, else enough for about 512 workgroups per list, at
// most 16 and at most the chunks of a full slab
inline int met_parts(int rows, int cols) {
    const int n_tile = (met_padded(rows) / MET_TILE) * (met_padded(cols) / MET_TILE), most = met_slab_hills(rows, cols) / MET_CHUNK;
    if (n_tile >= 256) return 1;
    const int want = 512 / n_tile < 16 ? 512 / n_tile : 16;
    return want < most ? want : most;
}

// the refusals the two entry points share; the guarded entry replaces "mbar:" by the entry point's name.  total: the hills of all lists
void metad_check_hills(const upk_metad_hills_t& H, long long& total) {
    if (H.d < 1 || H.d > UPK_METAD_MAX_DIM) MBAR_REFUSE("mbar: d = %d, 1 to %d collective variables are supported", H.d, UPK_METAD_MAX_DIM);
    if (H.n_list < 1) MBAR_REFUSE("mbar: n_list = %d, at least one list is needed", H.n_list);
    if (!H.hill_start || !H.centers || !H.weights || !H.sigma || !H.periods) MBAR_REFUSE("mbar: hill_start, centers, weights, sigma and periods must be given");
    if (H.hill_start[0] != 0) MBAR_REFUSE("mbar: hill_start[0] = %lld, the first list starts at 0", H.hill_start[0]);
    for (int l = 0; l < H.n_list; ++l) {
        const long long n = H.hill_start[l + 1] - H.hill_start[l];
        if (n < 0) MBAR_REFUSE("mbar: hill_start[%d] = %lld descends (hill_start[%d] = %lld)", l + 1, H.hill_start[l + 1], l, H.hill_start[l]);
        if (n > UPK_METAD_MAX_LIST) MBAR_REFUSE("mbar: hill_start: list %d holds %lld hills, at most 2^24 are supported", l, n);
        if (H.hill_start[l + 1] >= (1ll << 31)) MBAR_REFUSE("mbar: hill_start: %lld hills up to list %d, fewer than 2^31 in total are supported", H.hill_start[l + 1], l);
    }
    total = H.hill_start[H.n_list];
    const size_t d = (size_t)H.d;
    size_t at = 0;
    for (size_t c = 0; c < d; ++c) {
        if (!std::isfinite(H.sigma[c])) MBAR_REFUSE("mbar: sigma[%zu] is not finite", c);
        if (!(H.sigma[c] > 0.)) MBAR_REFUSE("mbar: sigma[%zu] = %g is not positive", c, H.sigma[c]);
        if (!std::isfinite(H.periods[c])) MBAR_REFUSE("mbar: periods[%zu] is not finite", c);
        if (H.periods[c] < 0.) MBAR_REFUSE("mbar: periods[%zu] is negative (0 = not periodic)", c);
    }
    if (!all_finite(H.centers, (size_t)total * d, &at)) MBAR_REFUSE("mbar: centers: hill %zu, CV %zu is not finite", at / d, at % d);
    if (!all_finite(H.weights, (size_t)total, &at)) MBAR_REFUSE("mbar: weights[%zu] is not finite", at);
}

// the hills on the device, once, and the stream of the solve
struct StagedHills {
    Stream st;
    DeviceBuffer start, centers, weights;
    MetadDev M{};
    StagedHills(const upk_metad_hills_t& H, long long total) {
        require_device();
        hip_ok(hipStreamCreate(&st.s), "hipStreamCreate");
        start.upload(st.s, H.hill_start, ((size_t)H.n_list + 1) * sizeof(long long), "copy of hill_start");
        centers.upload(st.s, H.centers, (size_t)total * H.d * sizeof(float), "copy of centers");
        weights.upload(st.s, H.weights, (size_t)total * sizeof(float), "copy of weights");
        for (int c = 0; c < H.d; ++c) { M.inv_sigma[c] = 1. / H.sigma[c]; M.period[c] = H.periods[c]; }
        M.hill_start = start.as<long long>(); M.centers = centers.as<float>(); M.weights = weights.as<float>();
    }
};

struct Event {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

#define METAD_DISPATCH(KERNEL, D, GRID, STREAM, ...)                                                                       \
    switch (D) {                                                                                                           \
    case 1: hipLaunchKernelGGL(KERNEL<1>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                           \
    case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                           \
    case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                           \
    default: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                          \
    }
#define METAD_DISPATCH_FACTORISED(KERNEL, D, GRID, STREAM, ...)                                                            \
    switch (D) {                                                                                                           \
    case 2: hipLaunchKernelGGL(KERNEL<2>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                           \
    case 3: hipLaunchKernelGGL(KERNEL<3>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                           \
    default: hipLaunchKernelGGL(KERNEL<4>, GRID, dim3(MET_BLOCK), 0, STREAM, __VA_ARGS__); break;                          \
    }
static_assert(UPK_METAD_MAX_DIM == 4, "METAD_DISPATCH lists d = 1 .. 4");

// every refusal of upside_hip_metad_bias; nothing here touches the device
void bias_check(const upk_metad_bias_problem_t& P, long long& n_hill, long long& n_point) {
    const upk_metad_hills_t& H = P.H;
    metad_check_hills(H, n_hill);
    if (!P.point_start || !P.points || !P.V) MBAR_REFUSE("metad_bias: point_start, points and V must be given");
    if (P.point_start[0] != 0) MBAR_REFUSE("metad_bias: point_start[0] = %lld, the first list starts at 0", P.point_start[0]);
    for (int l = 0; l < H.n_list; ++l) {
        if (P.point_start[l + 1] < P.point_start[l])
            MBAR_REFUSE("metad_bias: point_start[%d] = %lld descends (point_start[%d] = %lld)", l + 1, P.point_start[l + 1], l, P.point_start[l]);
        if (P.point_start[l + 1] >= (1ll << 31)) MBAR_REFUSE("metad_bias: point_start: %lld points up to list %d, fewer than 2^31 are supported", P.point_start[l + 1], l);
    }
    n_point = P.point_start[H.n_list];
    const size_t d = (size_t)H.d;
    size_t at = 0;
    if (!all_finite(P.points, (size_t)n_point * d, &at)) MBAR_REFUSE("metad_bias: points: point %zu, CV %zu is not finite", at / d, at % d);
    if (P.n_visible)
        for (int l = 0; l < H.n_list; ++l) {
            const long long n = H.hill_start[l + 1] - H.hill_start[l];
            for (long long i = P.point_start[l]; i < P.point_start[l + 1]; ++i)
                if (P.n_visible[i] < 0 || P.n_visible[i] > n) MBAR_REFUSE("metad_bias: n_visible[%lld] = %lld, list %d holds %lld hills", i, P.n_visible[i], l, n);
        }
}

void bias_run(const upk_metad_bias_problem_t& P) {
    long long n_hill = 0, n_point = 0;
    bias_check(P, n_hill, n_point);
    const upk_metad_hills_t& H = P.H;
    StagedHills staged(H, n_hill);
    Stream& st = staged.st;
    const auto wall0 = std::chrono::steady_clock::now();
    std::vector<int> block_list; std::vector<long long> block_first;
    double n_exp = 0.;
    for (int l = 0; l < H.n_list; ++l)
        for (long long p = P.point_start[l]; p < P.point_start[l + 1]; p += MET_BLOCK) { block_list.push_back(l); block_first.push_back(p); }
    if (P.stats)
        for (int l = 0; l < H.n_list; ++l)
            for (long long p = P.point_start[l]; p < P.point_start[l + 1]; ++p) n_exp += P.n_visible ? (double)P.n_visible[p] : (double)(H.hill_start[l + 1] - H.hill_start[l]);
    Event ev0, ev1;
    hip_ok(hipEventCreate(&ev0.e), "hipEventCreate"); hip_ok(hipEventCreate(&ev1.e), "hipEventCreate");
    DeviceBuffer pstart, points, visible, blist, bfirst, V;
    pstart.upload(st.s, P.point_start, ((size_t)H.n_list + 1) * sizeof(long long), "copy of point_start");
    points.upload(st.s, P.points, (size_t)n_point * H.d * sizeof(double), "copy of points");
    if (P.n_visible) visible.upload(st.s, P.n_visible, (size_t)n_point * sizeof(long long), "copy of n_visible");
    blist.upload(st.s, block_list.data(), block_list.size() * sizeof(int), "copy of the blocks");
    bfirst.upload(st.s, block_first.data(), block_first.size() * sizeof(long long), "copy of the blocks");
    V.alloc((size_t)n_point * sizeof(double), "V");
    hip_ok(hipEventRecord(ev0.e, st.s), "hipEventRecord");
    if (!block_list.empty()) {
        METAD_DISPATCH(k_metad_bias, H.d, dim3((unsigned)block_list.size()), st.s, staged.M, blist.as<int>(), bfirst.as<long long>(), pstart.as<long long>(),
                       points.as<double>(), P.n_visible ? visible.as<long long>() : (const long long*)nullptr, V.as<double>())
        upk_ok(launch_status(), "bias");
    }
    hip_ok(hipEventRecord(ev1.e, st.s), "hipEventRecord");
    if (n_point) hip_ok(hipMemcpyAsync(P.V, V.p, (size_t)n_point * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of V");
    hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
    if (P.stats) {
        float ms = 0.f;
        hip_ok(hipEventElapsedTime(&ms, ev0.e, ev1.e), "hipEventElapsedTime");
        P.stats[0] = ms; P.stats[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        P.stats[2] = n_exp; P.stats[3] = 0.; P.stats[4] = 1.; P.stats[5] = 1.;
    }
}

// every refusal of upside_hip_metad_grid; nothing here touches the device
void grid_check(const upk_metad_grid_problem_t& P, long long& n_hill, long long& G) {
    const upk_metad_hills_t& H = P.H;
    metad_check_hills(H, n_hill);
    if (!P.n_axis || !P.axes || !P.checkpoints) MBAR_REFUSE("metad_grid: n_axis, axes and checkpoints must be given");
    if (P.n_checkpoint < 1) MBAR_REFUSE("metad_grid: n_checkpoint = %d, at least one checkpoint is needed", P.n_checkpoint);
    if ((long long)H.n_list * P.n_checkpoint >= (1ll << 31)) MBAR_REFUSE("metad_grid: n_list x n_checkpoint = %d x %d is not below 2^31", H.n_list, P.n_checkpoint);
    if (P.n_scale < 0 || P.n_scale > UPK_METAD_MAX_SCALES) MBAR_REFUSE("metad_grid: n_scale = %d, 0 to %d scales are supported", P.n_scale, UPK_METAD_MAX_SCALES);
    if (P.n_scale > 0 && !P.scales) MBAR_REFUSE("metad_grid: scales must be given when n_scale > 0");
    if ((P.n_scale > 0) != (P.lse != nullptr)) MBAR_REFUSE("metad_grid: lse must be given exactly when n_scale > 0 (n_scale = %d)", P.n_scale);
    if (P.path < 0 || P.path > 2 || (P.path == 2 && H.d < 2)) MBAR_REFUSE("metad_grid: path = %d with d = %d (0: by shape, 1: direct, 2: factorised, d >= 2)", P.path, H.d);
    G = 1;
    long long n_value = 0;
    for (int c = 0; c < H.d; ++c) {
        if (P.n_axis[c] < 1) MBAR_REFUSE("metad_grid: n_axis[%d] = %d, an axis holds at least one value", c, P.n_axis[c]);
        n_value += P.n_axis[c];
        G *= P.n_axis[c];
        if (G > UPK_METAD_MAX_GRID) MBAR_REFUSE("metad_grid: n_axis: the grid holds more than 2^22 points (%lld up to axis %d)", G, c);
    }
    size_t at = 0;
    if (!all_finite(P.axes, (size_t)n_value, &at)) MBAR_REFUSE("metad_grid: axes[%zu] is not finite", at);
    if (P.n_scale > 0 && !all_finite(P.scales, (size_t)P.n_scale, &at)) MBAR_REFUSE("metad_grid: scales[%zu] is not finite", at);
    for (int l = 0; l < H.n_list; ++l) {
        const long long n = H.hill_start[l + 1] - H.hill_start[l];
        const long long* ck = P.checkpoints + (size_t)l * P.n_checkpoint;
        for (int j = 0; j < P.n_checkpoint; ++j) {
            if (ck[j] < 0 || ck[j] > n) MBAR_REFUSE("metad_grid: checkpoints: checkpoint %d of list %d = %lld, the list holds %lld hills", j, l, ck[j], n);
            if (j && ck[j] < ck[j - 1]) MBAR_REFUSE("metad_grid: checkpoints: checkpoint %d of list %d = %lld descends (the one before is %lld)", j, l, ck[j], ck[j - 1]);
        }
    }
}

void grid_run(const upk_metad_grid_problem_t& P) {
    long long n_hill = 0, G = 0;
    grid_check(P, n_hill, G);
    const upk_metad_hills_t& H = P.H;
    const int d = H.d, K = P.n_checkpoint, L = H.n_list;
    MetadGridDev Gd{};
    int n_value = 0;
    for (int c = 0; c < d; ++c) { Gd.n_axis[c] = P.n_axis[c]; Gd.axis_off[c] = n_value; n_value += P.n_axis[c]; }
    for (int c = d; c < UPK_METAD_MAX_DIM; ++c) { Gd.n_axis[c] = 1; Gd.axis_off[c] = 0; }
    const int n_row_dim = d == 2 ? 1 : 2;
    Gd.G = (int)G; Gd.rows = 1; Gd.n_checkpoint = K;
    for (int c = 0; c < n_row_dim && c < d; ++c) Gd.rows *= P.n_axis[c];
    Gd.cols = Gd.G / Gd.rows;
    const bool factorised = P.path == 2 || (P.path == 0 && d >= 2 && Gd.rows >= UPK_METAD_MIN_FACTORISED && Gd.cols >= UPK_METAD_MIN_FACTORISED);
    const int Rp = met_padded(Gd.rows), Cp = met_padded(Gd.cols), Rs = met_slab_hills(Gd.rows, Gd.cols), n_part = met_parts(Gd.rows, Gd.cols);
    const int n_tile = (Rp / MET_TILE) * (Cp / MET_TILE), n_piece = (int)((G + MET_PIECE - 1) / MET_PIECE), n_gb = (int)((G + MET_BLOCK - 1) / MET_BLOCK);
    if (factorised && (Rp + Cp) / MET_PANEL_ROWS > 65535) MBAR_REFUSE("metad_grid: path = 2: %d rows and %d columns are too many for the panels", Gd.rows, Gd.cols);
    // what is allocated follows the longest segment of the call (a slab's stride in the panels, the partial matrices of a list); what is
    // computed does not: slabs of Rs hills, cut by the slab's own length
    long long longest_any = 0;
    for (int l = 0; l < L; ++l)
        for (int j = 0; j < K; ++j) { const long long n = P.checkpoints[(size_t)l * K + j] - (j ? P.checkpoints[(size_t)l * K + j - 1] : 0); if (n > longest_any) longest_any = n; }
    const int ldp = (int)(longest_any >= Rs ? Rs : longest_any > 0 ? (longest_any + MET_CHUNK - 1) / MET_CHUNK * MET_CHUNK : MET_CHUNK);
    const int part_alloc = n_part < ldp / MET_CHUNK ? n_part : ldp / MET_CHUNK;
    const size_t panel_doubles = factorised ? ((size_t)Rp + Cp) * ldp : 0, partial_doubles = factorised && part_alloc > 1 ? (size_t)part_alloc * Rp * Cp : 0;
    const size_t lse_doubles = P.n_scale ? (size_t)n_piece * (2 + UPK_METAD_MAX_SCALES) : 0;
    const size_t per_list = ((size_t)G + panel_doubles + partial_doubles + lse_doubles) * sizeof(double);
    const size_t limit = P.workspace_limit && P.workspace_limit < UPK_METAD_WORKSPACE ? P.workspace_limit : UPK_METAD_WORKSPACE;
    const int chunk = (int)(limit / per_list < 1 ? 1 : limit / per_list < (size_t)L ? limit / per_list : (size_t)L);

    StagedHills staged(H, n_hill);
    Stream& st = staged.st;
    const auto wall0 = std::chrono::steady_clock::now();
    Event ev0, ev1;
    hip_ok(hipEventCreate(&ev0.e), "hipEventCreate"); hip_ok(hipEventCreate(&ev1.e), "hipEventCreate");
    DeviceBuffer axes, ckpt, V, panel, partial, range, psum, lse;
    axes.upload(st.s, P.axes, (size_t)n_value * sizeof(double), "copy of axes");
    ckpt.upload(st.s, P.checkpoints, (size_t)L * K * sizeof(long long), "copy of checkpoints");
    Gd.axes = axes.as<double>(); Gd.checkpoints = ckpt.as<long long>();
    V.alloc((size_t)chunk * G * sizeof(double), "V");
    if (factorised) panel.alloc((size_t)chunk * panel_doubles * sizeof(double), "panels");
    if (partial_doubles) partial.alloc((size_t)chunk * partial_doubles * sizeof(double), "partial sums");
    MetadScales Sc{};
    Sc.n = P.n_scale;
    for (int q = 0; q < P.n_scale; ++q) Sc.s[q] = P.scales[q];
    if (P.n_scale) {
        range.alloc((size_t)chunk * n_piece * 2 * sizeof(double), "workspace"); psum.alloc((size_t)chunk * n_piece * UPK_METAD_MAX_SCALES * sizeof(double), "workspace");
        lse.alloc((size_t)L * K * P.n_scale * sizeof(double), "lse");
    }

    double n_exp = 0., n_mfma = 0.; int n_chunks = 0;
    hip_ok(hipEventRecord(ev0.e, st.s), "hipEventRecord");
    for (int l0 = 0; l0 < L; l0 += chunk, ++n_chunks) {
        const int nl = L - l0 < chunk ? L - l0 : chunk;
        hip_ok(hipMemsetAsync(V.p, 0, (size_t)nl * G * sizeof(double), st.s), "hipMemsetAsync");
        for (int j = 0; j < K; ++j) {
            long long longest = 0;
            for (int l = l0; l < l0 + nl; ++l) {
                const long long* ck = P.checkpoints + (size_t)l * K;
                const long long n = ck[j] - (j ? ck[j - 1] : 0);
                if (n > longest) longest = n;
                if (P.stats && factorised) {
                    n_exp += (double)n * ((double)Gd.rows + Gd.cols);
                    for (long long r = 0; r < n; r += Rs) n_mfma += (double)n_tile * (double)(((n - r < Rs ? n - r : Rs) + MET_CHUNK - 1) / MET_CHUNK) * 128.;
                } else if (P.stats) n_exp += (double)n * (double)G;
            }
            if (longest > 0 && !factorised) {
                METAD_DISPATCH(k_metad_grid_direct, d, dim3((unsigned)((size_t)nl * n_gb)), st.s, staged.M, Gd, l0, j, V.as<double>())
            } else if (longest > 0) {
                for (int slab = 0; (long long)slab * Rs < longest; ++slab) {
                    const dim3 pgrid((unsigned)((size_t)nl * ((ldp + MET_BLOCK - 1) / MET_BLOCK)), (unsigned)((Rp + Cp) / MET_PANEL_ROWS));
                    METAD_DISPATCH_FACTORISED(k_metad_panel, d, pgrid, st.s, staged.M, Gd, l0, j, slab, Rs, ldp, Rp, Cp, panel_doubles, panel.as<double>())
                    hipLaunchKernelGGL(k_metad_tile, dim3((unsigned)((size_t)nl * n_tile), part_alloc), dim3(MET_BLOCK), 0, st.s, Gd, l0, j, slab, Rs, ldp, Rp, Cp, n_part,
                                       part_alloc, panel_doubles, panel.as<double>(), V.as<double>(), partial.as<double>());
                    if (part_alloc > 1)
                        hipLaunchKernelGGL(k_metad_reduce, dim3((unsigned)((size_t)nl * n_gb)), dim3(MET_BLOCK), 0, st.s, Gd, l0, j, slab, Rs, Rp, Cp, n_part, part_alloc,
                                           partial.as<double>(), V.as<double>());
                }
            }
            if (P.n_scale) {
                hipLaunchKernelGGL(k_metad_lse_range, dim3((unsigned)((size_t)nl * n_piece)), dim3(MET_BLOCK), 0, st.s, Gd.G, n_piece, V.as<double>(), range.as<double>());
                hipLaunchKernelGGL(k_metad_lse_sum, dim3((unsigned)((size_t)nl * n_piece)), dim3(MET_BLOCK), 0, st.s, Gd.G, n_piece, Sc, V.as<double>(), range.as<double>(),
                                   psum.as<double>());
                hipLaunchKernelGGL(k_metad_lse_finish, dim3((unsigned)(((size_t)nl * UPK_METAD_MAX_SCALES + MET_BLOCK - 1) / MET_BLOCK)), dim3(MET_BLOCK), 0, st.s, nl, l0, j, K,
                                   n_piece, Sc, range.as<double>(), psum.as<double>(), lse.as<double>());
            }
            upk_ok(launch_status(), "checkpoint");
        }
        if (P.V_last) hip_ok(hipMemcpyAsync(P.V_last + (size_t)l0 * G, V.p, (size_t)nl * G * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of V_last");
    }
    hip_ok(hipEventRecord(ev1.e, st.s), "hipEventRecord");
    if (P.n_scale) hip_ok(hipMemcpyAsync(P.lse, lse.p, (size_t)L * K * P.n_scale * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of lse");
    hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
    if (P.stats) {
        float ms = 0.f;
        hip_ok(hipEventElapsedTime(&ms, ev0.e, ev1.e), "hipEventElapsedTime");
        P.stats[0] = ms; P.stats[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        P.stats[2] = n_exp; P.stats[3] = n_mfma; P.stats[4] = factorised ? 2. : 1.; P.stats[5] = (double)n_chunks;
    }
}

}  // namespace

extern "C" int upk_metad_bias_solve(const upk_metad_bias_problem_t* P, char* message, int message_len) {
    return guarded_entry("metad_bias", message, message_len, [&] {
        if (!P) MBAR_REFUSE("metad_bias: no problem given");
        bias_run(*P);
    });
}
extern "C" int upk_metad_grid_solve(const upk_metad_grid_problem_t* P, char* message, int message_len) {
    return guarded_entry("metad_grid", message, message_len, [&] {
        if (!P) MBAR_REFUSE("metad_grid: no problem given");
        grid_run(*P);
    });
}

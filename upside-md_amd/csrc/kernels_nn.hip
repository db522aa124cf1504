// gfx950 kernels of the learned backbone potential (nn.cpp of the reference): backbone_featurizer, conv1d, scaled_sum.
// grid.y is the system index, as everywhere; one launch covers the batch.
//
// conv1d is a small dense contraction per output row (W * C_in terms for each of C_out channels).  A workgroup owns NN_TR rows of
// one system and a slice of the output channels: it stages that slice of the weights and the rows it reads (tile + W - 1 halo) in
// LDS once, then every lane produces whole outputs -- NN_RB rows x 2 adjacent channels, one packed fp32 fma per (row, term).
// The slice is cut over the OUTPUT channels of the pass (C_out forward, C_in backward) so that it fits: a 15 x 64 x 64 layer is
// 240 KB, its 8-channel slice 30 KB.
// Every value is ONE chain of fused multiply-adds in a fixed order (w ascending, then the contracted channel ascending; the
// weight gradient: rows ascending) that depends neither on the tiling, nor on the batch, nor on timing: no atomics anywhere.
// The backward pass is the same contraction with the roles swapped -- an input element gathers over the <= W output rows that read
// it -- and adds the finished sum into the parent's sens with one plain read-modify-write per element.
#include "device_math.h"
#include "../../include/upside_hip_kernels.h"
#include <cstring>

using namespace up;

#define ST(L) ((hipStream_t)(L)->stream)
#define C_OUT(c, s)  ((c).out  + (size_t)(s) * (c).n_elem * (c).stride)
#define C_SENS(c, s) ((c).sens + (size_t)(s) * (c).n_elem * (c).stride)
static inline int launch_status() { return (int)hipGetLastError(); }

#define NN_BLOCK 256
#define NN_TR 64                      // rows of a tile
#define NN_RB 4                       // rows per lane
#define NN_LDS_BUDGET (60 * 1024)     // bytes of dynamic LDS a workgroup may ask for
#define NN_PD_ROWS 32                 // rows per chunk of the weight-gradient kernel
#define NN_PD_PER_LANE 4              // table entries per lane there

typedef float v2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float nn_act(float x, int act) {
    return act == UPK_ACT_RELU ? fmaxf(x, 0.f) : act == UPK_ACT_TANH ? tanhf(x) : x;
}
// derivative of the activation from the stored OUTPUT (no pre-activation buffer)
__device__ __forceinline__ float nn_dact(float y, int act) {
    return act == UPK_ACT_RELU ? (y > 0.f ? 1.f : 0.f) : act == UPK_ACT_TANH ? 1.f - y * y : 1.f;
}

// ------------------------------------------------------------------------------------------------
// backbone_featurizer
__global__ void k_backbone_featurizer_fwd(upk_coord_t rama, upk_coord_t hbond, const int* __restrict__ rama_idx, const int* __restrict__ hbond_idx,
                                          upk_coord_t out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= out.n_elem) return;
    const int s = blockIdx.y;
    const float* a = C_OUT(rama, s) + (size_t)rama_idx[r] * rama.stride;
    const int d = hbond_idx[2 * r], c = hbond_idx[2 * r + 1];
    float* o = C_OUT(out, s) + (size_t)r * out.stride;
    o[0] = sinf(a[0]); o[1] = cosf(a[0]); o[2] = sinf(a[1]); o[3] = cosf(a[1]);
    o[4] = d < 0 ? 0.f : C_OUT(hbond, s)[(size_t)d * hbond.stride + 6];
    o[5] = c < 0 ? 0.f : C_OUT(hbond, s)[(size_t)c * hbond.stride + 6];
}
__global__ void k_backbone_featurizer_bwd(upk_coord_t rama, upk_coord_t hbond, const int* __restrict__ rama_idx, const int* __restrict__ hbond_idx,
                                          upk_coord_t self) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= self.n_elem) return;
    const int s = blockIdx.y;
    const float* o = C_OUT(self, s) + (size_t)r * self.stride;
    const float* g = C_SENS(self, s) + (size_t)r * self.stride;
    float* a = C_SENS(rama, s) + (size_t)rama_idx[r] * rama.stride;
    a[0] += g[0] * o[1] - g[1] * o[0];
    a[1] += g[2] * o[3] - g[3] * o[2];
    const int d = hbond_idx[2 * r], c = hbond_idx[2 * r + 1];
    if (d >= 0) C_SENS(hbond, s)[(size_t)d * hbond.stride + 6] += g[4];
    if (c >= 0) C_SENS(hbond, s)[(size_t)c * hbond.stride + 6] += g[5];
}
static inline dim3 nn_grid1(int n, int S) { return dim3((unsigned)(n > 0 ? (n + NN_BLOCK - 1) / NN_BLOCK : 1), (unsigned)S, 1); }
extern "C" int upk_backbone_featurizer_fwd(const upk_launch_t* L, upk_coord_t rama, upk_coord_t hbond, const int* rama_idx, const int* hbond_idx,
                                           upk_coord_t out) {
    UPK_FLUSH(L);
    if (out.width != 6 || rama.width < 2 || hbond.width < 7) return 9201;
    hipLaunchKernelGGL(k_backbone_featurizer_fwd, nn_grid1(out.n_elem, L->n_system), dim3(NN_BLOCK), 0, ST(L), rama, hbond, rama_idx, hbond_idx, out);
    return launch_status();
}
extern "C" int upk_backbone_featurizer_bwd(const upk_launch_t* L, upk_coord_t rama, upk_coord_t hbond, const int* rama_idx, const int* hbond_idx,
                                           upk_coord_t self) {
    UPK_FLUSH(L);
    if (self.width != 6 || rama.width < 2 || hbond.width < 7) return 9201;
    hipLaunchKernelGGL(k_backbone_featurizer_bwd, nn_grid1(self.n_elem, L->n_system), dim3(NN_BLOCK), 0, ST(L), rama, hbond, rama_idx, hbond_idx, self);
    return launch_status();
}

// ------------------------------------------------------------------------------------------------
// conv1d
// The contraction both passes share.  A workgroup has staged
//   wl [n_w * n_red][n_ch_tile]   the weights of its channel slice, term-major (zero beyond the layer's channels)
//   xl [NN_TR + n_w - 1][xs]      the rows its tile reads (zero outside the array)
// and lane item (row group, channel pair) accumulates, for its NN_RB rows and 2 channels,
//   acc[k] = init;  for w ascending, for c ascending:  acc[k] = fma(xl[row_k + shift(w)][c], wl[w][c][pair], acc[k])
// shift(w) = w forward (out[r] reads in[r + w]), n_w - 1 - w backward (in[j] gathers from g[j - w], staged from row j0 - (n_w - 1)).
template <bool BACKWARD, typename Finish>
__device__ __forceinline__ void nn_contract(const float* __restrict__ wl, const float* __restrict__ xl, int xs, int n_w, int n_red, int n_ch_tile,
                                            int n_row_valid, const float* __restrict__ init, int ch0, int n_ch, Finish finish) {
    const int n_cp = n_ch_tile >> 1;
    for (int item = threadIdx.x; item < (NN_TR / NN_RB) * n_cp; item += blockDim.x) {
        const int rg = item / n_cp, cp = item - rg * n_cp;
        const int rl = rg * NN_RB, c = cp * 2;
        if (rl >= n_row_valid) continue;
        v2f b;
        b.x = (init && ch0 + c < n_ch) ? init[ch0 + c] : 0.f;
        b.y = (init && ch0 + c + 1 < n_ch) ? init[ch0 + c + 1] : 0.f;
        v2f acc[NN_RB];
#pragma unroll
        for (int k = 0; k < NN_RB; ++k) acc[k] = b;
        for (int w = 0; w < n_w; ++w) {
            const float* wp = wl + (size_t)w * n_red * n_ch_tile + c;
            const float* xp = xl + (size_t)(rl + (BACKWARD ? n_w - 1 - w : w)) * xs;
            for (int q = 0; q < n_red; ++q) {
                const v2f wv = *(const v2f*)(wp + (size_t)q * n_ch_tile);
#pragma unroll
                for (int k = 0; k < NN_RB; ++k) {
                    const float x = xp[k * xs + q];
                    v2f xv; xv.x = x; xv.y = x;
                    acc[k] = __builtin_elementwise_fma(xv, wv, acc[k]);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NN_RB; ++k) if (rl + k < n_row_valid) finish(rl + k, ch0 + c, acc[k].x, acc[k].y);
    }
}

// largest even channel slice whose weights, beside the staged rows, fit the LDS budget; 0: not even two channels fit
static int nn_channel_tile(int n_w, int n_red, int n_ch) {
    const long rows = (long)(NN_TR + n_w - 1) * (n_red | 1) * 4;
    int t = (n_ch + 1) & ~1;
    while (t > 2 && (long)n_w * n_red * t * 4 + rows > NN_LDS_BUDGET) t = ((t / 2) + 1) & ~1;
    return (long)n_w * n_red * t * 4 + rows <= NN_LDS_BUDGET ? t : 0;
}
static inline size_t nn_lds_bytes(int n_w, int n_red, int tile) { return ((size_t)n_w * n_red * tile + (size_t)(NN_TR + n_w - 1) * (n_red | 1)) * 4; }
static inline size_t nn_pd_lds_bytes(int W, int C_in, int C_out) { return ((size_t)NN_PD_ROWS * C_out + (size_t)(NN_PD_ROWS + W - 1) * C_in) * 4; }
extern "C" int upk_conv1d_fits(int W, int C_in, int C_out) {
    if (W < 1 || C_in < 1 || C_out < 1) return 0;
    return nn_channel_tile(W, C_in, C_out) > 0 && nn_channel_tile(W, C_out, C_in) > 0 && nn_pd_lds_bytes(W, C_in, C_out) <= NN_LDS_BUDGET;
}

// grid.x = row tiles x channel tiles (channel tile fastest), grid.y = system
__global__ void __launch_bounds__(NN_BLOCK) k_conv1d_fwd(upk_conv1d_t P, upk_coord_t in, upk_coord_t out, int cot, int n_ct) {
    extern __shared__ float nn_lds[];
    const int s = blockIdx.y, rt = blockIdx.x / n_ct, ct = blockIdx.x - rt * n_ct;
    const int r0 = rt * NN_TR, co0 = ct * cot, xs = P.C_in | 1, n_term = P.W * P.C_in;
    float* wl = nn_lds;
    float* xl = nn_lds + (size_t)n_term * cot;
    for (int e = threadIdx.x; e < n_term * cot; e += blockDim.x) {
        const int k = e / cot, co = co0 + (e - k * cot);
        wl[e] = co < P.C_out ? P.param[(size_t)k * P.C_out + co] : 0.f;
    }
    const float* xin = C_OUT(in, s);
    for (int e = threadIdx.x; e < (NN_TR + P.W - 1) * P.C_in; e += blockDim.x) {
        const int row = e / P.C_in, ci = e - row * P.C_in, gr = r0 + row;
        xl[(size_t)row * xs + ci] = gr < in.n_elem ? xin[(size_t)gr * in.stride + ci] : 0.f;
    }
    __syncthreads();
    const float* bias = P.param + (size_t)n_term * P.C_out;
    float* o = C_OUT(out, s);
    const int n_valid = out.n_elem - r0 < NN_TR ? out.n_elem - r0 : NN_TR;
    nn_contract<false>(wl, xl, xs, P.W, P.C_in, cot, n_valid, bias, co0, P.C_out, [&](int rl, int co, float a, float b) {
        float* row = o + (size_t)(r0 + rl) * out.stride;
        if (co < P.C_out) row[co] = nn_act(a, P.act);
        if (co + 1 < P.C_out) row[co + 1] = nn_act(b, P.act);
    });
}
// the same over the input rows: tile rows are rows j of `in`, the staged rows are g[j0 - (W-1) ...], the slice is cut over C_in
__global__ void __launch_bounds__(NN_BLOCK) k_conv1d_bwd(upk_conv1d_t P, upk_coord_t in, upk_coord_t out, int cit, int n_ct) {
    extern __shared__ float nn_lds[];
    const int s = blockIdx.y, rt = blockIdx.x / n_ct, ct = blockIdx.x - rt * n_ct;
    const int j0 = rt * NN_TR, ci0 = ct * cit, gs = P.C_out | 1;
    float* wl = nn_lds;                                     // [W][C_out][cit]: the slice transposed, so that a lane's two channels are adjacent
    float* gl = nn_lds + (size_t)P.W * P.C_out * cit;
    for (int e = threadIdx.x; e < P.W * cit * P.C_out; e += blockDim.x) {      // (read in file order: consecutive lanes, consecutive co)
        const int w = e / (cit * P.C_out), rem = e - w * (cit * P.C_out), cl = rem / P.C_out, co = rem - cl * P.C_out, ci = ci0 + cl;
        wl[((size_t)w * P.C_out + co) * cit + cl] = ci < P.C_in ? P.param[((size_t)w * P.C_in + ci) * P.C_out + co] : 0.f;
    }
    const float* y = C_OUT(out, s); const float* ys = C_SENS(out, s);
    for (int e = threadIdx.x; e < (NN_TR + P.W - 1) * P.C_out; e += blockDim.x) {
        const int row = e / P.C_out, co = e - row * P.C_out, r = j0 - (P.W - 1) + row;
        float g = 0.f;
        if (r >= 0 && r < out.n_elem) { const size_t at = (size_t)r * out.stride + co; g = ys[at] * nn_dact(y[at], P.act); }
        gl[(size_t)row * gs + co] = g;
    }
    __syncthreads();
    float* xsens = C_SENS(in, s);
    const int n_valid = in.n_elem - j0 < NN_TR ? in.n_elem - j0 : NN_TR;
    nn_contract<true>(wl, gl, gs, P.W, P.C_out, cit, n_valid, nullptr, ci0, P.C_in, [&](int jl, int ci, float a, float b) {
        float* row = xsens + (size_t)(j0 + jl) * in.stride;
        if (ci < P.C_in) row[ci] += a;
        if (ci + 1 < P.C_in) row[ci + 1] += b;
    });
}
static int nn_check(const upk_conv1d_t* P, const upk_coord_t& in, const upk_coord_t& out) {
    if (!P || !P->param || P->W < 1 || in.width != P->C_in || out.width != P->C_out || out.n_elem != in.n_elem - P->W + 1 || out.n_elem < 1) return 9202;
    return 0;
}
extern "C" int upk_conv1d_fwd(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out) {
    UPK_FLUSH(L);
    if (const int r = nn_check(P, in, out)) return r;
    const int cot = nn_channel_tile(P->W, P->C_in, P->C_out);
    if (!cot) return 9203;
    const int n_ct = (P->C_out + cot - 1) / cot, n_rt = (out.n_elem + NN_TR - 1) / NN_TR;
    hipLaunchKernelGGL(k_conv1d_fwd, dim3((unsigned)(n_rt * n_ct), (unsigned)L->n_system), dim3(NN_BLOCK), nn_lds_bytes(P->W, P->C_in, cot), ST(L),
                       *P, in, out, cot, n_ct);
    return launch_status();
}
extern "C" int upk_conv1d_bwd(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out) {
    UPK_FLUSH(L);
    if (const int r = nn_check(P, in, out)) return r;
    const int cit = nn_channel_tile(P->W, P->C_out, P->C_in);
    if (!cit) return 9203;
    const int n_ct = (P->C_in + cit - 1) / cit, n_rt = (in.n_elem + NN_TR - 1) / NN_TR;
    hipLaunchKernelGGL(k_conv1d_bwd, dim3((unsigned)(n_rt * n_ct), (unsigned)L->n_system), dim3(NN_BLOCK), nn_lds_bytes(P->W, P->C_out, cit), ST(L),
                       *P, in, out, cit, n_ct);
    return launch_status();
}

// Weight gradient.  grid.x = slices of NN_BLOCK * NN_PD_PER_LANE table entries, grid.y = system (s0 + blockIdx.y, written to table row
// blockIdx.y).  A lane owns its entries from the first row to the last: rows are staged NN_PD_ROWS at a time (g of the chunk and the
// input rows it pairs with), and an entry is one fma chain over r ascending.  Entries past W*C_in*C_out are the bias: sum of g.
__global__ void __launch_bounds__(NN_BLOCK) k_conv1d_param_deriv(upk_conv1d_t P, upk_coord_t in, upk_coord_t out, int s0, float* __restrict__ table) {
    extern __shared__ float nn_lds[];
    const int s = s0 + blockIdx.y, n_w = P.W * P.C_in * P.C_out, n_param = n_w + P.C_out;
    float* gl = nn_lds;                                      // [NN_PD_ROWS][C_out]
    float* xl = nn_lds + (size_t)NN_PD_ROWS * P.C_out;       // [NN_PD_ROWS + W - 1][C_in]
    int go[NN_PD_PER_LANE], xo[NN_PD_PER_LANE]; float acc[NN_PD_PER_LANE];
#pragma unroll
    for (int k = 0; k < NN_PD_PER_LANE; ++k) {
        const int e = (blockIdx.x * NN_PD_PER_LANE + k) * NN_BLOCK + threadIdx.x;
        acc[k] = 0.f; go[k] = -1; xo[k] = -1;
        if (e < n_w) { const int co = e % P.C_out, t = e / P.C_out, ci = t % P.C_in, w = t / P.C_in; go[k] = co; xo[k] = w * P.C_in + ci; }
        else if (e < n_param) go[k] = e - n_w;
    }
    const float* y = C_OUT(out, s); const float* ys = C_SENS(out, s); const float* xin = C_OUT(in, s);
    for (int r0 = 0; r0 < out.n_elem; r0 += NN_PD_ROWS) {
        __syncthreads();
        for (int e = threadIdx.x; e < NN_PD_ROWS * P.C_out; e += blockDim.x) {
            const int row = e / P.C_out, co = e - row * P.C_out, r = r0 + row;
            float g = 0.f;
            if (r < out.n_elem) { const size_t at = (size_t)r * out.stride + co; g = ys[at] * nn_dact(y[at], P.act); }
            gl[e] = g;
        }
        for (int e = threadIdx.x; e < (NN_PD_ROWS + P.W - 1) * P.C_in; e += blockDim.x) {
            const int row = e / P.C_in, ci = e - row * P.C_in, r = r0 + row;
            xl[e] = r < in.n_elem ? xin[(size_t)r * in.stride + ci] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NN_PD_PER_LANE; ++k) {
            if (go[k] < 0) continue;
            float a = acc[k];
            if (xo[k] >= 0) for (int rr = 0; rr < NN_PD_ROWS; ++rr) a = fmaf(gl[rr * P.C_out + go[k]], xl[rr * P.C_in + xo[k]], a);
            else for (int rr = 0; rr < NN_PD_ROWS; ++rr) a += gl[rr * P.C_out + go[k]];
            acc[k] = a;
        }
    }
    float* t = table + (size_t)blockIdx.y * n_param;
#pragma unroll
    for (int k = 0; k < NN_PD_PER_LANE; ++k) {
        const int e = (blockIdx.x * NN_PD_PER_LANE + k) * NN_BLOCK + threadIdx.x;
        if (e < n_param) t[e] = acc[k];
    }
}
static int nn_param_deriv_launch(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out, int s0, int n_sys, float* table) {
    if (const int r = nn_check(P, in, out)) return r;
    const size_t lds = nn_pd_lds_bytes(P->W, P->C_in, P->C_out);
    if (lds > NN_LDS_BUDGET) return 9203;
    const int n_param = P->W * P->C_in * P->C_out + P->C_out, per = NN_BLOCK * NN_PD_PER_LANE;
    hipLaunchKernelGGL(k_conv1d_param_deriv, dim3((unsigned)((n_param + per - 1) / per), (unsigned)n_sys), dim3(NN_BLOCK), lds, ST(L), *P, in, out, s0, table);
    return launch_status();
}
extern "C" int upk_conv1d_param_deriv(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out, int system, float* table) {
    UPK_FLUSH(L);
    if (system < 0 || system >= L->n_system) return 9101;
    return nn_param_deriv_launch(L, P, in, out, system, 1, table);
}
extern "C" int upk_conv1d_param_deriv_all(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out, float* table) {
    UPK_FLUSH(L);
    return nn_param_deriv_launch(L, P, in, out, 0, L->n_system, table);
}

// ------------------------------------------------------------------------------------------------
// scaled_sum: the terms go to the node's deterministic reduction (upk_reduce_sum)
__global__ void k_scaled_sum(upk_coord_t in, const float* __restrict__ scale, float* __restrict__ pot_terms) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= in.n_elem) return;
    const int s = blockIdx.y;
    const float c = scale[0];
    C_SENS(in, s)[(size_t)i * in.stride] += c;
    if (pot_terms) pot_terms[(size_t)s * in.n_elem + i] = c * C_OUT(in, s)[(size_t)i * in.stride];
}
extern "C" int upk_scaled_sum(const upk_launch_t* L, upk_coord_t in, const float* scale, float* pot_terms) {
    UPK_FLUSH(L);
    if (in.width != 1) return 9204;
    hipLaunchKernelGGL(k_scaled_sum, nn_grid1(in.n_elem, L->n_system), dim3(NN_BLOCK), 0, ST(L), in, scale, pot_terms);
    return launch_status();
}

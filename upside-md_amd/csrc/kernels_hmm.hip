// gfx950 kernels of the sequence-dependent backbone prior (hmm.cpp of the reference): torus_dbn, the bivariate von-Mises emission
// energy of every hidden state from phi and psi, and fixed_hmm, a hidden Markov chain along the residues whose free energy is the
// potential and whose posterior state marginals are the gradient.
//
// fixed_hmm is sequential along the chain: one n_state x n_state matrix-vector product and one renormalisation per residue, forward
// and backward.  The parallelism is over the states inside a wavefront and over the systems across wavefronts:
//   * one wavefront owns one system from the first residue to the last and back; HMM_WAVES of them share a workgroup and with it
//     one copy of the transition matrix T in LDS (rows HMM_NSP + 1 floats apart: a lane group reads a row, forward, or a column,
//     backward, without a bank conflict);
//   * state j lives in lane j & 63, slot j >> 6 (one slot up to 64 states, two up to 128);
//   * a step of the product broadcasts one entry of the previous belief with v_readlane and is one fma per slot against the LDS row;
//     the normaliser is the fixed butterfly of device_math.h (wave_sum).
// Every number is one chain of operations in a fixed order -- the product over the source state ascending, the butterfly, the sum
// of the logs below -- so a system's bits depend neither on the batch nor on its place in it.  No atomics anywhere.
//
// The potential, -log Z = offset (n - 1) + sum_r e_min[r] - sum_r log norm_r, is accumulated in fp64: lane r & 63 keeps the
// normaliser and the minimum of residue r, every 64 residues each lane adds e_min - log(norm) of its own residue to its own fp64
// sum (64 logarithms for the price of one), and lane 0 adds the 64 sums in lane order at the end.
//
// Backward pass: with beta scaled so that f_r . beta_r = 1 the marginal of residue r is f_r * beta_r, and ONE reduction per residue
// normalises both (the reference's code scales beta to sum 1 and normalises the marginal separately; the marginals are the same).
// The forward beliefs are kept in the node's scratch buffer; the emission probabilities are recomputed from the energies.
#include "device_math.h"
#include "../../include/upside_hip_kernels.h"
#include <cmath>

using namespace up;

#define ST(L) ((hipStream_t)(L)->stream)
#define C_OUT(c, s)  ((c).out  + (size_t)(s) * (c).n_elem * (c).stride)
#define C_SENS(c, s) ((c).sens + (size_t)(s) * (c).n_elem * (c).stride)
static inline int launch_status() { return (int)hipGetLastError(); }

#define HMM_BLOCK 256
#define HMM_MAX_STATE 128
#define HMM_WAVES 4                   // systems (wavefronts) per workgroup of the chain kernels
#define HMM_UNROLL 8                  // steps of a matrix-vector product per trip (a wave-uniform broadcast cannot be unrolled with a remainder)
#define TD_ROWS 16                    // residues per workgroup of torus_dbn's forward kernel

// ------------------------------------------------------------------------------------------------
// torus_dbn: out[r][s] = (prior[restypes[r]][s] + M[6][s]) + sum_{k<6} cs_k(r) M[k][s], k ascending;
// cs = (cos phi, sin phi, cos psi, sin psi, cos(phi - psi), sin(phi - psi)), phi, psi = columns 0, 1 of rama row id[r]
__device__ __forceinline__ void td_cs(const float* __restrict__ a, float (&cs)[6]) {
    const float phi = a[0], psi = a[1];
    cs[0] = cosf(phi); cs[1] = sinf(phi); cs[2] = cosf(psi); cs[3] = sinf(psi); cs[4] = cosf(phi - psi); cs[5] = sinf(phi - psi);
}
__global__ void __launch_bounds__(HMM_BLOCK) k_torus_dbn_fwd(upk_torus_dbn_t P, upk_coord_t rama, upk_coord_t out) {
    __shared__ float csl[TD_ROWS][6];
    const int s = blockIdx.y, r0 = blockIdx.x * TD_ROWS, n_state = out.width;
    if (threadIdx.x < TD_ROWS && r0 + threadIdx.x < out.n_elem) {
        float cs[6];
        td_cs(C_OUT(rama, s) + (size_t)P.id[r0 + threadIdx.x] * rama.stride, cs);
#pragma unroll
        for (int k = 0; k < 6; ++k) csl[threadIdx.x][k] = cs[k];
    }
    __syncthreads();
    float* o = C_OUT(out, s);
    for (int e = threadIdx.x; e < TD_ROWS * n_state; e += blockDim.x) {
        const int rl = e / n_state, st = e - rl * n_state, r = r0 + rl;
        if (r >= out.n_elem) break;
        float v = P.prior[(size_t)P.restypes[r] * n_state + st] + P.cs_to_emission[6 * n_state + st];
#pragma unroll
        for (int k = 0; k < 6; ++k) v = fmaf(csl[rl][k], P.cs_to_emission[k * n_state + st], v);
        o[(size_t)r * out.stride + st] = v;
    }
}
// A 16-lane row per residue: a lane sums its states (lane, lane + 16, ...) in ascending order, the row's butterfly (four DPP steps)
// finishes g_k = sum_s sens[r][s] M[k][s]; lanes 0, 1, 2 of the row then take the chain rule of one angle each (phi, psi, phi - psi)
__global__ void __launch_bounds__(HMM_BLOCK) k_torus_dbn_bwd(upk_torus_dbn_t P, upk_coord_t rama, upk_coord_t self) {
    const int r = blockIdx.x * (HMM_BLOCK / 16) + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    if (r >= self.n_elem) return;      // (whole rows leave: the exchanges below stay inside a row)
    const int s = blockIdx.y, n_state = self.width;
    const float* g = C_SENS(self, s) + (size_t)r * self.stride;
    float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int st = sub; st < n_state; st += 16) {
        const float gv = g[st];
#pragma unroll
        for (int k = 0; k < 6; ++k) d[k] = fmaf(gv, P.cs_to_emission[k * n_state + st], d[k]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        float v = d[k];
        v += dpp_mov<UP_DPP_XOR1>(v); v += dpp_mov<UP_DPP_XOR2>(v); v += dpp_mov<UP_DPP_HALF_MIRROR>(v); v += dpp_mov<UP_DPP_ROW_MIRROR>(v);
        d[k] = v;
    }
    const int at = P.id[r];
    const float* a = C_OUT(rama, s) + (size_t)at * rama.stride;
    const float phi = a[0], psi = a[1];
    const float angle = sub == 0 ? phi : sub == 1 ? psi : phi - psi;
    const float dc = sub == 0 ? d[0] : sub == 1 ? d[2] : d[4], ds = sub == 0 ? d[1] : sub == 1 ? d[3] : d[5];
    const float t = cosf(angle) * ds - sinf(angle) * dc;      // d(cos) = -sin, d(sin) = cos
    const float t2 = dpp_mov<0xAA>(t);                        // quad_perm [2,2,2,2]: the phi - psi term
    float* o = C_SENS(rama, s) + (size_t)at * rama.stride;
    if (sub == 0) o[0] += t + t2;
    else if (sub == 1) o[1] += t - t2;
}
// table[t][s] = sum over r (ascending) with restypes[r] = t of sens[r][s]
__global__ void __launch_bounds__(HMM_BLOCK) k_torus_dbn_param_deriv(upk_torus_dbn_t P, upk_coord_t self, int s0, float* __restrict__ table) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n_state = self.width, n_param = P.n_restype * n_state;
    if (e >= n_param) return;
    const int t = e / n_state, st = e - t * n_state;
    const float* g = C_SENS(self, s0 + blockIdx.y);
    float acc = 0.f;
    for (int r = 0; r < self.n_elem; ++r) if (P.restypes[r] == t) acc += g[(size_t)r * self.stride + st];
    table[(size_t)blockIdx.y * n_param + e] = acc;
}
static int td_check(const upk_torus_dbn_t* P, const upk_coord_t& rama, const upk_coord_t& self) {
    if (!P || !P->id || !P->restypes || !P->prior || !P->cs_to_emission || P->n_restype < 1 || rama.width < 2 || self.width < 1 || self.n_elem < 1) return 9301;
    return 0;
}
extern "C" int upk_torus_dbn_fwd(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t rama, upk_coord_t out) {
    UPK_FLUSH(L);
    if (const int r = td_check(P, rama, out)) return r;
    hipLaunchKernelGGL(k_torus_dbn_fwd, dim3((unsigned)((out.n_elem + TD_ROWS - 1) / TD_ROWS), (unsigned)L->n_system), dim3(HMM_BLOCK), 0, ST(L), *P, rama, out);
    return launch_status();
}
extern "C" int upk_torus_dbn_bwd(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t rama, upk_coord_t self) {
    UPK_FLUSH(L);
    if (const int r = td_check(P, rama, self)) return r;
    hipLaunchKernelGGL(k_torus_dbn_bwd, dim3((unsigned)((self.n_elem + HMM_BLOCK / 16 - 1) / (HMM_BLOCK / 16)), (unsigned)L->n_system), dim3(HMM_BLOCK), 0, ST(L), *P, rama, self);
    return launch_status();
}
static int td_param_deriv_launch(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t self, int s0, int n_sys, float* table) {
    if (!P || !P->restypes || P->n_restype < 1 || self.width < 1 || self.n_elem < 1 || !table) return 9301;
    const int n_param = P->n_restype * self.width;
    hipLaunchKernelGGL(k_torus_dbn_param_deriv, dim3((unsigned)((n_param + HMM_BLOCK - 1) / HMM_BLOCK), (unsigned)n_sys), dim3(HMM_BLOCK), 0, ST(L), *P, self, s0, table);
    return launch_status();
}
extern "C" int upk_torus_dbn_param_deriv(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t self, int system, float* table) {
    UPK_FLUSH(L);
    if (system < 0 || system >= L->n_system) return 9101;
    return td_param_deriv_launch(L, P, self, system, 1, table);
}
extern "C" int upk_torus_dbn_param_deriv_all(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t self, float* table) {
    UPK_FLUSH(L);
    return td_param_deriv_launch(L, P, self, 0, L->n_system, table);
}

// ------------------------------------------------------------------------------------------------
// fixed_hmm
template <int K> struct HmmShape { static constexpr int NSP = 64 * K, LD = 64 * K + 1; };

__device__ __forceinline__ float lane_value(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// T[i][j] at tl[i * LD + j], zero outside the n_state x n_state block (NSP rows: a lane past the last state reads zeros)
template <int K>
__device__ __forceinline__ void hmm_stage(const float* __restrict__ T, int n_state, float* __restrict__ tl) {
    constexpr int NSP = HmmShape<K>::NSP, LD = HmmShape<K>::LD;
    for (int e = threadIdx.x; e < NSP * NSP; e += blockDim.x) {
        const int i = e / NSP, j = e - i * NSP;
        tl[i * LD + j] = (i < n_state && j < n_state) ? T[(size_t)i * n_state + j] : 0.f;
    }
    __syncthreads();
}
// b[k] = exp(e_min - e[j]), j = lane + 64 k, of one row of emission energies (0 past the last state)
template <int K>
__device__ __forceinline__ float hmm_emission(const float* __restrict__ row, int n_state, int lane, float (&b)[K]) {
    float e[K], m = INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { const int j = lane + 64 * k; e[k] = j < n_state ? row[j] : INFINITY; m = fminf(m, e[k]); }
    m = wave_reduce(m, [](float a, float c) { return fminf(a, c); });
#pragma unroll
    for (int k = 0; k < K; ++k) b[k] = lane + 64 * k < n_state ? expf(m - e[k]) : 0.f;
    return m;
}
// out[j] = sum_i x[i] T[i][j], i ascending (x spread over the lanes like every state vector)
template <int K>
__device__ __forceinline__ void hmm_row_times_T(const float* __restrict__ tl, int n_state, int lane, const float (&x)[K], float (&out)[K]) {
    constexpr int LD = HmmShape<K>::LD;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = 0.f;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        const int n = n_state - 64 * kk < 64 ? n_state - 64 * kk : 64;
        const float* tp = tl + (size_t)(64 * kk) * LD + lane;
        for (int i0 = 0; i0 < n; i0 += HMM_UNROLL) {      // (past n: zero entries of x against zero rows of T)
#pragma unroll
            for (int q = 0; q < HMM_UNROLL; ++q) {
                const int i = i0 + q;
                const float xi = lane_value(x[kk], i);
#pragma unroll
                for (int k = 0; k < K; ++k) out[k] = fmaf(xi, tp[i * LD + 64 * k], out[k]);
            }
        }
    }
}
// out[i] = sum_j T[i][j] x[j], j ascending
template <int K>
__device__ __forceinline__ void hmm_T_times_col(const float* __restrict__ tl, int n_state, int lane, const float (&x)[K], float (&out)[K]) {
    constexpr int LD = HmmShape<K>::LD;
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = 0.f;
#pragma unroll
    for (int kk = 0; kk < K; ++kk) {
        const int n = n_state - 64 * kk < 64 ? n_state - 64 * kk : 64;
        const float* tp = tl + (size_t)lane * LD + 64 * kk;
        for (int j0 = 0; j0 < n; j0 += HMM_UNROLL) {
#pragma unroll
            for (int q = 0; q < HMM_UNROLL; ++q) {
                const int j = j0 + q;
                const float xj = lane_value(x[kk], j);
#pragma unroll
                for (int k = 0; k < K; ++k) out[k] = fmaf(tp[(64 * k) * LD + j], xj, out[k]);
            }
        }
    }
}
template <int K> __device__ __forceinline__ float hmm_total(const float (&v)[K]) {
    float t = v[0];
#pragma unroll
    for (int k = 1; k < K; ++k) t += v[k];
    return wave_sum(t);
}

// forward recursion of one system: beliefs to fwd [n_residue][row_stride]; returns -log Z on every lane when want_pot
template <int K>
__device__ __forceinline__ float hmm_forward(const upk_fixed_hmm_t& H, const float* __restrict__ tl, const float* __restrict__ energy, int e_stride,
                                             float* fwd, int lane, bool want_pot) {
    const int n_state = H.n_state, N = H.n_residue;
    float f[K], b[K], g[K];
    double acc = 0.;
    float kept_norm = 1.f, kept_min = 0.f;
    for (int r = 0; r < N; ++r) {
        const float e_min = hmm_emission<K>(energy + (size_t)H.index[r] * e_stride, n_state, lane, b);
        if (r) hmm_row_times_T<K>(tl, n_state, lane, f, g);
        else {
#pragma unroll
            for (int k = 0; k < K; ++k) g[k] = 1.f;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) g[k] *= b[k];
        const float norm = hmm_total<K>(g), inv = 1.f / norm;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            f[k] = g[k] * inv;
            if (lane + 64 * k < n_state) fwd[(size_t)r * H.row_stride + lane + 64 * k] = f[k];
        }
        if (want_pot) {
            if (lane == (r & 63)) { kept_norm = norm; kept_min = e_min; }
            if (((r & 63) == 63 || r == N - 1) && lane <= (r & 63)) acc += (double)kept_min - log((double)kept_norm);
        }
    }
    if (!want_pot) return 0.f;
    double total = (double)H.offset[0] * (double)(N - 1);
    for (int l = 0; l < 64; ++l) total += __shfl(acc, l);
    return (float)total;
}
// backward recursion of one system from the stored beliefs.  ADD_SENS: the marginal of residue r is added to sens row index[r];
// w (or NULL): w[r][j] = beta_r[j] b_r[j] / s_r for r >= 1, s_r = sum_ij f_{r-1}[i] T[i][j] beta_r[j] b_r[j]: the factor of the
// expected transition counts of edge r - 1 -> r that belongs to its right end.
template <int K, bool ADD_SENS>
__device__ __forceinline__ void hmm_backward(const upk_fixed_hmm_t& H, const float* __restrict__ tl, const float* __restrict__ energy, int e_stride,
                                             const float* fwd, float* sens, float* w, int lane) {
    const int n_state = H.n_state, N = H.n_residue;
    float beta[K], m[K], f[K], b[K], v[K], u[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = lane + 64 * k;
        f[k] = j < n_state ? fwd[(size_t)(N - 1) * H.row_stride + j] : 0.f;
        m[k] = f[k];
    }
    {
        const float inv = 1.f / hmm_total<K>(m);
#pragma unroll
        for (int k = 0; k < K; ++k) { beta[k] = lane + 64 * k < n_state ? inv : 0.f; m[k] *= inv; }
    }
    for (int r = N - 1; r >= 0; --r) {
        if (ADD_SENS) {
            float* row = sens + (size_t)H.index[r] * e_stride;
#pragma unroll
            for (int k = 0; k < K; ++k) if (lane + 64 * k < n_state) row[lane + 64 * k] += m[k];
        }
        if (!r) break;
        hmm_emission<K>(energy + (size_t)H.index[r] * e_stride, n_state, lane, b);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = lane + 64 * k;
            v[k] = beta[k] * b[k];
            f[k] = j < n_state ? fwd[(size_t)(r - 1) * H.row_stride + j] : 0.f;
        }
        hmm_T_times_col<K>(tl, n_state, lane, v, u);
#pragma unroll
        for (int k = 0; k < K; ++k) m[k] = f[k] * u[k];
        const float inv = 1.f / hmm_total<K>(m);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            beta[k] = u[k] * inv; m[k] *= inv;
            if (w && lane + 64 * k < n_state) w[(size_t)r * H.row_stride + lane + 64 * k] = v[k] * inv;
        }
    }
}

// grid.x = groups of HMM_WAVES systems; wavefront w of a workgroup owns system blockIdx.x * HMM_WAVES + w
template <int K>
__global__ void __launch_bounds__(64 * HMM_WAVES) k_fixed_hmm(upk_fixed_hmm_t H, upk_coord_t in, int n_system, float* __restrict__ potential) {
    __shared__ float tl[HmmShape<K>::NSP * HmmShape<K>::LD];
    hmm_stage<K>(H.T, H.n_state, tl);
    const int s = blockIdx.x * HMM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n_system) return;
    float* fwd = H.fwd + (size_t)s * H.n_residue * H.row_stride;
    const float pot = hmm_forward<K>(H, tl, C_OUT(in, s), in.stride, fwd, lane, potential != nullptr);
    if (potential && lane == 0) potential[s] = pot;
    hmm_backward<K, true>(H, tl, C_OUT(in, s), in.stride, fwd, C_SENS(in, s), nullptr, lane);
}
// the backward recursion again, for the systems s0 .. s0 + n_sys - 1, leaving w for k_fixed_hmm_counts
template <int K>
__global__ void __launch_bounds__(64 * HMM_WAVES) k_fixed_hmm_edge_factors(upk_fixed_hmm_t H, upk_coord_t in, int s0, int n_sys) {
    __shared__ float tl[HmmShape<K>::NSP * HmmShape<K>::LD];
    hmm_stage<K>(H.T, H.n_state, tl);
    const int q = blockIdx.x * HMM_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= n_sys) return;
    const int s = s0 + q;
    const size_t at = (size_t)s * H.n_residue * H.row_stride;
    hmm_backward<K, false>(H, tl, C_OUT(in, s), in.stride, H.fwd + at, nullptr, H.w + at, lane);
}
// table[i][j] = T[i][j] * sum_{r >= 1} f_{r-1}[i] w_r[j], r ascending: the expected transition counts (hmm.cpp:188-197)
__global__ void __launch_bounds__(HMM_BLOCK) k_fixed_hmm_counts(upk_fixed_hmm_t H, int s0, float* __restrict__ table) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n_param = H.n_state * H.n_state;
    if (e >= n_param) return;
    const int i = e / H.n_state, j = e - i * H.n_state;
    const size_t at = (size_t)(s0 + blockIdx.y) * H.n_residue * H.row_stride;
    const float* f = H.fwd + at; const float* w = H.w + at;
    float acc = 0.f;
    for (int r = 1; r < H.n_residue; ++r) acc = fmaf(f[(size_t)(r - 1) * H.row_stride + i], w[(size_t)r * H.row_stride + j], acc);
    table[(size_t)blockIdx.y * n_param + e] = H.T[e] * acc;
}

extern "C" int upk_fixed_hmm_max_state(void) { return HMM_MAX_STATE; }
static int hmm_check(const upk_fixed_hmm_t* H, const upk_coord_t& in) {
    if (!H || !H->T || !H->offset || !H->index || !H->fwd || H->n_residue < 1 || H->n_state < 1 || H->n_state > HMM_MAX_STATE) return 9302;
    if (in.width != H->n_state || H->row_stride < H->n_state || in.stride < in.width) return 9303;
    return 0;
}
extern "C" int upk_fixed_hmm(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, float* potential) {
    UPK_FLUSH(L);
    if (const int r = hmm_check(H, in)) return r;
    const dim3 grid((unsigned)((L->n_system + HMM_WAVES - 1) / HMM_WAVES)), block(64 * HMM_WAVES);
    if (H->n_state <= 64) hipLaunchKernelGGL(k_fixed_hmm<1>, grid, block, 0, ST(L), *H, in, L->n_system, potential);
    else hipLaunchKernelGGL(k_fixed_hmm<2>, grid, block, 0, ST(L), *H, in, L->n_system, potential);
    return launch_status();
}
static int hmm_param_deriv_launch(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, int s0, int n_sys, float* table) {
    if (const int r = hmm_check(H, in)) return r;
    if (!H->w || !table) return 9302;
    const dim3 grid((unsigned)((n_sys + HMM_WAVES - 1) / HMM_WAVES)), block(64 * HMM_WAVES);
    if (H->n_state <= 64) hipLaunchKernelGGL(k_fixed_hmm_edge_factors<1>, grid, block, 0, ST(L), *H, in, s0, n_sys);
    else hipLaunchKernelGGL(k_fixed_hmm_edge_factors<2>, grid, block, 0, ST(L), *H, in, s0, n_sys);
    if (const int r = launch_status()) return r;
    const int n_param = H->n_state * H->n_state;
    hipLaunchKernelGGL(k_fixed_hmm_counts, dim3((unsigned)((n_param + HMM_BLOCK - 1) / HMM_BLOCK), (unsigned)n_sys), dim3(HMM_BLOCK), 0, ST(L), *H, s0, table);
    return launch_status();
}
extern "C" int upk_fixed_hmm_param_deriv(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, int system, float* table) {
    UPK_FLUSH(L);
    if (system < 0 || system >= L->n_system) return 9101;
    return hmm_param_deriv_launch(L, H, in, system, 1, table);
}
extern "C" int upk_fixed_hmm_param_deriv_all(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, float* table) {
    UPK_FLUSH(L);
    return hmm_param_deriv_launch(L, H, in, 0, L->n_system, table);
}

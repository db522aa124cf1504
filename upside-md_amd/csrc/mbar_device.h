// What the MBAR translation units share (kernels_mbar.hip: the iteration; kernels_mbar_gram.hip: the Gram pass): the reduced energy
// of a sample under a staged state, the per-d dispatch, and the host-side refusal and staging helpers.  One statement of each.
#pragma once
#include "cv_device.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

namespace up {
namespace mbar {

#define MBAR_BLOCK CV_BLOCK
#define MBAR_TILE UPK_MBAR_STATE_TILE
#define MBAR_FE UPK_MBAR_FE_TILE
static_assert(MBAR_FE <= CV_MAX_SUMS, "block_sum holds CV_MAX_SUMS totals");

// the doubles of one staged state: a, beta, then center, spring_const, flat_width of the D CVs
template <int D> constexpr int mbar_state_doubles() { return 2 + 3 * D; }

// state k of S into dst (one lane per double of the row; called by the lanes `lane`, `lane + stride`, ... of a workgroup)
template <int D>
__device__ __forceinline__ void mbar_stage_state(const upk_mbar_states_t& S, int k, double a, double* __restrict__ dst, int j) {
    if (j == 0) dst[0] = a;
    else if (j == 1) dst[1] = S.beta[k];
    else dst[j] = (double)S.rows[(size_t)k * (3 * D) + (j - 2)];
}

// E + sum_c 1/2 k u^2 of the sample (v, E) under the staged state st; P = the periods
template <int D>
__device__ __forceinline__ double mbar_energy(const double (&v)[D ? D : 1], double E, const double* __restrict__ st, const upk_mbar_states_t& S) {
    double e = E;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double x = v[c] - st[2 + c];
        const double P = S.period[c];
        if (P > 0.) x = x - P * rint(x / P);
        const double u = fmax(0., fabs(x) - st[2 + 2 * D + c]);
        e += 0.5 * st[2 + D + c] * u * u;
    }
    return e;
}

template <int D>
__device__ __forceinline__ void mbar_load_sample(const upk_mbar_samples_t& X, long long n, double (&v)[D ? D : 1], double& E) {
    v[0] = 0.;
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = (double)X.values[(size_t)n * D + c];
    E = X.energy ? X.energy[n] : 0.;
}

inline unsigned sample_blocks(long long n) { return (unsigned)((n + MBAR_BLOCK - 1) / MBAR_BLOCK); }
inline int launch_status() { return (int)hipGetLastError(); }
inline bool launch_args_ok(const upk_mbar_states_t* S, const upk_mbar_samples_t* X) {
    return S && X && S->d >= 0 && S->d <= UPK_MBAR_MAX_DIM && S->n_state >= 1 && X->n >= 1 && S->beta && (S->d == 0 || (S->rows && X->values)) &&
           (X->n + MBAR_BLOCK - 1) / MBAR_BLOCK <= 0x7fffffffll;
}

#define MBAR_DISPATCH(KERNEL, GRID, ...)                                                                                              \
    switch (S->d) {                                                                                                                   \
    case 0: hipLaunchKernelGGL(KERNEL<0>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 3: hipLaunchKernelGGL(KERNEL<3>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 5: hipLaunchKernelGGL(KERNEL<5>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 6: hipLaunchKernelGGL(KERNEL<6>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    case 7: hipLaunchKernelGGL(KERNEL<7>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                  \
    default: hipLaunchKernelGGL(KERNEL<8>, dim3(GRID), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, __VA_ARGS__); break;                 \
    }
static_assert(UPK_MBAR_MAX_DIM == 8, "MBAR_DISPATCH lists d = 0 .. 8");

// ---- host side -----------------------------------------------------------------------------------------------------------------------
struct MbarRefusal { char text[256]; };
#define MBAR_REFUSE(...) do { MbarRefusal r_; snprintf(r_.text, sizeof(r_.text), __VA_ARGS__); throw r_; } while (0)

template <class T>
bool all_finite(const T* p, size_t n, size_t* where) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite((double)p[i])) { *where = i; return false; }
    return true;
}

// every refusal of upside_hip_mbar; nothing here touches the device
inline void mbar_check(const upk_mbar_problem_t& P) {
    size_t at = 0;
    if (P.d < 0 || P.d > UPK_MBAR_MAX_DIM) MBAR_REFUSE("mbar: d = %d, at most %d CVs are supported (and d >= 0)", P.d, UPK_MBAR_MAX_DIM);
    if (P.n_state < 1) MBAR_REFUSE("mbar: n_state = %d, at least one state is needed", P.n_state);
    if (P.n_sample < 1) MBAR_REFUSE("mbar: n_sample = %lld, at least one sample is needed", P.n_sample);
    if (P.n_sample > ((1ll << 62) - 1) / P.n_state) MBAR_REFUSE("mbar: n_sample x n_state = %lld x %d is not below 2^62", P.n_sample, P.n_state);
    if (!P.beta || !P.n_k || !P.f) MBAR_REFUSE("mbar: beta, n_k and f must be given");
    if (P.d > 0 && (!P.values || !P.rows || !P.periods)) MBAR_REFUSE("mbar: values, rows and periods must be given when d > 0");
    if (P.has_target && (!P.log_w || !P.f_target)) MBAR_REFUSE("mbar: a target state needs log_w and f_target");
    if (!(P.tol >= 0.) || !std::isfinite(P.tol)) MBAR_REFUSE("mbar: tol must be finite and not negative");
    if (P.max_iter < 1) MBAR_REFUSE("mbar: max_iter = %d, at least one iteration is needed", P.max_iter);
    long long total = 0; bool any = false;
    for (int k = 0; k < P.n_state; ++k) {
        if (P.n_k[k] < 0) MBAR_REFUSE("mbar: n_k[%d] = %lld is negative", k, P.n_k[k]);
        if (P.n_k[k] > P.n_sample - total) MBAR_REFUSE("mbar: the sample counts n_k add up to more than n_sample = %lld", P.n_sample);
        total += P.n_k[k]; any = any || P.n_k[k] > 0;
    }
    if (!any) MBAR_REFUSE("mbar: no state has samples (every n_k is 0)");
    if (total != P.n_sample) MBAR_REFUSE("mbar: the sample counts n_k add up to %lld, n_sample is %lld", total, P.n_sample);
    if (!all_finite(P.beta, (size_t)P.n_state, &at)) MBAR_REFUSE("mbar: beta[%zu] is not finite", at);
    if (P.f0 && !all_finite(P.f0, (size_t)P.n_state, &at)) MBAR_REFUSE("mbar: f0[%zu] is not finite", at);
    if (P.has_target && !std::isfinite(P.beta_target)) MBAR_REFUSE("mbar: the target's beta is not finite");
    const size_t d = (size_t)P.d;
    for (size_t c = 0; c < d; ++c) {
        if (!std::isfinite(P.periods[c])) MBAR_REFUSE("mbar: periods[%zu] is not finite", c);
        if (P.periods[c] < 0.) MBAR_REFUSE("mbar: periods[%zu] is negative (0 = not periodic)", c);
    }
    for (int t = 0; t < (P.has_target && P.row_target && d ? 2 : 1); ++t) {
        const float* rows = t ? P.row_target : P.rows;
        const size_t n_row = t ? 1 : (size_t)P.n_state;
        const char* who = t ? "the target's row" : "rows";
        if (!d) break;
        if (!all_finite(rows, n_row * 3 * d, &at)) MBAR_REFUSE("mbar: %s: state %zu, entry %zu is not finite", who, at / (3 * d), at % (3 * d));
        for (size_t k = 0; k < n_row; ++k)
            for (size_t c = 0; c < d; ++c) {
                if (rows[k * 3 * d + d + c] < 0.f) MBAR_REFUSE("mbar: %s: spring_const of state %zu, CV %zu is negative", who, k, c);
                if (rows[k * 3 * d + 2 * d + c] < 0.f) MBAR_REFUSE("mbar: %s: flat_width of state %zu, CV %zu is negative", who, k, c);
            }
    }
    if (d && !all_finite(P.values, (size_t)P.n_sample * d, &at)) MBAR_REFUSE("mbar: values: sample %zu, CV %zu is not finite", at / d, at % d);
    if (P.energy && !all_finite(P.energy, (size_t)P.n_sample, &at)) MBAR_REFUSE("mbar: energy[%zu] is not finite", at);
}

inline void hip_ok(hipError_t e, const char* what) { if (e != hipSuccess) MBAR_REFUSE("mbar: %s: %s", what, hipGetErrorString(e)); }
inline void upk_ok(int code, const char* what) { if (code) MBAR_REFUSE("mbar: %s: launch failed (%d: %s)", what, code, code < 9000 ? hipGetErrorString((hipError_t)code) : "bad arguments"); }

struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    void alloc(size_t bytes, const char* what) { hip_ok(hipMalloc(&p, bytes ? bytes : 8), what); }
    template <class T> T* as() const { return (T*)p; }
};
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

}  // namespace mbar
}  // namespace up

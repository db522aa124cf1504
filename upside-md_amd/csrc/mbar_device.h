// What kernels_mbar.hip (the iteration), kernels_mbar_gram.hip (the Gram pass), kernels_mbar_boot.hip (the bootstrap batch) and
// kernels_series.hip (statistical inefficiency; the host side only) share.  Device: the reduced energy of a sample under a staged state,
// the staging of a tile of states, the workgroup maximum, the denominator pass and the free-energy pass, the per-d dispatch.  Host: the
// refusals, the staged problem of the three MBAR solves and the guarded entry of every *_solve.  One statement of each.
#pragma once
#include "cv_device.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
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

// the next tile of states, k0 .. k0 + nt - 1 of S, into tile by the whole workgroup, slot 0 of state k from a[k]; returns nt <= MBAR_TILE
template <int D>
__device__ __forceinline__ int mbar_stage_tile(const upk_mbar_states_t& S, int k0, const double* __restrict__ a, double* __restrict__ tile) {
    constexpr int W = mbar_state_doubles<D>();
    const int tid = threadIdx.x, nt = min(MBAR_TILE, S.n_state - k0);
    __syncthreads();      // (the previous tile has been read)
    for (int i = tid; i < nt * W; i += MBAR_BLOCK) { const int l = i / W, j = i - l * W; mbar_stage_state<D>(S, k0 + l, a[k0 + l], tile + l * W, j); }
    __syncthreads();
    return nt;
}

// states k0 .. k0 + MBAR_FE - 1 into st, one lane per double; states past the last are clamped to it.  Slot 0 is a[k], or 0. (a not read)
template <int D, bool WITH_A>
__device__ __forceinline__ void mbar_stage_fe(const upk_mbar_states_t& S, int k0, const double* __restrict__ a, double (*st)[mbar_state_doubles<D>()]) {
    constexpr int W = mbar_state_doubles<D>();
    const int tid = threadIdx.x;
    if (tid < MBAR_FE * W) { const int l = tid / W, j = tid - l * W, k = min(k0 + l, S.n_state - 1); mbar_stage_state<D>(S, k, WITH_A ? a[k] : 0., st[l], j); }
}
static_assert(MBAR_FE * mbar_state_doubles<UPK_MBAR_MAX_DIM>() <= MBAR_BLOCK, "one lane stages one double of the free-energy tile");

// the largest of v[j] over the workgroup, for every j; every lane receives it
template <int K>
__device__ __forceinline__ void mbar_block_max(double (&v)[K], double (*part)[MBAR_FE]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double w = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w = fmax(w, __shfl_xor(w, o, 64));
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = part[0][k];
#pragma unroll
        for (int w = 1; w < CV_WAVES; ++w) t = fmax(t, part[w][k]);
        v[k] = t;
    }
}

// denom[n] = logsumexp_{l : a[l] > -inf} (a[l] - u_l(n)) of the sample of this lane: the body of k_mbar_denominator and of
// k_mbar_boot_denominator, which differ in where a and denom point.  blockIdx.x counts the blocks of samples.
template <int D>
__device__ __forceinline__ void mbar_denominator_body(const upk_mbar_states_t& S, const upk_mbar_samples_t& X, const double* __restrict__ a,
                                                      double* __restrict__ denom) {
    constexpr int W = mbar_state_doubles<D>();
    __shared__ double tile[MBAR_TILE * W];
    const long long n_raw = (long long)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    const long long n = n_raw < X.n ? n_raw : X.n - 1;      // (a lane past the end repeats the last sample and stores nothing)
    double v[D ? D : 1], E;
    mbar_load_sample<D>(X, n, v, E);
    double m = -INFINITY, sum = 0.;
    for (int pass = 0; pass < 2; ++pass)
        for (int k0 = 0; k0 < S.n_state; k0 += MBAR_TILE) {
            const int nt = mbar_stage_tile<D>(S, k0, a, tile);
            for (int l = 0; l < nt; ++l) {
                const double* __restrict__ st = tile + l * W;
                if (st[0] == -INFINITY) continue;      // N_l = 0
                const double x = st[0] - st[1] * mbar_energy<D>(v, E, st, S);
                if (pass == 0) m = fmax(m, x); else sum += exp(x - m);
            }
        }
    if (n_raw < X.n) denom[n] = m + log(sum);
}

// one walk of a lane over its samples tid, tid + 256, ... ascending: PASS 0 takes the maxima m of the terms, PASS 1 adds exp(term - m) to s.
// Two walks written out, not one loop over a runtime pass: that loop costs k_mbar_free_energy 17 to 24 VGPRs and a wave of occupancy.
template <int D, bool COUNTED, int PASS>
__device__ __forceinline__ void mbar_free_energy_walk(const upk_mbar_states_t& S, const upk_mbar_samples_t& X, const unsigned short* __restrict__ counts,
                                                      const double* __restrict__ log_count, const double* __restrict__ denom,
                                                      const double (*st)[mbar_state_doubles<D>()], double (&m)[MBAR_FE], double (&s)[MBAR_FE]) {
    for (long long n = threadIdx.x; n < X.n; n += MBAR_BLOCK) {
        int c = 0;
        if constexpr (COUNTED) { c = counts[n]; if (!c) continue; }
        double v[D ? D : 1], E;
        mbar_load_sample<D>(X, n, v, E);
        const double dn = denom[n];
        double lc = 0.;
        if constexpr (COUNTED) lc = log_count[c];
#pragma unroll
        for (int l = 0; l < MBAR_FE; ++l) {
            double x = -(st[l][1] * mbar_energy<D>(v, E, st[l], S)) - dn;
            if constexpr (COUNTED) x = lc + x;
            if constexpr (PASS == 0) m[l] = fmax(m[l], x); else s[l] += exp(x - m[l]);
        }
    }
}

// f[k] = -logsumexp_n (-u_k(n) - denom[n]) for the MBAR_FE states of workgroup blockIdx.x; COUNTED: over the samples with a count
// c(n) > 0, each term plus ln c(n) = log_count[c(n)].  The body of k_mbar_free_energy and of k_mbar_boot_free_energy
template <int D, bool COUNTED>
__device__ __forceinline__ void mbar_free_energy_body(const upk_mbar_states_t& S, const upk_mbar_samples_t& X, const unsigned short* __restrict__ counts,
                                                      const double* __restrict__ log_count, const double* __restrict__ denom, double* __restrict__ f) {
    constexpr int W = mbar_state_doubles<D>();
    __shared__ double st[MBAR_FE][W];
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double partm[CV_WAVES][MBAR_FE];
    const int k0 = blockIdx.x * MBAR_FE;
    mbar_stage_fe<D, false>(S, k0, nullptr, st);
    __syncthreads();
    double m[MBAR_FE], s[MBAR_FE];
#pragma unroll
    for (int l = 0; l < MBAR_FE; ++l) { m[l] = -INFINITY; s[l] = 0.; }
    mbar_free_energy_walk<D, COUNTED, 0>(S, X, counts, log_count, denom, st, m, s);
    mbar_block_max<MBAR_FE>(m, partm);
    mbar_free_energy_walk<D, COUNTED, 1>(S, X, counts, log_count, denom, st, m, s);
    block_sum<MBAR_FE>(s, part);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int l = 0; l < MBAR_FE; ++l) if (k0 + l < S.n_state) f[k0 + l] = -(m[l] + log(s[l]));
    }
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

inline void require_device() {      // (the guarded entry names the entry point)
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) MBAR_REFUSE("mbar: no HIP device (this library has no CPU path)");
}

struct DeviceBuffer {
    void* p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    void alloc(size_t bytes, const char* what) { hip_ok(hipMalloc(&p, bytes ? bytes : 8), what); }
    void upload(hipStream_t s, const void* src, size_t bytes, const char* what) {
        alloc(bytes, what); if (bytes) hip_ok(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s), what);
    }
    template <class T> T* as() const { return (T*)p; }
};
struct Stream {
    hipStream_t s = nullptr;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

// the leading fields that upk_mbar_gram_problem_t and upk_mbar_boot_problem_t share with upk_mbar_problem_t, for mbar_check: the samples
// and the states are refused by one statement.  The caller adds tol, max_iter, f0 and f (which is only tested against NULL)
template <class Problem>
upk_mbar_problem_t as_mbar_problem(const Problem& P) {
    upk_mbar_problem_t Q{};
    Q.n_sample = P.n_sample; Q.n_state = P.n_state; Q.d = P.d; Q.values = P.values; Q.energy = P.energy; Q.beta = P.beta; Q.rows = P.rows;
    Q.n_k = P.n_k; Q.periods = P.periods;
    return Q;
}

// the samples and the states of a checked problem (any of the three problem structs) on the device, once, and the stream of the solve
struct StagedProblem {
    Stream st;
    DeviceBuffer values, energy, beta, rows;
    upk_mbar_states_t S{};
    upk_mbar_samples_t X{};
    template <class Problem>
    explicit StagedProblem(const Problem& P) {
        require_device();
        const size_t N = (size_t)P.n_sample, K = (size_t)P.n_state, d = (size_t)P.d;
        hip_ok(hipStreamCreate(&st.s), "hipStreamCreate");
        if (d) values.upload(st.s, P.values, N * d * sizeof(float), "copy of values");
        if (P.energy) energy.upload(st.s, P.energy, N * sizeof(double), "copy of energy");
        beta.upload(st.s, P.beta, K * sizeof(double), "copy of beta");
        if (d) rows.upload(st.s, P.rows, K * 3 * d * sizeof(float), "copy of rows");
        S.d = P.d; S.n_state = P.n_state; S.beta = beta.as<double>(); S.rows = rows.as<float>();
        for (size_t c = 0; c < d; ++c) S.period[c] = P.periods[c];
        X.n = P.n_sample; X.values = values.as<float>(); X.energy = energy.as<double>();
    }
};

// ln N_k, -inf for a state without samples
inline std::vector<double> log_sample_counts(const long long* n_k, int K) {
    std::vector<double> ln_n((size_t)K);
    for (int k = 0; k < K; ++k) ln_n[(size_t)k] = n_k[k] > 0 ? std::log((double)n_k[k]) : -INFINITY;
    return ln_n;
}
// a[k] = ln N_k + f[k] (f == NULL: f = 0), -inf for a state without samples whatever f[k] is
inline void log_counts_plus_f(const std::vector<double>& ln_n, const double* f, double* a) {
    for (size_t k = 0; k < ln_n.size(); ++k) a[k] = ln_n[k] == -INFINITY ? -INFINITY : ln_n[k] + (f ? f[k] : 0.);
}

// what every *_solve does around its body: 0, or 1 with the reason in message.  The checks and helpers above say "mbar: ..."; the
// message names the entry point that refused
template <class Body>
int guarded_entry(const char* entry, char* message, int message_len, Body body) {
    const bool say = message && message_len > 0;
    if (say) message[0] = 0;
    try {
        body();
        return 0;
    } catch (const MbarRefusal& r) {
        const bool shared = !strncmp(r.text, "mbar: ", 6);
        if (say && shared) snprintf(message, (size_t)message_len, "%s: %s", entry, r.text + 6);
        else if (say) snprintf(message, (size_t)message_len, "%s", r.text);
    } catch (const std::exception& e) {
        if (say) snprintf(message, (size_t)message_len, "%s: %s", entry, e.what());
    }
    return 1;
}

}  // namespace mbar
}  // namespace up

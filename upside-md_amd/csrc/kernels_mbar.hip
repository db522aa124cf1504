// gfx950 kernels and host driver of MBAR (Shirts & Chodera 2008) over the ladders this engine runs: K states ("windows") whose reduced
// energy of sample n is
//     u_k(n) = beta_k (E_n + sum_c 1/2 k_kc max(0, |wrap_c(v_nc - center_kc)| - w_kc)^2),   wrap_c(x) = x - P_c rint(x / P_c) for P_c > 0
// -- the cv_restraint bias (cv_harmonic_response / cv_wrap of cv_device.h, restated here in fp64 with a general period) on the
// recorded float32 CV bits v_n, plus an optional unbiased energy E_n.  d = 0 with E_n is a temperature ladder.  No force pass is
// needed: the bias depends on the recorded numbers alone.  One self-consistent iteration from f is
//     D_n  = logsumexp_{l : N_l > 0} (ln N_l + f_l - u_l(n))          k_mbar_denominator
//     f'_k = -logsumexp_n (-u_k(n) - D_n),  every k                   k_mbar_free_energy
//     f'   = f' - f'_0                                                 host (K doubles per iteration)
// Everything is fp64.  Every logsumexp takes its EXACT maximum first (a pass of its own over the same expression) and then sums
// exp(x - max), so a state 1e5 kT away contributes exp(-1e5) = 0 and neither overflows nor gives a NaN.  No atomics, and every sum
// has ONE order, so two runs give the same bits:
//   - k_mbar_denominator: one lane owns one sample (its d values and E_n stay in registers) and walks the states 0, 1, ... ascending.
//     The states are staged in LDS in tiles of UPK_MBAR_STATE_TILE as doubles [a_l = ln N_l + f_l | beta_l | center | k | w]; all
//     lanes read the same state, a broadcast.  a_l = -inf marks N_l = 0 and is skipped (uniform over the workgroup).  No cross-lane
//     reduction.
//   - k_mbar_free_energy: one workgroup owns UPK_MBAR_FE_TILE consecutive states, so a sample read serves that many; lane t takes
//     samples t, t + 256, ... ascending; the workgroup's maximum first, then the sum, combined by block_sum of cv_device.h (the
//     butterfly of every CV kernel, unchanged).  States past the last are clamped to it and not stored.
//   - k_mbar_log_weights: ln w_n = -u_t(n) - D_n + f_t of a target state, one lane per sample.
// The kernels are instantiated for d = 0 .. UPK_MBAR_MAX_DIM so that a sample's values are registers.  The first two are
// mbar_denominator_body and mbar_free_energy_body of mbar_device.h, which the bootstrap's kernels (kernels_mbar_boot.hip) call as well.
// upk_mbar_solve is the host side: argument checks (every refusal returns before any device call), one copy of the samples to the
// device, the iteration, the outputs.
#include "mbar_device.h"

using namespace up;
using namespace up::mbar;

namespace {

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_denominator(upk_mbar_states_t S, upk_mbar_samples_t X, const double* __restrict__ a,
                                                                  double* __restrict__ denom) {
    mbar_denominator_body<D>(S, X, a, denom);
}

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_free_energy(upk_mbar_states_t S, upk_mbar_samples_t X, const double* __restrict__ denom,
                                                                  double* __restrict__ f) {
    mbar_free_energy_body<D, false>(S, X, nullptr, nullptr, denom, f);
}

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_log_weights(upk_mbar_states_t S, upk_mbar_samples_t X, const double* __restrict__ denom,
                                                                  const double* __restrict__ f_target, double* __restrict__ log_w) {
    constexpr int W = mbar_state_doubles<D>();
    __shared__ double st[W];
    const int tid = threadIdx.x;
    if (tid < W) mbar_stage_state<D>(S, 0, 0., st, tid);
    __syncthreads();
    const long long n = (long long)blockIdx.x * MBAR_BLOCK + tid;
    if (n >= X.n) return;
    double v[D ? D : 1], E;
    mbar_load_sample<D>(X, n, v, E);
    log_w[n] = -(st[1] * mbar_energy<D>(v, E, st, S)) - denom[n] + f_target[0];
}

}  // namespace

extern "C" int upk_mbar_denominator(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* a, double* denom) {
    if (!launch_args_ok(S, X) || !a || !denom) return 9401;
    MBAR_DISPATCH(k_mbar_denominator, sample_blocks(X->n), *S, *X, a, denom)
    return launch_status();
}
extern "C" int upk_mbar_free_energy(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* denom, double* f) {
    if (!launch_args_ok(S, X) || !denom || !f) return 9402;
    MBAR_DISPATCH(k_mbar_free_energy, (unsigned)((S->n_state + MBAR_FE - 1) / MBAR_FE), *S, *X, denom, f)
    return launch_status();
}
extern "C" int upk_mbar_log_weights(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* denom,
                                    const double* f_target, double* log_w) {
    if (!launch_args_ok(S, X) || !denom || !f_target || !log_w) return 9403;
    MBAR_DISPATCH(k_mbar_log_weights, sample_blocks(X->n), *S, *X, denom, f_target, log_w)
    return launch_status();
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
namespace {

void mbar_run(const upk_mbar_problem_t& P) {
    mbar_check(P);
    StagedProblem staged(P);      // the samples and the states go to the device once
    const upk_mbar_states_t& S = staged.S; const upk_mbar_samples_t& X = staged.X; Stream& st = staged.st;
    const int K = P.n_state, d = P.d;
    const size_t N = (size_t)P.n_sample;
    DeviceBuffer a, f_dev, denom, tbeta, trow, tf, lw;
    a.alloc(K * sizeof(double), "a"); f_dev.alloc(K * sizeof(double), "f"); denom.alloc(N * sizeof(double), "denominators");

    std::vector<double> f(K, 0.), fn(K), av(K);
    const std::vector<double> ln_n = log_sample_counts(P.n_k, K);
    if (P.f0) for (int k = 0; k < K; ++k) f[k] = P.f0[k];
    auto denominators = [&]() {
        log_counts_plus_f(ln_n, f.data(), av.data());
        hip_ok(hipMemcpyAsync(a.p, av.data(), K * sizeof(double), hipMemcpyHostToDevice, st.s), "copy of f");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");      // (av is pageable and rewritten by the next iteration)
        upk_ok(upk_mbar_denominator(st.s, &S, &X, a.as<double>(), denom.as<double>()), "denominator pass");
    };
    int it = 0; double delta = INFINITY;
    while (it < P.max_iter) {
        denominators();
        upk_ok(upk_mbar_free_energy(st.s, &S, &X, denom.as<double>(), f_dev.as<double>()), "free-energy pass");
        hip_ok(hipMemcpyAsync(fn.data(), f_dev.p, K * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of f");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
        const double f0 = fn[0];
        delta = 0.;
        for (int k = 0; k < K; ++k) { fn[k] -= f0; const double dk = std::fabs(fn[k] - f[k]); if (!(dk <= delta)) delta = dk; }      // (a NaN is kept)
        f.swap(fn); ++it;
        if (delta < P.tol) break;
    }
    // the denominators of the returned f: D and the target's weights belong to it
    if (P.denominators || P.has_target) denominators();
    if (P.has_target) {
        std::vector<float> zero(3 * (size_t)(d ? d : 1), 0.f);
        tbeta.alloc(sizeof(double), "target"); hip_ok(hipMemcpyAsync(tbeta.p, &P.beta_target, sizeof(double), hipMemcpyHostToDevice, st.s), "copy of the target");
        trow.alloc(3 * (size_t)(d ? d : 1) * sizeof(float), "target");
        hip_ok(hipMemcpyAsync(trow.p, P.row_target && d ? P.row_target : zero.data(), 3 * (size_t)(d ? d : 1) * sizeof(float), hipMemcpyHostToDevice, st.s), "copy of the target");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
        tf.alloc(sizeof(double), "target"); lw.alloc(N * sizeof(double), "log-weights");
        upk_mbar_states_t T = S; T.n_state = 1; T.beta = tbeta.as<double>(); T.rows = trow.as<float>();
        upk_ok(upk_mbar_free_energy(st.s, &T, &X, denom.as<double>(), tf.as<double>()), "free-energy pass of the target");
        upk_ok(upk_mbar_log_weights(st.s, &T, &X, denom.as<double>(), tf.as<double>(), lw.as<double>()), "log-weights");
        hip_ok(hipMemcpyAsync(P.log_w, lw.p, N * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of log_w");
        hip_ok(hipMemcpyAsync(P.f_target, tf.p, sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of f_target");
    }
    if (P.denominators) hip_ok(hipMemcpyAsync(P.denominators, denom.p, N * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of D");
    hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
    for (int k = 0; k < K; ++k) P.f[k] = f[k];
    if (P.n_iter) *P.n_iter = it;
    if (P.last_delta) *P.last_delta = delta;
}

}  // namespace

extern "C" int upk_mbar_solve(const upk_mbar_problem_t* P, char* message, int message_len) {
    return guarded_entry("mbar", message, message_len, [&] {
        if (!P) MBAR_REFUSE("mbar: no problem given");
        mbar_run(*P);
    });
}
extern "C" int upk_mbar_state_tile(void) { return MBAR_TILE; }
extern "C" int upk_mbar_fe_tile(void) { return MBAR_FE; }

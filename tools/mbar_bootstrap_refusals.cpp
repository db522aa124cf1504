// Stand-alone driver of the host side of upside_hip_mbar_bootstrap (upk_mbar_boot_solve of csrc/kernels_mbar_boot.hip: argument checks
// and staging) for a sanitizer build: `make -C upside-md_amd/csrc mbar_boot_sanitize` compiles that file's host code and this file with
// -fsanitize=address,undefined and runs the program.  It walks every refusal and nothing else: each returns before any device call,
// so the program stays on the CPU whatever the machine holds (a good call after refusals is checked by tests/test_gpu_mbar_bootstrap.py).
#include "../include/upside_hip_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int n_bad = 0;
static void expect(const upk_mbar_boot_problem_t& P, const char* what, const char* fragment) {
    char msg[256];
    const int rc = upk_mbar_boot_solve(&P, msg, (int)sizeof(msg));
    const bool ok = rc == 1 && strstr(msg, fragment) && !strncmp(msg, "mbar_bootstrap: ", 16);
    printf("%-38s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}

int main() {
    const int K = 3, d = 2, B = 4, J = 2; const long long N = 30;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<float> values(N * d, 0.5f), rows(K * 3 * d, 1.f);
    std::vector<double> energy(N, -1.), beta(K, 1.), periods(d, 0.), f0(K, 0.), f_boot(B * K), cols(B * J), delta(B), lognum(J * N, -1.);
    std::vector<long long> n_k = {10, 10, 10};
    std::vector<int> origin(N), n_iter(B);
    for (long long n = 0; n < N; ++n) origin[n] = (int)(n % K);      // interleaved: sample n was drawn from state n mod K
    std::vector<unsigned short> counts(B * N, 1);
    counts[2 * N + 0] = 3; counts[2 * N + 3] = 0; counts[2 * N + 6] = 0;      // replicate 2: state 0 resampled within itself
    lognum[5] = -INFINITY;      // weight 0: allowed
    upk_mbar_boot_problem_t G{};
    G.n_sample = N; G.n_state = K; G.d = d; G.values = values.data(); G.energy = energy.data(); G.beta = beta.data(); G.rows = rows.data();
    G.n_k = n_k.data(); G.periods = periods.data(); G.state_of_sample = origin.data(); G.n_replicate = B; G.counts = counts.data(); G.tol = 0.;
    G.max_iter = 3; G.f0 = f0.data(); G.n_column = J; G.log_numerator = lognum.data(); G.workspace_bytes = 0; G.f_boot = f_boot.data();
    G.column_boot = cols.data(); G.n_iter = n_iter.data(); G.last_delta = delta.data();

    // its own refusals
    { auto P = G; P.n_replicate = 0; expect(P, "no replicate", "at least one replicate"); }
    { auto P = G; P.n_replicate = -3; expect(P, "a negative number of replicates", "n_replicate = -3"); }
    { auto P = G; P.counts = nullptr; expect(P, "counts missing", "counts and state_of_sample must be given"); }
    { auto P = G; P.state_of_sample = nullptr; expect(P, "state_of_sample missing", "counts and state_of_sample must be given"); }
    { auto P = G; P.f_boot = nullptr; expect(P, "f_boot missing", "f_boot must be given"); }
    { auto P = G; auto o = origin; o[N - 1] = K; P.state_of_sample = o.data(); expect(P, "the last origin above K - 1", "state_of_sample[29] = 3 is outside 0 .. 2"); }
    { auto P = G; auto o = origin; o[0] = -1; P.state_of_sample = o.data(); expect(P, "a negative origin", "state_of_sample[0] = -1"); }
    { auto P = G; std::vector<long long> c = {15, 15, 0}; P.n_k = c.data(); expect(P, "an origin without samples", "names a state without samples (n_k[2] = 0)"); }
    { auto P = G; auto o = origin; o[0] = 1; P.state_of_sample = o.data(); expect(P, "origins that do not add up", "names state 0 for 9 samples, n_k[0] is 10"); }
    { auto P = G; auto c = counts; c[3 * N + 29] = 0; P.counts = c.data(); expect(P, "the last replicate one short", "replicate 3: the counts of state 2 add up to 9, n_k[2] is 10"); }
    { auto P = G; auto c = counts; c[0] = 0; c[1] = 2; P.counts = c.data(); expect(P, "a count moved between states", "replicate 0: the counts of state 0 add up to 9"); }
    { auto P = G; auto c = counts; c[N + 4] = 65535; P.counts = c.data(); expect(P, "a count of 65535 too many", "replicate 1: the counts of state 1 add up to 65544"); }
    { auto P = G; P.n_column = -1; expect(P, "n_column below 0", "n_column = -1 is negative"); }
    { auto P = G; P.log_numerator = nullptr; expect(P, "columns without log_numerator", "log_numerator and column_boot must be given"); }
    { auto P = G; P.column_boot = nullptr; expect(P, "columns without column_boot", "log_numerator and column_boot must be given"); }
    { auto P = G; auto x = lognum; x[J * N - 1] = nan; P.log_numerator = x.data(); expect(P, "the last column entry not a number", "column 1, sample 29 is not a number"); }
    { auto P = G; auto x = lognum; x[N] = INFINITY; P.log_numerator = x.data(); expect(P, "a column entry +inf", "column 1, sample 0 is +inf"); }
    { auto P = G; auto x = f0; x[1] = nan; P.f0 = x.data(); expect(P, "f0 not a number", "f0[1] is not finite"); }
    { auto P = G; auto x = f0; x[2] = INFINITY; P.f0 = x.data(); expect(P, "f0 infinite", "f0[2] is not finite"); }
    { auto P = G; P.workspace_bytes = 8 * N - 1; expect(P, "a workspace below one replicate", "do not fit the workspace of 239 bytes"); }
    { auto P = G; P.workspace_bytes = UPK_MBAR_GRAM_MAX_WORKSPACE + 1; expect(P, "a workspace above the limit", "at most 536870912"); }
    // those it shares with upside_hip_mbar, reached through it
    { auto P = G; P.d = 9; expect(P, "d above 8", "at most 8"); }
    { auto P = G; P.d = -1; expect(P, "d below 0", "at most 8"); }
    { auto P = G; P.n_state = 0; expect(P, "no state", "at least one state"); }
    { auto P = G; P.n_sample = 0; expect(P, "no sample", "at least one sample"); }
    { auto P = G; P.n_sample = 1ll << 61; expect(P, "N x K at 2^62", "2^62"); }
    { auto P = G; P.beta = nullptr; expect(P, "beta missing", "must be given"); }
    { auto P = G; P.values = nullptr; expect(P, "values missing", "must be given"); }
    { auto P = G; P.tol = -1.; expect(P, "tol below 0", "tol"); }
    { auto P = G; P.tol = nan; expect(P, "tol not a number", "tol"); }
    { auto P = G; P.max_iter = 0; expect(P, "no iteration", "max_iter"); }
    { auto P = G; auto c = n_k; c[1] = -1; c[2] = 21; P.n_k = c.data(); expect(P, "a negative count n_k", "negative"); }
    { auto P = G; std::vector<long long> c(K, 0); P.n_k = c.data(); expect(P, "every n_k 0", "no state has samples"); }
    { auto P = G; auto c = n_k; c[2] = 9; P.n_k = c.data(); expect(P, "n_k below n_sample", "add up"); }
    { auto P = G; auto b = beta; b[2] = INFINITY; P.beta = b.data(); expect(P, "beta not finite", "beta[2]"); }
    { auto P = G; auto x = periods; x[0] = -6.28; P.periods = x.data(); expect(P, "period negative", "negative"); }
    { auto P = G; auto r = rows; r[1 * 3 * d + d + 1] = -1.f; P.rows = r.data(); expect(P, "spring_const negative", "spring_const of state 1, CV 1"); }
    { auto P = G; auto v = values; v[N * d - 1] = INFINITY; P.values = v.data(); expect(P, "last value not finite", "sample 29, CV 1"); }
    { auto P = G; auto e = energy; e[N - 1] = nan; P.energy = e.data(); expect(P, "last energy not finite", "energy[29]"); }
    {   char msg[256]; const int rc = upk_mbar_boot_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-38s %s: %s\n", "no problem", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    {   char msg[8]; auto P = G; P.n_replicate = 0; const int rc = upk_mbar_boot_solve(&P, msg, (int)sizeof(msg));      // a short message buffer is not overrun
        printf("%-38s rc %d: '%s'\n", "message buffer of 8 bytes", rc, msg); if (rc != 1 || strlen(msg) != 7) ++n_bad; }
    if (upk_mbar_boot_chunk(1000, 8000) != 1 || upk_mbar_boot_chunk(1000, 7999) != 0 || upk_mbar_boot_chunk(1, UPK_MBAR_GRAM_MAX_WORKSPACE) != UPK_MBAR_BOOT_MAX_CHUNK ||
        upk_mbar_boot_chunk(0, 1024) != 0 || upk_mbar_boot_chunk((1ll << 26) + 1, UPK_MBAR_GRAM_MAX_WORKSPACE) != 0) { printf("upk_mbar_boot_chunk NOT AS EXPECTED\n"); ++n_bad; }
    printf(n_bad ? "%d UNEXPECTED\n" : "all refusals as expected\n", n_bad);
    return n_bad ? 1 : 0;
}

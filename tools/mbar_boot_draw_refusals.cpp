// Stand-alone driver of the host side of upside_hip_mbar_bootstrap_drawn and upside_hip_mbar_bootstrap_counts (upk_mbar_boot_solve_drawn
// and upk_mbar_boot_draw_solve of csrc/kernels_mbar_boot.hip: argument checks and staging) for a sanitizer build:
// `make -C upside-md_amd/csrc mbar_boot_draw_sanitize` compiles that file's host code and this file with -fsanitize=address,undefined
// and runs the program.  It walks every refusal and nothing else: each returns before any device call, so the program stays on the CPU
// whatever the machine holds (good calls after refusals are checked by tests/test_gpu_mbar_boot_draw.py).
#include "../include/upside_hip_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int n_bad = 0;
static void report(int rc, const char* msg, const char* entry, const char* what, const char* fragment) {
    const bool ok = rc == 1 && strstr(msg, fragment) && !strncmp(msg, entry, strlen(entry));
    printf("%-40s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}
static void expect(const upk_mbar_boot_problem_t& P, const upk_mbar_boot_draw_t& D, const char* what, const char* fragment) {
    char msg[256];
    report(upk_mbar_boot_solve_drawn(&P, &D, msg, (int)sizeof(msg)), msg, "mbar_bootstrap_drawn: ", what, fragment);
}
struct CountsCall {
    int n_state; const long long* n_k; long long n_sample; const int* origin; long long n_replicate;
};
static void expect(const CountsCall& C, const upk_mbar_boot_draw_t& D, const char* what, const char* fragment) {
    char msg[256];
    report(upk_mbar_boot_draw_solve(C.n_state, C.n_k, C.n_sample, C.origin, C.n_replicate, &D, msg, (int)sizeof(msg)), msg, "mbar_bootstrap_counts: ", what, fragment);
}

int main() {
    const int K = 3, d = 2, B = 4, J = 2; const long long N = 30;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<float> values(N * d, 0.5f), rows(K * 3 * d, 1.f);
    std::vector<double> energy(N, -1.), beta(K, 1.), periods(d, 0.), f0(K, 0.), f_boot(B * K), cols(B * J), delta(B), lognum(J * N, -1.);
    std::vector<long long> n_k = {10, 10, 10}, block = {1, 4, 100};
    std::vector<int> origin(N), n_iter(B);
    for (long long n = 0; n < N; ++n) origin[n] = (int)(n % K);      // interleaved: sample n was drawn from state n mod K
    std::vector<unsigned short> counts(B * N, 1);
    upk_mbar_boot_problem_t G{};
    G.n_sample = N; G.n_state = K; G.d = d; G.values = values.data(); G.energy = energy.data(); G.beta = beta.data(); G.rows = rows.data();
    G.n_k = n_k.data(); G.periods = periods.data(); G.state_of_sample = origin.data(); G.n_replicate = B; G.counts = nullptr; G.tol = 0.;
    G.max_iter = 3; G.f0 = f0.data(); G.n_column = J; G.log_numerator = lognum.data(); G.workspace_bytes = 0; G.f_boot = f_boot.data();
    G.column_boot = cols.data(); G.n_iter = n_iter.data(); G.last_delta = delta.data();
    upk_mbar_boot_draw_t D{};
    D.seed = (1ull << 40) + 3; D.block = block.data(); D.first_replicate = 0; D.counts_out = counts.data();

    // ---- upk_mbar_boot_solve_drawn: what concerns the draw
    { auto Q = D; auto b = block; b[0] = 0; Q.block = b.data(); expect(G, Q, "a block of no sample", "block[0] = 0"); }
    { auto Q = D; auto b = block; b[2] = -7; Q.block = b.data(); expect(G, Q, "a negative block", "block[2] = -7"); }
    { auto Q = D; Q.first_replicate = -1; expect(G, Q, "a negative first replicate", "first_replicate = -1"); }
    { auto Q = D; Q.first_replicate = 1ll << 32; expect(G, Q, "a first replicate at 2^32", "first_replicate = 4294967296"); }
    { auto Q = D; Q.first_replicate = (1ll << 32) - 3; expect(G, Q, "replicates that reach 2^32", "a replicate index must stay below 2^32"); }
    { auto P = G; P.counts = counts.data(); expect(P, D, "counts next to a draw", "none may be given"); }
    { auto P = G; P.state_of_sample = nullptr; expect(P, D, "state_of_sample missing", "state_of_sample must be given"); }
    // what it shares with upside_hip_mbar_bootstrap
    { auto P = G; P.n_replicate = 0; expect(P, D, "no replicate", "at least one replicate"); }
    { auto P = G; P.n_replicate = -3; expect(P, D, "a negative number of replicates", "n_replicate = -3"); }
    { auto P = G; P.f_boot = nullptr; expect(P, D, "f_boot missing", "f_boot must be given"); }
    { auto P = G; auto o = origin; o[N - 1] = K; P.state_of_sample = o.data(); expect(P, D, "the last origin above K - 1", "state_of_sample[29] = 3 is outside 0 .. 2"); }
    { auto P = G; auto o = origin; o[0] = -1; P.state_of_sample = o.data(); expect(P, D, "a negative origin", "state_of_sample[0] = -1"); }
    { auto P = G; std::vector<long long> c = {15, 15, 0}; P.n_k = c.data(); expect(P, D, "an origin without samples", "names a state without samples (n_k[2] = 0)"); }
    { auto P = G; auto o = origin; o[0] = 1; P.state_of_sample = o.data(); expect(P, D, "origins that do not add up", "names state 0 for 9 samples, n_k[0] is 10"); }
    { auto P = G; P.n_column = -1; expect(P, D, "n_column below 0", "n_column = -1 is negative"); }
    { auto P = G; P.log_numerator = nullptr; expect(P, D, "columns without log_numerator", "log_numerator and column_boot must be given"); }
    { auto P = G; P.column_boot = nullptr; expect(P, D, "columns without column_boot", "log_numerator and column_boot must be given"); }
    { auto P = G; auto x = lognum; x[J * N - 1] = nan; P.log_numerator = x.data(); expect(P, D, "the last column entry not a number", "column 1, sample 29 is not a number"); }
    { auto P = G; auto x = lognum; x[N] = INFINITY; P.log_numerator = x.data(); expect(P, D, "a column entry +inf", "column 1, sample 0 is +inf"); }
    { auto P = G; auto x = f0; x[1] = nan; P.f0 = x.data(); expect(P, D, "f0 not a number", "f0[1] is not finite"); }
    { auto P = G; P.workspace_bytes = 8 * N - 1; expect(P, D, "a workspace below one replicate", "do not fit the workspace of 239 bytes"); }
    { auto P = G; P.workspace_bytes = UPK_MBAR_GRAM_MAX_WORKSPACE + 1; expect(P, D, "a workspace above the limit", "at most 536870912"); }
    { auto P = G; P.d = 9; expect(P, D, "d above 8", "at most 8"); }
    { auto P = G; P.n_state = 0; expect(P, D, "no state", "at least one state"); }
    { auto P = G; P.n_sample = 0; expect(P, D, "no sample", "at least one sample"); }
    { auto P = G; P.n_sample = 1ll << 61; expect(P, D, "N x K at 2^62", "2^62"); }
    { auto P = G; P.beta = nullptr; expect(P, D, "beta missing", "must be given"); }
    { auto P = G; P.tol = nan; expect(P, D, "tol not a number", "tol"); }
    { auto P = G; P.max_iter = 0; expect(P, D, "no iteration", "max_iter"); }
    { auto P = G; auto c = n_k; c[1] = -1; c[2] = 21; P.n_k = c.data(); expect(P, D, "a negative count n_k", "negative"); }
    { auto P = G; auto c = n_k; c[2] = 9; P.n_k = c.data(); expect(P, D, "n_k below n_sample", "add up"); }
    { auto P = G; auto v = values; v[N * d - 1] = INFINITY; P.values = v.data(); expect(P, D, "last value not finite", "sample 29, CV 1"); }
    {   char msg[256]; int rc = upk_mbar_boot_solve_drawn(nullptr, &D, msg, (int)sizeof(msg));
        report(rc, msg, "mbar_bootstrap_drawn: ", "no problem", "no problem or no draw");
        rc = upk_mbar_boot_solve_drawn(&G, nullptr, msg, (int)sizeof(msg));
        report(rc, msg, "mbar_bootstrap_drawn: ", "no draw", "no problem or no draw"); }
    {   char msg[8]; auto Q = D; Q.first_replicate = -1; const int rc = upk_mbar_boot_solve_drawn(&G, &Q, msg, (int)sizeof(msg));      // a short message buffer is not overrun
        printf("%-40s rc %d: '%s'\n", "message buffer of 8 bytes", rc, msg); if (rc != 1 || strlen(msg) != 7) ++n_bad; }

    // ---- upk_mbar_boot_draw_solve
    const CountsCall C{K, n_k.data(), N, origin.data(), B};
    { auto c = C; c.n_state = 0; expect(c, D, "no state", "at least one state"); }
    { auto c = C; c.n_sample = 0; expect(c, D, "no sample", "at least one sample"); }
    { auto c = C; c.n_k = nullptr; expect(c, D, "n_k missing", "n_k and counts_out must be given"); }
    { auto Q = D; Q.counts_out = nullptr; expect(C, Q, "counts_out missing", "n_k and counts_out must be given"); }
    { auto c = C; std::vector<long long> x = {10, -1, 21}; c.n_k = x.data(); expect(c, D, "a negative count n_k", "n_k[1] = -1 is negative"); }
    { auto c = C; c.n_sample = 31; expect(c, D, "n_k below n_sample", "add up to 30, n_sample is 31"); }
    { auto c = C; c.n_sample = 29; expect(c, D, "n_k above n_sample", "add up to more than n_sample = 29"); }
    { auto c = C; c.n_replicate = 0; expect(c, D, "no replicate", "at least one replicate"); }
    { auto c = C; c.n_replicate = -2; expect(c, D, "a negative number of replicates", "n_replicate = -2"); }
    { auto c = C; c.n_replicate = 1ll << 32; expect(c, D, "2^32 replicates", "a replicate index must stay below 2^32"); }
    { auto c = C; std::vector<long long> x = {(1ll << 26) + 1}; c.n_state = 1; c.n_k = x.data(); c.n_sample = x[0]; c.origin = nullptr;
      expect(c, D, "more than 2^26 samples", "at most 2^26 samples"); }
    { auto c = C; auto o = origin; o[N - 1] = K; c.origin = o.data(); expect(c, D, "the last origin above K - 1", "state_of_sample[29] = 3 is outside 0 .. 2"); }
    { auto c = C; auto o = origin; o[0] = 1; c.origin = o.data(); expect(c, D, "origins that do not add up", "names state 0 for 9 samples"); }
    { auto Q = D; auto b = block; b[1] = 0; Q.block = b.data(); expect(C, Q, "a block of no sample", "block[1] = 0"); }
    { auto Q = D; Q.first_replicate = -5; expect(C, Q, "a negative first replicate", "first_replicate = -5"); }
    { auto Q = D; Q.first_replicate = (1ll << 32) - 1; expect(C, Q, "replicates that reach 2^32", "a replicate index must stay below 2^32"); }
    {   char msg[256]; const int rc = upk_mbar_boot_draw_solve(K, n_k.data(), N, nullptr, B, nullptr, msg, (int)sizeof(msg));
        report(rc, msg, "mbar_bootstrap_counts: ", "no draw", "no draw given"); }
    printf(n_bad ? "%d UNEXPECTED\n" : "all refusals as expected\n", n_bad);
    return n_bad ? 1 : 0;
}

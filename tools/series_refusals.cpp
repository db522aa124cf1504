// Stand-alone driver of the host side of upside_hip_series_inefficiency (upk_series_solve of csrc/kernels_series.hip: argument checks
// and staging) for a sanitizer build: `make -C upside-md_amd/csrc series_sanitize` compiles that file's host code and this file with
// -fsanitize=address,undefined and runs the program.  It walks every refusal and nothing else: each returns before any device call,
// so the program stays on the CPU whatever the machine holds (a good call after refusals is checked by tests/test_gpu_series.py).
#include "../include/upside_hip_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int n_bad = 0;
static void expect(const upk_series_problem_t& P, const char* what, const char* fragment) {
    char msg[256];
    const int rc = upk_series_solve(&P, msg, (int)sizeof(msg));
    const bool ok = rc == 1 && strstr(msg, fragment);
    printf("%-34s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}

int main() {
    const int K = 3, J = 2; const long long T = 40;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> a(K * T), g(K * J), mean(K * J), variance(K * J);
    for (size_t i = 0; i < a.size(); ++i) a[i] = std::sin(0.37 * (double)i);
    std::vector<long long> length = {40, 31, 40}, origin = {0, 7}, stop(K * J);
    upk_series_problem_t G{};
    G.n_series = K; G.stride = T; G.length = length.data(); G.a = a.data(); G.n_origin = J; G.origin = origin.data(); G.mintime = 3;
    G.max_lag = 20; G.g = g.data(); G.stop_lag = stop.data(); G.mean = mean.data(); G.variance = variance.data();

    { auto P = G; P.n_series = 0; expect(P, "no series", "at least one series"); }
    { auto P = G; P.n_origin = 0; expect(P, "no origin", "at least one origin"); }
    { auto P = G; P.mintime = 0; expect(P, "mintime below 1", "mintime = 0"); }
    { auto P = G; P.max_lag = 0; expect(P, "max_lag below 1", "max_lag = 0"); }
    { auto P = G; P.a = nullptr; expect(P, "a missing", "must be given"); }
    { auto P = G; P.length = nullptr; expect(P, "length missing", "must be given"); }
    { auto P = G; P.origin = nullptr; expect(P, "origin missing", "must be given"); }
    { auto P = G; P.g = nullptr; expect(P, "g missing", "must be given"); }
    { auto P = G; P.stop_lag = nullptr; expect(P, "stop_lag missing", "must be given"); }
    { auto P = G; P.stride = 1ll << 39; expect(P, "n_series x stride at 2^40", "2^40"); }      // (3 x 2^39 is above it; refused before a is read)
    { auto P = G; P.n_series = 1; P.stride = 1ll << 40; expect(P, "one series of 2^40", "2^40"); }
    { auto P = G; P.stride = 0; expect(P, "stride 0", "stride >= 1"); }
    { auto P = G; auto o = origin; o[0] = -1; P.origin = o.data(); expect(P, "a negative origin", "origin[0] = -1 is negative"); }
    { auto P = G; auto o = origin; o[1] = 0; P.origin = o.data(); expect(P, "equal origins", "origin[1] = 0 does not ascend"); }
    { auto P = G; auto o = origin; o[0] = 9; P.origin = o.data(); expect(P, "descending origins", "does not ascend"); }
    { auto P = G; auto l = length; l[1] = 0; P.length = l.data(); expect(P, "a length of 0", "length[1] = 0"); }
    { auto P = G; auto l = length; l[2] = 41; P.length = l.data(); expect(P, "a length above stride", "length[2] = 41"); }
    { auto P = G; auto x = a; x[K * T - 1] = nan; P.a = x.data(); expect(P, "last entry not a number", "series 2, entry 39 is not finite"); }
    { auto P = G; auto x = a; x[T + 30] = INFINITY; P.a = x.data(); expect(P, "last entry of a short series +inf", "series 1, entry 30 is not finite"); }
    {   char msg[256]; const int rc = upk_series_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-34s %s: %s\n", "no problem", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    {   char msg[8]; auto P = G; P.n_series = 0; const int rc = upk_series_solve(&P, msg, (int)sizeof(msg));      // a short message buffer is not overrun
        printf("%-34s rc %d: '%s'\n", "message buffer of 8 bytes", rc, msg); if (rc != 1 || strlen(msg) != 7) ++n_bad; }
    if (upk_series_lag_block() != UPK_SERIES_LAG_BLOCK || upk_series_piece() != UPK_SERIES_PIECE) { printf("accessors NOT AS EXPECTED\n"); ++n_bad; }
    printf(n_bad ? "%d UNEXPECTED\n" : "all refusals as expected\n", n_bad);
    return n_bad ? 1 : 0;
}

// Stand-alone driver of the host side of upside_hip_mbar and upside_hip_mbar_gram (upk_mbar_solve of csrc/kernels_mbar.hip and
// upk_mbar_gram_solve of csrc/kernels_mbar_gram.hip: argument checks and staging) for a
// sanitizer build: `make -C upside-md_amd/csrc mbar_sanitize` compiles the two files' host code and this file with
// -fsanitize=address,undefined and runs the program.  It walks every refusal and nothing else: each returns before any device call,
// so the program stays on the CPU whatever the machine holds (a good call after refusals is checked by tests/test_gpu_mbar.py).
#include "../include/upside_hip_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int n_bad = 0;
static void expect(const upk_mbar_problem_t& P, const char* what, const char* fragment) {
    char msg[256];
    const int rc = upk_mbar_solve(&P, msg, (int)sizeof(msg));
    const bool ok = rc == 1 && strstr(msg, fragment);
    printf("%-34s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}

static void expect_gram(const upk_mbar_gram_problem_t& P, const char* what, const char* fragment) {
    char msg[256];
    const int rc = upk_mbar_gram_solve(&P, msg, (int)sizeof(msg));
    const bool ok = rc == 1 && strstr(msg, fragment);
    printf("%-34s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}

int main() {
    const int K = 3, d = 2; const long long N = 30;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<float> values(N * d, 0.5f), rows(K * 3 * d, 1.f), row_t(3 * d, 1.f);
    std::vector<double> energy(N, -1.), beta(K, 1.), periods(d, 0.), f0(K, 0.), f(K), D(N), lw(N);
    std::vector<long long> n_k = {10, 10, 10};
    double f_t = 0., delta = 0.; int n_iter = 0;
    upk_mbar_problem_t G{};
    G.n_sample = N; G.n_state = K; G.d = d; G.values = values.data(); G.energy = energy.data(); G.beta = beta.data(); G.rows = rows.data();
    G.n_k = n_k.data(); G.periods = periods.data(); G.tol = 0.; G.max_iter = 3; G.f0 = f0.data(); G.has_target = 1; G.beta_target = 1.;
    G.row_target = row_t.data(); G.f = f.data(); G.denominators = D.data(); G.log_w = lw.data(); G.f_target = &f_t; G.n_iter = &n_iter; G.last_delta = &delta;

    { auto P = G; P.d = 9; expect(P, "d above 8", "at most 8"); }
    { auto P = G; P.d = -1; expect(P, "d below 0", "at most 8"); }
    { auto P = G; P.n_state = 0; expect(P, "no state", "at least one state"); }
    { auto P = G; P.n_sample = 0; expect(P, "no sample", "at least one sample"); }
    { auto P = G; P.n_sample = 1ll << 61; expect(P, "N x K at 2^62", "2^62"); }
    { auto P = G; P.beta = nullptr; expect(P, "beta missing", "must be given"); }
    { auto P = G; P.values = nullptr; expect(P, "values missing", "must be given"); }
    { auto P = G; P.log_w = nullptr; expect(P, "a target without log_w", "target"); }
    { auto P = G; P.tol = -1.; expect(P, "tol below 0", "tol"); }
    { auto P = G; P.tol = nan; expect(P, "tol not a number", "tol"); }
    { auto P = G; P.max_iter = 0; expect(P, "no iteration", "max_iter"); }
    { auto P = G; auto c = n_k; c[1] = -1; c[2] = 21; P.n_k = c.data(); expect(P, "a negative count", "negative"); }
    { auto P = G; std::vector<long long> c(K, 0); P.n_k = c.data(); expect(P, "every count 0", "no state has samples"); }
    { auto P = G; auto c = n_k; c[2] = 9; P.n_k = c.data(); expect(P, "counts below n_sample", "add up"); }
    { auto P = G; auto c = n_k; c[0] = 1ll << 62; P.n_k = c.data(); expect(P, "counts above n_sample", "add up"); }
    { auto P = G; auto b = beta; b[2] = INFINITY; P.beta = b.data(); expect(P, "beta not finite", "beta[2]"); }
    { auto P = G; auto x = f0; x[1] = nan; P.f0 = x.data(); expect(P, "f0 not finite", "f0[1]"); }
    { auto P = G; P.beta_target = nan; expect(P, "target beta not finite", "target"); }
    { auto P = G; auto x = periods; x[1] = nan; P.periods = x.data(); expect(P, "period not finite", "periods[1]"); }
    { auto P = G; auto x = periods; x[0] = -6.28; P.periods = x.data(); expect(P, "period negative", "negative"); }
    { auto P = G; auto r = rows; r[K * 3 * d - 1] = NAN; P.rows = r.data(); expect(P, "last row entry not finite", "not finite"); }
    { auto P = G; auto r = rows; r[1 * 3 * d + d + 1] = -1.f; P.rows = r.data(); expect(P, "spring_const negative", "spring_const of state 1, CV 1"); }
    { auto P = G; auto r = rows; r[2 * 3 * d + 2 * d] = -1.f; P.rows = r.data(); expect(P, "flat_width negative", "flat_width of state 2, CV 0"); }
    { auto P = G; auto r = row_t; r[3 * d - 1] = -1.f; P.row_target = r.data(); expect(P, "target flat_width negative", "target"); }
    { auto P = G; auto v = values; v[N * d - 1] = INFINITY; P.values = v.data(); expect(P, "last value not finite", "sample 29, CV 1"); }
    { auto P = G; auto e = energy; e[N - 1] = nan; P.energy = e.data(); expect(P, "last energy not finite", "energy[29]"); }
    {   char msg[256]; const int rc = upk_mbar_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-34s %s: %s\n", "no problem", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    {   char msg[8]; auto P = G; P.d = 9; const int rc = upk_mbar_solve(&P, msg, (int)sizeof(msg));      // a short message buffer is not overrun
        printf("%-34s rc %d: '%s'\n", "message buffer of 8 bytes", rc, msg); if (rc != 1 || strlen(msg) != 7) ++n_bad; }

    // ---- upside_hip_mbar_gram: its own refusals, and those it shares with upside_hip_mbar reached through it
    const int n_extra = 2;
    std::vector<double> fk(K, 0.1), log_extra(n_extra * N, -1.), Gm((K + n_extra) * (K + n_extra)), colsum(K + n_extra);
    log_extra[3] = -INFINITY;      // weight 0: allowed
    upk_mbar_gram_problem_t Q{};
    Q.n_sample = N; Q.n_state = K; Q.d = d; Q.values = values.data(); Q.energy = energy.data(); Q.beta = beta.data(); Q.rows = rows.data();
    Q.n_k = n_k.data(); Q.periods = periods.data(); Q.f = fk.data(); Q.n_extra = n_extra; Q.log_extra = log_extra.data(); Q.G = Gm.data();
    Q.colsum = colsum.data(); Q.denominators = D.data();
    { auto P = Q; P.n_extra = -1; expect_gram(P, "gram: n_extra below 0", "n_extra = -1"); }
    { auto P = Q; P.n_extra = 8192 - K + 1; expect_gram(P, "gram: M above 8192", "at most 8192"); }
    { auto P = Q; P.n_state = 8193; P.n_extra = 0; expect_gram(P, "gram: n_state above 8192", "at most 8192"); }
    { auto P = Q; P.n_state = 0; expect_gram(P, "gram: no state", "at least one state"); }
    { auto P = Q; P.colsum = nullptr; expect_gram(P, "gram: colsum missing", "colsum must be given"); }
    { auto P = Q; P.f = nullptr; expect_gram(P, "gram: f missing", "f must be given"); }
    { auto P = Q; P.log_extra = nullptr; expect_gram(P, "gram: log_extra missing", "log_extra must be given"); }
    { auto P = Q; auto x = fk; x[2] = nan; P.f = x.data(); expect_gram(P, "gram: f not a number", "f[2] is not finite"); }
    { auto P = Q; auto x = fk; x[0] = -INFINITY; P.f = x.data(); expect_gram(P, "gram: f infinite", "f[0] is not finite"); }
    { auto P = Q; auto x = log_extra; x[n_extra * N - 1] = nan; P.log_extra = x.data(); expect_gram(P, "gram: last log_extra not a number", "column 1, sample 29 is not a number"); }
    { auto P = Q; auto x = log_extra; x[N] = INFINITY; P.log_extra = x.data(); expect_gram(P, "gram: a log_extra +inf", "column 1, sample 0 is +inf"); }
    { auto P = Q; P.d = 9; expect_gram(P, "gram: d above 8", "at most 8"); }
    { auto P = Q; P.n_sample = 0; expect_gram(P, "gram: no sample", "at least one sample"); }
    { auto P = Q; auto c = n_k; c[2] = 9; P.n_k = c.data(); expect_gram(P, "gram: counts below n_sample", "add up"); }
    { auto P = Q; auto v = values; v[0] = NAN; P.values = v.data(); expect_gram(P, "gram: a value not finite", "sample 0, CV 0"); }
    { auto P = Q; auto r = rows; r[d] = -1.f; P.rows = r.data(); expect_gram(P, "gram: spring_const negative", "spring_const of state 0, CV 0"); }
    {   char msg[256]; const int rc = upk_mbar_gram_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-34s %s: %s\n", "gram: no problem", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    if (upk_mbar_gram_tile() != UPK_MBAR_GRAM_TILE || upk_mbar_gram_rows(K, 0) != 0 || upk_mbar_gram_rows(65, upk_mbar_gram_partial_bytes(65) + 128 * 8 * 33) != 32 || upk_mbar_gram_partial_bytes(4096) != 0 ||
        upk_mbar_gram_rows(8193, (size_t)1 << 30) != 0) { printf("gram accessors NOT AS EXPECTED\n"); ++n_bad; }
    printf(n_bad ? "%d UNEXPECTED\n" : "all refusals as expected\n", n_bad);
    return n_bad ? 1 : 0;
}

// Stand-alone driver of the host sides of upside_hip_metad_bias and upside_hip_metad_grid (upk_metad_bias_solve and upk_metad_grid_solve
// of csrc/kernels_metad.hip: argument checks and staging) for a sanitizer build: `make -C upside-md_amd/csrc metad_sanitize` compiles
// that file's host code and this file with -fsanitize=address,undefined and runs the program.  It walks every refusal and nothing
// else: each returns before any device call, so the program stays on the CPU whatever the machine holds (a good call after refusals
// is checked by tests/test_gpu_metad.py).
#include "../include/upside_hip_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int n_bad = 0;
static void report(int rc, const char* msg, const char* what, const char* fragment) {
    const bool ok = rc == 1 && strstr(msg, fragment);
    printf("%-40s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}
static void expect(const upk_metad_bias_problem_t& P, const char* what, const char* fragment) {
    char msg[256];
    report(upk_metad_bias_solve(&P, msg, (int)sizeof(msg)), msg, what, fragment);
    if (strncmp(msg, "metad_bias: ", 12)) { printf("    the message does not name metad_bias\n"); ++n_bad; }
}
static void expect(const upk_metad_grid_problem_t& P, const char* what, const char* fragment) {
    char msg[256];
    report(upk_metad_grid_solve(&P, msg, (int)sizeof(msg)), msg, what, fragment);
    if (strncmp(msg, "metad_grid: ", 12)) { printf("    the message does not name metad_grid\n"); ++n_bad; }
}

// the refusals about the hills, which the two entry points share
template <class Problem>
static void hills(const Problem& G, const std::vector<long long>& hill_start, const std::vector<float>& centers, const std::vector<float>& weights,
                  const std::vector<double>& sigma, const std::vector<double>& periods) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    { auto P = G; P.H.d = 0; expect(P, "d = 0", "d = 0"); }
    { auto P = G; P.H.d = 5; expect(P, "d = 5", "d = 5"); }
    { auto P = G; P.H.n_list = 0; expect(P, "no list", "n_list = 0"); }
    { auto P = G; P.H.hill_start = nullptr; expect(P, "hill_start missing", "must be given"); }
    { auto P = G; P.H.centers = nullptr; expect(P, "centers missing", "must be given"); }
    { auto P = G; P.H.weights = nullptr; expect(P, "weights missing", "must be given"); }
    { auto P = G; P.H.sigma = nullptr; expect(P, "sigma missing", "must be given"); }
    { auto P = G; P.H.periods = nullptr; expect(P, "periods missing", "must be given"); }
    { auto P = G; auto s = hill_start; s[0] = 1; P.H.hill_start = s.data(); expect(P, "hill_start not from 0", "hill_start[0] = 1"); }
    { auto P = G; auto s = hill_start; s[1] = s[2] + 1; P.H.hill_start = s.data(); expect(P, "hill_start descending", "hill_start[2] = 7 descends"); }
    { auto P = G; std::vector<long long> s = {0, (1ll << 24) + 1, (1ll << 24) + 1}; P.H.hill_start = s.data(); expect(P, "a list above 2^24 hills", "list 0 holds 16777217 hills"); }
    {   auto P = G; std::vector<long long> s(130);      // 129 lists of 2^24 hills reach 2^31; refused before centers is read
        for (size_t l = 0; l < s.size(); ++l) s[l] = (long long)l << 24;
        P.H.n_list = 129; P.H.hill_start = s.data(); expect(P, "2^31 hills in total", "fewer than 2^31"); }
    { auto P = G; auto s = sigma; s[1] = nan; P.H.sigma = s.data(); expect(P, "a sigma that is not a number", "sigma[1] is not finite"); }
    { auto P = G; auto s = sigma; s[0] = 0.; P.H.sigma = s.data(); expect(P, "sigma = 0", "sigma[0] = 0 is not positive"); }
    { auto P = G; auto s = sigma; s[1] = -0.5; P.H.sigma = s.data(); expect(P, "sigma < 0", "sigma[1] = -0.5 is not positive"); }
    { auto P = G; auto s = periods; s[0] = INFINITY; P.H.periods = s.data(); expect(P, "a period that is not finite", "periods[0] is not finite"); }
    { auto P = G; auto s = periods; s[1] = -1.; P.H.periods = s.data(); expect(P, "a negative period", "periods[1] is negative"); }
    { auto P = G; auto c = centers; c[2 * 4 + 1] = NAN; P.H.centers = c.data(); expect(P, "a centre that is not a number", "hill 4, CV 1 is not finite"); }
    { auto P = G; auto c = centers; c.back() = INFINITY; P.H.centers = c.data(); expect(P, "the last centre +inf", "hill 6, CV 1 is not finite"); }
    { auto P = G; auto w = weights; w[6] = NAN; P.H.weights = w.data(); expect(P, "a weight that is not a number", "weights[6] is not finite"); }
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // two lists of 5 and 2 hills in d = 2
    std::vector<long long> hill_start = {0, 5, 7};
    std::vector<float> centers(14), weights(7);
    for (size_t i = 0; i < centers.size(); ++i) centers[i] = (float)std::sin(0.7 * (double)i);
    for (size_t i = 0; i < weights.size(); ++i) weights[i] = 0.1f + 0.01f * (float)i;
    std::vector<double> sigma = {0.3, 0.2}, periods = {0., 6.25};
    upk_metad_hills_t H{};
    H.n_list = 2; H.d = 2; H.hill_start = hill_start.data(); H.centers = centers.data(); H.weights = weights.data(); H.sigma = sigma.data(); H.periods = periods.data();

    // ---- upside_hip_metad_bias
    std::vector<long long> point_start = {0, 3, 4}, n_visible = {0, 5, 2, 2};
    std::vector<double> points(8), V(4);
    for (size_t i = 0; i < points.size(); ++i) points[i] = std::cos(0.3 * (double)i);
    upk_metad_bias_problem_t B{};
    B.H = H; B.point_start = point_start.data(); B.points = points.data(); B.n_visible = n_visible.data(); B.V = V.data();
    hills(B, hill_start, centers, weights, sigma, periods);
    { auto P = B; P.point_start = nullptr; expect(P, "point_start missing", "must be given"); }
    { auto P = B; P.points = nullptr; expect(P, "points missing", "must be given"); }
    { auto P = B; P.V = nullptr; expect(P, "V missing", "must be given"); }
    { auto P = B; auto s = point_start; s[0] = 2; P.point_start = s.data(); expect(P, "point_start not from 0", "point_start[0] = 2"); }
    { auto P = B; auto s = point_start; s[2] = 2; P.point_start = s.data(); expect(P, "point_start descending", "point_start[2] = 2 descends"); }
    { auto P = B; std::vector<long long> s = {0, 1ll << 31, 1ll << 31}; P.point_start = s.data(); expect(P, "2^31 points", "fewer than 2^31"); }      // (refused before points is read)
    { auto P = B; auto x = points; x[7] = nan; P.points = x.data(); expect(P, "the last point not a number", "point 3, CV 1 is not finite"); }
    { auto P = B; auto v = n_visible; v[1] = -1; P.n_visible = v.data(); expect(P, "n_visible below 0", "n_visible[1] = -1"); }
    { auto P = B; auto v = n_visible; v[3] = 3; P.n_visible = v.data(); expect(P, "n_visible above the list", "n_visible[3] = 3, list 1 holds 2 hills"); }
    {   char msg[256]; const int rc = upk_metad_bias_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-40s %s: %s\n", "no problem (bias)", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    {   char msg[8]; auto P = B; P.H.n_list = 0; const int rc = upk_metad_bias_solve(&P, msg, (int)sizeof(msg));      // a short message buffer is not overrun
        printf("%-40s rc %d: '%s'\n", "message buffer of 8 bytes", rc, msg); if (rc != 1 || strlen(msg) != 7) ++n_bad; }

    // ---- upside_hip_metad_grid
    std::vector<int> n_axis = {3, 4};
    std::vector<double> axes = {-1., 0., 1., 0., 1.5, 3., 4.5}, scales = {1., -2.5}, V_last(2 * 12), lse(2 * 2 * 2);
    std::vector<long long> checkpoints = {0, 5, 1, 2};
    upk_metad_grid_problem_t G{};
    G.H = H; G.n_axis = n_axis.data(); G.axes = axes.data(); G.n_checkpoint = 2; G.checkpoints = checkpoints.data(); G.n_scale = 2; G.scales = scales.data();
    G.V_last = V_last.data(); G.lse = lse.data();
    hills(G, hill_start, centers, weights, sigma, periods);
    { auto P = G; P.n_axis = nullptr; expect(P, "n_axis missing", "must be given"); }
    { auto P = G; P.axes = nullptr; expect(P, "axes missing", "must be given"); }
    { auto P = G; P.checkpoints = nullptr; expect(P, "checkpoints missing", "must be given"); }
    { auto P = G; P.scales = nullptr; expect(P, "scales missing", "scales must be given"); }
    { auto P = G; P.lse = nullptr; expect(P, "lse missing with scales", "lse must be given exactly when"); }
    { auto P = G; P.n_scale = 0; expect(P, "lse given without scales", "lse must be given exactly when"); }
    { auto P = G; P.n_checkpoint = 0; expect(P, "no checkpoint", "n_checkpoint = 0"); }
    { auto P = G; P.n_scale = -1; expect(P, "n_scale = -1", "n_scale = -1"); }
    { auto P = G; P.n_scale = 9; expect(P, "n_scale = 9", "n_scale = 9"); }
    { auto P = G; auto n = n_axis; n[1] = 0; P.n_axis = n.data(); expect(P, "an axis without values", "n_axis[1] = 0"); }
    { auto P = G; std::vector<int> n = {2048, 2049}; P.n_axis = n.data(); expect(P, "G above 2^22", "more than 2^22 points"); }      // (refused before axes is read)
    { auto P = G; auto a = axes; a[6] = nan; P.axes = a.data(); expect(P, "the last axis value not a number", "axes[6] is not finite"); }
    { auto P = G; auto s = scales; s[1] = INFINITY; P.scales = s.data(); expect(P, "a scale that is not finite", "scales[1] is not finite"); }
    { auto P = G; auto c = checkpoints; c[0] = -1; P.checkpoints = c.data(); expect(P, "a checkpoint below 0", "checkpoint 0 of list 0 = -1"); }
    { auto P = G; auto c = checkpoints; c[3] = 3; P.checkpoints = c.data(); expect(P, "a checkpoint above the list", "checkpoint 1 of list 1 = 3, the list holds 2 hills"); }
    { auto P = G; auto c = checkpoints; c[2] = 2; c[3] = 1; P.checkpoints = c.data(); expect(P, "checkpoints descending", "checkpoint 1 of list 1 = 1 descends"); }
    { auto P = G; P.path = 3; expect(P, "path = 3", "path = 3"); }
    { auto P = G; P.H.d = 1; P.path = 2; expect(P, "the factorised path with d = 1", "path = 2 with d = 1"); }
    {   char msg[256]; const int rc = upk_metad_grid_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-40s %s: %s\n", "no problem (grid)", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    printf(n_bad ? "%d UNEXPECTED\n" : "all refusals as expected\n", n_bad);
    return n_bad ? 1 : 0;
}

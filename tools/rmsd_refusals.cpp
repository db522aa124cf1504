// Stand-alone driver of the host sides of upside_hip_frames_create and upside_hip_rmsd_matrix / _nearest / _count
// (upk_rmsd_frames_create and upk_rmsd_solve of csrc/kernels_rmsd.hip: argument checks and staging) for a sanitizer build:
// `make -C upside-md_amd/csrc rmsd_sanitize` compiles that file's host code and this file with -fsanitize=address,undefined and runs
// the program.  It walks every refusal and nothing else: each returns before any device call, so the program stays on the CPU whatever
// the machine holds (a good call after refusals, and the refusal of a device allocation that fails, are checked by
// tests/test_gpu_rmsd.py).  The frame sets are descriptions without device memory: the refusals read no more of a set.
#include "../include/upside_hip_kernels.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

static int n_bad = 0;
static void report(int rc, const char* msg, const char* what, const char* fragment) {
    const bool ok = rc == 1 && strstr(msg, fragment);
    printf("%-48s %s: %s\n", what, ok ? "refused" : "NOT REFUSED AS EXPECTED", msg);
    if (!ok) ++n_bad;
}
static void expect(const upk_rmsd_problem_t& P, const char* what, const char* fragment) {
    static const char* const entry[3] = {"rmsd_matrix: ", "rmsd_nearest: ", "rmsd_count: "};
    char msg[256];
    report(upk_rmsd_solve(&P, msg, (int)sizeof(msg)), msg, what, fragment);
    if (P.mode >= 0 && P.mode <= 2 && strncmp(msg, entry[P.mode], strlen(entry[P.mode]))) { printf("    the message does not name its entry point\n"); ++n_bad; }
}
static void expect_create(int n_atom, long long n_frame, const float* pos, upk_rmsd_frames_t** frames, const char* what, const char* fragment) {
    char msg[256];
    report(upk_rmsd_frames_create(n_atom, n_frame, pos, frames, msg, (int)sizeof(msg)), msg, what, fragment);
    if (strncmp(msg, "frames_create: ", 15)) { printf("    the message does not name frames_create\n"); ++n_bad; }
    if (frames && *frames) { printf("    a handle was returned\n"); ++n_bad; }
}

static upk_rmsd_frames_t described(int n_atom, long long n_frame) {
    upk_rmsd_frames_t F{};
    F.magic = UPK_RMSD_MAGIC; F.n_atom = n_atom; F.n_pad = (n_atom + 3) / 4 * 4; F.n_frame = n_frame;
    return F;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // ---- upside_hip_frames_create
    std::vector<float> pos(9 * 5 * 3);
    for (size_t i = 0; i < pos.size(); ++i) pos[i] = (float)std::sin(0.37 * (double)i) * 10.f;
    upk_rmsd_frames_t* h = nullptr;
    expect_create(5, 9, pos.data(), nullptr, "no place for the handle", "frames (the place");
    expect_create(5, 9, nullptr, &h, "pos missing", "pos must be given");
    expect_create(2, 9, pos.data(), &h, "n_atom = 2", "n_atom = 2");
    expect_create(5, 0, pos.data(), &h, "n_frame = 0", "n_frame = 0");
    expect_create(5, -3, pos.data(), &h, "n_frame = -3", "n_frame = -3");
    expect_create(1 << 20, 1ll << 20, pos.data(), &h, "2^40 coordinates and more", "is not below 2^40");      // (refused before pos is read)
    expect_create(3, (1ll << 40) / 9 + 1, pos.data(), &h, "just at 2^40 coordinates", "is not below 2^40");
    { auto x = pos; x[7 * 15 + 2 * 3 + 1] = nan; expect_create(5, 9, x.data(), &h, "a coordinate that is not a number", "frame 7, atom 2 is not finite"); }
    { auto x = pos; x.back() = INFINITY; expect_create(5, 9, x.data(), &h, "the last coordinate +inf", "frame 8, atom 4 is not finite"); }
    {   char msg[8]; const int rc = upk_rmsd_frames_create(2, 9, pos.data(), &h, msg, (int)sizeof(msg));      // a short message buffer is not overrun
        printf("%-48s rc %d: '%s'\n", "message buffer of 8 bytes", rc, msg); if (rc != 1 || strlen(msg) != 7) ++n_bad; }
    upk_rmsd_frames_free(nullptr);      // (no set: nothing happens)

    // ---- the three calls, on described sets of 20 frames of 5 and of 6 atoms
    upk_rmsd_frames_t A = described(5, 20), A6 = described(6, 20), dead = described(5, 20), H1 = described(5, 1ll << 20), H2 = described(5, 1ll << 20);
    dead.magic = 0;
    std::vector<double> out(400), dist(20);
    std::vector<long long> index(20), count(20);
    std::vector<int> ia(20), big(1 << 20, 0);
    for (int i = 0; i < 20; ++i) ia[i] = 19 - i;
    for (int mode = 0; mode < 3; ++mode) {
        upk_rmsd_problem_t G{};
        G.mode = mode; G.A = &A; G.B = &A; G.nA = 20; G.nB = 20; G.cutoff = 1.;
        if (mode == UPK_RMSD_MATRIX) G.out = out.data();
        if (mode == UPK_RMSD_NEAREST) { G.index = index.data(); G.dist = dist.data(); }
        if (mode == UPK_RMSD_COUNT) G.count = count.data();
        { auto P = G; P.A = nullptr; expect(P, "A missing", "A must be given"); }
        { auto P = G; P.B = nullptr; expect(P, "B missing", "B must be given"); }
        { auto P = G; P.A = &dead; expect(P, "A freed", "A is not a live frame set"); }
        { auto P = G; P.B = &dead; expect(P, "B freed", "B is not a live frame set"); }
        { auto P = G; P.B = &A6; expect(P, "different n_atom", "hold 5 atoms, those of B 6"); }
        { auto P = G; P.nA = 0; expect(P, "nA = 0", "nA = 0"); }
        { auto P = G; P.nB = -2; expect(P, "nB = -2", "nB = -2"); }
        { auto P = G; P.nA = 19; expect(P, "nA not the set's size without a list", "nA = 19 without an index list"); }
        { auto P = G; P.nB = 21; expect(P, "nB not the set's size without a list", "nB = 21 without an index list"); }
        { auto P = G; auto i = ia; i[3] = 20; P.ia = i.data(); expect(P, "ia above the set", "ia[3] = 20 is outside the set of 20 frames"); }
        { auto P = G; auto i = ia; i[19] = -1; P.ib = i.data(); expect(P, "ib below 0", "ib[19] = -1 is outside"); }
    }
    {   upk_rmsd_problem_t G{}; G.mode = UPK_RMSD_MATRIX; G.A = &A; G.B = &A; G.nA = 20; G.nB = 20;
        expect(G, "out missing", "out must be given");
        G.out = out.data();
        { auto P = G; P.A = &H1; P.B = &H2; P.nA = P.nB = 1ll << 20; expect(P, "2^40 entries of whole sets", "nA x nB = 1048576 x 1048576 is not below 2^40"); }
        { auto P = G; P.ia = big.data(); P.ib = big.data(); P.nA = P.nB = 1ll << 20; expect(P, "2^40 entries through index lists", "is not below 2^40"); } }
    {   upk_rmsd_problem_t G{}; G.mode = UPK_RMSD_NEAREST; G.A = &A; G.B = &A; G.nA = 20; G.nB = 20;
        { auto P = G; P.dist = dist.data(); expect(P, "index missing", "index must be given"); }
        { auto P = G; P.index = index.data(); expect(P, "dist missing", "dist must be given"); } }
    {   upk_rmsd_problem_t G{}; G.mode = UPK_RMSD_COUNT; G.A = &A; G.B = &A; G.nA = 20; G.nB = 20; G.cutoff = 1.;
        expect(G, "count missing", "count must be given");
        G.count = count.data();
        { auto P = G; P.cutoff = -0.5; expect(P, "cutoff < 0", "cutoff = -0.5"); }
        { auto P = G; P.cutoff = std::numeric_limits<double>::quiet_NaN(); expect(P, "a cutoff that is not a number", "must be finite and not negative"); }
        { auto P = G; P.cutoff = INFINITY; expect(P, "cutoff +inf", "must be finite and not negative"); } }
    {   upk_rmsd_problem_t G{}; G.mode = 7; expect(G, "mode = 7", "mode = 7"); }
    {   char msg[256]; const int rc = upk_rmsd_solve(nullptr, msg, (int)sizeof(msg));
        printf("%-48s %s: %s\n", "no problem", rc == 1 ? "refused" : "NOT REFUSED", msg); if (rc != 1) ++n_bad; }
    printf(n_bad ? "%d UNEXPECTED\n" : "all refusals as expected\n", n_bad);
    return n_bad ? 1 : 0;
}

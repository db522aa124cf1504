// Prints the plans of upside-md_amd/csrc/launch_plan.h as text, for tests/test_launch_plan.py.  No HIP, no GPU.
//   launch_plan_host QUERY name=value ...      UPPER-CASE names set fields of a hand-filled PlanSwitches, the others are the query's numbers
//   launch_plan_host env                       the fields of plan_switches(), read from the environment
//   launch_plan_host sweep                     the self-consistency sweep of the side-chain pair passes: one line per violation, then a count
#include "../upside-md_amd/csrc/launch_plan.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

static std::map<std::string, double> arg;
static double num(const char* k, double dflt = 0) { auto it = arg.find(k); return it == arg.end() ? dflt : it->second; }
static int I(const char* k, int dflt = 0) { return (int)num(k, dflt); }

#define SW_FIELDS(X) X(BATCH) X(GRAPH) X(ASYNC_PREPARE) X(FUSE) X(FUSE_BARRIERS) X(FUSE_THREADS) X(SKIN_SCALE) X(NBR_CAP) X(ADJ_CAP) X(SLOT_FACTOR) \
    X(SLOT_SPLIT) X(IG_WGS) X(IG_POLY) X(ROT_POLY) X(IG_UNSTAGED) X(ROT_UNSTAGED) X(PLB_UNSTAGED) X(PAIR2) X(ROT_SORT_BEADS) X(ROTAMER_ATOMIC) \
    X(MAX_ROTAMER_NODES) X(BP_CLUSTER) X(BP_CLUSTER_TEST_ABORT) X(BP_COMPACT) X(BP_LAYOUT) X(BP_ENERGY_TABLE) X(BP_LDS_MSG_KB) \
    X(NODE_PROB_IN_SOLVE) X(BACKBONE_LIST) X(BACKBONE_SKIN) X(BACKBONE_LIST_CAP)

static void print_rot(const char* tag, const RotPass& p) {
    printf("%s.fits=%d\n%s.packed=%d\n%s.poly=%d\n%s.staged=%d\n%s.tab_floats=%d\n%s.lds_bytes=%zu\n%s.grid_x=%d\n%s.lanes=%d\n", tag, p.fits, tag, p.packed, tag, p.poly,
           tag, p.staged, tag, p.tab_floats, tag, p.lds_bytes, tag, p.grid_x, tag, p.lanes);
}
static int sweep() {
    long n = 0, bad = 0;
    const int widths[3][2] = {{34, 105}, {40, 132}, {62, 260}};      // n_param, n_poly of the three shipped side-chain libraries
    const PlanSwitches sw;
    for (int S : {1, 3, 16, 17, 64, 256, 512, 4096}) for (auto& w : widths) for (int n_bead = 1; n_bead <= 8191; ++n_bead) {
        const RotShape r = {n_bead, 20, w[0], w[1], true};
        const bool pack = plan_bead_pack(sw, r);
        const RotPass e = plan_rot_energy(sw, r, S, pack), g = plan_rot_grad(sw, r, S, pack);
        const char* why = nullptr;
        if (g.fits && !g.staged && !pack) why = "gradient unstaged without bead_pack";
        else if (!e.fits || !g.fits) why = "does not fit";
        else if (e.lds_bytes > PLAN_PAIR_LDS || g.lds_bytes > PLAN_PAIR_LDS) why = "over budget";
        else if (pack && (e.staged || g.staged)) why = "bead_pack, but a pass stages its beads";
        else if (e.staged != g.staged) why = "passes disagree on staging";
        ++n;
        if (why && ++bad <= 20) printf("violation: S=%d n_bead=%d n_param=%d: %s\n", S, n_bead, w[0], why);
    }
    printf("cases=%ld\nviolations=%ld\n", n, bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string q = argv[1];
    PlanSwitches sw;
    if (q == "env") sw = plan_switches();
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        arg[std::string(argv[i], eq - argv[i])] = atof(eq + 1);
    }
#define SET(x) if (arg.count(#x)) sw.x = (decltype(sw.x))arg[#x];
    SW_FIELDS(SET)
    const int S = I("S", 1);
    if (q == "env") {
#define PRINT(x) printf(#x "=%.10g\n", (double)sw.x);
        SW_FIELDS(PRINT)
    } else if (q == "sweep") return sweep();
    else if (q == "engine") {
        const bool merged = plan_merged_launches(sw, S, I("n_atom"));
        printf("merged=%d\ngraph=%d\n", merged, plan_graph_replay(sw, merged, I("trace") != 0));
        printf("lanes=%d\nlanes_heavy=%d\nheavy_alone=%d\n", plan_fuse_lanes(sw, S, false), plan_fuse_lanes(sw, S, true), plan_heavy_op_alone(S, I("n")));
    } else if (q == "graph") {
        printf("skin=%g\nskin_side_chain=%g\ngacc=%d\ngacc_symmetric=%d\n", plan_skin_scale(sw, S, false), plan_skin_scale(sw, S, true), plan_gacc(false, S), plan_gacc(true, S));
        const int n_cu = I("n_cu", 256);
        printf("upkeep_block=%d\nlist_build_rows=%d\nrefine_rows=%d\n", plan_upkeep_block(S, n_cu, 1024), plan_list_build_rows(S, n_cu), plan_refine_rows(S, n_cu, I("n_rows", 1000)));
    } else if (q == "geometry") {
        const PairGeometry g = plan_pair_geometry(sw, S, I("rows"), I("lanes_per_row"), I("rows_per_full_wg"));
        printf("wgs_per_system=%d\nlanes=%d\n", g.wgs_per_system, g.lanes);
    } else if (q == "pair") {
        const PairShape g = {I("coverage") != 0, I("has_poly") != 0, I("n1"), I("n2"), I("cap1"), I("cap2"), I("n_type1"), I("n_type2"), I("n_param"), I("n_poly")};
        const PairTable t = plan_pair_table(sw, g, (size_t)num("extra"));
        printf("table=%d\ntab_floats=%d\nlds_bytes=%zu\n", t.table, t.tab_floats, t.lds_bytes);
        const PairPass f = plan_pair_forward(sw, g, I("side", 1), I("mode")), b = plan_pair_backward(sw, g, I("side", 1), I("d_other", 6));
        printf("fwd.table=%d\nfwd.packed=%d\nfwd.lds_bytes=%zu\nbwd.table=%d\nbwd.packed=%d\nbwd.lds_bytes=%zu\n", f.table, f.packed, f.lds_bytes, b.table, b.packed, b.lds_bytes);
        printf("passes_staged=%d\n", plan_passes_staged(sw, g, I("side", 1)));
    } else if (q == "rot") {
        const RotShape r = {I("n_bead"), I("n_type"), I("n_param"), I("n_poly"), I("has_poly", 1) != 0};
        const bool pack = plan_bead_pack(sw, r);
        printf("bead_pack=%d\n", pack);
        print_rot("energy", plan_rot_energy(sw, r, S, pack)); print_rot("grad", plan_rot_grad(sw, r, S, pack));
        printf("grad_poly_packed_staged=%d\n", plan_rot_form(sw, r, S, pack, true, true, true).staged);
        printf("grad_scalar_exact_bytes=%zu\n", plan_rot_form(PlanSwitches(), r, S, false, true, false, false).lds_bytes);   // what plan_bead_pack bounds
    } else if (q == "solve") {
        const int n_node = I("n_node");
        printf("slot_cap=%d\nadj_cap=%d\nslot_split=%d\nlayout_record=%d\n", plan_slot_cap(sw, n_node), plan_adj_cap(sw, n_node), plan_slot_split(sw, S, n_node), plan_layout_record(sw, S));
        const int C = plan_cluster_size(sw, (long)num("need"), (long)num("widest"), n_node, I("n_node1"), S, I("n_cu", 256));
        printf("C=%d\nper_launch=%d\ngrid_x=%d\n", C, plan_cluster_per_launch(I("n_cu", 256), C), plan_cluster_grid_x(I("n", S)));
    } else if (q == "form") {
        const MatrixForm f = plan_matrix_form(sw, S, I("merged") != 0, I("C", 1), I("one_bead") != 0, I("layout_record") != 0);
        printf("node_prob_in_solve=%d\np_prob=%d\nprefold=%d\n", f.node_prob_in_solve, f.p_prob, f.prefold);
    } else if (q == "bp") {
        const BpSolve p = plan_bp_solve(sw, I("n_node"), I("slot_cap"), I("have_rows", 1) != 0, I("layout_record") != 0);
        printf("refused=%d\nlds_base=%zu\nmsg_bytes=%zu\nmsg_floats=%d\ndense=%d\nlayout_launch=%d\nscratch_words=%d\nlayout_lds=%zu\n", p.refused, p.lds_base, p.msg_bytes,
               p.msg_floats, p.dense, p.layout_launch, p.scratch_words, p.layout_lds);
    } else return 2;
    return 0;
}

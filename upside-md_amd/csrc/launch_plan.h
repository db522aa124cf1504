// Launch policy: which code path a batch size, a CU's LDS and the side-chain library select.  Host only, plain C++17, no HIP: constants
// the formulas need, the UPSIDE_HIP_* switches that select a path or size a capacity (PlanSwitches), and pure functions of numbers.
// Launchers and nodes ask here and then launch or allocate; they keep no size comparison and no budget of their own.
// tests/launch_plan_host.cpp prints these plans without a GPU.
#pragma once
#include "env_switch.h"
#include <climits>
#include <cstddef>

// ---- kernel shapes the formulas depend on ------------------------------------------------------------------------------
#ifndef PG_LANES
#define PG_LANES 8      // lanes per row group of the pair passes (pair_walk)
#endif
#ifndef P2_LANES
#define P2_LANES 4      // (measured at 4096 systems: 8 lanes within 0.5 %, 16 lanes -4.5 %: the LDS bank conflicts of the partner gathers --
                        //  two thirds of the LDS-active cycles -- are not what bounds the passes)
#endif
#define PG_WALK_LDS_WORDS(n_rows) ((n_rows) + ((n_rows) + 1) / 2)   // 32-bit words of LDS behind stage_ranges
#ifndef PLR_ROWS
#define PLR_ROWS 256    // rows per workgroup of the list refine in a batch that fills the device
#endif
// Lanes per row of the list refine (LPR), per instance: the symmetric side-chain graph with 32-bit words, and everyone else's 16-bit
// words.  LPR lanes serve a row and 64 / LPR rows share a wavefront trip.  From tools/refine_groups.py (profiles/refine_groups_ab.txt) on
// the benchmark protein, trips per row at LPR 16 / 32: side-chain graph 2.10 / 2.10, hydrophobe coverage 1.65 / 1.67, hbond coverage
// 1.11 / 1.17, environment 1.72 / 1.67 -- the same trips, and 16 shares each of them and the per-set bookkeeping among four rows
// instead of two.  Measured at 4096 systems on one box, LPR 16 / 32: VALU instructions per launch 131.7 M / 140.5 M (16-bit words) and
// 180.5 M / 189.1 M (side-chain graph), time per launch 387 / 471 us and 675 / 681 us.  Against the two-rows-per-trip refine this
// replaces (one wavefront per row pair, 64 words of each per trip), alternating runs on one box: 16-bit words 159.4 M -> 126.5 M VALU
// instructions and 496 -> 411 us per launch, side-chain graph 223.9 M -> 180.5 M and 691 -> 672 us (its 32-bit lists are most of what
// the kernel moves: with the old body for that instance alone the benchmark lost a third of the gain).
#ifndef PLR_LPR_SYM
#define PLR_LPR_SYM 16
#endif
#ifndef PLR_LPR_W16
#define PLR_LPR_W16 16
#endif
#ifndef PLR_AHEAD
#define PLR_AHEAD 128   // list words per row that the refine keeps in flight for the next set of rows
#endif
#define BP_BLOCK 1024
#ifndef BP_NODE_STRIDE
#define BP_NODE_STRIDE 6      // (8 = one b128 + one b64 per node row: measured equal, and 6 leaves 7 KB more of the LDS to the inbox)
#endif
#define BP_NODE_ARRAYS 2      // node arrays of BP_NODE_STRIDE floats in the one-workgroup solve's LDS: probabilities, beliefs
#ifndef BPL_THREADS
#define BPL_THREADS 512
#endif
#define BPC_BLOCK 512   // 8 waves: 256 VGPRs per lane keep the three slot states + a 6x6 matrix out of scratch
enum { N_CLASS = 5 };   // residue-pair slot classes of the solve: 3x3, 3x6, 6x6, 1x1, 1xN

// ---- LDS budgets (a CU has 160 KB) ---------------------------------------------------------------------------------------
constexpr size_t PLAN_CU_LDS = 160 * 1024;            // the one-workgroup solve, beliefs + inbox: all of it (the kernel has no static LDS)
constexpr size_t PLAN_PAIR_LDS = 158 * 1024;          // the staged pair passes (table + elements + accumulators + row order)
constexpr size_t PLAN_BP_CLUSTER_LDS = 156 * 1024;    // a workgroup of the cluster solve
constexpr size_t PLAN_BP_BASE_LDS = 155 * 1024;       // node arrays of the one-workgroup solve: past this the solve is refused (9004)
constexpr size_t PLAN_BP_LAYOUT_LDS = 40 * 1024;      // a quarter of a CU: the layout launch runs four workgroups per CU
constexpr size_t PLAN_LIST_LDS = 150 * 1024;          // the other side's positions staged by the list build and the refine

// ---- switches -------------------------------------------------------------------------------------------------------------
// Every UPSIDE_HIP_* switch that selects a path or sizes a capacity, with its value when unset.
// Diagnostics, PLUGINS, HAMILTONIAN_BATCH and the RANK / WORLD / COMM family are read where they are used.
struct PlanSwitches {
    int BATCH = INT_MIN;          // unset: plan_merged_launches decides; else != 0
    int GRAPH = -1;               // < 0: follows the merged launches
    int ASYNC_PREPARE = 1, FUSE = 1, FUSE_BARRIERS = 0, FUSE_THREADS = 0;
    float SKIN_SCALE = 0.f;       // <= 0: plan_skin_scale decides
    int NBR_CAP = 512, ADJ_CAP = 256;
    float SLOT_FACTOR = 96.f;
    int SLOT_SPLIT = 0, IG_WGS = 256, IG_POLY = 1, ROT_POLY = 1, IG_UNSTAGED = 0, ROT_UNSTAGED = 0, PLB_UNSTAGED = 0, PAIR2 = 1;
    int ROT_SORT_BEADS = 1, ROTAMER_ATOMIC = 0, MAX_ROTAMER_NODES = 1024;
    int BP_CLUSTER = -1;          // 1 disables, > 1 forces
    int BP_CLUSTER_TEST_ABORT = 0, BP_COMPACT = 1;
    int BP_LAYOUT = -1;           // 0 / 1: layout record off / on; 2: on, with no scratch, so that every system is handed back to its solve (tests)
    int BP_ENERGY_TABLE = 0, BP_LDS_MSG_KB = 160, NODE_PROB_IN_SOLVE = 1;
    int BACKBONE_LIST = 1;
    float BACKBONE_SKIN = 3.f;
    int BACKBONE_LIST_CAP = 128;
};
inline const PlanSwitches& plan_switches() {      // read once per process
    static const PlanSwitches sw = [] {
        PlanSwitches s;
        s.BATCH = env_int("UPSIDE_HIP_BATCH", s.BATCH); s.GRAPH = env_int("UPSIDE_HIP_GRAPH", s.GRAPH);
        s.ASYNC_PREPARE = env_int("UPSIDE_HIP_ASYNC_PREPARE", s.ASYNC_PREPARE); s.FUSE = env_int("UPSIDE_HIP_FUSE", s.FUSE);
        s.FUSE_BARRIERS = env_int("UPSIDE_HIP_FUSE_BARRIERS", s.FUSE_BARRIERS); s.FUSE_THREADS = env_int("UPSIDE_HIP_FUSE_THREADS", s.FUSE_THREADS);
        s.NBR_CAP = env_int("UPSIDE_HIP_NBR_CAP", s.NBR_CAP); s.ADJ_CAP = env_int("UPSIDE_HIP_ADJ_CAP", s.ADJ_CAP);
        s.SLOT_SPLIT = env_int("UPSIDE_HIP_SLOT_SPLIT", s.SLOT_SPLIT); s.IG_WGS = env_int("UPSIDE_HIP_IG_WGS", s.IG_WGS);
        s.IG_POLY = env_int("UPSIDE_HIP_IG_POLY", s.IG_POLY); s.ROT_POLY = env_int("UPSIDE_HIP_ROT_POLY", s.ROT_POLY);
        s.IG_UNSTAGED = env_int("UPSIDE_HIP_IG_UNSTAGED", s.IG_UNSTAGED); s.ROT_UNSTAGED = env_int("UPSIDE_HIP_ROT_UNSTAGED", s.ROT_UNSTAGED);
        s.PLB_UNSTAGED = env_int("UPSIDE_HIP_PLB_UNSTAGED", s.PLB_UNSTAGED); s.PAIR2 = env_int("UPSIDE_HIP_PAIR2", s.PAIR2);
        s.ROT_SORT_BEADS = env_int("UPSIDE_HIP_ROT_SORT_BEADS", s.ROT_SORT_BEADS);
        s.ROTAMER_ATOMIC = env_int("UPSIDE_HIP_ROTAMER_ATOMIC", s.ROTAMER_ATOMIC);
        s.MAX_ROTAMER_NODES = env_int("UPSIDE_HIP_MAX_ROTAMER_NODES", s.MAX_ROTAMER_NODES);
        s.BP_CLUSTER = env_int("UPSIDE_HIP_BP_CLUSTER", s.BP_CLUSTER);
        s.BP_CLUSTER_TEST_ABORT = env_int("UPSIDE_HIP_BP_CLUSTER_TEST_ABORT", s.BP_CLUSTER_TEST_ABORT);
        s.BP_COMPACT = env_int("UPSIDE_HIP_BP_COMPACT", s.BP_COMPACT); s.BP_LAYOUT = env_int("UPSIDE_HIP_BP_LAYOUT", s.BP_LAYOUT);
        s.BP_ENERGY_TABLE = env_int("UPSIDE_HIP_BP_ENERGY_TABLE", s.BP_ENERGY_TABLE);
        s.BP_LDS_MSG_KB = env_int("UPSIDE_HIP_BP_LDS_MSG_KB", s.BP_LDS_MSG_KB);
        s.NODE_PROB_IN_SOLVE = env_int("UPSIDE_HIP_NODE_PROB_IN_SOLVE", s.NODE_PROB_IN_SOLVE);
        s.BACKBONE_LIST = env_int("UPSIDE_HIP_BACKBONE_LIST", s.BACKBONE_LIST);
        s.BACKBONE_LIST_CAP = env_int("UPSIDE_HIP_BACKBONE_LIST_CAP", s.BACKBONE_LIST_CAP);
        s.SKIN_SCALE = env_float("UPSIDE_HIP_SKIN_SCALE", s.SKIN_SCALE); s.SLOT_FACTOR = env_float("UPSIDE_HIP_SLOT_FACTOR", s.SLOT_FACTOR);
        s.BACKBONE_SKIN = env_float("UPSIDE_HIP_BACKBONE_SKIN", s.BACKBONE_SKIN);
        return s;
    }();
    return sw;
}

// ---- engine -----------------------------------------------------------------------------------------------------------------
// merged launches (kernels_batch.h) for batches that are chains of dependent launches rather than work: measured on one MI355X,
// system-steps/s with / without -- 56 residues: 1 system 3.79 k / 3.18 k, 8: 25.9 k / 23.1 k; 300 residues: 1 system 1.83 k / 1.69 k,
// 64: 56 k / 62 k, 4096: 149 k / 184 k (there the upkeep kernels want their own launch shapes and the side streams).
// UPSIDE_HIP_BATCH=1 / 0 forces them on / off.  Where they stop winning depends on the protein as much as on the count (a launch of a
// 20-residue system is latency at 64 systems still): with / without merged launches + graph replay, k system-steps/s --
//   20 residues: 64 systems 290 / 207, 128: 532 / 407, 256: 729 / 715, 512: 940 / 1111;  56 residues: 32: 127 / 97, 64: 227 / 184,
//   128: 407 / 357, 256: 571 / 612;  150 residues: 32: 56.5 / 51.1, 48: 79.1 / 74.0, 64: 81.5 / 85.8;  300 residues: 24: 31.7 / 31.2,
//   32: 35.6 / 35.0 (54.1 / 52.5 at the 7 A list), 64: 56.3 / 62.1
// -- up to 16 systems always, else while atoms x systems <= 24 000 and systems <= 160.
inline bool plan_merged_launches(const PlanSwitches& sw, int S, int n_atom) {
    if (sw.BATCH != INT_MIN) return sw.BATCH != 0;
    return S <= 16 || ((long)S * n_atom <= 24000 && S <= 160);
}
// UPSIDE_HIP_GRAPH: six MD steps replayed from a captured hipGraph.  Default: wherever launches are merged, where a step is a chain of ~17
// dependent launches and a graph node boundary is cheaper than an eager one (one / eight 56-residue systems: 193 / 223 against
// 201 / 233 us per step; one 300-residue system 465 against 474; 64 x 150 residues 716 against 689: off there).  With the merged launches:
// one stream; a multi-stream capture replays slower than it launches.
// fuse_trace: UPSIDE_HIP_FUSE_TRACE reads its clocks back after every flush, and a capturing stream cannot be synchronised.
inline bool plan_graph_replay(const PlanSwitches& sw, bool merged, bool fuse_trace) {
    return fuse_trace ? false : (sw.GRAPH >= 0 ? sw.GRAPH != 0 : merged);
}
// workgroup size of a fused launch: enough lanes for the per-element loops of a system (a few hundred to a few thousand items) in a
// small batch, several systems resident per CU in a large one
// (256-lane workgroups fill a CU eight at a time: worth it once there are systems for all of them -- 512 lanes against 256, k
//  system-steps/s: 300 residues x 256 149 / 142, x 1024 178 / 175, x 2048 equal, x 4096 186 / 187; 56 residues x 256 664 / 613,
//  x 512 893 / 846, x 2048 1069 / 1099)
inline int plan_fuse_lanes(const PlanSwitches& sw, int S, bool heavy) {
    const int forced = (sw.FUSE_THREADS % 64 || sw.FUSE_THREADS > 1024) ? 0 : sw.FUSE_THREADS;
    const int t = forced ? forced : (S >= 2048 ? 256 : (S >= 256 ? 512 : 1024));
    return heavy && t > 512 ? 512 : t;           // (the heavy instances are built for at most 512 lanes)
}
// a large batch, or a system whose other ops want all 1024 lanes, runs the register-hungry op (n elements) in a launch of its own: the
// ops around it keep the light instance (its occupancy, its workgroup size)
inline bool plan_heavy_op_alone(int S, int n) { return S >= 256 || n > 64; }

struct BackboneList { bool on; int cap; float skin; };
inline BackboneList plan_backbone_list(const PlanSwitches& sw, int n_residue) {
    return {n_residue > 128 && sw.BACKBONE_LIST != 0, n_residue < sw.BACKBONE_LIST_CAP ? n_residue : sw.BACKBONE_LIST_CAP, sw.BACKBONE_SKIN};
}

// ---- pair graphs --------------------------------------------------------------------------------------------------------------
// Width of the cached-list margin relative to the reference's 1 + 0.2*cutoff (interaction_graph.h:395): any margin
// gives the same in-range pairs, it only trades rebuild frequency against list length.  Here the residue-pair slots of
// the side-chain solve are cut from the cached list too, so a long list also makes every belief-propagation sweep
// longer.  Measured at 1024 x 300 residues, system-steps/s by scale: 1.8: 73 k, 1.4: 79 k, 1.0: 85.6 k, 0.8: 89.2 k,
// 0.6: 91.2 k, 0.45: 90.6 k (256 systems: 78.0 / 82.4 / 82.2 k at 1.0 / 0.6 / 0.45); with the straight-line list
// build 0.6: 92.3 k, 0.5: 93.8 k, 0.4: 93.4 k.
// (round 4: a batch of a few systems is a chain of launches, not work -- a longer list is cheap there and every rebuild lengthens the
//  chain: 1.5 x the reference's margin up to 16 systems; 56 residues, 1 / 8 systems: 4.97 k / 34.4 k against 4.88 k / 32.8 k system-steps/s
//  at 0.5, one 300-residue system 2.09 k against 1.99 k; 64 systems: 57 k against 62 k)
// (round 5: with 16-bit list words and the cheaper refine a longer list costs less: 4096 systems 215.4 k at 0.75 against 212.7 k at 0.5, four
//  alternating runs each on one box; 1024 and 256 systems no difference, 64 systems 0.5 still ahead by 0.6 %)
// (the side-chain graph keeps 0.5 there: its cached residue pairs are the solve's slots, and the slot matrices of pairs that are cached
//  but out of range lie between the active ones -- solve 4.98 -> 5.26 ms, pair energies 1.23 -> 1.35 ms at 0.75; with it at 0.5 and the
//  others at 0.75: 217.1 against 214.6 k on one box, 220.6 against 219.8 k on another)
inline float plan_skin_scale(const PlanSwitches& sw, int S, bool side_chain_graph) {
    if (sw.SKIN_SCALE > 0.f) return sw.SKIN_SCALE;
    if (S <= 16) return 1.5f;
    return (S <= 256 || side_chain_graph) ? 0.5f : 0.75f;
}
// cross-workgroup accumulators of the backward passes (from 256 systems on a system has one workgroup)
inline bool plan_gacc(bool symmetric, int S) { return !symmetric && S < 256; }

// launch geometry of an LDS-staged pair pass: workgroups per system and lanes per workgroup.  A large batch runs one
// 1024-lane workgroup (16 wavefronts = 128 rows in flight) per system; small batches spread a system over several smaller
// workgroups (each stages the system again, so only as many as it takes to give every CU work).
// lanes_per_row, rows_per_full_wg: PG_LANES and 128 for the 8-row batches of pair_walk, P2_LANES and 256 for the 16-row batches of pair2_walk.
struct PairGeometry { int wgs_per_system, lanes; };
inline PairGeometry plan_pair_geometry(const PlanSwitches& sw, int S, int n_rows, int lanes_per_row, int rows_per_full_wg) {
    const int target = sw.IG_WGS < 1 ? 256 : sw.IG_WGS;
    int bps = (target + S - 1) / S;
    // every workgroup stages the whole system (table, elements, row order): at least one batch of rows per wavefront of a
    // 1024-lane workgroup, i.e. 128 (256) rows each -- a single system is served by ~10 fat workgroups, not by 40 thin ones
    const int max_bps = (n_rows + rows_per_full_wg - 1) / rows_per_full_wg;
    if (bps > max_bps) bps = max_bps;
    if (bps < 1) bps = 1;
    const int rows_per_wg = (n_rows + bps - 1) / bps;
    const int t = ((rows_per_wg * lanes_per_row + 63) / 64) * 64;      // one batch per wavefront
    return {bps, t < 256 ? 256 : (t > 1024 ? 1024 : t)};
}
inline PairGeometry plan_pair_geometry(const PlanSwitches& sw, int S, int n_rows, bool packed) {
    return packed ? plan_pair_geometry(sw, S, n_rows, P2_LANES, 256) : plan_pair_geometry(sw, S, n_rows, PG_LANES, 128);
}

// what a pass of a two-sided graph stages: has_poly = a coverage graph with its per-interval polynomial table
struct PairShape { bool coverage, has_poly; int n1, n2, cap1, cap2, n_type1, n_type2, n_param, n_poly; };
enum PlanTable { PLAN_TABLE_NONE = 0, PLAN_TABLE_COEF = 1, PLAN_TABLE_POLY = 2 };
struct PairTable { PlanTable table; int tab_floats; size_t lds_bytes; };     // NONE: the list-walking kernels
// the polynomial table when it fits LDS next to the elements (and extra bytes), else the spline coefficients, else nothing fits
inline PairTable plan_pair_table(const PlanSwitches& sw, const PairShape& g, size_t extra) {
    const int n_max = g.n1 > g.n2 ? g.n1 : g.n2;
    for (int poly = 1; poly >= 0; --poly) {
        if (poly && (!sw.IG_POLY || !g.has_poly)) continue;
        const int tab_floats = g.n_type1 * g.n_type2 * (poly ? g.n_poly : g.n_param);
        const size_t bytes = ((size_t)((tab_floats + 3) & ~3) + (size_t)(g.n1 + g.n2) * 8 + PG_WALK_LDS_WORDS(n_max) + 4) * sizeof(float);
        // (the staged hit ranges are first | end << 16)
        if (bytes <= PLAN_PAIR_LDS && !sw.IG_UNSTAGED && n_max < 65536 && g.cap1 < 65536 && g.cap2 < 65536 && bytes + extra <= PLAN_PAIR_LDS)
            return {poly ? PLAN_TABLE_POLY : PLAN_TABLE_COEF, tab_floats, bytes};
    }
    return {PLAN_TABLE_NONE, 0, 0};
}
// a pass with its table; packed: the two-partners-per-lane form of the coverage graphs (UPSIDE_HIP_PAIR2=0: never).  lds_bytes: of the launch
struct PairPass { PlanTable table; bool packed; int tab_floats; size_t lds_bytes; };
inline PairPass plan_pair_forward(const PlanSwitches& sw, const PairShape& g, int side, int mode) {
    const PairTable t = plan_pair_table(sw, g, 0);
    const bool packed = t.table && g.coverage && mode == 0 && side != 3 && sw.PAIR2 && t.lds_bytes + 64 <= PLAN_PAIR_LDS;
    return {t.table, packed, t.tab_floats, t.lds_bytes + (packed ? 64 : 0)};
}
// d_other: accumulated components per element of the other side (BackwardOp::DO)
inline PairPass plan_pair_backward(const PlanSwitches& sw, const PairShape& g, int row_side, int d_other) {
    const int n_other = row_side == 1 ? g.n2 : g.n1;
    const size_t acc_bytes = 8 + (size_t)n_other * d_other * sizeof(unsigned long long);
    const PairTable t = plan_pair_table(sw, g, acc_bytes);
    if (t.table && g.coverage && sw.PAIR2) {                     // packed pass: + sentinel rows and the sites' sensitivities
        const size_t extra = 64 + (size_t)g.n1 * sizeof(float);
        const PairTable t2 = plan_pair_table(sw, g, acc_bytes + extra);
        if (t2.table) return {t2.table, true, t2.tab_floats, t2.lds_bytes + acc_bytes + extra};
    }
    return {t.table, false, t.tab_floats, t.lds_bytes + acc_bytes};
}
// do the pair passes of a graph all gather over the rows of row_side from staged LDS (then only that side's lists are kept up to date)?
inline bool plan_passes_staged(const PlanSwitches& sw, const PairShape& g, int row_side) {
    if (row_side != 1 && row_side != 2) return false;
    const int n_other = row_side == 1 ? g.n2 : g.n1;
    return plan_pair_table(sw, g, 0).table && plan_pair_table(sw, g, 8 + (size_t)n_other * 8 * sizeof(unsigned long long)).table;   // (an upper bound of the accumulators)
}
// rows of n_param entries per workgroup so that a slice's fixed-point image fits the LDS of the pair passes; n_slice 0: one row alone does not fit
struct TableSlices { int rows, n_slice; };
inline TableSlices plan_pd_table_slices(int n_rows, int n_param) {
    const size_t row_bytes = (size_t)(n_param > 0 ? n_param : 1) * sizeof(unsigned long long);
    const int fit = (int)(PLAN_PAIR_LDS / row_bytes);
    if (fit < 1 || n_rows < 1) return {0, 0};
    const int n_slice = (n_rows + fit - 1) / fit;
    return {(n_rows + n_slice - 1) / n_slice, n_slice};      // balanced slices
}

// Workgroup size of the list-upkeep kernels (rebuild test, list build) when they are launched on their own.  A batch that fills the
// device runs them on side streams next to the pair passes of the main stream, whose 1024-lane workgroups hold ~100 registers per lane
// and 55-106 KB of LDS: what a CU has left beside one of those is 4 wavefront slots and ~96 registers per SIMD -- room for workgroups of
// 256 lanes at <= 40 registers, none for one of 1024.  With 256 lanes the vector-bound list build and the memory-bound rebuild test run
// BESIDE the LDS-bound pair passes instead of taking turns with them at workgroup granularity (4096 systems: 214.8 -> 218.2 k system-steps/s,
// three alternating runs; the build alone +0.8 %; the slot-numbering kernel at 320 lanes as well: no further change; 1024 systems +0.9 %,
// 512 x 150 residues +0.4 %, 256 systems -1.4 %: from two systems per CU on).  Smaller batches keep the large workgroups: there a
// system's latency is what a step waits for.
inline int plan_upkeep_block(int S, int n_cu, int large) { return S >= 2 * n_cu ? 256 : large; }
// rows per workgroup of the list build: every workgroup stages the whole other side first, so more rows per workgroup amortise that copy
// (128 rows: +0.4 % of the benchmark at 4096 systems; 256 leaves too few workgroups per system: -0.4 %), while a small
// batch wants its few rebuilds spread over many workgroups (64 rows: +1 % at 1 and 64 systems)
inline int plan_list_build_rows(int S, int n_cu) { return S >= n_cu ? 128 : 64; }
inline bool plan_list_build_staged(const PlanSwitches& sw, size_t lds_bytes) { return lds_bytes <= PLAN_LIST_LDS && !sw.PLB_UNSTAGED; }
// rows per workgroup of the refine: every workgroup stages the other side again: few fat workgroups for a large batch, many small ones for
// a small one.  A wavefront takes a contiguous run of a quarter of them, 64 / LPR rows (a set) at a time.  A side of a few hundred rows
// (environment graph: 300): smaller workgroups, or one of its two would walk 256 rows, 64 per wavefront, while the other has 44
// (0.30 -> 0.24 ms with the two-rows-per-trip refine of round 5)
inline int plan_refine_rows(int S, int n_cu, int n_rows) {
    const int rows = S >= n_cu ? PLR_ROWS : (S >= 16 ? 64 : 16);
    return n_rows <= 512 && rows > 128 ? 128 : rows;
}

// ---- side-chain pair passes -------------------------------------------------------------------------------------------------
struct RotShape { int n_bead, n_type, n_param, n_poly; bool has_poly; };
// One pass (energy: want_acc false; gradient: true).  fits false: the interaction table is larger than LDS (error 9005).
// packed: the two-partners-per-lane gradient pass; staged false: beads read from the packed global rows (bead_pack).
struct RotPass { bool fits, packed, poly, staged; int tab_floats; size_t lds_bytes; int grid_x, lanes; };
inline RotPass plan_rot_form(const PlanSwitches& sw, const RotShape& r, int S, bool bead_pack, bool want_acc, bool poly, bool packed) {
    const int tab_floats = (r.n_type * (r.n_type + 1) / 2) * (poly ? r.n_poly : r.n_param);
    const size_t fixed = ((size_t)((tab_floats + 3) & ~3) + PG_WALK_LDS_WORDS(r.n_bead) + 4) * sizeof(float);
    size_t lds = fixed + (size_t)r.n_bead * (want_acc ? 20 : 8) * sizeof(float) + (packed ? 32 : 0);
    bool staged = true;
    if (lds > PLAN_PAIR_LDS || sw.ROT_UNSTAGED || bead_pack) { staged = false; lds = fixed; }   // (a system whose gradient pass needs the packed copy uses it in both passes)
    const bool fits = lds <= PLAN_PAIR_LDS && (staged || bead_pack);
    const PairGeometry g = plan_pair_geometry(sw, S, r.n_bead, packed);
    return {fits, packed, poly, staged, tab_floats, lds, g.wgs_per_system, g.lanes};
}
// packed global bead rows: only when table + beads exceed the LDS budget of the pair kernels (triangle table + beads + accumulators +
// row order).  tab + 22 n + 8 words is an upper bound of what plan_rot_form asks for the scalar gradient pass on the coefficient table,
// (tab + 3 & ~3) + 21.5 n + 4.5 words at most, the form that decides "does not fit": whenever that pass cannot stage its beads the rows exist.
inline bool plan_bead_pack(const PlanSwitches& sw, const RotShape& r) {
    return ((size_t)(r.n_type * (r.n_type + 1) / 2) * r.n_param + (size_t)r.n_bead * 22 + 8) * sizeof(float) > PLAN_PAIR_LDS || sw.ROT_UNSTAGED != 0;
}
// energy pass: the polynomial table when it fits LDS with the beads (UPSIDE_HIP_ROT_POLY=0: never), else the spline coefficients
// (the packed two-partners-per-lane form of THIS pass was built in round 3 and removed in round 6: the pass is bound by its scattered
//  pair-matrix stores, and 16 rows x 4 partners per store instruction touch 1.7x the cache lines of 8 rows x 8 partners: 1.45 against 1.26 ms)
inline RotPass plan_rot_energy(const PlanSwitches& sw, const RotShape& r, int S, bool bead_pack) {
    if (r.has_poly && sw.ROT_POLY) { const RotPass p = plan_rot_form(sw, r, S, bead_pack, false, true, false); if (p.fits && p.staged) return p; }
    return plan_rot_form(sw, r, S, bead_pack, false, false, false);
}
// gradient pass: packed with the polynomial table if it fits beside the accumulators, else packed with the spline coefficients, else scalar
inline RotPass plan_rot_grad(const PlanSwitches& sw, const RotShape& r, int S, bool bead_pack) {
    if (sw.PAIR2) for (int poly = 1; poly >= 0; --poly) {
        if (poly && !r.has_poly) continue;
        const RotPass p = plan_rot_form(sw, r, S, bead_pack, true, poly != 0, true);
        if (p.fits && p.staged) return p;
    }
    return plan_rot_form(sw, r, S, bead_pack, true, false, false);
}

// ---- side-chain solve -------------------------------------------------------------------------------------------------------
inline int plan_slot_cap(const PlanSwitches& sw, int n_node) {
    const long full = (long)n_node * (n_node - 1) / 2, want = (long)(n_node * sw.SLOT_FACTOR);
    const long cap = full < want ? full : want;
    return (int)(cap > 1 ? cap : 1);
}
inline int plan_adj_cap(const PlanSwitches& sw, int n_node) { const int n = n_node > 1 ? n_node : 1; return n < sw.ADJ_CAP ? n : sw.ADJ_CAP; }
// workgroups per system of the slot numbering: several while the device has CUs to spare, one when systems fill it
inline int plan_slot_split(const PlanSwitches& sw, int S, int n_node) {
    const int split = (sw.SLOT_SPLIT < 0 || sw.SLOT_SPLIT > 16) ? 0 : sw.SLOT_SPLIT;
    return split ? split : ((S <= 256 && n_node > 64) ? 4 : 1);
}
// the dense inbox layout as a launch of its own in front of the one-workgroup solve (k_rotamer_bp_layout) once the solves of a launch
// run in several rounds over the CUs (a solve owns a whole CU): UPSIDE_HIP_BP_LAYOUT=0 / 1 forces the record off / on (tests)
inline bool plan_layout_record(const PlanSwitches& sw, int S) { return sw.BP_LAYOUT >= 1 || (sw.BP_LAYOUT < 0 && S >= 512); }
// floats of pair matrices one workgroup of the cluster solve can hold
inline int plan_cluster_capacity(int n_node) { return (int)(PLAN_BP_CLUSTER_LDS / sizeof(float)) - (n_node * 14 + 48); }
// clusters of C co-resident workgroups, one per CU: at most CUs / C systems per launch (multiples of 8 keep a
// cluster on one XCD under round-robin workgroup dispatch, so its exchange stays in that XCD's L2)
inline int plan_cluster_per_launch(int n_cu, int C) { const int n = C > 1 ? n_cu / C : 0; return n >= 8 ? n & ~7 : n; }
// grid.x of a cluster launch of n systems, rounded up to a multiple of 8 (the surplus workgroups leave at once): workgroup b is dispatched
// to XCD b mod 8, so the C workgroups of a system -- linear ids s + c * grid.x -- then share an XCD and their exchange stays in its L2, also
// when fewer than 8 systems are solved (placement for speed only: the protocol is placement independent).  One 300-residue system, 6
// workgroups: solve 211 -> 200 us.  (Round 6, measured on that placement and not taken: plain stores + sc1 loads and no acquire
// fence, which is valid only while the cluster shares an L2: 180 us, 2 235 -> 2 287 steps/s -- 0.9 us per barrier; the rest of a
// 10 us sweep is the counter round trips and the phases' own dependent loads.)
inline int plan_cluster_grid_x(int n) { return (n + 7) & ~7; }
// Workgroups per system of the belief-propagation solve: enough that the exp(-E) matrices of the multi-state residue pairs (need floats,
// widest class in slots) fit their LDS (15% slack for the fluctuation of the pair count; systems that outgrow it fall back to the
// one-workgroup kernel on the device).
// The cluster solve trades HBM/L2 traffic for two device-scope barriers per sweep.  Re-measured after the
// one-workgroup kernel got its batched loads and the short list margin (BP ms, cluster vs one workgroup):
//   300 residues / 10 A (C = 8):  1 system 0.19 vs 0.31, 8: 0.23 vs 0.35, 32: 0.35 vs 0.43, 48 (two launches):
//                                 0.63 vs 0.47, 64: 0.56 vs 0.48
//   300 residues / 7 A, 150 residues / 10 A (C = 3..4): 0.22 vs 0.19 at 1 system, 0.31 vs 0.24 at 32
//   56 and 20 residues (C = 1): the one-workgroup solve by construction
// so the cluster is used when the pair matrices need many workgroups (C >= 6) and the batch fits 4/5 of one
// launch (CUs / C systems); everything else takes the one-workgroup solve.  (A second cluster form that kept the
// matrices in global memory won nowhere after these measurements and is gone: `git log` has it.)
// (round 2, after the one-workgroup solve got its look-ahead loads: 32 systems 0.37 vs 0.38 ms, 40: 0.41 vs 0.39, 48 (two launches):
//  0.61 vs 0.39 -- the cluster up to 4/5 of one launch)
inline int plan_cluster_size(const PlanSwitches& sw, long need, long widest, int n_node, int n_node1, int S, int n_cu) {
    const int want = sw.BP_CLUSTER;
    if (want == 1) return 1;
    const int cap = plan_cluster_capacity(n_node);
    int C = cap > 0 ? (int)((need * 115 / 100 + cap - 1) / cap) : 1;
    const int by_lanes = (int)((widest * 115 / 100 + BPC_BLOCK - 1) / BPC_BLOCK);   // one slot per class per lane
    if (by_lanes > C) C = by_lanes;
    if (want > 1) C = want;
    if (C > 16 || n_node - n_node1 < C) C = 1;             // too large for a co-resident cluster: one-workgroup solve
    const int resident_limit = C >= 6 ? plan_cluster_per_launch(n_cu, C) * 4 / 5 : 0;
    if (want <= 1 && S > resident_limit) C = 1;
    return C < 1 ? 1 : C;
}
// node_prob_in_solve: a small batch is a chain of launches, so the 1-body pass rides in the prologue of the one-workgroup solve (a launch
// less where launches are what a step waits for; the cluster solve does the same for its own nodes).
// p_prob: one-workgroup solve with single-writer matrices: the pair-energy kernel writes exp(-E) itself and the matrices rest at 1
// (= no interaction) between evaluations, which removes the solve's exp pass over every active matrix.  The cluster solves and the
// accumulating (several beads per state) path keep energies resting at 0.
// prefold: the layout launch folds the 1-state partners into the node probabilities, which it can only where the matrices hold exp(-E)
// and the probabilities exist before the solve (the device reads the same three fields: UPK_ROTAMER_PREFOLD).
struct MatrixForm { int node_prob_in_solve, p_prob, prefold; };
inline MatrixForm plan_matrix_form(const PlanSwitches& sw, int S, bool merged, int C, bool one_bead_per_state, bool layout_record) {
    MatrixForm f;
    f.node_prob_in_solve = ((S <= 16 || merged) && sw.NODE_PROB_IN_SOLVE) ? 1 : 0;
    f.p_prob = (C <= 1 && one_bead_per_state && !sw.BP_ENERGY_TABLE) ? 1 : 0;
    f.prefold = (layout_record && !f.node_prob_in_solve && f.p_prob) ? 1 : 0;
    return f;
}
// The one-workgroup solve.  TWO compiled solves.  (i) dense: 512 lanes x 256 registers, the dense per-solve inbox, one slot of every class
// pinned in registers per lane: every batch size (round 4 measured it against two pinned 6x6 slots, a 1024-lane streaming form and larger
// pinned sets across proteins and batch sizes; the losers are gone: `git log` has them).  (ii) streaming: 1024 lanes streaming every matrix
// over the CACHED inbox layout: the hand-over solve behind a cluster launch (lds_base, no inbox, so that the normally empty launch does not
// wait for a whole CU's LDS), systems whose layout scratch does not fit, UPSIDE_HIP_BP_COMPACT=0 (tests).
// layout_launch: the dense layout as a launch of its own in front of the solve, when the record exists and its scratch fits a quarter of
// a CU's LDS; else inside the solve.  have_rows: the cached row arrays exist.
struct BpSolve { bool refused; size_t lds_base, msg_bytes; int msg_floats; bool dense, layout_launch; int scratch_words; size_t layout_lds; };
inline BpSolve plan_bp_solve(const PlanSwitches& sw, int n_node, int slot_cap, bool have_rows, bool layout_record) {
    BpSolve p = {};
    p.lds_base = ((size_t)n_node * (BP_NODE_ARRAYS * BP_NODE_STRIDE + 2) + 64 + 8) * sizeof(float);
    p.refused = p.lds_base > PLAN_BP_BASE_LDS;
    // LDS left over holds the messages to the 3-state nodes (at most all of the inbox: 16 floats per slot); UPSIDE_HIP_BP_LDS_MSG_KB=0
    // keeps every message in global memory (experiments)
    p.msg_bytes = (size_t)sw.BP_LDS_MSG_KB * 1024;
    if (p.lds_base + p.msg_bytes > PLAN_CU_LDS) p.msg_bytes = p.lds_base >= PLAN_CU_LDS ? 0 : PLAN_CU_LDS - p.lds_base;
    if (p.msg_bytes > (size_t)slot_cap * 64) p.msg_bytes = (size_t)slot_cap * 64;
    p.msg_bytes &= ~(size_t)15;
    p.msg_floats = (int)(p.msg_bytes / sizeof(float));
    // (the layout pass borrows the LDS inbox for an activity bit per cached row and a prefix per 32 rows: at most two rows per slot)
    const size_t layout_scratch = (((size_t)2 * slot_cap + 64) / 32 * 2 + 2) * sizeof(int);
    p.dense = sw.BP_COMPACT && have_rows && p.msg_bytes >= layout_scratch;
    // scratch of the layout launch: sized for a quarter of the slot capacity (the capacity allows 96 residue pairs per node, a protein has ~30)
    p.scratch_words = sw.BP_LAYOUT == 2 ? 1 : (int)((((size_t)2 * (slot_cap / 4 + 32) + 64) / 32) * 2 + 2);
    p.layout_lds = ((size_t)n_node * (BP_NODE_STRIDE + 1) + 64 + N_CLASS + 16) * sizeof(float) + (size_t)p.scratch_words * sizeof(int) + 64;
    p.layout_launch = p.dense && layout_record && p.layout_lds <= PLAN_BP_LAYOUT_LDS;
    return p;
}

/* Thin C-ABI between the host-side C++ engine (DerivEngine / DerivComputation nodes) and the hand-written
 * HIP kernels for gfx950.  Plain pointers, ints and floats only; every pointer is a DEVICE pointer unless
 * marked host.  All launchers are asynchronous on `L->stream` and return the hipError_t of the launch
 * (0 = success).  Arrays carry a leading system dimension S = L->n_system ("[S]" below): S independent
 * replicas / ensemble members of one topology are processed by one launch (grid.y = system).
 *
 * Each launcher names the reference loop it replaces (paths relative to /root/reference/).
 */
#ifndef UPSIDE_HIP_KERNELS_H
#define UPSIDE_HIP_KERNELS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fuse: the engine's queue of fused per-element ops (upk_fuse_create) or NULL.  Per-element launchers (marked "fusable" below)
 * append an op to it instead of launching; every other launcher runs the queue first (upk_fuse_flush), so the order of calls is
 * the order of effects.  A caller that enqueues its own work on `stream` must call upk_fuse_flush(L) first. */
typedef struct { int n_system; void* stream; void* fuse; void* batch; } upk_launch_t;
/* batch: merged launches (csrc/kernels_batch.h) or NULL.  Between upk_batch_begin and upk_batch_end the launchers of the list
 * upkeep and of the pair passes that have a batch form append to the chain named by upk_batch_chain instead of launching; launches
 * of one chain keep their order, the k-th launches of all chains run side by side as ONE launch.  The caller promises that
 * different chains do not depend on each other.  Any other launcher runs what the batch holds first. */
void* upk_batch_create(void);
void upk_batch_destroy(void* batch);
int upk_batch_begin(const upk_launch_t* L);
void upk_batch_chain(const upk_launch_t* L, int chain);
int upk_batch_run(const upk_launch_t* L);
void upk_batch_fused_submitted(const upk_launch_t* L);   /* (called by the fused-op queue) */
int upk_batch_end(const upk_launch_t* L);
void* upk_fuse_create(int n_system);
void upk_fuse_destroy(void* fuse);
int upk_fuse_flush(const upk_launch_t* L);          /* one launch for the pending ops (no-op when nothing is pending) */
int upk_fuse_pending(const upk_launch_t* L);        /* number of ops waiting */
long upk_fuse_launch_count(const upk_launch_t* L);  /* fused launches so far (diagnostics) */
int upk_fuse_table_size(const upk_launch_t* L);     /* distinct ops registered so far: constant once every op of the MD loop has been seen */
#define UPK_FLUSH(L) do { const int r_ = upk_fuse_flush(L); if (r_) return r_; } while (0)

/* A CoordNode's storage (src/deriv_engine.h:83-96): out/sens are [S][n_elem][stride] */
typedef struct { float* out; float* sens; int n_elem; int width; int stride; } upk_coord_t;

/* ---- generic ---------------------------------------------------------------------------------- */
/* out[s] (+)= sum_i in[s][i]; one workgroup per system, fixed tree order (deterministic).            */
int upk_reduce_sum(const upk_launch_t* L, const float* in, int n, float* out, int accumulate);
int upk_scale(const upk_launch_t* L, float* x, int n, float factor);   /* x[i] *= factor */
/* zero n_buf device buffers (float counts in sizes[], 16-byte aligned) in one launch:
 * the per-node "zero sensitivity" of deriv_engine.cpp:147-151 for the whole graph */
int upk_zero_many(const upk_launch_t* L, float* const* ptrs, const long* sizes, int n_buf);
/* deterministic gather of deferred derivative contributions into a node's sens:
 * sens[s][t][c] += sum_{e in csr[t]} arena[s][entry[e] + c], c < width  (replaces the scatter-adds of
 * e.g. src/bonds.cpp:315-316, src/placement.cpp:304-305, src/eig.cpp:467)                               */
int upk_gather_contrib(const upk_launch_t* L, const float* arena, long arena_stride, const int* csr_start,
                       const int* csr_entry, upk_coord_t target, int width, int comp_offset);

/* ---- Monte-Carlo pivot moves (src/monte_carlo_sampler.cpp:3-155, 255-284) -------------------------------- */
typedef struct {
    int n_loc, n_bin, n_layer;
    const int* atoms;          /* [n_loc][5] prevC, N, CA, C, nextN */
    const int* range;          /* [n_loc][2] rigid tail [first, end) rotated with the pivot */
    const int* restype;        /* [n_loc] layer of the proposal map */
    const float* pot;          /* [n_layer][n_bin*n_bin] -log proposal probability, normalised */
    const float* cdf;          /* [n_layer][n_bin*n_bin] cumulative proposal probability */
} upk_pivot_t;
/* every system: save the positions, draw a pivot (stream 2 keyed by `round`), rotate the tail; delta_lprob[s] out */
int upk_pivot_propose(const upk_launch_t* L, upk_coord_t pos, float* pos_copy, const upk_pivot_t* P, const uint32_t* seed,
                      uint64_t round, float* delta_lprob);
/* rigid-body jump of one chain segment (monte_carlo_sampler.cpp:157-251): translation by sigma_trans/sqrt(3) * N(0,1)^3
 * or rotation about the centre of mass by sigma_rot * N(0,1) around a random axis; random stream 3; delta_lprob = 0 */
typedef struct { int n_chain; const int* atom_range; /* [n_chain][2] */ const float* sigma_trans; const float* sigma_rot; } upk_jump_t;
int upk_jump_propose(const upk_launch_t* L, upk_coord_t pos, float* pos_copy, const upk_jump_t* J, const uint32_t* seed,
                     uint64_t round, float* delta_lprob);
/* Metropolis test of monte_carlo_step (second draw of the same generator); rejected systems get pos_copy back;
 * stats[s] = {n_success, n_attempt} accumulate */
int upk_mc_accept(const upk_launch_t* L, upk_coord_t pos, const float* pos_copy, const float* e_old, const float* e_new,
                  const float* delta_lprob, const float* temperature, const uint32_t* seed, uint64_t round, int stream,
                  int accept_draw, int* stats);   /* accept_draw: index of the generator's draw used for the test */

/* ---- integrator / thermostat (src/deriv_engine.cpp:11-48, src/thermostat.cpp:9-18, src/random.h) ---- */
int upk_integration_stage(const upk_launch_t* L, float* mom, upk_coord_t pos, float vel_factor, float pos_factor,
                          float max_force);
/* n_invocations[S] lives on the device, one (equal) entry per system -- all systems are thermalised at the same rounds --:
 * the op reads its system's entry and then advances it, so a captured MD graph replays correctly; mom is [S][n_atom][4] */
int upk_thermostat(const upk_launch_t* L, float* mom, int n_atom, const uint32_t* seed, unsigned long long* n_invocations,
                   const float* mom_scale, const float* noise_scale);
int upk_recenter(const upk_launch_t* L, upk_coord_t pos, int xy_only);
int upk_kinetic(const upk_launch_t* L, const float* mom, int n_atom, float* kin);

/* ---- backbone coordinate nodes ------------------------------------------------------------------ */
/* affine_alignment (src/eig.cpp:317-470): eig is [S][n_res][20] (4 eigenvalues + 4x4 eigenvectors) */
int upk_affine_fwd(const upk_launch_t* L, upk_coord_t pos, const int* atoms, const float* ref_geom, int n_res,
                   upk_coord_t out, float* eig);
/* writes per-residue 3 atoms x 3 comps into contrib[s][res*9 ...] */
int upk_affine_bwd(const upk_launch_t* L, upk_coord_t aff, const float* ref_geom, const float* eig, int n_res,
                   float* contrib, long contrib_stride);
/* rama_coord (src/bonds.cpp:205-247): jac [S][n_res][UPK_RAMA_JAC] -- the 2 x 5 x 3 derivatives of a residue in the first 30 floats
 * of a 128-byte row (written as eight 16-byte words: the buffer must be 16-byte aligned and hold UPK_RAMA_JAC floats per residue) */
#define UPK_RAMA_JAC 32
int upk_rama_fwd(const upk_launch_t* L, upk_coord_t pos, const int* atom, const int* dummy, int n_res, upk_coord_t out,
                 float* jac);
int upk_rama_bwd(const upk_launch_t* L, upk_coord_t rama, const float* jac, int n_res, float* contrib, long contrib_stride);
/* infer_H_O (src/hbond.cpp:59-119): dfd [S][n_virtual][12] */
int upk_infer_fwd(const upk_launch_t* L, upk_coord_t pos, const int* atom, const float* bond_length, int n_virtual,
                  upk_coord_t out, float* dfd);
int upk_infer_bwd(const upk_launch_t* L, upk_coord_t infer, const float* bond_length, const float* dfd, int n_virtual,
                  float* contrib, long contrib_stride);

/* ---- bonded potentials (src/bonds.cpp:297-318, 457-487, 519-545, 350-372) -------------------------- */
/* kind: 2 dist, 3 angle, 4 dihedral.  contrib: [term][kind][3]; pot_terms [S][n] (may be NULL).
 * System s reads equil / k / radius at base + s * par_stride (0 = one row shared by every system, n = a row per system) */
int upk_spring_strided(const upk_launch_t* L, int kind, upk_coord_t pos, const int* id, const float* equil, const float* k, long par_stride,
                       int n, float* contrib, long contrib_stride, float* pot_terms);
int upk_cavity_radial_strided(const upk_launch_t* L, upk_coord_t pos, const int* id, const float* radius, const float* k, long par_stride,
                              int n, float* contrib, long contrib_stride, float* pot_terms);

/* ---- placement (src/placement.cpp:264-307) ------------------------------------------------------- */
typedef struct {
    int n_elem, n_pos_dim, n_sig; int sig[3];              /* 0 scalar, 1 vector, 2 point */
    const int* affine_residue; const int* layer; const int* rama_residue;
    int is_rama; const float* fixed_data;                  /* (n_layer, n_pos_dim) */
    const float* spline_coeff; int nx, ny;                 /* (n_layer,nx,ny,n_pos_dim,16) */
} upk_placement_t;
int upk_placement_fwd(const upk_launch_t* L, const upk_placement_t* P, upk_coord_t aff, upk_coord_t rama, upk_coord_t out,
                      float* rama_deriv);
/* aff_contrib [elem][6] (com, torque); rama_contrib [elem][2] (NULL unless is_rama) */
int upk_placement_bwd(const upk_launch_t* L, const upk_placement_t* P, upk_coord_t aff, upk_coord_t out,
                      const float* rama_deriv, float* aff_contrib, long aff_stride, float* rama_contrib, long rama_stride);

/* ---- simple per-element nodes ---------------------------------------------------------------------- */
/* rama_map_pot (src/rama_map_pot.cpp:57-82): adds into rama.sens directly (residue ids are distinct) */
int upk_rama_map_pot(const upk_launch_t* L, upk_coord_t rama, const int* residue, const int* map_id, int n,
                     const float* coeff, int nx, float* pot_terms);
/* weighted_pos (src/environment.cpp:132-154) */
int upk_weighted_pos_fwd(const upk_launch_t* L, upk_coord_t pos, upk_coord_t energy, const int* index_pos,
                         const int* index_weight, upk_coord_t out);
int upk_weighted_pos_bwd(const upk_launch_t* L, upk_coord_t pos, upk_coord_t energy, const int* index_pos,
                         const int* index_weight, upk_coord_t self);
/* nonlinear_coupling (src/environment.cpp:358-369) */
int upk_nonlinear_coupling(const upk_launch_t* L, upk_coord_t input, const int* types, const float* coeff, int n_coeff,
                           float offset, float inv_dx, float* pot_terms);
/* hbond_energy (src/hbond.cpp:430-444), one energy scale per system: E_protein is a device array [S] */
int upk_hbond_energy_sys(const upk_launch_t* L, upk_coord_t protein_hbond, const float* E_protein, float* pot_terms);
/* backbone_pairs (src/backbone_steric.cpp:81-145): gather form over residue pairs; aff_contrib [res][6]; pot_terms [S][n_res]
 * (each pair counted once).  cache (may be NULL: every residue scans all others each step, what the reference does): per-row lists
 * of the residues within dist_cutoff + skin of the row's REFERENCE centre, rebuilt by the kernel when the two largest centre
 * displacements add up to the skin; used by the multi-workgroup launch (n_res > 128).  The caller flips `parity` on every call. */
typedef struct {
    int* list;            /* [S][n_res][cap] */
    int* cnt;             /* [S][n_res] */
    float *ref0, *ref1;   /* [S][n_res][4] reference centres, double buffered (initialised far away: the first call builds) */
    int cap, parity; float skin;
    int* error_flag;      /* set to 1 when a row outgrows cap */
} upk_backbone_list_t;
int upk_backbone_pairs(const upk_launch_t* L, upk_coord_t aff, const int* residue, const int* id, const int* n_atom,
                       const float* ref_pos, int n_res, float dist_cutoff, float* aff_contrib, long aff_stride,
                       float* pot_terms, const upk_backbone_list_t* cache);

/* ---- interaction graph (src/interaction_graph.h) ---------------------------------------------------- */
enum { UPK_IT_ROTAMER = 0, UPK_IT_HBOND_COVERAGE = 1, UPK_IT_ENVIRONMENT = 2, UPK_IT_PROTEIN_HBOND = 3,
       UPK_IT_RADIAL = 4 /* symmetric, sidechain_radial.cpp:16-79 */, UPK_IT_HBOND_SC_RADIAL = 5 /* the same functor between two nodes */ };

typedef struct {
    int itype, symmetric;
    int n1, n2;                          /* elements on each side */
    int dim1, dim2;                      /* components used (6/6, 7/6, 6/4) */
    upk_coord_t node1, node2;            /* source CoordNodes */
    const int *loc1, *loc2, *type1, *type2, *id1, *id2;
    const float* param; int n_type1, n_type2, n_param;
    int n_knot, n_knot_angular; float inv_dx, inv_dtheta;
    float cutoff, cache_cutoff;          /* cache_cutoff = cutoff + skin (interaction_graph.h:97,395-396) */
    /* cached Verlet lists: for side-1 rows nbr1[s][i][k] (neighbours on side 2, ascending) and count;
       for asymmetric graphs the transposed list nbr2 as well; symmetric graphs keep the full list in nbr1. */
    int cap1, cap2;
    int *nbr1, *cnt1, *nbr2, *cnt2;
    float *cache_pos1, *cache_pos2;      /* [S][n][4] positions the lists were built from; 4th word = element id (raw bits) */
    int* rebuild_flag;                   /* [S] system moved further than the skin allows */
    int* flagged; int parity, flag_stride; /* [2][flag_stride]: compact list of the systems flagged this step: entry 0 of
                                          * half `parity` is the count, entries 1.. the system ids; the other half is
                                          * reset for the next step.  Rebuild kernels loop over this list with a small
                                          * grid.y instead of launching (and retiring) workgroups for every system. */
    int* error_flag;                     /* [1] set to non-zero on capacity overflow */
    /* optional hook used by the rotamer node: while a symmetric list is rebuilt, mark_table[s][node(i)][node(j)]
       (mark_n rows of mark_ld bytes, cleared by the rebuild test that flags the system) is set to 1 for every cached pair */
    unsigned char* mark_table; const int* mark_node; int mark_n, mark_stride;   /* mark_stride: bytes per system (multiple of 16) */
    int mark_ld;                         /* bytes per row: mark_n rounded up to 64 (a row is whole 64-bit words of the packed bit matrix) */
    int mark_start3, mark_start6;        /* node of a bead id (rotamer.cpp:812-816): (id >> 8) + {0, mark_start3, mark_start6} by its state count */
    /* This step's in-range pairs ("hit lists", the refine of interaction_graph.h:201-257 done ONCE per step and side by
       upk_pairlist_refine): for every row of side 1 (hit1) / side 2 (hit2) the cached neighbours with d2 < cutoff2, in list
       order; hit[s][row][k] holds the list word unchanged, hcnt[s][row] their number (capacity per row = cap1 / cap2).
       Symmetric graphs: hlo1[s][row] = hits whose partner index is BELOW the row (lists ascend, so the partners above the
       row -- each pair once, i1 < i2 -- are the tail [hlo1, hcnt1) of the hit list).
       ord1 / ord2 [s][row]: rows sorted by descending hit count (upk_pairlist_order), ord1u by descending count of partners
       above the row: the pair passes hand 8 consecutive rows of that order to the 8 lane groups of a wavefront, so the
       groups of a wavefront run the same number of trips.
       The rotamer graph's list words carry the residue-pair slot above bit UPK_ROT_J_BITS. */
    int *hit1, *hit2, *hcnt1, *hcnt2, *hlo1;
    unsigned short *ord1, *ord2, *ord1u;
    float *cur_pos1, *cur_pos2;          /* [S][n][4] this step's positions (x, y, z, -), written by upk_pairlist_check */
    unsigned long long* gacc;            /* [S][n_other][8] exact fixed-point (x 2^32) gradient accumulators of upk_igraph_backward when several
                                            workgroups serve one system (small batches); NULL: one workgroup per system; zero between evaluations */
    int nbr_j_bits;                      /* 0: a list word is the element index; else the index is its low nbr_j_bits bits */
    /* quadspline graphs (hbond_coverage): the same table as `param`, every knot interval of every spline expanded on the host
       into its cubic's 4 monomial coefficients: [n_type1][n_type2][n_poly], n_poly = 8 (n_knot_angular - 3) + 8 (n_knot - 1),
       rows 16-byte aligned (layout: igraph_device.h, quadspline_pair<.., POLY>).  The LDS-staged pair passes read this one;
       NULL: they read `param`. */
    const float* param_poly; int n_poly;
    int sens_overlap;                    /* node1 and node2 are one node AND some element is listed on both sides (set by the host) */
    int word16;                          /* 1: the words of nbr1/nbr2/hit1/hit2 are 16 bits wide (bare element indices; every graph but the rotamer's:
                                            n1, n2 <= 65534), rows cap1 / cap2 such words apart in the first half of the arrays; 0: 32-bit words */
} upk_igraph_t;
#define UPK_ROT_J_BITS 13                /* rotamer list word = bead | slot << 13: <= 8191 beads (bead index n1 is the refine kernel's sentinel), < 2^19 - 1 slots */
#define UPK_ROT_SLOT_NONE 0x7FFFF        /* slot field of a cached bead pair whose residue pair got no slot (capacity overflow) */

/* K1: flag[s] |= any element moved more than (cache_cutoff-cutoff)/2 since the last build
 * (interaction_graph.h:57-90) */
int upk_pairlist_check(const upk_launch_t* L, const upk_igraph_t* G);
/* K2: where flag[s] is set rebuild the row lists with d < cache_cutoff and acceptable_id_pair
 * (interaction_graph.h:116-158); clears the flag */
int upk_pairlist_build(const upk_launch_t* L, const upk_igraph_t* G);
/* ... of the sides in `sides` only (bit 1: side-1 rows, bit 2: side-2 rows): a graph whose pair passes all gather over the rows of
 * one side never reads the other side's lists on the MD path (they can be built later from the same cache_pos) */
int upk_pairlist_build_sides(const upk_launch_t* L, const upk_igraph_t* G, int sides);
/* K2b: this step's in-range pairs of every system for the rows of `side` (hit lists above), from the cached lists and
 * cur_pos; then the rows of that side sorted by descending hit count (ord1 / ord2, and ord1u for symmetric graphs) */
int upk_pairlist_refine(const upk_launch_t* L, const upk_igraph_t* G, int side);
int upk_pairlist_order(const upk_launch_t* L, const upk_igraph_t* G, int side);
/* Pair passes over the hit lists (LDS-staged; fall back to the list-walking forms below for systems too large for LDS).
 * upk_igraph_rows: for every row of `side`
 *   mode 0: out[s][(out_row0 + row)*out_stride + out_comp] = sum over the row's in-range partners of the pair value
 *           (hbond.cpp:387-389, environment.cpp:85-91, hbond.cpp:316-319)
 *   mode 1: the same, and own_grad[s][row][8] = the UNWEIGHTED sum of d(value)/d(row element): when the pair sensitivity
 *           is the row element's own (coverage nodes), that side's backward pass is upk_igraph_apply_own_grad
 *   mode 2: sens(pair) * d(value)/d(row element) summed over the partners and added to the source node's sens at
 *           loc[row] (interaction_graph.h:525-555 as a per-row gather; no atomics, fixed summation order).
 *           Pair sensitivity: sens_mode 1: sens1[s][i1*sens_stride]; 2: sens2[s][i2*sens_stride]; 3: sens1[i1]+sens2[i2].
 * side = 3: the rows of side 1, then the rows of side 2, in one launch (protein_hbond; mode 0 writes side 2 at out_row0_2) */
int upk_igraph_rows(const upk_launch_t* L, const upk_igraph_t* G, int side, int mode, float* out, long out_sys_stride, int out_stride,
                    int out_comp, int out_row0, int out_row0_2, float* own_grad, int sens_mode, const float* sens1, const float* sens2,
                    long sens_sys_stride, int sens_stride);
int upk_igraph_apply_own_grad(const upk_launch_t* L, const upk_igraph_t* G, int side, const float* own_grad,
                              const float* sens, long sens_sys_stride, int sens_stride);
/* Backward over the hit lists of side `row_side`, ONE visit per pair: sens(pair) * d(value)/d(element) is added to the source
 * nodes' sens of BOTH elements (interaction_graph.h:525-555).  The row element's share accumulates in registers, the other
 * element's through 64-bit integer LDS atomics as exact fixed point, so results do not depend on the order of the pairs. */
int upk_igraph_backward(const upk_launch_t* L, const upk_igraph_t* G, int row_side, int sens_mode, const float* sens1,
                        const float* sens2, long sens_sys_stride, int sens_stride);
/* List-walking forms (no hit lists, no LDS staging; any system size): the radial potentials and the fallback of the two
 * launchers above.  Row sums of the pair value over one side's cached lists ... */
int upk_igraph_rowsum(const upk_launch_t* L, const upk_igraph_t* G, int side, float* out, long out_sys_stride,
                      int out_stride, int out_comp, int out_row0, float* own_grad /* may be NULL; as mode 1 above */);
/* ... and the per-row gather of sens(pair) * d(value)/d(row coords), added to the source node's sens at loc[row].
 * sens_mode 0: every pair has sensitivity 1 (potentials summed over edges, sidechain_radial.cpp:94-96) */
int upk_igraph_grad(const upk_launch_t* L, const upk_igraph_t* G, int side, int sens_mode, const float* sens1,
                    const float* sens2, long sens_sys_stride, int sens_stride);
/* parity/diagnostic: flags[s][i][k] = 1 where cached neighbour k of row i is in range this step */
int upk_igraph_inrange(const upk_launch_t* L, const upk_igraph_t* G, unsigned char* flags);

/* ---- rotamer (src/rotamer.cpp) ------------------------------------------------------------------- */
/* grid.y of the rebuild kernels: enough slices that the systems flagged in one step (about one in five with the
 * short list margin) are rebuilt side by side, few enough that a quiet step retires almost no idle workgroups
 * (measured at 1024 systems, same box: S/8 91.8 k, S/4 92.8 k, S/2 92.5 k system-steps/s) */
#define UPK_FLAG_DIV_DEFAULT 4
#ifndef UPK_FLAG_DIV
#define UPK_FLAG_DIV UPK_FLAG_DIV_DEFAULT
#endif
#define UPK_FLAG_GRID(S) ((S) < 16 ? (S) : ((S) / UPK_FLAG_DIV > 16 ? (S) / UPK_FLAG_DIV : 16))
#define UPK_FLAG_LIST(G) ((G).flagged + (size_t)(G).parity * (G).flag_stride)
/* (of upk_rotamer_t below) k_rotamer_bp_layout folds the edges to 1-state partners into the node probabilities, and the solve takes them over, under this
   condition and for the systems it laid out (word n_node + 7 of the record == 0).  Probability form only: the fold multiplies by the
   matrix rows as stored, and in energy form they hold E until the solve's own exp pass, which runs behind the layout launch. */
#define UPK_ROTAMER_PREFOLD(R) ((R).bp_layout && !(R).node_prob_in_solve && (R).p_prob)

typedef struct {
    upk_igraph_t G;                      /* symmetric bead graph */
    int n_node, n_node1, n_node3;        /* global node ids: class 1, then 3, then 6 */
    const int* node_nrot;                /* [n_node] */
    const int *bead_node, *bead_rot;     /* [n_bead] */
    const int *bead_orig;                /* [n_bead] the bead's index in the configuration's own order (NULL: unchanged); the parameter
                                            derivative orients a pair (i1 < i2) by it, as the reference's edge list does */
    const int *bead_meta;                /* [n_bead] type | rot<<8 | n_rot<<12 (staged into the LDS bead rows) */
    const float* param_tri;              /* upper triangle of the (symmetric) pair table: row tri(lo, hi) = interaction_param[lo][hi], lo <= hi;
                                            (hi, lo) reads the same row with its two angular blocks exchanged (is_compatible, bead_interaction.h:209-218) */
    const float* param_tri_poly; int n_poly;   /* the same triangle as per-interval polynomials (upk_igraph_t::param_poly layout, n_poly floats per row); the
                                            energy pass stages it when it fits LDS next to the beads (NULL / does not fit: param_tri) */
    float* bead_pack;                    /* [S][n_bead][8] packed bead rows for systems whose beads do not fit LDS (else NULL) */
    unsigned long long* grad_acc;        /* [S][n_bead][6] exact fixed-point (x 2^32) gradient accumulators of the gradient pass when a system is
                                            served by several workgroups or does not fit LDS; zero between evaluations */
    int one_bead_per_state;              /* every (residue, rotamer state) owns exactly one bead: each pair-matrix entry has a single writer */
    int node_prob_in_solve;              /* the one-workgroup solve computes the node probabilities itself (upk_rotamer_node_prob is then a no-op): small batches */
    int p_prob;                          /* the pair-energy kernel stores exp(-E) (resting value 1) instead of E (resting value 0): the
                                            one-workgroup solve then has no exp pass.  Needs one_bead_per_state and bp_C <= 1 */
    const int *node_bead_start, *node_bead_list;   /* CSR (node*6+rot) -> beads of that rotamer state */
    int n_prob; const float* const* prob_out; float* const* prob_sens; const int* prob_stride;   /* 1-body parents (device arrays of device ptrs) */
    const long* prob_sys_stride;
    /* per system state */
    float *node_prob, *node_off, *nb_cur;               /* [S][n_node][6], off [S][n_node] */
    int slot_cap, adj_cap;
    int *n_slot, *slot_a, *slot_b, *slot_of, *slot_active;   /* [S], [S][cap], [S][cap], [S][n_node^2], [S][cap] */
    unsigned char* mark;                 /* [S][n_node][G.mark_ld] residue pairs owning a cached bead pair (= G.mark_table) */
    int *adj_cnt, *adj_slot;             /* [S][n_node], [S][n_node][adj_cap] */
    int *bp_start, *slot_off;            /* [S][n_node+1] inbox CSR of BP messages, [S][cap][2] inbox offsets of a slot */
    int *row_start, *slot_row;           /* the same inbox counted in ROWS (one per message): [S][n_node+2] first row of a node (entry n_node: end;
                                            entry n_node+1: R6, the first row of the 6-state block = rows of the 3-state nodes rounded up to 32),
                                            [S][cap][2] rows of a slot's two messages.  The large-batch solve lays the messages of the slots ACTIVE
                                            in this evaluation out densely (3 / 6 floats per row) so that they fit the LDS; NULL: not kept */
    int *class_start;                    /* [S][6] slot ranges by class: 3x3, 3x6, 6x6, 1x1, 1xN */
    int *slot_active_last;               /* [S][cap] activity flags of the last solve (diagnostics) */
    float *P, *msg_cur, *marg;           /* P, marg: SoA [S][36][cap]; msg_cur: inbox [S][cap][16] floats at most: message rows grouped by
                                          * receiving node, 4 floats per message to a 3-state node, 8 to a 6-state node */
    float damping, tol; int max_iter, chunk;
    int* iters;                          /* [S] sweeps of the last solve */
    int* n_bad;                          /* [S] solves that ran into max_iter (rotamer.cpp:784-785), counted on the device */
    int* bp_rec;                         /* [S][slot_cap][4] scratch of the one-workgroup solve: per class, the slots active this step
                                            packed as {offset a, offset b, node a | node b << 16, slot} */
    int* bp_layout;                      /* [S][7 n_node + 8] the dense inbox layout of the last solve when k_rotamer_bp_layout computes it
                                            in front of the one-workgroup solve: first float of every node [n_node + 1], active slots per class [3],
                                            inbox floats, floats of the rows to 3-state nodes, row width, pad to n_node + 8, then the node
                                            probabilities with the 1-state partners folded in [n_node][6] (raw float bits); NULL: the solve lays
                                            its inbox out and folds itself (small batches) */
    long long* bp_trace;                 /* [S][32] 100 MHz phase clocks of the last solve ([16..24): sub-phase stamps), or NULL (diagnostics) */
    float* energy;                       /* [S] Bethe free energy (only when want_energy) */
    /* cluster solve (bp_C > 1 workgroups per system, pair matrices resident in LDS) */
    int bp_C;                            /* workgroups per system */
    int *bp_bar, *bp_fallback;           /* [S] barrier counter; [S] 1 = system did not fit or a cluster barrier gave up: solved by the one-workgroup kernel */
    int bp_test_abort;                   /* tests (UPSIDE_HIP_BP_CLUSTER_TEST_ABORT): the last workgroup of every cluster leaves at once, barriers give up early */
    float *bp_nbx, *bp_dev, *bp_en_part; /* [S][2][n_node][8] exchanged node beliefs, [S][2][16] deviations, [S][16] energy partial sums */
} upk_rotamer_t;
#define UPK_BP_LAYOUT_PER_NODE 7         /* ints of upk_rotamer_t::bp_layout per system: UPK_BP_LAYOUT_PER_NODE * n_node + UPK_BP_LAYOUT_EXTRA */
#define UPK_BP_LAYOUT_EXTRA 8

/* pair-list rebuild of flagged systems (replaces EdgeLocator, rotamer.cpp:134-206): clear the node x node table,
 * [upk_pairlist_build marks it through G.mark_table], number the slots by class + adjacency + inbox layout, and
 * record the slot of every cached bead pair */
int upk_rotamer_clear_slots(const upk_launch_t* L, const upk_rotamer_t* R);
int upk_rotamer_build_slots(const upk_launch_t* L, const upk_rotamer_t* R);
int upk_rotamer_nbr_slots(const upk_launch_t* L, const upk_rotamer_t* R);
/* 1-body energies -> node probabilities (rotamer.cpp:811-826, 239-256) */
int upk_rotamer_node_prob(const upk_launch_t* L, const upk_rotamer_t* R);
/* bead-pair energies accumulated into the residue-pair matrices (rotamer.cpp:829-846, interaction_graph.h:470-503) */
int upk_rotamer_pair_energy(const upk_launch_t* L, const upk_rotamer_t* R);
/* damped belief propagation + marginals (+ Bethe free energy): rotamer.cpp:1005-1061, 453-522, 283-302, 405-451, 854-866 */
int upk_rotamer_bp(const upk_launch_t* L, const upk_rotamer_t* R, int want_energy);
int upk_device_cu_count(void);   /* compute units of the current device: an input of the launch plan (csrc/launch_plan.h) */
/* derivative push: pair marginal x pair gradient gathered per bead, node marginals to the 1-body parents
 * (rotamer.cpp:956-985, interaction_graph.h:525-555) */
int upk_rotamer_grad(const upk_launch_t* L, const upk_rotamer_t* R);

/* ---- parameter derivatives (the reference's get_param_deriv under -DPARAM_DERIV, deriv_engine.h:71-74) ------------
 * Each call handles ONE system of the batch and ADDS into `table`, which the caller has zeroed; layout = the node's
 * get_param().  They read the outputs, sensitivities and cached lists of the last evaluate_deriv.  Off the MD path. */
/* interaction_graph.h:404-416: hbond_coverage (quadspline coefficients), environment_coverage (zeros,
 * environment.cpp:62-65); sens_mode as in upk_igraph_grad */
int upk_igraph_param_deriv(const upk_launch_t* L, const upk_igraph_t* G, int system, int sens_mode, const float* sens1,
                           const float* sens2, long sens_sys_stride, int sens_stride, float* table);
/* rotamer.cpp:1064-1066: bead pairs weighted by the beliefs / pair marginals of the last solve */
int upk_rotamer_param_deriv(const upk_launch_t* L, const upk_rotamer_t* R, int system, float* table);
/* placement.cpp:144-160 (fixed placements: [n_layer][n_pos_dim]) */
int upk_placement_param_deriv(const upk_launch_t* L, const upk_placement_t* P, upk_coord_t aff, upk_coord_t out, int system, float* table);
/* environment.cpp:375-389 ([n_restype][n_coeff]) */
int upk_nonlinear_coupling_param_deriv(const upk_launch_t* L, upk_coord_t input, const int* types, int n_coeff, float offset,
                                       float inv_dx, int system, float* table);
/* sum over the elements of output component `comp` (hbond.cpp:436-448: n_hbond) */
int upk_column_sum(const upk_launch_t* L, upk_coord_t c, int comp, int system, float* out);

/* ---- parameter derivatives of ALL systems in one launch (upside_hip_get_param_deriv_all) ---------------------------
 * The same quantities as the one-system launchers above, written whole (no zeroing needed) into table [n_system][n_param]
 * (n_param = the node's get_param() size).  Deterministic: every entry is summed exactly in 64-bit fixed point in LDS and
 * stored once, so a system's table is bit-identical run to run and whatever else shares its batch.  Off the MD path. */
int upk_igraph_param_deriv_all(const upk_launch_t* L, const upk_igraph_t* G, int sens_mode, const float* sens1, const float* sens2,
                               long sens_sys_stride, int sens_stride, float* table);
int upk_rotamer_param_deriv_all(const upk_launch_t* L, const upk_rotamer_t* R, float* table);
int upk_placement_param_deriv_all(const upk_launch_t* L, const upk_placement_t* P, upk_coord_t aff, upk_coord_t out, int n_param, float* table);
int upk_nonlinear_coupling_param_deriv_all(const upk_launch_t* L, upk_coord_t input, const int* types, int n_coeff, int n_param,
                                           float offset, float inv_dx, float* table);
/* n_param = 2 + n_coeff */
int upk_uniform_transform_param_deriv_all(const upk_launch_t* L, upk_coord_t in, const float* coeff, int n_coeff, float offset, float inv_dx,
                                          float* table);
int upk_linear_coupling_param_deriv_all(const upk_launch_t* L, upk_coord_t in, const int* types, int n_param, upk_coord_t inact,
                                        int has_inact, int inact_dim, float* table);
/* table [n_system][1] */
int upk_column_sum_all(const upk_launch_t* L, upk_coord_t c, int comp, float* table);
/* acc[p] += sum over s (ascending) of weight[s] * d[s][p], in double; weight NULL = all 1 */
int upk_param_deriv_reduce(const upk_launch_t* L, const float* d, int n_param, const float* weight, double* acc);

/* measured VALU issue ceilings of the device for the pair kernels' launch shape (one 1024-lane workgroup per CU): wave-level
 * fp32 FMA instructions per second, rates[0] for a dependent scalar chain, rates[1] with four independent chains per lane */
int upk_calibrate_valu(double* rates);

/* ---- optional restraint / external-field nodes (not emitted by the README configuration) ------------------------- */
/* single-atom potentials on pos; par is [n][8]:
 *   kind 0 atom_pos_spring (bonds.cpp:9-50)    x0[3], k
 *   kind 1 tension         (bonds.cpp:53-90)   tension_coeff[3]
 *   kind 2 AFM             (bonds.cpp:93-168)  k, starting_tip_pos[3], pulling_vel[3]; `time` = time_estimate
 *   kind 3 z_flat_bottom   (bonds.cpp:377-427) z0, radius, k
 * contrib: (n,3) contribution rows of pos' scatter plan.
 * System s reads par + s * par_stride (0 = one row shared by every system, n * 8 = a row per system) */
int upk_point_potential_strided(const upk_launch_t* L, int kind, upk_coord_t pos, const int* id, const float* par, long par_stride, int n,
                                float time, float* contrib, long contrib_stride, float* pot_terms);
/* contact (sidechain_radial.cpp:139-205): id (n,2); par [n][4] = energy, dist, 1/width, cutoff; contrib (n,2,3); par_stride as
 * above (0 or n * 4) */
int upk_contact_strided(const upk_launch_t* L, upk_coord_t bead, const int* id, const float* par, long par_stride, int n, float* contrib,
                        long contrib_stride, float* pot_terms);
/* constant (bonds.cpp:550-587), slice (bonds.cpp:589-621) */
int upk_broadcast_rows(const upk_launch_t* L, const float* value, upk_coord_t out);
int upk_slice_fwd(const upk_launch_t* L, upk_coord_t in, const int* id, upk_coord_t out);
int upk_slice_bwd(const upk_launch_t* L, upk_coord_t self, float* contrib, long contrib_stride);
/* uniform_transform (environment.cpp:158-235); jac [S][n_elem] */
int upk_uniform_transform_fwd(const upk_launch_t* L, upk_coord_t in, const float* coeff, int n_coeff, float offset, float inv_dx,
                              upk_coord_t out, float* jac);
int upk_uniform_transform_bwd(const upk_launch_t* L, upk_coord_t in, upk_coord_t self, const float* jac);
int upk_uniform_transform_param_deriv(const upk_launch_t* L, upk_coord_t in, const float* coeff, int n_coeff, float offset, float inv_dx,
                                      int system, float* table);
/* linear_coupling_uniform / linear_coupling_with_inactivation (environment.cpp:237-321) */
int upk_linear_coupling(const upk_launch_t* L, upk_coord_t in, const int* types, const float* couplings, upk_coord_t inact, int has_inact,
                        int inact_dim, float* pot_terms);
int upk_linear_coupling_param_deriv(const upk_launch_t* L, upk_coord_t in, const int* types, upk_coord_t inact, int has_inact, int inact_dim,
                                    int system, float* table);
/* membrane_potential (membrane_potential.cpp:13-155) */
typedef struct {
    int n_res, n_donor;
    const int *cb_index, *env_index, *restype;         /* [n_res] */
    const float *cov_midpoint, *cov_sharpness;          /* [n_restype] */
    const float *cb_coeff, *cb_table; int cb_nx;        /* monomial pieces [n_restype][cb_nx-1][4], raw table [n_restype][cb_nx] */
    const float *uhb_coeff, *uhb_table; int uhb_nx;     /* 2 layers: unpaired donor, unpaired acceptor */
    float cb_z_shift, cb_z_scale, uhb_z_shift, uhb_z_scale;
} upk_membrane_t;
int upk_membrane(const upk_launch_t* L, const upk_membrane_t* M, upk_coord_t cb, upk_coord_t env, upk_coord_t hb, float* pot_terms);

/* protein_hbond finish (src/hbond.cpp:320-335): copy the 6 infer components, out[6] = 1 - exp(-sum) */
int upk_protein_hbond_finish(const upk_launch_t* L, upk_coord_t infer, upk_coord_t out);
/* protein_hbond backward prologue/epilogue (src/hbond.cpp:343-365): sens_scaled and pass-through */
int upk_protein_hbond_bwd_pre(const upk_launch_t* L, upk_coord_t self, float* sens_scaled);
int upk_protein_hbond_passthrough(const upk_launch_t* L, upk_coord_t self, upk_coord_t infer, const int* loc1, int n1,
                                  const int* loc2, int n2);

/* ---- replica exchange (src/main.cpp:227-275) ----
 * One swap set, whoever issues it (the engine's temperature and Hamiltonian sets, csrc/comm_rccl.cpp over a ladder spread across
 * ranks), is these launches on the engine's stream, everything device-resident:
 * upk_sum_potentials: out[s] = total potential of system s (node order, fp32: the bits of the host sum).
 * upk_exchange_decide: Metropolis verdicts of the pairs (device array (n_pair,2)) with the REPLICA_EXCHANGE stream of the round's
 *   counter generator, one uniform per rejectable pair.  e_new == NULL: temperature exchange of one Hamiltonian on e_old; accepted
 *   pairs trade their e_old entries, so the later sets of the attempt need no evaluation.  e_new given: Hamiltonian set, e_old / e_new
 *   = energies before / after the pairs traded coordinates; nothing is traded.  beta = 1/T, indexed like the energies.
 *   draw0 >= 0: first draw of the set, < 0: continue from *draw_io; accepted [n_pair + 1] (last = next draw), *draw_io = next draw.
 * upk_swap_system_pairs: trade the coordinates of disjoint pairs of systems: all of them (accepted == NULL) or those with
 *   accepted[p] == want.
 * upk_replica_apply: the move of the accepted pairs where partners may live on another rank (plan[p] = {kind, a, b}: 1 = both local,
 *   swap; 2 = local system a takes staging row b, the partner's coordinates received from its rank). */
int upk_sum_potentials(const upk_launch_t* L, const float* const* node_pot, int n_node, float* out);
int upk_exchange_decide(const upk_launch_t* L, float* e_old, const float* e_new, const float* beta, int n_pair, const int* pairs,
                        uint32_t seed, uint64_t round, int draw0, int* draw_io, int* accepted);
int upk_swap_system_pairs(const upk_launch_t* L, upk_coord_t pos, int n_pair, const int* pairs, const int* accepted, int want);
int upk_replica_apply(const upk_launch_t* L, upk_coord_t pos, int n_pair, const int* plan, const int* accepted, const float* staging);

/* ---- learned backbone potential (src/nn.cpp: backbone_featurizer, conv1d, scaled_sum), csrc/kernels_nn.hip ----
 * backbone_featurizer: out row r = (sin phi, cos phi, sin psi, cos psi, don, acc); phi, psi = columns 0, 1 of rama row rama_idx[r],
 * don / acc = column 6 of hbond rows hbond_idx[2r] / hbond_idx[2r+1] (0 where the index is -1).  The backward pass ADDS into the
 * parents' sens with plain read-modify-writes: the indices must be distinct (checked by the node). */
int upk_backbone_featurizer_fwd(const upk_launch_t* L, upk_coord_t rama, upk_coord_t hbond, const int* rama_idx, const int* hbond_idx, upk_coord_t out);
int upk_backbone_featurizer_bwd(const upk_launch_t* L, upk_coord_t rama, upk_coord_t hbond, const int* rama_idx, const int* hbond_idx, upk_coord_t self);
/* conv1d: out[r,co] = act(bias[co] + sum_{w,ci} in[r+w,ci] * weights[w,ci,co]), r < n_in - W + 1.  param = weights [W][C_in][C_out]
 * followed by bias [C_out] in ONE device array (set_param rewrites it in place).  Every sum runs in one fixed order (w, then the
 * channel, ascending) whatever the batch or the tiling. */
enum { UPK_ACT_IDENTITY = 0, UPK_ACT_RELU = 1, UPK_ACT_TANH = 2 };
typedef struct { const float* param; int W, C_in, C_out, act; } upk_conv1d_t;
/* 1 when the layer's tiles (a slice of the weights + the rows of a tile and their halo) fit the workgroup's LDS for the forward,
 * backward and weight-gradient kernels: always for W <= 15 and C_in, C_out <= 64 */
int upk_conv1d_fits(int W, int C_in, int C_out);
int upk_conv1d_fwd(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out);
/* in.sens[j,ci] += sum_{w,co} g[j-w,co] * weights[w,ci,co], g = out.sens * act'(out.out): a gather over the <= W rows that read j */
int upk_conv1d_bwd(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out);
/* dW[w,ci,co] = sum_r g[r,co] * in[r+w,ci], db[co] = sum_r g[r,co] (r ascending), in the layout of param: one system into
 * table [n_param], or every system into table [n_system][n_param] */
int upk_conv1d_param_deriv(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out, int system, float* table);
int upk_conv1d_param_deriv_all(const upk_launch_t* L, const upk_conv1d_t* P, upk_coord_t in, upk_coord_t out, float* table);
/* scaled_sum: in.sens[r] += *scale, pot_terms[s][r] = *scale * in[r] (pot_terms may be NULL); scale is a device value */
int upk_scaled_sum(const upk_launch_t* L, upk_coord_t in, const float* scale, float* pot_terms);

/* ---- TorusDBN backbone prior (src/hmm.cpp: torus_dbn :218-358, fixed_hmm :38-216), csrc/kernels_hmm.hip ----
 * torus_dbn: out[r][s] = (prior[restypes[r]][s] + cs_to_emission[6][s]) + sum_{k<6} cs_k(r) * cs_to_emission[k][s], k ascending,
 * cs = (cos phi, sin phi, cos psi, sin psi, cos(phi - psi), sin(phi - psi)), phi, psi = columns 0, 1 of rama row id[r]; n_state is
 * out.width.  Rows 0..5 of cs_to_emission [7][n_state] are the reference constructor's matrix, row 6 the basins' log normalisation.
 * The backward pass contracts self.sens with the matrix (state ascending) and ADDS the chain rule into columns 0, 1 of rama's sens
 * row id[r] with plain read-modify-writes: id must be distinct and in range (checked by the node). */
typedef struct { const int* id; const int* restypes; const float* prior; const float* cs_to_emission; int n_restype; } upk_torus_dbn_t;
int upk_torus_dbn_fwd(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t rama, upk_coord_t out);
int upk_torus_dbn_bwd(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t rama, upk_coord_t self);
/* table[t][s] = sum over r (ascending) with restypes[r] == t of self.sens[r][s]: one system into table [n_restype * n_state], or every
 * system into table [n_system][n_restype * n_state] */
int upk_torus_dbn_param_deriv(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t self, int system, float* table);
int upk_torus_dbn_param_deriv_all(const upk_launch_t* L, const upk_torus_dbn_t* P, upk_coord_t self, float* table);
/* fixed_hmm over the rows index[0 .. n_residue) of `in` (width n_state <= upk_fixed_hmm_max_state()): emission b_r = exp(e_min_r -
 * in[index[r]]), scaled forward recursion f_r = normalise((f_{r-1} T) * b_r), T [n_state][n_state] and *offset device values;
 * potential[s] = *offset * (n_residue - 1) + sum_r e_min_r - sum_r log(norm_r) (accumulated in fp64; potential may be NULL), and the
 * posterior marginal of residue r is ADDED to in.sens row index[r] (index distinct and in range, checked by the node).  One wavefront
 * per system; fwd [n_system][n_residue][row_stride] keeps the forward beliefs of the last call. */
typedef struct { const float* T; const float* offset; const int* index; int n_residue, n_state, row_stride; float* fwd; float* w; } upk_fixed_hmm_t;
int upk_fixed_hmm_max_state(void);
int upk_fixed_hmm(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, float* potential);
/* expected transition counts table[i][j] = sum over the edges of the normalised T[i][j] f_{r-1}[i] b_r[j] beta_r[j] (hmm.cpp:188-197),
 * r ascending, from the beliefs and energies of the last upk_fixed_hmm call; w (as fwd) is scratch.  One system, or every system into
 * table [n_system][n_state * n_state].  Off the MD path. */
int upk_fixed_hmm_param_deriv(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, int system, float* table);
int upk_fixed_hmm_param_deriv_all(const upk_launch_t* L, const upk_fixed_hmm_t* H, upk_coord_t in, float* table);

/* ---- collective variables of every system (upside_hip_cv_*), csrc/kernels_cv.hip ---------------------------------------------
 * n_cv CVs, each over its own atom list atoms[atom_start[c] : atom_start[c+1]] (CSR):
 *   UPK_CV_RG        sqrt of the mean squared distance to the list's centroid
 *   UPK_CV_RMSD      minimum RMSD over proper rigid motions to ref rows aux_start[c].. (one per list atom, CENTRED by the host, fp64);
 *                    ref_g[c] = sum of their squared norms
 *   UPK_CV_CONTACTS  the list is interleaved pairs; mean over pairs of 1 / (1 + exp(beta[c] * (r - lambda[c] * r0))), r0 = r0[aux_start[c] + pair]
 *   UPK_CV_DISTANCE  |x(atoms[0]) - x(atoms[1])|
 *   UPK_CV_DIHEDRAL  the torsion of the list's 4 atoms in radians, in (-pi, pi]: with F = r1 - r2, G = r2 - r3, H = r4 - r3, A = F x G,
 *                    B = H x G it is atan2((B x A) . G, (A . B) |G|) (Blondel & Karplus; the backbone torsions' sign).  PERIODIC, period
 *                    2 pi: the biases below take differences of its values by the nearest image, wrap(d) = d - 2 pi rint(d / 2 pi)
 *   UPK_CV_DIHEDRAL_SIMILARITY  the list is interleaved quadruples; mean over quadruples of 1/2 (1 + cos(phi_i - phi0_i)), in [0, 1],
 *                    phi0_i = dihedral_ref[aux_start[c] + quadruple] (radians).  Not periodic
 *   UPK_CV_PATH_S, UPK_CV_PATH_Z  path CVs over K = path_n_frame[c] frames of the list's n >= 3 atoms (2 <= K <= UPK_CV_PATH_MAX_FRAMES): the
 *                    frames are ref rows aux_start[c] + k n + atom (frame-major, each CENTRED by the host, fp64) and
 *                    path_g[path_frame_start[c] + k] the sum of frame k's squared norms.  With d_k the minimum mean squared deviation
 *                    over proper rigid motions to frame k (Angstrom^2, the square of an rmsd), d_min = min_k d_k and
 *                    w_k = exp(-path_lambda[c] (d_k - d_min)):  path_s = sum_k k w_k / sum_k w_k in [1, K] (k = 1..K),
 *                    path_z = d_min - ln(sum_k w_k) / path_lambda[c] in Angstrom^2.  Not periodic.  The K alignments of one CV run side
 *                    by side (csrc/cv_path_device.h); a path_s and a path_z of the same path each align on their own.  Codes 6 and 7
 *                    are not in use
 * One workgroup per system, every sum in fp64 and in one fixed order, no atomics: a system's row is bit-identical run to run and
 * whatever else shares its batch.  The lists are not staged anywhere, so the only limits are UPK_CV_MAX CVs per definition,
 * UPK_CV_MAX_LIST entries per list (what the launch checks and the 32-bit indices hold) and UPK_CV_PATH_MAX_FRAMES frames per path CV
 * (their alignments are kept in LDS). */
enum { UPK_CV_RG = 0, UPK_CV_RMSD = 1, UPK_CV_CONTACTS = 2, UPK_CV_DISTANCE = 3, UPK_CV_DIHEDRAL = 4, UPK_CV_DIHEDRAL_SIMILARITY = 5,
       UPK_CV_PATH_S = 8, UPK_CV_PATH_Z = 9 };
#define UPK_CV_MAX 64
#define UPK_CV_MAX_LIST (1 << 24)   /* entries of one CV's list */
#define UPK_CV_PATH_MAX_FRAMES 64    /* frames of one path CV: one lane of a wavefront solves each frame's alignment */
typedef struct {
    int n_cv;
    const int *kind, *atom_start, *atoms, *aux_start;   /* [n_cv], [n_cv+1], [atom_start[n_cv]], [n_cv] */
    const double *ref, *ref_g;                          /* [n_ref_atom][3], [n_cv] */
    const float *r0, *beta, *lambda;                    /* [n_contact_pair], [n_cv], [n_cv] */
    const float* dihedral_ref;                          /* [n_similarity_quadruple] */
    const int *path_n_frame, *path_frame_start;         /* [n_cv] (0 for the other kinds), [n_cv] */
    const double* path_g;                               /* [n_path_frame] */
    const float* path_lambda;                           /* [n_cv], Angstrom^-2 */
} upk_cv_t;
/* out [S][n_cv] at the current positions */
int upk_cv_compute(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, float* out);
/* One completed MD round: system s advances rounds[s]; on every `every`-th round it takes sample number n_attempt[s]++, stored at
 * samples[sample][s][0..n_cv) while sample < capacity.  The decision is taken on the device from the system's own counters (equal
 * entries), so the launch replays unchanged from a captured graph. */
typedef struct { unsigned long long* rounds; int* n_attempt; int every, capacity; float* samples; } upk_cv_record_t;
int upk_cv_record(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_record_t* R);
/* cv_restraint (node of the force pass): E[s] = sum_c 1/2 k u^2 with u = max(0, |v_c - center| - flat_width) over the CVs of C, v_c
 * the very bits upk_cv_compute reports (a dihedral: |wrap(v_c - center)|, so center may be any finite number).  par + s * par_stride is system s's row [center | spring_const | flat_width] (3 n_cv floats;
 * stride 0: one row for all -- the cv_restraint node, the only caller, always passes a full table with stride 3 n_cv, so the
 * shared row is not exercised).  Writes dE/dx of every list entry to contrib[s][entry][3] (entry = index into C->atoms: a scatter
 * source of pos with one slot per entry; every slot is written on every launch), the CV values to values[s][n_cv] and, unless
 * pot_terms is NULL, the n_cv energy terms to pot_terms[s][n_cv].  Same kernel shape as upk_cv_compute: one workgroup per system,
 * fp64 sums in one order, no atomics.  An rg, rmsd or distance below UPK_CV_RESTRAINT_VMIN (Angstrom), a contact pair at r = 0 and a
 * torsion whose |G| is below UPK_CV_RESTRAINT_VMIN or whose first or last three atoms are collinear to within 1e-6 in the sine
 * (|A|^2 not above 1e-12 |F|^2 |G|^2, or |B|^2 not above 1e-12 |H|^2 |G|^2; coincident end atoms included) contribute zero force
 * (the energy is still counted; atan2(0, 0) = 0). */
#define UPK_CV_RESTRAINT_VMIN 1e-6
int upk_cv_restraint(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const float* par, long par_stride, float* contrib,
                     long contrib_stride, float* values, float* pot_terms);
/* cv_steer (node of the force pass + an advance per completed MD round): upk_cv_restraint with a centre that moves on a schedule.
 * par + s * par_stride is system s's row [center | rate | center_end | spring_const | flat_width] (5 n_cv floats; par_stride >= 5 n_cv)
 * and clock[s] its completed MD rounds t.  The centre in force is c(t) = center + rate * t in fp64 (product and sum rounded
 * separately), stopped at center_end on the side rate moves it to; d = v - c(t), wrapped for a periodic kind while c(t) itself
 * stays on the unwrapped line.  Outputs as upk_cv_restraint, and centers[s][n_cv] = c(t).  No argument changes between launches. */
int upk_cv_steer(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const float* par, long par_stride, const unsigned long long* clock,
                 float* contrib, long contrib_stride, float* values, float* pot_terms, double* centers);
/* one completed MD round: work[s] += sum_c E_c(v_c, c_c(t + 1)) - E_c(v_c, c_c(t)) in fp64, CVs ascending, with v_c the bits
 * upk_cv_compute reports at the current positions; then clock[s] = t + 1 and centers[s][n_cv] = c(t + 1).  Each system's workgroup
 * owns its entries: no atomics. */
int upk_cv_steer_advance(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const float* par, long par_stride, unsigned long long* clock,
                         double* work, double* centers);
/* cv_metadynamics (node of the force pass + a deposit per completed MD round): the d = C->n_cv <= UPK_METAD_MAX_DIM CVs of C span
 * one space and the bias is a sum of Gaussian hills,
 *   V(v) = sum_h w_h exp(-sum_c (v_c - s_hc)^2 / (2 sigma_c^2)),   dV/dv_c = sum_h -w_h (v_c - s_hc) / sigma_c^2 exp(...)
 * over ALL hills of the system's list (no cutoff, no grid), accumulated in fp64 in one order: lane t takes hills t, t + 256, ...
 * ascending, then the workgroup's fixed-order sum.  v_c is the fp64 value behind the bits upk_cv_compute reports.  In a dihedral's
 * dimension v_c - s_hc is wrap(v_c - s_hc): the nearest image of the hill only, no sum over images, so sigma_c is expected to be
 * well below pi.
 * Hills: hills[list][d + 1][capacity] floats (rows 0..d-1 the centres, row d the weights; consecutive lanes read consecutive
 * hills).  shared = 0: list = system, n_deposit[s] hills visible.  shared = 1: one list for all systems (walkers); deposit k of
 * system s is slot k * n_system + s and n_deposit[s] * n_system hills are visible (the entries of n_deposit are equal).
 * rounds[S], n_deposit[S], n_attempt[S] are device counters each system's workgroup advances for itself: no kernel argument
 * ever changes, so eager launches and a replayed graph give the same series. */
#define UPK_METAD_MAX_DIM 4
typedef struct {
    float* hills; int* n_deposit; int* n_attempt; unsigned long long* rounds;
    const float* sigma;                  /* [d] */
    int capacity, pace, shared; float height, kdT;
} upk_cv_metad_t;
/* force pass: contrib[s][entry][3] = dV/dv_c * dv_c/dx of every list entry (every slot written on every launch, zeros without
 * hills; the small-value rules of upk_cv_restraint), values[s][d], and unless NULL pot_terms[s][1] = V */
int upk_cv_metad(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_metad_t* M, float* contrib, long contrib_stride,
                 float* values, float* pot_terms);
/* one completed MD round: system s advances rounds[s]; on every pace-th round it counts an attempt and, while its deposit fits
 * (shared: while the deposits of ALL walkers fit), appends a hill centred on the float bits upk_cv_compute would report, of weight
 * height (kdT == 0) or height * exp(-V(centre) / kdT) (well-tempered), V over the hills visible before this launch.  A launch
 * reads only slots of earlier deposits and writes its own: no atomics. */
int upk_cv_metad_deposit(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_metad_t* M);

/* ---- MBAR over umbrella and temperature ladders (upside_hip_mbar), csrc/kernels_mbar.hip ---------------------------------------------
 * (The bodies of _denominator and _free_energy, the staging of the states and the host side's refusals and staging are stated once,
 * in csrc/mbar_device.h, for this section, the Gram pass and the bootstrap below.)
 * n_state states over n samples.  The reduced energy of sample n in state k is
 *   u_k(n) = beta[k] * (energy[n] + sum_c 1/2 k_kc max(0, |wrap_c(values[n][c] - center_kc)| - w_kc)^2),
 *   wrap_c(x) = x - period[c] * rint(x / period[c]) where period[c] > 0 (0: the plain difference),
 * rows + k * 3 d = [center | spring_const | flat_width] of state k: the layout of the cv_restraint per-system table.  values are the
 * recorded float32 CV bits; energy == NULL means 0; d = 0 (values, rows unused) with an energy is a temperature ladder.  All
 * arithmetic is fp64; every logsumexp subtracts its exact maximum; no atomics; every sum has one order, so two launches give the same
 * bits.  These three launchers take the stream itself (they belong to no engine) and return the launch's hipError_t, or 94xx for
 * arguments they cannot run (d outside 0 .. UPK_MBAR_MAX_DIM, no state, no sample, a NULL array).
 *   _denominator:  denom[n] = logsumexp over the states with a[l] > -inf, ascending, of a[l] - u_l(n); the caller passes
 *                  a[l] = ln N_l + f_l, and -inf for a state without samples.  One lane per sample; the states pass through LDS in
 *                  tiles of UPK_MBAR_STATE_TILE.
 *   _free_energy:  f[k] = -logsumexp_n (-u_k(n) - denom[n]) for every state.  One workgroup per UPK_MBAR_FE_TILE states; lane t takes
 *                  samples t, t + 256, ... ascending, then the workgroup's fixed-order sum.
 *   _log_weights:  log_w[n] = -u_0(n) - denom[n] + f_target[0] for state 0 of S (the target, passed as a set of one state).
 * upk_mbar_solve is the HOST side of upside_hip_mbar (include/upside_engine_c.h, which states the refusals): every pointer of
 * upk_mbar_problem_t is a host pointer.  It checks the arguments before it touches the device, copies the samples once, iterates
 * and fills the outputs; 0, or 1 with the reason in message. */
#define UPK_MBAR_MAX_DIM 8
#define UPK_MBAR_STATE_TILE 128
#define UPK_MBAR_FE_TILE 4
typedef struct {
    int d, n_state;
    const double* beta;                     /* [n_state] */
    const float* rows;                      /* [n_state][3 d] */
    double period[UPK_MBAR_MAX_DIM];
} upk_mbar_states_t;
typedef struct { long long n; const float* values; /* [n][d] */ const double* energy; /* [n] or NULL */ } upk_mbar_samples_t;
int upk_mbar_denominator(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* a, double* denom);
int upk_mbar_free_energy(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* denom, double* f);
int upk_mbar_log_weights(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* denom, const double* f_target,
                         double* log_w);
typedef struct {
    long long n_sample; int n_state, d;
    const float* values; const double* energy;                    /* host [n_sample][d], [n_sample] or NULL */
    const double* beta; const float* rows; const long long* n_k;  /* host [n_state], [n_state][3 d], [n_state] */
    const double* periods;                                        /* host [d] */
    double tol; int max_iter;
    const double* f0;                                             /* host [n_state] or NULL = 0 */
    int has_target; double beta_target; const float* row_target;  /* host [3 d] or NULL = no bias */
    double *f, *denominators, *log_w, *f_target;                  /* host out [n_state], [n_sample] or NULL, [n_sample], [1] */
    int* n_iter; double* last_delta;                              /* host out, either may be NULL */
} upk_mbar_problem_t;
int upk_mbar_solve(const upk_mbar_problem_t* P, char* message /* host */, int message_len);
int upk_mbar_state_tile(void);      /* UPK_MBAR_STATE_TILE and UPK_MBAR_FE_TILE of the library that was built */
int upk_mbar_fe_tile(void);

/* ---- the MBAR Gram pass (upside_hip_mbar_gram), csrc/kernels_mbar_gram.hip ------------------------------------------------------------
 * M = S->n_state + n_extra columns of the weight matrix over the X->n samples:
 *   W[n][k]                = exp(f[k] - u_k(n) - denom[n])      k < n_state, u_k as above, denom from upk_mbar_denominator
 *   W[n][n_state + j]      = exp(log_extra[j * n + n])          an explicit log-column; -inf is weight 0
 * G[M][M] = W^T W and colsum[M] = the column sums of W, all fp64, no atomics, one summation order (two launches give the same bits),
 * G bitwise symmetric (the upper triangle of UPK_MBAR_GRAM_TILE^2 tiles is computed with v_mfma_f64_16x16x4_f64 and mirrored).  W is
 * generated in slabs of upk_mbar_gram_rows(M, workspace_bytes) samples into workspace (device memory) and never held whole:
 * that is (workspace_bytes - upk_mbar_gram_partial_bytes(M)) / (8 * M rounded up to the tile) rounded down to UPK_MBAR_GRAM_GRANULE
 * rows.  The partial bytes hold the partial sums of the ranges a slab is cut into where M < 2048 leaves too few tiles to fill the
 * device (a function of M alone, 0 from M = 1985 on, at most 64 MB); they are added in ascending order.  With G == NULL only colsum is
 * computed, and workspace is not used.  Every pointer but S and X is a device pointer.  Returns the launch's hipError_t, 9404 for
 * arguments it cannot run (those of the launchers above; f or colsum NULL; n_extra < 0 or without log_extra; M above
 * UPK_MBAR_GRAM_MAX_COLUMNS), 9405 for a workspace below one granule of rows when G is wanted.
 * upk_mbar_gram_solve is the HOST side of upside_hip_mbar_gram (include/upside_engine_c.h states the refusals): host pointers, the
 * checks before any device call, denominators from f and n_k, a workspace whose size depends on M alone; 0, or 1 with the reason. */
#define UPK_MBAR_GRAM_TILE 64
#define UPK_MBAR_GRAM_GRANULE 32
#define UPK_MBAR_GRAM_MAX_COLUMNS 8192
#define UPK_MBAR_GRAM_MAX_WORKSPACE 536870912ull      /* 512 MB */
int upk_mbar_gram(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* denom, const double* f,
                  int n_extra, const double* log_extra /* [n_extra][n] */, double* G /* [M][M] or NULL */, double* colsum /* [M] */,
                  void* workspace, size_t workspace_bytes);
int upk_mbar_gram_tile(void);                                    /* UPK_MBAR_GRAM_TILE of the library that was built */
size_t upk_mbar_gram_partial_bytes(int m);                       /* the front of the workspace that holds partial sums; 0 for large M */
long long upk_mbar_gram_rows(int m, size_t workspace_bytes);     /* the slab length upk_mbar_gram takes from a workspace; 0: too small */
typedef struct {
    long long n_sample; int n_state, d;
    const float* values; const double* energy;                    /* host, as in upk_mbar_problem_t */
    const double* beta; const float* rows; const long long* n_k;
    const double* periods;
    const double* f;                                              /* host [n_state], finite */
    int n_extra; const double* log_extra;                         /* host [n_extra][n_sample]; -inf allowed, NaN and +inf refused */
    double *G, *colsum, *denominators;                            /* host out [M][M] or NULL, [M], [n_sample] or NULL */
} upk_mbar_gram_problem_t;
int upk_mbar_gram_solve(const upk_mbar_gram_problem_t* P, char* message /* host */, int message_len);

/* ---- the MBAR bootstrap (upside_hip_mbar_bootstrap), csrc/kernels_mbar_boot.hip --------------------------------------------------------
 * Replicates of one MBAR problem (S, X as above), replicate b weighting sample i by the unsigned 16-bit count counts[b * n + i], solved
 * together; include/upside_engine_c.h states the definitions.  The replicates are the second axis of every grid: active[slot] is the
 * replicate that slot = blockIdx.y serves (n_active of them, at most UPK_MBAR_BOOT_MAX_CHUNK), so a converged replicate leaves the
 * grid and nothing is moved.  a, f: [replicate][n_state]; denom, f_new, delta: [slot]...; every pointer but S and X is a device
 * pointer.  fp64, exact maxima, no atomics, one order per sum, and no workgroup reads what another replicate's workgroups wrote: the bits of a
 * replicate depend neither on n_active nor on the other replicates.  The launchers return the launch's hipError_t or 941x for
 * arguments they cannot run.
 *   _log_counts:   log_count[c] = ln c for c = 0 .. 65535 (-inf at 0): the table the two passes below read.
 *   _denominator:  denom[slot * n + i] = logsumexp over the states with a[b][l] > -inf of a[b][l] - u_l(i), b = active[slot].
 *   _free_energy:  f_new[slot * n_state + k] = -logsumexp_{i : c_b(i) > 0} (ln c_b(i) - u_k(i) - denom[slot * n + i]); one workgroup per
 *                  UPK_MBAR_FE_TILE states of one replicate, lane t takes samples t, t + 256, ... ascending.
 *   _update:       for b = active[slot]: f[b] = f_new[slot] - f_new[slot][0], a[b] = ln_n + f[b] (ln_n[k] = ln N_k, -inf for N_k = 0),
 *                  delta[slot] = max_k |f[b][k] - its value before| (a NaN is kept).
 *   _columns:      column[b * n_column + j] = -logsumexp_{i : c_b(i) > 0} (ln c_b(i) + log_numerator[j * n + i] - denom[slot * n + i]),
 *                  -inf entries skipped, +inf where nothing contributes.
 * upk_mbar_boot_chunk: the replicates whose denominators fit workspace_bytes, workspace_bytes / (8 n_sample), at most
 * UPK_MBAR_BOOT_MAX_CHUNK; 0: not even one.
 * upk_mbar_boot_solve is the HOST side of upside_hip_mbar_bootstrap (which states the refusals): host pointers, the checks before any
 * device call, one copy of the samples, chunks of upk_mbar_boot_chunk(n_sample, workspace_bytes) replicates each run to convergence
 * with one synchronisation per iteration; workspace_bytes = 0 means UPK_MBAR_GRAM_MAX_WORKSPACE, more than that is refused.  0, or 1
 * with the reason in message. */
#define UPK_MBAR_BOOT_MAX_CHUNK 32768
int upk_mbar_boot_log_counts(void* stream, double* log_count /* [65536] */);
int upk_mbar_boot_denominator(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* a, const int* active,
                              int n_active, double* denom);
int upk_mbar_boot_free_energy(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const unsigned short* counts,
                              const double* log_count, const int* active, int n_active, const double* denom, double* f_new);
int upk_mbar_boot_update(void* stream, int n_state, const double* ln_n, const int* active, int n_active, const double* f_new, double* f,
                         double* a, double* delta);
int upk_mbar_boot_columns(void* stream, long long n_sample, const unsigned short* counts, const double* log_count, const int* active,
                          int n_active, const double* denom, int n_column, const double* log_numerator, double* column);
long long upk_mbar_boot_chunk(long long n_sample, size_t workspace_bytes);
typedef struct {
    long long n_sample; int n_state, d;
    const float* values; const double* energy;                    /* host, as in upk_mbar_problem_t */
    const double* beta; const float* rows; const long long* n_k;
    const double* periods;
    const int* state_of_sample;                                   /* host [n_sample] */
    int n_replicate; const unsigned short* counts;                /* host [n_replicate][n_sample] */
    double tol; int max_iter;
    const double* f0;                                             /* host [n_state] or NULL = 0 */
    int n_column; const double* log_numerator;                    /* host [n_column][n_sample]; -inf allowed, NaN and +inf refused */
    size_t workspace_bytes;                                       /* of the denominators; 0 = UPK_MBAR_GRAM_MAX_WORKSPACE */
    double *f_boot, *column_boot;                                 /* host out [n_replicate][n_state], [n_replicate][n_column] */
    int* n_iter; double* last_delta;                              /* host out [n_replicate], either may be NULL */
} upk_mbar_boot_problem_t;
int upk_mbar_boot_solve(const upk_mbar_boot_problem_t* P, char* message /* host */, int message_len);

/* The counts drawn on the device (upside_hip_mbar_bootstrap_drawn and upside_hip_mbar_bootstrap_counts of include/upside_engine_c.h, which
 * states the draw): the circular block bootstrap per state, from the counter-based Threefry4x32-20.
 * upk_mbar_boot_draw fills counts[slot][n_sample] (uint16, device) for the n_replicate replicates first_replicate + slot.  The samples
 * of state k are the positions start[k] .. start[k + 1] - 1 of the GROUPED order (start: device [n_state + 1], start[0] = 0,
 * start[n_state] = n_sample); length[k] (device [n_state]) is the block length of state k, clipped to 1 .. n_k[k] by the caller;
 * position p of the grouped order is sample order[p] (device [n_sample], the stable argsort of state_of_sample), or p where order is
 * NULL.  A state of at most UPK_MBAR_BOOT_DRAW_TILE samples is counted by one workgroup in LDS (integer LDS atomics) and stored once;
 * a larger one is counted by integer global atomics into scratch[slot][n_sample] (device int32, zeroed by the launcher), then narrowed
 * to uint16 and stored.  largest_state = max_k n_k[k]: scratch may be NULL where it does not exceed the tile.  Integer sums have no
 * order, so both paths give the bits of the definition.  A count above 65535 is stored as 65535 and
 * *flag = min(*flag, (first_replicate + slot) << 32 | k); the caller sets *flag (device) to all ones before.  Every pointer is a device
 * pointer.  Returns the launch's hipError_t or 9415 for arguments it cannot launch.
 * upk_mbar_boot_solve_drawn is the HOST side of upside_hip_mbar_bootstrap_drawn: upk_mbar_boot_solve with P->counts == NULL and the
 * counts of every chunk drawn in place by upk_mbar_boot_draw (no host array of counts unless D->counts_out is given, no pass over
 * B x N on the host).  upk_mbar_boot_draw_solve is the host side of upside_hip_mbar_bootstrap_counts: the draw alone.  Both: 0, or 1
 * with the reason in message; every refusal returns before any device call. */
#define UPK_MBAR_BOOT_DRAW_TILE 8192
#define UPK_MBAR_BOOT_DRAW_KEY 0x4d424152u   /* key word 2 of the draw's generator */
int upk_mbar_boot_draw(void* stream, int n_state, long long n_sample, const int* start, const int* length, const int* order, int n_replicate,
                       unsigned int first_replicate, unsigned long long seed, long long largest_state, int* scratch, unsigned short* counts,
                       unsigned long long* flag);
typedef struct {
    unsigned long long seed;
    const long long* block;              /* host [n_state] block lengths, each >= 1 (clipped to n_k); NULL = 1 everywhere */
    long long first_replicate;           /* the global index of replicate 0 of the call */
    unsigned short* counts_out;          /* host out [n_replicate][n_sample] or NULL */
} upk_mbar_boot_draw_t;
int upk_mbar_boot_solve_drawn(const upk_mbar_boot_problem_t* P, const upk_mbar_boot_draw_t* D, char* message /* host */, int message_len);
int upk_mbar_boot_draw_solve(int n_state, const long long* n_k, long long n_sample, const int* state_of_sample /* or NULL: grouped */,
                             long long n_replicate, const upk_mbar_boot_draw_t* D, char* message /* host */, int message_len);

/* ---- statistical inefficiency of recorded series (upside_hip_series_inefficiency), csrc/kernels_series.hip ----------------------------
 * upk_series_solve is the HOST side of upside_hip_series_inefficiency (include/upside_engine_c.h states the definition and the
 * refusals): every pointer is a host pointer; the checks come before any device call; 0, or 1 with the reason in message.  The
 * series are centred once on the device, the lagged products of all origins come from one pass of v_mfma_f64_16x16x4_f64 tiles over
 * pieces of at most UPK_SERIES_PIECE samples, in blocks of UPK_SERIES_LAG_BLOCK lags, one launch per block over the series that are
 * not finished.  fp64, no atomics, one summation order.  A tail shorter than UPK_SERIES_MIN_TAIL has no estimate (g = 0,
 * stop_lag = -1).  stats (may be NULL) receives [0] the device time in ms between HIP events around the kernels (copies of the series
 * excluded), [1] the wall time in ms of the whole call after its checks, [2] the lag blocks launched, [3] the sum over them of the
 * unfinished series, [4] the v_mfma_f64_16x16x4_f64 instructions issued per wave summed over waves (2048 flop each). */
#define UPK_SERIES_MIN_TAIL 16
#define UPK_SERIES_LAG_BLOCK 128
#define UPK_SERIES_PIECE 2048
typedef struct {
    int n_series; long long stride;
    const long long* length;                                      /* host [n_series] */
    const double* a;                                              /* host, series k at a[k * stride .. k * stride + length[k]) */
    int n_origin; const long long* origin;                        /* host [n_origin], ascending */
    int mintime; long long max_lag;
    double* g; long long* stop_lag; double *mean, *variance;      /* host out [n_series][n_origin]; mean, variance may be NULL */
    double* stats;                                                /* host out [5] or NULL */
} upk_series_problem_t;
int upk_series_solve(const upk_series_problem_t* P, char* message /* host */, int message_len);
int upk_series_lag_block(void);     /* UPK_SERIES_LAG_BLOCK and UPK_SERIES_PIECE of the library that was built */
int upk_series_piece(void);

/* ---- metadynamics analysis (upside_hip_metad_bias, upside_hip_metad_grid), csrc/kernels_metad.hip ---------------------------------------
 * upk_metad_bias_solve and upk_metad_grid_solve are the HOST sides of the two entry points (include/upside_engine_c.h states the
 * definitions and the refusals): every pointer is a host pointer; the checks come before any device call; 0, or 1 with the reason in
 * message.  The grid solve takes two arguments the public entry point does not pass on: workspace_limit, the bytes a chunk of lists
 * may use (0: UPK_METAD_WORKSPACE; a list that needs more is still run, alone), and path (0: by shape, 1: the direct sum, 2: the
 * factorised sum whatever the shape, d >= 2).  Neither changes a bit of what a path returns.  stats (may be NULL) receives [0] the
 * device time in ms between HIP events around the kernels (the copies in and the last copies out excluded; with several chunks of lists
 * the V_last copies of the earlier ones lie between the events), [1] the wall time in ms of the call after its checks,
 * [2] the exponentials executed by the hill sums (the log-sum-exps not counted), [3] the v_mfma_f64_16x16x4_f64 instructions issued
 * per wave summed over waves (2048 flop each), [4] the path taken (1 or 2), [5] the chunks of lists. */
#define UPK_METAD_MAX_SCALES 8
#define UPK_METAD_MAX_GRID (1 << 22)
#define UPK_METAD_MAX_LIST (1 << 24)
#define UPK_METAD_WORKSPACE ((size_t)1 << 30)
#define UPK_METAD_MIN_FACTORISED 8
typedef struct {
    int n_list, d;
    const long long* hill_start;                                  /* host [n_list + 1] */
    const float *centers, *weights;                               /* host [hills][d], [hills] */
    const double *sigma, *periods;                                /* host [d] */
} upk_metad_hills_t;
typedef struct {
    upk_metad_hills_t H;
    const long long* point_start; const double* points;           /* host [n_list + 1], [points][d] */
    const long long* n_visible;                                   /* host [points] or NULL */
    double* V;                                                    /* host out [points] */
    double* stats;                                                /* host out [6] or NULL */
} upk_metad_bias_problem_t;
typedef struct {
    upk_metad_hills_t H;
    const int* n_axis; const double* axes;                        /* host [d], [sum n_axis] */
    int n_checkpoint; const long long* checkpoints;               /* host [n_list][n_checkpoint] */
    int n_scale; const double* scales;
    double *V_last, *lse;                                         /* host out [n_list][G] or NULL, [n_list][n_checkpoint][n_scale] */
    size_t workspace_limit; int path;
    double* stats;                                                /* host out [6] or NULL */
} upk_metad_grid_problem_t;
int upk_metad_bias_solve(const upk_metad_bias_problem_t* P, char* message /* host */, int message_len);
int upk_metad_grid_solve(const upk_metad_grid_problem_t* P, char* message /* host */, int message_len);

/* ---- pairwise RMSD of frames (upside_hip_frames_create, upside_hip_rmsd_matrix / _nearest / _count), csrc/kernels_rmsd.hip ----------------
 * upk_rmsd_frames_create and upk_rmsd_solve are the HOST sides of the entry points (include/upside_engine_c.h states the definitions and
 * the refusals): the checks come before any device call; 0, or 1 with the reason in message.  A frame set is a upk_rmsd_frames_t made
 * by upk_rmsd_frames_create: the centred coordinates in fp64, component-major, y[(c * n_frame + f) * n_pad + i] with the atoms padded
 * with zeros to n_pad (a multiple of the MFMA k-step of 4), and g[f] = sum_i |y_f,i|^2.  A workgroup (4 waves) owns UPK_RMSD_TILE_ROWS x
 * UPK_RMSD_TILE_COLS frame pairs; a wave owns 16 rows x 32 columns as 2 x 9 accumulators of v_mfma_f64_16x16x4_f64 and each lane solves
 * its eight pairs by cyclic Jacobi on Horn's matrix.  fp64, no atomics, one summation order.  stats (may be NULL) receives [0] the
 * device time in ms between HIP events around the tile kernel (copies excluded), [1] the wall time in ms of the call after its checks,
 * [2] the workgroups launched. */
#define UPK_RMSD_MAGIC 0x75706b52
#define UPK_RMSD_TILE_ROWS 64
#define UPK_RMSD_TILE_COLS 32
#define UPK_RMSD_MATRIX 0
#define UPK_RMSD_NEAREST 1
#define UPK_RMSD_COUNT 2
typedef struct {
    int magic, n_atom, n_pad;                                     /* UPK_RMSD_MAGIC while the set lives */
    long long n_frame;
    double *y, *g;                                                /* device */
    double create_ms[2];                                          /* [0] the copies to the device, [1] the centring kernel (wall, synchronised) */
} upk_rmsd_frames_t;
typedef struct {
    int mode;                                                     /* UPK_RMSD_MATRIX, _NEAREST or _COUNT */
    const upk_rmsd_frames_t *A, *B;
    long long nA, nB;
    const int *ia, *ib;                                           /* host [nA], [nB] positions into the sets, or NULL: all frames in order */
    double cutoff;                                                /* _COUNT */
    double* out;                                                  /* _MATRIX: host out [nA][nB] */
    long long* index; double* dist;                               /* _NEAREST: host out [nA] */
    long long* count;                                             /* _COUNT: host out [nA] */
    double* stats;                                                /* host out [3] or NULL */
} upk_rmsd_problem_t;
int upk_rmsd_frames_create(int n_atom, long long n_frame, const float* pos /* host (n_frame, n_atom, 3) */, upk_rmsd_frames_t** frames,
                           char* message /* host */, int message_len);
void upk_rmsd_frames_free(upk_rmsd_frames_t* frames);
int upk_rmsd_solve(const upk_rmsd_problem_t* P, char* message /* host */, int message_len);

#ifdef __cplusplus
}
#endif
#endif

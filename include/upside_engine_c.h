/* Drop-in boundary of the MI355X-native Upside engine (libupside_hip.so).
 *
 * Part 1 repeats, symbol for symbol, the reference's C-ABI
 *     /root/reference/src/engine_c_library.h:12-32   (+ upside_main, /root/reference/src/main.h:1-3)
 * so that `py/upside_engine.py:19-64` (ctypes) binds to this library unchanged.  Semantics kept:
 *   - construct_deriv_engine opens `potential_file` read-only and builds the DerivComputation graph from
 *     group /input/potential (engine_c_library.cpp:9-20); returns NULL on failure, never throws.
 *   - all other calls return 0 on success, 1 on failure after printing "ERROR: ..." to stderr
 *     (engine_c_library.cpp:37-45); get_param_deriv behaves like a -DPARAM_DERIV build of the reference (:93-100):
 *     the derivative of the potential w.r.t. get_param() of the named node, from the state the last evaluate_deriv
 *     left behind; a node without parameter derivatives has an empty vector (n_param must then be 0).
 *   - pos / deriv are dense row-major (n_atom,3) fp32 HOST buffers owned by the caller (:30-33,57-60);
 *     node outputs are dense (n_elem, elem_width) (:146-149); potential nodes report (1,1).
 *   - evaluate_* always run PotentialAndDerivMode and leave node output/sens inspectable (:34,55).
 * The force pass itself runs as HIP kernels on the current device; if no GPU / kernel image is usable the
 * calls FAIL (return NULL / 1) -- there is no CPU fallback in this library.
 *
 * Part 2 is the batched / device-resident extension the reference has no single call for: its MD loop
 * lives in upside_main (/root/reference/src/main.cpp:616-667).  These entry points keep S independent
 * systems (replicas / ensemble members) of one topology resident in HBM and step them together.
 */
#ifndef UPSIDE_ENGINE_C_H
#define UPSIDE_ENGINE_C_H
#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct DerivEngine;
typedef struct DerivEngine DerivEngine;

/* ---- Part 1: engine_c_library.h:12-32 ------------------------------------------------------ */
DerivEngine* construct_deriv_engine(int n_atom, const char* potential_file, bool quiet); /* engine_c_library.h:12  */
void free_deriv_engine(DerivEngine* engine);                                             /* :13 */
int evaluate_energy(float* energy, DerivEngine* engine, const float* pos);               /* :15 */
int evaluate_deriv(float* deriv, DerivEngine* engine, const float* pos);                 /* :16 */
int set_param(int n_param, const float* param, DerivEngine* engine, const char* node_name);        /* :18 */
int get_param_deriv(int n_param, float* deriv, DerivEngine* engine, const char* node_name);        /* :20 */
int get_param(int n_param, float* param, DerivEngine* engine, const char* node_name);              /* :21 */
int get_output_dims(int* n_elem, int* elem_width, DerivEngine* engine, const char* node_name);     /* :22 */
int get_output(int n_output, float* output, DerivEngine* engine, const char* node_name);           /* :23 */
int get_sens(int n_output, float* output, DerivEngine* engine, const char* node_name);             /* :24 */
int get_value_by_name(int n_output, float* output, DerivEngine* engine,
                      const char* node_name, const char* log_name);                                /* :26-27 */
int clamped_spline_solve(int N, float* bspline_coeff, const float* values);                        /* :29 */
int clamped_spline_value(int N, float* result, const float* bspline_coeff, int nx, float* x);      /* :30 */
int get_clamped_value_and_deriv(int N, float* result, const float* bspline_coeff, int nx, float* x); /* :31 */
int get_clamped_coeff_deriv(int N, float* result, const float* bspline_coeff, float x);            /* :32 */
int upside_main(int argc, const char* const* argv, int verbose);                                   /* main.h:1-3 */

/* ---- Part 2: batched device-resident extension ---------------------------------------------- */

/* select the HIP device used by engines constructed afterwards on this thread (one process per GPU) */
int upside_hip_set_device(int device);

/* Same as construct_deriv_engine but with n_system independent copies (replicas / ensemble members) of
 * the topology, all resident on the current HIP device.  construct_deriv_engine == n_system 1. */
DerivEngine* upside_hip_construct(int n_atom, const char* potential_file, int n_system, bool quiet);
int upside_hip_n_system(DerivEngine* engine);

/* host (n_system, n_atom, 3) <-> device positions / momenta */
int upside_hip_set_pos(DerivEngine* engine, const float* pos);
int upside_hip_get_pos(DerivEngine* engine, float* pos);
int upside_hip_set_mom(DerivEngine* engine, const float* mom);
int upside_hip_get_mom(DerivEngine* engine, float* mom);

/* force pass on all systems from the device-resident positions: energy (n_system) may be NULL
 * (DerivMode, deriv_engine.h:42-45); deriv (n_system,n_atom,3) may be NULL. */
int upside_hip_compute(DerivEngine* engine, float* energy, float* deriv);

/* Thermostat set-up of upside_main (main.cpp:515-523): per-system temperature and seed
 * (seed_s = base_seed + s, main.cpp:459), momenta fully resampled, n_invocations reset. */
int upside_hip_init_md(DerivEngine* engine, const float* temperature, uint32_t base_seed,
                       float thermostat_timescale, float dt, int thermostat_interval_rounds);
/* ... with one seed per system (a run whose systems are spread over several engines keeps seed = base + GLOBAL index) */
int upside_hip_init_md_seeds(DerivEngine* engine, const float* temperature, const uint32_t* seeds,
                             float thermostat_timescale, float dt, int thermostat_interval_rounds);

/* n_round integration cycles (3 leapfrog stages each, deriv_engine.cpp:172-192) with the
 * Ornstein-Uhlenbeck thermostat (thermostat.cpp:9-18) every thermostat_interval rounds; everything
 * stays on the device, the call returns after the stream has drained. */
int upside_hip_run_md(DerivEngine* engine, int n_round);
/* the weights of the three stages of a cycle (IntegratorType, /root/reference/src/deriv_engine.h:230, deriv_engine.cpp:173-180):
 * 0 = Verlet (the default; what main.cpp:663 uses), 1 = Predescu et al. 2012.  Between cycles only. */
int upside_hip_set_integrator(DerivEngine* engine, int type);
/* change the thermostat temperature of every system between run_md calls (simulated annealing, main.cpp:436-442,658-660) */
int upside_hip_set_temperature(DerivEngine* engine, const float* temperature);
/* the same loop counted in MD steps (one force evaluation + one leapfrog stage each, the unit of the reference's
 * "steps/s", main.cpp:677-682); a cycle left unfinished is resumed by the next call. */
int upside_hip_run_steps(DerivEngine* engine, int n_step);

/* Monte-Carlo moves (monte_carlo_sampler.cpp): load /input/pivot_moves and /input/jump_moves of a configuration
 * (returns the number of samplers found, 0 if neither group is present, -1 on error); one MC step of EVERY system at
 * `round` = the round number of main.cpp:628-630: each loaded sampler in the reference's order (pivot: proposal
 * from the Ramachandran proposal map, random stream 2; jump: rigid-body move of a chain segment, stream 3) spends two
 * energy evaluations and a Metropolis test at the system's temperature.  stats (n_system,2) = {n_success,
 * n_attempt} of sampler 0 (pivot) or 1 (jump). */
int upside_hip_load_mc(DerivEngine* engine, const char* config_file);
int upside_hip_mc_step(DerivEngine* engine, uint64_t round);
int upside_hip_mc_stats(DerivEngine* engine, int sampler, int* stats, int reset);
int upside_hip_mc_loaded(DerivEngine* engine, int sampler);

/* recenter (deriv_engine.cpp:37-48) all systems */
int upside_hip_recenter(DerivEngine* engine);
/* the same with the z component left alone when xy_only != 0 (--disable-z-recentering, main.cpp:358-360,416) */
int upside_hip_recenter_axes(DerivEngine* engine, int xy_only);

/* Replica-exchange swap attempt among the systems of THIS engine (main.cpp:227-275): pairs (n_pair,2) are
 * one swap set; energies are evaluated, Metropolis tested with the REPLICA_EXCHANGE random stream
 * (random.h:26, keyed by round) and accepted pairs exchange coordinates.  accepted (n_pair) out.  No system may appear
 * twice in a set ("Overlapping indices in swap set.", as in the reference). */
int upside_hip_replica_swap(DerivEngine* engine, int n_pair, const int* pairs, uint32_t base_seed,
                            uint64_t round, int* accepted);
/* the same for the second and later swap sets of one attempt (main.cpp:249: ONE generator per attempt_swaps call):
 * draw0 = accepted[n_pair] returned for the previous set; accepted has n_pair+1 entries here. */
int upside_hip_replica_swap_from(DerivEngine* engine, int n_pair, const int* pairs, uint32_t base_seed,
                                 uint64_t round, int draw0, int* accepted);
/* a later swap set of the SAME attempt without a new force evaluation: in a temperature-only exchange the accepted pairs
 * of the earlier sets merely traded their energies (the reference re-evaluates, main.cpp:251-259, and gets the same numbers).
 * Refused unless the first set of the same round came before with nothing evaluated and no coordinate or parameter written
 * in between (the attempt's own swaps excepted). */
int upside_hip_replica_swap_next(DerivEngine* engine, int n_pair, const int* pairs, uint32_t base_seed,
                                 uint64_t round, int draw0, int* accepted);

/* Replica exchange ACROSS engines / GPUs.  Each rank all-gathers one energy per system
 * (upside_hip_compute), every rank then calls upside_replica_decide on the identical global arrays: host arithmetic
 * only (no device needed), the same Metropolis test and random stream as main.cpp:251-273 with
 * lboltz_diff = (beta1-beta2)(E1-E2); pairs (n_pair,2) index the GLOBAL system list; accepted has n_pair+1 entries,
 * the last one is the generator position to pass as draw0 for the next swap set of the same round.
 * Accepted pairs exchange coordinates (momenta stay with the temperature slot, main.cpp:244-247): two systems of one
 * engine with upside_hip_swap_systems, otherwise get/set_system_pos around a point-to-point transfer. */
int upside_replica_decide(int n_pair, const int* pairs, const float* beta, const float* energy, uint32_t base_seed,
                          uint64_t round, int draw0, int* accepted);
/* Mixed Hamiltonians (one engine per distinct potential, main.cpp:450-571): the reference's own procedure, main.cpp:251-273 --
 * log-Boltzmann factors of every system before and after trading the coordinates of a set's pairs,
 * lboltz_diff[p] = (new[s1]+new[s2]) - (old[s1]+old[s2]), this Metropolis test on them (same generator, a uniform drawn
 * only for a rejectable pair), rejected pairs traded back.  upside_hip_swap_between moves coordinates device to device. */
int upside_replica_decide_lboltz(int n_pair, const float* lboltz_diff, uint32_t base_seed, uint64_t round, int draw0, int* accepted);
int upside_hip_swap_between(DerivEngine* engine1, int system1, DerivEngine* engine2, int system2);
int upside_hip_get_system_pos(DerivEngine* engine, int system, float* pos);        /* host (n_atom,3) */
int upside_hip_set_system_pos(DerivEngine* engine, int system, const float* pos);
int upside_hip_swap_systems(DerivEngine* engine, int system1, int system2);
/* the same for n_pair disjoint pairs (pairs: host array (n_pair,2)) in one launch: the accepted on-GPU pairs of a swap set */
int upside_hip_swap_system_pairs(DerivEngine* engine, int n_pair, const int* pairs);

/* Replica exchange across GPUs over RCCL / xGMI, one process per GPU, no host staging (csrc/comm_rccl.cpp; reference
 * semantics src/main.cpp:227-275 with the loop of :616-672).  Global system g = rank * n_system + local index, so a rank
 * holds a contiguous block of the temperature ladder and only the pairs straddling a block boundary cross GPUs.
 *   upside_hip_comm_get_unique_id: rank 0 makes the 128-byte ncclUniqueId; the launcher hands it to every rank (file, env,
 *     torch.distributed, MPI ...).  Ranks must be started BEFORE any of them touches the GPU.
 *   upside_hip_comm_init: ncclCommInitRank on the engine's device; temperature_global = the whole ladder (world * n_system).
 *   upside_hip_comm_replica_swap: ONE swap set (pairs of GLOBAL system ids).  first_set != 0: the first set of an attempt
 *     (force pass, device-side energy sum, ncclAllGather of one fp32 per replica); later sets of the attempt reuse the
 *     gathered energies, accepted pairs having traded theirs.  Verdicts are computed on the device, identically on every rank
 *     (Metropolis test and random stream of main.cpp:262-271); coordinates of straddling pairs move by grouped
 *     ncclSend/ncclRecv on the engine's stream; momenta and temperatures stay with the slot.  accepted (n_pair) may be NULL:
 *     then the call enqueues everything and returns without synchronising.
 * With world = 1 the result is bit for bit that of upside_hip_replica_swap_from / _next. */
#define UPSIDE_HIP_COMM_ID_BYTES 128
int upside_hip_comm_get_unique_id(char* id_out /* [128] */);
int upside_hip_comm_init(DerivEngine* engine, int rank, int world, const char* id /* [128] */, const float* temperature_global);
int upside_hip_comm_replica_swap(DerivEngine* engine, int n_pair, const int* pairs_global, uint32_t base_seed, uint64_t round,
                                 int first_set, int* accepted);
/* collective: *first_differing_rank = the lowest rank whose value differs from rank 0's, or -1 when all agree (the command
 * line uses it on the digest of /input/potential, so that a mixed launch ends on every rank together) */
int upside_hip_comm_agree(DerivEngine* engine, unsigned long long value, int* first_differing_rank);
int upside_hip_comm_free(DerivEngine* engine);

/* diagnostics: flags[s] = 1 where system s rebuilt the cached pair list of `node_name` in the last force pass */
int upside_hip_rebuild_flags(DerivEngine* engine, const char* node_name, int* flags);
/* diagnostics: out11 = n1, n2, cap1, cap2, cutoff, cache cutoff, then per-system means of the summed cached list lengths of
   side 1 / side 2 and of the in-range (hit) list lengths of side 1 / side 2, and the sides the MD path walks (bit mask) */
int upside_hip_igraph_stats(DerivEngine* engine, const char* node_name, double* out11);
/* Parity/diagnostic access: the in-range pair list of an interaction-graph node of system `sys` after the
 * last force pass, canonical order of interaction_graph.h:122-157.  Returns n_edge or -1. */
int upside_hip_get_pairlist(DerivEngine* engine, const char* node_name, int sys, int max_edge, int* i1, int* i2);
/* Diagnostic, read only: the lists the pair passes of the LAST force pass walked, for system `sys` and the rows of `side` (1 or 2)
 * of an interaction-graph node (rotamer, hbond_coverage*, environment_coverage, protein_hbond, radial, hbond_sc_radial), copied
 * as they lie on the device.  It launches nothing, builds no side on demand and changes no counter; it waits for the stream and
 * copies that system's slices.  Sizes first, then fill: with ints == floats == NULL only info20 / cutoffs2 / sources are written.
 * Returns 0; 1 on an error (no graph, bad system, bad side); 2 when the MD path does not keep that side; 3 when a buffer is too
 * small (info20[14], info20[15] say what is needed); upside_hip_last_error() states the reason.
 * info20: 0 n_rows, 1 n_other, 2 cap (words per row), 3 symmetric, 4 md_sides (bit mask of the sides kept), 5 graph type,
 *   6 bits per list word on the device, 7 nbr_j_bits (0: a word is the partner's element index; else the index is the low
 *   nbr_j_bits bits and the residue-pair slot lies above them), 8 n_slot of the system (rotamer; else -1), 9 has hit lists (the
 *   radial graphs walk their cached lists), 10 has hlo, 11 has ord, 12 has ordu, 13 elements renumbered, 14 ints needed,
 *   15 floats needed, 16 rows hold the partners above the row only, 17 refines so far, 18 the slot value "none", 19 the system's
 *   rebuild flag.   cutoffs2: cutoff, cache_cutoff (fp32, as the kernels use them).
 * sources: "<node of the rows>\n<node of the other side>", the coordinate nodes the positions were read from.
 * ints, in this order (a section that info20 says is absent is left out): cnt[n_rows], hcnt[n_rows], hlo[n_rows], ord[n_rows],
 *   ordu[n_rows], id of the rows, id of the other side, the caller's element number (orig_of) of the rows, of the other side,
 *   element of the source node (index) of the rows, of the other side, cached words [n_rows][cap], hit words [n_rows][cap]
 *   (words widened to 32 bits, otherwise unchanged).
 * floats: cur_pos of the rows [n_rows][4], of the other side [n_other][4] (what the refine tested), cache_pos of the rows, of the
 *   other side (4th word: the element id's bits), then the source nodes' own x, y, z of this system at the graph's elements:
 *   rows [n_rows][3], other side [n_other][3]. */
int upside_hip_get_walked_lists(DerivEngine* engine, const char* node_name, int sys, int side, int* info20, float* cutoffs2,
                                char* sources, int sources_len, int n_int, int* ints, int n_float, float* floats);
/* ... and the cached residue-pair list of a backbone_pairs node.  info2: n_residue, cap; cutoffs3: skin, dist_cutoff, and the node's
 * potential of this system in the last force pass that asked for energies (written with the lists, and when 2 is returned).
 * ints: cnt[n_residue], residue ids [n_residue], partners [n_residue][cap]; floats: [n_residue][4] the reference centres the NEXT
 * force pass will test the displacements against, then [n_residue][3] the residues' current centres (the alignment node's own rows of
 * this system).  Returns as above; 2 when the node keeps no list. */
int upside_hip_get_backbone_list(DerivEngine* engine, const char* node_name, int sys, int* info2, float* cutoffs3, int n_int, int* ints,
                                 int n_float, float* floats);

/* number of BP sweeps of the last rotamer solve per system (rotamer.cpp:1038-1051) */
int upside_hip_rotamer_iterations(DerivEngine* engine, int* iters);

/* last error text of this thread ("" if none) */
/* get_param_deriv (engine_c_library.h:20) for any system of the batch */
int upside_hip_get_param_deriv(DerivEngine* engine, const char* node_name, int system, int n_param, float* deriv);
/* Parameter derivatives of every system of the batch, for training (e.g. contrastive divergence: <dE/dtheta> over native
 * structures minus the same over simulated frames).  Semantics of get_param_deriv(system): the derivative at the state of the
 * LAST FORCE PASS, not at the current positions -- after set_pos or MD steps, call upside_hip_compute(engine, NULL, NULL) first.
 * n_param = the size of the node's get_param_deriv (= get_param() size; 0 for a node without a derivative, e.g. protein_hbond,
 * for which the calls do nothing and return 0).  Deterministic: a system's derivative is bit-identical run to run and whatever else
 * shares its batch.  Errors (unknown node, wrong n_param, NULL output) return 1 with upside_hip_last_error set.
 *   _get_param_deriv_all: deriv is host (n_system, n_param), row s = upside_hip_get_param_deriv(system s).
 *   _param_deriv_accumulate: enqueues sum[node] += sum over s (ascending) of weights[s] * dE_s/dtheta, in double; weights is host
 *     (n_system), NULL = all 1, negative allowed (one accumulator can hold "native minus simulated"); frames[node] += 1.  Returns
 *     without synchronising the engine's stream.
 *   _param_deriv_read: sum (n_param doubles) and the number of accumulate calls since the last reset (n_frame, never NULL);
 *     reset != 0 clears both after reading. */
int upside_hip_get_param_deriv_all(DerivEngine* engine, const char* node_name, int n_param, float* deriv);
int upside_hip_param_deriv_accumulate(DerivEngine* engine, const char* node_name, const float* weights);
int upside_hip_param_deriv_read(DerivEngine* engine, const char* node_name, int n_param, double* sum, long long* n_frame, int reset);

/* Hamiltonian ladders in one engine: systems whose potentials share their structure (node set, arguments, index datasets,
 * shapes) and differ only in the values of the per-system table (dist/angle/dihedral_spring equil_dist and spring_const,
 * cavity_radial, atom_pos_spring, tension, AFM, z_flat_bottom, contact values, the protein_hbond_energy attribute of
 * hbond_energy).
 *   _construct_files: one system per file, in order (a file may repeat).  NULL, with upside_hip_last_error naming the first
 *     file, node and dataset that differs in a way one engine cannot hold, otherwise.  Systems whose values agree share
 *     their arrays: n copies of one file compute what upside_hip_construct(file, n) computes, bit for bit.
 *   _group_configurations: the grouping upside_main uses (HDF5 only, no device): group_of[i] = group of files[i], groups
 *     numbered by first appearance; returns the number of groups, -1 on failure.  Files that are identical or differ only
 *     in the table's values share a group; UPSIDE_HIP_HAMILTONIAN_BATCH=0 groups by the whole /input/potential instead.
 *   _set_param_system / _get_param_system: set_param / get_param of one system (hbond_energy, cv_restraint, cv_steer).
 *     set_param keeps its meaning (every system); get_param returns system 0's values.  set_param first waits for the MD steps
 *     still in flight on the engine's stream, and it ends the exchange attempt whose energies a _replica_swap_next would reuse.
 *   _hamiltonian_swap: one swap set (main.cpp:251-273) on the engine's stream: energy pass, the pairs trade coordinates,
 *     energy pass, Metropolis verdicts of upside_replica_decide_lboltz (each system's own temperature), refused pairs trade
 *     back.  draw0 >= 0: first draw of the set (0 for the first set of an attempt); draw0 < 0: continue from the draw the
 *     previous set of this engine left on the device.  accepted (n_pair + 1: verdicts, then the next draw) may be NULL: the
 *     call then returns without synchronising. */
DerivEngine* upside_hip_construct_files(int n_atom, int n_file, const char* const* files, bool quiet);
int upside_hip_group_configurations(int n_file, const char* const* files, int* group_of);
int upside_hip_set_param_system(DerivEngine* engine, const char* node_name, int system, int n_param, const float* param);
int upside_hip_get_param_system(DerivEngine* engine, const char* node_name, int system, int n_param, float* param);
int upside_hip_hamiltonian_swap(DerivEngine* engine, int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0,
                                int* accepted);
const char* upside_hip_last_error(void);

/* Collective variables of every system, computed on the device in one launch (csrc/kernels_cv.hip) and recordable during MD with no
 * host round trip.  kind: 0 rg (radius of gyration of the selection), 1 rmsd (minimum over proper rigid motions to a reference given
 * for the same selection), 2 contacts (Q = mean over pairs of 1 / (1 + exp(beta (r_ij - lambda r0_ij)))), 3 distance, 4 dihedral (the
 * torsion of 4 atoms in radians, in (-pi, pi], with the sign of the backbone torsions: PERIODIC, period 2 pi -- cv_restraint and
 * cv_metadynamics take its differences by the nearest image), 5 dihedral_similarity (mean over quadruples of
 * 1/2 (1 + cos(phi_i - phi0_i)), in [0, 1]: helix content with phi0 = the helical (phi, psi), a torsional Q with the native angles).
 *   _cv_define: CSR layout -- atoms[atom_start[c] : atom_start[c+1]] is the selection of CV c (two atoms for a distance, interleaved
 *     pairs for contacts); ref_pos (rows of 3) holds the references of the rmsd CVs back to back in CV order, contact_r0 the r0 of the
 *     contacts CVs' pairs likewise; contact_beta / contact_lambda have n_cv entries (read for contacts CVs only).  Arrays a definition
 *     has no use for may be NULL.  Replaces any earlier definition (and stops a recording); n_cv = 0 clears it.  Refused, with
 *     upside_hip_last_error set and the earlier definition still in force: an unknown kind, an atom out of range, an empty selection,
 *     an rmsd selection under 3 atoms, an odd contacts list, a distance without exactly 2 atoms, r0 <= 0, more than 64 CVs
 *     (UPK_CV_MAX) or more than 2^24 entries in one list (UPK_CV_MAX_LIST); a kind 5 (this entry point carries no reference angles).
 *   _cv_define2: the same with dihedral_ref, the reference angles (radians) of the dihedral_similarity CVs' quadruples back to back in
 *     CV order; NULL where no CV is of that kind.  A dihedral's selection is its 4 atoms, a dihedral_similarity's is interleaved
 *     quadruples.  Further refusals: a dihedral without exactly 4 atoms, a dihedral_similarity list that is no multiple of 4, a
 *     quadruple with a repeated atom, dihedral_ref NULL or not finite where a dihedral_similarity exists.
 *   _cv_define3: the same with the arrays of the path kinds, 8 path_s (progress along a path of K reference frames, in [1, K]) and
 *     9 path_z (distance from the path, Angstrom^2) -- codes 6 and 7 are not in use: path_n_frame (n_cv; K of a path CV, 0 for the other
 *     kinds), path_lambda (n_cv; Angstrom^-2, read for path CVs only) and path_ref_pos (rows of 3: the K * n rows of each path CV, frame
 *     after frame, in CV order; n is the length of the CV's selection).  All three NULL where no CV is of a path kind.  Further
 *     refusals: K < 2 or K > 64 (UPK_CV_PATH_MAX_FRAMES), a path selection under 3 atoms, path_lambda not finite or not positive, frames
 *     not finite, any of the three arrays NULL where a path kind exists (so a kind 8 or 9 through _cv_define or _cv_define2).  A path_s
 *     and a path_z over the same frames each compute their own K alignments.
 *   _cv_load: the same from the group /input/collective_variables of a configuration (datasets kind, atom_start, atoms, ref_pos (n,3),
 *     contact_r0, contact_beta, contact_lambda, the optional dihedral_ref -- absent means empty; its length must be the number of
 *     dihedral_similarity quadruples --, the optional path_n_frame (n_cv) i32, path_lambda (n_cv) f32 and path_ref_pos (rows, 3) f32 --
 *     all three or none; the rows must be the sum of K * n over the path CVs -- and the fixed-length string vector names;
 *     config.add_collective_variables writes it).
 *     Returns the number of CVs, 0 without the group, -1 on error (the convention of upside_hip_load_mc).
 *   _cv_count: the number of CVs defined.
 *   _cv_compute: out is host (n_system, n_cv), at the current device positions; no force pass, pair lists untouched.
 *   _cv_record: from this call on every every_n_round-th completed MD round (three leapfrog stages; counted from the call) appends one
 *     (n_system, n_cv) sample to a device buffer of `capacity` samples, inside upside_hip_run_md / _run_steps, on the engine's stream,
 *     without synchronising.  The sample decision lives on the device, so the eager loop and the captured graph give the same
 *     series.  A full buffer stops storing; further samples are only counted.  every_n_round = 0 stops recording and frees the
 *     buffer; with recording off the MD loop enqueues nothing for it.  Samples follow the slot (temperature / Hamiltonian) like
 *     /output: a replica swap trades coordinates and the slot's series continues.  Monte-Carlo steps take no samples.
 *   _cv_read: samples [first, first + n) into out (n, n_system, n_cv) (n = 0: counts only, out may be NULL); *n_stored samples are held,
 *     *n_attempted were due since the last reset (either may be NULL); reset != 0 empties the buffer, the round count runs on.
 * A system's values are bit-identical run to run, whatever the batch size or its place in the batch, recorded or computed. */
int upside_hip_cv_define(DerivEngine* engine, int n_cv, const int* kind, const int* atom_start /* n_cv+1 */, const int* atoms,
                         const float* ref_pos, const float* contact_r0, const float* contact_beta /* n_cv */,
                         const float* contact_lambda /* n_cv */);
int upside_hip_cv_define2(DerivEngine* engine, int n_cv, const int* kind, const int* atom_start /* n_cv+1 */, const int* atoms,
                          const float* ref_pos, const float* contact_r0, const float* contact_beta /* n_cv */,
                          const float* contact_lambda /* n_cv */, const float* dihedral_ref);
int upside_hip_cv_define3(DerivEngine* engine, int n_cv, const int* kind, const int* atom_start /* n_cv+1 */, const int* atoms,
                          const float* ref_pos, const float* contact_r0, const float* contact_beta /* n_cv */,
                          const float* contact_lambda /* n_cv */, const float* dihedral_ref, const int* path_n_frame /* n_cv */,
                          const float* path_lambda /* n_cv */, const float* path_ref_pos);
int upside_hip_cv_load(DerivEngine* engine, const char* config_file);
int upside_hip_cv_count(DerivEngine* engine);
int upside_hip_cv_compute(DerivEngine* engine, float* out /* host (n_system, n_cv) */);
int upside_hip_cv_record(DerivEngine* engine, int every_n_round, int capacity);
int upside_hip_cv_read(DerivEngine* engine, int first, int n, float* out /* (n, n_system, n_cv) */, long long* n_stored,
                       long long* n_attempted, int reset);
/* The CV values a cv_restraint node saw in the last force pass: out is host (n_system, n_cv of the
 * node).  They are the bits upside_hip_cv_compute gives for the same definition at the same positions.  System 0's row is also
 * get_value_by_name(node, "cv_value").  Returns the node's n_cv, or -1 on error (the node is no cv_restraint); out may be NULL to
 * ask for n_cv alone. */
int upside_hip_cv_restraint_values(DerivEngine* engine, const char* node_name, float* out);
/* cv_metadynamics nodes: the hills live on the device in n_list lists of `capacity` slots (shared = 0: one
 * list per system, list = system; shared = 1: one list, list = 0, deposit k of system s in slot k * n_system + s).  d is the number
 * of CVs of the node.  All return 0, or 1 on error (upside_hip_last_error); any out pointer may be NULL.
 * _read: the visible hills of a list, centers (n_hill, d) and weights (n_hill) into host arrays of at least `capacity` rows, and
 *   n_attempt, the deposits attempted (it runs on when the list is full: n_attempt > deposits stored tells of the overflow).
 * _write: replaces a list by n_hill hills through stream-ordered copies (a captured MD graph sees them in its next replay) and
 *   sets the counters so that deposition continues after them; refuses n_hill > capacity, values that are not finite and, for a
 *   shared list, n_hill that is no multiple of n_system.
 * _values: out (n_system, d), the CV values of the last force pass (the bits upside_hip_cv_compute gives). */
int upside_hip_metad_info(DerivEngine* engine, const char* node_name, int* d, int* capacity, int* n_list);
int upside_hip_metad_read(DerivEngine* engine, const char* node_name, int list, float* centers, float* weights, int* n_hill, long long* n_attempt);
int upside_hip_metad_write(DerivEngine* engine, const char* node_name, int list, const float* centers, const float* weights, int n_hill);
int upside_hip_metad_values(DerivEngine* engine, const char* node_name, float* out);
/* cv_steer nodes: a cv_restraint whose centre moves with each system's own clock (completed MD rounds
 * since the clock was last written) while the work of moving it is accumulated in float64 on the device.  All return 0, or 1 on
 * error (upside_hip_last_error: the node is no cv_steer, ...); any out pointer may be NULL.
 * _info: the node's number of CVs.
 * _read: clock (n_system), work (n_system) and center (n_system, n_cv): the centres in force, as of the last force pass or
 *   completed round (after _write: from the next force pass on).  Synchronises.
 * _write: replaces every system's clock and / or work (NULL: kept) by stream-ordered copies; the next force pass, also one replayed
 *   from a captured graph, sees them.  Refused: a negative clock, work that is not finite.
 * _values: out (n_system, n_cv), the CV values of the last force pass (the bits upside_hip_cv_compute gives); system 0's row is also
 *   get_value_by_name(node, "cv_value").
 * Work and clock belong to the system index: a coordinate swap between systems leaves them where they are. */
int upside_hip_steer_info(DerivEngine* engine, const char* node_name, int* n_cv);
int upside_hip_steer_read(DerivEngine* engine, const char* node_name, long long* clock, double* work, double* center);
int upside_hip_steer_write(DerivEngine* engine, const char* node_name, const long long* clock, const double* work);
int upside_hip_steer_values(DerivEngine* engine, const char* node_name, float* out);

/* MBAR (Shirts & Chodera 2008) on the device over the ladders the engine runs, from recorded series alone (csrc/kernels_mbar.hip):
 * the free energies of n_state states ("windows") from n_sample samples, by self-consistent iteration in float64.  No engine is
 * needed; every array is a HOST array; the call runs on a stream of its own on the current device and returns when it is done.
 *   sample n: values[n][0..d) (float32: the recorded CV bits; d may be 0, values then unused) and energy[n] (the unbiased potential;
 *     NULL = 0).  The samples are copied to the device once, not once per iteration.
 *   state k: beta[k], the row rows[k][0..3d) = [center | spring_const | flat_width] in the layout of the cv_restraint per-system
 *     table, and its sample count n_k[k] >= 0 (the samples need not be sorted by state; only the counts enter).
 *   periods[c]: the period of CV c, 0 = not periodic (2 pi for a dihedral).
 *   u_k(n) = beta[k] (energy[n] + sum_c 1/2 spring_const_kc max(0, |wrap_c(values[n][c] - center_kc)| - flat_width_kc)^2),
 *     wrap_c(x) = x - periods[c] rint(x / periods[c]) where periods[c] > 0: the cv_restraint bias.  d = 0 with energy is a
 *     temperature ladder, beta[k] = 1 / T_k.
 *   one iteration from f:  D_n = logsumexp_{l : n_k[l] > 0} (ln n_k[l] + f_l - u_l(n)),  f'_k = -logsumexp_n (-u_k(n) - D_n) for
 *     every k (also where n_k[k] = 0),  f' = f' - f'_0.  Starts from f0 (NULL = 0) and stops when max_k |f'_k - f_k| < tol or after
 *     max_iter iterations (tol = 0: exactly max_iter).
 *   out: f[n_state]; D[n_sample] (may be NULL), the denominators OF THE RETURNED f (one more pass after the last iteration);
 *     *n_iter the iterations run and *last_delta the last max |f' - f| (either may be NULL).
 *   target (has_target != 0): a state of its own with beta_target and row_target[3d] (NULL = no bias).  log_w[n_sample] receives
 *     ln w_n = -u_t(n) - D_n - logsumexp_n (-u_t(n) - D_n), the normalised log-weights of the samples in the target state, and
 *     *f_target = -logsumexp_n (-u_t(n) - D_n) on the scale of f.  has_target == 0: log_w and f_target are not touched.
 * Every logsumexp subtracts its exact maximum (a state 1e5 kT away contributes 0: no overflow, no NaN); no atomics; every sum has
 * one fixed order, so two calls on one input return the same bits.  The iteration here is the self-consistent one; uncertainties and
 * a Newton step come from upside_hip_mbar_gram below.
 * Returns 0, or 1 with upside_hip_last_error set.  Refused before anything is launched or copied: d < 0 or d > 8; n_state < 1;
 * n_sample < 1; n_sample x n_state not below 2^62; beta, n_k or f NULL; values, rows or periods NULL with d > 0; a target without
 * log_w and f_target; tol negative or not finite; max_iter < 1; an n_k below 0; every n_k equal to 0; the n_k not adding up to
 * n_sample; a value, energy, beta, row entry, period, f0 or target entry that is not finite; a negative period, spring_const or
 * flat_width.  Without a HIP device the call fails like every other (no CPU path).  One limit is met only at the first launch, after
 * the samples have been copied: n_sample above 256 (2^31 - 1) (one lane per sample, 256 per workgroup; some 5e11 samples, beyond any
 * device's memory) fails with "launch failed (9401: bad arguments)". */
int upside_hip_mbar(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                    const float* rows, const long long* n_k, const double* periods, double tol, int max_iter, const double* f0,
                    int has_target, double beta_target, const float* row_target, double* f, double* D, double* log_w,
                    double* f_target, int* n_iter, double* last_delta);

/* The Gram matrix of the MBAR weight matrix (csrc/kernels_mbar_gram.hip), from which the asymptotic covariance of the free energies
 * and of reweighted averages (Shirts & Chodera 2008, eq. D8/D9) and the Hessian of the MBAR objective follow.  Samples, states and
 * periods are those of upside_hip_mbar; f[n_state] are the free energies (normally the ones upside_hip_mbar returned).  With
 * D_n = logsumexp_{l : n_k[l] > 0} (ln n_k[l] + f_l - u_l(n)) the weight matrix has M = n_state + n_extra columns,
 *   W[n][k] = exp(f_k - u_k(n) - D_n) for k < n_state,   W[n][n_state + j] = exp(log_extra[j * n_sample + n]),
 * the explicit log-columns carrying target states, observables and profile bins (-inf = weight 0).
 *   out: G[M * M] = W^T W (may be NULL: only colsum is computed, a cheap pass), colsum[M] = the column sums of W, D[n_sample] (may be
 *   NULL).  Float64 throughout, no atomics, one summation order: two calls return the same bits, on any machine state -- the slab of
 *   W that is formed at a time depends on M alone (at most 512 MB; W itself is never held).  G is bitwise symmetric.
 * Limits: M <= 8192; the covariance built from G is a large-sample estimate (upside_hip_mbar_bootstrap below gives bootstrap replicates
 * where few samples are kept) and assumes uncorrelated samples (upside_hip_series_inefficiency below gives the equilibration origin
 * and the stride to subsample a recorded series with).
 * Returns 0, or 1 with upside_hip_last_error set.  Refused before anything is launched or copied: everything upside_hip_mbar refuses
 * about samples, states, counts and periods; n_extra < 0; n_state + n_extra > 8192; colsum or f NULL; log_extra NULL with n_extra > 0;
 * an f that is not finite; a log_extra entry that is NaN or +inf. */
int upside_hip_mbar_gram(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                         const float* rows, const long long* n_k, const double* periods, const double* f, int n_extra,
                         const double* log_extra, double* G, double* colsum, double* D);

/* Bootstrap replicates of an MBAR problem, solved together in one batch on the device (csrc/kernels_mbar_boot.hip): what bootstrap
 * error bars of free energies, averages and profiles are formed from where the asymptotic covariance of upside_hip_mbar_gram is not
 * trusted (few samples per state after decorrelation, poorly overlapping neighbours).  The samples, the states, periods and u_k(n)
 * are those of upside_hip_mbar.  New inputs:
 *   state_of_sample[n]: the state that sample n was drawn from.
 *   counts[b][n]: an unsigned 16-bit count for replicate b = 0 .. n_replicate - 1 and sample n, with
 *     sum_{n : state_of_sample[n] = k} counts[b][n] = n_k[k] for every b and k -- the stratified bootstrap: each state keeps its
 *     sample count.
 * Per replicate, one iteration from f_b is
 *   D_b(n)   = logsumexp_{l : n_k[l] > 0} (ln n_k[l] + f_{b,l} - u_l(n))
 *   f'_{b,k} = -logsumexp_{n : c_b(n) > 0} (ln c_b(n) - u_k(n) - D_b(n)),   then f'_b -= f'_{b,0}
 * Every replicate starts from f0 (the full-sample solution; NULL = 0) and stops when max_k |f' - f| < tol or after max_iter iterations
 * (tol = 0: exactly max_iter).  All replicates iterate together; one that has stopped leaves the grid; the host synchronises once per
 * iteration for the whole batch; the samples are copied once.
 *   columns (n_column >= 0): log_numerator[j][n] carries a target state, an observable or a profile bin WITHOUT D (D differs per
 *     replicate), -inf = weight 0; at the returned f_b
 *       column_boot[b][j] = -logsumexp_{n : c_b(n) > 0} (ln c_b(n) + log_numerator[j][n] - D_b(n)),
 *     +inf for a column with no contributing sample in replicate b (that replicate only).
 *   out: f_boot[n_replicate][n_state]; column_boot[n_replicate][n_column]; n_iter[n_replicate] and last_delta[n_replicate] (either may
 *     be NULL).
 * Float64 throughout; every logsumexp takes its exact maximum first; no atomics; every sum has one order.  The bits of replicate b
 * depend neither on n_replicate, nor on which other replicates are in the batch, nor on when they converge, nor on how the batch is
 * cut into chunks (the denominators of a chunk fill at most 512 MB: 512 MB / (8 n_sample) replicates are solved at a time).
 * Bootstrapping correlated samples one by one underestimates the errors as the asymptotic estimate does: subsample first
 * (upside_hip_series_inefficiency), or resample blocks (upside_hip_mbar_bootstrap_drawn below).
 * Returns 0, or 1 with upside_hip_last_error set.  Refused before anything is launched or copied: everything upside_hip_mbar refuses
 * about samples, states, counts n_k, periods, tol, max_iter and f0; f_boot NULL; n_replicate < 1; counts or state_of_sample NULL; a
 * state index outside 0 .. n_state - 1 or naming a state with n_k = 0; origins that do not add up to n_k; a replicate whose counts of
 * some state do not add up to n_k (the message names the replicate and the state); n_column < 0; n_column > 0 without log_numerator
 * and column_boot; a log_numerator entry that is NaN or +inf; n_sample above 2^26 (not one replicate's denominators fit 512 MB).
 * Without a HIP device the call fails like every other (no CPU path).  It reads no environment switch. */
int upside_hip_mbar_bootstrap(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                              const float* rows, const long long* n_k, const double* periods, const int* state_of_sample,
                              int n_replicate, const unsigned short* counts, double tol, int max_iter, const double* f0, int n_column,
                              const double* log_numerator, double* f_boot, double* column_boot, int* n_iter, double* last_delta);

/* The same batch with the counts DRAWN ON THE DEVICE, chunk by chunk, into the buffer the solve reads (k_mbar_boot_draw*): no host
 * array of counts, no host pass over n_replicate x n_sample, no copy of counts.  The draw is the circular block bootstrap (Politis &
 * Romano 1992) per state, stated so that it can be restated exactly anywhere.  For replicate b (global index from 0) and state k with
 * m = n_k[k] > 0 samples and block length L = min(max(block[k], 1), m) (block NULL: L = 1, the plain stratified bootstrap):
 *   n_block = ceil(m / L); block j has length L, the last one m - L (n_block - 1): the lengths add up to m.
 *   Block j starts at s_j = floor(r_j m / 2^64) (the high 64 bits of the 128-bit product), r_j from Threefry4x32-20 with
 *     counter (q lo32, q hi32, k, b), q = j >> 1, and key (seed lo32, seed hi32, 0x4d424152, 0):
 *     r_j = X[0] | X[1] << 32 for even j, X[2] | X[3] << 32 for odd j.
 *   Block j covers the positions (s_j + t) mod m, t = 0 .. length_j - 1, of the state's samples in their order of appearance
 *     (state_of_sample), and the count of a sample is the number of blocks that cover it.  States with n_k = 0 are skipped.
 * So per state the counts add up to n_k by construction, and a replicate's counts depend on (seed, b, k, n_k[k], block[k]) alone: not
 * on n_replicate, the chunking, the other replicates or the layout.  Integer sums only: the bits are the definition's.  Blocks keep
 * runs of consecutive samples together, so block > 1 asks for each state's samples in time order; block[k] of a few statistical
 * inefficiencies (mbar.block_lengths of the Python layer: 5 g) keeps the error bars of correlated series honest without discarding
 * samples.
 *   upside_hip_mbar_bootstrap_drawn: the arguments of upside_hip_mbar_bootstrap with counts replaced by seed, block ([n_state] or
 *     NULL) and counts_out ([n_replicate][n_sample] uint16 or NULL: the drawn counts, copied back only when asked for).  The
 *     replicates are b = 0 .. n_replicate - 1.  Given the same counts, upside_hip_mbar_bootstrap returns the same bits.
 *   upside_hip_mbar_bootstrap_counts: the draw alone, replicates first_replicate .. first_replicate + n_replicate - 1 into counts_out;
 *     state_of_sample NULL: the samples are grouped by state.
 * A count above 65535 cannot be stored: the device raises a flag and the call fails naming the replicate and the state (the expected
 * coverage of a position is 1, so no legitimate input comes near).
 * Return 0, or 1 with upside_hip_last_error set.  Refused before anything is launched or copied: everything upside_hip_mbar_bootstrap
 * refuses apart from what concerns counts (_counts: about n_state, n_k, n_sample and state_of_sample); block[k] < 1; a first_replicate
 * or n_replicate that is negative, or replicate indices that reach 2^32; counts_out NULL (_counts).  block[k] > n_k[k] is clipped: one
 * block covers the whole series and every count is 1. */
int upside_hip_mbar_bootstrap_drawn(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                                    const float* rows, const long long* n_k, const double* periods, const int* state_of_sample,
                                    int n_replicate, unsigned long long seed, const long long* block, unsigned short* counts_out, double tol,
                                    int max_iter, const double* f0, int n_column, const double* log_numerator, double* f_boot,
                                    double* column_boot, int* n_iter, double* last_delta);
int upside_hip_mbar_bootstrap_counts(int n_state, const long long* n_k, long long n_sample, const int* state_of_sample, long long n_replicate,
                                     long long first_replicate, unsigned long long seed, const long long* block, unsigned short* counts_out);

/* Statistical inefficiency of recorded series at a set of origins (csrc/kernels_series.hip): what equilibration detection (Chodera
 * 2016) and subsampling to uncorrelated samples (Chodera et al. 2007) are built on, and what the covariance from upside_hip_mbar_gram
 * needs of its samples.  No engine is needed; every array is a HOST array; the call runs on a stream of its own on the current
 * device and returns when it is done.  For series k and origin t0 = origin[j], with Tt = length[k] - t0 and the tail
 * A_n = a[k * stride + t0 + n]:
 *   mu = mean(A),  s2 = mean((A - mu)^2)
 *   C(t) = sum_{n=0}^{Tt-1-t} (A_n - mu)(A_{n+t} - mu) / ((Tt - t) s2)            t = 1, 2, ...
 *   g = max(1, 1 + 2 sum_{t=1}^{t_stop-1} C(t) (1 - t / Tt))
 *   t_stop = the first t with (C(t) <= 0 and t > mintime), or t = max_lag + 1, or t = Tt - 1, whichever comes first
 * -- pymbar's statistical_inefficiency(fast=False): every lag is visited.  The number of effectively uncorrelated samples of the
 * tail is Tt / g.
 *   out, each [n_series][n_origin]: g, stop_lag = t_stop, and (either may be NULL) mean = mu and variance = s2.
 *   A tail with Tt < UPK_SERIES_MIN_TAIL = 16 (also an origin at or past the series' end) has no estimate: g = 0, stop_lag = -1
 *   (mean and variance are those of what there is, 0 for nothing).  A tail with s2 == 0 returns g = 1, stop_lag = 0.  Neither is an
 *   error and neither writes a NaN.
 * The mean is taken off before any product is formed (first the series' first value, then the mean of the rest: a series at 1e6
 * with unit scatter loses nothing and a constant series is exactly 0).  Float64 throughout, no atomics, one summation order: two
 * calls return the same bits, and a series' result depends neither on n_series nor on its place among the series.  All origins of
 * a series share one pass over the lagged products (v_mfma_f64_16x16x4_f64 tiles), so the cost is n_series x length x lags.
 * Returns 0, or 1 with upside_hip_last_error set.  Refused before anything is launched or copied: n_series < 1; n_origin < 1;
 * mintime < 1; max_lag < 1; a, length, origin, g or stop_lag NULL; n_series x stride not below 2^40; an origin that is negative or
 * not above the one before it; a length below 1 or above stride; an entry of a series that is not finite.  Without a HIP device the
 * call fails like every other (no CPU path).  It reads no environment switch. */
int upside_hip_series_inefficiency(int n_series, long long stride, const long long* length, const double* a, int n_origin,
                                   const long long* origin, int mintime, long long max_lag, double* g, long long* stop_lag, double* mean,
                                   double* variance);

/* Analysis of metadynamics runs on the device (csrc/kernels_metad.hip): the bias of lists of hills at points and on product grids,
 * and the log-sum-exps of the growing bias that the reweighting offset c(t) of Tiwary & Parrinello 2015 is made of.  No engine is
 * needed; every array is a HOST array; a call runs on a stream of its own on the current device and returns when it is done.
 * List l holds the hills hill_start[l] .. hill_start[l + 1] - 1 in deposit order: centres s_h (d float32) and weights w_h (float32),
 * widened exactly to double; sigma[d] and periods[d] (0 = not periodic) are double and shared by all lists.  With
 *   wrap_c(x) = x - periods[c] rint(x / periods[c])   where periods[c] > 0, else x
 *   e_h(x)    = exp(-1/2 sum_c wrap_c(x_c - s_hc)^2 / sigma_c^2)         (only the nearest image of a hill in a periodic dimension)
 *   V_m(x)    = sum_{h < m} w_h e_h(x)                                   the bias of the first m hills of the list
 * upside_hip_metad_bias: point i of list l (point_start as hill_start) receives V[i] = V_{n_visible[i]}(points[i]) over the hills of
 *   its own list (n_visible NULL: all of them); no hills give exactly 0.  A lane per point, hills staged through LDS, summed ascending;
 *   a workgroup of 256 consecutive points walks only as far as its largest prefix, so frames in time order cost the triangle.
 * upside_hip_metad_grid: the grid is the product of d axes (n_axis[c] values each, concatenated in axes), G = prod n_axis points in C
 *   order, shared by all lists.  Per list, V_last[l][g] = V_m(g) at the last checkpoint m = checkpoints[l][n_checkpoint - 1] (may be
 *   NULL) and lse[l][j][q] = ln sum_g exp(scales[q] V_{checkpoints[l][j]}(g)), every log-sum-exp with its exact maximum taken off.
 *   d = 1, and grids with fewer than 8 rows or columns, are summed directly like the points above.  Otherwise the grid is a matrix
 *   (rows: axis 0 for d = 2, axes 0 x 1 for d = 3 and 4; columns: the rest) and the hills between two checkpoints enter as V += A^T B,
 *   A[h][row] and B[h][col] = w_h x the factors of the row and column dimensions, generated in panels of hills and folded with
 *   v_mfma_f64_16x16x4_f64 tiles: H (rows + cols) exponentials, not H rows cols.
 * Float64 throughout, no atomics, one summation order: two calls return the same bits, and a list's results depend neither on the
 * other lists of the call, nor on its place among them, nor on how the lists are cut into chunks (a chunk's workspace stays below 1 GB).
 * Return 0, or 1 with upside_hip_last_error set.  Refused before anything is launched or copied: d outside 1 .. 4; n_list < 1; a NULL
 * among the required arrays (lse is required exactly when n_scale > 0); hill_start or point_start not starting at 0 or descending; a
 * list above 2^24 hills; 2^31 or more points, or hills in total; a centre, weight, sigma, period, point, axis value or scale that is
 * not finite; sigma <= 0; a negative period; an n_visible or a checkpoint below 0 or above its list's hill count; checkpoints that
 * descend; n_checkpoint < 1; n_scale outside 0 .. 8; an n_axis < 1; G > 2^22.  Without a HIP device the calls fail like every other. */
int upside_hip_metad_bias(int n_list, int d, const long long* hill_start /* n_list+1 */, const float* centers /* [hills][d] */,
                          const float* weights, const double* sigma, const double* periods, const long long* point_start /* n_list+1 */,
                          const double* points /* [points][d] */, const long long* n_visible /* per point, or NULL */, double* V /* per point */);
int upside_hip_metad_grid(int n_list, int d, const long long* hill_start, const float* centers, const float* weights, const double* sigma,
                          const double* periods, const int* n_axis /* d */, const double* axes /* concatenated, sum n_axis */,
                          int n_checkpoint, const long long* checkpoints /* [n_list][n_checkpoint], ascending, repeats allowed */,
                          int n_scale, const double* scales, double* V_last /* [n_list][G] or NULL */,
                          double* lse /* [n_list][n_checkpoint][n_scale], NULL iff n_scale == 0 */);

/* Pairwise RMSD of frames after optimal superposition, on the device (csrc/kernels_rmsd.hip): the distance matrix of two frame sets,
 * the nearest column frame of every row frame, and the number of column frames within a cutoff -- what clustering and the choice of
 * path frames are made of.  No engine is needed; every array is a HOST array; a call runs on a stream of its own on the current
 * device and returns when it is done.  Frame f holds n atoms x_f,i (float32, widened exactly).  In fp64,
 *   c_f = (1/n) sum_i x_f,i      y_f,i = x_f,i - c_f      G_f = sum_i |y_f,i|^2
 *   M_ab[c][d] = sum_i y_a,i[c] y_b,i[d]  (atoms ascending)      lambda_ab = the largest eigenvalue of Horn's 4 x 4 matrix of M_ab
 *   d2_ab = max(0, G_a + G_b - 2 lambda_ab) / n                  d_ab = sqrt(d2_ab)
 * (Horn 1987: the best PROPER rotation, no reflection, equal weights, every pair centred on its own).
 * upside_hip_frames_create centres the frames on the device and returns a handle; it is the only copy of coordinates to the device.
 * The three calls name frame sets by handle; ia / ib are int32 positions into the sets (repeats allowed) or NULL for all frames in
 * order, and nA / nB must then equal the set's size.
 *   upside_hip_rmsd_matrix:  out[p][q] = d of row position p and column position q, row-major (nA, nB).  With the same set and the
 *     same (or no) index list on both sides only pairs p < q are computed, the rest is mirrored and the diagonal is exactly 0.
 *   upside_hip_rmsd_nearest: index[p] = the column POSITION with the smallest d2 (the lowest on equal bits), dist[p] = that d.
 *   upside_hip_rmsd_count:   count[p] = the number of column positions with d2 <= cutoff^2.
 * The 3 x 3 matrices of 16 x 16 frame pairs are nine accumulators of v_mfma_f64_16x16x4_f64; a lane solves its pairs by cyclic
 * Jacobi.  Float64 throughout, no atomics, one summation order: the bits of an entry depend on its two frames (row, column) alone,
 * not on the rest of the call, the pair's place in a tile, or how a call is cut up.  Limits: distances below about
 * 1e-6 sqrt((G_a + G_b) / n) are rounding noise (two copies of a frame come out near 1e-7 A, not 0, off the diagonal); a set holds
 * 3 n_frame n_pad doubles on the device (n_pad = n_atom rounded up to 4); one device.
 * Return 0, or 1 with upside_hip_last_error set.  Refused before any device call: a NULL handle, one that was freed, or a NULL output; n_atom < 3; n_frame < 1;
 * n_atom x n_frame x 3 at or above 2^40; a coordinate that is not finite; different n_atom on the two sides; nA or nB < 1, or not the
 * set's size without an index list; an index outside its set; a cutoff that is negative or not finite; nA x nB at or above 2^40 for
 * the matrix.  A device allocation that fails is refused with its byte count.  Without a HIP device the calls fail like every other. */
int upside_hip_frames_create(int n_atom, long long n_frame, const float* pos /* (n_frame, n_atom, 3) */, void** frames);
void upside_hip_frames_free(void* frames);
int upside_hip_rmsd_matrix(void* A, long long nA, const int* ia, void* B, long long nB, const int* ib, double* out /* (nA, nB) */);
int upside_hip_rmsd_nearest(void* A, long long nA, const int* ia, void* B, long long nB, const int* ib, long long* index, double* dist);
int upside_hip_rmsd_count(void* A, long long nA, const int* ia, void* B, long long nB, const int* ib, double cutoff, long long* count);

/* Per-kernel timing hooks used by bench.py. With profiling enabled every interaction-graph / BP kernel
 * launch is bracketed by HIP events on the engine's stream.  upside_hip_profile_dump writes one text line per
 * kernel: "<kind>:<node> <total ms> <launches> <total algorithmic bytes> <total pair evaluations>" (bytes as defined in
 * DESIGN.md; pair evaluations = in-range pairs of system 0 x systems, per launch of a pair pass). */
int upside_hip_profile_reset(DerivEngine* engine, int enable);
int upside_hip_profile_dump(DerivEngine* engine, char* buf, int buflen);
/* VALU issue ceilings measured on this device with a known-instruction-count kernel of the pair kernels' launch shape
 * (wave-level fp32 FMA instructions per second: rates[0] dependent scalar chain, rates[1] four independent chains per lane):
 * the denominator of bench.py's roofline.igraph */
int upside_hip_calibrate_valu(double* rates /* [2] */);
/* algorithmic bytes of all interaction graphs for one force evaluation of one system */
double upside_hip_igraph_bytes_per_system(DerivEngine* engine);
/* bytes a belief-propagation launch must move at least once (active pair matrices in, marginals out, node rows), all systems, last solve */
double upside_hip_bp_min_bytes(DerivEngine* engine);

/* The per-interval polynomial image of one quadspline parameter row ([angular 1: ka][angular 2: ka][radial wide: k][radial narrow: k],
 * /root/reference/src/bead_interaction.h:30-84) that the LDS-staged pair passes read (layout: upside_hip_kernels.h, param_poly);
 * host arithmetic, exported so that it can be checked without a GPU.  poly_out: upside_hip_quadspline_poly_width floats. */
int upside_hip_quadspline_poly_width(int n_knot_angular, int n_knot);
int upside_hip_quadspline_poly_row(const float* spline_coeff, int n_knot_angular, int n_knot, float* poly_out);

/* Node types defined outside this library (include/upside_hip_plugin.h): load a shared library whose static initialisers
 * register them (the equivalent of linking another node's .cpp into the reference's libupside.so,
 * /root/reference/src/deriv_engine.h:297-335).  Must be called before the configuration that names the node is opened.
 * The libraries listed in the environment variable UPSIDE_HIP_PLUGINS (':'-separated) are loaded by the first engine
 * construction.  Returns 0 on success, 1 on failure (upside_hip_last_error has the dlopen / registry message). */
int upside_hip_load_plugin(const char* shared_library_path);
/* 1 if a node type is registered under exactly this name prefix (built in or from a plug-in), else 0 */
int upside_hip_node_type_registered(const char* name_prefix);

#ifdef __cplusplus
}
#endif
#endif

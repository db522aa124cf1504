// Host-side engine: the reference's differentiable-graph contract re-hosted for device-resident data.
//
// The class names and the plug-in contract follow /root/reference/src/deriv_engine.h:48-335 so that a node
// written for the reference maps one-to-one: DerivComputation (compute_value / propagate_deriv / get_param /
// set_param / get_value_by_name), CoordNode (n_elem, elem_width, output, sens), PotentialNode (potential),
// DerivEngine (nodes, pos, potential, compute, integration_cycle) and the name-prefix registry
// (node_creation_map / add_node_creation_function / RegisterNodeType<T,N>).
// What differs is WHERE data lives: output/sens are device buffers holding n_system independent systems, and a
// node's methods enqueue HIP kernels (through the C launchers of include/upside_hip_kernels.h) on the engine's
// stream instead of computing on the host.  None of the built-in nodes has a host fallback; node types defined outside
// the library plug in through include/upside_hip_plugin.h (device nodes, or HostPotentialNode / HostCoordNode whose maths
// runs on the host behind an explicit synchronisation).
#pragma once
#include "launch_plan.h"
#include "../../include/upside_hip_plugin.h"   // the public part of the contract: DerivComputation, CoordNode, PotentialNode, registry

struct Pos : public CoordNode {   // deriv_engine.h:122-141
    int n_atom;
    Pos(DeviceCtx* c, int n_atom_) : CoordNode(c, n_atom_, 3), n_atom(n_atom_) { library_launchers_only = true; fused_forward = fused_backward = true; }
    void compute_value(ComputeMode) override {}
    void propagate_deriv() override {}
};

// Parameter derivatives of every system of the batch at once (upside_hip_get_param_deriv_all / _param_deriv_accumulate).
// Engine-internal: the built-in nodes that override get_param_deriv implement it; the engine finds it by dynamic_cast, and
// falls back to get_param_deriv(s) system by system for any other node (plug-ins are compiled against the class layout of
// include/upside_hip_plugin.h, which this does not touch).
struct BatchedParamDeriv {
    virtual ~BatchedParamDeriv() {}
    virtual size_t param_deriv_size() const = 0;   // = get_param_deriv(s).size(); 0 = no derivative
    // enqueue, on the engine stream, the derivative of every system into dev [n_system][param_deriv_size()] (written whole),
    // from the state of the last force pass; deterministic: a system's row does not depend on the rest of the batch
    virtual void param_deriv_all(float* dev) = 0;
};

// Hamiltonian ladders in one engine (upside_hip_construct_files): nodes whose parameter VALUES may differ per system while the
// structure (node set, arguments, index datasets, shapes) is shared.  The table lists, per registry prefix, the datasets of the
// node's group (and attributes of the group itself) that may differ; everything else of the node must be byte-identical to
// system 0's file (checked by the engine before load_system_values is called).  Engine-internal, like BatchedParamDeriv; the nodes
// implement it once, over their PerSystemTable (nodes.cpp).
struct PerSystemValueSpec { std::string type; std::vector<std::string> datasets, attributes; };
const std::vector<PerSystemValueSpec>& per_system_value_table();
const PerSystemValueSpec* per_system_value_spec(const std::string& node_name);   // by the registry's prefix rule; NULL = not in the table
struct PerSystemValues {
    virtual ~PerSystemValues() {}
    // read system s's values from its own file's group of this node (system 0's are the node's construction values)
    virtual void load_system_values(int system, hid_t_compat group) = 0;
    // after every system is loaded, before the first force pass: a node whose systems all agree keeps its single array (stride 0)
    virtual void finish_system_values() = 0;
    // per-system set_param / get_param; the nodes whose values come from files only refuse both
    virtual void set_param_system(int system, const std::vector<float>& param) = 0;
    virtual std::vector<float> get_param_system(int system) const = 0;
};

// A checked definition of collective variables (the CSR arrays of upside_hip_cv_define, the rmsd references centred in double) and
// its device copy: shared by the engine's observables (upside_hip_cv_*) and the cv_restraint nodes.
struct CvHostDefinition {
    int n_cv = 0;
    std::vector<int> kind, atom_start, atoms, aux_start; std::vector<double> ref, ref_g; std::vector<float> r0, beta, lambda, dihedral_ref;
    std::vector<int> path_n_frame, path_frame_start; std::vector<double> path_g; std::vector<float> path_lambda;      // the path kinds (their centred frames follow the rmsd references in ref)
};
// throws a message naming the CV and what is wrong with it; touches no device memory
CvHostDefinition cv_check_definition(int n_atom, int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos,
                                     const float* contact_r0, const float* contact_beta, const float* contact_lambda, const float* dihedral_ref,
                                     const int* path_n_frame = nullptr, const float* path_lambda = nullptr, const float* path_ref_pos = nullptr);
// the same from a group with the datasets of /input/collective_variables (`where` names it in messages; `names` is not read; dihedral_ref and the three path_* datasets may be absent)
CvHostDefinition cv_read_definition(hid_t_compat group, int n_atom, const std::string& where);
struct CvDeviceDefinition {
    upk_cv_t C{};
    DevBuf<int> kind, atom_start, atoms, aux_start; DevBuf<double> ref, ref_g; DevBuf<float> r0, beta, lambda, dihedral_ref;
    DevBuf<int> path_n_frame, path_frame_start; DevBuf<double> path_g; DevBuf<float> path_lambda;
    void upload(const CvHostDefinition& d);
};

// A node with work at the end of every completed MD round (cv_metadynamics deposits its hills there).  Engine-internal, found by
// dynamic_cast at finalize(); md_step() enqueues round_end() next to the CV recording, so a captured graph holds the launch, and no
// force pass outside MD (energies, swap sets) ever issues it.  An engine without such a node issues no launch for it.
struct RoundEndWork {
    virtual ~RoundEndWork() {}
    virtual void round_end() = 0;
};

struct DerivEngine {   // deriv_engine.h:145-237
    struct Node {
        std::string name;
        std::unique_ptr<DerivComputation> computation;
        std::vector<size_t> parents, children;
        int germ_exec_level = -1, deriv_exec_level = -1;
    };
    DeviceCtx ctx;
    std::vector<Node> nodes;
    Pos* pos = nullptr;
    std::vector<float> potential;   // [S]

    // MD state (System of main.cpp:93-111, one entry per system)
    DevBuf<float> mom;              // [S][n_atom][4]
    DevBuf<uint32_t> seed; DevBuf<float> mom_scale, noise_scale;
    std::vector<float> temperature; std::vector<uint32_t> seeds;
    float thermostat_timescale = 5.f, dt = 0.009f; int thermostat_interval = 1;
    int integrator_type = 0;        // IntegratorType of deriv_engine.h:230: 0 = Verlet, 1 = Predescu
    uint64_t n_invocations = 0, round_num = 0;      // host mirrors; the thermostat reads the device copy below
    DevBuf<unsigned long long> n_invocations_dev;   // [S] (equal entries: each system's workgroup advances its own)
    void set_invocations(uint64_t n);

    // execution order of one force pass, fixed at finalize() (the BFS of deriv_engine.cpp:124-169 unrolled)
    struct Step { int node; bool backward; bool prepare = false; int batch = -1; bool skip_prepare = false; };   // batch: steps of one merged-launch group (consecutive, mutually independent)
    std::vector<Step> schedule;
    struct Side { hipStream_t stream = nullptr; hipEvent_t fork = nullptr, join = nullptr; bool owns_stream = true; };
    std::map<int, Side> side;                  // node index -> side stream of its prepare() (empty when disabled)
    int last_prepare_step = -1;                // index in `schedule` of the last prepare step
    DevBuf<float*> zero_ptrs; DevBuf<long> zero_sizes; int n_zero = 0;   // every CoordNode's sens, cleared by one launch per force pass
    std::vector<RoundEndWork*> round_end_work;  // in node order (usually empty)

    DerivEngine(int n_atom, int n_system);
    ~DerivEngine();
    void add_node(const std::string& name, std::unique_ptr<DerivComputation> fcn, std::vector<std::string> argument_names);
    Node& get(const std::string& name);
    int get_idx(const std::string& name, bool must_exist = true);
    template <typename T> T& get_computation(const std::string& name) {
        auto c = get(name).computation.get();
        if (!c) throw std::string("impossible pointer value");
        return dynamic_cast<T&>(*c);
    }
    void finalize();
    void print_schedule();
    int n_batch_group = 0;
    void compute(ComputeMode mode, bool keep_pending = false);   // enqueue; no synchronisation.  keep_pending: leave queued fused ops for the caller to extend (MD loop)
    void fetch_potentials();                   // D2H of every PotentialNode::potential + engine total
    void integration_cycle(float dt, float max_force = 0.f);   // deriv_engine.cpp:172-192 (Verlet weights)
    void integration_stage(int stage, float dt, float max_force);   // one force evaluation + leapfrog sub-step (deriv_engine.cpp:172-192)
    int stage_num = 0;                                              // sub-step the next upside_hip_run_steps call starts with
    void md_step();                                                 // thermostat (at round starts) + one integration stage, enqueued
    void run_steps(int n_step);                                     // n_step MD steps; replays a captured hipGraph where it can

    // A launch-bound batch (few systems) spends more time between kernels than in them: 6 MD steps (two rounds: the
    // period of the leapfrog stage AND of the list-parity pattern) are captured once into a hipGraph, side streams
    // included, and replayed.  Invalidated by anything that changes a kernel argument.
    hipGraph_t md_graph = nullptr; hipGraphExec_t md_graph_exec = nullptr;
    bool md_graph_ready = false; int md_graph_parity = 0; uint64_t steps_done = 0, n_compute = 0;
    DevBuf<float> swap_row;           // staging row of upside_hip_swap_between (exchange between engines, or two systems of one)
    bool graph_failed = false;   // capture was refused once: stay on plain launches
    void invalidate_graph();
    bool capture_md_graph();
    // Monte-Carlo pivot sampler (monte_carlo_sampler.cpp): loaded from /input/pivot_moves, all systems step together
    struct Pivot {
        bool loaded = false; upk_pivot_t P{};
        DevBuf<int> atoms, range, restype, stats; DevBuf<float> pot, cdf, pos_copy, delta_lprob, e_old, e_new, temperature;
    } pivot;
    struct Jump {   // rigid-body moves of chain segments (monte_carlo_sampler.cpp:157-251)
        bool loaded = false; upk_jump_t J{};
        DevBuf<int> range, stats; DevBuf<float> sigma_trans, sigma_rot;
    } jump;
    void load_pivot_moves(hid_t_compat input_group);   // throws if the group is malformed
    void load_jump_moves(hid_t_compat input_group);
    void mc_step(uint64_t round);                      // every loaded sampler in the reference's order (pivot, jump): two
                                                       // energy evaluations + proposal + Metropolis each, every system
    void* comm = nullptr; void (*comm_free)(void*) = nullptr;   // replica exchange across GPUs (comm_rccl.cpp), owned by the engine
    // per-node state of the batched parameter derivatives, allocated on first use
    struct ParamDeriv {
        size_t n_param = 0;
        DevBuf<float> table;       // [S][n_param], the last param_deriv_all
        DevBuf<double> sum;        // [n_param], sum over accumulate calls of sum_s weight[s] * table[s]
        DevBuf<float> weight;      // [S], the weights of the last accumulate
        long long n_frame = 0;     // accumulate calls since the last reset
    };
    std::map<int, ParamDeriv> param_derivs;
    ParamDeriv& param_deriv_state(int node);          // n_param known, nothing allocated yet
    const float* param_deriv_all(int node);            // enqueue every system's derivative; the device table [S][n_param]
    void param_deriv_accumulate(int node, const float* weights);   // enqueue sum += weights . table; no synchronisation
    // Replica exchange (main.cpp:227-275), one procedure for every swap set: energies summed on the device, upk_exchange_decide, one
    // coordinate move.  replica_swap (temperature sets of one Hamiltonian), hamiltonian_swap (a second energy pass around the trade) and
    // comm_rccl.cpp (the ladder spread over ranks: an all-gather between the sum and the verdicts) are its three callers.
    struct Exchange {
        DevBuf<const float*> node_pot; int n_node_pot = -1;     // the potential nodes' device arrays in node order, built once
        DevBuf<float> beta, e_old, e_new; std::vector<float> beta_host;
        DevBuf<int> draw, accepted;                             // draw counter of the attempt; verdicts [n_pair + 1] of the last set
        std::map<std::vector<int>, std::unique_ptr<DevBuf<int>>> pairs;   // uploaded once per distinct set
        // the attempt whose energies a later set may reuse: its round, the force passes done when they were summed, the array holding them
        uint64_t round = ~0ull, n_compute = 0; const float* energies = nullptr; bool valid = false;
    } exchange;
    void sum_potentials_into(float* dev);                       // enqueue dev[s] = total potential of the last force pass
    void begin_attempt(uint64_t round, const float* energies);
    void require_attempt(uint64_t round, const float* energies) const;   // throws unless nothing was evaluated or moved since begin_attempt
    void invalidate_attempt() { exchange.valid = false; }      // coordinates or parameters changed outside the attempt's own swaps
    const int* exchange_set(int n_pair, const int* pairs);      // a checked set on the device, beta and the verdict buffers in place
    void read_verdicts(int n_pair, int* accepted);              // accepted [n_pair + 1] of the last set (NULL: nothing, no synchronisation)
    void replica_swap(int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted, bool first_set);
    void hamiltonian_swap(int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted);
    // collective variables of every system (upside_hip_cv_*; kernels_cv.hip).  A definition is replaced whole; recording appends one
    // (n_system, n_cv) sample per `every` completed rounds from inside md_step, the decision taken on the device (captured graphs replay it)
    struct CollectiveVariables : CvDeviceDefinition {
        std::vector<std::string> names;
        DevBuf<float> out;                      // [S][n_cv] of upside_hip_cv_compute
        upk_cv_record_t R{};                    // R.every > 0: recording
        DevBuf<unsigned long long> rounds; DevBuf<int> n_attempt; DevBuf<float> samples;
    } cv;
    void cv_define(int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos, const float* contact_r0,
                   const float* contact_beta, const float* contact_lambda, const float* dihedral_ref, const int* path_n_frame = nullptr,
                   const float* path_lambda = nullptr, const float* path_ref_pos = nullptr);      // throws, leaving the previous definition in force
    void cv_install(const CvHostDefinition& def);      // a checked definition
    void cv_compute(float* out_host);
    void cv_record(int every_n_round, int capacity);
    void cv_read(int first, int n, float* out_host, long long* n_stored, long long* n_attempted, int reset);
    void check_device_errors();                // throws if a capacity overflow was flagged
    void sync();
};

// a swap set over n_system systems: every index in range, no system twice (the reference's messages, main.cpp:171,181)
void check_swap_set(int n_system, int n_pair, const int* pairs);
DerivEngine* initialize_engine_from_hdf5(int n_atom, int n_system, hid_t_compat potential_group, bool quiet = false,
                                         const std::function<void(DerivEngine&)>& before_finalize = nullptr);

// What nodes.cpp tells the C-ABI and upside_main about the nodes of an engine, by node name
int engine_pairlist(DerivEngine& e, const std::string& node_name, int sys, std::vector<std::pair<int, int>>& out);
int engine_rotamer_iterations(DerivEngine& e, std::vector<int>& iters);
int engine_cv_restraint_values(DerivEngine& e, const std::string& node_name, std::vector<float>* out);
std::vector<std::string> engine_metad_nodes(DerivEngine& e);      // the names of the engine's cv_metadynamics nodes
void engine_metad_info(DerivEngine& e, const std::string& node_name, int* d, int* capacity, int* n_list);
void engine_metad_read(DerivEngine& e, const std::string& node_name, int list, float* centers, float* weights, int* n_hill, long long* n_attempt);
void engine_metad_write(DerivEngine& e, const std::string& node_name, int list, const float* centers, const float* weights, int n_hill);
std::vector<float> engine_metad_values(DerivEngine& e, const std::string& node_name);
std::vector<std::string> engine_steer_nodes(DerivEngine& e);      // the names of the engine's cv_steer nodes
int engine_steer_n_cv(DerivEngine& e, const std::string& node_name);
void engine_steer_read(DerivEngine& e, const std::string& node_name, long long* clock, double* work, double* center);
void engine_steer_write(DerivEngine& e, const std::string& node_name, const long long* clock, const double* work);
std::vector<float> engine_steer_values(DerivEngine& e, const std::string& node_name);
int engine_rebuild_flags(DerivEngine& e, const std::string& node_name, std::vector<int>& flags);
int engine_igraph_stats(DerivEngine& e, const std::string& node_name, double* out);
double engine_bp_bytes(DerivEngine& e);
double engine_bp_min_bytes(DerivEngine& e);
double engine_igraph_bytes(DerivEngine& e);


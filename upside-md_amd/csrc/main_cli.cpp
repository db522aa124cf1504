// upside_main for the device engine: the MD loop of /root/reference/src/main.cpp:317-756 for systems that share
// one topology (replicas / ensemble members).  Supported flags are the ones that drive the hot path:
//   --duration --time-step --frame-interval --temperature a,b,c --seed --thermostat-timescale
//   --thermostat-interval --replica-interval --swap-set i-j,k-l (repeatable) --disable-recentering
// Trajectory output follows the reference's /output layout (state_logger.h:17-141, h5_support.cpp:181-274,
// main.cpp:473-541,594-596): extensible chunked datasets pos (frame,1,n_atom,3) f32, kinetic/potential/temperature
// (frame,1) f64, time (frame) f64, replica_index (frame,1) i32 under replica exchange, attribute `invocation`;
// a frame is taken at the START of every frame_interval-th round (frame 0 = the initial structure), after
// recentering, exactly as main.cpp:633-636.  The per-frame stdout line and the final "us/systems/step" line follow
// main.cpp:648-654,677-682.
#include "../../include/upside_engine_c.h"
#include "engine.h"
#include "h5util.h"
#include <chrono>
#include <csignal>
#include <ctime>
#include <fcntl.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

using namespace std;

// ---- /output logger ------------------------------------------------------------------------------------------
namespace {
struct EArray {   // h5_support.cpp:199-274: extensible along dimension 0, chunked (100 frames), shuffle + fletcher32 (+ deflate 1)
    hid_t dset = -1; hid_t type = -1; vector<hsize_t> row; size_t row_size = 1; vector<char> buffer; size_t elem = 4;
    void create(hid_t group, const char* name, hid_t type_, size_t elem_, vector<hsize_t> row_dims) {
        type = type_; elem = elem_; row = row_dims;
        vector<hsize_t> dims{0}, maxd{H5S_UNLIMITED}, chunk{100};
        for (auto d : row) { dims.push_back(d); maxd.push_back(d); chunk.push_back(d ? d : 1); row_size *= d; }
        hid_t space = H5Screate_simple((int)dims.size(), dims.data(), maxd.data());
        hid_t dcpl = H5Pcreate(H5P_DATASET_CREATE);
        H5Pset_chunk(dcpl, (int)chunk.size(), chunk.data());
        H5Pset_shuffle(dcpl);
        H5Pset_fletcher32(dcpl);
        if (H5Zfilter_avail(H5Z_FILTER_DEFLATE) > 0) H5Pset_deflate(dcpl, 1);
        dset = H5Dcreate2(group, name, type, space, H5P_DEFAULT, dcpl, H5P_DEFAULT);
        H5Pclose(dcpl); H5Sclose(space);
        if (dset < 0) throw string("unable to create /output/") + name;
    }
    void push(const void* data) { const char* c = (const char*)data; buffer.insert(buffer.end(), c, c + row_size * elem); }
    void flush() {
        if (!row_size) return;      // (a dataset with an empty row shape never receives records)
        const size_t n_rec = buffer.size() / (row_size * elem);
        if (!n_rec) return;
        hid_t space = H5Dget_space(dset);
        vector<hsize_t> dims(1 + row.size());
        H5Sget_simple_extent_dims(space, dims.data(), nullptr); H5Sclose(space);
        vector<hsize_t> start(dims.size(), 0), count = dims;
        start[0] = dims[0]; count[0] = n_rec; dims[0] += n_rec;
        if (H5Dset_extent(dset, dims.data()) < 0) throw string("H5Dset_extent failed");
        hid_t fspace = H5Dget_space(dset);
        hid_t mspace = H5Screate_simple((int)count.size(), count.data(), nullptr);
        H5Sselect_hyperslab(fspace, H5S_SELECT_SET, start.data(), nullptr, count.data(), nullptr);
        const herr_t rc = H5Dwrite(dset, type, mspace, fspace, H5P_DEFAULT, buffer.data());
        H5Sclose(mspace); H5Sclose(fspace);
        if (rc < 0) throw string("H5Dwrite failed");
        buffer.clear();
    }
    void close() { if (dset >= 0) { flush(); H5Dclose(dset); dset = -1; } }
};
struct OutputLogger {   // one per system / configuration file (H5Logger, state_logger.h:70-141)
    hid_t file = -1, group = -1; int n_buffered = 0;
    EArray pos, kinetic, potential, time, temperature, replica_index, replica_cumulative_swaps, pivot_stats, jump_stats; bool log_replica = false, log_pivot = false, log_jump = false;
    // swap_partners: the other system of every swap pair this system takes part in, in swap-set order (main.cpp:203-217:
    // `replica_swap_partner` written once, `replica_cumulative_swaps` (n_success, n_attempt) per pair and frame)
    void open(const string& path, int n_atom, const string& invocation, bool with_replica_index, bool with_pivot, bool with_jump,
              const vector<int>& swap_partners = vector<int>()) {
        file = H5Fopen(path.c_str(), H5F_ACC_RDWR, H5P_DEFAULT);
        if (file < 0) throw string("Unable to open configuration file at ") + path;
        if (H5Lexists(file, "output", H5P_DEFAULT) > 0) H5Ldelete(file, "/output", H5P_DEFAULT);   // main.cpp:473-477
        group = H5Gcreate2(file, "output", H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT);
        if (group < 0) throw string("unable to create /output in ") + path;
        {   // write_string_attribute(config, "output", "invocation", ...), main.cpp:490
            hid_t st = H5Tcopy(H5T_C_S1); H5Tset_size(st, invocation.size() + 1);
            hid_t sp = H5Screate(H5S_SCALAR);
            hid_t at = H5Acreate2(group, "invocation", st, sp, H5P_DEFAULT, H5P_DEFAULT);
            if (at >= 0) { H5Awrite(at, st, invocation.c_str()); H5Aclose(at); }
            H5Sclose(sp); H5Tclose(st);
        }
        pos.create(group, "pos", H5T_NATIVE_FLOAT, 4, {1, (hsize_t)n_atom, 3});
        kinetic.create(group, "kinetic", H5T_NATIVE_DOUBLE, 8, {1});
        potential.create(group, "potential", H5T_NATIVE_DOUBLE, 8, {1});
        time.create(group, "time", H5T_NATIVE_DOUBLE, 8, {});
        temperature.create(group, "temperature", H5T_NATIVE_DOUBLE, 8, {1});
        log_replica = with_replica_index;
        if (log_replica) {
            replica_index.create(group, "replica_index", H5T_NATIVE_INT, 4, {1});
            EArray partner; partner.create(group, "replica_swap_partner", H5T_NATIVE_INT, 4, {});
            for (int sp : swap_partners) partner.push(&sp);
            partner.close();
            replica_cumulative_swaps.create(group, "replica_cumulative_swaps", H5T_NATIVE_INT, 4, {(hsize_t)swap_partners.size(), 2});
        }
        log_pivot = with_pivot;
        if (log_pivot) pivot_stats.create(group, "pivot_stats", H5T_NATIVE_INT, 4, {2});   // monte_carlo_sampler.h:33-37
        log_jump = with_jump;
        if (log_jump) jump_stats.create(group, "jump_stats", H5T_NATIVE_INT, 4, {2});
    }
    // collective variables (/input/collective_variables present): cv (frame,1,n_cv) f32 and the attribute `names` on it and on /output
    EArray cv; bool log_cv = false;
    void add_cv(const vector<string>& names) {
        cv.create(group, "cv", H5T_NATIVE_FLOAT, 4, {1, (hsize_t)names.size()});
        log_cv = true;
        size_t w = 1; for (auto& n : names) w = max(w, n.size());
        vector<char> buf(names.size() * w, '\0');
        for (size_t i = 0; i < names.size(); ++i) memcpy(&buf[i * w], names[i].data(), names[i].size());
        hid_t st = H5Tcopy(H5T_C_S1); H5Tset_size(st, w);
        hsize_t n = names.size(); hid_t sp = H5Screate_simple(1, &n, nullptr);
        for (hid_t obj : {group, cv.dset}) {
            hid_t at = H5Acreate2(obj, obj == group ? "cv_names" : "names", st, sp, H5P_DEFAULT, H5P_DEFAULT);
            if (at >= 0) { H5Awrite(at, st, buf.data()); H5Aclose(at); }
        }
        H5Sclose(sp); H5Tclose(st);
    }
    // the nodes' own per-frame quantities (default_logger->add_logger in the reference's node constructors)
    vector<EArray> extra; vector<LogValue> extra_spec;
    void add_node_loggers(const vector<LogValue>& specs) {
        for (auto& l : specs) {
            if (H5Lexists(group, l.name.c_str(), H5P_DEFAULT) > 0) continue;      // a second node of the same kind: first one wins
            vector<hsize_t> row(l.dims.begin(), l.dims.end());
            extra.emplace_back();
            if (l.as_long) extra.back().create(group, l.name.c_str(), H5T_NATIVE_LONG, sizeof(long), row);
            else extra.back().create(group, l.name.c_str(), H5T_NATIVE_FLOAT, 4, row);
            extra_spec.push_back(l);
        }
    }
    void sample_node_loggers(int system) {
        vector<float> buf; vector<long> lbuf;
        for (size_t i = 0; i < extra.size(); ++i) {
            size_t n = 1; for (auto d : extra_spec[i].dims) n *= d;
            buf.assign(n, 0.f);
            extra_spec[i].fill(system, buf.data());
            if (extra_spec[i].as_long) { lbuf.assign(buf.begin(), buf.end()); extra[i].push(lbuf.data()); }
            else extra[i].push(buf.data());
        }
    }
    void sample(const float* x, double kin, double pot, double t, double temp, int rep, const int* mc, const int* mcj, const int* cum_swaps) {
        pos.push(x); kinetic.push(&kin); potential.push(&pot); time.push(&t); temperature.push(&temp);
        if (log_replica) { replica_index.push(&rep); if (replica_cumulative_swaps.row_size) replica_cumulative_swaps.push(cum_swaps); }
        if (log_pivot) pivot_stats.push(mc);
        if (log_jump) jump_stats.push(mcj);
        if (!(++n_buffered % 100)) flush();                       // state_logger.h:91-92
    }
    void flush() {
        pos.flush(); kinetic.flush(); potential.flush(); time.flush(); temperature.flush(); if (log_replica) { replica_index.flush(); replica_cumulative_swaps.flush(); }
        if (log_pivot) pivot_stats.flush();
        if (log_jump) jump_stats.flush();
        for (auto& x : extra) x.flush();
        if (log_cv) cv.flush();
        for (auto& x : steer) { x.work.flush(); x.clock.flush(); x.center.flush(); }
        if (file >= 0) H5Fflush(file, H5F_SCOPE_LOCAL);
    }
    // the hills of a cv_metadynamics node at the end of the run: /output/metadynamics/<node>/{hill_center (n, d), hill_weight (n),
    // n_attempt (1)}; copied to /input/metadynamics/<node> of the next configuration they continue the run
    void write_metadynamics(const string& node, int d, const vector<float>& centers, const vector<float>& weights, long n_attempt) {
        if (H5Lexists(group, "metadynamics", H5P_DEFAULT) <= 0) { hid_t g = H5Gcreate2(group, "metadynamics", H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT); if (g < 0) throw string("unable to create /output/metadynamics"); H5Gclose(g); }
        h5u::Handle mg(H5Gopen2(group, "metadynamics", H5P_DEFAULT), H5Gclose);
        h5u::Handle ng(H5Gcreate2(mg, node.c_str(), H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), H5Gclose);
        if (ng < 0) throw string("unable to create /output/metadynamics/") + node;
        EArray c, w, a;
        c.create(ng, "hill_center", H5T_NATIVE_FLOAT, 4, {(hsize_t)d}); w.create(ng, "hill_weight", H5T_NATIVE_FLOAT, 4, {}); a.create(ng, "n_attempt", H5T_NATIVE_LONG, sizeof(long), {});
        for (size_t i = 0; i < weights.size(); ++i) { c.push(&centers[i * d]); w.push(&weights[i]); }
        a.push(&n_attempt);
        c.close(); w.close(); a.close();
    }
    // a cv_steer node, at every frame: /output/cv_steer/<node>/{work (frame), clock (frame), center (frame, n_cv)} of the file's system
    struct SteerLog { EArray work, clock, center; };
    vector<SteerLog> steer;
    void add_steer(const string& node, int n_cv) {
        if (H5Lexists(group, "cv_steer", H5P_DEFAULT) <= 0) { hid_t g = H5Gcreate2(group, "cv_steer", H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT); if (g < 0) throw string("unable to create /output/cv_steer"); H5Gclose(g); }
        h5u::Handle sg(H5Gopen2(group, "cv_steer", H5P_DEFAULT), H5Gclose);
        h5u::Handle ng(H5Gcreate2(sg, node.c_str(), H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT), H5Gclose);
        if (ng < 0) throw string("unable to create /output/cv_steer/") + node;
        steer.emplace_back();
        steer.back().work.create(ng, "work", H5T_NATIVE_DOUBLE, 8, {}); steer.back().clock.create(ng, "clock", H5T_NATIVE_LLONG, sizeof(long long), {});
        steer.back().center.create(ng, "center", H5T_NATIVE_DOUBLE, 8, {(hsize_t)n_cv});
    }
    void close() {
        if (file < 0) return;
        for (auto& x : steer) { x.work.close(); x.clock.close(); x.center.close(); }
        pos.close(); kinetic.close(); potential.close(); time.close(); temperature.close(); replica_index.close(); replica_cumulative_swaps.close(); pivot_stats.close(); jump_stats.close();
        for (auto& x : extra) x.close();
        cv.close();
        H5Gclose(group); H5Fclose(file); file = group = -1;
    }
    ~OutputLogger() { try { close(); } catch (...) {} }
};
}  // namespace

// Orderly termination (main.cpp:24-92): SIGINT / SIGTERM stop the run at the next chunk boundary, the buffered frames
// are written, the caller's handlers come back (RAII, the library may be running inside Python), and with
// --re-raise-signal the signal is raised again for the caller.
namespace {
volatile sig_atomic_t g_received_signal = -1;
void note_signal(int signum) { g_received_signal = signum; }
struct SignalGuard {
    int signum; void (*old_handler)(int);
    explicit SignalGuard(int s) : signum(s), old_handler(signal(s, note_signal)) {
        if (old_handler == SIG_ERR) fprintf(stderr, "Warning: problem installing signal handler. Does not affect correctness of simulation.\n");
    }
    ~SignalGuard() { if (old_handler != SIG_ERR) signal(signum, old_handler); }
};
}  // namespace

static vector<string> split_string(const string& src, const string& sep) {
    vector<string> ret;
    size_t pos = 0;
    while (pos <= src.size()) {
        size_t nxt = src.find(sep, pos);
        if (nxt == string::npos) nxt = src.size();
        ret.emplace_back(src.substr(pos, nxt - pos));
        pos = nxt + sep.size();
        if (nxt == src.size()) break;
    }
    return ret;
}
static void ok(int rc) { if (rc) throw string(upside_hip_last_error()); }      // a C entry point failed: its message goes on

namespace {      // the phases of upside_main_impl and the three structs that carry its state between them
// ---- the command line, and this process's share of it -------------------------------------------------------
struct Options {
    double duration = -1., frame_interval = -1., time_step = 0.009, thermostat_timescale = 5., thermostat_interval = -1., replica_interval = 0., mc_interval = 0.;
    string temperature_str = "1.0", set_param_file, invocation;
    unsigned long seed = 42;
    bool recenter = true, write_output = true, xy_recenter_only = false, re_raise_signal = false, deriv_agreement = false;
    int log_level = 1;
    double anneal_factor = 1., anneal_duration = -1.;
    vector<string> swap_sets, files;      // files: every rank's until split_over_ranks, this rank's after it
    // intervals in rounds of 3 steps (main.cpp:399-411,445-447)
    float dt = 0.f; uint64_t n_round = 0; int frame_rounds = 1, thermo_rounds = 1, replica_rounds = 0, mc_rounds = 0; uint32_t base_seed = 0;
    // split_over_ranks: this rank simulates systems [sys_lo, sys_lo + n_system) of the n_total on the command line
    int world = 1, rank = 0, n_total = 0, n_system = 0, sys_lo = 0; bool use_comm = false;
    vector<float> temps_global, temps;      // of every system of the run; of this rank's, at the start
};

static Options parse_options(int argc, const char* const* argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        string a = argv[i];
        auto need = [&](const char* nm) -> string { if (i + 1 >= argc) throw string("missing value for ") + nm; return argv[++i]; };
        if (a == "--duration") o.duration = stod(need("--duration"));
        else if (a == "--frame-interval") o.frame_interval = stod(need("--frame-interval"));
        else if (a == "--time-step") o.time_step = stod(need("--time-step"));
        else if (a == "--temperature") o.temperature_str = need("--temperature");
        else if (a == "--seed") o.seed = stoul(need("--seed"));
        else if (a == "--thermostat-timescale") o.thermostat_timescale = stod(need("--thermostat-timescale"));
        else if (a == "--thermostat-interval") o.thermostat_interval = stod(need("--thermostat-interval"));
        else if (a == "--replica-interval") o.replica_interval = stod(need("--replica-interval"));
        else if (a == "--swap-set") o.swap_sets.push_back(need("--swap-set"));
        else if (a == "--disable-recentering") o.recenter = false;
        else if (a == "--no-output") o.write_output = false;       // extension: leave the configuration files untouched
        else if (a == "--disable-z-recentering") o.xy_recenter_only = true;   // main.cpp:358-360, 416
        else if (a == "--re-raise-signal") o.re_raise_signal = true;
        else if (a == "--monte-carlo-interval") o.mc_interval = stod(need("--monte-carlo-interval"));
        else if (a == "--log-level") {   // main.cpp:474-479: "" = detailed
            const string v = need("--log-level");
            if (v == "basic") o.log_level = 0; else if (v == "detailed" || v == "") o.log_level = 1; else if (v == "extensive") o.log_level = 2;
            else throw string("Illegal value for --log-level");
        }
        else if (a == "--anneal-factor") o.anneal_factor = stod(need("--anneal-factor"));
        else if (a == "--anneal-duration") o.anneal_duration = stod(need("--anneal-duration"));
        else if (a == "--set-param") o.set_param_file = need("--set-param");
        else if (a == "--potential-deriv-agreement") o.deriv_agreement = true;      // main.cpp:368-372
        else if (a.size() && a[0] == '-') throw string("unsupported flag ") + a;
        else o.files.push_back(a);
    }
    if (o.duration < 0.) throw string("--duration is required");
    if (o.frame_interval < 0.) throw string("--frame-interval is required");
    if (o.files.empty()) throw string("no configuration given");
    for (int i = 0; i < argc; ++i) { if (i) o.invocation += " "; o.invocation += argv[i]; }
    if (o.anneal_duration == -1.) o.anneal_duration = o.duration;      // main.cpp:434
    const float dt = o.dt = (float)o.time_step;
    o.n_round = (uint64_t)round(o.duration / (3 * dt));
    o.frame_rounds = (int)max(1., round(o.frame_interval / (3 * dt)));                                   // main.cpp:400
    o.thermo_rounds = o.thermostat_interval <= 0. ? 1 : (int)max(1., round(o.thermostat_interval / (3 * dt)));   // main.cpp:399
    o.replica_rounds = o.replica_interval > 0. ? max(1, (int)(o.replica_interval / (3 * dt))) : 0;
    o.mc_rounds = o.mc_interval > 0. ? max(1, (int)(o.mc_interval / (3 * dt))) : 0;   // main.cpp:411
    o.base_seed = (uint32_t)(o.seed % 4294967291ul);   // main.cpp:403-404
    return o;
}

// One process per GPU (started by any launcher that sets RANK / WORLD_SIZE / LOCAL_RANK, e.g. torch.distributed.run, or
// UPSIDE_HIP_RANK / _WORLD / _LOCAL_RANK): every rank receives the SAME command line; rank r simulates a contiguous
// block of the configuration files on device LOCAL_RANK and replica exchange runs over RCCL inside the library
// (upside_hip_comm_*, comm_rccl.cpp).  UPSIDE_HIP_COMM=1 takes the same path with a single process (tests).
static void split_over_ranks(Options& o) {
    auto env_int_of = [](const char* a, const char* b, int dflt) {
        return env_int(a, env_int(b, dflt)); };
    o.world = max(1, env_int_of("UPSIDE_HIP_WORLD", "WORLD_SIZE", 1));
    o.rank = env_int_of("UPSIDE_HIP_RANK", "RANK", 0);
    const int local_rank = env_int_of("UPSIDE_HIP_LOCAL_RANK", "LOCAL_RANK", 0);
    o.use_comm = o.world > 1 || env_int("UPSIDE_HIP_COMM", 0);
    if (o.rank < 0 || o.rank >= o.world) throw string("invalid rank");
    o.n_total = (int)o.files.size();
    if (o.n_total % o.world) throw to_string(o.n_total) + " systems do not divide over " + to_string(o.world) + " processes";
    o.n_system = o.n_total / o.world; o.sys_lo = o.rank * o.n_system;
    o.files = vector<string>(o.files.begin() + o.sys_lo, o.files.begin() + o.sys_lo + o.n_system);
    if (o.world > 1) ok(upside_hip_set_device(local_rank));
    for (auto& t : split_string(o.temperature_str, ",")) o.temps_global.push_back((float)stod(t));
    if (o.temps_global.size() != 1u && (int)o.temps_global.size() != o.n_total)
        throw string("Received ") + to_string(o.temps_global.size()) + " temperatures but have " + to_string(o.n_total) + " systems";
    if (o.temps_global.size() == 1u) o.temps_global.assign(o.n_total, o.temps_global[0]);
    o.temps.assign(o.temps_global.begin() + o.sys_lo, o.temps_global.begin() + o.sys_lo + o.n_system);
    if (o.use_comm && o.anneal_factor != 1.) throw string("--anneal-factor is not available together with replica exchange across processes");
}

// ---- the engines of the run ------------------------------------------------------------------------------------
// One engine per group of files (the reference builds one engine per file, main.cpp:450-571, which is what Hamiltonian
// replica exchange and mixed runs use): files whose /input/potential agree in everything but the values of the per-system
// table (upside_hip_group_configurations; a Hamiltonian ladder) share one batched engine, every other difference -- node
// set, arguments, index datasets, shapes, other values -- makes another group.  UPSIDE_HIP_HAMILTONIAN_BATCH=0: one group
// per distinct /input/potential (node names, arguments, attributes and dataset bytes alike).  The common case is one group.
// The struct alone knows how a system of the run (its index among this rank's files) maps to (engine, index in the engine):
// what it offers takes and returns per-system arrays in the order of the files, whatever the number of engines.
struct Fleet {
    vector<DerivEngine*> engines;       // by group; owned
    vector<vector<int>> members;        // the systems of every group, in the engine's order
    vector<int> group_of, local_of;     // of every system
    vector<char> ladder;                // the group's files differ in the values of the per-system table: one engine of several Hamiltonians
    int n_atom = 0;
    unsigned long long potential_digest = 0;      // of the first file's /input/potential (0 in a single-file run)
    vector<float> input_pos;            // /input/pos of every system
    Fleet() = default;
    Fleet(Fleet&&) = default;
    ~Fleet() { for (auto* x : engines) delete x; }
    int n_group() const { return (int)members.size(); }
    void compute(float* energy) {      // force pass of every system, potentials by system
        for (auto* x : engines) x->compute(PotentialAndDerivMode);          // enqueued on the engines' own streams, then collected
        for (int g = 0; g < n_group(); ++g) {
            // (no later swap set reuses energies from before this pass: require_attempt would refuse it anyway, by its count of passes)
            engines[g]->check_device_errors(); engines[g]->fetch_potentials(); engines[g]->invalidate_attempt();
            from_group(g, engines[g]->potential, energy, 1);
        }
    }
    void get_pos_mom(float* pos, float* mom) {
        const size_t n3 = (size_t)n_atom * 3;
        for (int g = 0; g < n_group(); ++g) {
            vector<float> gp(members[g].size() * n3), gm(gp.size());
            ok(upside_hip_get_pos(engines[g], gp.data())); ok(upside_hip_get_mom(engines[g], gm.data()));
            from_group(g, gp, pos, n3); from_group(g, gm, mom, n3);
        }
    }
    void set_pos(const float* pos) { for (int g = 0; g < n_group(); ++g) ok(upside_hip_set_pos(engines[g], to_group(g, pos, (size_t)n_atom * 3).data())); }
    // (thermostat streams are keyed by the GLOBAL system index, main.cpp:459: system ns draws from first_seed + ns)
    void init_md(const float* temps, uint32_t first_seed, float thermostat_timescale, float dt, int thermo_rounds) {
        for (int g = 0; g < n_group(); ++g) {
            vector<uint32_t> seeds; for (int ns : members[g]) seeds.push_back(first_seed + (uint32_t)ns);
            ok(upside_hip_init_md_seeds(engines[g], to_group(g, temps, 1).data(), seeds.data(), thermostat_timescale, dt, thermo_rounds));
        }
    }
    void set_temperature(const float* temps) { for (int g = 0; g < n_group(); ++g) ok(upside_hip_set_temperature(engines[g], to_group(g, temps, 1).data())); }
    void run_rounds(int n) {      // the engines run side by side on their own streams
        for (auto* x : engines) x->run_steps(3 * n);                   // main.cpp:657-663
        for (auto* x : engines) x->check_device_errors();
    }
    void recenter(bool xy_only) { for (auto* x : engines) ok(upside_hip_recenter_axes(x, xy_only)); }
    void sync() { for (auto* x : engines) x->sync(); }
private:      // per-system arrays (n floats each) <-> an engine's own order
    vector<float> to_group(int g, const float* all, size_t n) const { vector<float> v; v.reserve(members[g].size() * n); for (int ns : members[g]) v.insert(v.end(), all + (size_t)ns * n, all + (size_t)(ns + 1) * n); return v; }
    void from_group(int g, const vector<float>& v, float* all, size_t n) const { for (size_t l = 0; l < members[g].size(); ++l) memcpy(all + (size_t)members[g][l] * n, v.data() + l * n, n * sizeof(float)); }
};

// Monte-Carlo moves in a Hamiltonian ladder: one sampler for the whole engine, so its tables must be those of every file
static void require_same_moves(const vector<string>& files) {
    for (const char* grp : {"/input/pivot_moves", "/input/jump_moves"}) {
        unsigned long long d0 = 0ull;
        for (size_t ns = 0; ns < files.size(); ++ns) {
            auto f = h5u::open_config(files[ns]);
            const unsigned long long d = h5u::exists(f, grp) ? h5u::group_digest(h5u::open_group(f, grp)) : 1ull;
            if (ns == 0) d0 = d;
            else if (d != d0) throw string("Monte-Carlo moves need the same ") + grp + " in every file of a run: " + files[ns] + " differs from " + files[0];
        }
    }
}
// --set-param (main.cpp:384-395, 498-499): one 1-D float dataset per node name
static void apply_set_param(const string& path, Fleet& fleet) {
    auto pf = h5u::open_config(path);
    for (const string& node_name : h5u::node_names_in_group(pf)) {
        auto values = h5u::read<float>(pf, node_name, 1);
        bool applied = false;      // (a mixed run: every engine that has a node of this name)
        for (auto* x : fleet.engines) {
            if (fleet.n_group() > 1 && x->get_idx(node_name, false) < 0) continue;
            if (set_param((int)values.size(), values.data(), x, node_name.c_str())) throw string("--set-param: ") + upside_hip_last_error();
            applied = true;
        }
        if (!applied) throw string("--set-param: no node named ") + node_name;
    }
}
// groups this rank's files, reads their positions, refuses what a run cannot mix, and constructs the engines
static Fleet load_fleet(const Options& o, int verbose) {
    const vector<string>& files = o.files;
    Fleet fl;
    fl.group_of.resize(o.n_system); fl.local_of.resize(o.n_system);
    vector<unsigned long long> full_digest(o.n_system, 0ull);
    {
        vector<const char*> fp; for (auto& f : files) fp.push_back(f.c_str());
        if (o.n_total > 1 && upside_hip_group_configurations(o.n_system, fp.data(), fl.group_of.data()) < 0) throw string(upside_hip_last_error());
        if (o.n_total == 1) fl.group_of[0] = 0;
    }
    for (int ns = 0; ns < o.n_system; ++ns) {
        auto f = h5u::open_config(files[ns]);
        vector<hsize_t> dims;
        auto p = h5u::read<float>(f, "/input/pos", 3, &dims);
        if (dims[1] != 3 || dims[2] != 1) throw string("invalid dimensions for initial position");
        // (hashed only when there is something to compare with: a single-file run loads whatever the node loader accepts)
        full_digest[ns] = (o.n_total > 1) ? h5u::group_digest(h5u::open_group(f, "/input/potential")) : 0ull;
        if (ns == 0) { fl.n_atom = (int)dims[0]; fl.potential_digest = full_digest[0]; }
        else if ((int)dims[0] != fl.n_atom)      // (replica exchange trades coordinates between any two systems of the run)
            throw string("the systems of one run must have the same number of atoms: ") + files[ns] + " differs from " + files[0];
        const size_t g = (size_t)fl.group_of[ns];
        if (g >= fl.members.size()) fl.members.resize(g + 1);
        fl.local_of[ns] = (int)fl.members[g].size(); fl.members[g].push_back(ns);
        fl.input_pos.insert(fl.input_pos.end(), p.begin(), p.end());
    }
    const auto& members = fl.members;
    fl.ladder.assign(fl.n_group(), 0);
    for (int g = 0; g < fl.n_group(); ++g) for (int ns : members[g]) if (full_digest[ns] != full_digest[members[g][0]]) fl.ladder[g] = 1;
    // (past a refusal of several groups there is one group, and ladder[0] says whether that one is a Hamiltonian ladder)
    if (fl.n_group() > 1 && o.use_comm)
        throw string("systems must share one potential when the run is spread over several processes: /input/potential of ") + files[members[1][0]] +
              " differs from that of " + files[0];
    if (fl.ladder[0] && o.use_comm)      // (each rank's engine would be a ladder of its own: exchange across ranks assumes one Hamiltonian)
        throw string("Hamiltonian replica exchange across processes is not available: the /input/potential values of ") + files[members[0][1]] +
              " differ from those of " + files[0] + "; run the ladder in one process";
    if (fl.n_group() > 1 && o.mc_interval > 0.) throw string("Monte-Carlo moves are not available in a run that mixes potentials");
    if (fl.ladder[0] && o.mc_interval > 0.) require_same_moves(files);
    for (int g = 0; g < fl.n_group(); ++g) {
        if (fl.ladder[g]) {
            vector<const char*> fp; for (int ns : members[g]) fp.push_back(files[ns].c_str());
            fl.engines.push_back(upside_hip_construct_files(fl.n_atom, (int)fp.size(), fp.data(), !verbose));
        } else fl.engines.push_back(upside_hip_construct(fl.n_atom, files[members[g][0]].c_str(), (int)members[g].size(), !verbose));
        if (!fl.engines[g]) throw string("unable to construct the engine: ") + upside_hip_last_error();
    }
    if (!o.set_param_file.empty()) apply_set_param(o.set_param_file, fl);
    return fl;
}

// cv_metadynamics: a run continues from the hills under /input/metadynamics/<node> (a system's own file; a shared list: the
// engine's first file), read before the first force pass so that frame 0 sees them
static void read_hills(const Options& o, Fleet& fleet) {
    for (int g = 0; g < fleet.n_group(); ++g) for (const string& node : engine_metad_nodes(*fleet.engines[g])) {
        int d = 0, cap = 0, n_list = 0;
        engine_metad_info(*fleet.engines[g], node, &d, &cap, &n_list);
        for (int l = 0; l < n_list; ++l) {
            const string& path = o.files[fleet.members[g][n_list == 1 ? 0 : l]];
            auto f = h5u::open_config(path);
            const string grp = "/input/metadynamics/" + node;
            if (!h5u::exists(f, "/input/metadynamics") || !h5u::exists(f, grp)) continue;
            vector<hsize_t> dc;
            const auto centers = h5u::read<float>(f, grp + "/hill_center", 2, &dc); const auto weights = h5u::read<float>(f, grp + "/hill_weight", 1);
            if (dc[0] != weights.size() || (dc[0] && (int)dc[1] != d))
                throw path + ": " + grp + ": hill_center must be (n_hill, " + to_string(d) + ") and hill_weight (n_hill)";
            try { engine_metad_write(*fleet.engines[g], node, l, centers.data(), weights.data(), (int)weights.size()); }
            catch (const string& err) { throw path + ": " + grp + ": " + err; }
        }
    }
}
// ... and leaves the hills of the end of the run under /output/metadynamics/<node> of every system's file
static void write_hills(Fleet& fleet, vector<OutputLogger>& loggers) {
    for (size_t ns = 0; ns < loggers.size(); ++ns) {
        DerivEngine& e = *fleet.engines[fleet.group_of[ns]];
        for (const string& node : engine_metad_nodes(e)) {
            int d = 0, cap = 0, n_list = 0, n_hill = 0; long long n_att = 0;
            engine_metad_info(e, node, &d, &cap, &n_list);
            vector<float> centers((size_t)cap * d), weights((size_t)cap);
            engine_metad_read(e, node, n_list == 1 ? 0 : fleet.local_of[ns], centers.data(), weights.data(), &n_hill, &n_att);
            centers.resize((size_t)n_hill * d); weights.resize((size_t)n_hill);
            loggers[ns].write_metadynamics(node, d, centers, weights, (long)n_att);
        }
    }
}

// main.cpp:548-564: recentring would fight a potential that is not translation invariant
static void refuse_recentering_conflicts(const Options& o, const Fleet& fleet) {
    for (auto* x : fleet.engines) for (auto& n : x->nodes) {
        auto pre = [&](const char* p) { return n.name == string(p).substr(0, n.name.size()); };   // is_prefix(n.name, p), deriv_engine.cpp:72-74
        if (o.recenter && !o.xy_recenter_only && (pre("membrane_potential") || pre("z_flat_bottom") || pre("tension") || pre("AFM")))
            throw string("You have z-centering and a z-dependent potential turned on.  This is not what you want.  "
                         "Consider --disable-z-recentering or --disable-recentering.");
        if (o.recenter && pre("cavity_radial"))
            throw string("You have re-centering and a radial potential turned on.  This is not what you want.  Consider --disable-recentering.");
    }
}

// swap sets (main.cpp:146-219): pairs of GLOBAL system indices
static vector<vector<int>> parse_swap_sets(const Options& o) {
    vector<vector<int>> sets;
    for (auto& s : o.swap_sets) {
        vector<int> prs; set<int> used;
        for (auto& ps : split_string(s, ",")) {
            auto p = split_string(ps, "-");
            if (p.size() != 2u) throw string("invalid swap pair");
            int a = stoi(p[0]), b = stoi(p[1]);
            if (a >= o.n_total || b >= o.n_total || a < 0 || b < 0) throw string("invalid system");
            if (used.count(a) || used.count(b) || a == b) throw string("Overlapping indices in swap set.");
            used.insert(a); used.insert(b); prs.push_back(a); prs.push_back(b);
        }
        sets.push_back(prs);
    }
    if (!o.use_comm)      // (inside one process the swap sets address its own systems)
        for (auto& st : sets) for (int x : st) if (x >= o.n_system) throw string("invalid system");
    return sets;
}

// Rendezvous of the ranks of one launch: rank 0 creates the communicator id and leaves it in a file every rank of the job can see,
// stamped with a nonce of THIS launch -- what every rank of one launch shares and another launch does not: the launcher's address and
// port, its process id, torchrun's run id and restart count (or UPSIDE_HIP_COMM_NONCE).  A rank that finds a record
// with another nonce (an earlier crashed attempt under the same file name) keeps waiting for this launch's.  Rank 0
// publishes with an exclusive create + rename and removes the file once every rank has joined.  `e` is the rank's only engine
// (load_fleet refuses several together with a communicator); process_start: when this run began.
static void comm_rendezvous(const Options& o, DerivEngine* e, unsigned long long potential_digest, time_t process_start) {
    string launch;
    bool job_wide = false;      // the nonce is made of variables every rank of the job shares, on whatever node it runs
    if (const char* x = env_str("UPSIDE_HIP_COMM_NONCE")) { launch = x; job_wide = true; }
    else {
        for (const char* v : {"MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "TORCHELASTIC_RESTART_COUNT"}) {
            if (env_set(v)) job_wide = true;
            launch += string(env_set(v) ? env_str(v) : "") + "|";
        }
        launch += to_string(o.world) + "|";
        // the launcher's pid is the same for the ranks of ONE node only: it stands in for the job-wide variables where a launcher
        // exports none (plain RANK / WORLD_SIZE from a shell), never beside them (a multi-node job shares the file, not the agent)
        if (!job_wide) launch += to_string((long)getppid());
    }
    unsigned long long nonce = 1469598103934665603ull;               // FNV-1a
    for (unsigned char ch : launch) { nonce ^= ch; nonce *= 1099511628211ull; }
    string path;
    if (const char* f = env_str("UPSIDE_HIP_COMM_FILE")) path = f;
    else {
        path = string("/tmp/upside_hip_comm_") + (env_set("MASTER_PORT") ? env_str("MASTER_PORT") : "0") + "_" + to_string((long)getppid());
        for (const char* v : {"TORCHELASTIC_RUN_ID", "TORCHELASTIC_RESTART_COUNT"}) if (const char* x = env_str(v)) path += string("_") + x;
    }
    // Two attempts started one after the other from the same shell share nonce and file name: the record also carries the wall-clock
    // second it was written, and a rank takes only records written after (its own start - UPSIDE_HIP_COMM_SKEW_S: how far apart the
    // ranks of one launch may start) -- what a crashed earlier attempt left behind is older than that.  The skew defaults to the wait
    // window, UPSIDE_HIP_COMM_WAIT_S (120 s): a rank that starts late -- a staggered multi-node launch -- or whose node clock lags
    // still accepts rank 0's record for as long as rank 0 waits for it.
    struct Record { char id[UPSIDE_HIP_COMM_ID_BYTES]; unsigned long long nonce; long long stamp; } rec;
    memset(&rec, 0, sizeof(rec));
    const int wait_s = env_set("UPSIDE_HIP_COMM_WAIT_S") ? max(1, env_int("UPSIDE_HIP_COMM_WAIT_S", 0)) : 120;
    const long long skew_s = env_set("UPSIDE_HIP_COMM_SKEW_S") ? max(0, env_int("UPSIDE_HIP_COMM_SKEW_S", 0)) : wait_s;
    if (o.rank == 0) {
        remove(path.c_str());                                   // a stale record of an earlier attempt under this name
        ok(upside_hip_comm_get_unique_id(rec.id));
        rec.nonce = nonce; rec.stamp = (long long)time(nullptr);
        const string tmp = path + ".tmp." + to_string((long)getpid());
        const int fd = open(tmp.c_str(), O_CREAT | O_EXCL | O_WRONLY, 0600);
        if (fd < 0 || write(fd, &rec, sizeof(rec)) != (ssize_t)sizeof(rec)) { if (fd >= 0) close(fd); throw string("cannot write ") + tmp; }
        close(fd);
        if (rename(tmp.c_str(), path.c_str())) { remove(tmp.c_str()); throw string("cannot publish ") + path; }
    } else {
        bool got = false;
        for (int tries = 0; tries < wait_s * 10 && !got; ++tries) {
            FILE* f = fopen(path.c_str(), "rb");
            if (f) { got = fread(&rec, 1, sizeof(rec), f) == sizeof(rec); fclose(f); }
            if (got && rec.nonce != nonce) got = false;           // another launch's record
            if (got && rec.stamp < (long long)process_start - skew_s) got = false;      // an earlier attempt of the same launch line
            if (!got) this_thread::sleep_for(chrono::milliseconds(100));
        }
        if (!got) throw string("no communicator id of this launch at ") + path + " (is rank 0 running?  a multi-node job needs UPSIDE_HIP_COMM_FILE on a "
                               "shared file system and either a launcher that exports MASTER_ADDR / MASTER_PORT or UPSIDE_HIP_COMM_NONCE; a record older than this "
                               "rank's start by more than UPSIDE_HIP_COMM_SKEW_S = " + to_string(skew_s) + " s -- late start or clock skew between nodes -- is ignored; "
                               "waited UPSIDE_HIP_COMM_WAIT_S = " + to_string(wait_s) + " s)";
    }
    ok(upside_hip_comm_init(e, o.rank, o.world, rec.id, o.temps_global.data()));
    if (o.rank == 0) remove(path.c_str());                         // (ncclCommInitRank returns when every rank has joined)
    // every rank keeps its own files under ONE engine and the Metropolis kernel assumes one Hamiltonian for the whole ladder:
    // the ranks' potentials must agree as the files of one rank must.  Checked with the communicator, so that every rank
    // learns of a mismatch and none is left waiting for a peer that has gone.  (A run over several processes holds no Hamiltonian
    // ladder, refused in load_fleet, so the digest that groups its files is that of the whole /input/potential.)
    int differs = -1;
    ok(upside_hip_comm_agree(e, potential_digest, &differs));
    if (differs >= 0) {
        upside_hip_comm_free(e);
        // (which of the two has the wrong files the digests cannot tell: with more than two ranks the odd one out is usually it)
        throw string("the configuration files of ranks 0 and ") + to_string(differs) + " hold different /input/potential groups";
    }
}

// --potential-deriv-agreement (developer check, main.cpp:279-315 with deriv_engine.cpp:291-342): central differences of the total
// potential, eps = 1e-3 per coordinate, against the derivative the backward sweep produced; relative RMS deviation per system
// (relative_rms_deviation, deriv_engine.h:345-357: the finite differences are the reference).  All systems of an engine are displaced
// in the same coordinate at once: 2 x 3 n_atom force passes per engine whatever the number of systems.  Works engine by engine, in each
// engine's own order, on the positions the engines hold (the input); prints in the order of the engines.
static void potential_deriv_agreement(const Options& o, Fleet& fleet, int verbose) {
    const float eps = 1e-3f;
    const size_t n3 = (size_t)fleet.n_atom * 3;
    for (int g = 0; g < fleet.n_group(); ++g) {
        DerivEngine* eg = fleet.engines[g];
        const int S = (int)fleet.members[g].size();
        vector<float> pos0((size_t)S * n3), work, en((size_t)S), deriv((size_t)S * n3), ep((size_t)S), em((size_t)S);
        ok(upside_hip_get_pos(eg, pos0.data()));
        ok(upside_hip_compute(eg, en.data(), deriv.data()));
        if (verbose) {
            printf("Initial potential:\n");
            eg->fetch_potentials();
            for (int l = 0; l < S; ++l) {
                if (S > 1) printf("%s\n", o.files[fleet.members[g][l]].c_str());
                for (auto& nd : eg->nodes)
                    if (nd.computation->potential_term) printf("%s: % 4.3f\n", nd.name.c_str(), static_cast<PotentialNode*>(nd.computation.get())->potential[l]);
                printf("\n\n");
            }
        }
        vector<double> diff2((size_t)S, 0.), ref2((size_t)S, 0.);
        for (size_t ni = 0; ni < n3; ++ni) {
            for (int sign = -1; sign <= 1; sign += 2) {
                work = pos0;
                for (int l = 0; l < S; ++l) work[(size_t)l * n3 + ni] = pos0[(size_t)l * n3 + ni] + sign * eps;
                ok(upside_hip_set_pos(eg, work.data())); ok(upside_hip_compute(eg, sign < 0 ? em.data() : ep.data(), nullptr));
            }
            for (int l = 0; l < S; ++l) {
                const float fd = (ep[l] - em[l]) * (0.5f / eps);
                const double d = (double)fd - (double)deriv[(size_t)l * n3 + ni];
                diff2[l] += d * d; ref2[l] += (double)fd * (double)fd;
            }
        }
        ok(upside_hip_set_pos(eg, pos0.data()));      // (restore the input: the caller is not surprised)
        for (int l = 0; l < S; ++l) {
            if (verbose) printf("overall potential relative error: ");
            printf(" %.5f", sqrt(diff2[l] / ref2[l]));
            if (verbose) printf("\n");
        }
    }
}

// ---- what the loop carries from round to round -----------------------------------------------------------------------
struct PairRef { int set, pair; };
struct Run {
    vector<vector<int>> sets;                // swap sets, global indices
    vector<float> temps, energy;             // of this rank's systems, now
    vector<OutputLogger> loggers;            // one per configuration file
    bool have_mc = false, have_pivot = false, have_jump = false, any_node_logger = false;
    vector<int> n_cv_of;                     // collective variables, per engine
    vector<vector<string>> steer_nodes;      // cv_steer nodes, per engine
    // the swap pairs every system takes part in (set order, then pair order: main.cpp:176-192) and their running counts
    vector<vector<PairRef>> participating; vector<vector<int>> pair_success, pair_attempt;
    vector<long> n_attempt, n_success;       // per set
    vector<int> replica_index;               // by GLOBAL slot; every rank keeps the whole table (the verdicts are identical everywhere)
    vector<float> frame_pos, frame_mom; vector<vector<float>> frame_cv; vector<int> mc_stats, mcj_stats;      // the frame's buffers
};

// samplers, collective variables, one logger per configuration file (the engines have closed their read-only handles by now)
static void open_loggers(const Options& o, Fleet& fleet, Run& run) {
    const int n_system = o.n_system, n_group = fleet.n_group();
    DerivEngine* e = fleet.engines[0];      // (Monte-Carlo moves: the only engine, load_fleet refuses them with several)
    run.loggers = vector<OutputLogger>(n_system);
    if (o.mc_rounds) {
        const int n_sampler = upside_hip_load_mc(e, o.files[0].c_str());
        if (n_sampler < 0) throw string(upside_hip_last_error());
        run.have_mc = n_sampler > 0;
    }
    // collective variables: each engine takes the definition of its first file; its systems' files get /output/cv, sampled at the frames
    // (read before the loggers open the files for writing)
    run.n_cv_of.assign(n_group, 0);
    for (int g = 0; g < n_group; ++g) {
        run.n_cv_of[g] = upside_hip_cv_load(fleet.engines[g], o.files[fleet.members[g][0]].c_str());
        if (run.n_cv_of[g] < 0) throw string(upside_hip_last_error());
    }
    run.have_pivot = run.have_mc && upside_hip_mc_loaded(e, 0); run.have_jump = run.have_mc && upside_hip_mc_loaded(e, 1);
    run.mc_stats.assign((size_t)n_system * 2, 0); run.mcj_stats.assign((size_t)n_system * 2, 0);
    const auto& sets = run.sets;
    run.participating.resize(o.n_total); run.pair_success.resize(sets.size()); run.pair_attempt.resize(sets.size());
    for (size_t k = 0; k < sets.size(); ++k) {
        run.pair_success[k].assign(sets[k].size() / 2, 0); run.pair_attempt[k].assign(sets[k].size() / 2, 0);
        for (size_t i = 0; i < sets[k].size() / 2; ++i) for (int side = 0; side < 2; ++side) run.participating[sets[k][2 * i + side]].push_back(PairRef{(int)k, (int)i});
    }
    run.steer_nodes.resize(n_group);      // cv_steer: work, clock and centres of the file's system at every frame
    for (int g = 0; g < n_group; ++g) run.steer_nodes[g] = engine_steer_nodes(*fleet.engines[g]);
    run.frame_cv.resize(n_group);
    run.replica_index.resize(o.n_total);
    for (int ns = 0; ns < o.n_total; ++ns) run.replica_index[ns] = ns;
    run.frame_pos.resize((size_t)n_system * fleet.n_atom * 3); run.frame_mom.resize(run.frame_pos.size());
    run.n_attempt.assign(sets.size(), 0); run.n_success.assign(sets.size(), 0);
    if (!o.write_output) return;
    for (int ns = 0; ns < n_system; ++ns) {
        vector<int> partners;
        for (auto& pr : run.participating[o.sys_lo + ns]) { const int a = sets[pr.set][2 * pr.pair], b = sets[pr.set][2 * pr.pair + 1]; partners.push_back(a != o.sys_lo + ns ? a : b); }
        run.loggers[ns].open(o.files[ns], fleet.n_atom, o.invocation, !sets.empty(), run.have_pivot, run.have_jump, partners);
    }
    vector<vector<LogValue>> node_loggers(n_group);      // per engine, in node order, filtered by --log-level (state_logger.h:17-27)
    for (int g = 0; g < n_group; ++g)
        for (auto& n : fleet.engines[g]->nodes) {
            vector<LogValue> v; n.computation->add_loggers(v);
            for (auto& l : v) if (l.level <= o.log_level) { node_loggers[g].push_back(l); run.any_node_logger = true; }
        }
    for (int ns = 0; ns < n_system; ++ns) {
        const int g = fleet.group_of[ns];
        run.loggers[ns].add_node_loggers(node_loggers[g]);
        if (run.n_cv_of[g]) run.loggers[ns].add_cv(fleet.engines[g]->cv.names);
        for (const string& node : run.steer_nodes[g]) run.loggers[ns].add_steer(node, engine_steer_n_cv(*fleet.engines[g], node));
    }
}

// A frame (main.cpp:633-654): recenter, energy, log, print -- before the round is integrated
static void log_frame(const Options& o, Fleet& fleet, Run& run, uint64_t rnd, int verbose) {
    const int n_system = o.n_system, n_atom = fleet.n_atom;
    DerivEngine* e = fleet.engines[0];      // (Monte-Carlo statistics: the only engine)
    auto& loggers = run.loggers;
    if (o.recenter) fleet.recenter(o.xy_recenter_only);
    fleet.compute(run.energy.data());
    fleet.get_pos_mom(run.frame_pos.data(), run.frame_mom.data());
    for (int g = 0; g < fleet.n_group(); ++g) if (run.n_cv_of[g]) {
        run.frame_cv[g].resize(fleet.members[g].size() * (size_t)run.n_cv_of[g]);
        ok(upside_hip_cv_compute(fleet.engines[g], run.frame_cv[g].data()));
    }
    if (o.write_output) for (int g = 0; g < fleet.n_group(); ++g) for (size_t k = 0; k < run.steer_nodes[g].size(); ++k) {
        const auto& members = fleet.members[g];
        const int n_cv = engine_steer_n_cv(*fleet.engines[g], run.steer_nodes[g][k]);
        vector<long long> clk(members.size()); vector<double> wrk(members.size()), cen(members.size() * (size_t)n_cv);
        engine_steer_read(*fleet.engines[g], run.steer_nodes[g][k], clk.data(), wrk.data(), cen.data());
        for (size_t l = 0; l < members.size(); ++l) {
            auto& lg = loggers[members[l]].steer[k];
            lg.work.push(&wrk[l]); lg.clock.push(&clk[l]); lg.center.push(&cen[l * n_cv]);
        }
    }
    if (run.have_pivot) ok(upside_hip_mc_stats(e, 0, run.mc_stats.data(), 1));   // reset per frame
    if (run.have_jump) ok(upside_hip_mc_stats(e, 1, run.mcj_stats.data(), 1));
    if (o.write_output && run.any_node_logger) {
        for (auto* x : fleet.engines) for (auto& n : x->nodes) n.computation->begin_log_frame();
        for (int ns = 0; ns < n_system; ++ns) loggers[ns].sample_node_loggers(fleet.local_of[ns]);
        for (auto* x : fleet.engines) for (auto& n : x->nodes) n.computation->end_log_frame();
    }
    for (int ns = 0; ns < n_system; ++ns) {
        const int g = fleet.group_of[ns], local = fleet.local_of[ns];
        const float* x = &run.frame_pos[(size_t)ns * n_atom * 3]; const float* m = &run.frame_mom[(size_t)ns * n_atom * 3];
        double sum_kin = 0.;
        for (int i = 0; i < n_atom * 3; ++i) sum_kin += (double)(m[i] * m[i]);
        vector<int> cum;
        for (auto& pr : run.participating[o.sys_lo + ns]) { cum.push_back(run.pair_success[pr.set][pr.pair]); cum.push_back(run.pair_attempt[pr.set][pr.pair]); }
        if (o.write_output && loggers[ns].log_cv) loggers[ns].cv.push(&run.frame_cv[g][(size_t)local * run.n_cv_of[g]]);
        if (o.write_output) loggers[ns].sample(x, (0.5 / n_atom) * sum_kin, (double)run.energy[ns], (double)(3 * o.dt * (float)rnd) /* fp32 product as main.cpp:540 */, (double)run.temps[ns],
                                               run.replica_index[o.sys_lo + ns], &run.mc_stats[(size_t)ns * 2], &run.mcj_stats[(size_t)ns * 2], cum.data());
        double com[3] = {0, 0, 0}, rg = 0.;
        for (int i = 0; i < n_atom; ++i) for (int d = 0; d < 3; ++d) com[d] += x[i * 3 + d];
        for (int d = 0; d < 3; ++d) com[d] /= n_atom;
        for (int i = 0; i < n_atom; ++i) for (int d = 0; d < 3; ++d) rg += (x[i * 3 + d] - com[d]) * (x[i * 3 + d] - com[d]);
        if (verbose) {   // the line of main.cpp:649-654, hydrogen-bond count included (get_n_hbond, main.cpp:28-35)
            double n_hbond = 0.;
            for (auto& n : fleet.engines[g]->nodes) if (dynamic_cast<HBondCounter*>(n.computation.get())) {
                auto v = n.computation->get_param_deriv(local);      // d(potential)/d(E_protein) = the count
                if (!v.empty()) n_hbond += v[0];
            }
            printf("%*.0f / %*.0f elapsed %2i system %.2f temp %5.1f hbonds, Rg %5.1f A, potential % 8.2f\n", 8, rnd * 3 * double(o.dt), 8,
                   o.duration, o.sys_lo + ns, run.temps[ns], n_hbond, sqrt(rg / n_atom), run.energy[ns]);
        }
    }
    fflush(stdout);
}

// simulated annealing (main.cpp:436-442, 658-660): the temperature is reset before every thermostat application
static void anneal_temperatures(const Options& o, Fleet& fleet, Run& run, uint64_t rnd) {
    const double time = 3 * o.dt * (float)(rnd + 1);
    const double fraction = max(0., (time - (o.duration - o.anneal_duration)) / o.anneal_duration);
    for (int ns = 0; ns < o.n_system; ++ns) {
        const double T0 = o.temps[ns], T1 = o.temps[ns] * o.anneal_factor;
        const double r = sqrt(T0) * (1. - fraction) + sqrt(T1) * fraction;
        run.temps[ns] = (float)(r * r);
    }
    fleet.set_temperature(run.temps.data());
}

// One exchange attempt (main.cpp:667-668; one generator per attempt, main.cpp:249): every swap set in turn, by the procedure the run's
// engines call for.  One force evaluation per attempt where one Hamiltonian is shared: the later sets see the energies the accepted pairs traded.
static void exchange_attempt(const Options& o, Fleet& fleet, Run& run, uint64_t rnd) {
    DerivEngine* e = fleet.engines[0];      // (every procedure but the first: the only engine)
    const auto& sets = run.sets;
    int draw = 0;
    for (size_t k = 0; k < sets.size(); ++k) {
        const int np = (int)sets[k].size() / 2;
        vector<int> acc(np + 1);
        if (fleet.n_group() > 1) {     // several Hamiltonians: the reference's own procedure (main.cpp:251-273), two energy passes per set
            auto log_boltzmann = [&]() { vector<float> en(o.n_system), lb(o.n_system); fleet.compute(en.data()); for (int i = 0; i < o.n_system; ++i) lb[i] = -(1.f / run.temps[i]) * en[i]; return lb; };
            auto coord_swap = [&](int s1, int s2) {
                ok(upside_hip_swap_between(fleet.engines[fleet.group_of[s1]], fleet.local_of[s1], fleet.engines[fleet.group_of[s2]], fleet.local_of[s2])); };
            const auto old_lb = log_boltzmann();
            for (int i = 0; i < np; ++i) coord_swap(sets[k][2 * i], sets[k][2 * i + 1]);
            const auto new_lb = log_boltzmann();
            vector<float> diff(np);
            for (int i = 0; i < np; ++i) { const int s1 = sets[k][2 * i], s2 = sets[k][2 * i + 1]; diff[i] = (new_lb[s1] + new_lb[s2]) - (old_lb[s1] + old_lb[s2]); }
            ok(upside_replica_decide_lboltz(np, diff.data(), o.base_seed, rnd, draw, acc.data()));
            draw = acc.back();
            for (int i = 0; i < np; ++i) if (!acc[i]) coord_swap(sets[k][2 * i], sets[k][2 * i + 1]);      // a rejected swap is reversed
        } else if (fleet.ladder[0]) {     // one engine, several Hamiltonians: the same procedure on the device (upside_hip_hamiltonian_swap)
            ok(upside_hip_hamiltonian_swap(e, np, sets[k].data(), o.base_seed, rnd, draw, acc.data()));
            draw = acc.back();
        } else if (o.use_comm) {     // global indices; energies all-gathered, verdicts on the device, straddling pairs over RCCL
            ok(upside_hip_comm_replica_swap(e, np, sets[k].data(), o.base_seed, rnd, k == 0, acc.data()));
        } else {
            ok((k == 0 ? upside_hip_replica_swap_from : upside_hip_replica_swap_next)(e, np, sets[k].data(), o.base_seed, rnd, draw, acc.data()));
            draw = acc.back();
        }
        for (int i = 0; i < np; ++i) {
            run.n_attempt[k]++; run.n_success[k] += acc[i]; run.pair_attempt[k][i]++; run.pair_success[k][i] += acc[i];
            if (acc[i]) swap(run.replica_index[sets[k][2 * i]], run.replica_index[sets[k][2 * i + 1]]);
        }
    }
}
}  // namespace

int upside_main_impl(int argc, const char* const* argv, int verbose) {
    const time_t process_start = time(nullptr);      // (of this run: the rendezvous ignores records older than it)
    Options o = parse_options(argc, argv);
    split_over_ranks(o);
    H5Eset_auto2(H5E_DEFAULT, NULL, NULL);
    Fleet fleet = load_fleet(o, verbose);
    DerivEngine* e = fleet.engines[0];      // the only engine wherever a communicator or Monte-Carlo moves are in use (load_fleet)
    read_hills(o, fleet);
    refuse_recentering_conflicts(o, fleet);
    fleet.set_pos(fleet.input_pos.data());
    fleet.init_md(o.temps.data(), o.base_seed + (uint32_t)o.sys_lo, (float)o.thermostat_timescale, o.dt, o.thermo_rounds);
    Run run;
    run.sets = parse_swap_sets(o);
    if (o.use_comm && !run.sets.empty()) comm_rendezvous(o, e, fleet.potential_digest, process_start);
    if (o.deriv_agreement) potential_deriv_agreement(o, fleet, verbose);
    run.temps = o.temps; run.energy.resize(o.n_system);
    fleet.compute(run.energy.data());
    if (verbose) { printf("Initial potential energy:"); for (float en : run.energy) printf(" %.2f", en); printf("\n"); }
    open_loggers(o, fleet, run);

    auto tstart = chrono::high_resolution_clock::now();
    const uint64_t n_round = o.n_round;
    g_received_signal = -1;
    int stop_signal = -1;
    {
    SignalGuard on_int(SIGINT), on_term(SIGTERM);
    uint64_t sync_start = 0;      // round at which the reference's outer loop (main.cpp:616) last started an iteration
    for (uint64_t rnd = 0; rnd < n_round && g_received_signal == -1;) {
        // pivots before the frame of the same round, never at t = 0 (main.cpp:626-630)
        if (run.have_mc && rnd && !(rnd % o.mc_rounds)) ok(upside_hip_mc_step(e, rnd));
        if (!(rnd % o.frame_rounds)) log_frame(o, fleet, run, rnd, verbose);
        uint64_t next = min<uint64_t>(n_round, (rnd / o.frame_rounds + 1) * (uint64_t)o.frame_rounds);
        if (o.anneal_factor != 1.) {
            if (!(rnd % o.thermo_rounds)) anneal_temperatures(o, fleet, run, rnd);
            next = min<uint64_t>(next, (rnd / o.thermo_rounds + 1) * (uint64_t)o.thermo_rounds);
        }
        // the reference leaves its inner loop for an exchange attempt only at a round AFTER the one the loop started with
        // (main.cpp:665: nr > last_start), so with an interval of one round it attempts every second round
        const uint64_t next_sync = o.replica_rounds ? ((sync_start + 2 + o.replica_rounds - 1) / o.replica_rounds) * (uint64_t)o.replica_rounds : 0;
        if (o.replica_rounds) next = min<uint64_t>(next, next_sync);
        if (run.have_mc) next = min<uint64_t>(next, (rnd / o.mc_rounds + 1) * (uint64_t)o.mc_rounds);
        fleet.run_rounds((int)(next - rnd));
        rnd = next;
        const bool at_sync = o.replica_rounds && (rnd == n_round || rnd == next_sync);
        if (at_sync) sync_start = rnd;
        if (at_sync && !(rnd % o.replica_rounds)) exchange_attempt(o, fleet, run, rnd);
    }
    fleet.sync();
    if (o.write_output) write_hills(fleet, run.loggers);
    for (auto& lg : run.loggers) lg.close();          // buffered frames reach the files also after an early stop (and before the communicator goes)
    if (o.use_comm) upside_hip_comm_free(e);
    stop_signal = g_received_signal;
    }   // the caller's signal handlers are back
    if (stop_signal != -1) fprintf(stderr, "Received early termination signal\n");
    double elapsed = chrono::duration<double>(chrono::high_resolution_clock::now() - tstart).count();
    printf("\n\nfinished in %.1f seconds (%.2f us/systems/step, %.1e simulation_time_unit/hour)\n", elapsed,
           elapsed * 1e6 / o.n_system / max<uint64_t>(n_round, 1) / 3, n_round * 3 * o.time_step / elapsed * 3600.);
    for (size_t k = 0; k < run.sets.size(); ++k) printf("swap set %zu: %ld / %ld accepted\n", k, run.n_success[k], run.n_attempt[k]);
    if (o.re_raise_signal && stop_signal != -1) raise(stop_signal);     // main.cpp:742-743
    return 0;
}

// C-ABI of libupside_hip.so: the reference's engine_c_library entry points
// (/root/reference/src/engine_c_library.cpp) over the device engine, plus the batched extension declared in
// include/upside_engine_c.h.  No exception crosses the boundary: failures print "ERROR: ..." to stderr and
// return NULL / 1 exactly like engine_c_library.cpp:15-20,37-45.
#include "../../include/upside_engine_c.h"
#include "engine.h"
#include "h5util.h"
#include "spline_fit.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace std;

int upside_main_impl(int argc, const char* const* argv, int verbose);

static thread_local string g_last_error;
static int fail(const string& s) { g_last_error = s; fprintf(stderr, "ERROR: %s\n", s.c_str()); return 1; }
#define API_TRY try {
#define API_CATCH(ret) } catch (const string& s) { fail(s); return ret; } catch (const char* s) { fail(s); return ret; } \
    catch (const std::exception& e) { fail(e.what()); return ret; } catch (...) { fail("unknown error"); return ret; }

extern "C" const char* upside_hip_last_error(void) { return g_last_error.c_str(); }
extern "C" int upside_hip_calibrate_valu(double* rates) { API_TRY upk_check(upk_calibrate_valu(rates), "calibrate_valu"); return 0; API_CATCH(1) }
void load_plugin_library(const string& path);   // engine.cpp
extern "C" int upside_hip_load_plugin(const char* path) { API_TRY load_plugin_library(path); return 0; API_CATCH(1) }
extern "C" int upside_hip_node_type_registered(const char* prefix) { API_TRY return node_creation_map().count(prefix) ? 1 : 0; API_CATCH(0) }
extern "C" void upside_hip_set_last_error(const char* msg) { fail(msg); }   // (for the other translation units of the C-ABI)
// MBAR over recorded series: engine-free; the checks, the staging and the iteration are upk_mbar_solve (kernels_mbar.hip)
extern "C" int upside_hip_mbar(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                               const float* rows, const long long* n_k, const double* periods, double tol, int max_iter, const double* f0,
                               int has_target, double beta_target, const float* row_target, double* f, double* D, double* log_w,
                               double* f_target, int* n_iter, double* last_delta) {
    API_TRY
    upk_mbar_problem_t P{};
    P.n_sample = n_sample; P.n_state = n_state; P.d = d; P.values = values; P.energy = energy; P.beta = beta; P.rows = rows; P.n_k = n_k;
    P.periods = periods; P.tol = tol; P.max_iter = max_iter; P.f0 = f0; P.has_target = has_target; P.beta_target = beta_target;
    P.row_target = row_target; P.f = f; P.denominators = D; P.log_w = log_w; P.f_target = f_target; P.n_iter = n_iter; P.last_delta = last_delta;
    char msg[256];
    if (upk_mbar_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
// the Gram pass of MBAR: the checks and the staging are upk_mbar_gram_solve (kernels_mbar_gram.hip)
extern "C" int upside_hip_mbar_gram(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                                    const float* rows, const long long* n_k, const double* periods, const double* f, int n_extra,
                                    const double* log_extra, double* G, double* colsum, double* D) {
    API_TRY
    upk_mbar_gram_problem_t P{};
    P.n_sample = n_sample; P.n_state = n_state; P.d = d; P.values = values; P.energy = energy; P.beta = beta; P.rows = rows; P.n_k = n_k;
    P.periods = periods; P.f = f; P.n_extra = n_extra; P.log_extra = log_extra; P.G = G; P.colsum = colsum; P.denominators = D;
    char msg[256];
    if (upk_mbar_gram_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
// bootstrap replicates of MBAR in one batch: the checks, the staging and the iteration are upk_mbar_boot_solve (kernels_mbar_boot.hip)
extern "C" int upside_hip_mbar_bootstrap(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                                         const float* rows, const long long* n_k, const double* periods, const int* state_of_sample,
                                         int n_replicate, const unsigned short* counts, double tol, int max_iter, const double* f0, int n_column,
                                         const double* log_numerator, double* f_boot, double* column_boot, int* n_iter, double* last_delta) {
    API_TRY
    upk_mbar_boot_problem_t P{};
    P.n_sample = n_sample; P.n_state = n_state; P.d = d; P.values = values; P.energy = energy; P.beta = beta; P.rows = rows; P.n_k = n_k;
    P.periods = periods; P.state_of_sample = state_of_sample; P.n_replicate = n_replicate; P.counts = counts; P.tol = tol; P.max_iter = max_iter;
    P.f0 = f0; P.n_column = n_column; P.log_numerator = log_numerator; P.f_boot = f_boot; P.column_boot = column_boot; P.n_iter = n_iter;
    P.last_delta = last_delta;
    char msg[256];
    if (upk_mbar_boot_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
// the same batch with the counts drawn on the device (upk_mbar_boot_solve_drawn), and the draw alone (upk_mbar_boot_draw_solve)
extern "C" int upside_hip_mbar_bootstrap_drawn(long long n_sample, int n_state, int d, const float* values, const double* energy, const double* beta,
                                               const float* rows, const long long* n_k, const double* periods, const int* state_of_sample,
                                               int n_replicate, unsigned long long seed, const long long* block, unsigned short* counts_out, double tol,
                                               int max_iter, const double* f0, int n_column, const double* log_numerator, double* f_boot,
                                               double* column_boot, int* n_iter, double* last_delta) {
    API_TRY
    upk_mbar_boot_problem_t P{};
    P.n_sample = n_sample; P.n_state = n_state; P.d = d; P.values = values; P.energy = energy; P.beta = beta; P.rows = rows; P.n_k = n_k;
    P.periods = periods; P.state_of_sample = state_of_sample; P.n_replicate = n_replicate; P.tol = tol; P.max_iter = max_iter;
    P.f0 = f0; P.n_column = n_column; P.log_numerator = log_numerator; P.f_boot = f_boot; P.column_boot = column_boot; P.n_iter = n_iter;
    P.last_delta = last_delta;
    upk_mbar_boot_draw_t D{};
    D.seed = seed; D.block = block; D.counts_out = counts_out;
    char msg[256];
    if (upk_mbar_boot_solve_drawn(&P, &D, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_mbar_bootstrap_counts(int n_state, const long long* n_k, long long n_sample, const int* state_of_sample,
                                                long long n_replicate, long long first_replicate, unsigned long long seed, const long long* block,
                                                unsigned short* counts_out) {
    API_TRY
    upk_mbar_boot_draw_t D{};
    D.seed = seed; D.block = block; D.first_replicate = first_replicate; D.counts_out = counts_out;
    char msg[256];
    if (upk_mbar_boot_draw_solve(n_state, n_k, n_sample, state_of_sample, n_replicate, &D, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
// statistical inefficiency of recorded series: the checks and the staging are upk_series_solve (kernels_series.hip)
extern "C" int upside_hip_series_inefficiency(int n_series, long long stride, const long long* length, const double* a, int n_origin,
                                              const long long* origin, int mintime, long long max_lag, double* g, long long* stop_lag,
                                              double* mean, double* variance) {
    API_TRY
    upk_series_problem_t P{};
    P.n_series = n_series; P.stride = stride; P.length = length; P.a = a; P.n_origin = n_origin; P.origin = origin; P.mintime = mintime;
    P.max_lag = max_lag; P.g = g; P.stop_lag = stop_lag; P.mean = mean; P.variance = variance;
    char msg[256];
    if (upk_series_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
// metadynamics analysis: the checks and the staging are upk_metad_bias_solve and upk_metad_grid_solve (kernels_metad.hip)
extern "C" int upside_hip_metad_bias(int n_list, int d, const long long* hill_start, const float* centers, const float* weights, const double* sigma,
                                     const double* periods, const long long* point_start, const double* points, const long long* n_visible, double* V) {
    API_TRY
    upk_metad_bias_problem_t P{};
    P.H.n_list = n_list; P.H.d = d; P.H.hill_start = hill_start; P.H.centers = centers; P.H.weights = weights; P.H.sigma = sigma; P.H.periods = periods;
    P.point_start = point_start; P.points = points; P.n_visible = n_visible; P.V = V;
    char msg[256];
    if (upk_metad_bias_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_metad_grid(int n_list, int d, const long long* hill_start, const float* centers, const float* weights, const double* sigma,
                                     const double* periods, const int* n_axis, const double* axes, int n_checkpoint, const long long* checkpoints,
                                     int n_scale, const double* scales, double* V_last, double* lse) {
    API_TRY
    upk_metad_grid_problem_t P{};
    P.H.n_list = n_list; P.H.d = d; P.H.hill_start = hill_start; P.H.centers = centers; P.H.weights = weights; P.H.sigma = sigma; P.H.periods = periods;
    P.n_axis = n_axis; P.axes = axes; P.n_checkpoint = n_checkpoint; P.checkpoints = checkpoints; P.n_scale = n_scale; P.scales = scales;
    P.V_last = V_last; P.lse = lse;
    char msg[256];
    if (upk_metad_grid_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
// pairwise RMSD of frames: the checks and the staging are upk_rmsd_frames_create and upk_rmsd_solve (kernels_rmsd.hip)
extern "C" int upside_hip_frames_create(int n_atom, long long n_frame, const float* pos, void** frames) {
    API_TRY
    char msg[256];
    if (upk_rmsd_frames_create(n_atom, n_frame, pos, (upk_rmsd_frames_t**)frames, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
extern "C" void upside_hip_frames_free(void* frames) { upk_rmsd_frames_free((upk_rmsd_frames_t*)frames); }
static int rmsd_call(upk_rmsd_problem_t& P, void* A, long long nA, const int* ia, void* B, long long nB, const int* ib) {
    API_TRY
    P.A = (const upk_rmsd_frames_t*)A; P.nA = nA; P.ia = ia; P.B = (const upk_rmsd_frames_t*)B; P.nB = nB; P.ib = ib;
    char msg[256];
    if (upk_rmsd_solve(&P, msg, (int)sizeof(msg))) throw string(msg);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_rmsd_matrix(void* A, long long nA, const int* ia, void* B, long long nB, const int* ib, double* out) {
    upk_rmsd_problem_t P{};
    P.mode = UPK_RMSD_MATRIX; P.out = out;
    return rmsd_call(P, A, nA, ia, B, nB, ib);
}
extern "C" int upside_hip_rmsd_nearest(void* A, long long nA, const int* ia, void* B, long long nB, const int* ib, long long* index, double* dist) {
    upk_rmsd_problem_t P{};
    P.mode = UPK_RMSD_NEAREST; P.index = index; P.dist = dist;
    return rmsd_call(P, A, nA, ia, B, nB, ib);
}
extern "C" int upside_hip_rmsd_count(void* A, long long nA, const int* ia, void* B, long long nB, const int* ib, double cutoff, long long* count) {
    upk_rmsd_problem_t P{};
    P.mode = UPK_RMSD_COUNT; P.cutoff = cutoff; P.count = count;
    return rmsd_call(P, A, nA, ia, B, nB, ib);
}

// ---- construction ----------------------------------------------------------------------------------
extern "C" int upside_hip_set_device(int device) {
    API_TRY hip_check(hipSetDevice(device), "hipSetDevice"); return 0; API_CATCH(1) }
extern "C" DerivEngine* upside_hip_construct(int n_atom, const char* potential_file, int n_system, bool quiet) {
    API_TRY
    if (n_system < 1) throw string("n_system must be positive");
    H5Eset_auto2(H5E_DEFAULT, NULL, NULL);
    auto config = h5u::open_config(potential_file);
    auto potential_group = h5u::open_group(config, "/input/potential");
    return initialize_engine_from_hdf5(n_atom, n_system, (hid_t_compat)(hid_t)potential_group, quiet);
    API_CATCH(nullptr)
}
// ---- Hamiltonian ladders: one engine, parameter values per system ------------------------------------------
namespace {
bool hamiltonian_batch_enabled() { const char* v = env_str("UPSIDE_HIP_HAMILTONIAN_BATCH"); return !(v && !strcmp(v, "0")); }
bool listed(const vector<string>& v, const string& x) { return find(v.begin(), v.end(), x) != v.end(); }
// the value bytes the table lets differ, for objects named below /input/potential ("node", "node/dataset")
h5u::DigestSkip potential_value_skip() {
    return [](const string& obj, const string& attr) {
        const size_t slash = obj.find('/');
        const auto* sp = per_system_value_spec(obj.substr(0, slash));
        if (!sp) return false;
        if (attr.empty()) return slash != string::npos && obj.find('/', slash + 1) == string::npos && listed(sp->datasets, obj.substr(slash + 1));
        return slash == string::npos && listed(sp->attributes, attr);
    };
}
// the same for objects named below one node's group (".", "dataset")
h5u::DigestSkip node_value_skip(const PerSystemValueSpec* sp) {
    return [sp](const string& obj, const string& attr) {
        if (!sp) return false;
        if (attr.empty()) return obj != "." && listed(sp->datasets, obj);
        return obj == "." && listed(sp->attributes, attr);
    };
}
}  // namespace

extern "C" int upside_hip_group_configurations(int n_file, const char* const* files, int* group_of) {
    API_TRY
    if (n_file < 0 || (n_file && (!files || !group_of))) throw string("invalid file list");
    H5Eset_auto2(H5E_DEFAULT, NULL, NULL);
    const bool batch = hamiltonian_batch_enabled();
    const h5u::DigestSkip skip = potential_value_skip();
    vector<unsigned long long> keys;
    for (int i = 0; i < n_file; ++i) {
        auto cf = h5u::open_config(files[i]);
        auto pg = h5u::open_group(cf, "/input/potential");
        const unsigned long long k = h5u::group_digest(pg, batch ? &skip : nullptr);
        size_t g = 0;
        while (g < keys.size() && keys[g] != k) ++g;
        if (g == keys.size()) keys.push_back(k);
        group_of[i] = (int)g;
    }
    return (int)keys.size();
    API_CATCH(-1)
}

extern "C" DerivEngine* upside_hip_construct_files(int n_atom, int n_file, const char* const* files, bool quiet) {
    API_TRY
    if (n_file < 1 || !files) throw string("n_file must be positive");
    H5Eset_auto2(H5E_DEFAULT, NULL, NULL);
    vector<h5u::Handle> cf, pg;
    for (int i = 0; i < n_file; ++i) { cf.push_back(h5u::open_config(files[i])); pg.push_back(h5u::open_group(cf.back(), "/input/potential")); }
    // what each system loads on top of system 0's engine: (system, node) of every node group that is not byte-identical
    vector<pair<int, string>> to_load;
    const auto names0 = h5u::node_names_in_group(pg[0]);
    const unsigned long long full0 = h5u::group_digest(pg[0]);
    for (int i = 1; i < n_file; ++i) {
        if (h5u::group_digest(pg[i]) == full0) continue;
        const auto names = h5u::node_names_in_group(pg[i]);
        for (auto& nm : names) if (!listed(names0, nm)) throw string(files[i]) + ": node " + nm + " is not in " + files[0] + " (one engine holds one node set)";
        for (auto& nm : names0) if (!listed(names, nm)) throw string(files[i]) + ": node " + nm + " of " + files[0] + " is missing (one engine holds one node set)";
        for (auto& nm : names0) {
            auto g0 = h5u::open_group(pg[0], nm), g1 = h5u::open_group(pg[i], nm);
            if (h5u::group_digest(g0) == h5u::group_digest(g1)) continue;
            const PerSystemValueSpec* sp = per_system_value_spec(nm);
            const h5u::DigestSkip skip = node_value_skip(sp);
            const auto d0 = h5u::object_digests(g0, &skip), d1 = h5u::object_digests(g1, &skip);
            if (d0 != d1) {
                string what;
                for (auto& kv : d0) { auto it = d1.find(kv.first); if (it == d1.end() || it->second != kv.second) { what = kv.first; break; } }
                if (what.empty()) for (auto& kv : d1) if (!d0.count(kv.first)) { what = kv.first; break; }
                throw string(files[i]) + ": node " + nm + ", " + (what == "." ? string("the node's attributes") : "dataset " + what) + " differs from " + files[0] +
                      (sp ? string(" (only the values of the per-system table may differ)") : string(" (this node type's values cannot differ per system)"));
            }
            to_load.emplace_back(i, nm);
        }
    }
    return initialize_engine_from_hdf5(n_atom, n_file, (hid_t_compat)(hid_t)pg[0], quiet, [&](DerivEngine& e) {
        for (auto& sl : to_load) {
            auto* pv = dynamic_cast<PerSystemValues*>(e.get(sl.second).computation.get());
            if (!pv) throw string(files[sl.first]) + ": node " + sl.second + " cannot hold per-system values";
            auto g = h5u::open_group(pg[sl.first], sl.second);
            try { pv->load_system_values(sl.first, (hid_t_compat)(hid_t)g); }
            catch (const string& err) { throw string(files[sl.first]) + ": node " + sl.second + ": " + err; }
        }
        for (auto& n : e.nodes) if (auto* pv = dynamic_cast<PerSystemValues*>(n.computation.get())) pv->finish_system_values();
    });
    API_CATCH(nullptr)
}
static PerSystemValues& per_system_node(DerivEngine* e, const char* node_name, int system) {
    if (!e || !node_name) throw string("engine or node name is NULL");
    if (system < 0 || system >= e->ctx.n_system) throw string("system index out of range");
    auto* pv = dynamic_cast<PerSystemValues*>(e->get(string(node_name)).computation.get());
    if (!pv) throw string("node ") + node_name + " has no per-system values";
    return *pv;
}
extern "C" int upside_hip_set_param_system(DerivEngine* e, const char* node_name, int system, int n_param, const float* param) {
    API_TRY
    per_system_node(e, node_name, system).set_param_system(system, vector<float>(param, param + n_param));
    e->invalidate_attempt();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_get_param_system(DerivEngine* e, const char* node_name, int system, int n_param, float* param) {
    API_TRY
    auto v = per_system_node(e, node_name, system).get_param_system(system);
    if (v.size() != size_t(n_param)) throw string("Wrong number of parameters, expected ") + to_string(v.size()) + " but got " + to_string(n_param);
    copy(begin(v), end(v), param);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_hamiltonian_swap(DerivEngine* e, int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted) {
    API_TRY
    if (!e) throw string("engine is NULL");
    e->hamiltonian_swap(n_pair, pairs, base_seed, round, draw0, accepted);
    return 0;
    API_CATCH(1)
}

extern "C" DerivEngine* construct_deriv_engine(int n_atom, const char* potential_file, bool quiet) {
    return upside_hip_construct(n_atom, potential_file, 1, quiet);
}
extern "C" void free_deriv_engine(DerivEngine* engine) { delete engine; }
extern "C" int upside_hip_n_system(DerivEngine* engine) { return engine ? engine->ctx.n_system : 0; }

// ---- positions / momenta ----------------------------------------------------------------------------
// host rows [n][width] <-> device rows [n][stride] (stride >= width; the padding of a packed row is left as it was)
static void pack_rows(const float* in, size_t n, int width, int stride, float* out) {
    for (size_t i = 0; i < n; ++i) for (int d = 0; d < width; ++d) out[i * stride + d] = in[i * width + d];
}
static void unpack_rows(const float* in, size_t n, int stride, int width, float* out) {
    for (size_t i = 0; i < n; ++i) for (int d = 0; d < width; ++d) out[i * width + d] = in[i * stride + d];
}
static void upload_pos(DerivEngine* e, const float* pos, int n_sys_in) {
    const int S = e->ctx.n_system, na = e->pos->n_atom, st = e->pos->stride;
    vector<float> buf((size_t)S * na * st, 0.f);
    for (int s = 0; s < S; ++s) pack_rows(pos + (size_t)(n_sys_in == 1 ? 0 : s) * na * 3, na, 3, st, buf.data() + (size_t)s * na * st);
    hip_check(hipMemcpyAsync(e->pos->output.p, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice, e->ctx.stream), "H2D pos");
    e->sync();
    e->invalidate_attempt();
}
static void download_rows(DerivEngine* e, const float* dev, int n_elem, int stride, int width, float* out, int n_sys_out) {
    vector<float> buf((size_t)n_sys_out * n_elem * stride);
    e->sync();
    hip_check(hipMemcpy(buf.data(), dev, buf.size() * sizeof(float), hipMemcpyDeviceToHost), "D2H");
    unpack_rows(buf.data(), (size_t)n_sys_out * n_elem, stride, width, out);
}

extern "C" int upside_hip_set_pos(DerivEngine* e, const float* pos) { API_TRY upload_pos(e, pos, e->ctx.n_system); return 0; API_CATCH(1) }
extern "C" int upside_hip_get_pos(DerivEngine* e, float* pos) {
    API_TRY download_rows(e, e->pos->output.p, e->pos->n_atom, e->pos->stride, 3, pos, e->ctx.n_system); return 0; API_CATCH(1) }
extern "C" int upside_hip_set_mom(DerivEngine* e, const float* mom) {
    API_TRY
    const size_t n = (size_t)e->ctx.n_system * e->pos->n_atom;
    vector<float> buf(n * 4, 0.f);
    pack_rows(mom, n, 3, 4, buf.data());
    hip_check(hipMemcpy(e->mom.p, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice), "H2D mom");
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_get_mom(DerivEngine* e, float* mom) {
    API_TRY download_rows(e, e->mom.p, e->pos->n_atom, 4, 3, mom, e->ctx.n_system); return 0; API_CATCH(1) }

// ---- evaluation (engine_c_library.cpp:29-64) ----------------------------------------------------------
extern "C" int upside_hip_compute(DerivEngine* e, float* energy, float* deriv) {
    API_TRY
    e->compute(energy ? PotentialAndDerivMode : DerivMode);
    e->check_device_errors();
    if (energy) { e->fetch_potentials(); for (int s = 0; s < e->ctx.n_system; ++s) energy[s] = e->potential[s]; }
    if (deriv) download_rows(e, e->pos->sens.p, e->pos->n_atom, e->pos->stride, 3, deriv, e->ctx.n_system);
    return 0;
    API_CATCH(1)
}
extern "C" int evaluate_energy(float* energy, DerivEngine* e, const float* pos) {
    API_TRY
    upload_pos(e, pos, 1);
    e->compute(PotentialAndDerivMode);
    e->check_device_errors();
    e->fetch_potentials();
    *energy = e->potential[0];
    return 0;
    API_CATCH(1)
}
extern "C" int evaluate_deriv(float* deriv, DerivEngine* e, const float* pos) {
    API_TRY
    upload_pos(e, pos, 1);
    e->compute(PotentialAndDerivMode);
    e->check_device_errors();
    e->fetch_potentials();
    download_rows(e, e->pos->sens.p, e->pos->n_atom, e->pos->stride, 3, deriv, 1);
    return 0;
    API_CATCH(1)
}

// ---- parameters and node inspection (engine_c_library.cpp:67-193) ---------------------------------------
extern "C" int set_param(int n_param, const float* param, DerivEngine* e, const char* node_name) {
    API_TRY
    if (!e || !node_name || (n_param && !param)) throw string("engine, node name or parameter array is NULL");
    // run_steps returns with its steps still in flight on the engine's non-blocking stream, and the nodes upload their tables with
    // blocking copies that do not order behind it: wait first, so that no step in flight reads a half-written table and no
    // graph exec is destroyed while it runs
    e->sync();
    e->invalidate_graph();   // cut-offs travel as kernel arguments
    e->invalidate_attempt(); // the energies of an exchange attempt belong to the old parameters
    e->get(string(node_name)).computation->set_param(vector<float>(param, param + n_param)); return 0; API_CATCH(1) }
extern "C" int get_param(int n_param, float* param, DerivEngine* e, const char* node_name) {
    API_TRY
    auto v = e->get(string(node_name)).computation->get_param();
    if (v.size() != size_t(n_param)) throw string("Wrong number of parameters, expected ") + to_string(v.size()) + " but got " + to_string(n_param);
    copy(begin(v), end(v), param);
    return 0;
    API_CATCH(1)
}
// engine_c_library.cpp:93-109 as built with -DPARAM_DERIV: system 0 of the batch
static int param_deriv_of(int n_param, float* deriv, DerivEngine* e, const char* node_name, int system) {
    if (system < 0 || system >= e->ctx.n_system) throw string("system index out of range");
    auto v = e->get(string(node_name)).computation->get_param_deriv(system);
    if (v.size() != size_t(n_param)) throw string("Wrong number of parameters, expected ") + to_string(v.size()) + " but got " + to_string(n_param);
    copy(begin(v), end(v), deriv);
    return 0;
}
extern "C" int get_param_deriv(int n_param, float* deriv, DerivEngine* e, const char* node_name) {
    API_TRY
    return param_deriv_of(n_param, deriv, e, node_name, 0); API_CATCH(1) }
extern "C" int upside_hip_get_param_deriv(DerivEngine* e, const char* node_name, int system, int n_param, float* deriv) {
    API_TRY
    return param_deriv_of(n_param, deriv, e, node_name, system); API_CATCH(1) }
// every system at once, deterministic (DerivEngine::param_deriv_all); n_param = the size of get_param_deriv, 0 for a node without one
static DerivEngine::ParamDeriv& param_deriv_request(DerivEngine* e, const char* node_name, int n_param, const void* out) {
    if (!node_name) throw string("node name is NULL");
    const int node = e->get_idx(string(node_name), false);
    if (node < 0) throw string("name not found: ") + node_name;
    auto& st = e->param_deriv_state(node);
    if (st.n_param != size_t(n_param)) throw string("Wrong number of parameters, expected ") + to_string(st.n_param) + " but got " + to_string(n_param);
    if (n_param && !out) throw string("output array is NULL");
    return st;
}
extern "C" int upside_hip_get_param_deriv_all(DerivEngine* e, const char* node_name, int n_param, float* deriv) {
    API_TRY
    auto& st = param_deriv_request(e, node_name, n_param, deriv);
    if (!st.n_param) return 0;
    const float* d = e->param_deriv_all(e->get_idx(node_name));
    hip_check(hipMemcpyAsync(deriv, d, (size_t)e->ctx.n_system * st.n_param * sizeof(float), hipMemcpyDeviceToHost, e->ctx.stream), "D2H param_deriv");
    e->sync();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_param_deriv_accumulate(DerivEngine* e, const char* node_name, const float* weights) {
    API_TRY
    if (!node_name) throw string("node name is NULL");
    e->param_deriv_accumulate(e->get_idx(string(node_name)), weights);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_param_deriv_read(DerivEngine* e, const char* node_name, int n_param, double* sum, long long* n_frame, int reset) {
    API_TRY
    auto& st = param_deriv_request(e, node_name, n_param, sum);
    if (!n_frame) throw string("n_frame is NULL");
    if (st.n_param) {
        if (st.sum.n) hip_check(hipMemcpyAsync(sum, st.sum.p, st.n_param * sizeof(double), hipMemcpyDeviceToHost, e->ctx.stream), "D2H param_deriv sum");
        e->sync();
        if (!st.sum.n) fill(sum, sum + st.n_param, 0.);
        if (reset && st.sum.n) hip_check(hipMemsetAsync(st.sum.p, 0, st.n_param * sizeof(double), e->ctx.stream), "memset");
    }
    *n_frame = st.n_frame;
    if (reset) st.n_frame = 0;
    return 0;
    API_CATCH(1)
}

extern "C" int get_output_dims(int* n_elem, int* elem_width, DerivEngine* e, const char* node_name) {
    API_TRY
    auto& dc = *e->get(string(node_name)).computation;
    if (dc.potential_term) { *n_elem = 1; *elem_width = 1; }
    else { auto& c = dynamic_cast<CoordNode&>(dc); *n_elem = c.n_elem; *elem_width = c.elem_width; }
    return 0;
    API_CATCH(1)
}
static int get_array(int n_output, float* out, DerivEngine* e, const char* node_name, bool want_sens) {
    API_TRY
    auto& dc = *e->get(string(node_name)).computation;
    if (dc.potential_term) {
        if (n_output != 1) throw string("wrong size for potential node");
        auto& p = dynamic_cast<PotentialNode&>(dc);
        e->sync();
        *out = p.potential_dev.download()[0];
    } else {
        auto& c = dynamic_cast<CoordNode&>(dc);
        if (n_output != c.n_elem * c.elem_width) throw string("wrong size for CoordNode");
        download_rows(e, want_sens ? c.sens.p : c.output.p, c.n_elem, c.stride, c.elem_width, out, 1);
    }
    return 0;
    API_CATCH(1)
}
extern "C" int get_output(int n_output, float* output, DerivEngine* e, const char* node_name) { return get_array(n_output, output, e, node_name, false); }
extern "C" int get_sens(int n_output, float* output, DerivEngine* e, const char* node_name) { return get_array(n_output, output, e, node_name, true); }
extern "C" int get_value_by_name(int n_output, float* output, DerivEngine* e, const char* node_name, const char* log_name) {
    API_TRY
    auto value = e->get(string(node_name)).computation->get_value_by_name(log_name);
    if (n_output != int(value.size()))
        throw string("expected size (") + to_string(n_output) + " elements) inconsistent with actual size (" + to_string(value.size()) + ")";
    copy(begin(value), end(value), output);
    return 0;
    API_CATCH(1)
}

// ---- engine-free spline helpers (engine_c_library.cpp:196-276); host arithmetic as in the reference -------
namespace {
void de_boor(float& val, float& der, const float* c, float x) {   // spline.h:136-174 on the window starting at c[int(x)-1]
    int x_bin = (int)x; float e = x - x_bin; const float* p = c + (x_bin - 1);
    float yu1 = e + 2.f, yu2 = e + 1.f, yu3 = e, f13 = 1.f / 3.f;
    float a11 = f13 * yu1, a12 = f13 * yu2, a13 = f13 * yu3;
    float c11 = (1.f - a11) * p[0] + a11 * p[1], d11 = p[1] - p[0];
    float c12 = (1.f - a12) * p[1] + a12 * p[2], d12 = p[2] - p[1];
    float c13 = (1.f - a13) * p[2] + a13 * p[3], d13 = p[3] - p[2];
    float a22 = 0.5f * yu2, a23 = 0.5f * yu3;
    float c22 = (1.f - a22) * c11 + a22 * c12, d22 = (1.f - a22) * d11 + a22 * d12;
    float c23 = (1.f - a23) * c12 + a23 * c13, d23 = (1.f - a23) * d12 + a23 * d13;
    val = (1.f - yu3) * c22 + yu3 * c23; der = (1.f - yu3) * d22 + yu3 * d23;
}
void clamped_de_boor(float& val, float& der, const float* c, float x, int n, bool strict) {
    bool lo = strict ? x < 1.f : x <= 1.f, hi = (float)(n - 2) <= x;
    if (lo) { val = (1.f / 6.f) * c[0] + (2.f / 3.f) * c[1] + (1.f / 6.f) * c[2]; der = 0.f; return; }
    if (hi) { val = (1.f / 6.f) * c[n - 3] + (2.f / 3.f) * c[n - 2] + (1.f / 6.f) * c[n - 1]; der = 0.f; return; }
    de_boor(val, der, c, x);
}
}  // namespace
extern "C" int clamped_spline_solve(int N, float* bspline_coeff, const float* values) {
    if (N < 3) return 1;
    const vector<double> v(values, values + (N - 2));
    const vector<double> c = tablefit::clamped_control_values_with_ghosts(v.data(), N - 2);
    for (int i = 0; i < N; ++i) bspline_coeff[i] = (float)c[i];
    return 0;
}
extern "C" int clamped_spline_value(int N, float* result, const float* bspline_coeff, int nx, float* x) {
    for (int i = 0; i < nx; ++i) { float d; clamped_de_boor(result[i], d, bspline_coeff, x[i], N, true); }
    return 0;
}
extern "C" int get_clamped_value_and_deriv(int N, float* result, const float* bspline_coeff, int nx, float* x) {
    for (int i = 0; i < nx; ++i) clamped_de_boor(result[i * 2], result[i * 2 + 1], bspline_coeff, x[i], N, false);
    return 0;
}
extern "C" int get_clamped_coeff_deriv(int N, float* result, const float*, float x) {
    for (int i = 0; i < N; ++i) result[i] = 0.f;
    int start; float data[4];
    if (x <= 1.f) { start = 0; data[0] = 1.f / 6.f; data[1] = 2.f / 3.f; data[2] = 1.f / 6.f; data[3] = 0.f; }
    else if (x >= N - 2) { start = N - 4; data[0] = 0.f; data[1] = 1.f / 6.f; data[2] = 2.f / 3.f; data[3] = 1.f / 6.f; }
    else {
        int x_bin = (int)x; start = x_bin - 1; float y = x - x_bin + 1.f;
        for (int i = 0; i < 4; ++i) { float dc[4] = {0.f, 0.f, 0.f, 0.f}; dc[i] = 1.f; float d; de_boor(data[i], d, dc, y); }
    }
    for (int i = 0; i < 4; ++i) result[start + i] = data[i];
    return 0;
}

// ---- MD on the device (main.cpp:515-523, 616-667; thermostat.h:9-12) -------------------------------------
static void thermostat_params(DerivEngine* e, float delta_t) {
    const int S = e->ctx.n_system;
    vector<float> ms(S), ns(S);
    for (int s = 0; s < S; ++s) {
        ms[s] = (float)exp(-delta_t / e->thermostat_timescale);
        ns[s] = sqrtf(e->temperature[s] * (1 - ms[s] * ms[s]));
    }
    e->mom_scale.upload(ms); e->noise_scale.upload(ns);
}
// thermostat temperature of every system from now on (System::set_temperature, main.cpp:107-110; used by simulated annealing)
extern "C" int upside_hip_set_temperature(DerivEngine* e, const float* temperature) {
    API_TRY
    const int S = e->ctx.n_system;
    if ((int)e->noise_scale.n != S) throw string("upside_hip_set_temperature needs upside_hip_init_md first");
    const float delta_t = e->thermostat_interval * 3 * e->dt;
    vector<float> ns(S);
    for (int s = 0; s < S; ++s) {
        e->temperature[s] = temperature[s];
        const float ms = (float)exp(-delta_t / e->thermostat_timescale);
        ns[s] = sqrtf(temperature[s] * (1 - ms * ms));
    }
    e->sync();
    hip_check(hipMemcpy(e->noise_scale.p, ns.data(), S * sizeof(float), hipMemcpyHostToDevice), "H2D");
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_init_md(DerivEngine* e, const float* temperature, uint32_t base_seed, float thermostat_timescale, float dt,
                                  int thermostat_interval_rounds) {
    std::vector<uint32_t> seeds(e ? e->ctx.n_system : 0);
    for (size_t s = 0; s < seeds.size(); ++s) seeds[s] = base_seed + (uint32_t)s;   // main.cpp:459
    return upside_hip_init_md_seeds(e, temperature, seeds.data(), thermostat_timescale, dt, thermostat_interval_rounds);
}
extern "C" int upside_hip_init_md_seeds(DerivEngine* e, const float* temperature, const uint32_t* seeds, float thermostat_timescale, float dt,
                                        int thermostat_interval_rounds) {
    API_TRY
    const int S = e->ctx.n_system;
    if (thermostat_interval_rounds < 1) throw string("thermostat interval must be at least one round");
    e->thermostat_timescale = thermostat_timescale; e->dt = dt; e->thermostat_interval = thermostat_interval_rounds;
    for (int s = 0; s < S; ++s) { e->temperature[s] = temperature[s]; e->seeds[s] = seeds[s]; }
    e->seed.upload(e->seeds);
    e->mom.fill_bytes(0);
    e->invalidate_graph();
    e->set_invocations(0); e->round_num = 0; e->stage_num = 0;
    thermostat_params(e, 1e8f);                     // mom_scale = 0: momenta fully resampled (main.cpp:515-522)
    upk_check(upk_thermostat(&e->ctx.L, e->mom.p, e->pos->n_atom, e->seed.p, e->n_invocations_dev.p, e->mom_scale.p, e->noise_scale.p), "thermostat");
    e->n_invocations++;
    e->sync();
    thermostat_params(e, thermostat_interval_rounds * 3 * dt);   // main.cpp:523
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_set_integrator(DerivEngine* e, int type) {
    API_TRY
    if (type != 0 && type != 1) throw string("integrator type must be 0 (Verlet) or 1 (Predescu)");
    if (e->stage_num != 0) throw string("an integration cycle is in progress");
    e->sync();
    if (type != e->integrator_type) e->invalidate_graph();      // (the stage weights are launch arguments of the recorded steps)
    e->integrator_type = type;
    return 0;
    API_CATCH(1)
}
static void require_md(DerivEngine* e, const char* who) {
    if ((int)e->noise_scale.n != e->ctx.n_system) throw string(who) + " needs upside_hip_init_md first (the thermostat's seeds and scales are set there)";
}
extern "C" int upside_hip_run_md(DerivEngine* e, int n_round) {
    API_TRY
    require_md(e, "upside_hip_run_md");
    if (e->stage_num != 0) throw string("an integration cycle is in progress (upside_hip_run_steps left it unfinished)");
    e->run_steps(3 * n_round);                             // main.cpp:657-663
    e->check_device_errors();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_run_steps(DerivEngine* e, int n_step) {
    API_TRY
    require_md(e, "upside_hip_run_steps");
    e->run_steps(n_step);
    e->check_device_errors();
    return 0;
    API_CATCH(1)
}
// ---- collective variables of every system (kernels_cv.hip) ---------------------------------------------------
extern "C" int upside_hip_cv_define(DerivEngine* e, int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos,
                                    const float* contact_r0, const float* contact_beta, const float* contact_lambda) {
    return upside_hip_cv_define2(e, n_cv, kind, atom_start, atoms, ref_pos, contact_r0, contact_beta, contact_lambda, nullptr);
}
extern "C" int upside_hip_cv_define2(DerivEngine* e, int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos,
                                     const float* contact_r0, const float* contact_beta, const float* contact_lambda, const float* dihedral_ref) {
    return upside_hip_cv_define3(e, n_cv, kind, atom_start, atoms, ref_pos, contact_r0, contact_beta, contact_lambda, dihedral_ref, nullptr, nullptr, nullptr);
}
extern "C" int upside_hip_cv_define3(DerivEngine* e, int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos,
                                     const float* contact_r0, const float* contact_beta, const float* contact_lambda, const float* dihedral_ref,
                                     const int* path_n_frame, const float* path_lambda, const float* path_ref_pos) {
    API_TRY e->cv_define(n_cv, kind, atom_start, atoms, ref_pos, contact_r0, contact_beta, contact_lambda, dihedral_ref, path_n_frame, path_lambda,
                         path_ref_pos); return 0; API_CATCH(1)
}
namespace {
vector<string> read_string_dataset(hid_t loc, const string& name) {      // fixed-length strings, one dimension
    h5u::Handle d(H5Dopen2(loc, name.c_str(), H5P_DEFAULT), H5Dclose);
    if (d < 0) throw string("dataset '") + name + "' not found";
    h5u::Handle sp(H5Dget_space(d), H5Sclose), ty(H5Dget_type(d), H5Tclose);
    if (H5Tget_class(ty) != H5T_STRING || H5Tis_variable_str(ty) > 0) throw string("'") + name + "' must hold fixed-length strings";
    if (H5Sget_simple_extent_ndims(sp) != 1) throw string("'") + name + "' must have one dimension";
    hsize_t n = 0; H5Sget_simple_extent_dims(sp, &n, NULL);
    const size_t w = H5Tget_size(ty);
    vector<char> buf(n * w + 1, '\0');
    if (n && H5Dread(d, ty, H5S_ALL, H5S_ALL, H5P_DEFAULT, buf.data()) < 0) throw string("unable to read dataset '") + name + "'";
    vector<string> out;
    for (hsize_t i = 0; i < n; ++i) { string t(buf.data() + i * w, w); while (t.size() && (t.back() == '\0' || t.back() == ' ')) t.pop_back(); out.push_back(t); }
    return out;
}
}
extern "C" int upside_hip_cv_load(DerivEngine* e, const char* config_file) {
    API_TRY
    H5Eset_auto2(H5E_DEFAULT, NULL, NULL);
    auto config = h5u::open_config(config_file);
    auto input = h5u::open_group(config, "/input");
    if (!h5u::exists(input, "collective_variables")) return 0;
    auto g = h5u::open_group(input, "collective_variables");
    const CvHostDefinition def = cv_read_definition((hid_t_compat)(hid_t)g, e->pos->n_atom, "/input/collective_variables");
    const size_t n_cv = (size_t)def.n_cv;
    auto names = read_string_dataset(g, "names");
    if (names.size() != n_cv) throw string("/input/collective_variables: names must have n_cv entries");
    e->cv_install(def);
    e->cv.names = names;
    return (int)n_cv;
    API_CATCH(-1)
}
extern "C" int upside_hip_cv_count(DerivEngine* e) { return e ? e->cv.C.n_cv : 0; }
extern "C" int upside_hip_cv_compute(DerivEngine* e, float* out) { API_TRY e->cv_compute(out); return 0; API_CATCH(1) }
extern "C" int upside_hip_cv_record(DerivEngine* e, int every_n_round, int capacity) { API_TRY e->cv_record(every_n_round, capacity); return 0; API_CATCH(1) }
extern "C" int upside_hip_cv_read(DerivEngine* e, int first, int n, float* out, long long* n_stored, long long* n_attempted, int reset) {
    API_TRY e->cv_read(first, n, out, n_stored, n_attempted, reset); return 0; API_CATCH(1)
}
extern "C" int upside_hip_cv_restraint_values(DerivEngine* e, const char* node_name, float* out) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    vector<float> v;
    const int n_cv = engine_cv_restraint_values(*e, string(node_name), out ? &v : nullptr);
    if (n_cv < 0) throw string("node ") + node_name + " is not a cv_restraint";
    copy(v.begin(), v.end(), out);
    return n_cv;
    API_CATCH(-1)
}
// ---- cv_metadynamics: the hills of a node (nodes.cpp: CVMetadynamics) ---------------------------------------------------------------
extern "C" int upside_hip_metad_info(DerivEngine* e, const char* node_name, int* d, int* capacity, int* n_list) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    engine_metad_info(*e, string(node_name), d, capacity, n_list);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_metad_read(DerivEngine* e, const char* node_name, int list, float* centers, float* weights, int* n_hill, long long* n_attempt) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    engine_metad_read(*e, string(node_name), list, centers, weights, n_hill, n_attempt);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_metad_write(DerivEngine* e, const char* node_name, int list, const float* centers, const float* weights, int n_hill) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    engine_metad_write(*e, string(node_name), list, centers, weights, n_hill);
    e->invalidate_attempt();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_metad_values(DerivEngine* e, const char* node_name, float* out) {
    API_TRY
    if (!e || !node_name || !out) throw string("engine, node name or out is NULL");
    const auto v = engine_metad_values(*e, string(node_name));
    copy(v.begin(), v.end(), out);
    return 0;
    API_CATCH(1)
}
// ---- cv_steer: clocks, accumulated work and centres of a node (nodes.cpp: CVSteer) ---------------------------------------------------
extern "C" int upside_hip_steer_info(DerivEngine* e, const char* node_name, int* n_cv) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    const int n = engine_steer_n_cv(*e, string(node_name));
    if (n_cv) *n_cv = n;
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_steer_read(DerivEngine* e, const char* node_name, long long* clock, double* work, double* center) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    engine_steer_read(*e, string(node_name), clock, work, center);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_steer_write(DerivEngine* e, const char* node_name, const long long* clock, const double* work) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    engine_steer_write(*e, string(node_name), clock, work);
    e->invalidate_attempt();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_steer_values(DerivEngine* e, const char* node_name, float* out) {
    API_TRY
    if (!e || !node_name) throw string("engine or node name is NULL");
    const auto v = engine_steer_values(*e, string(node_name));
    if (out) copy(v.begin(), v.end(), out);
    return 0;
    API_CATCH(1)
}
// ---- Monte-Carlo pivot moves (monte_carlo_sampler.cpp; main.cpp:628-630) ---------------------------------
extern "C" int upside_hip_load_mc(DerivEngine* e, const char* config_file) {
    API_TRY
    H5Eset_auto2(H5E_DEFAULT, NULL, NULL);
    auto config = h5u::open_config(config_file);
    auto input = h5u::open_group(config, "/input");
    int n = 0;
    e->invalidate_graph();
    if (h5u::exists(input, "pivot_moves")) { e->load_pivot_moves((hid_t_compat)(hid_t)input); n += e->pivot.loaded; }
    if (h5u::exists(input, "jump_moves")) { e->load_jump_moves((hid_t_compat)(hid_t)input); n += e->jump.loaded; }
    return n;                                   // number of samplers loaded
    API_CATCH(-1)
}
extern "C" int upside_hip_mc_step(DerivEngine* e, uint64_t round) {
    API_TRY e->mc_step(round); e->check_device_errors(); return 0; API_CATCH(1)
}
extern "C" int upside_hip_mc_stats(DerivEngine* e, int sampler, int* stats, int reset) {
    API_TRY
    if (sampler != 0 && sampler != 1) throw string("sampler must be 0 (pivot) or 1 (jump)");
    if (sampler == 0 ? !e->pivot.loaded : !e->jump.loaded) throw string("sampler not loaded");
    auto& buf = sampler == 0 ? e->pivot.stats : e->jump.stats;
    e->sync();
    auto st = buf.download();
    for (size_t i = 0; i < st.size(); ++i) stats[i] = st[i];
    if (reset) buf.fill_bytes(0);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_mc_loaded(DerivEngine* e, int sampler) { return e ? (sampler == 0 ? e->pivot.loaded : (sampler == 1 ? e->jump.loaded : 0)) : 0; }
extern "C" int upside_hip_recenter(DerivEngine* e) {
    API_TRY upk_check(upk_recenter(&e->ctx.L, e->pos->coord(), 0), "recenter"); e->sync(); return 0; API_CATCH(1) }
extern "C" int upside_hip_recenter_axes(DerivEngine* e, int xy_only) {
    API_TRY upk_check(upk_recenter(&e->ctx.L, e->pos->coord(), xy_only ? 1 : 0), "recenter"); e->sync(); return 0; API_CATCH(1) }

// ---- replica exchange among the systems of this engine (DerivEngine::replica_swap; main.cpp:227-275) -----------------------
extern "C" int upside_hip_replica_swap_from(DerivEngine* e, int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted) {
    API_TRY e->replica_swap(n_pair, pairs, base_seed, round, draw0, accepted, true); return 0; API_CATCH(1)
}
extern "C" int upside_hip_replica_swap_next(DerivEngine* e, int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted) {
    API_TRY e->replica_swap(n_pair, pairs, base_seed, round, draw0, accepted, false); return 0; API_CATCH(1)
}
extern "C" int upside_hip_replica_swap(DerivEngine* e, int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int* accepted) {
    std::vector<int> acc((size_t)(n_pair > 0 ? n_pair : 0) + 1);
    const int rc = upside_hip_replica_swap_from(e, n_pair, pairs, base_seed, round, 0, acc.data());
    if (!rc) for (int i = 0; i < n_pair; ++i) accepted[i] = acc[i];
    return rc;
}

// ---- coordinates of single systems; exchange across engines (main.cpp:227-275) ----------------------------------
// trade the coordinates of system s1 of engine e1 and system s2 of engine e2 (same atom count; device to device)
extern "C" int upside_hip_swap_between(DerivEngine* e1, int s1, DerivEngine* e2, int s2) {
    API_TRY
    if (!e1 || !e2 || s1 < 0 || s2 < 0 || s1 >= e1->ctx.n_system || s2 >= e2->ctx.n_system) throw string("invalid system");
    if (e1->pos->n_elem != e2->pos->n_elem) throw string("the two systems differ in their number of atoms");
    if (e1 == e2 && s1 == s2) return 0;
    const size_t row = (size_t)e1->pos->n_elem * e1->pos->stride;
    // Both engines have drained their streams (their pending work reads or writes the rows); the three copies go through e1's
    // stream into a staging row the engine keeps (a rejected pair of a Hamiltonian exchange attempt across engines comes through
    // here twice), and e2 is made to wait for them by the final synchronisation.
    e1->sync(); e2->sync();
    if (e1->swap_row.n < row) e1->swap_row.alloc(row);
    float* a = e1->pos->output.p + (size_t)s1 * row; float* b = e2->pos->output.p + (size_t)s2 * row;
    hipStream_t st = e1->ctx.stream;
    hip_check(hipMemcpyAsync(e1->swap_row.p, a, row * sizeof(float), hipMemcpyDeviceToDevice, st), "D2D");
    hip_check(hipMemcpyAsync(a, b, row * sizeof(float), hipMemcpyDeviceToDevice, st), "D2D");
    hip_check(hipMemcpyAsync(b, e1->swap_row.p, row * sizeof(float), hipMemcpyDeviceToDevice, st), "D2D");
    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
    e1->invalidate_attempt(); e2->invalidate_attempt();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_swap_systems(DerivEngine* e, int s1, int s2) { return upside_hip_swap_between(e, s1, e, s2); }
extern "C" int upside_hip_swap_system_pairs(DerivEngine* e, int n_pair, const int* pairs) {
    API_TRY
    if (n_pair <= 0) return 0;
    check_swap_set(e->ctx.n_system, n_pair, pairs);
    DevBuf<int> d; d.upload(vector<int>(pairs, pairs + 2 * n_pair));
    upk_check(upk_swap_system_pairs(&e->ctx.L, e->pos->coord(), n_pair, d.p, nullptr, 0), "swap_system_pairs");
    e->sync();
    e->invalidate_attempt();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_get_system_pos(DerivEngine* e, int sys, float* pos) {
    API_TRY
    if (sys < 0 || sys >= e->ctx.n_system) throw string("invalid system");
    const int na = e->pos->n_atom, st = e->pos->stride;
    vector<float> buf((size_t)na * st);
    e->sync();
    hip_check(hipMemcpy(buf.data(), e->pos->output.p + (size_t)sys * na * st, buf.size() * sizeof(float), hipMemcpyDeviceToHost), "D2H");
    unpack_rows(buf.data(), na, st, 3, pos);
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_set_system_pos(DerivEngine* e, int sys, const float* pos) {
    API_TRY
    if (sys < 0 || sys >= e->ctx.n_system) throw string("invalid system");
    const int na = e->pos->n_atom, st = e->pos->stride;
    vector<float> buf((size_t)na * st, 0.f);
    pack_rows(pos, na, 3, st, buf.data());
    e->sync();
    hip_check(hipMemcpy(e->pos->output.p + (size_t)sys * na * st, buf.data(), buf.size() * sizeof(float), hipMemcpyHostToDevice), "H2D");
    e->invalidate_attempt();
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_rebuild_flags(DerivEngine* e, const char* node_name, int* flags) {
    API_TRY
    vector<int> f;
    if (engine_rebuild_flags(*e, node_name, f)) throw string("node has no interaction graph");
    for (size_t i = 0; i < f.size(); ++i) flags[i] = f[i];
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_igraph_stats(DerivEngine* e, const char* node_name, double* out11) {
    API_TRY
    if (engine_igraph_stats(*e, node_name, out11)) throw string("node has no interaction graph");
    return 0;
    API_CATCH(1)
}
extern "C" int upside_hip_get_pairlist(DerivEngine* e, const char* node_name, int sys, int max_edge, int* i1, int* i2) {
    API_TRY
    vector<pair<int, int>> pl;
    int n = engine_pairlist(*e, node_name, sys, pl);
    if (n < 0) throw string("node has no interaction graph");
    for (int k = 0; k < n && k < max_edge; ++k) { i1[k] = pl[k].first; i2[k] = pl[k].second; }
    return n;
    API_CATCH(-1)
}
extern "C" int upside_hip_rotamer_iterations(DerivEngine* e, int* iters) {
    API_TRY
    vector<int> it;
    if (engine_rotamer_iterations(*e, it)) throw string("no rotamer node");
    copy(it.begin(), it.end(), iters);
    return 0;
    API_CATCH(1)
}

extern "C" int upside_hip_profile_reset(DerivEngine* e, int enable) {
    API_TRY e->sync(); e->ctx.flush_profile(); e->ctx.families.clear(); e->ctx.profile = enable != 0; return 0; API_CATCH(1) }
extern "C" int upside_hip_profile_dump(DerivEngine* e, char* buf, int buflen) {
    API_TRY
    e->sync(); e->ctx.flush_profile();
    string out;
    char line[512];
    const double bp_bytes = engine_bp_bytes(*e);   // of the last solve; the step-to-step variation is a few per cent
    for (auto& kv : e->ctx.families) {
        if (kv.first.compare(0, 3, "bp:") == 0 && kv.second.bytes == 0.) kv.second.bytes = bp_bytes * kv.second.launches;
        snprintf(line, sizeof(line), "%s %.6f %ld %.1f %.1f\n", kv.first.c_str(), kv.second.ms, kv.second.launches, kv.second.bytes, kv.second.pairs);
        out += line;
    }
    if ((int)out.size() + 1 > buflen) throw string("profile buffer too small");
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
    API_CATCH(1)
}
extern "C" double upside_hip_bp_min_bytes(DerivEngine* e) {
    API_TRY return engine_bp_min_bytes(*e); API_CATCH(-1.)
}
extern "C" double upside_hip_igraph_bytes_per_system(DerivEngine* e) {
    API_TRY return engine_igraph_bytes(*e); API_CATCH(-1.)
}

extern "C" int upside_main(int argc, const char* const* argv, int verbose) {
    API_TRY return upside_main_impl(argc, argv, verbose); API_CATCH(1)
}

// Host-side engine core: graph construction from HDF5 (deriv_engine.cpp:195-270), the forward/backward
// schedule (deriv_engine.cpp:124-169) and the integration cycle (deriv_engine.cpp:172-192).  Everything here
// only enqueues work on the engine's HIP stream; data stays in HBM.
#include "engine.h"
#include "h5util.h"
#include <dlfcn.h>
#include <algorithm>
#include <cstdlib>
#include <set>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstring>

using namespace std;

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw string("HIP error in ") + what + ": " + hipGetErrorString(e);
}
void upk_check(int code, const char* what) {
    if (code == 0) return;
    if (code >= 9000) {
        const char* why = "";
        switch (code) {      // (the codes of the launchers in kernels_*.hip)
            case 9003: why = ": more than 1024 rotamer nodes"; break;
            case 9004: case 9005: case 9006: why = ": the system does not fit the 160 KB of LDS this kernel stages it in"; break;
            case 9007: case 9008: why = ": side / mode / interaction type outside what the launcher implements"; break;
            case 9009: why = ": more than 65535 rows (row ids are 16 bits wide)"; break;
            case 9010: why = ": the graph's pair lists were allocated with another word width than its kernels read (upk_igraph_t::word16: 16-bit element "
                             "indices for every graph but the rotamer's, <= 65534 elements per side)"; break;
            case 9011: why = ": the hit-list refine exists for the side-chain graph (symmetric, 32-bit words) and for two-sided graphs with 16-bit words; "
                             "a symmetric radial graph walks its cached lists and has no hit lists"; break;
            case 9012: why = ": a graph with 16-bit list words packs bits beside the partner's index (upk_igraph_t::nbr_j_bits): the refine reads such a "
                             "word as the index itself"; break;
            default: break;
        }
        throw string("kernel launcher ") + what + " rejected its arguments (code " + to_string(code) + ")" + why;
    }
    throw string("HIP launch failure in ") + what + ": " + hipGetErrorString((hipError_t)code);
}

// ---- DeviceCtx profiling --------------------------------------------------------------------------
void DeviceCtx::flush() { upk_check(upk_fuse_flush(&L), "fuse_flush"); }
void DeviceCtx::begin(const std::string& fam) {
    if (!profile) return;
    flush();      // the bracket times the launches made inside it
    hipEvent_t a, b;
    hip_check(hipEventCreate(&a), "hipEventCreate"); hip_check(hipEventCreate(&b), "hipEventCreate");
    hip_check(hipEventRecord(a, stream), "hipEventRecord");
    families[fam].pending.emplace_back(a, b);
}
void DeviceCtx::end(const std::string& fam, double algorithmic_bytes, double pair_evaluations) {
    if (!profile) return;
    flush();
    auto& f = families[fam];
    hip_check(hipEventRecord(f.pending.back().second, stream), "hipEventRecord");
    f.launches += 1; f.bytes += algorithmic_bytes; f.pairs += pair_evaluations;
}
void DeviceCtx::flush_profile() {
    for (auto& kv : families) {
        for (auto& ev : kv.second.pending) {
            hip_check(hipEventSynchronize(ev.second), "hipEventSynchronize");
            float ms = 0.f;
            hip_check(hipEventElapsedTime(&ms, ev.first, ev.second), "hipEventElapsedTime");
            kv.second.ms += ms;
            (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second);
        }
        kv.second.pending.clear();
    }
}

// ---- ScatterPlan -----------------------------------------------------------------------------------
int ScatterPlan::add_source(int n_term, int n_slot, int w, const vector<int>& targets) {
    if (finalized) throw string("scatter plan already finalized");
    if ((int)targets.size() != n_term * n_slot) throw string("scatter source: wrong target table size");
    if (width && width != w) throw string("scatter sources of one node must share a width");
    width = w;
    Source s; s.n_term = n_term; s.n_slot = n_slot; s.width = w; s.targets = targets; s.offset = arena_size;
    arena_size += (long)n_term * n_slot * w;
    sources.push_back(move(s));
    return (int)sources.size() - 1;
}
void ScatterPlan::finalize(int n_target, int n_system) {
    vector<int> count(n_target + 1, 0);
    for (auto& s : sources) for (int t : s.targets) if (t >= 0) { if (t >= n_target) throw string("scatter target out of range"); count[t + 1]++; }
    for (int t = 0; t < n_target; ++t) count[t + 1] += count[t];
    vector<int> fill(count.begin(), count.end() - 1), entry(count[n_target]);
    for (auto& s : sources)
        for (int i = 0; i < (int)s.targets.size(); ++i) {
            int t = s.targets[i];
            if (t >= 0) entry[fill[t]++] = (int)(s.offset + (long)i * s.width);
        }
    csr_start.upload(count); csr_entry.upload(entry);
    arena.alloc((size_t)n_system * (size_t)max(arena_size, 1L));
    // source offsets become per-system-relative pointers: source_ptr(id) + s*arena_size
    finalized = true;
}

CoordNode::CoordNode(DeviceCtx* c, int n_elem_, int elem_width_)
    : DerivComputation(false), n_elem(n_elem_), elem_width(elem_width_), stride(ru(elem_width_)) {
    ctx = c;
    output.alloc((size_t)c->n_system * n_elem * stride);
    sens.alloc((size_t)c->n_system * n_elem * stride);
}
void CoordNode::gather_contributions() {
    if (scatter.sources.empty()) return;
    upk_check(upk_gather_contrib(&ctx->L, scatter.arena.p, scatter.arena_size, scatter.csr_start.p, scatter.csr_entry.p, coord(),
                                 scatter.width, 0), "gather_contrib");
}

// ---- host-fallback nodes (include/upside_hip_plugin.h) ------------------------------------------------------
namespace {
vector<int> identity_targets(int n) { vector<int> v(n); for (int i = 0; i < n; ++i) v[i] = i; return v; }

// all systems of a CoordNode's output (or sens), padding dropped: dst[system][elem][width]
void fetch_dense(DeviceCtx* ctx, const CoordNode& n, const float* dev, vector<float>& stage, vector<float>& dst) {
    const size_t total = (size_t)ctx->n_system * n.n_elem * n.stride;
    stage.resize(total); dst.resize((size_t)ctx->n_system * n.n_elem * n.elem_width);
    if (!total) return;
    hip_check(hipMemcpyAsync(stage.data(), dev, total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream), "D2H");
    hip_check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    for (size_t e = 0; e < (size_t)ctx->n_system * n.n_elem; ++e)
        for (int d = 0; d < n.elem_width; ++d) dst[e * n.elem_width + d] = stage[e * n.stride + d];
}

// din[a][system][elem][width] -> the scatter source `src[a]` of argument a (gathered into its sens in the backward sweep)
void push_arg_derivs(DeviceCtx* ctx, const vector<CoordNode*>& args, const vector<int>& src, const vector<vector<float>>& din) {
    for (size_t a = 0; a < args.size(); ++a) {
        CoordNode& n = *args[a];
        const size_t per_sys = (size_t)n.n_elem * n.elem_width;
        for (int s = 0; s < ctx->n_system && per_sys; ++s)
            hip_check(hipMemcpyAsync(n.scatter.source_ptr(src[a]) + (size_t)s * n.scatter.arena_size, din[a].data() + s * per_sys,
                                     per_sys * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "H2D");
    }
    hip_check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");   // the host vectors may be reused right away
}
}  // namespace

HostPotentialNode::HostPotentialNode(DeviceCtx* c, const vector<CoordNode*>& args_) : PotentialNode(c), args(args_) {
    for (CoordNode* a : args) src_.push_back(a->scatter.add_source(a->n_elem, 1, a->elem_width, identity_targets(a->n_elem)));
    in_.resize(args.size()); din_.resize(args.size()); stage_.resize(args.size());
}
void HostPotentialNode::compute_value(ComputeMode) {
    for (size_t a = 0; a < args.size(); ++a) {
        fetch_dense(ctx, *args[a], args[a]->output.p, stage_[a], in_[a]);
        din_[a].assign(in_[a].size(), 0.f);
    }
    vector<const float*> in(args.size()); vector<float*> din(args.size());
    for (int s = 0; s < ctx->n_system; ++s) {
        for (size_t a = 0; a < args.size(); ++a) {
            const size_t off = (size_t)s * args[a]->n_elem * args[a]->elem_width;
            in[a] = in_[a].data() + off; din[a] = din_[a].data() + off;
        }
        potential[s] = host_potential(s, in, din);
    }
    hip_check(hipMemcpyAsync(potential_dev.p, potential.data(), ctx->n_system * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "H2D");
    push_arg_derivs(ctx, args, src_, din_);
}

HostCoordNode::HostCoordNode(DeviceCtx* c, int n_elem_, int elem_width_, const vector<CoordNode*>& args_)
    : CoordNode(c, n_elem_, elem_width_), args(args_) {
    for (CoordNode* a : args) src_.push_back(a->scatter.add_source(a->n_elem, 1, a->elem_width, identity_targets(a->n_elem)));
    in_.resize(args.size()); din_.resize(args.size()); stage_.resize(args.size());
}
void HostCoordNode::compute_value(ComputeMode) {
    for (size_t a = 0; a < args.size(); ++a) fetch_dense(ctx, *args[a], args[a]->output.p, stage_[a], in_[a]);
    out_.assign((size_t)ctx->n_system * n_elem * stride, 0.f);
    vector<const float*> in(args.size()); vector<float> dense((size_t)n_elem * elem_width);
    for (int s = 0; s < ctx->n_system; ++s) {
        for (size_t a = 0; a < args.size(); ++a) in[a] = in_[a].data() + (size_t)s * args[a]->n_elem * args[a]->elem_width;
        host_value(s, in, dense.data());
        for (int e = 0; e < n_elem; ++e) for (int d = 0; d < elem_width; ++d) out_[((size_t)s * n_elem + e) * stride + d] = dense[(size_t)e * elem_width + d];
    }
    if (!out_.empty()) hip_check(hipMemcpyAsync(output.p, out_.data(), out_.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream), "H2D");
    // the arguments' derivative slots must not keep the previous evaluation's values if the backward sweep is skipped
    hip_check(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
}
void HostCoordNode::propagate_deriv() {
    vector<float> stage;
    fetch_dense(ctx, *this, sens.p, stage, dout_);
    vector<const float*> in(args.size()); vector<float*> din(args.size());
    for (size_t a = 0; a < args.size(); ++a) din_[a].assign(in_[a].size(), 0.f);
    for (int s = 0; s < ctx->n_system; ++s) {
        for (size_t a = 0; a < args.size(); ++a) {
            const size_t off = (size_t)s * args[a]->n_elem * args[a]->elem_width;
            in[a] = in_[a].data() + off; din[a] = din_[a].data() + off;
        }
        host_deriv(s, in, dout_.data() + (size_t)s * n_elem * elem_width, din);
    }
    push_arg_derivs(ctx, args, src_, din_);
}

// ---- registry (deriv_engine.cpp:50-92, 272-281) ------------------------------------------------------
NodeCreationMap& node_creation_map() {
    static NodeCreationMap m;
    if (!m.size())
        m[string("pos")] = NodeCreationFunction([](DeviceCtx*, hid_t_compat, const ArgList&) -> DerivComputation* {
            throw string("Cannot create pos-type node"); });
    return m;
}
bool is_prefix(const string& s1, const string& s2) { return s1 == s2.substr(0, s1.size()); }
void add_node_creation_function(string name_prefix, NodeCreationFunction fcn) {
    auto& m = node_creation_map();
    for (const auto& kv : m) {
        if (is_prefix(kv.first, name_prefix)) throw string("Internal error.  Type name ") + kv.first + " is a prefix of " + name_prefix + ".";
        if (is_prefix(name_prefix, kv.first)) throw string("Internal error.  Type name ") + name_prefix + " is a prefix of " + kv.first + ".";
    }
    m[name_prefix] = fcn;
}
void check_elem_width_lower_bound(const CoordNode& node, int lb) {
    if (node.elem_width < lb) throw string("expected argument with width at least ") + to_string(lb) + " but received argument with width " + to_string(node.elem_width);
}
void check_elem_width(const CoordNode& node, int w) {
    if (node.elem_width != w) throw string("expected argument with width ") + to_string(w) + " but received argument with width " + to_string(node.elem_width);
}
void check_arguments_length(const ArgList& a, int n) {
    if ((int)a.size() != n) throw string("expected ") + to_string(n) + " arguments but got " + to_string(a.size());
}

// ---- DerivEngine -----------------------------------------------------------------------------------
static void warn_removed_switches();
DerivEngine::DerivEngine(int n_atom, int n_system) {
    warn_removed_switches();
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev < 1) throw string("no HIP device available (this library has no CPU fallback)");
    ctx.n_system = n_system;
    hip_check(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking), "hipStreamCreate");   // (stream priorities were tried: a low-priority upkeep stream delays the joins, -10 to -27 %)
    ctx.L.n_system = n_system; ctx.L.stream = (void*)ctx.stream;
    ctx.L.fuse = upk_fuse_create(n_system);      // queue of fused per-element ops (kernels_basic.hip)
    if (!ctx.L.fuse) throw string("cannot allocate the fused-op table");
    ctx.L.batch = plan_merged_launches(plan_switches(), n_system, n_atom) ? upk_batch_create() : nullptr;   // merged launches (kernels_batch.h)
    ctx.error_flag.alloc(1);
    potential.assign(n_system, 0.f);
    Node n; n.name = "pos"; n.computation.reset(new Pos(&ctx, n_atom));
    nodes.push_back(move(n));
    pos = dynamic_cast<Pos*>(nodes[0].computation.get());
    mom.alloc((size_t)n_system * n_atom * 4);
    seeds.assign(n_system, 0u); temperature.assign(n_system, 1.f);
}
DerivEngine::~DerivEngine() {
    if (ctx.stream) { (void)hipStreamSynchronize(ctx.stream); }
    if (comm && comm_free) { comm_free(comm); comm = nullptr; }
    invalidate_graph();
    for (auto& kv : side) {
        (void)hipStreamSynchronize(kv.second.stream);
        (void)hipEventDestroy(kv.second.fork); (void)hipEventDestroy(kv.second.join);
    }
    for (auto& kv : side) if (kv.second.owns_stream) (void)hipStreamDestroy(kv.second.stream);
    nodes.clear();
    upk_fuse_destroy(ctx.L.fuse); ctx.L.fuse = nullptr;
    upk_batch_destroy(ctx.L.batch); ctx.L.batch = nullptr;
    if (ctx.stream) (void)hipStreamDestroy(ctx.stream);
}
void DerivEngine::add_node(const string& name, unique_ptr<DerivComputation> fcn, vector<string> argument_names) {
    if (any_of(nodes.begin(), nodes.end(), [&](const Node& n) { return n.name == name; })) throw string("name conflict in DerivEngine");
    Node node; node.name = name; node.computation = move(fcn); node.computation->name = name;
    nodes.push_back(move(node));
    for (auto& nm : argument_names) {
        int parent_idx = get_idx(nm);
        nodes.back().parents.push_back(parent_idx);
        nodes[parent_idx].children.push_back(nodes.size() - 1);
    }
}
DerivEngine::Node& DerivEngine::get(const string& name) {
    auto loc = find_if(begin(nodes), end(nodes), [&](const Node& n) { return n.name == name; });
    if (loc == nodes.end()) throw string("name not found");
    return *loc;
}
int DerivEngine::get_idx(const string& name, bool must_exist) {
    auto loc = find_if(begin(nodes), end(nodes), [&](const Node& n) { return n.name == name; });
    if (must_exist && loc == nodes.end()) throw string("name not found");
    return loc != nodes.end() ? int(loc - begin(nodes)) : -1;
}

void DerivEngine::finalize() {
    for (auto& n : nodes) { n.computation->finalize(); if (!n.computation->capturable()) graph_failed = true; }
    round_end_work.clear();
    for (auto& n : nodes) if (auto* w = dynamic_cast<RoundEndWork*>(n.computation.get())) round_end_work.push_back(w);
    // Unroll the level-synchronous sweep of deriv_engine.cpp:124-169 once; the order of events is static.
    schedule.clear();
    for (auto& n : nodes) n.germ_exec_level = n.deriv_exec_level = -1;
    // Order of the sweep.  Any order that runs a node after its parents (forward) / after its children (backward) computes the
    // same graph; the reference walks it level by level.  Here steps that only enqueue fused per-element ops are drawn together:
    // forward, every such step whose parents are done, then ONE other step, and so on; then the same backward.  The per-element
    // work of a force pass then reaches the device in a handful of launches instead of one per level.
    {
        const size_t N = nodes.size();
        std::vector<char> done(N, 0);
        n_batch_group = 0;
        auto sweep = [&](bool backward) {
            std::fill(done.begin(), done.end(), 0);
            size_t n_pre = 0;
            if (backward)      // a potential term has no backward step (it pushed its derivatives in the forward sweep): nobody waits for it
                for (size_t i = 0; i < N; ++i) if (nodes[i].computation->potential_term) { done[i] = 1; ++n_pre; nodes[i].deriv_exec_level = 0; }
            auto ready = [&](size_t i) {
                const auto& deps = backward ? nodes[i].children : nodes[i].parents;
                return !done[i] && all_of(begin(deps), end(deps), [&](size_t d) { return done[d] != 0; });
            };
            auto fused = [&](size_t i) { auto* c = nodes[i].computation.get(); return backward ? c->fused_backward : c->fused_forward; };
            int lvl = 0;
            for (size_t n_done = n_pre; n_done < N;) {
                // (round by round: the fused steps that are ready NOW do not depend on each other -- their ops run without barriers
                //  between them, on different wavefronts of the system's workgroup -- then the ones they unlock, ...)
                for (;;) {
                    std::vector<size_t> round;
                    for (size_t i = 0; i < N; ++i) if (fused(i) && ready(i)) round.push_back(i);
                    if (round.empty()) break;
                    for (size_t i : round) {
                        schedule.push_back(Step{(int)i, backward}); done[i] = 1; ++n_done;
                        (backward ? nodes[i].deriv_exec_level : nodes[i].germ_exec_level) = lvl;
                    }
                    ++lvl;
                }
                ++lvl;
                // then every other step that is ready: they do not depend on each other, so their kernels may share launches
                // (kernels_batch.h); without merged launches, one at a time
                // A backward step (and the forward step of a potential term) ADDS into the sensitivities of its parents with plain
                // read-modify-writes: two steps share launches only if they have no parent in common
                std::vector<size_t> group;
                for (size_t i = 0; i < N; ++i) if (ready(i)) {
                    bool clash = false;
                    if (backward || nodes[i].computation->potential_term)
                        for (size_t j : group) for (size_t pa : nodes[i].parents)
                            if (std::find(begin(nodes[j].parents), end(nodes[j].parents), pa) != end(nodes[j].parents)) clash = true;
                    if (clash) continue;
                    group.push_back(i);      // (the same order with and without merged launches: the bits of a system's forces do not depend on the batch size)
                }
                const int gid = group.size() > 1 ? n_batch_group++ : -1;
                for (size_t i : group) {
                    Step st{(int)i, backward}; st.batch = gid;
                    schedule.push_back(st); done[i] = 1; ++n_done;
                    (backward ? nodes[i].deriv_exec_level : nodes[i].germ_exec_level) = lvl;
                }
                ++lvl;
            }
        };
        sweep(false); sweep(true);
    }
    // one launch clears every sensitivity buffer at the start of a force pass
    {
        vector<float*> ptrs; vector<long> sizes;
        for (auto& n : nodes) {
            if (n.computation->potential_term) continue;
            auto* cn = static_cast<CoordNode*>(n.computation.get());
            if (!cn->sens.n) continue;
            ptrs.push_back(cn->sens.p); sizes.push_back((long)cn->sens.n);
        }
        n_zero = (int)ptrs.size();
        zero_ptrs.upload(ptrs); zero_sizes.upload(sizes);
    }
    // hoist prepare() of the nodes that have one to just after the forward step of the last parent it reads, on a
    // side stream
    if (ctx.L.batch) {
        // Merged launches: the list upkeep of ALL graphs as one group, placed behind the last forward step any of it reads (the
        // graphs' lists do not depend on each other: check / rebuild / refine of the five graphs run side by side in a handful of
        // launches, kernels_batch.h).  On the main stream: the per-element steps it could overlap with are one fused launch now.
        std::vector<size_t> prep;
        for (size_t i = 0; i < nodes.size(); ++i) if (nodes[i].computation->has_prepare()) prep.push_back(i);
        if (!prep.empty()) {
            std::vector<char> is_dep(nodes.size(), 0);
            for (size_t i : prep) {
                auto& named = nodes[i].computation->prepare_deps;
                if (named.empty()) for (size_t ip : nodes[i].parents) is_dep[ip] = 1;
                else for (size_t j = 0; j < nodes.size(); ++j)
                    if (std::find(begin(named), end(named), nodes[j].computation.get()) != end(named)) is_dep[j] = 1;
            }
            size_t last = 0;
            for (size_t k = 0; k < schedule.size(); ++k) if (!schedule[k].backward && is_dep[schedule[k].node]) last = k;
            // (a fused step behind `last` that nobody waits for stays behind the upkeep; the forward steps of the graphs come later anyway)
            std::vector<Step> out(schedule.begin(), schedule.begin() + last + 1);
            const int gid = prep.size() > 1 ? n_batch_group++ : -1;
            for (size_t i : prep) { Step ps{(int)i, false}; ps.prepare = true; ps.batch = gid; out.push_back(ps); }
            for (size_t k = last + 1; k < schedule.size(); ++k) {
                Step st = schedule[k];
                if (!st.backward && nodes[st.node].computation->has_prepare()) st.skip_prepare = true;
                out.push_back(st);
            }
            schedule.swap(out);
        }
        print_schedule();
        return;
    }
    if (plan_switches().ASYNC_PREPARE == 0) { print_schedule(); return; }
    // nodes a prepare() reads: the ones it names (any node of the graph, e.g. a grandparent whose output a parent copies
    // through), else all its parents
    std::vector<std::vector<size_t>> deps_of(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
        if (!nodes[i].computation->has_prepare()) continue;
        auto& named = nodes[i].computation->prepare_deps;
        if (named.empty()) deps_of[i] = nodes[i].parents;
        else for (size_t j = 0; j < nodes.size(); ++j)
            if (std::find(begin(named), end(named), nodes[j].computation.get()) != end(named)) deps_of[i].push_back(j);
        std::sort(begin(deps_of[i]), end(deps_of[i]));
        deps_of[i].erase(std::unique(begin(deps_of[i]), end(deps_of[i])), end(deps_of[i]));
    }
    {   // Run the forward steps that the upkeep waits for (and their ancestors) FIRST, everything else after them in
        // the original order: the list rebuilds then start as early as the graph allows and overlap with the
        // forward steps nobody is waiting for (springs, Ramachandran maps, backbone sterics).  The moved set is closed
        // under "parent of", so every step still follows the steps it depends on.
        std::vector<char> unlock(nodes.size(), 0);
        std::function<void(size_t)> mark = [&](size_t i) { if (unlock[i]) return; unlock[i] = 1; for (size_t ip : nodes[i].parents) mark(ip); };
        for (size_t i = 0; i < nodes.size(); ++i) for (size_t d : deps_of[i]) mark(d);
        std::vector<Step> first, rest;
        for (auto& st : schedule) ((!st.backward && unlock[st.node]) ? first : rest).push_back(st);
        first.insert(first.end(), rest.begin(), rest.end());
        schedule.swap(first);
    }
    // One upkeep stream per node: the rebuilds of different graphs run side by side.  (A single shared upkeep stream was an option until
    // round 6, behind a switch of its own, and lost at every batch size since the per-element nodes became a dozen fused launches:
    // 128 systems 86.6 vs 98.3 k, 256: 124.4 vs 138.8 k, 1024: 168.9 vs 177.0 k, 4096: 182.8 vs 188.7 k system-steps/s.)
    std::vector<Step> hoisted;
    std::vector<int> n_dep_left(nodes.size(), -1);
    for (size_t i = 0; i < nodes.size(); ++i) if (nodes[i].computation->has_prepare()) n_dep_left[i] = (int)deps_of[i].size();
    for (auto& st : schedule) {
        hoisted.push_back(st);
        if (st.backward) continue;
        std::vector<size_t> ready;
        for (size_t c = 0; c < nodes.size(); ++c) {
            if (n_dep_left[c] <= 0 || !std::binary_search(begin(deps_of[c]), end(deps_of[c]), (size_t)st.node)) continue;
            if (--n_dep_left[c] == 0) { ready.push_back(c); n_dep_left[c] = -1; }
        }
        // several nodes may become ready at once: upkeep in the order of their forward steps
        std::sort(begin(ready), end(ready), [&](size_t a, size_t b) {
            auto pos = [&](size_t n) { for (size_t k = 0; k < schedule.size(); ++k) if (!schedule[k].backward && schedule[k].node == (int)n) return k; return schedule.size(); };
            return pos(a) < pos(b); });
        for (size_t c : ready) {
            Step ps{(int)c, false}; ps.prepare = true; hoisted.push_back(ps);
            Side sd;
            hip_check(hipStreamCreateWithFlags(&sd.stream, hipStreamNonBlocking), "hipStreamCreate");
            hip_check(hipEventCreateWithFlags(&sd.fork, hipEventDisableTiming), "hipEventCreate");
            hip_check(hipEventCreateWithFlags(&sd.join, hipEventDisableTiming), "hipEventCreate");
            side[(int)c] = sd;
        }
    }
    schedule.swap(hoisted);
    last_prepare_step = -1;
    for (size_t k = 0; k < schedule.size(); ++k) if (schedule[k].prepare) last_prepare_step = (int)k;
    print_schedule();
}
void DerivEngine::print_schedule() {
    if (!env_set("UPSIDE_HIP_PRINT_SCHEDULE")) return;
    for (auto& st : schedule) {
        auto& n = nodes[st.node];
        fprintf(stderr, "%-8s L%-2d batch %-2d %s%-44s parents:", st.prepare ? "prepare" : (st.backward ? "backward" : "forward"),
                st.backward ? n.deriv_exec_level : n.germ_exec_level, st.batch,
                (st.backward ? n.computation->fused_backward : n.computation->fused_forward) && !st.prepare ? "[fused] " : "        ", n.name.c_str());
        for (size_t ip : n.parents) fprintf(stderr, " %s", nodes[ip].name.c_str());
        fprintf(stderr, "\n");
    }
}

void DerivEngine::compute(ComputeMode mode, bool keep_pending) {
    ++n_compute;
    ctx.n_pass = n_compute;      // (nodes that double-buffer by step parity read it: always in step with what a graph capture rolled back)
    // zero sensitivity for later derivative writing (deriv_engine.cpp:147-151), all nodes at once: nothing writes a
    // node's sens before that node's own forward step
    upk_check(upk_zero_many(&ctx.L, zero_ptrs.p, zero_sizes.p, n_zero), "zero_many");
    auto on_stream = [&](hipStream_t st, const std::function<void()>& f) {     // (the fused-op queue is empty on entry; what f queues runs on st)
        hipStream_t main_stream = ctx.stream;
        ctx.stream = st; ctx.L.stream = (void*)st;
        try { f(); ctx.flush(); } catch (...) { ctx.stream = main_stream; ctx.L.stream = (void*)main_stream; throw; }
        ctx.stream = main_stream; ctx.L.stream = (void*)main_stream;
    };
    int open_batch = -1, chain = 0;
    for (size_t k = 0; k < schedule.size(); ++k) {
        const Step& st = schedule[k];
        auto* c = nodes[st.node].computation.get();
        // merged launches: the steps of a group append to their own chains; the group's launches go out at its end
        const int want_batch = (ctx.profile || !ctx.L.batch) ? -1 : st.batch;      // (profiling brackets single launches with events: no merged launches then)
        if (want_batch != open_batch) {
            if (open_batch >= 0) upk_check(upk_batch_end(&ctx.L), "batch_end");
            open_batch = want_batch; chain = 0;
            if (open_batch >= 0) upk_check(upk_batch_begin(&ctx.L), "batch_begin");
        }
        if (open_batch >= 0) {
            if (!c->library_launchers_only) { upk_check(upk_batch_run(&ctx.L), "batch_run"); }
            upk_batch_chain(&ctx.L, chain++);
        }
        if (!c->library_launchers_only) ctx.flush();       // a node that may enqueue work of its own on the stream
        if (st.prepare && side.find(st.node) == side.end()) { c->prepare(); continue; }     // (merged launches: upkeep inline, see finalize)
        if (st.prepare) {   // fork: side stream waits for everything enqueued so far, runs the upkeep, records `join`
            Side& sd = side[st.node];
            ctx.flush();
            hip_check(hipEventRecord(sd.fork, ctx.stream), "hipEventRecord");
            hip_check(hipStreamWaitEvent(sd.stream, sd.fork, 0), "hipStreamWaitEvent");
            on_stream(sd.stream, [&] { c->prepare(); });
            hip_check(hipEventRecord(sd.join, sd.stream), "hipEventRecord");
            continue;
        }
        if (!st.backward) {
            if (c->has_prepare() && !st.skip_prepare) {
                auto it = side.find(st.node);
                if (it != side.end()) { ctx.flush(); hip_check(hipStreamWaitEvent(ctx.stream, it->second.join, 0), "hipStreamWaitEvent"); }
                else c->prepare();
            }
            c->compute_value(mode);
        } else if (!c->potential_term) {
            auto* cn = static_cast<CoordNode*>(c);
            cn->gather_contributions();
            if (!c->library_launchers_only) ctx.flush();       // (the gather is a fused op; the node may read its sens through the stream)
            c->propagate_deriv();
        }
    }
    if (open_batch >= 0) upk_check(upk_batch_end(&ctx.L), "batch_end");
    if (!keep_pending) ctx.flush();       // callers outside the MD loop find the queue empty
}

void DerivEngine::fetch_potentials() {
    sync();
    fill(potential.begin(), potential.end(), 0.f);
    for (auto& n : nodes) {
        if (!n.computation->potential_term) continue;
        auto* p = static_cast<PotentialNode*>(n.computation.get());
        p->potential = p->potential_dev.download();
        for (int s = 0; s < ctx.n_system; ++s) potential[s] += p->potential[s];   // node order, deriv_engine.cpp:143-146
    }
}

void DerivEngine::integration_stage(int stage, float dt_, float max_force) {
    // deriv_engine.cpp:176-177 (integrator from Predescu et al., 2012: double constants narrowed to float there as here)
    const float a = integrator_type == 1 ? (float)0.108991425403425322 : (float)(1. / 6.);
    const float b = integrator_type == 1 ? (float)0.290485609075128726 : (float)(1. / 3.);
    const float mom_update[] = {1.5f - 3.f * a, 1.5f - 3.f * a, 6.f * a};
    const float pos_update[] = {3.f * b, 3.0f - 6.f * b, 3.f * b};
    compute(DerivMode, true);       // the tail of the backward sweep, the leapfrog update and the head of the next force pass share a launch
    upk_check(upk_integration_stage(&ctx.L, mom.p, pos->coord(), dt_ * mom_update[stage], dt_ * pos_update[stage], max_force), "integration_stage");
}
void DerivEngine::integration_cycle(float dt_, float max_force) {
    for (int stage = 0; stage < 3; ++stage) integration_stage(stage, dt_, max_force);
}

void DerivEngine::set_invocations(uint64_t n) {
    n_invocations = n;
    if (!n_invocations_dev.n) n_invocations_dev.alloc(ctx.n_system);
    std::vector<unsigned long long> v(ctx.n_system, (unsigned long long)n);     // one copy per system (kernels_basic.hip: c_thermostat)
    sync();
    hip_check(hipMemcpy(n_invocations_dev.p, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice), "H2D");
}
void DerivEngine::md_step() {
    if (stage_num == 0 && !(round_num % thermostat_interval)) {   // main.cpp:657-662
        upk_check(upk_thermostat(&ctx.L, mom.p, pos->n_atom, seed.p, n_invocations_dev.p, mom_scale.p, noise_scale.p), "thermostat");
        n_invocations++;
    }
    integration_stage(stage_num, dt, 0.f);                        // main.cpp:663
    if (++stage_num == 3) {
        stage_num = 0; ++round_num;
        if (cv.R.every > 0) upk_check(upk_cv_record(&ctx.L, pos->coord(), &cv.C, &cv.R), "cv_record");      // a completed round (recording off: no launch)
        for (auto* w : round_end_work) w->round_end();
    }
    ++steps_done;
}
void DerivEngine::invalidate_graph() {
    md_graph_ready = false;
    if (md_graph_exec) { (void)hipGraphExecDestroy(md_graph_exec); md_graph_exec = nullptr; }
    if (md_graph) { (void)hipGraphDestroy(md_graph); md_graph = nullptr; }
}
bool DerivEngine::capture_md_graph() {
    invalidate_graph();
    const int sn = stage_num; const uint64_t rn = round_num, ni = n_invocations, sd = steps_done, nc = n_compute;
    static const bool debug = env_set("UPSIDE_HIP_GRAPH_DEBUG");
    ctx.flush();
    hipError_t err = hipStreamBeginCapture(ctx.stream, hipStreamCaptureModeGlobal);
    if (err != hipSuccess) { if (debug) fprintf(stderr, "graph: begin capture failed: %s\n", hipGetErrorString(err)); (void)hipGetLastError(); return false; }
    bool ok = true;
    try { for (int i = 0; i < 6; ++i) md_step(); ctx.flush(); }
    catch (const string& e) { ok = false; if (debug) fprintf(stderr, "graph: capture threw: %s\n", e.c_str()); }
    catch (...) { ok = false; }
    hipGraph_t g = nullptr;
    err = hipStreamEndCapture(ctx.stream, &g);
    if (err != hipSuccess || !g) { if (debug) fprintf(stderr, "graph: end capture failed: %s\n", hipGetErrorString(err)); (void)hipGetLastError(); ok = false; }
    if (debug && ok) { size_t nn = 0; (void)hipGraphGetNodes(g, nullptr, &nn); fprintf(stderr, "graph: captured 6 MD steps, %zu nodes\n", nn); }
    stage_num = sn; round_num = rn; n_invocations = ni; steps_done = sd; n_compute = nc;   // nothing ran: capture only records
    if (!ok) { if (g) (void)hipGraphDestroy(g); return false; }
    md_graph = g;
    if (hipGraphInstantiate(&md_graph_exec, md_graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); invalidate_graph(); return false; }
    md_graph_parity = (int)(n_compute & 1);   // the pair-list double buffers alternate with every force pass
    md_graph_ready = true;
    return true;
}
void DerivEngine::run_steps(int n_step) {
    static const bool sync_diag = env_set("UPSIDE_HIP_FUSE_TRACE");
    const bool use_graph = plan_graph_replay(plan_switches(), ctx.L.batch != nullptr, sync_diag);   // six MD steps replayed from a captured hipGraph
    int left = n_step;
    while (left > 0) {
        const bool aligned = stage_num == 0 && thermostat_interval == 1 && !ctx.profile && steps_done >= 6;
        if (use_graph && !graph_failed && aligned && left >= 6 && (!md_graph_ready || md_graph_parity == (int)(n_compute & 1))) {
            if (!md_graph_ready && !capture_md_graph()) { graph_failed = true; md_step(); --left; continue; }
            ctx.flush();
            hip_check(hipGraphLaunch(md_graph_exec, ctx.stream), "hipGraphLaunch");
            round_num += 2; n_invocations += 2; steps_done += 6; n_compute += 6; left -= 6;
            continue;
        }
        md_step(); --left;
    }
    ctx.flush();
}
void DerivEngine::load_pivot_moves(hid_t_compat input_group_) {
    const hid_t input = (hid_t)input_group_;
    auto grp = h5u::open_group(input, "pivot_moves");
    vector<hsize_t> d;
    auto pot = h5u::read<float>(grp, "proposal_pot", 3, &d);
    const int n_layer = (int)d[0], n_bin = (int)d[1];
    if (d[2] != d[1]) throw string("proposal_pot must be (n_layer, n_bin, n_bin)");
    auto atoms = h5u::read<int>(grp, "pivot_atom", 2, &d);
    const int n_loc = (int)d[0];
    if (d[1] != 5) throw string("pivot_atom must be (n_pivot_loc, 5)");
    h5u::check_size(grp, "pivot_range", {(size_t)n_loc, 2}); h5u::check_size(grp, "pivot_restype", {(size_t)n_loc});
    auto range = h5u::read<int>(grp, "pivot_range", 2); auto restype = h5u::read<int>(grp, "pivot_restype", 1);
    for (int l = 0; l < n_loc; ++l) {   // monte_carlo_sampler.cpp:49-58
        if (restype[l] < 0 || restype[l] >= n_layer) throw string("invalid pivot restype");
        for (int a = 0; a < 5; ++a) {
            const int at = atoms[l * 5 + a];
            if (at < 0 || at >= pos->n_atom) throw string("pivot_atom out of range");
            if (range[l * 2] <= at && at < range[l * 2 + 1]) throw string("pivot_range cannot contain any atoms in pivot_atom");
        }
        if (range[l * 2] < 0 || range[l * 2 + 1] > pos->n_atom || range[l * 2] > range[l * 2 + 1]) throw string("invalid pivot_range");
    }
    // normalise -log p and build the cdf in double (monte_carlo_sampler.cpp:62-78)
    vector<float> cdf(pot.size());
    const size_t nb2 = (size_t)n_bin * n_bin;
    for (int nl = 0; nl < n_layer; ++nl) {
        double sum_prob = 0.;
        for (size_t i = 0; i < nb2; ++i) { sum_prob += exp(-pot[nl * nb2 + i]); cdf[nl * nb2 + i] = (float)sum_prob; }
        const double inv = 1. / sum_prob, ls = log(sum_prob);
        for (size_t i = 0; i < nb2; ++i) { cdf[nl * nb2 + i] = (float)(cdf[nl * nb2 + i] * inv); pot[nl * nb2 + i] = (float)(pot[nl * nb2 + i] + ls); }
        cdf[(nl + 1) * nb2 - 1] = 1.f;
    }
    const int S = ctx.n_system;
    pivot.atoms.upload(atoms); pivot.range.upload(range); pivot.restype.upload(restype); pivot.pot.upload(pot); pivot.cdf.upload(cdf);
    pivot.stats.alloc((size_t)S * 2); pivot.pos_copy.alloc((size_t)S * pos->n_atom * pos->stride);
    pivot.delta_lprob.alloc(S); pivot.e_old.alloc(S); pivot.e_new.alloc(S);
    pivot.P.n_loc = n_loc; pivot.P.n_bin = n_bin; pivot.P.n_layer = n_layer;
    pivot.P.atoms = pivot.atoms.p; pivot.P.range = pivot.range.p; pivot.P.restype = pivot.restype.p; pivot.P.pot = pivot.pot.p; pivot.P.cdf = pivot.cdf.p;
    pivot.loaded = n_loc > 0;
}
void DerivEngine::load_jump_moves(hid_t_compat input_group_) {
    const hid_t input = (hid_t)input_group_;
    auto grp = h5u::open_group(input, "jump_moves");
    vector<hsize_t> d;
    auto range = h5u::read<int>(grp, "atom_range", 2, &d);
    const int n_chain = (int)d[0];
    if (d[1] != 2) throw string("atom_range must be (n_chain, 2)");
    h5u::check_size(grp, "sigma_trans", {(size_t)n_chain}); h5u::check_size(grp, "sigma_rot", {(size_t)n_chain});
    auto st = h5u::read<float>(grp, "sigma_trans", 1); auto sr = h5u::read<float>(grp, "sigma_rot", 1);
    for (int i = 0; i < n_chain; ++i)
        if (range[i * 2] < 0 || range[i * 2 + 1] > pos->n_atom || range[i * 2] >= range[i * 2 + 1]) throw string("invalid jump atom_range");
    const int S = ctx.n_system;
    jump.range.upload(range); jump.sigma_trans.upload(st); jump.sigma_rot.upload(sr);
    jump.stats.alloc((size_t)S * 2);
    if (!pivot.pos_copy.n) { pivot.pos_copy.alloc((size_t)S * pos->n_atom * pos->stride); pivot.delta_lprob.alloc(S); pivot.e_old.alloc(S); pivot.e_new.alloc(S); }
    jump.J.n_chain = n_chain; jump.J.atom_range = jump.range.p; jump.J.sigma_trans = jump.sigma_trans.p; jump.J.sigma_rot = jump.sigma_rot.p;
    jump.loaded = n_chain > 0;
}
void DerivEngine::mc_step(uint64_t round) {   // MultipleMonteCarloSampler::execute, monte_carlo_sampler.cpp:255-288
    if (!pivot.loaded && !jump.loaded) throw string("no Monte-Carlo moves loaded");
    const size_t S = (size_t)ctx.n_system;
    if (pivot.temperature.n != S) pivot.temperature.alloc(S);          // (allocated once: no free / malloc / device-wide sync per move)
    auto refresh = [&](DevBuf<float>& b, const vector<float>& v) {
        if (b.n != S) b.alloc(S);
        hip_check(hipMemcpyAsync(b.p, v.data(), S * sizeof(float), hipMemcpyHostToDevice, ctx.stream), "H2D");
    };
    refresh(pivot.temperature, temperature);
    invalidate_attempt();                                               // coordinates may move: no swap set can reuse older energies
    for (int sampler = 0; sampler < 2; ++sampler) {
        if (sampler == 0 ? !pivot.loaded : !jump.loaded) continue;
        compute(PotentialAndDerivMode); fetch_potentials();
        refresh(pivot.e_old, potential);
        if (sampler == 0) upk_check(upk_pivot_propose(&ctx.L, pos->coord(), pivot.pos_copy.p, &pivot.P, seed.p, round, pivot.delta_lprob.p), "pivot_propose");
        else upk_check(upk_jump_propose(&ctx.L, pos->coord(), pivot.pos_copy.p, &jump.J, seed.p, round, pivot.delta_lprob.p), "jump_propose");
        compute(PotentialAndDerivMode); fetch_potentials();
        refresh(pivot.e_new, potential);
        // the acceptance uniform is the generator's next draw: the pivot proposal used one, the jump proposal two
        upk_check(upk_mc_accept(&ctx.L, pos->coord(), pivot.pos_copy.p, pivot.e_old.p, pivot.e_new.p, pivot.delta_lprob.p, pivot.temperature.p,
                                seed.p, round, sampler == 0 ? 2 : 3, sampler == 0 ? 1 : 2, (sampler == 0 ? pivot.stats : jump.stats).p), "mc_accept");
        sync();
    }
}
// switches that earlier rounds read and this build does not: said once, so that an A/B script does not compare a variant with itself
static void warn_removed_switches() {
    static bool done = false;
    if (done) return;
    done = true;
    for (const char* v : {"UPSIDE_HIP_BP_RESIDENT", "UPSIDE_HIP_BP_THREADS", "UPSIDE_HIP_BP_LDS_CAP_KB", "UPSIDE_HIP_FUSE_W8", "UPSIDE_HIP_BATCH_KINDS",
                          "UPSIDE_HIP_HB_THREADS", "UPSIDE_HIP_PLR_ROWS_SMALL", "UPSIDE_HIP_SLOT_WGS", "UPSIDE_HIP_ORDER_EVERY", "UPSIDE_HIP_CLEAR_SLOTS",
                          "UPSIDE_HIP_BP_CLUSTER_MIN_C", "UPSIDE_HIP_MAX_SYSTEMS", "UPSIDE_HIP_PAIR2_ENERGY", "UPSIDE_HIP_UPKEEP_STREAMS",
                          "UPSIDE_HIP_BP_SPLIT", "UPSIDE_HIP_SCHEDULE"})
        if (env_set(v)) fprintf(stderr, "upside_hip: %s is set but no longer read by this build (removed experiment switch, see INTEGRATION.md section 6)\n", v);
}
void DerivEngine::sync() { ctx.flush(); hip_check(hipStreamSynchronize(ctx.stream), "hipStreamSynchronize"); }

// ---- parameter derivatives of every system (upside_hip_get_param_deriv_all / _param_deriv_accumulate / _read) ----------------
DerivEngine::ParamDeriv& DerivEngine::param_deriv_state(int node) {
    DerivComputation* c = nodes.at(node).computation.get();
    if (!c) throw string("impossible pointer value");
    auto* b = dynamic_cast<BatchedParamDeriv*>(c);
    const size_t n = b ? b->param_deriv_size() : c->get_param_deriv(0).size();
    ParamDeriv& st = param_derivs[node];
    if (n != st.n_param) { st.n_param = n; st.table.alloc(0); st.sum.alloc(0); st.n_frame = 0; }   // (set_param may change the size)
    return st;
}
const float* DerivEngine::param_deriv_all(int node) {
    ParamDeriv& st = param_deriv_state(node);
    if (!st.n_param) return nullptr;
    const int S = ctx.n_system;
    if (!st.table.n) st.table.alloc((size_t)S * st.n_param);
    DerivComputation* c = nodes[node].computation.get();
    if (auto* b = dynamic_cast<BatchedParamDeriv*>(c)) { b->param_deriv_all(st.table.p); return st.table.p; }
    vector<float> h((size_t)S * st.n_param);   // a node without the batched form: one system at a time
    for (int s = 0; s < S; ++s) {
        auto v = c->get_param_deriv(s);
        if (v.size() != st.n_param) throw string("get_param_deriv returned a different size for system ") + to_string(s);
        copy(v.begin(), v.end(), h.begin() + (size_t)s * st.n_param);
    }
    hip_check(hipMemcpyAsync(st.table.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, ctx.stream), "H2D param_deriv");
    sync();
    return st.table.p;
}
void DerivEngine::param_deriv_accumulate(int node, const float* weights) {
    const float* d = param_deriv_all(node);
    ParamDeriv& st = param_derivs[node];
    if (d) {
        if (!st.sum.n) st.sum.alloc(st.n_param);
        const float* w = nullptr;
        if (weights) {
            if (!st.weight.n) st.weight.alloc(ctx.n_system);
            hip_check(hipMemcpyAsync(st.weight.p, weights, ctx.n_system * sizeof(float), hipMemcpyHostToDevice, ctx.stream), "H2D weights");
            w = st.weight.p;
        }
        upk_check(upk_param_deriv_reduce(&ctx.L, d, (int)st.n_param, w, st.sum.p), "param_deriv_reduce");
    }
    ++st.n_frame;
}

// ---- collective variables (upside_hip_cv_define / _compute / _record / _read) -----------------------------------------------------
CvHostDefinition cv_check_definition(int n_atom, int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos,
                                     const float* contact_r0, const float* contact_beta, const float* contact_lambda, const float* dihedral_ref,
                                     const int* path_n_frame, const float* path_lambda, const float* path_ref_pos) {
    static const char* kind_name[] = {"rg", "rmsd", "contacts", "distance", "dihedral", "dihedral_similarity", "", "", "path_s", "path_z"};
    if (n_cv < 0) throw string("collective variables: n_cv is negative");
    if (n_cv > UPK_CV_MAX) throw string("collective variables: ") + to_string(n_cv) + " CVs exceed the kernel's limit of " + to_string(UPK_CV_MAX) + " (UPK_CV_MAX)";
    if (n_cv && (!kind || !atom_start || !atoms)) throw string("collective variables: kind, atom_start and atoms must be given");
    CvHostDefinition def; def.n_cv = n_cv;
    vector<int>&h_kind = def.kind, &h_start = def.atom_start, &h_atoms = def.atoms, &h_aux = def.aux_start;
    vector<double>&h_ref = def.ref, &h_ref_g = def.ref_g;
    vector<float>&h_r0 = def.r0, &h_beta = def.beta, &h_lambda = def.lambda, &h_dref = def.dihedral_ref;
    h_aux.assign((size_t)n_cv, 0); h_ref_g.assign((size_t)n_cv, 0.); h_beta.assign((size_t)n_cv, 0.f); h_lambda.assign((size_t)n_cv, 0.f);
    def.path_n_frame.assign((size_t)n_cv, 0); def.path_frame_start.assign((size_t)n_cv, 0); def.path_lambda.assign((size_t)n_cv, 0.f);
    if (n_cv) {
        h_kind.assign(kind, kind + n_cv); h_start.assign(atom_start, atom_start + n_cv + 1);
        if (h_start[0] != 0) throw string("collective variables: atom_start[0] must be 0");
        size_t n_ref = 0, n_pair = 0, n_quad = 0, n_path_row = 0, n_path_frame = 0;
        for (int c = 0; c < n_cv; ++c) {
            const string who = "collective variable " + to_string(c);
            const bool is_path = h_kind[c] == UPK_CV_PATH_S || h_kind[c] == UPK_CV_PATH_Z;
            if (h_kind[c] < 0 || (h_kind[c] > UPK_CV_DIHEDRAL_SIMILARITY && !is_path))
                throw who + ": unknown kind " + to_string(h_kind[c]) + " (0 rg, 1 rmsd, 2 contacts, 3 distance, 4 dihedral, 5 dihedral_similarity, 8 path_s, 9 path_z)";
            const string whok = who + " (" + kind_name[h_kind[c]] + ")";
            const long n = (long)h_start[c + 1] - h_start[c];
            if (n < 0) throw whok + ": atom_start must not decrease";
            if (n == 0) throw whok + ": empty selection";
            if (n > UPK_CV_MAX_LIST) throw whok + ": " + to_string(n) + " list entries exceed the limit of " + to_string(UPK_CV_MAX_LIST) + " (UPK_CV_MAX_LIST)";
            for (long i = h_start[c]; i < h_start[c + 1]; ++i)
                if (atoms[i] < 0 || atoms[i] >= n_atom) throw whok + ": atom " + to_string(atoms[i]) + " out of range (n_atom " + to_string(n_atom) + ")";
            if (h_kind[c] == UPK_CV_RMSD) {
                if (n < 3) throw whok + ": an rmsd selection needs at least 3 atoms";
                if (!ref_pos) throw whok + ": ref_pos must be given";
                h_aux[c] = (int)n_ref; n_ref += (size_t)n;
            } else if (h_kind[c] == UPK_CV_CONTACTS) {
                if (n % 2) throw whok + ": a contacts list holds interleaved pairs, its length must be even";
                if (!contact_r0 || !contact_beta || !contact_lambda) throw whok + ": contact_r0, contact_beta and contact_lambda must be given";
                for (long i = 0; i < n / 2; ++i) { const float r = contact_r0[n_pair + i]; if (!(r > 0.f) || !std::isfinite(r)) throw whok + ": r0 must be positive and finite"; }
                if (!std::isfinite(contact_beta[c]) || !std::isfinite(contact_lambda[c])) throw whok + ": beta and lambda must be finite";
                h_aux[c] = (int)n_pair; n_pair += (size_t)(n / 2);
                h_beta[c] = contact_beta[c]; h_lambda[c] = contact_lambda[c];
            } else if (h_kind[c] == UPK_CV_DISTANCE) {
                if (n != 2) throw whok + ": a distance needs exactly 2 atoms";
            } else if (h_kind[c] == UPK_CV_DIHEDRAL || h_kind[c] == UPK_CV_DIHEDRAL_SIMILARITY) {
                if (h_kind[c] == UPK_CV_DIHEDRAL && n != 4) throw whok + ": a dihedral needs exactly 4 atoms";
                if (n % 4) throw whok + ": a dihedral_similarity list holds interleaved quadruples, its length must be a multiple of 4";
                for (long i = 0; i < n / 4; ++i) {
                    const int* q = atoms + h_start[c] + 4 * i;
                    if (q[0] == q[1] || q[0] == q[2] || q[0] == q[3] || q[1] == q[2] || q[1] == q[3] || q[2] == q[3])
                        throw whok + ": quadruple " + to_string(i) + " repeats an atom";
                }
                if (h_kind[c] == UPK_CV_DIHEDRAL_SIMILARITY) {
                    if (!dihedral_ref) throw whok + ": dihedral_ref must be given (upside_hip_cv_define2)";
                    for (long i = 0; i < n / 4; ++i) if (!std::isfinite(dihedral_ref[n_quad + i])) throw whok + ": dihedral_ref is not finite";
                    h_aux[c] = (int)n_quad; n_quad += (size_t)(n / 4);
                }
            } else if (is_path) {
                if (!path_n_frame || !path_lambda || !path_ref_pos)
                    throw whok + ": path_n_frame, path_lambda and path_ref_pos must be given (upside_hip_cv_define3)";
                const int K = path_n_frame[c];
                if (K < 2 || K > UPK_CV_PATH_MAX_FRAMES)
                    throw whok + ": " + to_string(K) + " frames; a path needs 2 to " + to_string(UPK_CV_PATH_MAX_FRAMES) + " (UPK_CV_PATH_MAX_FRAMES)";
                if (n < 3) throw whok + ": a path selection needs at least 3 atoms";
                if (!std::isfinite(path_lambda[c]) || !(path_lambda[c] > 0.f)) throw whok + ": path_lambda must be positive and finite";
                for (size_t i = 0; i < (size_t)K * n * 3; ++i)
                    if (!std::isfinite(path_ref_pos[n_path_row * 3 + i])) throw whok + ": path_ref_pos is not finite";
                h_aux[c] = (int)n_path_row;      // (rows of path_ref_pos for now: the rmsd references' rows are added below)
                def.path_n_frame[c] = K; def.path_frame_start[c] = (int)n_path_frame; def.path_lambda[c] = path_lambda[c];
                n_path_row += (size_t)K * n; n_path_frame += (size_t)K;
            }
        }
        h_atoms.assign(atoms, atoms + h_start[n_cv]);
        h_r0.assign(contact_r0, contact_r0 + (contact_r0 ? n_pair : 0));
        h_dref.assign(dihedral_ref, dihedral_ref + (dihedral_ref ? n_quad : 0));
        h_ref.resize((n_ref + n_path_row) * 3);
        def.path_g.assign(n_path_frame, 0.);
        for (int c = 0; c < n_cv; ++c) if (h_kind[c] == UPK_CV_PATH_S || h_kind[c] == UPK_CV_PATH_Z) {      // every frame centred in double, and its squared norm
            const size_t n = (size_t)(h_start[c + 1] - h_start[c]), in = (size_t)h_aux[c] * 3;
            h_aux[c] += (int)n_ref;
            for (int k = 0; k < def.path_n_frame[c]; ++k) {
                const float* f = path_ref_pos + in + (size_t)k * n * 3;
                double* o = h_ref.data() + ((size_t)h_aux[c] + (size_t)k * n) * 3;
                double cen[3] = {0., 0., 0.}, g = 0.;
                for (size_t i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) cen[d] += (double)f[3 * i + d];
                for (int d = 0; d < 3; ++d) cen[d] /= (double)n;
                for (size_t i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) { const double v = (double)f[3 * i + d] - cen[d]; o[3 * i + d] = v; g += v * v; }
                def.path_g[(size_t)def.path_frame_start[c] + k] = g;
            }
        }
        for (int c = 0; c < n_cv; ++c) if (h_kind[c] == UPK_CV_RMSD) {      // the reference centred in double, and its squared norm
            const size_t n = (size_t)(h_start[c + 1] - h_start[c]), o = (size_t)h_aux[c] * 3;
            double cen[3] = {0., 0., 0.};
            for (size_t i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) { const double v = ref_pos[o + 3 * i + d]; if (!std::isfinite(v)) throw string("collective variable ") + to_string(c) + " (rmsd): ref_pos is not finite"; cen[d] += v; }
            for (int d = 0; d < 3; ++d) cen[d] /= (double)n;
            double g = 0.;
            for (size_t i = 0; i < n; ++i) for (int d = 0; d < 3; ++d) { const double v = (double)ref_pos[o + 3 * i + d] - cen[d]; h_ref[o + 3 * i + d] = v; g += v * v; }
            h_ref_g[c] = g;
        }
    }
    return def;
}
CvHostDefinition cv_read_definition(hid_t_compat group, int n_atom, const string& where) {
    const hid_t g = (hid_t)group;
    auto kind = h5u::read<int>(g, "kind", 1);
    const size_t n_cv = kind.size();
    auto atom_start = h5u::read<int>(g, "atom_start", 1);
    if (atom_start.size() != n_cv + 1) throw where + ": atom_start must have n_cv + 1 entries";
    auto atoms = h5u::read<int>(g, "atoms", 1);
    if (atom_start.back() != (int)atoms.size() || atom_start[0] != 0) throw where + ": atom_start does not span atoms";
    vector<hsize_t> d;
    auto ref_pos = h5u::read<float>(g, "ref_pos", 2, &d);
    if (d[0] && d[1] != 3) throw where + ": ref_pos must be (n, 3)";
    auto r0 = h5u::read<float>(g, "contact_r0", 1);
    auto beta = h5u::read<float>(g, "contact_beta", 1), lambda = h5u::read<float>(g, "contact_lambda", 1);
    if (beta.size() != n_cv || lambda.size() != n_cv) throw where + ": contact_beta and contact_lambda must have n_cv entries";
    vector<float> dref;      // optional: a file without it has no dihedral_similarity
    if (h5u::exists(g, "dihedral_ref")) dref = h5u::read<float>(g, "dihedral_ref", 1);
    vector<int> path_k; vector<float> path_lam, path_ref;      // optional, all three or none: a file without them has no path kind
    const int n_path_set = (int)h5u::exists(g, "path_n_frame") + (int)h5u::exists(g, "path_lambda") + (int)h5u::exists(g, "path_ref_pos");
    if (n_path_set != 0 && n_path_set != 3) throw where + ": path_n_frame, path_lambda and path_ref_pos come together";
    if (n_path_set) {
        path_k = h5u::read<int>(g, "path_n_frame", 1); path_lam = h5u::read<float>(g, "path_lambda", 1);
        if (path_k.size() != n_cv || path_lam.size() != n_cv) throw where + ": path_n_frame and path_lambda must have n_cv entries";
        vector<hsize_t> pd;
        path_ref = h5u::read<float>(g, "path_ref_pos", 2, &pd);
        if (pd[0] && pd[1] != 3) throw where + ": path_ref_pos must be (n, 3)";
    }
    // the packed arrays must be as long as the kinds say (cv_check_definition reads them by those counts)
    size_t n_ref = 0, n_pair = 0, n_quad = 0, n_path_row = 0;
    for (size_t c = 0; c < n_cv; ++c) {
        const long n = (long)atom_start[c + 1] - atom_start[c];
        if (n < 0) throw where + ": atom_start must not decrease";
        if (kind[c] == UPK_CV_PATH_S || kind[c] == UPK_CV_PATH_Z) {
            if (!n_path_set) throw where + ": collective variable " + to_string(c) + " is a path kind, but path_n_frame, path_lambda and path_ref_pos are absent";
            if (path_k[c] < 2 || path_k[c] > UPK_CV_PATH_MAX_FRAMES)
                throw where + ": collective variable " + to_string(c) + ": " + to_string(path_k[c]) + " frames; a path needs 2 to " +
                      to_string(UPK_CV_PATH_MAX_FRAMES) + " (UPK_CV_PATH_MAX_FRAMES)";
            n_path_row += (size_t)path_k[c] * (size_t)n;
        }
        if (kind[c] == UPK_CV_RMSD) n_ref += (size_t)n; else if (kind[c] == UPK_CV_CONTACTS) n_pair += (size_t)(n / 2);
        else if (kind[c] == UPK_CV_DIHEDRAL_SIMILARITY) n_quad += (size_t)(n / 4);
    }
    if (ref_pos.size() != n_ref * 3) throw where + ": ref_pos holds " + to_string(ref_pos.size() / 3) + " rows, the rmsd selections " + to_string(n_ref);
    if (r0.size() != n_pair) throw where + ": contact_r0 holds " + to_string(r0.size()) + " entries, the contacts lists " + to_string(n_pair) + " pairs";
    if (dref.size() != n_quad)
        throw where + ": dihedral_ref holds " + to_string(dref.size()) + " entries, the dihedral_similarity lists " + to_string(n_quad) + " quadruples";
    if (path_ref.size() != n_path_row * 3)
        throw where + ": path_ref_pos holds " + to_string(path_ref.size() / 3) + " rows, the frames of the path kinds " + to_string(n_path_row);
    return cv_check_definition(n_atom, (int)n_cv, kind.data(), atom_start.data(), atoms.data(), ref_pos.data(), r0.data(), beta.data(), lambda.data(),
                               dref.data(), n_path_set ? path_k.data() : nullptr, n_path_set ? path_lam.data() : nullptr, n_path_set ? path_ref.data() : nullptr);
}
void CvDeviceDefinition::upload(const CvHostDefinition& d) {
    kind.upload(d.kind); atom_start.upload(d.atom_start); atoms.upload(d.atoms); aux_start.upload(d.aux_start);
    ref.upload(d.ref); ref_g.upload(d.ref_g); r0.upload(d.r0); beta.upload(d.beta); lambda.upload(d.lambda); dihedral_ref.upload(d.dihedral_ref);
    C.n_cv = d.n_cv; C.kind = kind.p; C.atom_start = atom_start.p; C.atoms = atoms.p; C.aux_start = aux_start.p;
    C.ref = ref.p; C.ref_g = ref_g.p; C.r0 = r0.p; C.beta = beta.p; C.lambda = lambda.p; C.dihedral_ref = dihedral_ref.p;
    path_n_frame.upload(d.path_n_frame); path_frame_start.upload(d.path_frame_start); path_g.upload(d.path_g); path_lambda.upload(d.path_lambda);
    C.path_n_frame = path_n_frame.p; C.path_frame_start = path_frame_start.p; C.path_g = path_g.p; C.path_lambda = path_lambda.p;
}
void DerivEngine::cv_define(int n_cv, const int* kind, const int* atom_start, const int* atoms, const float* ref_pos, const float* contact_r0,
                            const float* contact_beta, const float* contact_lambda, const float* dihedral_ref, const int* path_n_frame,
                            const float* path_lambda, const float* path_ref_pos) {
    // everything is checked and built on the host before the first device array is touched: a refusal leaves the old definition in force
    cv_install(cv_check_definition(pos->n_atom, n_cv, kind, atom_start, atoms, ref_pos, contact_r0, contact_beta, contact_lambda, dihedral_ref, path_n_frame,
                                   path_lambda, path_ref_pos));
}
void DerivEngine::cv_install(const CvHostDefinition& def) {
    sync();
    invalidate_graph();
    cv_record(0, 0);                       // samples of another definition have another width
    cv.names.clear();
    cv.upload(def);
    cv.out.alloc((size_t)ctx.n_system * def.n_cv);
}
void DerivEngine::cv_compute(float* out_host) {
    if (!cv.C.n_cv) throw string("no collective variables defined (upside_hip_cv_define / upside_hip_cv_load)");
    if (!out_host) throw string("upside_hip_cv_compute: out is NULL");
    upk_check(upk_cv_compute(&ctx.L, pos->coord(), &cv.C, cv.out.p), "cv_compute");
    hip_check(hipMemcpyAsync(out_host, cv.out.p, cv.out.n * sizeof(float), hipMemcpyDeviceToHost, ctx.stream), "D2H cv");
    sync();
}
void DerivEngine::cv_record(int every_n_round, int capacity) {
    if (every_n_round < 0) throw string("upside_hip_cv_record: every_n_round is negative");
    if (every_n_round > 0) {
        if (!cv.C.n_cv) throw string("no collective variables defined (upside_hip_cv_define / upside_hip_cv_load)");
        if (capacity < 1) throw string("upside_hip_cv_record: capacity must be positive");
    }
    if (!every_n_round && !cv.R.every) return;
    sync();
    invalidate_graph();                    // the captured rounds hold (or lack) the record launch and its arguments
    cv.R = upk_cv_record_t{};
    if (!every_n_round) { cv.rounds.alloc(0); cv.n_attempt.alloc(0); cv.samples.alloc(0); return; }
    cv.rounds.alloc(ctx.n_system); cv.n_attempt.alloc(ctx.n_system);       // (zeroed: rounds are counted from this call)
    cv.samples.alloc((size_t)capacity * ctx.n_system * cv.C.n_cv);
    cv.R.rounds = cv.rounds.p; cv.R.n_attempt = cv.n_attempt.p; cv.R.samples = cv.samples.p; cv.R.every = every_n_round; cv.R.capacity = capacity;
}
void DerivEngine::cv_read(int first, int n, float* out_host, long long* n_stored, long long* n_attempted, int reset) {
    if (cv.R.every <= 0) throw string("collective variables are not being recorded (upside_hip_cv_record)");
    sync();
    int attempted = 0;
    hip_check(hipMemcpy(&attempted, cv.n_attempt.p, sizeof(int), hipMemcpyDeviceToHost), "D2H cv counters");      // (equal entries)
    const long long stored = std::min<long long>(attempted, cv.R.capacity);
    if (n_stored) *n_stored = stored;
    if (n_attempted) *n_attempted = attempted;
    if (n > 0) {
        if (!out_host) throw string("upside_hip_cv_read: out is NULL");
        if (first < 0 || (long long)first + n > stored) throw string("upside_hip_cv_read: samples [") + to_string(first) + ", " + to_string((long long)first + n) + ") requested, " + to_string(stored) + " stored";
        const size_t row = (size_t)ctx.n_system * cv.C.n_cv;
        hip_check(hipMemcpy(out_host, cv.samples.p + (size_t)first * row, (size_t)n * row * sizeof(float), hipMemcpyDeviceToHost), "D2H cv samples");
    } else if (n < 0) throw string("upside_hip_cv_read: n is negative");
    if (reset) cv.n_attempt.fill_bytes(0);      // the round counter runs on: the sampling phase is kept
}

void DerivEngine::check_device_errors() {
    sync();
    auto f = ctx.error_flag.download();
    if (f[0]) {
        ctx.error_flag.fill_bytes(0);
        if (f[0] == 7)   // kernels_rotamer.hip: the LAST cluster_barrier (behind the epilogue) gave up waiting; earlier ones hand the system to the one-workgroup solve
            throw string("belief propagation: a workgroup of a solve cluster never arrived (the cluster solve needs all its workgroups "
                         "co-resident; something else occupied the device): the forces of this step are not valid.  Set UPSIDE_HIP_BP_CLUSTER=1 "
                         "to use the one-workgroup solve");
        if (f[0] == 8)   // kernels_rotamer.hip: RotGradOp2::flush
            throw string("side-chain gradient: a bead's gradient, or a pair's contribution to it, is not finite or beyond what the fixed-point "
                         "accumulators of the pair pass hold (2^24 per pair, 2^40 per bead): the forces of this step are not valid");
        if (f[0] == 10)  // kernels_pair.hip: CovBackwardOp2 (pair2_device.h: lds_add_fixed22_pairs)
            throw string("hbond_coverage gradient: a pair's contribution to a gradient is not finite or is 2^24 or more, beyond what the "
                         "fixed-point accumulators of the coverage pair pass hold: the forces of this step are not valid");
        if (f[0] == 9)   // kernels_rotamer.hip: k_rotamer_bp, layout of the message inbox
            throw string("belief propagation: 3-float message rows were laid out for a solve that does not hold its inbox in LDS (internal error): "
                         "the forces of this step are not valid");
        if (f[0] == 4)   // kernels_basic.hip: c_backbone_pairs
            throw string("backbone sterics: a residue has more neighbours within cutoff + skin than its cached row holds: raise "
                         "UPSIDE_HIP_BACKBONE_LIST_CAP (default 128) or set UPSIDE_HIP_BACKBONE_LIST=0");
        throw string("device capacity overflow (code ") + to_string(f[0]) +
            "): raise UPSIDE_HIP_NBR_CAP / UPSIDE_HIP_SLOT_FACTOR (1 = neighbour list, 2 = residue-pair slots, 3 = node adjacency)";
    }
}

// ---- graph construction (deriv_engine.cpp:195-270) ---------------------------------------------------
// external node types (include/upside_hip_plugin.h): their static initialisers call add_node_creation_function
void load_plugin_library(const string& path) {
    static set<string> loaded;
    if (loaded.count(path)) return;
    // RTLD_LOCAL: the plug-in finds this library through its own DT_NEEDED entry (it must be linked against libupside_hip.so);
    // a global load would also promote this library's C++ symbols -- add_node_creation_function, node_creation_map: the
    // reference's own names -- to the global scope, where a later-loaded libupside.so would bind to them
    if (!dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL)) throw string("cannot load plug-in ") + path + ": " + dlerror();
    loaded.insert(path);
}
static void load_plugins_from_env() {
    static bool done = false;
    if (done) return;
    done = true;
    const char* e = env_str("UPSIDE_HIP_PLUGINS");
    if (!e) return;
    string all(e);
    for (size_t b = 0; b <= all.size();) {
        size_t c = all.find(':', b); if (c == string::npos) c = all.size();
        if (c > b) load_plugin_library(all.substr(b, c - b));
        b = c + 1;
    }
}

DerivEngine* initialize_engine_from_hdf5(int n_atom, int n_system, hid_t_compat potential_group_, bool quiet,
                                         const std::function<void(DerivEngine&)>& before_finalize) {
    (void)quiet;
    load_plugins_from_env();
    hid_t potential_group = (hid_t)potential_group_;
    unique_ptr<DerivEngine> engine(new DerivEngine(n_atom, n_system));
    auto& m = node_creation_map();

    map<string, pair<bool, vector<string>>> dep_graph;
    dep_graph["pos"] = make_pair(true, vector<string>());
    for (const auto& name : h5u::node_names_in_group(potential_group))
        dep_graph[name] = make_pair(true, h5u::attr_strings(potential_group, name, "arguments"));
    for (auto& kv : dep_graph)
        for (auto& dep_name : kv.second.second)
            if (dep_graph.find(dep_name) == end(dep_graph))
                throw string("Node ") + kv.first + " takes " + dep_name + " as an argument, but no node of that name can be found.";

    vector<string> topo_order;
    auto in_topo = [&](const string& name) { return find(begin(topo_order), end(topo_order), name) != end(topo_order); };
    int graph_size = dep_graph.size();
    for (int round_num = 0; round_num < graph_size; ++round_num)
        for (auto it = begin(dep_graph); it != end(dep_graph); ++it) {
            if (!it->second.first) continue;
            if (all_of(begin(it->second.second), end(it->second.second), in_topo)) { topo_order.push_back(it->first); it->second.first = false; }
        }
    for (auto& kv : dep_graph) if (kv.second.first) throw string("Unsatisfiable dependency ") + kv.first + " in potential computation";

    for (auto& nm : topo_order) {
        if (nm == "pos") continue;
        string node_type_name = "";
        for (auto& kv : m) if (is_prefix(kv.first, nm)) node_type_name = kv.first;
        if (node_type_name == "") throw string("No node type found for name '") + nm + "'";
        NodeCreationFunction& node_func = m[node_type_name];
        auto argument_names = dep_graph[nm].second;
        ArgList arguments;
        for (const auto& arg_name : argument_names) {
            arguments.push_back(dynamic_cast<CoordNode*>(engine->get(arg_name).computation.get()));
            if (!arguments.back()) throw arg_name + " is not an intermediate value, but it is an argument of " + nm;
        }
        try {
            auto grp = h5u::open_group(potential_group, nm);
            auto computation = unique_ptr<DerivComputation>(node_func(&engine->ctx, (hid_t_compat)(hid_t)grp, arguments));
            engine->add_node(nm, move(computation), argument_names);
        } catch (const string& e) {
            throw "while adding '" + nm + "', " + e;
        }
    }
    if (before_finalize) before_finalize(*engine);
    engine->finalize();
    return engine.release();
}

// ---- replica exchange: one procedure for every swap set (engine.h: Exchange) ---------------------------------------------------
void check_swap_set(int n_system, int n_pair, const int* pairs) {
    if (n_pair < 0 || (n_pair && !pairs)) throw string("invalid swap pairs");
    vector<char> used(n_system, 0);
    for (int i = 0; i < 2 * n_pair; ++i) {
        if (pairs[i] < 0 || pairs[i] >= n_system) throw string("invalid system");
        if (used[pairs[i]]) throw string("Overlapping indices in swap set.");
        used[pairs[i]] = 1;
    }
}
void DerivEngine::sum_potentials_into(float* dev) {
    Exchange& X = exchange;
    if (X.n_node_pot < 0) {
        vector<const float*> ptrs;      // node order: the sum of fetch_potentials
        for (auto& n : nodes) if (n.computation->potential_term) ptrs.push_back(static_cast<PotentialNode*>(n.computation.get())->potential_dev.p);
        X.n_node_pot = (int)ptrs.size(); X.node_pot.upload(ptrs);
    }
    upk_check(upk_sum_potentials(&ctx.L, X.node_pot.p, X.n_node_pot, dev), "sum_potentials");
}
void DerivEngine::begin_attempt(uint64_t round, const float* energies) {
    exchange.round = round; exchange.n_compute = n_compute; exchange.energies = energies; exchange.valid = true;
}
void DerivEngine::require_attempt(uint64_t round, const float* energies) const {
    const Exchange& X = exchange;
    if (!X.valid || X.round != round || X.n_compute != n_compute || X.energies != energies)
        throw string("a later swap set needs the first set of the same attempt (same round, nothing evaluated or moved in between)");
}
const int* DerivEngine::exchange_set(int n_pair, const int* pairs) {
    const int S = ctx.n_system;
    check_swap_set(S, n_pair, pairs);
    Exchange& X = exchange;
    if (!X.e_old.n) { X.e_old.alloc(S); X.e_new.alloc(S); X.draw.alloc(1); }
    vector<float> beta(S);
    for (int s = 0; s < S; ++s) beta[s] = 1.f / temperature[s];
    if (beta != X.beta_host) { sync(); X.beta.upload(beta); X.beta_host = beta; }
    if ((int)X.accepted.n < n_pair + 1) { sync(); X.accepted.alloc(n_pair + 1); }
    if (!n_pair) return nullptr;
    // the device copies of the sets seen so far: a run alternates between a few.  A caller that keeps inventing sets starts over at 64
    const vector<int> key(pairs, pairs + 2 * (size_t)n_pair);
    auto it = X.pairs.find(key);
    if (it == X.pairs.end()) {
        sync();
        if (X.pairs.size() >= 64) X.pairs.clear();
        it = X.pairs.emplace(key, unique_ptr<DevBuf<int>>(new DevBuf<int>())).first;
        it->second->upload(key);
    }
    return it->second->p;
}
void DerivEngine::read_verdicts(int n_pair, int* accepted) {
    if (!accepted) return;
    check_device_errors();
    hip_check(hipMemcpyAsync(accepted, exchange.accepted.p, (size_t)(n_pair + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx.stream), "D2H accepted");
    sync();
}
// One temperature swap set of one Hamiltonian: the first set of an attempt evaluates, a later one finds the energies its
// predecessors left (accepted pairs traded theirs along with their coordinates).  An empty set, here and in hamiltonian_swap, goes
// through the verdict kernel like any other: it only sets or reports the draw counter (zero until a set has written it).
void DerivEngine::replica_swap(int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted, bool first_set) {
    const int* dp = exchange_set(n_pair, pairs);
    Exchange& X = exchange;
    if (first_set) {
        compute(PotentialAndDerivMode);
        sum_potentials_into(X.e_old.p);
        begin_attempt(round, X.e_old.p);
    } else require_attempt(round, X.e_old.p);
    upk_check(upk_exchange_decide(&ctx.L, X.e_old.p, nullptr, X.beta.p, n_pair, dp, base_seed, round, draw0, X.draw.p, X.accepted.p), "exchange_decide");
    upk_check(upk_swap_system_pairs(&ctx.L, pos->coord(), n_pair, dp, X.accepted.p, 1), "swap_system_pairs");
    read_verdicts(n_pair, accepted);
}
// One Hamiltonian swap set (systems of one engine whose parameter values differ): energy pass, the pairs trade coordinates, energy
// pass, verdicts, refused pairs trade back.  Nothing synchronises unless the caller wants the verdicts.
void DerivEngine::hamiltonian_swap(int n_pair, const int* pairs, uint32_t base_seed, uint64_t round, int draw0, int* accepted) {
    if ((int)noise_scale.n != ctx.n_system) throw string("a Hamiltonian swap needs the systems' temperatures: call upside_hip_init_md first");
    const int* dp = exchange_set(n_pair, pairs);
    Exchange& X = exchange;
    if (n_pair) {
        compute(PotentialAndDerivMode);
        sum_potentials_into(X.e_old.p);
        upk_check(upk_swap_system_pairs(&ctx.L, pos->coord(), n_pair, dp, nullptr, 0), "swap_system_pairs");
        compute(PotentialAndDerivMode);
        sum_potentials_into(X.e_new.p);
        invalidate_attempt();      // (e_old no longer holds a temperature attempt's energies)
    }
    upk_check(upk_exchange_decide(&ctx.L, X.e_old.p, X.e_new.p, X.beta.p, n_pair, dp, base_seed, round, draw0, X.draw.p, X.accepted.p), "exchange_decide");
    upk_check(upk_swap_system_pairs(&ctx.L, pos->coord(), n_pair, dp, X.accepted.p, 0), "swap_system_pairs");
    read_verdicts(n_pair, accepted);
}

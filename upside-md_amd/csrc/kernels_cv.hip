// gfx950 kernels of the collective variables: radius of gyration, RMSD after optimal superposition, fraction of native contacts,
// plain distances, torsions and torsional similarity of EVERY system in one launch -- as observables (upside_hip_cv_*, k_collective_variables) and as the
// coordinates of a bias in the force pass (node cv_restraint: k_cv_restraint, an umbrella; node cv_steer: k_cv_steer and
// k_cv_steer_advance, an umbrella whose centre moves while the work is accumulated; node cv_metadynamics: k_cv_metad and
// k_cv_metad_deposit at the end of this file, Gaussian hills deposited during MD).  The value of a CV is computed by cv_device.h for
// all of them, and its gradient for the two biases.
//
// One workgroup of CV_BLOCK lanes owns one system (blockIdx.x) and walks the system's CVs one after the other; a CV is a handful of
// sums over its atom list, read through the engine's position layout ([S][n_atom][stride]).  Nothing here is large: 300 CA atoms
// are 3.6 KB, so the kernel is bound by its launch and by the one read of the positions, and occupancy is no concern (LDS: 4 x
// CV_MAX_SUMS doubles and the frame rows of a path CV, 6 KB; no scratch).  What matters is that the numbers can be trusted:
//   - every sum is accumulated in fp64: the RMSD is sqrt((Ga + Gb - 2 lambda) / n), which cancels to the last bits near the
//     reference; fp32 sums would leave ~3e-4 x Rg where the answer is 0.
//   - every sum has ONE order: lane t adds elements t, t + CV_BLOCK, ... ascending; the 64 lanes of a wavefront combine in a fixed
//     butterfly of DPP / permlane exchanges (the two 32-bit halves of a double travel side by side); the four wavefront totals meet
//     in LDS and every lane adds them 0, 1, 2, 3.  No atomics.  A system's values are therefore bit-identical run to run, whatever
//     the batch size, the system's place in the batch, or the way the launch was issued (eagerly or from a captured graph).
//   - the largest eigenvalue of Horn's 4x4 quaternion matrix comes from cyclic Jacobi rotations in fp64 (one lane; 4x4).
// (The sums, the butterfly and the eigenvalue solver are in cv_device.h.)
// The path kinds (path_s, path_z: K reference frames per CV) have their own device functions in cv_path_device.h: every kernel here
// branches to them on the kind, uniformly over the workgroup, and lends them one LDS row of CV_PATH_ROW doubles per frame
// (UPK_CV_PATH_MAX_FRAMES rows, 5.5 KB; k_cv_metad keeps one such block per CV, 22 KB at D = 4).
// Recording (upk_cv_record) is the same kernel behind a sample decision taken on the device: each system's workgroup advances its
// own round counter (equal entries, like the thermostat's n_invocations) and stores a row on every `every`-th round while the
// buffer has room, so a captured MD graph replays it unchanged.
#include "cv_device.h"
#include "cv_path_device.h"

using namespace up;

#define ST(L) ((hipStream_t)(L)->stream)
static inline int launch_status() { return (int)hipGetLastError(); }

__global__ void __launch_bounds__(CV_BLOCK) k_collective_variables(upk_coord_t pos, upk_cv_t C, upk_cv_record_t R, float* __restrict__ out) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double path[UPK_CV_PATH_MAX_FRAMES][CV_PATH_ROW];
    const int s = blockIdx.x, tid = threadIdx.x;
    float* row;
    if (R.rounds) {       // recording: this system's own counters decide (uniform over the workgroup)
        const unsigned long long r = R.rounds[s] + 1ull;
        const int idx = R.n_attempt[s];
        __syncthreads();
        const bool take = !(r % (unsigned long long)R.every);
        if (tid == 0) { R.rounds[s] = r; if (take) R.n_attempt[s] = idx + 1; }
        if (!take || idx >= R.capacity) return;
        row = R.samples + ((size_t)idx * gridDim.x + s) * C.n_cv;
    } else row = out + (size_t)s * C.n_cv;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;

    for (int c = 0; c < C.n_cv; ++c) {
        double cen[3], rot[9];
        const double value = cv_is_path(C.kind[c]) ? cv_path_evaluate<false>(x, stride, C, c, part, cen, path) : cv_evaluate<false>(x, stride, C, c, part, cen, rot);
        if (tid == 0) row[c] = (float)value;
    }
}

static int cv_launch(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, upk_cv_record_t R, float* out) {
    UPK_FLUSH(L);
    if (C->n_cv < 1 || C->n_cv > UPK_CV_MAX || pos.width < 3) return 9301;
    hipLaunchKernelGGL(k_collective_variables, dim3((unsigned)L->n_system), dim3(CV_BLOCK), 0, ST(L), pos, *C, R, out);
    return launch_status();
}
extern "C" int upk_cv_compute(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, float* out) {
    upk_cv_record_t none{};
    if (!out) return 9302;
    return cv_launch(L, pos, C, none, out);
}
extern "C" int upk_cv_record(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_record_t* R) {
    if (!R->rounds || !R->n_attempt || !R->samples || R->every < 1 || R->capacity < 1) return 9303;
    return cv_launch(L, pos, C, *R, nullptr);
}

// ---- cv_restraint: E = sum_c 1/2 k_c u_c^2, u_c = max(0, |d_c| - flat_width_c), d_c = v_c - center_c, per system ---------------------
// A periodic CV (a dihedral, period 2 pi) takes d_c = cv_wrap(v_c - center_c): the nearest image of the centre, which may be any
// finite number.  The other kinds execute the plain difference.
// The shape of the kernel above: one workgroup per system walks the node's CVs.  Per CV the value v comes from cv_evaluate (the
// bits k_collective_variables reports), lane 0 turns it into dE/dv with this system's row [center | spring_const | flat_width]
// at par + s * par_stride and hands v, dE/dv and (rmsd) the rotation to the other lanes through LDS; a second lane-strided pass
// (cv_write_gradient) writes dE/dv * dv/dx of every list entry, as one fp32 3-vector, into the entry's own slot of the scatter source of pos
// (contrib[s][entry][3]: one writer per slot, every slot written on every launch; the parent gathers in its fixed order, so an
// atom may sit in several CVs and many pairs).  Small values: an rg, rmsd or distance below UPK_CV_RESTRAINT_VMIN, a contact
// pair at r = 0 and a torsion with coincident or collinear atoms have no direction; they contribute zero force (their energy is
// counted).
__global__ void __launch_bounds__(CV_BLOCK) k_cv_restraint(upk_coord_t pos, upk_cv_t C, const float* __restrict__ par, long par_stride,
                                                           float* __restrict__ contrib, long contrib_stride, float* __restrict__ values,
                                                           float* __restrict__ pot_terms) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double bc[2][11];      // v, dE/dv, R; by CV parity (a lane may still read CV c's while lane 0 writes CV c+1's)
    __shared__ double path[UPK_CV_PATH_MAX_FRAMES][CV_PATH_ROW];      // a path CV's frames (its R_k stay here)
    const int s = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;
    const float* __restrict__ row = par + (size_t)s * par_stride;
    float* __restrict__ out = contrib + (size_t)s * contrib_stride;

    for (int c = 0; c < C.n_cv; ++c) {
        double cen[3], rot[9];
        const int kind = C.kind[c];
        const bool is_path = cv_is_path(kind);
        const double value = is_path ? cv_path_evaluate<true>(x, stride, C, c, part, cen, path) : cv_evaluate<true>(x, stride, C, c, part, cen, rot);
        double* b = bc[c & 1];
        if (tid == 0) {
            double d = value - (double)row[c];
            if (cv_periodic(kind)) d = cv_wrap(d);
            const double k = (double)row[C.n_cv + c], w = (double)row[2 * C.n_cv + c];
            const double u = fmax(0., fabs(d) - w);
            b[0] = value; b[1] = d < 0. ? -(k * u) : k * u;
            if (kind == UPK_CV_RMSD) {
#pragma unroll
                for (int i = 0; i < 9; ++i) b[2 + i] = rot[i];
            }
            values[(size_t)s * C.n_cv + c] = (float)value;
            if (pot_terms) pot_terms[(size_t)s * C.n_cv + c] = (float)(0.5 * k * u * u);
        }
        __syncthreads();
        if (is_path) cv_path_write_gradient(x, stride, C, c, b[0], b[1], cen, path, out);
        else cv_write_gradient(x, stride, C, c, b[0], b[1], cen, b + 2, out);
    }
}

extern "C" int upk_cv_restraint(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const float* par, long par_stride, float* contrib,
                                long contrib_stride, float* values, float* pot_terms) {
    UPK_FLUSH(L);
    if (C->n_cv < 1 || C->n_cv > UPK_CV_MAX || pos.width < 3) return 9301;
    if (!par || !contrib || !values) return 9304;
    hipLaunchKernelGGL(k_cv_restraint, dim3((unsigned)L->n_system), dim3(CV_BLOCK), 0, ST(L), pos, *C, par, par_stride, contrib, contrib_stride,
                       values, pot_terms);
    return launch_status();
}

// ---- cv_steer: cv_restraint with a centre that moves on a schedule, and the work that moving it does --------------------------------
// System s has its own clock t_s (completed MD rounds, in device memory) and its own row [center | rate | center_end | spring_const |
// flat_width] at par + s * par_stride (5 n_cv floats).  The centre in force is c_c(t_s) = cv_steer_center(...): fixed over the three
// force passes of a round and switched between rounds, so no kernel argument ever changes and a captured graph replays the pulling.
// k_cv_steer is k_cv_restraint with that centre (d is wrapped for a periodic kind; the centre itself travels on the unwrapped line
// and may wind); it also reports the centres it used.
__global__ void __launch_bounds__(CV_BLOCK) k_cv_steer(upk_coord_t pos, upk_cv_t C, const float* __restrict__ par, long par_stride,
                                                       const unsigned long long* __restrict__ clock, float* __restrict__ contrib, long contrib_stride,
                                                       float* __restrict__ values, float* __restrict__ pot_terms, double* __restrict__ centers) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double bc[2][11];      // v, dE/dv, R; by CV parity (a lane may still read CV c's while lane 0 writes CV c+1's)
    __shared__ double path[UPK_CV_PATH_MAX_FRAMES][CV_PATH_ROW];      // a path CV's frames (its R_k stay here)
    const int s = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;
    const float* __restrict__ row = par + (size_t)s * par_stride;
    float* __restrict__ out = contrib + (size_t)s * contrib_stride;
    const unsigned long long t = tid == 0 ? clock[s] : 0ull;      // (lane 0 alone turns values into forces)

    for (int c = 0; c < C.n_cv; ++c) {
        double cen[3], rot[9];
        const int kind = C.kind[c];
        const bool is_path = cv_is_path(kind);
        const double value = is_path ? cv_path_evaluate<true>(x, stride, C, c, part, cen, path) : cv_evaluate<true>(x, stride, C, c, part, cen, rot);
        double* b = bc[c & 1];
        if (tid == 0) {
            const double centre = cv_steer_center((double)row[c], (double)row[C.n_cv + c], (double)row[2 * C.n_cv + c], t);
            double d = value - centre;
            if (cv_periodic(kind)) d = cv_wrap(d);
            double dEdv, E;
            cv_harmonic_response(d, (double)row[3 * C.n_cv + c], (double)row[4 * C.n_cv + c], dEdv, E);
            b[0] = value; b[1] = dEdv;
            if (kind == UPK_CV_RMSD) {
#pragma unroll
                for (int i = 0; i < 9; ++i) b[2 + i] = rot[i];
            }
            values[(size_t)s * C.n_cv + c] = (float)value;
            centers[(size_t)s * C.n_cv + c] = centre;
            if (pot_terms) pot_terms[(size_t)s * C.n_cv + c] = (float)E;
        }
        __syncthreads();
        if (is_path) cv_path_write_gradient(x, stride, C, c, b[0], b[1], cen, path, out);
        else cv_write_gradient(x, stride, C, c, b[0], b[1], cen, b + 2, out);
    }
}

// One completed MD round: the centre of system s switches from c(t_s) to c(t_s + 1) at the end-of-round positions.  The work of that
// switch is the change of the bias energy at fixed coordinates, summed over the CVs in ascending order, with v_c the bits
// upk_cv_compute reports ((float) of cv_evaluate<false>'s value), so that the accumulated work is a function of the recorded CV
// series alone.  Lane 0 of the system's workgroup owns work[s] and clock[s]: no atomics.  centers receives c(t_s + 1), the centres
// in force from now on.
__global__ void __launch_bounds__(CV_BLOCK) k_cv_steer_advance(upk_coord_t pos, upk_cv_t C, const float* __restrict__ par, long par_stride,
                                                               unsigned long long* __restrict__ clock, double* __restrict__ work, double* __restrict__ centers) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    const int s = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;
    const float* __restrict__ row = par + (size_t)s * par_stride;
    const unsigned long long t = tid == 0 ? clock[s] : 0ull;
    double dw = 0.;
    __shared__ double path[UPK_CV_PATH_MAX_FRAMES][CV_PATH_ROW];

    for (int c = 0; c < C.n_cv; ++c) {
        double cen[3], rot[9];
        const double value = cv_is_path(C.kind[c]) ? cv_path_evaluate<false>(x, stride, C, c, part, cen, path) : cv_evaluate<false>(x, stride, C, c, part, cen, rot);
        if (tid == 0) {
            const double v = (double)(float)value;
            const double c0 = (double)row[c], rate = (double)row[C.n_cv + c], c_end = (double)row[2 * C.n_cv + c];
            const double k = (double)row[3 * C.n_cv + c], w = (double)row[4 * C.n_cv + c];
            const double now = cv_steer_center(c0, rate, c_end, t), next = cv_steer_center(c0, rate, c_end, t + 1ull);
            double d0 = v - now, d1 = v - next;
            if (cv_periodic(C.kind[c])) { d0 = cv_wrap(d0); d1 = cv_wrap(d1); }
            double f0, e0, f1, e1;
            cv_harmonic_response(d0, k, w, f0, e0);
            cv_harmonic_response(d1, k, w, f1, e1);
            dw += e1 - e0;
            centers[(size_t)s * C.n_cv + c] = next;
        }
    }
    if (tid == 0) { work[s] += dw; clock[s] = t + 1ull; }
}

extern "C" int upk_cv_steer(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const float* par, long par_stride, const unsigned long long* clock,
                            float* contrib, long contrib_stride, float* values, float* pot_terms, double* centers) {
    UPK_FLUSH(L);
    if (C->n_cv < 1 || C->n_cv > UPK_CV_MAX || pos.width < 3) return 9301;
    if (!par || !clock || !contrib || !values || !centers || par_stride < 5L * C->n_cv) return 9306;
    hipLaunchKernelGGL(k_cv_steer, dim3((unsigned)L->n_system), dim3(CV_BLOCK), 0, ST(L), pos, *C, par, par_stride, clock, contrib, contrib_stride,
                       values, pot_terms, centers);
    return launch_status();
}
extern "C" int upk_cv_steer_advance(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const float* par, long par_stride, unsigned long long* clock,
                                    double* work, double* centers) {
    UPK_FLUSH(L);
    if (C->n_cv < 1 || C->n_cv > UPK_CV_MAX || pos.width < 3) return 9301;
    if (!par || !clock || !work || !centers || par_stride < 5L * C->n_cv) return 9306;
    hipLaunchKernelGGL(k_cv_steer_advance, dim3((unsigned)L->n_system), dim3(CV_BLOCK), 0, ST(L), pos, *C, par, par_stride, clock, work, centers);
    return launch_status();
}

// ---- cv_metadynamics: V(v) = sum_h w_h exp(-sum_c (v_c - s_hc)^2 / (2 sigma_c^2)) over the node's D CVs, per system ------------------
// The CVs are coupled through the hills, so the kernel cannot go CV by CV as k_cv_restraint does.  Three phases in one workgroup per
// system: (1) all D values by cv_evaluate, kept with centroid and rotation in LDS (13 doubles per CV); (2) the sum over ALL visible
// hills of the system's list -- no cutoff, no grid -- of V and its D partial derivatives in one order (lane t: hills t, t + CV_BLOCK,
// ... ascending, then block_sum<D + 1>); (3) dV/dv_c * dv_c/dx into the list entries' own scatter slots by cv_write_gradient, every
// slot on every launch (zeros while the list is empty).  Hills are stored [list][D + 1][capacity], so consecutive lanes read
// consecutive floats of each row.  In a periodic dimension (a dihedral; periodic[c], uniform over the launch) v_c - s_hc is folded
// by cv_wrap: the nearest image of the hill only, no sum over images -- sigma is expected to be well below pi, where the next
// image's exp(-(2 pi - |d|)^2 / (2 sigma^2)) is nothing.  The other dimensions execute the plain difference.
template <int D>
__device__ __forceinline__ void metad_hill_sum(const float* __restrict__ hills, int capacity, int n_hill, const double (&v)[D], const double (&inv_s2)[D],
                                               const bool (&periodic)[D], double (&acc)[D + 1]) {
#pragma unroll
    for (int k = 0; k <= D; ++k) acc[k] = 0.;
    for (int h = threadIdx.x; h < n_hill; h += CV_BLOCK) {
        double diff[D], e = 0.;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            diff[c] = v[c] - (double)hills[(size_t)c * capacity + h];
            if (periodic[c]) diff[c] = cv_wrap(diff[c]);
            e += diff[c] * diff[c] * inv_s2[c];
        }
        const double g = (double)hills[(size_t)D * capacity + h] * exp(-0.5 * e);
        acc[0] += g;
#pragma unroll
        for (int c = 0; c < D; ++c) acc[1 + c] -= g * diff[c] * inv_s2[c];
    }
}
// where a system's list starts in M.hills (floats) and how many of its hills are visible
__device__ __forceinline__ size_t metad_list(const upk_cv_metad_t& M, int d, int s, int n_system, int n_deposit, int& n_hill) {
    n_hill = M.shared ? n_deposit * n_system : n_deposit;
    return M.shared ? (size_t)0 : (size_t)s * (d + 1) * M.capacity;
}

template <int D>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_metad(upk_coord_t pos, upk_cv_t C, upk_cv_metad_t M, float* __restrict__ contrib, long contrib_stride,
                                                       float* __restrict__ values, float* __restrict__ pot_terms) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double st[D][13];      // per CV: v, centroid, R
    __shared__ double path[D][UPK_CV_PATH_MAX_FRAMES][CV_PATH_ROW];      // per path CV: d_k, R_k and w_k of its frames, kept from phase 1 to phase 3
    const int s = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;
    float* __restrict__ out = contrib + (size_t)s * contrib_stride;

#pragma unroll 1
    for (int c = 0; c < D; ++c) {
        double cen[3], rot[9];
        const bool is_path = cv_is_path(C.kind[c]);
        const double value = is_path ? cv_path_evaluate<true>(x, stride, C, c, part, cen, path[c]) : cv_evaluate<true>(x, stride, C, c, part, cen, rot);
        if (tid == 0) {
            const int kind = C.kind[c];
            st[c][0] = value;
            if (kind == UPK_CV_RG || kind == UPK_CV_RMSD || is_path) { st[c][1] = cen[0]; st[c][2] = cen[1]; st[c][3] = cen[2]; }
            if (kind == UPK_CV_RMSD) {
#pragma unroll
                for (int i = 0; i < 9; ++i) st[c][4 + i] = rot[i];
            }
            values[(size_t)s * D + c] = (float)value;
        }
    }
    __syncthreads();
    double v[D], inv_s2[D], acc[D + 1];
    bool periodic[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { v[c] = st[c][0]; const double sg = (double)M.sigma[c]; inv_s2[c] = 1. / (sg * sg); periodic[c] = cv_periodic(C.kind[c]); }
    int n_hill;
    const float* __restrict__ hills = M.hills + metad_list(M, D, s, (int)gridDim.x, M.n_deposit[s], n_hill);
    metad_hill_sum<D>(hills, M.capacity, n_hill, v, inv_s2, periodic, acc);
    block_sum<D + 1>(acc, part);
    if (tid == 0 && pot_terms) pot_terms[s] = (float)acc[0];
#pragma unroll 1
    for (int c = 0; c < D; ++c) {
        const double cen[3] = {st[c][1], st[c][2], st[c][3]};
        if (cv_is_path(C.kind[c])) cv_path_write_gradient(x, stride, C, c, v[c], acc[1 + c], cen, path[c], out);
        else cv_write_gradient(x, stride, C, c, v[c], acc[1 + c], cen, &st[c][4], out);
    }
}

// One completed MD round (the decision of k_collective_variables' recording, on this node's own counters).  On a pace-th round
// the system counts an attempt and, while the deposit fits, appends a hill: the centre is (float) of cv_evaluate<false>'s value --
// the bits upk_cv_compute reports -- and the weight height, or height * exp(-V(centre) / kdT) with V from metad_hill_sum over the
// hills visible before this launch, evaluated at the stored (rounded) centre so that the weights follow from the stored hills.
// shared: the workgroup of system s reads slots < k * n_system (earlier launches) and writes slot k * n_system + s.
template <int D>
__global__ void __launch_bounds__(CV_BLOCK) k_cv_metad_deposit(upk_coord_t pos, upk_cv_t C, upk_cv_metad_t M) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double st[D];
    __shared__ double path[UPK_CV_PATH_MAX_FRAMES][CV_PATH_ROW];
    const int s = blockIdx.x, tid = threadIdx.x, n_system = (int)gridDim.x;
    const unsigned long long r = M.rounds[s] + 1ull;
    const int k = M.n_deposit[s], na = M.n_attempt[s];
    __syncthreads();
    const bool take = !(r % (unsigned long long)M.pace);
    if (tid == 0) { M.rounds[s] = r; if (take) M.n_attempt[s] = na + 1; }
    const long need = M.shared ? ((long)k + 1) * n_system : (long)k + 1;      // slots in use once this deposit is in
    if (!take || need > (long)M.capacity) return;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;
#pragma unroll 1
    for (int c = 0; c < D; ++c) {
        double cen[3], rot[9];
        const double value = cv_is_path(C.kind[c]) ? cv_path_evaluate<false>(x, stride, C, c, part, cen, path) : cv_evaluate<false>(x, stride, C, c, part, cen, rot);
        if (tid == 0) st[c] = (double)(float)value;
    }
    __syncthreads();
    double v[D], inv_s2[D], acc[D + 1];
    bool periodic[D];
#pragma unroll
    for (int c = 0; c < D; ++c) { v[c] = st[c]; const double sg = (double)M.sigma[c]; inv_s2[c] = 1. / (sg * sg); periodic[c] = cv_periodic(C.kind[c]); }
    int n_hill;
    const size_t list = metad_list(M, D, s, n_system, k, n_hill);
    if (M.kdT > 0.f) {      // (uniform over the workgroup)
        metad_hill_sum<D>(M.hills + list, M.capacity, n_hill, v, inv_s2, periodic, acc);
        block_sum<D + 1>(acc, part);
    } else acc[0] = 0.;
    if (tid == 0) {
        float* mine = M.hills + list + (M.shared ? (size_t)k * n_system + s : (size_t)k);
#pragma unroll
        for (int c = 0; c < D; ++c) mine[(size_t)c * M.capacity] = (float)v[c];
        mine[(size_t)D * M.capacity] = M.kdT > 0.f ? (float)((double)M.height * exp(-acc[0] / (double)M.kdT)) : M.height;
        M.n_deposit[s] = k + 1;
    }
}

static int metad_check(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_metad_t* M) {
    if (C->n_cv < 1 || C->n_cv > UPK_METAD_MAX_DIM || pos.width < 3) return 9301;
    if (!M->hills || !M->n_deposit || !M->n_attempt || !M->rounds || !M->sigma || M->capacity < 1 || M->pace < 1) return 9305;
    return 0;
}
extern "C" int upk_cv_metad(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_metad_t* M, float* contrib, long contrib_stride,
                            float* values, float* pot_terms) {
    UPK_FLUSH(L);
    if (const int rc = metad_check(L, pos, C, M)) return rc;
    if (!contrib || !values) return 9304;
    const dim3 grid((unsigned)L->n_system), block(CV_BLOCK);
    switch (C->n_cv) {
        case 1: hipLaunchKernelGGL(k_cv_metad<1>, grid, block, 0, ST(L), pos, *C, *M, contrib, contrib_stride, values, pot_terms); break;
        case 2: hipLaunchKernelGGL(k_cv_metad<2>, grid, block, 0, ST(L), pos, *C, *M, contrib, contrib_stride, values, pot_terms); break;
        case 3: hipLaunchKernelGGL(k_cv_metad<3>, grid, block, 0, ST(L), pos, *C, *M, contrib, contrib_stride, values, pot_terms); break;
        default: hipLaunchKernelGGL(k_cv_metad<4>, grid, block, 0, ST(L), pos, *C, *M, contrib, contrib_stride, values, pot_terms); break;
    }
    return launch_status();
}
extern "C" int upk_cv_metad_deposit(const upk_launch_t* L, upk_coord_t pos, const upk_cv_t* C, const upk_cv_metad_t* M) {
    UPK_FLUSH(L);
    if (const int rc = metad_check(L, pos, C, M)) return rc;
    const dim3 grid((unsigned)L->n_system), block(CV_BLOCK);
    switch (C->n_cv) {
        case 1: hipLaunchKernelGGL(k_cv_metad_deposit<1>, grid, block, 0, ST(L), pos, *C, *M); break;
        case 2: hipLaunchKernelGGL(k_cv_metad_deposit<2>, grid, block, 0, ST(L), pos, *C, *M); break;
        case 3: hipLaunchKernelGGL(k_cv_metad_deposit<3>, grid, block, 0, ST(L), pos, *C, *M); break;
        default: hipLaunchKernelGGL(k_cv_metad_deposit<4>, grid, block, 0, ST(L), pos, *C, *M); break;
    }
    return launch_status();
}

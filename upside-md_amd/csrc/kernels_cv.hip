// gfx950 kernels of the collective variables: radius of gyration, RMSD after optimal superposition, fraction of native contacts
// and plain distances of EVERY system in one launch -- as observables (upside_hip_cv_*, k_collective_variables) and as the
// coordinates of an umbrella bias in the force pass (node cv_restraint, k_cv_restraint at the end of this file).  The value of a
// CV is computed by cv_device.h for both.
//
// One workgroup of CV_BLOCK lanes owns one system (blockIdx.x) and walks the system's CVs one after the other; a CV is a handful of
// sums over its atom list, read through the engine's position layout ([S][n_atom][stride]).  Nothing here is large: 300 CA atoms
// are 3.6 KB, so the kernel is bound by its launch and by the one read of the positions, and occupancy is no concern (no
// LDS beyond 4 x CV_MAX_SUMS doubles, 104 VGPRs).  What matters is that the numbers can be trusted:
//   - every sum is accumulated in fp64: the RMSD is sqrt((Ga + Gb - 2 lambda) / n), which cancels to the last bits near the
//     reference; fp32 sums would leave ~3e-4 x Rg where the answer is 0.
//   - every sum has ONE order: lane t adds elements t, t + CV_BLOCK, ... ascending; the 64 lanes of a wavefront combine in a fixed
//     butterfly of DPP / permlane exchanges (the two 32-bit halves of a double travel side by side); the four wavefront totals meet
//     in LDS and every lane adds them 0, 1, 2, 3.  No atomics.  A system's values are therefore bit-identical run to run, whatever
//     the batch size, the system's place in the batch, or the way the launch was issued (eagerly or from a captured graph).
//   - the largest eigenvalue of Horn's 4x4 quaternion matrix comes from cyclic Jacobi rotations in fp64 (one lane; 4x4).
// (The sums, the butterfly and the eigenvalue solver are in cv_device.h.)
// Recording (upk_cv_record) is the same kernel behind a sample decision taken on the device: each system's workgroup advances its
// own round counter (equal entries, like the thermostat's n_invocations) and stores a row on every `every`-th round while the
// buffer has room, so a captured MD graph replays it unchanged.
#include "cv_device.h"

using namespace up;

#define ST(L) ((hipStream_t)(L)->stream)
static inline int launch_status() { return (int)hipGetLastError(); }

__global__ void __launch_bounds__(CV_BLOCK) k_collective_variables(upk_coord_t pos, upk_cv_t C, upk_cv_record_t R, float* __restrict__ out) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
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
        const double value = cv_evaluate<false>(x, stride, C, c, part, cen, rot);
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

// ---- cv_restraint: E = sum_c 1/2 k_c u_c^2, u_c = max(0, |v_c - center_c| - flat_width_c), per system ------------------------------
// The shape of the kernel above: one workgroup per system walks the node's CVs.  Per CV the value v comes from cv_evaluate (the
// bits k_collective_variables reports), lane 0 turns it into dE/dv with this system's row [center | spring_const | flat_width]
// at par + s * par_stride and hands v, dE/dv and (rmsd) the rotation to the other lanes through LDS; a second lane-strided pass
// writes dE/dv * dv/dx of every list entry, as one fp32 3-vector, into the entry's own slot of the scatter source of pos
// (contrib[s][entry][3]: one writer per slot, every slot written on every launch; the parent gathers in its fixed order, so an
// atom may sit in several CVs and many pairs).  Small values: an rg, rmsd or distance below UPK_CV_RESTRAINT_VMIN and a contact
// pair at r = 0 have no direction; they contribute zero force (their energy is counted).
__global__ void __launch_bounds__(CV_BLOCK) k_cv_restraint(upk_coord_t pos, upk_cv_t C, const float* __restrict__ par, long par_stride,
                                                           float* __restrict__ contrib, long contrib_stride, float* __restrict__ values,
                                                           float* __restrict__ pot_terms) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double bc[2][11];      // v, dE/dv, R; by CV parity (a lane may still read CV c's while lane 0 writes CV c+1's)
    const int s = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = pos.out + (size_t)s * pos.n_elem * pos.stride;
    const int stride = pos.stride;
    const float* __restrict__ row = par + (size_t)s * par_stride;
    float* __restrict__ out = contrib + (size_t)s * contrib_stride;

    for (int c = 0; c < C.n_cv; ++c) {
        double cen[3], rot[9];
        const double value = cv_evaluate<true>(x, stride, C, c, part, cen, rot);
        const int kind = C.kind[c], a0 = C.atom_start[c], n = C.atom_start[c + 1] - a0;
        double* b = bc[c & 1];
        if (tid == 0) {
            const double d = value - (double)row[c], k = (double)row[C.n_cv + c], w = (double)row[2 * C.n_cv + c];
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
        const double v = b[0], dEdv = b[1];
        const int* __restrict__ atoms = C.atoms + a0;
        float* __restrict__ o = out + (size_t)a0 * 3;
        if (kind == UPK_CV_RG || kind == UPK_CV_RMSD) {
            const double f = v < UPK_CV_RESTRAINT_VMIN ? 0. : dEdv / ((double)n * v);
            if (kind == UPK_CV_RG) {
                for (int i = tid; i < n; i += CV_BLOCK) {
                    double px, py, pz; ld3d(x, atoms[i], stride, px, py, pz);
                    o[3 * i] = (float)(f * (px - cen[0])); o[3 * i + 1] = (float)(f * (py - cen[1])); o[3 * i + 2] = (float)(f * (pz - cen[2]));
                }
            } else {
                const double* __restrict__ ref = C.ref + (size_t)C.aux_start[c] * 3;
                double R[9];
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = b[2 + i];
                for (int i = tid; i < n; i += CV_BLOCK) {
                    double px, py, pz; ld3d(x, atoms[i], stride, px, py, pz);
                    const double bx = ref[3 * i], by = ref[3 * i + 1], bz = ref[3 * i + 2];
                    o[3 * i]     = (float)(f * (px - cen[0] - (R[0] * bx + R[1] * by + R[2] * bz)));
                    o[3 * i + 1] = (float)(f * (py - cen[1] - (R[3] * bx + R[4] * by + R[5] * bz)));
                    o[3 * i + 2] = (float)(f * (pz - cen[2] - (R[6] * bx + R[7] * by + R[8] * bz)));
                }
            }
        } else if (kind == UPK_CV_CONTACTS) {
            const int n_pair = n / 2;
            const float* __restrict__ r0 = C.r0 + C.aux_start[c];
            const double beta = (double)C.beta[c], lambda = (double)C.lambda[c];
            const double f = -dEdv * beta / (double)n_pair;
            for (int i = tid; i < n_pair; i += CV_BLOCK) {
                double ax, ay, az, bx, by, bz;
                ld3d(x, atoms[2 * i], stride, ax, ay, az); ld3d(x, atoms[2 * i + 1], stride, bx, by, bz);
                ax -= bx; ay -= by; az -= bz;
                const double r = sqrt(ax * ax + ay * ay + az * az);
                const double e = exp(-fabs(beta * (r - lambda * (double)r0[i])));      // q (1 - q) = e / (1 + e)^2, either sign of the argument
                const double g = r > 0. ? f * e / ((1. + e) * (1. + e) * r) : 0.;
                const float gx = (float)(g * ax), gy = (float)(g * ay), gz = (float)(g * az);
                o[6 * i] = gx; o[6 * i + 1] = gy; o[6 * i + 2] = gz; o[6 * i + 3] = -gx; o[6 * i + 4] = -gy; o[6 * i + 5] = -gz;
            }
        } else if (tid == 0) {      // UPK_CV_DISTANCE
            double ax, ay, az, bx, by, bz;
            ld3d(x, atoms[0], stride, ax, ay, az); ld3d(x, atoms[1], stride, bx, by, bz);
            const double f = v < UPK_CV_RESTRAINT_VMIN ? 0. : dEdv / v;
            const float gx = (float)(f * (ax - bx)), gy = (float)(f * (ay - by)), gz = (float)(f * (az - bz));
            o[0] = gx; o[1] = gy; o[2] = gz; o[3] = -gx; o[4] = -gy; o[5] = -gz;
        }
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

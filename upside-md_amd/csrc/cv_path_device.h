// Path collective variables (Branduardi, Gervasio & Parrinello 2007): progress s along and distance z from an ordered set of K
// reference frames of one selection of n atoms.  With d_k the minimum mean squared deviation over proper rigid motions between the
// selection and frame k (Angstrom^2: the square of what an rmsd reports), d_min = min_k d_k and w_k = exp(-lambda (d_k - d_min)),
//     path_s = sum_k k w_k / sum_k w_k  (k = 1..K),      path_z = d_min - ln(sum_k w_k) / lambda.
// Included by kernels_cv.hip; the kernels there branch here on the kind (cv_is_path) and never go through the rmsd branch of
// cv_evaluate.  The shape stays one workgroup of CV_BLOCK lanes per system:
//   1. the centroid of the selection by block_sum<3>, as rmsd does;
//   2. wavefront w owns frames w, w + CV_WAVES, ...: its lanes stride the atoms by 64, ascending, accumulate sum |a|^2 and the 3x3
//      correlation sums of the frame in fp64 and combine them by wave_sum64 -- no workgroup barrier per frame; lane 0 of the wavefront
//      leaves the ten sums in the frame's LDS row;
//   3. after one barrier lane k < K builds Horn's matrix of frame k, solves it (jacobi4_max_eigenvalue, cofactor_eigenvector4) and
//      leaves d_k and the rotation R_k in the row: the K eigenproblems run side by side on K lanes;
//   4. lane k < K forms w_k from the exact minimum of d_1..d_K taken in ascending order; every lane then adds the w_k (and k w_k)
//      in ascending order in fp64, so all lanes hold the same bits of s or z.
// The gradient (cv_path_write_gradient) turns the weights into c_k = dE/dv dv/dd_k 2/n in place and lets lanes stride the atoms:
// each list entry sums c_k (a_i - R_k b_ki) over k ascending in fp64 and writes one fp32 3-vector into its own scatter slot.
// No atomics, one order of every sum: a system's values and forces are bit-identical run to run, whatever the batch.
// A frame's LDS row (CV_PATH_ROW doubles) holds, in turn: the ten sums; then d_k, R_k (9) and w_k; then c_k in place of w_k.
#pragma once
#include "cv_device.h"

#define CV_PATH_ROW 11

namespace up {

__device__ __forceinline__ bool cv_is_path(int kind) { return kind == UPK_CV_PATH_S || kind == UPK_CV_PATH_Z; }

// sum_k w_k (and sum_k k w_k, k = 1..K) over the rows of P, ascending: the same bits on every lane
__device__ __forceinline__ void cv_path_weight_sums(const double (*P)[CV_PATH_ROW], int K, double& sw, double& skw) {
    sw = 0.; skw = 0.;
    for (int k = 0; k < K; ++k) { const double w = P[k][10]; sw += w; skw += (double)(k + 1) * w; }
}

// Value of the path CV c (kind path_s or path_z) of the system whose positions start at x.  Called by all lanes of the workgroup;
// the value and the centroid cen are valid on every lane.  Leaves d_k, (WANT_ROT) R_k and w_k of every frame in P[k] for
// cv_path_write_gradient; R_k is the proper rotation taking the centred frame onto the centred selection, row-major as cv_evaluate's.
template <bool WANT_ROT>
__device__ __forceinline__ double cv_path_evaluate(const float* __restrict__ x, int stride, const upk_cv_t& C, int c, double (*part)[CV_MAX_SUMS],
                                                   double (&cen)[3], double (*P)[CV_PATH_ROW]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int a0 = C.atom_start[c], n = C.atom_start[c + 1] - a0, K = min(C.path_n_frame[c], UPK_CV_PATH_MAX_FRAMES);      // (P has that many rows)
    const int* __restrict__ atoms = C.atoms + a0;
    const double* __restrict__ ref = C.ref + (size_t)C.aux_start[c] * 3;      // K frames of n rows, centred on the host
    const double* __restrict__ ref_g = C.path_g + C.path_frame_start[c];
    const double lambda = (double)C.path_lambda[c];
    cen[0] = 0.; cen[1] = 0.; cen[2] = 0.;
    for (int i = tid; i < n; i += CV_BLOCK) { double px, py, pz; ld3d(x, atoms[i], stride, px, py, pz); cen[0] += px; cen[1] += py; cen[2] += pz; }
    block_sum<3>(cen, part);      // (its first barrier also ends every read of P by the CV before this one)
    const double inv_n = 1. / (double)n;
    cen[0] *= inv_n; cen[1] *= inv_n; cen[2] *= inv_n;

    for (int k = wave; k < K; k += CV_WAVES) {      // (uniform over the wavefront)
        const double* __restrict__ frame = ref + (size_t)k * n * 3;
        double m[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};       // Ga, then S[u][v] = sum a_u b_v
        for (int i = lane; i < n; i += 64) {
            double a[3]; ld3d(x, atoms[i], stride, a[0], a[1], a[2]);
            a[0] -= cen[0]; a[1] -= cen[1]; a[2] -= cen[2];
            const double b[3] = {frame[3 * i], frame[3 * i + 1], frame[3 * i + 2]};
            m[0] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int v = 0; v < 3; ++v) m[1 + 3 * u + v] += a[u] * b[v];
        }
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            const double t = wave_sum64(m[j]);
            if (lane == 0) P[k][j] = t;
        }
    }
    __syncthreads();
    if (tid < K) {       // Horn 1987, as cv_evaluate's rmsd: one frame per lane
        double m[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) m[j] = P[tid][j];
        const double Sxx = m[1], Sxy = m[2], Sxz = m[3], Syx = m[4], Syy = m[5], Syz = m[6], Szx = m[7], Szy = m[8], Szz = m[9];
        double H[4][4];
        H[0][0] = Sxx + Syy + Szz; H[0][1] = Syz - Szy; H[0][2] = Szx - Sxz; H[0][3] = Sxy - Syx;
        H[1][1] = Sxx - Syy - Szz; H[1][2] = Sxy + Syx; H[1][3] = Szx + Sxz;
        H[2][2] = -Sxx + Syy - Szz; H[2][3] = Syz + Szy;
        H[3][3] = -Sxx - Syy + Szz;
        double H0[4][4];
        if (WANT_ROT) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = i; j < 4; ++j) H0[i][j] = H0[j][i] = H[i][j];
        }
        const double lam = jacobi4_max_eigenvalue(H);
        P[tid][0] = fmax(0., (m[0] + ref_g[tid] - 2. * lam) * inv_n);
        if (WANT_ROT) {      // H is built from S[u][v] = sum a_u b_v, whose eigenvector is the quaternion of R transposed
            double q[4]; cofactor_eigenvector4(H0, lam, q);
            const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
            P[tid][1] = w * w + qx * qx - qy * qy - qz * qz; P[tid][2] = 2. * (qx * qy + w * qz);           P[tid][3] = 2. * (qx * qz - w * qy);
            P[tid][4] = 2. * (qx * qy - w * qz);           P[tid][5] = w * w - qx * qx + qy * qy - qz * qz; P[tid][6] = 2. * (qy * qz + w * qx);
            P[tid][7] = 2. * (qx * qz + w * qy);           P[tid][8] = 2. * (qy * qz - w * qx);           P[tid][9] = w * w - qx * qx - qy * qy + qz * qz;
        }
    }
    __syncthreads();
    double d_min = P[0][0];
    for (int k = 1; k < K; ++k) d_min = fmin(d_min, P[k][0]);      // exact, so every lane holds the same bits
    if (tid < K) P[tid][10] = exp(-lambda * (P[tid][0] - d_min));      // (1 at the minimum; a far frame underflows to 0)
    __syncthreads();
    double sw, skw;
    cv_path_weight_sums(P, K, sw, skw);
    return C.kind[c] == UPK_CV_PATH_S ? skw / sw : d_min - log(sw) / lambda;
}

// dE/dv * dv/dx of the path CV c, one fp32 3-vector per list entry, into the entry's own slot out[(atom_start[c] + entry) * 3 ..]:
// lane t writes entries t, t + CV_BLOCK, ...  v is the CV's value, cen its centroid and P what cv_path_evaluate<true> left.  With
// p_k = w_k / sum w:  ds/dd_k = -lambda p_k (k - s),  dz/dd_k = p_k,  dd_k/dx_i = (2/n)(a_i - R_k b_ki)  (d_k is smooth at 0 and its
// gradient vanishes there: no small-value rule).  A frame whose coefficient is exactly 0 (an underflowed weight, k = s) is skipped,
// uniformly over the workgroup.  Every slot of the CV is written.  Called by all lanes, after a barrier that follows the evaluation.
__device__ __forceinline__ void cv_path_write_gradient(const float* __restrict__ x, int stride, const upk_cv_t& C, int c, double v, double dEdv,
                                                       const double (&cen)[3], double (*P)[CV_PATH_ROW], float* __restrict__ out) {
    const int tid = threadIdx.x;
    const int a0 = C.atom_start[c], n = C.atom_start[c + 1] - a0, K = min(C.path_n_frame[c], UPK_CV_PATH_MAX_FRAMES);
    const int* __restrict__ atoms = C.atoms + a0;
    const double* __restrict__ ref = C.ref + (size_t)C.aux_start[c] * 3;
    float* __restrict__ o = out + (size_t)a0 * 3;
    double sw, skw;
    cv_path_weight_sums(P, K, sw, skw);
    __syncthreads();      // (every lane has read the weights)
    if (tid < K) {
        const double p = P[tid][10] / sw;
        const double dvdd = C.kind[c] == UPK_CV_PATH_S ? -((double)C.path_lambda[c] * p * ((double)(tid + 1) - v)) : p;
        P[tid][10] = dEdv * dvdd * (2. / (double)n);
    }
    __syncthreads();
    for (int i = tid; i < n; i += CV_BLOCK) {
        double px, py, pz; ld3d(x, atoms[i], stride, px, py, pz);
        px -= cen[0]; py -= cen[1]; pz -= cen[2];
        double gx = 0., gy = 0., gz = 0.;
        for (int k = 0; k < K; ++k) {
            const double ck = P[k][10];
            if (ck == 0.) continue;
            const double* __restrict__ b = ref + ((size_t)k * n + i) * 3;
            const double bx = b[0], by = b[1], bz = b[2];
            const double* R = &P[k][1];
            gx += ck * (px - (R[0] * bx + R[1] * by + R[2] * bz));
            gy += ck * (py - (R[3] * bx + R[4] * by + R[5] * bz));
            gz += ck * (pz - (R[6] * bx + R[7] * by + R[8] * bz));
        }
        o[3 * i] = (float)gx; o[3 * i + 1] = (float)gy; o[3 * i + 2] = (float)gz;
    }
}

}  // namespace up

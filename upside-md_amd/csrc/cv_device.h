// Device code shared by the kernels that evaluate collective variables (kernels_cv.hip: k_collective_variables, k_cv_restraint,
// k_cv_metad, k_cv_metad_deposit, k_cv_steer, k_cv_steer_advance).  All compute a CV by cv_evaluate below, so a bias acts on exactly the number the observable
// reports: the same sums in the same order, bit for bit.  The two biases write their forces by cv_write_gradient.
//   - every sum is accumulated in fp64 and has ONE order: lane t adds elements t, t + CV_BLOCK, ... ascending; the 64 lanes of a
//     wavefront combine in a fixed butterfly of DPP / permlane exchanges (the two 32-bit halves of a double travel side by side);
//     the four wavefront totals meet in LDS and every lane adds them 0, 1, 2, 3.  No atomics.
//   - the largest eigenvalue of Horn's 4x4 quaternion matrix comes from cyclic Jacobi rotations in fp64 (one lane; 4x4); where the
//     gradient is wanted, its eigenvector is read off the cofactors of K - lambda I (the eigenvalue itself is untouched by that).
#pragma once
#include "device_math.h"
#include "../../include/upside_hip_kernels.h"

#define CV_BLOCK 256
#define CV_WAVES (CV_BLOCK / 64)
#define CV_MAX_SUMS 10       // rmsd: Ga + the 3x3 correlation matrix

namespace up {

template <int CTRL>
__device__ __forceinline__ double dpp_mov64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// every lane ends with the sum of all 64, by the butterfly of device_math.h's wave_reduce (each step adds a lane and its partner:
// commutative, so all lanes hold the same bits)
__device__ __forceinline__ double wave_sum64(double v) {
    v += dpp_mov64<UP_DPP_XOR1>(v);
    v += dpp_mov64<UP_DPP_XOR2>(v);
    v += dpp_mov64<UP_DPP_HALF_MIRROR>(v);
    v += dpp_mov64<UP_DPP_ROW_MIRROR>(v);
    {   const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double((int)rh[0], (int)rl[0]) + __hiloint2double((int)rh[1], (int)rl[1]); }
    {   const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = __hiloint2double((int)rh[0], (int)rl[0]) + __hiloint2double((int)rh[1], (int)rl[1]); }
    return v;
}
// v[0..K) summed over the workgroup; every lane receives the totals.  Called by all lanes.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*part)[CV_MAX_SUMS]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();          // (the previous totals have been read)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double w = wave_sum64(v[k]);
        if (lane == 0) part[wave][k] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = part[0][k];
#pragma unroll
        for (int w = 1; w < CV_WAVES; ++w) t += part[w][k];
        v[k] = t;
    }
}

// largest eigenvalue of the symmetric 4x4 matrix a (upper triangle used): cyclic Jacobi, eigenvalues only
__device__ inline double jacobi4_max_eigenvalue(double (&a)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) a[i][j] = a[j][i];
    double scale = 0.;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) scale += a[i][j] * a[i][j];
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[0][3] * a[0][3] + a[1][2] * a[1][2] + a[1][3] * a[1][3] + a[2][3] * a[2][3];
        if (!(off > 1e-40 * scale)) break;       // (also leaves on a NaN)
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.) continue;
                const double theta = (a[q][q] - a[p][p]) / (2. * apq);
                const double t = (theta >= 0. ? 1. : -1.) / (fabs(theta) + sqrt(theta * theta + 1.));
                const double c = 1. / sqrt(t * t + 1.), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {      // A <- A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {      // A <- J^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
            }
    }
    return fmax(fmax(a[0][0], a[1][1]), fmax(a[2][2], a[3][3]));
}

// unit eigenvector of the symmetric 4x4 matrix k (full) at its eigenvalue lam: K - lam I is singular, so every row of its adjugate
// is a multiple of the eigenvector; the row of largest norm is taken (its relative error is eps x |K| / gap to the next eigenvalue,
// the conditioning of the eigenvector itself).  A degenerate eigenvalue (adjugate 0) gives the identity quaternion.
__device__ inline void cofactor_eigenvector4(const double (&k)[4][4], double lam, double (&q)[4]) {
    double m[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[i][j] = k[i][j] - (i == j ? lam : 0.);
    double best = 0.;
    q[0] = 1.; q[1] = 0.; q[2] = 0.; q[3] = 0.;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double row[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {      // cofactor (i, j): the matrix without row i and column j
            const int r0 = 0 + (0 >= i), r1 = 1 + (1 >= i), r2 = 2 + (2 >= i), c0 = 0 + (0 >= j), c1 = 1 + (1 >= j), c2 = 2 + (2 >= j);
            const double d = m[r0][c0] * (m[r1][c1] * m[r2][c2] - m[r1][c2] * m[r2][c1])
                           - m[r0][c1] * (m[r1][c0] * m[r2][c2] - m[r1][c2] * m[r2][c0])
                           + m[r0][c2] * (m[r1][c0] * m[r2][c1] - m[r1][c1] * m[r2][c0]);
            row[j] = ((i + j) & 1) ? -d : d;
        }
        const double n2 = row[0] * row[0] + row[1] * row[1] + row[2] * row[2] + row[3] * row[3];
        if (n2 > best) { best = n2; q[0] = row[0]; q[1] = row[1]; q[2] = row[2]; q[3] = row[3]; }
    }
    if (best > 0.) { const double inv = 1. / sqrt(best); q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv; }
}

__device__ __forceinline__ void ld3d(const float* __restrict__ x, int atom, int stride, double& px, double& py, double& pz) {
    const float* p = x + (size_t)atom * stride;
    px = (double)p[0]; py = (double)p[1]; pz = (double)p[2];
}

// d folded into [-pi, pi]: the difference of two values of a periodic CV (period 2 pi) by its nearest image
#define CV_TWO_PI 6.283185307179586476925286766559
__device__ __forceinline__ double cv_wrap(double d) { return d - CV_TWO_PI * rint(d / CV_TWO_PI); }
__device__ __forceinline__ bool cv_periodic(int kind) { return kind == UPK_CV_DIHEDRAL; }
// the response of a flat-bottomed harmonic restraint to the (wrapped) difference d: u = max(0, |d| - w), dE/dv = +-k u, E = 1/2 k u^2
// (k_cv_steer, k_cv_steer_advance; k_cv_restraint keeps these three lines in its own body: through this function its instructions
// come out in another order)
__device__ __forceinline__ void cv_harmonic_response(double d, double k, double w, double& dEdv, double& E) {
    const double u = fmax(0., fabs(d) - w);
    dEdv = d < 0. ? -(k * u) : k * u;
    E = 0.5 * k * u * u;
}
// the centre of a moving restraint after t completed rounds: center + rate * t in fp64, product and sum rounded separately (what
// IEEE arithmetic on the host gives: no contraction), stopped at center_end on the side rate moves it to
__device__ __forceinline__ double cv_steer_center(double center, double rate, double center_end, unsigned long long t) {
    const double c = __dadd_rn(center, __dmul_rn(rate, (double)t));
    return rate > 0. ? fmin(c, center_end) : (rate < 0. ? fmax(c, center_end) : c);
}

// The torsion of the atoms q[0..4) in the notation of Blondel & Karplus (1996): F = r1 - r2, G = r2 - r3, H = r4 - r3, A = F x G,
// B = H x G, phi = atan2((B x A) . G, (A . B) |G|) in (-pi, pi] -- the sign convention of the reference's backbone torsions, so the
// atoms of a rama_coord row give that node's phi or psi.  A quadruple without a direction gives atan2(0, 0) = 0 (signed zeros are
// cleared first, so that neither -0 nor -pi can come out of a planar arrangement).
struct cv_torsion_t { double F[3], G[3], H[3], A[3], B[3]; };
__device__ __forceinline__ double cv_torsion(const float* __restrict__ x, int stride, const int* __restrict__ q, cv_torsion_t& t) {
    double r1[3], r2[3], r3[3], r4[3];
    ld3d(x, q[0], stride, r1[0], r1[1], r1[2]); ld3d(x, q[1], stride, r2[0], r2[1], r2[2]);
    ld3d(x, q[2], stride, r3[0], r3[1], r3[2]); ld3d(x, q[3], stride, r4[0], r4[1], r4[2]);
#pragma unroll
    for (int d = 0; d < 3; ++d) { t.F[d] = r1[d] - r2[d]; t.G[d] = r2[d] - r3[d]; t.H[d] = r4[d] - r3[d]; }
    t.A[0] = t.F[1] * t.G[2] - t.F[2] * t.G[1]; t.A[1] = t.F[2] * t.G[0] - t.F[0] * t.G[2]; t.A[2] = t.F[0] * t.G[1] - t.F[1] * t.G[0];
    t.B[0] = t.H[1] * t.G[2] - t.H[2] * t.G[1]; t.B[1] = t.H[2] * t.G[0] - t.H[0] * t.G[2]; t.B[2] = t.H[0] * t.G[1] - t.H[1] * t.G[0];
    const double c0 = t.B[1] * t.A[2] - t.B[2] * t.A[1], c1 = t.B[2] * t.A[0] - t.B[0] * t.A[2], c2 = t.B[0] * t.A[1] - t.B[1] * t.A[0];
    const double gmag = sqrt(t.G[0] * t.G[0] + t.G[1] * t.G[1] + t.G[2] * t.G[2]);
    double sn = c0 * t.G[0] + c1 * t.G[1] + c2 * t.G[2], cs = (t.A[0] * t.B[0] + t.A[1] * t.B[1] + t.A[2] * t.B[2]) * gmag;
    if (sn == 0.) sn = 0.;
    if (cs == 0.) cs = 0.;
    return atan2(sn, cs);
}
// f * dphi/dx of the four atoms into o[0..12).  Small values: |G| < UPK_CV_RESTRAINT_VMIN, or three atoms collinear to within 1e-6
// in the sine (|A|^2 not above 1e-12 |F|^2 |G|^2, or |B|^2 not above 1e-12 |H|^2 |G|^2): the torsion has no direction and all twelve
// are zero.
__device__ __forceinline__ void cv_torsion_gradient(const cv_torsion_t& t, double f, float* __restrict__ o) {
    const double F2 = t.F[0] * t.F[0] + t.F[1] * t.F[1] + t.F[2] * t.F[2], G2 = t.G[0] * t.G[0] + t.G[1] * t.G[1] + t.G[2] * t.G[2];
    const double H2 = t.H[0] * t.H[0] + t.H[1] * t.H[1] + t.H[2] * t.H[2];
    const double A2 = t.A[0] * t.A[0] + t.A[1] * t.A[1] + t.A[2] * t.A[2], B2 = t.B[0] * t.B[0] + t.B[1] * t.B[1] + t.B[2] * t.B[2];
    // (written as "not above": coincident end atoms, F = 0 or H = 0, make both sides 0 and have no direction either)
    const bool none = G2 < UPK_CV_RESTRAINT_VMIN * UPK_CV_RESTRAINT_VMIN || !(A2 > 1e-12 * F2 * G2) || !(B2 > 1e-12 * H2 * G2);
    const double gmag = sqrt(G2);
    const double ka = none ? 0. : f * gmag / A2, kb = none ? 0. : f * gmag / B2;                 // dphi/dr1 = -ka A, dphi/dr4 = kb B
    const double ma = none ? 0. : f * (t.F[0] * t.G[0] + t.F[1] * t.G[1] + t.F[2] * t.G[2]) / (A2 * gmag);
    const double mb = none ? 0. : f * (t.H[0] * t.G[0] + t.H[1] * t.G[1] + t.H[2] * t.G[2]) / (B2 * gmag);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double d1 = -ka * t.A[d], d4 = kb * t.B[d], mid = ma * t.A[d] - mb * t.B[d];
        o[d] = (float)d1; o[3 + d] = (float)(mid - d1); o[6 + d] = (float)(-d4 - mid); o[9 + d] = (float)d4;
    }
}

// Value of CV c of the system whose positions start at x.  Called by all lanes of the workgroup; the value is valid on lane 0
// (on every lane for rg, contacts and dihedral_similarity).  cen receives the selection's centroid (rg, rmsd; every lane).
// WANT_ROT: on lane 0 an rmsd also leaves in rot the optimal proper rotation R taking the centred reference onto the centred
// selection (row-major: a_i ~ sum_j rot[3 i + j] b_j).
template <bool WANT_ROT>
__device__ __forceinline__ double cv_evaluate(const float* __restrict__ x, int stride, const upk_cv_t& C, int c, double (*part)[CV_MAX_SUMS],
                                              double (&cen)[3], double (&rot)[9]) {
    const int tid = threadIdx.x;
    const int kind = C.kind[c], a0 = C.atom_start[c], n = C.atom_start[c + 1] - a0;
    const int* __restrict__ atoms = C.atoms + a0;
    double value = 0.;
    if (kind == UPK_CV_RG || kind == UPK_CV_RMSD) {
        cen[0] = 0.; cen[1] = 0.; cen[2] = 0.;
        for (int i = tid; i < n; i += CV_BLOCK) { double px, py, pz; ld3d(x, atoms[i], stride, px, py, pz); cen[0] += px; cen[1] += py; cen[2] += pz; }
        block_sum<3>(cen, part);
        const double inv_n = 1. / (double)n;
        cen[0] *= inv_n; cen[1] *= inv_n; cen[2] *= inv_n;
        if (kind == UPK_CV_RG) {
            double g[1] = {0.};
            for (int i = tid; i < n; i += CV_BLOCK) {
                double px, py, pz; ld3d(x, atoms[i], stride, px, py, pz);
                px -= cen[0]; py -= cen[1]; pz -= cen[2];
                g[0] += px * px + py * py + pz * pz;
            }
            block_sum<1>(g, part);
            value = sqrt(g[0] * inv_n);
        } else {
            const double* __restrict__ ref = C.ref + (size_t)C.aux_start[c] * 3;      // centred on the host
            double m[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};       // Ga, then S[i][j] = sum a_i b_j
            for (int i = tid; i < n; i += CV_BLOCK) {
                double a[3]; ld3d(x, atoms[i], stride, a[0], a[1], a[2]);
                a[0] -= cen[0]; a[1] -= cen[1]; a[2] -= cen[2];
                const double b[3] = {ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]};
                m[0] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
#pragma unroll
                for (int u = 0; u < 3; ++u)
#pragma unroll
                    for (int v = 0; v < 3; ++v) m[1 + 3 * u + v] += a[u] * b[v];
            }
            block_sum<10>(m, part);
            if (tid == 0) {       // Horn 1987: the largest eigenvalue of the quaternion matrix is the best proper rotation's sum a . R b
                const double Sxx = m[1], Sxy = m[2], Sxz = m[3], Syx = m[4], Syy = m[5], Syz = m[6], Szx = m[7], Szy = m[8], Szz = m[9];
                double K[4][4];
                K[0][0] = Sxx + Syy + Szz; K[0][1] = Syz - Szy; K[0][2] = Szx - Sxz; K[0][3] = Sxy - Syx;
                K[1][1] = Sxx - Syy - Szz; K[1][2] = Sxy + Syx; K[1][3] = Szx + Sxz;
                K[2][2] = -Sxx + Syy - Szz; K[2][3] = Syz + Szy;
                K[3][3] = -Sxx - Syy + Szz;
                double K0[4][4];
                if (WANT_ROT) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = i; j < 4; ++j) K0[i][j] = K0[j][i] = K[i][j];
                }
                const double lam = jacobi4_max_eigenvalue(K);
                value = sqrt(fmax(0., (m[0] + C.ref_g[c] - 2. * lam) * inv_n));
                if (WANT_ROT) {      // K is built from S[u][v] = sum a_u b_v, whose eigenvector is the quaternion of R transposed
                    double q[4]; cofactor_eigenvector4(K0, lam, q);
                    const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
                    rot[0] = w * w + qx * qx - qy * qy - qz * qz; rot[1] = 2. * (qx * qy + w * qz);           rot[2] = 2. * (qx * qz - w * qy);
                    rot[3] = 2. * (qx * qy - w * qz);           rot[4] = w * w - qx * qx + qy * qy - qz * qz; rot[5] = 2. * (qy * qz + w * qx);
                    rot[6] = 2. * (qx * qz + w * qy);           rot[7] = 2. * (qy * qz - w * qx);           rot[8] = w * w - qx * qx - qy * qy + qz * qz;
                }
            }
        }
    } else if (kind == UPK_CV_CONTACTS) {
        const int n_pair = n / 2;
        const float* __restrict__ r0 = C.r0 + C.aux_start[c];
        const double beta = (double)C.beta[c], lambda = (double)C.lambda[c];
        double q[1] = {0.};
        for (int i = tid; i < n_pair; i += CV_BLOCK) {
            double ax, ay, az, bx, by, bz;
            ld3d(x, atoms[2 * i], stride, ax, ay, az); ld3d(x, atoms[2 * i + 1], stride, bx, by, bz);
            ax -= bx; ay -= by; az -= bz;
            const double arg = beta * (sqrt(ax * ax + ay * ay + az * az) - lambda * (double)r0[i]);
            // 1 / (1 + exp(arg)) without an overflowing exponential: a pair 1e3 A apart contributes exactly 0
            const double e = exp(-fabs(arg));
            q[0] += (arg > 0. ? e : 1.) / (1. + e);
        }
        block_sum<1>(q, part);
        value = q[0] / (double)n_pair;
    } else if (kind == UPK_CV_DIHEDRAL_SIMILARITY) {
        const int n_quad = n / 4;
        const float* __restrict__ phi0 = C.dihedral_ref + C.aux_start[c];
        double q[1] = {0.};
        for (int i = tid; i < n_quad; i += CV_BLOCK) {
            cv_torsion_t t;
            q[0] += 0.5 * (1. + cos(cv_torsion(x, stride, atoms + 4 * i, t) - (double)phi0[i]));
        }
        block_sum<1>(q, part);
        value = q[0] / (double)n_quad;
    } else if (kind == UPK_CV_DIHEDRAL) {
        if (tid == 0) { cv_torsion_t t; value = cv_torsion(x, stride, atoms, t); }
    } else {      // UPK_CV_DISTANCE
        if (tid == 0) {
            double ax, ay, az, bx, by, bz;
            ld3d(x, atoms[0], stride, ax, ay, az); ld3d(x, atoms[1], stride, bx, by, bz);
            ax -= bx; ay -= by; az -= bz;
            value = sqrt(ax * ax + ay * ay + az * az);
        }
    }
    return value;
}

// dE/dv * dv/dx of CV c, one fp32 3-vector per list entry, into the entry's own slot out[(atom_start[c] + entry) * 3 ..]: lane t
// writes entries t, t + CV_BLOCK, ... (a distance or dihedral: lane 0; a dihedral_similarity: quadruples t, t + CV_BLOCK, ...).
// v is the CV's value, cen the centroid cv_evaluate left (rg, rmsd) and rot nine doubles in LDS holding its rotation (rmsd only;
// read inside that branch).  Small values: an rg, rmsd or distance below
// UPK_CV_RESTRAINT_VMIN, a contact pair at r = 0 and a torsion without a direction (cv_torsion_gradient) receive zero.  Every slot
// of the CV is written.
__device__ __forceinline__ void cv_write_gradient(const float* __restrict__ x, int stride, const upk_cv_t& C, int c, double v, double dEdv,
                                                  const double (&cen)[3], const double* rot, float* __restrict__ out) {
    const int tid = threadIdx.x;
    const int kind = C.kind[c], a0 = C.atom_start[c], n = C.atom_start[c + 1] - a0;
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
            for (int i = 0; i < 9; ++i) R[i] = rot[i];
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
    } else if (kind == UPK_CV_DIHEDRAL_SIMILARITY) {      // dv/dphi_i = -1/2 sin(phi_i - phi0_i) / m, into the quadruple's own 4 slots
        const int n_quad = n / 4;
        const float* __restrict__ phi0 = C.dihedral_ref + C.aux_start[c];
        const double f = -0.5 * dEdv / (double)n_quad;
        for (int i = tid; i < n_quad; i += CV_BLOCK) {
            cv_torsion_t t;
            const double phi = cv_torsion(x, stride, atoms + 4 * i, t);
            cv_torsion_gradient(t, f * sin(phi - (double)phi0[i]), o + 12 * i);
        }
    } else if (kind == UPK_CV_DIHEDRAL) {
        if (tid == 0) { cv_torsion_t t; cv_torsion(x, stride, atoms, t); cv_torsion_gradient(t, dEdv, o); }
    } else if (tid == 0) {      // UPK_CV_DISTANCE
        double ax, ay, az, bx, by, bz;
        ld3d(x, atoms[0], stride, ax, ay, az); ld3d(x, atoms[1], stride, bx, by, bz);
        const double f = v < UPK_CV_RESTRAINT_VMIN ? 0. : dEdv / v;
        const float gx = (float)(f * (ax - bx)), gy = (float)(f * (ay - by)), gz = (float)(f * (az - bz));
        o[0] = gx; o[1] = gy; o[2] = gz; o[3] = -gx; o[4] = -gy; o[5] = -gz;
    }
}

}  // namespace up

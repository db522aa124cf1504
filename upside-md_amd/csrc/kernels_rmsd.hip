// gfx950 kernels and host driver of the pairwise RMSD of frames (upside_hip_frames_create, upside_hip_rmsd_matrix, _nearest, _count;
// include/upside_engine_c.h states the definitions).  For frames a, b with centred coordinates y (fp64) and G_f = sum_i |y_f,i|^2,
//     M_ab[c][d] = sum_i y_a,i[c] y_b,i[d]      d2_ab = max(0, G_a + G_b - 2 lambda_ab) / n
// with lambda_ab the largest eigenvalue of Horn's 4 x 4 matrix of M_ab (the best proper rotation).  The nine entries of M for all pairs
// are the 3 x 3 blocks of one product A A^T, A = the centred coordinates laid out (frame, component) x atom.
//   - k_rmsd_prepare: one wave per frame.  Lane t adds atoms t, t + 64, ... ascending and the lanes meet in wave_sum64's butterfly:
//     the centroid, then y = (double)x - c and G.  y is stored component-major, y[(c * F + f) * n_pad + i], zeros in i = n .. n_pad.
//   - k_rmsd_tile<MODE>: a workgroup (4 waves) owns 64 row frames x 32 column frames; wave w owns rows 16 w .. 16 w + 15 against both
//     16-column blocks: 2 x 9 accumulators of v_mfma_f64_16x16x4_f64 (A = component c of the 16 row frames, B = component d of 16
//     column frames, k = atoms; lane l holds frame l & 15, atom l >> 4 of a k-step; D: column l & 15, row (l >> 4) + 4 reg -- the
//     same for all nine, so a lane ends with the whole 3 x 3 matrices of its 2 x 4 pairs).  The operands go through LDS in chunks of 16
//     atoms (stride 18 doubles per frame: the operand reads of a half-wave touch every bank once -- by the address arithmetic, as in
//     k_mbar_gram_tile).  Positions past the end of a list repeat its last frame and are never written.  After the atoms a lane solves
//     its eight pairs one after the other by the cyclic Jacobi of cv_device.h (no shuffles).  An element is summed by one lane in
//     ascending atom order through one instruction sequence whatever its place in a tile or the rest of the call: its bits depend
//     on the row frame and the column frame alone.
//     MODE matrix: grid over tiles, d written row-major.  Same set and list on both sides: only the tiles that hold a pair p < q, numbered
//     along one grid axis row by row as k_mbar_gram_tile does; the lane that solved (p, q) writes (q, p) too and the diagonal is 0.
//     MODE nearest / count: grid over row tiles; the workgroup walks the column tiles ascending, each lane keeps the running minimum
//     (d2, column) or the count of its four rows, and the 16 lanes of a row meet at the end in a butterfly whose step takes the
//     smaller d2 and on equal bits the lower column: the result does not depend on the order.  No atomics.
// upk_rmsd_frames_create and upk_rmsd_solve are the host sides: every refusal returns before any device call.
#include "mbar_device.h"
#include <chrono>
#include <climits>
#include <new>

using namespace up;
using namespace up::mbar;

#define RMSD_ROWS UPK_RMSD_TILE_ROWS
#define RMSD_COLS UPK_RMSD_TILE_COLS
#define RMSD_CHUNK 16
#define RMSD_STRIDE (RMSD_CHUNK + 2)
#define RMSD_BLOCK 256
#define RMSD_MAX_GRID (1ll << 30)
static_assert(RMSD_ROWS == 64 && RMSD_COLS == 32 && RMSD_BLOCK == 256, "k_rmsd_tile is written for 4 waves of 16 rows x 32 columns");

namespace {

typedef double rmsd_acc_t __attribute__((ext_vector_type(4)));

struct RmsdSide {
    const double* y; const double* g; const int* idx;      // device; idx NULL: position = frame
    long long n_frame, n;                                    // frames of the set; positions of this side
};
struct RmsdArgs {
    RmsdSide A, B;
    int n_atom, n_pad, sym;
    long long ntr, ntc, tile0;
    double cutoff2;
    double* out; long long* index; double* dist; long long* count;
};

__global__ void __launch_bounds__(64) k_rmsd_prepare(const float* __restrict__ pos, long long f0, int n_atom, int n_pad, long long n_frame,
                                                      double* __restrict__ y, double* __restrict__ g) {
    const int lane = threadIdx.x;
    const long long f = f0 + blockIdx.x;
    const float* __restrict__ x = pos + (size_t)blockIdx.x * n_atom * 3;
    double s[3] = {0., 0., 0.};
    for (int i = lane; i < n_atom; i += 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += (double)x[3 * i + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = wave_sum64(s[c]) / (double)n_atom;
    double gg = 0.;
    for (int i = lane; i < n_pad; i += 64) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double v = i < n_atom ? (double)x[3 * i + c] - s[c] : 0.;
            gg += v * v;
            y[((size_t)c * n_frame + f) * n_pad + i] = v;
        }
    }
    gg = wave_sum64(gg);
    if (lane == 0) g[f] = gg;
}

// the frames and the G of the positions first .. first + count of a side (clamped to the side's last position) into LDS
__device__ __forceinline__ void rmsd_stage_side(const RmsdSide& S, long long first, int count, long long* fr, double* gs) {
    const int t = threadIdx.x;
    if (t < count) {
        long long p = first + t;
        if (p > S.n - 1) p = S.n - 1;
        const long long f = S.idx ? (long long)S.idx[p] : p;
        fr[t] = f; gs[t] = S.g[f];
    }
}

template <int MODE>
__global__ void __launch_bounds__(RMSD_BLOCK, 2) k_rmsd_tile(RmsdArgs P) {
    __shared__ double As[3 * RMSD_ROWS * RMSD_STRIDE];
    __shared__ double Bs[3 * RMSD_COLS * RMSD_STRIDE];
    __shared__ long long fa[RMSD_ROWS], fb[RMSD_COLS];
    __shared__ double ga[RMSD_ROWS], gb[RMSD_COLS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const long long bid = P.tile0 + blockIdx.x;
    long long ti, tj0, tj1;
    if (MODE == UPK_RMSD_MATRIX) {
        if (P.sym) {      // row tile ti needs the column tiles 2 ti .. ntc - 1 (those that hold a pair p < q, and the diagonal)
            long long rest = bid; ti = 0;
            while (rest >= P.ntc - 2 * ti) { rest -= P.ntc - 2 * ti; ++ti; }
            tj0 = 2 * ti + rest;
        } else { ti = bid / P.ntc; tj0 = bid - ti * P.ntc; }
        tj1 = tj0 + 1;
    } else { ti = bid; tj0 = 0; tj1 = P.ntc; }
    const int n_pad = P.n_pad;
    const double n_atom = (double)P.n_atom;

    rmsd_stage_side(P.A, ti * RMSD_ROWS, RMSD_ROWS, fa, ga);
    double best_d2[4]; long long best_col[4], cnt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { best_d2[q] = INFINITY; best_col[q] = LLONG_MAX; cnt[q] = 0; }

    for (long long tj = tj0; tj < tj1; ++tj) {
        __syncthreads();      // (the previous tile's epilogue has read gb)
        rmsd_stage_side(P.B, tj * RMSD_COLS, RMSD_COLS, fb, gb);
        rmsd_acc_t acc[2][9];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 9; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[b][e][q] = 0.;

        for (int k0 = 0; k0 < n_pad; k0 += RMSD_CHUNK) {
            __syncthreads();      // (the previous chunk has been read; fa, fb are staged)
#pragma unroll 4
            for (int i = 0; i < 3 * RMSD_ROWS * RMSD_CHUNK / RMSD_BLOCK; ++i) {
                const int e = tid + i * RMSD_BLOCK, r = e & (RMSD_CHUNK - 1), fr = (e / RMSD_CHUNK) & (RMSD_ROWS - 1), c = e / (RMSD_CHUNK * RMSD_ROWS);
                As[(c * RMSD_ROWS + fr) * RMSD_STRIDE + r] = k0 + r < n_pad ? P.A.y[((size_t)c * P.A.n_frame + fa[fr]) * n_pad + k0 + r] : 0.;
            }
#pragma unroll 3
            for (int i = 0; i < 3 * RMSD_COLS * RMSD_CHUNK / RMSD_BLOCK; ++i) {
                const int e = tid + i * RMSD_BLOCK, r = e & (RMSD_CHUNK - 1), fr = (e / RMSD_CHUNK) & (RMSD_COLS - 1), c = e / (RMSD_CHUNK * RMSD_COLS);
                Bs[(c * RMSD_COLS + fr) * RMSD_STRIDE + r] = k0 + r < n_pad ? P.B.y[((size_t)c * P.B.n_frame + fb[fr]) * n_pad + k0 + r] : 0.;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < RMSD_CHUNK; kk += 4) {
                double a[3], b[2][3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    a[c] = As[(c * RMSD_ROWS + wave * 16 + li) * RMSD_STRIDE + kk + lk];
                    b[0][c] = Bs[(c * RMSD_COLS + li) * RMSD_STRIDE + kk + lk];
                    b[1][c] = Bs[(c * RMSD_COLS + 16 + li) * RMSD_STRIDE + kk + lk];
                }
#pragma unroll
                for (int blk = 0; blk < 2; ++blk)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int d = 0; d < 3; ++d)
                            acc[blk][3 * c + d] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c], b[blk][d], acc[blk][3 * c + d], 0, 0, 0);
            }
        }

        // the eight pairs of this lane, one after the other: s = 4 block + reg
#pragma unroll 1
        for (int s = 0; s < 8; ++s) {
            const int blk = s >> 2, q = s & 3;
            const int rl = wave * 16 + lk + 4 * q, cl = blk * 16 + li;
            const long long row = ti * RMSD_ROWS + rl, col = tj * RMSD_COLS + cl;
            if (row >= P.A.n || col >= P.B.n) continue;
            if (MODE == UPK_RMSD_MATRIX && P.sym) {
                if (row > col) continue;
                if (row == col) { P.out[(size_t)row * P.B.n + col] = 0.; continue; }
            }
            double m[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                double v = acc[0][e][0];
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) if (s == 4 * b + qq) v = acc[b][e][qq];
                m[e] = v;
            }
            // Horn 1987: the largest eigenvalue of the quaternion matrix is the best proper rotation's sum a . R b (as in cv_evaluate)
            const double Sxx = m[0], Sxy = m[1], Sxz = m[2], Syx = m[3], Syy = m[4], Syz = m[5], Szx = m[6], Szy = m[7], Szz = m[8];
#ifdef UPK_RMSD_STUB_SOLVE      // (timing builds only: the accumulation without the solve)
            const double lam = Sxx + Syy + Szz;
#else
            double K[4][4];
            K[0][0] = Sxx + Syy + Szz; K[0][1] = Syz - Szy; K[0][2] = Szx - Sxz; K[0][3] = Sxy - Syx;
            K[1][1] = Sxx - Syy - Szz; K[1][2] = Sxy + Syx; K[1][3] = Szx + Sxz;
            K[2][2] = -Sxx + Syy - Szz; K[2][3] = Syz + Szy;
            K[3][3] = -Sxx - Syy + Szz;
            const double lam = jacobi4_max_eigenvalue(K);
#endif
            const double d2 = fmax(0., ga[rl] + gb[cl] - 2. * lam) / n_atom;
            if (MODE == UPK_RMSD_MATRIX) {
                const double d = sqrt(d2);
                P.out[(size_t)row * P.B.n + col] = d;
                if (P.sym) P.out[(size_t)col * P.B.n + row] = d;
            } else if (MODE == UPK_RMSD_NEAREST) {
#pragma unroll
                for (int qq = 0; qq < 4; ++qq)
                    if (q == qq && (d2 < best_d2[qq] || (d2 == best_d2[qq] && col < best_col[qq]))) { best_d2[qq] = d2; best_col[qq] = col; }
            } else {
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) if (q == qq && d2 <= P.cutoff2) ++cnt[qq];
            }
        }
    }

    if (MODE == UPK_RMSD_NEAREST) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double d2 = best_d2[q]; long long col = best_col[q];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const double od = __shfl_xor(d2, off, 16);
                const long long oc = __shfl_xor(col, off, 16);
                if (od < d2 || (od == d2 && oc < col)) { d2 = od; col = oc; }
            }
            const long long row = ti * RMSD_ROWS + wave * 16 + lk + 4 * q;
            if (li == 0 && row < P.A.n) { P.index[row] = col; P.dist[row] = sqrt(d2); }
        }
    } else if (MODE == UPK_RMSD_COUNT) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            long long c = cnt[q];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) c += __shfl_xor(c, off, 16);
            const long long row = ti * RMSD_ROWS + wave * 16 + lk + 4 * q;
            if (li == 0 && row < P.A.n) P.count[row] = c;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
const char* const rmsd_entry[3] = {"rmsd_matrix", "rmsd_nearest", "rmsd_count"};

void rmsd_alloc(DeviceBuffer& b, size_t bytes, const char* who, const char* what) {
    if (hipMalloc(&b.p, bytes ? bytes : 8) != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();      // (the failure is reported here; it must not surface in a later call's launch status)
        MBAR_REFUSE("%s: the device allocation of %zu bytes for %s failed", who, bytes, what);
    }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// every refusal of upside_hip_frames_create; nothing here touches the device
void frames_check(int n_atom, long long n_frame, const float* pos, upk_rmsd_frames_t** frames) {
    if (!frames) MBAR_REFUSE("frames_create: frames (the place the handle is returned in) must be given");
    *frames = nullptr;
    if (!pos) MBAR_REFUSE("frames_create: pos must be given");
    if (n_atom < 3) MBAR_REFUSE("frames_create: n_atom = %d, at least 3 atoms are needed", n_atom);
    if (n_frame < 1) MBAR_REFUSE("frames_create: n_frame = %lld, at least one frame is needed", n_frame);
    if (n_frame > ((1ll << 40) - 1) / (3ll * n_atom)) MBAR_REFUSE("frames_create: n_atom x n_frame x 3 = %d x %lld x 3 is not below 2^40", n_atom, n_frame);
    size_t at = 0;
    if (!all_finite(pos, (size_t)n_frame * n_atom * 3, &at))
        MBAR_REFUSE("frames_create: pos: frame %zu, atom %zu is not finite", at / ((size_t)n_atom * 3), at % ((size_t)n_atom * 3) / 3);
}

void frames_run(int n_atom, long long n_frame, const float* pos, upk_rmsd_frames_t** frames) {
    frames_check(n_atom, n_frame, pos, frames);
    require_device();
    const int n_pad = (n_atom + 3) / 4 * 4;
    Stream st;
    hip_ok(hipStreamCreate(&st.s), "hipStreamCreate");
    DeviceBuffer y, g, stage;
    rmsd_alloc(y, (size_t)3 * n_frame * n_pad * sizeof(double), "frames_create", "the centred coordinates");
    rmsd_alloc(g, (size_t)n_frame * sizeof(double), "frames_create", "G");
    const size_t frame_floats = (size_t)n_atom * 3;
    long long slab = (long long)(((size_t)64 << 20) / (frame_floats * sizeof(float)));      // 64 MB of float32 at a time
    slab = slab < 1 ? 1 : (slab > n_frame ? n_frame : slab);
    rmsd_alloc(stage, (size_t)slab * frame_floats * sizeof(float), "frames_create", "a slab of pos");
    double copy_ms = 0., kernel_ms = 0.;
    for (long long f0 = 0; f0 < n_frame; f0 += slab) {
        const long long nf = n_frame - f0 < slab ? n_frame - f0 : slab;
        auto t0 = std::chrono::steady_clock::now();
        hip_ok(hipMemcpyAsync(stage.p, pos + (size_t)f0 * frame_floats, (size_t)nf * frame_floats * sizeof(float), hipMemcpyHostToDevice, st.s), "copy of pos");
        hip_ok(hipStreamSynchronize(st.s), "copy of pos");
        copy_ms += ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(k_rmsd_prepare, dim3((unsigned)nf), dim3(64), 0, st.s, stage.as<float>(), f0, n_atom, n_pad, n_frame, y.as<double>(), g.as<double>());
        upk_ok(launch_status(), "centring pass");
        hip_ok(hipStreamSynchronize(st.s), "centring pass");
        kernel_ms += ms_since(t0);
    }
    upk_rmsd_frames_t* F = new upk_rmsd_frames_t{};
    F->magic = UPK_RMSD_MAGIC; F->n_atom = n_atom; F->n_pad = n_pad; F->n_frame = n_frame;
    F->y = y.as<double>(); F->g = g.as<double>(); y.p = nullptr; g.p = nullptr;
    F->create_ms[0] = copy_ms; F->create_ms[1] = kernel_ms;
    *frames = F;
}

void side_check(const char* who, const char* name, const char* n_name, const char* i_name, const upk_rmsd_frames_t* S, long long n, const int* idx) {
    if (n < 1) MBAR_REFUSE("%s: %s = %lld, at least one frame is needed", who, n_name, n);
    if (!idx && n != S->n_frame) MBAR_REFUSE("%s: %s = %lld without an index list, the set of %s holds %lld frames", who, n_name, n, name, S->n_frame);
    if (idx)
        for (long long p = 0; p < n; ++p)
            if (idx[p] < 0 || idx[p] >= S->n_frame) MBAR_REFUSE("%s: %s[%lld] = %d is outside the set of %lld frames", who, i_name, p, idx[p], S->n_frame);
}

// every refusal of the three calls; nothing here touches the device
void rmsd_check(const upk_rmsd_problem_t& P) {
    if (P.mode < 0 || P.mode > 2) MBAR_REFUSE("rmsd: mode = %d", P.mode);
    const char* who = rmsd_entry[P.mode];
    if (!P.A) MBAR_REFUSE("%s: A must be given", who);
    if (!P.B) MBAR_REFUSE("%s: B must be given", who);
    if (P.A->magic != UPK_RMSD_MAGIC) MBAR_REFUSE("%s: A is not a live frame set", who);
    if (P.B->magic != UPK_RMSD_MAGIC) MBAR_REFUSE("%s: B is not a live frame set", who);
    if (P.mode == UPK_RMSD_MATRIX && !P.out) MBAR_REFUSE("%s: out must be given", who);
    if (P.mode == UPK_RMSD_NEAREST && !P.index) MBAR_REFUSE("%s: index must be given", who);
    if (P.mode == UPK_RMSD_NEAREST && !P.dist) MBAR_REFUSE("%s: dist must be given", who);
    if (P.mode == UPK_RMSD_COUNT && !P.count) MBAR_REFUSE("%s: count must be given", who);
    if (P.A->n_atom != P.B->n_atom) MBAR_REFUSE("%s: the frames of A hold %d atoms, those of B %d", who, P.A->n_atom, P.B->n_atom);
    side_check(who, "A", "nA", "ia", P.A, P.nA, P.ia);
    side_check(who, "B", "nB", "ib", P.B, P.nB, P.ib);
    if (P.mode == UPK_RMSD_COUNT && (!(P.cutoff >= 0.) || !std::isfinite(P.cutoff))) MBAR_REFUSE("%s: cutoff = %g must be finite and not negative", who, P.cutoff);
    if (P.mode == UPK_RMSD_MATRIX && P.nA > ((1ll << 40) - 1) / P.nB) MBAR_REFUSE("%s: nA x nB = %lld x %lld is not below 2^40", who, P.nA, P.nB);
}

void rmsd_run(const upk_rmsd_problem_t& P) {
    rmsd_check(P);
    const char* who = rmsd_entry[P.mode];
    require_device();
    const auto wall0 = std::chrono::steady_clock::now();
    Stream st;
    hip_ok(hipStreamCreate(&st.s), "hipStreamCreate");
    const size_t nA = (size_t)P.nA, nB = (size_t)P.nB;
    const bool sym = P.mode == UPK_RMSD_MATRIX && P.A == P.B && P.nA == P.nB &&
                     ((!P.ia && !P.ib) || (P.ia && P.ib && (P.ia == P.ib || !memcmp(P.ia, P.ib, nA * sizeof(int)))));
    DeviceBuffer ia, ib, out, index, dist, count;
    if (P.ia) { rmsd_alloc(ia, nA * sizeof(int), who, "ia"); hip_ok(hipMemcpyAsync(ia.p, P.ia, nA * sizeof(int), hipMemcpyHostToDevice, st.s), "copy of ia"); }
    if (P.ib) { rmsd_alloc(ib, nB * sizeof(int), who, "ib"); hip_ok(hipMemcpyAsync(ib.p, P.ib, nB * sizeof(int), hipMemcpyHostToDevice, st.s), "copy of ib"); }
    if (P.mode == UPK_RMSD_MATRIX) rmsd_alloc(out, nA * nB * sizeof(double), who, "the matrix");
    if (P.mode == UPK_RMSD_NEAREST) { rmsd_alloc(index, nA * sizeof(long long), who, "index"); rmsd_alloc(dist, nA * sizeof(double), who, "dist"); }
    if (P.mode == UPK_RMSD_COUNT) rmsd_alloc(count, nA * sizeof(long long), who, "count");

    RmsdArgs K{};
    K.A = RmsdSide{P.A->y, P.A->g, ia.as<int>(), P.A->n_frame, P.nA};
    K.B = RmsdSide{P.B->y, P.B->g, ib.as<int>(), P.B->n_frame, P.nB};
    K.n_atom = P.A->n_atom; K.n_pad = P.A->n_pad; K.sym = sym ? 1 : 0;
    K.ntr = (P.nA + RMSD_ROWS - 1) / RMSD_ROWS; K.ntc = (P.nB + RMSD_COLS - 1) / RMSD_COLS;
    K.cutoff2 = P.cutoff * P.cutoff;
    K.out = out.as<double>(); K.index = index.as<long long>(); K.dist = dist.as<double>(); K.count = count.as<long long>();
    long long n_group = K.ntr;
    if (P.mode == UPK_RMSD_MATRIX) {
        n_group = 0;
        if (sym) for (long long ti = 0; ti < K.ntr; ++ti) n_group += K.ntc - 2 * ti;      // (ntc >= 2 ntr - 1: every term is at least 1)
        else n_group = K.ntr * K.ntc;
    }
    hipEvent_t e0, e1;
    hip_ok(hipEventCreate(&e0), "hipEventCreate"); hip_ok(hipEventCreate(&e1), "hipEventCreate");
    hip_ok(hipEventRecord(e0, st.s), "hipEventRecord");
    for (long long t0 = 0; t0 < n_group; t0 += RMSD_MAX_GRID) {
        const unsigned grid = (unsigned)(n_group - t0 < RMSD_MAX_GRID ? n_group - t0 : RMSD_MAX_GRID);
        K.tile0 = t0;
        if (P.mode == UPK_RMSD_MATRIX) hipLaunchKernelGGL(k_rmsd_tile<UPK_RMSD_MATRIX>, dim3(grid), dim3(RMSD_BLOCK), 0, st.s, K);
        else if (P.mode == UPK_RMSD_NEAREST) hipLaunchKernelGGL(k_rmsd_tile<UPK_RMSD_NEAREST>, dim3(grid), dim3(RMSD_BLOCK), 0, st.s, K);
        else hipLaunchKernelGGL(k_rmsd_tile<UPK_RMSD_COUNT>, dim3(grid), dim3(RMSD_BLOCK), 0, st.s, K);
        const int rc = launch_status();
        if (rc) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); upk_ok(rc, "tile pass"); }
    }
    hipError_t err = hipEventRecord(e1, st.s);
    if (err == hipSuccess && P.mode == UPK_RMSD_MATRIX) err = hipMemcpyAsync(P.out, out.p, nA * nB * sizeof(double), hipMemcpyDeviceToHost, st.s);
    if (err == hipSuccess && P.mode == UPK_RMSD_NEAREST) err = hipMemcpyAsync(P.index, index.p, nA * sizeof(long long), hipMemcpyDeviceToHost, st.s);
    if (err == hipSuccess && P.mode == UPK_RMSD_NEAREST) err = hipMemcpyAsync(P.dist, dist.p, nA * sizeof(double), hipMemcpyDeviceToHost, st.s);
    if (err == hipSuccess && P.mode == UPK_RMSD_COUNT) err = hipMemcpyAsync(P.count, count.p, nA * sizeof(long long), hipMemcpyDeviceToHost, st.s);
    if (err == hipSuccess) err = hipStreamSynchronize(st.s);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    hip_ok(err, "tile pass and copies out");
    if (P.stats) { P.stats[0] = ms; P.stats[1] = ms_since(wall0); P.stats[2] = (double)n_group; }
}

}  // namespace

extern "C" int upk_rmsd_frames_create(int n_atom, long long n_frame, const float* pos, upk_rmsd_frames_t** frames, char* message, int message_len) {
    return guarded_entry("frames_create", message, message_len, [&] { frames_run(n_atom, n_frame, pos, frames); });
}

extern "C" void upk_rmsd_frames_free(upk_rmsd_frames_t* F) {
    if (!F || F->magic != UPK_RMSD_MAGIC) return;
    F->magic = 0;
    if (F->y) (void)hipFree(F->y);
    if (F->g) (void)hipFree(F->g);
    delete F;
}

extern "C" int upk_rmsd_solve(const upk_rmsd_problem_t* P, char* message, int message_len) {
    return guarded_entry(P && P->mode >= 0 && P->mode <= 2 ? rmsd_entry[P->mode] : "rmsd", message, message_len, [&] {
        if (!P) MBAR_REFUSE("rmsd: no problem given");
        rmsd_run(*P);
    });
}

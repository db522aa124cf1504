// gfx950 kernels and host driver of the statistical inefficiency of recorded series (upside_hip_series_inefficiency; Chodera et al. 2007,
// Chodera 2016): for series k and origin t0 = origin[j], with the tail A_n = a[k][t0 + n] of length Tt = length[k] - t0,
//     mu = mean(A),  s2 = mean((A - mu)^2),  C(t) = sum_{n=0}^{Tt-1-t} (A_n - mu)(A_{n+t} - mu) / ((Tt - t) s2),
//     g = max(1, 1 + 2 sum_{t=1}^{t_stop-1} C(t) (1 - t / Tt)),
//     t_stop = the first t with (C(t) <= 0 and t > mintime), or max_lag + 1, or Tt - 1, whichever comes first
// -- pymbar's statistical_inefficiency(fast=False).  Everything is fp64, there are no atomics, and every sum has ONE order.
//
// All origins of a series share one pass over the lagged products.  The series is centred once, d_n = (a_n - a_0) - mean(a - a_0)
// (a_0 is taken off first: a constant series becomes exactly 0 and a series at 1e6 loses nothing), and the time axis is cut at the
// origins into segments and every segment into PIECES of at most UPK_SERIES_PIECE samples.  Per piece and lag t
//     P[piece][t] = sum_{n in piece, n + t < length} d_n d_{n+t}
// and the tail of origin j has S(t) = sum of P[.][t] over the pieces from segment j on, ascending.  With Delta = mu - mean(a) and the
// running sums head(t) = d_{t0} + .. + d_{t0+t-1}, last(t) = d_{L-t} + .. + d_{L-1}, D = Tt Delta:
//     sum_n (d_n - Delta)(d_{n+t} - Delta) = S(t) - Delta ((D - last) + (D - head)) + (Tt - t) Delta^2.
// The cost is n_series x T x lags, not multiplied by n_origin.
//
// Lags are produced in blocks of UPK_SERIES_LAG_BLOCK = 128, ONE LAUNCH PER BLOCK OF LAGS over the series that are not finished (a
// series is finished when every origin has stopped); the host reads the per-series flags back after each block and launches the next
// over the rest.  (A loop inside a resident workgroup would save that read-back of n_series ints per 128 lags, but would hold a
// finished series' workgroups idle beside the few long ones; with one launch per block the grid shrinks with the work.)
//   - k_series_centre: a workgroup per series; lane t adds elements t, t + 256, ... ascending, block_sum of cv_device.h; d in place.
//   - k_series_segment: a workgroup per (segment, series): count, mean and sum of squared deviations from ITS mean, two passes.
//   - k_series_origins: a lane per series walks the segments from the last to the first and merges them (Chan et al.: a sum of
//     non-negative terms, so s2 is exactly 0 for a constant tail and never negative); tails below UPK_SERIES_MIN_TAIL and s2 == 0
//     are answered here.
//   - k_series_lags: a workgroup (4 waves) per (piece, unfinished series) and lag block [tb, tb + 128).  With x counted from the
//     piece's start, U[i][m] = d[x = 16 m + i] (0 past the piece) and V_q[m][j] = d[tb + 16 m + j + 16 q] (0 past the series), entry
//     (i, j) of U V_q belongs to lag tb + 16 q + j - i: nine tiles q = 0 .. 8 of v_mfma_f64_16x16x4_f64 hold the 128 lags completely,
//     lag tb + 16 q + r being the diagonal j - i = r of tile q plus the diagonal j - i = r - 16 of tile q + 1.  Operand layout as in
//     kernels_mbar_gram.hip (A: lane l holds i = l & 15, k = l >> 4; B: j = l & 15, k = l >> 4; D: column l & 15, row (l >> 4) +
//     4 reg), so a k-step of 4 time blocks reads 64 CONSECUTIVE doubles of the staged series for A and for each B: one conflict-free
//     ds_read_b64 per operand, 10 reads for 9 MFMAs -- the loop is bound by the matrix unit, which is why the operands go through
//     LDS (34 KB) and are not re-read from L2.  Wave w takes the w-th quarter of the piece's k-steps ascending; the four waves' tiles
//     are added in LDS in the order 0, 1, 2, 3; lane t < 128 then sums its diagonal over i = 0 .. 15 ascending.
//   - k_series_suffix: S[series][origin][t] = sum of P over the pieces from the origin's segment to the end, ascending.
//   - k_series_finish: a lane per (series, origin) walks the 128 lags ascending, keeps head, last and the sum of g, and stops.
// Nothing depends on n_series or on a series' place: pieces, orders and launches of a series are functions of its own length and of
// the origins alone.
// upk_series_solve is the host side: every refusal returns before any device call.
#include "mbar_device.h"
#include <chrono>

using namespace up;
using namespace up::mbar;

#define SER_BLOCK CV_BLOCK
#define SER_LAGS UPK_SERIES_LAG_BLOCK
#define SER_PIECE UPK_SERIES_PIECE
#define SER_TILES (SER_LAGS / 16 + 1)
#define SER_WINDOW (SER_PIECE + 16 * SER_TILES)
#define SER_RUNNING (-2ll)
static_assert(SER_BLOCK == 256 && SER_LAGS == 128 && SER_PIECE % 256 == 0, "k_series_lags is written for 4 waves, 128 lags and pieces of whole k-steps per wave");

namespace {

typedef double ser_acc_t __attribute__((ext_vector_type(4)));

// what the kernels share: device pointers
struct SeriesDev {
    int n_series, n_origin, mintime;
    long long stride, max_lag;
    const long long* length;      // [n_series]
    const long long* origin;      // [n_origin]
    double* d;                    // [n_series][stride]: the series, centred in place
    double* shift;                // [n_series][2]: a_0, mean(a - a_0)
    double* seg;                  // [n_series][n_origin][2]: mean and sum of squared deviations of a segment
    // per (series, origin)
    double *delta, *s2, *gsum, *head, *last;
    long long* stop;              // SER_RUNNING while lags are still wanted
    double *g, *mean, *variance;
    // pieces
    const long long* piece_start; // [n_piece_total]
    const int* piece_len;         // [n_piece_total]
    const long long* piece_off;   // [n_series + 1]
    const int* seg_first;         // [n_series][n_origin + 1]: the first piece of a segment, counted within the series
    double* P;                    // [n_piece_total][SER_LAGS]
    double* S;                    // [n_series][n_origin][SER_LAGS]
    int* active;                  // [n_series]
};

__device__ __forceinline__ void segment_range(const SeriesDev& V, int k, int j, long long& n0, long long& n1) {
    const long long L = V.length[k];
    n0 = V.origin[j] < L ? V.origin[j] : L;
    n1 = j + 1 < V.n_origin ? (V.origin[j + 1] < L ? V.origin[j + 1] : L) : L;
}

__global__ void __launch_bounds__(SER_BLOCK) k_series_centre(SeriesDev V) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    const int k = blockIdx.x, tid = threadIdx.x;
    const long long L = V.length[k];
    double* __restrict__ d = V.d + (size_t)k * V.stride;
    const double a0 = d[0];
    double s[1] = {0.};
    for (long long n = tid; n < L; n += SER_BLOCK) s[0] += d[n] - a0;
    block_sum<1>(s, part);
    const double m = s[0] / (double)L;
    __syncthreads();      // (every lane has read d[0])
    for (long long n = tid; n < L; n += SER_BLOCK) d[n] = (d[n] - a0) - m;
    if (tid == 0) { V.shift[2 * (size_t)k] = a0; V.shift[2 * (size_t)k + 1] = m; }
}

__global__ void __launch_bounds__(SER_BLOCK) k_series_segment(SeriesDev V) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    const int j = blockIdx.x % V.n_origin, k = blockIdx.x / V.n_origin, tid = threadIdx.x;
    long long n0, n1;
    segment_range(V, k, j, n0, n1);
    const double* __restrict__ d = V.d + (size_t)k * V.stride;
    double s[1] = {0.};
    for (long long n = n0 + tid; n < n1; n += SER_BLOCK) s[0] += d[n];
    block_sum<1>(s, part);
    const double m = n1 > n0 ? s[0] / (double)(n1 - n0) : 0.;
    double q[1] = {0.};
    for (long long n = n0 + tid; n < n1; n += SER_BLOCK) { const double x = d[n] - m; q[0] += x * x; }
    block_sum<1>(q, part);
    if (tid == 0) { double* o = V.seg + ((size_t)k * V.n_origin + j) * 2; o[0] = m; o[1] = q[0]; }
}

__global__ void __launch_bounds__(SER_BLOCK) k_series_origins(SeriesDev V) {
    const int k = blockIdx.x * SER_BLOCK + threadIdx.x;
    if (k >= V.n_series) return;
    long long n_tot = 0; double mean = 0., m2 = 0.;
    bool any = false;
    for (int j = V.n_origin - 1; j >= 0; --j) {
        long long n0, n1;
        segment_range(V, k, j, n0, n1);
        const long long nb = n1 - n0;
        const size_t e = (size_t)k * V.n_origin + j;
        if (nb > 0) {
            const double mb = V.seg[2 * e], qb = V.seg[2 * e + 1];
            if (n_tot == 0) { mean = mb; m2 = qb; }
            else {
                const double dm = mean - mb, n = (double)(n_tot + nb);
                m2 = (qb + m2) + dm * dm * ((double)n_tot * (double)nb / n);
                mean = mb + dm * ((double)n_tot / n);
            }
            n_tot += nb;
        }
        // the tail of origin j: n_tot samples, their mean `mean` (of d) and m2 = sum of squared deviations
        const double s2 = n_tot > 0 ? m2 / (double)n_tot : 0.;
        V.delta[e] = mean; V.s2[e] = s2; V.gsum[e] = 0.; V.head[e] = 0.; V.last[e] = 0.;
        if (V.mean) V.mean[e] = n_tot > 0 ? V.shift[2 * (size_t)k] + (V.shift[2 * (size_t)k + 1] + mean) : 0.;
        if (V.variance) V.variance[e] = s2;
        if (n_tot < UPK_SERIES_MIN_TAIL) { V.g[e] = 0.; V.stop[e] = -1; }
        else if (s2 == 0.) { V.g[e] = 1.; V.stop[e] = 0; }
        else { V.g[e] = 0.; V.stop[e] = SER_RUNNING; any = true; }
    }
    V.active[k] = any ? 1 : 0;
}

// grid: entry of the list of unfinished series x max_piece + piece within the series; tb = the first lag of the block
__global__ void __launch_bounds__(SER_BLOCK) k_series_lags(SeriesDev V, const int* __restrict__ list, int max_piece, long long tb) {
    __shared__ double As[SER_PIECE];
    __shared__ double Bs[SER_WINDOW];
    __shared__ double Ts[SER_TILES * 256];
    const int k = list[blockIdx.x / max_piece];
    const long long p_first = V.piece_off[k], p = p_first + blockIdx.x % max_piece;
    if (p >= V.piece_off[k + 1]) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long L = V.length[k], p0 = V.piece_start[p];
    const int plen = V.piece_len[p];
    double* __restrict__ out = V.P + (size_t)p * SER_LAGS;
    if (p0 + tb >= L) {      // every second factor lies past the end
        if (tid < SER_LAGS) out[tid] = 0.;
        return;
    }
    const double* __restrict__ d = V.d + (size_t)k * V.stride;
    const int n_step = (plen + 63) >> 6;                     // k-steps of 64 samples
    const int per_wave = (n_step + 3) >> 2;
    for (int x = tid; x < n_step * 64; x += SER_BLOCK) As[x] = x < plen ? d[p0 + x] : 0.;
    for (int y = tid; y < n_step * 64 + 16 * SER_TILES; y += SER_BLOCK) { const long long n = p0 + tb + y; Bs[y] = n < L ? d[n] : 0.; }
    __syncthreads();

    ser_acc_t acc[SER_TILES];
#pragma unroll
    for (int q = 0; q < SER_TILES; ++q) acc[q] = ser_acc_t{0., 0., 0., 0.};
    const int s_end = min(n_step, (wave + 1) * per_wave);
    for (int s = wave * per_wave; s < s_end; ++s) {
        const double a = As[64 * s + lane];
#pragma unroll
        for (int q = 0; q < SER_TILES; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[64 * s + lane + 16 * q], acc[q], 0, 0, 0);
    }

    // the four waves' tiles, added in the order 0, 1, 2, 3
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int q = 0; q < SER_TILES; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int at = q * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15);
                    Ts[at] = w ? Ts[at] + acc[q][r] : acc[q][r];
                }
        }
        __syncthreads();
    }
    if (tid < SER_LAGS) {
        const int q = tid >> 4, r = tid & 15;
        double sum = 0.;
#pragma unroll
        for (int i = 0; i < 16; ++i) sum += i + r < 16 ? Ts[q * 256 + i * 16 + i + r] : Ts[(q + 1) * 256 + i * 16 + i + r - 16];
        out[tid] = sum;
    }
}

// grid: entry of the list x n_origin + origin; lane t = lag tb + t
__global__ void __launch_bounds__(SER_LAGS) k_series_suffix(SeriesDev V, const int* __restrict__ list) {
    const int k = list[blockIdx.x / V.n_origin], j = blockIdx.x % V.n_origin, tid = threadIdx.x;
    const size_t e = (size_t)k * V.n_origin + j;
    if (V.stop[e] != SER_RUNNING) return;
    const long long p_first = V.piece_off[k];
    const int n_piece = (int)(V.piece_off[k + 1] - p_first);
    double sum = 0.;
    for (int p = V.seg_first[(size_t)k * (V.n_origin + 1) + j]; p < n_piece; ++p) sum += V.P[(size_t)(p_first + p) * SER_LAGS + tid];
    V.S[e * SER_LAGS + tid] = sum;
}

// a workgroup per entry of the list; lane = origin (strided)
__global__ void __launch_bounds__(SER_BLOCK) k_series_finish(SeriesDev V, const int* __restrict__ list, long long tb) {
    const int k = list[blockIdx.x];
    const long long L = V.length[k];
    const double* __restrict__ d = V.d + (size_t)k * V.stride;
    int running = 0;
    for (int j = threadIdx.x; j < V.n_origin; j += SER_BLOCK) {
        const size_t e = (size_t)k * V.n_origin + j;
        if (V.stop[e] != SER_RUNNING) continue;
        const long long t0 = V.origin[j], Tt = L - t0;
        const long long limit = V.max_lag < Tt - 2 ? V.max_lag : Tt - 2;      // the last lag that is evaluated
        const double delta = V.delta[e], s2 = V.s2[e], D = (double)Tt * delta;
        double gsum = V.gsum[e], head = V.head[e], last = V.last[e];
        long long stop = SER_RUNNING;
        const double* __restrict__ S = V.S + e * SER_LAGS;
        for (long long t = tb > 1 ? tb : 1; t < tb + SER_LAGS; ++t) {
            head += d[t0 + t - 1]; last += d[L - t];
            const double n = (double)(Tt - t);
            const double num = S[t - tb] - delta * ((D - last) + (D - head)) + n * delta * delta;
            const double c = num / (n * s2);
            if (c <= 0. && t > V.mintime) { stop = t; break; }
            gsum += 2. * c * (1. - (double)t / (double)Tt);
            if (t == limit) { stop = limit + 1; break; }
        }
        V.gsum[e] = gsum; V.head[e] = head; V.last[e] = last;
        if (stop != SER_RUNNING) { V.stop[e] = stop; V.g[e] = 1. + gsum > 1. ? 1. + gsum : 1.; }
        else running = 1;
    }
    running = __syncthreads_or(running);
    if (threadIdx.x == 0) V.active[k] = running;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------

// every refusal of upside_hip_series_inefficiency; nothing here touches the device
void series_check(const upk_series_problem_t& P) {
    if (P.n_series < 1) MBAR_REFUSE("series: n_series = %d, at least one series is needed", P.n_series);
    if (P.n_origin < 1) MBAR_REFUSE("series: n_origin = %d, at least one origin is needed", P.n_origin);
    if (P.mintime < 1) MBAR_REFUSE("series: mintime = %d, at least 1 is needed", P.mintime);
    if (P.max_lag < 1) MBAR_REFUSE("series: max_lag = %lld, at least 1 is needed", P.max_lag);
    if (!P.a || !P.length || !P.origin || !P.g || !P.stop_lag) MBAR_REFUSE("series: a, length, origin, g and stop_lag must be given");
    if (P.stride < 1 || P.stride > ((1ll << 40) - 1) / P.n_series)
        MBAR_REFUSE("series: n_series x stride = %d x %lld is not below 2^40 (and stride >= 1)", P.n_series, P.stride);
    for (int j = 0; j < P.n_origin; ++j) {
        if (P.origin[j] < 0) MBAR_REFUSE("series: origin[%d] = %lld is negative", j, P.origin[j]);
        if (j && P.origin[j] <= P.origin[j - 1]) MBAR_REFUSE("series: origin[%d] = %lld does not ascend (origin[%d] = %lld)", j, P.origin[j], j - 1, P.origin[j - 1]);
    }
    for (int k = 0; k < P.n_series; ++k)
        if (P.length[k] < 1 || P.length[k] > P.stride)
            MBAR_REFUSE("series: length[%d] = %lld, a length lies in 1 .. stride = %lld", k, P.length[k], P.stride);
    size_t at = 0;
    for (int k = 0; k < P.n_series; ++k)
        if (!all_finite(P.a + (size_t)k * P.stride, (size_t)P.length[k], &at)) MBAR_REFUSE("series: series %d, entry %zu is not finite", k, at);
}

struct Event {
    hipEvent_t e = nullptr;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

void series_run(const upk_series_problem_t& P) {
    series_check(P);
    require_device();
    const int K = P.n_series, J = P.n_origin;
    const size_t KJ = (size_t)K * J;
    const auto wall0 = std::chrono::steady_clock::now();

    // the pieces: the segments between the origins, cut every UPK_SERIES_PIECE samples from the segment's start
    std::vector<long long> piece_start, piece_off(K + 1, 0);
    std::vector<int> piece_len, seg_first((size_t)K * (J + 1));
    int max_piece = 0;
    for (int k = 0; k < K; ++k) {
        const long long L = P.length[k];
        const size_t first = piece_start.size();
        for (int j = 0; j < J; ++j) {
            seg_first[(size_t)k * (J + 1) + j] = (int)(piece_start.size() - first);
            const long long n0 = P.origin[j] < L ? P.origin[j] : L, n1 = j + 1 < J && P.origin[j + 1] < L ? P.origin[j + 1] : L;
            for (long long n = n0; n < n1; n += SER_PIECE) { piece_start.push_back(n); piece_len.push_back((int)(n1 - n < SER_PIECE ? n1 - n : SER_PIECE)); }
        }
        seg_first[(size_t)k * (J + 1) + J] = (int)(piece_start.size() - first);
        piece_off[k + 1] = (long long)piece_start.size();
        if ((int)(piece_start.size() - first) > max_piece) max_piece = (int)(piece_start.size() - first);
    }
    const size_t n_piece = piece_start.size();
    // one workgroup per (series, origin) and per (series, piece): a launch holds fewer than 2^32 lanes
    if (KJ >= ((size_t)1 << 23) || (size_t)max_piece * K >= ((size_t)1 << 23))
        MBAR_REFUSE("series: n_series x n_origin = %zu and n_series x pieces = %zu must stay below 2^23", KJ, (size_t)max_piece * K);

    Stream st; hip_ok(hipStreamCreate(&st.s), "hipStreamCreate");
    Event ev0, ev1;
    hip_ok(hipEventCreate(&ev0.e), "hipEventCreate"); hip_ok(hipEventCreate(&ev1.e), "hipEventCreate");
    DeviceBuffer length, origin, d, shift, seg, delta, s2, gsum, head, last, stop, g, mean, variance, pstart, plen, poff, sfirst, Pb, Sb, active, list;
    length.upload(st.s, P.length, K * sizeof(long long), "copy of length");
    origin.upload(st.s, P.origin, J * sizeof(long long), "copy of origin");
    d.alloc((size_t)K * P.stride * sizeof(double), "series");
    bool whole = true;
    for (int k = 0; k < K; ++k) whole = whole && P.length[k] == P.stride;
    if (whole) hip_ok(hipMemcpyAsync(d.p, P.a, (size_t)K * P.stride * sizeof(double), hipMemcpyHostToDevice, st.s), "copy of the series");
    else
        for (int k = 0; k < K; ++k)      // (what lies past a series' length is never read, on either side)
            hip_ok(hipMemcpyAsync(d.as<double>() + (size_t)k * P.stride, P.a + (size_t)k * P.stride, (size_t)P.length[k] * sizeof(double), hipMemcpyHostToDevice, st.s), "copy of the series");
    pstart.upload(st.s, piece_start.data(), n_piece * sizeof(long long), "copy of the pieces");
    plen.upload(st.s, piece_len.data(), n_piece * sizeof(int), "copy of the pieces");
    poff.upload(st.s, piece_off.data(), (K + 1) * sizeof(long long), "copy of the pieces");
    sfirst.upload(st.s, seg_first.data(), seg_first.size() * sizeof(int), "copy of the pieces");
    shift.alloc((size_t)K * 2 * sizeof(double), "workspace"); seg.alloc(KJ * 2 * sizeof(double), "workspace");
    for (DeviceBuffer* b : {&delta, &s2, &gsum, &head, &last, &g, &mean, &variance}) b->alloc(KJ * sizeof(double), "workspace");
    stop.alloc(KJ * sizeof(long long), "workspace");
    Pb.alloc(n_piece * SER_LAGS * sizeof(double), "lagged products"); Sb.alloc(KJ * SER_LAGS * sizeof(double), "lagged products");
    active.alloc(K * sizeof(int), "workspace"); list.alloc(K * sizeof(int), "workspace");

    SeriesDev V{};
    V.n_series = K; V.n_origin = J; V.mintime = P.mintime; V.stride = P.stride; V.max_lag = P.max_lag;
    V.length = length.as<long long>(); V.origin = origin.as<long long>(); V.d = d.as<double>(); V.shift = shift.as<double>(); V.seg = seg.as<double>();
    V.delta = delta.as<double>(); V.s2 = s2.as<double>(); V.gsum = gsum.as<double>(); V.head = head.as<double>(); V.last = last.as<double>();
    V.stop = stop.as<long long>(); V.g = g.as<double>(); V.mean = mean.as<double>(); V.variance = variance.as<double>();
    V.piece_start = pstart.as<long long>(); V.piece_len = plen.as<int>(); V.piece_off = poff.as<long long>(); V.seg_first = sfirst.as<int>();
    V.P = Pb.as<double>(); V.S = Sb.as<double>(); V.active = active.as<int>();

    hip_ok(hipEventRecord(ev0.e, st.s), "hipEventRecord");
    hipLaunchKernelGGL(k_series_centre, dim3(K), dim3(SER_BLOCK), 0, st.s, V);
    hipLaunchKernelGGL(k_series_segment, dim3((unsigned)KJ), dim3(SER_BLOCK), 0, st.s, V);
    hipLaunchKernelGGL(k_series_origins, dim3((K + SER_BLOCK - 1) / SER_BLOCK), dim3(SER_BLOCK), 0, st.s, V);
    upk_ok(launch_status(), "centring");

    std::vector<int> act(K), lst(K);
    double n_mfma = 0.; long long n_block = 0, n_series_blocks = 0;
    for (long long tb = 0;; tb += SER_LAGS) {
        hip_ok(hipMemcpyAsync(act.data(), active.p, K * sizeof(int), hipMemcpyDeviceToHost, st.s), "copy of the flags");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
        int n_act = 0;
        for (int k = 0; k < K; ++k) if (act[k]) lst[n_act++] = k;
        if (!n_act) break;
        hip_ok(hipMemcpyAsync(list.p, lst.data(), n_act * sizeof(int), hipMemcpyHostToDevice, st.s), "copy of the list");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");      // (lst is pageable and rewritten by the next block)
        hipLaunchKernelGGL(k_series_lags, dim3((unsigned)((size_t)max_piece * n_act)), dim3(SER_BLOCK), 0, st.s, V, list.as<int>(), max_piece, tb);
        hipLaunchKernelGGL(k_series_suffix, dim3((unsigned)((size_t)J * n_act)), dim3(SER_LAGS), 0, st.s, V, list.as<int>());
        hipLaunchKernelGGL(k_series_finish, dim3(n_act), dim3(SER_BLOCK), 0, st.s, V, list.as<int>(), tb);
        upk_ok(launch_status(), "lag block");
        ++n_block; n_series_blocks += n_act;
        if (P.stats)
            for (int i = 0; i < n_act; ++i)
                for (long long p = piece_off[lst[i]]; p < piece_off[lst[i] + 1]; ++p)
                    if (piece_start[p] + tb < P.length[lst[i]]) n_mfma += (double)((piece_len[p] + 63) / 64) * SER_TILES;
    }
    hip_ok(hipEventRecord(ev1.e, st.s), "hipEventRecord");
    hip_ok(hipMemcpyAsync(P.g, g.p, KJ * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of g");
    hip_ok(hipMemcpyAsync(P.stop_lag, stop.p, KJ * sizeof(long long), hipMemcpyDeviceToHost, st.s), "copy of stop_lag");
    if (P.mean) hip_ok(hipMemcpyAsync(P.mean, mean.p, KJ * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of mean");
    if (P.variance) hip_ok(hipMemcpyAsync(P.variance, variance.p, KJ * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of variance");
    hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");
    if (P.stats) {
        float ms = 0.f;
        hip_ok(hipEventElapsedTime(&ms, ev0.e, ev1.e), "hipEventElapsedTime");
        P.stats[0] = ms;
        P.stats[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        P.stats[2] = (double)n_block; P.stats[3] = (double)n_series_blocks; P.stats[4] = n_mfma;
    }
}

}  // namespace

extern "C" int upk_series_solve(const upk_series_problem_t* P, char* message, int message_len) {
    return guarded_entry("series", message, message_len, [&] {
        if (!P) MBAR_REFUSE("series: no problem given");
        series_run(*P);
    });
}
extern "C" int upk_series_lag_block(void) { return SER_LAGS; }
extern "C" int upk_series_piece(void) { return SER_PIECE; }

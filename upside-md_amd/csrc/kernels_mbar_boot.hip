// gfx950 kernels and host driver of the MBAR bootstrap (upside_hip_mbar_bootstrap): B replicates of one MBAR problem, replicate b
// weighting sample n by an unsigned 16-bit count c_b(n) (a stratified resample: per state of origin the counts add up to N_k), solved
// together.  Per replicate, one self-consistent iteration from f_b is
//     D_b(n)   = logsumexp_{l : N_l > 0} (ln N_l + f_{b,l} - u_l(n))                      k_mbar_boot_denominator
//     f'_{b,k} = -logsumexp_{n : c_b(n) > 0} (ln c_b(n) - u_k(n) - D_b(n)),  every k      k_mbar_boot_free_energy
//     f'_b     = f'_b - f'_{b,0},  delta_b = max_k |f'_{b,k} - f_{b,k}|                    k_mbar_boot_update
// with u_k(n) of kernels_mbar.hip (mbar_energy of mbar_device.h).  The arithmetic is that file's: fp64, every logsumexp takes its exact
// maximum first, no atomics, one order per sum.  The replicates share the samples and the states and nothing else, so they are the
// second axis of every grid:
//   - an array active[] maps blockIdx.y ("slot") to a replicate of the chunk; a replicate that has converged leaves the array, nothing
//     is moved, and its f and a = ln N + f stay as its last iteration left them;
//   - k_mbar_boot_denominator is the pass of k_mbar_denominator (mbar_denominator_body of mbar_device.h) with a[b][.] staged per
//     replicate; it writes D[slot][n];
//   - k_mbar_boot_free_energy is the pass of k_mbar_free_energy (mbar_free_energy_body, with counts): a workgroup owns UPK_MBAR_FE_TILE states of ONE replicate, lane t takes
//     samples t, t + 256, ... ascending, reads c_b(n) (consecutive uint16 of consecutive lanes) and skips c = 0; ln c comes from a table
//     of 65536 doubles that k_mbar_boot_log_counts fills once per call (an fp64 logarithm per sample and pass would cost a quarter of
//     the pass).  The workgroup's maximum first, then the sum, block_sum of cv_device.h.  A tile of replicates per workgroup was not
//     taken: k_mbar_free_energy is VGPR-limited from d = 4 on (profiles/mbar_rate.txt) and the exponentials are not shared;
//   - k_mbar_boot_update subtracts f'_0, writes f, a and delta[slot]: the host reads one array of deltas per iteration, its one
//     synchronisation for the whole batch;
//   - k_mbar_boot_columns: column_boot[b][j] = -logsumexp_{n : c_b(n) > 0} (ln c_b(n) + log_numerator[j][n] - D_b(n)) at the returned
//     f_b, the same reduction; -inf entries are skipped, a column without a contributing sample is +inf.
// No block of any kernel reads what another replicate wrote, every lane's walk is a function of (n_sample, n_state) alone, so the bits
// of a replicate depend neither on B, nor on the other replicates, nor on when they converge, nor on the chunking.
// The workspace D[slot][n] bounds the replicates solved together: upk_mbar_boot_chunk(n_sample, workspace_bytes) of them, each chunk
// run to convergence before the next.  upk_mbar_boot_solve is the host side: every refusal returns before any device call.
// The counts are given by the caller (upside_hip_mbar_bootstrap) or drawn here, chunk by chunk, into the buffer the passes read
// (upside_hip_mbar_bootstrap_drawn; upside_hip_mbar_bootstrap_counts is the draw alone): the circular block bootstrap per state from
// the counter-based Threefry4x32-20, k_mbar_boot_draw for states that fit an LDS tile, k_mbar_boot_draw_scatter and _narrow above,
// with the idle denominators D as their int32 scratch.  Integer atomics only, so the drawn counts are a function of (seed, replicate,
// state, N_k, block length) and a drawn batch returns the bits of the same counts given by the caller.
#include "mbar_device.h"
#include <algorithm>
#include <memory>

using namespace up;
using namespace up::mbar;

#define BOOT_MAX_CHUNK UPK_MBAR_BOOT_MAX_CHUNK
#define BOOT_COUNTS 65536      // the values of a count

namespace {

typedef unsigned short count_t;

__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_log_counts(double* __restrict__ log_count) {
    const int c = blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (c < BOOT_COUNTS) log_count[c] = c ? log((double)c) : -INFINITY;
}

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_denominator(upk_mbar_states_t S, upk_mbar_samples_t X, const double* __restrict__ a_all,
                                                                       const int* __restrict__ active, double* __restrict__ denom_all) {
    mbar_denominator_body<D>(S, X, a_all + (size_t)active[blockIdx.y] * S.n_state, denom_all + (size_t)blockIdx.y * X.n);
}

template <int D>
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_free_energy(upk_mbar_states_t S, upk_mbar_samples_t X, const count_t* __restrict__ counts_all,
                                                                       const double* __restrict__ log_count, const int* __restrict__ active,
                                                                       const double* __restrict__ denom_all, double* __restrict__ f_new) {
    mbar_free_energy_body<D, true>(S, X, counts_all + (size_t)active[blockIdx.y] * X.n, log_count, denom_all + (size_t)blockIdx.y * X.n,
                                   f_new + (size_t)blockIdx.y * S.n_state);
}

// one workgroup per active replicate: f = f' - f'_0, a = ln N + f, delta[slot] = max_k |f'_k - f_k| (a NaN is kept)
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_update(int n_state, const double* __restrict__ ln_n, const int* __restrict__ active,
                                                                  const double* __restrict__ f_new, double* __restrict__ f_all, double* __restrict__ a_all,
                                                                  double* __restrict__ delta) {
    __shared__ double part[MBAR_BLOCK];
    __shared__ int bad[MBAR_BLOCK];
    const int tid = threadIdx.x;
    const double* __restrict__ fn = f_new + (size_t)blockIdx.x * n_state;
    double* __restrict__ f = f_all + (size_t)active[blockIdx.x] * n_state;
    double* __restrict__ a = a_all + (size_t)active[blockIdx.x] * n_state;
    const double f0 = fn[0];
    double mx = 0.; int nan_seen = 0;
    for (int k = tid; k < n_state; k += MBAR_BLOCK) {
        const double x = fn[k] - f0, dk = fabs(x - f[k]);
        if (dk != dk) nan_seen = 1; else mx = fmax(mx, dk);
        f[k] = x;
        a[k] = ln_n[k] + x;      // (ln N = -inf where N = 0)
    }
    part[tid] = mx; bad[tid] = nan_seen;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < MBAR_BLOCK; ++i) { mx = fmax(mx, part[i]); nan_seen |= bad[i]; }
        delta[blockIdx.x] = nan_seen ? NAN : mx;
    }
}

// grid (column, slot): slot = blockIdx.y is replicate active[slot], with its denominators in D[slot]
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_columns(long long n_sample, const count_t* __restrict__ counts_all, const double* __restrict__ log_count,
                                                                   const int* __restrict__ active, const double* __restrict__ denom_all, int n_column,
                                                                   const double* __restrict__ log_numerator, double* __restrict__ column) {
    __shared__ double part[CV_WAVES][CV_MAX_SUMS];
    __shared__ double partm[CV_WAVES][MBAR_FE];
    const int tid = threadIdx.x, j = blockIdx.x, b = active[blockIdx.y];
    const count_t* __restrict__ counts = counts_all + (size_t)b * n_sample;
    const double* __restrict__ denom = denom_all + (size_t)blockIdx.y * n_sample;
    const double* __restrict__ ln = log_numerator + (size_t)j * n_sample;
    double m[1] = {-INFINITY}, s[1] = {0.};
    for (long long n = tid; n < n_sample; n += MBAR_BLOCK) {
        const int c = counts[n];
        const double x = ln[n];
        if (!c || x == -INFINITY) continue;
        m[0] = fmax(m[0], log_count[c] + (x - denom[n]));
    }
    mbar_block_max<1>(m, partm);
    if (m[0] != -INFINITY)      // (uniform: every lane holds the workgroup's maximum)
        for (long long n = tid; n < n_sample; n += MBAR_BLOCK) {
            const int c = counts[n];
            const double x = ln[n];
            if (!c || x == -INFINITY) continue;
            s[0] += exp(log_count[c] + (x - denom[n]) - m[0]);
        }
    block_sum<1>(s, part);
    if (tid == 0) column[(size_t)b * n_column + j] = m[0] == -INFINITY ? INFINITY : -(m[0] + log(s[0]));
}

inline bool boot_args_ok(const int* active, int n_active) { return active && n_active >= 1 && n_active <= BOOT_MAX_CHUNK; }

// ---- the draw of the counts (include/upside_engine_c.h states it): per replicate b and state k of m samples with block length L, step
// p = j L + t of the state's walk (block j, offset t; p = 0 .. m - 1) covers position (s_j + t) mod m, s_j = floor(r_j m / 2^64).  One lane
// per step, +1 per covered position by an INTEGER atomic (no order in the sum, so the bits are the definition's); a lane regenerates
// the r_j of its block (one Threefry block per step, m per state and replicate: nothing is staged, nothing depends on another lane).
#define DRAW_TILE UPK_MBAR_BOOT_DRAW_TILE
static_assert(DRAW_TILE < BOOT_COUNTS, "a state counted in LDS cannot reach a count of 65536");
static_assert(DRAW_TILE * sizeof(int) <= 32768, "the LDS tile of k_mbar_boot_draw leaves room for five workgroups per CU");

__device__ __forceinline__ int draw_position(unsigned long long seed, unsigned b, int k, int p, int m, int L) {
    const int j = p / L, t = p - j * L;
    const uint32_t key[4] = {(uint32_t)seed, (uint32_t)(seed >> 32), UPK_MBAR_BOOT_DRAW_KEY, 0u};
    uint32_t X[4] = {(uint32_t)(j >> 1), 0u, (uint32_t)k, b};      // (q = j >> 1 < 2^31: its high word is 0)
    threefry4x32_20(X, key);
    const unsigned long long r = (j & 1) ? ((unsigned long long)X[3] << 32 | X[2]) : ((unsigned long long)X[1] << 32 | X[0]);
    const unsigned long long s = __umul64hi(r, (unsigned long long)m) + (unsigned long long)t;      // s_j < m and t < L <= m
    return (int)(s >= (unsigned long long)m ? s - (unsigned long long)m : s);
}
// the state of position p of the grouped order: the largest k with start[k] <= p (states without samples are passed over)
__device__ __forceinline__ int draw_state_of(const int* __restrict__ start, int n_state, int p) {
    int lo = 0, hi = n_state - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (start[mid] <= p) lo = mid; else hi = mid - 1; }
    return lo;
}
__device__ __forceinline__ int draw_block_length(const int* __restrict__ length, int k, int m) { return min(max(length[k], 1), m); }

// grid (state, slot): a state of at most DRAW_TILE samples, counted in LDS and stored once; the other states are left to the two kernels below
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_draw(long long n_sample, const int* __restrict__ start, const int* __restrict__ length,
                                                                const int* __restrict__ order, unsigned first, unsigned long long seed,
                                                                count_t* __restrict__ counts_all) {
    __shared__ int cover[DRAW_TILE];
    const int tid = threadIdx.x, k = blockIdx.x, s0 = start[k], m = start[k + 1] - s0;
    if (m < 1 || m > DRAW_TILE) return;      // (uniform)
    const int L = draw_block_length(length, k, m);
    const unsigned b = first + blockIdx.y;
    for (int p = tid; p < m; p += MBAR_BLOCK) cover[p] = 0;
    __syncthreads();
    for (int p = tid; p < m; p += MBAR_BLOCK) atomicAdd(&cover[draw_position(seed, b, k, p, m, L)], 1);
    __syncthreads();
    count_t* __restrict__ counts = counts_all + (size_t)blockIdx.y * n_sample;
    for (int p = tid; p < m; p += MBAR_BLOCK) counts[order ? order[s0 + p] : s0 + p] = (count_t)cover[p];
}
// grid (blocks of positions, slot): the states above DRAW_TILE samples, +1 into scratch[slot][position] (zeroed before)
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_draw_scatter(int n_state, long long n_sample, const int* __restrict__ start,
                                                                        const int* __restrict__ length, unsigned first, unsigned long long seed,
                                                                        int* __restrict__ scratch) {
    const long long p = (long long)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (p >= n_sample) return;
    const int k = draw_state_of(start, n_state, (int)p), s0 = start[k], m = start[k + 1] - s0;
    if (m <= DRAW_TILE) return;
    const int at = draw_position(seed, first + blockIdx.y, k, (int)p - s0, m, draw_block_length(length, k, m));
    atomicAdd(scratch + (size_t)blockIdx.y * n_sample + s0 + at, 1);
}
// the same grid: scratch narrowed to a count and stored; a count above 65535 is stored as 65535 and reported in *flag
__global__ void __launch_bounds__(MBAR_BLOCK) k_mbar_boot_draw_narrow(int n_state, long long n_sample, const int* __restrict__ start,
                                                                       const int* __restrict__ order, unsigned first, const int* __restrict__ scratch,
                                                                       count_t* __restrict__ counts_all, unsigned long long* __restrict__ flag) {
    const long long p = (long long)blockIdx.x * MBAR_BLOCK + threadIdx.x;
    if (p >= n_sample) return;
    const int k = draw_state_of(start, n_state, (int)p);
    if (start[k + 1] - start[k] <= DRAW_TILE) return;
    int c = scratch[(size_t)blockIdx.y * n_sample + p];
    if (c >= BOOT_COUNTS) { atomicMin(flag, (unsigned long long)(first + blockIdx.y) << 32 | (unsigned)k); c = BOOT_COUNTS - 1; }
    counts_all[(size_t)blockIdx.y * n_sample + (order ? order[p] : p)] = (count_t)c;
}

}  // namespace

extern "C" long long upk_mbar_boot_chunk(long long n_sample, size_t workspace_bytes) {
    if (n_sample < 1) return 0;
    const unsigned long long fit = (unsigned long long)workspace_bytes / sizeof(double) / (unsigned long long)n_sample;
    return (long long)(fit < BOOT_MAX_CHUNK ? fit : BOOT_MAX_CHUNK);
}
extern "C" int upk_mbar_boot_log_counts(void* stream, double* log_count) {
    if (!log_count) return 9410;
    hipLaunchKernelGGL(k_mbar_boot_log_counts, dim3(BOOT_COUNTS / MBAR_BLOCK), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, log_count);
    return launch_status();
}
extern "C" int upk_mbar_boot_denominator(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const double* a, const int* active,
                                         int n_active, double* denom) {
    if (!launch_args_ok(S, X) || !boot_args_ok(active, n_active) || !a || !denom) return 9411;
    MBAR_DISPATCH(k_mbar_boot_denominator, dim3(sample_blocks(X->n), (unsigned)n_active), *S, *X, a, active, denom)
    return launch_status();
}
extern "C" int upk_mbar_boot_free_energy(void* stream, const upk_mbar_states_t* S, const upk_mbar_samples_t* X, const unsigned short* counts,
                                         const double* log_count, const int* active, int n_active, const double* denom, double* f_new) {
    if (!launch_args_ok(S, X) || !boot_args_ok(active, n_active) || !counts || !log_count || !denom || !f_new) return 9412;
    MBAR_DISPATCH(k_mbar_boot_free_energy, dim3((unsigned)((S->n_state + MBAR_FE - 1) / MBAR_FE), (unsigned)n_active), *S, *X, counts, log_count, active,
                  denom, f_new)
    return launch_status();
}
extern "C" int upk_mbar_boot_update(void* stream, int n_state, const double* ln_n, const int* active, int n_active, const double* f_new, double* f,
                                    double* a, double* delta) {
    if (n_state < 1 || !boot_args_ok(active, n_active) || !ln_n || !f_new || !f || !a || !delta) return 9413;
    hipLaunchKernelGGL(k_mbar_boot_update, dim3((unsigned)n_active), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, n_state, ln_n, active, f_new, f, a, delta);
    return launch_status();
}
extern "C" int upk_mbar_boot_columns(void* stream, long long n_sample, const unsigned short* counts, const double* log_count, const int* active,
                                     int n_active, const double* denom, int n_column, const double* log_numerator, double* column) {
    if (n_sample < 1 || !boot_args_ok(active, n_active) || !counts || !log_count || !denom || n_column < 1 || !log_numerator || !column) return 9414;
    hipLaunchKernelGGL(k_mbar_boot_columns, dim3((unsigned)n_column, (unsigned)n_active), dim3(MBAR_BLOCK), 0, (hipStream_t)stream, n_sample, counts,
                       log_count, active, denom, n_column, log_numerator, column);
    return launch_status();
}
extern "C" int upk_mbar_boot_draw(void* stream, int n_state, long long n_sample, const int* start, const int* length, const int* order, int n_replicate,
                                  unsigned int first_replicate, unsigned long long seed, long long largest_state, int* scratch, unsigned short* counts,
                                  unsigned long long* flag) {
    const bool large = largest_state > DRAW_TILE;
    if (n_state < 1 || n_sample < 1 || n_sample > 0x7fffffffll || !start || !length || n_replicate < 1 || n_replicate > BOOT_MAX_CHUNK ||
        (unsigned long long)first_replicate + (unsigned long long)n_replicate > (1ull << 32) || !counts || (large && (!scratch || !flag)))
        return 9415;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mbar_boot_draw, dim3((unsigned)n_state, (unsigned)n_replicate), dim3(MBAR_BLOCK), 0, s, n_sample, start, length, order,
                       first_replicate, seed, counts);
    if (large) {
        const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)n_replicate * (size_t)n_sample * sizeof(int), s);
        if (e != hipSuccess) return (int)e;
        const dim3 grid(sample_blocks(n_sample), (unsigned)n_replicate);
        hipLaunchKernelGGL(k_mbar_boot_draw_scatter, grid, dim3(MBAR_BLOCK), 0, s, n_state, n_sample, start, length, first_replicate, seed, scratch);
        hipLaunchKernelGGL(k_mbar_boot_draw_narrow, grid, dim3(MBAR_BLOCK), 0, s, n_state, n_sample, start, order, first_replicate, scratch, counts, flag);
    }
    return launch_status();
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
namespace {

struct PinnedBuffer {
    void* p = nullptr;
    ~PinnedBuffer() { if (p) (void)hipHostFree(p); }
    void alloc(size_t bytes, const char* what) { hip_ok(hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault), what); }
    template <class T> T* as() const { return (T*)p; }
};

// the refusals about state_of_sample (checked n_k, K states, N samples), for every entry that takes one
void origins_check(const char* who, int K, const long long* n_k, size_t N, const int* state_of_sample) {
    std::vector<long long> have((size_t)K, 0);
    for (size_t n = 0; n < N; ++n) {
        const int k = state_of_sample[n];
        if (k < 0 || k >= K) MBAR_REFUSE("%s: state_of_sample[%zu] = %d is outside 0 .. %d", who, n, k, K - 1);
        if (n_k[k] == 0) MBAR_REFUSE("%s: state_of_sample[%zu] = %d names a state without samples (n_k[%d] = 0)", who, n, k, k);
        ++have[(size_t)k];
    }
    for (int k = 0; k < K; ++k)
        if (have[(size_t)k] != n_k[k])
            MBAR_REFUSE("%s: state_of_sample names state %d for %lld samples, n_k[%d] is %lld", who, k, have[(size_t)k], k, n_k[k]);
}

// the refusals about the draw itself: the block lengths and the replicate indices, which are a 32-bit word of the generator's counter
void draw_check(const char* who, int K, const upk_mbar_boot_draw_t& D, long long n_replicate) {
    if (D.first_replicate < 0 || D.first_replicate >= (1ll << 32))
        MBAR_REFUSE("%s: first_replicate = %lld is outside 0 .. 2^32 - 1", who, D.first_replicate);
    if (n_replicate >= (1ll << 32) || D.first_replicate + n_replicate > (1ll << 32))
        MBAR_REFUSE("%s: replicates %lld .. %lld: a replicate index must stay below 2^32", who, D.first_replicate, D.first_replicate + n_replicate - 1);
    if (D.block)
        for (int k = 0; k < K; ++k)
            if (D.block[k] < 1) MBAR_REFUSE("%s: block[%d] = %lld, a block holds at least one sample", who, k, D.block[k]);
}

// every refusal of upside_hip_mbar_bootstrap (Dr == NULL: the counts are given) and of upside_hip_mbar_bootstrap_drawn (Dr: they are
// drawn); nothing here touches the device
void boot_check(const upk_mbar_boot_problem_t& P, const char* who, const upk_mbar_boot_draw_t* Dr) {
    // the samples, the states, tol, max_iter and f0: the refusals of upside_hip_mbar, one statement of them
    upk_mbar_problem_t Q = as_mbar_problem(P);
    Q.tol = P.tol; Q.max_iter = P.max_iter; Q.f0 = P.f0; Q.f = P.f_boot;
    if (!P.f_boot) MBAR_REFUSE("%s: f_boot must be given", who);
    mbar_check(Q);
    if (P.n_replicate < 1) MBAR_REFUSE("%s: n_replicate = %d, at least one replicate is needed", who, P.n_replicate);
    if (Dr && P.counts) MBAR_REFUSE("%s: the counts are drawn on the device, none may be given", who);
    if (Dr && !P.state_of_sample) MBAR_REFUSE("%s: state_of_sample must be given", who);
    if (!Dr && (!P.counts || !P.state_of_sample)) MBAR_REFUSE("%s: counts and state_of_sample must be given", who);
    if (P.n_column < 0) MBAR_REFUSE("%s: n_column = %d is negative", who, P.n_column);
    if (P.n_column > 0 && (!P.log_numerator || !P.column_boot)) MBAR_REFUSE("%s: log_numerator and column_boot must be given when n_column > 0", who);
    const size_t N = (size_t)P.n_sample; const int K = P.n_state;
    origins_check(who, K, P.n_k, N, P.state_of_sample);
    if (Dr) draw_check(who, K, *Dr, P.n_replicate);
    std::vector<long long> have((size_t)K);
    for (int b = 0; !Dr && b < P.n_replicate; ++b) {
        const unsigned short* c = P.counts + (size_t)b * N;
        std::fill(have.begin(), have.end(), 0ll);
        for (size_t n = 0; n < N; ++n) have[(size_t)P.state_of_sample[n]] += c[n];
        for (int k = 0; k < K; ++k)
            if (have[(size_t)k] != P.n_k[k])
                MBAR_REFUSE("%s: replicate %d: the counts of state %d add up to %lld, n_k[%d] is %lld", who, b, k, have[(size_t)k], k, P.n_k[k]);
    }
    for (size_t j = 0; j < (size_t)P.n_column; ++j)
        for (size_t n = 0; n < N; ++n) {
            const double x = P.log_numerator[j * N + n];
            if (std::isnan(x) || x == INFINITY)
                MBAR_REFUSE("%s: log_numerator: column %zu, sample %zu is %s (-inf is weight 0)", who, j, n, std::isnan(x) ? "not a number" : "+inf");
        }
    const size_t work = P.workspace_bytes ? P.workspace_bytes : (size_t)UPK_MBAR_GRAM_MAX_WORKSPACE;
    if (work > UPK_MBAR_GRAM_MAX_WORKSPACE) MBAR_REFUSE("%s: a workspace of %zu bytes, at most %llu are taken", who, work, UPK_MBAR_GRAM_MAX_WORKSPACE);
    if (upk_mbar_boot_chunk(P.n_sample, work) < 1)
        MBAR_REFUSE("%s: the denominators of one replicate (%lld samples x 8 bytes) do not fit the workspace of %zu bytes", who, P.n_sample, work);
}

// what a draw needs beside the seed, built on the host from checked arguments (the n_k add up to N <= 2^26) and staged once: the
// states' ranges of the grouped order, their clipped block lengths, the stable argsort of state_of_sample where the samples are not
// grouped (a counting sort), the overflow flag
struct DrawPlan {
    std::vector<int> start, length, order;
    long long largest = 0;
    DeviceBuffer start_d, length_d, order_d, flag_d;
    PinnedBuffer flag_h;
    DrawPlan(int K, const long long* n_k, size_t N, const int* state_of_sample, const long long* block) : start((size_t)K + 1, 0), length((size_t)K, 1) {
        for (int k = 0; k < K; ++k) {
            const long long m = n_k[k];
            start[(size_t)k + 1] = start[(size_t)k] + (int)m;
            largest = std::max(largest, m);
            if (block) length[(size_t)k] = (int)std::min(block[k], std::max(m, 1ll));
        }
        bool grouped = true;
        if (state_of_sample) for (size_t n = 1; n < N && grouped; ++n) grouped = state_of_sample[n - 1] <= state_of_sample[n];
        if (grouped) return;
        order.resize(N);
        std::vector<int> at(start.begin(), start.end() - 1);
        for (size_t n = 0; n < N; ++n) order[(size_t)at[(size_t)state_of_sample[n]]++] = (int)n;
    }
    void stage(hipStream_t s) {
        start_d.upload(s, start.data(), start.size() * sizeof(int), "copy of the states' ranges");
        length_d.upload(s, length.data(), length.size() * sizeof(int), "copy of the block lengths");
        if (!order.empty()) order_d.upload(s, order.data(), order.size() * sizeof(int), "copy of the sample order");
        flag_d.alloc(sizeof(unsigned long long), "overflow flag"); flag_h.alloc(sizeof(unsigned long long), "overflow flag");
    }
    bool needs_scratch() const { return largest > UPK_MBAR_BOOT_DRAW_TILE; }
    // replicates first .. first + nb - 1 into counts[nb][N]; scratch: nb x N int32 where needs_scratch().  Synchronises only to read the flag
    void draw(const char* who, hipStream_t s, size_t N, int nb, long long first, unsigned long long seed, int* scratch, count_t* counts) {
        if (needs_scratch()) hip_ok(hipMemsetAsync(flag_d.p, 0xff, sizeof(unsigned long long), s), "overflow flag");
        upk_ok(upk_mbar_boot_draw(s, (int)length.size(), (long long)N, start_d.as<int>(), length_d.as<int>(), order_d.as<int>(), nb, (unsigned)first, seed,
                                  largest, scratch, counts, flag_d.as<unsigned long long>()), "draw of the counts");
        if (!needs_scratch()) return;      // (a state counted in LDS holds fewer samples than a count can)
        hip_ok(hipMemcpyAsync(flag_h.p, flag_d.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, s), "copy of the overflow flag");
        hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize");
        const unsigned long long hit = *flag_h.as<unsigned long long>();
        if (hit != ~0ull)
            MBAR_REFUSE("%s: replicate %llu, state %llu: a count above 65535 cannot be stored", who, hit >> 32, hit & 0xffffffffull);
    }
};

// Dr == NULL: the counts of P; Dr: P.counts == NULL and every chunk's counts are drawn into the buffer the solve reads, with the idle
// denominators as the draw's scratch
void boot_run(const upk_mbar_boot_problem_t& P, const char* who, const upk_mbar_boot_draw_t* Dr) {
    boot_check(P, who, Dr);
    StagedProblem staged(P);      // the samples, the states and the columns go to the device once
    const upk_mbar_states_t& S = staged.S; const upk_mbar_samples_t& X = staged.X; Stream& st = staged.st;
    const int K = P.n_state, B = P.n_replicate, J = P.n_column;
    const size_t N = (size_t)P.n_sample;
    const int chunk = (int)std::min<long long>(B, upk_mbar_boot_chunk(P.n_sample, P.workspace_bytes ? P.workspace_bytes : (size_t)UPK_MBAR_GRAM_MAX_WORKSPACE));
    DeviceBuffer ln_n, log_count, lognum, counts, a, f, f_new, denom, active, delta, column;
    PinnedBuffer active_h, delta_h;
    const std::vector<double> ln_n_h = log_sample_counts(P.n_k, K);
    std::vector<double> start((size_t)chunk * K, 0.), a0((size_t)chunk * K);
    for (int b = 0; b < chunk; ++b) {
        if (P.f0) std::copy(P.f0, P.f0 + K, start.begin() + (size_t)b * K);
        log_counts_plus_f(ln_n_h, P.f0, a0.data() + (size_t)b * K);
    }
    ln_n.upload(st.s, ln_n_h.data(), K * sizeof(double), "copy of n_k");
    if (J) lognum.upload(st.s, P.log_numerator, (size_t)J * N * sizeof(double), "copy of log_numerator");
    log_count.alloc(BOOT_COUNTS * sizeof(double), "log-count table");
    counts.alloc((size_t)chunk * N * sizeof(count_t), "counts"); denom.alloc((size_t)chunk * N * sizeof(double), "denominators");
    a.alloc((size_t)chunk * K * sizeof(double), "a"); f.alloc((size_t)chunk * K * sizeof(double), "f"); f_new.alloc((size_t)chunk * K * sizeof(double), "f");
    active.alloc((size_t)chunk * sizeof(int), "active"); delta.alloc((size_t)chunk * sizeof(double), "delta");
    if (J) column.alloc((size_t)chunk * J * sizeof(double), "columns");
    active_h.alloc((size_t)chunk * sizeof(int), "active"); delta_h.alloc((size_t)chunk * sizeof(double), "delta");
    int* act = active_h.as<int>(); const double* dl = delta_h.as<double>();

    upk_ok(upk_mbar_boot_log_counts(st.s, log_count.as<double>()), "log-count table");
    std::unique_ptr<DrawPlan> plan;
    if (Dr) { plan.reset(new DrawPlan(K, P.n_k, N, P.state_of_sample, Dr->block)); plan->stage(st.s); }

    std::vector<int> iters((size_t)chunk); std::vector<double> last((size_t)chunk);
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        if (Dr) {
            plan->draw(who, st.s, N, nb, Dr->first_replicate + b0, Dr->seed, denom.as<int>(), counts.as<count_t>());
            if (Dr->counts_out)      // (the synchronisation that ends the chunk covers it)
                hip_ok(hipMemcpyAsync(Dr->counts_out + (size_t)b0 * N, counts.p, (size_t)nb * N * sizeof(count_t), hipMemcpyDeviceToHost, st.s), "copy of the drawn counts");
        } else
            hip_ok(hipMemcpyAsync(counts.p, P.counts + (size_t)b0 * N, (size_t)nb * N * sizeof(count_t), hipMemcpyHostToDevice, st.s), "copy of counts");
        hip_ok(hipMemcpyAsync(f.p, start.data(), (size_t)nb * K * sizeof(double), hipMemcpyHostToDevice, st.s), "copy of f0");
        hip_ok(hipMemcpyAsync(a.p, a0.data(), (size_t)nb * K * sizeof(double), hipMemcpyHostToDevice, st.s), "copy of f0");
        int n_active = nb;
        for (int i = 0; i < nb; ++i) { act[i] = i; iters[(size_t)i] = 0; last[(size_t)i] = INFINITY; }
        bool list_changed = true;
        for (int it = 1; n_active > 0; ++it) {
            if (list_changed) hip_ok(hipMemcpyAsync(active.p, act, (size_t)n_active * sizeof(int), hipMemcpyHostToDevice, st.s), "copy of the active list");
            upk_ok(upk_mbar_boot_denominator(st.s, &S, &X, a.as<double>(), active.as<int>(), n_active, denom.as<double>()), "denominator pass");
            upk_ok(upk_mbar_boot_free_energy(st.s, &S, &X, counts.as<count_t>(), log_count.as<double>(), active.as<int>(), n_active, denom.as<double>(),
                                             f_new.as<double>()), "free-energy pass");
            upk_ok(upk_mbar_boot_update(st.s, K, ln_n.as<double>(), active.as<int>(), n_active, f_new.as<double>(), f.as<double>(), a.as<double>(),
                                        delta.as<double>()), "update");
            hip_ok(hipMemcpyAsync(delta_h.p, delta.p, (size_t)n_active * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of delta");
            hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");      // the one synchronisation of the iteration
            int kept = 0;
            for (int i = 0; i < n_active; ++i) {
                const int b = act[i];
                iters[(size_t)b] = it; last[(size_t)b] = dl[i];
                if (!(dl[i] < P.tol) && it < P.max_iter) act[kept++] = b;      // (ascending order is kept)
            }
            list_changed = kept != n_active;
            n_active = kept;
        }
        if (J) {      // the denominators of the returned f of every replicate of the chunk, then the columns
            for (int i = 0; i < nb; ++i) act[i] = i;
            hip_ok(hipMemcpyAsync(active.p, act, (size_t)nb * sizeof(int), hipMemcpyHostToDevice, st.s), "copy of the active list");
            upk_ok(upk_mbar_boot_denominator(st.s, &S, &X, a.as<double>(), active.as<int>(), nb, denom.as<double>()), "denominator pass");
            upk_ok(upk_mbar_boot_columns(st.s, P.n_sample, counts.as<count_t>(), log_count.as<double>(), active.as<int>(), nb, denom.as<double>(), J,
                                         lognum.as<double>(), column.as<double>()), "column pass");
            hip_ok(hipMemcpyAsync(P.column_boot + (size_t)b0 * J, column.p, (size_t)nb * J * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of the columns");
        }
        hip_ok(hipMemcpyAsync(P.f_boot + (size_t)b0 * K, f.p, (size_t)nb * K * sizeof(double), hipMemcpyDeviceToHost, st.s), "copy of f");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");      // (the next chunk overwrites counts, f and a)
        for (int i = 0; i < nb; ++i) {
            if (P.n_iter) P.n_iter[b0 + i] = iters[(size_t)i];
            if (P.last_delta) P.last_delta[b0 + i] = last[(size_t)i];
        }
    }
}

// the draw alone: replicates D.first_replicate .. + n_replicate - 1 into D.counts_out, in chunks whose scratch fits the default workspace
void draw_counts_run(const char* who, int K, const long long* n_k, long long n_sample, const int* state_of_sample, long long n_replicate,
                     const upk_mbar_boot_draw_t& D) {
    if (K < 1) MBAR_REFUSE("%s: n_state = %d, at least one state is needed", who, K);
    if (n_sample < 1) MBAR_REFUSE("%s: n_sample = %lld, at least one sample is needed", who, n_sample);
    if (!n_k || !D.counts_out) MBAR_REFUSE("%s: n_k and counts_out must be given", who);
    long long total = 0;
    for (int k = 0; k < K; ++k) {
        if (n_k[k] < 0) MBAR_REFUSE("%s: n_k[%d] = %lld is negative", who, k, n_k[k]);
        if (n_k[k] > n_sample - total) MBAR_REFUSE("%s: the sample counts n_k add up to more than n_sample = %lld", who, n_sample);
        total += n_k[k];
    }
    if (total != n_sample) MBAR_REFUSE("%s: the sample counts n_k add up to %lld, n_sample is %lld", who, total, n_sample);
    if (n_replicate < 1) MBAR_REFUSE("%s: n_replicate = %lld, at least one replicate is needed", who, n_replicate);
    const long long fit = upk_mbar_boot_chunk(n_sample, (size_t)UPK_MBAR_GRAM_MAX_WORKSPACE);
    if (fit < 1) MBAR_REFUSE("%s: n_sample = %lld, at most 2^26 samples are taken", who, n_sample);
    const size_t N = (size_t)n_sample;
    if (state_of_sample) origins_check(who, K, n_k, N, state_of_sample);
    draw_check(who, K, D, n_replicate);
    require_device();
    Stream st;
    hip_ok(hipStreamCreate(&st.s), "hipStreamCreate");
    DrawPlan plan(K, n_k, N, state_of_sample, D.block);
    plan.stage(st.s);
    const int chunk = (int)std::min(n_replicate, fit);
    DeviceBuffer counts, scratch;
    counts.alloc((size_t)chunk * N * sizeof(count_t), "counts");
    if (plan.needs_scratch()) scratch.alloc((size_t)chunk * N * sizeof(int), "scratch of the draw");
    for (long long b0 = 0; b0 < n_replicate; b0 += chunk) {
        const int nb = (int)std::min<long long>(chunk, n_replicate - b0);
        plan.draw(who, st.s, N, nb, D.first_replicate + b0, D.seed, scratch.as<int>(), counts.as<count_t>());
        hip_ok(hipMemcpyAsync(D.counts_out + (size_t)b0 * N, counts.p, (size_t)nb * N * sizeof(count_t), hipMemcpyDeviceToHost, st.s), "copy of the drawn counts");
        hip_ok(hipStreamSynchronize(st.s), "hipStreamSynchronize");      // (the next chunk overwrites counts)
    }
}

}  // namespace

extern "C" int upk_mbar_boot_solve(const upk_mbar_boot_problem_t* P, char* message, int message_len) {
    return guarded_entry("mbar_bootstrap", message, message_len, [&] {
        if (!P) MBAR_REFUSE("mbar_bootstrap: no problem given");
        boot_run(*P, "mbar_bootstrap", nullptr);
    });
}
extern "C" int upk_mbar_boot_solve_drawn(const upk_mbar_boot_problem_t* P, const upk_mbar_boot_draw_t* D, char* message, int message_len) {
    return guarded_entry("mbar_bootstrap_drawn", message, message_len, [&] {
        if (!P || !D) MBAR_REFUSE("mbar_bootstrap_drawn: no problem or no draw given");
        boot_run(*P, "mbar_bootstrap_drawn", D);
    });
}
extern "C" int upk_mbar_boot_draw_solve(int n_state, const long long* n_k, long long n_sample, const int* state_of_sample, long long n_replicate,
                                        const upk_mbar_boot_draw_t* D, char* message, int message_len) {
    const char* who = "mbar_bootstrap_counts";
    return guarded_entry(who, message, message_len, [&] {
        if (!D) MBAR_REFUSE("%s: no draw given", who);
        draw_counts_run(who, n_state, n_k, n_sample, state_of_sample, n_replicate, *D);
    });
}

// The Metropolis rule of replica exchange (main.cpp:251-273) in host arithmetic, for exchange ACROSS engines / processes:
// every rank holds the same all-gathered energies and reaches the same verdicts.  No device, no engine: this file stands alone.
// The device states the same rule once in device_math.h (exchange_lboltz_diff, exchange_accept).
#include "../../include/upside_engine_c.h"
#include <cmath>

extern "C" void upside_hip_set_last_error(const char* msg);   // engine_c_api.cpp: prints "ERROR: ..." and keeps the message

namespace {
inline uint32_t h_rotl32(uint32_t x, unsigned n) { return (x << (n & 31)) | (x >> ((32 - n) & 31)); }
void h_threefry4x32_20(uint32_t X[4], const uint32_t key[4]) {   // Random123/threefry.h:110-117,172,296-430
    static const unsigned R[8][2] = {{10, 26}, {11, 21}, {13, 27}, {23, 5}, {6, 20}, {17, 11}, {25, 10}, {18, 20}};
    uint32_t ks[5]; ks[4] = 0x1BD11BDAu;
    for (int i = 0; i < 4; ++i) { ks[i] = key[i]; ks[4] ^= key[i]; }
    for (int i = 0; i < 4; ++i) X[i] += ks[i];
    for (int r = 0; r < 20; ++r) {
        if (r % 2 == 0) { X[0] += X[1]; X[1] = h_rotl32(X[1], R[r % 8][0]); X[1] ^= X[0]; X[2] += X[3]; X[3] = h_rotl32(X[3], R[r % 8][1]); X[3] ^= X[2]; }
        else            { X[0] += X[3]; X[3] = h_rotl32(X[3], R[r % 8][0]); X[3] ^= X[0]; X[2] += X[1]; X[1] = h_rotl32(X[1], R[r % 8][1]); X[1] ^= X[2]; }
        if (r % 4 == 3) { const int k = r / 4 + 1; for (int i = 0; i < 4; ++i) X[i] += ks[(k + i) % 5]; X[3] += k; }
    }
}
float h_u01(uint32_t in) {   // uniform.hpp:145-179, the product and the sum rounded separately
#pragma clang fp contract(off)
    const float factor = 1.f / 4294967296.f;
    volatile float t = (float)in * factor;
    return t + 0.5f * factor;
}
// the verdict on one log-Boltzmann difference: a uniform of the round's generator is drawn only for a rejectable pair
// (main.cpp:268); draw = the generator's position, advanced here
int h_exchange_accept(float lb, uint32_t base_seed, uint64_t round, int& draw) {
    if (!(lb < 0.f)) return 1;
    const uint32_t key[4] = {base_seed, 1u /* REPLICA_EXCHANGE_RANDOM_STREAM */, 0u, 0u};
    uint32_t X[4] = {(uint32_t)(round & 0xffffffffu), (uint32_t)(round >> 32), 0u, (uint32_t)draw++};
    h_threefry4x32_20(X, key);
    return !(expf(lb) < h_u01(X[0]));
}
}  // namespace

// on given differences (any mixture of Hamiltonians); accepted[n_pair] = generator position after this set
extern "C" int upside_replica_decide_lboltz(int n_pair, const float* lboltz_diff, uint32_t base_seed, uint64_t round, int draw0, int* accepted) {
    int draw = draw0;
    for (int p = 0; p < n_pair; ++p) accepted[p] = h_exchange_accept(lboltz_diff[p], base_seed, round, draw);
    accepted[n_pair] = draw;
    return 0;
}
// temperature exchange of one Hamiltonian: (new_lboltz[s1]+new_lboltz[s2]) - (old_lboltz[s1]+old_lboltz[s2]) with the energies traded
extern "C" int upside_replica_decide(int n_pair, const int* pairs, const float* beta, const float* energy, uint32_t base_seed,
                                     uint64_t round, int draw0, int* accepted) {
#pragma clang fp contract(off)
    int draw = draw0;
    for (int p = 0; p < n_pair; ++p) {
        const int s1 = pairs[p * 2], s2 = pairs[p * 2 + 1];
        if (s1 < 0 || s2 < 0) { upside_hip_set_last_error("invalid system"); return 1; }
        const float lb = (-beta[s1] * energy[s2] + -beta[s2] * energy[s1]) - (-beta[s1] * energy[s1] + -beta[s2] * energy[s2]);
        accepted[p] = h_exchange_accept(lb, base_seed, round, draw);
    }
    accepted[n_pair] = draw;   // generator position for the next swap set of this round
    return 0;
}

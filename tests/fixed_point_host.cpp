// Stand-alone host restatement of the two float -> fixed-point conversions of the pair passes' gradient accumulators, for
// tests/test_fixed_point_host.py (plain C++, no device code): the arithmetic of to_fixed32 (upside-md_amd/csrc/device_math.h) and of
// lds_add_fixed22_pairs / lds_add_fixed22_wide_scaled (upside-md_amd/csrc/pair2_device.h) statement by statement, with the three gfx950
// conversion instructions they compile to written out with the hardware's behaviour at the edges (saturation, NaN -> 0), which C++
// leaves undefined for a cast.
//
//   fixed_point_host 32 <bits>...      to_fixed32 of each float (given as 8 hex digits): one line "<signed 64-bit value>"
//   fixed_point_host 22 <bits>...      the packed passes' conversion of each SCALED contribution vs = v * 2^22 on the wide path:
//                                      "<value> 0", or "0 1" where the device sets the error flag instead of adding
//   fixed_point_host sq <bits>...      1 if a trip with these scaled contributions takes the 32-bit conversions, 0 if the wide path
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static float from_bits(const char* s) { uint32_t u = (uint32_t)strtoul(s, nullptr, 16); float f; memcpy(&f, &u, 4); return f; }

// v_cvt_i32_f32: toward zero, saturating, NaN -> 0
static int32_t cvt_i32_f32(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.f) return INT32_MAX;
    if (x <= -2147483648.f) return INT32_MIN;
    return (int32_t)x;
}
// v_cvt_rpi_i32_f32: floor(x + 0.5) (exact: evaluated in double), saturating, NaN -> 0
static int32_t cvt_rpi_i32_f32(float x) {
    if (x != x) return 0;
    const double r = std::floor((double)x + 0.5);
    if (r >= 2147483648.) return INT32_MAX;
    if (r <= -2147483648.) return INT32_MIN;
    return (int32_t)r;
}
// __float2ll_rn: nearest even, saturating (only reached below 2^46 here)
static int64_t float2ll_rn(float x) { return (int64_t)std::nearbyint((double)x); }

static uint64_t to_fixed32(float v) {
    const float h = std::nearbyintf(v);
    const int32_t hi = cvt_i32_f32(h), half = cvt_i32_f32((v - h) * 2147483648.f);
    return ((uint64_t)((uint32_t)hi + (uint32_t)(half >> 31)) << 32) | (uint32_t)((uint32_t)half << 1);
}

static const float FIX_NARROW = 1073741824.f, FIX_WIDE = 70368744177664.f;      // 2^30, 2^46
static bool fixed22_wide_scaled(float vs, int64_t& q) {       // false: the error flag
    const float a = std::fabs(vs);
    if (!(a < FIX_WIDE)) return false;
    q = a < FIX_NARROW ? (int64_t)cvt_rpi_i32_f32(vs) : float2ll_rn(vs);
    return true;
}
static bool trip_is_narrow(int n, const float* od) {           // values taken two by two as the halves of the packed registers
    float sx = 0.f, sy = 0.f;
    for (int c = 0; c < n; c += 2) {
        const float x = od[c], y = c + 1 < n ? od[c + 1] : 0.f;
        sx = c ? std::fmaf(x, x, sx) : x * x;
        sy = c ? std::fmaf(y, y, sy) : y * y;
    }
    return sx + sy < FIX_NARROW * FIX_NARROW;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (!strcmp(argv[1], "32")) {
        for (int i = 2; i < argc; ++i) printf("%lld\n", (long long)(int64_t)to_fixed32(from_bits(argv[i])));
    } else if (!strcmp(argv[1], "22")) {
        for (int i = 2; i < argc; ++i) {
            int64_t q = 0;
            const bool ok = fixed22_wide_scaled(from_bits(argv[i]), q);
            printf("%lld %d\n", (long long)(ok ? q : 0), ok ? 0 : 1);
        }
    } else if (!strcmp(argv[1], "sq")) {
        float od[64]; int n = 0;
        for (int i = 2; i < argc && n < 64; ++i) od[n++] = from_bits(argv[i]);
        printf("%d\n", trip_is_narrow(n, od) ? 1 : 0);
    } else return 2;
    return 0;
}

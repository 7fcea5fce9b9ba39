// check_fdiv1.hip -- is ONE residual correction enough in fdiv_n_bare (csrc/rtg_math.cuh, round 18)?  Device check of
// the library's own fdiv_n_bare / fdiv_n (as RTG_FDIV_CORRECTIONS builds them) against the compiler's IEEE a / b, and
// of cr_sqrt_nt at the exp-map read-out's argument 1 - w w.  NaN == NaN.  0 mismatches required.
//
//   check_fdiv1 exhaustive [chunks]   the proof: every mantissa pair a, b in [1, 2) (2^46 pairs; `chunks` of 2^36 pairs,
//                                      default all 1024), the reciprocal's scale invariance, and the read-out's root
//   check_fdiv1 sampled               the quick form tests/test_gpu_fdiv_one_correction.py runs
//   check_fdiv1 single                round 22's single quotients (tests/test_gpu_single_quotients.py): fdiv1 on its
//                                      regions [N] and [C], and each converted site against its a / b form
//
// Why the mantissa pairs are the whole window (the argument next to fdiv_n_bare): for |a|, |b| in [2^-47, 2^47] the
// sequence is  y = rcp(b); y = fma(fma(-b, y, 1), y, y); t = a y; q = fma(fma(-b, t, a), y, t)  in plain f32
// arithmetic.  Every operation is a single rounding of an exact expression, so it commutes with a factor 2^j on a,
// 2^k on b (y scales by 2^-k, t and q by 2^(j-k), the residual by 2^j) and with either sign, PROVIDED no
// intermediate leaves the normal range and v_rcp_f32 itself scales: [S] below checks rcp(+-m 2^k) = +-rcp(m) 2^-k for
// every mantissa m and every k in -47 .. 47.  fma(-b, y, 1) is the same number at every scale (b y is); the residual
// a - b t is exact in the fma, zero or a multiple of ulp(b) ulp(t) >= 2^-46 |b t| / 4 >= 2^-96, never subnormal, and
// q is at least 2^-95 and at most 2^95.  So q(a 2^j, b 2^k) = q(a, b) 2^(j-k) and likewise RN(a / b): equality on
// [1, 2) x [1, 2) is equality on the window.
//  [E]  exhaustive mantissa pairs: fdiv_n_bare<1> against a / b
//  [S]  v_rcp_f32 commutes with powers of two and signs over the window
//  [R]  cr_sqrt_nt(1 - w w) against __builtin_sqrtf (NaN == NaN) and, bit for bit with its NaNs, against cr_sqrt,
//       every f32 w (2^32)
//  [1]  sampled: fdiv_n<2>, fdiv_n<3> on 2^30 hashed in-window groups (sign, mantissa and exponent hashed)
//  [2.k] sampled: every mantissa of b (2^23 each): in [1, 2) with hashed numerators; in the window's lowest binade;
//       in its highest; in [1, 2) under the fixed numerator a = 0x3FB504F3 (and its neighbours as a1, a2)
//  [3.k] sampled: round 13's nine families outside the window, 2^22 groups each: every group takes the fallback
//  [N.k] single: fdiv1 behind fdiv1_in_n against a / b, every mantissa of b in the region's lowest binade, in [1, 2),
//       in its highest binade, and in the binade below / above the region (k = 0 .. 4), each under 15 numerators: both
//       numerator edges, one binade outside them, +-0, denormal, +-inf, NaN, and a hashed one inside
//  [C.k] single: fdiv1_const behind fdiv1_in_c against a / c, every f32 a, c = sqrt(3) (la_bdsqr3_entry) and 5 (mean5).
//       The gripper's a / C.orig is not converted (profiles/r22/single_quotients/sites.md): there is no third constant
//  [G] [P] [T] [X] single: la_larfg<1>, <2>, la_bdsqr3_pass, la_bdsqr3_entry and the exp-map read-out against their
//       a / b forms on 2^24 hashed operand sets each, scaled to sit inside, on and outside each test's edges
//  In `single` a guard's verdict is compared with one worked out here from the bit patterns: "in-region" counts both.
// Built with the library's arithmetic flags (csrc/Makefile check_fdiv1).
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "rtg_math.cuh"

using namespace rtg;

constexpr int kFamilies = 9, kMantFams = 4;
constexpr uint32_t kFamBits = 22;

__device__ unsigned long long g_done[8], g_bad[8], g_fallback[8];
__device__ unsigned long long g_fam_fallback[kFamilies], g_fam_bad[kFamilies], g_mant_bad[kMantFams], g_mant_fb[kMantFams];
__device__ uint32_t g_first[8][4];
enum { C_EXH = 0, C_SCALE, C_ROOT, C_RAND, C_MANT, C_OUT };

__device__ __forceinline__ bool same(float a, float b)
{
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}
__device__ __forceinline__ uint64_t mix(uint64_t h)
{
    h *= 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h;
}
__device__ __forceinline__ void first_bad(unsigned long long k, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b)
{
    if (k < 8) { g_first[k][0] = a0; g_first[k][1] = a1; g_first[k][2] = a2; g_first[k][3] = b; }
}
__device__ __forceinline__ void ran(int k, unsigned long long per_thread = 1ull)
{
    if (threadIdx.x == 0) atomicAdd(&g_done[k], (unsigned long long)blockDim.x * per_thread);
}

// [E] one thread per mantissa of b, 2^13 mantissas of a each: chunk c covers a's mantissas c 2^13 .. (c + 1) 2^13 - 1
constexpr uint32_t kALoop = 1u << 13;
__global__ __launch_bounds__(256) void k_exhaustive(uint32_t chunk)
{
    const uint32_t mb = blockIdx.x * blockDim.x + threadIdx.x;   // 0 .. 2^23 - 1
    const float b = __uint_as_float(0x3F800000u | mb);
    const uint32_t ua0 = 0x3F800000u | (chunk * kALoop);
    uint32_t nbad = 0, ubad = 0;
    for (uint32_t j = 0; j < kALoop; ++j) {
        const float a[1] = {__uint_as_float(ua0 + j)};
        float q[1];
        fdiv_n_bare<1>(a, b, q);
        if (__float_as_uint(q[0]) != __float_as_uint(a[0] / b)) { ++nbad; ubad = ua0 + j; }
    }
    ran(C_EXH, kALoop);
    if (nbad) {
        const unsigned long long k = atomicAdd(&g_bad[C_EXH], (unsigned long long)nbad);
        first_bad(k, ubad, 0u, 0u, __float_as_uint(b));
    }
}

// [S] i = mantissa + 2^23 * (exponent index 0 .. 94) ... sign handled in the thread
__global__ __launch_bounds__(256) void k_rcp_scale(uint32_t e)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    const float b1 = __uint_as_float(0x3F800000u | m);
    const int k = (int)e - 47;
    const float bk = __uint_as_float(((127u + (uint32_t)k) << 23) | m);   // b1 2^k, or 2^47 itself at the top (below)
    const float y1 = __builtin_amdgcn_rcpf(b1);
    const float want = __builtin_ldexpf(y1, -k);
    if (k < 47) ran(C_SCALE, 2);                                 // counted: the inputs evaluated below
    else if (m == 0u) atomicAdd(&g_done[C_SCALE], 2ull);
    int nbad = 0;
    if (k < 47 || m == 0u) {   // above 2^47 nothing is inside the window
        nbad += !same(__builtin_amdgcn_rcpf(bk), want);
        nbad += !same(__builtin_amdgcn_rcpf(-bk), -want);
    }
    if (nbad) {
        const unsigned long long q = atomicAdd(&g_bad[C_SCALE], (unsigned long long)nbad);
        first_bad(q, 0u, 0u, 0u, __float_as_uint(bk));
    }
}

// [R] every w
__global__ __launch_bounds__(256) void k_root(uint32_t base)
{
    const uint32_t u = base + blockIdx.x * blockDim.x + threadIdx.x;
    const float w = __uint_as_float(u);
    const float x = 1.0f - w * w;
    const float s = cr_sqrt_nt(x);
    ran(C_ROOT);
    // against cr_sqrt bit for bit, NaN patterns included (the site's swap); against the IEEE root NaN == NaN
    if (!same(s, __builtin_sqrtf(x)) || __float_as_uint(s) != __float_as_uint(cr_sqrt(x))) {
        const unsigned long long k = atomicAdd(&g_bad[C_ROOT], 1ull);
        first_bad(k, u, __float_as_uint(x), __float_as_uint(s), 0u);
    }
}

// ---- the sampled checks (check_fdiv.hip's groups: both forms of fdiv_n on one group)
__device__ __forceinline__ uint32_t with_exp(uint32_t u, uint32_t e) { return (u & 0x807FFFFFu) | (e << 23); }
constexpr uint32_t kELo = 127 - 47, kEHi = 127 + 47;
__device__ __forceinline__ uint32_t in_window(uint32_t u) { return with_exp(u, kELo + ((u >> 23) & 0xFFu) % (kEHi - kELo)); }
__device__ __forceinline__ int check_group(const uint32_t (&ua)[3], uint32_t ub, bool &fell)
{
    const float a3[3] = {__uint_as_float(ua[0]), __uint_as_float(ua[1]), __uint_as_float(ua[2])};
    const float a2[2] = {a3[0], a3[1]};
    const float b = __uint_as_float(ub);
    float q3[3], q2[2];
    fdiv_n<3>(a3, b, q3);
    fdiv_n<2>(a2, b, q2);
    const bool ok3 = same(q3[0], a3[0] / b) && same(q3[1], a3[1] / b) && same(q3[2], a3[2] / b);
    const bool ok2 = same(q2[0], a2[0] / b) && same(q2[1], a2[1] / b);
    bool win = fdiv_in_window(b);
    for (int i = 0; i < 3; ++i) win = win && fdiv_in_window(a3[i]);
    fell = !win;
    return (ok3 ? 0 : 1) + (ok2 ? 0 : 1);
}
__global__ __launch_bounds__(256) void k_rand(void)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t h = mix(i + 0x18ull), h2 = mix(i ^ 0x5DEECE66Dull);
    const uint32_t ua[3] = {in_window((uint32_t)h), in_window((uint32_t)(h >> 32)), in_window((uint32_t)h2)};
    const uint32_t ub = in_window((uint32_t)(h2 >> 32));
    ran(C_RAND);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    if (fell) atomicAdd(&g_fallback[C_RAND], 1ull);
    if (nbad) first_bad(atomicAdd(&g_bad[C_RAND], (unsigned long long)nbad), ua[0], ua[1], ua[2], ub);
}
// i = family * 2^23 + mantissa of b
__global__ __launch_bounds__(256) void k_mant(void)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t fam = i >> 23, mant = i & 0x7FFFFFu;
    const uint64_t h = mix(0xF00Dull + i);
    const uint32_t sign = (uint32_t)(h >> 63) << 31;
    const uint32_t eb = fam == 1 ? kELo : fam == 2 ? kEHi - 1 : 127u;
    const uint32_t ub = sign | (eb << 23) | mant;
    uint32_t ua[3];
    if (fam == 3) {   // a fixed numerator (RN sqrt 2) and its neighbours
        ua[0] = 0x3FB504F3u; ua[1] = 0x3FB504F2u; ua[2] = 0x3FB504F4u;
    } else {
        // a0: the far end of the window from b (around 1: either end); a1: b's neighbourhood; a2: hashed
        const uint32_t far = fam == 1 ? kEHi - 1 : fam == 2 ? kELo : ((h >> 40) & 1 ? kELo : kEHi - 1);
        ua[0] = with_exp((uint32_t)h, far);
        ua[1] = (ub ^ ((uint32_t)(h >> 32) & 0x80000000u)) + ((uint32_t)(h >> 41) & 7u) - 3u;
        ua[2] = in_window((uint32_t)(h >> 16));
        if ((ua[1] & 0x7FFFFFFFu) < (kELo << 23) || (ua[1] & 0x7FFFFFFFu) > (kEHi << 23)) ua[1] = ub;
    }
    ran(C_MANT);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    if (fell) atomicAdd(&g_mant_fb[fam], 1ull);
    if (nbad) {
        atomicAdd(&g_mant_bad[fam], (unsigned long long)nbad);
        first_bad(atomicAdd(&g_bad[C_MANT], (unsigned long long)nbad), ua[0], ua[1], ua[2], ub);
    }
}
// family = i >> kFamBits: round 13's nine families outside the window
__global__ __launch_bounds__(256) void k_out(void)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t fam = i >> kFamBits;
    const uint64_t h = mix(0xBEEFull + i), h2 = mix(i ^ 0x5DEECE66Dull);
    uint32_t ua[3] = {in_window((uint32_t)h), in_window((uint32_t)(h >> 32)), in_window((uint32_t)h2)};
    uint32_t ub = in_window((uint32_t)(h2 >> 32));
    const uint32_t r = (uint32_t)(h2 >> 7), k = r % 3u, k2 = r % 2u;   // k2: a numerator both forms read
    const uint32_t nz = (r >> 8) | 1u;                                   // a nonzero mantissa
    switch (fam) {
    case 0: ua[k2] &= 0x80000000u; break;                                        // +-0
    case 1: ua[k2] = (ua[k2] & 0x80000000u) | (nz & 0x7FFFFFu); break;           // denormal
    case 2: ua[k2] = (r & 256u) ? with_exp(ua[k2], kELo - 1) : (ua[k2] & 0x80000000u) | ((kELo << 23) - 1u); break;
    case 3: ua[k2] = (ua[k2] & 0x80000000u) | (kEHi << 23) | ((r & 256u) ? 1u : (nz & 0x7FFFFFu)); break;
    case 4: ub = (r & 256u) ? with_exp(ub, kELo - 1) : (ub & 0x80000000u) | ((kELo << 23) - 1u); break;
    case 5: ub = (ub & 0x80000000u) | (kEHi << 23) | ((r & 256u) ? 1u : (nz & 0x7FFFFFu)); break;
    case 6: ub = (ub & 0x80000000u) | (nz & 0x7FFFFFu); break;
    case 7: ub = (ub & 0x80000000u) | (k == 0 ? 0u : k == 1 ? 0x7F800000u : 0x7FC00000u | (r & 0x3FFFFFu)); break;
    default: {   // a0 / b (and sometimes a1 / b) subnormal or just normal: exponent(b) = exponent(a) + 126 .. 149
        const uint32_t ea = 1u + (r >> 9) % 100u, eb = ea + 126u + (r >> 20) % 24u;
        ua[0] = with_exp(ua[0], ea);
        if (r & 256u) ua[1] = with_exp(ua[1], ea + 1u);
        ub = with_exp(ub, eb < 254u ? eb : 254u);
        break;
    }
    }
    ran(C_OUT);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    if (fell) atomicAdd(&g_fam_fallback[fam], 1ull);
    if (nbad) {
        atomicAdd(&g_fam_bad[fam], (unsigned long long)nbad);
        first_bad(atomicAdd(&g_bad[C_OUT], (unsigned long long)nbad), ua[0], ua[1], ua[2], ub);
    }
}


// ---- single: round 22's single quotients
constexpr int kNFams = 5, kNCls = 15, kSites = 5;
__device__ unsigned long long g_n_bad[kNFams], g_n_in[kNFams], g_n_want[kNFams], g_n_verdict[kNFams];
__device__ unsigned long long g_c_bad[2], g_c_in[2], g_c_want[2], g_c_verdict[2], g_c_done[2];
__device__ unsigned long long g_s_bad[kSites], g_s_in[kSites], g_s_verdict[kSites], g_s_done[kSites];
__device__ __forceinline__ uint32_t absbits(float x) { return __float_as_uint(x) & 0x7FFFFFFFu; }
constexpr uint32_t kBitsNumLo = (127u - 76u) << 23, kBitsDivLo = (127u - 47u) << 23, kBitsDivHi = (127u + 47u) << 23;
constexpr uint32_t kBitsConstHi = (127u + 94u) << 23;
// i = family * 2^23 + mantissa of b; families: b's binade 2^-47 (lowest), [1, 2), 2^46 (highest), 2^-48, 2^47 (outside)
__global__ __launch_bounds__(256) void k_single_n(void)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t fam = i >> 23, mant = i & 0x7FFFFFu;
    const uint32_t eb = fam == 0 ? 127u - 47u : fam == 1 ? 127u : fam == 2 ? 127u + 46u : fam == 3 ? 127u - 48u : 127u + 47u;
    const uint64_t h0 = mix(0xD1Full + i);
    const uint32_t ub = ((uint32_t)(h0 >> 63) << 31) | (eb << 23) | ((fam == 4 && mant == 0u) ? 1u : mant);
    const float b = __uint_as_float(ub);
    const bool b_in = fam < 3;
    uint32_t nbad = 0, nin = 0, nwant = 0, nverdict = 0, ubad = 0;
    for (int c = 0; c < kNCls; ++c) {
        const uint64_t h = mix(h0 + 977ull * (uint64_t)(c + 1));
        const uint32_t m = (uint32_t)h & 0x7FFFFFu, sg = (uint32_t)(h >> 40) << 31;
        uint32_t ua;
        bool a_in;
        switch (c) {
        case 0: ua = kBitsNumLo | m; a_in = true; break;                      // the lowest binade inside
        case 1: ua = kBitsNumLo; a_in = true; break;                          // the lower edge
        case 2: ua = kBitsNumLo - 1u; a_in = false; break;                    // its predecessor
        case 3: ua = (kBitsNumLo - (1u << 23)) | m; a_in = false; break;      // one binade outside
        case 4: ua = (kBitsDivHi - (1u << 23)) | m; a_in = true; break;       // the highest binade inside
        case 5: ua = kBitsDivHi; a_in = true; break;                          // the upper edge
        case 6: ua = kBitsDivHi + 1u; a_in = false; break;                    // its successor
        case 7: ua = kBitsDivHi | (m | 1u); a_in = false; break;              // one binade outside
        case 8: ua = 0u; a_in = false; break;
        case 9: ua = 0x80000000u; a_in = false; break;
        case 10: ua = m | 1u; a_in = false; break;                            // denormal
        case 11: ua = 0x7F800000u; a_in = false; break;
        case 12: ua = 0xFF800000u; a_in = false; break;
        case 13: ua = 0x7FC00000u | (m >> 1); a_in = false; break;
        default: ua = ((127u - 76u + (uint32_t)(h >> 24) % 123u) << 23) | m; a_in = true; break;   // 2^-76 .. 2^46
        }
        if (c <= 7 || c == 10 || c == 13 || c == 14) ua |= sg;
        const float a = __uint_as_float(ua);
        const bool in = fdiv1_in_n(a, b), want = a_in && b_in;
        const float q = in ? fdiv1(a, b) : a / b;
        nin += in;
        nwant += want;
        nverdict += in != want;
        if (!same(q, a / b)) { ++nbad; ubad = ua; }
    }
    ran(C_RAND, kNCls);
    atomicAdd(&g_n_in[fam], (unsigned long long)nin);
    atomicAdd(&g_n_want[fam], (unsigned long long)nwant);
    if (nverdict) atomicAdd(&g_n_verdict[fam], (unsigned long long)nverdict);
    if (nbad) {
        atomicAdd(&g_n_bad[fam], (unsigned long long)nbad);
        first_bad(atomicAdd(&g_bad[C_RAND], (unsigned long long)nbad), ubad, 0u, 0u, ub);
    }
}
// every f32 numerator under constant k: 0 sqrt(3) as la_bdsqr3_entry divides, 1 five as mean5 does
__global__ __launch_bounds__(256) void k_single_c(uint32_t base, int k)
{
    const uint32_t u = base + blockIdx.x * blockDim.x + threadIdx.x;
    const float a = __uint_as_float(u);
    const bool in = fdiv1_in_c(a), want = absbits(a) >= kBitsNumLo && absbits(a) <= kBitsConstHi;
    float q, ref;
    if (k == 0) { q = in ? fdiv1_const(a, kSqrt3, kRcpSqrt3) : a / kSqrt3; ref = a / kSqrt3; }
    else { q = fdiv_by5(a); ref = a / 5.0f; }
    const unsigned long long nin = __popcll(__ballot(in)), nwant = __popcll(__ballot(want));
    const unsigned long long nver = __popcll(__ballot(in != want)), nbad = __popcll(__ballot(!same(q, ref)));
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&g_c_done[k], 64ull);
        atomicAdd(&g_c_in[k], nin);
        atomicAdd(&g_c_want[k], nwant);
        if (nver) atomicAdd(&g_c_verdict[k], nver);
        if (nbad) atomicAdd(&g_c_bad[k], nbad);
    }
    if (!same(q, ref)) first_bad(atomicAdd(&g_bad[C_MANT], 1ull), u, 0u, 0u, (uint32_t)k);
}
// a hashed value whose exponent is e0 + (0 .. spread - 1), hashed sign and mantissa
__device__ __forceinline__ float hval(uint64_t h, int e0, int spread)
{
    const int e = e0 + (int)((h >> 32) % (uint64_t)spread);
    const uint32_t eb = (uint32_t)(e < -126 ? -126 : e > 127 ? 127 : e) + 127u;
    return __uint_as_float(((uint32_t)(h >> 63) << 31) | (eb << 23) | ((uint32_t)h & 0x7FFFFFu));
}
// specials now and then: which = 0 none, else +-0, denormal, +-inf, NaN, 2^+-100
__device__ __forceinline__ float special(float x, uint32_t which, uint32_t m)
{
    switch (which) {
    case 1: return 0.0f;
    case 2: return -0.0f;
    case 3: return __uint_as_float((__float_as_uint(x) & 0x80000000u) | (m & 0x7FFFFFu) | 1u);
    case 4: return __uint_as_float(0x7F800000u);
    case 5: return __uint_as_float(0xFF800000u);
    case 6: return __uint_as_float(0x7FC00000u);
    case 7: return __builtin_copysignf(0x1p100f, x);
    case 8: return __builtin_copysignf(0x1p-100f, x);
    default: return x;
    }
}
// the base exponents the hashed operand sets are scaled to: around -76, -47 / -46, 0 and 45 .. 47
__device__ __forceinline__ int base_exp(uint32_t r)
{
    const int tab[16] = {-79, -77, -76, -75, -49, -48, -47, -46, -45, -20, 0, 20, 43, 44, 45, 46};
    return tab[r & 15u];
}
// site 0, 1: la_larfg<1>, <2>; 2: la_bdsqr3_pass; 3: la_bdsqr3_entry; 4: the exp-map read-out
__global__ __launch_bounds__(256) void k_single_sites(int site)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t h = mix(0x5173ull * (uint64_t)(site + 1) + i), h2 = mix(h ^ 0xABCDull), h3 = mix(h2 + 1ull);
    const uint64_t h4 = mix(h3 + 2ull), h5 = mix(h4 + 3ull), h6 = mix(h5 + 4ull);
    const int e0 = base_exp((uint32_t)(h6 >> 8));
    // one operand in 16 sets is special in one place; spread: 0 .. 2 binades, or wide (tiny mu, tiny e, near rank 1)
    const uint32_t sp = ((h6 >> 16) & 15u) == 0u ? 1u + (uint32_t)((h6 >> 20) % 8u) : 0u, where = (uint32_t)(h6 >> 24) % 5u;
    const int spread = ((h6 >> 28) & 3u) == 0u ? 40 : 3;
    float v[5] = {hval(h, e0, 3), hval(h2, e0, spread), hval(h3, e0, 3), hval(h4, e0, spread), hval(h5, e0, spread)};
    v[where] = special(v[where], sp, (uint32_t)h6);
    // one set in 32: all five denormal (a state the bare sequence cannot divide: v_rcp_f32 of a denormal sum), so a
    // fallback that left part of its group bare would show
    if (((h6 >> 40) & 31u) == 0u) {
        const uint64_t hd[5] = {h, h2, h3, h4, h5};
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = __uint_as_float(((uint32_t)(hd[k] >> 63) << 31) | ((uint32_t)hd[k] & 0x7FFFFFu) | 0x1000u);
    }
    bool in = false, want = false, bad = false;
    if (site <= 1) {
        float al = v[0], x0 = v[1], x1 = site ? v[3] : 0.0f, ar = al, y0 = x0, y1 = x1;
        in = site ? la_larfg_ok<2>(al, x0, x1) : la_larfg_ok<1>(al, x0, x1);
        // NaN in x is dropped by the max as in the site; the verdict here takes the larger bit pattern of the non-NaN
        const uint32_t b0 = absbits(x0) > 0x7F800000u ? 0u : absbits(x0), b1 = absbits(x1) > 0x7F800000u ? 0u : absbits(x1);
        const uint32_t w = site ? (b0 > b1 ? b0 : b1) : absbits(x0);
        want = w >= ((127u - 46u) << 23) && w <= ((127u + 45u) << 23) && absbits(al) <= ((127u + 45u) << 23);
        if (site == 0 && absbits(x0) > 0x7F800000u) want = false;
        const float t = site ? la_larfg<2>(al, x0, x1) : la_larfg<1>(al, x0, x1);
        const float tr = site ? la_larfg_ieee<2>(ar, y0, y1) : la_larfg_ieee<1>(ar, y0, y1);
        bad = !same(t, tr) || !same(al, ar) || !same(x0, y0) || !same(x1, y1);
    } else if (site == 2 || site == 3) {
        const float smax = la_bdsqr3_smax(v[0], v[1], v[2], v[3], v[4]);
        in = la_bdsqr3_state_ok(v[0], v[1], v[2], v[3], v[4], smax);
        uint32_t mn = 0xFFFFFFFFu, mx = 0u;
        for (int k = 0; k < 5; ++k) {
            const uint32_t u = absbits(v[k]);
            if (u > 0x7F800000u) continue;   // a NaN passes the chains (see la_bdsqr3)
            mn = u < mn ? u : mn;
            mx = u > mx ? u : mx;
        }
        want = mn >= ((127u - 46u) << 23) && mx <= ((127u + 46u) << 23) && mx != 0u;
        if (site == 2) {
            const BdsqrPass p = la_bdsqr3_pass(v[0], v[1], v[2], v[3], v[4], smax);
            const BdsqrPass r = la_bdsqr3_shift<false>(v[0], v[1], v[2], v[3], v[4], smax);
            bad = p.zero != r.zero || !same(p.shift, r.shift);
        } else {
            bad = !same(la_bdsqr3_entry(v[0], v[1], v[2], v[3], v[4]), la_bdsqr3_sminoa<false>(v[0], v[1], v[2], v[3], v[4]) / kSqrt3);
        }
    } else {
        // the read-out: sin_theta over (1e-5, 1] (and now and then under it: mask fails), qk scaled as a numerator
        const float st = ((h6 >> 32) & 7u) == 0u ? hval(h2, -40, 30) : fabsf(hval(h2, -17, 18));
        float qk = hval(h, e0, 3);
        qk = special(qk, sp, (uint32_t)h6);
        const ExpDof e{fabsf(hval(h3, -2, 3)), st, fabsf(st) > 1e-5f, false};
        in = !exp_dof_redo(e, qk);
        want = !e.mask || (absbits(qk) >= kBitsNumLo && absbits(qk) <= kBitsDivHi);
        const float got = in ? exp_dof_finish(e, qk) : e.angle * (qk / e.sin_theta);
        bad = !same(got, e.mask ? e.angle * (qk / e.sin_theta) : 0.0f);
    }
    const unsigned long long nin = __popcll(__ballot(in)), nver = __popcll(__ballot(in != want)), nbad = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&g_s_done[site], 64ull);
        atomicAdd(&g_s_in[site], nin);
        if (nver) atomicAdd(&g_s_verdict[site], nver);
        if (nbad) atomicAdd(&g_s_bad[site], nbad);
    }
    if (bad) first_bad(atomicAdd(&g_bad[C_OUT], 1ull), __float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), (uint32_t)site);
}

static bool sync_ok(const char *what)
{
    const hipError_t e = hipDeviceSynchronize(), l = hipGetLastError();
    if (e != hipSuccess || l != hipSuccess) {
        printf("launch/run failure in %s: %s\n", what, hipGetErrorString(e != hipSuccess ? e : l));
        return false;
    }
    return true;
}
static double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void print_first(unsigned long long nbad)
{
    uint32_t first[8][4];
    (void)hipMemcpyFromSymbol(first, HIP_SYMBOL(g_first), sizeof first);
    for (unsigned long long k = 0; k < (nbad < 8 ? nbad : 8); ++k)
        printf("  mismatch: a = %08x %08x %08x  b = %08x\n", first[k][0], first[k][1], first[k][2], first[k][3]);
}

static int run_exhaustive(uint32_t chunks)
{
    unsigned long long done[8], bad[8];
    // [S], [R] first: they are short
    for (uint32_t e = 0; e <= 94; ++e) hipLaunchKernelGGL(k_rcp_scale, dim3((1u << 23) / 256u), dim3(256), 0, 0, e);
    for (uint32_t c = 0; c < 4; ++c) hipLaunchKernelGGL(k_root, dim3((1u << 30) / 256u), dim3(256), 0, 0, c << 30);
    if (!sync_ok("[S] / [R]")) return 2;
    const double t0 = now_s();
    for (uint32_t c = 0; c < chunks; ++c) {
        hipLaunchKernelGGL(k_exhaustive, dim3((1u << 23) / 256u), dim3(256), 0, 0, c);
        if ((c & 63u) == 63u || c + 1 == chunks) {
            if (!sync_ok("[E]")) return 2;
            (void)hipMemcpyFromSymbol(bad, HIP_SYMBOL(g_bad), sizeof bad);
            printf("  [E] %u of %u chunks of 2^36 pairs, %.1f s, %llu mismatches so far\n", c + 1, chunks, now_s() - t0,
                   bad[C_EXH]);
            fflush(stdout);
        }
    }
    (void)hipMemcpyFromSymbol(done, HIP_SYMBOL(g_done), sizeof done);
    (void)hipMemcpyFromSymbol(bad, HIP_SYMBOL(g_bad), sizeof bad);
    const unsigned long long want_e = (unsigned long long)chunks << 36, want_s = (94ull << 24) + 2ull, want_r = 1ull << 32;
    if (done[C_EXH] != want_e || done[C_SCALE] != want_s || done[C_ROOT] != want_r) {
        printf("covered %llu / %llu / %llu of %llu / %llu / %llu inputs\n", done[C_EXH], done[C_SCALE], done[C_ROOT],
               want_e, want_s, want_r);
        return 2;
    }
    printf("RTG_FDIV_CORRECTIONS = %d, RTG_FIT_FAST_DIV_TU = %d\n", (int)RTG_FDIV_CORRECTIONS, (int)RTG_FIT_FAST_DIV_TU);
    printf("[E] fdiv_n_bare<1> on mantissa pairs a, b in [1, 2): %llu pairs (%s), %llu mismatches\n", want_e,
           chunks == 1024u ? "all 2^46" : "a partial run", bad[C_EXH]);
    printf("[S] v_rcp_f32 of +-m 2^k against +-rcp(m) 2^-k, every mantissa for k = -47 .. 46, and 2^47 itself: %llu inputs, %llu mismatches\n",
           want_s, bad[C_SCALE]);
    printf("[R] cr_sqrt_nt(1 - w w) against __builtin_sqrtf and cr_sqrt, every f32 w: %llu inputs, %llu mismatches\n",
           want_r, bad[C_ROOT]);
    const unsigned long long total = bad[C_EXH] + bad[C_SCALE] + bad[C_ROOT];
    print_first(total);
    return total ? 1 : 0;
}

static int run_sampled()
{
    hipLaunchKernelGGL(k_rand, dim3((1u << 30) / 256u), dim3(256), 0, 0);
    hipLaunchKernelGGL(k_mant, dim3(((unsigned)kMantFams << 23) / 256u), dim3(256), 0, 0);
    hipLaunchKernelGGL(k_out, dim3(((unsigned)kFamilies << kFamBits) / 256u), dim3(256), 0, 0);
    for (uint32_t c = 0; c < 4; ++c) hipLaunchKernelGGL(k_root, dim3((1u << 30) / 256u), dim3(256), 0, 0, c << 30);
    if (!sync_ok("sampled")) return 2;
    unsigned long long done[8], bad[8], fb[8], ffb[kFamilies], fbad[kFamilies], mbad[kMantFams], mfb[kMantFams];
    (void)hipMemcpyFromSymbol(done, HIP_SYMBOL(g_done), sizeof done);
    (void)hipMemcpyFromSymbol(bad, HIP_SYMBOL(g_bad), sizeof bad);
    (void)hipMemcpyFromSymbol(fb, HIP_SYMBOL(g_fallback), sizeof fb);
    (void)hipMemcpyFromSymbol(ffb, HIP_SYMBOL(g_fam_fallback), sizeof ffb);
    (void)hipMemcpyFromSymbol(fbad, HIP_SYMBOL(g_fam_bad), sizeof fbad);
    (void)hipMemcpyFromSymbol(mbad, HIP_SYMBOL(g_mant_bad), sizeof mbad);
    (void)hipMemcpyFromSymbol(mfb, HIP_SYMBOL(g_mant_fb), sizeof mfb);
    const unsigned long long nfam = 1ull << kFamBits, nmant = 1ull << 23;
    if (done[C_RAND] != 1ull << 30 || done[C_MANT] != kMantFams * nmant || done[C_OUT] != kFamilies * nfam ||
        done[C_ROOT] != 1ull << 32) {
        printf("a check did not cover its inputs: %llu %llu %llu %llu\n", done[C_RAND], done[C_MANT], done[C_OUT],
               done[C_ROOT]);
        return 2;
    }
    printf("RTG_FDIV_CORRECTIONS = %d, RTG_FIT_FAST_DIV_TU = %d\n", (int)RTG_FDIV_CORRECTIONS, (int)RTG_FIT_FAST_DIV_TU);
    printf("[1] fdiv_n<2>, fdiv_n<3>, in-window groups: %llu groups, %llu mismatches, fallback on %llu\n", 1ull << 30,
           bad[C_RAND], fb[C_RAND]);
    const char *mnames[kMantFams] = {"b in [1, 2)", "b in [2^-47, 2^-46)", "b in [2^46, 2^47)",
                                     "b in [1, 2) under a = RN(sqrt 2) and its neighbours"};
    bool ok = fb[C_RAND] == 0;
    for (int f = 0; f < kMantFams; ++f) {
        printf("[2.%d] every mantissa, %s: %llu groups, %llu mismatches, fallback on %llu\n", f, mnames[f], nmant, mbad[f],
               mfb[f]);
        ok = ok && mfb[f] == 0;
    }
    const char *names[kFamilies] = {"numerator +-0", "numerator denormal", "numerator just below the window",
                                    "numerator just above the window", "b just below the window",
                                    "b just above the window", "b denormal", "b +-0 / +-inf / NaN",
                                    "subnormal and near-subnormal quotients"};
    for (int f = 0; f < kFamilies; ++f) {
        printf("[3.%d] %s: %llu groups, %llu mismatches, fallback on %llu\n", f, names[f], nfam, fbad[f], ffb[f]);
        ok = ok && ffb[f] == nfam;
    }
    printf("[R] cr_sqrt_nt(1 - w w) against __builtin_sqrtf and cr_sqrt, every f32 w: %llu inputs, %llu mismatches\n",
           1ull << 32, bad[C_ROOT]);
    const unsigned long long total = bad[C_RAND] + bad[C_MANT] + bad[C_OUT] + bad[C_ROOT];
    print_first(total);
    if (!ok) printf("an in-window group took the fallback, or an out-of-window group did not\n");
    return (total || !ok) ? 1 : 0;
}


static int run_single()
{
    hipLaunchKernelGGL(k_single_n, dim3(((unsigned)kNFams << 23) / 256u), dim3(256), 0, 0);
    for (int k = 0; k < 2; ++k)
        for (uint32_t c = 0; c < 4; ++c) hipLaunchKernelGGL(k_single_c, dim3((1u << 30) / 256u), dim3(256), 0, 0, c << 30, k);
    for (int site = 0; site < kSites; ++site) hipLaunchKernelGGL(k_single_sites, dim3((1u << 24) / 256u), dim3(256), 0, 0, site);
    if (!sync_ok("single")) return 2;
    unsigned long long nbad[kNFams], nin[kNFams], nwant[kNFams], nver[kNFams], cbad[2], cin[2], cwant[2], cver[2], cdone[2];
    unsigned long long sbad[kSites], sin_[kSites], sver[kSites], sdone[kSites], done[8];
    (void)hipMemcpyFromSymbol(done, HIP_SYMBOL(g_done), sizeof done);
    (void)hipMemcpyFromSymbol(nbad, HIP_SYMBOL(g_n_bad), sizeof nbad);
    (void)hipMemcpyFromSymbol(nin, HIP_SYMBOL(g_n_in), sizeof nin);
    (void)hipMemcpyFromSymbol(nwant, HIP_SYMBOL(g_n_want), sizeof nwant);
    (void)hipMemcpyFromSymbol(nver, HIP_SYMBOL(g_n_verdict), sizeof nver);
    (void)hipMemcpyFromSymbol(cbad, HIP_SYMBOL(g_c_bad), sizeof cbad);
    (void)hipMemcpyFromSymbol(cin, HIP_SYMBOL(g_c_in), sizeof cin);
    (void)hipMemcpyFromSymbol(cwant, HIP_SYMBOL(g_c_want), sizeof cwant);
    (void)hipMemcpyFromSymbol(cver, HIP_SYMBOL(g_c_verdict), sizeof cver);
    (void)hipMemcpyFromSymbol(cdone, HIP_SYMBOL(g_c_done), sizeof cdone);
    (void)hipMemcpyFromSymbol(sbad, HIP_SYMBOL(g_s_bad), sizeof sbad);
    (void)hipMemcpyFromSymbol(sin_, HIP_SYMBOL(g_s_in), sizeof sin_);
    (void)hipMemcpyFromSymbol(sver, HIP_SYMBOL(g_s_verdict), sizeof sver);
    (void)hipMemcpyFromSymbol(sdone, HIP_SYMBOL(g_s_done), sizeof sdone);
    printf("RTG_FDIV_CORRECTIONS = %d, RTG_FIT_FAST_DIV_TU = %d\n", (int)RTG_FDIV_CORRECTIONS, (int)RTG_FIT_FAST_DIV_TU);
    unsigned long long total = 0, verdicts = 0;
    bool covered = done[C_RAND] == (unsigned long long)kNCls * kNFams << 23;
    const char *nn[kNFams] = {"b in [2^-47, 2^-46)", "b in [1, 2)", "b in [2^46, 2^47)", "b in [2^-48, 2^-47), outside",
                              "b in (2^47, 2^48), outside"};
    for (int f = 0; f < kNFams; ++f) {
        printf("[N.%d] fdiv1 behind fdiv1_in_n, every mantissa, %s: %llu quotients, %llu mismatches, in-region %llu (worked out here: %llu, %llu verdicts differ)\n",
               f, nn[f], (unsigned long long)kNCls << 23, nbad[f], nin[f], nwant[f], nver[f]);
        total += nbad[f];
        verdicts += nver[f] + (nin[f] != nwant[f]);
        if (nwant[f] != (f < 3 ? 5ull << 23 : 0ull)) covered = false;
    }
    const char *cn[2] = {"a / sqrt(3) (la_bdsqr3_entry)", "a / 5 (mean5)"};
    for (int k = 0; k < 2; ++k) {
        printf("[C.%d] %s, every f32 a: %llu quotients, %llu mismatches, in-region %llu (worked out here: %llu, %llu verdicts differ)\n",
               k, cn[k], cdone[k], cbad[k], cin[k], cwant[k], cver[k]);
        total += cbad[k];
        verdicts += cver[k] + (cin[k] != cwant[k]);
        if (cdone[k] != 1ull << 32 || cwant[k] != 2ull * (((unsigned long long)(kBitsConstHi - kBitsNumLo)) + 1ull)) covered = false;
    }
    const char *sn[kSites] = {"[G.1] la_larfg<1>", "[G.2] la_larfg<2>", "[P] la_bdsqr3_pass", "[T] la_bdsqr3_entry",
                              "[X] exp-map read-out"};
    for (int k = 0; k < kSites; ++k) {
        printf("%s against its a / b form: %llu operand sets, %llu mismatches, test passed on %llu (%llu verdicts differ)\n", sn[k],
               sdone[k], sbad[k], sin_[k], sver[k]);
        total += sbad[k];
        verdicts += sver[k];
        // both branches must have run: a test that never passes (or never fails) checks nothing
        if (sdone[k] != 1ull << 24 || sin_[k] < 1ull << 20 || sdone[k] - sin_[k] < 1ull << 20) covered = false;
    }
    print_first(total);
    if (verdicts) printf("a guard admitted operands outside its region, or refused operands inside it\n");
    if (!covered) printf("a check did not cover its inputs\n");
    return (total || verdicts) ? 1 : covered ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        const long chunks = argc >= 3 ? strtol(argv[2], nullptr, 10) : 1024;
        if (chunks < 1 || chunks > 1024) { printf("chunks: 1 .. 1024\n"); return 2; }
        return run_exhaustive((uint32_t)chunks);
    }
    if (argc >= 2 && !strcmp(argv[1], "sampled")) return run_sampled();
    if (argc >= 2 && !strcmp(argv[1], "single")) return run_single();
    printf("usage: check_fdiv1 exhaustive [chunks] | sampled | single\n");
    return 2;
}

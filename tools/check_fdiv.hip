// check_fdiv.hip -- device check of the shared-reciprocal division and the unscaled square root of csrc/rtg_math.cuh
// (round 13), against the compiler's IEEE division a / b and __builtin_sqrtf; NaN == NaN.  0 mismatches required.
//  [1] fdiv_n<2> and fdiv_n<3> on 2^32 hashed groups with b and every a_i inside the window [2^-47, 2^47]
//      (sign, mantissa and exponent hashed); no group may take the fallback;
//  [2] every f32 mantissa of b in the window's lowest binade [2^-47, 2^-46), its highest [2^46, 2^47), and [1, 2),
//      and b = 2^47 itself, either sign, with numerators at the far end of the window (the largest exponent
//      differences), next to b (quotients around 1) and hashed; no fallback;
//  [3] families outside the window, 2^24 groups each, every group must take the fallback: a numerator +-0; a
//      denormal numerator; a numerator just below / just above the window; b just below / just above the window;
//      b denormal; b one of +-0, +-inf, NaN; quotients in or next to the subnormal range;
//  [3b] every triple (a0, a1, b) of 48 special values with either sign (zeros, denormals, the window's edges and
//      their neighbours, 1, extremes, inf, NaN): both forms, whichever path the guard picks;
//  [4] cr_sqrt_nt on every f32 bit pattern that is >= 2^-96, +-0, +inf or NaN.
// For [3] the fallback count is the library's own guard (fdiv_in_window) evaluated on the group.
// Built with the library's flags and run by tests/test_gpu_fdiv.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

#include "rtg_math.cuh"

using namespace rtg;

enum { C_RAND = 0, C_MANT, C_OUT, C_SPECIAL, C_SQRT, C_N };
constexpr int kFamilies = 10;

__device__ unsigned long long g_done[C_N];             // inputs each check ran (a failed launch must not read as a pass)
__device__ unsigned long long g_bad[C_N];              // mismatches
__device__ unsigned long long g_fallback[C_N];         // groups the guard sends to the fallback
__device__ unsigned long long g_fam_fallback[kFamilies], g_fam_bad[kFamilies];
__device__ uint32_t g_first[8][4];                     // the first mismatching groups: a0, a1, a2, b

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
// sign and mantissa from u, biased exponent e
__device__ __forceinline__ uint32_t with_exp(uint32_t u, uint32_t e) { return (u & 0x807FFFFFu) | (e << 23); }
constexpr uint32_t kELo = 127 - 47, kEHi = 127 + 47;   // biased exponents of the window's edges 2^-47 and 2^47
// u with its exponent hashed into the window: [2^-47, 2^47)
__device__ __forceinline__ uint32_t in_window(uint32_t u) { return with_exp(u, kELo + ((u >> 23) & 0xFFu) % (kEHi - kELo)); }

// both forms on one group; returns the number of mismatching forms and whether the guard sends the group to the fallback
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
__device__ __forceinline__ void tally(int check, const uint32_t (&ua)[3], uint32_t ub, int nbad, bool fell)
{
    if (fell) atomicAdd(&g_fallback[check], 1ull);
    if (nbad) {
        const unsigned long long k = atomicAdd(&g_bad[check], (unsigned long long)nbad);
        if (k < 2) {
            uint32_t *f = g_first[2 * (check & 3) + k];
            f[0] = ua[0]; f[1] = ua[1]; f[2] = ua[2]; f[3] = ub;
        }
    }
}
__device__ __forceinline__ void ran(int k)
{
    if (threadIdx.x == 0) atomicAdd(&g_done[k], (unsigned long long)blockDim.x);
}

// [1]
__global__ void k_rand(uint64_t base)
{
    const uint64_t i = base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t h = mix(i), h2 = mix(i ^ 0x5DEECE66Dull);
    const uint32_t ua[3] = {in_window((uint32_t)h), in_window((uint32_t)(h >> 32)), in_window((uint32_t)h2)};
    const uint32_t ub = in_window((uint32_t)(h2 >> 32));
    ran(C_RAND);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    tally(C_RAND, ua, ub, nbad, fell);
}

// [2] i = binade (0..2) * 2^24 + sign * 2^23 + mantissa; the last block of 256 threads takes b = +-2^47
__global__ void k_mant(void)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t binade = i >> 24, mant = i & 0x7FFFFFu, sign = binade == 3 ? (mant >> 1) & 1u : (i >> 23) & 1u;
    const uint32_t eb = binade == 0 ? kELo : binade == 1 ? kEHi - 1 : binade == 2 ? 127u : kEHi;
    const uint32_t ub = (sign << 31) | (eb << 23) | (binade == 3 ? 0u : mant);
    const uint64_t h = mix(0xF00Dull + i);
    // a0: the far end of the window from b (for b around 1: either end); a1: b's neighbourhood; a2: hashed
    const uint32_t far = binade == 0 ? kEHi - 1 : binade == 1 || binade == 3 ? kELo : ((h >> 40) & 1 ? kELo : kEHi - 1);
    uint32_t ua[3] = {with_exp((uint32_t)h, far), (ub ^ ((uint32_t)(h >> 32) & 0x80000000u)) + ((uint32_t)(h >> 41) & 7u) - 3u,
                      in_window((uint32_t)(h >> 16))};
    if (binade == 3) ua[1] = with_exp((uint32_t)(h >> 32), kEHi - 1);   // b = 2^47: nothing above it is inside
    // keep b's neighbours inside the window
    if ((ua[1] & 0x7FFFFFFFu) < (kELo << 23) || (ua[1] & 0x7FFFFFFFu) > (kEHi << 23)) ua[1] = ub;
    if (binade == 3 && (mant & 1u)) ua[0] = (ua[0] & 0x80000000u) | (kEHi << 23);   // 2^47 / 2^47, and 2^-47.. / 2^47
    ran(C_MANT);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    tally(C_MANT, ua, ub, nbad, fell);
}

// [3] family = i >> 24
__global__ void k_out(void)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t fam = i >> 24;
    const uint64_t h = mix(0xBEEFull + i), h2 = mix(i ^ 0x5DEECE66Dull);
    uint32_t ua[3] = {in_window((uint32_t)h), in_window((uint32_t)(h >> 32)), in_window((uint32_t)h2)};
    uint32_t ub = in_window((uint32_t)(h2 >> 32));
    const uint32_t r = (uint32_t)(h2 >> 7), k = r % 3u, k2 = r % 2u;   // which numerator (k2: one both forms read)
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
    case 8: {   // a0 / b (and sometimes a1 / b) subnormal or just normal: exponent(b) = exponent(a) + 126 .. 149
        const uint32_t ea = 1u + (r >> 9) % 100u, eb = ea + 126u + (r >> 20) % 24u;
        ua[0] = with_exp(ua[0], ea);
        if (r & 256u) ua[1] = with_exp(ua[1], ea + 1u);
        ub = with_exp(ub, eb < 254u ? eb : 254u);
        break;
    }
    default: {   // raw bit patterns everywhere (mostly outside): whatever path the guard picks must be right
        ua[0] = (uint32_t)h; ua[1] = (uint32_t)(h >> 32); ua[2] = (uint32_t)h2; ub = (uint32_t)(h2 >> 32);
        break;
    }
    }
    ran(C_OUT);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    tally(C_OUT, ua, ub, nbad, fell);
    if (fell) atomicAdd(&g_fam_fallback[fam], 1ull);
    if (nbad) atomicAdd(&g_fam_bad[fam], (unsigned long long)nbad);
}

// [3b] 96 x 96 x 96 signed special values
__global__ void k_special(void)
{
    const uint32_t sp[48] = {
        0x00000000u, 0x00000001u, 0x00000002u, 0x00400000u, 0x007FFFFFu, 0x00800000u, 0x00800001u, 0x01000000u,
        0x0B800000u, 0x0C000000u, 0x0F800000u, 0x27000000u, 0x277FFFFFu, 0x27800000u, 0x27FFFFFEu, 0x27FFFFFFu,
        0x28000000u, 0x28000001u, 0x287FFFFFu, 0x28800000u, 0x2B800000u, 0x33800000u, 0x3EAAAAABu, 0x3F7FFFFFu,
        0x3F800000u, 0x3F800001u, 0x3FFFFFFFu, 0x40000000u, 0x40490FDBu, 0x4B800000u, 0x53800000u, 0x567FFFFFu,
        0x56800000u, 0x56FFFFFFu, 0x57000000u, 0x57000001u, 0x577FFFFFu, 0x57800000u, 0x5F000000u, 0x6F000000u,
        0x7E800000u, 0x7F000000u, 0x7F7FFFFFu, 0x7F800000u, 0x7F800001u, 0x7FA00000u, 0x7FC00000u, 0x7FFFFFFFu};
    const uint32_t i0 = threadIdx.x, i1 = blockIdx.x, ib = blockIdx.y;   // 96 each
    const uint32_t s0 = sp[i0 % 48u] | (i0 >= 48u ? 0x80000000u : 0u), s1 = sp[i1 % 48u] | (i1 >= 48u ? 0x80000000u : 0u);
    const uint32_t ub = sp[ib % 48u] | (ib >= 48u ? 0x80000000u : 0u);
    const uint32_t ua[3] = {s0, s1, sp[(i0 + i1 + ib) % 48u] | ((i0 ^ i1) & 1u ? 0x80000000u : 0u)};
    ran(C_SPECIAL);
    bool fell;
    const int nbad = check_group(ua, ub, fell);
    tally(C_SPECIAL, ua, ub, nbad, fell);
}

// [4] every bit pattern; the ones outside cr_sqrt_nt's domain (below 2^-96 and not 0, negative, -inf) are skipped
__device__ unsigned long long g_sqrt_inputs;
__global__ void k_sqrt_nt(uint64_t base)
{
    const uint32_t u = (uint32_t)(base + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    const float x = __uint_as_float(u);
    ran(C_SQRT);
    if (!((x >= 0x1p-96f) || x == 0.0f || x != x)) return;
    atomicAdd(&g_sqrt_inputs, 1ull);
    if (!same(cr_sqrt_nt(x), __builtin_sqrtf(x))) atomicAdd(&g_bad[C_SQRT], 1ull);
}

int main()
{
    const uint64_t chunk = 1ull << 30;
    for (uint64_t base = 0; base < (1ull << 32); base += chunk) {
        hipLaunchKernelGGL(k_rand, dim3((unsigned)(chunk / 256)), dim3(256), 0, 0, base);
        hipLaunchKernelGGL(k_sqrt_nt, dim3((unsigned)(chunk / 256)), dim3(256), 0, 0, base);
    }
    hipLaunchKernelGGL(k_mant, dim3((3u << 24) / 256u + 1u), dim3(256), 0, 0);
    hipLaunchKernelGGL(k_out, dim3(((unsigned)kFamilies << 24) / 256u), dim3(256), 0, 0);
    hipLaunchKernelGGL(k_special, dim3(96, 96), dim3(96), 0, 0);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) {
        printf("launch/run failure: %s\n", hipGetErrorString(hipGetLastError()));
        return 2;
    }
    unsigned long long done[C_N], bad[C_N], fb[C_N], ffb[kFamilies], fbad[kFamilies], nsqrt = 0;
    (void)hipMemcpyFromSymbol(done, HIP_SYMBOL(g_done), sizeof done);
    (void)hipMemcpyFromSymbol(bad, HIP_SYMBOL(g_bad), sizeof bad);
    (void)hipMemcpyFromSymbol(fb, HIP_SYMBOL(g_fallback), sizeof fb);
    (void)hipMemcpyFromSymbol(ffb, HIP_SYMBOL(g_fam_fallback), sizeof ffb);
    (void)hipMemcpyFromSymbol(fbad, HIP_SYMBOL(g_fam_bad), sizeof fbad);
    (void)hipMemcpyFromSymbol(&nsqrt, HIP_SYMBOL(g_sqrt_inputs), sizeof nsqrt);
    const unsigned long long nmant = (3ull << 24) + 256ull, nfam = 1ull << 24;
    const unsigned long long want[C_N] = {1ull << 32, nmant, (unsigned long long)kFamilies << 24, 96ull * 96ull * 96ull,
                                          1ull << 32};
    for (int k = 0; k < C_N; ++k)
        if (done[k] != want[k]) {
            printf("check %d covered %llu of %llu inputs\n", k, done[k], want[k]);
            return 2;
        }
    // 2^-96 .. +inf: (0x7F800000 - 0x0F800000) + 1 patterns; +-0; the NaNs of either sign: 2 (2^23 - 1)
    const unsigned long long want_sqrt = (0x7F800000ull - 0x0F800000ull + 1ull) + 2ull + 2ull * ((1ull << 23) - 1ull);
    if (nsqrt != want_sqrt) {
        printf("cr_sqrt_nt check covered %llu of %llu inputs\n", nsqrt, want_sqrt);
        return 2;
    }
    printf("[1] fdiv_n<2>, fdiv_n<3>, in-window groups: %llu groups, %llu mismatches, fallback on %llu\n", want[C_RAND],
           bad[C_RAND], fb[C_RAND]);
    printf("[2] every mantissa of b at the window's edge binades, at 1.0 and b = 2^47: %llu groups, %llu mismatches, "
           "fallback on %llu\n", nmant, bad[C_MANT], fb[C_MANT]);
    const char *names[kFamilies] = {"numerator +-0", "numerator denormal", "numerator just below the window",
                                    "numerator just above the window", "b just below the window",
                                    "b just above the window", "b denormal", "b +-0 / +-inf / NaN",
                                    "subnormal and near-subnormal quotients", "raw bit patterns"};
    bool fam_ok = true;
    for (int f = 0; f < kFamilies; ++f) {
        printf("[3.%d] %s: %llu groups, %llu mismatches, fallback on %llu\n", f, names[f], nfam, fbad[f], ffb[f]);
        if (f < kFamilies - 1 && ffb[f] != nfam) fam_ok = false;   // every such group is outside the window
        if (f == kFamilies - 1 && ffb[f] == 0) fam_ok = false;
    }
    printf("[3b] special values: %llu triples, %llu mismatches, fallback on %llu\n", want[C_SPECIAL], bad[C_SPECIAL],
           fb[C_SPECIAL]);
    printf("[4] cr_sqrt_nt: %llu inputs, %llu mismatches\n", want_sqrt, bad[C_SQRT]);
    uint32_t first[8][4];
    (void)hipMemcpyFromSymbol(first, HIP_SYMBOL(g_first), sizeof first);
    for (int c = 0; c < 4; ++c)
        for (unsigned long long k = 0; k < (bad[c] < 2 ? bad[c] : 2); ++k)
            printf("  check %d: a = %08x %08x %08x  b = %08x\n", c, first[2 * c + k][0], first[2 * c + k][1],
                   first[2 * c + k][2], first[2 * c + k][3]);
    const bool in_window_clean = fb[C_RAND] == 0 && fb[C_MANT] == 0;
    if (!in_window_clean) printf("an in-window group took the fallback\n");
    if (!fam_ok || fb[C_SPECIAL] == 0) printf("an out-of-window family did not take the fallback\n");
    unsigned long long total = 0;
    for (int k = 0; k < C_N; ++k) total += bad[k];
    return (total || !in_window_clean || !fam_ok || fb[C_SPECIAL] == 0) ? 1 : 0;
}

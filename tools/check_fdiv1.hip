// check_fdiv1.hip -- is ONE residual correction enough in fdiv_n_bare (csrc/rtg_math.cuh, round 18)?  Device check of
// the library's own fdiv_n_bare / fdiv_n (as RTG_FDIV_CORRECTIONS builds them) against the compiler's IEEE a / b, and
// of cr_sqrt_nt at the exp-map read-out's argument 1 - w w.  NaN == NaN.  0 mismatches required.
//
//   check_fdiv1 exhaustive [chunks]   the proof: every mantissa pair a, b in [1, 2) (2^46 pairs; `chunks` of 2^36 pairs,
//                                      default all 1024), the reciprocal's scale invariance, and the read-out's root
//   check_fdiv1 sampled               the quick form tests/test_gpu_fdiv_one_correction.py runs
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

int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "exhaustive")) {
        const long chunks = argc >= 3 ? strtol(argv[2], nullptr, 10) : 1024;
        if (chunks < 1 || chunks > 1024) { printf("chunks: 1 .. 1024\n"); return 2; }
        return run_exhaustive((uint32_t)chunks);
    }
    if (argc >= 2 && !strcmp(argv[1], "sampled")) return run_sampled();
    printf("usage: check_fdiv1 exhaustive [chunks] | sampled\n");
    return 2;
}

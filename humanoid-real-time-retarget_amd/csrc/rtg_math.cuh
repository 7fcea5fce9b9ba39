// rtg_math.cuh -- device math for the retargeting hot path (gfx950).
//
// Every float32 operation is rounded on its own, in the association order the
// reference's torch CPU ops use (build flag -ffp-contract=off plus the pragma
// below); the two places torch itself fuses (torch.linalg.norm of a 3-vector
// and torch.cross) use explicit __builtin_fmaf.  Measured op orders: DESIGN.md §3.
//
//  * torch.sqrt/acos/sin/cos run through MKL VML on the CPU (closed source):
//    here they are correctly rounded (evaluated in float64, rounded once).
//  * atan2 on the 30-element DOF tensor runs glibc's scalar atan2f: restated
//    exactly (fdlibm s_atanf/e_atan2f).
//  * torch.linalg.svd (MKL sgesdd) in the Kabsch fit: oneMKL 2024.2's 3x3 path
//    (SGEBD2 / SBDSQR / SORMBR with MKL's measured FMA placement), restated.
//  * scipy Rotation.as_euler / from_euler: float64 restatement.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtg_crmath.h"
#include "rtg_knobs.h"

#pragma clang fp contract(off)

namespace rtg {

struct Q { float x, y, z, w; };
struct V { float x, y, z; };

#define RTG_DEV __device__ __forceinline__

// ---------------------------------------------------------------- helpers
RTG_DEV float ieee_sqrtf(float x) { return __builtin_sqrtf(x); }   // IEEE sqrt (correctly rounded build)
// Correctly rounded f32 sqrt in f32 arithmetic (round 5): v_sqrt_f32 is within 1 ulp for x >= 2^-96, and of the
// candidates s - ulp, s, s + ulp the signs of the exact residuals x - (s - ulp) s and x - (s + ulp) s (one fma each)
// pick the correctly rounded one -- the sequence LLVM emits for a correctly rounded f32 sqrt.  +-0 comes out of the
// same sequence exactly (v_sqrt_f32(+-0) = +-0 and neither residual test moves it: quat_from_rotation_matrix clamps
// negative estimates to 0, so zeros are common there); x below 2^-96 (denormals, negatives) is scaled by 2^64 first
// (below).  No f64 instruction (round 4's v_sqrt_f64 + Newton form: three f64 ops and two quarter-rate f64
// transcendentals).  Proven equal to __builtin_sqrtf on all 2^32 inputs by tools/check_fastmath.hip [1] (run by
// tests/test_gpu_parity.py).
RTG_DEV float cr_sqrt(float x)
{
    // branch-free: x < 2^-96 (tiny and denormal positives; negatives and -0, which the scaling keeps negative / -0
    // and the sequence turns into NaN / -0) is scaled by 2^64 into the range where v_sqrt_f32 is within an ulp and
    // the result scaled back by 2^-32 (both exact: sqrt(2^-149 2^64) = 2^-42.5 and the result stays normal).  +-0,
    // inf and NaN come out of the sequence itself (v_sqrt_f32 returns them exactly; every residual test reads
    // false on them).  The branch it replaces was a call (the f64 form) at each of ~150 inlined sites of the side
    // kernel: each site's call set-up and call-clobbered registers cost more than the 4 instructions here.
    const bool tiny = x < 0x1p-96f;
    const float xs = tiny ? x * 0x1p64f : x;
    float s = __builtin_amdgcn_sqrtf(xs);
    const float sdn = __uint_as_float(__float_as_uint(s) - 1u), sup = __uint_as_float(__float_as_uint(s) + 1u);
    const float rdn = __builtin_fmaf(-sdn, s, xs), rup = __builtin_fmaf(-sup, s, xs);
    s = rdn <= 0.0f ? sdn : s;
    s = rup > 0.0f ? sup : s;
    return tiny ? s * 0x1p-32f : s;
}
// cr_sqrt for an argument that is "not tiny": x >= 2^-96, or +-0, +inf or NaN.  For such x cr_sqrt's `tiny` test
// selects the unscaled value both times (it reads true on +-0 too, but 0 * 2^64 = 0 and 0 * 2^-32 = 0 with the
// sign kept), so its five scaling instructions (compare, multiply, select; multiply, select) drop out and the rest
// is the same sequence: the same bits as cr_sqrt.  Only for call sites whose comment says why the argument is in
// that set; a positive argument below 2^-96 (denormals included) needs cr_sqrt.  A negative argument is a NaN either
// way (x 2^64 stays negative, v_sqrt_f32 of a negative is the same quiet NaN, and the 2^-32 product keeps it; no
// residual test moves a NaN), so a site whose argument is negative only where the result is a NaN in the reference
// too may use it (the exp-map read-out, below: its mask turns that NaN into +0).  tools/check_fdiv.hip checks it
// against __builtin_sqrtf on every bit pattern of the set, tools/check_fdiv1.hip [R] against cr_sqrt bit for bit,
// NaN patterns included, on 1 - w w for every f32 w.
RTG_DEV float cr_sqrt_nt(float x)
{
#if RTG_FIT_FAST_DIV_TU
    float s = __builtin_amdgcn_sqrtf(x);
    const float sdn = __uint_as_float(__float_as_uint(s) - 1u), sup = __uint_as_float(__float_as_uint(s) + 1u);
    const float rdn = __builtin_fmaf(-sdn, s, x), rup = __builtin_fmaf(-sup, s, x);
    s = rdn <= 0.0f ? sdn : s;
    s = rup > 0.0f ? sup : s;
    return s;
#else
    return cr_sqrt(x);
#endif
}
// Rounding test for an f64 approximation y of a value whose f32 rounding is wanted: true when the bits f32 rounding
// drops (29 of them, for an f32-normal |y|) are not within D f64 ulps of the midpoint 2^28, i.e. every value within
// D ulps of y rounds to (float)y.  An approximation with relative error <= 2^-k is within 2^(53-k) ulps.  Integer
// work only (v_and, v_sub, v_cmp).  0 and results below the f32 normal range read as not safe.
RTG_DEV bool f32_round_safe(double y, uint32_t D)
{
    const uint64_t b = (uint64_t)__double_as_longlong(y);
    const uint32_t lo = (uint32_t)b & 0x1FFFFFFFu;
    const uint32_t ex = (uint32_t)(b >> 52) & 0x7FFu;
    return ((lo - (0x10000000u - D)) > 2u * D) & (ex >= 1023u - 126u) & (ex <= 1023u + 127u);
}
RTG_DEV float acos_libm(float x) { return (float)::acos((double)x); }
// the rare-case call of cr_acos, out of line: inlined into the hot path, its registers raised the side kernel from
// 127 to 145 VGPRs (3 waves/SIMD instead of 4)
__device__ __attribute__((noinline)) float acos_libm_call(float x) { return acos_libm(x); }
// Correctly rounded f32 acos (round 5): torch.acos's value, rounded once.  acos x = pi/2 - sign(x) asin|x| for
// |x| <= 1/2 and 2 asin s (x > 0) / pi - 2 asin s (x < 0) with s = sqrt((1 - |x|) / 2) otherwise -- one instruction
// stream for both, asin s = s + s t P(t) with t = s^2 in [0, 1/4] (P: degree-9 minimax of (asin sqrt t - sqrt t) /
// t^1.5, error 2^-44 -> 2^-46 relative in asin), all in f64.  s comes from f32 seeds: s_hi = v_sqrt_f32(t), then
// s = s_hi + (t - s_hi^2) / (2 s_hi) with v_rcp_f32 (relative error <= 2^-46).  The result is within 2^-45 of acos
// x, i.e. 2^8 f64 ulps; f32_round_safe with D = 2^12 accepts it, otherwise (about 1 call in 2^16, and |x| > 1, NaN,
// x = +-1) the libm f64 acos runs behind one rare-case branch.  tools/check_fastmath.hip [6] proves it equal to
// (float)acos((double)x) for every f32 x.
RTG_DEV float acos_fast(float x, bool &ok)
{
    const float ax = __builtin_fabsf(x);
    const bool big = ax > 0.5f, neg = x < 0.0f;
    const float t32 = (1.0f - ax) * 0.5f;   // exact for ax in [1/2, 1]
    const float shi = __builtin_amdgcn_sqrtf(t32), rhi = __builtin_amdgcn_rcpf(shi);
    const double ad = (double)ax, sd = (double)shi;
    const double t = big ? (double)t32 : ad * ad;   // ad * ad is exact (24-bit operands)
    const double sb = __builtin_fma(__builtin_fma(-sd, sd, t), 0.5 * (double)rhi, sd);
    const double sv = big ? sb : ad;
    double p = 0.02812845967375316;
    p = __builtin_fma(p, t, -0.0031884549095405512);
    p = __builtin_fma(p, t, 0.0157919883306133);
    p = __builtin_fma(p, t, 0.013158578722490823);
    p = __builtin_fma(p, t, 0.01744580641234927);
    p = __builtin_fma(p, t, 0.02236569402301675);
    p = __builtin_fma(p, t, 0.03038220079156473);
    p = __builtin_fma(p, t, 0.04464285200108894);
    p = __builtin_fma(p, t, 0.07500000003992044);
    p = __builtin_fma(p, t, 0.16666666666661556);
    const double as = __builtin_fma(sv * t, p, sv);
    const double A = big ? (neg ? 3.141592653589793 : 0.0) : 1.5707963267948966;
    const double Bc = big ? (neg ? -2.0 : 2.0) : (neg ? 1.0 : -1.0);
    const double y = __builtin_fma(Bc, as, A);
    // x = +-1 (radians_between clamps its cosine to [-1, 1], so exactly parallel / antiparallel vectors give them):
    // acos is +0 / RN(pi), set here rather than through the rare-case branch
    const bool one = ax == 1.0f;
    ok = (f32_round_safe(y, 1u << 12) & (ax < 1.0f)) | one;
    return one ? (neg ? 3.14159274f : 0.0f) : (float)y;
}
// ------------------------------------------------ N-way leaf math (round 6; the only form since round 20)
// Each leaf function with a fast path and a rare exact path is ONE template over N elements: the fast paths of all N
// run first and the whole group shares ONE rare-case branch, behind which each element that declined takes its exact
// path.  A rare-case branch ends a basic block, and the scheduler does not move instructions across it: with a branch
// per element two independent chains (the two arms of a frame) could not interleave, ~17 branches per arm map.  The
// scalar name is the N = 1 call (arrays of one), so there is no second body to keep equal.
template <int N>
RTG_DEV void cr_acos_n(const float (&x)[N], float (&out)[N])
{
    bool ok[N], all = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        out[i] = acos_fast(x[i], ok[i]);
        all &= ok[i];
    }
    if (!(RTG_EXP_NO_RARE & 2) && __builtin_expect(!all, 0)) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!ok[i]) out[i] = acos_libm_call(x[i]);
    }
}
RTG_DEV float cr_acos(float x)
{
    const float a[1] = {x};
    float r[1];
    cr_acos_n<1>(a, r);
    return r[0];
}
RTG_DEV float cr_sin(float x) { return (float)::sin((double)x); }
RTG_DEV float cr_cos(float x) { return (float)::cos((double)x); }
// sin and cos of one argument, correctly rounded: fast shared-reduction path
// (rtg_crmath.h, exhaustively checked against glibc) with the libm f64 call as
// the exact fallback for the ~1-in-10^7 values the rounding test declines.
struct SC { float s, c; };
// the rare-case libm calls of cr_sincos, out of line (registers: see acos_libm_call)
__device__ __attribute__((noinline)) float sin_libm_call(double x) { return (float)::sin(x); }
__device__ __attribute__((noinline)) float cos_libm_call(double x) { return (float)::cos(x); }
template <int N>
RTG_DEV void cr_sincos_n(const double (&x)[N], SC (&out)[N])
{
    bool sok[N], cok[N], all = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const crm::SinCos r = crm::crm_sincos(x[i]);
        out[i] = SC{r.s, r.c};
        sok[i] = r.s_ok;
        cok[i] = r.c_ok;
        all &= r.s_ok & r.c_ok;
    }
    if (!(RTG_EXP_NO_RARE & 4) && __builtin_expect(!all, 0)) {   // one rare-case branch for every sine and cosine
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if (!sok[i]) out[i].s = sin_libm_call(x[i]);
            if (!cok[i]) out[i].c = cos_libm_call(x[i]);
        }
    }
}
RTG_DEV SC cr_sincos(double x)
{
    const double a[1] = {x};
    SC r[1];
    cr_sincos_n<1>(a, r);
    return r[0];
}
// k float divisions by one denominator n: RN(a/n) == (float)((double)a * RN(1/(double)n))
// for all f32 a, n.  (An f32 quotient is never within 2^-50 relative of an f32
// rounding midpoint, and the f64 product is within 2^-52; checked on 4.3e9
// random pairs incl. subnormals / zeros / infinities, tests/test_oracle_golden.py.)
// One f64 reciprocal replaces k correctly rounded f32 divide sequences.
// 1/n for k divisions by one denominator: v_rcp_f64 + two Newton steps, i.e. RN(1/n) to within an ulp even
// from a 14-bit estimate (the IEEE f64 divide sequence is twice as long).  0 / inf / NaN make the residual NaN;
// the raw v_rcp_f64 value (inf, 0, NaN) is then the IEEE answer.
struct Rcp {
    double r;
    float n;
};
RTG_DEV Rcp rcp64(float n)
{
    const double d = (double)n;
    const double r0 = __builtin_amdgcn_rcp(d);
    const double e0 = __builtin_fma(-d, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-d, r1, 1.0);
    return Rcp{e0 == e0 ? __builtin_fma(r1, e1, r1) : r0, n};
}
// RN(a/n) == (float)((double)a * 1/n) whenever the quotient is a normal f32: an f32 quotient is never within
// 2^-50 (relative) of an f32 midpoint and the f64 product is within 2^-52.  A subnormal quotient (absolute
// grid) takes the IEEE division; that branch is rare and divergent.  tools/check_fastmath.hip: 2^32 random
// pairs + all special-value pairs, 0 mismatches.
// K quotients by one denominator behind ONE rare-case branch: each is (float)(a_i * 1/n), and if any product is a
// nonzero subnormal, every quotient of the group takes the IEEE division -- identical to a branch per quotient (for a
// normal quotient the IEEE division equals the product, by the argument above), one branch instead of K.
template <int K>
RTG_DEV void mulr_k(const float (&a)[K], const Rcp &r, float (&q)[K])
{
    bool sub = false;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const double p = (double)a[i] * r.r;
        q[i] = (float)p;
        sub |= (__builtin_fabs(p) < 0x1p-126) & (p != 0.0);
    }
#if !RTG_EXP_MULR_NOBRANCH   // measurement knob: no subnormal-quotient branch (wrong on rare exact subnormal midpoints)
    if (!(RTG_EXP_NO_RARE & 8) && __builtin_expect(sub, 0)) {
#pragma unroll
        for (int i = 0; i < K; ++i) q[i] = a[i] / r.n;
    }
#endif
}
RTG_DEV float mulr(float a, const Rcp &r)
{
    const float n[1] = {a};
    float q[1];
    mulr_k<1>(n, r, q);
    return q[0];
}
RTG_DEV float clamp_lo(float v, float lo) { return v < lo ? lo : v; }          // NaN passes through
// n = max(RN32(sqrt(s)), lo) and its reciprocal for mulr -- the normalisation step every quat_unit / quat_normalize /
// axis normalisation takes (clamp(norm, 1e-9), then k divisions by it).  cr_sqrt + rcp64 issue three f64
// transcendentals (v_sqrt_f64, v_rcp_f64 in the sqrt correction, v_rcp_f64 for 1/n) on the dependent chain; this
// form issues ONE (v_rsq_f64): two coupled Goldschmidt steps refine sqrt(s) and 1/(2 sqrt(s)) together, the f32
// rounding of the first gives n, and two Newton steps from 2 * the second give 1/n.  s = 0, +inf, NaN, negative
// and a clamped n take the cr_sqrt + rcp64 path (rare, divergent).  tools/check_fastmath.hip [4] checks on the
// device that (n, r) are bitwise those of the cr_sqrt + rcp64 path for every f32 s (both lo used here).
struct NormRcp {
    float n;
    Rcp r;
};
// the fast path of sqrt_clamp_rcp; `ok` false where its value must be replaced by sqrt_clamp_rcp_exact's
RTG_DEV NormRcp sqrt_clamp_rcp_fast(float s, float lo, bool &ok)
{
    const double d = (double)s;
    const double y = __builtin_amdgcn_rsq(d);
    double g = d * y, h = 0.5 * y;
    double e = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, e, g);
    h = __builtin_fma(h, e, h);
    e = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, e, g);
    h = __builtin_fma(h, e, h);
    const float n = (float)g;
    const double dn = (double)n, r0 = h + h;
    const double e0 = __builtin_fma(-dn, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-dn, r1, 1.0);
    ok = (d > 0.0) & (d < __builtin_inf()) & (n >= lo);
    return NormRcp{n, Rcp{__builtin_fma(r1, e1, r1), n}};
}
RTG_DEV NormRcp sqrt_clamp_rcp_exact(float s, float lo)
{
    const float nc = clamp_lo(cr_sqrt(s), lo);
    return NormRcp{nc, rcp64(nc)};
}
template <int N>
RTG_DEV void sqrt_clamp_rcp_n(const float (&s)[N], float lo, NormRcp (&out)[N])
{
    // the fast path runs unconditionally (on s <= 0 / inf / NaN its values are discarded) and ONE rare-case branch
    // takes the cr_sqrt + rcp64 path for each s that is not a positive finite number or whose n needs the clamp
    bool ok[N], all = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        out[i] = sqrt_clamp_rcp_fast(s[i], lo, ok[i]);
        all &= ok[i];
    }
    if (!(RTG_EXP_NO_RARE & 16) && __builtin_expect(!all, 0)) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!ok[i]) out[i] = sqrt_clamp_rcp_exact(s[i], lo);
    }
}
RTG_DEV NormRcp sqrt_clamp_rcp(float s, float lo)
{
    const float a[1] = {s};
    NormRcp r[1];
    sqrt_clamp_rcp_n<1>(a, lo, r);
    return r[0];
}
// v_i * 1/n_i for N vectors of C components (V: 3, Q: 4), as mulr_k per vector: the products, and a vector with a
// nonzero subnormal product takes IEEE divisions for all its components.  mulr_products_n is the unconditional part
// (it returns whether any vector needs the divisions, `sub` says which); mulr_n adds the ONE rare-case branch.
RTG_DEV void comps_of(V v, float (&a)[3]) { a[0] = v.x; a[1] = v.y; a[2] = v.z; }
RTG_DEV void comps_of(Q v, float (&a)[4]) { a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
RTG_DEV V of_comps(const float (&a)[3]) { return V{a[0], a[1], a[2]}; }
RTG_DEV Q of_comps(const float (&a)[4]) { return Q{a[0], a[1], a[2], a[3]}; }
RTG_DEV V div_comps(V v, float n) { return V{v.x / n, v.y / n, v.z / n}; }
// four divisions out of line (registers: see acos_libm_call); returned by value
__device__ __attribute__((noinline)) Q div_q_call(Q v, float n) { return Q{v.x / n, v.y / n, v.z / n, v.w / n}; }
RTG_DEV Q div_comps(Q v, float n) { return div_q_call(v, n); }
template <typename T, int N>
RTG_DEV bool mulr_products_n(const T (&v)[N], const NormRcp (&r)[N], T (&out)[N], bool (&sub)[N])
{
    constexpr int C = sizeof(T) / sizeof(float);
    bool any = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float a[C], q[C];
        comps_of(v[i], a);
        sub[i] = false;
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const double p = (double)a[k] * r[i].r.r;
            q[k] = (float)p;
            sub[i] |= (__builtin_fabs(p) < 0x1p-126) & (p != 0.0);
        }
        out[i] = of_comps(q);
        any |= sub[i];
    }
    return any;
}
template <typename T, int N>
RTG_DEV void mulr_n(const T (&v)[N], const NormRcp (&r)[N], T (&out)[N])
{
    bool sub[N];
    const bool any = mulr_products_n(v, r, out, sub);
    if (!RTG_EXP_MULR_NOBRANCH && !(RTG_EXP_NO_RARE & 8) && __builtin_expect(any, 0)) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (sub[i]) out[i] = div_comps(v[i], r[i].r.n);
    }
}
template <typename T>
RTG_DEV T mulr_1(T v, const Rcp &r)
{
    const T a[1] = {v};
    const NormRcp n[1] = {NormRcp{r.n, r}};
    T q[1];
    mulr_n(a, n, q);
    return q[0];
}
RTG_DEV V mulr_v(V v, const Rcp &r) { return mulr_1(v, r); }
RTG_DEV Q mulr_q(Q v, const Rcp &r) { return mulr_1(v, r); }

RTG_DEV float tsign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }
RTG_DEV float clamp_lohi(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// glibc 2.35 float atanf (fdlibm s_atanf.c algorithm, decimal constants)
RTG_DEV float g_atanf(float x)
{
    const float atanhi0 = 4.6364760399e-01f, atanhi1 = 7.8539812565e-01f, atanhi2 = 9.8279368877e-01f,
                atanhi3 = 1.5707962513e+00f;
    const float atanlo0 = 5.0121582440e-09f, atanlo1 = 3.7748947079e-08f, atanlo2 = 3.4473217170e-08f,
                atanlo3 = 7.5497894159e-08f;
    const int32_t hx = __float_as_int(x);
    const int32_t ix = hx & 0x7fffffff;
    if (ix >= 0x4c000000) {
        if (ix > 0x7f800000) return x + x;
        return hx > 0 ? atanhi3 + atanlo3 : -atanhi3 - atanlo3;
    }
    int id;
    float hi = 0.0f, lo = 0.0f;
    if (ix < 0x3ee00000) {
        if (ix < 0x31000000) return x;
        id = -1;
    } else {
        x = fabsf(x);
        if (ix < 0x3f980000) {
            if (ix < 0x3f300000) { id = 0; x = (2.0f * x - 1.0f) / (2.0f + x); hi = atanhi0; lo = atanlo0; }
            else { id = 1; x = (x - 1.0f) / (x + 1.0f); hi = atanhi1; lo = atanlo1; }
        } else {
            if (ix < 0x401c0000) { id = 2; x = (x - 1.5f) / (1.0f + 1.5f * x); hi = atanhi2; lo = atanlo2; }
            else { id = 3; x = -1.0f / x; hi = atanhi3; lo = atanlo3; }
        }
    }
    const float z = x * x;
    const float w = z * z;
    const float s1 = z * (3.3333334327e-01f + w * (1.4285714924e-01f + w * (9.0908870101e-02f +
                     w * (6.6610731184e-02f + w * (4.9768779427e-02f + w * 1.6285819933e-02f)))));
    const float s2 = w * (-2.0000000298e-01f + w * (-1.1111110449e-01f + w * (-7.6918758452e-02f +
                     w * (-5.8335702866e-02f + w * -3.6531571299e-02f))));
    if (id < 0) return x - x * (s1 + s2);
    const float r = hi - ((x * (s1 + s2) - lo) - x);
    return hx < 0 ? -r : r;
}

// glibc 2.35 e_atan2f.c (torch.atan2 on <32-element tensors takes the scalar std::atan2 path)
RTG_DEV float g_atan2f(float y, float x)
{
    const float tiny = 1.0e-30f, pi_o_4 = 7.8539818525e-01f, pi_o_2 = 1.5707963705e+00f,
                pi = 3.1415927410e+00f, pi_lo = -8.7422776573e-08f;
    const int32_t hx = __float_as_int(x), hy = __float_as_int(y);
    const int32_t ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
    if (ix > 0x7f800000 || iy > 0x7f800000) return x + y;
    if (hx == 0x3f800000) return g_atanf(y);
    const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);
    if (iy == 0) {
        if (m <= 1) return y;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (ix == 0) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    if (ix == 0x7f800000) {
        if (iy == 0x7f800000) {
            if (m == 0) return pi_o_4 + tiny;
            if (m == 1) return -pi_o_4 - tiny;
            if (m == 2) return 3.0f * pi_o_4 + tiny;
            return -3.0f * pi_o_4 - tiny;
        }
        if (m == 0) return 0.0f;
        if (m == 1) return -0.0f;
        return m == 2 ? pi + tiny : -pi - tiny;
    }
    if (iy == 0x7f800000) return hy < 0 ? -pi_o_2 - tiny : pi_o_2 + tiny;
    const int32_t k = (iy - ix) >> 23;
    float z;
    if (k > 60) z = pi_o_2 + 0.5f * pi_lo;
    else if (hx < 0 && k < -60) z = 0.0f;
    else z = g_atanf(fabsf(y / x));
    if (m == 0) return z;
    if (m == 1) return -z;
    if (m == 2) return pi - (z - pi_lo);
    return (z - pi_lo) - pi;
}

// atan2f with the finite non-zero case branch-free (rtg_crmath.h); special
// operands take the branchy restatement above.
RTG_DEV float f_atan2f(float y, float x)
{
    return crm::crm_atan2f_regular(y, x) ? crm::crm_atan2f_sel(y, x) : g_atan2f(y, x);
}
RTG_DEV float normalize_angle(float a)   // rotation3d.py:582-584: atan2(sin a, cos a)
{
    const SC t = cr_sincos((double)a);
    return f_atan2f(t.s, t.c);
}

// ------------------------------------------------ quaternion algebra (rotation3d.py)
RTG_DEV Q qmul(Q a, Q b)   // :14-27, each component a left fold of four products
{
    Q r;
    r.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
    r.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
    r.y = ((a.w * b.y + a.y * b.w) + a.z * b.x) - a.x * b.z;
    r.z = ((a.w * b.z + a.z * b.w) + a.x * b.y) - a.y * b.x;
    return r;
}
RTG_DEV Q qconj(Q a) { return Q{-a.x, -a.y, -a.z, a.w}; }
RTG_DEV Q qident() { return Q{0.0f, 0.0f, 0.0f, 1.0f}; }

// ---- near-unit normalisation (round 6)
// Most quaternions the kinematics normalise are products of unit quaternions, or {e_ax sin, cos} from a correctly
// rounded pair: |q|^2 lands within a few f32 codes of 1.0f.  sqrt_clamp_rcp's (n, 1/n) for the 2K + 1 codes around
// 1.0f are a table, filled by the kernel with sqrt_clamp_rcp_exact itself (unit_tab_fill: one code per lane, while
// its loads are in flight), so a lookup returns exactly that function's values; a |q|^2 outside the table (a
// non-unit input row, NaN) takes the ordinary path.
constexpr int kUnitTabK = RTG_UNIT_TAB_K;
struct UnitEnt {
    double r;
    float n, pad;
};
RTG_DEV void unit_tab_fill(UnitEnt *tab, int t)   // t: the filling thread's index in a wave (0 .. 63)
{
    for (int e = t; e >= 0 && e <= 2 * kUnitTabK; e += 64) {
        const NormRcp n = sqrt_clamp_rcp_exact(__int_as_float(0x3F800000 - kUnitTabK + e), 1e-9f);
        tab[e] = UnitEnt{n.r.r, n.n, 0.0f};
    }
}
RTG_DEV bool unit_tab_index(float s, uint32_t &idx)
{
    idx = (uint32_t)(__float_as_int(s) - (0x3F800000 - kUnitTabK));
    const bool in = idx <= 2u * kUnitTabK;
    idx = in ? idx : 0u;
    return in;
}
// "Through the table or not" is the last argument `tab` of every function that normalises: NoTab (the default) is
// the ordinary path, a const UnitEnt * the table.  TabSel picks between the two at compile time.
struct NoTab {};
template <bool ON> struct TabSel {   // a table pointer where ON, NoTab elsewhere
    static RTG_DEV const UnitEnt *get(const UnitEnt *t) { return t; }
};
template <> struct TabSel<false> {
    static RTG_DEV NoTab get(const UnitEnt *) { return NoTab{}; }
};

// quat_pos (:92-98) of N quaternions and their |q|^2 (left fold)
template <int N>
RTG_DEV void quat_pos_norm2_n(const Q (&q0)[N], Q (&q)[N], float (&s)[N])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float f = 1.0f - 2.0f * (q0[i].w < 0.0f ? 1.0f : 0.0f);
        q[i] = Q{f * q0[i].x, f * q0[i].y, f * q0[i].z, f * q0[i].w};
        s[i] = ((q[i].x * q[i].x + q[i].y * q[i].y) + q[i].z * q[i].z) + q[i].w * q[i].w;
    }
}
template <int N>
RTG_DEV void qnormalize_n(const Q (&q0)[N], Q (&out)[N], NoTab = NoTab{})  // quat_unit(quat_pos(q)) :30-56,92-98
{
    Q q[N];
    float s[N];
    quat_pos_norm2_n<N>(q0, q, s);
    NormRcp r[N];
    sqrt_clamp_rcp_n<N>(s, 1e-9f, r);
    mulr_n(q, r, out);
}
RTG_DEV Q qnormalize(Q q, NoTab = NoTab{})
{
    const Q a[1] = {q};
    Q o[1];
    qnormalize_n<1>(a, o);
    return o[0];
}
// through the table: the same sign flip, sum, products and subnormal test, element by element; the ones off the
// table (or with a subnormal product) take the plain qnormalize, one rare-case branch per group
template <int N>
RTG_DEV void qnormalize_n(const Q (&q0)[N], Q (&out)[N], const UnitEnt *tab)
{
    Q q[N];
    float s[N];
    quat_pos_norm2_n<N>(q0, q, s);
    NormRcp r[N];
    bool in[N], sub[N], all = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        uint32_t idx;
        in[i] = unit_tab_index(s[i], idx);
        r[i] = NormRcp{tab[idx].n, Rcp{tab[idx].r, tab[idx].n}};
    }
    mulr_products_n(q, r, out, sub);
#pragma unroll
    for (int i = 0; i < N; ++i) all &= in[i] & !sub[i];
    if (__builtin_expect(!all, 0)) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!(in[i] & !sub[i])) out[i] = qnormalize(q0[i]);
    }
}
RTG_DEV Q qnormalize(Q q, const UnitEnt *tab)
{
    const Q a[1] = {q};
    Q o[1];
    qnormalize_n<1>(a, o, tab);
    return o[0];
}
template <typename Tab = NoTab>
RTG_DEV Q qmul_norm(Q a, Q b, Tab tab = Tab{}) { return qnormalize(qmul(a, b), tab); }
template <int N, typename Tab = NoTab>
RTG_DEV void qmul_norm_n(const Q (&a)[N], const Q (&b)[N], Q (&out)[N], Tab tab = Tab{})
{
    Q p[N];
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = qmul(a[i], b[i]);
    qnormalize_n<N>(p, out, tab);
}
RTG_DEV float qabs(Q q) { return cr_sqrt(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w); }   // :41-47
RTG_DEV Q qunit(Q q)                                                                                 // :50-56
{
    const Rcp r = sqrt_clamp_rcp(((q.x * q.x + q.y * q.y) + q.z * q.z) + q.w * q.w, 1e-9f).r;
    return mulr_q(q, r);
}
// quat_angle_axis (:230-240): angle = acos(clamp(2 w^2 - 1)), axis = xyz / max(|xyz|, 1e-9)
RTG_DEV Q qangle_axis_abs(Q q)
{
    const float s = clamp_lohi(2.0f * (q.w * q.w) - 1.0f, -1.0f, 1.0f);
    const Rcp r = sqrt_clamp_rcp((q.x * q.x + q.y * q.y) + q.z * q.z, 1e-9f).r;
    const V ax = mulr_v(V{q.x, q.y, q.z}, r);
    return Q{cr_acos(s), ax.x, ax.y, ax.z};
}

RTG_DEV V qrotate(Q q, V v)  // :205-211, two Hamilton products
{
    const Q r = qmul(qmul(q, Q{v.x, v.y, v.z, 0.0f}), qconj(q));
    return V{r.x, r.y, r.z};
}

RTG_DEV Q qfrom_angle_axis(float angle, V axis)  // :122-143
{
    const float theta = angle / 2.0f;
    // axis.norm(p=2, dim=-1) of a 3-vector: torch's fma chain (measured: 100 % vs 90 % for the plain left fold)
    const Rcp r = sqrt_clamp_rcp(__builtin_fmaf(axis.z, axis.z, __builtin_fmaf(axis.y, axis.y, axis.x * axis.x)),
                                 1e-9f).r;
    const V u = mulr_v(axis, r);
    const float ax = u.x, ay = u.y, az = u.z;
    const SC t = cr_sincos((double)theta);
    const float s = t.s, c = t.c;
    return qnormalize(Q{ax * s, ay * s, az * s, c});
}
// quat_from_angle_axis about an exact unit axis (ex / ey / ez): the axis normalisation is the identity
// (sqrt(1) = 1, +0 and 1 times RN(1/1) stay +0 and 1), so it is skipped -- the same bits.
template <int N, typename Tab = NoTab>
RTG_DEV void qfrom_angle_unit_axis_n(const float (&angle)[N], const V (&axis)[N], Q (&out)[N], Tab tab = Tab{})
{
    double th[N];
#pragma unroll
    for (int i = 0; i < N; ++i) th[i] = (double)(angle[i] / 2.0f);
    SC t[N];
    cr_sincos_n<N>(th, t);
    Q q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) q[i] = Q{axis[i].x * t[i].s, axis[i].y * t[i].s, axis[i].z * t[i].s, t[i].c};
    qnormalize_n<N>(q, out, tab);
}
template <typename Tab = NoTab>
RTG_DEV Q qfrom_angle_unit_axis(float angle, V axis, Tab tab = Tab{})
{
    const float a[1] = {angle};
    const V ax[1] = {axis};
    Q q[1];
    qfrom_angle_unit_axis_n<1>(a, ax, q, tab);
    return q[0];
}

template <typename Tab = NoTab>
RTG_DEV Q qfrom_rotmat(const float m[9], Tab tab = Tab{})  // :146-193 (the four overlapping branches, in order)
{
    const float d0 = m[0], d1 = m[4], d2 = m[8];
    float w = cr_sqrt(clamp_lo((((d0 + d1) + d2) + 1.0f) / 4.0f, 0.0f));
    float x = cr_sqrt(clamp_lo((((d0 - d1) - d2) + 1.0f) / 4.0f, 0.0f));
    float y = cr_sqrt(clamp_lo((((-d0 + d1) - d2) + 1.0f) / 4.0f, 0.0f));
    float z = cr_sqrt(clamp_lo((((-d0 - d1) + d2) + 1.0f) / 4.0f, 0.0f));
    if (w >= x && w >= y && w >= z) {
        x *= tsign(m[7] - m[5]);
        y *= tsign(m[2] - m[6]);
        z *= tsign(m[3] - m[1]);
    }
    if (x >= w && x >= y && x >= z) {
        w *= tsign(m[7] - m[5]);
        y *= tsign(m[3] + m[1]);
        z *= tsign(m[2] + m[6]);
    }
    if (y >= w && y >= x && y >= z) {
        w *= tsign(m[2] - m[6]);
        x *= tsign(m[3] + m[1]);
        z *= tsign(m[7] + m[5]);
    }
    if (z >= w && z >= x && z >= y) {
        w *= tsign(m[3] - m[1]);
        x *= tsign(m[6] + m[2]);
        y *= tsign(m[7] + m[5]);
    }
    return qnormalize(Q{x, y, z, w}, tab);
}

// quat_to_angle_axis + angle_axis_to_exp_map (:587-627), returns the 3 exp-map components
RTG_DEV V qexp_map(Q q)
{
    const float sin_theta = cr_sqrt(1.0f - q.w * q.w);
    float angle = 2.0f * cr_acos(q.w);
    angle = normalize_angle(angle);   // normalize_angle :582-584
    const bool mask = fabsf(sin_theta) > 1e-5f;
    const float a = mask ? angle : 0.0f;
    const float ax = mask ? q.x / sin_theta : 0.0f;
    const float ay = mask ? q.y / sin_theta : 0.0f;
    const float az = mask ? q.z / sin_theta : 1.0f;
    return V{a * ax, a * ay, a * az};
}
// quat_to_angle_axis (:587-608) as [angle, axis]
RTG_DEV Q qangle_axis(Q q)
{
    const float sin_theta = cr_sqrt(1.0f - q.w * q.w);
    float angle = 2.0f * cr_acos(q.w);
    angle = normalize_angle(angle);
    const bool mask = fabsf(sin_theta) > 1e-5f;
    const Rcp r = rcp64(sin_theta);
    const V u = mulr_v(V{q.x, q.y, q.z}, r);
    return Q{mask ? angle : 0.0f, mask ? u.x : 0.0f, mask ? u.y : 0.0f, mask ? u.z : 1.0f};
}
RTG_DEV float qexp_component(Q q, int k)
{
    const V e = qexp_map(q);
    return k == 0 ? e.x : (k == 1 ? e.y : e.z);
}

// ------------------------------------------------ exp-map angle table
// The angle of quat_to_angle_axis (:595-597) is R(w) = normalize_angle(2 acos w) = atan2f(RN sin A, RN cos A)
// with A = 2 RN(acos w): glibc atan2f is not correctly rounded, so R has no closed form.  For w in [0.25, 1) --
// joint angles below 151 degrees -- R(w) is stored as a short move from a cheap f32 estimate P(w) =
// 4 asin(sqrt((1 - w) / 2)) (v_sqrt_f32 and a degree-6 fma polynomial, within 3 ulps of R): the 3-bit code c in
// 1..7 means R = P + (c - 4) ulps, 0 means "not tabulated" (exact path).  2^24 entries, 10 per 32-bit word, in
// 6.7 MiB (4-bit codes, 8 per word in 8 MiB, measured no faster), built on the device by the exact path
// itself (ang_tab_code, k_build_ang_tab) with the same P.  qexp_component_tab thus skips acos, sincos and
// atan2f (290 of the 330 instructions of an exp-map); w outside the table or a code-0 entry takes the exact
// path.  tools/check_fastmath.hip checks qexp_component_tab == qexp_component for every f32 w.
constexpr uint32_t kAngTabLo = 0x3e800000u;                     // bits of 0.25f
constexpr uint32_t kAngTabEntries = 0x3f800000u - kAngTabLo;    // up to 1.0f (exclusive): 2^24
constexpr uint32_t kAngTabBits = 3;                             // moves -3..3
constexpr uint32_t kAngTabPer = 10u;                            // codes per 32-bit word
constexpr uint32_t kAngTabWords = (kAngTabEntries + kAngTabPer - 1) / kAngTabPer;
constexpr uint32_t kAngTabBias = 1u << (kAngTabBits - 1);      // code = move + bias; code 0 = not tabulated
RTG_DEV uint32_t ang_tab_word(uint32_t i) { return __umulhi(i, 0xCCCCCCCDu) >> 3; }   // i / 10
RTG_DEV float exp_angle_estimate(float w)
{
    const float t2 = (1.0f - w) * 0.5f;
    const float t = __builtin_amdgcn_sqrtf(t2);
    float p = __builtin_fmaf(0.04965998747593211f, t2, -0.005969297163659217f);
    p = __builtin_fmaf(p, t2, 0.029188122223620813f);
    p = __builtin_fmaf(p, t2, 0.02938421651028137f);
    p = __builtin_fmaf(p, t2, 0.0447135443846629f);
    p = __builtin_fmaf(p, t2, 0.07499796602478857f);
    p = __builtin_fmaf(p, t2, 0.1666666806527845f);
    return 4.0f * __builtin_fmaf(t, t2 * p, t);
}
RTG_DEV uint32_t ang_tab_code(float w)
{
    const float R = normalize_angle(2.0f * cr_acos(w));
    const float P = exp_angle_estimate(w);
    if (!(R > 0.0f) || !(P > 0.0f) || !(R < 4.0f) || !(P < 4.0f)) return 0u;
    const int32_t d = (int32_t)__float_as_uint(R) - (int32_t)__float_as_uint(P);
    const int32_t lim = (int32_t)kAngTabBias - 1;
    return (d >= -lim && d <= lim) ? (uint32_t)(d + (int32_t)kAngTabBias) : 0u;
}
// word wd of the table: the codes of entries wd * kAngTabPer ... (k_build_ang_tab, tools/check_fastmath.hip)
RTG_DEV uint32_t ang_tab_build_word(uint32_t wd)
{
    uint32_t word = 0;
    for (uint32_t e = 0; e < kAngTabPer; ++e) {
        const uint32_t i = wd * kAngTabPer + e;
        if (i < kAngTabEntries) word |= ang_tab_code(__uint_as_float(kAngTabLo + i)) << (kAngTabBits * e);
    }
    return word;
}
// quat_to_exp_map(q)[k] given only w = q.w and qk = q[k]: for |sin_theta| <= 1e-5 the reference's product is
// 0 * (0 or 1) = +0 whatever k is, so the component index itself is not needed.
// sin_theta's argument x = RN(1 - RN(w w)) is never tiny (round 18), so cr_sqrt_nt returns cr_sqrt's bits: for
// |w| <= 1, RN(w w) is an f32 in [0, 1], so x is 0 (w = +-1) or at least 1 - (1 - 2^-24) = 2^-24; for |w| > 1,
// RN(w w) >= 1 + 2^-23 and x is negative, which v_sqrt_f32 turns into the same NaN scaled or not; a NaN w is a NaN
// either way.  tools/check_fdiv1.hip [R] compares the two and __builtin_sqrtf on every f32 w.
RTG_DEV float exp_dof_tab(float w, float qk, const uint32_t *__restrict__ tab)
{
    const uint32_t i = __float_as_uint(w) - kAngTabLo;
    const bool in = i < kAngTabEntries;
#if RTG_EXP_NO_TABLE   // measurement knob (tools/build_variants.sh): no table traffic, wrong angles
    const uint32_t wd = ang_tab_word(i);
    const uint32_t word = 0x24924924u + 0u * tab[0];
#else
    const uint32_t wd = ang_tab_word(i);
    const uint32_t word = tab[in ? wd : 0u];
#endif
    const float sin_theta = cr_sqrt_nt(1.0f - w * w);   // never tiny: see exp_dof_tab
    const bool mask = fabsf(sin_theta) > 1e-5f;
    const float P = exp_angle_estimate(w);
    const uint32_t code = in ? (word >> ((i - wd * kAngTabPer) * kAngTabBits)) & ((1u << kAngTabBits) - 1u) : 0u;
    float angle = __uint_as_float(__float_as_uint(P) + code - kAngTabBias);
    if (__builtin_expect(mask && code == 0u, 0)) angle = normalize_angle(2.0f * cr_acos(w));
    return mask ? angle * (qk / sin_theta) : 0.0f;
}
// exp_dof_tab split for a batch of read-outs that shares ONE rare-case branch (Emit::finalize): the table angle
// and whether this w needs the exact path; then exp_dof_finish.  Same operations, same values as exp_dof_tab.
struct ExpDof {
    float angle, sin_theta;
    bool mask, exact;
};
// the table word a read-out of w needs (word 0 when w is outside the table: its code is not used)
RTG_DEV uint32_t ang_tab_word_of(float w)
{
    const uint32_t i = __float_as_uint(w) - kAngTabLo;
    return i < kAngTabEntries ? ang_tab_word(i) : 0u;
}
RTG_DEV ExpDof exp_dof_word_part(float w, uint32_t word);
RTG_DEV ExpDof exp_dof_table_part(float w, const uint32_t *__restrict__ tab)
{
#if RTG_EXP_NO_TABLE
    const uint32_t word = 0x24924924u + 0u * tab[0];
#else
    const uint32_t word = tab[ang_tab_word_of(w)];
#endif
    return exp_dof_word_part(w, word);
}
// the read-out of w from its table word (loaded by the caller: exp_dof_table_part, or early into LDS, Emit::wd)
RTG_DEV ExpDof exp_dof_word_part(float w, uint32_t word)
{
    const uint32_t i = __float_as_uint(w) - kAngTabLo;
    const bool in = i < kAngTabEntries;
    const uint32_t wd = ang_tab_word(i);
#if RTG_EXP_NO_TABLE
    word = 0x24924924u;
#endif
    const float sin_theta = cr_sqrt_nt(1.0f - w * w);   // never tiny: see exp_dof_tab
    const bool mask = fabsf(sin_theta) > 1e-5f;
    const float P = exp_angle_estimate(w);
    const uint32_t code = in ? (word >> ((i - wd * kAngTabPer) * kAngTabBits)) & ((1u << kAngTabBits) - 1u) : 0u;
    return ExpDof{__uint_as_float(__float_as_uint(P) + code - kAngTabBias), sin_theta, mask, mask && code == 0u};
}
// Round 22: the quotient runs bare (fdiv1, region [N]): where mask holds sin_theta
// lies in (1e-5, 1], inside the window, and the numerator's test joins the batch's rare-case word (exp_dof_redo), whose
// exact path divides as the compiler does.  Where mask fails the quotient is not read.
RTG_DEV float fdiv1(float a, float b);   // with the Kabsch fits' divisions below
RTG_DEV float exp_dof_finish(const ExpDof &e, float qk) { return e.mask ? e.angle * fdiv1(qk, e.sin_theta) : 0.0f; }
// whether the read-out is to be redone on the exact path: the table says so, or qk is outside [2^-76, 2^47] (zeros,
// -0 among them, NaN and inf included)
RTG_DEV bool exp_dof_redo(const ExpDof &e, float qk)
{
    const float a = fabsf(qk);
    return e.exact | (e.mask & !((a >= 0x1p-76f) & (a <= 0x1p47f)));
}
// the exact path of one read-out whose mask holds (w outside the table or a code-0 entry), out of line
__device__ __attribute__((noinline)) float exp_dof_exact(float w, float qk)
{
    const float angle = normalize_angle(2.0f * cr_acos(w));
    return angle * (qk / cr_sqrt_nt(1.0f - w * w));   // never tiny: see exp_dof_tab
}
RTG_DEV float qexp_component_tab(Q q, int k, const uint32_t *__restrict__ tab)
{
    return exp_dof_tab(q.w, k == 0 ? q.x : (k == 1 ? q.y : q.z), tab);
}

// ------------------------------------------------ vectors (transform3d.py)
RTG_DEV float dot3(V a, V b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }          // torch.dot
RTG_DEV float lnorm3(V a)                                                              // torch.linalg.norm
{
    return cr_sqrt(__builtin_fmaf(a.z, a.z, __builtin_fmaf(a.y, a.y, a.x * a.x)));
}
RTG_DEV V cross3(V a, V b)                                                             // torch.cross
{
    return V{__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)),
             __builtin_fmaf(a.x, b.y, -(a.y * b.x))};
}
RTG_DEV V vsub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
RTG_DEV V vdiv(V a, float s)
{
    const Rcp r = rcp64(s);
    return mulr_v(a, r);
}
RTG_DEV V vmul(V a, float s) { return V{s * a.x, s * a.y, s * a.z}; }
// v / torch.linalg.norm(v): vdiv(v, lnorm3(v)) through one sqrt_clamp_rcp (lo = 0 clamps nothing), N vectors
template <int N>
RTG_DEV void vunit_n(const V (&a)[N], V (&u)[N])
{
    float s[N];
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = __builtin_fmaf(a[i].z, a[i].z, __builtin_fmaf(a[i].y, a[i].y, a[i].x * a[i].x));
    NormRcp r[N];
    sqrt_clamp_rcp_n<N>(s, 0.0f, r);
    mulr_n(a, r, u);
}

RTG_DEV V proj_in_plane(V v, V n)  // :61-75
{
    const float nn = lnorm3(n);
    return vsub(v, vmul(n, dot3(v, n) / (nn * nn)));
}

// the three unit vectors through one vunit_n (one rare-case branch instead of three)
RTG_DEV float radians_between(V v1, V v2, V n)  // :77-100
{
    const V in[3] = {v1, v2, n};
    V u[3];
    vunit_n<3>(in, u);
    const float c = clamp_lohi(dot3(u[0], u[1]), -1.0f, 1.0f);
    return cr_acos(c) * tsign(dot3(u[2], cross3(u[0], u[1])));
}

// ------------------------------------------------ the rest of the rotation3d / transform3d surface
// (not on the solver path; the elementwise ops 18-31 of rtg_quat_op_f32).  torch's norm(dim=-1) of a 3-vector is
// the fma chain of lnorm3, torch.sum over 4 a left fold, x**2 = x*x, atan2 on small tensors glibc's atan2f.

// exp_map_to_angle_axis (rotation3d.py:629-646) as [angle, axis]
RTG_DEV Q exp_map_angle_axis(V e)
{
    const NormRcp nr = sqrt_clamp_rcp(__builtin_fmaf(e.z, e.z, __builtin_fmaf(e.y, e.y, e.x * e.x)), 0.0f);
    const float n = nr.n;
    const Rcp r = nr.r;
    const float a = normalize_angle(n);
    const bool mask = fabsf(a) > 1e-5f;
    const V u = mulr_v(e, r);
    return Q{mask ? a : 0.0f, mask ? u.x : 0.0f, mask ? u.y : 0.0f, mask ? u.z : 1.0f};
}
// quat_slerp (transform3d.py:152-174), t per row
RTG_DEV Q qslerp(Q q0, Q q1, float t)
{
    float ch = ((q0.x * q1.x + q0.y * q1.y) + q0.z * q1.z) + q0.w * q1.w;
    if (ch < 0.0f) q1 = Q{-q1.x, -q1.y, -q1.z, -q1.w};
    ch = fabsf(ch);
    const float half = cr_acos(ch);
    const float sh = cr_sqrt(1.0f - ch * ch);
    const float ra = cr_sin((1.0f - t) * half) / sh;
    const float rb = cr_sin(t * half) / sh;
    if (fabsf(ch) >= 1.0f) return q0;
    if (fabsf(sh) < 0.001f)
        return Q{0.5f * q0.x + 0.5f * q1.x, 0.5f * q0.y + 0.5f * q1.y, 0.5f * q0.z + 0.5f * q1.z, 0.5f * q0.w + 0.5f * q1.w};
    return Q{ra * q0.x + rb * q1.x, ra * q0.y + rb * q1.y, ra * q0.z + rb * q1.z, ra * q0.w + rb * q1.w};
}
// rot_matrix_det (rotation3d.py:338-350), m row-major
RTG_DEV float rotmat_det(const float m[9])
{
    const float t1 = m[0] * (m[4] * m[8] - m[5] * m[7]);
    const float t2 = m[1] * (m[3] * m[8] - m[5] * m[6]);
    const float t3 = m[2] * (m[3] * m[7] - m[4] * m[6]);
    return (t1 - t2) + t3;
}
// rot_matrix_from_quaternion (rotation3d.py:398-427): [i, j, k, r] = [x, y, z, w], row-major out
RTG_DEV void rotmat_from_quat(Q q, float o[9])
{
    const float i = q.x, j = q.y, k = q.z, r = q.w;
    const float two_s = 2.0f / (((i * i + j * j) + k * k) + r * r);
    o[0] = 1.0f - two_s * (j * j + k * k);
    o[1] = two_s * (i * j - k * r);
    o[2] = two_s * (i * k + j * r);
    o[3] = two_s * (i * j + k * r);
    o[4] = 1.0f - two_s * (i * i + k * k);
    o[5] = two_s * (j * k - i * r);
    o[6] = two_s * (i * k - j * r);
    o[7] = two_s * (j * k + i * r);
    o[8] = 1.0f - two_s * (i * i + j * j);
}
// extract_rotation_along_axis (rotation3d.py:534-556) / the angles of project_quat_to_axis_* (:479-530)
RTG_DEV float axis_angle_of(Q q, int axis)
{
    if (axis == 0) return g_atan2f(2.0f * (q.w * q.x + q.y * q.z), 1.0f - 2.0f * (q.x * q.x + q.z * q.z));
    if (axis == 1) return g_atan2f(2.0f * (q.w * q.y + q.x * q.z), 1.0f - 2.0f * (q.y * q.y + q.z * q.z));
    return g_atan2f(2.0f * (q.w * q.z + q.x * q.y), 1.0f - 2.0f * (q.z * q.z + q.y * q.y));
}
// [sin(a/2) e_axis, cos(a/2)], unnormalised (the new_q of project_quat_to_axis_*)
RTG_DEV Q axis_half_quat(int axis, float a)
{
    const float h = a / 2.0f;
    const float s = cr_sin(h), c = cr_cos(h);
    return Q{axis == 0 ? s : 0.0f, axis == 1 ? s : 0.0f, axis == 2 ? s : 0.0f, c};
}

// ------------------------------------------------ Kabsch: torch.linalg.svd as MKL sgesdd computes it
// transform3d.py:40-45 runs torch.linalg.svd on one (1,3,3) float32 matrix, i.e. oneMKL 2024.2 SGESDD(JOBZ='A').
// For 3x3 that is SGEBD2 -> SBDSDC('U','I') -> SLASDQ -> SBDSQR -> SORMBR('Q') on U / SORMBR('P') on VT.  Each
// routine follows the published LAPACK algorithm; the FMA placement inside MKL's BLAS kernels was measured stage
// by stage against MKL's own entry points (tools/mkl_sgesdd_probe.py) and matches bit for bit.  The
// oracle (oracle/rtg_oracle.c, la_gesdd3) restates the same routines independently.  All divisions / square
// roots are IEEE-exact (fdiv = the compiler's IEEE f32 division; quotients by one denominator fdiv_n; cr_sqrt / cr_sqrt_nt).  Matrices are column-major: a[r + 3 c].
RTG_DEV float fdiv(float a, float b)
{
    return a / b;   // the compiler's IEEE f32 division sequence (measured 6 % faster here than rcp64 + mulr)
}
RTG_DEV float la_sqrt(float x)
{
    return cr_sqrt(x);
}
RTG_DEV float la_sqrt_nt(float x) { return cr_sqrt_nt(x); }   // the argument cannot be tiny: see cr_sqrt_nt, and say why
// ---- N IEEE f32 quotients a_i / b by one denominator (round 13).  The compiler's division is, per quotient,
//   bs = v_div_scale(b), as = v_div_scale(a);  y = v_rcp_f32(bs);  y = fma(fma(-bs, y, 1), y, y);
//   q = as * y;  q = fma(fma(-bs, q, as), y, q);  q = v_div_fmas(fma(-bs, q, as), y, q);  v_div_fixup(q, b, a)
// and it rebuilds all of it for every quotient, the reciprocal included, because v_div_scale reads the numerator.
// Inside the window below nothing is scaled and nothing fixed up, so the sequence is plain f32 arithmetic whose
// reciprocal part (three VALU, the one transcendental) depends on b alone: fdiv_n computes it once and runs the
// quotient instructions per numerator -- the same instructions on the same operands, hence the same bits (five of
// them in the compiler's sequence; three since round 18, see fdiv_n_bare).
//
// The window: |b| and every |a_i| in [2^-47, 2^47] (kDivLo, kDivHi; la_lartg passes its own test, see there).  By
// the ISA's definition v_div_scale_f32 returns its operand unscaled and VCC = 0 unless one of: an operand is 0 or
// NaN; exponent(a) - exponent(b) >= 96; b is denormal; 1 / b is denormal (|b| > 2^126); a / b is denormal
// (exponent(a) - exponent(b) <= -126 or so); exponent(a) <= 23 (|a| < 2^-103).  In the window the exponents differ
// by at most 94 and each lies in [-47, 47], so none holds; with VCC = 0 v_div_fmas is an FMA.  v_div_fixup changes
// q only for 0 / inf / NaN operands, an exponent difference below -150 or an infinite q, none of which can occur:
// |a / b| lies in [2^-94, 2^94].  47 is the widest power of two for which the exponent difference stays under 96;
// SGESDD's rescaling holds the fitted matrix inside [2^-40, 2^40], so ordinary fits stay well inside.  A zero
// numerator fails the guard (the bare sequence would turn -0 / b into +0), as do inf and NaN (every comparison
// reads false).  A lane outside the window sends its whole group through a_i / b behind ONE rare-case branch
// (N-way, as mulr_k).  tools/check_fdiv.hip (tests/test_gpu_fdiv.py) checks it on the device against a / b.
constexpr float kDivLo = 0x1p-47f, kDivHi = 0x1p47f;
RTG_DEV bool fdiv_in_window(float x)
{
    const float ax = fabsf(x);
    return (ax >= kDivLo) & (ax <= kDivHi);
}
//
// One residual correction (round 18, RTG_FDIV_CORRECTIONS = 1).  The compiler's second correction never moves the
// quotient inside the window: after the first, q already is RN(a / b).  Proved by exhaustion, not by an error bound
// (the bound is too close: the refined y is within 2^-24 or so of 1 / b, the corrected quotient within about 2^-47
// of a / b relatively, and a quotient of two 24-bit mantissas can lie that close to a rounding boundary).  In the
// window every operation of the sequence is ONE rounding of an exact expression in operands that scale with a and
// b: y with 2^-k for b 2^k (v_rcp_f32 itself does, checked for every mantissa and every k of the window), t and q
// with 2^(j-k) for a 2^j, the residual a - b t (exact inside the fma; zero or at least 2^-46 |a| / 4 >= 2^-96, so
// never subnormal) with 2^j, and fma(-b, y, 1) not at all; RN is sign-symmetric.  So the sequence commutes with
// powers of two and signs, as RN(a / b) does, and agreement on every mantissa pair a, b in [1, 2) -- 2^46 pairs,
// tools/check_fdiv1.hip `exhaustive`, 0 mismatches, profiles/r18/check_fdiv1.log -- is agreement on the whole window.
// tests/test_gpu_fdiv_one_correction.py runs the tool's sampled form.  2 rebuilds the compiler's sequence.
// the bare sequence: a_i / b only where b and a_i are in the window (the caller tests that and redoes the rest)
template <int N>
RTG_DEV void fdiv_n_bare(const float (&a)[N], float b, float (&q)[N])
{
    float y = __builtin_amdgcn_rcpf(b);
    y = __builtin_fmaf(__builtin_fmaf(-b, y, 1.0f), y, y);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float t = a[i] * y;
#pragma unroll
        for (int k = 0; k < RTG_FDIV_CORRECTIONS; ++k) t = __builtin_fmaf(__builtin_fmaf(-b, t, a[i]), y, t);
        q[i] = t;
    }
}
template <int N>
RTG_DEV void fdiv_n(const float (&a)[N], float b, float (&q)[N])
{
#if RTG_FIT_FAST_DIV_TU
    bool ok = fdiv_in_window(b);
#pragma unroll
    for (int i = 0; i < N; ++i) ok &= fdiv_in_window(a[i]);
    fdiv_n_bare<N>(a, b, q);
    if (__builtin_expect(!ok, 0)) {
#pragma unroll
        for (int i = 0; i < N; ++i) q[i] = a[i] / b;
    }
#else
#pragma unroll
    for (int i = 0; i < N; ++i) q[i] = a[i] / b;
#endif
}
RTG_DEV float la_sign(float a, float b) { return __builtin_copysignf(fabsf(a), b); }   // Fortran SIGN
// ---- ONE IEEE f32 quotient through the bare sequence (round 22): fdiv1(a, b) is fdiv_n_bare<1>, RN(a / b) wherever
// every step of it is one rounding in the normal range -- the scale argument above, which needs nothing of
// v_div_scale's conditions except that they describe the compiler's sequence and not this one (both are RN(a / b)
// there); they hold anyway in each region.  The caller owns the guard, and pays for it per GROUP of quotients:
//   [W] the symmetric window: |a|, |b| in [2^-47, 2^47] (fdiv_n's).
//   [N] narrow denominator, wide numerator: |b| in [2^-47, 2^47], |a| in [2^-76, 2^47] (kNumLo, kDivHi).  Below
//       the window the numerator meets three edges: |a| >= 2^-103 (v_div_scale's last condition) and
//       exponent(a) - exponent(b) > -126, i.e. a / b normal (its fifth), both implied by |a| >= 2^-78 under
//       |b| <= 2^47; and the residual a - b t, a multiple of ulp(b) ulp(t) >= 2^-48 |a|, normal: |a| >= 2^-78 again.
//       kNumLo = 2^-76 keeps two binades of margin.  y, fma(-b, y, 1) are as in [W]; t and q are at least 2^-124.
//   [C] a constant denominator c in [1, 8): [N] with the wider numerator range [2^-76, 2^94], since the exponent
//       difference stays under 96 and the quotient under 2^95 (fdiv1_const: the refined reciprocal is a constant too).
// A numerator of +0 gives +0 through the bare sequence (t = 0, the residual 0), which is RN(0 / b) for b > 0; -0
// would come out +0, so a zero numerator is admitted only where it is an absolute value or b's sign is its own.
// NaN in, NaN out (either operand), as a / b; +-inf must fail the guard (inf y - inf).  tools/check_fdiv1.hip
// `single` checks each region's edges on the device against a / b.
constexpr float kNumLo = 0x1p-76f;
RTG_DEV float fdiv1(float a, float b)
{
    const float num[1] = {a};
    float q[1];
    fdiv_n_bare<1>(num, b, q);
    return q[0];
}
RTG_DEV bool fdiv1_in_n(float a, float b)   // region [N] (which contains [W])
{
    const float aa = fabsf(a);
    return fdiv_in_window(b) & (aa >= kNumLo) & (aa <= kDivHi);
}
constexpr float kConstNumHi = 0x1p94f;
RTG_DEV bool fdiv1_in_c(float a)            // region [C]'s numerators
{
    const float aa = fabsf(a);
    return (aa >= kNumLo) & (aa <= kConstNumHi);
}
// a / c for the constant c in [1, 8) with y = the refined reciprocal of c (RN(1 / c) where that is its own
// refinement), on region [C]'s numerators
RTG_DEV float fdiv1_const(float a, float c, float y)
{
    const float t = a * y;
    return __builtin_fmaf(__builtin_fmaf(-c, t, a), y, t);
}
// a / b as the build divides it behind a group's guard: the bare sequence (the guard holds) or the compiler's
template <bool BARE>
RTG_DEV float fdiv_g(float a, float b)
{
    if constexpr (BARE) return fdiv1(a, b);
    else return a / b;
}
RTG_DEV float la_lapy2(float x, float y)                                                 // SLAPY2
{
    const float xa = fabsf(x), ya = fabsf(y);
    const float w = fmaxf(xa, ya), z = fminf(xa, ya);
    const float r = fdiv(z, w);
    return z == 0.0f ? w : w * la_sqrt_nt(1.0f + r * r);   // 1 + r^2 >= 1 (or NaN): not tiny
}
// SLAPY2 for w = max(|x|, |y|) in [2^-47, 2^47] and z = min(|x|, |y|) anything from +0 up: z >= 2^-76 is region [N];
// below it z / w < 2^-29 and the bare sequence returns at most 2 z / w (t = RN(z y), a residual of at most 2 z), so
// 1 + r^2 rounds to 1 either way and the value is w, as SLAPY2's.  z = 0 is selected away as before.
RTG_DEV float la_lapy2_bare(float xa, float ya)   // xa = |x|, ya = |y|
{
    const float w = fmaxf(xa, ya), z = fminf(xa, ya);
    const float r = fdiv1(z, w);
    return z == 0.0f ? w : w * la_sqrt_nt(1.0f + r * r);
}
// SLARFG(n, alpha, x): n = 3 (x = x0, x1) or n = 2 (x = x0); returns tau, updates alpha (= beta) and x
template <int NX>
RTG_DEV float la_larfg_ieee(float &alpha, float &x0, float &x1)
{
    const float safmin = 1.17549435e-38f / 5.96046448e-08f, rsafmn = 1.0f / safmin;
    float xn = NX == 1 ? fabsf(x0) : la_lapy2(x0, x1);
    float beta = -__builtin_copysignf(la_lapy2(alpha, xn), alpha);   // discarded when xn == 0
    int knt = 0;
    if (__builtin_expect((xn == 0.0f) | (fabsf(beta) < safmin), 0)) {   // ONE rare-case branch for both cases
        if (xn == 0.0f) return 0.0f;
        do {
            ++knt;
            x0 *= rsafmn;
            if (NX == 2) x1 *= rsafmn;
            beta *= rsafmn;
            alpha *= rsafmn;
        } while (fabsf(beta) < safmin && knt < 20);
        xn = NX == 1 ? fabsf(x0) : la_lapy2(x0, x1);
        beta = -__builtin_copysignf(la_lapy2(alpha, xn), alpha);
    }
    const float tau = fdiv(beta - alpha, beta);
    const float sc = fdiv(1.0f, alpha - beta);
    x0 *= sc;
    if (NX == 2) x1 *= sc;
    for (int j = 0; j < knt; ++j) beta *= safmin;
    alpha = beta;
    return tau;
}
template <int NX>
RTG_DEV bool la_larfg_ok(float alpha, float x0, float x1)   // the reflector's test (la_larfg)
{
    const float xa0 = fabsf(x0), w = NX == 1 ? xa0 : fmaxf(xa0, fabsf(x1));
    return (w >= 0x1p-46f) & (w <= 0x1p45f) & (fabsf(alpha) <= 0x1p45f);
}
// S1 false: the caller knows the tests would refuse (the general three-point fit, cal_joint_quat) and keeps a / b
template <int NX, bool S1 = true>
RTG_DEV float la_larfg(float &alpha, float &x0, float &x1)
{
#if RTG_FIT_FAST_DIV_TU
    if constexpr (!S1) return la_larfg_ieee<NX>(alpha, x0, x1);
    // One test per reflector (round 22), in place of SLARFG's own two (xn == 0, |beta| < safmin: it implies neither
    // holds): w = max |x_i| in [2^-46, 2^45] and |alpha| <= 2^45.  Then xn = SLAPY2(x) lies in [w, sqrt(2) w], inside
    // the window, so la_lapy2_bare holds for it and for SLAPY2(alpha, xn), whose larger operand is at least xn;
    // |beta| lies in [2^-46, sqrt(3) 2^45] and, beta and alpha having opposite signs, |beta - alpha| = |beta| + |alpha|
    // in [2^-46, 2^47): both quotients below are in region [W].  NaN or inf in alpha fails the second comparison,
    // inf in x the first; a NaN in x is dropped by SLAPY2's max / min exactly as in the reference form.  A lane the
    // test refuses takes SLARFG as it was, behind the same one branch.
    if (__builtin_expect(!la_larfg_ok<NX>(alpha, x0, x1), 0)) return la_larfg_ieee<NX>(alpha, x0, x1);
    const float xa0 = fabsf(x0);
    const float xn = NX == 1 ? xa0 : la_lapy2_bare(xa0, fabsf(x1));
    const float beta = -__builtin_copysignf(la_lapy2_bare(fabsf(alpha), xn), alpha);
    const float tau = fdiv1(beta - alpha, beta);
    const float sc = fdiv1(1.0f, alpha - beta);
    x0 *= sc;
    if (NX == 2) x1 *= sc;
    alpha = beta;
    return tau;
#else
    return la_larfg_ieee<NX>(alpha, x0, x1);
#endif
}
RTG_DEV void la_lartg(float f, float g, float &c, float &s, float &r)   // SLARTG (LAPACK >= 3.10)
{
    const float safmin = 1.17549435e-38f, safmax = 1.0f / safmin;
    const float rtmin = 1.08420217e-19f, rtmax = 1.30438176e+19f;   // sqrt(safmin), sqrt(safmax / 2)
    const float f1 = fabsf(f), g1 = fabsf(g);
    // the common case (f, g nonzero and in range) runs unconditionally; the other three cases of SLARTG redo the
    // outputs behind ONE rare-case branch -- the same operations per case as the reference's cascade
#if RTG_FIT_FAST_DIV_TU
    // the unconditional form is the bare shared-reciprocal one, valid for |f|, |g| in fdiv_n's window [2^-47, 2^47]:
    // then f^2 + g^2 lies in [2^-93, 2^95] (not tiny: cr_sqrt_nt; no overflow) and d in [2^-47, 2^47.5], whose
    // exponent is still at most 47, so the exponents of f1 and g differ from d's by at most 94 and fdiv_n's argument
    // holds for both quotients (which are <= 1 and >= 2^-95).  The window test takes the place of the four range
    // comparisons and two zero tests below (it implies them all); a lane outside it takes the rare-case branch,
    // where SLARTG's common case is redone with fdiv and cr_sqrt.
    const bool common = (f1 >= kDivLo) & (f1 <= kDivHi) & (g1 >= kDivLo) & (g1 <= kDivHi);
    {
        const float d = la_sqrt_nt(f * f + g * g);
        const float num[2] = {f1, g};
        float quo[2];
        fdiv_n_bare<2>(num, d, quo);
        c = quo[0];
        r = __builtin_copysignf(d, f);
        s = f < 0.0f ? -quo[1] : quo[1];   // g / r with r = +-d (RN is sign-symmetric)
    }
#else
    const bool common = (g != 0.0f) & (f != 0.0f) & (f1 > rtmin) & (f1 < rtmax) & (g1 > rtmin) & (g1 < rtmax);
    {
        const float d = la_sqrt(f * f + g * g);
        const float quo[2] = {fdiv(f1, d), fdiv(g, d)};
        c = quo[0];
        r = __builtin_copysignf(d, f);
        s = f < 0.0f ? -quo[1] : quo[1];   // g / r with r = +-d (RN is sign-symmetric)
    }
#endif
    if (__builtin_expect(!common, 0)) {
        if (g == 0.0f) { c = 1.0f; s = 0.0f; r = f; }
        else if (f == 0.0f) { c = 0.0f; s = __builtin_copysignf(1.0f, g); r = g1; }
#if RTG_FIT_FAST_DIV_TU
        else if ((f1 > rtmin) & (f1 < rtmax) & (g1 > rtmin) & (g1 < rtmax)) {   // the common case outside the window
            const float d = la_sqrt(f * f + g * g), q = fdiv(g, d);
            c = fdiv(f1, d);
            r = __builtin_copysignf(d, f);
            s = f < 0.0f ? -q : q;
        }
#endif
        else {
            const float u = fminf(safmax, fmaxf(safmin, fmaxf(f1, g1)));
            const float fs = fdiv(f, u), gs = fdiv(g, u), d = la_sqrt(fs * fs + gs * gs);
            c = fdiv(fabsf(fs), d);
            r = __builtin_copysignf(d, f);
            s = fdiv(gs, r);
            r *= u;
        }
    }
}
// BARE (round 22): the caller (la_bdsqr3's per-pass test) holds |f|, |g|, |h| in kStLo .. kStHi = [2^-46, 2^46], and
// every quotient below runs bare with no test of its own.  By denominator: fhmx, and ga where ga >= fhmx, are state
// values, in the window; so are the numerators fhmn, ga and fhmx (region [W]; fhmx / ga >= 2^-92 is never 0).
// fhmx - fhmn is +0 (a difference of absolute values, fhmx >= fhmn) or at least ulp(fhmn) >= 2^-69 (region [N]).  The
// two sums of roots are plain numbers: as = 1 + fhmn / fhmx in [1, 2], at <= 1, au < 1 in the first form, so the sum
// lies in [1, sqrt 5 + sqrt 2]; p = as au <= 2 and q <= 1 in the second, so it lies in [2, sqrt 5 + sqrt 2].
template <bool BARE = false>
RTG_DEV float la_las2_min(float f, float g, float h)   // SLAS2, SSMIN only (the shift)
{
    const float fa = fabsf(f), ga = fabsf(g), ha = fabsf(h);
    const float fhmn = fminf(fa, ha), fhmx = fmaxf(fa, ha);
    if (fhmn == 0.0f) return 0.0f;
    if (ga < fhmx) {
        const float num[3] = {fhmn, fhmx - fhmn, ga};
        float quo[3];
        if constexpr (BARE) fdiv_n_bare<3>(num, fhmx, quo);
        else fdiv_n<3>(num, fhmx, quo);
        const float as = 1.0f + quo[0], at = quo[1];
        float au = quo[2];
        au = au * au;
        // as >= 1 (the quotient is >= 0), so as^2 + au >= 1: not tiny.  at^2 + au can be (at = 0, au tiny): cr_sqrt
        const float c = fdiv_g<BARE>(2.0f, la_sqrt_nt(as * as + au) + la_sqrt(at * at + au));
        return fhmn * c;
    }
    const float au = fdiv_g<BARE>(fhmx, ga);
    if (au == 0.0f) return fdiv(fhmn * fhmx, ga);
    const float num[2] = {fhmn, fhmx - fhmn};
    float quo[2];
    if constexpr (BARE) fdiv_n_bare<2>(num, fhmx, quo);
    else fdiv_n<2>(num, fhmx, quo);
    const float as = 1.0f + quo[0], at = quo[1], p = as * au, q = at * au;
    // 1 + p^2 and 1 + q^2 are >= 1 (or NaN): not tiny
    const float c = fdiv_g<BARE>(1.0f, la_sqrt_nt(1.0f + p * p) + la_sqrt_nt(1.0f + q * q));
    const float mn = (fhmn * c) * au;
    return mn + mn;
}
// SLASV2
RTG_DEV void la_lasv2(float f, float g, float h, float &ssmin, float &ssmax, float &snr, float &csr, float &snl,
                      float &csl)
{
    const float eps = 5.96046448e-08f;
    float ft = f, fa = fabsf(ft), ht = h, ha = fabsf(h), gt = g;
    float clt = 1.0f, crt = 1.0f, slt = 0.0f, srt = 0.0f;
    int pmax = 1;
    const bool swap = ha > fa;
    if (swap) { pmax = 3; float t = ft; ft = ht; ht = t; t = fa; fa = ha; ha = t; }
    const float ga = fabsf(gt);
    if (ga == 0.0f) { ssmin = ha; ssmax = fa; }
    else {
        bool gasmal = true;
        if (ga > fa) {
            pmax = 2;
            if (fdiv(fa, ga) < eps) {
                gasmal = false;
                ssmax = ga;
                ssmin = ha > 1.0f ? fdiv(fa, fdiv(ga, ha)) : fdiv(fa, ga) * ha;
                const float num[2] = {ht, ft};
                float quo[2];
                fdiv_n<2>(num, gt, quo);
                clt = 1.0f; slt = quo[0]; srt = 1.0f; crt = quo[1];
            }
        }
        if (gasmal) {
            // one form for both settings of RTG_FIT_FAST_DIV_TU (round 20): with 0, fdiv_n is a plain division loop and
            // la_sqrt_nt is cr_sqrt, so the grouped order below computes the values the ungrouped order did
            const float d = fa - ha, l = d == fa ? 1.0f : fdiv(d, fa);
            const float numf[2] = {gt, ht};
            float quof[2];
            fdiv_n<2>(numf, ft, quof);   // m = gt / ft, and ht / ft for slt
            const float m = quof[0], mm = m * m;
            float t = 2.0f - l;
            const float tt = t * t;
            // l = (fa - ha) / fa lies in [0, 1], so t = 2 - l >= 1 and tt + mm >= 1 (or NaN): not tiny.
            // No such bound is claimed for l^2 + mm: cr_sqrt
            const float s = la_sqrt_nt(tt + mm);
            const float r = l == 0.0f ? fabsf(m) : la_sqrt(l * l + mm);
            const float a = 0.5f * (s + r);
            ssmax = fa * a;
            if (mm == 0.0f) t = l == 0.0f ? la_sign(2.0f, ft) * la_sign(1.0f, gt) : fdiv(gt, la_sign(d, ft)) + fdiv(m, t);
            else t = (fdiv(m, s + t) + fdiv(m, r + l)) * (1.0f + a);
            const float l2 = la_sqrt_nt(t * t + 4.0f);   // >= 4 (or NaN): not tiny
            const float numl[2] = {2.0f, t};
            float quol[2];
            fdiv_n<2>(numl, l2, quol);
            crt = quol[0];
            srt = quol[1];
            const float numa[3] = {ha, crt + srt * m, quof[1] * srt};
            float quoa[3];
            fdiv_n<3>(numa, a, quoa);
            ssmin = quoa[0];
            clt = quoa[1];
            slt = quoa[2];
        }
    }
    if (swap) { csl = srt; snl = crt; csr = slt; snr = clt; }
    else { csl = clt; snl = slt; csr = crt; snr = srt; }
    const float tsg = pmax == 1 ? la_sign(1.0f, csr) * la_sign(1.0f, csl) * la_sign(1.0f, f)
                    : pmax == 2 ? la_sign(1.0f, snr) * la_sign(1.0f, csl) * la_sign(1.0f, g)
                                : la_sign(1.0f, snr) * la_sign(1.0f, snl) * la_sign(1.0f, h);
    ssmax = la_sign(ssmax, tsg);
    ssmin = la_sign(ssmin, tsg * la_sign(1.0f, f) * la_sign(1.0f, h));
}
RTG_DEV void la_rot(float &x, float &y, float c, float s)   // MKL's SROT / SLASR pair update
{
    const float xv = x, yv = y;
    x = __builtin_fmaf(s, yv, c * xv);
    y = __builtin_fmaf(c, yv, -(s * xv));
}
struct Svd3 { float u[9], vt[9]; };
// rotate VT rows (p, p+1) / U columns (p, p+1), p = p1 ? 1 : 0 chosen per lane by selects (no divergence)
RTG_DEV void vt_rot(Svd3 &z, bool p1, float c, float s)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x = p1 ? z.vt[1 + 3 * k] : z.vt[3 * k], y = p1 ? z.vt[2 + 3 * k] : z.vt[1 + 3 * k];
        la_rot(x, y, c, s);
        z.vt[3 * k] = p1 ? z.vt[3 * k] : x;
        z.vt[1 + 3 * k] = p1 ? x : y;
        z.vt[2 + 3 * k] = p1 ? y : z.vt[2 + 3 * k];
    }
}
RTG_DEV void u_rot(Svd3 &z, bool p1, float c, float s)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float x = p1 ? z.u[k + 3] : z.u[k], y = p1 ? z.u[k + 6] : z.u[k + 3];
        la_rot(x, y, c, s);
        z.u[k] = p1 ? z.u[k] : x;
        z.u[k + 3] = p1 ? x : y;
        z.u[k + 6] = p1 ? y : z.u[k + 6];
    }
}
// la_rot on a pair of slots (lo, hi) held in chase order (la_bdsqr3), both directions as one instruction sequence
// with fixed destinations.  Top to bottom (mir false) it is la_rot(lo, hi, c, s); bottom to top the pair is
// (x, y) = (hi, lo) and the sine is negated (SBDSQR stores -SN): la_rot(hi, lo, c, -s).  Written out,
//   !mir: lo' = fma(s, hi, c lo),      hi' = fma(c, hi, (-s) lo)
//    mir: lo' = fma(c, lo, s hi),      hi' = fma(-s, lo, c hi)
// i.e. lo' = fma(P, Q, R S), hi' = fma(P2, Q, R2 S) with Q = mir ? lo : hi, S = mir ? hi : lo; -(s x) and (-s) x
// are the same bits.  Two selects per pair, four per rotation (shared by its three pairs), none on the outputs.
struct SlotRot {
    bool mir;
    float P, R, P2, R2;
    RTG_DEV SlotRot(bool mir_, float c, float s)   // s: the sine before SBDSQR's negation
        : mir(mir_), P(mir_ ? c : s), R(mir_ ? s : c), P2(mir_ ? -s : c), R2(mir_ ? c : -s) {}
    RTG_DEV void operator()(float &lo, float &hi) const
    {
        const float Q = mir ? lo : hi, S = mir ? hi : lo;
        lo = __builtin_fmaf(P, Q, R * S);
        hi = __builtin_fmaf(P2, Q, R2 * S);
    }
};
// the end of SBDSQR: singular values made positive, then sorted decreasing, with their VT rows / U columns
RTG_DEV void la_bdsqr3_sort(float &d1, float &d2, float &d3, Svd3 &z)
{
    // singular values made positive (VT rows negated), then sorted decreasing (SBDSQR :160-190)
    if (d1 < 0.0f) { d1 = -d1; z.vt[0] = -z.vt[0]; z.vt[3] = -z.vt[3]; z.vt[6] = -z.vt[6]; }
    if (d2 < 0.0f) { d2 = -d2; z.vt[1] = -z.vt[1]; z.vt[4] = -z.vt[4]; z.vt[7] = -z.vt[7]; }
    if (d3 < 0.0f) { d3 = -d3; z.vt[2] = -z.vt[2]; z.vt[5] = -z.vt[5]; z.vt[8] = -z.vt[8]; }
    // pass 1: smallest of (d1, d2, d3), ties to the later index, moves to position 3
    {
        int isub = 1;
        float mn = d1;
        if (d2 <= mn) { isub = 2; mn = d2; }
        if (d3 <= mn) { isub = 3; mn = d3; }
        const bool s1 = isub == 1, s2 = isub == 2;
        d1 = s1 ? d3 : d1;
        d2 = s2 ? d3 : d2;
        d3 = mn;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v0 = z.vt[3 * k], v1 = z.vt[1 + 3 * k], v2 = z.vt[2 + 3 * k];
            z.vt[3 * k] = s1 ? v2 : v0;
            z.vt[1 + 3 * k] = s2 ? v2 : v1;
            z.vt[2 + 3 * k] = s1 ? v0 : (s2 ? v1 : v2);
            const float u0 = z.u[k], u1 = z.u[k + 3], u2 = z.u[k + 6];
            z.u[k] = s1 ? u2 : u0;
            z.u[k + 3] = s2 ? u2 : u1;
            z.u[k + 6] = s1 ? u0 : (s2 ? u1 : u2);
        }
    }
    // pass 2: smaller of (d1, d2), ties to d2, moves to position 2
    {
        const bool sw = !(d2 <= d1);
        const float t0 = d1;
        d1 = sw ? d2 : d1;
        d2 = sw ? t0 : d2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v0 = z.vt[3 * k], v1 = z.vt[1 + 3 * k];
            z.vt[3 * k] = sw ? v1 : v0;
            z.vt[1 + 3 * k] = sw ? v0 : v1;
            const float u0 = z.u[k], u1 = z.u[k + 3];
            z.u[k] = sw ? u1 : u0;
            z.u[k + 3] = sw ? u0 : u1;
        }
    }
}
// SBDSQR('U', 3, ncvt = 3, nru = 3, ncc = 0) from U = VT = I (SBDSDC / SLASDQ), n = 3 specialised: the only
// multi-element block is (ll, m) = (1, 3); every other case ends in one 2x2 SLASV2 block.  A bottom-to-top
// chase (IDIR = 2) is the top-to-bottom chase (IDIR = 1) of the reversed bidiagonal (d3, d2, d1; e2, e1) -- the
// same scalar recurrences, with the rotations applied to the mirrored row / column pairs and negated sines
// (SBDSQR :130/:150 store -SN) -- so both directions run one code path and a wave never executes both.
//
// The single quotients of SBDSQR's bookkeeping run bare behind ONE test of the bidiagonal per group (round 22): the
// entry's three, and each pass's (the mu chain, smin / smax, SLAS2's, shift / sll).  The test: all of |d1..3|, |e1|,
// |e2| in [kStLo, kStHi] = [2^-46, 2^46], a min chain next to the max chain smax already is.  What follows from it,
// per quotient (regions as named at fdiv1):
//   mu / (mu + |e|), first link: mu = |d1| and the sum, at most 2^47, are in the window [W].  Second link: the sum is
//     in [2^-46, 2^47]; mu = |d2| q1 can be far below the state.  mu >= kNumLo is region [N].  Below that the exact
//     quotient is under 2^-76 / 2^-46 = 2^-30 and the bare one at most twice it (t = RN(mu y), a residual of at most
//     2 mu): at the ENTRY the value matters (thresh), so the entry tests its final sminoa >= kNumLo, which bounds both
//     links' numerators and the constant division's from below; in a PASS the second link feeds only smin, and
//   smin / smax is read by one comparison, against 1 / 30: smin >= kNumLo is region [N] (smax is a state value);
//     under it both the exact and the bare quotient are below 2^-29, and so is any quotient formed from a second
//     link that was itself below 2^-30 -- the comparison reads the same.  No test beyond the state's.
//   SLAS2: see la_las2_min.
//   shift / sll: sll = |D1| is a state value and 0 <= shift <= 2^46 (shift = +0 gives +0).  The quotient is read by
//     q q < eps alone.  q q >= eps needs shift >= 2^-12 sll >= 2^-58: region [N]; below kNumLo the exact q is under
//     2^-30, the bare one under 2^-29, and the shift is zeroed.  (The sweep's own shift / D1 is left as it was.)
// inf fails the max test.  A NaN passes the chains (max / min keep the other operand) and makes NaN of every
// quotient it enters in either form.  A lane whose state fails takes the group in the compiler's a / b form.
constexpr float kStLo = 0x1p-46f, kStHi = 0x1p46f;
constexpr float kSqrt3 = 1.73205078f, kRcpSqrt3 = 0x1.279a74p-1f;   // sqrt(real(3)); RN(1 / kSqrt3), its own refinement
// SBDSQR's sminoa before its division by sqrt(3)
template <bool BARE>
RTG_DEV float la_bdsqr3_sminoa(float d1, float d2, float d3, float e1, float e2)
{
    float sminoa = fabsf(d1);
    if (sminoa != 0.0f) {
        float mu = fabsf(d2) * fdiv_g<BARE>(sminoa, sminoa + fabsf(e1));
        sminoa = fminf(sminoa, mu);
        if (sminoa != 0.0f) {
            mu = fabsf(d3) * fdiv_g<BARE>(mu, mu + fabsf(e2));
            sminoa = fminf(sminoa, mu);
        }
    }
    return sminoa;
}
// One pass over the block (1, 3) in chase order: SBDSQR's convergence tests, and for a lane that sweeps (zero = 0)
// the shift.  zero = 1, 2: E1, E2 is negligible; the caller zeroes it and the lane is done with
// this pass.  Returned by value: nothing here is stored through a pointer, so every value stays in a register.
struct BdsqrPass { int zero; float shift; };
template <bool BARE>
RTG_DEV BdsqrPass la_bdsqr3_shift(float D1, float D2, float D3, float E1, float E2, float smax)
{
    const float eps = 5.96046448e-08f, tol = 10.0f * eps;
    BdsqrPass p{0, 0.0f};
    if (fabsf(E2) <= fabsf(tol) * fabsf(D3)) p.zero = 2;
    else {
        float mu = fabsf(D1), smin = mu;
        if (fabsf(E1) <= tol * mu) p.zero = 1;
        else {
            mu = fabsf(D2) * fdiv_g<BARE>(mu, mu + fabsf(E1));
            smin = fminf(smin, mu);
            if (fabsf(E2) <= tol * mu) p.zero = 2;
            else {
                mu = fabsf(D3) * fdiv_g<BARE>(mu, mu + fabsf(E2));
                smin = fminf(smin, mu);
                if (!((3.0f * tol) * fdiv_g<BARE>(smin, smax) <= fmaxf(eps, 0.01f * tol))) {
                    const float sll = fabsf(D1), sh = la_las2_min<BARE>(D2, E2, D3);
                    const float q = fdiv_g<BARE>(sh, sll);   // sll > 0 where BARE: a state value; else unread
                    p.shift = ((BARE || sll > 0.0f) && q * q < eps) ? 0.0f : sh;
                }
            }
        }
    }
    return p;
}
// the state's test; smax: the max of the five magnitudes
RTG_DEV bool la_bdsqr3_state_ok(float D1, float D2, float D3, float E1, float E2, float smax)
{
    const float smn = fminf(fminf(fabsf(D3), fminf(fabsf(D2), fabsf(E2))), fminf(fabsf(D1), fabsf(E1)));
    return (smn >= kStLo) & (smax <= kStHi);
}
RTG_DEV float la_bdsqr3_smax(float D1, float D2, float D3, float E1, float E2)
{
    // max over a set (a NaN only ever yields to the other operand): the same value in either order
    return fmaxf(fmaxf(fabsf(D3), fmaxf(fabsf(D2), fabsf(E2))), fmaxf(fabsf(D1), fabsf(E1)));
}
// the pass behind the state's test
template <bool S1 = true>
RTG_DEV BdsqrPass la_bdsqr3_pass(float D1, float D2, float D3, float E1, float E2, float smax)
{
#if RTG_FIT_FAST_DIV_TU
    if (S1 && __builtin_expect(la_bdsqr3_state_ok(D1, D2, D3, E1, E2, smax), 1)) return la_bdsqr3_shift<true>(D1, D2, D3, E1, E2, smax);
#endif
    return la_bdsqr3_shift<false>(D1, D2, D3, E1, E2, smax);
}
// SBDSQR's sminoa / sqrt(real(3)) behind the state's test and the one on its own numerator
template <bool S1 = true>
RTG_DEV float la_bdsqr3_entry(float d1, float d2, float d3, float e1, float e2)
{
#if RTG_FIT_FAST_DIV_TU
    if constexpr (!S1) return fdiv(la_bdsqr3_sminoa<false>(d1, d2, d3, e1, e2), kSqrt3);
    const float s = la_bdsqr3_sminoa<true>(d1, d2, d3, e1, e2);
    const bool ok = la_bdsqr3_state_ok(d1, d2, d3, e1, e2, la_bdsqr3_smax(d1, d2, d3, e1, e2)) & (s >= kNumLo);
    float q = fdiv1_const(s, kSqrt3, kRcpSqrt3);
    if (__builtin_expect(!ok, 0)) q = fdiv(la_bdsqr3_sminoa<false>(d1, d2, d3, e1, e2), kSqrt3);
    return q;
#else
    return fdiv(la_bdsqr3_sminoa<false>(d1, d2, d3, e1, e2), kSqrt3);
#endif
}
template <bool S1 = true>
RTG_DEV void la_bdsqr3(float &d1, float &d2, float &d3, float e1, float e2, Svd3 &z)
{
    const float eps = 5.96046448e-08f, tol = 10.0f * eps, unfl = 1.17549435e-38f;
    const float sminoa = la_bdsqr3_entry<S1>(d1, d2, d3, e1, e2);
    const float thresh = fmaxf(tol * sminoa, 6.0f * (3.0f * (3.0f * unfl)));
    int m = 3, iter = -1, iterdivn = 0;
    // mir: IDIR = 2.  SBDSQR picks the direction when (ll, m) = (1, 3) is new, from |d1| >= |d3|; nothing changes d
    // before the first sweep and m never returns to 3 after it, so the entry values decide it once.
    const bool mir = !(fabsf(d1) >= fabsf(d3));
    // The whole loop works in chase order: slot k of (D1, D2, D3), of VT's rows and columns and of U's rows and
    // columns holds index mir ? 2 - k : k, and (E1, E2) = mir ? (e2, e1) : (e1, e2) -- the IDIR = 1 form of the
    // (mirrored) bidiagonal.  U = VT = I on entry is its own mirror (rows and columns both reversed); rows of U
    // and columns of VT are never mixed, so reversing them too costs nothing in the loop.  Index order returns
    // once, after the loop.
    float D1 = mir ? d3 : d1, D2 = d2, D3 = mir ? d1 : d3, E1 = mir ? e2 : e1, E2 = mir ? e1 : e2;
    // A lane whose last step is a 2x2 block leaves the loop with blk set, and the block (SLASV2 + its two
    // rotations) runs once after the loop for every such lane: the lanes of a wave finish at different sweeps,
    // and inside the loop the block would execute once per distinct exit sweep.  Same operations, same values.
    bool blk = false, p1 = false, run = true;
    // One structured loop (no break / continue: every exit carries the same live values, so the loop head holds no
    // copies of the 18 U / VT entries): a pass classifies the lane, and only a lane that sweeps enters the body.
    while (run) {
        bool sweep = false;
        float shift = 0.0f;
        const float e1t = mir ? E2 : E1, e2t = mir ? E1 : E2;   // e1, e2 in index order
        bool capped = false;
        if (iter >= 3) { iter -= 3; capped = ++iterdivn >= 18; }   // no convergence: INFO > 0 (never seen)
        if (capped) run = false;
        else if (m == 2) {                       // block (1, 2)
            blk = !(fabsf(e1t) <= thresh);
            run = false;
        }
        // deflation at E(2) and the split at E(1) store a zero that nothing reads again (the block (1, 2) reads e1
        // alone, the block (2, 3) e2 alone): not stored
        else if (fabsf(e2t) <= thresh) m = 2;
        else if (fabsf(e1t) <= thresh) { blk = true; p1 = true; run = false; }   // split at E(1): block (2, 3)
        else {
            const float smax = la_bdsqr3_smax(D1, D2, D3, E1, E2);
            // a lane with a zeroed e is done with this pass (sweep stays false)
            const BdsqrPass ps = la_bdsqr3_pass<S1>(D1, D2, D3, E1, E2, smax);
            E1 = ps.zero == 1 ? 0.0f : E1;
            E2 = ps.zero == 2 ? 0.0f : E2;
            sweep = ps.zero == 0;
            shift = ps.shift;
        }
        if (sweep) {
            iter += 2;
            // rotations of the two steps: (ac, as) / (bc, bs) at the first, (cc, cs) / (dc, ds) at the second
            float ac, as, bc, bs, cc, cs, dc, ds;
            if (shift == 0.0f) {
                float r, h;
                la_lartg(D1, E1, ac, as, r);                 // cs = 1
                la_lartg(r, D2 * as, bc, bs, D1);            // oldcs = 1
                la_lartg(D2 * ac, E2, cc, cs, r);
                E1 = bs * r;
                la_lartg(bc * r, D3 * cs, dc, ds, D2);
                h = D3 * cc;
                D3 = h * dc;
                E2 = h * ds;
            } else {
                float f = (fabsf(D1) - shift) * (__builtin_copysignf(1.0f, D1) + fdiv(shift, D1)), g = E1, r;
                la_lartg(f, g, ac, as, r);
                f = ac * D1 + as * E1;
                E1 = ac * E1 - as * D1;
                g = as * D2;
                D2 = ac * D2;
                la_lartg(f, g, bc, bs, r);
                D1 = r;
                f = bc * E1 + bs * D2;
                D2 = bc * D2 - bs * E1;
                g = bs * E2;
                E2 = bc * E2;
                la_lartg(f, g, cc, cs, r);
                E1 = r;
                f = cc * D2 + cs * E2;
                E2 = cc * E2 - cs * D2;
                g = cs * D3;
                D3 = cc * D3;
                la_lartg(f, g, dc, ds, r);
                D2 = r;
                f = dc * E2 + ds * D3;
                D3 = dc * D3 - ds * E2;
                E2 = f;
            }
            if (fabsf(E2) <= thresh) E2 = 0.0f;
            // IDIR = 1: VT pairs (1,2) then (2,3) by (a, c), U by (b, d).  IDIR = 2: VT (2,3) then (1,2) by (b, d),
            // U by (a, c), sines negated.  In chase order both are slots (0,1) then (1,2).
            const SlotRot va(mir, mir ? bc : ac, mir ? bs : as), vc(mir, mir ? dc : cc, mir ? ds : cs);
            const SlotRot ub(mir, mir ? ac : bc, mir ? as : bs), ud(mir, mir ? cc : dc, mir ? cs : ds);
#pragma unroll
            for (int k = 0; k < 3; ++k) va(z.vt[3 * k], z.vt[1 + 3 * k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) vc(z.vt[1 + 3 * k], z.vt[2 + 3 * k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) ub(z.u[k], z.u[k + 3]);
#pragma unroll
            for (int k = 0; k < 3; ++k) ud(z.u[k + 3], z.u[k + 6]);
        }
    }
    // back to index order: (d, e) unmirrored, U and VT turned by half a turn (rows and columns both reversed)
    d1 = mir ? D3 : D1; d2 = D2; d3 = mir ? D1 : D3;
    e1 = mir ? E2 : E1; e2 = mir ? E1 : E2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float v0 = z.vt[i], v1 = z.vt[8 - i], u0 = z.u[i], u1 = z.u[8 - i];
        z.vt[i] = mir ? v1 : v0;
        z.vt[8 - i] = mir ? v0 : v1;
        z.u[i] = mir ? u1 : u0;
        z.u[8 - i] = mir ? u0 : u1;
    }
    if (blk) {   // 2x2 block (p1 ? 2 : 1, +1)
        float sigmn, sigmx, sinr, cosr, sinl, cosl;
        la_lasv2(p1 ? d2 : d1, p1 ? e2 : e1, p1 ? d3 : d2, sigmn, sigmx, sinr, cosr, sinl, cosl);
        d1 = p1 ? d1 : sigmx;
        d2 = p1 ? sigmx : sigmn;
        d3 = p1 ? sigmn : d3;
        vt_rot(z, p1, cosr, sinr);
        u_rot(z, p1, cosl, sinl);
    }
    la_bdsqr3_sort(d1, d2, d3, z);
}
// Stage marks for the timestamp measurement builds (RTG_EXP_TIMESTAMPS): hook(k) at a stage boundary, a no-op otherwise.
// cal_joint_quat: 0 A formed, 1 rotation done; la_gesdd3: 10 bidiagonal form (SGEBD2) done, 11 SBDSQR done.
struct NoHook {
    RTG_DEV void operator()(int) const {}
};
// SGEBD2 after H_0: G_0 from the right (v = (1, a6)), then i = 1: H_1 from the left (v = (1, a5)) on column 2;
// G_1 = I (one-element reflector), i = 2: H_2 = I
template <bool S1 = true>
RTG_DEV void la_gebd2_rest(float a[9], float &tp0, float &tq1, float &e1, float &d2, float &e2, float &d3)
{
    float dum = 0.0f;
    tp0 = la_larfg<1, S1>(a[3], a[6], dum);
    e1 = a[3];
    if (tp0 != 0.0f) {
        const float tv1 = -(tp0 * 1.0f), tv2 = -(tp0 * a[6]);
#pragma unroll
        for (int r = 1; r < 3; ++r) {
            const float w = __builtin_fmaf(a[r + 6], a[6], a[r + 3]);
            a[r + 3] = __builtin_fmaf(w, tv1, a[r + 3]);
            a[r + 6] = __builtin_fmaf(w, tv2, a[r + 6]);
        }
    }
    // i = 1: H_1 from the left (v = (1, a5)) on column 2; G_1 = I (one-element reflector)
    tq1 = la_larfg<1, S1>(a[4], a[5], dum);
    d2 = a[4];
    if (tq1 != 0.0f) {
        const float w = a[7] + a[8] * a[5];
        const float tw = -(tq1 * w);
        a[7] = __builtin_fmaf(1.0f, tw, a[7]);
        a[8] = __builtin_fmaf(a[5], tw, a[8]);
    }
    e2 = a[7];
    d3 = a[8];   // i = 2: H_2 = I
}
// SORMBR of the 3x3 SGESDD: U := H_0 H_1 U, VT := VT G_0^T
RTG_DEV void la_ormbr3(const float a[9], float tq0, float tq1, float tp0, Svd3 &z)
{
    // SORMBR('Q','L','N'): U := H_0 H_1 U (H_1 first), the unit row fused as fma(-tau, w, c)
    if (tq1 != 0.0f) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float w = z.u[1 + 3 * j] + z.u[2 + 3 * j] * a[5];
            const float tw = -(tq1 * w);
            z.u[1 + 3 * j] = __builtin_fmaf(-tq1, w, z.u[1 + 3 * j]);
            z.u[2 + 3 * j] = __builtin_fmaf(a[5], tw, z.u[2 + 3 * j]);
        }
    }
    if (tq0 != 0.0f) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float w = z.u[3 * j] + (z.u[1 + 3 * j] * a[1] + z.u[2 + 3 * j] * a[2]);
            const float tw = -(tq0 * w);
            z.u[3 * j] = __builtin_fmaf(-tq0, w, z.u[3 * j]);
            z.u[1 + 3 * j] = __builtin_fmaf(a[1], tw, z.u[1 + 3 * j]);
            z.u[2 + 3 * j] = __builtin_fmaf(a[2], tw, z.u[2 + 3 * j]);
        }
    }
    // SORMBR('P','R','T'): VT := VT G_0^T on columns 1..2
    if (tp0 != 0.0f) {
        const float tv1 = -(tp0 * 1.0f), tv2 = -(tp0 * a[6]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float w = __builtin_fmaf(z.vt[r + 6], a[6], z.vt[r + 3]);
            z.vt[r + 3] = __builtin_fmaf(w, tv1, z.vt[r + 3]);
            z.vt[r + 6] = __builtin_fmaf(w, tv2, z.vt[r + 6]);
        }
    }
}
// SGESDD(JOBZ='A') of a 3x3 (column-major a, overwritten): U and VT (column-major) in z
template <bool S1 = true, typename Hook = NoHook>
RTG_DEV void la_gesdd3(float a[9], Svd3 &z, const Hook &hook = Hook{})
{
    const float smlnum = 9.09494702e-13f, bignum = 1.0f / smlnum;   // sqrt(slamch('S')) / slamch('P') = 2^-40
    float anrm = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) anrm = fmaxf(anrm, fabsf(a[i]));
    if (__builtin_expect((anrm > 0.0f && anrm < smlnum) || anrm > bignum, 0)) {
        const float mul = anrm < smlnum ? fdiv(smlnum, anrm) : fdiv(bignum, anrm);
#pragma unroll
        for (int i = 0; i < 9; ++i) a[i] *= mul;
    }
    // SGEBD2, i = 0: H_0 from the left (v = (1, a1, a2)), G_0 from the right (v = (1, a6))
    const float tq0 = la_larfg<2, S1>(a[0], a[1], a[2]);
    const float d1 = a[0];
    if (tq0 != 0.0f) {
#pragma unroll
        for (int j = 1; j < 3; ++j) {
            const float w = a[3 * j] + (a[1 + 3 * j] * a[1] + a[2 + 3 * j] * a[2]);
            const float tw = -(tq0 * w);
            a[3 * j] = __builtin_fmaf(1.0f, tw, a[3 * j]);
            a[1 + 3 * j] = __builtin_fmaf(a[1], tw, a[1 + 3 * j]);
            a[2 + 3 * j] = __builtin_fmaf(a[2], tw, a[2 + 3 * j]);
        }
    }
    float tp0, tq1, e1, d2, e2, d3;
    la_gebd2_rest<S1>(a, tp0, tq1, e1, d2, e2, d3);
    hook(10);
    // SBDSDC('U','I') -> SLASDQ -> SBDSQR with U = VT = I
#pragma unroll
    for (int i = 0; i < 9; ++i) { z.u[i] = (i % 4 == 0) ? 1.0f : 0.0f; z.vt[i] = z.u[i]; }
    float s1 = d1, s2 = d2, s3 = d3;
    la_bdsqr3<S1>(s1, s2, s3, e1, e2, z);
    hook(11);
    la_ormbr3(a, tq0, tq1, tp0, z);
}
// ---- SGESDD of a 3x3 whose first column is +-0 (a[0..2], not read): the FULL_BODY_POS torso fit, whose zero-pose
// vectors all have x = 0, so column 0 of A = M^T Z is +-0 for finite M.  la_gesdd3 takes one fixed path on such a
// matrix, through branches it treats as rare; this runs that path alone -- the same operations on the same operands,
// minus those whose result is known:
//   * H_0: SLARFG(3, +-0, (+-0, +-0)) has xnorm = 0 and returns tau = 0 after two SLAPY2 (two divisions, two square
//     roots); H_0 = I, d1 = a[0] = +-0, and columns 1..2 go on unchanged.
//   * SBDSQR: sminoa = |d1| = 0, so thresh = max(tol 0, 18 unfl) = 18 unfl.  With |e2| > thresh, |e1| > thresh and
//     d3 != 0 the block is (1, 3) and |d1| = 0 < |d3| chases bottom to top: (D1, D2, D3; E1, E2) = (d3, d2, +-0; e2, e1).
//     The convergence tests: |E2| <= tol |D3| = 0 is false (|e1| > thresh); |E1| <= tol |D1| must be false (tested);
//     mu2 = |D2| RN(|D1| / (|D1| + |E1|)) <= |D2| (the quotient is <= 1 and RN is monotone), so |E2| > tol |D2| (tested)
//     makes |E2| <= tol mu2 false; mu3 = |D3| q = 0 q = 0 for the finite q, so smin = 0, 3 tol (0 / smax) = 0 <= eps
//     and the shift is 0.  The zero-shift sweep's fourth SLARTG has g = D3 cs = +-0 (cs finite): c = 1, s = +0, r = f
//     -- after its common path's square root and two divisions.  Then D3 = (+-0 cc) 1 = +-0, E2 = +-0 (+0) -> +0 by the
//     threshold test.  Back in (d, e) order e1 = 0, e2 = bs r: the next pass either drops e2 (|e2| <= thresh: m = 2,
//     then |e1| = 0 ends it with no block) or splits at e1 = 0 into the 2x2 block (2, 3) -- per lane, as la_bdsqr3's
//     blk.  The rotations act on U = VT = I with the pair index known (vt_rot / u_rot's selects fold away).
//   * d1 stays +-0 to the end and its sign is never read: d1 < 0 is false for -0, the sort compares values, and
//     only U and VT leave the routine.  So the sign of the zero column (the signs of M's entries, or a -0 in the
//     zero pose) cannot reach an output.
// Everything is finite on this path: the caller tests M (and bounds Z), SGESDD's rescaling then holds |a| <= 2^40,
// and SLARFG / SLARTG / SLASV2 return finite values for such inputs.  The assumptions are tested per lane and
// voted per wave: on a miss of ANY active lane the function returns false before z is written and the whole wave
// runs la_gesdd3 -- never a divergent second copy.  `fin`: this lane's M is finite and small enough (caller).
template <typename Hook = NoHook>
RTG_DEV bool la_gesdd3_x0(float a[9], bool fin, Svd3 &z, const Hook &hook = Hook{})
{
    const float smlnum = 9.09494702e-13f, bignum = 1.0f / smlnum;
    const float eps = 5.96046448e-08f, tol = 10.0f * eps, unfl = 1.17549435e-38f;
    float anrm = 0.0f;
#pragma unroll
    for (int i = 3; i < 9; ++i) anrm = fmaxf(anrm, fabsf(a[i]));
    if (__builtin_expect((anrm > 0.0f && anrm < smlnum) || anrm > bignum, 0)) {
        const float mul = anrm < smlnum ? fdiv(smlnum, anrm) : fdiv(bignum, anrm);
#pragma unroll
        for (int i = 3; i < 9; ++i) a[i] *= mul;
    }
    float tp0, tq1, e1, d2, e2, d3;
    la_gebd2_rest(a, tp0, tq1, e1, d2, e2, d3);
    hook(10);
    const float thresh = 6.0f * (3.0f * (3.0f * unfl));
    const bool ok = fin && fabsf(e2) > thresh && fabsf(e1) > thresh && fabsf(d3) > 0.0f &&
                    !(fabsf(e2) <= tol * fabsf(d3)) && fabsf(e1) > tol * fabsf(d2);
    if (__builtin_amdgcn_ballot_w64(!ok) != 0) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) { z.u[i] = (i % 4 == 0) ? 1.0f : 0.0f; z.vt[i] = z.u[i]; }
    // the zero-shift sweep on (d3, d2, +-0; e2, e1); its fourth rotation is (1, +0) and D2 = its f
    float ac, as, bc, bs, cc, cs, r, s3;
    la_lartg(d3, e2, ac, as, r);
    la_lartg(r, d2 * as, bc, bs, s3);
    la_lartg(d2 * ac, e1, cc, cs, r);
    float s1 = 0.0f, s2 = bc * r;
    e2 = bs * r;
    vt_rot(z, true, bc, -bs);
    vt_rot(z, false, 1.0f, -0.0f);
    u_rot(z, true, ac, -as);
    u_rot(z, false, cc, -cs);
    if (!(fabsf(e2) <= thresh)) {   // 2x2 block (2, 3)
        float sigmn, sigmx, sinr, cosr, sinl, cosl;
        la_lasv2(s2, e2, s3, sigmn, sigmx, sinr, cosr, sinl, cosl);
        s2 = sigmx;
        s3 = sigmn;
        vt_rot(z, true, cosr, sinr);
        u_rot(z, true, cosl, sinl);
    }
    la_bdsqr3_sort(s1, s2, s3, z);
    hook(11);
    la_ormbr3(a, 0.0f, tq1, tp0, z);
    return true;
}
// transform3d.py:40-45: R = U Vt ((p0 + p1) + p2, torch's bmm order); det(R) < 0 -> Vt[-1,:] *= -1; R = U Vt.
// A and R row-major.  det only decides a sign (|det| = 1 up to rounding), taken in float64.
RTG_DEV void kabsch_of_svd(Svd3 &z, float R[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            R[i * 3 + k] = (z.u[i] * z.vt[3 * k] + z.u[i + 3] * z.vt[1 + 3 * k]) + z.u[i + 6] * z.vt[2 + 3 * k];
    // R = U Vt is orthogonal to ~1e-6 (U and Vt are products of plane rotations and reflectors) or all NaN, so
    // |det R| = 1 +- 1e-6 and the sign any f32 evaluation gives is torch.linalg.det's (the oracle keeps f64)
    const float det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
                      R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (det < 0.0f) {
#pragma unroll
        for (int k = 0; k < 3; ++k) z.vt[2 + 3 * k] = -z.vt[2 + 3 * k];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                R[i * 3 + k] = (z.u[i] * z.vt[3 * k] + z.u[i + 3] * z.vt[1 + 3 * k]) + z.u[i + 6] * z.vt[2 + 3 * k];
    }
}
template <bool S1 = true, typename Hook = NoHook>
RTG_DEV void kabsch_rot(const float A[9], float R[9], const Hook &hook = Hook{})
{
#if RTG_EXP_STUB_SVD
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0f : A[i] * 1e-3f;
    return;
#endif
    float a[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) a[i + 3 * k] = A[i * 3 + k];
    Svd3 z;
    la_gesdd3<S1>(a, z, hook);
    kabsch_of_svd(z, R);
}

// cal_joint_quat (transform3d.py:31-50): A = M^T Z by einsum (sequential in j, no FMA).  `hook(k)` marks the
// stages (NoHook above) for the latency-phase measurement knob; a no-op otherwise.
// `svd_nan` is set when A has a NaN entry: torch.linalg.svd refuses such a matrix (LAPACK sgesdd returns info = -4
// on a NaN norm and torch raises "linalg.svd: ... contained non-finite values", transform3d.py:40), so the reference
// frame raises there (an inf entry alone does not raise).
// A = M^T Z (torch.matmul's summation order, measured) and whether it holds a NaN
template <int N>
RTG_DEV bool form_joint_A(const V (&Z)[N], const V (&M)[N], float (&A)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float mi = i == 0 ? M[j].x : (i == 1 ? M[j].y : M[j].z);
                const float zk = k == 0 ? Z[j].x : (k == 1 ? Z[j].y : Z[j].z);
                const float pr = mi * zk;
                acc = j == 0 ? pr : acc + pr;
            }
            A[i * 3 + k] = acc;
        }
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 9; ++i) nan |= A[i] != A[i];
    return nan;
}
// the rotation of a formed A: Kabsch then quat_from_rotation_matrix
template <bool S1 = true, typename Hook = NoHook, typename Tab = NoTab>
RTG_DEV Q joint_quat_of_A(const float (&A)[9], const Hook &hook = Hook{}, Tab tab = Tab{})
{
    hook(0);
    float R[9];
    kabsch_rot<S1>(A, R, hook);
    hook(1);
    return qfrom_rotmat(R, tab);
}
// The torso fit when every zero vector has x = 0 (SolverConsts::torso_x0): A without the zero column's products,
// then la_gesdd3_x0.  Returns false, wave-uniformly, when some active lane is off that path (non-finite or huge M --
// form_joint_A then sees the NaN of inf * 0 in column 0 -- or one of la_gesdd3_x0's tests); the caller then runs
// form_joint_A + joint_quat_of_A for the whole wave.  On true no A entry is NaN: |M| < 2^60 and |Z| <= 2^60 (host)
// bound every product by 2^120 and every sum by 2^122.
template <typename Hook = NoHook, typename Tab = NoTab>
RTG_DEV bool torso_quat_x0(const V (&Z)[3], const V (&M)[3], Q &q, const Hook &hook = Hook{}, Tab tab = Tab{})
{
    float a[9];   // column-major: a[i + 3 k] = A[i][k]
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) sum += fabsf(i == 0 ? M[j].x : (i == 1 ? M[j].y : M[j].z));
#pragma unroll
        for (int k = 1; k < 3; ++k) {
            float acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float mi = i == 0 ? M[j].x : (i == 1 ? M[j].y : M[j].z);
                const float pr = mi * (k == 1 ? Z[j].y : Z[j].z);
                acc = j == 0 ? pr : acc + pr;   // form_joint_A's order
            }
            a[i + 3 * k] = acc;
        }
        a[i] = 0.0f;
    }
    hook(0);
    Svd3 z;
    if (!la_gesdd3_x0(a, sum < 0x1p60f, z, hook)) return false;
    float R[9];
    kabsch_of_svd(z, R);
    hook(1);
    q = qfrom_rotmat(R, tab);
    return true;
}
template <int N, typename Hook = NoHook, typename Tab = NoTab>
RTG_DEV Q cal_joint_quat(const V (&Z)[N], const V (&M)[N], bool &svd_nan, const Hook &hook = Hook{}, Tab tab = Tab{})
{
    float A[9];
    svd_nan = form_joint_A<N>(Z, M, A);
    // Round 22's single-quotient tests are for fits of more than three points.  In the units that have them the
    // three-point fit is the torso's general path, whose matrix has an exactly zero column for the shipped zero poses
    // (x = 0): d1 = 0, so every test would refuse and the fit would pay for them (measured: the upper-body solver
    // 2 % slower with the tests).  It keeps a / b.
    return joint_quat_of_A<N != 3>(A, hook, tab);
}
template <int N, typename Hook = NoHook>
RTG_DEV Q cal_joint_quat(const V (&Z)[N], const V (&M)[N], const Hook &hook = Hook{})
{
    bool unused;
    return cal_joint_quat<N>(Z, M, unused, hook);
}

// ------------------------------------------------ the host libm's float64 atan2 / hypot for the Euler split
// scipy's as_euler runs on the host libm (the reference and the oracle: glibc 2.35, x86-64).  With the device library's
// atan2 / hypot about a third of the angles differed from it in their last bits, and an angle that cancels to ~1e-16
// or sits on the +-pi wrap carries that bit into float32 (tests/test_gpu_other_solvers.py).  RTG_EULER_LIBM:
//  * hypot as that libm computes it, bit for bit (libm_hypot_f64 below);
//  * atan2 evaluated in double-double and rounded once (cr_atan2_f64).  The quotient, the reduction against a table of
//    atan(k / 32) and r - r^3 / 3 are double-double (~2^-100); the tail of the series from r^5 on is plain double, which
//    leaves ~2^-79 relative to the result.  So the result is the correctly rounded one unless the exact value lies
//    within ~2^-79 of a rounding boundary (about one argument in 2^25); no fallback catches those.  Against a 300-bit
//    evaluation 0 of 4000 results were misrounded.  glibc's own atan2 is not correctly rounded: it differs from this
//    one on 7.4e-4 of random arguments, and that much of a difference from the oracle remains.
// Another libm (an older or newer glibc, its FMA build of atan2, another platform's) may round differently: the
// bit-exact comparisons with the oracle hold against the libm named here.
struct DD { double h, l; };
RTG_DEV DD dd_fast_sum(double a, double b) { const double s = a + b; return DD{s, b - (s - a)}; }   // |a| >= |b|
RTG_DEV DD dd_two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return DD{s, (a - (s - bb)) + (b - bb)};
}
RTG_DEV DD dd_two_prod(double a, double b) { const double p = a * b; return DD{p, __builtin_fma(a, b, -p)}; }
RTG_DEV DD dd_add(DD a, DD b)
{
    const DD s = dd_two_sum(a.h, b.h), t = dd_two_sum(a.l, b.l);
    const DD u = dd_fast_sum(s.h, s.l + t.h);
    return dd_fast_sum(u.h, u.l + t.l);
}
RTG_DEV DD dd_neg(DD a) { return DD{-a.h, -a.l}; }
RTG_DEV DD dd_mul(DD a, DD b)
{
    const DD p = dd_two_prod(a.h, b.h);
    return dd_fast_sum(p.h, p.l + __builtin_fma(a.h, b.l, a.l * b.h));
}
RTG_DEV DD dd_div(DD a, DD b)
{
    // one division: q1 from the reciprocal (any approximation good to ~2^-50 will do), its remainder exact through the
    // fma products, the second quotient digit from the same reciprocal: a / b to ~2^-100
    const double inv = 1.0 / b.h;
    const double q1 = a.h * inv;
    const DD p = dd_two_prod(q1, b.h);
    const double r = (((a.h - p.h) - p.l) + a.l) - q1 * b.l;
    return dd_fast_sum(q1, r * inv);
}
// atan(k / 32), k = 0 .. 32, as double-double
RTG_DEV DD dd_atan_tab(int k)
{
    static constexpr double T[33][2] = {
    {0x0.0p+0, 0x0.0p+0},
    {0x1.ffd55bba97625p-6, -0x1.5ec431444912cp-60},
    {0x1.ff55bb72cfdeap-5, -0x1.c934d86d23f1dp-60},
    {0x1.7ee182602f10fp-4, -0x1.cfb654c0c3d98p-58},
    {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59},
    {0x1.3d6eee8c6626cp-3, 0x1.61a3b0ce9281bp-57},
    {0x1.7b97b4bce5b02p-3, 0x1.347b0b4f881cap-58},
    {0x1.b90d7529260a2p-3, 0x1.17b10d2e0e5abp-61},
    {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},
    {0x1.18bf5a30bf178p-2, 0x1.30ca4748b1bf9p-57},
    {0x1.362773707ebccp-2, -0x1.963a544b672d8p-57},
    {0x1.530ad9951cd4ap-2, -0x1.2566480884082p-57},
    {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56},
    {0x1.8b24d394a1b25p-2, 0x1.b6d0ba3748fa8p-56},
    {0x1.a64eec3cc23fdp-2, -0x1.24dec1b50b7ffp-56},
    {0x1.c0db4c94ec9f0p-2, -0x1.cc1ce70934c34p-56},
    {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56},
    {0x1.f40dd0b541418p-2, -0x1.a3992dc382a23p-57},
    {0x1.0657e94db30d0p-1, -0x1.d5b495f6349e6p-56},
    {0x1.1255d9bfbd2a9p-1, -0x1.2bdaee1c0ee35p-58},
    {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},
    {0x1.2958e59308e31p-1, -0x1.09e73b0c6c087p-56},
    {0x1.345f01cce37bbp-1, 0x1.1021137c71102p-55},
    {0x1.3f13fb89e96f4p-1, 0x1.ecf8b492644f0p-56},
    {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56},
    {0x1.538f57b89061fp-1, -0x1.1bb74abda520cp-55},
    {0x1.5d58987169b18p-1, 0x1.0028e4bc5e7cap-57},
    {0x1.66d663923e087p-1, -0x1.6ea6febe8bbbap-56},
    {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56},
    {0x1.78f6bbd5d315ep-1, 0x1.406a089803740p-55},
    {0x1.819d0b7158a4dp-1, -0x1.bf76229d3b917p-56},
    {0x1.89ff5ff57f1f8p-1, -0x1.55b9a5e177a1bp-55},
    {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55}};
    return DD{T[k][0], T[k][1]};
}
RTG_DEV DD dd_atan01(DD t)   // atan of 0 <= t <= 1
{
    const int k = (int)__builtin_rint(t.h * 32.0);
    DD r = t;
    if (k != 0) {
        const double c = (double)k * 0.03125;
        const DD num = dd_add(t, DD{-c, 0.0});
        const DD tc = dd_mul(t, DD{c, 0.0});
        r = dd_div(num, dd_add(DD{1.0, 0.0}, tc));
    }
    // atan(r), |r| <= 1/64 + : r - r^3 / 3 in double-double, the tail r^5/5 - ... - r^19/19 in double
    const DD r2 = dd_mul(r, r);
    const DD third = dd_mul(dd_mul(r2, r), DD{0x1.5555555555555p-2, 0x1.5555555555555p-56});
    const double z = r2.h;
    double p = -1.0 / 19.0;
    p = __builtin_fma(p, z, 1.0 / 17.0);
    p = __builtin_fma(p, z, -1.0 / 15.0);
    p = __builtin_fma(p, z, 1.0 / 13.0);
    p = __builtin_fma(p, z, -1.0 / 11.0);
    p = __builtin_fma(p, z, 1.0 / 9.0);
    p = __builtin_fma(p, z, -1.0 / 7.0);
    p = __builtin_fma(p, z, 1.0 / 5.0);
    const double tail = p * (z * z) * r.h;
    DD a = dd_add(r, dd_neg(third));
    a = dd_add(a, DD{tail, 0.0});
    return dd_add(dd_atan_tab(k), a);
}
RTG_DEV double cr_atan2_f64(double y, double x)
{
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const double lo = ax < ay ? ax : ay, hi = ax < ay ? ay : ax;
    // zeros, infinities, NaN and ratios beyond 2^+-200 (where the answer is a constant or the quotient itself): the library's
    if (!(lo > 0.0) || !(hi < 0x1p900) || !(lo > 0x1p-900) || lo < hi * 0x1p-200) return ::atan2(y, x);
    DD a = dd_atan01(dd_div(DD{lo, 0.0}, DD{hi, 0.0}));
    if (ay > ax) a = dd_add(DD{0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54}, dd_neg(a));
    if (x < 0.0) a = dd_add(DD{0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53}, dd_neg(a));
    return __builtin_copysign(a.h + a.l, y);
}
// hypot as glibc 2.35 and later compute it where the compiler has no fused multiply-add (the x86-64 baseline build):
// the algorithm of C. F. Borges, "An Improved Algorithm for hypot(a, b)" (arXiv:1904.09481: the plain square root,
// then one correction step from differences that are exact in floating point), in the order of operations of the
// non-FMA kernel of glibc's sysdeps/ieee754/dbl-64/e_hypot.c -- restated like glibc's e_atan2f.c above, because the
// reference's values are that libm's.  Bit-identical with that libm's
// hypot on 2e7 random arguments (host run).  It is not correctly rounded (0.45 % of random arguments), which is why a
// correctly rounded hypot would not do.  Arguments outside [2^-500, 2^500], where libm rescales, take the library's.
RTG_DEV double libm_hypot_f64(double x, double y)
{
    double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    if (ax < ay) { const double t = ax; ax = ay; ay = t; }
    if (!(ax < 0x1p500) || !(ay > 0x1p-500)) return ::hypot(x, y);   // inf, NaN, zeros, its scaled ranges
    if (ay <= ax * 0x1p-54) return ax + ay;
    double h = __builtin_sqrt(ax * ax + ay * ay), t1, t2;
    if (h <= 2.0 * ay) {
        const double delta = h - ay;
        t1 = ax * (2.0 * delta - ax);
        t2 = (delta - 2.0 * (ax - ay)) * delta;
    } else {
        const double delta = h - ax;
        t1 = 2.0 * delta * (ax - 2.0 * ay);
        t2 = (4.0 * delta - ay) * ay + delta * delta;
    }
    h -= (t1 + t2) / (2.0 * h);
    return h;
}
RTG_DEV double euler_atan2(double y, double x) { return RTG_EULER_LIBM ? cr_atan2_f64(y, x) : ::atan2(y, x); }
RTG_DEV double euler_hypot(double x, double y) { return RTG_EULER_LIBM ? libm_hypot_f64(x, y) : ::hypot(x, y); }

// ------------------------------------------------ scipy Rotation (float64)
// from_quat(q).as_euler(seq): quaternion method of Bernardes & Viollet (2022),
// as scipy 1.15 implements it; seq given as axis indices + intrinsic flag.  Returns true when from_quat would
// refuse q: its float64 norm is not > 0 (all four components zero, or a NaN) -- scipy raises
// "ValueError: Found zero norm quaternions in `quat`." there (transform3d.py:53).
RTG_DEV bool scipy_as_euler(Q qf, int s0, int s1, int s2, bool extrinsic, double ang[3])
{
    double q[4] = {(double)qf.x, (double)qf.y, (double)qf.z, (double)qf.w};
    const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const bool refused = !(nrm > 0.0);
    q[0] /= nrm; q[1] /= nrm; q[2] /= nrm; q[3] /= nrm;
    int i = extrinsic ? s0 : s2, j = s1, k = extrinsic ? s2 : s0;
    const bool symmetric = i == k;
    if (symmetric) k = 3 - i - j;
    const int sign = (i - j) * (j - k) * (k - i) / 2;
    const double qi = i == 0 ? q[0] : (i == 1 ? q[1] : q[2]);
    const double qj = j == 0 ? q[0] : (j == 1 ? q[1] : q[2]);
    const double qk = k == 0 ? q[0] : (k == 1 ? q[1] : q[2]);
    double a, b, c, d;
    if (symmetric) {
        a = q[3]; b = qi; c = qj; d = qk * sign;
    } else {
        a = q[3] - qj; b = qi + qk * sign; c = qj + q[3]; d = qk * sign - qi;
    }
    ang[1] = 2.0 * euler_atan2(euler_hypot(c, d), euler_hypot(a, b));
    int kase = 0;
    if (fabs(ang[1]) <= 1e-7) kase = 1;
    else if (fabs(ang[1] - M_PI) <= 1e-7) kase = 2;
    const double half_sum = euler_atan2(b, a), half_diff = euler_atan2(d, c);
    if (kase == 0) {
        ang[0] = half_sum - half_diff;
        ang[2] = half_sum + half_diff;
    } else if (extrinsic) {
        ang[2] = 0.0;
        ang[0] = kase == 1 ? 2.0 * half_sum : -2.0 * half_diff;
    } else {
        ang[0] = 0.0;
        ang[2] = kase == 1 ? 2.0 * half_sum : 2.0 * half_diff;
    }
    if (!symmetric) {
        ang[2] *= sign;
        ang[1] -= M_PI / 2.0;
    }
    if (!extrinsic) { const double tt = ang[0]; ang[0] = ang[2]; ang[2] = tt; }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (ang[t] < -M_PI) ang[t] += 2.0 * M_PI;
        else if (ang[t] > M_PI) ang[t] -= 2.0 * M_PI;
    }
    return refused;
}

// from_euler(axis, angle).as_quat() for one elementary rotation, cast to float32
RTG_DEV Q elementary_quat(int axis, double angle)
{
    const double h = angle / 2.0;
    const SC t = cr_sincos(h);
    const float s = t.s, c = t.c;
    return Q{axis == 0 ? s : 0.0f, axis == 1 ? s : 0.0f, axis == 2 ? s : 0.0f, c};
}

// ---- the 'XYZ' split of the solvers without atan2 (round 5)
// scipy's as_euler('XYZ') (intrinsic; scipy_as_euler with i = 2, j = 1, k = 0, sign -1) of q = (x, y, z, w) gives,
// with a = w - y, b = z - x, c = w + y, d = -(x + z) and hs = atan2(b, a), hd = atan2(d, c):
//   X: -(hs + hd)   Y: 2 atan2(|c + id|, |a + ib|) - pi/2   Z: hs - hd,   each wrapped into [-pi, pi]
// and each elementary quaternion is (sin A/2, cos A/2).  Every A is the principal argument of a complex number whose
// half angle needs no trigonometry:  e^{-i(hs + hd)} ~ conj((a + ib)(c + id)) = (ac - bd) - i(ad + bc);
// e^{i(hs - hd)} ~ (a + ib)(c - id) = (ac + bd) + i(bc - ad);  and e^{i A_Y} ~ m + 2i(yw + xz) with
// m = |a + ib| |c + id| (the modulus of the other two; n2 = |q|^2 is this one's).  For z = re + i im of modulus M,
// u = M + |re| (no cancellation) and t = 1 / sqrt(2 M u):  re >= 0: (sin, cos)(A/2) = (im t, u t);
// re < 0: (sign(im) u t, |im| t).  The products of the exact f64 differences a..d are single-rounded (fma), so every
// output is within 2^-48 of its value; the reference's own f64 pipeline (normalise, hypot, atan2, the angle sums,
// the wrap, sin / cos) is within ~2^-50 (1 + 1/|a + ib| + 1/|c + id|) |q| absolute.  An output is accepted when its
// f32 rounding is the same at +-2^-49 (1 + ...) -- the first version, with a fixed 2^-47, differed from the
// restatement on 5,892 of 2^30 near-gimbal quaternions (check [7]); otherwise -- and for n2 not > 0 (scipy
// refuses), NaN / inf, the gimbal cases (m < 1e-6 n2:
// scipy's 1e-7 tests), the wrap boundary (re < 0 with |im| < 2^-30 M) and im == 0 -- the scipy restatement below runs
// (quat_in_xyz_axis).  tools/check_fastmath.hip [7] compares the two on 2^30 quaternions.
RTG_DEV double rsq_nr(double v)   // 1 / sqrt(v), v > 0 finite: v_rsq_f64 (2^-23) and two Newton steps
{
    double r = __builtin_amdgcn_rsq(v);
    const double h = 0.5 * v;
    r = r * __builtin_fma(-h * r, r, 1.5);
    r = r * __builtin_fma(-h * r, r, 1.5);
    return r;
}
RTG_DEV bool f32_round_abs_safe(double y, double E, float &out)   // every value within E of y rounds alike
{
    out = (float)y;
    return (float)(y - E) == (float)(y + E);
}
// (sin, cos) of half the principal argument of re + i im (modulus M > 0), given t = 1 / sqrt(2 M u) with
// u = M + |re|; false when the rounding test at +-E or the wrap boundary declines
RTG_DEV bool half_arg(double re, double im, double M, double u, double t, double E, float &s, float &c)
{
    const double P = u * t, Qv = im * t;
    const bool pos = re >= 0.0;
    const double sv = pos ? Qv : __builtin_copysign(P, im), cv = pos ? P : __builtin_fabs(Qv);
    bool ok = f32_round_abs_safe(sv, E, s);
    ok = f32_round_abs_safe(cv, E, c) && ok;
    return ok && im != 0.0 && (pos || __builtin_fabs(im) >= 0x1p-30 * M);
}
RTG_DEV bool quat_in_xyz_fast(Q qf, Q out[3])
{
    const double X = qf.x, Y = qf.y, Z = qf.z, W = qf.w;
    const double a = W - Y, b = Z - X, c = W + Y, d = -(X + Z);   // exact: f32 operands
    const double n2 = __builtin_fma(W, W, __builtin_fma(Z, Z, __builtin_fma(Y, Y, X * X)));
    const double rab2 = __builtin_fma(b, b, a * a), rcd2 = __builtin_fma(d, d, c * c);
    const double m2 = rab2 * rcd2;
    const double m = m2 * rsq_nr(m2);
    const double bd = b * d, ad = a * d, bc = b * c;
    // Y: re = m, im = 2 (yw + xz), modulus n2
    const double u1 = n2 + m, t1 = rsq_nr(2.0 * n2 * u1);
    // The reference's a..d carry ~2^-52 |q| of rounding (its normalised q), which its atan2 of (b, a) / (d, c)
    // amplifies by |q| / |a + ib| and |q| / |c + id|: near gimbal lock the margin widens with
    // 1 / |a + ib| + 1 / |c + id| = sqrt(2 n2 u1) / m = 1 / (t1 m)
    const double E = 0x1p-49 * (1.0 + __builtin_amdgcn_rcp(t1 * m));
    float sx, cx, sy, cy, sz, cz;
    bool ok = n2 > 0.0 && n2 < 0x1p1000 && m >= 1e-6 * n2;
    ok = half_arg(m, 2.0 * __builtin_fma(Y, W, X * Z), n2, u1, t1, E, sy, cy) && ok;
    const double re0 = __builtin_fma(a, c, -bd), re2 = __builtin_fma(a, c, bd);
    const double u0 = m + __builtin_fabs(re0), u2 = m + __builtin_fabs(re2);
    ok = half_arg(re0, -__builtin_fma(a, d, bc), m, u0, rsq_nr(2.0 * m * u0), E, sx, cx) && ok;
    ok = half_arg(re2, __builtin_fma(b, c, -ad), m, u2, rsq_nr(2.0 * m * u2), E, sz, cz) && ok;
    out[0] = Q{sx, 0.0f, 0.0f, cx};
    out[1] = Q{0.0f, sy, 0.0f, cy};
    out[2] = Q{0.0f, 0.0f, sz, cz};
    return ok;
}

// quat_in_xyz_axis (transform3d.py:52-59); true where the reference raises (scipy_as_euler)
RTG_DEV bool quat_in_xyz_axis(Q q, int s0, int s1, int s2, bool extrinsic, Q out[3])
{
    double ang[3];
    const bool refused = scipy_as_euler(q, s0, s1, s2, extrinsic, ang);
    out[0] = elementary_quat(s0, ang[0]);
    out[1] = elementary_quat(s1, ang[1]);
    out[2] = elementary_quat(s2, ang[2]);
    return refused;
}
// quat_in_xyz_axis(q, 'XYZ') as the solvers call it (full_body_pos_retargeter.py:142/165, full_body_retargeter.py
// :121/138): the atan2-free form above, the scipy restatement where it declines.  Same values (check [7]).
RTG_DEV bool quat_in_xyz_intrinsic(Q q, Q out[3])
{
    bool refused = false;
    if (__builtin_expect(!quat_in_xyz_fast(q, out), 0)) refused = quat_in_xyz_axis(q, 0, 1, 2, false, out);
    return refused;
}

// ------------------------------------------------ arm joint maps
// Frame-independent halves of cal_shoulderPR / cal_elbowP_and_shoulderY:
// theta0 / phi0 depend only on the zero-pose vector v0 and are evaluated once.
struct ArmZero { float th0, ph0; };

RTG_DEV ArmZero shoulder_zero(V v0)
{
    const V ex{1.f, 0.f, 0.f}, ey{0.f, 1.f, 0.f};
    const V v0p = proj_in_plane(v0, ey);
    return ArmZero{radians_between(ex, v0p, ey), radians_between(v0p, v0, cross3(v0p, ey))};
}
RTG_DEV ArmZero elbow_zero(V v0)
{
    const V ex{1.f, 0.f, 0.f}, ez{0.f, 0.f, 1.f};
    const V v0p = proj_in_plane(v0, ez);
    return ArmZero{radians_between(ex, v0p, ez), radians_between(v0p, v0, cross3(ez, v0p))};
}

// cal_shoulderPR (SHOULDER; full_body_pos_retargeter.py:246-278: pitch about ey, then roll about ex) /
// cal_elbowP_and_shoulderY (:220-243: yaw about ez, then the elbow about ey) of NA arms at once.  Per arm:
//   v1r = v1 in the parent's frame, v1p = its projection into the plane of the first angle (normal pn);
//   first angle = radians_between(ex, v1p, pn) - th0: ex and pn are exact unit axes, whose normalisation is the
//     identity (lnorm3 = sqrt(1) = 1, x * RN(1/1) = x), so only v1p is normalised -- the same bits, 2/3 fewer divides;
//   second angle = radians_between(v1p, v1r, n) - ph0, with the unit v1p of the first angle.
template <bool SHOULDER, int NA, typename Tab = NoTab>
RTG_DEV void arm_pair_n(const V (&v1)[NA], const ArmZero (&z0)[NA], const Q (&parent)[NA], Q (&first)[NA],
                        Q (&second)[NA], Tab tab = Tab{})
{
    const V ex{1.f, 0.f, 0.f}, ey{0.f, 1.f, 0.f}, ez{0.f, 0.f, 1.f};
    const V pn = SHOULDER ? ey : ez;   // the plane of the first angle
    V vec[3 * NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const V v1r = qrotate(qconj(parent[a]), v1[a]);
        const V v1p = proj_in_plane(v1r, pn);
        vec[3 * a] = v1p;
        vec[3 * a + 1] = v1r;
        vec[3 * a + 2] = SHOULDER ? cross3(v1p, ey) : cross3(ez, v1p);
    }
    V u[3 * NA];
    vunit_n<3 * NA>(vec, u);
    float c[2 * NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        c[2 * a] = clamp_lohi(dot3(ex, u[3 * a]), -1.0f, 1.0f);                  // radians_between(ex, v1p, pn)
        c[2 * a + 1] = clamp_lohi(dot3(u[3 * a], u[3 * a + 1]), -1.0f, 1.0f);    // radians_between(v1p, v1r, n)
    }
    float ac[2 * NA];
    cr_acos_n<2 * NA>(c, ac);
    float ang[2 * NA];
    V ax[2 * NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        ang[2 * a] = ac[2 * a] * tsign(dot3(pn, cross3(ex, u[3 * a]))) - z0[a].th0;
        ax[2 * a] = pn;
        ang[2 * a + 1] = ac[2 * a + 1] * tsign(dot3(u[3 * a + 2], cross3(u[3 * a], u[3 * a + 1]))) - z0[a].ph0;
        ax[2 * a + 1] = SHOULDER ? ex : ey;
    }
    Q q[2 * NA];
    qfrom_angle_unit_axis_n<2 * NA>(ang, ax, q, tab);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        first[a] = q[2 * a];
        second[a] = q[2 * a + 1];
    }
}
template <bool SHOULDER, typename Tab>
RTG_DEV void arm_pair_1(V v1, ArmZero z0, Q parent, Q &first, Q &second, Tab tab)
{
    const V v[1] = {v1};
    const ArmZero z[1] = {z0};
    const Q par[1] = {parent};
    Q a[1], b[1];
    arm_pair_n<SHOULDER, 1>(v, z, par, a, b, tab);
    first = a[0];
    second = b[0];
}
template <typename Tab = NoTab>
RTG_DEV void shoulder_pr(V v1, ArmZero z0, Q parent, Q &pitch, Q &roll, Tab tab = Tab{})
{
    arm_pair_1<true>(v1, z0, parent, pitch, roll, tab);
}
template <typename Tab = NoTab>
RTG_DEV void elbow_py(V v1, ArmZero z0, Q parent, Q &yaw, Q &elbow, Tab tab = Tab{})
{
    arm_pair_1<false>(v1, z0, parent, yaw, elbow, tab);
}

// s / 5 (round 22): region [C] behind the numerator's test; RN(1 / 5) is its own refinement.  The sum is signed and
// can be -0, which the test refuses with every other value under kNumLo
RTG_DEV float fdiv_by5(float s)
{
    float q = fdiv1_const(s, 5.0f, 0x1.99999ap-3f);
    if (__builtin_expect(!fdiv1_in_c(s), 0)) q = s / 5.0f;
    return q;
}
// torch sum of 5 elements (cascade reduce order, measured) / 5
RTG_DEV float mean5(float v0, float v1, float v2, float v3, float v4)
{
    return fdiv_by5(((((v0 + v4) + v1) + v2) + v3));
}

// Hu_v5.Hu_DOF_AXIS (retarget/robot_config/Hu_v5.py:12-18), dof k <-> link k+1
__constant__ static const int8_t kHuDofAxis[30] = {2, 0, 1, 1, 1, 2, 0, 1, 1, 1, 2, 1, 0, 2, 1,
                                                   0, 1, 2, 1, 1, 1, 0, 2, 1, 0, 1, 2, 1, 1, 2};
__host__ __device__ constexpr int hu_dof_axis(int k)
{
    // compile-time table for unrolled uses; avoids a constant-memory load
    constexpr int8_t t[30] = {2, 0, 1, 1, 1, 2, 0, 1, 1, 1, 2, 1, 0, 2, 1,
                              0, 1, 2, 1, 1, 1, 0, 2, 1, 0, 1, 2, 1, 1, 2};
    return t[k];
}

}  // namespace rtg

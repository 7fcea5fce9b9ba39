// rtg_fk_adjoint.cuh -- one joint of the kinematics' reverse sweep and the joint-angle model's local rotation, shared
// by the adjoint kernels (rtg_fk_grad.hip) and the fused keypoint fit (rtg_dof_fit.hip).  The derivation is in the
// header comment of rtg_fk_grad.hip.  No operation order is owed to anyone here: explicit fmaf, the device sincosf.
#pragma once
#include "rtg_fk_group.cuh"

namespace rtg {

RTG_DEV float fdot4(const Q &a, const Q &b)
{
    return __builtin_fmaf(a.w, b.w, __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)));
}
RTG_DEV float fdot3(const V &a, const V &b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }

struct JointAdj {
    Q gp;    // this joint's contribution to its parent's rotation adjoint
    Q lqb;   // the adjoint of its local rotation
};
// one joint of the reverse sweep: gb, pb are the joint's complete adjoints (its own upstream rows plus its children's
// contributions)
RTG_DEV JointAdj joint_adjoint(const Q &Gp, const Q &Gj, const Q &lq, const V &zl, const Q &gb, const V &pb)
{
    const Q u = qmul(Gp, lq);
    const float n = __builtin_sqrtf(fdot4(u, u));
    const float f = fdot4(u, Gj) < 0.0f ? -1.0f : 1.0f;
    Q ub;
    if (!(n < 1e-9f)) {   // NaN takes the regular path and stays NaN
        const float r = f / n, d = fdot4(gb, Gj);
        ub = Q{r * __builtin_fmaf(-d, Gj.x, gb.x), r * __builtin_fmaf(-d, Gj.y, gb.y), r * __builtin_fmaf(-d, Gj.z, gb.z),
               r * __builtin_fmaf(-d, Gj.w, gb.w)};
    } else {   // quat_unit divides by clamp(|u|, 1e-9): a constant there
        const float r = f * 1e9f;
        ub = Q{r * gb.x, r * gb.y, r * gb.z, r * gb.w};
    }
    JointAdj out;
    out.gp = qmul(ub, qconj(lq));
    out.lqb = qmul(qconj(Gp), ub);
    // r = q v conj(q) = (w^2 - a.a) v + 2 (a.v) a + 2 w (a x v) for q = (a, w), unit or not; with g = pb:
    //   d(g.r)/dw = 2 (w g.v + a.(v x g)),   d(g.r)/da = 2 (-(g.v) a + (a.v) g + (g.a) v + w (v x g))
    const V a{Gp.x, Gp.y, Gp.z};
    const float w = Gp.w;
    const V c{zl.y * pb.z - zl.z * pb.y, zl.z * pb.x - zl.x * pb.z, zl.x * pb.y - zl.y * pb.x};
    const float gv = fdot3(pb, zl), av = fdot3(a, zl), ga = fdot3(pb, a);
    out.gp.x += 2.0f * __builtin_fmaf(w, c.x, __builtin_fmaf(ga, zl.x, __builtin_fmaf(av, pb.x, -gv * a.x)));
    out.gp.y += 2.0f * __builtin_fmaf(w, c.y, __builtin_fmaf(ga, zl.y, __builtin_fmaf(av, pb.y, -gv * a.y)));
    out.gp.z += 2.0f * __builtin_fmaf(w, c.z, __builtin_fmaf(ga, zl.z, __builtin_fmaf(av, pb.z, -gv * a.z)));
    out.gp.w += 2.0f * __builtin_fmaf(w, gv, fdot3(a, c));
    return out;
}

// the joint-angle model's local rotation and its derivative: lq = (sn e_ax, cs), d lq / d a = (cs e_ax, -sn) / 2, with
// quat_from_angle_axis's w >= 0 flip already in sn, cs.  The clip is the forward's (clamp_st).
struct AngleRot {
    float sn, cs;
    int ax;
};
template <bool CLIP>
RTG_DEV AngleRot angle_rot(float a, int ax, float lo, float hi)
{
    if (CLIP) a = clamp_st(a, lo, hi);
    float sn, cs;
    sincosf(a * 0.5f, &sn, &cs);
    const float f = cs < 0.0f ? -1.0f : 1.0f;
    return AngleRot{f * sn, f * cs, ax};
}
RTG_DEV Q angle_quat(const AngleRot &r)
{
    return Q{r.ax == 0 ? r.sn : 0.0f, r.ax == 1 ? r.sn : 0.0f, r.ax == 2 ? r.sn : 0.0f, r.cs};
}
RTG_DEV float angle_grad(const AngleRot &r, const Q &lqb)
{
    const float v = r.ax == 0 ? lqb.x : (r.ax == 1 ? lqb.y : lqb.z);
    return 0.5f * __builtin_fmaf(r.cs, v, -r.sn * lqb.w);
}

}  // namespace rtg

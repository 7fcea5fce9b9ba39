// rtg_fk_grad.hip -- the adjoints of the forward kinematics kernels (rtg_fk.hip): a reverse sweep over the same
// parent-indexed tree, for the joint-angle model (k_dof_fk_group / k_dof_fk_walk) and for plain FK (k_fk_group /
// k_fk, non-STATE).  The reference's kinematics are plain torch and differentiable (kinematics.py:13-39,
// hu_forward_model.py:17-33); these kernels compute what its autograd computes.
//
// Forward, per joint j >= 1 with parent p:   u = G_p o lq_j,   G_j = f u / |u| (f = +-1 so that w >= 0),
// P_j = qrotate(G_p, zl_j) + P_p;  the root is G_0 = local[0] (as given, unnormalised), P_0 = the root translation.
// Reverse, children first, with the adjoints Gb, Pb started from the upstream gradients:
//   Pb_p += Pb_j
//   Gb_p += (d qrotate(G_p, zl_j) / d G_p)^T Pb_j            qrotate is q v conj(q): |q|^2 times a rotation
//   ub    = f (Gb_j - (Gb_j . G_j) G_j) / |u|                through the normalisation (no projection under its clamp)
//   Gb_p += ub o conj(lq_j),   lqb_j = conj(G_p) o ub        the two transposes of the Hamilton product
// G_p and G_j come from the saved forward output, |u| is recomputed, and f is the sign of u . G_j (the forward's own
// choice, whatever the last bit of the rebuilt lq_j).  The joint-angle model rebuilds lq_j = f' (sin(a'/2) e, cos(a'/2))
// from the (clipped) angle and returns ab = lqb_j . d lq_j / d a; the clip is straight-through, so only a' is clamped.
// No operation order is owed to anyone here (there are no reference bits to match): explicit fmaf, the device sincosf.
#include "rtg_device.cuh"
#include "rtg_fk_adjoint.cuh"
#include "rtg_fk_group.cuh"

namespace rtg {

// ----------------------------------------------------------------------------
// Lane groups (J <= kGroupMaxJ): the forward's tile -- F frames per wave, 64 / F lanes per frame -- and its schedule
// run backwards: at reverse step s, sub-lane u of each frame's group takes the joint the forward composed at step s.
// Its children were composed at later forward steps, so they are already done.  LDS images, all rows as coalesced
// pieces:
//   G [F J] float4   the saved forward rotations
//   A [F J] float4   in: the upstream rotation gradient rows (zeros when absent); a finished joint leaves its
//                    contribution to its parent's adjoint here, the root its complete adjoint
//   P [F J 3] float  in: the upstream position gradient rows; a finished joint leaves its complete adjoint here
//   X                DOF: the angles [F (J - 1)] float, replaced by their gradients; plain FK: the local rotations
//                    [F J] float4, replaced by theirs
// Without an upstream rotation gradient (ROT = false: a loss on positions only, the common case) A has nothing to
// hold at the start, and a joint's saved rotation is last read when the joint itself is processed (its children, who
// read it as their parent's, come first): the joint's contribution goes into its G row, and the A image is not
// allocated -- a third less LDS, more tiles per CU.  The sums start from +0 and add the same terms in the same order,
// so the bits are those of an explicit zero gradient.
// Siblings: a joint does not add into its parent's rows.  The parent, when its turn comes, pulls its children's rows
// in ascending index order (first child / next sibling links, in the schedule entries and a J-entry table), so every
// sum has one fixed order whatever the schedule, and no LDS atomic is needed.
// ----------------------------------------------------------------------------
template <int F>
constexpr int pos_pieces() { return (3 * Grp<F>::NR + 3) / 4; }   // float4 pieces per lane of a tile's position rows

__host__ __device__ inline size_t bwd_group_lds_floats(int J, int F, int steps, bool dof, bool rot)
{
    return (size_t)(rot ? 8 : 4) * F * J + pad16f((size_t)3 * F * J) + (dof ? pad16f((size_t)F * (J - 1)) + (size_t)4 * J : (size_t)4 * F * J) +
           (size_t)steps * (64 / F) * 8 + pad16f((size_t)J);
}

template <bool DOF, bool CLIP, bool ROT, int F>
__global__ __launch_bounds__(64) void k_fk_bwd_group(TopoView T, DofView D, const float *__restrict__ lq_in,
                                                     const float *__restrict__ g_rot, const float *__restrict__ grad_g_rot,
                                                     const float *__restrict__ grad_g_pos, int64_t B,
                                                     float *__restrict__ lq_grad, float *__restrict__ grad_root_rot,
                                                     float *__restrict__ grad_root_t)
{
    extern __shared__ __attribute__((aligned(16))) float bw_lds[];
    using G = Grp<F>;
    constexpr int NP = pos_pieces<F>();
    const int J = T.J, lane = (int)threadIdx.x, nd = J - 1;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = (int)((B - f0) < F ? (B - f0) : F);
    const int nrec = nfr * J, npos = 3 * nrec, nang = nfr * nd;
    f4v *Gi = reinterpret_cast<f4v *>(bw_lds);
    f4v *A = ROT ? Gi + F * J : Gi;
    float *P = bw_lds + (ROT ? 8 : 4) * F * J;
    float *X = P + pad16f((size_t)3 * F * J);
    f4v *X4 = reinterpret_cast<f4v *>(X);
    float *after = X + (DOF ? pad16f((size_t)F * nd) : (size_t)4 * F * J);
    f4v *ntab = reinterpret_cast<f4v *>(after);   // DOF: per joint {axis, lower, upper}
    GEnt *sch = reinterpret_cast<GEnt *>(after + (DOF ? 4 * J : 0));
    int *nsib = reinterpret_cast<int *>(sch + T.gsteps * G::L);

    // every global load of the tile first, then the LDS image
    GroupRows<F> rg, ra, rx;
    rg.load(g_rot + f0 * J * 4, nrec);
    if (ROT) ra.load(grad_g_rot + f0 * J * 4, nrec);
    if (!DOF) rx.load(lq_in + f0 * J * 4, nrec);
    float ang[G::NR];
    if (DOF) {
        const float *drow = lq_in + f0 * nd;   // J = 1: no angles, the host passes a readable dummy
#pragma unroll
        for (int k = 0; k < G::NR; ++k) {
            const int i = k * 64 + lane;
            ang[k] = drow[i < nang ? i : 0];
        }
    }
    const float *prow = grad_g_pos ? grad_g_pos + f0 * J * 3 : nullptr;
    const bool paligned = (reinterpret_cast<uintptr_t>(prow) & 15u) == 0;
    const int n4 = npos >> 2;
    f4v pv[NP];
    float ptail = 0.0f;
    if (prow && paligned) {
        const f4v *ps = reinterpret_cast<const f4v *>(prow);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = k * 64 + lane;
            pv[k] = ps[i < n4 ? i : 0];
        }
        if (4 * n4 + lane < npos) ptail = prow[4 * n4 + lane];
    }
    for (int i = lane; i < T.gsteps * G::L; i += 64) {
        const GEnt e = T.gsched[i];
        sch[i] = e;
        const int j = e.code & 0xFF;
        if (j != 0xFF) nsib[j] = (e.code >> 24) & 0xFF;
    }
    if (DOF) {
        for (int j = 1 + lane; j < J; j += 64)
            ntab[j] = f4v{__int_as_float(ld_const(D.axis + (j - 1))), CLIP ? ld_const(D.lower + (j - 1)) : 0.0f,
                          CLIP ? ld_const(D.upper + (j - 1)) : 0.0f, 0.0f};
    }
    rg.to_lds(Gi, nrec);
    if (ROT) ra.to_lds(A, nrec);
    if (DOF) {
#pragma unroll
        for (int k = 0; k < G::NR; ++k) {
            const int i = k * 64 + lane;
            if (i < nang) X[i] = ang[k];
        }
    } else {
        rx.to_lds(X4, nrec);
    }
    if (!prow) {
        for (int i = lane; i < npos; i += 64) P[i] = 0.0f;
    } else if (paligned) {
        f4v *pd = reinterpret_cast<f4v *>(P);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int i = k * 64 + lane;
            if (i < n4) pd[i] = pv[k];
        }
        if (4 * n4 + lane < npos) P[4 * n4 + lane] = ptail;
    } else {
        for (int i = lane; i < npos; i += 64) P[i] = prow[i];
    }
    wave_sync();

    const int fr = lane >> G::LOG_L, sub = lane & (G::L - 1);
    const bool live = fr < nfr;
    const int base = fr * J;
    for (int s = T.gsteps - 1; s >= 0; --s) {
        const GEnt e = sch[s * G::L + sub];
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF) {
            f4v a = ROT ? A[base + j] : f4v{0.0f, 0.0f, 0.0f, 0.0f};
            float *pj = P + 3 * (base + j);
            V pb{pj[0], pj[1], pj[2]};
            for (int c = (e.code >> 16) & 0xFF; c != 0xFF; c = nsib[c]) {   // the children, ascending
                a += A[base + c];
                const float *pc = P + 3 * (base + c);
                pb.x += pc[0]; pb.y += pc[1]; pb.z += pc[2];
            }
            pj[0] = pb.x; pj[1] = pb.y; pj[2] = pb.z;
            if (j == 0) {   // the root is taken as given: its adjoints are the root gradients
                A[base] = a;
                if (!DOF) X4[base] = a;
            } else {
                const f4v gpv = Gi[base + p], gjv = Gi[base + j];
                const Q Gp{gpv.x, gpv.y, gpv.z, gpv.w}, Gj{gjv.x, gjv.y, gjv.z, gjv.w};
                const Q gb{a.x, a.y, a.z, a.w};
                const V zl{e.lx, e.ly, e.lz};
                if (DOF) {
                    const f4v t = ntab[j];
                    const AngleRot r = angle_rot<CLIP>(X[fr * nd + j - 1], __float_as_int(t.x), t.y, t.z);
                    const JointAdj o = joint_adjoint(Gp, Gj, angle_quat(r), zl, gb, pb);
                    A[base + j] = f4v{o.gp.x, o.gp.y, o.gp.z, o.gp.w};
                    X[fr * nd + j - 1] = angle_grad(r, o.lqb);
                } else {
                    const f4v lv = X4[base + j];
                    const JointAdj o = joint_adjoint(Gp, Gj, Q{lv.x, lv.y, lv.z, lv.w}, zl, gb, pb);
                    A[base + j] = f4v{o.gp.x, o.gp.y, o.gp.z, o.gp.w};
                    X4[base + j] = f4v{o.lqb.x, o.lqb.y, o.lqb.z, o.lqb.w};
                }
            }
        }
        wave_sync();   // this step's rows before the next step's parents pull them (other lanes)
    }

    if (lq_grad) {
        if (DOF) {
            float *gd = lq_grad + f0 * nd;
#pragma unroll
            for (int k = 0; k < G::NR; ++k) {
                const int i = k * 64 + lane;
                if (i < nang) gd[i] = X[i];
            }
        } else {
            f4v *dst = reinterpret_cast<f4v *>(lq_grad + f0 * J * 4);
#pragma unroll
            for (int k = 0; k < G::NR; ++k) {
                const int rec = k * 64 + lane;
                if (rec < nrec) st_out(dst + rec, X4[rec]);
            }
        }
    }
    if (grad_root_rot && lane < nfr) reinterpret_cast<f4v *>(grad_root_rot)[f0 + lane] = A[lane * J];
    if (grad_root_t && lane < 3 * nfr) {
        const int q = lane / 3;
        grad_root_t[f0 * 3 + lane] = P[3 * J * q + (lane - 3 * q)];
    }
}

// ----------------------------------------------------------------------------
// Lane walk (J > kGroupMaxJ): one frame per lane, joints J-1 ... 1 in turn, each adding into its parent's adjoint
// rows -- one lane, one order.  The adjoint rows of a frame (7 J floats) live in LDS, lane-interleaved, so a block
// walks as many frames as fit (fw <= 64 lanes of the wave; the others idle); the saved rotations and the angles /
// local rotations are read, and their gradients written, straight from / to the frame's rows.
// ----------------------------------------------------------------------------
constexpr size_t kWalkLdsBytes = 64 * 1024;
inline int bwd_walk_frames(int J)
{
    const size_t f = kWalkLdsBytes / ((size_t)28 * J);
    return (int)(f > 64 ? 64 : f);
}

template <bool DOF, bool CLIP>
__global__ __launch_bounds__(64) void k_fk_bwd_walk(TopoView T, DofView D, const float *__restrict__ lq_in,
                                                    const float *__restrict__ g_rot, const float *__restrict__ grad_g_rot,
                                                    const float *__restrict__ grad_g_pos, int64_t B, int fw,
                                                    float *__restrict__ lq_grad, float *__restrict__ grad_root_rot,
                                                    float *__restrict__ grad_root_t)
{
    extern __shared__ __attribute__((aligned(16))) float bw_lds[];
    const int J = T.J, lane = (int)threadIdx.x;
    const int64_t f = (int64_t)blockIdx.x * fw + lane;
    if (lane >= fw || f >= B) return;   // a lane touches only its own columns of the LDS rows: no barrier below
    f4v *A = reinterpret_cast<f4v *>(bw_lds);
    float *P = bw_lds + (size_t)4 * J * fw;
    const float *gr = g_rot + f * J * 4;
    for (int j = 0; j < J; ++j) {
        const Q a = grad_g_rot ? ld4(grad_g_rot + (f * J + j) * 4) : Q{0.0f, 0.0f, 0.0f, 0.0f};
        const V v = grad_g_pos ? ld3(grad_g_pos + (f * J + j) * 3) : V{0.0f, 0.0f, 0.0f};
        A[j * fw + lane] = f4v{a.x, a.y, a.z, a.w};
        P[(3 * j) * fw + lane] = v.x;
        P[(3 * j + 1) * fw + lane] = v.y;
        P[(3 * j + 2) * fw + lane] = v.z;
    }
    for (int j = J - 1; j > 0; --j) {
        const int p = ld_const(T.parents + j);
        const f4v a = A[j * fw + lane];
        const V pb{P[(3 * j) * fw + lane], P[(3 * j + 1) * fw + lane], P[(3 * j + 2) * fw + lane]};
        const Q Gp = ld4(gr + 4 * p), Gj = ld4(gr + 4 * j), gb{a.x, a.y, a.z, a.w};
        const V zl = ld_const(T.local_t + j);
        JointAdj o;
        if (DOF) {
            const AngleRot r = angle_rot<CLIP>(lq_in[f * (J - 1) + j - 1], ld_const(D.axis + (j - 1)),
                                               CLIP ? ld_const(D.lower + (j - 1)) : 0.0f,
                                               CLIP ? ld_const(D.upper + (j - 1)) : 0.0f);
            o = joint_adjoint(Gp, Gj, angle_quat(r), zl, gb, pb);
            if (lq_grad) lq_grad[f * (J - 1) + j - 1] = angle_grad(r, o.lqb);
        } else {
            o = joint_adjoint(Gp, Gj, ld4(lq_in + (f * J + j) * 4), zl, gb, pb);
            if (lq_grad) st4(lq_grad + (f * J + j) * 4, o.lqb);
        }
        A[p * fw + lane] += f4v{o.gp.x, o.gp.y, o.gp.z, o.gp.w};
        P[(3 * p) * fw + lane] += pb.x;
        P[(3 * p + 1) * fw + lane] += pb.y;
        P[(3 * p + 2) * fw + lane] += pb.z;
    }
    const f4v a0 = A[lane];
    if (!DOF && lq_grad) st4(lq_grad + f * J * 4, Q{a0.x, a0.y, a0.z, a0.w});
    if (grad_root_rot) st4(grad_root_rot + f * 4, Q{a0.x, a0.y, a0.z, a0.w});
    if (grad_root_t) st3(grad_root_t + f * 3, V{P[lane], P[fw + lane], P[2 * fw + lane]});
}

hipError_t launch_fk_backward(const TopoView &T, const DofView *D, bool clip, const float *lq_in, const float *g_rot,
                              const float *grad_g_rot, const float *grad_g_pos, int64_t B, float *lq_grad,
                              float *grad_root_rot, float *grad_root_t, hipStream_t s)
{
    const DofView dv = D ? *D : DofView{nullptr, nullptr, nullptr};
#define RTG_BWD_ARGS T, dv, lq_in, g_rot, grad_g_rot, grad_g_pos, B
#define RTG_BWD_OUTS lq_grad, grad_root_rot, grad_root_t
    if (T.gsched) {
        const int F = T.gF;
        const bool rot = grad_g_rot != nullptr;
        const size_t lds = sizeof(float) * bwd_group_lds_floats(T.J, F, T.gsteps, D != nullptr, rot);
        const dim3 g(grid_for(B, F)), b(64);
#define RTG_BWD_GROUP(DOF, CLIP, ROT, FR) \
    hipLaunchKernelGGL((k_fk_bwd_group<DOF, CLIP, ROT, FR>), g, b, lds, s, RTG_BWD_ARGS, RTG_BWD_OUTS)
#define RTG_BWD_GROUP_F(DOF, CLIP, ROT) \
    do { if (F == 16) RTG_BWD_GROUP(DOF, CLIP, ROT, 16); else RTG_BWD_GROUP(DOF, CLIP, ROT, 8); } while (0)
#define RTG_BWD_GROUP_R(DOF, CLIP) \
    do { if (rot) RTG_BWD_GROUP_F(DOF, CLIP, true); else RTG_BWD_GROUP_F(DOF, CLIP, false); } while (0)
        if (!D) RTG_BWD_GROUP_R(false, false);
        else if (clip) RTG_BWD_GROUP_R(true, true);
        else RTG_BWD_GROUP_R(true, false);
#undef RTG_BWD_GROUP_R
#undef RTG_BWD_GROUP_F
#undef RTG_BWD_GROUP
    } else {   // J > kGroupMaxJ: lane walk
        const int fw = bwd_walk_frames(T.J);
        if (fw < 1) return hipErrorInvalidValue;
        const size_t lds = (size_t)28 * T.J * fw;
        const dim3 g(grid_for(B, fw)), b(64);
        if (!D) hipLaunchKernelGGL((k_fk_bwd_walk<false, false>), g, b, lds, s, RTG_BWD_ARGS, fw, RTG_BWD_OUTS);
        else if (clip) hipLaunchKernelGGL((k_fk_bwd_walk<true, true>), g, b, lds, s, RTG_BWD_ARGS, fw, RTG_BWD_OUTS);
        else hipLaunchKernelGGL((k_fk_bwd_walk<true, false>), g, b, lds, s, RTG_BWD_ARGS, fw, RTG_BWD_OUTS);
    }
#undef RTG_BWD_ARGS
#undef RTG_BWD_OUTS
    return hipGetLastError();
}

}  // namespace rtg

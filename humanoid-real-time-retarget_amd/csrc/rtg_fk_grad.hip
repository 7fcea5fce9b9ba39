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
// Its children were composed at later forward steps, so they are already done.  The LDS images (BwdImages), all rows
// moved as coalesced pieces by the kit's row movers (rtg_fk_group.cuh).
// Without an upstream rotation gradient (ROT = false: a loss on positions only, the common case) A has nothing to
// hold at the start, and a joint's saved rotation is last read when the joint itself is processed (its children, who
// read it as their parent's, come first): the joint's contribution goes into its G row, and the A image is not
// allocated -- a third less LDS, more tiles per CU.  The sums start from +0 and add the same terms in the same order,
// so the bits are those of an explicit zero gradient.
// Siblings: a joint does not add into its parent's rows.  The parent, when its turn comes, pulls its children's rows
// in ascending index order (child_pull: first child / next sibling links, in the schedule entries and a J-entry
// table), so every sum has one fixed order whatever the schedule, and no LDS atomic is needed.
// ----------------------------------------------------------------------------
struct BwdImages {
    f4v *G;       // [F J] the saved forward rotations
    f4v *A;       // [F J] in: the upstream rotation gradient rows; a finished joint leaves its contribution to its
                  // parent's adjoint here, the root its complete adjoint.  Not ROT: the G image
    float *P;     // [F J 3] in: the upstream position gradient rows; a finished joint leaves its complete adjoint here
    float *X;     // DOF: [F (J - 1)] the angles, replaced by their gradients
    f4v *X4;      // plain FK: [F J] the local rotations, replaced by theirs
    f4v *ntab;    // DOF: [J] per joint {axis, lower, upper}
    GEnt *sch;    // [gsteps L] the schedule
    int *nsib;    // [J] the next-sibling table
    size_t floats;
    __host__ __device__ BwdImages(float *base, int J, int F, int steps, bool dof, bool rot)
    {
        LdsCarve c(base);
        G = c.take<f4v>((size_t)F * J);
        A = rot ? c.take<f4v>((size_t)F * J) : G;
        P = c.take<float>((size_t)3 * F * J);
        X = c.take<float>(dof ? (size_t)F * (J - 1) : 0);
        X4 = c.take<f4v>(dof ? 0 : (size_t)F * J);
        ntab = c.take<f4v>(dof ? J : 0);
        sch = c.take<GEnt>((size_t)steps * (64 / F));
        nsib = c.take<int>(J);
        floats = c.floats;
    }
};

template <bool DOF, bool CLIP, bool ROT, int F>
__global__ __launch_bounds__(64) void k_fk_bwd_group(TopoView T, DofView D, const float *__restrict__ lq_in,
                                                     const float *__restrict__ g_rot, const float *__restrict__ grad_g_rot,
                                                     const float *__restrict__ grad_g_pos, int64_t B,
                                                     float *__restrict__ lq_grad, float *__restrict__ grad_root_rot,
                                                     float *__restrict__ grad_root_t)
{
    extern __shared__ __attribute__((aligned(16))) float bw_lds[];
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x, nd = J - 1;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(B, f0);
    const int nrec = nfr * J, npos = 3 * nrec, nang = nfr * nd;
    const BwdImages I(bw_lds, J, F, T.gsteps, DOF, ROT);
    f4v *Gi = I.G, *A = I.A, *X4 = I.X4;
    float *P = I.P, *X = I.X;
    const f4v *ntab = I.ntab;
    const GEnt *sch = I.sch;
    const int *nsib = I.nsib;

    // every global load of the tile first, then the LDS image
    GroupRows<F> rg, ra, rx;
    ScalarRows<F> ang;
    PosRows<F> rp;
    rg.load(g_rot + f0 * J * 4, nrec);
    if (ROT) ra.load(grad_g_rot + f0 * J * 4, nrec);
    if (DOF) ang.load(lq_in + f0 * nd, nang);   // J = 1: no angles, the host passes a readable dummy
    else rx.load(lq_in + f0 * J * 4, nrec);
    const float *prow = grad_g_pos ? grad_g_pos + f0 * J * 3 : nullptr;
    if (prow) rp.load(prow, npos);
    group_sched_fill(T, G::L, I.sch, I.nsib);
    if (DOF) joint_tab_fill<CLIP, false>(D, J, I.ntab);
    rg.store(Gi, nrec);
    if (ROT) ra.store(A, nrec);
    if (DOF) ang.store(X, nang);
    else rx.store(X4, nrec);
    if (!prow) {
        for (int i = lane; i < npos; i += 64) P[i] = 0.0f;
    } else {
        rp.to_lds(P, prow, npos);
    }
    wave_sync();

    const int fr = lane >> G::LOG_L, sub = lane & (G::L - 1);
    const bool live = fr < nfr;
    const int base = fr * J;
    for (int s = T.gsteps - 1; s >= 0; --s) {
        const GEnt e = sch[s * G::L + sub];
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF) {
            V pb;
            const f4v a = child_pull(ROT ? A[base + j] : f4v{0.0f, 0.0f, 0.0f, 0.0f}, A, P, base, j, (e.code >> 16) & 0xFF, nsib, pb);
            if (j == 0) {   // the root is taken as given: its adjoints are the root gradients
                A[base] = a;
                if (!DOF) X4[base] = a;
            } else {
                const Q Gp = q_of(Gi[base + p]), Gj = q_of(Gi[base + j]), gb = q_of(a);
                const V zl{e.lx, e.ly, e.lz};
                if (DOF) {
                    const f4v t = ntab[j];
                    const AngleRot r = angle_rot<CLIP>(X[fr * nd + j - 1], __float_as_int(t.x), t.y, t.z);
                    const JointAdj o = joint_adjoint(Gp, Gj, angle_quat(r), zl, gb, pb);
                    A[base + j] = v_of(o.gp);
                    X[fr * nd + j - 1] = angle_grad(r, o.lqb);
                } else {
                    const JointAdj o = joint_adjoint(Gp, Gj, q_of(X4[base + j]), zl, gb, pb);
                    A[base + j] = v_of(o.gp);
                    X4[base + j] = v_of(o.lqb);
                }
            }
        }
        wave_sync();   // this step's rows before the next step's parents pull them (other lanes)
    }

    if (lq_grad) {
        if (DOF) {
            ScalarRows<F>::copy_out(X, lq_grad + f0 * nd, nang);
        } else {
            GroupRows<F>::copy_out(X4, lq_grad + f0 * J * 4, nrec);
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
    if (T.gsched) {
        const int F = T.gF;
        const bool dof = D != nullptr, rot = grad_g_rot != nullptr;
        const size_t lds = sizeof(float) * BwdImages(nullptr, T.J, F, T.gsteps, dof, rot).floats;
        group_dispatch(F, [&](auto f, auto d, auto c, auto r) {
            hipLaunchKernelGGL((k_fk_bwd_group<d(), d() && c(), r(), f()>), dim3(grid_for(B, F)), dim3(64), lds, s, T, dv,
                               lq_in, g_rot, grad_g_rot, grad_g_pos, B, lq_grad, grad_root_rot, grad_root_t);
        }, dof, clip, rot);
    } else {   // J > kGroupMaxJ: lane walk
        const int fw = bwd_walk_frames(T.J);
        if (fw < 1) return hipErrorInvalidValue;
        const size_t lds = (size_t)28 * T.J * fw;
        const dim3 g(grid_for(B, fw)), b(64);
        dispatch_bools([&](auto d, auto c) {
            hipLaunchKernelGGL((k_fk_bwd_walk<d(), d() && c()>), g, b, lds, s, T, dv, lq_in, g_rot, grad_g_rot, grad_g_pos,
                               B, fw, lq_grad, grad_root_rot, grad_root_t);
        }, D != nullptr, clip);
    }
    return hipGetLastError();
}

}  // namespace rtg

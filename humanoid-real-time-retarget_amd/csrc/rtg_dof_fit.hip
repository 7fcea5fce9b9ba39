// rtg_dof_fit.hip -- fit joint angles to target keypoints in one launch: the joint-angle forward model
// (hu_forward_model.py:17-33), the weighted keypoint loss L_f = sum_j w_j |P_j(a_f) - T_fj|^2, its gradient and
// `iters` steps of Adam (torch.optim.Adam without weight decay or amsgrad), all on the lane-group tile of
// rtg_fk.hip / rtg_fk_grad.hip.  Frames are independent and a frame's whole state -- angles, both moments, the FK rows
// and the targets -- fits next to its tile in LDS, so the targets are read once, the angles written once, and nothing
// in between touches global memory.
//
// A tile is one wave: F = group_frames(J) frames, 64 / F lanes per frame.  One iteration runs the topology's host
// schedule forwards (sub-lane u of a frame's group composes the joint the schedule names at each step) and then
// backwards (k_fk_bwd_group's sweep with ROT = false: a joint's contribution to its parent's rotation adjoint goes
// into its own G row, a parent pulls its children's rows in ascending index order -- one order per sum, no atomics).
// The lane that finishes joint j's reverse step holds d L / d a_j and owns that angle: it takes the Adam step for it
// on the spot, so there is no gradient image and no separate update pass.  The root is given, not fitted: its rows
// are written once and the reverse sweep stops above it.
//
// LDS images of a tile: FitImages below (every image starts 16-byte aligned).
// 33-link Hu, F = 16 (10 steps): 29.3 KiB; a 64-joint chain, F = 8, 64 steps: 43.9 KiB (the largest: gsteps <= J).
//
// Arithmetic: as in rtg_fk_grad.hip no operation order is owed to a reference (explicit fmaf, the device sincosf,
// -ffp-contract=fast); the forward here is the float32 restatement of rtg_dof_fk_f32's, not its bit-exact f64 sincos.
// Every value of a frame is computed by that frame's lanes from that frame's rows in an order fixed by the schedule
// alone, so a frame's results do not depend on its tile, the batch or another frame's NaNs.  The loss is a fixed-order
// sum: sub-lane u adds its joints u, u + L, ... in index order, then the group's L partials are added in lane order.
// A DOF whose subtree carries no weight gets the exact +-0 the reverse sweep computes for it, and from a zero state
// the update subtracts +0: the angle's bits stay.
#include "rtg_device.cuh"
#include "rtg_fk_adjoint.cuh"
#include "rtg_fk_group.cuh"

namespace rtg {

constexpr size_t kFitMaxLdsBytes = 64 * 1024;   // the dynamic-LDS attribute the launcher sets (J = 64, 64 steps: 43.9 KiB)

// beta^t in float64 by squaring: a function of (beta, t) alone, so a launch that starts at step0 = k takes the very
// step the k-th iteration of a longer launch takes
RTG_DEV double pow_int(double b, int t)
{
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

struct FitImages {
    f4v *G;          // [F J] forward: global rotations; reverse: a finished joint's contribution to its parent
    float *P;        // [F J 3] positions, then in place the residual adjoints 2 w_j (P_j - T_j), then the complete ones
    float *T;        // [F J 3] the targets, loaded once as coalesced pieces
    float *A, *M, *V;   // [F (J-1)] the angles and the two Adam moments; in the evaluation sweep after the last step
                        // (the moments are out by then) M receives the gradient rows
    f4v *tab;        // [J] per joint {axis, lower, upper, weight}
    GEnt *sch;       // [gsteps L] the schedule
    int *nsib;       // [J] the next-sibling table
    float *lossp;    // [64] loss partials
    float *adam;     // [128] {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)} of 64 steps
    size_t floats;
    __host__ __device__ FitImages(float *base, int J, int F, int steps)
    {
        LdsCarve c(base);
        G = c.take<f4v>((size_t)F * J);
        P = c.take<float>((size_t)3 * F * J);
        T = c.take<float>((size_t)3 * F * J);
        A = c.take<float>((size_t)F * (J - 1));
        M = c.take<float>((size_t)F * (J - 1));
        V = c.take<float>((size_t)F * (J - 1));
        tab = c.take<f4v>(J);
        sch = c.take<GEnt>((size_t)steps * (64 / F));
        nsib = c.take<int>(J);
        lossp = c.take<float>(64);
        adam = c.take<float>(128);
        floats = c.floats;
    }
};

// the forward sweep: G and P of every joint below the root from the angles (the root's rows stay as loaded)
template <bool CLIP, int F>
RTG_DEV void fit_forward(const FitImages &I, int J, int gsteps, bool live, int fr, int sub)
{
    using G = Grp<F>;
    const int base = fr * J, nd = J - 1;
    GEnt en = I.sch[sub];
    for (int s = 0; s < gsteps; ++s) {
        const GEnt e = en;
        if (s + 1 < gsteps) en = I.sch[(s + 1) * G::L + sub];   // the next step's entry: its latency under this step
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF && j != 0) {
            const f4v t = I.tab[j];
            const AngleRot r = angle_rot<CLIP>(I.A[fr * nd + j - 1], __float_as_int(t.x), t.y, t.z);
            const Q Gp = q_of(I.G[base + p]);
            const Q u = qmul(Gp, angle_quat(r));
            const float n = __builtin_sqrtf(fdot4(u, u));
            const float rn = (u.w < 0.0f ? -1.0f : 1.0f) / (n < 1e-9f ? 1e-9f : n);   // quat_unit(quat_pos(u)); NaN passes
            I.G[base + j] = f4v{u.x * rn, u.y * rn, u.z * rn, u.w * rn};
            const V rv = qrotate(Gp, V{e.lx, e.ly, e.lz});
            const float *pp = I.P + 3 * (base + p);
            float *pj = I.P + 3 * (base + j);
            pj[0] = rv.x + pp[0]; pj[1] = rv.y + pp[1]; pj[2] = rv.z + pp[2];
        }
        wave_sync();   // this step's rows before the next step's parent reads (other lanes)
    }
}

// positions -> residual adjoints in place (the root's row stays: it is not fitted); returns this lane's part of the
// frame's loss, its joints in index order
template <int F>
RTG_DEV float fit_residual(const FitImages &I, int J, bool live, int fr, int sub)
{
    using G = Grp<F>;
    float acc = 0.0f;
    if (live) {
        for (int j = sub; j < J; j += G::L) {
            const float w = I.tab[j].w;
            float *pj = I.P + 3 * (fr * J + j);
            const float *tj = I.T + 3 * (fr * J + j);
            const V d{pj[0] - tj[0], pj[1] - tj[1], pj[2] - tj[2]};
            acc = __builtin_fmaf(w, fdot3(d, d), acc);
            if (j != 0) {
                const float w2 = 2.0f * w;
                pj[0] = w2 * d.x; pj[1] = w2 * d.y; pj[2] = w2 * d.z;
            }
        }
    }
    wave_sync();
    return acc;
}

struct AdamStep {
    float b1, omb1, b2, omb2, eps;
    float step, rbc2s;   // lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)
};

// the reverse sweep; EVAL: the gradient rows into the M image, else the Adam step of each angle where its gradient
// appears
template <bool CLIP, bool EVAL, int F>
RTG_DEV void fit_reverse(const FitImages &I, int J, int gsteps, bool live, int fr, int sub, const AdamStep &S)
{
    using G = Grp<F>;
    const int base = fr * J, nd = J - 1;
    GEnt en = I.sch[(gsteps - 1) * G::L + sub];
    for (int s = gsteps - 1; s >= 0; --s) {
        const GEnt e = en;
        if (s > 0) en = I.sch[(s - 1) * G::L + sub];   // the next step's entry: its latency under this step
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF && j != 0) {
            V pb;
            const f4v a = child_pull(f4v{0.0f, 0.0f, 0.0f, 0.0f}, I.G, I.P, base, j, (e.code >> 16) & 0xFF, I.nsib,
                                     pb);
            const Q Gp = q_of(I.G[base + p]), Gj = q_of(I.G[base + j]);
            const f4v t = I.tab[j];
            const int i = fr * nd + j - 1;
            const float ang = I.A[i];
            const AngleRot r = angle_rot<CLIP>(ang, __float_as_int(t.x), t.y, t.z);
            const JointAdj o = joint_adjoint(Gp, Gj, angle_quat(r), V{e.lx, e.ly, e.lz}, q_of(a), pb);
            I.G[base + j] = v_of(o.gp);
            const float g = angle_grad(r, o.lqb);
            if (EVAL) {
                I.M[i] = g;
            } else {   // torch.optim.Adam's step on the unprojected iterate
                const float m = __builtin_fmaf(S.omb1, g, S.b1 * I.M[i]);
                const float v = __builtin_fmaf(S.omb2 * g, g, S.b2 * I.V[i]);
                I.M[i] = m;
                I.V[i] = v;
                I.A[i] = __builtin_fmaf(-S.step, m / __builtin_fmaf(__builtin_sqrtf(v), S.rbc2s, S.eps), ang);
            }
        }
        wave_sync();   // this step's rows before the next step's parents pull them (other lanes)
    }
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_group(TopoView T, DofView D, DofFitArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float ft_lds[];
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x, nd = J - 1;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(A.B, f0);
    const int npos = 3 * nfr * J, nang = nfr * nd;
    const FitImages I(ft_lds, J, F, T.gsteps);
    float *lossp = I.lossp, *adam = I.adam;

    // every global load of the tile first (a lane past the rows re-reads element 0), then the LDS images
    const bool state = A.m != nullptr;
    ScalarRows<F> ang, m0 = {}, v0 = {};
    ang.load(A.dof_in + f0 * nd, nang);   // J = 1: no angles, the host passes a readable dummy
    if (state) {
        m0.load(A.m + f0 * nd, nang);
        v0.load(A.v + f0 * nd, nang);
    }
    const float *trow = A.target_pos + f0 * J * 3;
    PosRows<F> tp;
    tp.load(trow, npos);
    const f4v rr = root_rot_load(A.root_rot, f0, nfr);
    const float rt = root_t_load(A.root_t, f0, nfr);
    group_sched_fill(T, G::L, I.sch, I.nsib);
    joint_tab_fill<CLIP, true>(D, J, I.tab, A.weight);
    ang.store(I.A, nang);
    m0.store(I.M, nang);
    v0.store(I.V, nang);
    tp.to_lds(I.T, trow, npos);
    root_preset(I.G, I.P, J, nfr, rr, rt);   // the root rotation, unnormalised (hu_forward_model.py:24)
    wave_sync();

    const int fr = lane >> G::LOG_L, sub = lane & (G::L - 1);
    const bool live = fr < nfr;
    AdamStep S;
    S.b1 = A.beta1;
    S.omb1 = 1.0f - A.beta1;
    S.b2 = A.beta2;
    S.omb2 = 1.0f - A.beta2;
    S.eps = A.eps;
    S.step = 0.0f;
    S.rbc2s = 0.0f;
    for (int k = 1; k <= A.iters; ++k) {   // wave-uniform; no global memory traffic inside
        if (((k - 1) & 63) == 0) {   // the bias corrections of the next 64 steps, one step per lane (float64)
            const int t = A.step0 + k + lane;
            adam[2 * lane] = (float)((double)A.lr / (1.0 - pow_int((double)A.beta1, t)));
            adam[2 * lane + 1] = (float)(1.0 / __builtin_sqrt(1.0 - pow_int((double)A.beta2, t)));
            wave_sync();
        }
        S.step = adam[2 * ((k - 1) & 63)];
        S.rbc2s = adam[2 * ((k - 1) & 63) + 1];
        fit_forward<CLIP, F>(I, J, T.gsteps, live, fr, sub);
        (void)fit_residual<F>(I, J, live, fr, sub);
        fit_reverse<CLIP, false, F>(I, J, T.gsteps, live, fr, sub, S);
    }

    // the iterate and its state out (coalesced), then loss and gradient there by one more sweep
    if (A.dof_out) ScalarRows<F>::copy_out(I.A, A.dof_out + f0 * nd, nang);
    if (state) {
        ScalarRows<F>::copy_out(I.M, A.m + f0 * nd, nang);
        ScalarRows<F>::copy_out(I.V, A.v + f0 * nd, nang);
    }
    if (!A.loss && !A.grad) return;
    wave_sync();   // the M image is read out before the evaluation sweep writes gradients into it
    fit_forward<CLIP, F>(I, J, T.gsteps, live, fr, sub);
    const float part = fit_residual<F>(I, J, live, fr, sub);
    if (A.loss) {
        lossp[lane] = part;
        wave_sync();
        if (lane < nfr) {
            float l = lossp[lane * G::L];
#pragma unroll
            for (int u = 1; u < G::L; ++u) l += lossp[lane * G::L + u];
            A.loss[f0 + lane] = l;
        }
    }
    if (A.grad) {
        fit_reverse<CLIP, true, F>(I, J, T.gsteps, live, fr, sub, S);
        ScalarRows<F>::copy_out(I.M, A.grad + f0 * nd, nang);
    }
}

hipError_t launch_dof_fit(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A, hipStream_t s)
{
    if (!T.gsched) return hipErrorInvalidValue;   // J > kGroupMaxJ: the caller reports it as unsupported
    const int F = T.gF;
    const size_t lds = sizeof(float) * FitImages(nullptr, T.J, F, T.gsteps).floats;
    if (lds > kFitMaxLdsBytes) return hipErrorInvalidValue;
    hipError_t attr = hipSuccess;
    group_dispatch(F, [&](auto f, auto cl) {
        attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_group<cl(), f()>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
        if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A);
    }, clip);
    if (attr != hipSuccess) return attr;
    return hipGetLastError();
}

}  // namespace rtg

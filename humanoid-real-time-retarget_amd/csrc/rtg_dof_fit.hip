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
// on the spot, so there is no gradient image and no separate update pass.  In k_dof_fit_group the root is given, not
// fitted: its rows are written once and the reverse sweep stops above it.
//
// k_dof_fit_root_group (rtg_dof_fit_root_f32) is the same tile with the floating base among the parameters (ROOT):
// the root translation t and rotation q of a frame and their moments live in a root image of 21 floats per frame.  The
// lane the schedule gives the root presets G_0 = q / max(|q|, 1e-9) (no sign flip; a given rotation stays as it is)
// and P_0 = t at the top of each forward sweep, the residual adjoint of row 0 is kept, and the reverse sweep ends at
// the root: that lane pulls its children (k_fk_bwd_group's j == 0), holds dL/dt and dL/dG_0, applies the
// normalisation's adjoint (g - (g.G_0) G_0) / |q| and takes the 3 + 4 Adam steps, renormalising q after its step.
// The fit_root mask is a launch argument (wave-uniform branches in that one lane's work).
//
// k_dof_fit_orient_group (rtg_dof_fit_orient_f32) is the root tile with orientation targets for up to
// RTG_FIT_MAX_ROT_LINKS chosen links (ORI): L_f gains sum_k rot_weight[k] 4 (1 - c_k^2), c_k = <G_j, Rh_fk> for
// j = rot_joint[k], G_j the global rotation the forward sweep holds and Rh_fk the target row over max(|row|, 1e-9) (no
// sign flip; normalised once, on its way into LDS).  4 (1 - c^2) = (2 sin(theta / 2))^2 of the angle theta between
// the two rotations: even in either quaternion, theta^2 to second order, and stationary at theta = pi as well as at 0
// (a link exactly half a turn off gets no pull from this term).  Its adjoint dL/dG_j = -8 rot_weight[k] c_k Rh_fk is
// the joint's own upstream rotation adjoint: child_pull's first argument at that joint's reverse step (the root's in
// fit_root_reverse), formed from G_j before the row takes the joint's contribution to its parent.  Everything behind
// it -- the normalisation's tangent projection, angle_grad, the Adam steps -- is the position fit's.  rot_joint comes
// in the launch arguments (checked on the host), so a joint's {slot, rot_weight} entry is filled from them.  The loss
// adds the links after the positions, in k order, by the lane that writes the frame's loss.
//
// k_dof_fit_prior_group / k_dof_fit_orient_prior_group (rtg_dof_fit_prior_f32, K == 0 / K > 0) are the root tile and
// the oriented tile with a posture prior on the angles and a projection onto the limits (PRIOR): L_f gains
// sum_d prior_weight[d] (a_d - prior_d)^2 on the iterate a -- not on the clamped angle the forward model uses, so the
// term pulls a run-away iterate back -- and its gradient 2 prior_weight[d] (a_d - prior_d) joins dL/da_d in the lane
// that holds it, before the Adam step; with RTG_FIT_PROJECT that lane clamps the angle to the limits the step already
// holds after its step (torch.clamp: NaN passes; the moments stay).  Whether a prior is given and whether to project
// are launch arguments (wave-uniform).  The prior rows are loaded with the angles, before the tile writes anything, so
// they may alias dof_in or dof_out.  The loss adds the term per sub-lane (its DOFs u, u + L, ... in index order) to that
// lane's position part.
//
// k_dof_fit_apart_group / k_dof_fit_orient_apart_group (rtg_dof_fit_apart_f32, K == 0 / K > 0) are the prior tiles with
// keep-apart spheres and a floor (APART): S <= RTG_FIT_MAX_SPHERES spheres ride on links, c_s = P_j + rot(G_j, o_s),
// and L_f gains sum_p pair_weight[p] max(0, r_a + r_b + margin - |c_a - c_b|)^2 over Pn <= RTG_FIT_MAX_PAIRS pairs and
// floor_weight max(0, r_s + h0 - n . c_s)^2 over the spheres of a mask.  The term is a pass between the forward sweep
// and the residuals (apart_pass): sub-lane u of a frame owns the spheres u, u + L, ...; it writes their centres, and
// once the frame's centres are in LDS walks the pair list -- a wave-uniform loop, the lane's part under a predicate --
// and the floor to form g_s = dL/dc_s of its spheres (pairs in pair order, then the floor; no atomics), which then
// takes c_s's place in the image.  fit_residual adds the g_s of a link's spheres to the link's residual row in sphere
// order (row 0 for the root's), and a joint's spheres with a non-zero offset add sum_s d(g_s . rot(G_j, o_s)) / dG_j --
// joint_adjoint's closed form -- to the joint's own upstream rotation adjoint, where orient_adjoint's enters, from G_j
// before the row is overwritten; a zero offset adds nothing there, not a zero.  The loss: pair p is counted by the
// owner of a_p, a floor term by the sphere's owner, and the lane's part joins its position part like the prior's.
// Spheres, pairs and plane travel in the launch arguments (host-checked) and are read with constant indices only, on
// their way into small LDS tables; the per-joint table holds the bit mask of a joint's spheres.
//
// k_dof_fit_robust_group and its three siblings (rtg_dof_fit_robust_f32) are the four PRIOR-family tiles with
// per-frame keypoint weights and a robust keypoint loss (ROBUST): the keypoint term is sum_j e_fj rho(s) over the
// keypoints with frame_weight[f,j] != 0, e_fj = weight[j] frame_weight[f,j], s = |P_j - T_fj|^2, rho(s) = s or, with
// robust_scale = delta > 0, the pseudo-Huber 2 s / (sqrt(1 + s / delta^2) + 1); its adjoint 2 e_fj d / sqrt(1 + s /
// delta^2) enters where 2 w_j d enters, fit_residual's in-place row.  The tile loads frame_weight's rows with its
// other global loads and keeps e_fj in one more image of [F J] floats (RobustImages), a skipped keypoint as a bit
// pattern no product has; fit_residual reads its weight there and *selects*: a skipped keypoint adds nothing to the
// loss and leaves a +0 row whatever its target row holds.  Robust on or off is wave-uniform; 1 / delta^2 comes
// rounded from the host's double.  Nothing else of the tile changes.
//
// LDS images of a tile: FitImages below (every image starts 16-byte aligned).
// 33-link Hu, F = 16 (10 steps): 29.3 KiB; a 64-joint chain, F = 8, 64 steps: 43.9 KiB (the largest: gsteps <= J).
// With the root image and the two more step sizes per Adam step: 31.1 KiB (still 5 tiles per CU) and 45.1 KiB.
// ORI adds 8 J + 16 F K bytes, sized by the launch's own K: Hu keeps 5 tiles per CU up to K = 2 and has 4 from there
// (K = 8: 34,160 B of the 40,960 a tile may have there); the 64-joint chain with K = 8: 47,680 B.
// PRIOR adds 4 F (J - 1) + 4 (J - 1) bytes: Hu 34,016 B (K = 8: 36,336 B), the chain 48,416 B (K = 8: 49,952 B).
// Measured: a Hu tile keeps its fifth place on a CU up to 32,000 B of dynamic LDS, not 32,768, so the
// PRIOR tiles -- and every ORI tile -- run four to a CU, and that is where their time over k_dof_fit_root_group sits.
// APART adds ApartImages behind them, sized by the launch's own S and Pn: 12 F S (centres) + 16 S + 4 S + 4 J + 8 Pn
// bytes, each image padded to 16.  Hu with S = 16, Pn = 32: 3,072 + 256 + 64 + 144 + 256 = 3,792 B, a tile of
// 37,808 B (K = 8: 40,128 B) -- under the 40,960 B that keep four tiles on a CU; the chain: 2,368 B, 50,784 B
// (K = 8: 52,320 B).
// ROBUST adds RobustImages behind those: 4 F J bytes (Hu 2,112 B, the chain 2,048 B: its largest tile 54,368 B).
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

constexpr size_t kFitMaxLdsBytes = 64 * 1024;   // the dynamic-LDS attribute the launcher sets (J = 64, 64 steps: 45.1 KiB)

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

struct OriEnt {
    int slot;
    float w;
};

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
    float *adam;     // [128] {lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)} of 64 steps; root: [256], with
                     // {lr_root_t, lr_root_rot} / (1 - beta1^t) behind them
    f4v *Rq;         // root: [F] the root rotations, the iterate where fitted (as given until the first step)
    float *Rt;       // root: [F 3] the root translations, likewise
    float *Rs;       // root: [F 14] root_state's rows {m_t, m_q, v_t, v_q}; in the evaluation sweep after the last step
                     // (the moments are out by then) [F 7]: grad_root's rows {dL/dt, dL/dq}
    f4v *Rh;         // ORI: [F K] the unit target rotations of the oriented links
    OriEnt *otab;    // ORI: [J] per joint {slot in 0..K-1 or -1: not oriented, rot_weight}
    float *Pr;       // PRIOR: [F (J-1)] the prior rows (zeros where no prior is given)
    float *Pw;       // PRIOR: [J-1] prior_weight
    size_t floats;
    // K < 0: no orientation images; the prior images come last, so every other offset is what it is without them
    __host__ __device__ FitImages(float *base, int J, int F, int steps, bool root, int K = -1, bool prior = false)
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
        adam = c.take<float>(root ? 256 : 128);
        Rq = c.take<f4v>(root ? F : 0);
        Rt = c.take<float>(root ? 3 * F : 0);
        Rs = c.take<float>(root ? 14 * F : 0);
        Rh = c.take<f4v>(K > 0 ? (size_t)F * K : 0);
        otab = c.take<OriEnt>(K >= 0 ? J : 0);
        Pr = c.take<float>(prior ? (size_t)F * (J - 1) : 0);
        Pw = c.take<float>(prior ? J - 1 : 0);
        floats = c.floats;
    }
};

// APART: the keep-apart images, carved behind the tile's FitImages (base: the first float after them), so every offset
// there is what it is without them.  A carve of their own: the tiles without the term do not see it at all, and their
// code is the parent's instruction for instruction
struct ApartImages {
    float *C;        // [F S 3] the sphere centres, then in place their gradients g_s
    f4v *sph;        // [S] per sphere {offset in its link's frame, radius}
    int *slink;      // [S] a sphere's joint
    int *jtab;       // [J] per joint the bit mask of its spheres, and << 16 of those with a non-zero offset
    int *pair;       // [Pn, padded to whole fours with 0] a | b << 8
    float *pairw;    // [Pn, padded likewise with 0] pair_weight
    size_t floats;
    __host__ __device__ ApartImages(float *base, int J, int F, int S, int Pn)
    {
        LdsCarve c(base);
        C = c.take<float>((size_t)3 * F * S);
        sph = c.take<f4v>(S);
        slink = c.take<int>(S);
        jtab = c.take<int>(J);
        pair = c.take<int>(Pn);
        pairw = c.take<float>(Pn);
        floats = c.floats;
    }
};

// ROBUST: the effective keypoint weights, carved behind the tile's other images (base: the first float after them), so
// the tiles without the term do not see it and their code stays what it was
struct RobustImages {
    float *W;        // [F J] e_fj = weight[j] frame_weight[f,j]; kSkipKeypoint's bits where frame_weight[f,j] == 0
    size_t floats;
    __host__ __device__ RobustImages(float *base, int J, int F)
    {
        LdsCarve c(base);
        W = c.take<float>((size_t)F * J);
        floats = c.floats;
    }
};
// a signalling NaN: a float32 product is never that (the multiplier quiets every NaN it passes on), so the image needs
// no second word for "skip this keypoint"
constexpr int kSkipKeypoint = 0x7F800001;

// G_0 = q / max(|q|, 1e-9) of a fitted root rotation: no sign flip (q and -q are one rotation and the iterate stays
// continuous); NaN passes
RTG_DEV f4v root_unit(f4v q)
{
    const float n = __builtin_sqrtf(fdot4(q_of(q), q_of(q)));
    const float rn = 1.0f / (n < 1e-9f ? 1e-9f : n);
    return f4v{q.x * rn, q.y * rn, q.z * rn, q.w * rn};
}

// the forward sweep: G and P of every joint below the root from the angles (the root's rows stay as loaded; ROOT: the
// lane with the root's entry presets them from the root image, the rotation normalised where it is fitted)
template <bool CLIP, int F, bool ROOT>
RTG_DEV void fit_forward(const FitImages &I, int J, int gsteps, bool live, int fr, int sub, int fit_root)
{
    using G = Grp<F>;
    const int base = fr * J, nd = J - 1;
    GEnt en = I.sch[sub];
    for (int s = 0; s < gsteps; ++s) {
        const GEnt e = en;
        if (s + 1 < gsteps) en = I.sch[(s + 1) * G::L + sub];   // the next step's entry: its latency under this step
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (ROOT && live && j == 0) {
            const f4v q = I.Rq[fr];
            I.G[base] = (fit_root & RTG_FIT_ROOT_ROT) ? root_unit(q) : q;
            float *p0 = I.P + 3 * base;
            const float *t0 = I.Rt + 3 * fr;
            p0[0] = t0[0]; p0[1] = t0[1]; p0[2] = t0[2];
        }
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

// positions -> residual adjoints in place (the root's row stays where the root's adjoint is not taken; ROOT: it is
// dL/dt's own term); returns this lane's part of the frame's loss, its joints in index order
// APART (S spheres): the row then takes the centre gradients g_s of the link's spheres, in sphere order
// ROBUST: the weight is e_fj from the W image, a keypoint marked there is skipped by selects (nothing to the loss, a +0
// row before the spheres' part, whatever d holds), and with `robust` (wave-uniform) the term is e rho(s) with the
// adjoint 2 e d / sqrt(1 + s inv_d2)
template <int F, bool ROOT, bool APART = false, bool ROBUST = false>
RTG_DEV float fit_residual(const FitImages &I, int J, bool live, int fr, int sub, const ApartImages *X = nullptr, int S = 0,
                           const float *W = nullptr, bool robust = false, float inv_d2 = 0.0f)
{
    using G = Grp<F>;
    float acc = 0.0f;
    if (live) {
        for (int j = sub; j < J; j += G::L) {
            const float w = ROBUST ? W[fr * J + j] : I.tab[j].w;
            float *pj = I.P + 3 * (fr * J + j);
            const float *tj = I.T + 3 * (fr * J + j);
            const V d{pj[0] - tj[0], pj[1] - tj[1], pj[2] - tj[2]};
            float w2 = 2.0f * w;
            if constexpr (ROBUST) {
                const bool on = __float_as_int(w) != kSkipKeypoint;
                const float s = fdot3(d, d);
                float rho = s;
                if (robust) {
                    const float q = __builtin_sqrtf(__builtin_fmaf(s, inv_d2, 1.0f));
                    rho = (2.0f * s) / (q + 1.0f);
                    w2 = w2 / q;
                }
                acc = on ? __builtin_fmaf(w, rho, acc) : acc;
                if (ROOT || j != 0) {
                    V r{on ? w2 * d.x : 0.0f, on ? w2 * d.y : 0.0f, on ? w2 * d.z : 0.0f};
                    if constexpr (APART) {
                        for (int m = X->jtab[j] & 0xFFFF; m; m &= m - 1) {
                            const float *g = X->C + 3 * (fr * S + __builtin_ctz(m));
                            r.x += g[0]; r.y += g[1]; r.z += g[2];
                        }
                    }
                    pj[0] = r.x; pj[1] = r.y; pj[2] = r.z;
                }
                continue;
            }
            acc = __builtin_fmaf(w, fdot3(d, d), acc);
            if (ROOT || j != 0) {
                if constexpr (APART) {
                    V r{w2 * d.x, w2 * d.y, w2 * d.z};
                    for (int m = X->jtab[j] & 0xFFFF; m; m &= m - 1) {
                        const float *g = X->C + 3 * (fr * S + __builtin_ctz(m));
                        r.x += g[0]; r.y += g[1]; r.z += g[2];
                    }
                    pj[0] = r.x; pj[1] = r.y; pj[2] = r.z;
                } else {
                    pj[0] = w2 * d.x; pj[1] = w2 * d.y; pj[2] = w2 * d.z;
                }
            }
        }
    }
    wave_sync();
    return acc;
}

// APART: the keep-apart pass between the forward sweep and the residuals.  Sub-lane u of a frame owns the spheres
// u, u + L, ...: it writes their centres c_s = P_j + rot(G_j, o_s) from the forward's rows, then -- the centres of the
// whole frame in LDS -- walks the pair list (wave-uniform, the lane's part under a predicate) and the floor and forms
// g_s = dL/dc_s of each of its spheres: its pairs' terms in pair order, then the floor's.  g_s takes c_s's place in
// the image once every walk has read the centres.  Returns the lane's part of the term's loss: pair p by the owner of
// a_p, in pair order, then the lane's floor terms in sphere order.  h = max(0, .) as torch.clamp does it: NaN passes.
template <int F>
RTG_DEV float apart_pass(const FitImages &I, const ApartImages &X, const DofFitApartArgs &Z, int J, bool live, int fr,
                         int sub)
{
    using G = Grp<F>;
    constexpr int NS = RTG_FIT_MAX_SPHERES / G::L;
    const int S = Z.S, base = fr * J;
    float *C = X.C + 3 * fr * S;
    if (live) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = k * G::L + sub;
            if (s < S) {
                const f4v o = X.sph[s];
                const int j = X.slink[s];
                const V rv = qrotate(q_of(I.G[base + j]), V{o.x, o.y, o.z});
                const float *pj = I.P + 3 * (base + j);
                C[3 * s] = rv.x + pj[0]; C[3 * s + 1] = rv.y + pj[1]; C[3 * s + 2] = rv.z + pj[2];
            }
        }
    }
    wave_sync();
    V g[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) g[k] = V{0.0f, 0.0f, 0.0f};
    float acc = 0.0f;
    // every lane computes every pair and takes its part by selects: no branch in the body, so the steps of several
    // pairs overlap (one wave per SIMD: a chain of dependent steps per pair would cost its full latency 32 times)
    // (four pairs per trip, the table padded with pairs of weight 0 that join sphere 0 with itself: they add +-0)
    for (int p0 = 0; p0 < Z.Pn; p0 += 4) {
#pragma unroll
      for (int p = p0; p < p0 + 4; ++p) {
        const int ab = __builtin_amdgcn_readfirstlane(X.pair[p]);
        const int a = ab & 0xFF, b = ab >> 8;
        const bool ia = (a & (G::L - 1)) == sub, ib = (b & (G::L - 1)) == sub;
        const float w = X.pairw[p];
        const float *ca = C + 3 * a, *cb = C + 3 * b;
        const V d{ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
        const float dd = __builtin_sqrtf(fdot3(d, d));
        const float x = (X.sph[a].w + X.sph[b].w + Z.margin) - dd;
        const float h = x < 0.0f ? 0.0f : x;
        const float c = -2.0f * w * h / (dd < 1e-9f ? 1e-9f : dd);
        const V t{c * d.x, c * d.y, c * d.z};
#pragma unroll
        for (int k = 0; k < NS; ++k) {   // a != b: a lane owns at most one end of the pair in slot k
            const bool ka = ia && k == (a >> G::LOG_L), kb = ib && k == (b >> G::LOG_L);
            g[k].x += ka ? t.x : (kb ? -t.x : 0.0f);
            g[k].y += ka ? t.y : (kb ? -t.y : 0.0f);
            g[k].z += ka ? t.z : (kb ? -t.z : 0.0f);
        }
        acc = ia ? __builtin_fmaf(w, h * h, acc) : acc;
      }
    }
    if (Z.floor_mask != 0u && live) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = k * G::L + sub;
            if (s < S && ((Z.floor_mask >> s) & 1u)) {
                const V n{Z.plane[0], Z.plane[1], Z.plane[2]};
                const float x = (X.sph[s].w + Z.plane[3]) - fdot3(n, V{C[3 * s], C[3 * s + 1], C[3 * s + 2]});
                const float h = x < 0.0f ? 0.0f : x;
                const float c = -2.0f * Z.floor_weight * h;
                acc = __builtin_fmaf(Z.floor_weight, h * h, acc);
                g[k].x += c * n.x; g[k].y += c * n.y; g[k].z += c * n.z;
            }
        }
    }
    wave_sync();   // every walk has read the centres: the gradients take their place
    if (live) {
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int s = k * G::L + sub;
            if (s < S) { C[3 * s] = g[k].x; C[3 * s + 1] = g[k].y; C[3 * s + 2] = g[k].z; }
        }
    }
    wave_sync();
    return acc;
}

// APART: joint j's part of dL/dG_j from its spheres with a non-zero offset, sum_s d(g_s . rot(G_j, o_s)) / dG_j in
// sphere order -- joint_adjoint's closed form with Gp -> G_j, zl -> o_s, pb -> g_s -- from the forward's G_j (the
// caller forms it before the row is overwritten); a joint without such a sphere: +0, nothing read
RTG_DEV f4v apart_adjoint(const FitImages &I, const ApartImages &X, int S, int fr, int row, int j)
{
    f4v out{0.0f, 0.0f, 0.0f, 0.0f};
    int m = (int)((unsigned)X.jtab[j] >> 16);
    if (m == 0) return out;
    const f4v Gj = I.G[row];
    const V a{Gj.x, Gj.y, Gj.z};
    for (; m; m &= m - 1) {
        const int s = __builtin_ctz(m);
        const f4v o = X.sph[s];
        const float *gs = X.C + 3 * (fr * S + s);
        const V zl{o.x, o.y, o.z}, pb{gs[0], gs[1], gs[2]};
        const V c{zl.y * pb.z - zl.z * pb.y, zl.z * pb.x - zl.x * pb.z, zl.x * pb.y - zl.y * pb.x};
        const float gv = fdot3(pb, zl), av = fdot3(a, zl), ga = fdot3(pb, a);
        out.x += 2.0f * __builtin_fmaf(Gj.w, c.x, __builtin_fmaf(ga, zl.x, __builtin_fmaf(av, pb.x, -gv * a.x)));
        out.y += 2.0f * __builtin_fmaf(Gj.w, c.y, __builtin_fmaf(ga, zl.y, __builtin_fmaf(av, pb.y, -gv * a.y)));
        out.z += 2.0f * __builtin_fmaf(Gj.w, c.z, __builtin_fmaf(ga, zl.z, __builtin_fmaf(av, pb.z, -gv * a.z)));
        out.w += 2.0f * __builtin_fmaf(Gj.w, gv, fdot3(a, c));
    }
    return out;
}

// ORI: joint j's own upstream rotation adjoint, -8 w c Rh with c = <G_j, Rh>, from the forward's G_j (the caller
// forms it before the row is overwritten); +0 for a joint that is not oriented
template <bool ORI>
RTG_DEV f4v orient_adjoint(const FitImages &I, int K, int fr, int row, int j)
{
    if (!ORI) return f4v{0.0f, 0.0f, 0.0f, 0.0f};
    const OriEnt o = I.otab[j];
    if (o.slot < 0) return f4v{0.0f, 0.0f, 0.0f, 0.0f};
    const f4v R = I.Rh[fr * K + o.slot];
    const float s = -8.0f * o.w * fdot4(q_of(I.G[row]), q_of(R));
    return f4v{s * R.x, s * R.y, s * R.z, s * R.w};
}

// ORI: the links' part of frame fr's loss from the forward's G rows, added to l in k order
RTG_DEV float orient_loss(const FitImages &I, const DofFitOriArgs &O, int J, int fr, float l)
{
#pragma unroll
    for (int k = 0; k < RTG_FIT_MAX_ROT_LINKS; ++k) {
        if (k < O.K) {
            const int j = O.joint[k];
            const float c = fdot4(q_of(I.G[fr * J + j]), q_of(I.Rh[fr * O.K + k]));
            l = __builtin_fmaf(I.otab[j].w, 4.0f * __builtin_fmaf(-c, c, 1.0f), l);
        }
    }
    return l;
}

// PRIOR: this lane's part of the posture term sum_d prior_weight[d] (a_d - prior_d)^2 of frame fr: sub-lane u takes
// the DOFs u, u + L, ... in index order, and the caller adds it to the lane's position part, so the loss keeps one order
template <int F>
RTG_DEV float prior_loss_part(const FitImages &I, int nd, bool live, int fr, int sub)
{
    using G = Grp<F>;
    float acc = 0.0f;
    if (live) {
        for (int d = sub; d < nd; d += G::L) {
            const float e = I.A[fr * nd + d] - I.Pr[fr * nd + d];
            acc = __builtin_fmaf(I.Pw[d], e * e, acc);
        }
    }
    return acc;
}

struct AdamStep {
    float b1, omb1, b2, omb2, eps;
    float step, rbc2s;   // lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)
    float step_t, step_q;   // ROOT: lr_root_t / (1 - beta1^t), lr_root_rot / (1 - beta1^t)
};

// torch.optim.Adam's step on one parameter: the moments in place, returns the new value
RTG_DEV float adam_step(const AdamStep &S, float step, float g, float &m, float &v, float x)
{
    m = __builtin_fmaf(S.omb1, g, S.b1 * m);
    v = __builtin_fmaf(S.omb2 * g, g, S.b2 * v);
    return __builtin_fmaf(-step, m / __builtin_fmaf(__builtin_sqrtf(v), S.rbc2s, S.eps), x);
}

// The root's reverse step (one lane per frame): its children's rows pulled as k_fk_bwd_group's j == 0 does, giving
// dL/dt (the root's own residual included) and dL/dG_0; a fitted rotation's gradient goes through G_0 = q / |q|: it is
// tangent, (g - (g.G_0) G_0) / |q| (under the norm's clamp the divisor is a constant), a given one's is dL/dG_0 itself
// (the unnormalised model, as rtg_dof_fk_backward_f32 reports it).  ORI: an oriented root's own adjoint leads the pull
// (G_0 as the model uses it: the row the forward sweep preset, which nothing has overwritten).  EVAL: grad_root's row into the Rs image, else the
// Adam steps of the fitted blocks, q renormalised after its step.
template <bool EVAL, bool ORI, bool APART = false>
RTG_DEV void fit_root_reverse(const FitImages &I, int J, int K, int fr, int first_child, int fit_root, const AdamStep &S,
                              const ApartImages *X = nullptr, int NSPH = 0)
{
    const int base = fr * J;
    V pb;
    f4v own = orient_adjoint<ORI>(I, K, fr, base, 0);
    if constexpr (APART) own += apart_adjoint(I, *X, NSPH, fr, base, 0);   // the root's spheres: G_0 as the model uses it
    f4v g = child_pull(own, I.G, I.P, base, 0, first_child, I.nsib, pb);
    const f4v q = I.Rq[fr];
    if (fit_root & RTG_FIT_ROOT_ROT) {
        const float n = __builtin_sqrtf(fdot4(q_of(q), q_of(q)));
        if (!(n < 1e-9f)) {   // NaN takes the regular path and stays NaN
            const f4v G0 = I.G[base];
            const float r = 1.0f / n, d = fdot4(q_of(g), q_of(G0));
            g = f4v{r * __builtin_fmaf(-d, G0.x, g.x), r * __builtin_fmaf(-d, G0.y, g.y), r * __builtin_fmaf(-d, G0.z, g.z),
                    r * __builtin_fmaf(-d, G0.w, g.w)};
        } else {
            g = f4v{1e9f * g.x, 1e9f * g.y, 1e9f * g.z, 1e9f * g.w};
        }
    }
    if (EVAL) {
        float *o = I.Rs + 7 * fr;
        o[0] = pb.x; o[1] = pb.y; o[2] = pb.z;
        o[3] = g.x; o[4] = g.y; o[5] = g.z; o[6] = g.w;
        return;
    }
    float *st = I.Rs + 14 * fr;   // {m_t(3), m_q(4), v_t(3), v_q(4)}
    if (fit_root & RTG_FIT_ROOT_T) {
        float *t = I.Rt + 3 * fr;
        t[0] = adam_step(S, S.step_t, pb.x, st[0], st[7], t[0]);
        t[1] = adam_step(S, S.step_t, pb.y, st[1], st[8], t[1]);
        t[2] = adam_step(S, S.step_t, pb.z, st[2], st[9], t[2]);
    }
    if (fit_root & RTG_FIT_ROOT_ROT) {
        const f4v u{adam_step(S, S.step_q, g.x, st[3], st[10], q.x), adam_step(S, S.step_q, g.y, st[4], st[11], q.y),
                    adam_step(S, S.step_q, g.z, st[5], st[12], q.z), adam_step(S, S.step_q, g.w, st[6], st[13], q.w)};
        I.Rq[fr] = root_unit(u);
    }
}

// the reverse sweep; EVAL: the gradient rows into the M image, else the Adam step of each angle where its gradient
// appears; ROOT: the sweep ends with the root's step (fit_root_reverse); ORI: an oriented joint's own rotation adjoint
// leads its pull (orient_adjoint); PRIOR: with `prior` the posture term's 2 prior_weight[d] (a - prior) joins the
// angle's gradient where that appears (a: the iterate, not the clamped angle), and with `project` the angle is clamped
// to its limits after its Adam step (torch.clamp: NaN passes; the moments are not touched).  The two reads of the prior
// images are issued at the top of the joint's step, off the chain that ends in angle_grad.
// APART (NSPH spheres): a joint's spheres with a non-zero offset add apart_adjoint to its own rotation adjoint.
template <bool CLIP, bool EVAL, int F, bool ROOT, bool ORI, bool PRIOR = false, bool APART = false>
RTG_DEV void fit_reverse(const FitImages &I, int J, int K, int gsteps, bool live, int fr, int sub, const AdamStep &S,
                         int fit_root, bool prior = false, bool project = false, const ApartImages *X = nullptr, int NSPH = 0)
{
    using G = Grp<F>;
    const int base = fr * J, nd = J - 1;
    GEnt en = I.sch[(gsteps - 1) * G::L + sub];
    for (int s = gsteps - 1; s >= 0; --s) {
        const GEnt e = en;
        if (s > 0) en = I.sch[(s - 1) * G::L + sub];   // the next step's entry: its latency under this step
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF && j != 0) {
            float pv = 0.0f, pw = 0.0f;
            if constexpr (PRIOR) {
                pv = I.Pr[fr * nd + j - 1];
                pw = I.Pw[j - 1];
            }
            V pb;
            f4v own = orient_adjoint<ORI>(I, K, fr, base + j, j);
            if constexpr (APART) own += apart_adjoint(I, *X, NSPH, fr, base + j, j);
            const f4v a = child_pull(own, I.G, I.P, base, j, (e.code >> 16) & 0xFF, I.nsib, pb);
            const Q Gp = q_of(I.G[base + p]), Gj = q_of(I.G[base + j]);
            const f4v t = I.tab[j];
            const int i = fr * nd + j - 1;
            const float ang = I.A[i];
            const AngleRot r = angle_rot<CLIP>(ang, __float_as_int(t.x), t.y, t.z);
            const JointAdj o = joint_adjoint(Gp, Gj, angle_quat(r), V{e.lx, e.ly, e.lz}, q_of(a), pb);
            I.G[base + j] = v_of(o.gp);
            float g = angle_grad(r, o.lqb);
            if constexpr (PRIOR) {   // on a +-0 gradient this is fl(2 pw) fl(a - p): one rounding each
                if (prior) g = __builtin_fmaf(2.0f * pw, ang - pv, g);
            }
            if (EVAL) {
                I.M[i] = g;
            } else {   // torch.optim.Adam's step on the iterate; PRIOR with project: then the clamp to the limits
                const float m = __builtin_fmaf(S.omb1, g, S.b1 * I.M[i]);
                const float v = __builtin_fmaf(S.omb2 * g, g, S.b2 * I.V[i]);
                I.M[i] = m;
                I.V[i] = v;
                float x = __builtin_fmaf(-S.step, m / __builtin_fmaf(__builtin_sqrtf(v), S.rbc2s, S.eps), ang);
                if constexpr (PRIOR) {
                    if (project) x = x < t.y ? t.y : (x > t.z ? t.z : x);
                }
                I.A[i] = x;
            }
        }
        if (ROOT && live && j == 0) fit_root_reverse<EVAL, ORI, APART>(I, J, K, fr, (e.code >> 16) & 0xFF, fit_root, S, X, NSPH);
        wave_sync();   // this step's rows before the next step's parents pull them (other lanes)
    }
}

using RootStateRows = LaneRows<float, 4>;   // a tile's root_state rows: 14 F <= 256 floats
using OriRows = LaneRows<f4v, 2>;           // a tile's target rotations: F K <= 128 records

// one tile of the fit; ROOT: the root's rows come from the root image and its adjoints are taken (R: the root's
// arguments, not looked at otherwise); ORI: with orientation targets (O: theirs, likewise); PRIOR: with the posture
// prior and the projection onto the limits (H: theirs, likewise; what H asks for is wave-uniform, like fit_root);
// APART: with keep-apart spheres and a floor (Z: theirs, likewise; S >= 1 and a pair or the plane: the host sees to it)
// ROBUST: with per-frame keypoint weights and the robust keypoint loss (U: theirs, likewise; robust on or off is
// wave-uniform)
template <bool CLIP, int F, bool ROOT, bool ORI, bool PRIOR = false, bool APART = false, bool ROBUST = false>
RTG_DEV void dof_fit_tile(const TopoView &T, const DofView &D, const DofFitArgs &A, const DofFitRootArgs &R,
                          const DofFitOriArgs &O, const DofFitPriorArgs &H = DofFitPriorArgs{},
                          const DofFitApartArgs &Z = DofFitApartArgs{}, const DofFitRobustArgs &U = DofFitRobustArgs{})
{
    static_assert(PRIOR || !ROBUST, "the robust tile is the prior tile's");
    static_assert(ROOT || !ORI, "the oriented tile carries the root image");
    static_assert(ROOT || !PRIOR, "the prior tile carries the root image");
    static_assert(PRIOR || !APART, "the keep-apart tile is the prior tile's");
    extern __shared__ __attribute__((aligned(16))) float ft_lds[];
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x, nd = J - 1;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(A.B, f0);
    const int npos = 3 * nfr * J, nang = nfr * nd;
    const int K = ORI ? O.K : 0;
    const FitImages I(ft_lds, J, F, T.gsteps, ROOT, ORI ? K : -1, PRIOR);
    const int NSPH = APART ? Z.S : 0;
    [[maybe_unused]] const ApartImages X(APART ? ft_lds + I.floats : nullptr, J, F, NSPH, APART ? Z.Pn : 0);
    [[maybe_unused]] const RobustImages Y(ROBUST ? ft_lds + I.floats + (APART ? X.floats : 0) : nullptr, J, F);
    [[maybe_unused]] const bool robust = ROBUST && U.robust_scale > 0.0f;
    float *lossp = I.lossp, *adam = I.adam;
    const int fit_root = ROOT ? R.fit_root : 0;
    const bool prior = PRIOR && H.prior != nullptr, project = PRIOR && (H.flags & RTG_FIT_PROJECT) != 0;

    // every global load of the tile first (a lane past the rows re-reads element 0), then the LDS images
    const bool state = A.m != nullptr;
    const bool rstate = ROOT && fit_root != 0 && R.state != nullptr;   // nothing fitted: not read, not written
    ScalarRows<F> ang, m0 = {}, v0 = {};
    RootStateRows rs = {};
    ang.load(A.dof_in + f0 * nd, nang);   // J = 1: no angles, the host passes a readable dummy
    if (state) {
        m0.load(A.m + f0 * nd, nang);
        v0.load(A.v + f0 * nd, nang);
    }
    if (rstate) rs.load(R.state + f0 * 14, 14 * nfr);
    ScalarRows<F> pr = {};   // PRIOR: the tile's prior rows, read here -- before the tile writes a row -- so they may alias
                             // dof_in or dof_out
    if constexpr (PRIOR) {
        if (prior) pr.load(H.prior + f0 * nd, nang);
    }
    OriRows tr = {};
    if (ORI && K > 0) tr.load(O.target_rot + f0 * K * 4, nfr * K);
    ScalarRows<F> fw = {};   // ROBUST: the tile's frame_weight rows (no pointer: ones)
    if constexpr (ROBUST) {
        if (U.frame_weight) fw.load(U.frame_weight + f0 * J, nfr * J);
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
    if constexpr (PRIOR) {
        pr.store(I.Pr, nang);
        for (int d = lane; d < nd; d += 64) I.Pw[d] = prior && H.prior_weight ? ld_const(H.prior_weight + d) : (prior ? 1.0f : 0.0f);
        if (!CLIP && project)   // the table carries the limits only under the clip: this lane's own entries, again
            for (int j = lane; j < J; j += 64) {
                if (j == 0) continue;
                f4v t = I.tab[j];
                t.y = ld_const(D.lower + (j - 1));
                t.z = ld_const(D.upper + (j - 1));
                I.tab[j] = t;
            }
    }
    if (ORI) {   // the unit targets, and each joint's entry from the launch's link list
#pragma unroll
        for (int k = 0; k < 2; ++k) tr.v[k] = root_unit(tr.v[k]);
        tr.store(I.Rh, nfr * K);
        for (int j = lane; j < J; j += 64) {
            int slot = -1;
#pragma unroll
            for (int k = 0; k < RTG_FIT_MAX_ROT_LINKS; ++k)
                if (k < K && O.joint[k] == j) slot = k;
            I.otab[j] = OriEnt{slot, slot >= 0 && O.rot_weight ? ld_const(O.rot_weight + slot) : 1.0f};
        }
    }
    if constexpr (APART) {   // the spheres, the pairs and each joint's spheres from the launch's lists
        f4v sv{0.0f, 0.0f, 0.0f, 0.0f};
        int lk = 0;
#pragma unroll
        for (int s = 0; s < RTG_FIT_MAX_SPHERES; ++s)
            if (lane == s) {
                sv = f4v{Z.sphere[s][0], Z.sphere[s][1], Z.sphere[s][2], Z.sphere[s][3]};
                lk = Z.link[s];
            }
        if (lane < NSPH) {
            X.sph[lane] = sv;
            X.slink[lane] = lk;
        }
        int ab = 0;
        float pw = 0.0f;
#pragma unroll
        for (int p = 0; p < RTG_FIT_MAX_PAIRS; ++p)
            if (lane == p) {
                ab = Z.pair[p];
                pw = Z.pair_weight[p];
            }
        if (lane < ((Z.Pn + 3) & ~3)) {   // the carve pads the tables to whole fours: the pad holds pairs of weight 0
            X.pair[lane] = lane < Z.Pn ? ab : 0;
            X.pairw[lane] = lane < Z.Pn ? pw : 0.0f;
        }
        for (int j = lane; j < J; j += 64) {
            int m = 0;
#pragma unroll
            for (int s = 0; s < RTG_FIT_MAX_SPHERES; ++s)
                if (s < NSPH && Z.link[s] == j) {
                    m |= 1 << s;
                    if (Z.sphere[s][0] != 0.0f || Z.sphere[s][1] != 0.0f || Z.sphere[s][2] != 0.0f) m |= 0x10000 << s;
                }
            X.jtab[j] = m;
        }
    }
    if constexpr (ROBUST) {   // e_fj = weight[j] frame_weight[f,j] from the table's weights (other lanes wrote them)
        wave_sync();
        const float rJ = item_rcp(J);
        const bool given = U.frame_weight != nullptr;
        lane_items<Grp<F>::NR>([&](int k, int i) {
            if (i < nfr * J) {
                const float c = given ? fw.v[k] : 1.0f;
                const float e = I.tab[item_split(i, rJ, J).j].w * c;
                Y.W[i] = c == 0.0f ? __int_as_float(kSkipKeypoint) : e;
            }
        });
    }
    if (ROOT) {   // the root image; fit_forward presets the root's rows from it
        if (lane < nfr) I.Rq[lane] = rr;
        if (lane < 3 * nfr) I.Rt[lane] = rt;
        rs.store(I.Rs, 14 * nfr);
    } else {
        root_preset(I.G, I.P, J, nfr, rr, rt);   // the root rotation, unnormalised (hu_forward_model.py:24)
    }
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
    S.step_t = 0.0f;
    S.step_q = 0.0f;
    for (int k = 1; k <= A.iters; ++k) {   // wave-uniform; no global memory traffic inside
        if (((k - 1) & 63) == 0) {   // the bias corrections of the next 64 steps, one step per lane (float64)
            const int t = A.step0 + k + lane;
            if (ROOT) {
                const double bc1 = 1.0 - pow_int((double)A.beta1, t);
                adam[2 * lane] = (float)((double)A.lr / bc1);
                adam[128 + 2 * lane] = (float)((double)R.lr_t / bc1);
                adam[128 + 2 * lane + 1] = (float)((double)R.lr_rot / bc1);
            } else {
                adam[2 * lane] = (float)((double)A.lr / (1.0 - pow_int((double)A.beta1, t)));
            }
            adam[2 * lane + 1] = (float)(1.0 / __builtin_sqrt(1.0 - pow_int((double)A.beta2, t)));
            wave_sync();
        }
        S.step = adam[2 * ((k - 1) & 63)];
        S.rbc2s = adam[2 * ((k - 1) & 63) + 1];
        if (ROOT) {
            S.step_t = adam[128 + 2 * ((k - 1) & 63)];
            S.step_q = adam[128 + 2 * ((k - 1) & 63) + 1];
        }
        fit_forward<CLIP, F, ROOT>(I, J, T.gsteps, live, fr, sub, fit_root);
        if constexpr (APART) {
            (void)apart_pass<F>(I, X, Z, J, live, fr, sub);
            (void)fit_residual<F, ROOT, true, ROBUST>(I, J, live, fr, sub, &X, NSPH, Y.W, robust, U.inv_d2);
            fit_reverse<CLIP, false, F, ROOT, ORI, PRIOR, true>(I, J, K, T.gsteps, live, fr, sub, S, fit_root, prior, project,
                                                                &X, NSPH);
        } else {
            (void)fit_residual<F, ROOT, false, ROBUST>(I, J, live, fr, sub, nullptr, 0, Y.W, robust, U.inv_d2);
            fit_reverse<CLIP, false, F, ROOT, ORI, PRIOR>(I, J, K, T.gsteps, live, fr, sub, S, fit_root, prior, project);
        }
    }

    // the iterate and its state out (coalesced), then loss and gradient there by one more sweep
    if (A.dof_out) ScalarRows<F>::copy_out(I.A, A.dof_out + f0 * nd, nang);
    if (state) {
        ScalarRows<F>::copy_out(I.M, A.m + f0 * nd, nang);
        ScalarRows<F>::copy_out(I.V, A.v + f0 * nd, nang);
    }
    if (ROOT) {   // a given block, or iters == 0: the input's bits
        if (R.rot_out && lane < nfr) reinterpret_cast<f4v *>(R.rot_out)[f0 + lane] = I.Rq[lane];
        if (R.t_out && lane < 3 * nfr) R.t_out[f0 * 3 + lane] = I.Rt[lane];
        if (rstate) RootStateRows::copy_out(I.Rs, R.state + f0 * 14, 14 * nfr);
    }
    if (!A.loss && !A.grad && !(ROOT && R.grad)) return;
    wave_sync();   // the M image is read out before the evaluation sweep writes gradients into it
    fit_forward<CLIP, F, ROOT>(I, J, T.gsteps, live, fr, sub, fit_root);
    float apart = 0.0f;
    if constexpr (APART) apart = apart_pass<F>(I, X, Z, J, live, fr, sub);
    float part = fit_residual<F, ROOT, APART, ROBUST>(I, J, live, fr, sub, &X, NSPH, Y.W, robust, U.inv_d2);
    if constexpr (PRIOR) {
        if (prior) part += prior_loss_part<F>(I, nd, live, fr, sub);
    }
    if constexpr (APART) part += apart;
    if (A.loss) {
        lossp[lane] = part;
        wave_sync();
        if (lane < nfr) {
            float l = lossp[lane * G::L];
#pragma unroll
            for (int u = 1; u < G::L; ++u) l += lossp[lane * G::L + u];
            if (ORI) l = orient_loss(I, O, J, lane, l);   // G still holds the forward's rotations
            A.loss[f0 + lane] = l;
        }
    }
    if (A.grad || (ROOT && R.grad)) {
        fit_reverse<CLIP, true, F, ROOT, ORI, PRIOR, APART>(I, J, K, T.gsteps, live, fr, sub, S, fit_root, prior, project, &X, NSPH);
        if (A.grad) ScalarRows<F>::copy_out(I.M, A.grad + f0 * nd, nang);
        if (ROOT && R.grad) RootStateRows::copy_out(I.Rs, R.grad + f0 * 7, 7 * nfr);
    }
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_group(TopoView T, DofView D, DofFitArgs A)
{
    dof_fit_tile<CLIP, F, false, false>(T, D, A, DofFitRootArgs{}, DofFitOriArgs{});
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_root_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R)
{
    dof_fit_tile<CLIP, F, true, false>(T, D, A, R, DofFitOriArgs{});
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_orient_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                             DofFitOriArgs O)
{
    dof_fit_tile<CLIP, F, true, true>(T, D, A, R, O);
}

// rtg_dof_fit_prior_f32 without oriented links (the ORI instantiation measured 25 % slower at K = 0) and with them
template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_prior_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                            DofFitPriorArgs H)
{
    dof_fit_tile<CLIP, F, true, false, true>(T, D, A, R, DofFitOriArgs{}, H);
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_orient_prior_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                                   DofFitOriArgs O, DofFitPriorArgs H)
{
    dof_fit_tile<CLIP, F, true, true, true>(T, D, A, R, O, H);
}

// rtg_dof_fit_apart_f32 (with a sphere and a pair or the plane) without oriented links and with them
template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_apart_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                            DofFitPriorArgs H, DofFitApartArgs Z)
{
    dof_fit_tile<CLIP, F, true, false, true, true>(T, D, A, R, DofFitOriArgs{}, H, Z);
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_orient_apart_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                                   DofFitOriArgs O, DofFitPriorArgs H, DofFitApartArgs Z)
{
    dof_fit_tile<CLIP, F, true, true, true, true>(T, D, A, R, O, H, Z);
}

// rtg_dof_fit_robust_f32 (with frame weights or a robust scale): the four tiles above with ROBUST
template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_robust_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                             DofFitPriorArgs H, DofFitRobustArgs U)
{
    dof_fit_tile<CLIP, F, true, false, true, false, true>(T, D, A, R, DofFitOriArgs{}, H, DofFitApartArgs{}, U);
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_orient_robust_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                                    DofFitOriArgs O, DofFitPriorArgs H, DofFitRobustArgs U)
{
    dof_fit_tile<CLIP, F, true, true, true, false, true>(T, D, A, R, O, H, DofFitApartArgs{}, U);
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_apart_robust_group(TopoView T, DofView D, DofFitArgs A, DofFitRootArgs R,
                                                                   DofFitPriorArgs H, DofFitApartArgs Z, DofFitRobustArgs U)
{
    dof_fit_tile<CLIP, F, true, false, true, true, true>(T, D, A, R, DofFitOriArgs{}, H, Z, U);
}

template <bool CLIP, int F>
__global__ __launch_bounds__(64) void k_dof_fit_orient_apart_robust_group(TopoView T, DofView D, DofFitArgs A,
                                                                          DofFitRootArgs R, DofFitOriArgs O,
                                                                          DofFitPriorArgs H, DofFitApartArgs Z,
                                                                          DofFitRobustArgs U)
{
    dof_fit_tile<CLIP, F, true, true, true, true, true>(T, D, A, R, O, H, Z, U);
}

template <bool ROOT>
static hipError_t launch_fit(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A, const DofFitRootArgs &R,
                             hipStream_t s)
{
    if (!T.gsched) return hipErrorInvalidValue;   // J > kGroupMaxJ: the caller reports it as unsupported
    const int F = T.gF;
    const size_t lds = sizeof(float) * FitImages(nullptr, T.J, F, T.gsteps, ROOT).floats;
    if (lds > kFitMaxLdsBytes) return hipErrorInvalidValue;
    hipError_t attr = hipSuccess;
    group_dispatch(F, [&](auto f, auto cl) {
        if constexpr (ROOT) {
            attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_root_group<cl(), f()>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
            if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_root_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A, R);
        } else {
            attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_group<cl(), f()>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
            if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A);
        }
    }, clip);
    if (attr != hipSuccess) return attr;
    return hipGetLastError();
}

hipError_t launch_dof_fit(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A, hipStream_t s)
{
    return launch_fit<false>(T, D, clip, A, DofFitRootArgs{}, s);
}

hipError_t launch_dof_fit_root(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                               const DofFitRootArgs &R, hipStream_t s)
{
    return launch_fit<true>(T, D, clip, A, R, s);
}

hipError_t launch_dof_fit_orient(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                 const DofFitRootArgs &R, const DofFitOriArgs &O, hipStream_t s)
{
    if (!T.gsched || O.K < 0 || O.K > RTG_FIT_MAX_ROT_LINKS) return hipErrorInvalidValue;
    for (int k = 0; k < O.K; ++k)   // the kernel indexes rows with them
        if (O.joint[k] < 0 || O.joint[k] >= T.J) return hipErrorInvalidValue;
    const int F = T.gF;
    const size_t lds = sizeof(float) * FitImages(nullptr, T.J, F, T.gsteps, true, O.K).floats;
    if (lds > kFitMaxLdsBytes) return hipErrorInvalidValue;
    hipError_t attr = hipSuccess;
    group_dispatch(F, [&](auto f, auto cl) {
        attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_orient_group<cl(), f()>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
        if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_orient_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A, R, O);
    }, clip);
    if (attr != hipSuccess) return attr;
    return hipGetLastError();
}

hipError_t launch_dof_fit_prior(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                const DofFitRootArgs &R, const DofFitOriArgs &O, const DofFitPriorArgs &H, hipStream_t s)
{
    if (!T.gsched || O.K < 0 || O.K > RTG_FIT_MAX_ROT_LINKS) return hipErrorInvalidValue;
    if ((H.flags & RTG_FIT_PROJECT) && (!D.lower || !D.upper)) return hipErrorInvalidValue;   // the kernel reads them
    for (int k = 0; k < O.K; ++k)   // the kernel indexes rows with them
        if (O.joint[k] < 0 || O.joint[k] >= T.J) return hipErrorInvalidValue;
    const int F = T.gF;
    const size_t lds = sizeof(float) * FitImages(nullptr, T.J, F, T.gsteps, true, O.K > 0 ? O.K : -1, true).floats;
    if (lds > kFitMaxLdsBytes) return hipErrorInvalidValue;
    hipError_t attr = hipSuccess;
    group_dispatch(F, [&](auto f, auto cl) {
        if (O.K > 0) {
            attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_orient_prior_group<cl(), f()>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
            if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_orient_prior_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A, R, O, H);
        } else {
            attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_prior_group<cl(), f()>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
            if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_prior_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A, R, H);
        }
    }, clip);
    if (attr != hipSuccess) return attr;
    return hipGetLastError();
}

hipError_t launch_dof_fit_apart(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                const DofFitRootArgs &R, const DofFitOriArgs &O, const DofFitPriorArgs &H,
                                const DofFitApartArgs &Z, hipStream_t s)
{
    if (!T.gsched || O.K < 0 || O.K > RTG_FIT_MAX_ROT_LINKS) return hipErrorInvalidValue;
    if ((H.flags & RTG_FIT_PROJECT) && (!D.lower || !D.upper)) return hipErrorInvalidValue;   // the kernel reads them
    for (int k = 0; k < O.K; ++k)   // the kernel indexes rows with them
        if (O.joint[k] < 0 || O.joint[k] >= T.J) return hipErrorInvalidValue;
    if (Z.S < 1 || Z.S > RTG_FIT_MAX_SPHERES || Z.Pn < 0 || Z.Pn > RTG_FIT_MAX_PAIRS) return hipErrorInvalidValue;
    if (Z.S < 32 && (Z.floor_mask >> Z.S) != 0u) return hipErrorInvalidValue;
    for (int i = 0; i < Z.S; ++i)   // likewise
        if (Z.link[i] < 0 || Z.link[i] >= T.J) return hipErrorInvalidValue;
    for (int p = 0; p < Z.Pn; ++p)
        if ((Z.pair[p] & 0xFF) >= Z.S || (Z.pair[p] >> 8) < 0 || (Z.pair[p] >> 8) >= Z.S) return hipErrorInvalidValue;
    const int F = T.gF;
    const size_t lds = sizeof(float) * (FitImages(nullptr, T.J, F, T.gsteps, true, O.K > 0 ? O.K : -1, true).floats +
                                        ApartImages(nullptr, T.J, F, Z.S, Z.Pn).floats);
    if (lds > kFitMaxLdsBytes) return hipErrorInvalidValue;
    hipError_t attr = hipSuccess;
    group_dispatch(F, [&](auto f, auto cl) {
        if (O.K > 0) {
            attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_orient_apart_group<cl(), f()>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
            if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_orient_apart_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A, R, O, H, Z);
        } else {
            attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dof_fit_apart_group<cl(), f()>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFitMaxLdsBytes);
            if (attr == hipSuccess) hipLaunchKernelGGL((k_dof_fit_apart_group<cl(), f()>), dim3(grid_for(A.B, F)), dim3(64), lds, s, T, D, A, R, H, Z);
        }
    }, clip);
    if (attr != hipSuccess) return attr;
    return hipGetLastError();
}

// apart: Z holds a term (launch_dof_fit_apart's checks then); without one Z is not looked at
hipError_t launch_dof_fit_robust(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                 const DofFitRootArgs &R, const DofFitOriArgs &O, const DofFitPriorArgs &H,
                                 const DofFitApartArgs &Z, bool apart, const DofFitRobustArgs &U, hipStream_t s)
{
    if (!T.gsched || O.K < 0 || O.K > RTG_FIT_MAX_ROT_LINKS) return hipErrorInvalidValue;
    if ((H.flags & RTG_FIT_PROJECT) && (!D.lower || !D.upper)) return hipErrorInvalidValue;   // the kernel reads them
    for (int k = 0; k < O.K; ++k)   // the kernel indexes rows with them
        if (O.joint[k] < 0 || O.joint[k] >= T.J) return hipErrorInvalidValue;
    if (apart) {
        if (Z.S < 1 || Z.S > RTG_FIT_MAX_SPHERES || Z.Pn < 0 || Z.Pn > RTG_FIT_MAX_PAIRS) return hipErrorInvalidValue;
        if (Z.S < 32 && (Z.floor_mask >> Z.S) != 0u) return hipErrorInvalidValue;
        for (int i = 0; i < Z.S; ++i)   // likewise
            if (Z.link[i] < 0 || Z.link[i] >= T.J) return hipErrorInvalidValue;
        for (int p = 0; p < Z.Pn; ++p)
            if ((Z.pair[p] & 0xFF) >= Z.S || (Z.pair[p] >> 8) < 0 || (Z.pair[p] >> 8) >= Z.S) return hipErrorInvalidValue;
    }
    if (!(U.robust_scale >= 0.0f) || !(U.inv_d2 >= 0.0f)) return hipErrorInvalidValue;
    const int F = T.gF;
    const size_t lds = sizeof(float) * (FitImages(nullptr, T.J, F, T.gsteps, true, O.K > 0 ? O.K : -1, true).floats +
                                        (apart ? ApartImages(nullptr, T.J, F, Z.S, Z.Pn).floats : 0) +
                                        RobustImages(nullptr, T.J, F).floats);
    if (lds > kFitMaxLdsBytes) return hipErrorInvalidValue;
    hipError_t attr = hipSuccess;
    const dim3 grid(grid_for(A.B, F));
    auto go = [&](auto kern, auto... args) {
        attr = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kFitMaxLdsBytes);
        if (attr == hipSuccess) hipLaunchKernelGGL(kern, grid, dim3(64), lds, s, T, D, A, R, args...);
    };
    group_dispatch(F, [&](auto f, auto cl) {
        if (apart && O.K > 0) go(&k_dof_fit_orient_apart_robust_group<cl(), f()>, O, H, Z, U);
        else if (apart) go(&k_dof_fit_apart_robust_group<cl(), f()>, H, Z, U);
        else if (O.K > 0) go(&k_dof_fit_orient_robust_group<cl(), f()>, O, H, U);
        else go(&k_dof_fit_robust_group<cl(), f()>, H, U);
    }, clip);
    if (attr != hipSuccess) return attr;
    return hipGetLastError();
}

}  // namespace rtg

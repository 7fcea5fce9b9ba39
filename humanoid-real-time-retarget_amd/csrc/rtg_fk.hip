// rtg_fk.hip -- forward / inverse kinematics kernels (kinematics.py:13-63, skeleton3d.py:402-484,
// hu_forward_model.py:17-33) and their launchers.  Every topology of J <= kGroupMaxJ joints (all shipped skeletons)
// runs the lane-group kernels below; larger trees fall back to the lane walks (one frame per thread).
#include "rtg_device.cuh"
#include "rtg_fk_group.cuh"
#include "rtg_group_sched.h"

namespace rtg {

// ----------------------------------------------------------------------------
// forward kinematics -- one frame per lane, joints in topological (index) order.
// The parent's global rotation / position is reused from registers when the
// parent is the previous joint (chains), else re-read from the output rows this
// lane has just written (branch points; L2-resident).  Topology is uniform
// across the grid, so the loop body and all topology loads are scalar.
// ----------------------------------------------------------------------------
template <bool STATE>
RTG_DEV void fk_frame(const TopoView &T, const float *__restrict__ lr, const float *__restrict__ rt,
                      float *__restrict__ gr, float *__restrict__ gp)
{
    Q g = ld4(lr);            // root: global = local (not normalised) kinematics.py:27-29
    V t = ld3(rt);
    st4(gr, g);
    st3(gp, t);
    for (int j = 1; j < T.J; ++j) {
        const int p = T.parents[j];
        if (p != j - 1) {
            g = ld4(gr + 4 * p);
            t = ld3(gp + 3 * p);
        }
        Q lq = ld4(lr + 4 * j);
        if (STATE) lq = qmul_norm(T.tree_quat[j], lq);   // skeleton3d.py:412-418
        const V zl = T.local_t[j];
        const V rot = qrotate(g, zl);
        const Q ng = qmul_norm(g, lq);
        const V nt = V{rot.x + t.x, rot.y + t.y, rot.z + t.z};
        st4(gr + 4 * j, ng);
        st3(gp + 3 * j, nt);
        g = ng;
        t = nt;
    }
}

template <bool STATE>
__global__ __launch_bounds__(256) void k_fk(TopoView T, const float *__restrict__ local_rot,
                                            const float *__restrict__ root_t, int64_t B, float *__restrict__ g_rot,
                                            float *__restrict__ g_pos)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= B) return;
    fk_frame<STATE>(T, local_rot + f * T.J * 4, root_t + f * 3, g_rot + f * T.J * 4, g_pos + f * T.J * 3);
}

template <bool STATE>
__global__ __launch_bounds__(256) void k_local_rotation(TopoView T, const float *__restrict__ g_rot, int64_t B,
                                                        float *__restrict__ local_rot)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= B) return;
    const float *g = g_rot + f * T.J * 4;
    float *l = local_rot + f * T.J * 4;
    st4(l, ld4(g));
    for (int j = 1; j < T.J; ++j) {
        const int p = T.parents[j];
        Q q = qmul_norm(qconj(ld4(g + 4 * p)), ld4(g + 4 * j));
        if (STATE) q = qmul_norm(qnormalize(qconj(T.tree_quat[j])), q);   // skeleton3d.py:477-481
        st4(l + 4 * j, q);
    }
}

__global__ __launch_bounds__(256) void k_fk_multi(FkMultiArgs A)
{
    int s = 0;
#pragma unroll
    for (int i = 1; i < RTG_MAX_SEGMENTS; ++i)
        if (i < A.n && (int64_t)blockIdx.x >= A.block_start[i]) s = i;
    const FkSeg &S = A.seg[s];
    const int64_t f = ((int64_t)blockIdx.x - A.block_start[s]) * blockDim.x + threadIdx.x;
    if (f >= S.B) return;
    if (S.op == 0) {
        fk_frame<false>(S.T, S.local_rot + f * S.T.J * 4, S.root_t + f * 3, S.g_rot + f * S.T.J * 4,
                        S.g_pos + f * S.T.J * 3);
        return;
    }
    const float *g = S.local_rot + f * S.T.J * 4;   // inverse FK, kinematics.py:41-63
    float *l = S.g_rot + f * S.T.J * 4;
    st4(l, ld4(g));
    for (int j = 1; j < S.T.J; ++j) st4(l + 4 * j, qmul_norm(qconj(ld4(g + 4 * S.T.parents[j])), ld4(g + 4 * j)));
}


// HuForwardModel lane walk (J > kGroupMaxJ): joint j's local rotation from its DOF, then fk_frame's composition
template <bool CLIP>
__global__ __launch_bounds__(256) void k_dof_fk_walk(TopoView T, DofView D, const float *__restrict__ dof,
                                                     const float *__restrict__ root_rot,
                                                     const float *__restrict__ root_t, int64_t B,
                                                     float *__restrict__ g_rot, float *__restrict__ g_pos)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= B) return;
    const int J = T.J;
    const float *drow = dof + f * (J - 1);
    float *gr = g_rot + f * J * 4, *gp = g_pos + f * J * 3;
    st4(gr, ld4(root_rot + f * 4));   // root: the root rotation, unnormalised (hu_forward_model.py:24)
    st3(gp, ld3(root_t + f * 3));
    for (int j = 1; j < T.J; ++j) {
        const int p = T.parents[j];
        float a = drow[j - 1];
        if (CLIP) a = clamp_st(a, D.lower[j - 1], D.upper[j - 1]);
        const int ax = D.axis[j - 1];
        const Q lq = qfrom_angle_unit_axis(a, V{ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f});
        const Q g = ld4(gr + 4 * p);
        const V t = ld3(gp + 3 * p);
        const V rv = qrotate(g, T.local_t[j]);
        st4(gr + 4 * j, qmul_norm(g, lq));
        st3(gp + 3 * j, V{rv.x + t.x, rv.y + t.y, rv.z + t.z});
    }
}

// ----------------------------------------------------------------------------
// Lane-group kinematics (round 6): a frame's joints spread over a GROUP of lanes, F frames per wave (F = 16: four
// lanes per frame for J <= 36; F = 8: eight lanes for J <= 64), so the tile's rows move as whole coalesced pieces.
// The windowed kernels above keep one frame per lane, and each of their load / store instructions touches 64 rows
// ~500 bytes apart (FETCH 1.75x, WRITE 1.22x the algorithmic bytes on Hu FK, round 4 PMC; a memory-pattern probe of
// those pieces alone tops out at 3.45 TB/s).  Here the F frames of a tile are F J consecutive 16-byte records: lane
// l of load k takes record 64 k + l, so every instruction reads or writes 1 KiB of consecutive bytes, each line of
// the rows is requested once, and the positions leave as consecutive dwordx4 pieces.  The records go through LDS:
//   1. every record of the tile is loaded (all loads in flight) and stored into the LDS image of the rows;
//   2. the joints are composed by a host-built list schedule (group_list_schedule, rtg_group_sched.h): at step s,
//      sub-lane u of each frame's group composes the joint the schedule names, reading its parent's global transform
//      from the image and writing its own over its local rotation -- a parent is always composed earlier.  Each joint is
//      composed exactly as in kinematics.py:27-37 / fk_stream_tile (same device functions, same operands, same
//      order), so the bits are the same whatever the schedule; only which lane does it and when changes.  Hu: 31
//      joints in 10 steps (its depth + 1) on four lanes;
//   3. the global rotations and positions leave from the image, record-ordered (coalesced).
// LDS per wave: F J 28 bytes plus the schedule (Hu: 13.9 + 1.3 KiB).  Inverse FK (kinematics.py:41-63) has no chain:
// each record's parent is read from the image and its local rotation stored straight from the lane that loaded it.
// ----------------------------------------------------------------------------
template <bool STATE, int F>
RTG_DEV void fk_group_tile(const TopoView &T, const float *__restrict__ local_rot, const float *__restrict__ root_t,
                           int64_t B, int64_t f0, float *__restrict__ g_rot, float *__restrict__ g_pos, float *lds)
{
    const int J = T.J;
    const int nfr = tile_frames<F>(B, f0), nrec = nfr * J;
    const FkImages I(lds, J, F, T.gsteps, false);
    GroupRows<F> rows;
    rows.load(local_rot + f0 * J * 4, nrec);
    const float r = root_t_load(root_t, f0, nfr);
    group_sched_fill(T, Grp<F>::L, I.sch);
    if (RTG_FK_UNIT_TAB) unit_tab_fill(I.utab, (int)threadIdx.x);
    rows.store(I.rot, nrec);
    root_preset(I.pos, J, nfr, r);
    wave_sync();
    group_compose<F>(T, I.rot, I.pos, I.sch, nfr, I.utab, [&](int, Q lq, const GEnt &e, int) {
        if (STATE) lq = qmul_norm(Q{e.qx, e.qy, e.qz, e.qw}, lq, fk_tab(I.utab));   // skeleton3d.py:412-418
        return lq;
    });
    group_store<F>(I.rot, I.pos, nrec, g_rot + f0 * J * 4, g_pos + f0 * J * 3);
}

template <bool STATE, int F>
__global__ __launch_bounds__(64, 4) void k_fk_group(TopoView T, const float *__restrict__ local_rot,
                                                 const float *__restrict__ root_t, int64_t B, float *__restrict__ g_rot,
                                                 float *__restrict__ g_pos)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    fk_group_tile<STATE, F>(T, local_rot, root_t, B, (int64_t)blockIdx.x * F, g_rot, g_pos, fk_lds);
}

// inverse FK
constexpr int kLrotFrames = 8;   // frames per wave of the inverse tiles (any J <= kGroupMaxJ)
struct LrotImages {
    f4v *rot;        // [F J] the global rotations
    int *par;        // [J] the parents
    f4v *tqn;        // [J] STATE: the normalised conjugate tree quaternions
    UnitEnt *utab;   // the near-unit table
    size_t floats;
    __host__ __device__ LrotImages(float *base, int J, int F)
    {
        LdsCarve c(base);
        rot = c.take<f4v>((size_t)F * J);
        par = c.take<int>(J);
        tqn = c.take<f4v>(J);
        utab = c.take_unit_tab();
        floats = c.floats;
    }
};
template <bool STATE, int F>
RTG_DEV void lrot_group_tile(const TopoView &T, const float *__restrict__ g_rot, int64_t B, int64_t f0,
                             float *__restrict__ local_rot, float *lds)
{
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x;
    const int nfr = tile_frames<F>(B, f0), nrec = nfr * J;
    const LrotImages I(lds, J, F);
    f4v *rot = I.rot;
    const UnitEnt *utab = I.utab;
    GroupRows<F> rows;
    rows.load(g_rot + f0 * J * 4, nrec);
    if (RTG_FK_UNIT_TAB) unit_tab_fill(I.utab, (int)threadIdx.x);
    for (int j = lane; j < J; j += 64) {
        I.par[j] = ld_const(T.parents + j);
        // skeleton3d.py:470-478: quat_normalize(quat_conjugate(tree quat)), once per joint
        if (STATE) I.tqn[j] = v_of(qnormalize(qconj(ld_const(T.tree_quat + j))));
    }
    rows.store(rot, nrec);
    wave_sync();
    const float rJ = item_rcp(J);
    f4v *dst = reinterpret_cast<f4v *>(local_rot + f0 * J * 4);
#pragma unroll 3
    for (int k = 0; k < G::NR; ++k) {   // the records from the image: the loaded registers are free by now
        const int rec = k * 64 + lane;
        if (rec < nrec) {
            const Item it = item_split(rec, rJ, J);
            const Q gj = q_of(rot[rec]);
            Q q = gj;   // root copied (kinematics.py:49)
            if (it.j > 0) {
                q = qmul_norm(qconj(q_of(rot[it.fr * J + I.par[it.j]])), gj, fk_tab(utab));
                if (STATE) q = qmul_norm(q_of(I.tqn[it.j]), q, fk_tab(utab));
            }
            st_out(dst + rec, v_of(q));
        }
    }
}

template <bool STATE, int F>
__global__ __launch_bounds__(64, 4) void k_lrot_group(TopoView T, const float *__restrict__ g_rot, int64_t B,
                                                   float *__restrict__ local_rot)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    lrot_group_tile<STATE, F>(T, g_rot, B, (int64_t)blockIdx.x * F, local_rot, fk_lds);
}

// HuForwardModel (hu_forward_model.py:17-33) on the lane groups.  The local rotations do not depend on the chain, so
// they are built first, all at once: each lane turns the DOFs it loaded (the tile's rows are nfr (J - 1) consecutive
// floats, NR loads per lane) into joint rotations -- quat_from_angle_axis of the clipped angle about the joint's unit
// axis -- and writes them into the tile image where FK's local rotations would be; then FK's compose runs as is.  (A
// first version built each joint's rotation inside its compose step: the f64 sincos sat on the chain's critical path
// and the kernel took 128 us against FK's 88, profiles/r06/fk/.)  LDS: FkImages with the per-joint table.
template <bool CLIP, int F>
__global__ __launch_bounds__(64, 4) void k_dof_fk_group(TopoView T, DofView D, const float *__restrict__ dof,
                                                     const float *__restrict__ root_rot,
                                                     const float *__restrict__ root_t, int64_t B,
                                                     float *__restrict__ g_rot, float *__restrict__ g_pos)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x, nd = J - 1;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(B, f0), nrec = nfr * J, nang = nfr * nd;
    const FkImages I(fk_lds, J, F, T.gsteps, true);
    f4v *rot = I.rot;
    const f4v *ntab = I.ntab;
    const UnitEnt *utab = I.utab;
    ScalarRows<F> a;
    a.load(dof + f0 * nd, nang);
    const f4v rr = root_rot_load(root_rot, f0, nfr);
    const float rt = root_t_load(root_t, f0, nfr);
    group_sched_fill(T, G::L, I.sch);
    if (kUnitTab) unit_tab_fill(I.utab, (int)threadIdx.x);
    joint_tab_fill<CLIP, false>(D, J, I.ntab);
    root_preset(rot, I.pos, J, nfr, rr, rt);
    wave_sync();
    const float rnd = item_rcp(nd > 0 ? nd : 1);
    const DofRotations<CLIP, F> rotations{a, ntab, utab, rot, J, nd, nang, lane, rnd};
    constexpr int NW = RTG_DOF_NWAY, NFULL = G::NR - G::NR % NW;
#pragma unroll
    for (int k = 0; k < NFULL; k += NW) rotations(std::integral_constant<int, NW>{}, k);
#pragma unroll
    for (int k = NFULL; k < G::NR; ++k) rotations(std::integral_constant<int, 1>{}, k);
    wave_sync();
    group_compose<F>(T, rot, I.pos, I.sch, nfr, utab, [&](int, Q lq, const GEnt &, int) { return lq; });
    group_store<F>(rot, I.pos, nrec, g_rot + f0 * J * 4, g_pos + f0 * J * 3);
}

// Link velocities from joint velocities (rtg_dof_fk_vel_f32): k_dof_fk_group's tile with a twist image [F J 6] behind
// FkImages (24 F J bytes more: Hu v5 at F = 16, 11.6 KiB) and group_compose_vel's tangent sweep in place of the
// compose.  The tile's joint velocities are loaded with its angles (the same row shape); after the table fill each
// one goes, through the clip select, into the first float of its joint's twist row, where it waits for the joint's
// step; the root twists (6 nfr consecutive floats, +0 without root_vel) are preset like the root poses.  The twist
// rows leave as consecutive 16-byte pieces (a tile's rows start 16-byte aligned when g_vel does: F is a multiple of
// 8); g_rot / g_pos leave as in k_dof_fk_group, or not at all (nullptr: the velocity-only call, the same g_vel).
struct FkVelImages {
    FkImages fk;
    float *tw;       // [F J 6] the twists {v, w}
    size_t floats;
    __host__ __device__ FkVelImages(float *base, int J, int F, int steps) : fk(base, J, F, steps, true)
    {
        tw = base ? base + fk.floats : nullptr;
        floats = fk.floats + pad16f((size_t)6 * F * J);
    }
};
template <bool CLIP, int F>
__global__ __launch_bounds__(64, 4) void k_dof_fk_vel_group(TopoView T, DofView D, const float *__restrict__ dof,
                                                         const float *__restrict__ dof_vel,
                                                         const float *__restrict__ root_rot,
                                                         const float *__restrict__ root_t,
                                                         const float *__restrict__ root_vel, int64_t B,
                                                         float *__restrict__ g_rot, float *__restrict__ g_pos,
                                                         float *__restrict__ g_vel)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x, nd = J - 1;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(B, f0), nrec = nfr * J, nang = nfr * nd;
    const FkVelImages IV(fk_lds, J, F, T.gsteps);
    const FkImages &I = IV.fk;
    f4v *rot = I.rot;
    float *tw = IV.tw;
    const f4v *ntab = I.ntab;
    const UnitEnt *utab = I.utab;
    ScalarRows<F> a, ad;
    a.load(dof + f0 * nd, nang);
    ad.load(dof_vel + f0 * nd, nang);
    const f4v rr = root_rot_load(root_rot, f0, nfr);
    const float rt = root_t_load(root_t, f0, nfr);
    float rw[2] = {0.0f, 0.0f};   // the root twists: float 64 k + lane of the tile's 6 nfr (F <= 16: two pieces)
    if (root_vel) {
#pragma unroll
        for (int k = 0; k < 2; ++k) rw[k] = root_vel[f0 * 6 + (64 * k + lane < 6 * nfr ? 64 * k + lane : 0)];
    }
    group_sched_fill(T, G::L, I.sch);
    if (kUnitTab) unit_tab_fill(I.utab, (int)threadIdx.x);
    joint_tab_fill<CLIP, false>(D, J, I.ntab);
    root_preset(rot, I.pos, J, nfr, rr, rt);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = 64 * k + lane, fr = i / 6;
        if (i < 6 * nfr) tw[6 * J * fr + (i - 6 * fr)] = rw[k];
    }
    wave_sync();
    const float rnd = item_rcp(nd > 0 ? nd : 1);
    lane_items<G::NR>([&](int k, int i) {   // the rates into their joints' twist rows
        if (i < nang) {
            const Item it = item_split(i, rnd, nd);
            tw[6 * (it.fr * J + it.j + 1)] = joint_rate<CLIP>(a.v[k], ad.v[k], ntab[it.j + 1]);
        }
    });
    const DofRotations<CLIP, F> rotations{a, ntab, utab, rot, J, nd, nang, lane, rnd};
    constexpr int NW = RTG_DOF_NWAY, NFULL = G::NR - G::NR % NW;
#pragma unroll
    for (int k = 0; k < NFULL; k += NW) rotations(std::integral_constant<int, NW>{}, k);
#pragma unroll
    for (int k = NFULL; k < G::NR; ++k) rotations(std::integral_constant<int, 1>{}, k);
    wave_sync();
    group_compose_vel<F>(T, rot, I.pos, tw, I.sch, ntab, nfr, utab);
    if (g_rot) group_store<F>(rot, I.pos, nrec, g_rot + f0 * J * 4, g_pos + f0 * J * 3);
    PosRows<F>::out(tw, g_vel + f0 * J * 6, 6 * nrec);
}

// Mixed-target kinematics on the lane groups (config 5): a block is one tile of one segment; the segment's F comes
// from its topology
__global__ __launch_bounds__(64, 4) void k_fk_multi_group(FkMultiArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float fk_lds[];
    int s = 0;
#pragma unroll
    for (int i = 1; i < RTG_MAX_SEGMENTS; ++i)
        if (i < A.n && (int64_t)blockIdx.x >= A.block_start[i]) s = i;
    const FkSeg &S = A.seg[s];
    const int64_t t = (int64_t)blockIdx.x - A.block_start[s];
    if (S.op == 1) lrot_group_tile<false, kLrotFrames>(S.T, S.local_rot, S.B, t * kLrotFrames, S.g_rot, fk_lds);
    else if (S.T.gF == 16) fk_group_tile<false, 16>(S.T, S.local_rot, S.root_t, S.B, t * 16, S.g_rot, S.g_pos, fk_lds);
    else fk_group_tile<false, 8>(S.T, S.local_rot, S.root_t, S.B, t * 8, S.g_rot, S.g_pos, fk_lds);
}

// Host: a topology's lane-group schedule: group_list_schedule's order over all J joints (the root takes an entry), each
// entry with its joint's local translation, tree quaternion and child links.  Returns the step count, or -1 if it
// would exceed max_steps.
int32_t fk_group_schedule(const int32_t *parents, const V *local_t, const Q *tree_quat, int32_t J, int32_t F,
                          GEnt *out, int32_t max_steps)
{
    std::vector<int> order;
    const int steps = group_list_schedule(parents, J, nullptr, true, 64 / F, max_steps, order);
    std::vector<uint32_t> fc, ns;
    group_child_links(parents, J, fc, ns);
    for (size_t i = 0; steps > 0 && i < order.size(); ++i) {
        const int j = order[i];
        out[i] = GEnt{0.f, 0.f, 0.f, 0xFFFF, 0.f, 0.f, 0.f, 1.f};
        if (j < 0) continue;
        const uint32_t code = (uint32_t)j | ((uint32_t)(j ? parents[j] : 0xFF) << 8) | (fc[j] << 16) | (ns[j] << 24);
        out[i] = GEnt{local_t[j].x, local_t[j].y, local_t[j].z, (int32_t)code,
                      tree_quat[j].x, tree_quat[j].y, tree_quat[j].z, tree_quat[j].w};
    }
    return steps;
}

hipError_t launch_fk(const TopoView &T, bool state, const float *lr, const float *rt, int64_t B, float *gr, float *gp,
                     hipStream_t s)
{
    if (T.gsched) {
        const int F = T.gF;
        const size_t lds = sizeof(float) * FkImages(nullptr, T.J, F, T.gsteps, false).floats;
        group_dispatch(F, [&](auto f, auto st) {
            hipLaunchKernelGGL((k_fk_group<st(), f()>), dim3(grid_for(B, F)), dim3(64), lds, s, T, lr, rt, B, gr, gp);
        }, state);
    } else if (state) {   // J > kGroupMaxJ: lane walk
        hipLaunchKernelGGL(k_fk<true>, dim3(grid_for(B, 256)), dim3(256), 0, s, T, lr, rt, B, gr, gp);
    } else {
        hipLaunchKernelGGL(k_fk<false>, dim3(grid_for(B, 256)), dim3(256), 0, s, T, lr, rt, B, gr, gp);
    }
    return hipGetLastError();
}

hipError_t launch_local_rotation(const TopoView &T, bool state, const float *g, int64_t B, float *l, hipStream_t s)
{
    if (T.gsched) {   // 8 frames per wave whatever J: no chain here, so the smallest tile -- the most waves per CU --
                      // wins (Hu: 41.4 vs 46.8 us at 16 frames, profiles/r06/fk/)
        const size_t lds = sizeof(float) * LrotImages(nullptr, T.J, kLrotFrames).floats;
        dispatch_bools([&](auto st) {
            hipLaunchKernelGGL((k_lrot_group<st(), kLrotFrames>), dim3(grid_for(B, kLrotFrames)), dim3(64), lds, s, T, g,
                               B, l);
        }, state);
    } else if (state) {   // J > kGroupMaxJ: lane walk
        hipLaunchKernelGGL(k_local_rotation<true>, dim3(grid_for(B, 256)), dim3(256), 0, s, T, g, B, l);
    } else {
        hipLaunchKernelGGL(k_local_rotation<false>, dim3(grid_for(B, 256)), dim3(256), 0, s, T, g, B, l);
    }
    return hipGetLastError();
}

hipError_t launch_fk_multi(FkMultiArgs &A, hipStream_t s)
{
    bool group = true;
    for (int i = 0; i < A.n; ++i) group = group && A.seg[i].T.gsched != nullptr;
    // every segment on the lane groups: one block per F-frame tile of its segment; else every segment's lane walk
    int64_t blocks = 0;
    size_t lds = 0;
    for (int i = 0; i < A.n; ++i) {
        const TopoView &T = A.seg[i].T;
        A.block_start[i] = blocks;
        blocks += grid_for(A.seg[i].B, group ? (A.seg[i].op == 0 ? T.gF : kLrotFrames) : 256);
        if (group) {
            const size_t need = A.seg[i].op == 0 ? FkImages(nullptr, T.J, T.gF, T.gsteps, false).floats
                                                 : LrotImages(nullptr, T.J, kLrotFrames).floats;
            lds = need > lds ? need : lds;
        }
    }
    for (int i = A.n; i < RTG_MAX_SEGMENTS; ++i) A.block_start[i] = blocks;
    if (blocks == 0) return hipSuccess;
    if (group) hipLaunchKernelGGL(k_fk_multi_group, dim3((unsigned)blocks), dim3(64), sizeof(float) * lds, s, A);
    else hipLaunchKernelGGL(k_fk_multi, dim3((unsigned)blocks), dim3(256), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_dof_fk(const TopoView &T, const DofView &D, bool clip, const float *dof, const float *root_rot,
                         const float *root_t, int64_t B, float *gr, float *gp, hipStream_t s)
{
    if (T.gsched) {
        const int F = T.gF;
        const size_t lds = sizeof(float) * FkImages(nullptr, T.J, F, T.gsteps, true).floats;
        group_dispatch(F, [&](auto f, auto cl) {
            hipLaunchKernelGGL((k_dof_fk_group<cl(), f()>), dim3(grid_for(B, F)), dim3(64), lds, s, T, D, dof, root_rot,
                               root_t, B, gr, gp);
        }, clip);
    } else if (clip) {   // J > kGroupMaxJ: lane walk
        hipLaunchKernelGGL(k_dof_fk_walk<true>, dim3(grid_for(B, 256)), dim3(256), 0, s, T, D, dof, root_rot, root_t, B,
                           gr, gp);
    } else {
        hipLaunchKernelGGL(k_dof_fk_walk<false>, dim3(grid_for(B, 256)), dim3(256), 0, s, T, D, dof, root_rot, root_t, B,
                           gr, gp);
    }
    return hipGetLastError();
}

// lane groups only (T.gsched); g_rot / g_pos both nullptr: the velocity-only call
hipError_t launch_dof_fk_vel(const TopoView &T, const DofView &D, bool clip, const float *dof, const float *dof_vel,
                             const float *root_rot, const float *root_t, const float *root_vel, int64_t B, float *gr,
                             float *gp, float *gv, hipStream_t s)
{
    const int F = T.gF;
    const size_t lds = sizeof(float) * FkVelImages(nullptr, T.J, F, T.gsteps).floats;
    group_dispatch(F, [&](auto f, auto cl) {
        hipLaunchKernelGGL((k_dof_fk_vel_group<cl(), f()>), dim3(grid_for(B, F)), dim3(64), lds, s, T, D, dof, dof_vel,
                           root_rot, root_t, root_vel, B, gr, gp, gv);
    }, clip);
    return hipGetLastError();
}

}  // namespace rtg

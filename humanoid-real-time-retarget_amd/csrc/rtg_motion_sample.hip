// rtg_motion_sample.hip -- sample a motion library at arbitrary (clip, time) pairs in ONE launch on the lane groups of
// rtg_fk_group.cuh: the index rule (rtg_motion_index.h), the gather of the two frames, quat_slerp
// (transform3d.py:152-174) per joint, the optional quat_normalize, the linear blends of the root translation and the
// vector rows, and the optional forward kinematics of the blended pose.
//
// A library is C clips of one skeleton packed frame-major: rot (F_total, J, 4), root_t (F_total, 3), vec
// (F_total, K, 3) and one 16-byte entry {start, len, fps} per clip (MotionClip, validated on the host at creation: a
// valid clip id never indexes outside the arrays).  A tile is one wave and F queries (group_frames(J)), 64 / F lanes
// per query:
//   1. the first F lanes load (clip, time) and the clip entry and run the index rule; {row0, row1, b, valid} per query
//      goes to an LDS table.  A lane past N repeats query 0; an invalid query gets rows 0 (never dereferenced with a
//      bad index) and its flag;
//   2. record r = 64 k + lane is (query, joint) by item_split: the lane loads the two source records, takes qslerp (and
//      qnormalize through the near-unit table when asked) and stores the local rotation, record-ordered: whole-wave
//      stores.  The J records of a query are consecutive (496 B on Hu), so each wave instruction reads whole rows.  At
//      most four record pairs per lane are in flight at a time (registers: 4 waves per SIMD);
//   3. the root translation and the vector rows are dword gathers blended as torch's (1 - b) * a + b * c: four f32
//      roundings, no FMA (the TU is built with -ffp-contract=off);
//   4. with GLOBAL the local rotations also go into the FK tile's image, the roots are preset, and group_compose /
//      group_store run as in fk_group_tile: the bits of rtg_fk_f32 / rtg_state_fk_f32 on this launch's own outputs.
// An invalid query's rows are the quiet NaN 0x7FC00000 everywhere; the rest of its tile is unaffected.  Every value is
// computed by the device functions the element-wise ops use (qslerp, qnormalize) on the reference's operands, so the
// bits do not depend on N, on the query's place in its tile or on the grouping.
#include "rtg_device.cuh"
#include "rtg_fk_group.cuh"
#include "rtg_motion_index.h"

namespace rtg {

// one query of the tile's table
struct alignas(16) MsQuery {
    int32_t row0, row1;   // library rows (start + i0, start + i1); 0 for an invalid query
    float b;
    int32_t valid;
};

// The sampler tile's images.  Without GLOBAL only the query table and the near-unit table are carved.
struct MsImages {
    MsQuery *qt;     // [F] the query table
    UnitEnt *utab;   // the near-unit table
    f4v *rot;        // GLOBAL: [F J] the local rotations, overwritten by the global ones
    float *pos;      // GLOBAL: [F J 3] the positions, the root's preset
    GEnt *sch;       // GLOBAL: [gsteps L] the schedule
    size_t floats;
    __host__ __device__ MsImages(float *base, int J, int F, int steps, bool global)
    {
        LdsCarve c(base);
        qt = c.take<MsQuery>((size_t)F);
        utab = c.take_unit_tab();
        rot = c.take<f4v>(global ? (size_t)F * J : 0);
        pos = c.take<float>(global ? (size_t)3 * F * J : 0);
        sch = c.take<GEnt>(global ? (size_t)steps * (64 / F) : 0);
        floats = c.floats;
    }
};

RTG_DEV float ms_nan() { return __int_as_float(0x7FC00000); }
// torch's (1 - b) * a + b * c: each operation rounds on its own
RTG_DEV float ms_blend(float a, float c, float b) { return ((1.0f - b) * a) + (b * c); }

template <int F, bool NORM, bool GLOBAL, bool STATE>
__global__ __launch_bounds__(64, 4) void k_motion_sample(TopoView T, MotionLibView L, MotionSampleArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float ms_lds[];
    using G = Grp<F>;
    constexpr int NW = 4;   // record pairs per lane in flight
    const int J = T.J, lane = (int)threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(A.N, f0), nrec = nfr * J;
    const MsImages I(ms_lds, J, F, T.gsteps, GLOBAL);
    MsQuery *qt = I.qt;

    // 1. the query table
    if (lane < F) {
        const int64_t n = lane < nfr ? f0 + lane : 0;
        const int32_t clip = A.clip[n];
        const float time = A.time[n];
        const bool valid = motion_clip_valid(clip, L.C);
        const MotionClip ce = L.clips[valid ? clip : 0];
        const MotionIdx ix = motion_index(time, ce.fps, ce.len);
        qt[lane] = valid ? MsQuery{(int32_t)(ce.start + ix.i0), (int32_t)(ce.start + ix.i1), ix.b, 1}
                         : MsQuery{0, 0, 0.0f, 0};
    }
    if (GLOBAL) group_sched_fill(T, G::L, I.sch);
    if (kUnitTab && (NORM || GLOBAL)) unit_tab_fill(I.utab, lane);
    wave_sync();

    // 2. gather, slerp, normalize: record r = (query, joint)
    const float rJ = item_rcp(J);
    const f4v *src = reinterpret_cast<const f4v *>(A.rot);
    f4v *dst = reinterpret_cast<f4v *>(A.local_rot_out) + f0 * J;
    const f4v nan4{ms_nan(), ms_nan(), ms_nan(), ms_nan()};
#pragma unroll
    for (int k0 = 0; k0 < G::NR; k0 += NW) {
        if (k0 * 64 >= nrec) break;   // wave-uniform: no lane has a record in this group
        f4v a[NW], c[NW];
        float b[NW];
        bool ok[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (k0 + w >= G::NR) continue;
            const int rec = (k0 + w) * 64 + lane;
            const Item it = item_split(rec < nrec ? rec : 0, rJ, J);   // a lane past the records repeats record 0
            const MsQuery q = qt[it.fr];
            a[w] = src[(int64_t)q.row0 * J + it.j];
            c[w] = src[(int64_t)q.row1 * J + it.j];
            b[w] = q.b;
            ok[w] = q.valid != 0;
        }
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (k0 + w >= G::NR) continue;
            const int rec = (k0 + w) * 64 + lane;
            Q q = qslerp(q_of(a[w]), q_of(c[w]), b[w]);
            if (NORM) q = qnormalize(q, fk_tab(I.utab));
            const f4v v = ok[w] ? v_of(q) : nan4;
            if (rec < nrec) {
                st_out(dst + rec, v);
                if (GLOBAL) I.rot[rec] = v;
            }
        }
    }

    // 3. the blends: the root translations (lane = 3 query + component), then the vector rows query by query
    bool any_invalid = false;
    {
        const int fr = lane / 3, cpt = lane - 3 * fr;
        const bool live = lane < 3 * nfr;
        const MsQuery q = qt[live ? fr : 0];
        const float va = A.root_t[(int64_t)q.row0 * 3 + cpt], vc = A.root_t[(int64_t)q.row1 * 3 + cpt];
        const float r = q.valid ? ms_blend(va, vc, q.b) : ms_nan();
        if (live) {
            A.root_t_out[f0 * 3 + lane] = r;
            if (GLOBAL) I.pos[3 * J * fr + cpt] = r;
        }
        any_invalid = __builtin_amdgcn_ballot_w64(live && !q.valid) != 0;
    }
    if (A.vec) {
        const int64_t K3 = (int64_t)3 * A.K;
        for (int fr = 0; fr < nfr; ++fr) {
            const MsQuery q = qt[fr];
            const float *ra = A.vec + (int64_t)q.row0 * K3, *rc = A.vec + (int64_t)q.row1 * K3;
            float *o = A.vec_out + (f0 + fr) * K3;
            for (int64_t e0 = 0; e0 < K3; e0 += 64 * NW) {   // NW dword pairs per lane in flight (a lane past the row
                float va[NW], vc[NW];                         // re-reads element 0)
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int64_t e = e0 + 64 * w + lane;
                    va[w] = ra[e < K3 ? e : 0];
                    vc[w] = rc[e < K3 ? e : 0];
                }
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int64_t e = e0 + 64 * w + lane;
                    if (e < K3) o[e] = q.valid ? ms_blend(va[w], vc[w], q.b) : ms_nan();
                }
            }
        }
    }

    // 4. forward kinematics of the blended poses
    if (GLOBAL) {
        wave_sync();
        group_compose<F>(T, I.rot, I.pos, I.sch, nfr, I.utab, [&](int, Q lq, const GEnt &e, int) {
            if (STATE) lq = qmul_norm(Q{e.qx, e.qy, e.qz, e.qw}, lq, fk_tab(I.utab));   // skeleton3d.py:412-418
            return lq;
        });
        if (any_invalid) {   // wave-uniform: an invalid query's global rows are the quiet NaN too, whatever FK made of them
            for (int rec = lane; rec < nrec; rec += 64) {
                const Item it = item_split(rec, rJ, J);
                if (!qt[it.fr].valid) {
                    I.rot[rec] = nan4;
                    I.pos[3 * rec] = I.pos[3 * rec + 1] = I.pos[3 * rec + 2] = ms_nan();
                }
            }
            wave_sync();
        }
        group_store<F>(I.rot, I.pos, nrec, A.g_rot + f0 * J * 4, A.g_pos + f0 * J * 3);
    }
}

hipError_t launch_motion_sample(const TopoView &T, const MotionLibView &L, bool normalize, bool global, bool state,
                                const MotionSampleArgs &A, hipStream_t s)
{
    const int F = T.gF;
    const size_t lds = sizeof(float) * MsImages(nullptr, T.J, F, T.gsteps, global).floats;
    group_dispatch(F, [&](auto f, auto nm, auto gl, auto st) {
        hipLaunchKernelGGL((k_motion_sample<f(), nm(), gl(), st()>), dim3(grid_for(A.N, F)), dim3(64), lds, s, T, L, A);
    }, normalize, global, state && global);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The same for a library of JOINT-ANGLE clips (rtg_dof_motion_sample_f32): dof (F_total, J - 1), root_rot (F_total, 4),
// root_t (F_total, 3) on the same clip table -- what the pose fit returns.  Slerp between two rotations about one axis
// is the blend of the angle, so per query the launch reads two rows of J - 1 floats instead of J quaternions:
//   1. the query table as above, with dt = (float)(1 / (double)fps) per query;
//   2. the first F lanes take their query's root: qslerp (qnormalize when asked) of the rotation, ms_blend of the
//      translation, and with the velocities (t1 - t0) / dt and k_angular_raw's expression on the pair (r0, r1); the
//      translation and the velocity rows leave through small LDS images, lane = 3 query + component;
//   3. element i = 64 k + lane is (query, dof) by item_split: two dword gathers, ms_blend, (a1 - a0) / dt, whole-wave
//      stores; the blended angles stay in the lane's registers as k_dof_fk_group's loaded ones do;
//   4. with FK (g_rot / g_pos and / or key_pos) DofRotations, group_compose and group_store run as in
//      k_dof_fk_group on the launch's own roots, and key_pos is gathered from the image: g_pos[:, key] bit for bit.
// An invalid query's rows are the quiet NaN everywhere.  A one-joint model has no angles: dof* are not dereferenced.
struct DmImages {
    MsQuery *qt;     // [F] the query table
    float *dt;       // [F] the frame time of each query's clip
    float *rt;       // [F 3] the root translations out
    float *rv;       // [F 6] the root velocities out
    UnitEnt *utab;   // the near-unit table
    f4v *rot;        // FK: [F J] the local rotations, overwritten by the global ones
    float *pos;      // FK: [F J 3] the positions, the root's preset
    GEnt *sch;       // FK: [gsteps L] the schedule
    f4v *ntab;       // FK: [J] the per-joint {axis, lower, upper} table
    float *tw;       // VEL: [F J 6] the twists {v, w}
    size_t floats;
    __host__ __device__ DmImages(float *base, int J, int F, int steps, bool fk, bool vel = false)
    {
        LdsCarve c(base);
        qt = c.take<MsQuery>((size_t)F);
        dt = c.take<float>((size_t)F);
        rt = c.take<float>((size_t)3 * F);
        rv = c.take<float>((size_t)6 * F);
        utab = c.take_unit_tab();
        rot = c.take<f4v>(fk ? (size_t)F * J : 0);
        pos = c.take<float>(fk ? (size_t)3 * F * J : 0);
        sch = c.take<GEnt>(fk ? (size_t)steps * (64 / F) : 0);
        ntab = c.take<f4v>(fk ? J : 0);
        tw = c.take<float>(vel ? (size_t)6 * F * J : 0);
        floats = c.floats;
    }
};

template <int F, bool CLIP, bool FK>
__global__ __launch_bounds__(64, 4) void k_dof_motion_sample(TopoView T, DofView D, MotionLibView L, DofMotionArgs A)
{
    extern __shared__ __attribute__((aligned(16))) float ms_lds[];
    using G = Grp<F>;
    const int J = T.J, nd = J - 1, lane = (int)threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(A.N, f0), nrec = nfr * J, nang = nfr * nd;
    const DmImages I(ms_lds, J, F, T.gsteps, FK);
    const bool vel = A.root_vel_out != nullptr;   // launch-uniform (dof_vel_out goes with it)

    // 1. the query table
    if (lane < F) {
        const int64_t n = lane < nfr ? f0 + lane : 0;
        const int32_t clip = A.clip[n];
        const float time = A.time[n];
        const bool valid = motion_clip_valid(clip, L.C);
        const MotionClip ce = L.clips[valid ? clip : 0];
        const MotionIdx ix = motion_index(time, ce.fps, ce.len);
        I.qt[lane] = valid ? MsQuery{(int32_t)(ce.start + ix.i0), (int32_t)(ce.start + ix.i1), ix.b, 1}
                           : MsQuery{0, 0, 0.0f, 0};
        I.dt[lane] = (float)(1.0 / (double)ce.fps);
    }
    if (FK) {
        group_sched_fill(T, G::L, I.sch);
        joint_tab_fill<CLIP, false>(D, J, I.ntab);
    }
    if (kUnitTab) unit_tab_fill(I.utab, lane);
    wave_sync();

    // 2. the roots (a lane past the tile's queries holds query 0 and stores nothing)
    if (lane < F) {
        const MsQuery q = I.qt[lane];
        const float dt = I.dt[lane];
        const f4v *rr = reinterpret_cast<const f4v *>(A.root_rot);
        const Q r0 = q_of(rr[q.row0]), r1 = q_of(rr[q.row1]);
        const V t0 = ld3(A.root_t + (int64_t)q.row0 * 3), t1 = ld3(A.root_t + (int64_t)q.row1 * 3);
        Q r = qslerp(r0, r1, q.b);
        if (A.normalize) r = qnormalize(r, fk_tab(I.utab));
        float t[3] = {ms_blend(t0.x, t1.x, q.b), ms_blend(t0.y, t1.y, q.b), ms_blend(t0.z, t1.z, q.b)};
        float w[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (vel) {
            w[0] = (t1.x - t0.x) / dt;
            w[1] = (t1.y - t0.y) / dt;
            w[2] = (t1.z - t0.z) / dt;
            // skeleton3d.py:1137-1146 on the pair: k_angular_raw's expression (rtg_ops.hip)
            const Q aa = qangle_axis_abs(qmul_norm(r1, qconj(r0)));
            w[3] = (aa.y * aa.x) / dt;
            w[4] = (aa.z * aa.x) / dt;
            w[5] = (aa.w * aa.x) / dt;
        }
        f4v rv = v_of(r);
        if (!q.valid) {
            rv = f4v{ms_nan(), ms_nan(), ms_nan(), ms_nan()};
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = ms_nan();
#pragma unroll
            for (int c = 0; c < 6; ++c) w[c] = ms_nan();
        }
        if (lane < nfr) {
            reinterpret_cast<f4v *>(A.root_rot_out)[f0 + lane] = rv;
#pragma unroll
            for (int c = 0; c < 3; ++c) I.rt[3 * lane + c] = t[c];
#pragma unroll
            for (int c = 0; c < 6; ++c) I.rv[6 * lane + c] = w[c];
            if (FK) {
                I.rot[lane * J] = rv;
#pragma unroll
                for (int c = 0; c < 3; ++c) I.pos[3 * J * lane + c] = t[c];
            }
        }
    }
    const bool any_invalid = __builtin_amdgcn_ballot_w64(lane < nfr && !I.qt[lane < nfr ? lane : 0].valid) != 0;

    // 3. the angles: element i = (query, dof)
    ScalarRows<F> x;
    {
        const float rnd = item_rcp(nd > 0 ? nd : 1);
        float a0[G::NR], a1[G::NR];
#pragma unroll
        for (int k = 0; k < G::NR; ++k) {
            a0[k] = a1[k] = 0.0f;
            if (k * 64 >= nang) continue;   // wave-uniform: no lane has an angle in this piece
            const int i = k * 64 + lane;
            const Item it = item_split(i < nang ? i : 0, rnd, nd);   // a lane past the angles repeats angle 0
            const MsQuery q = I.qt[it.fr];
            a0[k] = A.dof[(int64_t)q.row0 * nd + it.j];
            a1[k] = A.dof[(int64_t)q.row1 * nd + it.j];
        }
#pragma unroll
        for (int k = 0; k < G::NR; ++k) {
            x.v[k] = 0.0f;
            if (k * 64 >= nang) continue;
            const int i = k * 64 + lane;
            const Item it = item_split(i < nang ? i : 0, rnd, nd);
            const MsQuery q = I.qt[it.fr];
            x.v[k] = ms_blend(a0[k], a1[k], q.b);   // (an invalid query's angles stay finite for the FK: its rows are
            if (i < nang) {                         // overwritten below)
                A.dof_out[f0 * nd + i] = q.valid ? x.v[k] : ms_nan();
                if (vel) A.dof_vel_out[f0 * nd + i] = q.valid ? (a1[k] - a0[k]) / I.dt[it.fr] : ms_nan();
            }
        }
    }

    // the root translations and velocities out, lane = 3 query + component
    wave_sync();
    if (lane < 3 * nfr) A.root_t_out[f0 * 3 + lane] = I.rt[lane];
    if (vel)
        for (int i = lane; i < 6 * nfr; i += 64) A.root_vel_out[f0 * 6 + i] = I.rv[i];

    // 4. forward kinematics of the blended angles on the launch's own roots
    if (FK) {
        const float rnd = item_rcp(nd > 0 ? nd : 1);
        const DofRotations<CLIP, F> rotations{x, I.ntab, I.utab, I.rot, J, nd, nang, lane, rnd};
        constexpr int NW = RTG_DOF_NWAY, NFULL = G::NR - G::NR % NW;
#pragma unroll
        for (int k = 0; k < NFULL; k += NW) rotations(std::integral_constant<int, NW>{}, k);
#pragma unroll
        for (int k = NFULL; k < G::NR; ++k) rotations(std::integral_constant<int, 1>{}, k);
        wave_sync();
        group_compose<F>(T, I.rot, I.pos, I.sch, nfr, I.utab, [&](int, Q lq, const GEnt &, int) { return lq; });
        if (any_invalid) {   // wave-uniform
            const float rJ = item_rcp(J);
            const f4v nan4{ms_nan(), ms_nan(), ms_nan(), ms_nan()};
            for (int rec = lane; rec < nrec; rec += 64) {
                const Item it = item_split(rec, rJ, J);
                if (!I.qt[it.fr].valid) {
                    I.rot[rec] = nan4;
                    I.pos[3 * rec] = I.pos[3 * rec + 1] = I.pos[3 * rec + 2] = ms_nan();
                }
            }
            wave_sync();
        }
        if (A.g_rot) group_store<F>(I.rot, I.pos, nrec, A.g_rot + f0 * J * 4, A.g_pos + f0 * J * 3);
        if (A.key_pos) {   // element e = (query, key link, component): consecutive floats of the output
            const int K3 = 3 * A.K, n = nfr * K3;
            float *o = A.key_pos + f0 * K3;
            for (int e = lane; e < n; e += 64) {
                const int fr = e / K3, r = e - fr * K3, k = r / 3;
                o[e] = I.pos[3 * (fr * J + (int)A.key[k]) + (r - 3 * k)];
            }
        }
    }
}

// rtg_dof_motion_sample_vel_f32: k_dof_motion_sample with the FK always on, a twist image [F J 6] behind the others and
// group_compose_vel's tangent sweep as step 4.  The rate of each joint is the launch's own dof_vel_out value, through
// the clip select on its dof_out value, stored into its joint's twist row in step 3; the root twist is root_vel_out's
// row (step 2); g_vel leaves as consecutive 16-byte pieces and key_vel is gathered from the image like key_pos.  A
// kernel of its own and not a template argument of k_dof_motion_sample: with the body shared (one tile function, both
// ways of passing the arguments tried) the device listings of the existing instantiations moved.
template <int F, bool CLIP>
__global__ __launch_bounds__(64, 4) void k_dof_motion_sample_vel(TopoView T, DofView D, MotionLibView L,
                                                              DofMotionVelArgs AV)
{
    extern __shared__ __attribute__((aligned(16))) float ms_lds[];
    const DofMotionArgs &A = AV.A;
    float *const g_vel = AV.g_vel, *const key_vel = AV.key_vel;
    using G = Grp<F>;
    const int J = T.J, nd = J - 1, lane = (int)threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * F;
    const int nfr = tile_frames<F>(A.N, f0), nrec = nfr * J, nang = nfr * nd;
    const DmImages I(ms_lds, J, F, T.gsteps, true, true);   // (dof_vel_out and root_vel_out are always given here)

    // 1. the query table
    if (lane < F) {
        const int64_t n = lane < nfr ? f0 + lane : 0;
        const int32_t clip = A.clip[n];
        const float time = A.time[n];
        const bool valid = motion_clip_valid(clip, L.C);
        const MotionClip ce = L.clips[valid ? clip : 0];
        const MotionIdx ix = motion_index(time, ce.fps, ce.len);
        I.qt[lane] = valid ? MsQuery{(int32_t)(ce.start + ix.i0), (int32_t)(ce.start + ix.i1), ix.b, 1}
                           : MsQuery{0, 0, 0.0f, 0};
        I.dt[lane] = (float)(1.0 / (double)ce.fps);
    }
    group_sched_fill(T, G::L, I.sch);
    joint_tab_fill<CLIP, false>(D, J, I.ntab);
    if (kUnitTab) unit_tab_fill(I.utab, lane);
    wave_sync();

    // 2. the roots (a lane past the tile's queries holds query 0 and stores nothing)
    if (lane < F) {
        const MsQuery q = I.qt[lane];
        const float dt = I.dt[lane];
        const f4v *rr = reinterpret_cast<const f4v *>(A.root_rot);
        const Q r0 = q_of(rr[q.row0]), r1 = q_of(rr[q.row1]);
        const V t0 = ld3(A.root_t + (int64_t)q.row0 * 3), t1 = ld3(A.root_t + (int64_t)q.row1 * 3);
        Q r = qslerp(r0, r1, q.b);
        if (A.normalize) r = qnormalize(r, fk_tab(I.utab));
        float t[3] = {ms_blend(t0.x, t1.x, q.b), ms_blend(t0.y, t1.y, q.b), ms_blend(t0.z, t1.z, q.b)};
        // skeleton3d.py:1137-1146 on the pair: k_angular_raw's expression (rtg_ops.hip)
        const Q aa = qangle_axis_abs(qmul_norm(r1, qconj(r0)));
        float w[6] = {(t1.x - t0.x) / dt, (t1.y - t0.y) / dt, (t1.z - t0.z) / dt,
                      (aa.y * aa.x) / dt, (aa.z * aa.x) / dt,  (aa.w * aa.x) / dt};
        f4v rv = v_of(r);
        if (!q.valid) {
            rv = f4v{ms_nan(), ms_nan(), ms_nan(), ms_nan()};
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = ms_nan();
#pragma unroll
            for (int c = 0; c < 6; ++c) w[c] = ms_nan();
        }
        if (lane < nfr) {
            reinterpret_cast<f4v *>(A.root_rot_out)[f0 + lane] = rv;
#pragma unroll
            for (int c = 0; c < 3; ++c) I.rt[3 * lane + c] = t[c];
#pragma unroll
            for (int c = 0; c < 6; ++c) I.rv[6 * lane + c] = I.tw[6 * J * lane + c] = w[c];   // the root twist
            I.rot[lane * J] = rv;
#pragma unroll
            for (int c = 0; c < 3; ++c) I.pos[3 * J * lane + c] = t[c];
        }
    }
    const bool any_invalid = __builtin_amdgcn_ballot_w64(lane < nfr && !I.qt[lane < nfr ? lane : 0].valid) != 0;

    // 3. the angles: element i = (query, dof)
    ScalarRows<F> x;
    {
        const float rnd = item_rcp(nd > 0 ? nd : 1);
        float a0[G::NR], a1[G::NR];
#pragma unroll
        for (int k = 0; k < G::NR; ++k) {
            a0[k] = a1[k] = 0.0f;
            if (k * 64 >= nang) continue;   // wave-uniform: no lane has an angle in this piece
            const int i = k * 64 + lane;
            const Item it = item_split(i < nang ? i : 0, rnd, nd);   // a lane past the angles repeats angle 0
            const MsQuery q = I.qt[it.fr];
            a0[k] = A.dof[(int64_t)q.row0 * nd + it.j];
            a1[k] = A.dof[(int64_t)q.row1 * nd + it.j];
        }
#pragma unroll
        for (int k = 0; k < G::NR; ++k) {
            x.v[k] = 0.0f;
            if (k * 64 >= nang) continue;
            const int i = k * 64 + lane;
            const Item it = item_split(i < nang ? i : 0, rnd, nd);
            const MsQuery q = I.qt[it.fr];
            x.v[k] = ms_blend(a0[k], a1[k], q.b);   // (an invalid query's angles stay finite for the FK: its rows are
            if (i < nang) {                         // overwritten below)
                A.dof_out[f0 * nd + i] = q.valid ? x.v[k] : ms_nan();
                const float xd = (a1[k] - a0[k]) / I.dt[it.fr];
                A.dof_vel_out[f0 * nd + i] = q.valid ? xd : ms_nan();
                // dof_vel_out's value through the clip select on dof_out's, into the joint's twist row
                I.tw[6 * (it.fr * J + it.j + 1)] = joint_rate<CLIP>(x.v[k], xd, I.ntab[it.j + 1]);
            }
        }
    }

    // the root translations and velocities out, lane = 3 query + component
    wave_sync();
    if (lane < 3 * nfr) A.root_t_out[f0 * 3 + lane] = I.rt[lane];
    for (int i = lane; i < 6 * nfr; i += 64) A.root_vel_out[f0 * 6 + i] = I.rv[i];

    // 4. forward kinematics and the tangent sweep of the blended angles on the launch's own roots
    {
        const float rnd = item_rcp(nd > 0 ? nd : 1);
        const DofRotations<CLIP, F> rotations{x, I.ntab, I.utab, I.rot, J, nd, nang, lane, rnd};
        constexpr int NW = RTG_DOF_NWAY, NFULL = G::NR - G::NR % NW;
#pragma unroll
        for (int k = 0; k < NFULL; k += NW) rotations(std::integral_constant<int, NW>{}, k);
#pragma unroll
        for (int k = NFULL; k < G::NR; ++k) rotations(std::integral_constant<int, 1>{}, k);
        wave_sync();
        group_compose_vel<F>(T, I.rot, I.pos, I.tw, I.sch, I.ntab, nfr, I.utab);
        if (any_invalid) {   // wave-uniform
            const float rJ = item_rcp(J);
            const f4v nan4{ms_nan(), ms_nan(), ms_nan(), ms_nan()};
            for (int rec = lane; rec < nrec; rec += 64) {
                const Item it = item_split(rec, rJ, J);
                if (!I.qt[it.fr].valid) {
                    I.rot[rec] = nan4;
                    I.pos[3 * rec] = I.pos[3 * rec + 1] = I.pos[3 * rec + 2] = ms_nan();
#pragma unroll
                    for (int c = 0; c < 6; ++c) I.tw[6 * rec + c] = ms_nan();
                }
            }
            wave_sync();
        }
        if (A.g_rot) group_store<F>(I.rot, I.pos, nrec, A.g_rot + f0 * J * 4, A.g_pos + f0 * J * 3);
        if (A.key_pos) {   // element e = (query, key link, component): consecutive floats of the output
            const int K3 = 3 * A.K, n = nfr * K3;
            float *o = A.key_pos + f0 * K3;
            for (int e = lane; e < n; e += 64) {
                const int fr = e / K3, r = e - fr * K3, k = r / 3;
                o[e] = I.pos[3 * (fr * J + (int)A.key[k]) + (r - 3 * k)];
            }
        }
        if (g_vel) PosRows<F>::out(I.tw, g_vel + f0 * J * 6, 6 * nrec);
        if (key_vel) {   // element e = (query, key link, component)
            const int K6 = 6 * A.K, n = nfr * K6;
            float *o = key_vel + f0 * K6;
            for (int e = lane; e < n; e += 64) {
                const int fr = e / K6, r = e - fr * K6, k = r / 6;
                o[e] = I.tw[6 * (fr * J + (int)A.key[k]) + (r - 6 * k)];
            }
        }
    }
}

hipError_t launch_dof_motion_sample(const TopoView &T, const DofView &D, const MotionLibView &L, bool clip,
                                    const DofMotionArgs &A, hipStream_t s)
{
    const int F = T.gF;
    const bool fk = A.g_rot != nullptr || A.key_pos != nullptr;
    const size_t lds = sizeof(float) * DmImages(nullptr, T.J, F, T.gsteps, fk).floats;
    group_dispatch(F, [&](auto f, auto cl, auto k) {
        hipLaunchKernelGGL((k_dof_motion_sample<f(), cl(), k()>), dim3(grid_for(A.N, F)), dim3(64), lds, s, T, D, L, A);
    }, clip && fk, fk);
    return hipGetLastError();
}

hipError_t launch_dof_motion_sample_vel(const TopoView &T, const DofView &D, const MotionLibView &L, bool clip,
                                        const DofMotionVelArgs &A, hipStream_t s)
{
    const int F = T.gF;
    const size_t lds = sizeof(float) * DmImages(nullptr, T.J, F, T.gsteps, true, true).floats;
    group_dispatch(F, [&](auto f, auto cl) {
        hipLaunchKernelGGL((k_dof_motion_sample_vel<f(), cl()>), dim3(grid_for(A.A.N, F)), dim3(64), lds, s, T, D, L, A);
    }, clip);
    return hipGetLastError();
}

}  // namespace rtg

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

}  // namespace rtg

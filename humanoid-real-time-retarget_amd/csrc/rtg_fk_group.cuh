// rtg_fk_group.cuh -- the lane-group tile kit shared by the forward kinematics kernels (rtg_fk.hip), their adjoints
// (rtg_fk_grad.hip), the keypoint fit (rtg_dof_fit.hip), retarget_to (rtg_retarget_to.hip) and the motion sampler
// (rtg_motion_sample.hip): a tile is one wave, F frames, 64 / F lanes per frame, rows moved as 1 KiB pieces through
// LDS images (the layout comment in rtg_fk.hip).  The parts: the LDS carve (LdsCarve: a kernel and its launcher call
// the same carve function), the row movers (LaneRows as GroupRows: float4 records, and ScalarRows: scalars; PosRows:
// position rows), the table fills, the root preset, the reverse sweep's child pull, the FK tile itself (FkImages,
// group_compose, group_store: rtg_fk.hip and rtg_motion_sample.hip; group_compose_vel, joint_rate: the same tile with a
// twist per link, the same two), the joint-angle model's rotations (joint_rot_n,
// DofRotations: the same two), the item split, the Q <-> f4v converters, the
// straight-through clamp and the launch dispatch.  The multi-wave tile of rtg_rot_ingest.hip takes only the
// converters and the item split.
#pragma once
#include "rtg_device.cuh"

#include <type_traits>

namespace rtg {

// A lane-group tile is one wave, so ordering its LDS traffic needs no block
// barrier: a wave's LDS instructions execute in issue order, and the
// wavefront-scope fence + wave_barrier only stop the compiler from moving
// memory operations across this point.  (__syncthreads would also make the
// compiler drain every outstanding global store, s_waitcnt vmcnt(0), per step.)
RTG_DEV void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

typedef float f4v __attribute__((ext_vector_type(4)));
RTG_DEV Q q_of(f4v v) { return Q{v.x, v.y, v.z, v.w}; }
RTG_DEV f4v v_of(Q q) { return f4v{q.x, q.y, q.z, q.w}; }
// the lane-group tiles' output pieces (whole 1 KiB wave stores): non-temporal (RTG_FK_NT_OUT): never read back here,
// they would only evict the rows still to be read from the L2
RTG_DEV void st_out(f4v *p, f4v v)
{
    if (RTG_FK_NT_OUT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

template <int F>
struct Grp {
    static_assert(F == 16 || F == 8, "lane groups of 4 or 8 lanes");
    static constexpr int L = 64 / F;             // lanes per frame
    static constexpr int LOG_L = F == 16 ? 2 : 3;
    static constexpr int NR = F == 16 ? 9 : 8;   // records per lane: F J <= 64 NR (group_frames)
    static constexpr int NP = (3 * NR + 3) / 4;  // float4 pieces per lane of a tile's position rows
};
// the frames of the tile that starts at frame f0 (the last tile of a batch is ragged)
template <int F>
RTG_DEV int tile_frames(int64_t B, int64_t f0) { return (int)((B - f0) < F ? (B - f0) : F); }

// the near-unit normalisation table (rtg_math.cuh) in the lane-group tiles' LDS, when any of them uses it
constexpr bool kUnitTab = RTG_FK_UNIT_TAB || RTG_DOF_UNIT_TAB;
constexpr size_t kUnitTabEnts = kUnitTab ? 2 * kUnitTabK + 1 : 0;
// the `tab` argument of the FK-side normalisations (qmul_norm, qnormalize): the table where RTG_FK_UNIT_TAB, else NoTab
RTG_DEV auto fk_tab(const UnitEnt *utab) { return TabSel<RTG_FK_UNIT_TAB != 0>::get(utab); }

// item i of a tile's (frame, joint) items, J per frame: i / J as ((i + 1/2) / J) truncated with rJ = item_rcp(J),
// exact for i < 2^12, J <= 64
RTG_DEV float item_rcp(int J) { return 1.0f / (float)J; }
struct Item {
    int fr, j;
};
RTG_DEV Item item_split(int i, float rJ, int J)
{
    const int fr = (int)(((float)i + 0.5f) * rJ);
    return Item{fr, i - fr * J};
}

// torch.clamp (min then max; NaN passes), then the straight-through sum (hu_forward_model.py:20-22)
RTG_DEV float clamp_st(float a, float lo, float hi)
{
    float c = a < lo ? lo : a;
    c = c > hi ? hi : c;
    return (c - a) + a;
}

// ---------------------------------------------------------------------------------------------------- the LDS carve
// A kernel's images are taken in order from its dynamic LDS, each starting 16-byte aligned.  One carve per kernel does
// it, the constructor of its *Images struct: the kernel calls it on the real base and uses the pointers, its launcher
// calls it on a null base and asks for `floats` of dynamic LDS.
__host__ __device__ inline size_t pad16f(size_t nfloats) { return (nfloats + 3) & ~(size_t)3; }
struct LdsCarve {
    float *base;
    size_t floats = 0;
    __host__ __device__ explicit LdsCarve(float *b) : base(b) {}
    template <typename T>
    __host__ __device__ T *take(size_t n)
    {
        static_assert(sizeof(T) % sizeof(float) == 0, "images of whole floats");
        T *p = base ? reinterpret_cast<T *>(base + floats) : nullptr;
        floats += pad16f(n * (sizeof(T) / sizeof(float)));
        return p;
    }
    __host__ __device__ UnitEnt *take_unit_tab() { return take<UnitEnt>(kUnitTabEnts); }
};

// ---------------------------------------------------------------------------------------------------- row movers
// f(k, i) for a lane's N items i = 64 k + lane: one 64-item piece per k, consecutive lanes on consecutive items
template <int N, typename Fn>
RTG_DEV void lane_items(const Fn &f)
{
#pragma unroll
    for (int k = 0; k < N; ++k) f(k, k * 64 + (int)threadIdx.x);
}
RTG_DEV void st_out(float *p, float v) { *p = v; }

// N items per lane of n consecutive Ts, global rows or an LDS image.  `load` is unconditional (a lane past the rows
// re-reads element 0), so no branch separates the loads and all are in flight; `store` into an LDS image comes after
// the caller's other loads; `out` writes output rows (st_out).  `copy_out` moves an image out item by item: for rows
// that leave long after the tile's loads, where the clamped indices of a second `load` would stay live in between.
template <typename T, int N>
struct LaneRows {
    T v[N];
    RTG_DEV void load(const void *rows, int n)
    {
        const T *s = static_cast<const T *>(rows);
        lane_items<N>([&](int k, int i) { v[k] = s[i < n ? i : 0]; });
    }
    RTG_DEV void store(T *img, int n) const
    {
        lane_items<N>([&](int k, int i) { if (i < n) img[i] = v[k]; });
    }
    RTG_DEV void out(void *rows, int n) const
    {
        T *d = static_cast<T *>(rows);
        lane_items<N>([&](int k, int i) { if (i < n) st_out(d + i, v[k]); });
    }
    RTG_DEV static void copy_out(const T *img, void *rows, int n)
    {
        T *d = static_cast<T *>(rows);
        lane_items<N>([&](int, int i) { if (i < n) st_out(d + i, img[i]); });
    }
};
template <int F>
using GroupRows = LaneRows<f4v, Grp<F>::NR>;    // the tile's float4 records
template <int F>
using ScalarRows = LaneRows<float, Grp<F>::NR>;   // the joint angles, the Adam moments, the gradient rows

// the tile's position rows (npos = 3 nrec floats): consecutive dwordx4 pieces and a dword tail when the rows are
// 16-byte aligned, dword by dword at any other alignment
template <int F>
struct PosRows {
    f4v v[Grp<F>::NP];
    float tail;
    bool aligned;
    RTG_DEV void load(const float *__restrict__ rows, int npos)
    {
        const int lane = (int)threadIdx.x, n4 = npos >> 2;
        aligned = (reinterpret_cast<uintptr_t>(rows) & 15u) == 0;
        tail = 0.0f;
        if (!aligned) return;   // to_lds copies dword by dword
        const f4v *src = reinterpret_cast<const f4v *>(rows);
        // (a lone one-joint frame has no whole piece to re-read)
        if (n4 > 0) lane_items<Grp<F>::NP>([&](int k, int i) { v[k] = src[i < n4 ? i : 0]; });
        if (4 * n4 + lane < npos) tail = rows[4 * n4 + lane];
    }
    RTG_DEV void to_lds(float *img, const float *__restrict__ rows, int npos) const
    {
        const int lane = (int)threadIdx.x, n4 = npos >> 2;
        if (aligned) {
            f4v *d = reinterpret_cast<f4v *>(img);
            lane_items<Grp<F>::NP>([&](int k, int i) { if (i < n4) d[i] = v[k]; });
            if (4 * n4 + lane < npos) img[4 * n4 + lane] = tail;
        } else {
            for (int i = lane; i < npos; i += 64) img[i] = rows[i];
        }
    }
    RTG_DEV static void out(const float *img, float *__restrict__ rows, int npos)   // the image out (st_out pieces)
    {
        const int lane = (int)threadIdx.x;
        if ((reinterpret_cast<uintptr_t>(rows) & 15u) == 0) {
            const int n4 = npos >> 2;
            f4v *pd = reinterpret_cast<f4v *>(rows);
            const f4v *ps = reinterpret_cast<const f4v *>(img);
            for (int i = lane; i < n4; i += 64) st_out(pd + i, ps[i]);
            for (int i = 4 * n4 + lane; i < npos; i += 64) rows[i] = img[i];
        } else {
            for (int i = lane; i < npos; i += 64) rows[i] = img[i];
        }
    }
};

// ---------------------------------------------------------------------------------------------------- fills
// the tile's schedule into LDS (float4 copies, in flight with the tile's own loads)
RTG_DEV void group_sched_fill(const TopoView &T, int L, GEnt *sch)
{
    const int n = T.gsteps * L * 2;
    const f4v *gs = reinterpret_cast<const f4v *>(T.gsched);
    f4v *d = reinterpret_cast<f4v *>(sch);
    for (int i = (int)threadIdx.x; i < n; i += 64) d[i] = gs[i];
}
// the same with the next-sibling table of the reverse sweep (child_pull), from the entries' codes
RTG_DEV void group_sched_fill(const TopoView &T, int L, GEnt *sch, int *nsib)
{
    const f4v *gs = reinterpret_cast<const f4v *>(T.gsched);
    f4v *d = reinterpret_cast<f4v *>(sch);
    for (int i = (int)threadIdx.x; i < T.gsteps * L; i += 64) {
        const f4v lo = gs[2 * i], hi = gs[2 * i + 1];   // {lx, ly, lz, code}, the tree quaternion
        d[2 * i] = lo;
        d[2 * i + 1] = hi;
        const int code = __float_as_int(lo.w), j = code & 0xFF;
        if (j != 0xFF) nsib[j] = (code >> 24) & 0xFF;
    }
}

// the joint-angle model's per-joint table {axis, lower, upper, weight}: joints 1 .. J - 1, and with WEIGHT the root's
// weight too (weight == nullptr: ones)
template <bool CLIP, bool WEIGHT>
RTG_DEV void joint_tab_fill(const DofView &D, int J, f4v *tab, const float *weight = nullptr)
{
    for (int j = (WEIGHT ? 0 : 1) + (int)threadIdx.x; j < J; j += 64) {
        const float w = !WEIGHT ? 0.0f : (weight ? ld_const(weight + j) : 1.0f);
        tab[j] = WEIGHT && j == 0
                     ? f4v{0.0f, 0.0f, 0.0f, w}
                     : f4v{__int_as_float(ld_const(D.axis + (j - 1))), CLIP ? ld_const(D.lower + (j - 1)) : 0.0f,
                           CLIP ? ld_const(D.upper + (j - 1)) : 0.0f, w};
    }
}

// the tile's roots.  Lane l loads frame l's root rotation and float l of the root translations (a lane past them
// re-reads element 0); root_preset puts them into the images' root rows: position = the root translation
// (kinematics.py:27-29), global = the root rotation as given (hu_forward_model.py:24)
RTG_DEV f4v root_rot_load(const float *__restrict__ root_rot, int64_t f0, int nfr)
{
    return reinterpret_cast<const f4v *>(root_rot)[f0 + ((int)threadIdx.x < nfr ? (int)threadIdx.x : 0)];
}
RTG_DEV float root_t_load(const float *__restrict__ root_t, int64_t f0, int nfr)
{
    return root_t[f0 * 3 + ((int)threadIdx.x < 3 * nfr ? (int)threadIdx.x : 0)];
}
RTG_DEV void root_preset(float *pos, int J, int nfr, float rt)
{
    const int lane = (int)threadIdx.x, fr = lane / 3;
    if (lane < 3 * nfr) pos[3 * J * fr + (lane - 3 * fr)] = rt;
}
RTG_DEV void root_preset(f4v *rot, float *pos, int J, int nfr, f4v rr, float rt)
{
    if ((int)threadIdx.x < nfr) rot[(int)threadIdx.x * J] = rr;
    root_preset(pos, J, nfr, rt);
}

// The reverse sweep's pull: joint j (rows at base + j) adds its children's rows in ascending index order (the first
// child from the entry's code, then the next-sibling table), so every sum has one fixed order whatever the
// schedule.  Returns a plus the children's rotation-adjoint rows of A; writes the summed position adjoint to P's row
// j and returns it in pb.
RTG_DEV f4v child_pull(f4v a, const f4v *A, float *P, int base, int j, int first_child, const int *nsib, V &pb)
{
    float *pj = P + 3 * (base + j);
    pb = V{pj[0], pj[1], pj[2]};
    for (int c = first_child; c != 0xFF; c = nsib[c]) {
        a += A[base + c];
        const float *pc = P + 3 * (base + c);
        pb.x += pc[0]; pb.y += pc[1]; pb.z += pc[2];
    }
    pj[0] = pb.x; pj[1] = pb.y; pj[2] = pb.z;
    return a;
}

// ---------------------------------------------------------------------------------------------------- joint angles
// qfrom_angle_unit_axis(angle, e_ax) for N joints, element by element the same values: qnormalize's sign flip f
// (on cos), its |q|^2 in any component order (the zero components add +0 exactly), (n, 1/n) from the table, the two
// nonzero components' products by 1/n, and the zero components keep the sign of f sin (0 sin, times f, times 1/n > 0).
// A |q|^2 outside the table (NaN / inf angles) or a subnormal product: the scalar path, one rare-case branch per group.
template <int N>
RTG_DEV void joint_rot_n(const float (&angle)[N], const int (&ax)[N], const UnitEnt *tab, Q (&out)[N])
{
    double th[N];
#pragma unroll
    for (int i = 0; i < N; ++i) th[i] = (double)(angle[i] / 2.0f);
    SC t[N];
    cr_sincos_n<N>(th, t);
    bool ok[N], all = true;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float f = 1.0f - 2.0f * (t[i].c < 0.0f ? 1.0f : 0.0f);
        const float s = f * t[i].s, c = f * t[i].c;
        const float n2 = s * s + c * c;
        uint32_t idx;
        const bool in = unit_tab_index(n2, idx);
        const double r = tab[idx].r;
        const double ps = (double)s * r, pc = (double)c * r;
        const float qs = (float)ps, z = __builtin_copysignf(0.0f, s);
        out[i] = Q{ax[i] == 0 ? qs : z, ax[i] == 1 ? qs : z, ax[i] == 2 ? qs : z, (float)pc};
        ok[i] = in & !((__builtin_fabs(ps) < 0x1p-126) & (ps != 0.0)) & !((__builtin_fabs(pc) < 0x1p-126) & (pc != 0.0));
        all &= ok[i];
    }
    if (__builtin_expect(!all, 0)) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (!ok[i])
                out[i] = qfrom_angle_unit_axis(angle[i], V{ax[i] == 0 ? 1.0f : 0.0f, ax[i] == 1 ? 1.0f : 0.0f,
                                                           ax[i] == 2 ? 1.0f : 0.0f});
    }
}
// The "rotations" stage of the joint-angle kernels (k_dof_fk_group, k_dof_motion_sample): the tile's angles a (angle
// i = 64 k + lane, nang of them, nd = J - 1 per frame) through the per-joint table ntab {axis, lower, upper} into the
// image's local rotations.  angle i = (frame fr, joint i mod nd + 1): its rotation into record fr J + j.
// operator(): NW loads' rotations at a time on the N-way leaf math (one rare-case branch per group, the same bits); a
// lane past the angles computes a dummy rotation (its j is still a joint) and does not store it.  The kernel calls it
// RTG_DOF_NWAY pieces at a time and one by one for the rest (as a closure in the kernel's own body: the device listing
// of k_dof_fk_group is then what it was with the stage written in place).
template <bool CLIP, int F>
struct DofRotations {
    const ScalarRows<F> &a;
    const f4v *const &ntab;
    const UnitEnt *const &utab;
    f4v *const &rot;
    const int &J, &nd, &nang, &lane;
    const float &rnd;   // item_rcp(nd > 0 ? nd : 1)
    template <typename NWay>
    RTG_DEV void operator()(NWay, int k0) const
    {
        constexpr int NW = NWay::value;
        if (k0 * 64 >= nang) return;   // wave-uniform: no lane has an angle in this group
        float x[NW];
        int axi[NW], rec[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int i = (k0 + w) * 64 + lane;
            const Item it = item_split(i, rnd, nd);
            const int fr = it.fr, j = it.j + 1;
            const f4v t = ntab[j];
            x[w] = CLIP ? clamp_st(a.v[k0 + w], t.y, t.z) : a.v[k0 + w];
            // the axis is an exact unit vector: quat_from_angle_axis's normalisation is the identity (round 5)
            axi[w] = __float_as_int(t.x);
            rec[w] = i < nang ? fr * J + j : -1;
        }
        Q q[NW];
#if RTG_DOF_UNIT_TAB
        joint_rot_n<NW>(x, axi, utab, q);
#else
        V axv[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w)
            axv[w] = V{axi[w] == 0 ? 1.0f : 0.0f, axi[w] == 1 ? 1.0f : 0.0f, axi[w] == 2 ? 1.0f : 0.0f};
        qfrom_angle_unit_axis_n<NW>(x, axv, q);
#endif
#pragma unroll
        for (int w = 0; w < NW; ++w)
            if (rec[w] >= 0) rot[rec[w]] = v_of(q[w]);
    }
};

// ---------------------------------------------------------------------------------------------------- the FK tile
// The FK tile's images; dof: the joint-angle model's per-joint {axis, lower, upper} table behind them
struct FkImages {
    f4v *rot;        // [F J] the local rotations, overwritten by the global ones
    float *pos;      // [F J 3] the positions, the root's preset
    GEnt *sch;       // [gsteps L] the schedule
    UnitEnt *utab;   // the near-unit table
    f4v *ntab;       // dof: [J]
    size_t floats;
    __host__ __device__ FkImages(float *base, int J, int F, int steps, bool dof)
    {
        LdsCarve c(base);
        rot = c.take<f4v>((size_t)F * J);
        pos = c.take<float>((size_t)3 * F * J);
        sch = c.take<GEnt>((size_t)steps * (64 / F));
        utab = c.take_unit_tab();
        ntab = c.take<f4v>(dof ? J : 0);
        floats = c.floats;
    }
};

// The schedule's steps over the tile image (rot: global rotations written over the local ones; pos: positions, the
// root's preset).  LQ(j, lq) gives joint j's local rotation from its image record (FK: the record itself, with the
// tree quaternion when STATE; DOF FK: built from the joint angle).
template <int F, typename LocalQ>
RTG_DEV void group_compose(const TopoView &T, f4v *rot, float *pos, const GEnt *sch, int nfr, const UnitEnt *utab,
                           const LocalQ &LQ)
{
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x;
    const int fr = lane >> G::LOG_L, sub = lane & (G::L - 1);
    const bool live = fr < nfr;
    const int base = fr * J;
    for (int s = 0; s < T.gsteps; ++s) {
        const GEnt e = sch[s * G::L + sub];
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF) {
            const f4v lv = rot[base + j];
            Q ng;
            V nt;
            if (j == 0) {   // root: global = local, unnormalised; position = the root translation (kinematics.py:27-29)
                ng = q_of(lv);
                nt = V{pos[3 * base], pos[3 * base + 1], pos[3 * base + 2]};
            } else {
                const Q lq = LQ(j, q_of(lv), e, fr);
                const Q g = q_of(rot[base + p]);
                const float *tp = pos + 3 * (base + p);
                const V t{tp[0], tp[1], tp[2]};
                const V rv = qrotate(g, V{e.lx, e.ly, e.lz});
                ng = qmul_norm(g, lq, fk_tab(utab));
                nt = V{rv.x + t.x, rv.y + t.y, rv.z + t.z};
            }
            rot[base + j] = v_of(ng);
            float *op = pos + 3 * (base + j);
            op[0] = nt.x; op[1] = nt.y; op[2] = nt.z;
        }
        wave_sync();   // this step's records before the next step's parent reads (other lanes)
    }
}

// The same steps for the joint-angle model with a twist per link (rtg_dof_fk_vel_f32, rtg_dof_motion_sample_vel_f32):
// the forward-mode counterpart of rtg_fk_grad.hip's reverse sweep.  tw: [F J 6] {v (3), w (3)}, world frame; the root's
// row preset to the root twist, row j >= 1 holding the joint's rate s in its first float until its step (the clip
// select already applied).  Joint j with parent p, every operation one rounding (the TUs that use this are built with
// -ffp-contract=off):
//   r = qrotate(G_p, l_j) -- the value FK adds to P_p;  c = w_p x r, each component (product) - (product);
//   v_j = v_p + c;  u = qrotate(G_j, e_j), G_j the joint's own global rotation;  w_j = w_p + (u * s).
// rot / pos get exactly group_compose's values (the same device functions on the same operands in the same order; the
// root's records are already in place, so its entry is passed over).  A function of its own: group_compose is shared
// by five TUs and stays what it compiles to.
template <int F>
RTG_DEV void group_compose_vel(const TopoView &T, f4v *rot, float *pos, float *tw, const GEnt *sch, const f4v *ntab,
                               int nfr, const UnitEnt *utab)
{
    using G = Grp<F>;
    const int J = T.J, lane = (int)threadIdx.x;
    const int fr = lane >> G::LOG_L, sub = lane & (G::L - 1);
    const bool live = fr < nfr;
    const int base = fr * J;
    for (int s = 0; s < T.gsteps; ++s) {
        const GEnt e = sch[s * G::L + sub];
        const int j = e.code & 0xFF, p = (e.code >> 8) & 0xFF;
        if (live && j != 0xFF && j != 0) {
            const Q lq = q_of(rot[base + j]);
            const Q g = q_of(rot[base + p]);
            const float *tp = pos + 3 * (base + p);
            const V t{tp[0], tp[1], tp[2]};
            const V rv = qrotate(g, V{e.lx, e.ly, e.lz});
            const Q ng = qmul_norm(g, lq, fk_tab(utab));
            const V nt = V{rv.x + t.x, rv.y + t.y, rv.z + t.z};
            const float *wp = tw + 6 * (base + p);
            float *wj = tw + 6 * (base + j);
            const V vp{wp[0], wp[1], wp[2]}, w{wp[3], wp[4], wp[5]};
            const float rate = wj[0];
            const int ax = __float_as_int(ntab[j].x);
            const V u = qrotate(ng, V{ax == 0 ? 1.0f : 0.0f, ax == 1 ? 1.0f : 0.0f, ax == 2 ? 1.0f : 0.0f});
            const V c{(w.y * rv.z) - (w.z * rv.y), (w.z * rv.x) - (w.x * rv.z), (w.x * rv.y) - (w.y * rv.x)};
            rot[base + j] = v_of(ng);
            float *op = pos + 3 * (base + j);
            op[0] = nt.x; op[1] = nt.y; op[2] = nt.z;
            wj[0] = vp.x + c.x; wj[1] = vp.y + c.y; wj[2] = vp.z + c.z;
            wj[3] = w.x + (u.x * rate); wj[4] = w.y + (u.y * rate); wj[5] = w.z + (u.z * rate);
        }
        wave_sync();   // this step's records before the next step's parent reads (other lanes)
    }
}
// a joint's rate as the sweep takes it: with CLIP a joint whose angle lies outside its limits does not turn (the twist
// is the derivative of the pose put out, not the optimiser's straight-through gradient); a NaN angle and an angle
// exactly at a limit keep the rate
template <bool CLIP>
RTG_DEV float joint_rate(float angle, float rate, f4v tab)
{
    return CLIP && (angle < tab.y || angle > tab.z) ? 0.0f : rate;
}

// the tile image out: rotations record-ordered, positions as consecutive pieces (PosRows)
template <int F>
RTG_DEV void group_store(const f4v *rot, const float *pos, int nrec, float *__restrict__ g_rot, float *__restrict__ g_pos)
{
    GroupRows<F> o;
    o.load(rot, nrec);
    o.out(g_rot, nrec);
    PosRows<F>::out(pos, g_pos, 3 * nrec);
}

// ---------------------------------------------------------------------------------------------------- launch dispatch
// run-time bools, and the run-time F, as compile-time arguments: fn(std::integral_constant<int, F>{},
// std::bool_constant<b0>{}, ...)
template <typename Fn>
inline void dispatch_bools(Fn &&fn) { fn(); }
template <typename Fn, typename... B>
inline void dispatch_bools(Fn &&fn, bool b, B... rest)
{
    if (b) dispatch_bools([&](auto... c) { fn(std::true_type{}, c...); }, rest...);
    else dispatch_bools([&](auto... c) { fn(std::false_type{}, c...); }, rest...);
}
template <typename Fn, typename... B>
inline void group_dispatch(int F, Fn &&fn, B... bools)
{
    if (F == 16) dispatch_bools([&](auto... c) { fn(std::integral_constant<int, 16>{}, c...); }, bools...);
    else dispatch_bools([&](auto... c) { fn(std::integral_constant<int, 8>{}, c...); }, bools...);
}

}  // namespace rtg

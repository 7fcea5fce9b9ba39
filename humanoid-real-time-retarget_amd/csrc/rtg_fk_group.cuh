// rtg_fk_group.cuh -- the lane-group helpers shared by the forward kinematics kernels (rtg_fk.hip) and their
// adjoints (rtg_fk_grad.hip): a tile is one wave, F frames, 64 / F lanes per frame, rows moved as 1 KiB pieces
// through an LDS image (see the layout comment in rtg_fk.hip).
#pragma once
#include "rtg_device.cuh"

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
};
// the near-unit normalisation table (rtg_math.cuh) in the lane-group tiles' LDS, when any of them uses it
constexpr bool kUnitTab = RTG_FK_UNIT_TAB || RTG_DOF_UNIT_TAB;
constexpr size_t kUnitTabFloats = kUnitTab ? 4 * (2 * kUnitTabK + 1) : 0;
RTG_DEV Q qmul_norm_tab(Q a, Q b, const UnitEnt *tab)
{
    if (!RTG_FK_UNIT_TAB) return qmul_norm(a, b);
    return qnormalize_t(qmul(a, b), tab);
}

__host__ __device__ inline size_t pad16f(size_t nfloats) { return (nfloats + 3) & ~(size_t)3; }

// the tile's schedule into LDS (float4 copies, in flight with the tile's own loads)
RTG_DEV void group_sched_fill(const TopoView &T, int L, GEnt *sch)
{
    const int n = T.gsteps * L * 2;
    const f4v *gs = reinterpret_cast<const f4v *>(T.gsched);
    f4v *d = reinterpret_cast<f4v *>(sch);
    for (int i = (int)threadIdx.x; i < n; i += 64) d[i] = gs[i];
}

// the tile's NR records per lane, all loads in flight (unconditional: a lane past the tile re-reads record 0, so no
// branch separates them), then -- after the caller's other loads -- into the LDS image
template <int F>
struct GroupRows {
    f4v v[Grp<F>::NR];
    RTG_DEV void load(const float *__restrict__ rows, int nrec)
    {
        const f4v *src = reinterpret_cast<const f4v *>(rows);
#pragma unroll
        for (int k = 0; k < Grp<F>::NR; ++k) {
            const int rec = k * 64 + (int)threadIdx.x;
            v[k] = src[rec < nrec ? rec : 0];
        }
    }
    RTG_DEV void to_lds(f4v *rot, int nrec) const
    {
#pragma unroll
        for (int k = 0; k < Grp<F>::NR; ++k) {
            const int rec = k * 64 + (int)threadIdx.x;
            if (rec < nrec) rot[rec] = v[k];
        }
    }
};

}  // namespace rtg

// rtg_api.cpp -- C ABI (include/rtg.h) over the gfx950 kernels.
//
// Host-side only: argument validation (mirroring the reference's assertions),
// handle lifetime, and stream-ordered launches.  Launch entry points never
// allocate, copy or synchronise, so callers may capture them into hipGraphs.
//
// Device resources live in the owner types below (DevBuf, PinnedWord, Event): a handle struct holds owners, so a
// constructor that fails part-way just returns and `delete handle` is the whole destructor.  Argument checks whose
// text agrees up to the function's name are written once (check_tree, check_layout, check_overlap, parse_seq, ...).
// Every message here is pinned by tests/api_message_cases.py: a new entry point adds its cases there
// (rtg_dof_motion_sample_f32's are written out in tests/test_dof_motion_host.py and tests/test_gpu_dof_motion.py).
#include <immintrin.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>
#include <string>
#include <utility>

#include "rtg_kernels.cuh"

using namespace rtg;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int hip_check(hipError_t e, const char *what)
{
    if (e == hipSuccess) return RTG_OK;
    return fail(e == hipErrorOutOfMemory ? RTG_ERR_OUT_OF_MEMORY : RTG_ERR_DEVICE, "%s: %s", what,
                hipGetErrorString(e));
}

// a HIP call, or anything else that returns an rtg_status: leave with it unless it is RTG_OK
#define RTG_TRY(expr, what) RTG_CHECK(hip_check((expr), (what)))
#define RTG_CHECK(expr)                              \
    do {                                             \
        int rc_ = (expr);                            \
        if (rc_ != RTG_OK) return rc_;               \
    } while (0)

// ---------------------------------------------------------------- owners
// What a handle (or a constructor that may still fail) holds of the device: released with its owner, move-only.
struct DevFree { void operator()(void *p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void *p) const { (void)hipHostFree(p); } };
struct EventFree { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };

// Device memory (hipMalloc) of n elements of T.
template <class T>
struct DevBuf {
    std::unique_ptr<T, DevFree> p;
    T *get() const { return p.get(); }
    int alloc(size_t n, const char *what)
    {
        T *raw = nullptr;
        RTG_TRY(hipMalloc(&raw, sizeof(T) * n), what);
        p.reset(raw);
        return RTG_OK;
    }
    int upload(const T *src, size_t n, const char *what = "hipMemcpy")
    {
        return hip_check(hipMemcpy(p.get(), src, sizeof(T) * n, hipMemcpyHostToDevice), what);
    }
    int alloc_upload(const T *src, size_t n, const char *what)
    {
        RTG_CHECK(alloc(n, what));
        return upload(src, n);
    }
};

// One zeroed word of host-mapped pinned memory (a solver's device error word).
struct PinnedWord {
    std::unique_ptr<uint32_t, PinnedFree> p;
    uint32_t *get() const { return p.get(); }
    int alloc(const char *what)
    {
        void *raw = nullptr;
        RTG_TRY(hipHostMalloc(&raw, sizeof(uint32_t), hipHostMallocMapped), what);
        p.reset(static_cast<uint32_t *>(raw));
        *p = 0;
        return RTG_OK;
    }
};

struct Event {
    std::unique_ptr<std::remove_pointer<hipEvent_t>::type, EventFree> e;
    hipEvent_t get() const { return e.get(); }
    int create()
    {
        hipEvent_t raw = nullptr;
        RTG_TRY(hipEventCreate(&raw), "hipEventCreate");
        e.reset(raw);
        return RTG_OK;
    }
};

}  // namespace

struct rtg_topology_s {
    int32_t J = 0;
    DevBuf<int32_t> parents;
    DevBuf<V> local_t;
    DevBuf<Q> tree_quat;
    DevBuf<GEnt> gsched;   // lane-group FK schedule (J <= kGroupMaxJ), see fk_group_schedule
    int32_t gF = 0, gsteps = 0;
    std::vector<int32_t> h_parents;   // host copies, for the plans built over this tree (rtg_retarget_plan_create)
    std::vector<Q> h_tree_quat;
    std::vector<V> h_local_t;
    TopoView view() const
    {
        return TopoView{parents.get(), local_t.get(), tree_quat.get(), J, gsched.get(), gF, gsteps};
    }
};

// HuForwardModel: the topology is borrowed (it must outlive the model); axis / limits are owned.
struct rtg_dof_model_s {
    rtg_topology_t topo = nullptr;
    DevBuf<int32_t> axis;
    DevBuf<float> lower, upper;
    bool has_limits = false;
    DofView view() const { return DofView{axis.get(), lower.get(), upper.get()}; }
};

// SkeletonState.retarget_to: the view (layout, R, scale, roots) and the device blob it points into.
struct rtg_retarget_plan_s {
    RetargetView view{};
    DevBuf<float> blob;
};

// Keypoint targets for the pose fit: the view (layout, constants) and the device blob it points into.
struct rtg_fit_targets_plan_s {
    FitTargetsView view{};
    DevBuf<float> blob;
};

// The zero-pose transform of mocap rotations: the view and the device blob it points into.
struct rtg_rot_ingest_s {
    RotIngestView view{};
    DevBuf<float> blob;
};

// A motion library's clip table on the device; F_total bounds the caller's arrays (the overlap checks).
struct rtg_motion_lib_s {
    DevBuf<MotionClip> clips;
    int32_t C = 0;
    int64_t F_total = 0;
};

struct rtg_solver_s {
    int kind = 0;
    int precise = 0;
    SolverConsts consts{};
    DevBuf<uint32_t> ang_tab;   // exp-map angle table (consts.ang_tab), device of creation
    PinnedWord err;             // the device error word (consts.err is its device alias)
};

namespace {

inline hipStream_t as_stream(rtg_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline V v3(const float *p, int j) { return V{p[3 * j], p[3 * j + 1], p[3 * j + 2]}; }

// ---------------------------------------------------------------- shared checks (the text agrees up to fn)
// parent-indexed tree in topological order (skeleton3d.py:87-88 asserts equal lengths; the FK loop kinematics.py:27
// requires parents before children)
int check_tree(const char *fn, const int32_t *parents, int J)
{
    if (J >= 1 && parents[0] != -1) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: joint 0 must be the root", fn);
    for (int j = 1; j < J; ++j)
        if (parents[j] < 0 || parents[j] >= j)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: parents[%d]=%d is not < %d", fn, j, parents[j], j);
    return RTG_OK;
}

int check_layout(const char *fn, int layout)
{
    if (layout != RTG_LAYOUT_AOS && layout != RTG_LAYOUT_SOA)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: bad layout %d", fn, layout);
    return RTG_OK;
}

// No span of a[] may share a byte with a span of b[] or with a later span of a[]; NULL spans are skipped.
struct Span {
    const void *p;
    uint64_t bytes;
    const char *name;
};
int check_overlap(const char *fn, const Span *a, size_t na, const Span *b, size_t nb)
{
    auto hit = [](const Span &x, const Span &y) {
        const uintptr_t px = reinterpret_cast<uintptr_t>(x.p), py = reinterpret_cast<uintptr_t>(y.p);
        return x.p && y.p && px < py + y.bytes && py < px + x.bytes;
    };
    for (size_t i = 0; i < na; ++i) {
        for (size_t k = 0; k < nb; ++k)
            if (hit(a[i], b[k])) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: %s and %s overlap", fn, a[i].name, b[k].name);
        for (size_t k = i + 1; k < na; ++k)
            if (hit(a[i], a[k])) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: %s and %s overlap", fn, a[i].name, a[k].name);
    }
    return RTG_OK;
}

int axis_of(char c, int *ax, int *lower)
{
    switch (c) {
    case 'x': *ax = 0; *lower = 1; return 1;
    case 'y': *ax = 1; *lower = 1; return 1;
    case 'z': *ax = 2; *lower = 1; return 1;
    case 'X': *ax = 0; *lower = 0; return 1;
    case 'Y': *ax = 1; *lower = 0; return 1;
    case 'Z': *ax = 2; *lower = 0; return 1;
    default: return 0;
    }
}

// scipy's Euler sequence: 3 chars of xyz (extrinsic) or XYZ (intrinsic), consecutive axes different
int parse_seq(const char *fn, const char *seq, int ax[3], int *extrinsic)
{
    if (!seq || std::strlen(seq) != 3) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: seq must have 3 axes", fn);
    int lower[3];
    for (int i = 0; i < 3; ++i)
        if (!axis_of(seq[i], &ax[i], &lower[i])) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: bad axis '%c'", fn, seq[i]);
    if (lower[0] != lower[1] || lower[1] != lower[2])
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: mixed intrinsic/extrinsic seq '%s'", fn, seq);
    if (ax[0] == ax[1] || ax[1] == ax[2])
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: consecutive axes must differ ('%s')", fn, seq);
    *extrinsic = lower[0];
    return RTG_OK;
}

int check_fk(rtg_topology_t t, const void *a, const void *b, const void *c, const void *d, int64_t B, const char *fn)
{
    if (!t) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL topology", fn);
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: negative batch %lld", fn, (long long)B);
    if (B > 0 && (!a || !b || !c || !d)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    return RTG_OK;
}

int run_fk(const char *fn, bool state, rtg_topology_t t, const float *local_rot, const float *root_t, int64_t B,
           float *g_rot, float *g_pos, rtg_stream_t stream)
{
    int rc = check_fk(t, local_rot, root_t, g_rot, g_pos, B, fn);
    if (rc != RTG_OK || B == 0) return rc;
    RTG_TRY(launch_fk(t->view(), state, local_rot, root_t, B, g_rot, g_pos, as_stream(stream)),
            state ? "k_fk<state>" : "k_fk");
    return RTG_OK;
}

int run_local_rotation(const char *fn, bool state, rtg_topology_t t, const float *g_rot, int64_t B, float *local_rot,
                       rtg_stream_t stream)
{
    int rc = check_fk(t, g_rot, local_rot, g_rot, local_rot, B, fn);
    if (rc != RTG_OK || B == 0) return rc;
    RTG_TRY(launch_local_rotation(t->view(), state, g_rot, B, local_rot, as_stream(stream)),
            state ? "k_local_rotation<state>" : "k_local_rotation");
    return RTG_OK;
}

// the FK segments of a mixed launch, checked, into dst[0..n)
int fill_fk_segments(const char *fn, const rtg_fk_segment *segs, int n, FkSeg *dst)
{
    for (int i = 0; i < n; ++i) {
        const rtg_fk_segment &s = segs[i];
        RTG_CHECK(check_fk(s.topo, s.local_rot, s.root_t, s.g_rot, s.g_pos, s.B, fn));
        dst[i] = FkSeg{s.topo->view(), s.local_rot, s.root_t, s.g_rot, s.g_pos, s.B, 0};
    }
    return RTG_OK;
}

// the argument checks both backward entry points share (everything that needs no handle first)
int check_fk_backward(const char *fn, int64_t B, const void *grad_g_rot, const void *grad_g_pos, bool any_out)
{
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: B=%lld < 0", fn, (long long)B);
    if (B == 0) return RTG_OK;   // empty buffers have no address to give
    if (!grad_g_rot && !grad_g_pos)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: both upstream gradients are NULL", fn);
    if (!any_out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: every output is NULL", fn);
    return RTG_OK;
}

// rtg_dof_fit_apart_f32's host struct, checked as far as no handle is needed, into the launch's arguments; `on`: the
// term is there (a sphere, and a pair or a plane with mask bits)
int fill_fit_apart(const char *fn, const rtg_fit_apart &a, DofFitApartArgs &Z, bool &on)
{
    if (a.S < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: S=%d < 0", fn, a.S);
    if (a.Pn < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: Pn=%d < 0", fn, a.Pn);
    if (a.S > RTG_FIT_MAX_SPHERES)
        return fail(RTG_ERR_UNSUPPORTED, "%s: S=%d spheres, at most %d", fn, a.S, RTG_FIT_MAX_SPHERES);
    if (a.Pn > RTG_FIT_MAX_PAIRS)
        return fail(RTG_ERR_UNSUPPORTED, "%s: Pn=%d pairs, at most %d", fn, a.Pn, RTG_FIT_MAX_PAIRS);
    if (a.S > 0 && (!a.sphere_link || !a.sphere))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: S=%d with sphere_link or sphere NULL", fn, a.S);
    if (a.Pn > 0 && !a.pair) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: Pn=%d with pair NULL", fn, a.Pn);
    if (!std::isfinite(a.margin)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: margin=%g must be finite", fn, (double)a.margin);
    Z.S = a.S;
    Z.Pn = a.Pn;
    Z.margin = a.margin;
    for (int s = 0; s < a.S; ++s) {
        const float *row = a.sphere + 4 * s;
        if (!std::isfinite(row[0]) || !std::isfinite(row[1]) || !std::isfinite(row[2]) || !std::isfinite(row[3]))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: sphere[%d] is not finite", fn, s);
        if (row[3] < 0.0f)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: sphere[%d] has the negative radius %g", fn, s, (double)row[3]);
        if (a.sphere_link[s] < 0)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: sphere_link[%d]=%d < 0", fn, s, a.sphere_link[s]);
        Z.link[s] = a.sphere_link[s];
        for (int c = 0; c < 4; ++c) Z.sphere[s][c] = row[c];
    }
    for (int p = 0; p < a.Pn; ++p) {
        const int32_t i = a.pair[2 * p], k = a.pair[2 * p + 1];
        if (i < 0 || i >= a.S || k < 0 || k >= a.S)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: pair[%d]=(%d, %d) is outside 0..%d", fn, p, i, k, a.S - 1);
        if (i == k) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: pair[%d] joins sphere %d with itself", fn, p, i);
        const float w = a.pair_weight ? a.pair_weight[p] : 1.0f;
        if (!std::isfinite(w) || w < 0.0f)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: pair_weight[%d]=%g must be finite and not negative", fn, p, (double)w);
        Z.pair[p] = i | (k << 8);
        Z.pair_weight[p] = w;
    }
    if (a.plane) {   // without one the mask and the weight are not looked at
        const float *n = a.plane;
        if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]) || !std::isfinite(n[3]))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: plane is not finite", fn);
        const double len = std::sqrt((double)n[0] * n[0] + (double)n[1] * n[1] + (double)n[2] * n[2]);
        if (!(len > 0.0)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: plane normal has zero length", fn);
        if (!std::isfinite(a.floor_weight) || a.floor_weight < 0.0f)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: floor_weight=%g must be finite and not negative", fn,
                        (double)a.floor_weight);
        if (a.S < 32 && (a.floor_mask >> a.S) != 0u)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: floor_mask=0x%x has bits at or above S=%d", fn, a.floor_mask, a.S);
        for (int c = 0; c < 3; ++c) Z.plane[c] = (float)(n[c] / len);
        Z.plane[3] = n[3];
        Z.floor_mask = a.floor_mask;
        Z.floor_weight = a.floor_weight;
    }
    on = a.S > 0 && (a.Pn > 0 || Z.floor_mask != 0u);
    return RTG_OK;
}

// rtg_dof_fit_f32 (R == nullptr), rtg_dof_fit_root_f32 (R: the root block), rtg_dof_fit_orient_f32 (O too: the
// orientation block, rot_joint its K host-side joint indices), rtg_dof_fit_prior_f32 (H too: the posture prior and
// the projection), rtg_dof_fit_apart_f32 (apart too: the keep-apart spheres and the floor) and rtg_dof_fit_robust_f32
// (U too: the frame weights and the robust scale, inv_d2 filled here): one checked path, eleven kernels
int run_dof_fit(const char *fn, rtg_dof_model_t m, int clip, DofFitArgs A, const DofFitRootArgs *R, rtg_stream_t stream,
                DofFitOriArgs *O = nullptr, const int32_t *rot_joint = nullptr, const DofFitPriorArgs *H = nullptr,
                const rtg_fit_apart *apart = nullptr, DofFitRobustArgs *U = nullptr)
{
    // everything that needs no handle first
    if (A.B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: B=%lld < 0", fn, (long long)A.B);
    if (R && (R->fit_root & ~(RTG_FIT_ROOT_T | RTG_FIT_ROOT_ROT)))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: fit_root=%d has unknown bits", fn, R->fit_root);
    if (A.iters < 0 || A.iters > RTG_DOF_FIT_MAX_ITERS)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: iters=%d is outside 0..%d", fn, A.iters, RTG_DOF_FIT_MAX_ITERS);
    if (A.step0 < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: step0=%d < 0", fn, A.step0);
    if (!std::isfinite(A.lr) || !std::isfinite(A.eps))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: lr=%g, eps=%g must be finite", fn, (double)A.lr, (double)A.eps);
    if (R && (!std::isfinite(R->lr_t) || !std::isfinite(R->lr_rot) || R->lr_t < 0.0f || R->lr_rot < 0.0f))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: lr_root_t=%g, lr_root_rot=%g must be finite and not negative", fn,
                    (double)R->lr_t, (double)R->lr_rot);
    if (!std::isfinite(A.beta1) || !std::isfinite(A.beta2) || A.beta1 < 0.0f || A.beta1 >= 1.0f || A.beta2 < 0.0f ||
        A.beta2 >= 1.0f)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: betas (%g, %g) must lie in [0, 1)", fn, (double)A.beta1, (double)A.beta2);
    if ((A.m == nullptr) != (A.v == nullptr))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both Adam moment buffers (m, v) or neither", fn);
    if (R && (R->state == nullptr) != (A.m == nullptr))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give root_state with the Adam moment buffers (m, v), or none of them", fn);
    const bool root_out = R && (R->rot_out || R->t_out || R->grad);
    if (A.B > 0) {   // empty buffers have no address to give
        if (!A.dof_out && !A.loss && !A.grad && !root_out)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: every output is NULL", fn);
        if (!A.target_pos || !A.root_rot || !A.root_t) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    }
    if (O) {
        if (O->K < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: K=%d < 0", fn, O->K);
        if (O->K > RTG_FIT_MAX_ROT_LINKS)
            return fail(RTG_ERR_UNSUPPORTED, "%s: K=%d oriented links, at most %d", fn, O->K, RTG_FIT_MAX_ROT_LINKS);
        if (O->K > 0 && (!rot_joint || (A.B > 0 && !O->target_rot)))   // empty buffers have no address to give
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: K=%d with rot_joint or target_rot NULL", fn, O->K);
        if (O->K > 0 && (reinterpret_cast<uintptr_t>(O->target_rot) & 15u))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: target_rot is not 16-byte aligned", fn);
        for (int k = 0; k < O->K; ++k) {
            if (rot_joint[k] < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: rot_joint[%d]=%d < 0", fn, k, rot_joint[k]);
            for (int i = 0; i < k; ++i)
                if (rot_joint[i] == rot_joint[k])
                    return fail(RTG_ERR_INVALID_ARGUMENT, "%s: joint %d is listed twice (rot_joint[%d] and [%d])", fn,
                                rot_joint[k], i, k);
            O->joint[k] = rot_joint[k];
        }
        if (O->K == 0) O->target_rot = O->rot_weight = nullptr;   // not looked at
    }
    if (H) {
        if (H->flags & ~RTG_FIT_PROJECT) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: flags=%d has unknown bits", fn, H->flags);
        if (H->prior_weight && !H->prior)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: prior_weight given without prior", fn);
        if (!H->prior && !H->flags) H = nullptr;   // neither term nor projection: rtg_dof_fit_orient_f32 itself
    }
    if (U) {
        if (!std::isfinite(U->robust_scale) || U->robust_scale < 0.0f)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: robust_scale=%g must be finite and not negative", fn,
                        (double)U->robust_scale);
        U->inv_d2 = U->robust_scale > 0.0f ? (float)(1.0 / ((double)U->robust_scale * (double)U->robust_scale)) : 0.0f;
        if (!U->frame_weight && U->robust_scale == 0.0f) U = nullptr;   // neither: rtg_dof_fit_apart_f32 itself
    }
    DofFitApartArgs Z{};
    bool keep_apart = false;   // no sphere, or neither a pair nor a floor: rtg_dof_fit_prior_f32 itself
    if (apart) RTG_CHECK(fill_fit_apart(fn, *apart, Z, keep_apart));
    if (!m) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL model", fn);
    if (clip && !m->has_limits)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: clip_angles requested but the model has no DOF limits", fn);
    if (H && (H->flags & RTG_FIT_PROJECT) && !m->has_limits)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: RTG_FIT_PROJECT requested but the model has no DOF limits", fn);
    const int J = m->topo->J;
    if (J > kGroupMaxJ)
        return fail(RTG_ERR_UNSUPPORTED, "%s: serves models of 1..%d joints (this one has %d)", fn, kGroupMaxJ, J);
    for (int k = 0; O && k < O->K; ++k)
        if (O->joint[k] >= J)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: rot_joint[%d]=%d is outside 0..%d", fn, k, O->joint[k], J - 1);
    for (int s = 0; s < Z.S; ++s)
        if (Z.link[s] >= J)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: sphere_link[%d]=%d is outside 0..%d", fn, s, Z.link[s], J - 1);
    if (A.B == 0) return RTG_OK;
    if (J > 1 && !A.dof_in) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    if (J == 1) {   // no angles: only a fitted root can step; the kernel's unconditional first-element loads get readable memory
        A.dof_in = A.root_rot;
        A.m = A.v = A.dof_out = A.grad = nullptr;
        if (!R || !R->fit_root) A.iters = 0;
        if (!A.loss && !root_out) return RTG_OK;
        H = nullptr;   // no angles: nothing to hold or to project, and neither pointer is dereferenced
    }
    if (U)   // always the prior family's tiles, with no prior where none is given
        RTG_TRY(launch_dof_fit_robust(m->topo->view(), m->view(), clip != 0, A, *R, *O, H ? *H : DofFitPriorArgs{}, Z,
                                      keep_apart, *U, as_stream(stream)),
                keep_apart ? (O->K > 0 ? "k_dof_fit_orient_apart_robust" : "k_dof_fit_apart_robust")
                           : (O->K > 0 ? "k_dof_fit_orient_robust" : "k_dof_fit_robust"));
    else if (keep_apart)
        RTG_TRY(launch_dof_fit_apart(m->topo->view(), m->view(), clip != 0, A, *R, *O, H ? *H : DofFitPriorArgs{}, Z,
                                     as_stream(stream)),
                O->K > 0 ? "k_dof_fit_orient_apart" : "k_dof_fit_apart");
    else if (H)
        RTG_TRY(launch_dof_fit_prior(m->topo->view(), m->view(), clip != 0, A, *R, *O, *H, as_stream(stream)),
                O->K > 0 ? "k_dof_fit_orient_prior" : "k_dof_fit_prior");
    else if (O && O->K > 0)   // K == 0 is the pose fit itself: its kernel measured 250 us per iteration against 313 through the oriented one
        RTG_TRY(launch_dof_fit_orient(m->topo->view(), m->view(), clip != 0, A, *R, *O, as_stream(stream)),
                "k_dof_fit_orient");
    else if (R)
        RTG_TRY(launch_dof_fit_root(m->topo->view(), m->view(), clip != 0, A, *R, as_stream(stream)), "k_dof_fit_root");
    else
        RTG_TRY(launch_dof_fit(m->topo->view(), m->view(), clip != 0, A, as_stream(stream)), "k_dof_fit");
    return RTG_OK;
}

// what a mapping that retarget_tables refuses returns: more than kGroupMaxJ joints is a limit of ours, the rest the caller's
int fail_tables(const char *fn, int Js, int Jt, const std::string &err)
{
    return fail(Js > kGroupMaxJ || Jt > kGroupMaxJ ? RTG_ERR_UNSUPPORTED : RTG_ERR_INVALID_ARGUMENT, "%s: %s", fn, err.c_str());
}

int make_taps(const double *w, int32_t radius, GaussTaps *taps, const char *fn)
{
    if (!w) return RTG_OK;
    if (radius < 0 || radius > RTG_MAX_FILTER_RADIUS)
        return fail(RTG_ERR_UNSUPPORTED, "%s: filter radius %d (max %d)", fn, radius, RTG_MAX_FILTER_RADIUS);
    taps->radius = radius;
    for (int i = 0; i < 2 * radius + 1; ++i) taps->w[i] = w[i];
    return RTG_OK;
}

// A device error a previous launch of this solver reported (rtg.h RTG_DEVERR_*): returned once, then cleared.
int take_device_error(uint32_t *word, const char *fn)
{
    const uint32_t e = word ? __atomic_exchange_n(word, 0u, __ATOMIC_ACQ_REL) : 0u;
    if (e == 0) return RTG_OK;
    return fail(RTG_ERR_DEVICE, "%s: a previous launch reported device error 0x%x%s", fn, e,
                (e & RTG_DEVERR_HANDOVER_TIMEOUT) ? " (a wave hand-over timed out: that launch's outputs are not valid)"
                                                  : "");
}

}  // namespace

extern "C" {

int rtg_abi_version(void) { return RTG_ABI_VERSION; }

const char *rtg_last_error(void) { return g_err.c_str(); }

int rtg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------- topology
int rtg_topology_create(const int32_t *parents, const float *local_t, const float *tree_quat, int32_t J,
                        rtg_topology_t *out)
{
    const char *fn = "rtg_topology_create";
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    *out = nullptr;
    if (!parents || !local_t) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL parents/local_t", fn);
    if (J < 1 || J > 1024) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: J=%d out of range", fn, J);
    RTG_CHECK(check_tree(fn, parents, J));
    std::unique_ptr<rtg_topology_s> t(new (std::nothrow) rtg_topology_s());
    if (!t) return fail(RTG_ERR_OUT_OF_MEMORY, "%s: host allocation failed", fn);
    t->J = J;
    t->h_parents.assign(parents, parents + J);
    std::vector<Q> &tq = t->h_tree_quat;
    tq.resize(J);
    for (int j = 0; j < J; ++j)
        tq[j] = tree_quat ? Q{tree_quat[4 * j], tree_quat[4 * j + 1], tree_quat[4 * j + 2], tree_quat[4 * j + 3]}
                          : Q{0.f, 0.f, 0.f, 1.f};
    std::vector<V> &lt = t->h_local_t;
    lt.resize(J);
    for (int j = 0; j < J; ++j) lt[j] = v3(local_t, j);
    RTG_CHECK(t->parents.alloc(J, "hipMalloc(parents)"));
    RTG_CHECK(t->local_t.alloc(J, "hipMalloc(local_t)"));
    RTG_CHECK(t->tree_quat.alloc(J, "hipMalloc(tree_quat)"));
    RTG_CHECK(t->parents.upload(parents, J));
    RTG_CHECK(t->local_t.upload(lt.data(), J));
    RTG_CHECK(t->tree_quat.upload(tq.data(), J));
    // the lane-group schedule (rtg_fk.hip): J <= kGroupMaxJ, at most J steps
    const int gF = group_frames(J);
    if (gF > 0) {
        std::vector<GEnt> gs((size_t)J * (64 / gF));
        const int steps = fk_group_schedule(parents, lt.data(), tq.data(), J, gF, gs.data(), J);
        if (steps > 0) {
            RTG_CHECK(t->gsched.alloc_upload(gs.data(), (size_t)steps * (64 / gF), "hipMalloc(group schedule)"));
            t->gF = gF;
            t->gsteps = steps;
        }
    }
    *out = t.release();
    return RTG_OK;
}

int rtg_topology_destroy(rtg_topology_t t)
{
    delete t;
    return RTG_OK;
}

int rtg_topology_num_joints(rtg_topology_t t) { return t ? t->J : -1; }

// ---------------------------------------------------------------- kinematics
int rtg_fk_f32(rtg_topology_t t, const float *local_rot, const float *root_t, int64_t B, float *g_rot, float *g_pos,
               rtg_stream_t stream)
{
    return run_fk("rtg_fk_f32", false, t, local_rot, root_t, B, g_rot, g_pos, stream);
}

int rtg_state_fk_f32(rtg_topology_t t, const float *local_rot, const float *root_t, int64_t B, float *g_rot,
                     float *g_pos, rtg_stream_t stream)
{
    return run_fk("rtg_state_fk_f32", true, t, local_rot, root_t, B, g_rot, g_pos, stream);
}

int rtg_local_rotation_f32(rtg_topology_t t, const float *g_rot, int64_t B, float *local_rot, rtg_stream_t stream)
{
    return run_local_rotation("rtg_local_rotation_f32", false, t, g_rot, B, local_rot, stream);
}

int rtg_state_local_rotation_f32(rtg_topology_t t, const float *g_rot, int64_t B, float *local_rot,
                                 rtg_stream_t stream)
{
    return run_local_rotation("rtg_state_local_rotation_f32", true, t, g_rot, B, local_rot, stream);
}

// (not a forward to rtg_kinematics_multi_f32: the messages name the function and count the segments differently)
int rtg_fk_multi_f32(const rtg_fk_segment *segs, int32_t n, rtg_stream_t stream)
{
    const char *fn = "rtg_fk_multi_f32";
    if (n < 0 || n > RTG_MAX_SEGMENTS)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: %d segments (max %d)", fn, n, RTG_MAX_SEGMENTS);
    if (n > 0 && !segs) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL segments", fn);
    FkMultiArgs A{};
    A.n = n;
    RTG_CHECK(fill_fk_segments(fn, segs, n, A.seg));
    RTG_TRY(launch_fk_multi(A, as_stream(stream)), "k_fk_multi");
    return RTG_OK;
}

int rtg_kinematics_multi_f32(const rtg_fk_segment *fk, int32_t n_fk, const rtg_local_rotation_segment *inv,
                             int32_t n_inv, rtg_stream_t stream)
{
    const char *fn = "rtg_kinematics_multi_f32";
    if (n_fk < 0 || n_inv < 0 || n_fk + n_inv > RTG_MAX_SEGMENTS)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: %d + %d segments (max %d in total)", fn, n_fk, n_inv, RTG_MAX_SEGMENTS);
    if ((n_fk > 0 && !fk) || (n_inv > 0 && !inv)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL segments", fn);
    FkMultiArgs A{};
    A.n = n_fk + n_inv;
    RTG_CHECK(fill_fk_segments(fn, fk, n_fk, A.seg));
    for (int i = 0; i < n_inv; ++i) {
        const rtg_local_rotation_segment &s = inv[i];
        RTG_CHECK(check_fk(s.topo, s.g_rot, s.local_rot, s.g_rot, s.local_rot, s.B, fn));
        A.seg[n_fk + i] = FkSeg{s.topo->view(), s.g_rot, nullptr, s.local_rot, nullptr, s.B, 1};
    }
    RTG_TRY(launch_fk_multi(A, as_stream(stream)), "k_fk_multi");
    return RTG_OK;
}

int rtg_local_rotation_multi_f32(const rtg_local_rotation_segment *segs, int32_t n, rtg_stream_t stream)
{
    return rtg_kinematics_multi_f32(nullptr, 0, segs, n, stream);
}

// ---------------------------------------------------------------- joint-angle forward model
int rtg_dof_model_create(rtg_topology_t topo, const int32_t *axis, const float *lower, const float *upper,
                         rtg_dof_model_t *out)
{
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_model_create: out is NULL");
    *out = nullptr;
    if (!topo) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_model_create: NULL topology");
    const int n = topo->J - 1;
    if (n > 0 && !axis) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_model_create: NULL axis");
    for (int k = 0; k < n; ++k)
        if (axis[k] < 0 || axis[k] > 2)
            return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_model_create: axis[%d]=%d is not 0, 1 or 2", k, axis[k]);
    if ((lower == nullptr) != (upper == nullptr))
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_model_create: give both DOF limit arrays or neither");
    std::unique_ptr<rtg_dof_model_s> m(new (std::nothrow) rtg_dof_model_s());
    if (!m) return fail(RTG_ERR_OUT_OF_MEMORY, "rtg_dof_model_create: host allocation failed");
    m->topo = topo;
    m->has_limits = lower != nullptr;
    const size_t cap = n > 0 ? n : 1;   // a one-joint model still owns (unread) tables
    RTG_CHECK(m->axis.alloc(cap, "hipMalloc(axis)"));
    if (n > 0) RTG_CHECK(m->axis.upload(axis, n));
    if (m->has_limits) {
        RTG_CHECK(m->lower.alloc(cap, "hipMalloc(lower)"));
        RTG_CHECK(m->upper.alloc(cap, "hipMalloc(upper)"));
        if (n > 0) RTG_CHECK(m->lower.upload(lower, n));
        if (n > 0) RTG_CHECK(m->upper.upload(upper, n));
    }
    *out = m.release();
    return RTG_OK;
}

int rtg_dof_model_destroy(rtg_dof_model_t m)
{
    delete m;
    return RTG_OK;
}

int rtg_dof_fk_f32(rtg_dof_model_t m, const float *dof, const float *root_rot, const float *root_t, int64_t B,
                   int clip, float *g_rot, float *g_pos, rtg_stream_t stream)
{
    if (!m) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_fk_f32: NULL model");
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_fk_f32: B=%lld < 0", (long long)B);
    if (clip && !m->has_limits)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_fk_f32: clip_angles requested but the model has no DOF limits");
    if (B == 0) return RTG_OK;
    if ((m->topo->J > 1 && !dof) || !root_rot || !root_t || !g_rot || !g_pos)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_fk_f32: NULL buffer");
    if (m->topo->J == 1) dof = root_rot;   // no angles: the kernel's unconditional first-element load gets readable memory
    RTG_TRY(launch_dof_fk(m->topo->view(), m->view(), clip != 0, dof, root_rot, root_t, B, g_rot, g_pos,
                          as_stream(stream)),
            "k_dof_fk");
    return RTG_OK;
}

int rtg_dof_fk_vel_f32(rtg_dof_model_t m, const float *dof, const float *root_rot, const float *root_t,
                       const float *dof_vel, const float *root_vel, int64_t B, int clip, float *g_rot, float *g_pos,
                       float *g_vel, rtg_stream_t stream)
{
    const char *fn = "rtg_dof_fk_vel_f32";
    // what does not depend on the handle first (rtg_dof_motion_sample_f32's order)
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: B=%lld < 0", fn, (long long)B);
    if (B > 0) {   // empty buffers have no address to give
        if ((g_rot == nullptr) != (g_pos == nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both g_rot and g_pos or neither", fn);
        if (!root_rot || !root_t || !g_vel) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    }
    if ((reinterpret_cast<uintptr_t>(root_rot) | reinterpret_cast<uintptr_t>(g_rot)) & 15)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: root_rot / g_rot not 16-byte aligned", fn);
    if (!m) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL model", fn);
    const int J = m->topo->J;
    if (J > kGroupMaxJ || !m->topo->gsched.get())
        return fail(RTG_ERR_UNSUPPORTED, "%s: serves models of 1..%d joints (this one has %d)", fn, kGroupMaxJ, J);
    if (clip && !m->has_limits)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: clip_angles requested but the model has no DOF limits", fn);
    if (B == 0) return RTG_OK;
    if (J > 1 && (!dof || !dof_vel)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    {   // no output may overlap an input (or another output)
        const uint64_t n = (uint64_t)B, j = (uint64_t)J;
        const Span in[] = {{dof, n * (j - 1) * 4, "dof"}, {dof_vel, n * (j - 1) * 4, "dof_vel"},
                           {root_rot, n * 16, "root_rot"}, {root_t, n * 12, "root_t"}, {root_vel, n * 24, "root_vel"}};
        const Span outs[] = {{g_rot, n * j * 16, "g_rot"}, {g_pos, n * j * 12, "g_pos"}, {g_vel, n * j * 24, "g_vel"}};
        RTG_CHECK(check_overlap(fn, outs, 3, in, 5));
    }
    if (J == 1) dof = dof_vel = root_rot;   // no angles: the kernel's unconditional first-element loads get readable memory
    RTG_TRY(launch_dof_fk_vel(m->topo->view(), m->view(), clip != 0, dof, dof_vel, root_rot, root_t, root_vel, B, g_rot,
                              g_pos, g_vel, as_stream(stream)),
            "k_dof_fk_vel");
    return RTG_OK;
}

// ---------------------------------------------------------------- gradients of the kinematics
int rtg_dof_fk_backward_f32(rtg_dof_model_t m, const float *dof, const float *g_rot, const float *grad_g_rot,
                            const float *grad_g_pos, int64_t B, int clip, float *grad_dof, float *grad_root_rot,
                            float *grad_root_t, rtg_stream_t stream)
{
    RTG_CHECK(check_fk_backward("rtg_dof_fk_backward_f32", B, grad_g_rot, grad_g_pos,
                                grad_dof || grad_root_rot || grad_root_t));
    if (!m) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_fk_backward_f32: NULL model");
    if (clip && !m->has_limits)
        return fail(RTG_ERR_INVALID_ARGUMENT,
                    "rtg_dof_fk_backward_f32: clip_angles requested but the model has no DOF limits");
    if (B == 0) return RTG_OK;
    const int J = m->topo->J;
    if ((J > 1 && !dof) || !g_rot) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_dof_fk_backward_f32: NULL buffer");
    if (J == 1) {   // no angles: the kernel's unconditional first-element load gets readable memory
        dof = g_rot;
        grad_dof = nullptr;
    }
    const DofView D = m->view();
    RTG_TRY(launch_fk_backward(m->topo->view(), &D, clip != 0, dof, g_rot, grad_g_rot, grad_g_pos, B, grad_dof,
                               grad_root_rot, grad_root_t, as_stream(stream)),
            "k_fk_bwd<dof>");
    return RTG_OK;
}

int rtg_fk_backward_f32(rtg_topology_t t, const float *local_rot, const float *g_rot, const float *grad_g_rot,
                        const float *grad_g_pos, int64_t B, float *grad_local_rot, float *grad_root_t,
                        rtg_stream_t stream)
{
    RTG_CHECK(check_fk_backward("rtg_fk_backward_f32", B, grad_g_rot, grad_g_pos, grad_local_rot || grad_root_t));
    if (!t) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_fk_backward_f32: NULL topology");
    if (B == 0) return RTG_OK;
    if (!local_rot || !g_rot) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_fk_backward_f32: NULL buffer");
    RTG_TRY(launch_fk_backward(t->view(), nullptr, false, local_rot, g_rot, grad_g_rot, grad_g_pos, B, grad_local_rot,
                               nullptr, grad_root_t, as_stream(stream)),
            "k_fk_bwd");
    return RTG_OK;
}

// ---------------------------------------------------------------- keypoint fit of the joint-angle model
int rtg_dof_fit_f32(rtg_dof_model_t m, const float *target_pos, const float *weight, const float *root_rot,
                    const float *root_t, const float *dof_in, int64_t B, int clip, int32_t iters, float lr, float beta1,
                    float beta2, float eps, int32_t step0, float *mom1, float *mom2, float *dof_out, float *loss,
                    float *grad, rtg_stream_t stream)
{
    const DofFitArgs A{target_pos, weight, root_rot, root_t, dof_in, B, iters, step0, lr, beta1, beta2, eps,
                       mom1, mom2, dof_out, loss, grad};
    return run_dof_fit("rtg_dof_fit_f32", m, clip, A, nullptr, stream);
}

int rtg_dof_fit_root_f32(rtg_dof_model_t m, const float *target_pos, const float *weight, const float *root_rot,
                         const float *root_t, const float *dof_in, int64_t B, int clip, int32_t fit_root, int32_t iters,
                         float lr, float lr_root_t, float lr_root_rot, float beta1, float beta2, float eps,
                         int32_t step0, float *mom1, float *mom2, float *root_state, float *dof_out,
                         float *root_rot_out, float *root_t_out, float *loss, float *grad, float *grad_root,
                         rtg_stream_t stream)
{
    const DofFitArgs A{target_pos, weight, root_rot, root_t, dof_in, B, iters, step0, lr, beta1, beta2, eps,
                       mom1, mom2, dof_out, loss, grad};
    const DofFitRootArgs R{fit_root, lr_root_t, lr_root_rot, root_state, root_rot_out, root_t_out, grad_root};
    return run_dof_fit("rtg_dof_fit_root_f32", m, clip, A, &R, stream);
}

int rtg_dof_fit_orient_f32(rtg_dof_model_t m, const float *target_pos, const float *weight, const int32_t *rot_joint,
                           const float *target_rot, const float *rot_weight, int32_t K, const float *root_rot,
                           const float *root_t, const float *dof_in, int64_t B, int clip, int32_t fit_root, int32_t iters,
                           float lr, float lr_root_t, float lr_root_rot, float beta1, float beta2, float eps,
                           int32_t step0, float *mom1, float *mom2, float *root_state, float *dof_out,
                           float *root_rot_out, float *root_t_out, float *loss, float *grad, float *grad_root,
                           rtg_stream_t stream)
{
    const DofFitArgs A{target_pos, weight, root_rot, root_t, dof_in, B, iters, step0, lr, beta1, beta2, eps,
                       mom1, mom2, dof_out, loss, grad};
    const DofFitRootArgs R{fit_root, lr_root_t, lr_root_rot, root_state, root_rot_out, root_t_out, grad_root};
    DofFitOriArgs O{target_rot, rot_weight, K, {}};
    return run_dof_fit("rtg_dof_fit_orient_f32", m, clip, A, &R, stream, &O, rot_joint);
}

int rtg_dof_fit_prior_f32(rtg_dof_model_t m, const float *target_pos, const float *weight, const int32_t *rot_joint,
                          const float *target_rot, const float *rot_weight, int32_t K, const float *prior,
                          const float *prior_weight, int32_t flags, const float *root_rot, const float *root_t,
                          const float *dof_in, int64_t B, int clip, int32_t fit_root, int32_t iters, float lr,
                          float lr_root_t, float lr_root_rot, float beta1, float beta2, float eps, int32_t step0, float *mo,
                          float *v, float *root_state, float *dof_out, float *root_rot_out, float *root_t_out, float *loss,
                          float *grad, float *grad_root, rtg_stream_t stream)
{
    const DofFitArgs A{target_pos, weight, root_rot, root_t, dof_in, B, iters, step0, lr, beta1, beta2, eps,
                       mo, v, dof_out, loss, grad};
    const DofFitRootArgs R{fit_root, lr_root_t, lr_root_rot, root_state, root_rot_out, root_t_out, grad_root};
    DofFitOriArgs O{target_rot, rot_weight, K, {}};
    const DofFitPriorArgs H{prior, prior_weight, flags};
    return run_dof_fit("rtg_dof_fit_prior_f32", m, clip, A, &R, stream, &O, rot_joint, &H);
}

int rtg_dof_fit_apart_f32(rtg_dof_model_t m, const float *target_pos, const float *weight, const int32_t *rot_joint,
                          const float *target_rot, const float *rot_weight, int32_t K, const float *prior,
                          const float *prior_weight, int32_t flags, const float *root_rot, const float *root_t,
                          const float *dof_in, int64_t B, int clip, int32_t fit_root, int32_t iters, float lr,
                          float lr_root_t, float lr_root_rot, float beta1, float beta2, float eps, int32_t step0, float *mo,
                          float *v, float *root_state, float *dof_out, float *root_rot_out, float *root_t_out, float *loss,
                          float *grad, float *grad_root, const rtg_fit_apart *apart, rtg_stream_t stream)
{
    const DofFitArgs A{target_pos, weight, root_rot, root_t, dof_in, B, iters, step0, lr, beta1, beta2, eps,
                       mo, v, dof_out, loss, grad};
    const DofFitRootArgs R{fit_root, lr_root_t, lr_root_rot, root_state, root_rot_out, root_t_out, grad_root};
    DofFitOriArgs O{target_rot, rot_weight, K, {}};
    const DofFitPriorArgs H{prior, prior_weight, flags};
    return run_dof_fit("rtg_dof_fit_apart_f32", m, clip, A, &R, stream, &O, rot_joint, &H, apart);
}

int rtg_dof_fit_robust_f32(rtg_dof_model_t m, const float *target_pos, const float *weight, const int32_t *rot_joint,
                           const float *target_rot, const float *rot_weight, int32_t K, const float *prior,
                           const float *prior_weight, int32_t flags, const float *root_rot, const float *root_t,
                           const float *dof_in, int64_t B, int clip, int32_t fit_root, int32_t iters, float lr,
                           float lr_root_t, float lr_root_rot, float beta1, float beta2, float eps, int32_t step0, float *mo,
                           float *v, float *root_state, float *dof_out, float *root_rot_out, float *root_t_out, float *loss,
                           float *grad, float *grad_root, const rtg_fit_apart *apart, const float *frame_weight,
                           float robust_scale, rtg_stream_t stream)
{
    const DofFitArgs A{target_pos, weight, root_rot, root_t, dof_in, B, iters, step0, lr, beta1, beta2, eps,
                       mo, v, dof_out, loss, grad};
    const DofFitRootArgs R{fit_root, lr_root_t, lr_root_rot, root_state, root_rot_out, root_t_out, grad_root};
    DofFitOriArgs O{target_rot, rot_weight, K, {}};
    const DofFitPriorArgs H{prior, prior_weight, flags};
    DofFitRobustArgs U{frame_weight, robust_scale, 0.0f};
    return run_dof_fit("rtg_dof_fit_robust_f32", m, clip, A, &R, stream, &O, rot_joint, &H, apart, &U);
}

// ---------------------------------------------------------------- SkeletonState.retarget_to
int rtg_retarget_plan_tables(const int32_t *src_parents, int32_t Js, const int32_t *tgt_parents, int32_t Jt,
                             const int32_t *src_joint, const int32_t *tgt_joint, int32_t K, int32_t *kept_src,
                             int32_t *src_reduced_parents, int32_t *kept_tgt, int32_t *tgt_reduced_parents,
                             int32_t *perm, int32_t *src_of)
{
    const char *fn = "rtg_retarget_plan_tables";
    if (!src_parents || !tgt_parents) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL parents", fn);
    RTG_CHECK(check_tree(fn, src_parents, Js));   // the trees rtg_topology_create accepts
    RTG_CHECK(check_tree(fn, tgt_parents, Jt));
    RetargetTables T;
    std::string err;
    if (!retarget_tables(src_parents, Js, tgt_parents, Jt, src_joint, tgt_joint, K, T, err))
        return fail_tables(fn, Js, Jt, err);
    auto put = [](int32_t *dst, const std::vector<int32_t> &v) {
        if (dst) memcpy(dst, v.data(), sizeof(int32_t) * v.size());
    };
    put(kept_src, T.kept_s);
    put(src_reduced_parents, T.sred_par);
    put(kept_tgt, T.kept_t);
    put(tgt_reduced_parents, T.tred_par);
    put(perm, T.perm);
    put(src_of, T.src_of);
    return RTG_OK;
}

int rtg_retarget_plan_create(rtg_topology_t src, rtg_topology_t tgt, const int32_t *src_joint,
                             const int32_t *tgt_joint, int32_t K, const float *src_tpose_local_rot,
                             const float *src_tpose_root_t, const float *tgt_tpose_local_rot,
                             const float *tgt_tpose_root_t, const float *rotation_to_target, float scale,
                             rtg_retarget_plan_t *out)
{
    const char *fn = "rtg_retarget_plan_create";
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    *out = nullptr;
    if (!src || !tgt) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL topology", fn);
    if (!src_tpose_local_rot || !src_tpose_root_t || !tgt_tpose_local_rot || !tgt_tpose_root_t || !rotation_to_target)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL t-pose / rotation", fn);
    const int Js = src->J, Jt = tgt->J;
    RetargetTables T;
    std::string err;
    if (!retarget_tables(src->h_parents.data(), Js, tgt->h_parents.data(), Jt, src_joint, tgt_joint, K, T, err))
        return fail_tables(fn, Js, Jt, err);
    std::unique_ptr<rtg_retarget_plan_s> p(new (std::nothrow) rtg_retarget_plan_s());
    if (!p) return fail(RTG_ERR_OUT_OF_MEMORY, "%s: host allocation failed", fn);
    std::vector<float> blob;
    RetargetView &V_ = p->view;
    retarget_blob(T, src->h_parents.data(), src->h_tree_quat.data(), tgt->h_parents.data(), tgt->h_tree_quat.data(),
                  blob, V_);
    V_.R = Q{rotation_to_target[0], rotation_to_target[1], rotation_to_target[2], rotation_to_target[3]};
    V_.scale = scale;
    V_.tgt_root = v3(tgt_tpose_root_t, 0);
    V_.t_tp = V{0.f, 0.f, 0.f};
    // The constants, on the device: the t-poses normalised (from_rotation_and_root_translation, :610), the source one
    // through stages 1-6 of the kernel itself, the target one through the state FK kernel.  Scratch, in floats:
    // src rows | src root | tgt rows | tgt root | dump (4 K + 3, padded) | tgt global rows | tgt positions | the two
    // t-poses as given
    const size_t o_sr = 0, o_st = o_sr + 4 * (size_t)Js, o_tr = o_st + 4, o_tt = o_tr + 4 * (size_t)Jt, o_d = o_tt + 4,
                 o_g = o_d + 4 * (size_t)K + 4, o_p = o_g + 4 * (size_t)Jt, o_sraw = o_p + 4 * (size_t)Jt,
                 o_traw = o_sraw + 4 * (size_t)Js, n_ws = o_traw + 4 * (size_t)Jt;
    std::vector<float> h(n_ws, 0.0f);
    memcpy(&h[o_sraw], src_tpose_local_rot, sizeof(float) * 4 * Js);
    memcpy(&h[o_st], src_tpose_root_t, sizeof(float) * 3);
    memcpy(&h[o_traw], tgt_tpose_local_rot, sizeof(float) * 4 * Jt);
    DevBuf<float> scratch;   // gone when this function returns
    RTG_CHECK(scratch.alloc(n_ws, "hipMalloc(plan scratch)"));
    RTG_CHECK(p->blob.alloc(blob.size(), "hipMalloc(plan blob)"));
    RTG_CHECK(scratch.upload(h.data(), n_ws));
    RTG_CHECK(p->blob.upload(blob.data(), blob.size()));
    V_.blob = p->blob.get();
    float *ws = scratch.get();
    RTG_TRY(launch_quat_op(RTG_OP_QUAT_NORMALIZE, ws + o_sraw, nullptr, nullptr, Js, ws + o_sr, nullptr),
            "quat_normalize(source t-pose)");
    RTG_TRY(launch_quat_op(RTG_OP_QUAT_NORMALIZE, ws + o_traw, nullptr, nullptr, Jt, ws + o_tr, nullptr),
            "quat_normalize(target t-pose)");
    RTG_TRY(launch_retarget_to(V_, true, ws + o_sr, ws + o_st, 1, nullptr, nullptr, ws + o_d, nullptr),
            "k_retarget_to(t-pose)");
    RTG_TRY(launch_fk(tgt->view(), true, ws + o_tr, ws + o_tt, 1, ws + o_g, ws + o_p, nullptr),
            "k_fk<state>(target t-pose)");
    RTG_TRY(hipMemcpy(h.data(), ws, sizeof(float) * n_ws, hipMemcpyDeviceToHost), "hipMemcpy");
    for (int k = 0; k < K; ++k) {
        float *cg = &blob[4 * ((size_t)V_.o_cg + k)], *tg = &blob[4 * ((size_t)V_.o_tg + k)];
        const float *g = &h[o_d + 4 * (size_t)k], *t = &h[o_g + 4 * (size_t)T.kept_t[k]];
        cg[0] = -g[0], cg[1] = -g[1], cg[2] = -g[2], cg[3] = g[3];   // quat_inverse = the conjugate (:214-219)
        memcpy(tg, t, sizeof(float) * 4);
    }
    V_.t_tp = V{h[o_d + 4 * (size_t)K], h[o_d + 4 * (size_t)K + 1], h[o_d + 4 * (size_t)K + 2]};
    RTG_CHECK(p->blob.upload(blob.data(), blob.size()));
    *out = p.release();
    return RTG_OK;
}

int rtg_retarget_plan_destroy(rtg_retarget_plan_t p)
{
    delete p;
    return RTG_OK;
}

int rtg_retarget_to_f32(rtg_retarget_plan_t p, const float *src_rot, const float *src_root_t, int src_is_local,
                        int64_t B, float *tgt_local_rot, float *tgt_root_t, rtg_stream_t stream)
{
    if (!p) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_to_f32: NULL plan");
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_to_f32: negative batch %lld", (long long)B);
    if (B == 0) return RTG_OK;
    if (!src_rot || !src_root_t || !tgt_local_rot || !tgt_root_t)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_to_f32: NULL buffer");
    RTG_TRY(launch_retarget_to(p->view, src_is_local != 0, src_rot, src_root_t, B, tgt_local_rot, tgt_root_t, nullptr,
                               as_stream(stream)),
            "k_retarget_to");
    return RTG_OK;
}

// ---------------------------------------------------------------- keypoint targets for the pose fit
int rtg_fit_targets_plan_tables(int32_t Js, const int32_t *tgt_parents, const float *tgt_local_t, int32_t Jt,
                                const int32_t *src_joint, const int32_t *tgt_joint, int32_t K, int32_t *anchor,
                                float *seg, float *weight, int32_t *src_of)
{
    const char *fn = "rtg_fit_targets_plan_tables";
    if (!tgt_parents || !tgt_local_t) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL parents/local_t", fn);
    RTG_CHECK(check_tree(fn, tgt_parents, Jt));   // the trees rtg_topology_create accepts
    FitTargetsTables T;
    std::string err;
    if (!fit_targets_tables(Js, tgt_parents, tgt_local_t, Jt, src_joint, tgt_joint, K, T, err))
        return fail_tables(fn, Js, Jt, err);
    if (anchor) memcpy(anchor, T.anchor.data(), sizeof(int32_t) * K);
    if (seg) memcpy(seg, T.seg.data(), sizeof(float) * 3 * K);
    if (weight) memcpy(weight, T.weight.data(), sizeof(float) * Jt);
    if (src_of) memcpy(src_of, T.src_of.data(), sizeof(int32_t) * Jt);
    return RTG_OK;
}

int rtg_fit_targets_plan_create(rtg_topology_t src, rtg_topology_t tgt, const int32_t *src_joint,
                                const int32_t *tgt_joint, int32_t K, const float *dir, const float *root_scale,
                                const float *root_offset, rtg_fit_targets_plan_t *out)
{
    const char *fn = "rtg_fit_targets_plan_create";
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    *out = nullptr;
    if (!src || !tgt) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL topology", fn);
    const int Js = src->J, Jt = tgt->J;
    FitTargetsTables T;
    std::string err;
    if (!fit_targets_tables(Js, tgt->h_parents.data(), &tgt->h_local_t[0].x, Jt, src_joint, tgt_joint, K, T, err))
        return fail_tables(fn, Js, Jt, err);
    std::unique_ptr<rtg_fit_targets_plan_s> p(new (std::nothrow) rtg_fit_targets_plan_s());
    if (!p) return fail(RTG_ERR_OUT_OF_MEMORY, "%s: host allocation failed", fn);
    std::vector<float> blob;
    FitTargetsView &V_ = p->view;
    fit_targets_blob(T, src_joint, tgt_joint, blob, V_);
    V_.dir_on = dir != nullptr, V_.scale_on = root_scale != nullptr, V_.offset_on = root_offset != nullptr;
    if (dir) V_.dir = v3(dir, 0);
    if (root_scale) V_.root_scale = v3(root_scale, 0);
    if (root_offset) V_.root_offset = v3(root_offset, 0);
    RTG_CHECK(p->blob.alloc_upload(blob.data(), blob.size(), "hipMalloc(plan blob)"));
    V_.blob = p->blob.get();
    *out = p.release();
    return RTG_OK;
}

int rtg_fit_targets_plan_destroy(rtg_fit_targets_plan_t p)
{
    delete p;
    return RTG_OK;
}

int rtg_fit_targets_f32(rtg_fit_targets_plan_t p, const float *src_pos, int64_t B, float *target_pos,
                        rtg_stream_t stream)
{
    const char *fn = "rtg_fit_targets_f32";
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: B=%lld < 0", fn, (long long)B);   // needs no handle
    if (!p) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL plan", fn);
    if (B == 0) return RTG_OK;
    if (!src_pos || !target_pos) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    if (B > (int64_t)0x7fffffff * 8) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: batch too large", fn);
    const Span in{src_pos, (uint64_t)B * p->view.Js * 12u, "src_pos"}, o{target_pos, (uint64_t)B * p->view.Jt * 12u, "target_pos"};
    RTG_CHECK(check_overlap(fn, &in, 1, &o, 1));
    RTG_TRY(launch_fit_targets(p->view, src_pos, B, target_pos, as_stream(stream)), "k_fit_targets");
    return RTG_OK;
}

// ---------------------------------------------------------------- VTRDyn ingest
int rtg_ingest_vtrdyn_f32(const float *bp, const float *lhp, const float *rhp, int64_t B, int layout, float *body,
                          float *lh, float *rh, uint8_t *valid, rtg_stream_t stream)
{
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_ingest_vtrdyn_f32: B < 0");
    RTG_CHECK(check_layout("rtg_ingest_vtrdyn_f32", layout));
    if (B == 0) return RTG_OK;
    if (!bp || !lhp || !rhp || !body || !lh || !rh || !valid)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_ingest_vtrdyn_f32: NULL buffer");
    RTG_TRY(launch_ingest_vtrdyn(bp, lhp, rhp, B, layout, body, lh, rh, valid, as_stream(stream)), "k_ingest_vtrdyn");
    return RTG_OK;
}

// ---------------------------------------------------------------- rotation ingest (the zero-pose transforms)
int rtg_rot_ingest_create(int32_t J_in, int32_t J_out, const int32_t *src, const float *pre, const float *post,
                          rtg_rot_ingest_t *out)
{
    const char *fn = "rtg_rot_ingest_create";
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    *out = nullptr;
    if (J_in < 1 || J_in > kRotIngMaxJ || J_out < 1 || J_out > kRotIngMaxJ)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: J_in %d / J_out %d outside 1..%d", fn, J_in, J_out, kRotIngMaxJ);
    if (!pre || !post) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL pre / post", fn);
    if (!src && J_in != J_out)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: src is NULL (the identity) but J_in %d != J_out %d", fn, J_in, J_out);
    for (int j = 0; src && j < J_out; ++j)
        if (src[j] < 0 || src[j] >= J_in)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: src[%d] = %d outside 0..%d", fn, j, src[j], J_in - 1);
    std::unique_ptr<rtg_rot_ingest_s> h(new (std::nothrow) rtg_rot_ingest_s());
    if (!h) return fail(RTG_ERR_OUT_OF_MEMORY, "%s: host allocation failed", fn);
    std::vector<float> blob;
    rot_ingest_blob(J_in, J_out, src, pre, post, blob, h->view);
    RTG_CHECK(h->blob.alloc_upload(blob.data(), blob.size(), "hipMalloc(rot ingest blob)"));
    RTG_TRY(launch_rot_ingest_tab(h->blob.get() + 4 * h->view.o_tab, nullptr), "k_rot_ingest_tab");
    RTG_TRY(hipStreamSynchronize(nullptr), "hipStreamSynchronize");
    h->view.blob = h->blob.get();
    *out = h.release();
    return RTG_OK;
}

void rtg_rot_ingest_destroy(rtg_rot_ingest_t h) { delete h; }

int rtg_rot_ingest_f32(rtg_rot_ingest_t h, const float *q, int64_t B, int layout, float *out, rtg_stream_t stream)
{
    const char *fn = "rtg_rot_ingest_f32";
    // what does not depend on the handle first: a caller (and a test on a machine without a GPU) sees these reasons
    // whatever the handle is
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: B < 0", fn);
    RTG_CHECK(check_layout(fn, layout));
    if (B > 0 && (!q || !out)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    if (B > 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(out)) & 15))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: q / out not 16-byte aligned", fn);
    if (!h) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL handle", fn);
    if (B == 0) return RTG_OK;
    const Span in{q, (uint64_t)B * h->view.J_in * 16, "q"}, o{out, (uint64_t)B * h->view.J_out * 16, "out"};
    RTG_CHECK(check_overlap(fn, &in, 1, &o, 1));
    RTG_TRY(launch_rot_ingest(h->view, q, B, layout, out, as_stream(stream)), "k_rot_ingest");
    return RTG_OK;
}

// ---------------------------------------------------------------- motion sampling
int rtg_motion_lib_create(const int64_t *start, const int32_t *len, const float *fps, int32_t C, int64_t F_total,
                          rtg_motion_lib_t *out)
{
    const char *fn = "rtg_motion_lib_create";
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
    *out = nullptr;
    if (!start || !len || !fps) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL start / len / fps", fn);
    if (C < 1) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: C=%d clips (need at least 1)", fn, C);
    if (F_total < 1 || F_total > INT32_MAX)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: F_total=%lld outside 1..2^31-1", fn, (long long)F_total);
    std::vector<MotionClip> tab((size_t)C);
    for (int c = 0; c < C; ++c) {
        if (len[c] < 1) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: len[%d]=%d < 1", fn, c, len[c]);
        if (start[c] < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: start[%d]=%lld < 0", fn, c, (long long)start[c]);
        if (start[c] > F_total - len[c])
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: clip %d ends at row %lld, past F_total=%lld", fn, c,
                        (long long)start[c] + len[c], (long long)F_total);
        if (!std::isfinite(fps[c]) || !(fps[c] > 0.0f))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: fps[%d]=%g must be finite and positive", fn, c, (double)fps[c]);
        tab[c] = MotionClip{start[c], len[c], fps[c]};
    }
    std::unique_ptr<rtg_motion_lib_s> h(new (std::nothrow) rtg_motion_lib_s());
    if (!h) return fail(RTG_ERR_OUT_OF_MEMORY, "%s: host allocation failed", fn);
    RTG_CHECK(h->clips.alloc_upload(tab.data(), C, "hipMalloc(motion clip table)"));
    h->C = C;
    h->F_total = F_total;
    *out = h.release();
    return RTG_OK;
}

void rtg_motion_lib_destroy(rtg_motion_lib_t h) { delete h; }

int rtg_motion_sample_f32(rtg_topology_t topo, rtg_motion_lib_t lib, const float *rot, const float *root_t,
                          const float *vec, int32_t K, const int32_t *clip, const float *time, int64_t N, int flags,
                          float *local_rot_out, float *root_t_out, float *vec_out, float *g_rot, float *g_pos,
                          rtg_stream_t stream)
{
    const char *fn = "rtg_motion_sample_f32";
    // what does not depend on the handles first: a caller (and a test on a machine without a GPU) sees these reasons
    // whatever the handles are
    if (N < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: N=%lld < 0", fn, (long long)N);
    if (K < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: K=%d < 0", fn, K);
    if (flags & ~(RTG_MOTION_NORMALIZE | RTG_MOTION_GLOBAL | RTG_MOTION_STATE))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", fn, flags);
    const bool global = (flags & RTG_MOTION_GLOBAL) != 0;
    if (N > 0) {   // empty buffers have no address to give
        if ((vec == nullptr) != (vec_out == nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both vec and vec_out or neither", fn);
        if (vec && K < 1) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: vec rows given with K=%d", fn, K);
        if ((g_rot == nullptr) != (g_pos == nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both g_rot and g_pos or neither", fn);
        if (global != (g_rot != nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: g_rot / g_pos go with RTG_MOTION_GLOBAL (flag %d, buffers %s)",
                        fn, (int)global, g_rot ? "given" : "NULL");
        if (!rot || !root_t || !clip || !time || !local_rot_out || !root_t_out)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    }
    if ((reinterpret_cast<uintptr_t>(rot) | reinterpret_cast<uintptr_t>(local_rot_out) |
         reinterpret_cast<uintptr_t>(g_rot)) & 15)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: rot / local_rot_out / g_rot not 16-byte aligned", fn);
    if (!topo) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL topology", fn);
    if (!lib) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL library", fn);
    const int J = topo->J;
    if (J > kGroupMaxJ || !topo->gsched.get())
        return fail(RTG_ERR_UNSUPPORTED, "%s: serves skeletons of 1..%d joints (this one has %d)", fn, kGroupMaxJ, J);
    if (N == 0) return RTG_OK;
    {   // no output may overlap an input (or another output)
        const uint64_t Ft = (uint64_t)lib->F_total, n = (uint64_t)N, j = (uint64_t)J, k = (uint64_t)K;
        const Span in[] = {{rot, Ft * j * 16, "rot"}, {root_t, Ft * 12, "root_t"}, {vec, Ft * k * 12, "vec"},
                           {clip, n * 4, "clip"}, {time, n * 4, "time"}};
        const Span outs[] = {{local_rot_out, n * j * 16, "local_rot_out"}, {root_t_out, n * 12, "root_t_out"},
                             {vec_out, n * k * 12, "vec_out"}, {g_rot, n * j * 16, "g_rot"}, {g_pos, n * j * 12, "g_pos"}};
        RTG_CHECK(check_overlap(fn, outs, 5, in, 5));
    }
    const MotionSampleArgs A{rot, root_t, vec, K, clip, time, N, local_rot_out, root_t_out, vec_out, g_rot, g_pos};
    RTG_TRY(launch_motion_sample(topo->view(), MotionLibView{lib->clips.get(), lib->C},
                                 (flags & RTG_MOTION_NORMALIZE) != 0, global, (flags & RTG_MOTION_STATE) != 0, A,
                                 as_stream(stream)),
            "k_motion_sample");
    return RTG_OK;
}

// rtg_dof_motion_sample_f32 (g_vel and key_vel nullptr: its checks, its messages, its launch) and
// rtg_dof_motion_sample_vel_f32 (at least one of the two given) on one checked path
static int dof_motion_sample(const char *fn, rtg_dof_model_t m, rtg_motion_lib_t lib, const float *dof,
                             const float *root_rot, const float *root_t, const int32_t *clip, const float *time,
                             int64_t N, int flags, const int32_t *key_links, int32_t K, float *dof_out,
                             float *dof_vel_out, float *root_rot_out, float *root_t_out, float *root_vel_out,
                             float *g_rot, float *g_pos, float *key_pos, float *g_vel, float *key_vel,
                             rtg_stream_t stream)
{
    const bool link_vel = g_vel != nullptr || key_vel != nullptr;
    // what does not depend on the handles first: a caller (and a test on a machine without a GPU) sees these reasons
    // whatever the handles are
    if (N < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: N=%lld < 0", fn, (long long)N);
    if (K < 0 || K > RTG_DOF_MOTION_MAX_KEY_LINKS)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: K=%d key links outside 0..%d", fn, K, RTG_DOF_MOTION_MAX_KEY_LINKS);
    if (flags & ~(RTG_DOF_MOTION_NORMALIZE | RTG_DOF_MOTION_CLIP))
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: unknown flags 0x%x", fn, flags);
    if (K > 0 && !key_links) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: K=%d with key_links NULL", fn, K);
    DofMotionArgs A{};
    for (int k = 0; k < K; ++k) {   // (no model has more than kGroupMaxJ joints here; its own J is checked below)
        if (key_links[k] < 0 || key_links[k] >= kGroupMaxJ)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: key_links[%d]=%d is outside 0..J-1", fn, k, key_links[k]);
        A.key[k] = (uint8_t)key_links[k];
    }
    if (N > 0) {   // empty buffers have no address to give
        if (dof_vel_out && !root_vel_out)   // (the other half needs the model: a one-joint model has no dof_vel_out)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both dof_vel_out and root_vel_out or neither", fn);
        if ((g_rot == nullptr) != (g_pos == nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both g_rot and g_pos or neither", fn);
        if (link_vel && (K > 0) != (key_pos != nullptr || key_vel != nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: key_pos / key_vel go with K > 0 (K=%d, key_pos %s, key_vel %s)",
                        fn, K, key_pos ? "given" : "NULL", key_vel ? "given" : "NULL");
        if (!link_vel && (K > 0) != (key_pos != nullptr))
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: key_pos goes with K > 0 (K=%d, key_pos %s)", fn, K,
                        key_pos ? "given" : "NULL");
        if (link_vel && !root_vel_out)   // the sweep's tangent inputs are the launch's own velocity rows
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: g_vel / key_vel need dof_vel_out and root_vel_out", fn);
        if (!root_rot || !root_t || !clip || !time || !root_rot_out || !root_t_out)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    }
    if ((reinterpret_cast<uintptr_t>(root_rot) | reinterpret_cast<uintptr_t>(root_rot_out) |
         reinterpret_cast<uintptr_t>(g_rot)) & 15)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: root_rot / root_rot_out / g_rot not 16-byte aligned", fn);
    if (!m) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL model", fn);
    if (!lib) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL library", fn);
    const int J = m->topo->J;
    if (J > kGroupMaxJ || !m->topo->gsched.get())
        return fail(RTG_ERR_UNSUPPORTED, "%s: serves models of 1..%d joints (this one has %d)", fn, kGroupMaxJ, J);
    if ((flags & RTG_DOF_MOTION_CLIP) && !m->has_limits)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: RTG_DOF_MOTION_CLIP requested but the model has no DOF limits", fn);
    for (int k = 0; k < K; ++k)
        if (key_links[k] >= J)
            return fail(RTG_ERR_INVALID_ARGUMENT, "%s: key_links[%d]=%d is outside 0..%d", fn, k, key_links[k], J - 1);
    if (N == 0) return RTG_OK;
    // a one-joint model has no angles: the dof pointers are not looked at
    if (J > 1 && root_vel_out && !dof_vel_out)
        return fail(RTG_ERR_INVALID_ARGUMENT, "%s: give both dof_vel_out and root_vel_out or neither", fn);
    if (J > 1 && (!dof || !dof_out)) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    {   // no output may overlap an input (or another output)
        const uint64_t Ft = (uint64_t)lib->F_total, n = (uint64_t)N, j = (uint64_t)J, k = (uint64_t)K;
        const Span in[] = {{dof, Ft * (j - 1) * 4, "dof"}, {root_rot, Ft * 16, "root_rot"}, {root_t, Ft * 12, "root_t"},
                           {clip, n * 4, "clip"}, {time, n * 4, "time"}};
        const Span outs[] = {{dof_out, n * (j - 1) * 4, "dof_out"}, {dof_vel_out, n * (j - 1) * 4, "dof_vel_out"},
                             {root_rot_out, n * 16, "root_rot_out"}, {root_t_out, n * 12, "root_t_out"},
                             {root_vel_out, n * 24, "root_vel_out"}, {g_rot, n * j * 16, "g_rot"},
                             {g_pos, n * j * 12, "g_pos"}, {key_pos, n * k * 12, "key_pos"},
                             {g_vel, n * j * 24, "g_vel"}, {key_vel, n * k * 24, "key_vel"}};
        RTG_CHECK(check_overlap(fn, outs, 10, in, 5));
    }
    A.dof = dof; A.root_rot = root_rot; A.root_t = root_t;
    A.clip = clip; A.time = time; A.N = N;
    A.normalize = (flags & RTG_DOF_MOTION_NORMALIZE) != 0;
    A.K = K;
    A.dof_out = dof_out; A.dof_vel_out = dof_vel_out; A.root_rot_out = root_rot_out; A.root_t_out = root_t_out;
    A.root_vel_out = root_vel_out; A.g_rot = g_rot; A.g_pos = g_pos; A.key_pos = key_pos;
    if (link_vel) {
        RTG_TRY(launch_dof_motion_sample_vel(m->topo->view(), m->view(), MotionLibView{lib->clips.get(), lib->C},
                                             (flags & RTG_DOF_MOTION_CLIP) != 0, DofMotionVelArgs{A, g_vel, key_vel},
                                             as_stream(stream)),
                "k_dof_motion_sample_vel");
        return RTG_OK;
    }
    RTG_TRY(launch_dof_motion_sample(m->topo->view(), m->view(), MotionLibView{lib->clips.get(), lib->C},
                                     (flags & RTG_DOF_MOTION_CLIP) != 0, A, as_stream(stream)),
            "k_dof_motion_sample");
    return RTG_OK;
}

int rtg_dof_motion_sample_f32(rtg_dof_model_t m, rtg_motion_lib_t lib, const float *dof, const float *root_rot,
                              const float *root_t, const int32_t *clip, const float *time, int64_t N, int flags,
                              const int32_t *key_links, int32_t K, float *dof_out, float *dof_vel_out,
                              float *root_rot_out, float *root_t_out, float *root_vel_out, float *g_rot, float *g_pos,
                              float *key_pos, rtg_stream_t stream)
{
    return dof_motion_sample("rtg_dof_motion_sample_f32", m, lib, dof, root_rot, root_t, clip, time, N, flags,
                             key_links, K, dof_out, dof_vel_out, root_rot_out, root_t_out, root_vel_out, g_rot, g_pos,
                             key_pos, nullptr, nullptr, stream);
}

// with g_vel and key_vel both NULL this is rtg_dof_motion_sample_f32, its messages under its name included
int rtg_dof_motion_sample_vel_f32(rtg_dof_model_t m, rtg_motion_lib_t lib, const float *dof, const float *root_rot,
                                  const float *root_t, const int32_t *clip, const float *time, int64_t N, int flags,
                                  const int32_t *key_links, int32_t K, float *dof_out, float *dof_vel_out,
                                  float *root_rot_out, float *root_t_out, float *root_vel_out, float *g_rot,
                                  float *g_pos, float *key_pos, float *g_vel, float *key_vel, rtg_stream_t stream)
{
    return dof_motion_sample(g_vel || key_vel ? "rtg_dof_motion_sample_vel_f32" : "rtg_dof_motion_sample_f32", m, lib,
                             dof, root_rot, root_t, clip, time, N, flags, key_links, K, dof_out, dof_vel_out,
                             root_rot_out, root_t_out, root_vel_out, g_rot, g_pos, key_pos, g_vel, key_vel, stream);
}

// ---------------------------------------------------------------- motion-level prep (retarget/main.py)
int rtg_rescale_motion_f32(rtg_topology_t topo, const float *motion, int64_t B, const float *dir, float *out,
                           rtg_stream_t stream)
{
    if (!topo) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rescale_motion_f32: NULL topology");
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rescale_motion_f32: B < 0");
    if (B == 0) return RTG_OK;
    if (!motion || !out) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rescale_motion_f32: NULL buffer");
    RTG_TRY(launch_rescale_motion(topo->view(), motion, B, dir, out, as_stream(stream)), "k_rescale_motion");
    return RTG_OK;
}

int rtg_quat_between_f32(const float *v1, const float *v2, int64_t n, float *out, float *ws, rtg_stream_t stream)
{
    if (n < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_quat_between_f32: n < 0");
    if (n == 0) return RTG_OK;
    if (!v1 || !v2 || !out || !ws) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_quat_between_f32: NULL buffer");
    RTG_TRY(launch_quat_between(v1, v2, n, out, ws, as_stream(stream)), "k_quat_between");
    return RTG_OK;
}

int rtg_rebuild_vtrdyn_f32(rtg_topology_t topo, const float *motion, int64_t B, float *g_rot, float *root_t,
                           float *ws, rtg_stream_t stream)
{
    if (!topo) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rebuild_vtrdyn_f32: NULL topology");
    if (topo->J != 21)   // main.py:126-136 index the VTRDYN joints 0, 1, 4, 7, 10, 11, 13, 17
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rebuild_vtrdyn_f32: expects the 21-joint VTRDYN zero pose, got %d",
                    topo->J);
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rebuild_vtrdyn_f32: B < 0");
    if (B == 0) return RTG_OK;
    if (!motion || !g_rot || !root_t || !ws) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_rebuild_vtrdyn_f32: NULL buffer");
    RTG_TRY(launch_rebuild_vtrdyn(topo->view(), motion, B, g_rot, root_t, ws, as_stream(stream)), "k_rebuild_vtrdyn");
    return RTG_OK;
}

// ---------------------------------------------------------------- solvers
int rtg_solver_create(int kind, const float *zl, const float *zg, const int32_t *parents, int32_t Js,
                      int precise_gripper, rtg_solver_t *out)
{
    if (!out) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_solver_create: out is NULL");
    *out = nullptr;
    if (!zl) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_solver_create: NULL zero-pose local translation");
    SolverConsts C{};
    switch (kind) {
    case RTG_SOLVER_FULL_BODY_POS: {
        if (Js != 59) return fail(RTG_ERR_INVALID_ARGUMENT, "FULL_BODY_POS expects the 59-joint VTRDYN_FULL zero pose, got %d", Js);
        if (!zg) return fail(RTG_ERR_INVALID_ARGUMENT, "FULL_BODY_POS needs the zero-pose global translation");
        // full_body_pos_retargeter.py:69, :139, :162, :78/:86/:99/:107, :184
        C.Zt[0] = v3(zl, 11); C.Zt[1] = v3(zl, 36); C.Zt[2] = v3(zl, 34);
        // the zero-column torso fit (torso_quat_x0): from Zt itself; -0 qualifies (the column's sign reaches no output)
        C.torso_x0 = 1;
        for (int j = 0; j < 3; ++j)
            if (!(C.Zt[j].x == 0.0f && std::fabs(C.Zt[j].y) <= 0x1p60f && std::fabs(C.Zt[j].z) <= 0x1p60f)) C.torso_x0 = 0;
        const int li[5] = {16, 20, 24, 28, 32}, ri[5] = {41, 45, 49, 53, 56}, gi[5] = {18, 22, 26, 30, 33};
        for (int t = 0; t < 5; ++t) {
            C.Zl[t] = v3(zl, li[t]);
            C.Zr[t] = v3(zl, ri[t]);
            C.grip_d[t] = zg[3 * gi[t]] - zg[3 * 14];
        }
        C.v0_lsh = v3(zl, 13); C.v0_lel = v3(zl, 14); C.v0_rsh = v3(zl, 38); C.v0_rel = v3(zl, 39);
        break;
    }
    case RTG_SOLVER_UPPER_BODY:
        if (Js != 21) return fail(RTG_ERR_INVALID_ARGUMENT, "UPPER_BODY expects the 21-joint VTRDYN zero pose, got %d", Js);
        // retarget_solver.py:49-86
        C.Zt[0] = v3(zl, 17); C.Zt[1] = v3(zl, 13); C.Zt[2] = v3(zl, 11);
        C.v0_lsh = v3(zl, 19); C.v0_lel = v3(zl, 20); C.v0_rsh = v3(zl, 15); C.v0_rel = v3(zl, 16);
        break;
    case RTG_SOLVER_FULL_BODY_ROT: {
        if (Js != 59) return fail(RTG_ERR_INVALID_ARGUMENT, "FULL_BODY_ROT expects the 59-joint VTRDYN_FULL zero pose, got %d", Js);
        // full_body_retargeter.py:64,72,85,93,152 (gripper uses LOCAL translations, joint 24)
        C.v0_lsh = v3(zl, 13); C.v0_lel = v3(zl, 14); C.v0_rsh = v3(zl, 38); C.v0_rel = v3(zl, 39);
        const int gi[5] = {18, 22, 26, 30, 33};
        for (int t = 0; t < 5; ++t) C.grip_d[t] = zl[3 * gi[t]] - zl[3 * 24];
        break;
    }
    case RTG_SOLVER_BODY_ROT:
        if (Js != 21) return fail(RTG_ERR_INVALID_ARGUMENT, "BODY_ROT expects the 21-joint VTRDYN zero pose, got %d", Js);
        if (!parents) return fail(RTG_ERR_INVALID_ARGUMENT, "BODY_ROT needs the source parent indices");
        C.par[0] = parents[18]; C.par[1] = parents[14]; C.par[2] = parents[19]; C.par[3] = parents[15];
        for (int i = 0; i < 4; ++i)
            if (C.par[i] < 0 || C.par[i] >= 21) return fail(RTG_ERR_INVALID_ARGUMENT, "BODY_ROT: bad parent index");
        break;
    default:
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_solver_create: unknown solver kind %d", kind);
    }
    {   // the zero-pose-only terms: evaluated on the device, read back
        DevBuf<SolverConsts> d;
        RTG_CHECK(d.alloc(1, "hipMalloc(solver consts)"));
        RTG_CHECK(d.upload(&C, 1, "hipMemcpy(consts)"));
        if (kind != RTG_SOLVER_BODY_ROT) RTG_TRY(launch_solver_prep(d.get(), nullptr), "k_solver_prep");
        RTG_TRY(hipMemcpy(&C, d.get(), sizeof C, hipMemcpyDeviceToHost), "hipMemcpy(consts)");
    }
    // exp-map angle table: built once per solver on the current device (6.7 MiB), read by every launch
    DevBuf<uint32_t> tab;
    RTG_CHECK(tab.alloc(kAngTabWords, "hipMalloc(exp-map angle table)"));
    RTG_TRY(launch_build_ang_tab(tab.get(), nullptr), "k_build_ang_tab");
    RTG_TRY(hipStreamSynchronize(nullptr), "k_build_ang_tab");
    C.ang_tab = tab.get();
    // the error word: host-mapped, so the device's report is read on the next call without a HIP call
    PinnedWord err;
    RTG_CHECK(err.alloc("hipHostMalloc(error word)"));
    RTG_TRY(hipHostGetDevicePointer(reinterpret_cast<void **>(&C.err), err.get(), 0), "hipHostGetDevicePointer");
    std::unique_ptr<rtg_solver_s> s(new (std::nothrow) rtg_solver_s());
    if (!s) return fail(RTG_ERR_OUT_OF_MEMORY, "rtg_solver_create: host allocation failed");
    s->kind = kind;
    s->precise = precise_gripper ? 1 : 0;
    s->consts = C;
    s->ang_tab = std::move(tab);
    s->err = std::move(err);
    *out = s.release();
    return RTG_OK;
}

int rtg_solver_destroy(rtg_solver_t s)
{
    delete s;
    return RTG_OK;
}

int rtg_retarget_f32(rtg_solver_t s, const float *in0, const float *in1, const float *in2, const float *in3,
                     int64_t B, int layout, float *dof, float *local_rot, float *body_rot, rtg_stream_t stream)
{
    if (!s) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: NULL solver");
    RTG_CHECK(take_device_error(s->err.get(), "rtg_retarget_f32"));
    if (B < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: negative batch");
    RTG_CHECK(check_layout("rtg_retarget_f32", layout));
    if (B == 0) return RTG_OK;
    if (B > (int64_t)0x7fffffff * 256) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: batch too large");
    if (!dof) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: NULL dof");
    const int need = s->kind == RTG_SOLVER_FULL_BODY_ROT ? 4 : (s->kind == RTG_SOLVER_FULL_BODY_POS ? 3 : 1);
    const float *ins[4] = {in0, in1, in2, in3};
    for (int i = 0; i < 4; ++i) {
        if (i < need && !ins[i]) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: input %d is NULL", i);
        if (i >= need && ins[i]) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: input %d must be NULL", i);
    }
    if (body_rot && s->kind != RTG_SOLVER_FULL_BODY_POS)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_retarget_f32: body_rot is only produced by FULL_BODY_POS");
    RTG_TRY(launch_retarget(s->kind, s->precise, s->consts, in0, in1, in2, in3, B, layout, dof, local_rot, body_rot,
                            as_stream(stream)),
            "rtg_retarget_f32 launch");
    return RTG_OK;
}

int rtg_frame_server_launch(rtg_solver_t s, const float *in, float *dof, float *local_rot, float *body_rot,
                            uint32_t *ctl, uint32_t idle_ms, rtg_stream_t stream)
{
    if (!s) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_launch: NULL solver");
    if (s->kind != RTG_SOLVER_FULL_BODY_POS)
        return fail(RTG_ERR_UNSUPPORTED, "rtg_frame_server_launch: only FULL_BODY_POS solvers are served per frame");
    if (!in || !dof || !ctl) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_launch: NULL in / dof / ctl");
    if (idle_ms == 0 || idle_ms > 60000)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_launch: idle_ms=%u (1..60000)", idle_ms);
    RTG_TRY(launch_frame_server(s->precise, s->consts, in, dof, local_rot, body_rot, ctl, (uint64_t)idle_ms * 100000u,
                                as_stream(stream)),
            "k_frame_server");
    return RTG_OK;
}

// The inbox's sequence word, stored after everything the host wrote before it and drained to the device: a device
// inbox (rtg_server_inbox_alloc) is mapped write-combining, so its stores sit in the CPU's write-combining buffers
// until a fence pushes them out (without one the device saw them 72 us - 7 ms late, tools/bar_probe.hip)
static void store_inbox_seq(float *in, uint32_t word)
{
    _mm_sfence();   // the frame's rows first (write-combined stores are not ordered by x86's TSO)
    __atomic_store_n(reinterpret_cast<uint32_t *>(in + RTG_SERVER_SEQ_WORD), word, __ATOMIC_RELEASE);
    _mm_sfence();   // ... and the word itself out now
}

// (the inbox is handed to the caller raw: no owner here)
int rtg_server_inbox_alloc(float **inbox)
{
    if (!inbox) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_server_inbox_alloc: NULL inbox");
    *inbox = nullptr;
    void *p = nullptr;
    const size_t bytes = RTG_SERVER_INBOX_FLOATS * sizeof(float);
    int rc = hip_check(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached), "hipExtMallocWithFlags(inbox)");
    if (rc != RTG_OK) return rc;
    // the host reaches device memory at its own address only on a large-BAR device (MI355X: the whole HBM is in the
    // BAR; hipPointerGetAttributes reports no separate host pointer for it); otherwise the caller keeps a pinned inbox
    int dev = 0, large_bar = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev) != hipSuccess ||
        !large_bar) {
        (void)hipGetLastError();
        (void)hipFree(p);
        return fail(RTG_ERR_UNSUPPORTED, "rtg_server_inbox_alloc: not a large-BAR device (the host cannot store into its memory)");
    }
    // zeroed by the host itself, through the BAR (no device-wide synchronize: a server may be running elsewhere)
    std::memset(p, 0, bytes);
    _mm_sfence();
    *inbox = static_cast<float *>(p);
    return RTG_OK;
}

int rtg_server_inbox_free(float *inbox)
{
    if (!inbox) return RTG_OK;
    return hip_check(hipFree(inbox), "hipFree(inbox)");
}

int rtg_frame_server_signal(float *in, uint32_t word)
{
    if (!in) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_signal: NULL inbox");
    store_inbox_seq(in, word);
    return RTG_OK;
}

int rtg_frame_server_post(uint32_t *ctl, uint32_t seq, float *in, const float *body, const float *left_hand,
                          const float *right_hand, const float *dof, const float *local_rot, const float *body_rot,
                          float *dof_dst, float *local_rot_dst, float *body_rot_dst, uint32_t timeout_us)
{
    if (!ctl || !in || !body || !left_hand || !right_hand || !dof)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_post: NULL ctl / in / inputs / dof");
    if (seq == RTG_SERVER_QUIT) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_post: seq is the quit value");
    if ((local_rot_dst && !local_rot) || (body_rot_dst && !body_rot))
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_frame_server_post: an output the server does not write");
    std::memcpy(in, body, 63 * sizeof(float));
    std::memcpy(in + 63, left_hand, 60 * sizeof(float));
    std::memcpy(in + 123, right_hand, 60 * sizeof(float));
    store_inbox_seq(in, seq);   // after the rows (the device acquires the word at system scope)
    struct timespec t0, t;
    bool timed = false;
    for (uint32_t spins = 1; __atomic_load_n(ctl + 1, __ATOMIC_ACQUIRE) != seq; ++spins) {
        if ((spins & 255u) != 0) continue;
        if (__atomic_load_n(ctl + 2, __ATOMIC_ACQUIRE) && __atomic_load_n(ctl + 1, __ATOMIC_ACQUIRE) != seq)
            return RTG_SERVER_ENDED;   // it ended on idle before it saw this frame
        clock_gettime(CLOCK_MONOTONIC, timed ? &t : &t0);
        if (!timed) { timed = true; continue; }
        const int64_t us = (int64_t)(t.tv_sec - t0.tv_sec) * 1000000 + (t.tv_nsec - t0.tv_nsec) / 1000;
        if (us > (int64_t)timeout_us) return fail(RTG_ERR_TIMEOUT, "rtg_frame_server_post: frame %u not served within %u us", seq, timeout_us);
    }
    if (dof_dst) std::memcpy(dof_dst, dof, 30 * sizeof(float));
    if (local_rot_dst) std::memcpy(local_rot_dst, local_rot, 124 * sizeof(float));
    if (body_rot_dst) std::memcpy(body_rot_dst, body_rot, 236 * sizeof(float));
    return take_device_error(ctl + 3, "rtg_frame_server_post");
}

// ---------------------------------------------------------------- primitives
int rtg_quat_op_f32(int op, const float *a, const float *b, const float *c, int64_t n, float *out,
                    rtg_stream_t stream)
{
    if (op < RTG_OP_QUAT_MUL || op > RTG_OP_PROJECT_QUAT_XZ) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_quat_op_f32: bad op %d", op);
    if (n < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_quat_op_f32: negative n");
    if (n == 0) return RTG_OK;
    const bool needs_b = op == RTG_OP_QUAT_MUL || op == RTG_OP_QUAT_MUL_NORM || op == RTG_OP_QUAT_ROTATE ||
                         op == RTG_OP_QUAT_FROM_ANGLE_AXIS || op == RTG_OP_RADIANS_BETWEEN ||
                         op == RTG_OP_PROJ_IN_PLANE || op == RTG_OP_SHOULDER_PR || op == RTG_OP_ELBOW_PY ||
                         op == RTG_OP_QUAT_SLERP;
    const bool needs_c = op == RTG_OP_RADIANS_BETWEEN || op == RTG_OP_SHOULDER_PR || op == RTG_OP_ELBOW_PY ||
                         op == RTG_OP_QUAT_SLERP;
    if (!a || !out || (needs_b && !b) || (needs_c && !c))
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_quat_op_f32: NULL operand for op %d", op);
    RTG_TRY(launch_quat_op(op, a, b, c, n, out, as_stream(stream)), "k_quat_op");
    return RTG_OK;
}

int rtg_cal_joint_quat_f32(const float *Z, const float *M, int32_t npts, int64_t n, float *out, rtg_stream_t stream)
{
    if (npts < 1 || npts > 8) return fail(RTG_ERR_UNSUPPORTED, "rtg_cal_joint_quat_f32: npts=%d (1..8)", npts);
    if (n < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_cal_joint_quat_f32: negative n");
    if (n == 0) return RTG_OK;
    if (!Z || !M || !out) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_cal_joint_quat_f32: NULL buffer");
    RTG_TRY(launch_cal_joint_quat(Z, M, npts, n, out, as_stream(stream)), "k_cal_joint_quat");
    return RTG_OK;
}

int rtg_quat_in_xyz_axis_f32(const float *q, const char *seq, int64_t n, float *out, rtg_stream_t stream)
{
    const char *fn = "rtg_quat_in_xyz_axis_f32";
    int ax[3], extrinsic;
    RTG_CHECK(parse_seq(fn, seq, ax, &extrinsic));
    if (n < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: negative n", fn);
    if (n == 0) return RTG_OK;
    if (!q || !out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    RTG_TRY(launch_quat_in_xyz_axis(q, ax[0], ax[1], ax[2], extrinsic, n, out, as_stream(stream)), "k_quat_in_xyz_axis");
    return RTG_OK;
}

int rtg_quat_as_euler_f64(const float *q, const char *seq, int degrees, int64_t n, double *out, rtg_stream_t stream)
{
    const char *fn = "rtg_quat_as_euler_f64";
    int ax[3], extrinsic;
    RTG_CHECK(parse_seq(fn, seq, ax, &extrinsic));
    if (n < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: negative n", fn);
    if (n == 0) return RTG_OK;
    if (!q || !out) return fail(RTG_ERR_INVALID_ARGUMENT, "%s: NULL buffer", fn);
    RTG_TRY(launch_quat_as_euler(q, ax[0], ax[1], ax[2], extrinsic, degrees != 0, n, out, as_stream(stream)),
            "k_quat_as_euler");
    return RTG_OK;
}

// ---------------------------------------------------------------- motion velocities
int rtg_linear_velocity_f32(const float *p, int64_t nseq, int64_t L, int64_t S, float dt, const double *w,
                            int32_t radius, float *tmp, float *out, rtg_stream_t stream)
{
    if (nseq < 0 || L < 0 || S < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_linear_velocity_f32: negative shape");
    if (nseq * L * S == 0) return RTG_OK;
    if (L < 2) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_linear_velocity_f32: np.gradient needs >= 2 frames");
    if (!p || !out || (w && !tmp)) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_linear_velocity_f32: NULL buffer");
    GaussTaps taps{};
    RTG_CHECK(make_taps(w, radius, &taps, "rtg_linear_velocity_f32"));
    RTG_TRY(launch_linear_velocity(p, nseq, L, S, dt, w ? &taps : nullptr, tmp, out, as_stream(stream)),
            "rtg_linear_velocity_f32 launch");
    return RTG_OK;
}

int rtg_angular_velocity_f32(const float *r, int64_t nseq, int64_t L, int64_t J, float dt, const double *w,
                             int32_t radius, float *tmp, float *out, rtg_stream_t stream)
{
    if (nseq < 0 || L < 0 || J < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_angular_velocity_f32: negative shape");
    if (nseq * L * J == 0) return RTG_OK;
    if (!r || !out || (w && !tmp)) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_angular_velocity_f32: NULL buffer");
    GaussTaps taps{};
    RTG_CHECK(make_taps(w, radius, &taps, "rtg_angular_velocity_f32"));
    RTG_TRY(launch_angular_velocity(r, nseq, L, J, dt, w ? &taps : nullptr, tmp, out, as_stream(stream)),
            "rtg_angular_velocity_f32 launch");
    return RTG_OK;
}

// ---------------------------------------------------------------- box probe
int rtg_box_probe(double *out, int32_t n_out, rtg_stream_t stream)
{
    if (!out || n_out < RTG_PROBE_FIELDS)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_box_probe: out needs %d doubles", RTG_PROBE_FIELDS);
    hipStream_t s = as_stream(stream);
    int dev = 0;
    hipDeviceProp_t prop{};
    RTG_TRY(hipGetDevice(&dev), "hipGetDevice");
    RTG_TRY(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
    const int nblk = prop.multiProcessorCount * 8;   // 8 workgroups of 4 waves per CU: 8 waves per SIMD
    const int nrec = (nblk + 63) / 64;
    const int64_t nf4 = (int64_t)1 << 26;             // 1 GiB per buffer: far beyond the 256 MiB Infinity Cache
    DevBuf<float> src, dst;
    DevBuf<uint64_t> clk;
    Event e0, e1;
    RTG_CHECK(src.alloc((size_t)nf4 * 4, "hipMalloc(probe)"));
    RTG_CHECK(dst.alloc((size_t)nf4 * 4, "hipMalloc(probe)"));
    RTG_CHECK(clk.alloc((size_t)nrec * 2, "hipMalloc(probe)"));
    RTG_CHECK(e0.create());
    RTG_CHECK(e1.create());
    RTG_TRY(hipMemsetAsync(src.get(), 0, nf4 * 16, s), "hipMemsetAsync");
    // one timed launch between the two events, in ms
    auto timed = [&](auto launch, const char *what, float *ms) {
        RTG_TRY(hipEventRecord(e0.get(), s), "hipEventRecord");
        RTG_TRY(launch(), what);
        RTG_TRY(hipEventRecord(e1.get(), s), "hipEventRecord");
        RTG_TRY(hipEventSynchronize(e1.get()), "hipEventSynchronize");
        RTG_TRY(hipEventElapsedTime(ms, e0.get(), e1.get()), "hipEventElapsedTime");
        return (int)RTG_OK;
    };
    float best_valu = 1e30f, best_copy = 1e30f, ms = 0.0f;
    for (int rep = 0; rep < 4; ++rep) {   // rep 0 warms up; the best of the other three counts
        RTG_CHECK(timed([&] { return launch_probe_valu(nblk, dst.get(), clk.get(), s); }, "k_probe_valu", &ms));
        if (rep > 0 && ms < best_valu) best_valu = ms;
        RTG_CHECK(timed([&] { return launch_probe_copy(src.get(), dst.get(), nf4, s); }, "k_probe_copy", &ms));
        if (rep > 0 && ms < best_copy) best_copy = ms;
    }
    uint64_t h[2 * 64] = {};
    const int nr = nrec < 64 ? nrec : 64;
    RTG_TRY(hipMemcpy(h, clk.get(), nr * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
    double mhz[64];   // shader cycles per 100 MHz tick of each recording workgroup (the last rep), median
    int m = 0;
    for (int i = 0; i < nr; ++i)
        if (h[2 * i + 1] > 0) mhz[m++] = 100.0 * (double)h[2 * i] / (double)h[2 * i + 1];
    for (int i = 1; i < m; ++i)
        for (int j = i; j > 0 && mhz[j - 1] > mhz[j]; --j) std::swap(mhz[j - 1], mhz[j]);
    out[0] = m ? mhz[m / 2] : 0.0;
    out[1] = (double)nblk * 256 * probe_valu_iters() * 8 / (best_valu * 1e-3) / 1e12;
    out[2] = 2.0 * (double)nf4 * 16 / (best_copy * 1e-3) / 1e9;
    out[3] = best_valu;
    out[4] = best_copy;
    out[5] = prop.multiProcessorCount;
    return RTG_OK;
}

// ---------------------------------------------------------------- side-kernel residency
int rtg_side_kernel_residency(int kind, int precise_gripper, int layout, int32_t *blocks_per_cu)
{
    if (!blocks_per_cu) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_side_kernel_residency: blocks_per_cu is NULL");
    if (kind < RTG_SOLVER_FULL_BODY_POS || kind > RTG_SOLVER_BODY_ROT)
        return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_side_kernel_residency: bad solver kind %d", kind);
    RTG_CHECK(check_layout("rtg_side_kernel_residency", layout));
    int n = 0;
    RTG_TRY(side_kernel_residency(kind, precise_gripper != 0, layout, &n), "hipOccupancyMaxActiveBlocksPerMultiprocessor");
    *blocks_per_cu = n;
    return RTG_OK;
}

// ---------------------------------------------------------------- synthetic input
int rtg_synth_full_body_f32(rtg_topology_t t, uint64_t seed, int64_t off, int64_t B, int layout, float *body,
                            float *lh, float *rh, float *body_rot, rtg_stream_t stream)
{
    RTG_CHECK(check_layout("rtg_synth_full_body_f32", layout));
    if (!t || t->J != 59) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_synth_full_body_f32: needs the 59-joint VTRDYN_FULL topology");
    if (B < 0 || off < 0) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_synth_full_body_f32: negative batch/offset");
    if (B == 0) return RTG_OK;
    if (!body || !lh || !rh) return fail(RTG_ERR_INVALID_ARGUMENT, "rtg_synth_full_body_f32: NULL buffer");
    RTG_TRY(launch_synth_full_body(t->view(), seed, off, B, body, lh, rh, body_rot, layout, as_stream(stream)),
            "k_synth_full_body");
    return RTG_OK;
}

}  // extern "C"

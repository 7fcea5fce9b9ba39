// rtg_kernels.cuh -- types shared by the kernels and the C-ABI layer.
#pragma once
#include "rtg_math.cuh"
#include "rtg.h"

#include <string>
#include <vector>

namespace rtg {

// One (step, sub-lane) entry of the lane-group FK schedule (group_list_schedule, rtg_group_sched.h): at step s, sub-lane u of
// every frame's lane group composes joint `code & 0xFF` (0xFF: idle) from its parent `(code >> 8) & 0xFF`, with that
// joint's zero-pose local translation and tree quaternion alongside (two ds_read_b128 per step).  The upper half of
// `code` links the joint's children for the reverse sweep (rtg_fk_grad.hip): `(code >> 16) & 0xFF` its first child,
// `(code >> 24) & 0xFF` its next sibling, both by ascending index, 0xFF for none; the forward kernels mask them off.
struct alignas(16) GEnt {
    float lx, ly, lz;
    int32_t code;
    float qx, qy, qz, qw;
};
constexpr int kGroupMaxJ = 64;   // the lane-group kernels serve J <= 64 (every shipped skeleton); larger: lane walks

// Device view of a topology (all pointers device memory, uniform per launch).
struct TopoView {
    const int32_t *parents;   // (J)   parents[j] < j, root -1
    const V *local_t;         // (J)   zero-pose local translation
    const Q *tree_quat;       // (J)   SkeletonTree pre-rotation
    int32_t J;
    const GEnt *gsched;       // (gsteps * 64 / gF) lane-group schedule, or nullptr (J > kGroupMaxJ: lane walks)
    int32_t gF;               // frames per wave of the lane-group kernels (16: J <= 36, 8: J <= 64)
    int32_t gsteps;           // steps of the lane-group schedule
};
// the lane-group frames per wave for J joints (0: J too large, the lane-walk kernels run); F J <= 64 * 9 records
inline int group_frames(int J) { return J <= RTG_FK_F16_MAXJ ? 16 : (J <= kGroupMaxJ ? 8 : 0); }
// a topology's schedule entries (rtg_fk.hip): fills `out` (steps x (64 / F) entries) and returns the step count
int32_t fk_group_schedule(const int32_t *parents, const V *local_t, const Q *tree_quat, int32_t J, int32_t F,
                          GEnt *out, int32_t max_steps);

// Per-solver constants, passed by value (kernel argument -> SGPRs).
struct SolverConsts {
    V Zt[3];          // torso Kabsch zero vectors
    V Zl[5], Zr[5];   // wrist Kabsch zero vectors
    V v0_lsh, v0_lel, v0_rsh, v0_rel;
    ArmZero lsh, lel, rsh, rel;   // theta0 / phi0, filled by k_solver_prep
    float grip_d[5];  // zero-pose x distances of the 5 finger tips to the wrist
    float orig;       // their mean (gripper denominator), filled by k_solver_prep
    int32_t par[4];   // BODY_ROT: parents of joints 18, 14, 19, 15
    int32_t torso_x0; // FULL_BODY_POS: every Zt[j].x is +-0 and |Zt| <= 2^60 (torso_quat_x0, rtg_math.cuh)
    const uint32_t *ang_tab;   // exp-map angle table (kAngTabWords words, device), owned by the solver handle
    uint32_t *err;             // host-mapped error word of the solver handle: a wave hand-over that timed out ORs
                               // RTG_DEVERR_HANDOVER_TIMEOUT in (rtg_retarget_f32 reports it on the next call)
};

// Joint-angle forward model (HuForwardModel): per-DOF axis and optional limits, device memory.
struct DofView {
    const int32_t *axis;   // (J-1) 0/1/2
    const float *lower;    // (J-1) or nullptr
    const float *upper;    // (J-1) or nullptr
};

struct FkSeg {
    TopoView T;
    const float *local_rot;   // op 1 (inverse FK): the global rotations in
    const float *root_t;      // op 1: unused
    float *g_rot;             // op 1: the local rotations out
    float *g_pos;             // op 1: unused
    int64_t B;
    int32_t op;               // 0: FK (kinematics.py:13-39), 1: inverse FK (kinematics.py:41-63)
};
struct FkMultiArgs {
    FkSeg seg[RTG_MAX_SEGMENTS];
    int64_t block_start[RTG_MAX_SEGMENTS];
    int32_t n;
};

hipError_t launch_solver_prep(SolverConsts *dev_consts, hipStream_t s);
hipError_t launch_build_ang_tab(uint32_t *tab, hipStream_t s);   // kAngTabWords words
hipError_t launch_frame_server(int precise, const SolverConsts &C, const float *in, float *dof, float *local_rot,
                               float *body_rot, uint32_t *ctl, uint64_t idle_ticks, hipStream_t s);
hipError_t launch_retarget(int kind, int precise, const SolverConsts &C, const float *in0, const float *in1,
                           const float *in2, const float *in3, int64_t B, int layout, float *dof, float *local_rot,
                           float *body_rot, hipStream_t s);
// resident blocks per CU of the k_solve_sides instantiation that launch_retarget picks for a batch beyond the small-batch
// kernels (hipOccupancyMaxActiveBlocksPerMultiprocessor)
hipError_t side_kernel_residency(int kind, int precise, int layout, int *blocks_per_cu);
hipError_t launch_fk(const TopoView &T, bool state, const float *lr, const float *rt, int64_t B, float *gr, float *gp,
                     hipStream_t s);
hipError_t launch_local_rotation(const TopoView &T, bool state, const float *g, int64_t B, float *l, hipStream_t s);
hipError_t launch_fk_multi(FkMultiArgs &A, hipStream_t s);
hipError_t launch_dof_fk(const TopoView &T, const DofView &D, bool clip, const float *dof, const float *root_rot,
                         const float *root_t, int64_t B, float *gr, float *gp, hipStream_t s);
// rtg_dof_fk_vel_f32: launch_dof_fk with the tangent sweep (link twists gv (B,J,6) from the joint velocities and the
// root twist; root_vel nullptr: zero).  Lane groups only (T.gsched); gr / gp both nullptr: velocities only
hipError_t launch_dof_fk_vel(const TopoView &T, const DofView &D, bool clip, const float *dof, const float *dof_vel,
                             const float *root_rot, const float *root_t, const float *root_vel, int64_t B, float *gr,
                             float *gp, float *gv, hipStream_t s);
// the adjoints of launch_dof_fk / launch_fk (rtg_fk_grad.hip); lq_in: the joint angles (B,J-1) when D, else the local
// rotations (B,J,4); lq_grad: their gradient rows; either upstream gradient and any output may be nullptr
hipError_t launch_fk_backward(const TopoView &T, const DofView *D, bool clip, const float *lq_in, const float *g_rot,
                              const float *grad_g_rot, const float *grad_g_pos, int64_t B, float *lq_grad,
                              float *grad_root_rot, float *grad_root_t, hipStream_t s);
// rtg_dof_fit_f32 (rtg_dof_fit.hip): the keypoint loss of the joint-angle model, its gradient and `iters` Adam steps
// in one launch; lane groups only (T.gsched).  The pointers are rtg.h's (device memory; optional ones nullptr)
struct DofFitArgs {
    const float *target_pos, *weight, *root_rot, *root_t, *dof_in;
    int64_t B;
    int32_t iters, step0;
    float lr, beta1, beta2, eps;
    float *m, *v, *dof_out, *loss, *grad;
};
hipError_t launch_dof_fit(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A, hipStream_t s);
// rtg_dof_fit_root_f32: the same launch with the floating base among the parameters.  A's root_rot / root_t are the
// start (or given) values; fit_root: RTG_FIT_ROOT_* bits; state: root_state (B,14); grad: grad_root (B,7)
struct DofFitRootArgs {
    int32_t fit_root;
    float lr_t, lr_rot;
    float *state, *rot_out, *t_out, *grad;
};
hipError_t launch_dof_fit_root(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                               const DofFitRootArgs &R, hipStream_t s);
// rtg_dof_fit_orient_f32: the root launch with orientation targets for K <= RTG_FIT_MAX_ROT_LINKS links.  joint: the
// links' joint indices (host-checked: in range, none twice), carried in the launch arguments; target_rot (B,K,4),
// rot_weight (K) or nullptr: device memory
struct DofFitOriArgs {
    const float *target_rot, *rot_weight;
    int32_t K;
    int32_t joint[RTG_FIT_MAX_ROT_LINKS];
};
hipError_t launch_dof_fit_orient(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                 const DofFitRootArgs &R, const DofFitOriArgs &O, hipStream_t s);
// rtg_dof_fit_prior_f32: the root launch (O.K == 0) or the oriented one with the posture prior and the projection.
// prior (B,J-1) or nullptr: no term; prior_weight (J-1) or nullptr: ones; flags: RTG_FIT_PROJECT (the model then has
// limits: host-checked)
struct DofFitPriorArgs {
    const float *prior, *prior_weight;
    int32_t flags;
};
hipError_t launch_dof_fit_prior(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                const DofFitRootArgs &R, const DofFitOriArgs &O, const DofFitPriorArgs &H, hipStream_t s);
// rtg_dof_fit_apart_f32: the prior launch with keep-apart spheres and a floor.  Everything travels in the launch
// arguments (host-checked: links in 0..J-1, pair ends distinct and in 0..S-1, radii and weights finite and not
// negative, the plane's normal unit, mask bits below S).  link: a sphere's joint; sphere: {offset in the link's frame,
// radius}; pair: a | b << 8; floor_mask == 0: no plane
struct DofFitApartArgs {
    int32_t S, Pn;
    uint32_t floor_mask;
    float margin, floor_weight;
    float plane[4];   // {unit normal, h0}
    int32_t link[RTG_FIT_MAX_SPHERES];
    float sphere[RTG_FIT_MAX_SPHERES][4];
    int32_t pair[RTG_FIT_MAX_PAIRS];
    float pair_weight[RTG_FIT_MAX_PAIRS];
};
hipError_t launch_dof_fit_apart(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                const DofFitRootArgs &R, const DofFitOriArgs &O, const DofFitPriorArgs &H,
                                const DofFitApartArgs &Z, hipStream_t s);
// rtg_dof_fit_robust_f32: the prior or the keep-apart launch (`apart`: Z holds a term) with per-frame keypoint weights
// and the robust keypoint loss.  frame_weight (B,J) or nullptr: ones; robust_scale 0: the quadratic loss, else delta
// (finite, > 0) with inv_d2 = (float)(1 / delta^2), formed in double by the host
struct DofFitRobustArgs {
    const float *frame_weight;
    float robust_scale, inv_d2;
};
hipError_t launch_dof_fit_robust(const TopoView &T, const DofView &D, bool clip, const DofFitArgs &A,
                                 const DofFitRootArgs &R, const DofFitOriArgs &O, const DofFitPriorArgs &H,
                                 const DofFitApartArgs &Z, bool apart, const DofFitRobustArgs &U, hipStream_t s);
// SkeletonState.retarget_to (poselib skeleton3d.py:742-889) as one launch, rtg_retarget_to.hip.
// The host tables of a mapping of K (source joint, target joint) pairs: S_red / T_red are the trees with only the
// mapped joints kept, each hung from its nearest kept ancestor (drop_nodes_by_names, :226-259).
struct RetargetTables {
    int32_t Js = 0, Jt = 0, K = 0;
    std::vector<int32_t> kept_s, kept_t;       // (K) the mapped joints of S / T, ascending: S_red / T_red's joints
    std::vector<int32_t> sred_par, tred_par;   // (K) parents in S_red / T_red (root -1)
    std::vector<int32_t> perm;                 // (K) index in S_red of the source joint mapped to T_red's k-th (:721-740)
    std::vector<int32_t> src_of;               // (Jt) index in T_red of target joint j's nearest mapped ancestor-or-self
};
// fills `out`; on a bad mapping returns false with the reason in `err`
bool retarget_tables(const int32_t *src_parents, int32_t Js, const int32_t *tgt_parents, int32_t Jt,
                     const int32_t *src_joint, const int32_t *tgt_joint, int32_t K, RetargetTables &out,
                     std::string &err);
// The plan's device blob, in 16-byte units: both list schedules, then the per-joint tables (retarget_blob).
struct RetargetView {
    const float *blob;          // device
    int32_t Js, Jt, K, F;       // F: frames per wave, group_frames(max(Js, Jt))
    int32_t steps1, steps6;     // list-schedule steps of stage 1 (S, pruned) and stage 6 (T_red)
    int32_t n16;                // the blob's size
    int32_t o_sch6, o_cg, o_tg, o_ttq, o_int;   // offsets of its parts
    Q R;                        // rotation_to_target_skeleton
    float scale;                // f32(scale_to_target_skeleton)
    V tgt_root, t_tp;           // the target t-pose's root translation; quat_rotate(R, source t-pose root)
};
// host image of the blob (constants cG / TG zeroed: filled after the t-pose pass) and the view's layout fields
void retarget_blob(const RetargetTables &T, const int32_t *src_parents, const Q *src_tq, const int32_t *tgt_parents,
                   const Q *tgt_tq, std::vector<float> &blob, RetargetView &view);
// dump != nullptr: stop after stage 6 and write the K global rotations on T_red and the rotated root translation
// (4 K + 3 floats) of frame 0 there (the t-pose pass of plan creation)
hipError_t launch_retarget_to(const RetargetView &P, bool local_in, const float *rot, const float *root_t, int64_t B,
                              float *out_rot, float *out_root_t, float *dump, hipStream_t s);
// Keypoint targets for the pose fit (rtg.h rtg_fit_targets_*; rtg_retarget_to.hip).  The host tables of a mapping of
// K (source joint, target link) pairs, numbered as given.
struct FitTargetsTables {
    int32_t Js = 0, Jt = 0, K = 0;
    int32_t levels = 0;             // the deepest pair's depth in the reduced target tree (the root pair: 0)
    std::vector<int32_t> anchor;    // (K) the pair of t_k's nearest mapped proper ancestor, -1 for the root pair
    std::vector<int32_t> depth;     // (K)
    std::vector<float> seg;         // (K,3) G[t_k] - G[t_a(k)] in float32
    std::vector<float> weight;      // (Jt)
    std::vector<int32_t> src_of;    // (Jt) the pair of link j's nearest mapped ancestor-or-self
};
bool fit_targets_tables(int32_t Js, const int32_t *tgt_parents, const float *tgt_local_t, int32_t Jt,
                        const int32_t *src_joint, const int32_t *tgt_joint, int32_t K, FitTargetsTables &out,
                        std::string &err);
// The plan's device blob: K 16-byte entries {seg, code} with code = s_k | s_a << 6 | t_k << 12 | t_a << 18 |
// depth << 24, then Jt int32 (the row an unmapped link copies, its own for a mapped one); the constants travel in the
// launch arguments
struct FitTargetsView {
    const float *blob;          // device
    int32_t Js, Jt, K, F;       // F: frames per wave, group_frames(max(Js, Jt))
    int32_t levels;
    int32_t dir_on, scale_on, offset_on;
    V dir, root_scale, root_offset;
};
void fit_targets_blob(const FitTargetsTables &T, const int32_t *src_joint, const int32_t *tgt_joint,
                      std::vector<float> &blob, FitTargetsView &view);
hipError_t launch_fit_targets(const FitTargetsView &P, const float *src_pos, int64_t B, float *target_pos, hipStream_t s);
// The zero-pose transform out[f, j] = qmul_norm(qmul_norm(q[f, src[j]], pre), post[j]) as one launch,
// rtg_rot_ingest.hip.  The handle's device blob, in 16-byte units: pre | post (J_out) | src (J_out int32, padded) | the
// near-unit table (2 kUnitTabK + 1 entries, written on the device by launch_rot_ingest_tab).
constexpr int kRotIngAosTile = RTG_ROT_INGEST_TILE_AOS, kRotIngSoaTile = RTG_ROT_INGEST_TILE_SOA;   // frames per block
constexpr int kRotIngMaxJ = 64;
struct RotIngestView {
    const float *blob;         // device
    int32_t J_in, J_out;
    int32_t n16;               // the blob's size
    int32_t o_src, o_tab;      // offsets of its parts (post is at 1)
};
// host image of the blob (the table zeroed) and the view's layout fields; src == nullptr: the identity
void rot_ingest_blob(int32_t J_in, int32_t J_out, const int32_t *src, const float *pre, const float *post,
                     std::vector<float> &blob, RotIngestView &view);
hipError_t launch_rot_ingest_tab(float *blob_tab, hipStream_t s);
hipError_t launch_rot_ingest(const RotIngestView &P, const float *q, int64_t B, int layout, float *out, hipStream_t s);
// The motion sampler (rtg_motion_sample.hip): a library's clip table, one 16-byte entry per clip (device), and the
// arguments of one launch (rtg.h's pointers; vec / vec_out, g_rot / g_pos nullptr when not asked for).
struct alignas(16) MotionClip {
    int64_t start;   // first row of the clip in the packed arrays
    int32_t len;     // frames, >= 1
    float fps;       // finite, > 0
};
struct MotionLibView {
    const MotionClip *clips;   // device, (C)
    int32_t C;
};
struct MotionSampleArgs {
    const float *rot, *root_t, *vec;
    int32_t K;
    const int32_t *clip;
    const float *time;
    int64_t N;
    float *local_rot_out, *root_t_out, *vec_out, *g_rot, *g_pos;
};
// lane groups only (T.gsched); g_rot / g_pos are written iff `global`, as rtg_state_fk_f32 (`state`) or rtg_fk_f32
hipError_t launch_motion_sample(const TopoView &T, const MotionLibView &L, bool normalize, bool global, bool state,
                                const MotionSampleArgs &A, hipStream_t s);
// rtg_dof_motion_sample_f32: a library of joint-angle clips (dof (F_total,J-1), root_rot (F_total,4), root_t
// (F_total,3)) on the same clip table.  dof_vel_out / root_vel_out, g_rot / g_pos and key_pos nullptr when not asked
// for; key: the K <= RTG_DOF_MOTION_MAX_KEY_LINKS link indices (host-checked: in 0..J-1), carried in the launch
// arguments
struct DofMotionArgs {
    const float *dof, *root_rot, *root_t;
    const int32_t *clip;
    const float *time;
    int64_t N;
    int32_t normalize, K;
    uint8_t key[RTG_DOF_MOTION_MAX_KEY_LINKS];
    float *dof_out, *dof_vel_out, *root_rot_out, *root_t_out, *root_vel_out, *g_rot, *g_pos, *key_pos;
};
// lane groups only (T.gsched); the forward kinematics runs iff g_rot or key_pos is given
hipError_t launch_dof_motion_sample(const TopoView &T, const DofView &D, const MotionLibView &L, bool clip,
                                    const DofMotionArgs &A, hipStream_t s);
// rtg_dof_motion_sample_vel_f32: the same launch with the link twists of the sampled state (g_vel (N,J,6) and / or
// key_vel (N,K,6), at least one given; A.dof_vel_out / A.root_vel_out are then given too).  The forward kinematics
// always runs
struct DofMotionVelArgs {
    DofMotionArgs A;
    float *g_vel, *key_vel;
};
hipError_t launch_dof_motion_sample_vel(const TopoView &T, const DofView &D, const MotionLibView &L, bool clip,
                                        const DofMotionVelArgs &A, hipStream_t s);
hipError_t launch_rescale_motion(const TopoView &T, const float *motion, int64_t B, const float *dir, float *out,
                                 hipStream_t s);
hipError_t launch_quat_between(const float *v1, const float *v2, int64_t n, float *out, float *ws, hipStream_t s);
hipError_t launch_rebuild_vtrdyn(const TopoView &T, const float *motion, int64_t B, float *g_rot, float *root_t,
                                 float *ws, hipStream_t s);
hipError_t launch_ingest_vtrdyn(const float *bp, const float *lhp, const float *rhp, int64_t B, int layout,
                                float *body, float *lh, float *rh, uint8_t *valid, hipStream_t s);
hipError_t launch_quat_op(int op, const float *a, const float *b, const float *c, int64_t n, float *out,
                          hipStream_t s);
hipError_t launch_cal_joint_quat(const float *Z, const float *M, int npts, int64_t n, float *out, hipStream_t s);
hipError_t launch_quat_as_euler(const float *q, int s0, int s1, int s2, int extrinsic, int degrees, int64_t n,
                               double *out, hipStream_t s);
hipError_t launch_quat_in_xyz_axis(const float *q, int s0, int s1, int s2, int extrinsic, int64_t n, float *out,
                                   hipStream_t s);
struct GaussTaps {
    double w[2 * RTG_MAX_FILTER_RADIUS + 1];
    int32_t radius;
};
hipError_t launch_linear_velocity(const float *p, int64_t nseq, int64_t L, int64_t S, float dt, const GaussTaps *taps,
                                  float *tmp, float *out, hipStream_t s);
hipError_t launch_angular_velocity(const float *r, int64_t nseq, int64_t L, int64_t J, float dt,
                                   const GaussTaps *taps, float *tmp, float *out, hipStream_t s);
hipError_t launch_synth_full_body(const TopoView &T, uint64_t seed, int64_t off, int64_t B, float *body, float *lh,
                                  float *rh, float *body_rot, int layout, hipStream_t s);
hipError_t launch_probe_valu(int nblocks, float *sink, uint64_t *clk, hipStream_t s);
hipError_t launch_probe_copy(const float *src, float *dst, int64_t nfloat4, hipStream_t s);
int probe_valu_iters();

}  // namespace rtg

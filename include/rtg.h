/*
 * rtg.h -- C ABI of the MI355X-native retargeting hot path (librtg_hip.so).
 *
 * The reference (shuoshuof/Humanoid-Real-Time-Retarget) has no native
 * boundary: its operator API is the set of Python classes / TorchScript
 * functions called in-process on CPU float32 tensors.  Each entry point below
 * replaces one of those (cited per function); the Python drop-in modules in
 * humanoid-real-time-retarget_amd/{retarget,robot_kinematics_model,poselib}
 * bind them with ctypes.
 *
 * Conventions
 *  - quaternions are [x, y, z, w] float32 (poselib/poselib/core/rotation3d.py:14-27);
 *  - every pointer argument is a caller-owned DEVICE pointer (hipMalloc / torch
 *    device tensor), C-contiguous, float32 unless stated; the library never
 *    frees caller memory and never allocates in a launch call;
 *  - launches are stream-ordered on `stream` (a hipStream_t; NULL = default
 *    stream) and thread-safe across distinct streams; nothing synchronises;
 *  - every call returns an rtg_status; on failure rtg_last_error() returns a
 *    thread-local message.  Argument errors mirror the reference's Python
 *    assertions (e.g. proj_in_plane's |n| > 1e-6, transform3d.py:70).
 */
#ifndef RTG_H
#define RTG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTG_ABI_VERSION 7   /* 7: the zero-pose transform of mocap rotations (rtg_rot_ingest_*); rtg_dof_fit_f32,
                                  rtg_dof_fit_root_f32, rtg_dof_fit_orient_f32, rtg_dof_fit_prior_f32, rtg_dof_fit_apart_f32, rtg_dof_fit_robust_f32, rtg_dof_motion_sample_f32, rtg_dof_fk_vel_f32 and rtg_dof_motion_sample_vel_f32 came later as new symbols only -- nothing that existed changed, so the version stays 7;
                               6: SkeletonState.retarget_to (rtg_retarget_plan_*, rtg_retarget_to_f32);
                               5: the kinematics' gradients (rtg_dof_fk_backward_f32, rtg_fk_backward_f32);
                               4: the frame server's sequence word lives in its inbox (in[RTG_SERVER_SEQ_WORD]; ctl[0]
                                  reserved), the inbox may be device memory (rtg_server_inbox_alloc), rtg_frame_server_signal;
                               3: frames the reference raises on are marked (rtg_frame_error), the solver error word, ctl[3];
                               2: the input-layout argument of rtg_retarget_f32 / rtg_ingest_vtrdyn_f32 / rtg_synth_full_body_f32 */

typedef enum rtg_status {
    RTG_OK = 0,
    RTG_ERR_INVALID_ARGUMENT = 1,
    RTG_ERR_DEVICE = 2,          /* a HIP runtime call failed */
    RTG_ERR_OUT_OF_MEMORY = 3,
    RTG_ERR_UNSUPPORTED = 4,
    RTG_ERR_TIMEOUT = 5,         /* rtg_frame_server_post: the frame was not served in time */
    RTG_SERVER_ENDED = 6         /* rtg_frame_server_post: the server ended (idle) before it took the frame */
} rtg_status;

/* Frame-batch layout of solver inputs.  AOS: the reference's (B, P, C) rows (e.g. body
 * (B,21,3)), what sim_full_body_teleop.py:109-119 hands over.  SOA: component planes (P, C, B) -- element
 * (frame f, point j, component c) at [(j*C + c)*B + f] -- so a wavefront's load of one component of 64
 * consecutive frames is one 256-byte contiguous read.  The batched producers (ingest, synth) emit either. */
typedef enum rtg_layout { RTG_LAYOUT_AOS = 0, RTG_LAYOUT_SOA = 1 } rtg_layout;

typedef struct rtg_topology_s *rtg_topology_t;
typedef struct rtg_solver_s *rtg_solver_t;
typedef void *rtg_stream_t; /* hipStream_t */

/* Library / error handling. */
int rtg_abi_version(void);
const char *rtg_last_error(void);
/* Number of visible devices (0 when no GPU / driver). */
int rtg_device_count(void);
/* The compile-time configuration of this library as a JSON object: every RTG_* build knob and its value, and
 * "wrong_answer_knobs" = 1 when any measurement-only knob that changes results is on (RTG_EXP_STUB_SVD, _NO_TABLE,
 * _HOT_INPUTS, _FK_COPY, _FK_NOPOS, _MULR_NOBRANCH, _TIMESTAMPS, _SKIP_SIGNAL).  A product library has 0; the Python
 * binding refuses any other. */
const char *rtg_build_info(void);

/* ------------------------------------------------------------------------
 * Topology: a parent-indexed skeleton (SkeletonTree, skeleton3d.py:83-96;
 * RobotZeroPose, robot_kinematics_model/base_robot.py:24-58).
 * parents[J] (root = -1, parents[j] < j), local_t[J*3] zero-pose local
 * translation, tree_quat[J*4] the SkeletonTree pre-rotation (NULL = identity).
 * Host pointers; the data is copied to device memory owned by the handle.
 * ---------------------------------------------------------------------- */
int rtg_topology_create(const int32_t *parents, const float *local_t, const float *tree_quat, int32_t J,
                        rtg_topology_t *out);
int rtg_topology_destroy(rtg_topology_t topo);
int rtg_topology_num_joints(rtg_topology_t topo);

/* ------------------------------------------------------------------------
 * Kinematics
 * ---------------------------------------------------------------------- */
/* cal_forward_kinematics (robot_kinematics_model/kinematics.py:13-39).
 * local_rot (B,J,4), root_t (B,3) -> g_rot (B,J,4), g_pos (B,J,3). */
int rtg_fk_f32(rtg_topology_t topo, const float *local_rot, const float *root_t, int64_t B, float *g_rot,
               float *g_pos, rtg_stream_t stream);
/* cal_local_rotation (kinematics.py:41-63). g_rot (B,J,4) -> local_rot (B,J,4). */
int rtg_local_rotation_f32(rtg_topology_t topo, const float *g_rot, int64_t B, float *local_rot,
                           rtg_stream_t stream);
/* SkeletonState.global_transformation (poselib skeleton3d.py:402-425): FK with the
 * tree pre-rotation; local_rot must hold the state's (normalised) rotations. */
int rtg_state_fk_f32(rtg_topology_t topo, const float *local_rot, const float *root_t, int64_t B, float *g_rot,
                     float *g_pos, rtg_stream_t stream);
/* SkeletonState.local_rotation (skeleton3d.py:460-484): inverse FK incl. tree-quat fix-up. */
int rtg_state_local_rotation_f32(rtg_topology_t topo, const float *g_rot, int64_t B, float *local_rot,
                                 rtg_stream_t stream);

/* Mixed-target FK: up to RTG_MAX_SEGMENTS independent (topology, frame batch)
 * segments in ONE launch (BASELINE config 5). */
#define RTG_MAX_SEGMENTS 8
typedef struct rtg_fk_segment {
    rtg_topology_t topo;
    const float *local_rot; /* (B,J,4) */
    const float *root_t;    /* (B,3)   */
    float *g_rot;           /* (B,J,4) */
    float *g_pos;           /* (B,J,3) */
    int64_t B;
} rtg_fk_segment;
int rtg_fk_multi_f32(const rtg_fk_segment *segments, int32_t n_segments, rtg_stream_t stream);
/* Mixed-target inverse FK (cal_local_rotation, kinematics.py:41-63): up to RTG_MAX_SEGMENTS (topology, batch)
 * segments in one launch. */
typedef struct rtg_local_rotation_segment {
    rtg_topology_t topo;
    const float *g_rot;     /* (B,J,4) */
    float *local_rot;       /* (B,J,4) */
    int64_t B;
} rtg_local_rotation_segment;
int rtg_local_rotation_multi_f32(const rtg_local_rotation_segment *segments, int32_t n_segments, rtg_stream_t stream);
/* FK segments and inverse-FK segments together in ONE launch (BASELINE config 5: "FK plus inverse FK" on the
 * four robot_config skeletons); n_fk + n_inv <= RTG_MAX_SEGMENTS. */
int rtg_kinematics_multi_f32(const rtg_fk_segment *fk, int32_t n_fk, const rtg_local_rotation_segment *inv,
                             int32_t n_inv, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Joint-angle forward model: HuForwardModel (robot_kinematics_model/
 * hu_forward_model.py:13-33).  A topology plus one rotation axis per DOF
 * (J-1 entries, 0=x 1=y 2=z: torch.eye(3)[Hu_DOF_AXIS], :16) and optional
 * DOF limits (J-1 each; both NULL = none).  Host pointers, copied.
 * ---------------------------------------------------------------------- */
typedef struct rtg_dof_model_s *rtg_dof_model_t;
int rtg_dof_model_create(rtg_topology_t topo, const int32_t *axis, const float *lower, const float *upper,
                         rtg_dof_model_t *out);
int rtg_dof_model_destroy(rtg_dof_model_t model);
/* forward_kinematics(motion_joint_angles (B,J-1), motion_root_translation (B,3),
 * motion_root_rotation (B,4), clip_angles) -> g_rot (B,J,4), g_pos (B,J,3).
 * clip != 0 applies a' = (clamp(a, lower, upper) - a) + a (:27-33) and needs limits.
 * local[j] = quat_from_angle_axis(a'[j-1], axis[j-1]) (:21-23), local[0] = root rotation (:24). */
int rtg_dof_fk_f32(rtg_dof_model_t model, const float *dof, const float *root_rot, const float *root_t, int64_t B,
                   int clip, float *g_rot, float *g_pos, rtg_stream_t stream);
/* Link velocities from joint velocities: rtg_dof_fk_f32 with a tangent sweep down the tree, in one launch -- the
 * forward-mode counterpart of rtg_dof_fk_backward_f32.  Per frame: the angles a (J-1), the joint velocities
 * ad = dof_vel (J-1), the root rotation (used as given) and translation, and the root twist root_vel = {v0 (3), w0 (3)},
 * linear then angular, both in the world frame (rtg_dof_motion_sample_f32's root_vel_out layout; NULL: zero).
 * -> g_vel (B,J,6) = {v_j (3), w_j (3)}: the world-frame linear velocity of link j's origin and its angular velocity.
 * With G, P the g_rot, g_pos of rtg_dof_fk_f32 on the same inputs and clip flag, l_j joint j's local translation,
 * e_j the unit axis of DOF j-1 and p the parent of j, every operation ONE float32 rounding and no FMA:
 *   - row 0 is the six floats of root_vel bit for bit (+0 when root_vel is NULL);
 *   - r   = RTG_OP_QUAT_ROTATE(G_p, l_j): the value the FK step adds to P_p (P_j - P_p does not have these bits);
 *   - c   = w_p x r as  c.x = (w.y r.z) - (w.z r.y),  c.y = (w.z r.x) - (w.x r.z),  c.z = (w.x r.y) - (w.y r.x):
 *           two products and their difference per component (not torch.cross's fused form);
 *   - v_j = v_p + c;
 *   - u   = RTG_OP_QUAT_ROTATE(G_j, e_j), with the joint's OWN global rotation;
 *   - w_j = w_p + (u * s), a product then a sum per component, with s = ad[j-1] -- and with clip != 0
 *           s = (a[j-1] < lower[j-1] || a[j-1] > upper[j-1]) ? +0.0f : ad[j-1].
 * With clip the velocity is the derivative of the pose that is put out: a joint held at a limit does not turn.  (It is
 * not the straight-through gradient of rtg_dof_fk_backward_f32.)  A NaN angle keeps ad (its rows are NaN anyway), an
 * angle exactly at a limit keeps ad.  For a unit root rotation this is the exact tangent of the model; a non-unit
 * root rotation scales r exactly as it scales g_pos.  A frame's NaN / inf stays in that frame's rows.
 * g_vel is required.  g_rot and g_pos are given together -- then they are rtg_dof_fk_f32's bits -- or both NULL: a
 * velocity-only call with the same g_vel bits.  root_rot and g_rot rows are 16-byte aligned; no output overlaps an
 * input or another output.  A one-joint model has no angles: dof and dof_vel are then not dereferenced and may be
 * NULL.  Never allocates or synchronises; B == 0 is a no-op after the argument checks.  A model of more than 64 joints
 * is RTG_ERR_UNSUPPORTED; every other rejection -- B < 0, a NULL handle or buffer, g_rot without g_pos, clip on a model
 * without limits, a misaligned or overlapping buffer -- is RTG_ERR_INVALID_ARGUMENT, decided before any HIP call,
 * with the reason in rtg_last_error(). */
int rtg_dof_fk_vel_f32(rtg_dof_model_t model, const float *dof, const float *root_rot, const float *root_t,
                       const float *dof_vel, const float *root_vel /* (B,6) or NULL */, int64_t B, int clip,
                       float *g_rot, float *g_pos, float *g_vel, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Gradients of the kinematics.  The reference's FK is plain torch, so a loss on its outputs back-propagates to the
 * joint angles / local rotations; these are the same vector-Jacobian products as one launch each.  g_rot is the
 * SAVED OUTPUT of the forward call on the same inputs (nothing else of the forward is kept).  grad_g_rot (B,J,4) /
 * grad_g_pos (B,J,3) are the upstream gradients; either may be NULL (taken as zero, not read), not both.  Every
 * output may be NULL (not written), not all.  The root rotation is taken as given (unnormalised), the normalisation
 * of every other joint and quat_rotate's |q|^2 scaling are differentiated as torch does.  Results are bit-identical
 * from run to run; a frame's NaN / inf stays in that frame's rows.  B == 0 is a no-op (no pointer is looked at).
 * ---------------------------------------------------------------------- */
/* rtg_dof_fk_f32's adjoint: dof (B,J-1) and clip as in the forward call.  The clip is straight-through
 * (hu_forward_model.py:27-33): the local rotations are built from the clamped angles, the gradient passes unchanged.
 * -> grad_dof (B,J-1), grad_root_rot (B,4), grad_root_t (B,3). */
int rtg_dof_fk_backward_f32(rtg_dof_model_t model, const float *dof, const float *g_rot, const float *grad_g_rot,
                            const float *grad_g_pos, int64_t B, int clip, float *grad_dof, float *grad_root_rot,
                            float *grad_root_t, rtg_stream_t stream);
/* rtg_fk_f32's adjoint (not rtg_state_fk_f32's): local_rot (B,J,4) as in the forward call (it may be non-unit).
 * -> grad_local_rot (B,J,4) (row 0: the root rotation's gradient), grad_root_t (B,3). */
int rtg_fk_backward_f32(rtg_topology_t topo, const float *local_rot, const float *g_rot, const float *grad_g_rot,
                        const float *grad_g_pos, int64_t B, float *grad_local_rot, float *grad_root_t,
                        rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Fit joint angles to target keypoints: the loop a caller of the differentiable joint-angle model runs (a keypoint
 * loss minimised over the angles with torch.optim.Adam), as ONE launch.  Per frame f
 *     L_f = sum_j weight[j] |P_j(a_f) - target_pos[f,j]|^2,
 * P the g_pos of rtg_dof_fk_f32 on the same model, root and clip (float32 arithmetic with the device sincosf, not the
 * forward call's bit-exact one; the clip is straight-through, hu_forward_model.py:27-33).  The call takes `iters`
 * steps of Adam (no weight decay, no amsgrad) on the angles, k = 1..iters, t = step0 + k, g = dL_f/da_f:
 *     m = beta1 m + (1 - beta1) g,  v = beta2 v + (1 - beta2) g^2,
 *     a -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps).
 * The iterate is not projected onto the limits (like the torch loop: the final pose is the clamp the caller applies);
 * rtg_dof_fit_prior_f32's RTG_FIT_PROJECT projects it after every step.
 * iters == 0 is the fused evaluate-only call.
 *   target_pos (B,J,3); weight (J) or NULL = all 1; root_rot (B,4), root_t (B,3): given, not fitted;
 *   dof_in (B,J-1) the start; step0: Adam steps already taken; m, v (B,J-1): the moments, read and written in place --
 *   both NULL = start at 0 and do not write them;
 *   -> dof_out (B,J-1) (may alias dof_in), loss (B) and grad (B,J-1): the loss and its gradient AT dof_out (one more
 *   sweep after the last step; with iters == 0 that is at dof_in).  Each output may be NULL, not all three.
 * A DOF whose subtree carries no weight (a leaf joint's DOF among them: a leaf's rotation moves no position) gets a
 * gradient of exactly +-0, and from a zero state its angle keeps its bits.  A frame's results depend on that frame's
 * rows alone: not on the batch, the tile, or another frame's NaN / inf; runs are bit-identical, and one launch of n
 * steps equals n launches of one step that carry (m, v, step0).
 * Errors: iters outside 0..4096, step0 < 0, lr / betas / eps not finite, betas outside [0, 1), exactly one of m, v
 * NULL, clip without limits -> RTG_ERR_INVALID_ARGUMENT; more than 64 joints -> RTG_ERR_UNSUPPORTED.  B == 0 is a
 * no-op.
 * ---------------------------------------------------------------------- */
#define RTG_DOF_FIT_MAX_ITERS 4096   /* bounds one launch's run time */
int rtg_dof_fit_f32(rtg_dof_model_t model, const float *target_pos, const float *weight, const float *root_rot,
                    const float *root_t, const float *dof_in, int64_t B, int clip, int32_t iters, float lr, float beta1,
                    float beta2, float eps, int32_t step0, float *m, float *v, float *dof_out, float *loss, float *grad,
                    rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * rtg_dof_fit_f32 with the floating base among the parameters (a new symbol under ABI 7): per frame the angles a, and
 * -- selected by the fit_root bit mask -- the root translation t (3) and the root rotation q (4, [x, y, z, w]).  Mocap
 * keypoints come from a body of other proportions; with the root pinned the legs cannot reach them.
 *   A block whose bit is clear is given, exactly as in rtg_dof_fit_f32 (a given rotation is used unnormalised).
 *   RTG_FIT_ROOT_ROT: the forward model uses G_0 = q / max(|q|, 1e-9) -- no sign flip, q and -q are one rotation and
 *   the iterate stays continuous; the gradient goes through that normalisation (it is tangent: (g - (g.G_0) G_0) / |q|)
 *   and after each Adam step q is renormalised the same way: root_rot_out is unit, and feeding it back continues the
 *   run.  RTG_FIT_ROOT_T: dL/dt = sum_j 2 weight[j] (P_j - target_pos[f,j]), the root's own residual included.
 * Loss, Adam formulas, bias corrections, step0, the iters cap and the clip are rtg_dof_fit_f32's; the three blocks
 * have their own step sizes lr (angles), lr_root_t, lr_root_rot and share betas and eps: torch.optim.Adam with three
 * parameter groups.
 *   root_rot (B,4), root_t (B,3): the start, or the given values; root_state (B,14): the root's moments {m_t(3),
 *   m_q(4), v_t(3), v_q(4)}, read and written in place -- NULL exactly when m and v are NULL (start at 0, not written);
 *   with fit_root == 0 it is neither read nor written;
 *   -> dof_out, loss, grad as in rtg_dof_fit_f32; root_rot_out (B,4), root_t_out (B,3) (they may alias the inputs;
 *   with iters == 0, or for a given block, they carry the input's bits); grad_root (B,7) = {dL/dt, dL/dq} at the
 *   outputs -- for a given rotation dL/dq is that of the unnormalised model, as rtg_dof_fk_backward_f32 reports it.
 *   Each output may be NULL, not all six.  root_rot and root_rot_out are 16-byte aligned rows.  A one-joint model
 *   has no angles: dof_in, dof_out, grad, m and v are not dereferenced (m, v still say whether a state is given).
 * rtg_dof_fit_f32's guarantees hold: a frame depends on its own rows alone, runs are bit-identical, n launches of one
 * step that carry (m, v, root_state, step0) equal one launch of n steps, DOFs over zero-weight subtrees keep their
 * bits; with every weight zero a fitted t keeps its bits; and fit_root == 0 gives rtg_dof_fit_f32's outputs bit for bit.
 * Errors: rtg_dof_fit_f32's, and unknown fit_root bits, lr_root_* not finite or negative, root_state given without
 * m, v or the reverse -> RTG_ERR_INVALID_ARGUMENT; more than 64 joints -> RTG_ERR_UNSUPPORTED.  B == 0 is a no-op.
 * ---------------------------------------------------------------------- */
#define RTG_FIT_ROOT_T 1     /* fit the root translation */
#define RTG_FIT_ROOT_ROT 2   /* fit the root rotation */
int rtg_dof_fit_root_f32(rtg_dof_model_t model, const float *target_pos, const float *weight, const float *root_rot,
                         const float *root_t, const float *dof_in, int64_t B, int clip, int32_t fit_root, int32_t iters,
                         float lr, float lr_root_t, float lr_root_rot, float beta1, float beta2, float eps,
                         int32_t step0, float *m, float *v, float *root_state, float *dof_out, float *root_rot_out,
                         float *root_t_out, float *loss, float *grad, float *grad_root, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * rtg_dof_fit_root_f32 with orientation targets for K chosen links (a new symbol under ABI 7).  Positions alone cannot
 * pose a leaf joint (its rotation moves no keypoint) nor the twist of a link about the line through its keypoints;
 * here link rot_joint[k] is also pulled towards the global rotation target_rot[f,k].  Per frame f
 *     L_f = sum_j weight[j] |P_j - target_pos[f,j]|^2 + sum_k rot_weight[k] 4 (1 - c_k^2),
 *     c_k = <G_j, Rh_fk>,  j = rot_joint[k],  Rh_fk = target_rot[f,k] / max(|target_rot[f,k]|, 1e-9) (no sign flip),
 * G_j the global rotation of link j as the forward model holds it (unit below the root; the root's G_0 is
 * q / max(|q|, 1e-9) where RTG_FIT_ROOT_ROT is set, else q as given).  4 (1 - c^2) = (2 sin(theta/2))^2 for the
 * angle theta between the two rotations: it does not see the sign of either quaternion and is theta^2 to second
 * order, so rot_weight reads "per rad^2" next to weight's "per m^2".  It is stationary at theta = pi as well as at
 * 0: a link exactly half a turn from its target gets no pull from this term.  Its gradient enters the reverse sweep
 * as dL/dG_j = -8 rot_weight[k] c_k Rh_fk; everything else -- Adam, the three step sizes, the root's normalisation,
 * step0, the clip, the outputs -- is rtg_dof_fit_root_f32's.  An oriented root (rot_joint[k] == 0) that is given, not
 * fitted, adds to the loss and to grad_root's dL/dq (of the unnormalised model) and moves nothing.
 *   rot_joint (K): joint indices, a HOST pointer, read before the call returns (the launch carries the K <= 8 values
 *   in its arguments, so the call neither allocates nor synchronises, and they are checked here: in 0..J-1, none
 *   twice); target_rot (B,K,4) [x, y, z, w], device memory, 16-byte aligned; rot_weight (K) device memory, or
 *   NULL = all 1; 0 <= K <= RTG_FIT_MAX_ROT_LINKS.  With K == 0 the three pointers are not looked at.
 * Guarantees: K == 0 gives rtg_dof_fit_root_f32's outputs bit for bit (so fit_root == 0 with K == 0 gives
 * rtg_dof_fit_f32's).  A DOF gets a gradient of exactly +-0, and from a zero state keeps its bits, when its strict
 * subtree carries no position weight and its subtree, its own link included, holds no oriented link (a link with
 * rot_weight 0 still counts as oriented).  A frame depends on its own rows alone (not on the batch, the tile or
 * another frame's NaN / inf), runs are bit-identical, and n launches of one step that carry (m, v, root_state, step0)
 * equal one launch of n steps.  A zero target row has Rh = 0: it adds the constant 4 rot_weight[k] and no gradient; a
 * NaN row makes that frame's loss and gradients NaN -- in both cases exactly where the float32 restatement of the
 * formula above does, and in no other frame.
 * Errors: rtg_dof_fit_root_f32's, and K < 0, K > 0 with rot_joint or target_rot NULL, target_rot not 16-byte
 * aligned, a joint index outside 0..J-1 or listed twice -> RTG_ERR_INVALID_ARGUMENT; K > RTG_FIT_MAX_ROT_LINKS ->
 * RTG_ERR_UNSUPPORTED; all before any device work.  B == 0 is a no-op.
 * ---------------------------------------------------------------------- */
#define RTG_FIT_MAX_ROT_LINKS 8   /* the links' target rows share the tile's LDS */
int rtg_dof_fit_orient_f32(rtg_dof_model_t model, const float *target_pos, const float *weight,
                           const int32_t *rot_joint, const float *target_rot, const float *rot_weight, int32_t K,
                           const float *root_rot, const float *root_t, const float *dof_in, int64_t B, int clip,
                           int32_t fit_root, int32_t iters, float lr, float lr_root_t, float lr_root_rot, float beta1,
                           float beta2, float eps, int32_t step0, float *m, float *v, float *root_state,
                           float *dof_out, float *root_rot_out, float *root_t_out, float *loss, float *grad,
                           float *grad_root, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * rtg_dof_fit_orient_f32 with a posture prior on the angles and, on request, the iterate projected onto the joint
 * limits (a new symbol under ABI 7).  A DOF that no target observes, or the swivel of a redundant chain, has nothing
 * to hold it; the prior holds it to a rest pose, to the previous frame's solution or to a clip's smoothed neighbours.
 * Per frame f
 *     L_f = rtg_dof_fit_orient_f32's loss + sum_d prior_weight[d] (a_{f,d} - prior[f,d])^2,
 * a the ITERATE (the parameter), not the clamped angle the forward model uses under `clip`: the term pulls an iterate
 * that ran past a limit back.  Its gradient 2 prior_weight[d] (a - prior) is added to dL/da_d before the Adam step;
 * loss and grad at dof_out include the term.
 *   prior (B,J-1) device memory, or NULL: the term is absent (not zero times something); it may alias dof_in or
 *   dof_out ("stay near where you started": a tile reads its own rows before it writes them).  prior_weight (J-1)
 *   device memory, or NULL = all 1; it needs prior.
 *   flags: RTG_FIT_PROJECT -- after each Adam step of an angle, a <- a < lower ? lower : (a > upper ? upper : a)
 *   (torch.clamp: NaN passes).  The moments are not touched: this is the loop `opt.step(); a.clamp_(lower, upper)`.
 *   It needs a model with limits, whatever `clip` is.  iters == 0 projects nothing: dof_out carries dof_in's bits.
 *   Everything else is rtg_dof_fit_orient_f32's.  The root is not regularised here: weight[0] with target_pos[f,0]
 *   is a prior on its translation, an orientation target on joint 0 one on its rotation.
 * Guarantees: (a) prior == NULL with flags == 0 gives rtg_dof_fit_orient_f32's outputs bit for bit.  (b) With
 * prior_weight all zero and finite inputs every output equals (a)'s as a number (a zero may change sign).  (c) A DOF
 * to which rtg_dof_fit_orient_f32 gives a gradient of +-0 gets exactly fl(2 prior_weight[d]) * fl(a - prior) in
 * float32, one rounding each; with prior_weight[d] == 0 it still gets +-0 and from a zero state keeps its bits.
 * (d) A frame depends on its own rows alone, runs are bit-identical (the loss keeps one summation order), and n
 * launches of one step that carry (m, v, root_state, step0) equal one launch of n steps, with and without the
 * projection.  (e) After a launch with RTG_FIT_PROJECT and iters >= 1 every angle of dof_out that is not NaN lies in
 * [lower, upper] exactly.  (f) A NaN prior row makes that frame's loss and gradient NaN, and no other frame's.
 * Errors: rtg_dof_fit_orient_f32's, and unknown flags bits, prior_weight without prior, RTG_FIT_PROJECT on a model
 * without limits -> RTG_ERR_INVALID_ARGUMENT; all before any device work.  For a one-joint model neither pointer is
 * dereferenced.  B == 0 is a no-op.
 * ---------------------------------------------------------------------- */
#define RTG_FIT_PROJECT 1   /* clamp each angle to its limits after its Adam step */
int rtg_dof_fit_prior_f32(rtg_dof_model_t model, const float *target_pos, const float *weight,
                          const int32_t *rot_joint, const float *target_rot, const float *rot_weight, int32_t K,
                          const float *prior, const float *prior_weight, int32_t flags, const float *root_rot,
                          const float *root_t, const float *dof_in, int64_t B, int clip, int32_t fit_root,
                          int32_t iters, float lr, float lr_root_t, float lr_root_rot, float beta1, float beta2,
                          float eps, int32_t step0, float *m, float *v, float *root_state, float *dof_out,
                          float *root_rot_out, float *root_t_out, float *loss, float *grad, float *grad_root,
                          rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * rtg_dof_fit_prior_f32 with keep-apart spheres and a floor (a new symbol under ABI 7).  Every other term pulls the
 * robot towards something; keypoints of a body of other proportions then leave a wrist inside the torso, one gripper
 * inside the other or an ankle under the ground.  Here up to RTG_FIT_MAX_SPHERES spheres ride on links, up to
 * RTG_FIT_MAX_PAIRS pairs of them are pushed apart where they overlap, and spheres chosen by a mask are pushed out
 * of one half-space.  Sphere s sits on link j_s = sphere_link[s] with offset o_s in the link's frame and radius r_s:
 *     c_s = P_j + rot(G_j, o_s),  rot(q, v) = q v conj(q) as the forward model applies it to bone offsets,
 * G_j the global rotation as the forward model holds it (the root's: rtg_dof_fit_orient_f32's rule).  Per frame f
 *     L_f = rtg_dof_fit_prior_f32's loss + sum_p pair_weight[p] h_p^2 + sum_{s in floor_mask} floor_weight hf_s^2,
 *     h_p = max(0, r_a + r_b + margin - |c_a - c_b|) for pair p = (a, b),  hf_s = max(0, r_s + h0 - n . c_s)
 * for the plane {n, h0} (n . x = h0 is the floor, n points up out of it).  dL/dc_a of a pair is
 * -2 pair_weight[p] h_p (c_a - c_b) / max(|c_a - c_b|, 1e-9) and dL/dc_b its negative; the floor gives
 * -2 floor_weight hf_s n.  A sphere's g_s = dL/dc_s is the sum of its pairs' terms in pair order, then the floor's;
 * dL/dP_j gains sum g_s over the link's spheres in sphere order and dL/dG_j gains sum_s d(g_s . rot(G_j, o_s)) / dG_j,
 * which enters the reverse sweep where an orientation target's adjoint does.  A sphere with a zero offset adds no
 * rotation term at all.  Everything else -- Adam, the prior, the projection, the outputs -- is
 * rtg_dof_fit_prior_f32's.
 *   apart: a HOST struct, read before the call returns (its values travel in the launch's arguments, so the call
 *   neither allocates nor synchronises, and they are checked here); NULL: no term.  sphere_link (S) joint indices in
 *   0..J-1 (a link may carry several spheres); sphere (S,4) rows {o_x, o_y, o_z, r}, r >= 0; pair (Pn,2) sphere
 *   indices, a != b; pair_weight (Pn) >= 0, or NULL = all 1; margin (any finite value: negative lets spheres
 *   overlap that far); plane {n_x, n_y, n_z, h0}, or NULL: no floor -- the normal of any non-zero length, normalised
 *   here (h0 is taken as given, in units of the unit normal); floor_mask: bit s set = sphere s is held above the
 *   plane; floor_weight >= 0.  Without a plane the mask and the weight are not looked at.
 * Guarantees: (a) apart == NULL, S == 0, or neither a pair nor a plane with mask bits gives rtg_dof_fit_prior_f32's
 * outputs bit for bit.  (b) With every pair apart and every masked sphere above the plane, and finite inputs, every
 * output equals (a)'s as a number (a zero may change sign).  (c) Coincident centres add the finite
 * pair_weight[p] (r_a + r_b + margin)^2 and no gradient.  (d) With zero offsets a DOF that rtg_dof_fit_prior_f32
 * leaves at +-0 and that has no sphere strictly below it stays at +-0.  (e) A frame depends on its own rows alone,
 * runs are bit-identical (every sum has one order), and n launches of one step that carry (m, v, root_state, step0)
 * equal one launch of n steps.  (f) A NaN in a frame's rows makes that frame's loss and gradient NaN (h = max(0, .)
 * passes NaN, as torch.clamp does) and no other frame's.
 * Errors: rtg_dof_fit_prior_f32's, and S or Pn negative, S > 0 or Pn > 0 with its arrays NULL, a pair index outside
 * 0..S-1 or a == b, a negative radius or weight, a non-finite radius, weight, margin, offset or plane, a plane normal
 * of zero length, mask bits at or above S, a link outside 0..J-1 -> RTG_ERR_INVALID_ARGUMENT; S >
 * RTG_FIT_MAX_SPHERES or Pn > RTG_FIT_MAX_PAIRS -> RTG_ERR_UNSUPPORTED; all before any device work.  B == 0 is a
 * no-op.
 * ---------------------------------------------------------------------- */
#define RTG_FIT_MAX_SPHERES 16   /* the spheres' centres share the tile's LDS */
#define RTG_FIT_MAX_PAIRS 32
typedef struct rtg_fit_apart {
    int32_t S;
    const int32_t *sphere_link;   /* (S) */
    const float *sphere;          /* (S,4) {offset, radius} */
    int32_t Pn;
    const int32_t *pair;          /* (Pn,2) */
    const float *pair_weight;     /* (Pn), or NULL */
    float margin;
    const float *plane;           /* (4) {normal, h0}, or NULL */
    uint32_t floor_mask;
    float floor_weight;
} rtg_fit_apart;
int rtg_dof_fit_apart_f32(rtg_dof_model_t model, const float *target_pos, const float *weight,
                          const int32_t *rot_joint, const float *target_rot, const float *rot_weight, int32_t K,
                          const float *prior, const float *prior_weight, int32_t flags, const float *root_rot,
                          const float *root_t, const float *dof_in, int64_t B, int clip, int32_t fit_root,
                          int32_t iters, float lr, float lr_root_t, float lr_root_rot, float beta1, float beta2,
                          float eps, int32_t step0, float *m, float *v, float *root_state, float *dof_out,
                          float *root_rot_out, float *root_t_out, float *loss, float *grad, float *grad_root,
                          const rtg_fit_apart *apart, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * rtg_dof_fit_apart_f32 with per-frame keypoint weights and a robust keypoint loss (a new symbol under ABI 7).  Every
 * other term assumes the keypoints are good; mocap drops frames, occludes markers and glitches.  Per frame f, with
 * e_fj = weight[j] frame_weight[f,j], d = P_j - target_pos[f,j], s = |d|^2, the keypoint term becomes
 *     sum over the j with frame_weight[f,j] != 0 of  e_fj rho(s),
 *     rho(s) = s                                  robust_scale == 0 (the quadratic loss of the other entry points)
 *     rho(s) = 2 s / (sqrt(1 + s / delta^2) + 1)  delta = robust_scale > 0
 * -- the pseudo-Huber kernel 2 delta^2 (sqrt(1 + s / delta^2) - 1) in the form that does not cancel for small s: s to
 * first order, 2 delta |d| far out, so one marker half a metre off pulls like one delta off does.  Its adjoint
 * dL/dP_j = 2 e_fj d / sqrt(1 + s / delta^2) enters where 2 weight[j] d does.  1 / delta^2 is formed in double and
 * rounded to float32 once; s / delta^2 is s times that.  The kernel applies to the keypoint term only: the
 * orientation, prior, keep-apart and floor terms are rtg_dof_fit_apart_f32's.
 *   frame_weight: (B,J) device memory, or NULL = all 1.  A keypoint with frame_weight[f,j] == 0 (either zero) is
 *   SKIPPED -- a select, not a multiplication: it adds exactly nothing to the loss and its residual row is exactly +0
 *   whatever its target row holds, NaN and inf included.  (weight[j] == 0 is still a multiplication, as in every
 *   other entry point.)  The values are device data and are not checked: a negative frame weight is used as given.
 *   Only a weight[j] or frame_weight[f,j] whose bits are 0x7F800001 is undefined: the tile marks a skipped keypoint
 *   with that signalling NaN, which no float32 product has.
 *   robust_scale: 0, or a finite positive number of metres.
 * Guarantees: (a) frame_weight == NULL with robust_scale == 0 gives rtg_dof_fit_apart_f32's outputs bit for bit (the
 * call runs its kernels).  (b) frame_weight all ones behaves exactly like NULL: with robust_scale == 0 and finite
 * inputs every output equals (a)'s as a number, with robust_scale > 0 ones and NULL agree bit for bit.  (c) A masked
 * keypoint contributes nothing whatever its target row holds; a frame with every keypoint masked has a keypoint loss
 * of exactly 0 and its DOFs get the exact +-0 of rtg_dof_fit_f32's guarantee; a DOF whose strict subtree has no
 * non-zero e_fj in frame f, and no oriented link or sphere below it, gets +-0 in that frame and from a zero state
 * keeps its bits; a masked root row leaves a fitted root translation its bits when nothing else pulls.  (d) A frame
 * depends on its own rows alone, runs are bit-identical, and n launches of one step that carry (m, v, root_state,
 * step0) equal one launch of n steps.  (e) A NaN or inf in frame_weight[f,.] makes frame f's loss and gradient
 * non-finite exactly where the float32 restatement of the formulas above does, and no other frame's.
 * Errors: rtg_dof_fit_apart_f32's, and robust_scale negative or not finite -> RTG_ERR_INVALID_ARGUMENT; all before
 * any device work.  B == 0 is a no-op.  For a one-joint model frame_weight still applies to the root's row.
 * ---------------------------------------------------------------------- */
int rtg_dof_fit_robust_f32(rtg_dof_model_t model, const float *target_pos, const float *weight,
                           const int32_t *rot_joint, const float *target_rot, const float *rot_weight, int32_t K,
                           const float *prior, const float *prior_weight, int32_t flags, const float *root_rot,
                           const float *root_t, const float *dof_in, int64_t B, int clip, int32_t fit_root,
                           int32_t iters, float lr, float lr_root_t, float lr_root_rot, float beta1, float beta2,
                           float eps, int32_t step0, float *m, float *v, float *root_state, float *dof_out,
                           float *root_rot_out, float *root_t_out, float *loss, float *grad, float *grad_root,
                           const rtg_fit_apart *apart, const float *frame_weight, float robust_scale,
                           rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * SkeletonState.retarget_to (poselib skeleton3d.py:742-889): the generic skeleton-to-skeleton retarget, rotations
 * relative to the source t-pose re-applied to the target t-pose, as ONE launch per call.
 * A plan holds everything that does not depend on the frame.  src / tgt: the source and target trees (borrowed only
 * during the call).  src_joint[K] / tgt_joint[K]: the joint mapping as index pairs (source joint -> target joint);
 * both roots must be mapped ("the root node cannot be dropped", :243) and no joint may occur twice ("the joint
 * mapping is not consistent with the skeleton trees", :729).  The t-poses' local rotations (J_s,4) / (J_t,4) and root
 * translations (3) as handed to retarget_to (normalised here, as the reference does), rotation_to_target (4) and the
 * scale: host pointers.  The constants (the source t-pose through the reduced trees, the target t-pose's global
 * rotations) are evaluated on the current device, synchronously; use the plan on that device only.  Trees of more
 * than 64 joints are RTG_ERR_UNSUPPORTED.  The pairwise average translation the reference computes (:826) never
 * reaches its result and is not computed.
 * ---------------------------------------------------------------------- */
typedef struct rtg_retarget_plan_s *rtg_retarget_plan_t;
int rtg_retarget_plan_create(rtg_topology_t src, rtg_topology_t tgt,
                             const int32_t *src_joint, const int32_t *tgt_joint, int32_t K,
                             const float *src_tpose_local_rot, const float *src_tpose_root_t,
                             const float *tgt_tpose_local_rot, const float *tgt_tpose_root_t,
                             const float *rotation_to_target, float scale, rtg_retarget_plan_t *out);
int rtg_retarget_plan_destroy(rtg_retarget_plan_t plan);
/* src_rot (B,J_s,4): the source state's rotations as the state stores them -- local (src_is_local != 0: the kernel
 * runs the state FK with the source tree's quaternions) or global; src_root_t (B,3) -> tgt_local_rot (B,J_t,4), the
 * local rotations of the target state, and tgt_root_t (B,3).  The rotation buffers are 16-byte aligned rows (any
 * hipMalloc / torch tensor), the root translations any float alignment.  Never allocates or synchronises; B == 0 is
 * a no-op.  A frame's NaN / inf stays in that frame's rows. */
int rtg_retarget_to_f32(rtg_retarget_plan_t plan, const float *src_rot, const float *src_root_t, int src_is_local,
                        int64_t B, float *tgt_local_rot, float *tgt_root_t, rtg_stream_t stream);
/* The host tables a plan is built from (host only, no HIP call; for inspection and tests).  parents as for
 * rtg_topology_create.  Every output may be NULL: kept_src / kept_tgt (K) the mapped joints ascending, i.e. the
 * joints of the reduced trees (drop_nodes_by_names, :226-259); src_reduced_parents / tgt_reduced_parents (K) their
 * parents there; perm (K) the index in the reduced source tree of the joint mapped to the reduced target tree's k-th
 * (:721-740); src_of (J_t) the index in the reduced target tree of target joint j's nearest mapped ancestor-or-self
 * (:876-880).  Same validation and messages as rtg_retarget_plan_create. */
int rtg_retarget_plan_tables(const int32_t *src_parents, int32_t J_s, const int32_t *tgt_parents, int32_t J_t,
                             const int32_t *src_joint, const int32_t *tgt_joint, int32_t K, int32_t *kept_src,
                             int32_t *src_reduced_parents, int32_t *kept_tgt, int32_t *tgt_reduced_parents,
                             int32_t *perm, int32_t *src_of);

/* ------------------------------------------------------------------------
 * Keypoint targets for the pose fit from mocap positions of a body of other proportions: the limb-wise rescale of
 * Retarget.rescale_motion_to_standard_size (retarget/main.py:37-47) across TWO skeletons joined by a joint mapping,
 * as ONE launch.  src_joint[K] / tgt_joint[K]: the mapping as index pairs (source joint s_k -> target link t_k).
 *
 * The plan, evaluated on the host: a(k) is the pair whose target link is the nearest mapped proper ancestor of t_k in
 * the target tree; G the target zero pose's global translations, float32 sums taken parents first (G[root] = 0,
 * G[j] = G[parent] + local_t[j]); seg[k] = G[t_k] - G[t_a(k)] in float32; weight[j] = 1 for a mapped link, else 0;
 * src_of[j] the pair of link j's nearest mapped ancestor-or-self.
 *
 * The launch, per frame, every operation one float32 rounding (no FMA):
 *   m(j) = src_pos[j], or src_pos[j] * dir per component with dir (coord_transform, transform3d.py:24-29);
 *   the root pair:   out[t] = m(s), then * root_scale, then + root_offset (an absent operand adds no operation: with
 *                    all three NULL the root row keeps the source row's bits);
 *   any other pair:  d = m(s_k) - m(s_a(k)); scale = norm(d) / norm(seg[k]); out[t_k] = out[t_a(k)] + d / scale, with
 *                    torch.linalg.norm's sqrt(fma(z, z, fma(y, y, x x))): rtg_rescale_motion_f32's expressions;
 *   an unmapped link j: out[j] = out[t_src_of(j)], a finite placeholder whose weight is 0.
 * With the same tree on both sides and the identity mapping this is rtg_rescale_motion_f32 wherever seg[k] has
 * local_t[k]'s bits.  A zero-length target segment is accepted (scale = inf: the child sits on its anchor).
 *
 * dir, root_scale, root_offset: 3 host floats each or NULL, copied into the plan.  The tables are copied to the
 * current device (synchronously); use the plan on that device only.  RTG_ERR_INVALID_ARGUMENT -- a NULL handle or
 * buffer, K < 1, an index out of range, a joint named twice on either side, the target root not mapped, B < 0,
 * overlapping buffers -- and RTG_ERR_UNSUPPORTED -- more than 64 joints on either side -- are decided before any HIP
 * call, with the reason in rtg_last_error().
 * ---------------------------------------------------------------------- */
typedef struct rtg_fit_targets_plan_s *rtg_fit_targets_plan_t;
int rtg_fit_targets_plan_create(rtg_topology_t src, rtg_topology_t tgt, const int32_t *src_joint,
                                const int32_t *tgt_joint, int32_t K, const float *dir, const float *root_scale,
                                const float *root_offset, rtg_fit_targets_plan_t *out);
int rtg_fit_targets_plan_destroy(rtg_fit_targets_plan_t plan);
/* src_pos (B,J_s,3) -> target_pos (B,J_t,3), device memory of any float alignment (16-byte aligned rows move as
 * whole pieces).  Never allocates or synchronises; B == 0 is a no-op.  A frame's NaN / inf stays in that frame's
 * rows, in the links hung from the segment that has it. */
int rtg_fit_targets_f32(rtg_fit_targets_plan_t plan, const float *src_pos, int64_t B, float *target_pos,
                        rtg_stream_t stream);
/* The host tables of a plan (host only, no HIP call).  tgt_parents / tgt_local_t as for rtg_topology_create; of the
 * source tree only its joint count matters.  Every output may be NULL: anchor (K) the pair a(k), -1 for the root
 * pair; seg (K,3), zeros for the root pair; weight (J_t); src_of (J_t).  Pairs are numbered as given.  Same validation
 * and messages as rtg_fit_targets_plan_create. */
int rtg_fit_targets_plan_tables(int32_t J_s, const int32_t *tgt_parents, const float *tgt_local_t, int32_t J_t,
                                const int32_t *src_joint, const int32_t *tgt_joint, int32_t K, int32_t *anchor,
                                float *seg, float *weight, int32_t *src_of);

/* ------------------------------------------------------------------------
 * VTRDyn ingest (sim_full_body_teleop.py:92, :109-112)
 * ---------------------------------------------------------------------- */
/* Raw broadcast frames body_pos (B,23,3), left/right_hand_pos (B,20,3) -> solver inputs body (B,21,3)
 * (23 -> 21 joint reindex), hands (B,20,3) (point reorder), and valid (B) uint8: 0 where every body value
 * is within 1e-8 of 0 (np.allclose(body_pos, 0): the teleop loop keeps the previous DOFs), else 1.
 * layout: of the outputs body / lh / rh (the raw inputs are the reference's rows). */
int rtg_ingest_vtrdyn_f32(const float *body_pos, const float *left_hand, const float *right_hand, int64_t B,
                          int layout, float *body, float *lh, float *rh, uint8_t *valid, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Rotation ingest: the zero-pose transforms every caller puts recorded quaternions through before a rotation solver
 * (retarget/utils/parse_mocap.py:65-134, zero_pose_transform.py:16-41), as ONE launch:
 *     out[f, j] = quat_mul_norm(quat_mul_norm(q[f, src[j]], pre), post[j])
 * pre (4) is the one axis rotation, post (J_out,4) = quat_inverse(t2zero[j]); src (J_out) picks the input row of
 * output joint j (the broadcast's 23 -> 21 rows; NULL = the identity, which needs J_in == J_out).  The two products
 * are the reference's, in its order, each normalised: bit for bit RTG_OP_QUAT_MUL_NORM applied twice, for any input
 * (non-unit, zero, NaN, inf, -0 included).  1 <= J_in, J_out <= 64.  src, pre, post are host pointers, copied once
 * into the handle's device blob on the current device (synchronously); use the handle on that device only.
 * ---------------------------------------------------------------------- */
typedef struct rtg_rot_ingest_s *rtg_rot_ingest_t;
int rtg_rot_ingest_create(int32_t J_in, int32_t J_out, const int32_t *src, const float *pre, const float *post,
                          rtg_rot_ingest_t *out);
void rtg_rot_ingest_destroy(rtg_rot_ingest_t h);
/* q (B,J_in,4) rows -> out in `layout`: (B,J_out,4) rows (RTG_LAYOUT_AOS) or component planes (J_out,4,B)
 * (RTG_LAYOUT_SOA), what rtg_retarget_f32 reads as FULL_BODY_ROT's in0 / BODY_ROT's in0.  q and out are 16-byte
 * aligned and must not overlap.  Never allocates or synchronises; B == 0 is a no-op (after the layout check).
 * RTG_ERR_INVALID_ARGUMENT -- a NULL handle or buffer, B < 0, a bad layout, a misaligned or overlapping buffer; for
 * rtg_rot_ingest_create a J outside 1..64, src[j] outside 0..J_in-1, src == NULL with J_in != J_out, a NULL pre /
 * post / out -- is decided before any HIP call, with the reason in rtg_last_error(). */
int rtg_rot_ingest_f32(rtg_rot_ingest_t h, const float *q, int64_t B, int layout, float *out, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Motion sampling: many clips of one skeleton, sampled at arbitrary (clip, time) pairs in ONE launch -- the index
 * rule, the gather of the two frames, quat_slerp (transform3d.py:152-174) per joint, the linear blends and, when
 * asked, the forward kinematics of the blended pose.
 *
 * A library is C clips packed frame-major into arrays the caller owns: rot (F_total,J,4) local rotations, root_t
 * (F_total,3), optionally vec (F_total,K,3) vector rows (velocities, say), and per clip start[c] (first row), len[c]
 * (frames) and fps[c].  For query n with c = clip[n], t = time[n] (seconds from the clip's first frame):
 *   - the query is valid iff 0 <= c < C; every output element of an invalid query is the quiet NaN 0x7FC00000 and it
 *     reads no library row;
 *   - p = (double)t * (double)fps[c]; !(p > 0) -> p = 0 (NaN, -0, negatives);
 *   - p >= len[c] - 1: i0 = i1 = len[c] - 1, b = 0; else i0 = trunc(p), i1 = i0 + 1, b = (float)(p - (double)i0).
 *     No wrap-around; i1 never leaves the clip;
 *   - local_rot_out[n, j] = RTG_OP_QUAT_SLERP(rot[start+i0, j], rot[start+i1, j], b) bit for bit (pairs whose half
 *     angle's sine is below 0.001 return the midpoint whatever b is, as the reference has it), then
 *     RTG_OP_QUAT_NORMALIZE with RTG_MOTION_NORMALIZE;
 *   - root_t_out[n] and vec_out[n] = ((1.0f - b) * a) + (b * c) per component: four float32 roundings, no FMA;
 *   - with RTG_MOTION_GLOBAL, g_rot / g_pos are what rtg_fk_f32 (rtg_state_fk_f32 with RTG_MOTION_STATE) gives on
 *     local_rot_out[n], root_t_out[n].
 * rtg_motion_lib_create takes HOST arrays, validates them (C >= 1, len >= 1, start >= 0, start + len <= F_total <
 * 2^31, fps finite and positive, no NULL: RTG_ERR_INVALID_ARGUMENT before any HIP call, the reason in
 * rtg_last_error()) and copies one table to the current device (synchronously); use the handle on that device only.
 * ---------------------------------------------------------------------- */
typedef struct rtg_motion_lib_s *rtg_motion_lib_t;
typedef enum rtg_motion_flags {
    RTG_MOTION_NORMALIZE = 1,   /* quat_normalize after the slerp */
    RTG_MOTION_GLOBAL = 2,      /* also the forward kinematics: g_rot, g_pos */
    RTG_MOTION_STATE = 4        /* with RTG_MOTION_GLOBAL: SkeletonState FK (the tree quaternions), rtg_state_fk_f32 */
} rtg_motion_flags;
int rtg_motion_lib_create(const int64_t *start, const int32_t *len, const float *fps, int32_t C, int64_t F_total,
                          rtg_motion_lib_t *out);
void rtg_motion_lib_destroy(rtg_motion_lib_t lib);
/* rot / root_t / vec are the library's arrays (device), clip (N) int32 and time (N) float32 the queries; outputs
 * local_rot_out (N,J,4), root_t_out (N,3), vec_out (N,K,3), g_rot (N,J,4), g_pos (N,J,3).  vec and vec_out are given
 * together (K >= 1) or both NULL; g_rot and g_pos are both given with RTG_MOTION_GLOBAL and both NULL without it.
 * rot, local_rot_out and g_rot are 16-byte aligned; no output overlaps an input.  Never allocates or synchronises;
 * N == 0 is a no-op after the argument checks.  A topology of more than 64 joints is RTG_ERR_UNSUPPORTED; every
 * other rejection is RTG_ERR_INVALID_ARGUMENT, decided before any HIP call. */
int rtg_motion_sample_f32(rtg_topology_t topo, rtg_motion_lib_t lib, const float *rot, const float *root_t,
                          const float *vec, int32_t K, const int32_t *clip, const float *time, int64_t N, int flags,
                          float *local_rot_out, float *root_t_out, float *vec_out, float *g_rot, float *g_pos,
                          rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Motion sampling of JOINT-ANGLE clips: what rtg_dof_fit_root_f32 and its successors return -- per frame J-1 joint
 * angles, a root rotation and a root translation -- packed frame-major as dof (F_total,J-1), root_rot (F_total,4),
 * root_t (F_total,3) on an rtg_motion_lib_t clip table (the same handle type, index rule and validity rule as
 * above), sampled at (clip, time) pairs in ONE launch.  Every joint of the model turns about one fixed axis, so the
 * slerp of a joint is the linear blend of its angle.  With (i0, i1, b) of the index rule, rows r0 = start + i0,
 * r1 = start + i1 and dt = (float)(1.0 / (double)fps[c]):
 *   - dof_out[n, d]     = ((1.0f - b) * dof[r0, d]) + (b * dof[r1, d]): four float32 roundings, no FMA;
 *   - dof_vel_out[n, d] = (dof[r1, d] - dof[r0, d]) / dt: one float32 subtraction, one correctly rounded float32
 *     division -- the forward difference of the bracketing frames, constant over the bracket; at and past the clip's
 *     last frame r0 == r1 and it is +0 for finite rows;
 *   - root_rot_out[n]   = RTG_OP_QUAT_SLERP(root_rot[r0], root_rot[r1], b), then RTG_OP_QUAT_NORMALIZE with
 *     RTG_DOF_MOTION_NORMALIZE; root_t_out[n] the blend of dof_out's form;
 *   - root_vel_out[n, 0:3] = (root_t[r1] - root_t[r0]) / dt; root_vel_out[n, 3:6] = SkeletonMotion's unfiltered
 *     angular velocity of the pair (skeleton3d.py:1137-1146; rtg_angular_velocity_f32 without taps on the two-frame
 *     sequence [root_rot[r0], root_rot[r1]], frame 0): with d = quat_mul_norm(r1, quat_conjugate(r0)),
 *     ((d.xyz / max(|d.xyz|, 1e-9)) * acos(clamp(2 d.w^2 - 1, -1, 1))) / dt;
 *   - g_rot / g_pos are what rtg_dof_fk_f32 gives on dof_out[n], root_rot_out[n], root_t_out[n], with clip_angles =
 *     RTG_DOF_MOTION_CLIP; key_pos[n, k] = g_pos[n, key_links[k]] bit for bit, and may be asked for without g_rot /
 *     g_pos (their rows are then not written at all);
 *   - every output element of an invalid query (clip id outside 0..C-1) is the quiet NaN 0x7FC00000.
 * dof_out, root_rot_out, root_t_out are always given; dof_vel_out (N,J-1) and root_vel_out (N,6) together or both NULL; g_rot
 * and g_pos together or both NULL; key_pos (N,K,3) iff K > 0, with key_links K HOST int32 values in 0..J-1 (repeats
 * allowed, 0 <= K <= RTG_DOF_MOTION_MAX_KEY_LINKS) read before the call returns.  root_rot, root_rot_out and g_rot are
 * 16-byte aligned; no output overlaps an input or another output.  A one-joint model has no angles: dof, dof_out and
 * dof_vel_out are then not dereferenced and may be NULL (rtg_dof_fit_root_f32's rule).  Never allocates or
 * synchronises; N == 0 is a no-op after the argument checks.  A model of more than 64 joints is RTG_ERR_UNSUPPORTED;
 * every other rejection -- N < 0, K outside its range, a key link outside 0..J-1, unknown flags,
 * RTG_DOF_MOTION_CLIP on a model without limits, a NULL handle or buffer, an unpaired optional output, key_pos
 * without K or K without key_pos, a misaligned or overlapping buffer -- is RTG_ERR_INVALID_ARGUMENT, decided before
 * any HIP call, with the reason in rtg_last_error().
 * ---------------------------------------------------------------------- */
#define RTG_DOF_MOTION_MAX_KEY_LINKS 32   /* the key links travel in the launch arguments */
typedef enum rtg_dof_motion_flags {
    RTG_DOF_MOTION_NORMALIZE = 1,   /* quat_normalize after the root rotation's slerp */
    RTG_DOF_MOTION_CLIP = 2         /* the global outputs from the angles clamped to the model's limits (straight-through,
                                       as rtg_dof_fk_f32's clip_angles); dof_out stays the blend */
} rtg_dof_motion_flags;
int rtg_dof_motion_sample_f32(rtg_dof_model_t model, rtg_motion_lib_t lib, const float *dof, const float *root_rot,
                              const float *root_t, const int32_t *clip, const float *time, int64_t N, int flags,
                              const int32_t *key_links, int32_t K, float *dof_out, float *dof_vel_out,
                              float *root_rot_out, float *root_t_out, float *root_vel_out, float *g_rot, float *g_pos,
                              float *key_pos, rtg_stream_t stream);
/* The same launch with the link velocities of the sampled state, so that a full reference state -- position, rotation,
 * linear and angular velocity of every tracked link -- leaves in one launch.  The parameters up to key_pos are
 * rtg_dof_motion_sample_f32's.  g_vel (N,J,6) is rtg_dof_fk_vel_f32's g_vel on the launch's own outputs: angles
 * dof_out[n] (the clip test of RTG_DOF_MOTION_CLIP runs on them), joint velocities dof_vel_out[n], root rotation and
 * translation root_rot_out[n], root_t_out[n], root twist root_vel_out[n]; key_vel[n, k] = g_vel[n, key_links[k]] bit
 * for bit (N,K,6).  g_vel and key_vel are each optional and need neither g_rot / g_pos nor each other; either of them
 * requires dof_vel_out and root_vel_out.  K > 0 exactly when key_pos or key_vel is given.  An invalid query's rows
 * are the quiet NaN in both; at and past a clip's last frame (finite rows) they are +0.  With g_vel and key_vel both
 * NULL the call IS rtg_dof_motion_sample_f32: the same kernels, bits and messages.  Rejections as there. */
int rtg_dof_motion_sample_vel_f32(rtg_dof_model_t model, rtg_motion_lib_t lib, const float *dof, const float *root_rot,
                                  const float *root_t, const int32_t *clip, const float *time, int64_t N, int flags,
                                  const int32_t *key_links, int32_t K, float *dof_out, float *dof_vel_out,
                                  float *root_rot_out, float *root_t_out, float *root_vel_out, float *g_rot,
                                  float *g_pos, float *key_pos, float *g_vel /* (N,J,6) */,
                                  float *key_vel /* (N,K,6) */, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Motion-level prep of the legacy motion path (retarget/main.py)
 * ---------------------------------------------------------------------- */
/* Retarget.rescale_motion_to_standard_size (main.py:37-47) after coord_transform(p, dir=dir) (:170;
 * transform3d.py:24-29).  motion (B,J,3) -> out (B,J,3): every bone scaled to its zero-pose length and hung
 * from the parent's rescaled position.  dir: 3 floats (host) or NULL. */
int rtg_rescale_motion_f32(rtg_topology_t topo, const float *motion, int64_t B, const float *dir, float *out,
                           rtg_stream_t stream);
/* quat_between_two_vecs (transform3d.py:8-21): v1, v2 (n,3) -> (n,4).  The identity branch is decided over the
 * whole batch (max norm <= 1e-6, :11-12), as the reference does.  workspace: 2 floats of device memory. */
int rtg_quat_between_f32(const float *v1, const float *v2, int64_t n, float *out, float *workspace,
                         rtg_stream_t stream);
/* RetargetHuV5fromMocap._rebuild_with_vtrdyn_zero_pose (main.py:116-165) up to the SkeletonState it builds
 * (rotations normalised, skeleton3d.py:610).  topo: the 21-joint VTRDYN zero pose; motion (B,21,3) rescaled
 * positions -> g_rot (B,21,4) global rotations, root_t (B,3).  workspace: J floats of device memory. */
int rtg_rebuild_vtrdyn_f32(rtg_topology_t topo, const float *motion, int64_t B, float *g_rot, float *root_t,
                           float *workspace, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Retarget solvers (retarget/retarget_solver/__init__.py:9-14)
 * ---------------------------------------------------------------------- */
typedef enum rtg_solver_kind {
    /* VtrdynFullBodyPosRetargeter.retarget  full_body_pos_retargeter.py:25-217
     * in0 = body (B,21,3), in1 = left hand (B,20,3), in2 = right hand (B,20,3);
     * source zero pose = VTRDYN_FULL (59 joints). */
    RTG_SOLVER_FULL_BODY_POS = 0,
    /* HuUpperBodyFromMocapRetarget.retarget_from_global_translation  retarget_solver.py:40-99
     * in0 = raw VTRDyn positions (B,21,3); source zero pose = VTRDYN (21). */
    RTG_SOLVER_UPPER_BODY = 1,
    /* VtrdynFullBodyRetargeter.retarget  full_body_retargeter.py:19-177
     * in0 = body rotations (B,21,4), in1 = body positions (B,21,3),
     * in2 = left hand (B,20,3), in3 = right hand (B,20,3); source = VTRDYN_FULL (59). */
    RTG_SOLVER_FULL_BODY_ROT = 2,
    /* Mocap2HuBodyRetargeter.retarget_from_pose  body_retargeter.py:34-81
     * in0 = global rotations (B,21,4); source = VTRDYN (21). */
    RTG_SOLVER_BODY_ROT = 3
} rtg_solver_kind;

/* Create a solver.  src_zero_local_t / src_zero_global_t: the source
 * RobotZeroPose local / global translations (Js,3), src_parents (Js) -- host
 * pointers.  The target is always Hu v5 (31 links, 30 DOFs; Hu_v5.py:12-18).
 * Zero-pose-only terms of the joint maps (theta0 / phi0, Kabsch zero vectors,
 * gripper denominator) are evaluated once here, on the device.  The solver
 * also owns a 6.7 MiB exp-map angle table, built here on the current device
 * (synchronously); use the solver on that device only.  Replaces the
 * constructors at full_body_pos_retargeter.py:18, retarget_solver.py:28,
 * full_body_retargeter.py:16, body_retargeter.py:31. */
int rtg_solver_create(int kind, const float *src_zero_local_t, const float *src_zero_global_t,
                      const int32_t *src_parents, int32_t Js, int precise_gripper, rtg_solver_t *out);
int rtg_solver_destroy(rtg_solver_t solver);

/* Frames on which the reference raises.  The reference solves one frame per call and, on some degenerate
 * frames, raises instead of returning:
 *   RTG_FRAME_SVD_NONFINITE   cal_joint_quat's Kabsch matrix has a NaN entry: torch.linalg.svd raises
 *                             RuntimeError "linalg.svd: (Batch element 0): The algorithm failed to converge because
 *                             the input matrix contained non-finite values." (transform3d.py:40);
 *   RTG_FRAME_ZERO_NORM_QUAT  the quaternion handed to quat_in_xyz_axis is all zero or has a NaN: scipy raises
 *                             ValueError "Found zero norm quaternions in `quat`." (transform3d.py:53) -- e.g. a
 *                             zero-length arm segment, an upper arm along the shoulder plane's normal, a straight
 *                             elbow (radians_between_vecs of a zero projection is NaN, transform3d.py:77-100).
 * The code is the first raise in the reference's own order (torso fit, left wrist fit, left Euler split, right
 * wrist fit, right Euler split; full_body_pos_retargeter.py:68-167).  A batched launch marks such a frame instead
 * of raising: every dof of its row is NaN, and dof[f*30 + 0] -- exactly 0 for every other frame, the solvers never
 * write DOF 0 -- has the bit pattern RTG_FRAME_NAN | code; its local_rot / body_rot rows are RTG_FRAME_NAN. */
typedef enum rtg_frame_error {
    RTG_FRAME_OK = 0,
    RTG_FRAME_SVD_NONFINITE = 1,
    RTG_FRAME_ZERO_NORM_QUAT = 2
} rtg_frame_error;
#define RTG_FRAME_NAN 0x7FC00000u   /* quiet NaN; the low payload bits carry the rtg_frame_error code in dof[f*30] */

/* Errors a launch reports on the solver's NEXT call (launches never synchronise): the device ORs these into the
 * solver's host-mapped error word and rtg_retarget_f32 returns RTG_ERR_DEVICE with the word in rtg_last_error(),
 * then clears it.  A wave that waited ~0.1 s for its partner wave's hand-over flag gives up and sets
 * RTG_DEVERR_HANDOVER_TIMEOUT: that launch's outputs are not to be trusted. */
#define RTG_DEVERR_HANDOVER_TIMEOUT 0x1u

/* Batched retarget of B frames.  dof (B,30) required; local_rot (B,31,4) and
 * body_rot (B,59,4, FULL_BODY_POS only: the returned body_global_rotation) may
 * be NULL.  Unused in* must be NULL.  layout (rtg_layout) describes the inputs
 * only; the outputs are always (B, ...) rows.  Frames on which the reference
 * raises are marked as described at rtg_frame_error.  Replaces the per-frame
 * .retarget calls of sim_full_body_teleop.py:115-119 / sim_teleop_mujoco.py:104-108
 * / sim_teleop.py:102. */
int rtg_retarget_f32(rtg_solver_t solver, const float *in0, const float *in1, const float *in2,
                     const float *in3, int64_t B, int layout, float *dof, float *local_rot, float *body_rot,
                     rtg_stream_t stream);

/* Per-frame server for the teleop loop (sim_full_body_teleop.py:109-119 retargets one captured frame per
 * iteration through VtrdynFullBodyPosRetargeter.retarget, full_body_pos_retargeter.py:60-176): launches ONE
 * resident workgroup that serves FULL_BODY_POS frames without a launch per frame.
 *   in        the server's inbox, RTG_SERVER_INBOX_FLOATS floats: the frame in floats 0..182 -- body (21,3) | left
 *             hand (20,3) | right hand (20,3), rows as rtg_retarget_f32's AoS inputs -- and the frame sequence number
 *             (uint32) in float RTG_SERVER_SEQ_WORD, stored by the host after the frame's rows.  Either device memory
 *             from rtg_server_inbox_alloc (the host stores into it through the PCIe BAR: the faster hand-over) or
 *             device-accessible pinned host memory.
 *   dof (30), local_rot (31,4, may be NULL), body_rot (59,4, may be NULL): pinned host memory the server OWNS while it
 *             runs.  The dof row and the frame-dependent local_rot / body_rot rows are written per frame; the 73
 *             rows that never change (local_rot's fixed links, body_rot's identity rows) are written once per
 *             launch and again after a frame the reference raises on.  A client that clears or edits these
 *             buffers between frames must copy the rows out instead (rtg_frame_server_post does) or relaunch.
 *   ctl       4 x uint32, pinned host memory: [0] reserved (ABI <= 3: the sequence number);
 *             [1] the last sequence number served, written by the device after that frame's outputs;
 *             [2] set to 1 by the device when the server has ended;
 *             [3] the server's error word (RTG_DEVERR_*), set before [1] of the frame it concerns.
 *             Zero ctl[1..3] before the launch, and have the inbox's sequence word equal ctl[1] (both 0 at first).
 * Storing RTG_SERVER_QUIT as the sequence number (rtg_frame_server_signal) ends the server; so does idle_ms
 * (1..60000) without a new frame.  The stream is occupied until the server ends.  The values in the buffers after a
 * frame is served (ctl[1]) are bit-identical to rtg_retarget_f32's at B = 1. */
#define RTG_SERVER_QUIT 0xFFFFFFFFu
#define RTG_SERVER_INBOX_FLOATS 256
#define RTG_SERVER_SEQ_WORD 192
int rtg_frame_server_launch(rtg_solver_t solver, const float *in, float *dof, float *local_rot, float *body_rot,
                            uint32_t *ctl, uint32_t idle_ms, rtg_stream_t stream);

/* A frame-server inbox in device memory that the host can store into (hipExtMallocWithFlags, uncached; the CPU
 * reaches it through the PCIe BAR): RTG_SERVER_INBOX_FLOATS floats, zeroed.  Host stores into it are
 * write-combined: rtg_frame_server_post / rtg_frame_server_signal drain them (sfence) in order.  Free with
 * rtg_server_inbox_free.  A 184-float ping-pong through it takes 4.0 us against 4.8 us through pinned host memory
 * on MI355X (tools/bar_probe.hip). */
int rtg_server_inbox_alloc(float **inbox);
int rtg_server_inbox_free(float *inbox);

/* Stores `word` as the inbox's sequence number and drains it to the device (host only, no HIP call): RTG_SERVER_QUIT
 * ends a running server; after it has ended, store ctl[1] back before a relaunch. */
int rtg_frame_server_signal(float *in, uint32_t word);

/* One frame through a running rtg_frame_server_launch server, on the host alone (no HIP call): the whole per-frame
 * round trip of the teleop loop (sim_full_body_teleop.py:115-119) in one C call.  Copies the frame's rows into the
 * server's inbox `in` (body (21,3) | left hand (20,3) | right hand (20,3)), stores `seq` (!= the last one posted,
 * != RTG_SERVER_QUIT) as its sequence number after them, spins until the device publishes it in ctl[1], then copies
 * the pinned outputs the server writes (dof 30, local_rot 124, body_rot 236 floats) into the *_dst buffers that are
 * not NULL.  Returns RTG_OK; RTG_SERVER_ENDED if the server ended (idle_ms) before it took the frame -- relaunch it
 * and post the same seq again; RTG_ERR_TIMEOUT after timeout_us (the frame may still be served later);
 * RTG_ERR_DEVICE if the server set its error word (ctl[3]) while serving the frame (the outputs are copied anyway;
 * the word is cleared). */
int rtg_frame_server_post(uint32_t *ctl, uint32_t seq, float *in, const float *body, const float *left_hand,
                          const float *right_hand, const float *dof, const float *local_rot, const float *body_rot,
                          float *dof_dst, float *local_rot_dst, float *body_rot_dst, uint32_t timeout_us);

/* ------------------------------------------------------------------------
 * Elementwise primitives (poselib rotation3d.py, retarget transform3d.py)
 * ---------------------------------------------------------------------- */
typedef enum rtg_quat_op {
    RTG_OP_QUAT_MUL = 0,            /* a (n,4), b (n,4) -> (n,4)   rotation3d.py:14-27   */
    RTG_OP_QUAT_MUL_NORM = 1,       /* a, b -> (n,4)               :196-202             */
    RTG_OP_QUAT_NORMALIZE = 2,      /* a -> (n,4)                  :92-98               */
    RTG_OP_QUAT_ROTATE = 3,         /* q (n,4), v (n,3) -> (n,3)   :205-211             */
    RTG_OP_QUAT_INVERSE = 4,        /* a -> (n,4)                  :214-219             */
    RTG_OP_QUAT_FROM_ANGLE_AXIS = 5,/* angle (n), axis (n,3) -> (n,4)  :122-143         */
    RTG_OP_QUAT_FROM_ROTMAT = 6,    /* m (n,3,3) -> (n,4)          :146-193             */
    RTG_OP_QUAT_TO_EXP_MAP = 7,     /* q (n,4) -> (n,3)            :620-627             */
    RTG_OP_RADIANS_BETWEEN = 8,     /* v1 (n,3), v2 (n,3), c = n (n,3) -> (n)  transform3d.py:77-100 */
    RTG_OP_PROJ_IN_PLANE = 9,       /* v (n,3), n (n,3) -> (n,3)   transform3d.py:61-75 */
    RTG_OP_QUAT_TO_DOF_POS = 10,    /* local_rot (n,31,4) -> dof (n,30)  transform3d.py:176-183 (Hu) */
    RTG_OP_SHOULDER_PR = 11,        /* v1 (n,3), v0 (n,3), parent c (n,4) -> (n,2,4)  full_body_pos_retargeter.py:246-278 */
    RTG_OP_ELBOW_PY = 12,           /* v1, v0, parent -> (n,2,4)   full_body_pos_retargeter.py:220-243 */
    RTG_OP_QUAT_TO_ANGLE_AXIS = 13, /* q (n,4) -> (n,4) = [angle, axis xyz]  rotation3d.py:587-608 */
    RTG_OP_NORMALIZE_ANGLE = 14,    /* x (n) -> (n) atan2(sin x, cos x)      rotation3d.py:582-584 */
    RTG_OP_QUAT_ABS = 15,           /* q (n,4) -> (n) |q|                    rotation3d.py:41-47  */
    RTG_OP_QUAT_UNIT = 16,          /* q (n,4) -> q / max(|q|, 1e-9)         rotation3d.py:50-56  */
    RTG_OP_QUAT_ANGLE_AXIS = 17,    /* q (n,4) -> [acos(2w^2-1), xyz/|xyz|]  rotation3d.py:230-240 */
    /* the rest of the rotation3d / transform3d surface (off the solver path; same op-order contract) */
    RTG_OP_EXP_MAP_TO_ANGLE_AXIS = 18, /* e (n,3) -> (n,4) [angle, axis]      rotation3d.py:629-646 */
    RTG_OP_EXP_MAP_TO_QUAT = 19,    /* e (n,3) -> (n,4)      rotation3d.py:648-652 = transform3d.py:146-150 */
    RTG_OP_QUAT_SLERP = 20,         /* q0 a (n,4), q1 b (n,4), t c (n) -> (n,4)   transform3d.py:152-174 */
    RTG_OP_QUAT_FROM_XYZ = 21,      /* xyz (n,3) -> (n,4) [xyz, 1 - |xyz|], per row  rotation3d.py:101-108 */
    RTG_OP_ROT_MATRIX_DET = 22,     /* m (n,3,3) -> (n)                      rotation3d.py:338-350 */
    RTG_OP_ROT_MATRIX_FROM_QUAT = 23, /* q (n,4) -> (n,3,3)                  rotation3d.py:398-427 */
    RTG_OP_ROTATION_ALONG_X = 24,   /* q (n,4) -> (n) extract_rotation_along_axis(q, 0)  rotation3d.py:534-556 */
    RTG_OP_ROTATION_ALONG_Y = 25,   /* ... axis 1 */
    RTG_OP_ROTATION_ALONG_Z = 26,   /* ... axis 2 */
    RTG_OP_PROJECT_QUAT_X = 27,     /* q (n,4) -> (n,4)  project_quat_to_axis_x   rotation3d.py:479-486 */
    RTG_OP_PROJECT_QUAT_Y = 28,     /*                   project_quat_to_axis_y   :488-495 */
    RTG_OP_PROJECT_QUAT_Z = 29,     /*                   project_quat_to_axis_z   :497-504 */
    RTG_OP_PROJECT_QUAT_XY = 30,    /*                   project_quat_to_axis_xy  :506-517 */
    RTG_OP_PROJECT_QUAT_XZ = 31     /*                   project_quat_to_axis_xz  :519-530 */
} rtg_quat_op;
int rtg_quat_op_f32(int op, const float *a, const float *b, const float *c, int64_t n, float *out,
                    rtg_stream_t stream);

/* cal_joint_quat (transform3d.py:31-50): Kabsch fit of npts (1..8) point pairs.
 * Z (n,npts,3) zero-pose vectors, M (n,npts,3) motion vectors -> (n,4).  A fit whose Kabsch matrix has a NaN
 * entry (where torch.linalg.svd raises, rtg_frame_error) gets all four components = RTG_FRAME_NAN |
 * RTG_FRAME_SVD_NONFINITE. */
int rtg_cal_joint_quat_f32(const float *Z, const float *M, int32_t npts, int64_t n, float *out,
                           rtg_stream_t stream);

/* quat_in_xyz_axis (transform3d.py:52-59): scipy Euler split (float64) into three
 * single-axis quaternions.  seq: 3 chars of xyz/XYZ (upper = intrinsic). q (n,4) -> (n,3,4).  A quaternion scipy
 * refuses (zero norm or NaN, rtg_frame_error) gets all twelve outputs = RTG_FRAME_NAN | RTG_FRAME_ZERO_NORM_QUAT. */
int rtg_quat_in_xyz_axis_f32(const float *q, const char *seq, int64_t n, float *out, rtg_stream_t stream);
/* scipy Rotation.from_quat(q).as_euler(seq, degrees) in float64 (rotation3d.py:658-661 quat_to_eular uses
 * 'xyz', degrees=True; degrees multiply by 180/pi like np.rad2deg).  q (n,4) f32 -> out (n,3) f64.  A quaternion
 * scipy refuses gets the three f64 NaNs 0x7FF8000000000000 | RTG_FRAME_ZERO_NORM_QUAT. */
int rtg_quat_as_euler_f64(const float *q, const char *seq, int degrees, int64_t n, double *out, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Motion velocities (SkeletonMotion.from_skeleton_state, poselib skeleton3d.py:1026-1049,
 * _compute_velocity :1126-1135, _compute_angular_velocity :1137-1146).
 * Time is the middle axis: nseq independent sequences of L frames of S channels.
 * weights: the 2*radius+1 Gaussian taps (scipy _gaussian_kernel1d, sigma=2 ->
 * radius 8, applied with mode='nearest' and float64 accumulation); NULL = no
 * smoothing.  tmp: caller-owned scratch of the output's size (required with
 * weights; the one-pass kernel, used while a 16-frame tile's raw rows fit
 * 48 KB of LDS, leaves it untouched; wider rows filter through it).
 * ---------------------------------------------------------------------- */
#define RTG_MAX_FILTER_RADIUS 16
/* p (nseq,L,S) -> out (nseq,L,S): np.gradient over frames / dt, then smoothing. */
int rtg_linear_velocity_f32(const float *p, int64_t nseq, int64_t L, int64_t S, float dt, const double *weights,
                            int32_t radius, float *tmp, float *out, rtg_stream_t stream);
/* r (nseq,L,J,4) global rotations -> out (nseq,L,J,3): axis*angle of
 * quat_mul_norm(r[t+1], conj(r[t])) / dt (last frame 0), then smoothing. */
int rtg_angular_velocity_f32(const float *r, int64_t nseq, int64_t L, int64_t J, float dt, const double *weights,
                             int32_t radius, float *tmp, float *out, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Synthetic mocap (bench / tests): FK of the VTRDYN_FULL zero pose with random
 * rotations, generated on the device from a counter-based RNG.
 * topo must be the 59-joint VTRDYN_FULL topology.  Frame f uses stream
 * (seed, frame_offset + f).  Outputs body (B,21,3), lh (B,20,3), rh (B,20,3)
 * and optionally body_rot (B,21,4), in the given layout.
 * ---------------------------------------------------------------------- */
int rtg_synth_full_body_f32(rtg_topology_t topo, uint64_t seed, int64_t frame_offset, int64_t B, int layout,
                            float *body, float *lh, float *rh, float *body_rot, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Box probe (diagnostics, no reference counterpart): what the current GPU delivers right now, so throughput
 * measured on one box can be set against another's.  Synchronous; allocates 2 GiB of scratch for its duration.
 * out (host, >= RTG_PROBE_FIELDS doubles):
 *   [0] shader clock under full VALU load, MHz (shader-cycle counter / 100 MHz wall clock, median workgroup)
 *   [1] f32 FMA issue rate, T lane-ops/s      [2] HBM copy bandwidth (read + write), GB/s
 *   [3] VALU kernel ms                        [4] copy kernel ms (1 GiB -> 1 GiB)     [5] compute units
 * ---------------------------------------------------------------------- */
#define RTG_PROBE_FIELDS 6
int rtg_box_probe(double *out, int32_t n_out, rtg_stream_t stream);

/* ------------------------------------------------------------------------
 * Side-kernel residency (diagnostics, no reference counterpart): how many workgroups of the throughput kernel that
 * rtg_retarget_f32 launches for this solver kind / gripper mode / input layout at a large batch the runtime keeps
 * resident on one compute unit (hipOccupancyMaxActiveBlocksPerMultiprocessor for its block size).  A workgroup is
 * RTG_SIDES_TILES x 128 threads (rtg_build_info), so with two tiles the figure is also the waves per SIMD.  Launches
 * nothing.
 * ---------------------------------------------------------------------- */
int rtg_side_kernel_residency(int kind, int precise_gripper, int layout, int32_t *blocks_per_cu);

#ifdef __cplusplus
}
#endif

#endif /* RTG_H */

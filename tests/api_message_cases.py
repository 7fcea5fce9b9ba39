"""A catalogue of named calls into the C ABI (rtg._lib) that end in an argument error -- or, for the handle
constructors on a machine without a device, in the failure of their first device call -- so that a status and the
text of rtg_last_error() can be recorded once (tools/record_api_messages.py -> tests/golden/api_messages.json) and
compared byte for byte afterwards (tests/test_api_messages_host.py, tests/test_gpu_api_messages.py).

``host_cases(lib)`` needs no device: NULL handles, never-dereferenced dummy addresses and small host arrays where a
check reads them.  A case whose name starts with ``nodev:`` is a valid call that fails at its first device call: run
it only where rtg_device_count() == 0 (with a device it would succeed and allocate).  ``gpu_cases(lib)`` needs live
handles (a device); every case there is still rejected before any launch.  Both yield ``(name, callable -> rc)``.
A case that returns RTG_OK is recorded with an empty message (rtg_last_error() keeps the previous failure's text)."""
from ctypes import POINTER, byref, c_double, c_float, c_int32, c_int64, c_void_p

import numpy as np

X = c_void_p(64)        # a dummy address no check dereferences
A0, A1, A2, A3 = (c_void_p(0x10000 + 0x4000 * i) for i in range(4))   # 16-byte aligned dummies, 16 KiB apart
ODD = c_void_p(0x10008)  # not 16-byte aligned
NODEV = "nodev:"


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32))
    return a, a.ctypes.data_as(POINTER(c_int32))


def _i64(a):
    a = np.ascontiguousarray(np.asarray(a, np.int64))
    return a, a.ctypes.data_as(POINTER(c_int64))


def _f32(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    return a, a.ctypes.data_as(POINTER(c_float))


def _named(group, name):
    """group/name, the nodev: mark moved to the front."""
    return f"{NODEV}{group}/{name[len(NODEV):]}" if name.startswith(NODEV) else f"{group}/{name}"


def _chain(J):
    return np.arange(-1, J - 1, dtype=np.int32)


def _fit_args(**kw):
    """rtg_dof_fit_f32's arguments: a NULL model and dummy addresses, fields overridden by name."""
    a = dict(model=None, target_pos=X, weight=X, root_rot=X, root_t=X, dof_in=X, B=1, clip=0, iters=1, lr=0.02,
             beta1=0.9, beta2=0.999, eps=1e-8, step0=0, m=X, v=X, dof_out=X, loss=X, grad=X, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return tuple(a.values())


def _pose_args(**kw):
    """rtg_dof_fit_root_f32's arguments, likewise."""
    a = dict(model=None, target_pos=X, weight=X, root_rot=X, root_t=X, dof_in=X, B=1, clip=0, fit_root=3, iters=1,
             lr=0.02, lr_root_t=0.02, lr_root_rot=0.02, beta1=0.9, beta2=0.999, eps=1e-8, step0=0, m=X, v=X,
             root_state=X, dof_out=X, root_rot_out=X, root_t_out=X, loss=X, grad=X, grad_root=X, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    return tuple(a.values())


NAN, INF = float("nan"), float("inf")
# (case, overrides) shared by the two fits: every check that needs no handle, then the edges that must fall through to
# the NULL-model message
FIT_COMMON = [
    ("null_model", {}), ("b_zero_null_model", dict(B=0)), ("b_negative", dict(B=-1)),
    ("iters_negative", dict(iters=-1)), ("iters_too_many", dict(iters=4097)), ("step0_negative", dict(step0=-1)),
    ("lr_nan", dict(lr=NAN)), ("lr_inf", dict(lr=INF)), ("eps_nan", dict(eps=NAN)), ("eps_neg_inf", dict(eps=-INF)),
    ("beta1_nan", dict(beta1=NAN)), ("beta1_one", dict(beta1=1.0)), ("beta1_negative", dict(beta1=-0.1)),
    ("beta2_inf", dict(beta2=INF)), ("beta2_one", dict(beta2=1.0)), ("beta2_negative", dict(beta2=-1e-3)),
    ("m_only", dict(v=None)), ("v_only", dict(m=None)),
    ("target_null", dict(target_pos=None)), ("root_rot_null", dict(root_rot=None)), ("root_t_null", dict(root_t=None)),
    ("edge_iters_zero", dict(iters=0)), ("edge_iters_max", dict(iters=4096)), ("edge_betas_zero", dict(beta1=0.0, beta2=0.0)),
    ("edge_no_weight", dict(weight=None)), ("edge_step0_max", dict(step0=2 ** 31 - 1)),
    ("edge_lr_eps_zero", dict(lr=0.0, eps=0.0)),
]
FIT_ONLY = [("every_output_null", dict(dof_out=None, loss=None, grad=None)), ("edge_no_state", dict(m=None, v=None)),
            ("edge_loss_only", dict(dof_out=None, grad=None))]
POSE_ONLY = [
    ("every_output_null", dict(dof_out=None, root_rot_out=None, root_t_out=None, loss=None, grad=None, grad_root=None)),
    ("fit_root_unknown_bit", dict(fit_root=4)), ("fit_root_negative", dict(fit_root=-1)),
    ("lr_root_t_nan", dict(lr_root_t=NAN)), ("lr_root_t_negative", dict(lr_root_t=-1.0)),
    ("lr_root_rot_inf", dict(lr_root_rot=INF)), ("lr_root_rot_negative", dict(lr_root_rot=-0.5)),
    ("root_state_without_moments", dict(m=None, v=None)), ("moments_without_root_state", dict(root_state=None)),
    ("edge_no_state", dict(m=None, v=None, root_state=None)), ("edge_fit_root_zero", dict(fit_root=0)),
    ("edge_lr_root_zero", dict(lr_root_t=0.0, lr_root_rot=0.0)),
    ("edge_loss_only", dict(dof_out=None, root_rot_out=None, root_t_out=None, grad=None, grad_root=None)),
]

# rtg_quat_op_f32's operand table (rtg.h rtg_quat_op): the ops that read b, and those that read c as well
QUAT_OPS_B = (0, 1, 3, 5, 8, 9, 11, 12, 20)
QUAT_OPS_C = (8, 11, 12, 20)


def _motion_args(topo=None, mlib=None, rot=0x10000, root=0x11000, vec=None, K=0, clip=0x12000, time=0x13000, N=4,
                 flags=0, lo=0x14000, ro=0x15000, vo=None, gr=None, gp=None):
    p = lambda x: None if x is None else c_void_p(x)   # noqa: E731
    return (topo, mlib, p(rot), p(root), p(vec), K, p(clip), p(time), N, flags, p(lo), p(ro), p(vo), p(gr), p(gp), None)


def host_cases(lib):
    """(name, callable -> rc): every check before a function's first use of a handle or of the device."""
    from rtg import _lib as L
    h = c_void_p()
    out = byref(h)

    # ---- rtg_topology_create: the tree checks
    fn = lib.rtg_topology_create
    lt_a, lt = _f32(np.full((3, 3), 0.1))
    for name, par, J, a_lt, a_out in (
            ("out_null", [-1, 0, 1], 3, lt, None), ("parents_null", None, 3, lt, out),
            ("local_t_null", [-1, 0, 1], 3, None, out), ("j_zero", [-1, 0, 1], 0, lt, out),
            ("j_too_large", [-1, 0, 1], 1025, lt, out), ("root_not_first", [0, 0, 1], 3, lt, out),
            ("parent_is_self", [-1, 1, 0], 3, lt, out), ("parent_negative", [-1, 0, -1], 3, lt, out),
            (NODEV + "valid", [-1, 0, 1], 3, lt, out)):
        pa, pp = (None, None) if par is None else _i32(par)
        yield _named("topology_create", name), \
            (lambda pp=pp, pa=pa, a_lt=a_lt, J=J, a_out=a_out, keep=lt_a: fn(pp, a_lt, None, J, a_out))
    for sym in ("rtg_topology_destroy", "rtg_dof_model_destroy", "rtg_retarget_plan_destroy", "rtg_solver_destroy",
                "rtg_server_inbox_free"):
        yield f"{sym[4:]}/null_is_ok", (lambda f=getattr(lib, sym): f(None))

    # ---- kinematics: the NULL-topology message of each entry point, the segment tables
    yield "fk/null_topology", lambda: lib.rtg_fk_f32(None, X, X, 1, X, X, None)
    yield "state_fk/null_topology", lambda: lib.rtg_state_fk_f32(None, X, X, 1, X, X, None)
    yield "local_rotation/null_topology", lambda: lib.rtg_local_rotation_f32(None, X, 1, X, None)
    yield "state_local_rotation/null_topology", lambda: lib.rtg_state_local_rotation_f32(None, X, 1, X, None)
    fseg = (L.FkSegment * 1)(L.FkSegment(None, 64, 64, 64, 64, 1))
    iseg = (L.LocalRotationSegment * 1)(L.LocalRotationSegment(None, 64, 64, 1))
    yield "fk_multi/n_negative", lambda: lib.rtg_fk_multi_f32(fseg, -1, None)
    yield "fk_multi/n_too_many", lambda: lib.rtg_fk_multi_f32(fseg, 9, None)
    yield "fk_multi/segments_null", lambda: lib.rtg_fk_multi_f32(None, 1, None)
    yield "fk_multi/null_topology", lambda: lib.rtg_fk_multi_f32(fseg, 1, None)
    yield "local_rotation_multi/n_negative", lambda: lib.rtg_local_rotation_multi_f32(iseg, -1, None)
    yield "local_rotation_multi/n_too_many", lambda: lib.rtg_local_rotation_multi_f32(iseg, 9, None)
    yield "local_rotation_multi/segments_null", lambda: lib.rtg_local_rotation_multi_f32(None, 1, None)
    yield "local_rotation_multi/null_topology", lambda: lib.rtg_local_rotation_multi_f32(iseg, 1, None)
    yield "kinematics_multi/n_fk_negative", lambda: lib.rtg_kinematics_multi_f32(fseg, -1, iseg, 1, None)
    yield "kinematics_multi/n_inv_negative", lambda: lib.rtg_kinematics_multi_f32(fseg, 1, iseg, -1, None)
    yield "kinematics_multi/too_many_in_total", lambda: lib.rtg_kinematics_multi_f32(fseg, 5, iseg, 4, None)
    yield "kinematics_multi/fk_null", lambda: lib.rtg_kinematics_multi_f32(None, 1, iseg, 1, None)
    yield "kinematics_multi/inv_null", lambda: lib.rtg_kinematics_multi_f32(fseg, 1, None, 1, None)
    yield "kinematics_multi/fk_null_topology", lambda: lib.rtg_kinematics_multi_f32(fseg, 1, iseg, 1, None)
    yield "kinematics_multi/inv_null_topology", lambda: lib.rtg_kinematics_multi_f32(None, 0, iseg, 1, None)

    # ---- the joint-angle model and the gradients
    yield "dof_model_create/out_null", lambda: lib.rtg_dof_model_create(None, None, None, None, None)
    yield "dof_model_create/null_topology", lambda: lib.rtg_dof_model_create(None, None, None, None, out)
    yield "dof_fk/null_model", lambda: lib.rtg_dof_fk_f32(None, X, X, X, 1, 0, X, X, None)
    bw = lib.rtg_dof_fk_backward_f32
    yield "dof_fk_backward/b_negative", lambda: bw(None, X, X, X, X, -1, 0, X, X, X, None)
    yield "dof_fk_backward/no_upstream", lambda: bw(None, X, X, None, None, 1, 0, X, X, X, None)
    yield "dof_fk_backward/no_output", lambda: bw(None, X, X, X, X, 1, 0, None, None, None, None)
    yield "dof_fk_backward/null_model", lambda: bw(None, X, X, X, None, 1, 0, None, None, X, None)
    yield "dof_fk_backward/b_zero_null_model", lambda: bw(None, None, None, None, None, 0, 0, None, None, None, None)
    fb = lib.rtg_fk_backward_f32
    yield "fk_backward/b_negative", lambda: fb(None, X, X, X, X, -1, X, X, None)
    yield "fk_backward/no_upstream", lambda: fb(None, X, X, None, None, 1, X, X, None)
    yield "fk_backward/no_output", lambda: fb(None, X, X, X, X, 1, None, None, None)
    yield "fk_backward/null_topology", lambda: fb(None, X, X, None, X, 1, X, None, None)
    yield "fk_backward/b_zero_null_topology", lambda: fb(None, None, None, None, None, 0, None, None, None)

    # ---- the two fits
    for name, kw in FIT_COMMON + FIT_ONLY:
        yield f"dof_fit/{name}", (lambda a=_fit_args(**kw): lib.rtg_dof_fit_f32(*a))
    for name, kw in FIT_COMMON + POSE_ONLY:
        yield f"dof_fit_root/{name}", (lambda a=_pose_args(**kw): lib.rtg_dof_fit_root_f32(*a))

    # ---- retarget_to: the tree checks of the tables, the mapping's reasons, the plan's own checks
    tab = lib.rtg_retarget_plan_tables
    ok3 = [-1, 0, 1]
    for name, sp, Js, tp, Jt, sj, tj in (
            ("parents_null", None, 3, ok3, 3, [0], [0]), ("tgt_parents_null", ok3, 3, None, 3, [0], [0]),
            ("src_root_not_first", [0, 0, 1], 3, ok3, 3, [0], [0]), ("tgt_root_not_first", ok3, 3, [1, 0, 1], 3, [0], [0]),
            ("src_parent_is_self", [-1, 1, 0], 3, ok3, 3, [0], [0]), ("tgt_parent_negative", ok3, 3, [-1, 0, -2], 3, [0], [0]),
            ("src_empty", ok3, 0, ok3, 3, [0], [0]), ("tgt_too_large", ok3, 3, _chain(65), 65, [0], [0]),
            ("mapping_empty", ok3, 3, ok3, 3, [], []), ("pair_out_of_range", ok3, 3, ok3, 3, [0, 3], [0, 1]),
            ("joint_twice", ok3, 3, ok3, 3, [0, 1, 1], [0, 1, 2]), ("root_dropped", ok3, 3, ok3, 3, [1], [1]),
            ("valid", ok3, 3, ok3, 3, [0, 2], [0, 1])):
        a = [(None, None) if x is None else _i32(x) for x in (sp, tp)] + [_i32(x if len(x) else [0]) for x in (sj, tj)]
        yield f"retarget_plan_tables/{name}", \
            (lambda a=a, Js=Js, Jt=Jt, K=len(sj): tab(a[0][1], Js, a[1][1], Jt, a[2][1], a[3][1], K, *([None] * 6)))
    yield "retarget_plan_tables/mapping_null", \
        (lambda a=_i32(ok3): tab(a[1], 3, a[1], 3, None, None, 1, *([None] * 6)))
    pc = lib.rtg_retarget_plan_create
    yield "retarget_plan_create/out_null", lambda: pc(None, None, None, None, 1, None, None, None, None, None, 1.0, None)
    yield "retarget_plan_create/null_topology", lambda: pc(None, None, None, None, 1, None, None, None, None, None, 1.0, out)
    yield "retarget_to/null_plan", lambda: lib.rtg_retarget_to_f32(None, X, X, 1, 1, X, X, None)

    # ---- ingest
    ing = lib.rtg_ingest_vtrdyn_f32
    yield "ingest_vtrdyn/b_negative", lambda: ing(X, X, X, -1, 0, X, X, X, X, None)
    yield "ingest_vtrdyn/bad_layout", lambda: ing(X, X, X, 1, 2, X, X, X, X, None)
    yield "ingest_vtrdyn/null_buffer", lambda: ing(X, X, X, 1, 1, X, X, X, None, None)
    yield "ingest_vtrdyn/b_zero_is_ok", lambda: ing(None, None, None, 0, 0, None, None, None, None, None)
    ric = lib.rtg_rot_ingest_create
    pre_a, pre = _f32([0, 0, 0, 1])
    post_a, post = _f32(np.tile([0, 0, 0, 1], (3, 1)))
    src_ok, src_bad, src_neg = _i32([2, 1, 0]), _i32([0, 3, 1]), _i32([0, 1, -1])
    for name, Ji, Jo, s, a_pre, a_post, a_out in (
            ("out_null", 3, 3, None, pre, post, None), ("j_in_zero", 0, 3, None, pre, post, out),
            ("j_out_too_large", 3, 65, None, pre, post, out), ("pre_null", 3, 3, None, None, post, out),
            ("post_null", 3, 3, None, pre, None, out), ("identity_needs_equal_j", 4, 3, None, pre, post, out),
            ("src_too_large", 3, 3, src_bad[1], pre, post, out), ("src_negative", 3, 3, src_neg[1], pre, post, out),
            (NODEV + "valid", 3, 3, src_ok[1], pre, post, out)):
        yield _named("rot_ingest_create", name), \
            (lambda Ji=Ji, Jo=Jo, s=s, a_pre=a_pre, a_post=a_post, a_out=a_out,
             keep=(pre_a, post_a, src_ok, src_bad, src_neg): ric(Ji, Jo, s, a_pre, a_post, a_out))
    ri = lib.rtg_rot_ingest_f32
    yield "rot_ingest/b_negative", lambda: ri(None, A0, -1, 0, A1, None)
    yield "rot_ingest/bad_layout", lambda: ri(None, A0, 1, 7, A1, None)
    yield "rot_ingest/q_null", lambda: ri(None, None, 1, 0, A1, None)
    yield "rot_ingest/out_null", lambda: ri(None, A0, 1, 1, None, None)
    yield "rot_ingest/q_misaligned", lambda: ri(None, ODD, 1, 0, A1, None)
    yield "rot_ingest/out_misaligned", lambda: ri(None, A0, 1, 0, ODD, None)
    yield "rot_ingest/null_handle", lambda: ri(None, A0, 1, 0, A1, None)
    yield "rot_ingest/b_zero_null_handle", lambda: ri(None, None, 0, 0, None, None)

    # ---- motion library and sampling
    mlc = lib.rtg_motion_lib_create
    for name, start, length, fps, F, a_out in (
            ("out_null", [0], [2], [30.0], 10, None), ("start_null", None, [2], [30.0], 10, out),
            ("len_null", [0], None, [30.0], 10, out), ("fps_null", [0], [2], None, 10, out),
            ("no_clips", [], [], [], 10, out), ("f_total_zero", [0], [2], [30.0], 0, out),
            ("f_total_too_large", [0], [2], [30.0], 2 ** 31, out), ("len_zero", [0], [0], [30.0], 10, out),
            ("start_negative", [-1], [2], [30.0], 10, out), ("past_f_total", [0, 8], [4, 3], [30.0, 30.0], 10, out),
            ("fps_nan", [0], [2], [NAN], 10, out), ("fps_inf", [0], [2], [INF], 10, out),
            ("fps_zero", [0], [2], [0.0], 10, out), ("fps_negative", [0], [2], [-30.0], 10, out),
            (NODEV + "valid", [0, 4], [4, 3], [30.0, 60.0], 10, out)):
        s, n, f = (None, None) if start is None else _i64(start or [0]), \
            (None, None) if length is None else _i32(length or [0]), (None, None) if fps is None else _f32(fps or [0])
        C = 0 if not length else len(length)
        if name in ("len_null",):
            C = 1
        yield _named("motion_lib_create", name), \
            (lambda s=s, n=n, f=f, C=C, F=F, a_out=a_out: mlc(s[1], n[1], f[1], C, F, a_out))
    ms = lib.rtg_motion_sample_f32
    G = L.MOTION_GLOBAL
    for name, kw in (("n_negative", dict(N=-1)), ("k_negative", dict(K=-1)), ("unknown_flags", dict(flags=64)),
                     ("vec_without_vec_out", dict(vec=0x16000, K=2)), ("vec_out_without_vec", dict(vo=0x16000, K=2)),
                     ("vec_with_k_zero", dict(vec=0x16000, vo=0x17000, K=0)),
                     ("g_rot_without_g_pos", dict(gr=0x16000)), ("g_pos_without_g_rot", dict(gp=0x16000)),
                     ("global_without_buffers", dict(flags=G)), ("buffers_without_global", dict(gr=0x16000, gp=0x17000)),
                     ("rot_null", dict(rot=None)), ("root_t_null", dict(root=None)), ("clip_null", dict(clip=None)),
                     ("time_null", dict(time=None)), ("local_rot_out_null", dict(lo=None)),
                     ("root_t_out_null", dict(ro=None)), ("rot_misaligned", dict(rot=0x10008)),
                     ("local_rot_out_misaligned", dict(lo=0x14008)),
                     ("g_rot_misaligned", dict(flags=G, gr=0x16008, gp=0x17000)),
                     ("n_zero_misaligned", dict(N=0, rot=0x10008)), ("null_topology", dict()),
                     ("n_zero_null_topology", dict(N=0))):
        yield f"motion_sample/{name}", (lambda a=_motion_args(**kw): ms(*a))

    # ---- motion-level prep
    yield "rescale_motion/null_topology", lambda: lib.rtg_rescale_motion_f32(None, X, 1, None, X, None)
    yield "quat_between/n_negative", lambda: lib.rtg_quat_between_f32(X, X, -1, X, X, None)
    yield "quat_between/null_workspace", lambda: lib.rtg_quat_between_f32(X, X, 1, X, None, None)
    yield "quat_between/n_zero_is_ok", lambda: lib.rtg_quat_between_f32(None, None, 0, None, None, None)
    yield "rebuild_vtrdyn/null_topology", lambda: lib.rtg_rebuild_vtrdyn_f32(None, X, 1, X, X, X, None)

    # ---- solvers: kinds and joint counts
    sc = lib.rtg_solver_create
    z59a, z59 = _f32(np.linspace(0.0, 1.0, 59 * 3).reshape(59, 3))
    z21a, z21 = _f32(np.linspace(0.0, 1.0, 21 * 3).reshape(21, 3))
    p21_bad = _chain(21)
    p21_bad[18] = 21
    p21b, p21 = _i32(_chain(21)), _i32(p21_bad)
    for name, kind, zl, zg, par, Js, a_out in (
            ("out_null", 0, z59, z59, None, 59, None), ("zl_null", 0, None, z59, None, 59, out),
            ("full_body_pos_joint_count", 0, z21, z21, None, 21, out), ("full_body_pos_needs_zg", 0, z59, None, None, 59, out),
            ("upper_body_joint_count", 1, z59, None, None, 59, out), ("full_body_rot_joint_count", 2, z21, None, None, 21, out),
            ("body_rot_joint_count", 3, z59, None, None, 59, out), ("body_rot_needs_parents", 3, z21, None, None, 21, out),
            ("body_rot_bad_parent", 3, z21, None, p21[1], 21, out), ("unknown_kind", 4, z21, None, None, 21, out),
            ("negative_kind", -1, z21, None, None, 21, out),
            (NODEV + "full_body_pos", 0, z59, z59, None, 59, out), (NODEV + "upper_body", 1, z21, None, None, 21, out),
            (NODEV + "full_body_rot", 2, z59, None, None, 59, out), (NODEV + "body_rot", 3, z21, None, p21b[1], 21, out)):
        yield _named("solver_create", name), \
            (lambda kind=kind, zl=zl, zg=zg, par=par, Js=Js, a_out=a_out, keep=(z59a, z21a, p21, p21b):
             sc(kind, zl, zg, par, Js, 1, a_out))
    yield "retarget/null_solver", lambda: lib.rtg_retarget_f32(None, X, X, X, None, 1, 0, X, None, None, None)

    # ---- the frame server
    yield "frame_server_launch/null_solver", lambda: lib.rtg_frame_server_launch(None, X, X, None, None, X, 100, None)
    yield "server_inbox_alloc/inbox_null", lambda: lib.rtg_server_inbox_alloc(None)
    yield NODEV + "server_inbox_alloc/valid", lambda: lib.rtg_server_inbox_alloc(byref(c_void_p()))
    yield "frame_server_signal/inbox_null", lambda: lib.rtg_frame_server_signal(None, 1)
    post = lib.rtg_frame_server_post
    for name, i in (("ctl_null", 0), ("in_null", 2), ("body_null", 3), ("left_hand_null", 4), ("right_hand_null", 5),
                    ("dof_null", 6)):
        a = [X, 1, X, X, X, X, X, X, X, X, X, X, 1000]
        a[i] = None
        yield f"frame_server_post/{name}", (lambda a=tuple(a): post(*a))
    yield "frame_server_post/seq_is_quit", lambda: post(X, L.SERVER_QUIT, X, X, X, X, X, X, X, X, X, X, 1000)
    yield "frame_server_post/local_rot_not_written", lambda: post(X, 1, X, X, X, X, X, None, X, X, X, None, 1000)
    yield "frame_server_post/body_rot_not_written", lambda: post(X, 1, X, X, X, X, X, X, None, X, None, X, 1000)

    # ---- primitives
    qo = lib.rtg_quat_op_f32
    yield "quat_op/op_negative", lambda: qo(-1, X, X, X, 1, X, None)
    yield "quat_op/op_too_large", lambda: qo(32, X, X, X, 1, X, None)
    yield "quat_op/n_negative", lambda: qo(0, X, X, X, -1, X, None)
    yield "quat_op/n_zero_is_ok", lambda: qo(0, None, None, None, 0, None, None)
    for op in range(32):
        yield f"quat_op/op{op}_a_null", (lambda op=op: qo(op, None, X, X, 1, X, None))
        yield f"quat_op/op{op}_out_null", (lambda op=op: qo(op, X, X, X, 1, None, None))
        if op in QUAT_OPS_B:
            yield f"quat_op/op{op}_b_null", (lambda op=op: qo(op, X, None, X, 1, X, None))
        if op in QUAT_OPS_C:
            yield f"quat_op/op{op}_c_null", (lambda op=op: qo(op, X, X, None, 1, X, None))
    cj = lib.rtg_cal_joint_quat_f32
    yield "cal_joint_quat/npts_zero", lambda: cj(X, X, 0, 1, X, None)
    yield "cal_joint_quat/npts_too_many", lambda: cj(X, X, 9, 1, X, None)
    yield "cal_joint_quat/n_negative", lambda: cj(X, X, 3, -1, X, None)
    yield "cal_joint_quat/null_buffer", lambda: cj(X, None, 3, 1, X, None)
    yield "cal_joint_quat/n_zero_is_ok", lambda: cj(None, None, 8, 0, None, None)
    for tag, call in (("quat_in_xyz_axis", lambda q, seq, n, o: lib.rtg_quat_in_xyz_axis_f32(q, seq, n, o, None)),
                      ("quat_as_euler", lambda q, seq, n, o: lib.rtg_quat_as_euler_f64(q, seq, 1, n, o, None))):
        for name, seq, n, q, o in (("seq_null", None, 1, X, X), ("seq_too_short", b"xy", 1, X, X),
                                   ("seq_too_long", b"xyzx", 1, X, X), ("bad_first_axis", b"wyz", 1, X, X),
                                   ("bad_last_axis", b"xy1", 1, X, X), ("mixed_case", b"xYz", 1, X, X),
                                   ("mixed_case_last", b"XYz", 1, X, X), ("repeated_axis", b"xxy", 1, X, X),
                                   ("repeated_axis_last", b"ZYY", 1, X, X), ("n_negative", b"xyz", -1, X, X),
                                   ("q_null", b"ZYX", 1, None, X), ("out_null", b"xyx", 1, X, None),
                                   ("n_zero_is_ok", b"XZX", 0, None, None)):
            yield f"{tag}/{name}", (lambda call=call, seq=seq, n=n, q=q, o=o: call(q, seq, n, o))

    # ---- velocities
    W = X   # the taps are read only after the radius check
    for tag, f in (("linear_velocity", lib.rtg_linear_velocity_f32), ("angular_velocity", lib.rtg_angular_velocity_f32)):
        for name, a in (("nseq_negative", (X, -1, 4, 3, 0.1, None, 0, None, X, None)),
                        ("length_negative", (X, 1, -4, 3, 0.1, None, 0, None, X, None)),
                        ("width_negative", (X, 1, 4, -3, 0.1, None, 0, None, X, None)),
                        ("empty_is_ok", (None, 0, 4, 3, 0.1, None, 0, None, None, None)),
                        ("one_frame", (X, 1, 1, 3, 0.1, None, 0, None, X, None)),
                        ("in_null", (None, 1, 4, 3, 0.1, None, 0, None, X, None)),
                        ("out_null", (X, 1, 4, 3, 0.1, None, 0, None, None, None)),
                        ("weights_without_tmp", (X, 1, 4, 3, 0.1, W, 8, None, X, None)),
                        ("radius_negative", (X, 1, 4, 3, 0.1, W, -1, X, X, None)),
                        ("radius_too_large", (X, 1, 4, 3, 0.1, W, 17, X, X, None))):
            if tag == "angular_velocity" and name == "one_frame":
                continue   # no such check there: a one-frame sequence has velocity 0 (the call would launch)
            yield f"{tag}/{name}", (lambda f=f, a=a: f(*a))

    # ---- diagnostics, synthetic input
    probe = (c_double * 6)()
    yield "box_probe/out_null", lambda: lib.rtg_box_probe(None, 6, None)
    yield "box_probe/out_too_short", lambda: lib.rtg_box_probe(probe, 5, None)
    yield NODEV + "box_probe/valid", lambda: lib.rtg_box_probe(probe, 6, None)
    n = c_int32()
    skr = lib.rtg_side_kernel_residency
    yield "side_kernel_residency/out_null", lambda: skr(0, 0, 0, None)
    yield "side_kernel_residency/kind_negative", lambda: skr(-1, 0, 0, byref(n))
    yield "side_kernel_residency/kind_too_large", lambda: skr(4, 0, 0, byref(n))
    yield "side_kernel_residency/bad_layout", lambda: skr(0, 1, 2, byref(n))
    yield NODEV + "side_kernel_residency/valid", lambda: skr(0, 1, 0, byref(n))
    syn = lib.rtg_synth_full_body_f32
    yield "synth_full_body/bad_layout", lambda: syn(None, 1, 0, 1, 2, X, X, X, None, None)
    yield "synth_full_body/null_topology", lambda: syn(None, 1, 0, 1, 0, X, X, X, None, None)


def gpu_cases(lib):
    """(name, callable -> rc): the checks behind a live handle.  Every case is rejected before any launch; the only
    device work is what creating a dozen tiny handles does.  The handles live as long as the generator's closures."""
    import os

    import torch

    from rtg import _lib as L
    from rtg import assets
    from rtg.runtime import DofModel, MotionLib, RetargetPlan, Solver, Topology

    def topo(J):
        return Topology(_chain(J), np.full((J, 3), 0.1, np.float32))

    t3, t21, t59, t65 = topo(3), topo(21), topo(59), topo(65)
    m3 = DofModel(t3, [0, 1])                       # no limits: clip is rejected
    m65 = DofModel(t65, np.zeros(64, np.int32), np.full(64, -1.0), np.full(64, 1.0))
    zp = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zero_pose.npz"))
    solvers = {}
    for kind, name in ((L.SOLVER_FULL_BODY_POS, "vtrdyn_full"), (L.SOLVER_UPPER_BODY, "vtrdyn"),
                       (L.SOLVER_FULL_BODY_ROT, "vtrdyn_full"), (L.SOLVER_BODY_ROT, "vtrdyn")):
        solvers[kind] = Solver(kind, zp[f"{name}_local_t"], zp[f"{name}_global_t"], assets.parents(name), False)
    mlib = MotionLib([0, 4], [4, 3], [30.0, 60.0], 8)
    ident = np.tile(np.array([0, 0, 0, 1], np.float32), (3, 1))
    plan = RetargetPlan(t3, t3, [0, 1, 2], [0, 1, 2], ident, np.zeros(3), ident, np.zeros(3), [0, 0, 0, 1], 1.0)
    keep = (t3, t21, t59, t65, m3, m65, solvers, mlib, plan)
    h = c_void_p()
    out = byref(h)
    T3, T21, T59, T65 = t3.handle, t21.handle, t59.handle, t65.handle
    # a real device buffer for the overlap cases: addresses inside it are never dereferenced either
    buf = torch.zeros(4096, device="cuda", dtype=torch.float32)
    base = buf.data_ptr()
    assert base % 16 == 0
    D = lambda off: c_void_p(base + off)   # noqa: E731

    # ---- kinematics behind a live topology
    yield "fk/b_negative", lambda: lib.rtg_fk_f32(T3, X, X, -1, X, X, None)
    yield "fk/null_buffer", lambda: lib.rtg_fk_f32(T3, X, None, 1, X, X, None)
    yield "fk/b_zero_is_ok", lambda: lib.rtg_fk_f32(T3, None, None, 0, None, None, None)
    yield "state_fk/b_negative", lambda: lib.rtg_state_fk_f32(T3, X, X, -2, X, X, None)
    yield "state_fk/null_buffer", lambda: lib.rtg_state_fk_f32(T3, X, X, 1, X, None, None)
    yield "local_rotation/b_negative", lambda: lib.rtg_local_rotation_f32(T3, X, -1, X, None)
    yield "local_rotation/null_buffer", lambda: lib.rtg_local_rotation_f32(T3, None, 1, X, None)
    yield "state_local_rotation/b_negative", lambda: lib.rtg_state_local_rotation_f32(T3, X, -1, X, None)
    yield "state_local_rotation/null_buffer", lambda: lib.rtg_state_local_rotation_f32(T3, X, 1, None, None)
    seg = lambda B, g_pos=64: (L.FkSegment * 2)(L.FkSegment(T3.value, 64, 64, 64, 64, 0),   # noqa: E731
                                                 L.FkSegment(T3.value, 64, 64, 64, g_pos, B))
    iseg = lambda B, lr=64: (L.LocalRotationSegment * 2)(L.LocalRotationSegment(T3.value, 64, 64, 0),   # noqa: E731
                                                          L.LocalRotationSegment(T3.value, 64, lr, B))
    yield "fk_multi/b_negative", (lambda s=seg(-1): lib.rtg_fk_multi_f32(s, 2, None))
    yield "fk_multi/null_buffer", (lambda s=seg(1, None): lib.rtg_fk_multi_f32(s, 2, None))
    yield "local_rotation_multi/b_negative", (lambda s=iseg(-1): lib.rtg_local_rotation_multi_f32(s, 2, None))
    yield "local_rotation_multi/null_buffer", (lambda s=iseg(1, None): lib.rtg_local_rotation_multi_f32(s, 2, None))
    yield "kinematics_multi/fk_b_negative", (lambda s=seg(-1), i=iseg(1): lib.rtg_kinematics_multi_f32(s, 2, i, 2, None))
    yield "kinematics_multi/fk_null_buffer", (lambda s=seg(1, None), i=iseg(1): lib.rtg_kinematics_multi_f32(s, 2, i, 2, None))
    yield "kinematics_multi/inv_b_negative", (lambda s=seg(0), i=iseg(-3): lib.rtg_kinematics_multi_f32(s, 2, i, 2, None))
    yield "kinematics_multi/inv_null_buffer", (lambda s=seg(0), i=iseg(1, None): lib.rtg_kinematics_multi_f32(s, 2, i, 2, None))

    # ---- the joint-angle model
    ax_ok, ax_bad, ax_neg = _i32([0, 2]), _i32([0, 3]), _i32([-1, 0])
    lim = _f32([-1.0, -1.0])
    dmc = lib.rtg_dof_model_create
    yield "dof_model_create/axis_null", lambda: dmc(T3, None, None, None, out)
    yield "dof_model_create/axis_too_large", lambda: dmc(T3, ax_bad[1], None, None, out)
    yield "dof_model_create/axis_negative", lambda: dmc(T3, ax_neg[1], None, None, out)
    yield "dof_model_create/lower_only", lambda: dmc(T3, ax_ok[1], lim[1], None, out)
    yield "dof_model_create/upper_only", lambda: dmc(T3, ax_ok[1], None, lim[1], out)
    M3, M65 = m3.handle, m65.handle
    yield "dof_fk/b_negative", lambda: lib.rtg_dof_fk_f32(M3, X, X, X, -1, 0, X, X, None)
    yield "dof_fk/clip_without_limits", lambda: lib.rtg_dof_fk_f32(M3, X, X, X, 1, 1, X, X, None)
    yield "dof_fk/dof_null", lambda: lib.rtg_dof_fk_f32(M3, None, X, X, 1, 0, X, X, None)
    yield "dof_fk/g_pos_null", lambda: lib.rtg_dof_fk_f32(M3, X, X, X, 1, 0, X, None, None)
    yield "dof_fk/b_zero_is_ok", lambda: lib.rtg_dof_fk_f32(M3, None, None, None, 0, 0, None, None, None)
    bw = lib.rtg_dof_fk_backward_f32
    yield "dof_fk_backward/clip_without_limits", lambda: bw(M3, X, X, X, X, 1, 1, X, X, X, None)
    yield "dof_fk_backward/dof_null", lambda: bw(M3, None, X, X, X, 1, 0, X, X, X, None)
    yield "dof_fk_backward/g_rot_null", lambda: bw(M3, X, None, X, X, 1, 0, X, X, X, None)
    yield "dof_fk_backward/b_zero_is_ok", lambda: bw(M3, None, None, None, None, 0, 0, None, None, None, None)
    fb = lib.rtg_fk_backward_f32
    yield "fk_backward/local_rot_null", lambda: fb(T3, None, X, X, X, 1, X, X, None)
    yield "fk_backward/g_rot_null", lambda: fb(T3, X, None, X, X, 1, X, X, None)
    yield "fk_backward/b_zero_is_ok", lambda: fb(T3, None, None, None, None, 0, None, None, None)
    for tag, f, args in (("dof_fit", lib.rtg_dof_fit_f32, _fit_args), ("dof_fit_root", lib.rtg_dof_fit_root_f32, _pose_args)):
        yield f"{tag}/clip_without_limits", (lambda f=f, a=args(model=M3, clip=1): f(*a))
        yield f"{tag}/too_many_joints", (lambda f=f, a=args(model=M65, clip=1): f(*a))
        yield f"{tag}/too_many_joints_b_zero", (lambda f=f, a=args(model=M65, B=0): f(*a))
        yield f"{tag}/dof_in_null", (lambda f=f, a=args(model=M3, dof_in=None): f(*a))
        yield f"{tag}/b_zero_is_ok", (lambda f=f, a=args(model=M3, B=0): f(*a))

    # ---- retarget_to
    pc = lib.rtg_retarget_plan_create
    q3, q65, z3 = _f32(ident), _f32(np.tile([0, 0, 0, 1], (65, 1))), _f32(np.zeros(3))
    R = _f32([0, 0, 0, 1])
    j012, j011, j12, j03 = _i32([0, 1, 2]), _i32([0, 1, 1]), _i32([1, 2]), _i32([0, 3])

    def plan_case(src=T3, tgt=T3, sj=j012, tj=j012, K=3, sq=q3, st=z3, tq=q3, tt=z3, rot=R):
        return lambda: pc(src, tgt, sj[1], tj[1], K, sq[1], st[1], tq[1], tt[1], rot[1], 1.0, out)

    yield "retarget_plan_create/tgt_null", plan_case(tgt=None)
    yield "retarget_plan_create/src_tpose_null", plan_case(sq=(None, None))
    yield "retarget_plan_create/tgt_root_t_null", plan_case(tt=(None, None))
    yield "retarget_plan_create/rotation_null", plan_case(rot=(None, None))
    yield "retarget_plan_create/too_many_joints", plan_case(src=T65, sq=q65)
    yield "retarget_plan_create/mapping_empty", plan_case(K=0)
    yield "retarget_plan_create/mapping_null", plan_case(sj=(None, None))
    yield "retarget_plan_create/pair_out_of_range", plan_case(sj=j03, tj=j03, K=2)
    yield "retarget_plan_create/joint_twice", plan_case(sj=j011)
    yield "retarget_plan_create/root_dropped", plan_case(sj=j12, tj=j12, K=2)
    P = plan.handle
    yield "retarget_to/b_negative", lambda: lib.rtg_retarget_to_f32(P, X, X, 1, -1, X, X, None)
    yield "retarget_to/null_buffer", lambda: lib.rtg_retarget_to_f32(P, X, X, 0, 1, X, None, None)
    yield "retarget_to/b_zero_is_ok", lambda: lib.rtg_retarget_to_f32(P, None, None, 1, 0, None, None, None)

    # ---- rotation ingest: one live handle (3 -> 3), the overlap test
    pre, post = _f32([0, 0, 0, 1]), _f32(ident)
    rh = c_void_p()
    rc = lib.rtg_rot_ingest_create(3, 3, None, pre[1], post[1], byref(rh))
    assert rc == 0, lib.rtg_last_error()
    ri = lib.rtg_rot_ingest_f32
    try:
        yield "rot_ingest/in_place", lambda: ri(rh, D(0), 4, 0, D(0), None)
        yield "rot_ingest/out_starts_inside_q", lambda: ri(rh, D(0), 4, 0, D(4 * 48 - 16), None)
        yield "rot_ingest/q_starts_inside_out", lambda: ri(rh, D(4 * 48 - 16), 4, 1, D(0), None)
        yield "rot_ingest/b_negative", lambda: ri(rh, D(0), -1, 0, D(1024), None)
        yield "rot_ingest/bad_layout", lambda: ri(rh, D(0), 1, -1, D(1024), None)
        yield "rot_ingest/q_misaligned", lambda: ri(rh, D(8), 1, 0, D(1024), None)
        yield "rot_ingest/b_zero_is_ok", lambda: ri(rh, None, 0, 1, None, None)

        # ---- motion sampling: handles, the joint limit, the overlap test (3 joints, 8 library rows, 4 queries, K = 2)
        ms = lib.rtg_motion_sample_f32
        ML = mlib.handle
        # a layout without overlaps, by byte offset into buf: rot 8*3*16 = 384, root_t 96, vec 8*2*12 = 192, clip 16,
        # time 16 | local_rot_out 192, root_t_out 48, vec_out 96, g_rot 192, g_pos 144
        lay = dict(rot=0, root=512, vec=768, clip=1024, time=1088, lo=2048, ro=2304, vo=2432, gr=2560, gp=2816)

        def sample(topo=T3, lib_=ML, N=4, K=2, flags=L.MOTION_GLOBAL, **kw):
            a = dict(lay)
            a.update(kw)
            a = {k: (None if v is None else base + v) for k, v in a.items()}
            return lambda: ms(*_motion_args(topo=topo, mlib=lib_, N=N, K=K, flags=flags, **a))

        yield "motion_sample/null_library", sample(lib_=None)
        yield "motion_sample/too_many_joints", sample(topo=T65)
        yield "motion_sample/too_many_joints_n_zero", sample(topo=T65, N=0)
        yield "motion_sample/n_zero_is_ok", sample(N=0)
        yield "motion_sample/local_rot_out_over_rot", sample(lo=368)
        yield "motion_sample/local_rot_out_over_root_t", sample(lo=512 + 80)
        yield "motion_sample/root_t_out_over_vec", sample(ro=768 + 188)
        yield "motion_sample/root_t_out_over_clip", sample(ro=1024 + 12)
        yield "motion_sample/vec_out_over_time", sample(vo=1088 + 12)
        yield "motion_sample/g_rot_over_rot", sample(gr=0)
        yield "motion_sample/g_pos_over_root_t", sample(gp=512 + 92)
        yield "motion_sample/local_rot_out_over_root_t_out", sample(ro=2048 + 188)
        yield "motion_sample/local_rot_out_over_g_pos", sample(gp=2048 - 140)
        yield "motion_sample/root_t_out_over_vec_out", sample(vo=2304 + 44)
        yield "motion_sample/vec_out_over_g_rot", sample(gr=2432 + 80)
        yield "motion_sample/g_rot_over_g_pos", sample(gp=2560 + 188)
        yield "motion_sample/no_vec_no_global_over_rot", sample(K=0, flags=0, vec=None, vo=None, gr=None, gp=None, ro=380)
        yield "motion_sample/rot_misaligned", sample(rot=8)

        # ---- motion-level prep, synthetic input: the joint counts
        yield "rescale_motion/b_negative", lambda: lib.rtg_rescale_motion_f32(T3, X, -1, None, X, None)
        yield "rescale_motion/null_buffer", lambda: lib.rtg_rescale_motion_f32(T3, X, 1, None, None, None)
        yield "rescale_motion/b_zero_is_ok", lambda: lib.rtg_rescale_motion_f32(T3, None, 0, None, None, None)
        rb = lib.rtg_rebuild_vtrdyn_f32
        yield "rebuild_vtrdyn/three_joints", lambda: rb(T3, X, 1, X, X, X, None)
        yield "rebuild_vtrdyn/fifty_nine_joints", lambda: rb(T59, X, 1, X, X, X, None)
        yield "rebuild_vtrdyn/b_negative", lambda: rb(T21, X, -1, X, X, X, None)
        yield "rebuild_vtrdyn/null_workspace", lambda: rb(T21, X, 1, X, X, None, None)
        yield "rebuild_vtrdyn/b_zero_is_ok", lambda: rb(T21, None, 0, None, None, None, None)
        syn = lib.rtg_synth_full_body_f32
        yield "synth_full_body/three_joints", lambda: syn(T3, 1, 0, 1, 0, X, X, X, None, None)
        yield "synth_full_body/twenty_one_joints", lambda: syn(T21, 1, 0, 1, 1, X, X, X, None, None)
        yield "synth_full_body/bad_layout", lambda: syn(T59, 1, 0, 1, 3, X, X, X, None, None)
        yield "synth_full_body/b_negative", lambda: syn(T59, 1, 0, -1, 0, X, X, X, None, None)
        yield "synth_full_body/offset_negative", lambda: syn(T59, 1, -1, 1, 0, X, X, X, None, None)
        yield "synth_full_body/null_buffer", lambda: syn(T59, 1, 0, 1, 0, X, X, None, None, None)
        yield "synth_full_body/b_zero_is_ok", lambda: syn(T59, 1, 0, 0, 0, None, None, None, None, None)

        # ---- solvers: the inputs of each kind
        rt = lib.rtg_retarget_f32
        need = {L.SOLVER_FULL_BODY_POS: 3, L.SOLVER_UPPER_BODY: 1, L.SOLVER_FULL_BODY_ROT: 4, L.SOLVER_BODY_ROT: 1}
        for kind, S in solvers.items():
            H = S.handle
            yield f"retarget/kind{kind}_b_negative", (lambda H=H: rt(H, X, X, X, X, -1, 0, X, None, None, None))
            yield f"retarget/kind{kind}_bad_layout", (lambda H=H: rt(H, X, X, X, X, 1, 2, X, None, None, None))
            yield f"retarget/kind{kind}_b_zero_is_ok", (lambda H=H: rt(H, None, None, None, None, 0, 1, None, None, None, None))
            yield f"retarget/kind{kind}_batch_too_large", (lambda H=H: rt(H, X, X, X, X, 0x7fffffff * 256 + 1, 0, X, None, None, None))
            yield f"retarget/kind{kind}_dof_null", (lambda H=H: rt(H, X, X, X, X, 1, 0, None, None, None, None))
            for i in range(4):
                ins = [X if k < need[kind] else None for k in range(4)]
                ins[i] = None if i < need[kind] else X
                yield f"retarget/kind{kind}_input{i}_{'null' if i < need[kind] else 'given'}", \
                    (lambda H=H, ins=tuple(ins): rt(H, *ins, 1, 0, X, None, None, None))
            if kind != L.SOLVER_FULL_BODY_POS:
                ins = [X if k < need[kind] else None for k in range(4)]
                yield f"retarget/kind{kind}_body_rot", (lambda H=H, ins=tuple(ins): rt(H, *ins, 1, 0, X, None, X, None))
                yield f"frame_server_launch/kind{kind}", (lambda H=H: lib.rtg_frame_server_launch(H, X, X, None, None, X, 100, None))
        fsl = lib.rtg_frame_server_launch
        H0 = solvers[L.SOLVER_FULL_BODY_POS].handle
        yield "frame_server_launch/in_null", lambda: fsl(H0, None, X, None, None, X, 100, None)
        yield "frame_server_launch/dof_null", lambda: fsl(H0, X, None, None, None, X, 100, None)
        yield "frame_server_launch/ctl_null", lambda: fsl(H0, X, X, X, X, None, 100, None)
        yield "frame_server_launch/idle_zero", lambda: fsl(H0, X, X, None, None, X, 0, None)
        yield "frame_server_launch/idle_too_long", lambda: fsl(H0, X, X, None, None, X, 60001, None)
    finally:
        lib.rtg_rot_ingest_destroy(rh)
        del keep


def run(cases, lib, no_device_cases: bool):
    """{name: [rc, message]} of the cases; ``nodev:`` cases only where asked for (no device is visible)."""
    res = {}
    for name, call in cases:
        if name.startswith(NODEV) and not no_device_cases:
            continue
        assert name not in res, f"duplicate case name {name}"
        rc = int(call())
        res[name] = [rc, lib.rtg_last_error().decode() if rc != 0 else ""]
    return res


def comparable(name, entry):
    """What of a recorded / observed entry is ours: a device failure's text up to and including the first ': ' (what
    follows is the HIP runtime's)."""
    rc, msg = entry
    if name.startswith(NODEV) and ": " in msg:
        msg = msg[:msg.index(": ") + 2]
    return [rc, msg]

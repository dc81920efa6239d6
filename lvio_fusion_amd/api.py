"""Thin numpy-facing handles over the C-ABI (include/lvf.h).  Used by tests/ and bench.py; the C++ adapter
(include/lvf_ceres_adapter.hpp) is the reference-shaped host interface.  Everything here runs on the GPU —
errors from the library are raised, never papered over."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LidarExtractDebug, LidarParams, WindowOptions, Camera, IcpOptions, IcpSummary, ScanMatchJob, ScanMatchOptions, ScanMatchResult, EdgeIcpOptions, EdgeParams, EdgeExtractDebug, SolverOptions, SolverSummary, NavsatBcOptions, NavsatBcResult, FlowOptions, OrbOptions, Distortion

POSES, VEL, BA, BG, INV_DEPTH, W_VISUAL = range(6)
IMU_BLOCK_SIZES = (7, 3, 3, 3, 7, 3, 3, 3)


class LvfError(RuntimeError):
    pass


def _chk(rc):
    if rc != 0:
        raise LvfError(f"lvf error {rc}: {_lib.lib().lvf_last_error().decode()}")


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _dp(a):
    return a.ctypes.data_as(_lib.c_double_p)


def _ip(a):
    return a.ctypes.data_as(_lib.c_int_p)


def make_camera(c):
    k = Camera()
    k.fx, k.fy, k.cx, k.cy = c["fx"], c["fy"], c["cx"], c["cy"]
    for i in range(7):
        k.extrinsic[i] = float(c["extrinsic"][i])
    return k


class Context:
    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        _chk(_lib.lib().lvf_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self.h)))
        self.L = _lib.lib()

    def synchronize(self):
        _chk(self.L.lvf_ctx_synchronize(self.h))

    def timer_begin(self):
        _chk(self.L.lvf_timer_begin(self.h))

    def timer_end(self):
        _chk(self.L.lvf_timer_end(self.h))

    def timer_ms(self):
        ms = C.c_float()
        _chk(self.L.lvf_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            self.L.lvf_ctx_destroy(self.h)
            self.h = C.c_void_p()


class State:
    def __init__(self, ctx, n_kf, n_lm):
        self.ctx, self.n_kf, self.n_lm = ctx, n_kf, n_lm
        self.h = C.c_void_p()
        _chk(ctx.L.lvf_state_create(ctx.h, n_kf, n_lm, C.byref(self.h)))

    def _size(self, field):
        return {POSES: 7 * self.n_kf, VEL: 3 * self.n_kf, BA: 3 * self.n_kf, BG: 3 * self.n_kf, INV_DEPTH: self.n_lm,
                W_VISUAL: self.n_kf}[field]

    def set(self, field, arr):
        a = _d(arr)
        if a.size != self._size(field):
            raise ValueError(f"state field {field}: expected {self._size(field)} doubles, got {a.size}")
        _chk(self.ctx.L.lvf_state_set(self.h, field, _dp(a)))

    def get(self, field):
        out = np.empty(self._size(field))
        _chk(self.ctx.L.lvf_state_get(self.h, field, _dp(out)))
        return out

    def copy_from(self, other):
        """device-to-device copy of every field (asynchronous)"""
        _chk(self.ctx.L.lvf_state_copy(self.h, other.h))

    def close(self):
        if self.h:
            self.ctx.L.lvf_state_destroy(self.h)
            self.h = C.c_void_p()


class Batch:
    """One functor type's residual blocks.  evaluate() == batched CostFunction::Evaluate."""

    def __init__(self, ctx, h, n, n_res, block_sizes):
        self.ctx, self.h, self.n, self.n_res, self.block_sizes = ctx, h, n, n_res, tuple(block_sizes)

    def evaluate(self, state=None, rpyxyz=None, jacobians=True):
        r = _d(rpyxyz) if rpyxyz is not None else None
        _chk(self.ctx.L.lvf_batch_evaluate(self.h, state.h if state is not None else None, _dp(r) if r is not None else None,
                                           1 if jacobians else 0))

    def residuals(self):
        out = np.empty((self.n, self.n_res))
        _chk(self.ctx.L.lvf_batch_download_residuals(self.h, _dp(out)))
        return out

    def jacobian(self, block):
        out = np.empty((self.n, self.n_res, self.block_sizes[block]))
        _chk(self.ctx.L.lvf_batch_download_jacobian(self.h, block, _dp(out)))
        return out

    def evaluate_local(self, state, huber_a=0.0, jacobians=True):
        """Problem::Evaluate-shaped outputs: robustified residuals [n][R] and LOCAL Jacobians [n][R][L]."""
        L = self.ctx.L.lvf_batch_local_columns(self.h)
        r = np.empty((self.n, self.n_res)); J = np.empty((self.n, self.n_res, L)) if jacobians else None
        _chk(self.ctx.L.lvf_batch_evaluate_local(self.h, state.h, C.c_double(huber_a), _dp(r), _dp(J) if jacobians else None))
        return r, J

    def set_block_weights(self, weight):
        w = None if weight is None else _d(weight)
        _chk(self.ctx.L.lvf_two_camera_set_block_weights(self.h, _dp(w) if w is not None else None))

    def normals(self):
        out = np.empty((self.n, 3))
        _chk(self.ctx.L.lvf_batch_download_normals(self.h, _dp(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.L.lvf_batch_destroy(self.h)
            self.h = C.c_void_p()


def pose_only_batch(ctx, cam0, ob, kf_idx, pw_idx, pw):
    ob, pw, kf_idx, pw_idx = _d(ob), _d(pw), _i(kf_idx), _i(pw_idx)
    h = C.c_void_p()
    cam = make_camera(cam0)
    _chk(ctx.L.lvf_pose_only_create(ctx.h, C.byref(cam), ob.shape[0], _dp(ob), _ip(kf_idx), _ip(pw_idx), pw.shape[0], _dp(pw), C.byref(h)))
    return Batch(ctx, h, ob.shape[0], 2, (7,))


def two_frame_batch(ctx, left, right, first_ob, ob, lm_idx, kf1_idx, kf2_idx):
    first_ob, ob = _d(first_ob), _d(ob)
    lm_idx, kf1_idx, kf2_idx = _i(lm_idx), _i(kf1_idx), _i(kf2_idx)
    h = C.c_void_p()
    cl, cr = make_camera(left), make_camera(right)
    _chk(ctx.L.lvf_two_frame_create(ctx.h, C.byref(cl), C.byref(cr), ob.shape[0], _dp(first_ob), _dp(ob), _ip(lm_idx), _ip(kf1_idx),
                                    _ip(kf2_idx), C.byref(h)))
    return Batch(ctx, h, ob.shape[0], 2, (1, 7, 7))


def two_camera_batch(ctx, left, right, left_ob, right_ob, lm_idx, kf_idx):
    left_ob, right_ob, lm_idx, kf_idx = _d(left_ob), _d(right_ob), _i(lm_idx), _i(kf_idx)
    h = C.c_void_p()
    cl, cr = make_camera(left), make_camera(right)
    _chk(ctx.L.lvf_two_camera_create(ctx.h, C.byref(cl), C.byref(cr), left_ob.shape[0], _dp(left_ob), _dp(right_ob), _ip(lm_idx),
                                     _ip(kf_idx), C.byref(h)))
    return Batch(ctx, h, left_ob.shape[0], 2, (1,))


def imu_batch(ctx, pre, kf_i, kf_j):
    pre, kf_i, kf_j = _d(pre), _i(kf_i), _i(kf_j)
    assert pre.ndim == 2 and pre.shape[1] == 467
    h = C.c_void_p()
    _chk(ctx.L.lvf_imu_create(ctx.h, pre.shape[0], _dp(pre), _ip(kf_i), _ip(kf_j), C.byref(h)))
    return Batch(ctx, h, pre.shape[0], 15, IMU_BLOCK_SIZES)


def lidar_plane_batch(ctx, mode, p, pa, pb, pc, Twc1, weight):
    p, pa, pb, pc, Twc1 = map(_d, (p, pa, pb, pc, Twc1))
    h = C.c_void_p()
    _chk(ctx.L.lvf_lidar_plane_create(ctx.h, int(mode), p.shape[0], _dp(p), _dp(pa), _dp(pb), _dp(pc), _dp(Twc1), float(weight), C.byref(h)))
    return Batch(ctx, h, p.shape[0], 1, (1, 1, 1))


class LidarPoseBatch(Batch):
    """LiDAR planes on keyframe poses (lvf_lidar_pose_*): a Batch with its inputs readable."""

    def num_valid(self):
        """blocks of weight > 0; on a device-built batch the one call that waits for the gather"""
        n = C.c_int()
        _chk(self.ctx.L.lvf_lidar_pose_num_valid(self.h, C.byref(n)))
        return n.value

    def download(self):
        """dict(p, pa [n][3], kf_idx, weight, huber_a [n]) as the device holds them"""
        p, pa = np.empty((self.n, 3)), np.empty((self.n, 3))
        kf, w, a = np.empty(self.n, np.int32), np.empty(self.n), np.empty(self.n)
        _chk(self.ctx.L.lvf_lidar_pose_download(self.h, _dp(p), _dp(pa), _ip(kf), _dp(w), _dp(a)))
        return dict(p=p, pa=pa, kf_idx=kf, weight=w, huber_a=a)


def _opt_d(a, n):
    if a is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), (n,)))


def lidar_pose_batch(ctx, p, pa, pb, pc, kf_idx, weight=None, huber_a=None):
    """LidarPlaneError<1,7> blocks on pose[kf_idx[i]] (lvf_lidar_pose_create): p in the keyframe's body frame, pa, pb, pc in the world frame;
    weight (None = 1) and huber_a (None or <= 0 = no loss) per block or scalar."""
    p, pa, pb, pc, kf_idx = _d(p).reshape(-1, 3), _d(pa).reshape(-1, 3), _d(pb).reshape(-1, 3), _d(pc).reshape(-1, 3), _i(kf_idx)
    n = p.shape[0]
    w, a = _opt_d(weight, n), _opt_d(huber_a, n)
    h = C.c_void_p()
    _chk(ctx.L.lvf_lidar_pose_create(ctx.h, n, _dp(p), _dp(pa), _dp(pb), _dp(pc), _ip(kf_idx), _dp(w) if w is not None else None,
                                     _dp(a) if a is not None else None, C.byref(h)))
    return LidarPoseBatch(ctx, h, n, 1, (7,))


def lidar_pose_from_scans(ctx, maps, scans, kf_idx, weight=None, huber_a=None):
    """The same batch gathered on the device from what knn3 left in each (map, scan) pair (lvf_lidar_pose_from_scans): scan k's queries are
    blocks on keyframe kf_idx[k] (non-decreasing); a query that failed the gate is a block of weight 0.  Nothing is waited for."""
    n = len(scans)
    kf_idx = _i(kf_idx)
    w, a = _opt_d(weight, n), _opt_d(huber_a, n)
    hm = (C.c_void_p * max(n, 1))(*[m.h for m in maps]); hs = (C.c_void_p * max(n, 1))(*[s.h for s in scans])
    h = C.c_void_p()
    _chk(ctx.L.lvf_lidar_pose_from_scans(ctx.h, n, hm, hs, _ip(kf_idx), _dp(w) if w is not None else None, _dp(a) if a is not None else None, C.byref(h)))
    return LidarPoseBatch(ctx, h, sum(s.Q for s in scans), 1, (7,))


def pose_prior_batch(ctx, kf_a, kf_b, target, weight, v):
    """kf_a[i] < 0: PoseError on pose kf_b[i] with origin target[i][:7]; else PoseGraphError(kf_a, kf_b) with
    target[i][:6] = rpyxyz_ (see relative_rpyxyz)."""
    kf_a, kf_b, target, weight, v = _i(kf_a), _i(kf_b), _d(target), _d(weight), _d(v)
    n = kf_a.shape[0]
    assert target.shape == (n, 7)
    h = C.c_void_p()
    _chk(ctx.L.lvf_pose_prior_create(ctx.h, n, _ip(kf_a), _ip(kf_b), _dp(target), _dp(weight), _dp(v), C.byref(h)))
    return Batch(ctx, h, n, 6, (7, 7))


def relative_rpyxyz(last_pose, pose):
    a, b, out = _d(last_pose), _d(pose), np.empty(6)
    _chk(_lib.lib().lvf_relative_rpyxyz(_dp(a), _dp(b), _dp(out)))
    return out


def relocate_r_evaluate(ctx, relocated, unrelocated, q4, jacobians=True):
    """RelocateRError <7,4> batched: returns r[n][7], J[n][7][4] (ambient) or None."""
    a, b, q = _d(relocated), _d(unrelocated), _d(q4)
    n = a.shape[0]
    r = np.empty((n, 7)); J = np.empty((n, 7, 4)) if jacobians else None
    _chk(ctx.L.lvf_relocate_r_evaluate(ctx.h, n, _dp(a), _dp(b), _dp(q), _dp(r), _dp(J) if jacobians else None))
    return r, J


def relocate_rotation_solve(ctx, relocated, unrelocated, q4, opt=None):
    """Relocator::UpdateNewSubmap's rotation solve; returns (q4_new, SolverSummary)."""
    a, b = _d(relocated), _d(unrelocated)
    q = _d(q4).copy()
    opt = opt or default_solver_options()
    summ = _lib.SolverSummary()
    _chk(ctx.L.lvf_relocate_rotation_solve(ctx.h, a.shape[0], _dp(a), _dp(b), _dp(q), C.byref(opt), C.byref(summ)))
    return q, summ


def forward_update(ctx, transform, poses, vw=None):
    """PoseGraph::ForwardUpdate on host arrays; returns updated copies."""
    T = _d(transform); P = _d(poses).copy(); V = None if vw is None else _d(vw).copy()
    _chk(ctx.L.lvf_forward_update(ctx.h, _dp(T), P.shape[0], _dp(P), _dp(V) if V is not None else None))
    return P, V


def navsat_init_evaluate(ctx, p0, p1, cov, x3, jacobians=True):
    """NavsatInitError <3,1,1,1> batched at x3 = (yaw, x, y): returns r[n][3], J[n][3][3] or None."""
    a, b, c, x = _d(p0).reshape(-1, 3), _d(p1).reshape(-1, 3), _d(cov).reshape(-1, 3), _d(x3)
    n = a.shape[0]
    r = np.empty((n, 3)); J = np.empty((n, 3, 3)) if jacobians else None
    _chk(ctx.L.lvf_navsat_init_evaluate(ctx.h, n, _dp(a), _dp(b), _dp(c), _dp(x), _dp(r), _dp(J) if jacobians else None))
    return r, J


def navsat_rx_evaluate(ctx, p0, p1, pose, cov, x6, jacobians=True):
    """NavsatRXError <3,1,1,1,1,1,1> batched at x6 = (yaw, pitch, roll, x, y, z): returns r[n][3], J[n][3][6] or None."""
    a, b, c, P, x = _d(p0).reshape(-1, 3), _d(p1).reshape(-1, 3), _d(cov).reshape(-1, 3), _d(pose), _d(x6)
    n = a.shape[0]
    r = np.empty((n, 3)); J = np.empty((n, 3, 6)) if jacobians else None
    _chk(ctx.L.lvf_navsat_rx_evaluate(ctx.h, n, _dp(a), _dp(b), _dp(P), _dp(c), _dp(x), _dp(r), _dp(J) if jacobians else None))
    return r, J


def navsat_r_evaluate(ctx, y3, pose, roll, jacobians=True):
    """NavsatRError <1,1>: returns (residual, d residual / d roll or None)."""
    y, P = _d(y3), _d(pose)
    r, J = C.c_double(), C.c_double()
    _chk(ctx.L.lvf_navsat_r_evaluate(ctx.h, _dp(y), _dp(P), C.c_double(roll), C.byref(r), C.byref(J) if jacobians else None))
    return r.value, (J.value if jacobians else None)


def navsat_initialize(ctx, position, raw, cov, opt=None):
    """Navsat::Initialize; returns (para6, extrinsic7, summary of stage 1, summary of stage 2)."""
    a, b, c = _d(position).reshape(-1, 3), _d(raw).reshape(-1, 3), _d(cov).reshape(-1, 3)
    opt = opt or default_solver_options()
    para, ext = np.empty(6), np.empty(7)
    s1, s2 = _lib.SolverSummary(), _lib.SolverSummary()
    _chk(ctx.L.lvf_navsat_initialize(ctx.h, a.shape[0], _dp(a), _dp(b), _dp(c), C.byref(opt), _dp(para), _dp(ext), C.byref(s1), C.byref(s2)))
    return para, ext, s1, s2


def navsat_bc_options(**kw):
    o = NavsatBcOptions()
    _lib.lib().lvf_navsat_bc_options_default(C.byref(o))
    for k, v in kw.items():
        if k == "solver":
            o.solver = v
        else:
            getattr(o, k)          # (an unknown field is an error, not a new attribute)
            setattr(o, k, v)
    return o


def navsat_optimize_bc(ctx, poses, n_active, has_fix, fix_point, cov, opt):
    """Navsat::OptimizeBC on the host array `poses` ([n_active + n_update][7], frame first), updated IN PLACE; returns NavsatBcResult."""
    if not (isinstance(poses, np.ndarray) and poses.dtype == np.float64 and poses.flags.c_contiguous):
        raise TypeError("poses must be a C-contiguous float64 array (it is updated in place)")
    n = int(n_active)
    total = poses.size // 7
    h, f, c = _i(has_fix), _d(fix_point).reshape(-1, 3), _d(cov).reshape(-1, 3)
    if not (0 <= n <= total and h.size == n and f.shape[0] == n and c.shape[0] == n):
        raise ValueError("navsat_optimize_bc: has_fix / fix_point / cov must have one entry per active keyframe")
    res = NavsatBcResult()
    _chk(ctx.L.lvf_navsat_optimize_bc(ctx.h, n, total - n, _dp(poses), _ip(h), _dp(f), _dp(c), C.byref(opt), C.byref(res)))
    return res


def navsat_fix_chain(ctx, poses, has_fix, fix_point, cov, huber_a=0.1, opt=None):
    """The per-keyframe loop of Navsat::Optimize / QuickFix on the host array `poses` ([n][7]: the keyframes after B, C last), updated IN
    PLACE; returns (x[n-1], iterations[n-1], SolverSummary)."""
    if not (isinstance(poses, np.ndarray) and poses.dtype == np.float64 and poses.flags.c_contiguous):
        raise TypeError("poses must be a C-contiguous float64 array (it is updated in place)")
    n = poses.size // 7
    steps = max(n - 1, 0)
    h, f, c = _i(has_fix), _d(fix_point).reshape(-1, 3), _d(cov).reshape(-1, 3)
    if not (h.size == steps and f.shape[0] == steps and c.shape[0] == steps):
        raise ValueError("navsat_fix_chain: has_fix / fix_point / cov must have n - 1 entries")
    opt = opt or default_solver_options()
    x, it = np.zeros(steps), np.zeros(steps, np.int32)
    summ = _lib.SolverSummary()
    _chk(ctx.L.lvf_navsat_fix_chain(ctx.h, n, _dp(poses), _ip(h), _dp(f), _dp(c), C.c_double(huber_a), C.byref(opt), _dp(x), _ip(it), C.byref(summ)))
    return x, it, summ


def navsat_quick_fix(ctx, poses, has_fix, fix_point, cov, bc_opt, between=None):
    """Navsat::QuickFix's two steps (navsat.cpp:169-176) on poses [n][7] = the keyframes B .. C in time order, updated in place:
    OptimizeBC(B, C, mode 0) over all of them, then the per-keyframe chain over the keyframes strictly after B.  has_fix / fix_point / cov have
    one entry per keyframe.  `between` (navsat_optimize's OptimizeAB) runs between the two.  Host composition only.
    Returns (NavsatBcResult, x, iterations, chain summary)."""
    n = poses.size // 7
    h, f, c = _i(has_fix), _d(fix_point).reshape(-1, 3), _d(cov).reshape(-1, 3)
    o = NavsatBcOptions.from_buffer_copy(bc_opt)
    o.mode = 0
    res = navsat_optimize_bc(ctx, poses, n, h, f, c, o)
    if between is not None:
        between(poses)
    tail = poses.reshape(-1, 7)[1:]
    x, it, summ = navsat_fix_chain(ctx, tail, h[1:n - 1], f[1:n - 1], c[1:n - 1], o.huber_a, o.solver) if n >= 1 else (np.zeros(0), np.zeros(0, np.int32), _lib.SolverSummary())
    return res, x, it, summ


def navsat_optimize(ctx, poses, has_fix, fix_point, cov, bc_opt, optimize_ab):
    """Navsat::Optimize (navsat.cpp:135-156): OptimizeBC(B, C, mode 0), the caller's OptimizeAB (a callable handed the pose array, run on
    the host; navsat_optimize_section runs that step on the device), then the per-keyframe chain."""
    return navsat_quick_fix(ctx, poses, has_fix, fix_point, cov, bc_opt, between=optimize_ab)


CHAIN_NONE, CHAIN_T, CHAIN_R = 0, 1, 2


def pose_chain_capacity():
    return int(_lib.lib().lvf_pose_chain_capacity())


def _chain_args(poses, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight):
    n = poses.size // 7
    tg = None if edge_target is None else _d(edge_target).reshape(-1, 6)
    ew, ev, uk, ut, uw = _d(edge_weight).ravel(), _d(edge_v).ravel(), _i(unary_kind).ravel(), _d(unary_target).reshape(-1, 4), _d(unary_weight).ravel()
    m1 = max(n - 1, 0)
    if not ((tg is None or tg.shape[0] == m1) and ew.size == m1 and ev.size == m1 and uk.size == n and ut.shape[0] == n and uw.size == n):
        raise ValueError("pose chain: edge arrays have n - 1 entries, unary arrays n")
    keep = (tg, ew, ev, uk, ut, uw)
    return n, keep, (_dp(tg) if tg is not None else None, _dp(ew), _dp(ev), _ip(uk), _dp(ut), _dp(uw))


def pose_chain_solve(ctx, poses, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight, huber_a=0.0, opt=None):
    """The pose-chain solve (lvf_pose_chain_solve) on the host array `poses` ([n][7], both ends constant), updated IN PLACE.  edge_target
    [n-1][6] or None (taken from the poses as they come), edge_weight / edge_v [n-1]; unary_kind [n] (CHAIN_NONE / CHAIN_T / CHAIN_R),
    unary_target [n][4] (p3 or q4), unary_weight [n].  Returns SolverSummary."""
    if not (isinstance(poses, np.ndarray) and poses.dtype == np.float64 and poses.flags.c_contiguous):
        raise TypeError("poses must be a C-contiguous float64 array (it is updated in place)")
    n, keep, ptrs = _chain_args(poses, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight)
    opt = opt or default_solver_options()
    summ = _lib.SolverSummary()
    _chk(ctx.L.lvf_pose_chain_solve(ctx.h, n, _dp(poses), *ptrs, C.c_double(huber_a), C.byref(opt), C.byref(summ)))
    return summ


def pose_chain_debug_step(ctx, poses, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight, huber_a, radius):
    """One linearisation at `poses` and one damped solve at `radius` (Jacobi scaling from this linearisation); nothing is written back.
    Returns dict(dx [6 (n-2)], model, cost, fail)."""
    P = _d(poses)
    n, keep, ptrs = _chain_args(P, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight)
    dx = np.zeros(6 * max(n - 2, 0))
    model, cost, fail = C.c_double(), C.c_double(), C.c_int32()
    _chk(ctx.L.lvf_pose_chain_debug_step(ctx.h, n, _dp(P), *ptrs, C.c_double(huber_a), C.c_double(radius), _dp(dx), C.byref(model), C.byref(cost), C.byref(fail)))
    return dict(dx=dx, model=model.value, cost=cost.value, fail=bool(fail.value))


def pose_chain_debug_system(ctx, poses, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight, huber_a=0.0):
    """The undamped normal equations of one linearisation: D [m][6][6], O [m-1][6][6] (block-row i+1, block-column i), g [6 m]; m = n - 2."""
    P = _d(poses)
    n, keep, ptrs = _chain_args(P, edge_target, edge_weight, edge_v, unary_kind, unary_target, unary_weight)
    m = max(n - 2, 0)
    D, O, g = np.zeros((m, 6, 6)), np.zeros((max(m - 1, 0), 6, 6)), np.zeros(6 * m)
    _chk(ctx.L.lvf_pose_chain_debug_system(ctx.h, n, _dp(P), *ptrs, C.c_double(huber_a), _dp(D), _dp(O), _dp(g)))
    return D, O, g


def navsat_optimize_ab(ctx, poses, stamps, fix_point, relative_B, huber_a=0.1, opt=None):
    """Navsat::OptimizeAB on the host array `poses` ([n][7] = A, the keyframes of AB, B), updated IN PLACE; stamps [n], fix_point [n][3] (what
    GetFixPoint returns; the entries of A and B are not read), relative_B [7].  Returns SolverSummary."""
    if not (isinstance(poses, np.ndarray) and poses.dtype == np.float64 and poses.flags.c_contiguous):
        raise TypeError("poses must be a C-contiguous float64 array (it is updated in place)")
    n = poses.size // 7
    t, f, rb = _d(stamps).ravel(), _d(fix_point).reshape(-1, 3), _d(relative_B).ravel()
    if not (t.size == n and f.shape[0] == n and rb.size == 7):
        raise ValueError("navsat_optimize_ab: stamps / fix_point must have one entry per pose, relative_B seven numbers")
    opt = opt or default_solver_options()
    summ = _lib.SolverSummary()
    _chk(ctx.L.lvf_navsat_optimize_ab(ctx.h, n, _dp(poses), _dp(t), _dp(f), _dp(rb), C.c_double(huber_a), C.byref(opt), C.byref(summ)))
    return summ


def navsat_optimize_section(ctx, poses_ab, stamps_ab, fix_ab, relative_B, poses_bc, has_fix, fix_point, cov, bc_opt):
    """Navsat::Optimize (navsat.cpp:135-156) entirely on the device: OptimizeBC(B .. C, mode 0), OptimizeAB, then the per-keyframe chain.
    poses_ab [na][7] = A, the keyframes of AB, B — its last row is overwritten with B as OptimizeBC leaves it (B is poses_bc[0]); na < 3 or
    None: A == B, no OptimizeAB.  The other arguments are those of navsat_optimize_ab and navsat_quick_fix; both pose arrays are updated in
    place.  Returns (NavsatBcResult, summary of AB or None, x, iterations, chain summary)."""
    ab = []

    def between(poses):
        if poses_ab is not None and poses_ab.size // 7 >= 3:
            poses_ab.reshape(-1, 7)[-1] = poses.reshape(-1, 7)[0]
            ab.append(navsat_optimize_ab(ctx, poses_ab, stamps_ab, fix_ab, relative_B, bc_opt.huber_a, bc_opt.solver))

    res, x, it, summ = navsat_quick_fix(ctx, poses_bc, has_fix, fix_point, cov, bc_opt, between=between)
    return res, (ab[0] if ab else None), x, it, summ


def _gray(gray, who):
    """a 2-D uint8 array whose rows are contiguous (a padded row stride is kept)"""
    g = np.asarray(gray)
    if g.dtype != np.uint8 or g.ndim != 2:
        raise ValueError(f"{who}: a 2-D uint8 array is expected")
    if g.strides[1] != 1 or g.strides[0] < g.shape[1]:
        g = np.ascontiguousarray(g)
    return g


class Image:
    """Device image of the feature tracker: the uint8 pyramid (max_level + 1 levels) with the Scharr pair of every level.  `gray` is a 2-D
    uint8 array; a view with padded rows (a row stride larger than the width) is uploaded as it is."""

    def __init__(self, ctx, gray, max_level=3):
        g = _gray(gray, "Image")
        self.ctx, self._keep = ctx, g
        self.h = C.c_void_p()
        _chk(ctx.L.lvf_image_create(ctx.h, C.cast(C.c_void_p(g.ctypes.data), _lib.c_u8_p), g.shape[1], g.shape[0], g.strides[0], int(max_level), C.byref(self.h)))
        self._keep = None
        self.width, self.height, self.levels = g.shape[1], g.shape[0], int(max_level) + 1

    @classmethod
    def _adopt(cls, ctx, h, width, height, max_level):
        """an lvf_image the library has already built (Undistort.image / pair)"""
        im = cls.__new__(cls)
        im.ctx, im._keep, im.h = ctx, None, h
        im.width, im.height, im.levels = width, height, int(max_level) + 1
        return im

    def size(self):
        w, h, l = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(self.ctx.L.lvf_image_size(self.h, C.byref(w), C.byref(h), C.byref(l)))
        return w.value, h.value, l.value

    def level(self, level):
        """(gray [h, w] uint8, deriv [h, w, 2] int16) of one pyramid level (debug / tests)"""
        w, h = C.c_int32(), C.c_int32()
        _chk(self.ctx.L.lvf_image_download_level(self.h, int(level), C.byref(w), C.byref(h), None, None))
        g, d = np.empty((h.value, w.value), np.uint8), np.empty((h.value, w.value, 2), np.int16)
        _chk(self.ctx.L.lvf_image_download_level(self.h, int(level), None, None, g.ctypes.data_as(_lib.c_u8_p), d.ctypes.data_as(C.POINTER(C.c_int16))))
        return g, d

    def close(self):
        if self.h:
            self.ctx.L.lvf_image_destroy(self.h)
            self.h = C.c_void_p()


class Undistort:
    """cv::undistort of Estimator::InputImage on the device: the fixed-point map of one camera (cam: fx, fy, cx, cy; dist =
    (k1, k2, p1, p2), None for zero distortion) and image size, built once.  image() / pair() return ordinary api.Image objects."""

    def __init__(self, ctx, cam, dist, width, height):
        self.ctx, self.width, self.height = ctx, int(width), int(height)
        k = Camera()
        k.fx, k.fy, k.cx, k.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        k.extrinsic[3] = 1.0
        d = Distortion(*[float(c) for c in dist]) if dist is not None else None
        self.h = C.c_void_p()
        _chk(ctx.L.lvf_undistort_create(ctx.h, C.byref(k), C.byref(d) if d is not None else None, self.width, self.height, C.byref(self.h)))

    def map(self):
        """(xy [h, w, 2] int16 = top-left source tap, frac [h, w] uint16 = b * 32 + a) (debug / tests)"""
        xy, frac = np.empty((self.height, self.width, 2), np.int16), np.empty((self.height, self.width), np.uint16)
        _chk(self.ctx.L.lvf_undistort_download_map(self.h, xy.ctypes.data_as(C.POINTER(C.c_int16)), frac.ctypes.data_as(C.POINTER(C.c_uint16))))
        return xy, frac

    def image(self, raw, max_level=3):
        """api.Image of the undistorted `raw` (2-D uint8; a padded row stride is uploaded as it is)"""
        g = _gray(raw, "Undistort.image")
        h = C.c_void_p()
        _chk(self.ctx.L.lvf_image_create_undistorted(self.h, C.cast(C.c_void_p(g.ctypes.data), _lib.c_u8_p), g.shape[1], g.shape[0], g.strides[0], int(max_level),
                                                     C.byref(h)))
        return Image._adopt(self.ctx, h, g.shape[1], g.shape[0], max_level)

    def pair(self, other, raw0, raw1, max_level=3):
        """Estimator::InputImage: (api.Image, api.Image) of raw0 through this map and raw1 through `other`'s, one wait for both"""
        g0, g1 = _gray(raw0, "Undistort.pair"), _gray(raw1, "Undistort.pair")
        if g0.shape != g1.shape:
            raise ValueError("Undistort.pair: the two images differ in size")
        h0, h1 = C.c_void_p(), C.c_void_p()
        _chk(self.ctx.L.lvf_image_pair_create_undistorted(self.h, other.h, C.cast(C.c_void_p(g0.ctypes.data), _lib.c_u8_p), C.cast(C.c_void_p(g1.ctypes.data), _lib.c_u8_p),
                                                          g0.shape[1], g0.shape[0], g0.strides[0], g1.strides[0], int(max_level), C.byref(h0), C.byref(h1)))
        return Image._adopt(self.ctx, h0, g0.shape[1], g0.shape[0], max_level), Image._adopt(other.ctx, h1, g0.shape[1], g0.shape[0], max_level)

    def close(self):
        if self.h:
            self.ctx.L.lvf_undistort_destroy(self.h)
            self.h = C.c_void_p()


def flow_options(**kw):
    """lvf_flow_options with the reference's values (utility.cpp:64-79), fields overridden by keyword."""
    o = FlowOptions()
    _lib.lib().lvf_flow_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise ValueError(f"flow_options: no field {k}")
        setattr(o, k, v)
    return o


def _fp(a):
    return a.ctypes.data_as(_lib.c_float_p)


def _u8p(a):
    return a.ctypes.data_as(_lib.c_u8_p)


def _pts(a):
    return np.array(a, dtype=np.float32, order="C").reshape(-1, 2)


def optical_flow(prev_img, next_img, prev_pts, next_init, opt=None):
    """optical_flow (utility.cpp:55-89): returns next [n, 2] float32, status [n] uint8, fb [n] float32 (forward-backward distance)."""
    p, q = _pts(prev_pts), _pts(next_init)
    if p.shape != q.shape:
        raise ValueError("optical_flow: prev_pts and next_init differ in shape")
    n = len(p)
    st, fb = np.zeros(n, np.uint8), np.zeros(n, np.float32)
    _chk(prev_img.ctx.L.lvf_optical_flow(prev_img.h, next_img.h, n, _fp(p), _fp(q), _u8p(st), _fp(fb), C.byref(opt) if opt is not None else None))
    return q, st, fb


def stereo_triangulate(left, right, cam0, cam1, baseline, kps_left, opt=None):
    """LocalMap::Triangulate (local_map.cpp:233-269): returns kps_right [n, 2] float32, status [n] (0 lost, 1 accepted, 2 behind camera 0),
    inv_depth [n], p_robot [n, 3]."""
    p = _pts(kps_left)
    n = len(p)
    q, st, inv, pb = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n), np.zeros((n, 3))
    c0, c1 = make_camera(cam0), make_camera(cam1)
    _chk(left.ctx.L.lvf_stereo_triangulate(left.h, right.h, C.byref(c0), C.byref(c1), C.c_double(baseline), n, _fp(p), _fp(q), _u8p(st), _dp(inv), _dp(pb),
                                           C.byref(opt) if opt is not None else None))
    return q, st, inv, pb


def track_last_frame(last, current, cam0, baseline, current_pose, pw, kps_last, remove_moving_points=True, num_features_tracking_bad=20, opt=None):
    """Frontend::TrackLastFrame's numeric part (frontend.cpp:163-256): returns kps_current [n, 2] float32, cls [n] (0 lost, 1 far, 2 near,
    3 moving), the number of good points, and the predictions [n, 2] float32."""
    p, w, pose = _pts(kps_last), _d(pw).reshape(-1, 3), _d(current_pose)
    n = len(p)
    if len(w) != n:
        raise ValueError("track_last_frame: pw and kps_last differ in length")
    q, pred, cls, good = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), C.c_int32(0)
    c0 = make_camera(cam0)
    _chk(last.ctx.L.lvf_track_last_frame(last.h, current.h, C.byref(c0), C.c_double(baseline), _dp(pose), n, _dp(w), _fp(p), int(bool(remove_moving_points)),
                                         int(num_features_tracking_bad), _fp(q), _fp(pred), _u8p(cls), C.byref(good), C.byref(opt) if opt is not None else None))
    return q, cls, good.value, pred


def orb_options(**kw):
    """lvf_orb_options with the reference's values (extractor.h:26), fields overridden by keyword."""
    o = OrbOptions()
    _lib.lib().lvf_orb_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise ValueError(f"orb_options: no field {k}")
        setattr(o, k, v)
    return o


ERR_ORB_CAPACITY, ERR_ORB_OVERFLOW = 5, 6


class Orb:
    """Extractor on the device: the scale pyramid of the last image, FAST / quadtree detection, ICAngle and rBRIEF.  `pattern`:
    int8 [256, 4] = (x1, y1, x2, y2) per descriptor bit, None for the built-in table."""

    def __init__(self, ctx, opt=None, pattern=None):
        self.ctx, self.opt = ctx, opt if opt is not None else orb_options()
        self.h = C.c_void_p()
        pat = None
        if pattern is not None:
            pat = np.ascontiguousarray(pattern, dtype=np.int8)
            if pat.shape != (256, 4):
                raise ValueError("Orb: the pattern is int8 [256, 4]")
        _chk(ctx.L.lvf_orb_create(ctx.h, C.byref(self.opt), pat.ctypes.data_as(C.POINTER(C.c_int8)) if pat is not None else None, C.byref(self.h)))

    def pattern(self):
        p = np.zeros((256, 4), np.int8)
        _chk(self.ctx.L.lvf_orb_pattern(self.h, p.ctypes.data_as(C.POINTER(C.c_int8))))
        return p

    def level_info(self, level):
        """(scale_factor_per_levels_[level] as float32, num_desired_features_[level])"""
        s, n = C.c_float(), C.c_int32()
        _chk(self.ctx.L.lvf_orb_level_info(self.h, int(level), C.byref(s), C.byref(n)))
        return np.float32(s.value), n.value

    def capacity(self, width, height):
        n = C.c_int32()
        _chk(self.ctx.L.lvf_orb_capacity(self.h, int(width), int(height), C.byref(n)))
        return n.value

    def set_image(self, img):
        """pyramid and FAST score maps of level 0 of an api.Image, without detection (for compute / orientation of tracked points)"""
        _chk(self.ctx.L.lvf_orb_set_image(self.h, img.h))

    def detect(self, img, capacity=None):
        """Extractor::Detect: dict(level_count, pt [n, 2] float32, octave, angle, response, size), level-major, each level sorted by (y, x)"""
        cap = self.capacity(img.width, img.height) if capacity is None else int(capacity)
        n, lc = C.c_int32(), np.zeros(self.opt.num_levels, np.int32)
        pt, octave = np.zeros((cap, 2), np.float32), np.zeros(cap, np.int32)
        angle, resp, size = np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        _chk(self.ctx.L.lvf_orb_detect(self.h, img.h, cap, C.byref(n), _ip(lc), _fp(pt), _ip(octave), _fp(angle), _fp(resp), _fp(size)))
        k = n.value
        return dict(level_count=lc, pt=pt[:k].copy(), octave=octave[:k].copy(), angle=angle[:k].copy(), response=resp[:k].copy(), size=size[:k].copy())

    def orientation(self, pt, octave):
        p, o = _pts(pt), _i(octave)
        a = np.zeros(len(p), np.float32)
        _chk(self.ctx.L.lvf_orb_orientation(self.h, len(p), _fp(p), _ip(o), _fp(a)))
        return a

    def compute(self, pt, octave, angle):
        """Extractor::Compute: descriptors [n, 32] uint8 of keypoints of the image of the last detect / set_image"""
        p, o, a = _pts(pt), _i(octave), _f(angle)
        d = np.zeros((len(p), 32), np.uint8)
        _chk(self.ctx.L.lvf_orb_compute(self.h, len(p), _fp(p), _ip(o), _fp(a), _u8p(d)))
        return d

    def level(self, level):
        """(gray, blurred, score) [h, w] uint8 of one pyramid level (debug / tests)"""
        w, h = C.c_int32(), C.c_int32()
        _chk(self.ctx.L.lvf_orb_download_level(self.h, int(level), C.byref(w), C.byref(h), None, None, None))
        g, b, s = (np.empty((h.value, w.value), np.uint8) for _ in range(3))
        _chk(self.ctx.L.lvf_orb_download_level(self.h, int(level), None, None, _u8p(g), _u8p(b), _u8p(s)))
        return g, b, s

    def close(self):
        if self.h:
            self.ctx.L.lvf_orb_destroy(self.h)
            self.h = C.c_void_p()


def orb_search(ctx, cam0, last_pose, last_pt, last_octave, last_angle, last_desc, cur_pw, cur_octave, cur_angle, cur_desc, skip=None, opt=None):
    """The numeric part of LocalMap::Search (local_map.cpp:313-368): returns match [n_cur] (index into the last features, -1 where none),
    best, second [n_cur] (the two Hamming distances, -1 where there is no such candidate)."""
    lp, lo, la = _pts(last_pt), _i(last_octave), _f(last_angle)
    ld = np.ascontiguousarray(last_desc, dtype=np.uint8).reshape(-1, 32)
    pw, co, ca = _d(cur_pw).reshape(-1, 3), _i(cur_octave), _f(cur_angle)
    cd = np.ascontiguousarray(cur_desc, dtype=np.uint8).reshape(-1, 32)
    if not (len(lp) == len(lo) == len(la) == len(ld)) or not (len(pw) == len(co) == len(ca) == len(cd)):
        raise ValueError("orb_search: feature arrays differ in length")
    n = len(pw)
    sk = np.ascontiguousarray(skip, dtype=np.uint8) if skip is not None else None
    if sk is not None and len(sk) != n:
        raise ValueError("orb_search: skip and the current features differ in length")
    m, b, s2 = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    c0 = make_camera(cam0)
    _chk(ctx.L.lvf_orb_search(ctx.h, C.byref(opt) if opt is not None else None, C.byref(c0), _dp(_d(last_pose)), len(lp), _fp(lp), _ip(lo), _fp(la), _u8p(ld), n,
                              _dp(pw), _ip(co), _fp(ca), _u8p(cd), _u8p(sk) if sk is not None else None, _ip(m), _ip(b), _ip(s2)))
    return m, b, s2


def _options(cls, default, who, kw):
    o = cls()
    getattr(_lib.lib(), default)(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise ValueError(f"{who}: no field {k}")
        setattr(o, k, v)
    return o


def match_options(**kw):
    """lvf_match_options with its defaults (max_distance 50, ratio 0.8f, cross_check 1), fields overridden by keyword."""
    return _options(_lib.MatchOptions, "lvf_match_options_default", "match_options", kw)


def pnp_options(**kw):
    """lvf_pnp_options with its defaults (512 hypotheses, seed 0, 3 px, min_matches 21, 2 rounds of 10 iterations, Huber 1), overridden by keyword."""
    return _options(_lib.PnpOptions, "lvf_pnp_options_default", "pnp_options", kw)


def _desc(a):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)


def orb_match(ctx, query_desc, train_desc, opt=None):
    """Brute-force Hamming 2-NN with the ratio gate and the cross-check: returns match [nq] (train index, -1 where none), best, second [nq]."""
    q, t = _desc(query_desc), _desc(train_desc)
    n = len(q)
    m, b, s2 = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    _chk(ctx.L.lvf_orb_match(ctx.h, n, _u8p(q), len(t), _u8p(t), C.byref(opt) if opt is not None else None, _ip(m), _ip(b), _ip(s2)))
    return m, b, s2


def pnp_ransac(ctx, cam0, pw, pt, init_pose=None, opt=None):
    """P3P RANSAC + refinement on given 3D-2D correspondences: returns dict(pose (None when left untouched), score, inlier [n] uint8, summary)."""
    w, p = _d(pw).reshape(-1, 3), _pts(pt)
    if len(w) != len(p):
        raise ValueError("pnp_ransac: pw and pt differ in length")
    n = len(w)
    ini = _d(init_pose) if init_pose is not None else None
    pose, score, inl, summ = np.full(7, np.nan), C.c_int32(0), np.zeros(n, np.uint8), SolverSummary()
    c0 = make_camera(cam0)
    _chk(ctx.L.lvf_pnp_ransac(ctx.h, C.byref(c0), n, _dp(w), _fp(p), _dp(ini) if ini is not None else None, C.byref(opt) if opt is not None else None, _dp(pose),
                              C.byref(score), _u8p(inl), C.byref(summ)))
    return dict(pose=None if np.isnan(pose).any() else pose, score=score.value, inlier=inl, summary=summ)


def relocate_by_image(ctx, cam0, old_pose, old_pw, old_desc, cur_pt, cur_desc, relative_o_c, match_opt=None, pnp_opt=None):
    """The body of Relocator::RelocateByImage: returns dict(relative_o_c (the caller's value when the candidate is rejected), score, match [n_cur],
    inlier [n_cur] uint8, summary)."""
    w, od, p, cd = _d(old_pw).reshape(-1, 3), _desc(old_desc), _pts(cur_pt), _desc(cur_desc)
    if len(w) != len(od) or len(p) != len(cd):
        raise ValueError("relocate_by_image: feature arrays differ in length")
    n = len(p)
    rel, score, m, inl, summ = _d(relative_o_c).copy(), C.c_int32(0), np.full(n, -1, np.int32), np.zeros(n, np.uint8), SolverSummary()
    c0 = make_camera(cam0)
    _chk(ctx.L.lvf_relocate_by_image(ctx.h, C.byref(c0), _dp(_d(old_pose)), len(w), _dp(w), _u8p(od), n, _fp(p), _u8p(cd), C.byref(match_opt) if match_opt is not None else None,
                                     C.byref(pnp_opt) if pnp_opt is not None else None, _dp(rel), C.byref(score), _ip(m), _u8p(inl), C.byref(summ)))
    return dict(relative_o_c=rel, score=score.value, match=m, inlier=inl, summary=summ)


def pnp_debug_hypotheses(ctx, cam0, pw, pt, opt=None):
    """Test tap: triples [H, 3], n_poses [H], count [H], poses [H, 7] of the hypotheses lvf_pnp_ransac would score."""
    w, p = _d(pw).reshape(-1, 3), _pts(pt)
    o = opt if opt is not None else pnp_options()
    H = o.num_hypotheses
    tri, npo, cnt, poses = np.zeros((H, 3), np.int32), np.zeros(H, np.int32), np.zeros(H, np.int32), np.zeros((H, 7))
    c0 = make_camera(cam0)
    _chk(ctx.L.lvf_pnp_debug_hypotheses(ctx.h, C.byref(c0), len(w), _dp(w), _fp(p), C.byref(o), _ip(tri), _ip(npo), _ip(cnt), _dp(poses)))
    return tri, npo, cnt, poses


def prior3_evaluate(ctx, mode, target3, weight, x3):
    """PoseErrorRPZ / PoseErrorYXY stand-alone (lvf_prior3_evaluate): returns r[3], J[3 blocks][3 rows]."""
    t, x = _d(target3), _d(x3)
    r, J = np.empty(3), np.empty(9)
    _chk(ctx.L.lvf_prior3_evaluate(ctx.h, int(mode), _dp(t), C.c_double(weight), _dp(x), _dp(r), _dp(J)))
    return r, J.reshape(3, 3)


def preintegrate(ctx, samples_list, acc0, gyr0, ba, bg, noise4):
    n = len(samples_list)
    offset = np.zeros(n + 1, np.int32)
    offset[1:] = np.cumsum([s.shape[0] for s in samples_list])
    samples = _d(np.concatenate(samples_list)) if n else np.zeros((0, 7))
    acc0, gyr0, ba, bg, noise4 = map(_d, (acc0, gyr0, ba, bg, noise4))
    out = np.zeros((n, 467))
    _chk(ctx.L.lvf_preintegrate(ctx.h, n, _ip(offset), _dp(samples), _dp(acc0), _dp(gyr0), _dp(ba), _dp(bg), _dp(noise4), _dp(out)))
    return out


def preintegrate_or_none(ctx, cfg):
    """Device pre-integration of a synthetic window's IMU samples (None when the window has no IMU factors)."""
    from . import synthetic as syn
    imu = cfg["imu"]
    if not imu:
        return None
    return preintegrate(ctx, [f["samples"] for f in imu], np.stack([f["acc0"] for f in imu]), np.stack([f["gyr0"] for f in imu]),
                        np.stack([f["ba"] for f in imu]), np.stack([f["bg"] for f in imu]), syn.IMU_NOISE)


class Cloud:
    """Device-resident (x, y, z, intensity) float32 cloud; every method returns a new device cloud."""

    def __init__(self, ctx, xyzi=None, _h=None):
        self.ctx = ctx
        if _h is not None:
            self.h = _h
        else:
            a = _f(xyzi)
            assert a.ndim == 2 and a.shape[1] >= 3
            self.h = C.c_void_p()
            _chk(ctx.L.lvf_cloud_create(ctx.h, a.ctypes.data_as(_lib.c_float_p), a.shape[0], a.shape[1], 3 if a.shape[1] > 3 else -1, C.byref(self.h)))

    def __len__(self):
        return self.ctx.L.lvf_cloud_size(self.h)

    def download(self):
        out = np.empty((len(self), 4), np.float32)
        _chk(self.ctx.L.lvf_cloud_download(self.h, out.ctypes.data_as(_lib.c_float_p)))
        return out

    def _new(self, fn, *args):
        h = C.c_void_p()
        _chk(fn(self.h, *args, C.byref(h)))
        return Cloud(self.ctx, _h=h)

    def transform(self, pose):
        p = _d(pose)
        return self._new(self.ctx.L.lvf_cloud_transform, _dp(p))

    def voxel_filter(self, leaf):
        return self._new(self.ctx.L.lvf_cloud_voxel_filter, float(leaf))

    def radius_outlier_filter(self, radius, min_neighbors):
        return self._new(self.ctx.L.lvf_cloud_radius_outlier_filter, float(radius), int(min_neighbors))

    def segment_plane(self, thr, max_iterations=100, seed=12345):
        h = C.c_void_p(); co = np.empty(4); it = C.c_int()
        _chk(self.ctx.L.lvf_cloud_segment_plane(self.h, float(thr), int(max_iterations), int(seed), C.byref(h), _dp(co), C.byref(it)))
        return Cloud(self.ctx, _h=h), co, it.value

    def deskew(self, traj, frame_time, frame_pose, cycle_time, extrinsic):
        """FeatureAssociation::UndistortPointCloud on a sensor-frame cloud whose intensity carries ring + time offset"""
        fp, e = _d(frame_pose), _d(extrinsic)
        h = C.c_void_p()
        _chk(self.ctx.L.lvf_cloud_deskew(self.h, traj.h if traj is not None else None, float(frame_time), _dp(fp), float(cycle_time), _dp(e), C.byref(h)))
        return Cloud(self.ctx, _h=h)

    @staticmethod
    def concat(ctx, parts):
        arr = (C.c_void_p * len(parts))(*[p.h for p in parts])
        h = C.c_void_p()
        _chk(ctx.L.lvf_cloud_concat(ctx.h, arr, len(parts), C.byref(h)))
        return Cloud(ctx, _h=h)

    @staticmethod
    def align_scan(pc1, stamp1, pc2, stamp2, cycle_time, time):
        """FeatureAssociation::AlignScan on device: (Cloud, True) or (empty Cloud, False) where the reference returns false."""
        h = C.c_void_p(); ok = C.c_int()
        _chk(pc1.ctx.L.lvf_cloud_align_scan(pc1.h, float(stamp1), pc2.h, float(stamp2), float(cycle_time), float(time), C.byref(h), C.byref(ok)))
        return Cloud(pc1.ctx, _h=h), bool(ok.value)

    def scan_context(self, opt=None):
        """Scan Context descriptor of this sensor-frame cloud: desc [num_sectors, num_rings] uint8 (row j = column j of the polar image),
        norm [num_sectors] uint32."""
        o = opt if opt is not None else scanctx_options()
        desc, norm = np.zeros((o.num_sectors, o.num_rings), np.uint8), np.zeros(o.num_sectors, np.uint32)
        _chk(self.ctx.L.lvf_scanctx_describe(self.ctx.h, self.h, C.byref(o), _u8p(desc), norm.ctypes.data_as(C.POINTER(C.c_uint32))))
        return desc, norm

    def close(self):
        if self.h:
            self.ctx.L.lvf_cloud_destroy(self.h)
            self.h = C.c_void_p()


def scanctx_options(**kw):
    """lvf_scanctx_options with its defaults (20 rings x 60 sectors, 0.5 .. 80 m, sensor 2 m above ground, 10 height steps per metre), overridden by keyword."""
    return _options(_lib.ScanCtxOptions, "lvf_scanctx_options_default", "scanctx_options", kw)


class ScanContextDb:
    """The place-recognition database: Scan Context entries of old keyframes on the device, their stamps on the host."""

    def __init__(self, ctx, capacity, opt=None):
        self.ctx = ctx
        self.opt = opt if opt is not None else scanctx_options()
        self.h = C.c_void_p()
        _chk(ctx.L.lvf_scanctx_db_create(ctx.h, C.byref(self.opt), int(capacity), C.byref(self.h)))

    def __len__(self):
        return self.ctx.L.lvf_scanctx_db_size(self.h)

    def _desc(self, desc):
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        if d.shape != (self.opt.num_sectors, self.opt.num_rings):
            raise ValueError("ScanContextDb: descriptor of shape %r, expected (%d, %d)" % (d.shape, self.opt.num_sectors, self.opt.num_rings))
        return d

    def append(self, cloud, stamp):
        _chk(self.ctx.L.lvf_scanctx_db_append(self.h, cloud.h, float(stamp)))

    def append_descriptor(self, desc, stamp):
        d = self._desc(desc)
        _chk(self.ctx.L.lvf_scanctx_db_append_descriptor(self.h, _u8p(d), float(stamp)))

    def download(self, index):
        desc, norm = np.zeros((self.opt.num_sectors, self.opt.num_rings), np.uint8), np.zeros(self.opt.num_sectors, np.uint32)
        _chk(self.ctx.L.lvf_scanctx_db_download(self.h, int(index), _u8p(desc), norm.ctypes.data_as(C.POINTER(C.c_uint32))))
        return desc, norm

    def search(self, desc, max_stamp=np.inf, k=1):
        """the k best entries with stamps <= max_stamp: index [k], shift [k] (both -1 in unused slots), distance [k] (+inf there)"""
        d = self._desc(desc)
        idx, sh, dist = np.zeros(max(int(k), 0), np.int32), np.zeros(max(int(k), 0), np.int32), np.zeros(max(int(k), 0))
        _chk(self.ctx.L.lvf_scanctx_search(self.h, _u8p(d), float(max_stamp), int(k), _ip(idx), _ip(sh), _dp(dist)))
        return idx, sh, dist

    def detect(self, cloud, stamp, max_stamp=np.inf, k=1, append=True):
        """describe + search + (append) append in one launch chain; the search sees the database as it was before the call"""
        idx, sh, dist = np.zeros(max(int(k), 0), np.int32), np.zeros(max(int(k), 0), np.int32), np.zeros(max(int(k), 0))
        _chk(self.ctx.L.lvf_scanctx_detect(self.h, cloud.h, float(stamp), float(max_stamp), int(k), _ip(idx), _ip(sh), _dp(dist), 1 if append else 0))
        return idx, sh, dist

    def close(self):
        if self.h:
            self.ctx.L.lvf_scanctx_db_destroy(self.h)
            self.h = C.c_void_p()


def lidar_depth_options(**kw):
    """lvf_lidar_depth_options with its defaults (cell 8 px, radius 12 px, 0.5 .. 80 m, spread 2 m, min_det 4 px^2, extrapolation 0.5, far_factor 50,
    replace_lost 1), overridden by keyword."""
    return _options(_lib.LidarDepthOptions, "lvf_lidar_depth_options_default", "lidar_depth_options", kw)


def cam_from_lidar(cam0, lidar_extrinsic):
    """The 3x4 matrix [R | t] that takes LiDAR sensor coordinates into camera 0: SE3(cam0 extrinsic).inverse() * SE3(lidar_extrinsic), both
    sensor -> robot as [qx, qy, qz, qw, tx, ty, tz].  The device takes the matrix as data, so nothing depends on how it was rounded."""
    from .synthetic import rotmat
    e0, el = _d(cam0["extrinsic"]), _d(lidar_extrinsic)
    r0t = rotmat(e0[:4]).T
    return np.ascontiguousarray(np.hstack([r0t @ rotmat(el[:4]), (r0t @ (el[4:] - e0[4:]))[:, None]]))


LIDAR_DEPTH_RECORD = np.dtype([("u", np.float32), ("v", np.float32), ("z", np.float32), ("source_index", np.int32)])


class LidarDepth:
    """A sweep projected into camera 0 and binned on a pixel grid.  `cloud` is a sensor-frame Cloud deskewed to the image's pose,
    `matrix` = cam_from_lidar(cam0, lidar_extrinsic)."""

    def __init__(self, ctx, cloud, cam0, matrix, width, height, opt=None):
        self.ctx, self.cam0, self.width, self.height = ctx, cam0, int(width), int(height)
        self.opt = opt if opt is not None else lidar_depth_options()
        m = _d(matrix).reshape(12)
        c0 = make_camera(cam0)
        self.h = C.c_void_p()
        _chk(ctx.L.lvf_lidar_depth_create(ctx.h, cloud.h, C.byref(c0), _dp(m), self.width, self.height, C.byref(self.opt), C.byref(self.h)))

    def __len__(self):
        n = self.ctx.L.lvf_lidar_depth_size(self.h)
        if n < 0:
            raise LvfError("lvf_lidar_depth_size: %s" % _lib.lib().lvf_last_error().decode())
        return n

    @property
    def grid(self):
        """(cell columns, cell rows)"""
        c = self.opt.cell
        return (self.width + c - 1) // c, (self.height + c - 1) // c

    def download(self):
        """records [len(self)] (LIDAR_DEPTH_RECORD, in the device's order: unordered inside a cell) and cell_start [cells + 1]"""
        ncx, ncy = self.grid
        rec, start = np.zeros(len(self), LIDAR_DEPTH_RECORD), np.zeros(ncx * ncy + 1, np.int32)
        _chk(self.ctx.L.lvf_lidar_depth_download(self.h, rec.ctypes.data_as(C.c_void_p), _ip(start)))
        return rec, start

    def query(self, cam1, kps_left):
        """depth of every feature: status [n] (1 accepted; 0 / 3 / 4 / 2 / 5 the gates of include/lvf.h), depth [n], inv_depth [n], p_robot [n, 3],
        kps_right [n, 2] float32 — zero where status != 1"""
        p = _pts(kps_left)
        n = len(p)
        st, dz, inv, pb, q = np.zeros(n, np.uint8), np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros((n, 2), np.float32)
        c0, c1 = make_camera(self.cam0), make_camera(cam1)
        _chk(self.ctx.L.lvf_lidar_depth_query(self.h, C.byref(c0), C.byref(c1), n, _fp(p), _u8p(st), _dp(dz), _dp(inv), _dp(pb), _fp(q)))
        return st, dz, inv, pb, q

    def close(self):
        if self.h:
            self.ctx.L.lvf_lidar_depth_destroy(self.h)
            self.h = C.c_void_p()


def stereo_triangulate_lidar(left, right, cam0, cam1, baseline, kps_left, depth, opt=None):
    """stereo_triangulate with the sweep's depth merged in behind it (one launch chain, one wait): returns kps_right, status, inv_depth, p_robot as
    stereo_triangulate does, and source [n]: 0 no depth, 1 stereo, 2 LiDAR."""
    p = _pts(kps_left)
    n = len(p)
    q, st, inv, pb, src = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n), np.zeros((n, 3)), np.zeros(n, np.uint8)
    c0, c1 = make_camera(cam0), make_camera(cam1)
    _chk(left.ctx.L.lvf_stereo_triangulate_lidar(left.h, right.h, C.byref(c0), C.byref(c1), C.c_double(baseline), n, _fp(p), _fp(q), _u8p(st), _dp(inv), _dp(pb),
                                                 C.byref(opt) if opt is not None else None, depth.h, _u8p(src)))
    return q, st, inv, pb, src


class Trajectory:
    """Map::keyframes as Map::ComputePose reads it, on the device: stamps [n] strictly increasing, poses [n, 7] = [qx,qy,qz,qw,tx,ty,tz]."""

    def __init__(self, ctx, stamps, poses):
        self.ctx = ctx
        t, p = _d(stamps).reshape(-1), _d(poses).reshape(-1, 7)
        if len(t) != len(p):
            raise ValueError("Trajectory: %d stamps for %d poses" % (len(t), len(p)))
        self.h = C.c_void_p()
        _chk(ctx.L.lvf_trajectory_create(ctx.h, _dp(t), _dp(p), len(t), C.byref(self.h)))

    def __len__(self):
        return self.ctx.L.lvf_trajectory_size(self.h)

    def append(self, stamp, pose):
        p = _d(pose)
        _chk(self.ctx.L.lvf_trajectory_append(self.h, float(stamp), _dp(p)))

    def set_pose(self, i, pose):
        p = _d(pose)
        _chk(self.ctx.L.lvf_trajectory_set_pose(self.h, int(i), _dp(p)))

    def compute_pose(self, times):
        """Map::ComputePose for every time: [m, 7]"""
        t = _d(times).reshape(-1)
        out = np.empty((len(t), 7))
        _chk(self.ctx.L.lvf_trajectory_compute_pose(self.h, _dp(t), len(t), _dp(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.L.lvf_trajectory_destroy(self.h)
            self.h = C.c_void_p()


def lidar_params(**kw):
    p = LidarParams()
    _lib.lib().lvf_lidar_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def extract_host_counts(ctx, on):
    """test / A-B hook: route lidar_extract through the host-counted path (process-wide); returns the previous setting"""
    return bool(ctx.L.lvf_debug_extract_host_counts(1 if on else 0))


def extract_fallbacks(ctx):
    """test hook: scans that entered the device-counted path and were handed to the host-counted one, since the library was loaded"""
    return int(ctx.L.lvf_debug_extract_fallbacks())


def _lidar_extract(ctx, points, extrinsic, params, debug, call):
    a = _f(points); e = _d(extrinsic)
    prm = params if params is not None else lidar_params()
    hg, hs = C.c_void_p(), C.c_void_p()
    dbg = None
    if debug:
        npix = prm.num_scans * prm.horizon_scan
        cap = max(npix, 1)
        keep = dict(label_mat=np.zeros(npix, np.int32), ground_mat=np.zeros(npix, np.int8), range_mat=np.zeros(npix, np.float32),
                    ground_raw=np.zeros((cap, 4), np.float32), surf_raw=np.zeros((cap, 4), np.float32))
        dbg = LidarExtractDebug()
        dbg.label_mat = keep["label_mat"].ctypes.data_as(C.POINTER(C.c_int32)); dbg.ground_mat = keep["ground_mat"].ctypes.data_as(C.POINTER(C.c_int8))
        dbg.range_mat = keep["range_mat"].ctypes.data_as(_lib.c_float_p); dbg.ground_raw = keep["ground_raw"].ctypes.data_as(_lib.c_float_p)
        dbg.surf_raw = keep["surf_raw"].ctypes.data_as(_lib.c_float_p)
    _chk(call(a, prm, e, hg, hs, C.byref(dbg) if dbg is not None else None))
    g, s = Cloud(ctx, _h=hg), Cloud(ctx, _h=hs)
    if not debug:
        return g, s
    R, Cn = prm.num_scans, prm.horizon_scan
    out = dict(label_mat=keep["label_mat"].reshape(R, Cn), ground_mat=keep["ground_mat"].reshape(R, Cn), range_mat=keep["range_mat"].reshape(R, Cn),
               ground_raw=keep["ground_raw"][:dbg.n_ground_raw].copy(), surf_raw=keep["surf_raw"][:dbg.n_surf_raw].copy(),
               n_filtered=dbg.n_filtered, n_segmented=dbg.n_segmented)
    return g, s, out


def lidar_extract(ctx, points, extrinsic, params=None, debug=False):
    """FeatureAssociation::Process on device: raw sensor-frame scan -> (ground Cloud, surf Cloud[, debug dict])."""
    return _lidar_extract(ctx, points, extrinsic, params, debug, lambda a, prm, e, hg, hs, dbg: ctx.L.lvf_lidar_extract(
        ctx.h, a.ctypes.data_as(_lib.c_float_p), a.shape[0], a.shape[1], C.byref(prm), _dp(e), C.byref(hg), C.byref(hs), dbg))


def lidar_extract_deskewed(ctx, points, extrinsic, traj, frame_time, frame_pose, params=None, debug=False):
    """lidar_extract with the sweep deskewed along `traj` where AdjustDistortion's TODO stands; the debug dict's ground_raw /
    surf_raw are the deskewed picks."""
    fp = _d(frame_pose)
    return _lidar_extract(ctx, points, extrinsic, params, debug, lambda a, prm, e, hg, hs, dbg: ctx.L.lvf_lidar_extract_deskewed(
        ctx.h, a.ctypes.data_as(_lib.c_float_p), a.shape[0], a.shape[1], C.byref(prm), _dp(e), traj.h if traj is not None else None, float(frame_time), _dp(fp),
        C.byref(hg), C.byref(hs), dbg))


def edge_params(**kw):
    p = EdgeParams()
    _lib.lib().lvf_edge_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def lidar_extract_edges(ctx, points, extrinsic, edge=None, traj=None, frame_time=0.0, frame_pose=None, params=None, debug=False):
    """lidar_extract (traj None) / lidar_extract_deskewed with the edge picks made inside the same launch chain:
    (ground, surf, sharp, less_sharp Clouds[, debug dict]).  The debug dict is lidar_extract's plus sharp_raw / less_sharp_raw (the picks in the
    sensor frame, before any deskew) and, per segmented point, curvature / sharp_flags / less_sharp_flags."""
    ep = edge if edge is not None else edge_params()
    fp = _d(frame_pose) if frame_pose is not None else None
    prm = params if params is not None else lidar_params()
    hsh, hls = C.c_void_p(), C.c_void_p()
    ed = keep = None
    if debug:
        cap = max(prm.num_scans * prm.horizon_scan, 1)
        keep = dict(sharp_raw=np.zeros((cap, 4), np.float32), less_sharp_raw=np.zeros((cap, 4), np.float32), curvature=np.zeros(cap, np.float32),
                    sharp_flags=np.zeros(cap, np.int32), less_sharp_flags=np.zeros(cap, np.int32))
        ed = EdgeExtractDebug()
        ed.sharp_raw, ed.less_sharp_raw, ed.curvature = (keep[k].ctypes.data_as(_lib.c_float_p) for k in ("sharp_raw", "less_sharp_raw", "curvature"))
        ed.sharp_flags, ed.less_sharp_flags = (keep[k].ctypes.data_as(C.POINTER(C.c_int32)) for k in ("sharp_flags", "less_sharp_flags"))
    out = _lidar_extract(ctx, points, extrinsic, prm, debug, lambda a, prm_, e, hg, hs, dbg: ctx.L.lvf_lidar_extract_edges(
        ctx.h, a.ctypes.data_as(_lib.c_float_p), a.shape[0], a.shape[1], C.byref(prm_), _dp(e), C.byref(ep), traj.h if traj is not None else None, float(frame_time),
        _dp(fp) if fp is not None else None, C.byref(hg), C.byref(hs), C.byref(hsh), C.byref(hls), dbg, C.byref(ed) if ed is not None else None))
    sh, ls = Cloud(ctx, _h=hsh), Cloud(ctx, _h=hls)
    if not debug:
        return out[0], out[1], sh, ls
    d = out[2]
    ns = d["n_segmented"]
    d.update(sharp_raw=keep["sharp_raw"][:ed.n_sharp_raw].copy(), less_sharp_raw=keep["less_sharp_raw"][:ed.n_less_sharp_raw].copy(), curvature=keep["curvature"][:ns].copy(),
             sharp_flags=keep["sharp_flags"][:ns].copy(), less_sharp_flags=keep["less_sharp_flags"][:ns].copy())
    return out[0], out[1], sh, ls, d


class Map:
    def __init__(self, ctx, xyz, max_radius2):
        self.ctx = ctx
        self.h = C.c_void_p()
        if isinstance(xyz, Cloud):
            self.M = len(xyz)
            _chk(ctx.L.lvf_map_create_from_cloud(xyz.h, float(max_radius2), C.byref(self.h)))
            return
        a = _f(xyz)
        self.ctx, self.M = ctx, a.shape[0]
        _chk(ctx.L.lvf_map_create(ctx.h, a.ctypes.data_as(_lib.c_float_p), a.shape[0], a.shape[1] if a.ndim == 2 else 3,
                                  float(max_radius2), C.byref(self.h)))

    def close(self):
        if self.h:
            self.ctx.L.lvf_map_destroy(self.h)
            self.h = C.c_void_p()

    @classmethod
    def create_batch(cls, ctx, clouds, max_radius2):
        """lvf_map_create_batch: one Map per cloud (host arrays of one column count, or device-resident Cloud objects: no upload), the host
        waits shared between them"""
        n = len(clouds)
        if n and all(isinstance(c, Cloud) for c in clouds):
            thr = np.ascontiguousarray(np.broadcast_to(np.asarray(max_radius2, np.float32), (n,)))
            hc = (C.c_void_p * n)(*[c.h for c in clouds])
            hs = (C.c_void_p * n)()
            _chk(ctx.L.lvf_map_create_batch_from_clouds(ctx.h, n, hc, thr.ctypes.data_as(_lib.c_float_p), hs))
            out = []
            for i in range(n):
                m = cls.__new__(cls)
                m.ctx, m.M, m.h = ctx, len(clouds[i]), C.c_void_p(hs[i])
                out.append(m)
            return out
        arrs = [_f(c) for c in clouds]
        thr = np.ascontiguousarray(np.broadcast_to(np.asarray(max_radius2, np.float32), (n,)))
        if n == 0:
            return []
        stride = arrs[0].shape[1] if arrs[0].ndim == 2 else 3
        assert all((a.shape[1] if a.ndim == 2 else 3) == stride for a in arrs), "clouds of one batch share their column count"
        ptrs = (_lib.c_float_p * n)(*[a.ctypes.data_as(_lib.c_float_p) for a in arrs])
        Ms = np.array([a.shape[0] for a in arrs], np.int32)
        hs = (C.c_void_p * n)()
        _chk(ctx.L.lvf_map_create_batch(ctx.h, n, ptrs, Ms.ctypes.data_as(_lib.c_int_p), stride, thr.ctypes.data_as(_lib.c_float_p), hs))
        out = []
        for i in range(n):
            m = cls.__new__(cls)
            m.ctx, m.M, m.h = ctx, int(Ms[i]), C.c_void_p(hs[i])
            out.append(m)
        return out


class Scan:
    def __init__(self, ctx, xyz):
        self.ctx = ctx
        self.h = C.c_void_p()
        if isinstance(xyz, Cloud):
            self.Q = len(xyz)
            _chk(ctx.L.lvf_scan_create_from_cloud(xyz.h, C.byref(self.h)))
            return
        a = _f(xyz)
        self.ctx, self.Q = ctx, a.shape[0]
        _chk(ctx.L.lvf_scan_create(ctx.h, a.ctypes.data_as(_lib.c_float_p), a.shape[0], a.shape[1] if a.ndim == 2 else 3, C.byref(self.h)))

    def download(self):
        idx = np.empty((self.Q, 3), np.int32); d2 = np.empty((self.Q, 3), np.float32); valid = np.empty(self.Q, np.uint8)
        _chk(self.ctx.L.lvf_scan_download(self.h, _ip(idx), d2.ctypes.data_as(_lib.c_float_p), valid.ctypes.data_as(_lib.c_u8_p)))
        return idx, d2, valid

    def download_edges(self):
        """lvf_edge_associate's outputs: idx5 [Q][5], d2_5 [Q][5], valid [Q], scan point p [Q][3], centroid c [Q][3], projector proj6 [Q][6]
        (00 01 02 11 12 22; p, c and proj6 read zero for an invalid point)"""
        idx = np.empty((self.Q, 5), np.int32); d2 = np.empty((self.Q, 5), np.float32); valid = np.empty(self.Q, np.uint8)
        corr = np.empty((12, self.Q), np.float64)
        _chk(self.ctx.L.lvf_scan_download_edges(self.h, _ip(idx), d2.ctypes.data_as(_lib.c_float_p), valid.ctypes.data_as(_lib.c_u8_p), _dp(corr)))
        return idx, d2, valid, np.ascontiguousarray(corr[0:3].T), np.ascontiguousarray(corr[3:6].T), np.ascontiguousarray(corr[6:12].T)

    def close(self):
        if self.h:
            self.ctx.L.lvf_scan_destroy(self.h)
            self.h = C.c_void_p()


def knn3(map_, scan, pose, thr):
    p = _d(pose)
    _chk(map_.ctx.L.lvf_knn3(map_.h, scan.h, _dp(p), float(thr)))


def icp_solve(map_, scan, map_pose, frame_pose, rpyxyz, mode, thr, weight, huber_a, prior_weight=0.0, max_num_iterations=4):
    """rpyxyz is updated IN PLACE (numpy float64[6]); returns the summary struct."""
    assert rpyxyz.dtype == np.float64 and rpyxyz.flags.c_contiguous and rpyxyz.size == 6
    mp, fp = _d(map_pose), _d(frame_pose)
    opt = IcpOptions(int(mode), float(thr), float(weight), float(huber_a), float(prior_weight), int(max_num_iterations))
    summ = IcpSummary()
    _chk(map_.ctx.L.lvf_icp_solve(map_.h, scan.h, _dp(mp), _dp(fp), _dp(rpyxyz), C.byref(opt), C.byref(summ)))
    return summ


def edge_associate(map_, scan, pose, thr, min_eigen_ratio=3.0):
    """5-NN + line fit of every scan point against a map of edge points (lvf_edge_associate); results: scan.download_edges()"""
    p = _d(pose)
    _chk(map_.ctx.L.lvf_edge_associate(map_.h, scan.h, _dp(p), float(thr), float(min_eigen_ratio)))


def lidar_edge_evaluate(ctx, mode, p, c, proj6, Twc1, rpyxyz, weight, jacobians=True):
    """LidarEdgeErrorRPZ (mode 0) / LidarEdgeErrorYXY (mode 1) for n blocks: residuals [n][3], Jacobians [n][3][3] (row k, parameter j) or None"""
    p, c, pr, T, x = _d(p).reshape(-1, 3), _d(c).reshape(-1, 3), _d(proj6).reshape(-1, 6), _d(Twc1), _d(rpyxyz)
    n = p.shape[0]
    r = np.empty((n, 3)); J = np.empty((n, 3, 3)) if jacobians else None
    _chk(ctx.L.lvf_lidar_edge_evaluate(ctx.h, int(mode), n, _dp(p), _dp(c), _dp(pr), _dp(T), _dp(x), float(weight), _dp(r), _dp(J) if jacobians else None))
    return r, J


def edge_icp_options(resolution=0.2, **kw):
    o = EdgeIcpOptions()
    _lib.lib().lvf_edge_icp_options_default(C.byref(o), float(resolution))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def icp_solve_edges(map_surf, scan_surf, map_edge, scan_edge, map_pose, frame_pose, rpyxyz, thr, weight, huber_a, edge_opt=None, prior_weight=0.0,
                    max_num_iterations=4):
    """The (yaw, x, y) solve over planes and lines (lvf_icp_solve_edges); either pair may be None.  rpyxyz is updated IN PLACE."""
    assert rpyxyz.dtype == np.float64 and rpyxyz.flags.c_contiguous and rpyxyz.size == 6
    mp, fp = _d(map_pose), _d(frame_pose)
    opt = IcpOptions(1, float(thr), float(weight), float(huber_a), float(prior_weight), int(max_num_iterations))
    summ = IcpSummary()
    anyh = map_surf if map_surf is not None else map_edge
    h = lambda x: x.h if x is not None else None
    _chk(anyh.ctx.L.lvf_icp_solve_edges(h(map_surf), h(scan_surf), h(map_edge), h(scan_edge), _dp(mp), _dp(fp), _dp(rpyxyz), C.byref(opt),
                                        C.byref(edge_opt) if edge_opt is not None else None, C.byref(summ)))
    return summ


def scan_match_edges(map_ground, scan_ground, map_surf, scan_surf, map_edge, scan_edge, map_pose, frame_pose, opt, edge_opt=None, last_pose=None):
    """lvf_scan_match with planes and lines in the (yaw, x, y) sub-problem; with the edge pair None it is scan_match."""
    mp, fp = _d(map_pose), _d(frame_pose)
    lp = _d(last_pose) if last_pose is not None else None
    res = ScanMatchResult()
    anyh = next(x for x in (map_ground, map_surf, map_edge) if x is not None)
    h = lambda x: x.h if x is not None else None
    _chk(anyh.ctx.L.lvf_scan_match_edges(h(map_ground), h(scan_ground), h(map_surf), h(scan_surf), h(map_edge), h(scan_edge), _dp(mp), _dp(fp),
                                         _dp(lp) if lp is not None else None, C.byref(opt), C.byref(edge_opt) if edge_opt is not None else None, C.byref(res)))
    return res


def scan_match_options(resolution=0.2, outer_iterations=1, prior_weight=0.0):
    o = ScanMatchOptions()
    _lib.lib().lvf_scan_match_options_default(C.byref(o), float(resolution))
    o.outer_iterations, o.prior_weight = int(outer_iterations), float(prior_weight)
    return o


def scan_match(map_ground, scan_ground, map_surf, scan_surf, map_pose, frame_pose, opt, last_pose=None):
    """Mapping::Optimize's per-frame body (outer_iterations=1, prior) / Mapping::Relocate (outer_iterations=4, no prior)."""
    mp, fp = _d(map_pose), _d(frame_pose)
    lp = _d(last_pose) if last_pose is not None else None
    res = ScanMatchResult()
    anyh = map_ground if map_ground is not None else map_surf
    h = lambda x: x.h if x is not None else None
    _chk(anyh.ctx.L.lvf_scan_match(h(map_ground), h(scan_ground), h(map_surf), h(scan_surf), _dp(mp), _dp(fp), _dp(lp) if lp is not None else None,
                                   C.byref(opt), C.byref(res)))
    return res


def scan_match_batch(ctx, jobs, opt, relocate_base_score=20):
    """Many scan-to-map updates side by side (lvf_scan_match_batch).  jobs: list of dicts with map_ground / scan_ground / map_surf /
    scan_surf (handles or None), map_pose, frame_pose, last_pose (or None).  Returns (results list, best index or -1)."""
    n = len(jobs)
    arr = (ScanMatchJob * max(n, 1))()
    h = lambda x: x.h if x is not None else None
    for j, a in zip(jobs, arr):
        a.map_ground, a.scan_ground, a.map_surf, a.scan_surf = h(j.get("map_ground")), h(j.get("scan_ground")), h(j.get("map_surf")), h(j.get("scan_surf"))
        a.map_pose[:] = list(_d(j["map_pose"])); a.frame_pose[:] = list(_d(j["frame_pose"]))
        lp = j.get("last_pose")
        a.has_last_pose = 0 if lp is None else 1
        if lp is not None:
            a.last_pose[:] = list(_d(lp))
    res = (ScanMatchResult * max(n, 1))()
    best = C.c_int32(-1)
    _chk(ctx.L.lvf_scan_match_batch(ctx.h, arr, n, C.byref(opt), int(relocate_base_score), res, C.byref(best)))
    return list(res)[:n], int(best.value)


def lidar_solve(batch, rpyxyz, huber_a, prior_weight=0.0, max_num_iterations=4):
    """3-DoF LM over a caller-built lidar batch; rpyxyz (float64[6]) is updated IN PLACE."""
    assert rpyxyz.dtype == np.float64 and rpyxyz.flags.c_contiguous and rpyxyz.size == 6
    opt = IcpOptions(0, 0.0, 0.0, float(huber_a), float(prior_weight), int(max_num_iterations))
    summ = IcpSummary()
    _chk(batch.ctx.L.lvf_lidar_solve(batch.h, _dp(rpyxyz), C.byref(opt), C.byref(summ)))
    return summ


class Window:
    """Persistent sliding window (lvf_window_*): Backend::BuildProblem's assembly kept incrementally across ticks."""

    def __init__(self, ctx, left, right, baseline=None, weak_visual_threshold=20, device_assembly=None):
        self.ctx = ctx
        o = WindowOptions()
        ctx.L.lvf_window_options_default(C.byref(o))
        if baseline is not None:
            o.baseline = float(baseline)
        o.weak_visual_threshold = int(weak_visual_threshold)
        if device_assembly is not None:
            o.device_assembly = 1 if device_assembly else 0
        self.h = C.c_void_p()
        cl, cr = make_camera(left), make_camera(right)
        _chk(ctx.L.lvf_window_create(ctx.h, C.byref(cl), C.byref(cr), C.byref(o), C.byref(self.h)))

    def add_keyframe(self, kf_id, pose, w_visual):
        p = _d(pose)
        _chk(self.ctx.L.lvf_window_add_keyframe(self.h, int(kf_id), _dp(p), float(w_visual)))

    def set_imu(self, kf_id, vel, ba, bg, pre=None):
        v, a, g = _d(vel), _d(ba), _d(bg)
        pr = _d(pre) if pre is not None else None
        _chk(self.ctx.L.lvf_window_set_imu(self.h, int(kf_id), _dp(v), _dp(a), _dp(g), _dp(pr) if pr is not None else None))

    def add_landmark(self, lm_id, birth_kf, left_ob, right_ob, inv_depth):
        l, r = _d(left_ob), _d(right_ob)
        _chk(self.ctx.L.lvf_window_add_landmark(self.h, int(lm_id), int(birth_kf), _dp(l), _dp(r), float(inv_depth)))

    def add_observation(self, lm_id, kf_id, ob):
        o = _d(ob)
        _chk(self.ctx.L.lvf_window_add_observation(self.h, int(lm_id), int(kf_id), _dp(o)))

    def remove_observation(self, lm_id, kf_id):
        _chk(self.ctx.L.lvf_window_remove_observation(self.h, int(lm_id), int(kf_id)))

    def reject_outliers(self, max_px=10.0, capacity=4096):
        """Backend::Optimize's outlier gate; returns the removed (landmark id, keyframe id) pairs."""
        lm = (C.c_int64 * capacity)(); kf = (C.c_int64 * capacity)(); n = C.c_int(0)
        _chk(self.ctx.L.lvf_window_reject_outliers(self.h, C.c_double(max_px), lm, kf, capacity, C.byref(n)))
        return [(int(lm[i]), int(kf[i])) for i in range(min(n.value, capacity))], n.value

    def slide(self, first_active_kf):
        _chk(self.ctx.L.lvf_window_slide(self.h, int(first_active_kf)))

    def solve(self, opt):
        s = SolverSummary()
        _chk(self.ctx.L.lvf_window_solve(self.h, C.byref(opt), C.byref(s)))
        return s

    def pose(self, kf_id):
        out = np.empty(7)
        _chk(self.ctx.L.lvf_window_get_pose(self.h, int(kf_id), _dp(out)))
        return out

    def set_pose(self, kf_id, pose):
        p = _d(pose)
        _chk(self.ctx.L.lvf_window_set_pose(self.h, int(kf_id), _dp(p)))

    def imu(self, kf_id):
        v, a, g = np.empty(3), np.empty(3), np.empty(3)
        _chk(self.ctx.L.lvf_window_get_imu(self.h, int(kf_id), _dp(v), _dp(a), _dp(g)))
        return v, a, g

    def inv_depth(self, lm_id):
        d = C.c_double()
        _chk(self.ctx.L.lvf_window_get_inv_depth(self.h, int(lm_id), C.byref(d)))
        return d.value

    def debug_blocks(self, kind):
        """(ids [n][3] int64, vals [n][8]) of the last solve's blocks of one kind (lvf_window_debug_blocks: 0 TwoCamera, 1 PoseOnly, 2 TwoFrame,
        3 ImuError, 4 priors)"""
        n = C.c_int()
        _chk(self.ctx.L.lvf_window_debug_blocks(self.h, int(kind), 0, None, None, C.byref(n)))
        ids = np.zeros((max(n.value, 1), 3), np.int64); vals = np.zeros((max(n.value, 1), 8))
        _chk(self.ctx.L.lvf_window_debug_blocks(self.h, int(kind), n.value, ids.ctypes.data_as(C.c_void_p), _dp(vals), C.byref(n)))
        return ids[:n.value], vals[:n.value]

    def marginal(self, opt, kf_ids):
        """(info, cov, stats) of the keyframes with ids `kf_ids` (1 .. 8) at the window's current state (lvf_window_marginal): the layout of
        Problem.marginal."""
        ids = np.ascontiguousarray(kf_ids, dtype=np.int64).ravel()
        m = 15 * ids.size
        info, cov, st = np.empty((m, m)), np.empty((m, m)), _lib.MarginalStats()
        _chk(self.ctx.L.lvf_window_marginal(self.h, C.byref(opt), ids.ctypes.data_as(C.POINTER(C.c_int64)), int(ids.size), _dp(info), _dp(cov), C.byref(st)))
        return _marginal_result(info, cov, st)

    def set_dense_prior(self, kf_ids, x0=None, info=None, eta=None, c0=0.0):
        """the window's dense prior by keyframe id (DensePrior's arrays; lvf_window_set_dense_prior); kf_ids None or empty removes it"""
        ids = np.zeros(0, np.int64) if kf_ids is None else np.ascontiguousarray(kf_ids, dtype=np.int64).ravel()
        n = int(ids.size)
        if n == 0:
            _chk(self.ctx.L.lvf_window_set_dense_prior(self.h, 0, None, None, None, None, 0.0))
            return
        x0, info = _d(x0), _d(info)
        if n <= 8 and (x0.size != 16 * n or info.shape != (15 * n, 15 * n) or (eta is not None and np.size(eta) != 15 * n)):
            raise ValueError(f"Window.set_dense_prior: {n} keyframes need x0 [{n}][16], info [{15 * n}][{15 * n}] and eta [{15 * n}]")
        eta = None if eta is None else _d(eta)
        _chk(self.ctx.L.lvf_window_set_dense_prior(self.h, n, ids.ctypes.data_as(C.POINTER(C.c_int64)), _dp(x0), _dp(info), None if eta is None else _dp(eta), float(c0)))

    def get_dense_prior(self):
        """dict(kf_ids, x0 [n][16], info, eta, c0) of the window's dense prior, or None (lvf_window_get_dense_prior)"""
        n, ids, x0, info, eta, c0 = C.c_int(), np.zeros(8, np.int64), np.zeros((8, 16)), np.zeros(120 * 120), np.zeros(120), C.c_double()
        _chk(self.ctx.L.lvf_window_get_dense_prior(self.h, C.byref(n), ids.ctypes.data_as(C.POINTER(C.c_int64)), _dp(x0), _dp(info), _dp(eta), C.byref(c0)))
        k = n.value
        if k == 0:
            return None
        return dict(kf_ids=ids[:k].copy(), x0=x0[:k].copy(), info=info[:225 * k * k].reshape(15 * k, 15 * k).copy(), eta=eta[:15 * k].copy(), c0=c0.value)

    def slide_marginalize(self, first_active_kf, opt):
        """slide() that leaves what the departing keyframes knew as a dense prior on the first kept one (lvf_window_slide_marginalize);
        returns the marginalisation's stats (fail != 0: the window slid without a prior)"""
        st = _lib.MarginalStats()
        _chk(self.ctx.L.lvf_window_slide_marginalize(self.h, int(first_active_kf), C.byref(opt), C.byref(st)))
        return dict(fail=int(st.fail), n_present=int(st.n_present), n_absent=int(st.n_absent), min_pivot_ratio=float(st.min_pivot_ratio))

    def set_lidar_planes(self, kf_id, p, pa, pb, pc, weight=None, huber_a=None):
        """the plane blocks of keyframe kf_id's sweep (lidar_pose_batch's arrays); replaces that keyframe's set, empty arrays remove it"""
        p, pa, pb, pc = _d(p).reshape(-1, 3), _d(pa).reshape(-1, 3), _d(pb).reshape(-1, 3), _d(pc).reshape(-1, 3)
        n = p.shape[0]
        w, a = _opt_d(weight, n), _opt_d(huber_a, n)
        _chk(self.ctx.L.lvf_window_set_lidar_planes(self.h, int(kf_id), n, _dp(p), _dp(pa), _dp(pb), _dp(pc), _dp(w) if w is not None else None,
                                                    _dp(a) if a is not None else None))

    def set_lidar_scan(self, kf_id, map_, scan, weight=1.0, huber_a=0.0):
        """the same from what knn3 left in `scan` against `map_`, gathered on the device"""
        _chk(self.ctx.L.lvf_window_set_lidar_scan(self.h, int(kf_id), map_.h, scan.h, float(weight), float(huber_a)))

    def lidar_count(self):
        n = np.zeros(1, np.int32)
        _chk(self.ctx.L.lvf_window_lidar_count(self.h, _ip(n)))
        return int(n[0])

    def counts(self):
        c = np.zeros(8, np.int32)
        _chk(self.ctx.L.lvf_window_counts(self.h, _ip(c)))
        return dict(zip(("kf", "lm", "tc", "tf", "po", "imu", "prior", "lm_known"), c.tolist()))

    def close(self):
        if self.h:
            self.ctx.L.lvf_window_destroy(self.h)
            self.h = C.c_void_p()


def event_pair_us(ctx, reps=25):
    """Microseconds a HIP event pair measures with NOTHING enqueued between its two records (median of `reps`): the marker's own cost,
    which every event-bracketed stage time carries once (bench.py subtracts it so stage times agree with rocprofv3's kernel durations)."""
    ctx.synchronize()
    v = []
    for _ in range(reps):
        ctx.timer_begin(); ctx.timer_end()
        v.append(1e3 * ctx.timer_ms())
    return float(np.median(v))


def box_calibration(ctx):
    """lvf_box_calibration as a dict (see include/lvf.h)"""
    v = np.zeros(8)
    _chk(ctx.L.lvf_box_calibration(ctx.h, _dp(v)))
    return {"ns_per_dependent_fp64_fma": float(v[0]), "shader_clocks_per_dependent_fp64_fma": float(v[1]), "effective_sclk_mhz": float(v[2]),
            "empty_launch_us_back_to_back": float(v[3]), "empty_launch_plus_wait_us": float(v[4]), "rated_sclk_mhz": float(v[5]),
            "rated_mclk_mhz": float(v[6]), "compute_units": int(v[7])}


def comm_unique_id():
    """lvf_comm_get_unique_id: the 128 bytes rank 0 hands to the other ranks out of band"""
    buf = (C.c_ubyte * 128)()
    _chk(_lib.lib().lvf_comm_get_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


class Comm:
    """lvf_comm_*: the path's one exchange through the C-ABI (RCCL opened by the library; world_size 1 needs none)"""
    def __init__(self, ctx, world_size=1, rank=0, unique_id=None):
        self.ctx, self.h = ctx, C.c_void_p()
        idbuf = None
        if unique_id is not None:
            if len(unique_id) != 128:
                raise ValueError("unique id must be the 128 bytes of comm_unique_id()")
            idbuf = C.cast((C.c_ubyte * 128).from_buffer_copy(unique_id), C.c_void_p)
        _chk(ctx.L.lvf_comm_create(ctx.h, int(world_size), int(rank), idbuf, C.byref(self.h)))

    @property
    def world_size(self):
        return int(self.ctx.L.lvf_comm_world_size(self.h))

    @property
    def rank(self):
        return int(self.ctx.L.lvf_comm_rank(self.h))

    def allgather(self, send):
        a = _d(send).ravel()
        out = np.empty((self.world_size, a.size))
        _chk(self.ctx.L.lvf_comm_allgather(self.h, _dp(a), int(a.size), _dp(out)))
        return out

    def close(self):
        if self.h:
            self.ctx.L.lvf_comm_destroy(self.h)
            self.h = C.c_void_p()


def fail_codes():
    """(sparse base, hand-over base) of the failure flag debug_step() returns (lvf_debug_fail_codes): 1 + kb below the first = block step kb of
    the dense corner, [sparse, hand-over) = an elimination level, from the second on = a hand-over time-out"""
    a, b = C.c_int(), C.c_int()
    _lib.lib().lvf_debug_fail_codes(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def debug_landmark_window():
    """entries of a landmark's E band (from its 16-aligned start) requested before the wait for the pose increments (lvf_debug_landmark_window)"""
    return int(_lib.lib().lvf_debug_landmark_window())


def _marginal_result(info, cov, st):
    stats = dict(fail=int(st.fail), n_present=int(st.n_present), n_absent=int(st.n_absent), min_pivot_ratio=float(st.min_pivot_ratio))
    return (info, cov, stats) if st.fail == 0 else (None, None, stats)


def marginal_dense(ctx, S, sel):
    """(info, cov, stats) of the unknowns `sel` (at most 120, distinct, any order) of the symmetric system S [d x d] (lower triangle read;
    S_jj == 0 marks unknown j absent): info = S_ss - S_sr S_rr^-1 S_rs, cov = info^-1 = (S^-1)_ss, row i for sel[i] (lvf_marginal_dense).
    After a numeric failure (stats["fail"] != 0) both matrices are None."""
    S, s = _d(S), _i(sel).ravel()
    if S.ndim != 2 or S.shape[0] != S.shape[1]:
        raise ValueError(f"marginal_dense: S {S.shape} is not square")
    m = max(int(s.size), 1)
    info, cov, st = np.empty((m, m)), np.empty((m, m)), _lib.MarginalStats()
    _chk(ctx.L.lvf_marginal_dense(ctx.h, _dp(S), int(S.shape[0]), _ip(s), int(s.size), _dp(info), _dp(cov), C.byref(st)))
    return _marginal_result(info, cov, st)


class DensePrior:
    """A dense prior on the 15 tangent unknowns of up to eight keyframes (lvf_dense_prior_create; semantics: tests/dense_prior_ref.py):
    cost = c0 + eta^T e + 1/2 e^T info e, e = x [-] x0.  kfs: keyframe positions; x0 [n][16] = pose 7, v 3, ba 3, bg 3; info [15 n][15 n]
    (lower triangle read); eta [15 n] or None."""

    def __init__(self, ctx, kfs, x0, info, eta=None, c0=0.0):
        self.ctx = ctx
        self.h = C.c_void_p()
        k, x0, info = _i(kfs).ravel(), _d(x0), _d(info)
        n = int(k.size)
        if n >= 1 and (x0.size != 16 * n or info.shape != (15 * n, 15 * n) or (eta is not None and np.size(eta) != 15 * n)):
            raise ValueError(f"DensePrior: {n} keyframes need x0 [{n}][16], info [{15 * n}][{15 * n}] and eta [{15 * n}]")
        eta = None if eta is None else _d(eta)
        self.n_sel, self.m = n, 15 * n
        _chk(ctx.L.lvf_dense_prior_create(ctx.h, n, _ip(k), _dp(x0), _dp(info), None if eta is None else _dp(eta), float(c0), C.byref(self.h)))

    def evaluate(self, state, const_bits=None):
        """(cost, gradient [m], matrix [m][m]) at `state` (lvf_dense_prior_evaluate); const_bits: one byte per keyframe of the state"""
        g, H, c = np.empty(self.m), np.empty((self.m, self.m)), C.c_double()
        cb = None
        if const_bits is not None:
            cb = np.ascontiguousarray(const_bits, dtype=np.uint8)
            if cb.size != state.n_kf:
                raise ValueError(f"DensePrior.evaluate: const_bits has {cb.size} entries, the state {state.n_kf} keyframes")
        _chk(self.ctx.L.lvf_dense_prior_evaluate(self.h, state.h, None if cb is None else cb.ctypes.data_as(_lib.c_u8_p), C.byref(c), _dp(g), _dp(H)))
        return c.value, g, H

    def download(self):
        """dict(kfs, x0, info, eta, c0) as created"""
        k, x0, info, eta, c0 = np.empty(self.n_sel, np.int32), np.empty((self.n_sel, 16)), np.empty((self.m, self.m)), np.empty(self.m), C.c_double()
        _chk(self.ctx.L.lvf_dense_prior_download(self.h, _ip(k), _dp(x0), _dp(info), _dp(eta), C.byref(c0)))
        return dict(kfs=k, x0=x0, info=info, eta=eta, c0=c0.value)

    def close(self):
        if self.h:
            self.ctx.L.lvf_dense_prior_destroy(self.h)
            self.h = C.c_void_p()


def default_solver_options():
    o = SolverOptions()
    _lib.lib().lvf_solver_options_default(C.byref(o))
    return o


class Problem:
    def __init__(self, ctx, state, two_camera=None, two_frame=None, pose_only=None, imu=None):
        self.ctx, self.state = ctx, state
        self.h = C.c_void_p()
        hs = [b.h if b is not None else None for b in (two_camera, two_frame, pose_only, imu)]
        _chk(ctx.L.lvf_problem_create(ctx.h, state.h, hs[0], hs[1], hs[2], hs[3], C.byref(self.h)))

    def set_pose_priors(self, batch):
        _chk(self.ctx.L.lvf_problem_set_pose_priors(self.h, batch.h if batch is not None else None))

    def set_lidar_planes(self, batch):
        """adds (None: removes) LiDAR plane blocks on the keyframe poses (lidar_pose_batch / lidar_pose_from_scans); the batch is borrowed"""
        _chk(self.ctx.L.lvf_problem_set_lidar_planes(self.h, batch.h if batch is not None else None))

    def set_dense_prior(self, prior):
        """adds (None: removes) a DensePrior on keyframes of this problem; the prior is borrowed (lvf_problem_set_dense_prior)"""
        _chk(self.ctx.L.lvf_problem_set_dense_prior(self.h, prior.h if prior is not None else None))

    def set_pose_constant(self, kf, const=True):
        _chk(self.ctx.L.lvf_problem_set_pose_constant(self.h, int(kf), 1 if const else 0))

    def set_vbb_constant(self, kf, v=True, ba=True, bg=True):
        _chk(self.ctx.L.lvf_problem_set_vbb_constant(self.h, int(kf), int(bool(v)), int(bool(ba)), int(bool(bg))))

    def cost(self, opt):
        c = C.c_double()
        _chk(self.ctx.L.lvf_problem_cost(self.h, C.byref(opt), C.byref(c)))
        return c.value

    def lm_iteration(self, opt, radius, decrease_factor=2.0):
        r, d, c0, c1, acc = C.c_double(radius), C.c_double(decrease_factor), C.c_double(), C.c_double(), C.c_int()
        _chk(self.ctx.L.lvf_problem_lm_iteration(self.h, C.byref(opt), C.byref(r), C.byref(d), C.byref(c0), C.byref(c1), C.byref(acc)))
        return dict(radius=r.value, decrease_factor=d.value, cost_before=c0.value, cost_after=c1.value, accepted=bool(acc.value))

    def solve(self, opt):
        s = SolverSummary()
        _chk(self.ctx.L.lvf_problem_solve(self.h, C.byref(opt), C.byref(s)))
        return s

    def debug_force_handover_timeout(self, n=1):
        """test hook: the next n chained hand-overs of this problem time out (lvf_problem_debug_force_handover_timeout)"""
        _chk(self.ctx.L.lvf_problem_debug_force_handover_timeout(self.h, int(n)))

    def debug_back_product(self):
        """1 when the current chain takes the (v, ba, bg) back substitution as a product with G, 0 for the sequential levels (lvf_problem_debug_back_product)"""
        return int(self.ctx.L.lvf_problem_debug_back_product(self.h))

    def debug_back_blocks(self):
        """1 when the current chain solves the dense corner on the stored block products T_kj, 0 when it reads S and Dinv (lvf_problem_debug_back_blocks)"""
        return int(self.ctx.L.lvf_problem_debug_back_blocks(self.h))

    def debug_override_reduced(self, S, rhs):
        """test tap: every further iteration of this problem solves (S, rhs) — layout of reduced_system(), lower triangle read — with the
        production chain instead of the system it assembled (lvf_problem_debug_override_reduced).  A single None or a wrong size raises."""
        d = self.ctx.L.lvf_problem_reduced_dim(self.h)
        if S is None or rhs is None:
            _chk(self.ctx.L.lvf_problem_debug_override_reduced(self.h, None if S is None else _dp(_d(S)), None if rhs is None else _dp(_d(rhs))))
            return
        S, rhs = _d(S), _d(rhs)
        if S.shape != (d, d) or rhs.shape != (d,):
            raise ValueError(f"debug_override_reduced: S {S.shape} / rhs {rhs.shape}, the problem's reduced system is {d} x {d}")
        _chk(self.ctx.L.lvf_problem_debug_override_reduced(self.h, _dp(S), _dp(rhs)))

    def debug_clear_override(self):
        _chk(self.ctx.L.lvf_problem_debug_override_reduced(self.h, None, None))

    def debug_last_solved(self):
        """True / False: the last iteration's linear solve succeeded or not (lvf_problem_debug_last_solved); None before any iteration"""
        v = self.ctx.L.lvf_problem_debug_last_solved(self.h)
        return None if v < 0 else bool(v)

    def debug_plan(self):
        """(nb, dense_kf [n_kf] bool): block steps of the dense corner, and which keyframes' (v, ba, bg) blocks stayed in it (lvf_problem_debug_plan)"""
        nb = C.c_int(); dense = np.zeros(self.state.n_kf, np.int32)
        _chk(self.ctx.L.lvf_problem_debug_plan(self.h, C.byref(nb), _ip(dense)))
        return int(nb.value), dense.astype(bool)

    def debug_step(self):
        """(x [d], fail): the reduced step of the last iteration in reduced_system()'s order, and its raw failure flag (lvf_problem_debug_download_step)"""
        d = self.ctx.L.lvf_problem_reduced_dim(self.h)
        x = np.empty(d); fail = C.c_int()
        _chk(self.ctx.L.lvf_problem_debug_download_step(self.h, _dp(x), C.byref(fail)))
        return x, int(fail.value)

    def stage_times(self, opt, radius=1e4, reps=10, spans=False):
        """[(stage name, average microseconds, launches)] of `reps` LM iterations from the current state: the sum of the stage's KERNEL
        durations (start / stop events recorded with every launch — the dispatch timestamps rocprofv3's kernel trace reports).
        spans=True appends the between-stage event span (kernels + gaps + marker cost) as a fourth entry."""
        L = self.ctx.L
        n = L.lvf_problem_stage_count()
        us = np.zeros(n); sp = np.zeros(n); la = (C.c_int * n)()
        _chk(L.lvf_problem_stage_times2(self.h, C.byref(opt), float(radius), int(reps), _dp(us), _dp(sp), la))
        if spans:
            return [(L.lvf_problem_stage_name(i).decode(), float(us[i]), int(la[i]), float(sp[i])) for i in range(n)]
        return [(L.lvf_problem_stage_name(i).decode(), float(us[i]), int(la[i])) for i in range(n)]

    def gradient(self, opt):
        d = self.ctx.L.lvf_problem_reduced_dim(self.h)
        gc = np.empty(d); gl = np.empty(max(self.state.n_lm, 1))
        _chk(self.ctx.L.lvf_problem_gradient(self.h, C.byref(opt), _dp(gc), _dp(gl)))
        return gc, gl[:self.state.n_lm]

    def reduced_system(self):
        d = self.ctx.L.lvf_problem_reduced_dim(self.h)
        S = np.empty((d, d)); rhs = np.empty(d)
        _chk(self.ctx.L.lvf_problem_download_reduced(self.h, _dp(S), _dp(rhs)))
        return S, rhs

    def marginal(self, opt, kfs):
        """(info, cov, stats) of keyframes `kfs` (1 .. 8 positions) at the current state: [15 n x 15 n] each, a keyframe's unknowns in the order
        [pose 6, v 3, ba 3, bg 3] (lvf_problem_marginal).  After a numeric failure (stats["fail"] != 0) both matrices are None."""
        k = _i(kfs).ravel()
        m = 15 * k.size
        info, cov, st = np.empty((m, m)), np.empty((m, m)), _lib.MarginalStats()
        _chk(self.ctx.L.lvf_problem_marginal(self.h, C.byref(opt), _ip(k), int(k.size), _dp(info), _dp(cov), C.byref(st)))
        return _marginal_result(info, cov, st)

    def marginal_prior(self, opt, kfs):
        """(info [15 n x 15 n], eta [15 n], c0, stats): what minimising the problem's local model at the current state over everything but
        keyframes `kfs` leaves on them (lvf_problem_marginal_prior) — with x0 = their current state, the arguments of DensePrior.  After a
        numeric failure (stats["fail"] != 0) info, eta and c0 are None."""
        k = _i(kfs).ravel()
        m = 15 * k.size
        info, eta, c0, st = np.empty((m, m)), np.empty(m), C.c_double(), _lib.MarginalStats()
        _chk(self.ctx.L.lvf_problem_marginal_prior(self.h, C.byref(opt), _ip(k), int(k.size), _dp(info), _dp(eta), C.byref(c0), C.byref(st)))
        stats = dict(fail=int(st.fail), n_present=int(st.n_present), n_absent=int(st.n_absent), min_pivot_ratio=float(st.min_pivot_ratio))
        return (info, eta, c0.value, stats) if st.fail == 0 else (None, None, None, stats)

    def close(self):
        if self.h:
            self.ctx.L.lvf_problem_destroy(self.h)
            self.h = C.c_void_p()


class ProblemBatch:
    """W independent windows advanced by one chain of launches per LM iteration (lvf_problem_batch_*)."""

    def __init__(self, ctx, problems):
        self.ctx, self.problems = ctx, list(problems)
        self.h = C.c_void_p()
        arr = (C.c_void_p * len(self.problems))(*[p.h for p in self.problems])
        _chk(ctx.L.lvf_problem_batch_create(ctx.h, arr, len(self.problems), C.byref(self.h)))

    def uses_tables(self, opt):
        return self.ctx.L.lvf_problem_batch_uses_tables(self.h, C.byref(opt))

    def lm_iteration(self, opt, radius, decrease_factor):
        n = len(self.problems)
        r, d = _d(radius).copy(), _d(decrease_factor).copy()
        c0, c1, acc = np.empty(n), np.empty(n), np.zeros(n, np.int32)
        _chk(self.ctx.L.lvf_problem_batch_lm_iteration(self.h, C.byref(opt), _dp(r), _dp(d), _dp(c0), _dp(c1), _ip(acc)))
        return [dict(radius=r[i], decrease_factor=d[i], cost_before=c0[i], cost_after=c1[i], accepted=bool(acc[i])) for i in range(n)]

    def solve(self, opt):
        out = (SolverSummary * len(self.problems))()
        _chk(self.ctx.L.lvf_problem_batch_solve(self.h, C.byref(opt), out))
        return list(out)

    def close(self):
        if self.h:
            self.ctx.L.lvf_problem_batch_destroy(self.h)
            self.h = C.c_void_p()

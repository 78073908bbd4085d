"""Goal poses with an end-effector orientation: the float64 statement of naf_chain_ik_solve_pose (include/naf_hip.h, "Oriented goal
poses"; csrc/chain_env.hip: chain_ik_pose_kernel). environment/kinematic.py takes every name back in, and KinematicEnvironment
inherits PoseGoalRule: the rule stands beside jacobian / ik_step / solve_ik, which it extends and leaves as they are.

R_ee is the rotation of the frame the walk of jacobian() ends with: the frame whose origin plus R_ee ee_point is ee. An orientation
goal is of one of two kinds per call — ORIENT_FULL: R_goal, nine values row-major; ORIENT_AXIS: a unit direction d in the world
that t = R_ee tool_axis is to point along, the roll about t free. orientation_error() states the angular error e_w of both, a
rotation vector in the world; ik_pose_step() the update; solve_ik_pose() the iteration and its three numbers residual, angle, merit.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

from .urdf_chain import PRISMATIC, axis_rotation

ORIENT_FULL, ORIENT_AXIS = 0, 1       # the two kinds of orientation goal (naf_chain_ik_solve_pose's mode)
ORIENT_SMALL = 1e-6                   # |v| or |t x d| at or below it: the angular error's limit forms


def orientation_error(R_ee, mode: int, goal, tool_axis=(0.0, 0.0, 1.0), tool_normal=(1.0, 0.0, 0.0)) -> np.ndarray:
    """The angular error e_w[..., 3] of the end-effector rotation R_ee[..., 3, 3], a rotation vector in the world.
    ORIENT_FULL, goal = R_goal[..., 3, 3] (or [..., 9] row-major): E = R_goal R_ee^T; its quaternion by the largest-of-four rule
    (Shepperd) — of tr E, E00, E11, E22 the largest decides, the first of equals, which of the four proportional forms
        (E21 - E12, E02 - E20, E10 - E01, 1 + tr)            (1 + E00 - E11 - E22, E01 + E10, E02 + E20, E21 - E12)
        (E01 + E10, 1 + E11 - E00 - E22, E12 + E21, E02 - E20)      (E02 + E20, E12 + E21, 1 + E22 - E00 - E11, E10 - E01)
    of (x, y, z, w) is taken — scaled to unit length, its sign chosen so that w >= 0; theta = 2 atan2(|v|, w); e_w = v theta / |v|,
    or 2 v where |v| <= 1e-6. Well conditioned at theta -> pi, where the (E - E^T) / 2 form is not.
    ORIENT_AXIS, goal = d[..., 3]: t = R_ee tool_axis, x = t x d, theta = atan2(|x|, t . d), e_w = x theta / |x|; where |x| <= 1e-6:
    x if t . d > 0, otherwise pi R_ee tool_normal (half a turn about a fixed axis perpendicular to the tool's)."""
    R = np.asarray(R_ee, float)
    goal = np.asarray(goal, float)
    if mode == ORIENT_AXIS:
        t = R @ np.asarray(tool_axis, float)
        x = np.cross(t, goal)
        nx = np.sqrt(np.sum(x * x, axis=-1))[..., None]
        c = np.sum(t * goal, axis=-1)[..., None]
        small = nx <= ORIENT_SMALL
        turned = x * (np.arctan2(nx, c) / np.where(small, 1.0, nx))
        return np.where(small, np.where(c > 0.0, x, np.pi * (R @ np.asarray(tool_normal, float))), turned)
    if mode != ORIENT_FULL:
        raise ValueError(f"mode is ORIENT_FULL (0) or ORIENT_AXIS (1): got {mode!r}")
    if goal.shape[-1] == 9:
        goal = goal.reshape(goal.shape[:-1] + (3, 3))
    E = goal @ np.swapaxes(R, -1, -2)
    e00, e01, e02, e10, e11, e12, e20, e21, e22 = (E[..., i, j] for i in range(3) for j in range(3))
    tr = e00 + e11 + e22
    forms = np.stack([np.stack([e21 - e12, e02 - e20, e10 - e01, 1.0 + tr], -1),
                      np.stack([1.0 + e00 - e11 - e22, e01 + e10, e02 + e20, e21 - e12], -1),
                      np.stack([e01 + e10, 1.0 + e11 - e00 - e22, e12 + e21, e02 - e20], -1),
                      np.stack([e02 + e20, e12 + e21, 1.0 + e22 - e00 - e11, e10 - e01], -1)], 0)
    k = np.argmax(np.stack([tr, e00, e11, e22], 0), axis=0)      # (the first of equals)
    quat = np.take_along_axis(forms, k[None, ..., None], axis=0)[0]
    quat = quat / np.sqrt(np.sum(quat * quat, axis=-1))[..., None]
    quat = np.where(quat[..., 3:] < 0.0, -quat, quat)
    v, w = quat[..., :3], quat[..., 3:]
    nv = np.sqrt(np.sum(v * v, axis=-1))[..., None]
    small = nv <= ORIENT_SMALL
    return np.where(small, 2.0 * v, v * (2.0 * np.arctan2(nv, w) / np.where(small, 1.0, nv)))


def spd6_solve(M, e):
    """y with M y = e for symmetric positive definite M[..., n, n] and e[..., n] (n = 6 in ik_pose_step) by M = L D L^T without
    pivoting, in the fixed order the device's registers follow: column j = 0 .. n - 1: v_k = l_jk d_k (k < j), d_j = M_jj -
    sum_k l_jk v_k, r_j = 1 / d_j, l_ij = (M_ji - sum_k l_ik v_k) r_j (i > j); z_i = e_i - sum_{k < i} l_ik z_k upwards;
    y_i = z_i r_i - sum_{k > i} l_ki y_k downwards. Only M's upper triangle is read."""
    M, e = np.asarray(M, float), np.asarray(e, float)
    n = M.shape[-1]
    l = [[None] * n for _ in range(n)]
    d, r = [None] * n, [None] * n
    for j in range(n):
        v = [l[j][k] * d[k] for k in range(j)]
        s = M[..., j, j]
        for k in range(j):
            s = s - l[j][k] * v[k]
        d[j], r[j] = s, 1.0 / s
        for i in range(j + 1, n):
            s = M[..., j, i]
            for k in range(j):
                s = s - l[i][k] * v[k]
            l[i][j] = s * r[j]
    z = []
    for i in range(n):
        s = e[..., i]
        for k in range(i):
            s = s - l[i][k] * z[k]
        z.append(s)
    y = [None] * n
    for i in reversed(range(n)):
        s = z[i] * r[i]
        for k in range(i + 1, n):
            s = s - l[k][i] * y[k]
        y[i] = s
    return np.stack(y, axis=-1)


def quaternion_matrix(quaternion) -> np.ndarray:
    """R[..., 3, 3] float32 of the quaternion (x, y, z, w)[..., 4], the convention of a URDF / PyBullet link orientation; it is
    scaled to unit length first (in float64)."""
    quat = np.asarray(quaternion, np.float64)
    quat = quat / np.sqrt(np.sum(quat * quat, axis=-1))[..., None]
    x, y, z, w = (quat[..., k] for k in range(4))
    R = np.stack([np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)], -1),
                  np.stack([2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)], -1),
                  np.stack([2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)], -1)], -2)
    return R.astype(np.float32)


def tool_normal_of(tool_axis) -> np.ndarray:
    """the fixed unit vector perpendicular to the unit tool_axis[3]: tool_axis x e_k, scaled to unit length, with e_k the basis
    vector of tool_axis' smallest component in magnitude (the first of equals)"""
    a = np.asarray(tool_axis, np.float64)
    n = np.cross(a, np.eye(3)[int(np.argmin(np.abs(a)))])
    return n / np.linalg.norm(n)


class OrientationGoal(NamedTuple):
    """The orientation goals of N queries as twin and device are given them, float32 values"""
    mode: int                         # ORIENT_FULL | ORIENT_AXIS
    goals: np.ndarray                 # [N][9] float32: R_goal row-major | [N][3] float32: the unit direction d
    tool_axis: np.ndarray             # [3] float32, unit
    tool_normal: np.ndarray           # [3] float32, unit, perpendicular to tool_axis
    angle_length: float               # float32(tolerance) / float32(orientation_tolerance), formed in float32
    orientation_tolerance: float


def _unit_rows(name: str, value, width: int, N: int) -> np.ndarray:
    """value as [N][width] float64 rows of unit length; [width] stands for every query. ValueError names the query otherwise."""
    try:
        a = np.array(value, float)
    except (TypeError, ValueError):
        raise ValueError(f"{name} is not an array of numbers") from None
    if a.shape == (width,):
        a = np.broadcast_to(a, (N, width))
    if a.shape != (N, width):
        raise ValueError(f"{name} is [N][{width}] with N = {N}, the number of queries, or [{width}] for all of them: got shape {a.shape}")
    bad = np.nonzero(~np.isfinite(a).all(axis=1))[0]
    if len(bad):
        raise ValueError(f"{name}[{int(bad[0])}] is not finite: {a[bad[0]].tolist()}")
    norm = np.sqrt(np.sum(a * a, axis=1))
    bad = np.nonzero(~(norm > 0.0))[0]
    if len(bad):
        raise ValueError(f"{name}[{int(bad[0])}] has length 0: it names no {'rotation' if width == 4 else 'direction'}")
    return a / norm[:, None]


def orientation_goal(N: int, orientations=None, approach_directions=None, tool_axis=(0.0, 0.0, 1.0), tolerance: float = 1e-3,
                     orientation_tolerance: float = 1e-3) -> Optional[OrientationGoal]:
    """The orientation goal of a call's N queries, None where neither kind is given: orientations [N][4] or [4], quaternions
    (x, y, z, w) -> ORIENT_FULL; approach_directions [N][3] or [3] -> ORIENT_AXIS, for tool_axis[3] in the end-effector frame.
    ValueError — both kinds at once, a wrong shape, a value that is not finite, a zero-length quaternion, direction or tool axis,
    an orientation_tolerance that is no positive angle — with the query named."""
    if orientations is None and approach_directions is None:
        return None
    if orientations is not None and approach_directions is not None:
        raise ValueError("orientations and approach_directions are the two kinds of orientation goal: a call takes one of them")
    if isinstance(orientation_tolerance, bool) or not isinstance(orientation_tolerance, (int, float, np.floating)) or \
            not np.isfinite(orientation_tolerance) or not orientation_tolerance > 0.0:
        raise ValueError(f"orientation_tolerance is a positive angle in radians: got {orientation_tolerance!r}")
    try:
        shape = np.shape(tool_axis)
    except ValueError:
        shape = None
    if shape != (3,):
        raise ValueError(f"tool_axis is [3], a direction in the end-effector frame: got shape {shape}")
    axis = _unit_rows("tool_axis", tool_axis, 3, 1)[0]
    if orientations is not None:
        mode, goals = ORIENT_FULL, quaternion_matrix(_unit_rows("orientations", orientations, 4, N)).reshape(N, 9)
    else:
        mode, goals = ORIENT_AXIS, _unit_rows("approach_directions", approach_directions, 3, N).astype(np.float32)
    angle_length = float(np.float32(tolerance) / np.float32(orientation_tolerance))
    return OrientationGoal(mode, np.ascontiguousarray(goals), axis.astype(np.float32), tool_normal_of(axis).astype(np.float32),
                           angle_length, float(orientation_tolerance))


class PoseGoalRule:
    """The oriented goal-pose rule as methods of KinematicEnvironment (which supplies model, n, q, frames, joint_limits, ik_defaults)"""

    def end_effector_frame(self, q: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(R_ee[..., 3, 3], ee[..., 3]) at the driven joint values q"""
        R, p = self.frames(q)[self.model.ee_frame]
        return R, p + R @ self.model.ee_point

    def jacobian6(self, q: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(ee[..., 3], R_ee[..., 3, 3], Jp[..., 3, A], Ja[..., 3, A]): jacobian()'s walk and positional columns Jp, and the angular
        columns Ja: a_m for a revolute joint, 0 for a prismatic one and for a joint behind the end-effector frame."""
        q = self.q if q is None else np.asarray(q, float)
        lead = q.shape[:-1]
        R, p = np.broadcast_to(np.eye(3), lead + (3, 3)), np.zeros(lead + (3,))
        axes, points = [], []
        for m, j in enumerate(self.model.joints[:self.model.ee_frame]):
            p = p + R @ j.pre_xyz
            R = R @ j.pre_rot
            a = R @ j.axis
            axes.append(a)
            points.append(p)
            if j.type == PRISMATIC:
                p = p + a * q[..., m, None]
            else:
                R = R @ axis_rotation(j.axis, q[..., m])
        ee = p + R @ self.model.ee_point
        Jp, Ja = np.zeros(lead + (3, self.n)), np.zeros(lead + (3, self.n))
        for m, j in enumerate(self.model.joints[:self.model.ee_frame]):
            if j.type == PRISMATIC:
                Jp[..., m] = axes[m]
            else:
                Jp[..., m] = np.cross(axes[m], ee - points[m])
                Ja[..., m] = axes[m]
        return ee, R, Jp, Ja

    def ik_pose_defaults(self) -> dict:
        """the oriented iteration's own constants where the caller names none: weight L = 0.25 reach (metres per radian),
        w_max = 0.5 rad; lam, e_max and dq_max are ik_defaults()'s"""
        return dict(weight=0.25 * self.model.reach, w_max=0.5)

    def ik_pose_step(self, q, g, mode: int, goal, lam: float, e_max: float, dq_max: float, weight: float, w_max: float,
                     tool_axis=(0.0, 0.0, 1.0), tool_normal=(1.0, 0.0, 0.0)) -> np.ndarray:
        """One update of the oriented iteration at q[..., A] towards the position g[..., 3] and the orientation goal
        (goal[..., 3, 3] or [..., 9] for ORIENT_FULL, [..., 3] for ORIENT_AXIS): e_p = g - ee cut to e_max as ik_step cuts it, e_w =
        orientation_error cut to w_max; e6 = [e_p ; L e_w]; column m of J6 = [c_m ; L a_m] revolute, [a_m ; 0] prismatic, 0 behind
        the end-effector frame; M = J6 J6^T + lam^2 I; M y = e6 (spd6_solve); dq_m = J6[:, m] . y; then ik_step's dq_max scaling
        and position limits."""
        q = np.asarray(q, float)
        ee, R, Jp, Ja = self.jacobian6(q)
        e = np.asarray(g, float) - ee
        n = np.sqrt(np.sum(e * e, axis=-1))[..., None]
        e = np.where(n > e_max, e * (e_max / np.where(n > 0.0, n, 1.0)), e)
        w = orientation_error(R, mode, goal, tool_axis, tool_normal)
        n = np.sqrt(np.sum(w * w, axis=-1))[..., None]
        w = np.where(n > w_max, w * (w_max / np.where(n > 0.0, n, 1.0)), w)
        J6 = np.concatenate([Jp, weight * Ja], axis=-2)
        e6 = np.concatenate([e, weight * w], axis=-1)
        M = J6 @ np.swapaxes(J6, -1, -2) + (lam * lam) * np.eye(6)
        dq = np.sum(J6 * spd6_solve(M, e6)[..., :, None], axis=-2)
        big = np.max(np.abs(dq), axis=-1)[..., None]
        dq = np.where(big > dq_max, dq * (dq_max / np.where(big > 0.0, big, 1.0)), dq)
        lo, hi = self.joint_limits()
        return np.minimum(np.maximum(q + dq, lo), hi)

    def pose_errors(self, q, g, mode: int, goal, tool_axis=(0.0, 0.0, 1.0), tool_normal=(1.0, 0.0, 0.0)):
        """(residual[...], angle[...]) at q[..., A]: |g - ee| and |e_w|, uncut"""
        R, ee = self.end_effector_frame(np.asarray(q, float))
        d = np.asarray(g, float) - ee
        w = orientation_error(R, mode, goal, tool_axis, tool_normal)
        return np.sqrt(np.sum(d * d, axis=-1)), np.sqrt(np.sum(w * w, axis=-1))

    def solve_ik_pose(self, targets, mode: int, goals, seeds, angle_length: float, lam: Optional[float] = None,
                      e_max: Optional[float] = None, dq_max: Optional[float] = None, weight: Optional[float] = None,
                      w_max: Optional[float] = None, tool_axis=(0.0, 0.0, 1.0), tool_normal=(1.0, 0.0, 0.0), iterations: int = 32):
        """(q[..., A], residual[...], angle[...], merit[...]) per candidate: from seeds[..., A], `iterations` updates by
        ik_pose_step — a fixed trip count — then residual = |g - ee|, angle = |e_w| uncut and merit = max(residual, angle
        angle_length), angle_length = tolerance / orientation_tolerance: a candidate is converged iff merit <= tolerance."""
        d, dp = self.ik_defaults(), self.ik_pose_defaults()
        lam, e_max, dq_max = (d["lam"] if lam is None else lam, d["e_max"] if e_max is None else e_max,
                              d["dq_max"] if dq_max is None else dq_max)
        weight, w_max = dp["weight"] if weight is None else weight, dp["w_max"] if w_max is None else w_max
        q = np.array(seeds, float)
        lead = q.shape[:-1]
        g = np.broadcast_to(np.asarray(targets, float), lead + (3,))
        goals = np.asarray(goals, float)
        if mode == ORIENT_FULL:
            goals = goals.reshape(goals.shape[:-1] + (3, 3)) if goals.shape[-1] == 9 else goals
            goals = np.broadcast_to(goals, lead + (3, 3))
        else:
            goals = np.broadcast_to(goals, lead + (3,))
        for _ in range(int(iterations)):
            q = self.ik_pose_step(q, g, mode, goals, lam, e_max, dq_max, weight, w_max, tool_axis, tool_normal)
        residual, angle = self.pose_errors(q, g, mode, goals, tool_axis, tool_normal)
        return q, residual, angle, np.maximum(residual, angle * angle_length)

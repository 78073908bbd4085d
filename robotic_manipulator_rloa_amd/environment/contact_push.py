"""Goal poses pushed out of contact in the task's null space: the rule of naf_chain_ik_clear (csrc/chain_env.hip; include/naf_hip.h,
"Goal poses out of contact"), stated once, in float64 on the float32 values the device is given.

A candidate's pose q reaches its target and leans on something. The least of all the clearance tests the selection compares with the
margin has a witness — the point x on a capsule's axis where the distance is attained and the unit direction n away from the
geometry — and with it a gradient in the joints, the envelope derivative of the least clearance (Maciejewski & Klein's
obstacle-avoidance point velocity). Each update is the goal-pose iteration's task step (KinematicEnvironment.ik_step) plus that
gradient projected off the task, scaled to the Gauss-Newton length that would lift the one active test to clearance_goal.

  least_test, clearance_gradient, ik_clear_step, refine_goal_poses : the rule on a twin (KinematicEnvironment)
  *_of                                                             : its arithmetic on arrays of whatever float type they are
                                                                     given (every constant is taken into that type): the twin
                                                                     feeds it clear_walk's float64 walk, the tests' float32
                                                                     rehearsal a float32 walk of its own
  clear_defaults, pop_push, note_pushed                            : what goal_poses_host and chain_tools.GoalPoseSolver share

Positional goals only: the 6-row task of an orientation goal is refused (PUSH_ORIENTATION_REFUSAL). What a later 6-row form needs is
one more task_columns_of / clear_update_of pair on PoseGoalRule's columns; least_test and clearance_gradient do not depend on the task.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

from .urdf_chain import PRISMATIC, ChainModel, axis_rotation

CLEAR_SIGMA_FLOOR = 1e-6              # sigma = gamma . h at or below this: no push (the gradient lies in the task's row space)
CLEAR_WITNESS_FLOOR = 1e-6            # a witness distance below this gives a zero gradient (an axis inside a box, two crossing axes):
                                      # a micrometre, above what float32 leaves of a zero distance between points half a metre out
CLEAR_SAME_WITNESS = 1e-6             # two tests whose x and n agree to this are one contact (LeastTest.second does not count it)
CLEAR_ITERATIONS, CLEAR_SETTLE, CLEAR_PUSH_MAX, CLEAR_GOAL_OVER_MARGIN = 16, 4, 0.1, 0.02
CLEAR_KINDS = ("obstacle", "self", "workcell")                           # clear_out[3]
CLEAR_TESTS = ("obstacle", "self", "sphere", "half-space", "box")        # LeastTest.test


def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _unit_or_zero(v, d):
    """v / d where d >= CLEAR_WITNESS_FLOOR, 0 elsewhere"""
    ok = d >= CLEAR_WITNESS_FLOOR
    return np.where(ok[..., None], v / np.where(ok, d, 1.0)[..., None], 0.0).astype(v.dtype)


def segment_point_witness(a, b, c):
    """(x, d): the point of the segment a-b nearest to c — the clamped projection parameter of segment_point_distance2 — and its
    distance from c"""
    ab, ac = b - a, c - a
    den = _dot(ab, ab)
    t = np.clip(_dot(ac, ab) / np.where(den > 0.0, den, 1.0), 0.0, 1.0)
    x = a + t[..., None] * ab
    return x, np.sqrt(_dot(x - c, x - c))


def segment_segment_witness(a1, b1, a2, b2):
    """(x, x', d): the points on a1-b1 and a2-b2 of whichever of segment_segment_distance2's five candidates is least (ties to the
    first: the lines' pair, then a1, b1 against the second segment, a2, b2 against the first) and their distance"""
    u, v, w = b1 - a1, b2 - a2, a1 - a2
    a, b, c = _dot(u, u), _dot(u, v), _dot(v, v)
    d, e = _dot(u, w), _dot(v, w)
    den = a * c - b * b
    ok = den > (1e-14 if a.dtype == np.float64 else 1e-7) * a * c
    s = np.clip(np.where(ok, (b * e - c * d) / np.where(ok, den, 1.0), 0.0), 0.0, 1.0)
    t = np.clip((b * s + e) / np.where(c > 0.0, c, 1.0), 0.0, 1.0) * (c > 0.0)
    s = np.clip((b * t - d) / np.where(a > 0.0, a, 1.0), 0.0, 1.0) * (a > 0.0)
    x, y = a1 + s[..., None] * u, a2 + t[..., None] * v
    best = _dot(x - y, x - y)
    for p, on_first in ((a1, True), (b1, True), (a2, False), (b2, False)):
        near, dist = segment_point_witness(a2, b2, p) if on_first else segment_point_witness(a1, b1, p)
        take = (dist * dist < best)[..., None]
        px, py = (p, near) if on_first else (near, p)
        x, y = np.where(take, px, x), np.where(take, py, y)
        best = np.minimum(best, dist * dist)
    return x, y, np.sqrt(_dot(x - y, x - y))


def segment_box_witness(a, b, half):
    """(t, nearest, d) in the box's frame: the parameter segment_box_distance ends with, the clamp of that point into the box and
    their distance"""
    u = b - a
    one, zero = np.ones(a.shape[:-1] + (1,), a.dtype), np.zeros(a.shape[:-1] + (1,), a.dtype)

    def slope(t):
        x = a + t[..., None] * u
        return np.sum((x - np.clip(x, -half, half)) * u, axis=-1)

    with np.errstate(divide="ignore", invalid="ignore"):
        knots = np.concatenate([(half - a) / u, (-half - a) / u], axis=-1)
    knots = np.where(np.isfinite(knots), np.clip(knots, 0.0, 1.0), 0.0).astype(a.dtype)
    knots = np.sort(np.concatenate([zero, knots, one], axis=-1), axis=-1)
    g = np.stack([slope(knots[..., k]) for k in range(8)], axis=-1)
    n_neg = np.sum(np.cumsum(g > 0.0, axis=-1) == 0, axis=-1)
    lo, hi = np.clip(n_neg - 1, 0, 7)[..., None], np.clip(n_neg, 0, 7)[..., None]
    t_lo, t_hi = np.take_along_axis(knots, lo, -1)[..., 0], np.take_along_axis(knots, hi, -1)[..., 0]
    g_lo, g_hi = np.take_along_axis(g, lo, -1)[..., 0], np.take_along_axis(g, hi, -1)[..., 0]
    den = g_hi - g_lo
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(den > 0.0, t_lo - g_lo * (t_hi - t_lo) / np.where(den > 0.0, den, 1.0), t_lo)
    t = np.where(n_neg == 0, 0.0, np.where(n_neg == 8, 1.0, np.clip(t, t_lo, t_hi))).astype(a.dtype)
    x = a + t[..., None] * u
    near = np.clip(x, -half, half)
    return t, near, np.sqrt(_dot(x - near, x - near))


class LeastTest(NamedTuple):
    """The least clearance test of a pose and its witness; every field has the poses' leading shape [...]."""
    c: np.ndarray                     # the least clearance: the smaller of the three numbers the selection compares with the margin
    kind: np.ndarray                  # int: index into CLEAR_KINDS
    test: np.ndarray                  # int: index into CLEAR_TESTS
    x: np.ndarray                     # [..., 3]: the point on the capsule's axis where the distance is attained
    n: np.ndarray                     # [..., 3]: the unit direction from the geometry's nearest point to x; 0: no gradient
    frame: np.ndarray                 # int: the capsule's frame f: joints m < f move x
    x2: np.ndarray                    # [..., 3]: a self pair's second point x' (n points from x' to x)
    frame2: np.ndarray                # int: its frame f', 0 for every other kind (no joint moves it)
    second: np.ndarray                # the second-least test's clearance, +inf when there is one test only; a test with the
                                      # least one's x and n (two capsules sharing an end point), or like it without a direction, does not count


def least_test_of(model: ChainModel, seg_a, seg_b, obstacle, obstacle_radius) -> LeastTest:
    """least_test on the capsules' world end points seg_a / seg_b [..., segments, 3], in their float type. The tests are taken in the
    device's order — per capsule the obstacle, then the workcell geometries its mask names (spheres, half-spaces, boxes), then
    the self pairs — and a later test replaces the running least only when it is smaller."""
    dt = seg_a.dtype
    k = lambda v: np.asarray(v, dt)      # noqa: E731
    lead = seg_a.shape[:-2]
    obstacle = np.broadcast_to(np.asarray(obstacle, dt), lead + (3,))
    zero3 = np.zeros(lead + (3,), dt)
    state = dict(c=np.full(lead, np.inf, dt), kind=np.zeros(lead, np.int64), test=np.zeros(lead, np.int64), x=zero3, n=zero3,
                 frame=np.zeros(lead, np.int64), x2=zero3, frame2=np.zeros(lead, np.int64), second=np.full(lead, np.inf, dt))

    def offer(c, kind, test, x, n, frame, x2=None, frame2=0):
        take = c < state["c"]
        # the same contact seen through two capsules that share an end point — the same x and n — is one test, not a second one
        # — and so are two tests without a direction (two axes inside boxes): both gradients are zero
        same = (np.max(np.abs(n - state["n"]), axis=-1) <= CLEAR_SAME_WITNESS) & \
            ((np.max(np.abs(x - state["x"]), axis=-1) <= CLEAR_SAME_WITNESS) | ~(np.any(n != 0.0, axis=-1) | np.any(state["n"] != 0.0, axis=-1)))
        state["second"] = np.where(same, state["second"], np.where(take, state["c"], np.minimum(state["second"], c)))
        state["c"] = np.where(take, c, state["c"])
        for key, v in (("kind", kind), ("test", test), ("frame", frame), ("frame2", frame2)):
            state[key] = np.where(take, v, state[key])
        for key, v in (("x", x), ("n", n), ("x2", zero3 if x2 is None else x2)):
            state[key] = np.where(take[..., None], v, state[key])

    G, GH = len(model.cell_spheres), len(model.cell_spheres) + len(model.cell_planes)
    for s, seg in enumerate(model.segments):
        a, b, r = seg_a[..., s, :], seg_b[..., s, :], k(seg.radius)
        x, d = segment_point_witness(a, b, obstacle)
        offer(d - r - k(obstacle_radius), 0, 0, x, _unit_or_zero(x - obstacle, d), seg.frame)
        for g in sorted(g for s2, g in model.cell_pairs if s2 == s):
            if g < G:
                sph = k(model.cell_spheres[g])
                x, d = segment_point_witness(a, b, sph[:3])
                offer(d - sph[3] - r, 2, 2, x, _unit_or_zero(x - sph[:3], d), seg.frame)
            elif g < GH:
                pl = k(model.cell_planes[g - G])
                na, nb = _dot(a, pl[:3]), _dot(b, pl[:3])
                first = (na <= nb)[..., None]
                offer(np.minimum(na, nb) - pl[3] - r, 2, 3, np.where(first, a, b), np.broadcast_to(pl[:3], lead + (3,)), seg.frame)
            else:
                box = k(model.cell_boxes[g - GH])
                R = box[3:12].reshape(3, 3)
                la, lb = (a - box[:3]) @ R, (b - box[:3]) @ R
                t, near, d = segment_box_witness(la, lb, box[12:15])
                local = la + t[..., None] * (lb - la)
                offer(d - box[15] - r, 2, 4, a + t[..., None] * (b - a), _unit_or_zero(local - near, d) @ R.T, seg.frame)
    for s, t in model.self_pairs:
        x, y, d = segment_segment_witness(seg_a[..., s, :], seg_b[..., s, :], seg_a[..., t, :], seg_b[..., t, :])
        offer(d - k(model.segments[s].radius) - k(model.segments[t].radius), 1, 1, x, _unit_or_zero(x - y, d),
              model.segments[s].frame, y, model.segments[t].frame)
    return LeastTest(**state)


def clearance_gradient_of(model: ChainModel, axes, points, lt: LeastTest):
    """gamma[..., A] from the joints' world axes and points [..., A, 3]: n . (a_m x (x - p_m)) for a revolute joint m < f, n . a_m for a
    prismatic one, 0 otherwise; for a self pair minus the same expression at (x', f')"""
    prismatic = np.array([j.type == PRISMATIC for j in model.joints])
    m = np.arange(model.A)

    def at(x, frame):
        moved = np.cross(axes, x[..., None, :] - points)
        return np.where(m < frame[..., None], _dot(lt.n[..., None, :], np.where(prismatic[:, None], axes, moved)), 0.0)

    return (at(lt.x, lt.frame) - at(lt.x2, lt.frame2)).astype(axes.dtype)


def task_columns_of(model: ChainModel, ee, axes, points):
    """[..., A, 3]: the Jacobian's columns c_m of jacobian(), 0 for the joints behind the end-effector frame"""
    prismatic = np.array([j.type == PRISMATIC for j in model.joints])
    cols = np.where(prismatic[:, None], axes, np.cross(axes, ee[..., None, :] - points))
    return np.where((np.arange(model.A) < model.ee_frame)[:, None], cols, 0.0).astype(axes.dtype)


def clear_update_of(model: ChainModel, q, g, ee, axes, points, gamma, c, push_on, lam2, e_max, dq_max, clearance_goal, push_max):
    """One update from a walk's numbers: §15's task step, plus — where push_on and c < clearance_goal — the push
    h (c* - c) / sigma with h = gamma - J^T M^-1 J gamma, sigma = gamma . h > CLEAR_SIGMA_FLOOR, scaled so that max |.| <= push_max;
    then the position limits. Returns (q_next, h)."""
    dt = q.dtype
    e = g - ee
    n = np.sqrt(_dot(e, e))[..., None]
    e = np.where(n > e_max, e * (np.asarray(e_max, dt) / np.where(n > 0.0, n, 1.0)), e)
    cols = task_columns_of(model, ee, axes, points)
    J = np.swapaxes(cols, -1, -2)
    M = J @ cols + np.asarray(lam2, dt) * np.eye(3, dtype=dt)
    dq = _dot(cols, spd3_solve_of(M, e)[..., None, :])
    big = np.max(np.abs(dq), axis=-1)[..., None]
    dq = np.where(big > dq_max, dq * (np.asarray(dq_max, dt) / np.where(big > 0.0, big, 1.0)), dq)
    z = spd3_solve_of(M, _dot(J, gamma[..., None, :]))
    h = gamma - _dot(cols, z[..., None, :])
    sigma = _dot(gamma, h)
    on = push_on & (c < clearance_goal) & (sigma > CLEAR_SIGMA_FLOOR)
    push = h * ((np.asarray(clearance_goal, dt) - c) / np.where(on, sigma, 1.0))[..., None]
    top = np.max(np.abs(push), axis=-1)[..., None]
    push = np.where(top > push_max, push * (np.asarray(push_max, dt) / np.where(top > 0.0, top, 1.0)), push)
    push = np.where(on[..., None], push, 0.0)
    lo = np.array([j.lower if j.limited else -np.inf for j in model.joints]).astype(dt)
    hi = np.array([j.upper if j.limited else np.inf for j in model.joints]).astype(dt)
    return np.minimum(np.maximum(q + dq.astype(dt) + push.astype(dt), lo), hi), h


def spd3_solve_of(M, e):
    """spd3_solve in the float type of its arguments"""
    m00, m01, m02, m11, m12, m22 = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 1], M[..., 1, 2], M[..., 2, 2]
    c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
    c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    det = m00 * c00 + m01 * c01 + m02 * c02
    e0, e1, e2 = e[..., 0], e[..., 1], e[..., 2]
    return np.stack([c00 * e0 + c01 * e1 + c02 * e2, c01 * e0 + c11 * e1 + c12 * e2, c02 * e0 + c12 * e1 + c22 * e2], axis=-1) / det[..., None]


class ClearWalk(NamedTuple):
    ee: np.ndarray                    # [..., 3]
    axes: np.ndarray                  # [..., A, 3]: a_m of ALL driven joints — jacobian()'s record, not stopped at the end-effector frame
    points: np.ndarray                # [..., A, 3]: p_m
    seg_a: np.ndarray                 # [..., segments, 3]: the capsules' world end points
    seg_b: np.ndarray


def clear_walk(twin, q) -> ClearWalk:
    """The walk of the rule at q[..., A]: frames()' and jacobian()'s expressions, all A joints"""
    model = twin.model
    q = np.asarray(q, float)
    lead = q.shape[:-1]
    R, p = np.broadcast_to(np.eye(3), lead + (3, 3)), np.zeros(lead + (3,))
    axes, points, frames = [], [], [(R, p)]
    for m, j in enumerate(model.joints):
        p = p + R @ j.pre_xyz
        R = R @ j.pre_rot
        a = R @ j.axis
        axes.append(a)
        points.append(p)
        if j.type == PRISMATIC:
            p = p + a * q[..., m, None]
        else:
            R = R @ axis_rotation(j.axis, q[..., m])
        frames.append((R, p))
    Re, pe = frames[model.ee_frame]
    seg_a = [frames[s.frame][1] + frames[s.frame][0] @ s.a for s in model.segments]
    seg_b = [frames[s.frame][1] + frames[s.frame][0] @ s.b for s in model.segments]
    return ClearWalk(pe + Re @ model.ee_point, np.stack(axes, -2), np.stack(points, -2), np.stack(seg_a, -2), np.stack(seg_b, -2))


def least_test(twin, q, obstacle, walk: Optional[ClearWalk] = None) -> LeastTest:
    """The least of all the clearance tests at q[..., A] in the scenes obstacle[..., 3] — min(clearance - obstacle radius,
    self_clearance, cell_clearance) — with its witness"""
    w = clear_walk(twin, q) if walk is None else walk
    return least_test_of(twin.model, w.seg_a, w.seg_b, np.asarray(obstacle, float), twin.obstacle_radius)


def clearance_gradient(twin, q, obstacle) -> Tuple[np.ndarray, LeastTest]:
    """(gamma[..., A], the least test): the derivative of the least clearance by the joints at q, where one test is least"""
    w = clear_walk(twin, q)
    lt = least_test(twin, q, obstacle, w)
    return clearance_gradient_of(twin.model, w.axes, w.points, lt), lt


def clear_defaults(margin: float = 0.0, clearance_goal: Optional[float] = None,
                   push_iterations: Optional[int] = None, push_settle: Optional[int] = None, push_max: Optional[float] = None) -> dict:
    """the refinement's constants where the caller names none; ValueError for what naf_chain_ik_clear refuses"""
    out = dict(clearance_goal=float(margin) + CLEAR_GOAL_OVER_MARGIN if clearance_goal is None else clearance_goal,
               iterations=CLEAR_ITERATIONS if push_iterations is None else push_iterations,
               settle=CLEAR_SETTLE if push_settle is None else push_settle, push_max=CLEAR_PUSH_MAX if push_max is None else push_max)
    K, settle = out["iterations"], out["settle"]
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"push_iterations is a number of updates, at least 1: got {K!r}")
    if isinstance(settle, bool) or not isinstance(settle, (int, np.integer)) or not 0 <= settle <= K:
        raise ValueError(f"push_settle is a number of updates without a push, from 0 to push_iterations = {K}: got {settle!r}")
    if not np.isfinite(out["clearance_goal"]):
        raise ValueError(f"clearance_goal is a finite length: got {out['clearance_goal']!r}")
    if not np.isfinite(out["push_max"]) or not out["push_max"] > 0.0:
        raise ValueError(f"push_max is a positive joint update: got {out['push_max']!r}")
    return out


def ik_clear_step(twin, q, g, obstacle, k: int, lam: float, e_max: float, dq_max: float, clearance_goal: float,
                  iterations: int = CLEAR_ITERATIONS, settle: int = CLEAR_SETTLE, push_max: float = CLEAR_PUSH_MAX):
    """Update k (0-based) of the refinement at q[..., A] towards g[..., 3] in the scenes obstacle[..., 3]: (q_next, gamma, least
    test, residual at q). The push is applied only while c < clearance_goal and k < iterations - settle."""
    q = np.asarray(q, float)
    w = clear_walk(twin, q)
    lt = least_test(twin, q, obstacle, w)
    gamma = clearance_gradient_of(twin.model, w.axes, w.points, lt)
    g = np.broadcast_to(np.asarray(g, float), q.shape[:-1] + (3,))
    push_on = np.full(q.shape[:-1], int(k) < int(iterations) - int(settle))
    q_next, _ = clear_update_of(twin.model, q, g, w.ee, w.axes, w.points, gamma, lt.c, push_on, lam * lam, e_max, dq_max, clearance_goal,
                                push_max)
    return q_next, gamma, lt, np.sqrt(_dot(g - w.ee, g - w.ee))


class RefinedPoses(NamedTuple):
    """refine_goal_poses' result, the candidates' leading shape [...]: what naf_chain_ik_clear writes"""
    q: np.ndarray                     # [..., A]: the returned pose
    residual: np.ndarray              # [...]: |g - ee| at it
    clear: np.ndarray                 # [..., 4]: c at the input | c at the returned pose | the returned iterate's index | its kind
    iters: Optional[np.ndarray]       # record: [K + 1, ..., A] the pose before the first and after every update
    rec: Optional[np.ndarray]         # record: [K, ..., A + 2] gamma | c | kind at each update's walk
    second: Optional[np.ndarray]      # record: [K + 1, ...] the second-least test's clearance at every walk


def refine_goal_poses(twin, q, targets, obstacles, tolerance: float = 1e-3, margin: float = 0.0,
                      clearance_goal: Optional[float] = None, push_iterations: Optional[int] = None, push_settle: Optional[int] = None,
                      push_max: Optional[float] = None, lam: Optional[float] = None, e_max: Optional[float] = None,
                      dq_max: Optional[float] = None, record: bool = False) -> RefinedPoses:
    """The refinement of the candidates q[..., A] (a solve's output) towards targets[..., 3] in the scenes obstacles[..., 3].
    Iterate 0 is the input pose; every walk — the K before the updates and one after the last — yields (residual, c); the returned
    pose is the iterate with the largest min(c, clearance_goal) among those with residual <= tolerance, ties to the earliest. A
    candidate whose input keeps clearance_goal, or is not converged, comes back bit for bit."""
    d = twin.ik_defaults()
    lam, e_max, dq_max = (d["lam"] if lam is None else lam, d["e_max"] if e_max is None else e_max, d["dq_max"] if dq_max is None else dq_max)
    p = clear_defaults(margin, clearance_goal, push_iterations, push_settle, push_max)
    K, goal = int(p["iterations"]), float(p["clearance_goal"])
    q0 = np.array(q, float)
    lead = q0.shape[:-1]
    g = np.broadcast_to(np.asarray(targets, float), lead + (3,))
    ob = np.broadcast_to(np.asarray(obstacles, float), lead + (3,))
    qk = q0
    iters, rec, second = [q0], [], []
    for k in range(K + 1):
        if k < K:
            q_next, gamma, lt, res = ik_clear_step(twin, qk, g, ob, k, lam, e_max, dq_max, goal, K, int(p["settle"]), p["push_max"])
        else:
            w = clear_walk(twin, qk)
            lt, res = least_test(twin, qk, ob, w), np.sqrt(_dot(g - w.ee, g - w.ee))
        key = np.where(res <= tolerance, np.minimum(lt.c, goal), -np.inf)
        if k == 0:
            early = (lt.c >= goal) | (res > tolerance)
            c0, best_key = lt.c, key
            best = dict(q=q0, res=res, c=lt.c, index=np.zeros(lead), kind=lt.kind.astype(float))
        else:
            take = (key > best_key) & ~early
            best_key = np.where(take, key, best_key)
            best = dict(q=np.where(take[..., None], qk, best["q"]), res=np.where(take, res, best["res"]), c=np.where(take, lt.c, best["c"]),
                        index=np.where(take, float(k), best["index"]), kind=np.where(take, lt.kind.astype(float), best["kind"]))
        second.append(lt.second)
        if k < K:
            rec.append(np.concatenate([gamma, lt.c[..., None], lt.kind[..., None].astype(float)], axis=-1))
            qk = np.where(early[..., None], q0, q_next)
            iters.append(qk)
    clear = np.stack([c0, best["c"], best["index"], best["kind"]], axis=-1)
    more = (np.stack(iters), np.stack(rec), np.stack(second)) if record else (None, None, None)
    return RefinedPoses(best["q"], best["res"], clear, *more)


PUSH_ARGUMENTS = ("avoid_contact", "clearance_goal", "push_iterations", "push_settle", "push_max")
PUSH_ORIENTATION_REFUSAL = ("avoid_contact pushes goal poses of a position only: with orientations or approach_directions the "
                            "task has six rows and the null-space push is not built for it yet")


def pop_push(kw: dict, orientations=None, approach_directions=None) -> Optional[dict]:
    """Takes PUSH_ARGUMENTS out of a solver's keyword arguments `kw`: None without avoid_contact, otherwise refine_goal_poses' own
    keyword arguments. Refused together with an orientation goal."""
    given = {k: kw.pop(k) for k in PUSH_ARGUMENTS if k in kw}
    if not given.pop("avoid_contact", False):
        return None
    if orientations is not None or approach_directions is not None:
        raise ValueError(PUSH_ORIENTATION_REFUSAL)
    return given


def note_pushed(out, clear, choice=None):
    """fills GoalPoses.pushed / .input_clearance of `out` from the candidates' clear records [N][R][4]; a no-op where clear is None"""
    if clear is not None:
        pick = np.asarray(out.restart if choice is None else choice, np.int64)[:, None, None]
        rec = np.take_along_axis(np.asarray(clear), pick, axis=1)[:, 0]
        out.pushed, out.input_clearance = rec[:, 2] > 0, rec[:, 0]
    return out

"""Line moves: the end effector travels along a straight line in the world, orientation held — the float64 statement of
naf_chain_line_track (include/naf_hip.h, "Line moves"; csrc/chain_env.hip: chain_line_track_kernel) and the one control flow of
ManipulatorFramework.plan_linear_moves, which the device (chain_line.LineTracker + chain_tools.JointPathChecker) and the twin run
alike: track -> verdict -> collision check -> gather. KinematicEnvironment supplies ik_step, ik_pose_step, pose_errors,
end_effector_frame and end_effector; nothing here restates an update.

The rule. Query n has a pose q_start[n] inside the limits and a displacement disp[n] in the world, not zero. W waypoints (1 .. 63)
of U updates each (U >= 1, W U <= 4096). What is held: HOLD_FULL R_goal = R_ee(q_start); HOLD_AXIS d = R_ee(q_start) tool_axis, the
roll free; HOLD_POSITION nothing. The goal is formed ONCE, at q_start, with p0 = ee(q_start). Node 0 is q_start; for i = 1 .. W the
pose of node i - 1 takes U updates towards g_i = p0 + (i / W) disp — ik_pose_step with the held goal, or ik_step — and is node i. The
trip counts are fixed: the updates go on behind a waypoint that was missed. Per waypoint four floats (TRACK_FLOATS): [0] the residual
|g_i - ee(node i)|, [1] the angle |e_w| uncut (0 for HOLD_POSITION), [2] max_m |node[i]_m - node[i - 1]_m|, [3] |ee((node[i - 1] +
node[i]) / 2) - (p0 + ((i - 1/2) / W) disp)|, how far the joint-linear leg is from the line's point at its middle.
The verdict (line_verdict) is the host's: waypoint i is tracked iff [0] <= tolerance and [1] <= orientation_tolerance, K is the
number of leading tracked waypoints. The tracker knows no collision: the W legs go through the edge evaluator plan_paths uses.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

TRACK_FLOATS = 4                      # NAF_CHAIN_TRACK_FLOATS
LINE_WAYPOINTS_MAX = 63               # W + 1 nodes <= 64 = DEMO_MAX_LEGS + 1, the edge launch's V
LINE_UPDATES_MAX = 4096               # W U
HOLD_FULL, HOLD_AXIS, HOLD_POSITION = 0, 1, 2      # naf_chain_line_track's mode
HOLD_MODES = {"orientation": HOLD_FULL, "axis": HOLD_AXIS, "position": HOLD_POSITION}
LINE_OUTCOMES = ("tracked", "lost", "blocked", "start")


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def line_waypoints_ok(W) -> bool:
    return _is_int(W) and 1 <= W <= LINE_WAYPOINTS_MAX


def line_updates_ok(W, U) -> bool:
    return _is_int(U) and U >= 1 and int(W) * int(U) <= LINE_UPDATES_MAX


def line_constants(model, lam=None, e_max=None, dq_max=None, weight=None, w_max=None) -> dict:
    """The updates' constants as device and twin are both given them, float32 values: ik_defaults' lam (as lam2 = lam^2, and the
    lam that is its root), e_max, dq_max and ik_pose_defaults' weight and w_max, unless named"""
    f = lambda v: float(np.float32(v))      # noqa: E731
    lam2 = f((0.05 * model.reach if lam is None else lam) ** 2)
    return dict(lam2=lam2, lam=float(np.sqrt(lam2)), e_max=f(0.25 * model.reach if e_max is None else e_max),
                dq_max=f(0.5 if dq_max is None else dq_max), weight=f(0.25 * model.reach if weight is None else weight),
                w_max=f(0.5 if w_max is None else w_max))


def track_line(twin, q_start, disp, mode: int, W: int, U: int, constants: Optional[dict] = None, tool_axis=(0.0, 0.0, 1.0),
               tool_normal=(1.0, 0.0, 0.0), record: bool = False):
    """(nodes[N][W + 1][A], track[N][W][TRACK_FLOATS]) in float64 — and, with record, iters[W U + 1][N][A], the pose before the
    first and after every update — of the rule above on the values the device is given: q_start[N][A] and disp[N][3] rounded to
    float32, the constants of line_constants."""
    if mode not in (HOLD_FULL, HOLD_AXIS, HOLD_POSITION):
        raise ValueError(f"mode is HOLD_FULL (0), HOLD_AXIS (1) or HOLD_POSITION (2): got {mode!r}")
    if not line_waypoints_ok(W) or not line_updates_ok(W, U):
        raise ValueError(f"W is 1 .. {LINE_WAYPOINTS_MAX} waypoints of U >= 1 updates, W U <= {LINE_UPDATES_MAX}: got {W!r}, {U!r}")
    c = line_constants(twin.model) if constants is None else constants
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)      # noqa: E731
    q, disp = r32(q_start).reshape(-1, twin.model.A), r32(disp).reshape(-1, 3)
    axis, normal = np.asarray(tool_axis, float), np.asarray(tool_normal, float)
    R0, p0 = twin.end_effector_frame(q)
    goal = R0 if mode == HOLD_FULL else R0 @ axis
    nodes, iters = [q], [q]
    track = np.zeros((len(q), W, TRACK_FLOATS))
    for i in range(1, W + 1):
        g, prev = p0 + (i / W) * disp, q
        for _ in range(U):
            if mode == HOLD_POSITION:
                q = twin.ik_step(q, g, c["lam"], c["e_max"], c["dq_max"])
            else:
                q = twin.ik_pose_step(q, g, mode, goal, c["lam"], c["e_max"], c["dq_max"], c["weight"], c["w_max"], axis, normal)
            if record:
                iters.append(q)
        track[:, i - 1] = line_record(twin, prev, q, p0, disp, i, W, mode, goal, axis, normal)
        nodes.append(q)
    out = (np.stack(nodes, axis=1), track)
    return out + (np.stack(iters),) if record else out


def line_record(twin, prev, q, p0, disp, i: int, W: int, mode: int, goal, tool_axis=(0.0, 0.0, 1.0), tool_normal=(1.0, 0.0, 0.0)):
    """[..., TRACK_FLOATS]: waypoint i's record for the nodes prev = node[i - 1] and q = node[i] of a line from p0 along disp"""
    prev, q = np.asarray(prev, float), np.asarray(q, float)
    g = p0 + (i / W) * disp
    if mode == HOLD_POSITION:
        d = g - twin.end_effector(q)
        residual, angle = np.sqrt(np.sum(d * d, axis=-1)), np.zeros(q.shape[:-1])
    else:
        residual, angle = twin.pose_errors(q, g, mode, goal, tool_axis, tool_normal)
    h = twin.end_effector((prev + q) / 2) - (p0 + ((i - 0.5) / W) * disp)
    return np.stack([residual, angle, np.max(np.abs(q - prev), axis=-1), np.sqrt(np.sum(h * h, axis=-1))], axis=-1)


def line_verdict(track, tolerance: float, orientation_tolerance: float) -> Tuple[np.ndarray, np.ndarray]:
    """(K[N], first_lost[N]) from track[N][W][TRACK_FLOATS]: K the number of leading tracked waypoints ([0] <= tolerance and
    [1] <= orientation_tolerance), first_lost = K + 1, the first waypoint that is not, or -1 when K == W. Every comparison is made on
    the values as given, so the device's float32 records and the twin's go through the same rule."""
    track = np.asarray(track)
    W = track.shape[1]
    ok = (track[:, :, 0] <= tolerance) & (track[:, :, 1] <= orientation_tolerance)
    K = np.where(ok.all(axis=1), W, np.argmin(ok, axis=1)).astype(np.int64)
    return K, np.where(K == W, -1, K + 1)


def line_outcomes(K, records, W: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(outcome[N], first_blocked_leg[N], fraction[N]) from the verdict K[N] and the W legs' edge records[N][W][>= EDGE_FLOATS]:
    'start' where sample 0 of leg 0 is blocked; otherwise 'blocked' where a leg l < K of the tracked prefix has a blocked sample
    ([4] > 0), first_blocked_leg the first such; otherwise 'lost' where K < W; otherwise 'tracked'. fraction = min(K, the first
    blocked leg if any) / W, the collision-free tracked share of the line; 'start' has first_blocked_leg 0 and fraction 0."""
    K, rec = np.asarray(K, np.int64), np.asarray(records)
    inside = np.arange(W)[None, :] < K[:, None]
    hit = inside & (rec[:, :, 4] > 0)
    first = np.where(hit.any(axis=1), np.argmax(hit, axis=1), -1).astype(np.int64)
    start = rec[:, 0, 3] == 0
    first = np.where(start, 0, first)
    outcome = np.where(start, "start", np.where(first >= 0, "blocked", np.where(K < W, "lost", "tracked"))).astype("<U8")
    return outcome, first, np.where(first >= 0, np.minimum(K, first), K) / float(W)


class LinearMoves(NamedTuple):
    """Straight-line end-effector moves of N queries (ManipulatorFramework.plan_linear_moves). The collision check is SAMPLED, as
    JointPaths' is: as_joint_paths() hands the tracked lines to certify_joint_paths. With reverse the nodes run from the far end to
    the given pose; first_lost and first_blocked_leg count from the given pose either way."""
    outcome: np.ndarray                 # [N] str: 'tracked' | 'lost' | 'blocked' | 'start' (line_outcomes)
    fraction: np.ndarray                # [N]: the collision-free tracked share of the line
    first_lost: np.ndarray              # [N] int: the first waypoint (1 .. W) that was not tracked, -1: none
    first_blocked_leg: np.ndarray       # [N] int: the first leg (0 .. W - 1) of the tracked prefix with a blocked sample, -1: none
    position_error: np.ndarray          # [N]: the largest residual over the tracked prefix; NaN where it is empty
    angle_error: np.ndarray             # [N]: the largest angle over it; 0 for hold='position'
    joint_step: np.ndarray              # [N]: the largest joint step between two neighbouring nodes, all W waypoints
    line_deviation: np.ndarray          # [N]: the largest mid-leg distance from the line over the tracked prefix
    min_clearance: np.ndarray           # [N]: the least obstacle clearance over the samples of the tracked prefix's legs; NaN: empty
    min_self_clearance: np.ndarray      # [N]: ... self-clearance, +inf without pairs
    min_cell_clearance: np.ndarray      # [N]: ... workcell clearance, +inf without a workcell
    sample_step: np.ndarray             # [N]: the largest max-norm distance between neighbouring samples over those legs
    samples: np.ndarray                 # [N] int: S, the samples per leg
    nodes: np.ndarray                   # [N][W + 1][A]: the tracked prefix's nodes, NaN behind them
    n_nodes: np.ndarray                 # [N] int: K + 1
    start: np.ndarray                   # [N][A]: the first node (with reverse: the far end)
    goal: np.ndarray                    # [N][A]: the last tracked node (with reverse: the given pose)
    end_effector_start: np.ndarray      # [N][3]: p0, the end effector at the given pose
    displacement: np.ndarray            # [N][3]: as given

    def as_joint_paths(self):
        """The 'tracked' lines as a JointPaths that certify_joint_paths and demonstrate_joint_paths(polylines=True) take unchanged:
        outcome 'line', candidate -1, via NaN, nodes and n_nodes = W + 1, length the legs' summed max-norm length, the minima,
        sample_step, samples, start, goal. Every other query gets n_nodes = 0 and outcome 'blocked': it has no path."""
        from .kinematic import JointPaths, joint_distance32
        ok = np.asarray(self.outcome) == "tracked"
        N, A = self.start.shape
        kind = np.asarray(self.min_clearance).dtype           # (float32 where the device's, float64 where the twin's)
        nodes32 = np.asarray(self.nodes, np.float32)
        with np.errstate(invalid="ignore"):
            legs = joint_distance32(nodes32[:, 1:], nodes32[:, :-1])
        length = np.zeros(N, np.float32)
        for l in range(legs.shape[1]):                    # (in path order, in float32: roadmap_search's sum)
            length = length + legs[:, l]
        nan = lambda a: np.where(ok, a, np.nan).astype(kind)      # noqa: E731
        out = JointPaths(np.where(ok, "line", "blocked").astype("<U8"), np.full(N, -1, np.int64), np.full((N, A), np.nan, kind),
                         nan(length), joint_distance32(self.goal, self.start).astype(kind), nan(self.min_clearance),
                         nan(self.min_self_clearance), nan(self.min_cell_clearance), np.full(N, -1, np.int64), nan(self.sample_step),
                         np.asarray(self.samples, np.int64), np.array(self.start), np.array(self.goal), np.zeros(N, bool),
                         np.full(N, np.nan, kind), np.zeros(N, np.int64))
        out.nodes = np.where(ok[:, None, None], self.nodes, np.nan)
        out.n_nodes = np.where(ok, self.n_nodes, 0).astype(np.int64)
        out.roadmap_free_edges = np.full(N, -1, np.int64)
        return out


def gather_linear_moves(nodes, track, records, samples, K, p0, disp, W: int, reverse: bool = False) -> LinearMoves:
    """LinearMoves from the tracker's nodes[N][W + 1][A] and track[N][W][4], the W legs' edge records[N][W][>= EDGE_FLOATS] at
    `samples` samples, the verdict K[N], p0[N][3] and disp[N][3]; reverse flips the order of the tracked prefix's nodes"""
    nodes, track, rec, K = np.asarray(nodes), np.asarray(track), np.asarray(records), np.asarray(K, np.int64)
    N = len(K)
    outcome, first_blocked, fraction = line_outcomes(K, rec, W)
    inside = np.arange(W)[None, :] < K[:, None]
    some = K > 0

    def over(a, fold, fill):
        return np.where(some, fold(np.where(inside, a, fill), axis=1), np.nan).astype(a.dtype)

    kept = np.where((np.arange(W + 1)[None, :] <= K[:, None])[:, :, None], nodes, np.nan)
    if reverse:
        idx = np.clip(K[:, None] - np.arange(W + 1)[None, :], 0, W)
        kept = np.where((np.arange(W + 1)[None, :] <= K[:, None])[:, :, None], np.take_along_axis(nodes, idx[:, :, None], axis=1), np.nan)
    last = np.take_along_axis(kept, K[:, None, None], axis=1)[:, 0]
    return LinearMoves(outcome, fraction.astype(track.dtype), np.where(K == W, -1, K + 1), first_blocked,
                       over(track[:, :, 0], np.max, -np.inf), over(track[:, :, 1], np.max, -np.inf), track[:, :, 2].max(axis=1),
                       over(track[:, :, 3], np.max, -np.inf), over(rec[:, :, 0], np.min, np.inf), over(rec[:, :, 1], np.min, np.inf),
                       over(rec[:, :, 2], np.min, np.inf), over(rec[:, :, 6], np.max, -np.inf), np.full(N, int(samples), np.int64),
                       kept, K + 1, kept[:, 0].copy(), last.copy(), np.asarray(p0), np.asarray(disp))


def plan_line_moves(backend, q_start, disp, obstacles, mode: int, W: int, U: int, tolerance: float = 1e-3,
                    orientation_tolerance: float = 1e-3, resolution: float = 0.02, margin: float = 0.0, reverse: bool = False,
                    tool_axis=(0.0, 0.0, 1.0), tool_normal=None, budget: Optional[int] = None, **constants) -> LinearMoves:
    """The one orchestration of line moves, run by the device and by the twin alike: track -> verdict -> collision check ->
    gather. What differs is the backend, an object with
      dtype, chain  : the records' dtype and the ChainModel
      track(q_start[N][A], disp[N][3], mode, W, U, constants, tool_axis, tool_normal) : (nodes[N][W + 1][A], track[N][W][4])
      end_effectors(q[N][A])                                                           : p0[N][3], for the result only
      edge_records(nodes[n][V][A], edges[E][2], obstacles[n], S, margin)              : records[n][E][EDGE_FLOATS], plan_paths'
    The W legs (l, l + 1) of every query run in one launch per chunk of whole queries (queries x W x S within `budget`
    edge-samples) at S = edge_samples(the call's longest leg, resolution); the edges are shared by the queries. A leg counts only
    inside the tracked prefix l < K (line_outcomes)."""
    from .kinematic import EDGE_FLOATS, PATH_CHUNK, edge_samples, joint_distance32
    from .orientation import tool_normal_of
    W, U = int(W), int(U)
    axis = np.asarray(tool_axis, np.float64)
    axis = (axis / np.linalg.norm(axis)).astype(np.float32)
    normal = (tool_normal_of(axis.astype(np.float64)) if tool_normal is None else np.asarray(tool_normal)).astype(np.float32)
    c = line_constants(backend.chain, **constants)
    q_start = np.ascontiguousarray(q_start, np.float32).reshape(-1, backend.chain.A)
    N = len(q_start)
    disp = np.ascontiguousarray(disp, np.float32).reshape(N, 3)
    obstacles = np.ascontiguousarray(obstacles, np.float32).reshape(N, 3)
    nodes, track = backend.track(q_start, disp, int(mode), W, U, c, axis, normal)
    K, _ = line_verdict(track, backend.dtype(tolerance), backend.dtype(orientation_tolerance))
    nodes32 = np.ascontiguousarray(nodes, np.float32)
    S = edge_samples(joint_distance32(nodes32[:, 1:], nodes32[:, :-1]), resolution)
    edges = np.stack([np.arange(W), np.arange(1, W + 1)], axis=1).astype(np.int32)
    records = np.empty((N, W, EDGE_FLOATS), backend.dtype)
    per = max(1, int(PATH_CHUNK if budget is None else budget) // (W * S))
    for first in range(0, N, per):
        sl = slice(first, first + per)
        records[sl] = backend.edge_records(nodes32[sl], edges, obstacles[sl], S, margin)
    return gather_linear_moves(nodes, track, records, S, K, backend.end_effectors(q_start), disp, W, reverse)


class _TwinLines:
    """plan_line_moves' backend through the twin alone: track_line, and _TwinPaths' edge evaluator on the float32 nodes"""
    dtype = np.float64

    def __init__(self, twin):
        from .kinematic import _TwinPaths
        self.twin, self.chain, self._paths = twin, twin.model, _TwinPaths(twin)

    def track(self, q_start, disp, mode, W, U, constants, tool_axis, tool_normal):
        return track_line(self.twin, q_start, disp, mode, W, U, constants, np.asarray(tool_axis, np.float64),
                          np.asarray(tool_normal, np.float64))

    def end_effectors(self, q):
        return self.twin.end_effector(np.asarray(q, np.float64))

    def edge_records(self, nodes, edges, obstacles, S, margin):
        return self._paths.edge_records(np.asarray(nodes), edges, np.asarray(obstacles, np.float64), S, margin)


def linear_moves_host(twin, q_start, disp, obstacles, mode: int, W: int, U: int, **kw) -> LinearMoves:
    """plan_linear_moves through the twin alone, under the device's rule and on the values the device is given"""
    return plan_line_moves(_TwinLines(twin), q_start, disp, obstacles, mode, W, U, **kw)

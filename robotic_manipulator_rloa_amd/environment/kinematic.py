"""KinematicEnvironment: the float64 host twin of csrc/chain_env.hip, behind the reference Environment's protocol
(environment/environment.py: reset(verbose) -> state[S]; step(action) -> (state, reward, done); observation_space /
action_space as zero arrays), exactly as SyntheticEnvironment offers it.

Built from a ChainModel (environment/urdf_chain.py) and evaluated from the MODEL, not from the packed blob, so that a packing
error shows as a disagreement with the kernel. Kinematic: the commanded velocity is applied exactly for one 1/240 s tick
(environment.py:453-485 with an ideal motor). NOT a port of Bullet: no dynamics, no mesh collision. Self-collision is the
reference's rule (environment.py:311-343, :394-412) between the capsules of model.self_pairs, when the model was compiled with it.
  state  = [pos(A), vel(A), end-effector xyz, target xyz, obstacle xyz], slot k of pos / vel reporting joint INDEX k
           (environment.py:442-451)
  reward = +250 reached (dist < 0.05) | -1000 obstacle contact, self-contact or workcell contact | -(dist - 0.05), done on any
           of them (environment.py:311-371, :416-429). The workcell — fixed spheres, half-spaces and rounded oriented boxes,
           environment/urdf_chain.py — is the model's, and has no slot in the state.
With target_range / obstacle_range every episode gets a scene of its own: choose_scene below is the rule's float64 statement
(include/naf_hip.h, "Scene ranges", is the kernel's).
"""
from __future__ import annotations

import random
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .contact_push import (CLEAR_KINDS, CLEAR_TESTS, PUSH_ORIENTATION_REFUSAL, LeastTest, RefinedPoses, clear_defaults, clear_walk,  # noqa: F401
                           clearance_gradient, ik_clear_step, least_test, note_pushed, pop_push, refine_goal_poses)
from .orientation import (ORIENT_AXIS, ORIENT_FULL, OrientationGoal, PoseGoalRule, orientation_error,  # noqa: F401
                          orientation_goal, quaternion_matrix, spd6_solve, tool_normal_of)
from .segment_distance import segment_box_distance, segment_point_distance2, segment_segment_distance2  # noqa: F401
from .urdf_chain import (DT, OBSTACLE_RADIUS, PRISMATIC, SCENE_TRIES, TARGET_THRESHOLD, ChainModel, axis_rotation, compile_chain,
                         load_urdf)


SCENE_CONDITIONS = ("the target is within reach of the start pose's end effector", "the obstacle touches the arm at the start pose",
                    "the target lies inside the obstacle")


def choose_scene(twin: "KinematicEnvironment", q0, uniforms):
    """The scene of an episode that starts at the joint values q0, from uniforms[K, 6] in [0, 1) — row c: target xyz | obstacle
    xyz of candidate c, K <= SCENE_TRIES rows:
      target_c = target_centre + (2u - 1) * target_range,  obstacle_c = obstacle_centre + (2u - 1) * obstacle_range
    (a half-width of 0 leaves the centre). margins[c] = how far candidate c is on the admissible side of
      (1) |ee(q0) - target_c| >= 0.05 + m     (2) clearance(q0, obstacle_c) - obstacle radius >= m
      (3) |target_c - obstacle_c| >= obstacle radius + 0.05 + m,      m = scene_margin;
    admissible = all three >= 0. Returns (target, obstacle, index, margins[K, 3]): the first admissible candidate, or the
    centres and index -1 when there is none. Batches: q0[..., A] with uniforms[..., K, 6] give arrays with the same lead.
    clearance(q0, obstacle_c) is KinematicEnvironment.clearance's expression, for K centres per pose."""
    u = np.asarray(uniforms, float)
    u = u.reshape((-1, 6)) if u.ndim < 2 else u
    if u.shape[-1] != 6 or u.shape[-2] > SCENE_TRIES:
        raise ValueError(f"choose_scene: uniforms are [K, 6] with at most {SCENE_TRIES} candidates")
    q0 = np.asarray(q0, float)
    targets = twin.target_centre + (2.0 * u[..., :3] - 1.0) * twin.target_range
    obstacles = twin.obstacle_centre + (2.0 * u[..., 3:] - 1.0) * twin.obstacle_range
    m, orad = twin.scene_margin, twin.obstacle_radius
    ee = twin.end_effector(q0)[..., None, :]
    clear = np.min([np.sqrt(segment_point_distance2(a[..., None, :], b[..., None, :], obstacles)) - r
                    for a, b, r in twin.world_segments(q0)], axis=0)
    margins = np.stack([np.linalg.norm(ee - targets, axis=-1) - (TARGET_THRESHOLD + m), clear - orad - m,
                        np.linalg.norm(targets - obstacles, axis=-1) - (orad + TARGET_THRESHOLD + m)], axis=-1)
    ok = np.all(margins >= 0.0, axis=-1)
    index = np.where(np.any(ok, axis=-1), np.argmax(ok, axis=-1), -1)
    pick = np.maximum(index, 0)[..., None, None]
    target = np.where((index < 0)[..., None], twin.target_centre, np.take_along_axis(targets, pick, axis=-2)[..., 0, :])
    obstacle = np.where((index < 0)[..., None], twin.obstacle_centre, np.take_along_axis(obstacles, pick, axis=-2)[..., 0, :])
    return target, obstacle, (int(index) if index.ndim == 0 else index), margins


def _half_widths(v) -> np.ndarray:
    out = np.zeros(3) if v is None else np.array(v, float).reshape(3)
    if not np.all(np.isfinite(out)) or np.any(out < 0.0):
        raise ValueError(f"a scene range is three non-negative half-widths, got {v!r}")
    return out


OUTCOMES = ("frames", "reached", "obstacle", "self", "workcell")      # by outcome code: naf_chain_env_rollout_step's outcome[0]


class Trace(NamedTuple):
    """KinematicEnvironment.trace's result; every field has the queries' leading shape [...]."""
    code: np.ndarray                  # int: index into OUTCOMES (0: the frame budget was used up)
    frames: np.ndarray                # int: steps taken
    final_distance: np.ndarray        # |ee - target| after the last step
    min_clearance: np.ndarray         # min over the steps of clearance - obstacle radius
    min_self_clearance: np.ndarray    # min over the steps of the self-clearance, +inf without pairs
    score: np.ndarray                 # sum of the rewards, in step order
    joint_positions: np.ndarray       # [..., frames + 1, A]: the path; a finished query repeats its final pose
    margins: np.ndarray               # [..., frames, 3]: distance - 0.05 | clearance - obstacle radius | self-clearance; NaN: no step
    min_cell_clearance: np.ndarray    # min over the steps of the workcell clearance, +inf without a workcell (a capsule whose axis
                                      # is inside a box reads -radius - r there: the box rule reports no penetration depth)
    cell_margins: np.ndarray          # [..., frames]: the workcell clearance; NaN: no step


class KinematicEnvironment(PoseGoalRule):

    def __init__(self, model: ChainModel, target_position: Sequence[float], obstacle_position: Sequence[float],
                 obstacle_radius: float = OBSTACLE_RADIUS, target_range: Optional[Sequence[float]] = None,
                 obstacle_range: Optional[Sequence[float]] = None, scene_margin: float = 0.02):
        """target_range / obstacle_range: half-widths xyz of the boxes around target_position / obstacle_position from which
        reset() draws every episode's scene (choose_scene); None or zeros: the scene is fixed."""
        self.model = model
        self.n = model.A
        self.involved_joints = [j.index for j in model.joints]
        self.target_centre = np.array(target_position, float)
        self.obstacle_centre = np.array(obstacle_position, float)
        self.target_range, self.obstacle_range = _half_widths(target_range), _half_widths(obstacle_range)
        self.scene_margin = float(scene_margin)
        if not np.isfinite(self.scene_margin) or self.scene_margin < 0.0:
            raise ValueError(f"scene_margin is a non-negative length, got {scene_margin!r}")
        self.scene_index = -1                                 # the candidate the last reset() took, -1: the centres
        self.target_pos = self.target_centre.copy()           # the episode's scene
        self.obstacle_pos = self.obstacle_centre.copy()
        self.obstacle_radius = float(obstacle_radius)
        self.initial_joint_positions = np.array([j.init for j in model.joints])
        self.initial_positions_variation_range = model.initial_positions_variation_range
        self._observation_space = np.zeros((model.state_size,))
        self._action_space = np.zeros((self.n,))
        self.q = self.initial_joint_positions.copy()          # driven joints, by action index
        self.qd = np.zeros(self.n)
        self.last_distance = float("nan")                     # |ee - target| of the last step
        self.last_clearance = float("nan")                    # min over segments of (distance to the obstacle centre - radius)
        self.last_self_clearance = float("nan")               # min over model.self_pairs of the pair clearance (+inf without pairs)
        self.last_cell_clearance = float("nan")               # min over model.cell_pairs of the workcell clearance (+inf without)

    @property
    def observation_space(self) -> np.ndarray:
        return self._observation_space

    @property
    def action_space(self) -> np.ndarray:
        return self._action_space

    # ---- kinematics -------------------------------------------------------------------------------------------------------
    # Every function below takes q[A] or a batch q[..., A] (and, for the clearance, obstacle centres [..., 3]): the tests drive
    # E device envs against ONE statement of the rule.
    def frames(self, q: Optional[np.ndarray] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
        """(R, p) of frames 0 .. A in the world for driven joint values q."""
        q = self.q if q is None else np.asarray(q, float)
        lead = q.shape[:-1]
        R, p = np.broadcast_to(np.eye(3), lead + (3, 3)), np.zeros(lead + (3,))
        out = [(R, p)]
        for m, j in enumerate(self.model.joints):
            p = p + R @ j.pre_xyz
            R = R @ j.pre_rot
            if j.type == PRISMATIC:
                p = p + (R @ j.axis) * q[..., m, None]
            else:
                R = R @ axis_rotation(j.axis, q[..., m])
            out.append((R, p))
        return out

    def end_effector(self, q: Optional[np.ndarray] = None) -> np.ndarray:
        R, p = self.frames(q)[self.model.ee_frame]
        return p + R @ self.model.ee_point

    def world_segments(self, q: Optional[np.ndarray] = None) -> List[Tuple[np.ndarray, np.ndarray, float]]:
        fr = self.frames(q)
        return [(fr[s.frame][1] + fr[s.frame][0] @ s.a, fr[s.frame][1] + fr[s.frame][0] @ s.b, s.radius)
                for s in self.model.segments]

    def clearance(self, q: Optional[np.ndarray] = None, obstacle: Optional[np.ndarray] = None):
        """min over the capsules of (distance(segment, obstacle centre) - radius); contact iff < obstacle radius."""
        c = self.obstacle_pos if obstacle is None else np.asarray(obstacle, float)
        return np.min([np.sqrt(segment_point_distance2(a, b, c)) - r for a, b, r in self.world_segments(q)], axis=0)

    def pair_clearances(self, q: Optional[np.ndarray] = None) -> np.ndarray:
        """[pairs, ...]: distance(segment s, segment t) - radius_s - radius_t of every pair of model.self_pairs; contact iff < 0."""
        segs = self.world_segments(q)
        lead = np.shape(segs[0][0])[:-1]
        out = np.empty((len(self.model.self_pairs),) + lead)
        for k, (s, t) in enumerate(self.model.self_pairs):
            out[k] = np.sqrt(segment_segment_distance2(segs[s][0], segs[s][1], segs[t][0], segs[t][1])) - segs[s][2] - segs[t][2]
        return out

    def self_clearance(self, q: Optional[np.ndarray] = None):
        """min over model.self_pairs of the pair clearance, +inf without pairs; self-contact iff < 0."""
        lead = np.shape(self.q if q is None else q)[:-1]
        if not self.model.self_pairs:
            return np.full(lead, np.inf) if lead else float("inf")
        return np.min(self.pair_clearances(q), axis=0)

    def cell_clearances(self, q: Optional[np.ndarray] = None) -> np.ndarray:
        """[pairs, ...]: clearance of every (segment, geometry) pair of model.cell_pairs — distance(segment, centre) - radius -
        sphere radius, min(n.a, n.b) - d - radius against a half-space, or segment_box_distance in the box's frame - radius -
        rounding radius against a box; contact iff < 0."""
        segs = self.world_segments(q)
        lead = np.shape(segs[0][0])[:-1]
        pairs, G, GH = self.model.cell_pairs, len(self.model.cell_spheres), len(self.model.cell_spheres) + len(self.model.cell_planes)
        out = np.empty((len(pairs),) + lead)
        for k, (s, g) in enumerate(pairs):
            a, b, r = segs[s]
            if g < G:
                c = np.array(self.model.cell_spheres[g])
                out[k] = np.sqrt(segment_point_distance2(a, b, c[:3])) - r - c[3]
            elif g >= GH:
                x = np.array(self.model.cell_boxes[g - GH])
                R = x[3:12].reshape(3, 3)                     # its columns are the box's axes: v in the box's frame is R^T v = v @ R
                out[k] = segment_box_distance((a - x[:3]) @ R, (b - x[:3]) @ R, x[12:15]) - r - x[15]
            else:
                n = np.array(self.model.cell_planes[g - G])
                out[k] = np.minimum(a @ n[:3], b @ n[:3]) - n[3] - r
        return out

    def cell_clearance(self, q: Optional[np.ndarray] = None):
        """min over model.cell_pairs of the pair's clearance, +inf without a workcell; workcell contact iff < 0."""
        lead = np.shape(self.q if q is None else q)[:-1]
        if not self.model.cell_pairs:
            return np.full(lead, np.inf) if lead else float("inf")
        return np.min(self.cell_clearances(q), axis=0)

    # ---- goal poses: damped least squares on the end effector's positional Jacobian (include/naf_hip.h, "Goal poses") ----
    def jacobian(self, q: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(ee[..., 3], J[..., 3, A]) at the driven joint values q: column m is a_m x (ee - p_m) for a revolute joint, a_m for a
        prismatic one and 0 for a joint behind the end-effector frame (m >= ee_frame), with a_m = (F.R R_pre) axis the joint's axis
        in the world and p_m = F.p + F.R t_pre a point on it — what frames() forms before it applies the joint's motion."""
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
        J = np.zeros(lead + (3, self.n))
        for m, j in enumerate(self.model.joints[:self.model.ee_frame]):
            J[..., m] = axes[m] if j.type == PRISMATIC else np.cross(axes[m], ee - points[m])
        return ee, J

    def joint_limits(self) -> Tuple[np.ndarray, np.ndarray]:
        """(lower[A], upper[A]) as a step applies them: -inf / +inf for a joint without limits"""
        return (np.array([j.lower if j.limited else -np.inf for j in self.model.joints]),
                np.array([j.upper if j.limited else np.inf for j in self.model.joints]))

    def ik_step(self, q, g, lam: float, e_max: float, dq_max: float) -> np.ndarray:
        """One update of the goal-pose iteration at q[..., A] towards g[..., 3]: e = g - ee, scaled to length e_max when longer;
        M = J J^T + lam^2 I; M y = e (spd3_solve); dq = J^T y, the whole of it scaled so that max |dq_m| <= dq_max; q + dq, then
        the position limits exactly as a step applies them."""
        q = np.asarray(q, float)
        ee, J = self.jacobian(q)
        e = np.asarray(g, float) - ee
        n = np.sqrt(np.sum(e * e, axis=-1))[..., None]
        e = np.where(n > e_max, e * (e_max / np.where(n > 0.0, n, 1.0)), e)
        M = J @ np.swapaxes(J, -1, -2) + (lam * lam) * np.eye(3)
        dq = np.sum(J * spd3_solve(M, e)[..., :, None], axis=-2)
        big = np.max(np.abs(dq), axis=-1)[..., None]
        dq = np.where(big > dq_max, dq * (dq_max / np.where(big > 0.0, big, 1.0)), dq)
        lo, hi = self.joint_limits()
        return np.minimum(np.maximum(q + dq, lo), hi)

    def ik_defaults(self) -> dict:
        """the iteration's constants where the caller names none: lam = 0.05 reach, e_max = 0.25 reach, dq_max = 0.5"""
        return dict(lam=0.05 * self.model.reach, e_max=0.25 * self.model.reach, dq_max=0.5)

    def solve_ik(self, targets, seeds, lam: Optional[float] = None, e_max: Optional[float] = None, dq_max: Optional[float] = None,
                 iterations: int = 32) -> Tuple[np.ndarray, np.ndarray]:
        """(q[..., A], residual[...]) per candidate: from the pose seeds[..., A], `iterations` updates by ik_step towards
        targets[..., 3] (broadcast against the seeds' lead) — a fixed trip count, nothing loops until converged — then
        residual = |g - ee(q)|."""
        d = self.ik_defaults()
        lam, e_max, dq_max = (d["lam"] if lam is None else lam, d["e_max"] if e_max is None else e_max,
                              d["dq_max"] if dq_max is None else dq_max)
        q = np.array(seeds, float)
        g = np.broadcast_to(np.asarray(targets, float), q.shape[:-1] + (3,))
        for _ in range(int(iterations)):
            q = self.ik_step(q, g, lam, e_max, dq_max)
        d = g - self.end_effector(q)
        return q, np.sqrt(np.sum(d * d, axis=-1))

    # Goal poses with an end-effector orientation — end_effector_frame, jacobian6, ik_pose_step, pose_errors, solve_ik_pose — are
    # this class's too: environment/orientation.py (PoseGoalRule) states them, beside orientation_error and spd6_solve.

    def get_state(self) -> np.ndarray:
        A = self.n
        out = np.empty(2 * A + 9)
        for k, (src, const) in enumerate(self.model.slots):
            out[k] = self.q[src] if src >= 0 else const
            out[A + k] = self.qd[src] if src >= 0 else 0.0
        out[2 * A:2 * A + 3] = self.end_effector()
        out[2 * A + 3:2 * A + 6] = self.target_pos
        out[2 * A + 6:] = self.obstacle_pos
        return out

    # ---- protocol ---------------------------------------------------------------------------------------------------------
    def reset(self, verbose: bool = True) -> np.ndarray:
        """Joint index k starts at initial_joint_positions[k] + U(-variation[k], +variation[k]) from Python's global RNG
        (environment.py:284-293); only driven joints vary. With scene ranges the episode's target and obstacle follow from the
        same RNG: candidates are drawn one at a time (components of half-width 0 are not drawn) until choose_scene admits one, at
        most SCENE_TRIES."""
        self.q = np.array([random.uniform(j.init - j.variation, j.init + j.variation) if j.variation > 0.0 else j.init
                           for j in self.model.joints])
        self.qd = np.zeros(self.n)
        if self.scene_ranges_on:
            half = np.concatenate([self.target_range, self.obstacle_range])
            self.target_pos, self.obstacle_pos, self.scene_index = self.target_centre.copy(), self.obstacle_centre.copy(), -1
            for c in range(SCENE_TRIES):
                u = [random.random() if h > 0.0 else 0.5 for h in half]
                target, obstacle, index, _ = choose_scene(self, self.q, [u])
                if index == 0:
                    self.target_pos, self.obstacle_pos, self.scene_index = target, obstacle, c
                    break
        return self.get_state()

    @property
    def scene_ranges_on(self) -> bool:
        return bool(np.any(self.target_range > 0.0) or np.any(self.obstacle_range > 0.0))

    def step(self, action) -> Tuple[np.ndarray, float, int]:
        a = np.asarray(action, float).reshape(self.n)
        q = self.q + DT * a                                   # velocity control: commanded velocity held for one tick
        qd = a.copy()
        for m, j in enumerate(self.model.joints):
            if j.limited and not (j.lower <= q[m] <= j.upper):
                q[m] = min(max(q[m], j.lower), j.upper)       # a joint its limit stopped reports velocity 0
                qd[m] = 0.0
        self.q, self.qd = q, qd
        state = self.get_state()
        A = self.n
        dist = float(np.linalg.norm(state[2 * A:2 * A + 3] - self.target_pos))
        clear = float(self.clearance())
        self_clear = float(self.self_clearance())
        cell_clear = float(self.cell_clearance())
        self.last_distance, self.last_clearance, self.last_self_clearance = dist, clear, self_clear
        self.last_cell_clearance = cell_clear
        reached = dist < TARGET_THRESHOLD
        # environment.py:311-343: either collision ends the episode; so does contact with the workcell
        hit = clear < self.obstacle_radius or self_clear < 0.0 or cell_clear < 0.0
        reward = 250 if reached else (-1000 if hit else -1 * (dist - TARGET_THRESHOLD))
        return state, reward, 1 if (reached or hit) else 0


    def trace(self, q0, actions, target, obstacle, frames: int) -> Trace:
        """The rollout rule of naf_chain_env_rollout_step in float64: from the joint values q0[..., A] (clamped into the limits),
        step t applies actions[..., t, A] under step()'s rule in the scene target[..., 3] / obstacle[..., 3], until the query
        reaches the target, touches the obstacle, itself or the workcell, or has taken `frames` steps; from then on it is held. Pure: neither
        self.q, the episode's scene nor any RNG is touched."""
        q = np.array(q0, float)
        lead = q.shape[:-1]
        A, frames = self.n, int(frames)
        actions = np.broadcast_to(np.asarray(actions, float), lead + (frames, A))
        target = np.broadcast_to(np.asarray(target, float), lead + (3,))
        obstacle = np.broadcast_to(np.asarray(obstacle, float), lead + (3,))
        lo = np.array([j.lower if j.limited else -np.inf for j in self.model.joints])
        hi = np.array([j.upper if j.limited else np.inf for j in self.model.joints])
        q = np.minimum(np.maximum(q, lo), hi)
        code, steps = np.zeros(lead, np.int64), np.zeros(lead, np.int64)
        live = np.ones(lead, bool)
        dist, score = np.full(lead, np.nan), np.zeros(lead)
        min_clear, min_self, min_cell = np.full(lead, np.inf), np.full(lead, np.inf), np.full(lead, np.inf)
        cell_margins = np.full(lead + (frames,), np.nan)
        path = np.empty(lead + (frames + 1, A))
        margins = np.full(lead + (frames, 3), np.nan)
        path[..., 0, :] = q
        for t in range(frames):
            q = np.where(live[..., None], np.minimum(np.maximum(q + DT * actions[..., t, :], lo), hi), q)
            path[..., t + 1, :] = q
            # step()'s own expression, vector by vector (a norm taken along an axis rounds differently from the norm of one vector)
            d = (self.end_effector(q) - target).reshape(-1, 3)
            d = np.array([np.linalg.norm(v) for v in d]).reshape(lead)
            clear = self.clearance(q, obstacle) - self.obstacle_radius
            self_clear = self.self_clearance(q) + np.zeros(lead)
            cell_clear = self.cell_clearance(q) + np.zeros(lead)
            reached, hit, self_hit, cell_hit = d < TARGET_THRESHOLD, clear < 0.0, self_clear < 0.0, cell_clear < 0.0
            reward = np.where(reached, 250.0, np.where(hit | self_hit | cell_hit, -1000.0, -1 * (d - TARGET_THRESHOLD)))
            cell_margins[..., t] = np.where(live, cell_clear, np.nan)
            margins[..., t, :] = np.where(live[..., None], np.stack([d - TARGET_THRESHOLD, clear, self_clear], axis=-1), np.nan)
            dist = np.where(live, d, dist)
            score = np.where(live, score + reward, score)
            min_clear = np.where(live, np.minimum(min_clear, clear), min_clear)
            min_self = np.where(live, np.minimum(min_self, self_clear), min_self)
            min_cell = np.where(live, np.minimum(min_cell, cell_clear), min_cell)
            steps = steps + live
            code = np.where(live, np.where(reached, 1, np.where(hit, 2, np.where(self_hit, 3, np.where(cell_hit, 4, 0)))), code)
            live = live & ~(reached | hit | self_hit | cell_hit)
        return Trace(code, steps, dist, min_clear, min_self, score, path, margins, min_cell, cell_margins)


def spd3_solve(M, e):
    """y with M y = e for symmetric positive definite M[..., 3, 3] and e[..., 3], in closed form: the adjugate over the determinant
    (only M's upper triangle is read)."""
    M, e = np.asarray(M, float), np.asarray(e, float)
    m00, m01, m02, m11, m12, m22 = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2], M[..., 1, 1], M[..., 1, 2], M[..., 2, 2]
    c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
    c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    det = m00 * c00 + m01 * c01 + m02 * c02
    e0, e1, e2 = e[..., 0], e[..., 1], e[..., 2]
    return np.stack([c00 * e0 + c01 * e1 + c02 * e2, c01 * e0 + c11 * e1 + c12 * e2, c02 * e0 + c12 * e1 + c22 * e2], axis=-1) / det[..., None]


def joint_distance32(q, q_start) -> np.ndarray:
    """max_m |q_m - q_start_m| in float32, operation for operation what the device forms (one subtraction per joint, exact abs / max)"""
    q, q_start = np.asarray(q, np.float32), np.asarray(q_start, np.float32)
    return np.max(np.abs(q - q_start), axis=-1)


def select_goal_pose(residual, joint_distance, clearance, self_clearance, cell_clearance, tolerance: float, margin: float = 0.0):
    """The selection among the R candidates of each query, arrays [..., R] (clearance already minus the obstacle radius; +inf where
    there are no pairs / no workcell): class 0 = converged (residual <= tolerance) and free (all three clearances >= margin),
    1 = converged but not free, 2 = not converged. The lowest class wins; inside classes 0 and 1 the smallest joint_distance,
    inside class 2 the smallest residual; ties go to the lowest r. Returns (choice[...], class[...]): reachable iff class <= 1, free
    iff class == 0. Every comparison is made on the values as given, so float32 inputs give the device's answer bit for bit."""
    residual, jd = np.asarray(residual), np.asarray(joint_distance)
    free = (np.asarray(clearance) >= margin) & (np.asarray(self_clearance) >= margin) & (np.asarray(cell_clearance) >= margin)
    cls = np.where(residual <= tolerance, np.where(free, 0, 1), 2)
    value = np.where(cls == 2, residual, jd).astype(np.float64)
    R = cls.shape[-1]
    best_c, best_v, best_r = cls[..., 0], value[..., 0], np.zeros(cls.shape[:-1], np.int64)
    for r in range(1, R):
        c, v = cls[..., r], value[..., r]
        take = (c < best_c) | ((c == best_c) & (v < best_v))
        best_c, best_v, best_r = np.where(take, c, best_c), np.where(take, v, best_v), np.where(take, r, best_r)
    return best_r, best_c


class _GoalPoseFields(NamedTuple):
    """the ten members of GoalPoses' tuple"""
    reachable: np.ndarray             # [N] bool: a restart converged (|target - end effector| <= tolerance)
    free: np.ndarray                  # [N] bool: ... and its pose keeps clearance_margin from obstacle, arm and workcell
    joint_positions: np.ndarray       # [N][A]: the chosen pose, entry m = involved_joints[m] (not a goal pose where not reachable)
    residual: np.ndarray              # [N]: |target - end effector| at that pose
    clearance: np.ndarray             # [N]: arm to obstacle surface at that pose
    self_clearance: np.ndarray        # [N]: +inf without self-collision pairs
    cell_clearance: np.ndarray        # [N]: +inf without a workcell
    joint_distance: np.ndarray        # [N]: max_m |pose_m - start pose_m|, the straight joint-space distance in the max-norm
    restart: np.ndarray               # [N] int: the chosen restart; 0 is the one seeded with the start pose
    converged_restarts: np.ndarray    # [N] int: how many of the restarts converged


class GoalPoses(_GoalPoseFields):
    """Goal poses of N queries (ManipulatorFramework.solve_goal_poses): per query the restart the selection rule chose. With an
    orientation goal `angle_residual` is filled, a candidate is converged iff merit = max(residual, angle_residual tolerance /
    orientation_tolerance) <= tolerance, and `reachable` / `converged_restarts` count that. It is an attribute behind the tuple, as
    JointPaths' later ones are: the tuple's ten fields are what they were and every loop over them runs as before. _replace keeps it."""
    angle_residual: Optional[np.ndarray] = None      # [N]: |e_w| at the chosen pose, radians; None without an orientation goal
    # with avoid_contact (refine_goal_poses), None without it:
    pushed: Optional[np.ndarray] = None              # [N] bool: the chosen pose is a later iterate of the refinement than its input
    input_clearance: Optional[np.ndarray] = None     # [N]: the least clearance of the chosen candidate before the refinement

    def _replace(self, **kw):
        out = super()._replace(**kw)
        out.__dict__.update(self.__dict__)
        return out


def ik_restarts_ok(restarts) -> bool:
    return isinstance(restarts, (int, np.integer)) and not isinstance(restarts, bool) and 1 <= restarts <= 64 and \
        (restarts & (restarts - 1)) == 0


def ik_seeds(model: ChainModel, n_queries: int, restarts: int, seed: int) -> np.ndarray:
    """[N][R][A] float32: the seed poses of restarts 1 .. R - 1, uniform inside the limits (+-pi for a revolute joint without
    limits) from numpy's default Generator of `seed`; entry [n][0] is not a seed (restart 0 starts at the query's start pose) and
    holds zeros."""
    lo = np.array([j.lower if j.limited else -np.pi for j in model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in model.joints])
    out = np.zeros((n_queries, restarts, model.A), np.float32)
    draw = np.random.default_rng(seed).uniform(lo, hi, (n_queries, restarts - 1, model.A)).astype(np.float32)
    out[:, 1:] = np.minimum(np.maximum(draw, lo.astype(np.float32)), hi.astype(np.float32))     # (the limits as the device holds them)
    return out


def gather_goal_poses(choice, cls, q, residual, clearance, self_clearance, cell_clearance, joint_distance, tolerance, angle=None,
                      merit=None) -> GoalPoses:
    """GoalPoses from the per-candidate arrays [N][R](, [A]) and the selection (choice[N], class[N]); with an orientation goal
    angle[N][R] and merit[N][R] too: converged_restarts then counts merit <= tolerance"""
    pick = np.asarray(choice, np.int64)[:, None]
    take = lambda a: np.take_along_axis(np.asarray(a), pick, axis=1)[:, 0]      # noqa: E731
    cls = np.asarray(cls)
    out = GoalPoses(cls <= 1, cls == 0, np.take_along_axis(np.asarray(q), pick[:, :, None], axis=1)[:, 0], take(residual),
                    take(clearance), take(self_clearance), take(cell_clearance), take(joint_distance), pick[:, 0],
                    np.sum(np.asarray(residual if merit is None else merit) <= tolerance, axis=1))
    if angle is not None:
        out.angle_residual = take(angle)
    return out


def concatenate_goal_poses(parts: Sequence[GoalPoses]) -> GoalPoses:
    """the GoalPoses of the chunks of one call, in order"""
    out = GoalPoses(*[np.concatenate([getattr(p, f) for p in parts]) for f in GoalPoses._fields])
    for name in ("angle_residual", "pushed", "input_clearance"):
        if getattr(parts[0], name) is not None:
            setattr(out, name, np.concatenate([getattr(p, name) for p in parts]))
    return out


def goal_poses_host(twin: KinematicEnvironment, q0, targets, obstacles, restarts: int = 8, iterations: int = 32,
                    tolerance: float = 1e-3, margin: float = 0.0, seed: int = 0, orientations=None, approach_directions=None,
                    tool_axis=(0.0, 0.0, 1.0), orientation_tolerance: float = 1e-3, orientation_weight: Optional[float] = None,
                    **constants) -> GoalPoses:
    """solve_goal_poses through the twin alone, under the device's rule and on the values the device is given: start poses,
    targets, obstacles and seeds rounded to float32, the iteration and the clearances in float64, joint_distance in float32.
    With orientations or approach_directions (orientation_goal) the iteration is solve_ik_pose on the float32 goal the device is
    given, and the selection is fed merit in the place of residual.
    avoid_contact=True (with clearance_goal, push_iterations, push_settle, push_max: contact_push.PUSH_ARGUMENTS): between the solve and
    the clearances every candidate goes through refine_goal_poses (positional goals only); GoalPoses.pushed and .input_clearance
    are then filled."""
    push = pop_push(constants, orientations, approach_directions)
    r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)      # noqa: E731
    q0, targets, obstacles = r32(q0), r32(targets), r32(obstacles)
    N, R = len(q0), int(restarts)
    seeds = ik_seeds(twin.model, N, R, seed).astype(np.float64)
    seeds[:, 0] = q0
    og = orientation_goal(N, orientations, approach_directions, tool_axis, tolerance, orientation_tolerance)
    angle = merit = None
    if og is None:
        q, residual = twin.solve_ik(targets[:, None, :], seeds, iterations=iterations, **constants)
    else:
        q, residual, angle, merit = twin.solve_ik_pose(
            targets[:, None, :], og.mode, og.goals.astype(np.float64)[:, None, :], seeds, og.angle_length, weight=orientation_weight,
            tool_axis=og.tool_axis.astype(np.float64), tool_normal=og.tool_normal.astype(np.float64), iterations=iterations, **constants)
    obstacle = np.broadcast_to(obstacles[:, None, :], q.shape[:-1] + (3,))
    refined = None if push is None else refine_goal_poses(twin, q, targets[:, None, :], obstacle, tolerance, margin, **push, **constants)
    if refined is not None:
        q, residual = refined.q, refined.residual
    clear = twin.clearance(q, obstacle) - twin.obstacle_radius
    self_clear, cell_clear = twin.self_clearance(q) + np.zeros(clear.shape), twin.cell_clearance(q) + np.zeros(clear.shape)
    jd = joint_distance32(q, q0[:, None, :])
    choice, cls = select_goal_pose(residual if merit is None else merit, jd, clear, self_clear, cell_clear, tolerance, margin)
    return note_pushed(gather_goal_poses(choice, cls, q, residual, clear, self_clear, cell_clear, jd, tolerance, angle, merit),
                       None if refined is None else refined.clear, choice)


# ---- joint paths: the sampled collision check of start -> via -> goal polylines (include/naf_hip.h, "Joint paths") ----------------
PATH_FLOATS = 8                       # NAF_CHAIN_PATH_FLOATS
PATH_SAMPLES_MIN, PATH_SAMPLES_MAX = 64, 2048
PATH_CANDIDATES_MAX = 64
PATH_CHUNK = 1 << 23                  # candidate-samples per chunk, on the device and through the twin alike
PATH_OUTCOMES = ("straight", "via", "blocked", "start", "goal")
PATH_CERT_FLOATS = 12                 # NAF_CHAIN_PATH_CERT_FLOATS


def path_samples_ok(S) -> bool:
    return isinstance(S, (int, np.integer)) and not isinstance(S, bool) and PATH_SAMPLES_MIN <= S <= PATH_SAMPLES_MAX and S % 64 == 0


def path_pose(a, via, b, i, S: int) -> np.ndarray:
    """Sample i of the S poses of the joint-space polyline a -> via -> b, in float64; a, via, b [..., A] and i [...] broadcast.
    With h = S / 2: i < h lies on leg 1 at f = i / h (the start included, the via not), i >= h on leg 2 at f = (i - h) / (h - 1)
    (the via and the goal included); q_m = lo_m + f (hi_m - lo_m) between the leg's end poses, and the end pose itself at f = 1. No
    limits are applied and an unlimited revolute joint is interpolated numerically, with no wrap-around."""
    a, via, b = np.asarray(a, float), np.asarray(via, float), np.asarray(b, float)
    i, h = np.asarray(i), int(S) // 2
    second = i >= h
    f = np.where(second, (i - h) / (h - 1), i / h)[..., None]
    lo, hi = np.where(second[..., None], via, a), np.where(second[..., None], b, via)
    return np.where(f == 1.0, hi, lo + f * (hi - lo))


def check_joint_path(twin: KinematicEnvironment, q_start, via, q_goal, obstacle, S: int, margin: float = 0.0) -> np.ndarray:
    """[..., PATH_FLOATS] float64: the record of the candidate paths q_start[..., A] -> via[..., A] -> q_goal[..., A] in the scenes
    obstacle[..., 3] (all broadcast), sampled at the S poses of path_pose: [0] [1] [2] the minima over the samples of the obstacle
    clearance (the obstacle radius subtracted), the self-clearance and the workcell clearance | [3] the index of the first blocked
    sample, -1: none | [4] how many are blocked | [5] L1 + L2 with L = joint_distance32 of a leg, in float32 | [6] the sample step
    max(L1 / h, L2 / (h - 1)), in float32 | [7] 1 iff the last sample, the goal pose, is blocked. A sample is blocked iff one of
    its three clearances is < margin. SAMPLED: the verdict holds at the samples and says nothing between them."""
    if not path_samples_ok(S):
        raise ValueError(f"S is a multiple of 64 from {PATH_SAMPLES_MIN} to {PATH_SAMPLES_MAX}: got {S!r}")
    q_start, via, q_goal = np.broadcast_arrays(np.asarray(q_start, float), np.asarray(via, float), np.asarray(q_goal, float))
    lead = via.shape[:-1]
    obstacle = np.broadcast_to(np.asarray(obstacle, float), lead + (3,))
    q = path_pose(q_start[..., None, :], via[..., None, :], q_goal[..., None, :], np.arange(S), S)
    clear = twin.clearance(q, obstacle[..., None, :]) - twin.obstacle_radius
    self_clear, cell_clear = twin.self_clearance(q) + np.zeros(clear.shape), twin.cell_clearance(q) + np.zeros(clear.shape)
    blocked = (clear < margin) | (self_clear < margin) | (cell_clear < margin)
    h = np.float32(S // 2)
    l1, l2 = joint_distance32(via, q_start), joint_distance32(q_goal, via)
    out = np.empty(lead + (PATH_FLOATS,))
    out[..., 0], out[..., 1], out[..., 2] = clear.min(axis=-1), self_clear.min(axis=-1), cell_clear.min(axis=-1)
    out[..., 3] = np.where(blocked.any(axis=-1), np.argmax(blocked, axis=-1), -1)
    out[..., 4] = blocked.sum(axis=-1)
    out[..., 5] = l1 + l2
    out[..., 6] = np.maximum(l1 / h, l2 / (h - np.float32(1.0)))
    out[..., 7] = blocked[..., -1]
    return out


def path_vias(model: ChainModel, q_start, q_goal, candidates: int, seed: int) -> np.ndarray:
    """[N][C][A] float32: the via poses of the C candidate paths of each query, from the poses as float32 holds them. Candidate 0
    is the midpoint 0.5 (a + b): the straight line. Candidate c >= 1 is mid + (2u - 1) w_c per joint, w_c = 0.5 2^((c - 1) mod 3)
    max(D, 0.5) with D the straight max-norm distance, u from ONE np.random.default_rng(seed).random((N, C - 1, A)) call; clipped
    into the limits of limited joints (as the device holds them), so every sample of every candidate lies inside the limits."""
    a = np.asarray(q_start, np.float32).astype(np.float64).reshape(-1, model.A)
    b = np.asarray(q_goal, np.float32).astype(np.float64).reshape(-1, model.A)
    N, C = len(a), int(candidates)
    mid = 0.5 * (a + b)
    D = np.max(np.abs(b - a), axis=-1)
    out = np.empty((N, C, model.A))
    out[:, 0] = mid
    if C > 1:
        u = np.random.default_rng(seed).random((N, C - 1, model.A))
        w = 0.5 * 2.0 ** ((np.arange(1, C) - 1) % 3)[None, :, None] * np.maximum(D, 0.5)[:, None, None]
        out[:, 1:] = mid[:, None, :] + (2.0 * u - 1.0) * w
    lo = np.array([j.lower if j.limited else -np.inf for j in model.joints]).astype(np.float32)
    hi = np.array([j.upper if j.limited else np.inf for j in model.joints]).astype(np.float32)
    return np.minimum(np.maximum(out.astype(np.float32), lo), hi)


def path_samples(lengths, resolution: float) -> int:
    """S for legs of the given max-norm lengths: the smallest multiple of 64 whose sample step is <= resolution on the longest of
    them — L / (S / 2 - 1), the coarser of the two legs' steps — capped at PATH_SAMPLES_MAX (the step is then what it is)."""
    longest = float(np.max(lengths)) if np.size(lengths) else 0.0
    for S in range(PATH_SAMPLES_MIN, PATH_SAMPLES_MAX, 64):
        if longest / (S // 2 - 1) <= resolution:
            return S
    return PATH_SAMPLES_MAX


def path_chunks(leg_lengths, candidates: int, resolution: float, budget: int = PATH_CHUNK) -> List[Tuple[int, int, int]]:
    """[(first query, queries, S)]: consecutive queries share a chunk, and its S = path_samples of all its legs
    (leg_lengths[N][C][2]), as long as queries x candidates x S stays within `budget` candidate-samples; a chunk holds at least
    one query."""
    longest = np.max(np.asarray(leg_lengths, float).reshape(len(leg_lengths), -1), axis=1)
    out, first, N = [], 0, len(longest)
    while first < N:
        n, S = 1, path_samples(longest[first], resolution)
        while first + n < N:
            S2 = max(S, path_samples(longest[first + n], resolution))
            if (n + 1) * candidates * S2 > budget:
                break
            n, S = n + 1, S2
        out.append((first, n, S))
        first += n
    return out


def select_joint_path(records) -> Tuple[np.ndarray, np.ndarray]:
    """(outcome[N] str, candidate[N] int) from records[N][C][PATH_FLOATS]. A candidate is free iff [4] == 0; the free candidate
    with the smallest length [5] wins, ties to the lowest c (candidate 0, the straight line, whenever it is free). 'start': candidate 0's [3] == 0, the start pose itself is blocked;
    'goal': [7] == 1, the goal pose is; 'straight': candidate 0 wins; 'via': a candidate c >= 1 does; 'blocked': none is free.
    start before goal before the rest; candidate is -1 wherever no path is returned. Every comparison is made on the values as
    given, so the device's float32 records and the twin's are chosen from by the same rule."""
    rec = np.asarray(records)
    free = rec[..., 4] == 0
    length = np.where(free, rec[..., 5].astype(np.float64), np.inf)
    # No polyline is shorter than the straight line (the triangle inequality), and in the max-norm many are exactly as long; the
    # float32 sum L1 + L2 may then come out an ulp below candidate 0's. A free candidate 0 wins: the rule in exact arithmetic.
    length[..., 0] = np.where(free[..., 0], -np.inf, np.inf)
    best = np.argmin(length, axis=-1)                        # (the first of equal minima: ties to the lowest c)
    found = free.any(axis=-1)
    outcome = np.where(found, np.where(best == 0, "straight", "via"), "blocked").astype("<U8")
    outcome = np.where(rec[..., 0, 7] == 1, "goal", outcome)
    outcome = np.where(rec[..., 0, 3] == 0, "start", outcome)
    return outcome, np.where((outcome == "straight") | (outcome == "via"), best, -1)


class _JointPathFields(NamedTuple):
    """the sixteen members of JointPaths' tuple"""
    outcome: np.ndarray                 # [N] str: 'straight' | 'via' | 'blocked' | 'start' | 'goal' (select_joint_path); with
                                        # certify 'straight' and 'via' name a certified path, and 'sampled' one that is free at
                                        # its samples only (select_certified_path); with roadmap 'roadmap' names a polyline
                                        # over the query's roadmap (roadmap_search)
    candidate: np.ndarray               # [N] int: the chosen candidate, 0 = the straight line; -1: no free path
    via: np.ndarray                     # [N][A]: its via pose, entry m = involved_joints[m]; NaN: no free path
    length: np.ndarray                  # [N]: its length L1 + L2 in the joints' max-norm ('straight': straight_length); NaN: none
    straight_length: np.ndarray         # [N]: max_m |goal_m - start_m|, what GoalPoses.joint_distance reports
    min_clearance: np.ndarray           # [N]: least obstacle clearance over the samples of the chosen path; of the straight line
    min_self_clearance: np.ndarray      # [N]: ... self-clearance, +inf without pairs         for 'blocked', 'start' and 'goal'
    min_cell_clearance: np.ndarray      # [N]: ... workcell clearance, +inf without a workcell
    straight_first_blocked: np.ndarray  # [N] int: the first blocked sample of the straight line, -1: it is free
    sample_step: np.ndarray             # [N]: the largest max-norm distance between neighbouring samples of the reported path
    samples: np.ndarray                 # [N] int: S, the samples per candidate path of the query's chunk
    start: Optional[np.ndarray] = None  # [N][A]: the queries' start and goal poses, as checked (waypoints() needs them)
    goal: Optional[np.ndarray] = None
    # filled by certify; without it nothing is certified: all False, NaN and 0
    certified: Optional[np.ndarray] = None        # [N] bool: the reported path is certified at `samples`
    certified_slack: Optional[np.ndarray] = None  # [N]: the least of its three slacks (the straight line's where no path is
                                                  # reported); certified iff >= margin
    refinements: Optional[np.ndarray] = None      # [N] int: how often the query's samples were doubled



class JointPaths(_JointPathFields):
    """Collision-checked joint paths of N queries (ManipulatorFramework.plan_joint_paths). Without `certify` the check is SAMPLED: a
    free verdict holds at the `samples` poses of the path, `sample_step` apart in the joints' max-norm, and nothing certifies the
    path between them. With `certify` the last three fields are filled: where `certified`, no pose of the polyline, between the
    samples included, brings a capsule closer than the margin to anything the samples are tested against (certify_joint_path).
    With `roadmap` the three attributes below are filled too, and the outcome 'roadmap' names a polyline over the query's roadmap
    (roadmap_search): its candidate is -1 and its via NaN, so whatever reads start -> via -> goal sees a query without such a path;
    length, the three minima, sample_step and samples are its edges'. They are attributes behind the tuple, not members of it: the
    tuple's sixteen fields are what they were, and every loop over them runs as before. _replace keeps them."""
    nodes: Optional[np.ndarray] = None               # [N][K][A]: the polyline start .. goal of a 'roadmap' query, NaN-padded; K is
                                                     # the largest node count of the call
    n_nodes: Optional[np.ndarray] = None             # [N] int: its node count, 0 where there is no roadmap path
    roadmap_free_edges: Optional[np.ndarray] = None  # [N] int: how many of the roadmap's E edges were free; -1: no roadmap was built
    roadmap_length: Optional[np.ndarray] = None      # with shortcut (polyline.shortcut_round; nodes, n_nodes, length and the rest are
                                                     # then the shortened polyline's): [N] the 'roadmap' length before the round; NaN: none
    shortcut_free_edges: Optional[np.ndarray] = None  # [N] int: how many of the round's all-pairs edges were free; -1: no round ran

    def _replace(self, **kw):
        out = super()._replace(**kw)
        out.__dict__.update(self.__dict__)               # the attributes behind the tuple, those that are set
        return out

    def waypoints(self, n: int) -> np.ndarray:
        """[N][n][A]: n >= 2 poses along each query's path, start and goal included, uniform in the path's length (max-norm):
        the first leg takes the share L1 / (L1 + L2) of them, and an edge of a 'roadmap' polyline its length's share likewise.
        Resampled on the host, not the checked samples. NaN rows where there is no free path."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 2:
            raise ValueError(f"waypoints(n): n is a number of poses, at least 2: got {n!r}")
        a, b, via = np.asarray(self.start, float), np.asarray(self.goal, float), np.asarray(self.via, float)
        l1, l2 = np.max(np.abs(via - a), axis=-1), np.max(np.abs(b - via), axis=-1)
        total = l1 + l2
        with np.errstate(divide="ignore", invalid="ignore"):
            split = np.where(total > 0.0, l1 / np.where(total > 0.0, total, 1.0), 0.5)[:, None]
            t = np.linspace(0.0, 1.0, n)[None, :]
            f1 = np.where(split > 0.0, t / np.where(split > 0.0, split, 1.0), 1.0)
            f2 = np.where(split < 1.0, (t - split) / np.where(split < 1.0, 1.0 - split, 1.0), 0.0)
        first = (t < split)[..., None]
        leg1 = a[:, None, :] + f1[..., None] * (via - a)[:, None, :]
        leg2 = np.where((f2 >= 1.0)[..., None], b[:, None, :], via[:, None, :] + f2[..., None] * (b - via)[:, None, :])
        out = np.where(first, leg1, leg2)
        out = np.where((np.asarray(self.candidate) >= 0)[:, None, None], out, np.nan)
        for q in np.nonzero(np.asarray(self.n_nodes) >= 2)[0] if self.n_nodes is not None else ():
            out[q] = polyline_waypoints(np.asarray(self.nodes, float)[q, :int(self.n_nodes[q])], n)
        return out


def _gather_paths(rec, vias, q_start, q_goal, samples, outcome, cand) -> Tuple[list, np.ndarray]:
    """JointPaths' first thirteen fields for the choice (outcome[N], cand[N]) among records[N][C][>= PATH_FLOATS], and each query's
    chosen record (candidate 0's where none is chosen)"""
    has = cand >= 0
    pick = np.maximum(cand, 0)[:, None]
    row = np.take_along_axis(rec, pick[:, :, None], axis=1)[:, 0]
    straight = joint_distance32(q_goal, q_start)
    length = np.where(has, np.where(cand == 0, straight, row[:, 5]), np.nan).astype(rec.dtype)
    via = np.where(has[:, None], np.take_along_axis(np.asarray(vias), pick[:, :, None], axis=1)[:, 0], np.nan)
    return [outcome, cand, via, length, straight.astype(rec.dtype), row[:, 0].copy(), row[:, 1].copy(), row[:, 2].copy(),
            rec[:, 0, 3].astype(np.int64), row[:, 6].copy(), np.asarray(samples, np.int64), np.array(q_start), np.array(q_goal)], row


def gather_joint_paths(records, vias, q_start, q_goal, samples) -> JointPaths:
    """JointPaths from the records[N][C][PATH_FLOATS] of the vias[N][C][A] between q_start[N][A] and q_goal[N][A], and S per query"""
    rec = np.asarray(records)
    fields, _ = _gather_paths(rec, vias, q_start, q_goal, samples, *select_joint_path(rec))
    return JointPaths(*fields, np.zeros(len(rec), bool), np.full(len(rec), np.nan, rec.dtype), np.zeros(len(rec), np.int64))


def path_leg_lengths(vias, q_start, q_goal) -> np.ndarray:
    """[N][C][2]: joint_distance32 of both legs of every candidate"""
    vias = np.asarray(vias, np.float32)
    a, b = np.asarray(q_start, np.float32)[:, None, :], np.asarray(q_goal, np.float32)[:, None, :]
    return np.stack([joint_distance32(vias, a), joint_distance32(b, vias)], axis=-1)


def joint_paths_host(twin: KinematicEnvironment, q_start, q_goal, obstacles, candidates: int = 16, resolution: float = 0.02,
                     margin: float = 0.0, seed: int = 0, chunk: int = PATH_CHUNK, certify: bool = False, roadmap: int = 0,
                     shortcut: int = 0) -> JointPaths:
    """plan_joint_paths through the twin alone, under the device's rule and on the values the device is given: start and goal
    poses, vias and obstacles rounded to float32, the poses and the clearances in float64, the lengths in float32. Chunks and
    their S are the device's (path_chunks). certify: certify_joint_path's records and the device's rounds (certify_rounds).
    roadmap = M > 0: the 'blocked' queries get a roadmap of M milestones (roadmap_round: the device's chunks and S, check_joint_edge's
    records); roadmap edges are checked at their samples only, so not together with certify. shortcut = W > 0 (with roadmap): the
    'roadmap' polylines are searched again over W nodes of their own (polyline.shortcut_round)."""
    return plan_paths(_TwinPaths(twin), q_start, q_goal, obstacles, candidates, resolution, margin, seed, chunk, certify, roadmap, shortcut)


def plan_paths(backend, q_start, q_goal, obstacles, candidates: int = 16, resolution: float = 0.02, margin: float = 0.0, seed: int = 0,
               budget: int = PATH_CHUNK, certify: bool = False, roadmap: int = 0, shortcut: int = 0) -> JointPaths:
    """The one orchestration of collision-checked joint paths, run by the device (chain_tools.JointPathChecker.check) and by the
    twin (joint_paths_host) alike: the refusals, the vias, then either the refinement rounds of certify (certify_rounds) or the
    one-via chunks (path_chunks) and, with roadmap = M > 0, the roadmap round over the queries they left 'blocked' (roadmap_round)
    and, with shortcut = W > 0 behind it, the shortcut round over the 'roadmap' polylines (polyline.shortcut_round; the same evaluator).
    Chunks, their S and the choice among the records are the same for both; what differs is the backend, an object with
      dtype, prefix, roadmap_certify_refusal : the records' dtype and the words of its refusals
      chain                                  : the ChainModel
      prepare(q_start, q_goal, obstacles, C) : the queries as the backend takes them, [N][A], [N][A], [N][3]
      path_records / certified_records (q_start[n], q_goal[n], obstacles[n], vias[n][C], S, margin) : records[n][C][PATH_FLOATS] /
                                               [n][C][PATH_CERT_FLOATS] of one chunk of whole queries at S samples
      edge_records(nodes[n][V][A], edges[E][2], obstacles[n], S, margin) : records[n][E][EDGE_FLOATS] of one chunk of roadmaps
    A backend with a budget of its own refuses in its evaluators what exceeds it."""
    if not roadmap_size_ok(roadmap):
        raise ValueError(f"{backend.prefix}roadmap is a number of milestones from 0 to {ROADMAP_MAX}: got {roadmap!r}")
    if roadmap and certify:
        raise ValueError(backend.prefix + backend.roadmap_certify_refusal)
    check_shortcut(backend.prefix, shortcut, roadmap)
    C = int(candidates)
    q_start, q_goal, obstacles = backend.prepare(q_start, q_goal, obstacles, C)
    vias = path_vias(backend.chain, q_start, q_goal, C, seed)
    legs = path_leg_lengths(vias, q_start, q_goal)
    if certify:
        def run(idx, S):
            return backend.certified_records(q_start[idx], q_goal[idx], obstacles[idx], vias[idx], S, margin)

        records, samples, refinements = certify_rounds(run, legs, C, resolution, budget, backend.dtype)
        return gather_certified_paths(records, vias, q_start, q_goal, samples, refinements)
    records, samples = np.empty((len(legs), C, PATH_FLOATS), backend.dtype), np.empty(len(legs), np.int64)
    for first, n, S in path_chunks(legs, C, resolution, budget):
        sl = slice(first, first + n)
        records[sl], samples[sl] = backend.path_records(q_start[sl], q_goal[sl], obstacles[sl], vias[sl], S, margin), S
    base = gather_joint_paths(records, vias, q_start, q_goal, samples)
    if not roadmap:
        return base

    def run(queries, nodes, edges, S):
        return backend.edge_records(nodes, edges, obstacles[queries], S, margin)

    return shortcut_round(roadmap_round(base, backend.chain, int(roadmap), seed, resolution, budget, run, backend.dtype), int(shortcut),
                          resolution, budget, run, backend.dtype)


class _TwinPaths:
    """plan_paths' backend through the twin alone: the poses and the clearances in float64 on the values the device is given, a few
    queries (or edges) at a time — the twin holds every sample's segments at once, 65536 samples here. It has no budget and refuses
    nothing."""
    dtype, prefix = np.float64, ""
    roadmap_certify_refusal = "roadmap edges are checked at their samples only: roadmap > 0 does not go with certify=True"

    def __init__(self, twin: KinematicEnvironment):
        self.twin, self.chain = twin, twin.model

    def prepare(self, q_start, q_goal, obstacles, C: int):
        r32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)      # noqa: E731
        return r32(q_start), r32(q_goal), r32(obstacles)

    def _records(self, rule, floats, q_start, q_goal, obstacles, vias, S, margin) -> np.ndarray:
        n, C = vias.shape[:2]
        out = np.empty((n, C, floats))
        block = max(1, 65536 // (C * S))
        for k in range(0, n, block):
            sl = slice(k, k + block)
            out[sl] = rule(self.twin, q_start[sl, None, :], vias[sl].astype(np.float64), q_goal[sl, None, :], obstacles[sl, None, :],
                           S, margin)
        return out

    def path_records(self, *chunk) -> np.ndarray:
        return self._records(check_joint_path, PATH_FLOATS, *chunk)

    def certified_records(self, *chunk) -> np.ndarray:
        return self._records(certify_joint_path, PATH_CERT_FLOATS, *chunk)

    def edge_records(self, nodes, edges, obstacles, S, margin) -> np.ndarray:
        nodes = nodes.astype(np.float64)
        out = np.empty((len(nodes), len(edges), EDGE_FLOATS))
        block = max(1, 65536 // S)
        for n in range(len(nodes)):
            for k in range(0, len(edges), block):
                e = edges[k:k + block]
                out[n, k:k + block] = check_joint_edge(self.twin, nodes[n, e[:, 0]], nodes[n, e[:, 1]], obstacles[n], S, margin)
        return out


# ---- roadmaps: several straight edges where one via is blocked (include/naf_hip.h, "Roadmap edges") --------------------------------
ROADMAP_MAX = 62                      # milestones per query: V = M + 2 nodes, at most 64
EDGE_FLOATS = 8                       # NAF_CHAIN_EDGE_FLOATS
ROADMAP_STREAM = 0x726F6164           # what the milestones' Generator is seeded with beside `seed`: not path_vias' draws again


def roadmap_size_ok(M) -> bool:
    return isinstance(M, (int, np.integer)) and not isinstance(M, bool) and 0 <= M <= ROADMAP_MAX


def roadmap_milestones(model: ChainModel, q_start, q_goal, M: int, seed: int) -> np.ndarray:
    """[N][M][A] float32: the milestones of every query's roadmap, from the poses as float32 holds them and ONE
    np.random.default_rng([seed, ROADMAP_STREAM]).random((N, M, A)) call — drawn for all N queries of the call, whichever of them
    get a roadmap, so that a query's milestones do not depend on the others' outcomes. The first ceil(M / 2) are "near": path_vias'
    rule, mid + (2u - 1) w_k with w_k = 0.5 2^(k mod 3) max(D, 0.5) around the midpoint of the straight line. The rest are uniform
    inside the limits, lo + u (hi - lo), +-pi for a revolute joint without limits. Clipped into the limits of limited joints as the
    device holds them. A prismatic joint without limits has no range to draw from and is refused by name."""
    for m, j in enumerate(model.joints):
        if j.type == PRISMATIC and not j.limited:
            raise ValueError(f"roadmap_milestones: joint {m} (involved_joints[{m}]) is a prismatic joint without limits: there is no "
                             f"range to draw its milestones from")
    a = np.asarray(q_start, np.float32).astype(np.float64).reshape(-1, model.A)
    b = np.asarray(q_goal, np.float32).astype(np.float64).reshape(-1, model.A)
    N, M = len(a), int(M)
    near = (M + 1) // 2
    u = np.random.default_rng([int(seed), ROADMAP_STREAM]).random((N, M, model.A))
    out = np.empty((N, M, model.A))
    mid, D = 0.5 * (a + b), np.max(np.abs(b - a), axis=-1)
    w = 0.5 * 2.0 ** (np.arange(near) % 3)[None, :, None] * np.maximum(D, 0.5)[:, None, None]
    out[:, :near] = mid[:, None, :] + (2.0 * u[:, :near] - 1.0) * w
    lo = np.array([j.lower if j.limited else -np.pi for j in model.joints])
    hi = np.array([j.upper if j.limited else np.pi for j in model.joints])
    out[:, near:] = lo + u[:, near:] * (hi - lo)
    lo32 = np.array([j.lower if j.limited else -np.inf for j in model.joints]).astype(np.float32)
    hi32 = np.array([j.upper if j.limited else np.inf for j in model.joints]).astype(np.float32)
    return np.minimum(np.maximum(out.astype(np.float32), lo32), hi32)


def edge_pose(a, b, i, S: int) -> np.ndarray:
    """Sample i of the S poses of the straight joint-space edge a -> b, in float64; a, b [..., A] and i [...] broadcast. Sample i
    lies at f = i / (S - 1), both ends included: q_m = a_m + f (b_m - a_m), and b itself at f = 1. No limits are applied and
    nothing wraps."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    f = (np.asarray(i) / (int(S) - 1))[..., None]
    return np.where(f == 1.0, b, a + f * (b - a))


def check_joint_edge(twin: KinematicEnvironment, a, b, obstacle, S: int, margin: float = 0.0) -> np.ndarray:
    """[..., EDGE_FLOATS] float64: the record of the edges a[..., A] -> b[..., A] in the scenes obstacle[..., 3] (all broadcast),
    sampled at the S poses of edge_pose: [0] [1] [2] the minima over the samples of the obstacle clearance (the obstacle radius
    subtracted), the self-clearance and the workcell clearance (+inf where the model has none) | [3] the index of the first
    blocked sample, -1: none | [4] how many are blocked | [5] L = joint_distance32(b, a), in float32 | [6] the sample step
    L / (S - 1), in float32 | [7] 0. A sample is blocked iff one of its three clearances is < margin. SAMPLED, as check_joint_path."""
    if not path_samples_ok(S):
        raise ValueError(f"S is a multiple of 64 from {PATH_SAMPLES_MIN} to {PATH_SAMPLES_MAX}: got {S!r}")
    a, b = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float))
    lead = a.shape[:-1]
    obstacle = np.broadcast_to(np.asarray(obstacle, float), lead + (3,))
    q = edge_pose(a[..., None, :], b[..., None, :], np.arange(S), S)
    clear = twin.clearance(q, obstacle[..., None, :]) - twin.obstacle_radius
    self_clear, cell_clear = twin.self_clearance(q) + np.zeros(clear.shape), twin.cell_clearance(q) + np.zeros(clear.shape)
    blocked = (clear < margin) | (self_clear < margin) | (cell_clear < margin)
    length = joint_distance32(b, a)
    out = np.empty(lead + (EDGE_FLOATS,))
    out[..., 0], out[..., 1], out[..., 2] = clear.min(axis=-1), self_clear.min(axis=-1), cell_clear.min(axis=-1)
    out[..., 3] = np.where(blocked.any(axis=-1), np.argmax(blocked, axis=-1), -1)
    out[..., 4] = blocked.sum(axis=-1)
    out[..., 5] = length
    out[..., 6] = length / np.float32(S - 1)
    out[..., 7] = 0.0
    return out


def roadmap_edges(V: int) -> np.ndarray:
    """[E][2] int32, E = V (V - 1) / 2: every pair i < j of the V nodes in np.triu_indices(V, 1) order; edge 0 = (0, 1) is the
    straight line start -> goal"""
    return np.stack(np.triu_indices(int(V), 1), axis=1).astype(np.int32)


def edge_samples(lengths, resolution: float) -> int:
    """S for edges of the given max-norm lengths: the smallest multiple of 64 whose sample step L / (S - 1) is <= resolution on the
    longest of them, capped at PATH_SAMPLES_MAX (the step is then what it is)."""
    longest = float(np.max(lengths)) if np.size(lengths) else 0.0
    for S in range(PATH_SAMPLES_MIN, PATH_SAMPLES_MAX, 64):
        if longest / (S - 1) <= resolution:
            return S
    return PATH_SAMPLES_MAX


def roadmap_chunks(edge_lengths, resolution: float, budget: int = PATH_CHUNK) -> List[Tuple[int, int, int]]:
    """[(first query, queries, S)] over edge_lengths[N][E]: path_chunks' rule with edge_samples — consecutive queries share a
    chunk and its S while queries x E x S stays within `budget` edge-samples; a chunk holds at least one query."""
    lengths = np.asarray(edge_lengths, float).reshape(len(edge_lengths), -1)
    longest, E = np.max(lengths, axis=1), lengths.shape[1]
    out, first, N = [], 0, len(longest)
    while first < N:
        n, S = 1, edge_samples(longest[first], resolution)
        while first + n < N:
            S2 = max(S, edge_samples(longest[first + n], resolution))
            if (n + 1) * E * S2 > budget:
                break
            n, S = n + 1, S2
        out.append((first, n, S))
        first += n
    return out


def roadmap_nodes(q_start, q_goal, milestones) -> np.ndarray:
    """[N][M + 2][A] float32: node 0 the start pose, node 1 the goal pose, nodes 2 .. the milestones"""
    a, b = np.asarray(q_start, np.float32), np.asarray(q_goal, np.float32)
    return np.concatenate([a[:, None, :], b[:, None, :], np.asarray(milestones, np.float32)], axis=1)


def roadmap_edge_lengths(nodes, edges) -> np.ndarray:
    """[N][E] float32: joint_distance32 of every edge of every query's nodes[N][V][A]"""
    nodes, edges = np.asarray(nodes, np.float32), np.asarray(edges)
    return joint_distance32(nodes[:, edges[:, 1]], nodes[:, edges[:, 0]])


def roadmap_search(records, edges, V: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(n_nodes[N] int, node_index[N][V] int, length[N] float32) from records[N][E][EDGE_FLOATS] of the edges[E][2] over V nodes:
    the shortest path from node 0 to node 1 over the usable edges. An edge is usable iff [4] == 0; its weight is [5] as float32,
    the same in both directions. Bellman-Ford in Jacobi rounds in float32: d = 0 at node 0 and +inf elsewhere; a round forms
    d[i] + w[i][j] for all i from the PREVIOUS round's d, the lowest i among equal minima is the predecessor, and a node changes
    only on a strict improvement; the rounds end when nothing changes, after at most V - 1. The path is read back from node 1 along
    the predecessors: node_index holds it from 0 to 1, -1 behind it, n_nodes its node count (0: node 1 was not reached) and length
    the float32 sum of its edges' weights in path order from node 0 (NaN: none). No polyline is shorter than a free straight line
    (the triangle inequality), and in the max-norm many are exactly as long, so that a float32 sum may come out an ulp below it: a
    usable edge (0, 1) wins outright, select_joint_path's refinement. Every comparison is made on the values as given, so the
    device's float32 records and the twin's are searched by the same rule."""
    rec, edges, V = np.asarray(records), np.asarray(edges, np.int64).reshape(-1, 2), int(V)
    N = len(rec)
    if edges.size and not (np.all(edges[:, 0] >= 0) and np.all(edges[:, 0] < edges[:, 1]) and np.all(edges[:, 1] < V)):
        raise ValueError(f"roadmap_search: every edge is (i, j) with 0 <= i < j < {V}")
    inf = np.float32(np.inf)
    w = np.full((N, V, V), inf, np.float32)
    weight = np.where(rec[..., 4] == 0, rec[..., 5].astype(np.float32), inf)
    w[:, edges[:, 0], edges[:, 1]] = weight
    w[:, edges[:, 1], edges[:, 0]] = weight
    d = np.full((N, V), inf, np.float32)
    d[:, 0] = 0.0
    pred = np.full((N, V), -1, np.int64)
    for _ in range(V - 1):
        through = d[:, :, None] + w                          # [n][i][j], float32
        best, arg = through.min(axis=1), through.argmin(axis=1)      # (argmin: the first of equal minima, the lowest i)
        better = best < d
        if not better.any():
            break
        d, pred = np.where(better, best, d), np.where(better, arg, pred)
    straight = np.zeros(N, bool)
    for e in np.nonzero((edges[:, 0] == 0) & (edges[:, 1] == 1))[0]:
        straight |= np.isfinite(weight[:, e])
    n_nodes, index, length = np.zeros(N, np.int64), np.full((N, V), -1, np.int64), np.full(N, np.nan, np.float32)
    for n in np.nonzero(np.isfinite(d[:, 1]))[0]:
        back = [1]
        while back[-1] != 0 and len(back) <= V:
            back.append(0 if straight[n] else int(pred[n, back[-1]]))
        assert back[-1] == 0, "roadmap_search: the predecessors do not lead back to node 0"
        path = back[::-1]
        total = np.float32(0.0)
        for i, j in zip(path[:-1], path[1:]):
            total = np.float32(total + w[n, i, j])
        n_nodes[n], index[n, :len(path)], length[n] = len(path), path, total
    return n_nodes, index, length


def polyline_waypoints(nodes, n: int) -> np.ndarray:
    """[n][A]: n poses along the polyline nodes[K][A], uniform in its max-norm length, both ends included (the end pose itself at
    the end of the last edge)"""
    nodes = np.asarray(nodes, float)
    legs = np.max(np.abs(np.diff(nodes, axis=0)), axis=1)
    ends = np.cumsum(legs)
    total = ends[-1]
    out = np.empty((n, nodes.shape[1]))
    for k, t in enumerate(np.linspace(0.0, 1.0, n)):
        s = t * total
        e = min(int(np.searchsorted(ends, s, side="left")), len(legs) - 1)
        f = (s - (ends[e] - legs[e])) / legs[e] if legs[e] > 0.0 else 1.0
        out[k] = nodes[e + 1] if f >= 1.0 else nodes[e] + f * (nodes[e + 1] - nodes[e])
    out[0], out[-1] = nodes[0], nodes[-1]
    return out


def gather_roadmap_paths(base: JointPaths, blocked, records, nodes, edges, samples) -> JointPaths:
    """`base` (the one-via round's JointPaths of N queries) with the roadmaps of its queries blocked[Nb] (indices) filled in:
    records[Nb][E][EDGE_FLOATS] of the edges[E][2] between nodes[Nb][V][A], samples[Nb] their S. A query with a path over its
    usable edges becomes 'roadmap': candidate -1 and via NaN as before, length the float32 sum of its edges, the three minima the
    minima over its edges' records, sample_step the largest [6] among them, samples their S. The others stay as they are. Sets
    nodes, n_nodes and roadmap_free_edges."""
    blocked, rec, nodes = np.asarray(blocked, np.int64), np.asarray(records), np.asarray(nodes)
    N, A, V = len(base.outcome), np.asarray(base.start).shape[1], nodes.shape[1] if nodes.ndim == 3 else 2
    n_nodes, free_edges = np.zeros(N, np.int64), np.full(N, -1, np.int64)
    fields = {name: np.array(getattr(base, name)) for name in ("outcome", "length", "min_clearance", "min_self_clearance",
                                                               "min_cell_clearance", "sample_step", "samples")}
    polylines = {}
    if len(blocked):
        count, index, length = roadmap_search(rec, edges, V)
        edge_of = {(int(i), int(j)): e for e, (i, j) in enumerate(np.asarray(edges))}
        free_edges[blocked] = np.sum(rec[..., 4] == 0, axis=1)
        for k in np.nonzero(count > 0)[0]:
            q, path = blocked[k], index[k, :count[k]]
            rows = rec[k, [edge_of[(min(i, j), max(i, j))] for i, j in zip(path[:-1], path[1:])]]
            n_nodes[q], polylines[q] = count[k], nodes[k, path]
            fields["outcome"][q], fields["length"][q], fields["samples"][q] = "roadmap", length[k], samples[k]
            fields["min_clearance"][q], fields["min_self_clearance"][q] = rows[:, 0].min(), rows[:, 1].min()
            fields["min_cell_clearance"][q], fields["sample_step"][q] = rows[:, 2].min(), rows[:, 6].max()
    out = base._replace(**fields)
    K = int(n_nodes.max()) if N else 0
    out.nodes = np.full((N, K, A), np.nan, np.asarray(base.start).dtype)
    for q, poly in polylines.items():
        out.nodes[q, :len(poly)] = poly
    out.n_nodes, out.roadmap_free_edges = n_nodes, free_edges
    return out


def roadmap_round(base: JointPaths, model: ChainModel, M: int, seed: int, resolution: float, budget: int, run, dtype) -> JointPaths:
    """The roadmap round behind the one-via round's `base`, on the device and through the twin alike: the milestones of all N
    queries, the nodes of the blocked ones, their chunks (roadmap_chunks) and run(queries[n], nodes[n][V][A] float32, edges, S) ->
    records[n][E][EDGE_FLOATS] per chunk (queries: the chunk's indices into the call's N), then gather_roadmap_paths."""
    blocked = np.nonzero(np.asarray(base.outcome) == "blocked")[0]
    V = int(M) + 2
    edges = roadmap_edges(V)
    nodes = roadmap_nodes(base.start, base.goal, roadmap_milestones(model, base.start, base.goal, M, seed))[blocked]
    records, samples = np.empty((len(blocked), len(edges), EDGE_FLOATS), dtype), np.zeros(len(blocked), np.int64)
    for first, n, S in roadmap_chunks(roadmap_edge_lengths(nodes, edges), resolution, budget) if len(blocked) else ():
        records[first:first + n], samples[first:first + n] = run(blocked[first:first + n], nodes[first:first + n], edges, S), S
    return gather_roadmap_paths(base, blocked, records, nodes, edges, samples)


# ---- demonstrations: planned joint paths as replay rows (include/naf_hip.h, "Demonstrations") --------------------------------------
DEMO_FLOATS = 8                       # NAF_CHAIN_DEMO_FLOATS
DEMO_MAX_TICKS = 1024                 # NAF_CHAIN_DEMO_MAX_TICKS
DEMO_CHUNK = 1 << 19                  # rows per chunk of a DemonstrationWriter (128 MiB of 64-float rows)
DEMO_END_CODES = ("frames", "reached", "obstacle", "self", "workcell", "end")      # by end code: records_out[n][1]
DEMO_KEPT = ("reached", "frames", "end")


class DemonstrationPlan(NamedTuple):
    """The time parametrisation of N paths start -> via -> goal (demonstration_plan): all the kernel sees of them."""
    q_start: np.ndarray               # [N][A] float32: the start poses
    leg_actions: np.ndarray           # [N][2][A] float32: the constant action of each leg ([N][K][A] of demonstration_plan_legs)
    n_ticks: np.ndarray               # [N][2] int32: ticks per leg, each >= 1 ([N][K]: 0 for the padding behind a query's last leg)
    rows: np.ndarray                  # [N] int: T_n = min(sum of the ticks, frames)


class Demonstrations(NamedTuple):
    """Planned joint paths as replay rows (ManipulatorFramework.demonstrate_joint_paths): the episodes the environment's own step
    rule produces when the arm is driven along each path open loop."""
    outcome: np.ndarray               # [N] str: 'reached' | 'frames' | 'end' (the path ended short of 0.05 from the target) |
                                      # 'obstacle' | 'self' | 'workcell' | 'none' (the query had no path)
    frames: np.ndarray                # [N] int: rows of the demonstration, up to and including the first done; 0 for 'none'
    final_distance: np.ndarray        # [N]: |ee - target| after its last row; NaN for 'none'
    min_clearance: np.ndarray         # [N]: minima over its rows of the obstacle clearance (radius subtracted),
    min_self_clearance: np.ndarray    # [N]: ... the self-clearance (+inf without pairs)
    min_cell_clearance: np.ndarray    # [N]: ... and the workcell clearance (+inf without a workcell)
    planned_ticks: np.ndarray         # [N] int: n1 + n2; 0 for 'none'
    kept: np.ndarray                  # [N] bool: its rows are in `rows`
    rows: object                      # [rows_total][row_floats] float32, query order then tick order: a device tensor, or numpy
                                      # through the twin
    rows_total: int
    action_size: int = 0              # A of the arm the rows belong to
    tracking_error: Optional[np.ndarray] = None      # [N]: the last three from demonstrate_trajectories only: max |p_i - Q_i| of the host's
    saturated_ticks: Optional[np.ndarray] = None     # float32 recurrence against the law | ticks with a component clamped to [-1, 1] |
    peak_action: Optional[np.ndarray] = None         # the largest |a_i|


def demonstration_speed_ok(speed) -> bool:
    return isinstance(speed, (int, float, np.integer, np.floating)) and not isinstance(speed, bool) and 0.0 < float(speed) <= 1.0


def demonstration_plan(q_start, via, q_goal, speed: float = 1.0, frames: int = 400) -> DemonstrationPlan:
    """q_start, via, q_goal [N][A] (taken as float32 holds them) -> the plan: polyline.demonstration_plan_legs of the three nodes
    start, via, goal. Leg k of length L_k = joint_distance32 takes n_k = max(1, ceil(L_k / (speed DT))) ticks (float64) at the
    constant action (b - a) / (n_k DT), formed in float64 from the float32 end poses and rounded to float32; |a|_inf <= speed (a leg
    whose rounded action would exceed it gets one tick more). A leg of length 0 is one tick at action 0
    (polyline.leg_ticks_and_action, where the per-leg rule is written once)."""
    a = np.asarray(q_start, np.float32)
    a = a.reshape(-1, a.shape[-1])
    v, b = np.asarray(via, np.float32).reshape(a.shape), np.asarray(q_goal, np.float32).reshape(a.shape)
    return demonstration_plan_legs(np.stack([a, v, b], axis=1), np.full(len(a), 3), speed, frames)


def demo_row_layout(A: int) -> Tuple[int, int, int, int]:
    """(S, next_state offset, done offset, row floats) of the chain environment's replay row (include/naf_hip.h)"""
    S = 2 * A + 9
    off_s2 = (S + A + 1 + 3) // 4 * 4
    need, rf = off_s2 + S + 1, 32
    while rf < need:
        rf *= 2
    return S, off_s2, off_s2 + S, rf


def demo_observations(twin: KinematicEnvironment, q, qd, target, obstacle) -> np.ndarray:
    """[..., 2A + 9]: get_state() for batches of poses q[..., A], reported velocities qd[..., A] and scenes"""
    q = np.asarray(q, float)
    A = twin.n
    out = np.empty(q.shape[:-1] + (2 * A + 9,))
    for k, (src, const) in enumerate(twin.model.slots):
        out[..., k] = q[..., src] if src >= 0 else const
        out[..., A + k] = qd[..., src] if src >= 0 else 0.0
    out[..., 2 * A:2 * A + 3] = twin.end_effector(q)
    out[..., 2 * A + 3:2 * A + 6] = target
    out[..., 2 * A + 6:] = obstacle
    return out


def gather_demonstrations(records, has_path, kept_rows_of, keep_contact: bool) -> Demonstrations:
    """Demonstrations from records[N][DEMO_FLOATS] (rows of queries without a path are ignored), has_path[N] and the rows that
    kept_rows_of(kept[N], valid[N]) selects — the one place that states keep / drop."""
    rec = np.asarray(records)
    has = np.asarray(has_path, bool)
    code = np.where(has, rec[:, 1], 0).astype(np.int64)
    outcome = np.where(has, np.array(DEMO_END_CODES)[code], "none").astype("<U8")
    kept = has & (np.isin(outcome, DEMO_KEPT) | bool(keep_contact))
    valid = np.where(has, rec[:, 0], 0).astype(np.int64)
    nan = lambda k: np.where(has, rec[:, k], np.nan).astype(rec.dtype)      # noqa: E731
    out_rows = kept_rows_of(kept, valid)
    return Demonstrations(outcome, valid, nan(2), nan(3), nan(4), nan(5), np.where(has, rec[:, 6], 0).astype(np.int64), kept, out_rows,
                          int(np.sum(valid[kept])))


def demonstration_rows_host(twin: KinematicEnvironment, plan: DemonstrationPlan, targets, obstacles, frames: int = 400,
                            keep_contact: bool = False, has_path=None, full: bool = False):
    """naf_chain_demo_rows through the twin alone: KinematicEnvironment.trace — the float64 episode under given actions — from
    the plan's start poses under its actions, cut at T_n = min(n1 + n2, frames); the rows are get_state() before and after every
    step, the velocity slots what the step before reported. `plan` is a DemonstrationPlan, whose actions are demo_actions', or a
    tick_demo.TickPlan with a table of its own (naf_chain_demo_rows_ticks' twin): one body, and record [6] the planned ticks of
    either. Returns Demonstrations with `rows` a float32 numpy array; full=True
    returns (demonstrations, records[N][8] float64, rows[N][T][row floats] float64 with NaN where there is no row, poses[N][T + 1][A])."""
    N, A = plan.q_start.shape
    S, off_s2, off_d, rf = demo_row_layout(A)
    has = np.ones(N, bool) if has_path is None else np.asarray(has_path, bool)
    targets = np.broadcast_to(np.asarray(targets, np.float32).astype(np.float64), (N, 3))
    obstacles = np.broadcast_to(np.asarray(obstacles, np.float32).astype(np.float64), (N, 3))
    from .tick_demo import plan_source
    planned, Tn, T, actions = plan_source(plan, int(frames))
    tr = twin.trace(plan.q_start.astype(np.float64), actions, targets, obstacles, T)
    valid = np.minimum(tr.frames, Tn)
    done = (tr.code != 0) & (tr.frames <= Tn)
    m = np.concatenate([tr.margins, tr.cell_margins[..., None]], axis=-1)                 # [N, T, 4]
    live = np.arange(T)[None, :] < valid[:, None]
    last = np.take_along_axis(m, (valid - 1)[:, None, None], axis=1)[:, 0]
    records = np.zeros((N, DEMO_FLOATS))
    records[:, 0] = valid
    records[:, 1] = np.where(done, tr.code, np.where(Tn < planned, 0, 5))
    records[:, 2] = last[:, 0] + TARGET_THRESHOLD
    for k, col in ((3, 1), (4, 2), (5, 3)):
        records[:, k] = np.min(np.where(live, m[:, :, col], np.inf), axis=1)
    records[:, 6] = planned
    # the rows: state t = obs(p_t) with step t - 1's reported velocities, next_state t = state t + 1
    lo, hi = twin.joint_limits()
    path = tr.joint_positions                                                              # [N, T + 1, A], held behind the end
    pre = path[:, :-1] + DT * actions
    vel = np.where((pre < lo) | (pre > hi), 0.0, actions)
    qd = np.concatenate([np.zeros((N, 1, A)), vel], axis=1)
    obs = demo_observations(twin, path, qd, targets[:, None, :], obstacles[:, None, :])    # [N, T + 1, S]
    # trace's own margin d - 0.05: reached iff it is negative (x - y < 0 iff x < y in IEEE arithmetic), and the shaped reward is its
    # negative, bit for bit step()'s -1 * (d - 0.05) — adding the threshold back and subtracting it again loses the last bit
    reached = m[:, :, 0] < 0.0
    hit = (m[:, :, 1] < 0.0) | (m[:, :, 2] < 0.0) | (m[:, :, 3] < 0.0)
    rows = np.zeros((N, T, rf))
    rows[:, :, :S] = obs[:, :-1]
    rows[:, :, S:S + A] = actions
    with np.errstate(invalid="ignore"):
        rows[:, :, S + A] = np.where(reached, 250.0, np.where(hit, -1000.0, -1 * m[:, :, 0]))
    rows[:, :, off_s2:off_s2 + S] = obs[:, 1:]
    rows[:, :, off_d] = reached | hit
    rows[~live] = np.nan

    def kept_rows(kept, valid_):
        mask = kept[:, None] & (np.arange(T)[None, :] < valid_[:, None])
        return rows[mask].astype(np.float32)
    demos = gather_demonstrations(records, has, kept_rows, keep_contact)._replace(action_size=A)
    return (demos, records, rows, path) if full else demos


def cell_box_gaps(model: ChainModel, centre, half) -> np.ndarray:
    """[G + H + B]: how near the box centre +- half (a point when half is 0) comes to each workcell geometry. Against a half-space
    the box corner with the smallest n.x decides: min over the box of n.x - d = n.centre - |n|.half - d. Against a sphere: the
    distance from its centre to the box (0 inside) minus its radius. Against an oriented box: the closest pair of two disjoint
    boxes has a point on an edge of one of them, so the minimum of segment_box_distance over the 12 edges of each box against the
    other, minus the rounding radius; intersecting boxes give 0 - r."""
    centre, half = np.asarray(centre, float), np.asarray(half, float)
    out = [np.linalg.norm(np.maximum(np.abs(np.array(c[:3]) - centre) - half, 0.0)) - c[3] for c in model.cell_spheres]
    out += [float(np.dot(n[:3], centre) - np.dot(np.abs(n[:3]), half) - n[3]) for n in model.cell_planes]
    for x in model.cell_boxes:
        x = np.array(x)
        c, R, h = x[:3], x[3:12].reshape(3, 3), x[12:15]
        ea, eb = _box_edges(half)                             # the target box's edges, in its own (world-aligned) frame
        d1 = segment_box_distance((ea + centre - c) @ R, (eb + centre - c) @ R, h)
        ea, eb = _box_edges(h)                                # the oriented box's edges, taken to the world, about the target's centre
        d2 = segment_box_distance(ea @ R.T + c - centre, eb @ R.T + c - centre, half)
        out.append(float(min(d1.min(), d2.min())) - x[15])
    return np.array(out, float)


def _box_edges(half: np.ndarray):
    """(a[12, 3], b[12, 3]): the 12 edges of the box |x_i| <= half_i"""
    a, b = [], []
    for axis in range(3):
        for s1 in (-1.0, 1.0):
            for s2 in (-1.0, 1.0):
                p = np.zeros(3)
                p[(axis + 1) % 3], p[(axis + 2) % 3] = s1 * half[(axis + 1) % 3], s2 * half[(axis + 2) % 3]
                lo, hi = p.copy(), p.copy()
                lo[axis], hi[axis] = -half[axis], half[axis]
                a.append(lo)
                b.append(hi)
    return np.array(a), np.array(b)


def reach_queries(model: ChainModel, targets, obstacles, initial_joint_positions, frames, nominal_obstacle=None, nominal_start=None):
    """The arguments of a rollout to given targets, checked and broadcast: (q0[N, A], targets[N, 3], obstacles[N, 3], frames) as
    float64 arrays. targets: [N][3], or [3] for one query. obstacles: [N][3], [3] (every query's) or None (nominal_obstacle).
    initial_joint_positions: [N][A], [A] (every query's) or None (nominal_start, else the model's initial positions); entry m is
    the value of driven joint m, i.e. of involved_joints[m]. ValueError for a wrong shape, a number that is not finite, a joint
    value outside its limits (the message names the joint and the query) or frames < 1."""
    A = model.A
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1:
        raise ValueError(f"frames is a number of steps, at least 1: got {frames!r}")

    def numbers(v, what):
        try:
            out = np.array(v, float)
        except (TypeError, ValueError):
            raise ValueError(f"{what} is not an array of numbers") from None
        if not np.all(np.isfinite(out)):
            raise ValueError(f"{what} holds a number that is not finite")
        return out
    t = numbers(targets, "targets")
    if t.shape == (3,):
        t = t[None]
    if t.ndim != 2 or t.shape[1] != 3 or len(t) == 0:
        raise ValueError(f"targets is [N][3], or [3] for one query: got shape {t.shape}")
    N = len(t)
    if obstacles is None:
        if nominal_obstacle is None:
            raise ValueError("obstacles=None needs the scene's nominal obstacle")
        obstacles = nominal_obstacle
    o = numbers(obstacles, "obstacles")
    if o.shape != (3,) and o.shape != (N, 3):
        raise ValueError(f"obstacles is [N][3] with N = {N}, or [3] for all queries: got shape {o.shape}")
    if initial_joint_positions is None:
        initial_joint_positions = [j.init for j in model.joints] if nominal_start is None else nominal_start
    q = numbers(initial_joint_positions, "initial_joint_positions")
    if q.shape != (A,) and q.shape != (N, A):
        raise ValueError(f"initial_joint_positions is [N][{A}] with N = {N}, or [{A}] for all queries (one value per involved "
                         f"joint): got shape {q.shape}")
    q = np.broadcast_to(q, (N, A))
    for m, j in enumerate(model.joints):
        bad = np.nonzero((q[:, m] < j.lower) | (q[:, m] > j.upper))[0] if j.limited else ()
        if len(bad):
            raise ValueError(f"initial_joint_positions of query {int(bad[0])}: joint {j.index} (involved_joints[{m}]) at "
                             f"{q[bad[0], m]:.6g} is outside its limits [{j.lower:.6g}, {j.upper:.6g}]")
    return q.copy(), t, np.broadcast_to(o, (N, 3)).copy(), int(frames)


def build_kinematic(manipulator_file, endeffector_index, fixed_joints, involved_joints, target_position, obstacle_position,
                    initial_joint_positions=None, initial_positions_variation_range=None, link_radius=0.0,
                    obstacle_radius=OBSTACLE_RADIUS, consider_autocollision=False, autocollision_ignore=None, *, target_range=None,
                    obstacle_range=None, scene_margin=0.02, floor_height=None, workcell_planes=None, workcell_spheres=None,
                    cell_ignore=None, workcell_boxes=None) -> KinematicEnvironment:
    """Picklable factory (HostVectorEnv's worker processes call it through functools.partial)."""
    model = compile_chain(load_urdf(manipulator_file), endeffector_index, involved_joints, fixed_joints,
                          initial_joint_positions, initial_positions_variation_range, link_radius, consider_autocollision,
                          autocollision_ignore or (), floor_height, workcell_planes, workcell_spheres, cell_ignore or (),
                          workcell_boxes)
    return KinematicEnvironment(model, target_position, obstacle_position, obstacle_radius, target_range, obstacle_range,
                                scene_margin)


# polylines of any number of legs and the shortcut round are stated in environment/polyline.py and belong to the rule as these do
from .polyline import (DEMO_MAX_LEGS, SHORTCUT_MAX, SHORTCUT_MIN, check_shortcut, demo_actions, demonstration_plan_legs,  # noqa: E402,F401
                       leg_ticks_and_action, shortcut_nodes, shortcut_round, shortcut_size_ok)
from .path_certificate import (_round_up32, certificate_guard, certify_joint_path, certify_rounds, gather_certified_paths,  # noqa: E402,F401
                               path_half_steps, path_slacks, reach_table, select_certified_path)
from .edge_certificate import (EDGE_CERT_FLOATS, PathCertificates, certify_joint_edge, certify_polylines,  # noqa: E402,F401
                               certify_polylines_host, edge_half_steps, polyline_nodes)

"""KinematicEnvironment: the float64 host twin of csrc/chain_env.hip, behind the reference Environment's protocol
(environment/environment.py: reset(verbose) -> state[S]; step(action) -> (state, reward, done); observation_space /
action_space as zero arrays), exactly as SyntheticEnvironment offers it.

Built from a ChainModel (environment/urdf_chain.py) and evaluated from the MODEL, not from the packed blob, so that a packing
error shows as a disagreement with the kernel. Kinematic: the commanded velocity is applied exactly for one 1/240 s tick
(environment.py:453-485 with an ideal motor). NOT a port of Bullet: no dynamics, no mesh collision, no self-collision.
  state  = [pos(A), vel(A), end-effector xyz, target xyz, obstacle xyz], slot k of pos / vel reporting joint INDEX k
           (environment.py:442-451)
  reward = +250 reached (dist < 0.05) | -1000 contact | -(dist - 0.05), done on either (environment.py:311-371, :416-429)
"""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .urdf_chain import DT, OBSTACLE_RADIUS, PRISMATIC, TARGET_THRESHOLD, ChainModel, axis_rotation, compile_chain, load_urdf


def segment_point_distance2(a: np.ndarray, b: np.ndarray, c: np.ndarray):
    """Squared distance from point c to the segment a-b (projection clamped to [0, 1]); arrays of points [..., 3] broadcast."""
    ab, ac = b - a, c - a
    den = np.sum(ab * ab, axis=-1)
    t = np.clip(np.sum(ac * ab, axis=-1) / np.where(den > 0.0, den, 1.0), 0.0, 1.0)
    d = ac - t[..., None] * ab
    return np.sum(d * d, axis=-1)


class KinematicEnvironment:

    def __init__(self, model: ChainModel, target_position: Sequence[float], obstacle_position: Sequence[float],
                 obstacle_radius: float = OBSTACLE_RADIUS):
        self.model = model
        self.n = model.A
        self.involved_joints = [j.index for j in model.joints]
        self.target_pos = np.array(target_position, float)
        self.obstacle_pos = np.array(obstacle_position, float)
        self.obstacle_radius = float(obstacle_radius)
        self.initial_joint_positions = np.array([j.init for j in model.joints])
        self.initial_positions_variation_range = model.initial_positions_variation_range
        self._observation_space = np.zeros((model.state_size,))
        self._action_space = np.zeros((self.n,))
        self.q = self.initial_joint_positions.copy()          # driven joints, by action index
        self.qd = np.zeros(self.n)
        self.last_distance = float("nan")                     # |ee - target| of the last step
        self.last_clearance = float("nan")                    # min over segments of (distance to the obstacle centre - radius)

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
        (environment.py:284-293); only driven joints vary."""
        self.q = np.array([random.uniform(j.init - j.variation, j.init + j.variation) if j.variation > 0.0 else j.init
                           for j in self.model.joints])
        self.qd = np.zeros(self.n)
        return self.get_state()

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
        self.last_distance, self.last_clearance = dist, clear
        reached = dist < TARGET_THRESHOLD
        hit = clear < self.obstacle_radius
        reward = 250 if reached else (-1000 if hit else -1 * (dist - TARGET_THRESHOLD))
        return state, reward, 1 if (reached or hit) else 0


def build_kinematic(manipulator_file, endeffector_index, fixed_joints, involved_joints, target_position, obstacle_position,
                    initial_joint_positions=None, initial_positions_variation_range=None, link_radius=0.0,
                    obstacle_radius=OBSTACLE_RADIUS) -> KinematicEnvironment:
    """Picklable factory (HostVectorEnv's worker processes call it through functools.partial)."""
    model = compile_chain(load_urdf(manipulator_file), endeffector_index, involved_joints, fixed_joints,
                          initial_joint_positions, initial_positions_variation_range, link_radius)
    return KinematicEnvironment(model, target_position, obstacle_position, obstacle_radius)

"""ManipulatorFramework's trajectory methods (TrajectoryMethods) and what they do once the facade has looked at the environment:
demonstrate_trajectories and plan_trajectories: the refusals, then
environment.trajectory.plan_trajectories with the float64 twin as its backend (trajectories_host), or with the cached device tool
(chain_traj.TrajectoryChecker, kind 'trajectories' in arm_planner.ArmPlanner's cache). The checks shared with the other arm-planning
methods are arm_planner's."""
from __future__ import annotations

from typing import Optional

import numpy as np

from .arm_planner import ArmPlanner, _finite_number, _on_device, _refusing, check_arguments
from .environment.kinematic import JointPaths, demonstration_rows_host, reach_table
from .environment.tick_demo import trajectory_tick_plan
from .environment.trajectory import Trajectories, limits_of, trajectories_host
from .utils.exceptions import InvalidEnvironmentParameter


def plan_trajectories(planner: ArmPlanner, paths, obstacles, max_velocity, max_acceleration, dt, certify, clearance_margin, positions,
                      on_device) -> Trajectories:
    env = planner.env
    if not isinstance(paths, JointPaths) or paths.start is None or paths.goal is None:
        raise InvalidEnvironmentParameter('paths is the JointPaths that plan_joint_paths() or LinearMoves.as_joint_paths() returned')
    check_arguments(certify=certify, clearance_margin=clearance_margin)
    if not isinstance(positions, (bool, np.bool_)):
        raise InvalidEnvironmentParameter(f'positions is a bool: got {positions!r}')
    if isinstance(dt, bool) or not _finite_number(dt) or not dt > 0.0:
        raise InvalidEnvironmentParameter(f'dt is a positive time in seconds, the controller\'s period: got {dt!r}')
    if max_acceleration is None:
        raise InvalidEnvironmentParameter('max_acceleration has no default, the model has no acceleration limits: give a positive '
                                          'number, or one per joint')
    N, A = np.asarray(paths.start).shape
    if A != env.model.A:
        raise InvalidEnvironmentParameter(f'paths holds poses of {A} joints, the environment\'s arm has {env.model.A}')
    with _refusing():
        vmax, amax = limits_of('max_velocity', max_velocity, A), limits_of('max_acceleration', max_acceleration, A)
    _, _, obstacles, _ = planner.queries(np.zeros((N, 3)), obstacles, None)
    if certify:
        with _refusing():
            reach_table(env.model)                            # an unlimited prismatic joint, by name
    kw = dict(dt=float(dt), certify=bool(certify), margin=float(clearance_margin), positions=bool(positions))
    with _refusing():                                         # (a trajectory of too many ticks, by the query's name)
        if not _on_device(on_device):
            return trajectories_host(env, paths, obstacles, vmax, amax, **kw)
        from .chain_traj import TrajectoryChecker, TrajectoryLdsRefusal
        try:
            return planner.tool('trajectories', TrajectoryChecker).plan(paths, obstacles, vmax, amax, **kw)
        except TrajectoryLdsRefusal as err:
            raise InvalidEnvironmentParameter(f'plan_trajectories(): {err} (NAF_CHAIN_ERR_LDS); on_device=False answers this arm '
                                              f'through the float64 twin') from None


def demonstrate_trajectories(planner: ArmPlanner, traj, targets, obstacles, frames, keep_contact, feedback, on_device):
    """The ONE control flow of ManipulatorFramework.demonstrate_trajectories for device and twin: the refusals, the
    tick plan of the trajectories (environment.tick_demo.trajectory_tick_plan), then the writer's tick entry or
    demonstration_rows_host on the same plan"""
    env = planner.env
    if not isinstance(traj, Trajectories):
        raise InvalidEnvironmentParameter('trajectories is the Trajectories that plan_trajectories() returned')
    check_arguments(frames=frames)
    for name, v in (('keep_contact', keep_contact), ('feedback', feedback)):
        if not isinstance(v, (bool, np.bool_)):
            raise InvalidEnvironmentParameter(f'{name} is a bool: got {v!r}')
    A = np.asarray(traj.peak_velocity).shape[-1]
    if A != env.model.A:
        raise InvalidEnvironmentParameter(f'trajectories holds poses of {A} joints, the environment\'s arm has {env.model.A}')
    count = np.asarray(traj.n_nodes, np.int64)
    N = len(count)
    has = (count >= 1) & (np.asarray(traj.outcome) != 'none')
    with _refusing():
        plan = trajectory_tick_plan(traj, int(frames), bool(feedback), env.joint_limits(),
                                    np.asarray(env.initial_joint_positions, np.float64))
    if targets is None:      # the end effector of each trajectory's last node, by the twin; a query without one: where it stands
        nodes = np.asarray(traj.nodes, np.float64)
        last = np.where(has[:, None], nodes[np.arange(N), np.maximum(count - 1, 0)] if nodes.shape[1] else 0.0,
                        plan.q_start.astype(np.float64))
        targets = env.end_effector(last.astype(np.float32).astype(np.float64))
    _, targets, obstacles, _ = planner.queries(targets, obstacles, None)
    if len(targets) != N:
        raise InvalidEnvironmentParameter(f'targets is [N][3] with N = {N}, the number of trajectories: got {len(targets)}')
    if not _on_device(on_device):
        demos = demonstration_rows_host(env, plan, targets, obstacles, int(frames), bool(keep_contact), has)
    else:
        from .chain_tools import DemonstrationWriter
        demos = planner.tool('demonstrations', DemonstrationWriter).write(plan, targets, obstacles, bool(keep_contact), has)
    nan = lambda v: np.where(has, v, np.nan)      # noqa: E731
    return demos._replace(tracking_error=nan(plan.tracking_error), saturated_ticks=np.where(has, plan.saturated_ticks, 0),
                          peak_action=nan(plan.peak_action))


class TrajectoryMethods:
    """ManipulatorFramework's two trajectory methods (it inherits them): guards and one delegating call each, as its other arm-planning
    methods are"""

    def plan_trajectories(self, paths, obstacles=None, max_velocity=1.0, max_acceleration=None, dt: float = 1.0 / 240.0, certify: bool = False,
                          clearance_margin: float = 0.0, positions: bool = True, on_device: Optional[bool] = None):
        """Time-parameterised trajectories along planned joint paths, collision-checked at the controller's ticks (kinematic
        environment only; needs no agent). Every query of `paths` that has a path is driven as linear segments with parabolic
        blends under the joints' velocity and acceleration limits (environment/trajectory.py states the schedule and the law): the
        arm starts and ends at rest and does not stop at a corner, so it passes a corner NEAR it, not through it — a verdict or a
        certificate of the polyline does not carry over. The trajectory is therefore sampled every `dt`, walked and tested again.
          paths            : JointPaths of plan_joint_paths(), of any kind, or LinearMoves.as_joint_paths(); it is not changed
          obstacles        : as reach_targets() takes them — the scenes the paths were planned in
          max_velocity     : a scalar or [A], per joint (rad/s, m/s); the default 1.0 is the environment's own action bound
          max_acceleration : a scalar or [A]; it has to be given (None is refused) — the model has no acceleration limits
          dt               : the tick; the default is the environment's. With both defaults the sampled poses are a legal action
                             sequence under the step rule. A trajectory holds at most 8192 ticks; a longer one is refused by name.
          certify          : also decide the poses BETWEEN the ticks: every test at every tick has to keep clearance_margin plus
                             how far the tested capsule can travel over half a tick at the joints' peak speeds
          positions        : return the pose at every tick
          on_device        : None: the device when there is one (one naf_chain_traj_check / naf_chain_traj_certify launch per
                             chunk); False: the float64 host twin under the same rule (slow)
        Returns environment.trajectory.Trajectories, arrays over the queries: outcome ('free' | 'certified' | 'sampled': free at
        the ticks, not certified | 'blocked' | 'none': no path), duration, rest_to_rest_duration (with a stop at every corner: the
        blended trajectory is usually, not always, the shorter), n_samples, first_blocked, first_blocked_time, the three minima,
        corner_deviation, peak_velocity, peak_acceleration, slack and certified (with certify), leg_times, blend_times, positions
        [N][Smax][A]; velocities() and at(times) evaluate the float64 law. A 'blocked' trajectory is not re-timed: a lower
        max_velocity shrinks the corner deviation quadratically."""
        planner = self._kinematic_planner('plan_trajectories', 'chain model to drive')
        return plan_trajectories(planner, paths, obstacles, max_velocity, max_acceleration, dt, certify, clearance_margin, positions, on_device)

    def demonstrate_trajectories(self, trajectories, targets=None, obstacles=None, frames: int = 400, keep_contact: bool = False,
                                 feedback: bool = True, on_device: Optional[bool] = None):
        """Time-parameterised trajectories as demonstrations (kinematic environment only; needs no agent): query n drives the arm
        along the LAW plan_trajectories() checked — blends included — at the environment's own ticks, one action per tick, and
        every tick becomes the replay row run_training's environment would have written. The action of tick i aims at the law's
        pose at tick i + 1 from where the float32 arm is (environment/tick_demo.py states the rule), so the roundings do not add
        up: the arm stays within tracking_error of the law, a few float32 ulps while no action is clamped. The demonstration then
        visits the poses the trajectory's verdict is about, to within that error: a 'certified' trajectory planned with a
        clearance_margin above it (times the arm's reach) does not end in contact.
          trajectories : Trajectories of plan_trajectories() with max_velocity <= 1 (the action's bound: a faster joint is refused
                         by name); queries with outcome 'none' stand still and are reported 'none'; 'blocked' ones are driven
                         like any other, and their contact drops them unless keep_contact
          targets      : [N][3], or None: the end effector at each trajectory's last node; obstacles: as reach_targets() takes them
          frames       : the episode budget, 1 .. 1024: a longer trajectory is cut there (outcome 'frames')
          keep_contact : as demonstrate_joint_paths() takes it
          feedback     : False: the open-loop form a_i = (Q_{i+1} - Q_i) / DT, whose roundings add up — for comparison
          on_device    : None: the device when there is one (one naf_chain_demo_rows_ticks launch per chunk); False: the float64
                         host twin, `rows` a numpy array (slow)
        Returns environment.kinematic.Demonstrations as demonstrate_joint_paths() does, with tracking_error, saturated_ticks and
        peak_action filled (NaN / 0 for 'none'); planned_ticks is ceil(duration / DT). run_training(demonstrations=) and
        add_demonstrations() take it as they take the others."""
        planner = self._kinematic_planner('demonstrate_trajectories', 'chain model to drive')
        return demonstrate_trajectories(planner, trajectories, targets, obstacles, frames, keep_contact, feedback, on_device)

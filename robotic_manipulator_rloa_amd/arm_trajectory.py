"""What ManipulatorFramework.plan_trajectories does once the facade has looked at the environment: the refusals, then
environment.trajectory.plan_trajectories with the float64 twin as its backend (trajectories_host), or with the cached device tool
(chain_traj.TrajectoryChecker, kind 'trajectories' in arm_planner.ArmPlanner's cache). The checks shared with the other arm-planning
methods are arm_planner's."""
from __future__ import annotations

import numpy as np

from .arm_planner import ArmPlanner, _finite_number, _on_device, _refusing, check_arguments
from .environment.kinematic import JointPaths, reach_table
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

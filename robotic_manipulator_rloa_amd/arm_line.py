"""What ManipulatorFramework.plan_linear_moves does once the facade has looked at the environment: the refusals, then
environment.line_moves.plan_line_moves with the float64 twin as its backend, or with the cached device tools — chain_line.LineTracker
(kind 'line_moves' in arm_planner.ArmPlanner's cache) for the tracking launch and chain_tools.JointPathChecker (kind 'paths', the
one plan_joint_paths uses) for the legs' edge launch. The checks shared with the other arm-planning methods are arm_planner's."""
from __future__ import annotations

import numpy as np

from .arm_planner import ArmPlanner, _on_device, _refusing, check_arguments
from .environment.kinematic import reach_queries
from .environment.line_moves import HOLD_MODES, LINE_UPDATES_MAX, LinearMoves, _TwinLines, line_updates_ok, plan_line_moves
from .utils.exceptions import InvalidEnvironmentParameter


class _DeviceLines:
    """plan_line_moves' backend on the device: the planner's LineTracker and its JointPathChecker"""
    dtype = np.float32

    def __init__(self, planner: ArmPlanner):
        from .chain_line import LineTracker
        from .chain_tools import JointPathChecker
        self.chain = planner.env.model
        self.tracker, self.checker = planner.tool('line_moves', LineTracker), planner.tool('paths', JointPathChecker)
        self.twin = planner.env

    def track(self, q_start, disp, mode, W, U, constants, tool_axis, tool_normal):
        return self.tracker.track(q_start, disp, mode, W, U, constants, tool_axis, tool_normal)

    def end_effectors(self, q):
        return self.twin.end_effector(np.asarray(q, np.float64)).astype(np.float32)

    def edge_records(self, nodes, edges, obstacles, S, margin):
        return self.checker.edge_records(nodes, edges, obstacles, S, margin)


def _rows(name: str, value, width: int, N=None) -> np.ndarray:
    """value as [N][width] float64, [width] standing for one query (N None) or for all N; ValueError otherwise"""
    try:
        a = np.array(value, float)
    except (TypeError, ValueError):
        raise ValueError(f'{name} is not an array of numbers') from None
    if a.shape == (width,):
        a = np.broadcast_to(a, (1 if N is None else N, width))
    if a.ndim != 2 or a.shape[1] != width or len(a) == 0 or (N is not None and len(a) != N):
        many = f'[N][{width}]' if N is None else f'[N][{width}] with N = {N}, the number of queries'
        raise ValueError(f'{name} is {many}, or [{width}] for {"one query" if N is None else "all of them"}: got shape {a.shape}')
    bad = np.nonzero(~np.isfinite(a).all(axis=1))[0]
    if len(bad):
        raise ValueError(f'{name}[{int(bad[0])}] is not finite: {a[bad[0]].tolist()}')
    return a.copy()


def plan_linear_moves(planner: ArmPlanner, joint_positions, displacements, obstacles, hold, tool_axis, waypoints, updates, tolerance,
                      orientation_tolerance, resolution, clearance_margin, reverse, on_device) -> LinearMoves:
    env = planner.env
    model = env.model
    if not isinstance(hold, str) or hold not in HOLD_MODES:
        raise InvalidEnvironmentParameter(f'hold is one of {", ".join(map(repr, HOLD_MODES))}: got {hold!r}')
    check_arguments(waypoints=waypoints)
    if not line_updates_ok(waypoints, updates):
        raise InvalidEnvironmentParameter(f'updates is a positive number of updates per waypoint with waypoints x updates <= '
                                          f'{LINE_UPDATES_MAX}: got {updates!r} at waypoints={waypoints!r}')
    check_arguments(tolerance=tolerance, orientation_tolerance=orientation_tolerance, resolution=resolution,
                    clearance_margin=clearance_margin, reverse=reverse)
    with _refusing():
        q = _rows('joint_positions', joint_positions, model.A)
        far = np.zeros((len(q), 3))
        try:                                                  # the limits, by the path start and goal poses take
            q = reach_queries(model, far, far, q, 1)[0]
        except ValueError as err:
            raise ValueError(str(err).replace('initial_joint_positions', 'joint_positions')) from None
        N = len(q)
        disp = _rows('displacements', displacements, 3, N)
        d32 = disp.astype(np.float32).astype(np.float64)      # (as the device is given it)
        bad = np.nonzero(~(np.sum(d32 * d32, axis=1) > 0.0))[0]
        if len(bad):
            raise ValueError(f'displacements[{int(bad[0])}] has length 0: it names no line')
        try:
            shape = np.shape(tool_axis)
        except ValueError:
            shape = None
        if shape != (3,):
            raise ValueError(f'tool_axis is [3], a direction in the end-effector frame: got shape {shape}')
        axis = _rows('tool_axis', tool_axis, 3)[0]
        if not np.linalg.norm(axis) > 0.0:
            raise ValueError('tool_axis has length 0: it names no direction')
    _, _, obstacles, _ = planner.queries(far, obstacles, None)
    backend = _DeviceLines(planner) if _on_device(on_device) else _TwinLines(env)
    from .chain_line import LineLdsRefusal
    try:
        return plan_line_moves(backend, q, disp, obstacles, HOLD_MODES[hold], int(waypoints), int(updates), tolerance=float(tolerance),
                               orientation_tolerance=float(orientation_tolerance), resolution=float(resolution),
                               margin=float(clearance_margin), reverse=bool(reverse), tool_axis=axis)
    except LineLdsRefusal as err:
        raise InvalidEnvironmentParameter(f'plan_linear_moves(): {err} (NAF_CHAIN_ERR_LDS); on_device=False answers this arm '
                                          f'through the float64 twin') from None

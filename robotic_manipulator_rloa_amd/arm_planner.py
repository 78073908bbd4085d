"""ArmPlanner: what ManipulatorFramework's arm-planning methods do once the facade has looked at environment and agent — goal poses
by IK, collision-checked joint paths, their demonstrations, and the goal / path measures of a rollout to given targets. The checks
the methods share are written once here, and the device tools (chain_tools.py) live in one cache.

The planner belongs to a framework object and reads its `env` at every call: it survives delete_environment() followed by
initialize_kinematic_environment(), and the cache's key — the model's digest and the obstacle radius — decides what is rebuilt, not
the identity of the environment object.
"""
from __future__ import annotations

import contextlib
import functools
import weakref

import numpy as np
import torch

from .environment.kinematic import (DEMO_MAX_TICKS, PATH_CANDIDATES_MAX, PUSH_ORIENTATION_REFUSAL, ROADMAP_MAX, JointPaths, demonstration_plan,
                                    demonstration_rows_host, demonstration_speed_ok, goal_poses_host, ik_restarts_ok, joint_paths_host,
                                    orientation_goal, reach_queries, roadmap_milestones, roadmap_size_ok, shortcut_size_ok)
from .environment.line_moves import LINE_WAYPOINTS_MAX, line_waypoints_ok
from .environment.polyline import SHORTCUT_MAX, SHORTCUT_MIN, pad_shortcut, polyline_plan, roadmap_arguments, roadmap_queries
from .utils.exceptions import InvalidEnvironmentParameter
from .utils.logger import get_global_logger

logger = get_global_logger()


def _positive_int(v) -> bool:
    return isinstance(v, int) and v > 0


@contextlib.contextmanager
def _refusing():
    """a ValueError of the host-side checks (reach_queries and its like) leaves as InvalidEnvironmentParameter, text unchanged"""
    try:
        yield
    except ValueError as err:
        raise InvalidEnvironmentParameter(str(err)) from None


def _on_device(on_device) -> bool:
    """on_device=None: the device when there is one"""
    return torch.cuda.is_available() if on_device is None else on_device


def _finite_number(v) -> bool:
    return isinstance(v, (int, float)) and bool(np.isfinite(v))


# argument -> (what it has to be, how its refusal says so): the checks of single values, each written once
_ARGUMENT_RULES = {
    'restarts': (ik_restarts_ok, 'a power of two from 1 to 64'),
    'iterations': (_positive_int, 'a positive number of updates'),
    'tolerance': (lambda v: _finite_number(v) and v > 0.0, 'a positive length'),
    'clearance_margin': (_finite_number, 'a finite length'),
    'seed': (lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer)) and v >= 0, 'a non-negative integer'),
    'candidates': (lambda v: _positive_int(v) and v <= PATH_CANDIDATES_MAX, f'a number of paths from 1 to {PATH_CANDIDATES_MAX}'),
    'resolution': (lambda v: not isinstance(v, bool) and _finite_number(v) and v > 0.0, 'a positive joint-space distance'),
    'certify': (lambda v: isinstance(v, (bool, np.bool_)), 'a bool'),
    'speed': (demonstration_speed_ok, 'a share of the unit action, 0 < speed <= 1'),
    'frames': (lambda v: _positive_int(v) and v <= DEMO_MAX_TICKS, f'a number of steps from 1 to {DEMO_MAX_TICKS}'),
    'shortcut': (shortcut_size_ok, f'a number of nodes, 0 (no shortcut round) or from {SHORTCUT_MIN} to {SHORTCUT_MAX}'),
    'polylines': (lambda v: isinstance(v, (bool, np.bool_)), 'a bool'),
    'orientation_tolerance': (lambda v: not isinstance(v, bool) and _finite_number(v) and v > 0.0, 'a positive angle in radians'),
    'orientation_weight': (lambda v: v is None or (not isinstance(v, bool) and _finite_number(v) and v > 0.0),
                           'a positive length per radian, or None for a quarter of the reach'),
    'avoid_contact': (lambda v: isinstance(v, (bool, np.bool_)), 'a bool'),
    'clearance_goal': (lambda v: v is None or (not isinstance(v, bool) and _finite_number(v)), 'a finite length, or None for clearance_margin + 0.02'),
    'push_iterations': (lambda v: not isinstance(v, bool) and _positive_int(v) and v >= 4, 'a number of updates, at least 4 (the last four settle without a push)'),
    'waypoints': (line_waypoints_ok, f'a number of waypoints from 1 to {LINE_WAYPOINTS_MAX}'),
    'reverse': (lambda v: isinstance(v, (bool, np.bool_)), 'a bool'),
}

ORIENTATION_ARGUMENTS = ('orientations', 'approach_directions', 'tool_axis', 'orientation_tolerance', 'orientation_weight')


def orientation_given(orientation) -> bool:
    """whether a method's orientation keyword arguments ask for an orientation goal"""
    return bool(orientation) and (orientation.get('orientations') is not None or orientation.get('approach_directions') is not None)


def check_orientation(orientation, N: int, tolerance: float = 1e-3) -> dict:
    """The orientation keyword arguments of a call with N queries through their refusals (environment.kinematic.orientation_goal
    names the query): {} where no orientation goal is asked for, otherwise the arguments as the solvers take them."""
    if not orientation_given(orientation):
        return {}
    kw = {k: orientation[k] for k in ORIENTATION_ARGUMENTS if k in orientation}
    check_arguments(orientation_tolerance=kw.get('orientation_tolerance', 1e-3), orientation_weight=kw.get('orientation_weight'))
    with _refusing():
        orientation_goal(N, kw.get('orientations'), kw.get('approach_directions'), kw.get('tool_axis', (0.0, 0.0, 1.0)), tolerance,
                         kw.get('orientation_tolerance', 1e-3))
    return kw


def check_push(push, orientation) -> dict:
    """The avoid_contact keyword arguments of a call through their refusals: {} where no push is asked for, otherwise the arguments
    as the solvers take them. Positional goals only: refused together with an orientation goal."""
    if not push:
        return {}
    check_arguments(avoid_contact=push.get('avoid_contact', False))
    if not push.get('avoid_contact'):
        return {}
    check_arguments(clearance_goal=push.get('clearance_goal'), push_iterations=push.get('push_iterations', 16))
    if orientation_given(orientation):
        raise InvalidEnvironmentParameter(PUSH_ORIENTATION_REFUSAL)
    return dict(avoid_contact=True, clearance_goal=push.get('clearance_goal'), push_iterations=int(push.get('push_iterations', 16)))


def check_arguments(**given) -> None:
    """refuses the first of the given arguments, in the order they are given, that breaks its rule"""
    for name, v in given.items():
        ok, words = _ARGUMENT_RULES[name]
        if not ok(v):
            raise InvalidEnvironmentParameter(f'{name} is {words}: got {v!r}')


def check_roadmap(roadmap, certify, who, shortcut=0) -> None:
    if not roadmap_size_ok(roadmap):
        raise InvalidEnvironmentParameter(f'roadmap is a number of milestones from 0 to {ROADMAP_MAX} (0: no roadmap): '
                                          f'got {roadmap!r}')
    if roadmap and certify:
        raise InvalidEnvironmentParameter(f'{who}(roadmap={roadmap!r}, certify=True): roadmap edges are checked at their samples '
                                          f'only, and nothing certifies a \'roadmap\' path between them')
    check_arguments(shortcut=shortcut)
    if shortcut and not roadmap:
        raise InvalidEnvironmentParameter(f'{who}(shortcut={shortcut!r}) shortens \'roadmap\' polylines: it needs roadmap=M with M > 0')


class ArmPlanner:

    def __init__(self, framework) -> None:
        self._framework = weakref.ref(framework)      # (the framework owns the planner: no cycle keeps the device tools alive)
        self.tools = {}                               # kind -> (key, tool): one live tool of each kind
        self._path_step_warned = False

    @property
    def env(self):
        return self._framework().env

    @property
    def nominal_obstacle(self):
        env = self.env
        return env.obstacle_centre if env.scene_ranges_on else env.obstacle_pos

    def queries(self, targets, obstacles, initial_joint_positions, frames=1):
        """reach_queries of the environment's arm, with its nominal obstacle and start pose where none is given"""
        env = self.env
        with _refusing():
            return reach_queries(env.model, targets, obstacles, initial_joint_positions, frames,
                                 nominal_obstacle=self.nominal_obstacle, nominal_start=env.initial_joint_positions)

    def tool(self, kind: str, factory):
        """The device tool of this kind for the environment's arm: factory(model, obstacle_radius) on the first call and whenever
        the model or the radius has changed — the old tool, its handle and buffers, is dropped before the new one is built."""
        env = self.env
        key = (kind, env.model.digest(), float(env.obstacle_radius))
        if kind not in self.tools or self.tools[kind][0] != key:
            self.tools.pop(kind, None)
            self.tools[kind] = (key, factory(env.model, env.obstacle_radius))
        return self.tools[kind][1]

    # ---- goal poses ---------------------------------------------------------------------------------------------------------------
    def solve_goal_poses(self, targets, obstacles, initial_joint_positions, restarts, iterations, tolerance, clearance_margin, seed,
                         on_device, orientation=None, push=None):
        check_arguments(restarts=restarts, iterations=iterations, tolerance=tolerance, clearance_margin=clearance_margin, seed=seed)
        push = check_push(push, orientation)
        q0, targets, obstacles, _ = self.queries(targets, obstacles, initial_joint_positions)
        kw = dict(restarts=int(restarts), iterations=int(iterations), tolerance=float(tolerance), margin=float(clearance_margin),
                  seed=int(seed), **check_orientation(orientation, len(q0), float(tolerance)), **push)
        if not _on_device(on_device):
            return goal_poses_host(self.env, q0, targets, obstacles, **kw)
        from .chain_tools import GoalPoseSolver
        return self.tool('goal_poses', GoalPoseSolver).solve(q0, targets, obstacles, **kw)

    # ---- joint paths --------------------------------------------------------------------------------------------------------------
    def _goal_queries(self, goal_joint_positions, obstacles, initial_joint_positions):
        """(q0, q_goal, obstacles) of plan_joint_paths(goal_joint_positions=): the goal poses go through the same refusals as start
        poses do — shape, finite numbers, the joints' limits"""
        model = self.env.model
        with _refusing():
            try:
                goals = np.array(goal_joint_positions, float)
            except (TypeError, ValueError):
                raise ValueError('goal_joint_positions is not an array of numbers') from None
            if goals.shape == (model.A,):
                goals = goals[None]
            if goals.ndim != 2 or goals.shape[1] != model.A or len(goals) == 0:
                raise ValueError(f'goal_joint_positions is [N][{model.A}], or [{model.A}] for one query (one value per '
                                 f'involved joint): got shape {goals.shape}')
            far = np.zeros((len(goals), 3))
            try:
                q_goal = reach_queries(model, far, far, goals, 1)[0]
            except ValueError as err:
                raise ValueError(str(err).replace('initial_joint_positions', 'goal_joint_positions')) from None
        q0, _, obstacles, _ = self.queries(far, obstacles, initial_joint_positions)
        return q0, q_goal, obstacles

    def plan_joint_paths(self, targets, obstacles, initial_joint_positions, goal_joint_positions, candidates, resolution,
                         clearance_margin, seed, on_device, certify, roadmap, shortcut=0, orientation=None, push=None):
        model = self.env.model
        if (targets is None) == (goal_joint_positions is None):
            raise InvalidEnvironmentParameter('plan_joint_paths() takes exactly one of targets and goal_joint_positions')
        if goal_joint_positions is not None and orientation_given(orientation):
            raise InvalidEnvironmentParameter('plan_joint_paths(goal_joint_positions=) is given the goal poses themselves: orientations '
                                              'and approach_directions are goals of the poses solved for targets')
        if goal_joint_positions is not None and push and push.get('avoid_contact'):
            raise InvalidEnvironmentParameter('plan_joint_paths(goal_joint_positions=) is given the goal poses themselves: avoid_contact '
                                              'refines the poses solved for targets')
        push = check_push(push, orientation)
        check_arguments(candidates=candidates, resolution=resolution, clearance_margin=clearance_margin, seed=seed, certify=certify)
        check_roadmap(roadmap, certify, 'plan_joint_paths', shortcut)
        if roadmap:
            try:
                roadmap_milestones(model, np.zeros((0, model.A)), np.zeros((0, model.A)), int(roadmap), 0)
            except ValueError as err:
                raise InvalidEnvironmentParameter(f'roadmap: {err}') from None
        kw = dict(candidates=candidates, resolution=resolution, clearance_margin=clearance_margin, seed=seed, on_device=on_device,
                  certify=bool(certify), roadmap=int(roadmap), shortcut=int(shortcut))
        if targets is None:
            return self.plan_checked(*self._goal_queries(goal_joint_positions, obstacles, initial_joint_positions), **kw)
        q0, targets, obstacles, _ = self.queries(targets, obstacles, initial_joint_positions)
        goal = self._framework().solve_goal_poses(targets, obstacles, q0, seed=seed, on_device=on_device,
                                                  **check_orientation(orientation, len(q0)), **push)
        return self.paths_to_goals(goal, q0, obstacles, kw)

    def plan_checked(self, q0, q_goal, obstacles, candidates=16, resolution=0.02, clearance_margin=0.0, seed=0, on_device=None,
                     certify=False, roadmap=0, shortcut=0) -> JointPaths:
        """the paths of queries that have passed the refusals: the twin's, or the cached checker's of the kind asked for"""
        kw = dict(candidates=int(candidates), resolution=float(resolution), margin=float(clearance_margin), seed=int(seed),
                  roadmap=int(roadmap), shortcut=int(shortcut))
        if not _on_device(on_device):
            out = joint_paths_host(self.env, q0, q_goal, obstacles, certify=bool(certify), **kw)
        else:
            from .chain_tools import JointPathChecker
            # the plain and the certifying checker are kinds of their own: calls may alternate without rebuilding handle and buffers
            kind, build = ('certified_paths', functools.partial(JointPathChecker, certify=True)) if certify else ('paths', JointPathChecker)
            out = self.tool(kind, build).check(q0, q_goal, obstacles, **kw)
        with np.errstate(invalid='ignore'):
            coarse = np.asarray(out.sample_step, np.float64) > resolution
        if coarse.any() and not self._path_step_warned:
            self._path_step_warned = True
            logger.warning(f'plan_joint_paths: {int(coarse.sum())} queries are sampled at the cap of 2048 poses per path, '
                           f'{float(np.max(np.asarray(out.sample_step)[coarse])):.4g} apart, coarser than resolution={resolution!r}')
        return out

    def paths_to_goals(self, goal, q0, obstacles, kw) -> JointPaths:
        """plan_joint_paths to the poses of `goal` (GoalPoses): queries without a reachable pose get outcome 'goal' and NaN numbers"""
        ok = np.asarray(goal.reachable, bool)
        N, A = len(ok), self.env.model.A
        if ok.all():
            return self.plan_checked(q0, np.asarray(goal.joint_positions, np.float64), obstacles, **kw)
        # (the poses a solver returned lie inside the limits: they are not put through the refusals again)
        found = self.plan_checked(q0[ok], np.asarray(goal.joint_positions, np.float64)[ok], obstacles[ok], **kw) if ok.any() else None
        kind = np.float32 if found is None else found.length.dtype
        nan = lambda *shape: np.full((N,) + shape, np.nan, kind)      # noqa: E731
        parts = [np.full(N, 'goal', '<U8'), np.full(N, -1, np.int64), nan(A), nan(), nan(), nan(), nan(), nan(), np.full(N, -1, np.int64),
                 nan(), np.zeros(N, np.int64), np.asarray(q0, kind), nan(A), np.zeros(N, bool), nan(), np.zeros(N, np.int64)]
        for dst, src in zip(parts, found or ()):
            dst[ok] = src
        out = JointPaths(*parts)
        if found is not None and found.n_nodes is not None:      # the roadmap's attributes, padded as the fields are
            out.nodes = np.full((N,) + found.nodes.shape[1:], np.nan, found.nodes.dtype)
            out.n_nodes, out.roadmap_free_edges = np.zeros(N, np.int64), np.full(N, -1, np.int64)
            out.nodes[ok], out.n_nodes[ok], out.roadmap_free_edges[ok] = found.nodes, found.n_nodes, found.roadmap_free_edges
        elif kw.get('roadmap'):
            out.nodes = np.full((N, 0, A), np.nan, kind)
            out.n_nodes, out.roadmap_free_edges = np.zeros(N, np.int64), np.full(N, -1, np.int64)
        pad_shortcut(out, found, ok, kind, kw.get('shortcut'))
        return out

    # ---- demonstrations -----------------------------------------------------------------------------------------------------------
    def demonstrate_joint_paths(self, paths, targets, obstacles, speed, frames, keep_contact, on_device, polylines=False):
        env = self.env
        if not isinstance(paths, JointPaths) or paths.start is None or paths.goal is None:
            raise InvalidEnvironmentParameter('paths is the JointPaths that plan_joint_paths() returned')
        check_arguments(speed=speed, frames=frames, polylines=polylines)
        has = np.asarray(paths.candidate) >= 0
        start = np.asarray(paths.start, np.float64)
        N, A = start.shape
        if A != env.model.A:
            raise InvalidEnvironmentParameter(f'paths holds poses of {A} joints, the environment\'s arm has {env.model.A}')
        # a query without a path stands still at its start pose for the launch and is reported 'none'
        via = np.where(has[:, None], np.asarray(paths.via, np.float64), start)
        has = has | roadmap_queries(paths, polylines)         # polylines: a 'roadmap' query has a path too, all its nodes
        goal = np.where(has[:, None], np.asarray(paths.goal, np.float64), start)
        if targets is None:
            targets = env.end_effector(np.asarray(goal, np.float32).astype(np.float64))
        _, targets, obstacles, _ = self.queries(targets, obstacles, None)
        if len(targets) != N:
            raise InvalidEnvironmentParameter(f'targets is [N][3] with N = {N}, the number of paths: got {len(targets)}')
        plan = (polyline_plan(paths, start, via, goal, float(speed), int(frames)) if polylines else
                demonstration_plan(start, via, goal, float(speed), int(frames)))
        if not _on_device(on_device):
            return demonstration_rows_host(env, plan, targets, obstacles, int(frames), bool(keep_contact), has)
        from .chain_tools import DemonstrationWriter
        return self.tool('demonstrations', DemonstrationWriter).write(plan, targets, obstacles, bool(keep_contact), has)

    # ---- rollouts to given targets ------------------------------------------------------------------------------------------------
    def reach_targets(self, agent, targets, obstacles, initial_joint_positions, frames, noise_scale, n_envs, trajectories, goal_poses,
                      joint_paths, certify, roadmap, shortcut=0, orientation=None, push=None):
        """the queries and the refusals of reach_targets(), the agent's rollout, then the goal poses, the paths and their ratios"""
        env = self.env
        q0, targets, obstacles, frames = self.queries(targets, obstacles, initial_joint_positions, frames)
        goal_poses = bool(goal_poses or joint_paths)
        if orientation_given(orientation) and not goal_poses:
            raise InvalidEnvironmentParameter('reach_targets(orientations= / approach_directions=) is a goal of the goal poses: it needs '
                                              'goal_poses=True or joint_paths=True (the policy and its outcome know no orientation)')
        if push and push.get('avoid_contact') and not goal_poses:
            raise InvalidEnvironmentParameter('reach_targets(avoid_contact=True) refines the goal poses: it needs goal_poses=True or '
                                              'joint_paths=True')
        push = check_push(push, orientation)
        orientation = check_orientation(orientation, len(q0))
        if not isinstance(certify, (bool, np.bool_)) or (certify and not joint_paths):
            raise InvalidEnvironmentParameter('reach_targets(certify=True) certifies the joint paths: it is a bool and needs joint_paths=True')
        check_roadmap(roadmap, certify, 'reach_targets', shortcut)
        if roadmap and not joint_paths:
            raise InvalidEnvironmentParameter('reach_targets(roadmap=M) builds roadmaps for the joint paths: it needs joint_paths=True')
        if goal_poses and not trajectories:
            raise InvalidEnvironmentParameter('reach_targets(goal_poses=True) measures the joint path: it needs trajectories=True')
        result = agent.rollout_vectorized(env.model, targets, obstacles, q0, frames=frames, noise_scale=float(noise_scale),
                                          n_envs=n_envs, trajectories=bool(trajectories), scene={'obstacle_radius': env.obstacle_radius})
        if goal_poses:
            result.goal = self._framework().solve_goal_poses(targets, obstacles, q0, **orientation, **push)
            path = np.asarray(result.joint_positions, np.float64)
            length = np.sum(np.max(np.abs(np.diff(path, axis=1)), axis=2), axis=1)
            with np.errstate(divide='ignore', invalid='ignore'):
                ratio = length / np.asarray(result.goal.joint_distance, np.float64)
            result.path_ratio = np.where((np.asarray(result.outcome) == 'reached') & result.goal.free, ratio, np.nan)
        if joint_paths:
            result.path = self.paths_to_goals(result.goal, q0, obstacles,
                                              {'certify': True} if certify else roadmap_arguments(roadmap, shortcut))
            with np.errstate(divide='ignore', invalid='ignore'):
                ratio = length / np.asarray(result.path.length, np.float64)
            # a query has a path when its length is a number: a candidate of the one-via round, or a 'roadmap' polyline
            has_path = np.isfinite(np.asarray(result.path.length, np.float64))
            result.planned_ratio = np.where((np.asarray(result.outcome) == 'reached') & has_path, ratio, np.nan)
        return result

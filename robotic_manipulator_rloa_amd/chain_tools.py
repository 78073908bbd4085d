"""Device tools on a chain model that need no agent, no learner and no graph (csrc/chain_env.hip): each owns the model's handle
and its buffers, uploads a chunk of queries, launches, and downloads the records the host chooses from.

  _ChainHandle       : the one owner of a chain model's device handle (engine.DeviceEnvLoop and DeviceRollout hold one too).
  GoalPoseSolver     : joint values that reach given targets: batched damped least squares over queries x restarts, the pinned
                       clearances at the solved poses, the selection per query (GoalPoses).
  JointPathChecker   : sampled collision checks of start -> via -> goal joint paths: ONE launch over queries x candidate vias x
                       samples, eight floats per candidate back, the choice per query on the host (JointPaths). certify=True:
                       naf_chain_path_certify's twelve floats and the refinement rounds over the open queries. It is the device
                       backend of environment.kinematic.plan_paths, whose other backend is the float64 twin.
  DemonstrationWriter: planned joint paths as replay rows: ONE launch per chunk, the kept rows as a device tensor (Demonstrations).

Every launch goes to the stream torch reports as current. An upload is one copy_ on that stream; a download is the one .cpu() that
waits for the launches in front of it.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .chain_clear import ClearLaunch
from .chain_ticks import TicksLaunch
from .environment.kinematic import (DEMO_CHUNK, DEMO_FLOATS, DEMO_MAX_TICKS, EDGE_FLOATS, PATH_CERT_FLOATS, PATH_CHUNK, PATH_FLOATS,
                                    GoalPoses, JointPaths, certificate_guard, concatenate_goal_poses, demo_row_layout,
                                    gather_demonstrations, gather_goal_poses, ik_seeds, note_pushed, orientation_goal, plan_paths,
                                    reach_table)


class _ChainHandle:
    """The one owner of a chain model's device handle (csrc/chain_env.hip): packs the blob, creates the handle on `self.lib` and
    destroys it with the object. `_chain_env` stays None until a model is opened."""
    _chain_env = None

    def _create_chain_env(self, chain) -> None:
        blob = np.ascontiguousarray(chain.pack(), np.float32)
        handle = ctypes.c_void_p()
        check(self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(handle)), "chain_env_create")
        self.chain, self._chain_env = chain, handle
        self.has_cell = bool(chain.cell_spheres or chain.cell_planes or chain.cell_boxes)

    def __del__(self):
        if self._chain_env is not None:
            self.lib.naf_chain_env_destroy(self._chain_env)
            self._chain_env = None


class _ChainTool(_ChainHandle):
    """What the three tools share: the library, the model and its handle, the device, the obstacle radius as float32 holds it, and a
    chunk — the class's CHUNK unless given, refused below its CHUNK_MIN with its CHUNK_REFUSAL."""

    def __init__(self, chain, obstacle_radius: float, chunk: Optional[int], device) -> None:
        _lib.require_gpu()
        self.lib, self.chain, self.A = _lib.load(), chain, chain.A
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        self.obstacle_radius = float(np.float32(obstacle_radius))
        self.chunk = int(self.CHUNK if chunk is None else chunk)
        if self.chunk < self.CHUNK_MIN:
            raise ValueError(self.CHUNK_REFUSAL)
        self._create_chain_env(chain)

    def _zeros(self, *shape, dtype=torch.float32) -> torch.Tensor:
        return torch.zeros(*shape, dtype=dtype, device=self.dev)

    @staticmethod
    def _upload(buf: torch.Tensor, a, dtype=np.float32) -> None:
        """a[n][...] into the first n rows of buf: one copy_ on the current stream"""
        a = np.ascontiguousarray(a, dtype)
        buf[:len(a)].copy_(torch.from_numpy(a))

    @staticmethod
    def _download(buf: torch.Tensor, n: int, *shape) -> np.ndarray:
        """the first n rows of buf as a numpy array, reshaped where a shape is given"""
        out = buf[:n].cpu().numpy()
        return out.reshape(shape) if shape else out


class GoalPoseSolver(ClearLaunch, _ChainTool):
    """Goal poses on a chain model (csrc/chain_env.hip, "goal poses"): per chunk of candidates naf_chain_ik_solve, then the
    clearances of the solved poses by naf_chain_env_reset_given + naf_chain_env_probe (+ naf_chain_env_probe_cell with a workcell),
    then naf_chain_ik_select. Owns the handle and the buffers; needs no agent. A chunk holds a fixed number of candidates,
    `chunk` rounded down to whole queries; a query's result does not depend on the chunk or the lane it lands in.
    With an orientation goal (solve(orientations=) or solve(approach_directions=)) the first launch is naf_chain_ik_solve_pose
    and the selection is fed its merit; the goal, angle and merit buffers are allocated on the first such call. Without one
    the launches are the ones above and those buffers do not exist.
    With solve(avoid_contact=True) one launch, naf_chain_ik_clear (chain_clear.ClearLaunch), sits between the solve and the
    clearances: it refines the poses in self.q and their residuals in place, so the launches behind it are the ones above on better
    poses. Its obstacle, working-pose and record buffers are allocated on the first such call; positional goals only."""
    CHUNK, CHUNK_MIN, CHUNK_REFUSAL = 32768, 64, "GoalPoseSolver: a chunk holds at least 64 candidates"

    def __init__(self, chain, obstacle_radius: float = 0.06, chunk: Optional[int] = None, device=None):
        super().__init__(chain, obstacle_radius, chunk, device)
        C, A, z = self.chunk, self.A, self._zeros
        self.targets, self.q_start, self.seeds = z(C, 3), z(C, A), z(C, A)
        self.q, self.residual, self.distance = z(C, A), z(C), z(C)
        self.env_state = z(C, self.lib.naf_chain_env_state_floats(self._chain_env))
        self.obs, self.scene = z(C, 2 * A + 9), z(C, 6)
        self.probe, self.cell = z(C, 5), torch.full((C,), float("inf"), dtype=torch.float32, device=self.dev)
        self.choice, self.cls = z(C, dtype=torch.int32), z(C, dtype=torch.int32)
        self.goals = self.angle = self.merit = None      # with an orientation goal only

    def params(self, iterations: int, lam=None, e_max=None, dq_max=None) -> "_lib.IkParams":
        reach = self.chain.reach
        lam = 0.05 * reach if lam is None else lam
        return _lib.IkParams(int(iterations), float(lam) ** 2, float(0.25 * reach if e_max is None else e_max),
                             float(0.5 if dq_max is None else dq_max))

    def pose_params(self, og, weight=None, w_max=None) -> "_lib.IkPoseParams":
        """naf_chain_ik_pose_params_t of an OrientationGoal: weight 0.25 reach and w_max 0.5 rad unless given"""
        f3 = ctypes.c_float * 3
        return _lib.IkPoseParams(float(0.25 * self.chain.reach if weight is None else weight), float(0.5 if w_max is None else w_max),
                                 og.angle_length, f3(*map(float, og.tool_axis)), f3(*map(float, og.tool_normal)))

    def launch(self, n: int, R: int, prm, tolerance: float, margin: float, solve_only: bool = False, mode=None, pose=None,
               clear=None) -> None:
        """the launches of one chunk of n queries x R restarts already in the buffers, on the current stream; mode / pose: the
        chunk's orientation goals are in self.goals and the first launch is naf_chain_ik_solve_pose; clear (clear_setup): the
        chunk's obstacles are in self.obstacles and naf_chain_ik_clear follows the solve"""
        st, E = stream_ptr(), n * R
        measure = self.residual
        if mode is None:
            check(self.lib.naf_chain_ik_solve(self._chain_env, ptr(self.targets), ptr(self.q_start), ptr(self.seeds), n, R, prm,
                                              ptr(self.q), ptr(self.residual), None, st), "chain_ik_solve")
        else:
            check(self.lib.naf_chain_ik_solve_pose(self._chain_env, ptr(self.targets), ptr(self.goals), int(mode), ptr(self.q_start),
                                                   ptr(self.seeds), n, R, prm, pose, ptr(self.q), ptr(self.residual), ptr(self.angle),
                                                   ptr(self.merit), None, st), "chain_ik_solve_pose")
            measure = self.merit
        if solve_only:
            return
        if clear is not None:
            self.launch_clear(n, R, clear)
        check(self.lib.naf_chain_env_reset_given(self._chain_env, ptr(self.env_state), ptr(self.obs), E, ptr(self.q), ptr(self.scene),
                                                 self.obstacle_radius, st), "chain_env_reset_given")
        check(self.lib.naf_chain_env_probe(self._chain_env, ptr(self.env_state), ptr(self.probe), E, st), "chain_env_probe")
        if self.has_cell:
            check(self.lib.naf_chain_env_probe_cell(self._chain_env, ptr(self.env_state), ptr(self.cell), E, st), "chain_env_probe_cell")
        check(self.lib.naf_chain_ik_select(self._chain_env, ptr(self.q), ptr(self.q_start), ptr(measure), ptr(self.probe),
                                           ptr(self.cell) if self.has_cell else None, n, R, tolerance, margin, ptr(self.choice),
                                           ptr(self.cls), ptr(self.distance), st), "chain_ik_select")

    def load(self, q0, targets, obstacles, seeds) -> None:
        """a chunk's queries into the buffers: q0[n][A], targets[n][3], obstacles[n][3], seeds[n][R][A] (float32)"""
        n, R = seeds.shape[:2]
        self._upload(self.targets, targets)
        self._upload(self.q_start, q0)
        self._upload(self.seeds, np.asarray(seeds, np.float32).reshape(n * R, self.A))
        scene = np.concatenate([np.asarray(targets, np.float32), np.asarray(obstacles, np.float32)], axis=1)
        self._upload(self.scene, np.repeat(scene, R, axis=0))

    def solve(self, q0, targets, obstacles, restarts: int = 8, iterations: int = 32, tolerance: float = 1e-3, margin: float = 0.0,
              seed: int = 0, orientations=None, approach_directions=None, tool_axis=(0.0, 0.0, 1.0),
              orientation_tolerance: float = 1e-3, orientation_weight: Optional[float] = None, w_max: Optional[float] = None,
              **constants) -> GoalPoses:
        """q0[N][A] (action order), targets[N][3], obstacles[N][3] -> GoalPoses of numpy arrays (float32 where the device's).
        orientations[N][4] | [4] (quaternions x, y, z, w) or approach_directions[N][3] | [3] (for tool_axis, in the end-effector
        frame): an orientation goal (environment.kinematic.orientation_goal); GoalPoses.angle_residual is then filled.
        avoid_contact=True (with clearance_goal, push_iterations, push_settle, push_max): every chunk's candidates go through
        naf_chain_ik_clear before their clearances are taken (positional goals only); GoalPoses.pushed and .input_clearance are
        then filled."""
        A, R = self.A, int(restarts)
        q0 = np.ascontiguousarray(q0, np.float32).reshape(-1, A)
        N = len(q0)
        targets, obstacles = np.asarray(targets, np.float32).reshape(N, 3), np.asarray(obstacles, np.float32).reshape(N, 3)
        seeds = ik_seeds(self.chain, N, R, seed)
        og = orientation_goal(N, orientations, approach_directions, tool_axis, tolerance, orientation_tolerance)
        mode = pose = None
        if og is not None:
            mode, pose = og.mode, self.pose_params(og, orientation_weight, w_max)
            if self.goals is None:
                self.goals, self.angle, self.merit = self._zeros(self.chunk, 9), self._zeros(self.chunk), self._zeros(self.chunk)
        tolerance, margin = float(np.float32(tolerance)), float(np.float32(margin))
        clear = self.clear_setup(constants, tolerance, margin, orientations, approach_directions)
        prm = self.params(iterations, **constants)
        per = self.chunk // R
        parts, get = [], self._download
        for first in range(0, N, per):
            n = min(per, N - first)
            sl = slice(first, first + n)
            self.load(q0[sl], targets[sl], obstacles[sl], seeds[sl])
            if og is not None:      # the chunk's goals, [n][9] or [n][3] rows packed at the front of the buffer
                self.goals.view(-1)[:og.goals[sl].size].copy_(torch.from_numpy(np.ascontiguousarray(og.goals[sl]).reshape(-1)))
            self.launch(n, R, prm, tolerance, margin, mode=mode, pose=pose, clear=self.load_clear(clear, obstacles[sl]))
            E = n * R
            cell = get(self.cell, E, n, R) if self.has_cell else np.full((n, R), np.inf, np.float32)
            probe = get(self.probe, E, n, R, 5)
            more = () if og is None else (get(self.angle, E, n, R), get(self.merit, E, n, R))
            parts.append(note_pushed(gather_goal_poses(get(self.choice, n), get(self.cls, n), get(self.q, E, n, R, A), get(self.residual, E, n, R),
                                           probe[:, :, 3], probe[:, :, 4], cell, get(self.distance, E, n, R), np.float32(tolerance),
                                           *more), clear and get(self.clear, E, n, R, 4)))
        return concatenate_goal_poses(parts)


class JointPathChecker(_ChainTool):
    """Collision-checked joint paths on a chain model (csrc/chain_env.hip, "joint paths"): per chunk of queries ONE
    naf_chain_path_check launch over queries x candidate vias, S sampled poses each, formed on the fly — no pose is materialised and
    eight floats per candidate come back; the choice among a query's candidates is environment.kinematic.select_joint_path on the
    host. Owns the handle and the buffers; needs no agent. A chunk holds at most `chunk` candidate-samples (queries x candidates x
    S, whole queries) and its S is path_samples of its own legs (path_chunks); a candidate's record does not depend on where in a
    launch it lies. The check is SAMPLED: see JointPaths. certify=True: the launches are naf_chain_path_certify's, twelve floats per
    candidate, with the model's reach table uploaded once; check() then runs the refinement rounds over the open queries
    (environment.kinematic.certify_rounds) and fills JointPaths' last three fields. The certifying launch keeps the handle's lanes
    and adds a reduction row and three small tables to its LDS: an arm with pairs whose rows only just fit a workgroup is refused
    (NAF_CHAIN_ERR_LDS) where the sampled check runs; joint_paths_host(certify=True) answers it.
    check(roadmap=M): behind the one-via chunks, the queries that ended 'blocked' get a roadmap of M milestones each
    (environment.kinematic.roadmap_round): per chunk of whole queries ONE naf_chain_edge_check launch over queries x E edges, S
    samples each, within the same budget; the node, edge and record buffers are allocated on the first such call. The records — a
    few KB per blocked query — are downloaded and roadmap_search runs on the host, as the one-via selection does.
    The control flow of check() is environment.kinematic.plan_paths', which the twin runs too: this class is its device backend —
    dtype, prefix, the refusal's text, prepare() and the three evaluators path_records, certified_records and edge_records, each of
    which refuses what exceeds the chunk, uploads, launches and downloads."""
    CHUNK, CHUNK_MIN = PATH_CHUNK, 64
    CHUNK_REFUSAL = "JointPathChecker: a chunk holds at least 64 candidate-samples, one candidate path"
    dtype, prefix = np.float32, "JointPathChecker: "
    roadmap_certify_refusal = "roadmap edges are checked at their samples only, so not by a certifying checker"

    def __init__(self, chain, obstacle_radius: float = 0.06, chunk: Optional[int] = None, device=None, certify: bool = False):
        super().__init__(chain, obstacle_radius, chunk, device)
        K, A, z = self.chunk // 64, self.A, self._zeros      # the most candidates a chunk can hold: S is at least 64
        self.q_start, self.q_goal, self.obstacles = z(K, A), z(K, A), z(K, 3)
        self.vias, self.out = z(K, A), z(K, PATH_FLOATS)
        self.certify = bool(certify)
        if self.certify:
            self.reach = torch.from_numpy(reach_table(chain)).to(self.dev).contiguous()
            self.guard = certificate_guard(chain)
            self.out_cert = z(K, PATH_CERT_FLOATS)
        self.edge_nodes = self.edge_list = self.edge_out = self.edge_obstacles = None
        self.edge_launches = 0

    def _edge_buffers(self, n: int, V: int, E: int) -> None:
        """room for n queries of V nodes and E edges: allocated on the first roadmap call, and again only to grow"""
        if self.edge_nodes is None or self.edge_nodes.numel() < n * V * self.A:
            self.edge_nodes = self._zeros(n * V * self.A)
        if self.edge_obstacles is None or len(self.edge_obstacles) < n:
            self.edge_obstacles = self._zeros(n, 3)
        if self.edge_list is None or len(self.edge_list) < E:
            self.edge_list = self._zeros(E, 2, dtype=torch.int32)
        if self.edge_out is None or len(self.edge_out) < n * E:
            self.edge_out = self._zeros(n * E, EDGE_FLOATS)

    def load_edges(self, nodes, edges, obstacles) -> None:
        """a chunk's roadmaps into the buffers: nodes[n][V][A] (float32), edges[E][2] (int32, shared by the chunk's queries),
        obstacles[n][3]. Every edge is validated here, before the upload: 0 <= i < j < V."""
        nodes, edges = np.ascontiguousarray(nodes, np.float32), np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        n, V = nodes.shape[:2]
        if len(edges) < 1 or not (np.all(edges[:, 0] >= 0) and np.all(edges[:, 0] < edges[:, 1]) and np.all(edges[:, 1] < V)):
            raise ValueError(f"JointPathChecker: every roadmap edge is (i, j) with 0 <= i < j < {V}")
        self._edge_buffers(n, V, len(edges))
        self._upload(self.edge_nodes, nodes.reshape(-1))
        self._upload(self.edge_list, edges, np.int32)
        self._upload(self.edge_obstacles, np.asarray(obstacles, np.float32).reshape(n, 3))

    def launch_edges(self, n: int, V: int, E: int, S: int, margin: float) -> None:
        """the edge launch of one chunk of n roadmaps already in the buffers, on the current stream"""
        check(self.lib.naf_chain_edge_check(self._chain_env, ptr(self.edge_nodes), ptr(self.edge_list), ptr(self.edge_obstacles),
                                            self.obstacle_radius, n, V, E, S, margin, ptr(self.edge_out), None, stream_ptr()),
              "chain_edge_check")
        self.edge_launches += 1

    def launch(self, n: int, C: int, S: int, margin: float) -> None:
        """the launch of one chunk of n queries x C candidates already in the buffers, on the current stream"""
        check(self.lib.naf_chain_path_check(self._chain_env, ptr(self.q_start), ptr(self.q_goal), ptr(self.vias), ptr(self.obstacles),
                                            self.obstacle_radius, n, C, S, margin, ptr(self.out), None, stream_ptr()),
              "chain_path_check")

    def launch_certify(self, n: int, C: int, S: int, margin: float) -> None:
        """the certifying launch of one chunk already in the buffers, into out_cert, on the current stream"""
        check(self.lib.naf_chain_path_certify(self._chain_env, ptr(self.q_start), ptr(self.q_goal), ptr(self.vias), ptr(self.obstacles),
                                              self.obstacle_radius, ptr(self.reach), self.guard, n, C, S, margin, ptr(self.out_cert),
                                              None, stream_ptr()), "chain_path_certify")

    def load(self, q_start, q_goal, obstacles, vias) -> None:
        """a chunk's queries into the buffers: q_start[n][A], q_goal[n][A], obstacles[n][3], vias[n][C][A] (float32)"""
        n, C = vias.shape[:2]
        self._upload(self.q_start, q_start)
        self._upload(self.q_goal, q_goal)
        self._upload(self.obstacles, obstacles)
        self._upload(self.vias, np.asarray(vias, np.float32).reshape(n * C, self.A))

    def prepare(self, q_start, q_goal, obstacles, C: int):
        """the queries as the device takes them, float32; refused when the chunk does not hold one query at the fewest samples"""
        q_start = np.ascontiguousarray(q_start, np.float32).reshape(-1, self.A)
        N = len(q_start)
        q_goal, obstacles = np.ascontiguousarray(q_goal, np.float32).reshape(N, self.A), np.asarray(obstacles, np.float32).reshape(N, 3)
        if 64 * C > self.chunk:
            raise ValueError(f"JointPathChecker: a chunk of {self.chunk} candidate-samples does not hold one query's {C} candidates")
        return q_start, q_goal, obstacles

    def _records(self, launch, out, floats, q_start, q_goal, obstacles, vias, S, margin) -> np.ndarray:
        n, C = vias.shape[:2]
        if n * C * S > self.chunk:
            raise ValueError(f"JointPathChecker: one query's {C} candidates at {S} samples exceed the chunk of {self.chunk}")
        self.load(q_start, q_goal, obstacles, vias)
        launch(n, C, S, float(np.float32(margin)))
        return self._download(out, n * C, n, C, floats)

    def path_records(self, *chunk) -> np.ndarray:
        """records[n][C][PATH_FLOATS] of the chunk (q_start[n], q_goal[n], obstacles[n], vias[n][C], S, margin): one launch"""
        return self._records(self.launch, self.out, PATH_FLOATS, *chunk)

    def certified_records(self, *chunk) -> np.ndarray:
        """records[n][C][PATH_CERT_FLOATS] of the same chunk by the certifying launch"""
        return self._records(self.launch_certify, self.out_cert, PATH_CERT_FLOATS, *chunk)

    def edge_records(self, nodes, edges, obstacles, S, margin) -> np.ndarray:
        """records[n][E][EDGE_FLOATS] of the roadmaps nodes[n][V][A] over edges[E][2] in the scenes obstacles[n]: one launch"""
        n, V, E = len(nodes), nodes.shape[1], len(edges)
        if n * E * S > self.chunk:
            raise ValueError(f"JointPathChecker: one query's {E} roadmap edges at {S} samples exceed the chunk of {self.chunk}")
        self.load_edges(nodes, edges, obstacles)
        self.launch_edges(n, V, E, S, float(np.float32(margin)))
        return self._download(self.edge_out, n * E, n, E, EDGE_FLOATS)

    def check(self, q_start, q_goal, obstacles, candidates: int = 16, resolution: float = 0.02, margin: float = 0.0,
              seed: int = 0, roadmap: int = 0, shortcut: int = 0) -> JointPaths:
        """q_start[N][A], q_goal[N][A] (action order), obstacles[N][3] -> JointPaths of numpy arrays (float32 where the device's).
        roadmap = M in 1 .. 62: the queries that end 'blocked' get a roadmap of M milestones; not with a certifying checker.
        shortcut = W in 4 .. 64 (with roadmap): the 'roadmap' polylines are searched again over W nodes of their own, all pairs
        through the same edge launch (environment.polyline.shortcut_round)."""
        return plan_paths(self, q_start, q_goal, obstacles, candidates, resolution, margin, seed, self.chunk, self.certify, roadmap, shortcut)


def demonstration_chunks(rows_of, budget: int) -> List[Tuple[int, int, int]]:
    """[(first query, queries, T_cap)]: consecutive queries share a chunk, and its T_cap is the largest T_n among them, as long as
    queries x T_cap stays within `budget` rows; a chunk holds at least one query."""
    rows_of = np.asarray(rows_of, np.int64)
    out, first, N = [], 0, len(rows_of)
    while first < N:
        n, T = 1, int(rows_of[first])
        while first + n < N:
            T2 = max(T, int(rows_of[first + n]))
            if (n + 1) * T2 > budget:
                break
            n, T = n + 1, T2
        out.append((first, n, T))
        first += n
    return out


class DemonstrationWriter(TicksLaunch, _ChainTool):
    """Planned joint paths as replay rows on a chain model (csrc/chain_env.hip, "demonstrations"): per chunk of queries ONE
    naf_chain_demo_rows launch that writes every row of every demonstration, then torch plumbing — the mask `t < valid[n] and
    kept[n]` and a boolean index — to a contiguous device tensor of the kept rows in query order, then tick order. Owns the handle
    and staging buffers for `chunk` rows; needs no agent. A demonstration's rows do not depend on where in a launch it lies.
    A plan of two legs of at least one tick each takes that launch; any other plan of K <= 63 legs (demonstration_plan_legs: a
    polyline, 0 ticks for the padding behind a query's last leg) takes naf_chain_demo_rows_legs (chain_legs.LegsLaunch), whose staging
    [chunk][K][A] / [chunk][K] is allocated on the first such call; a tick_demo.TickPlan — one action per tick, a trajectory driven
    at its own ticks — takes naf_chain_demo_rows_ticks (chain_ticks.TicksLaunch), whose staging [chunk rows][A] / [chunk] is
    allocated on the first such call too. Chunks, keep / drop and the gather are the same for all three."""
    CHUNK, CHUNK_MIN, CHUNK_REFUSAL = DEMO_CHUNK, 1, "DemonstrationWriter: a chunk holds at least one row"

    def __init__(self, chain, obstacle_radius: float = 0.06, chunk: Optional[int] = None, device=None):
        super().__init__(chain, obstacle_radius, chunk, device)
        self.row_floats = self.lib.naf_replay_row_floats(2 * self.A + 9, self.A)
        assert self.row_floats == demo_row_layout(self.A)[3]
        K, A, z = self.chunk, self.A, self._zeros             # the most queries a chunk can hold: T_cap is at least 1
        self.q_start, self.leg_actions = z(K, A), z(K, 2, A)
        self.n_ticks = torch.ones(K, 2, dtype=torch.int32, device=self.dev)
        self.targets, self.obstacles = z(K, 3), z(K, 3)
        self.records = z(K, DEMO_FLOATS)
        self.rows = z(self.chunk, self.row_floats)
        self.launches = 0

    def launch(self, n: int, T_cap: int) -> None:
        """the launch of one chunk of n demonstrations already in the buffers, on the current stream"""
        check(self.lib.naf_chain_demo_rows(self._chain_env, ptr(self.q_start), ptr(self.leg_actions), ptr(self.n_ticks), ptr(self.targets),
                                           ptr(self.obstacles), self.obstacle_radius, n, T_cap, ptr(self.rows), self.row_floats,
                                           ptr(self.records), None, stream_ptr()), "chain_demo_rows")
        self.launches += 1

    def load(self, plan, targets, obstacles, sl: slice) -> int:
        self._upload(self.q_start, plan.q_start[sl])
        self._upload(self.leg_actions, plan.leg_actions[sl])
        self._upload(self.n_ticks, plan.n_ticks[sl], np.int32)
        self._upload(self.targets, targets[sl])
        self._upload(self.obstacles, obstacles[sl])
        return sl.stop - sl.start

    def write(self, plan, targets, obstacles, keep_contact: bool = False, has_path=None):
        """plan (environment.kinematic.DemonstrationPlan of N queries), targets[N][3], obstacles[N][3] -> Demonstrations whose `rows`
        is a device tensor [rows_total][row_floats]. has_path[N] (default all): queries without one are launched with whatever
        plan holds for them and reported 'none'."""
        N = len(plan.q_start)
        load, launch = self.entry_for(plan)                   # the two-leg entry, the legs entry or, for a TickPlan, the tick entry
        T_of = np.asarray(plan.rows, np.int64)
        if N and (T_of.min() < 1 or T_of.max() > DEMO_MAX_TICKS):
            raise ValueError(f"DemonstrationWriter: a demonstration holds 1 .. {DEMO_MAX_TICKS} rows")
        if N and T_of.max() > self.chunk:
            raise ValueError(f"DemonstrationWriter: a chunk of {self.chunk} rows does not hold one demonstration of {int(T_of.max())}")
        targets, obstacles = np.asarray(targets, np.float32).reshape(N, 3), np.asarray(obstacles, np.float32).reshape(N, 3)
        has = np.ones(N, bool) if has_path is None else np.asarray(has_path, bool)
        records, parts = np.zeros((N, DEMO_FLOATS), np.float32), []
        for first, n, T_cap in demonstration_chunks(T_of, self.chunk):
            sl = slice(first, first + n)
            load(plan, targets, obstacles, sl)
            launch(n, T_cap)
            records[sl] = self._download(self.records, n)
            # (the staging rows are reused by the next chunk: this chunk's kept rows are taken now)
            parts.append(self._kept_of(self.rows[:n * T_cap].view(n, T_cap, self.row_floats), records[sl], has[sl], keep_contact))
        rows = torch.cat(parts) if parts else torch.zeros(0, self.row_floats, device=self.dev)
        return gather_demonstrations(records, has, lambda kept, valid: rows, keep_contact)._replace(action_size=self.A)

    def _kept_of(self, rows, rec, has, keep_contact):
        """the kept rows of one chunk: gather_demonstrations' keep rule on this chunk's records"""
        box = []
        gather_demonstrations(rec, has, lambda kept, valid: box.append((kept, valid)), keep_contact)
        kept, valid = box[0]
        t = torch.arange(rows.shape[1], device=self.dev)[None, :]
        mask = torch.from_numpy(kept).to(self.dev)[:, None] & (t < torch.from_numpy(valid).to(self.dev)[:, None])
        return rows[mask]

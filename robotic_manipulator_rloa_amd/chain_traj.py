"""TrajectoryChecker: the device backend of environment.trajectory.plan_trajectories (csrc/chain_env.hip, "trajectories"; DESIGN
§27). A chain-model tool in the manner of chain_tools.py — it owns the model's handle and its buffers, needs no agent, no learner and
no graph: per chunk of whole queries ONE naf_chain_traj_check (or naf_chain_traj_certify) launch, one workgroup per trajectory, S
ticks each; eight (twelve) floats per trajectory back, and every tick's pose where the positions are asked for. The schedule, the
chunks and the outcomes are the host's, the same ones the float64 twin runs.

Every launch goes to the stream torch reports as current. An upload is one copy_ on that stream; a download is the one .cpu() that
waits for the launches in front of it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import NafHipError, check, ptr, stream_ptr
from .chain_tools import _ChainTool
from .environment.edge_certificate import polyline_nodes
from .environment.kinematic import certificate_guard, reach_table
from .environment.trajectory import (TRAJ_CERT_FLOATS, TRAJ_CHUNK, TRAJ_FLOATS, TRAJ_NODES_MAX, TRAJ_SAMPLES_MAX, TRAJ_SAMPLES_MIN,
                                     DeviceSchedule, Trajectories, plan_trajectories)

CHAIN_ERR_LDS = -20                   # NAF_CHAIN_ERR_LDS


class TrajectoryLdsRefusal(NafHipError):
    """naf_chain_traj_certify answered NAF_CHAIN_ERR_LDS: the table and the second reduction row do not fit beside the arm's rows"""


class TrajectoryChecker(_ChainTool):
    """Trajectories on a chain model. Every buffer is allocated on the first use and again only to grow; the reach table is uploaded
    on the first certifying call (reach_table refuses a prismatic joint without limits there). A chunk holds at most `chunk` samples
    (queries x S, whole queries); a trajectory's record and poses do not depend on where in a launch it lies."""
    CHUNK, CHUNK_MIN = TRAJ_CHUNK, TRAJ_SAMPLES_MIN
    CHUNK_REFUSAL = "TrajectoryChecker: a chunk holds at least 64 samples, one trajectory's launch"
    dtype = np.float32

    def __init__(self, chain, obstacle_radius: float = 0.06, chunk: Optional[int] = None, device=None):
        super().__init__(chain, obstacle_radius, chunk, device)
        self.nodes = self.times = self.vpeak = self.n_nodes = self.n_samples = self.obstacles = self.out = self.poses = None
        self.reach, self.guard = None, None
        self.launches = 0

    def _buffers(self, n: int, V: int, S: int, positions: bool) -> None:
        A = self.A
        if self.nodes is None or self.nodes.numel() < n * V * A:
            self.nodes, self.times = self._zeros(n * V * A), self._zeros(n * V * 3)
        if self.vpeak is None or len(self.vpeak) < n:
            self.vpeak, self.obstacles, self.out = self._zeros(n, A), self._zeros(n, 3), self._zeros(n, TRAJ_CERT_FLOATS)
            self.n_nodes, self.n_samples = self._zeros(n, dtype=torch.int32), self._zeros(n, dtype=torch.int32)
        if positions and (self.poses is None or self.poses.numel() < n * S * A):
            self.poses = self._zeros(n * S * A)

    def load(self, ds: DeviceSchedule, obstacles, S: int) -> None:
        """a chunk's schedule into the buffers; the counts are validated here, before the upload"""
        n, V = ds.nodes.shape[:2]
        if not (2 <= V <= TRAJ_NODES_MAX) or not (np.all(ds.n_nodes >= 1) and np.all(ds.n_nodes <= V)):
            raise ValueError(f"TrajectoryChecker: a trajectory has 1 .. V nodes, V in 2 .. {TRAJ_NODES_MAX}")
        if not (np.all(ds.n_samples >= 1) and np.all(ds.n_samples <= S)):
            raise ValueError(f"TrajectoryChecker: a trajectory has 1 .. {S} samples in a launch of {S}")
        if not np.all(np.isfinite(ds.times)) or not np.all(np.isfinite(ds.nodes)) or not np.all(np.isfinite(ds.vpeak)):
            raise ValueError("TrajectoryChecker: the schedule holds finite numbers")
        self._upload(self.nodes, ds.nodes.reshape(-1))
        self._upload(self.times, ds.times.reshape(-1))
        self._upload(self.vpeak, ds.vpeak)
        self._upload(self.n_nodes, ds.n_nodes, np.int32)
        self._upload(self.n_samples, ds.n_samples, np.int32)
        self._upload(self.obstacles, np.asarray(obstacles, np.float32).reshape(n, 3))

    def launch(self, n: int, V: int, S: int, dt: float, margin: float, certify: bool, positions: bool) -> None:
        """the launch of one chunk of n trajectories already in the buffers, on the current stream"""
        poses = ptr(self.poses) if positions else None
        if certify:
            code = self.lib.naf_chain_traj_certify(self._chain_env, ptr(self.nodes), ptr(self.n_nodes), ptr(self.times), ptr(self.vpeak),
                                                   ptr(self.n_samples), ptr(self.obstacles), self.obstacle_radius, ptr(self.reach),
                                                   self.guard, dt, n, V, S, margin, ptr(self.out), poses, stream_ptr())
            if code == CHAIN_ERR_LDS:
                raise TrajectoryLdsRefusal("chain_traj_certify: the table of half-steps and the second reduction row do not fit a "
                                           "workgroup's LDS beside this arm's capsule rows")
            check(code, "chain_traj_certify")
        else:
            check(self.lib.naf_chain_traj_check(self._chain_env, ptr(self.nodes), ptr(self.n_nodes), ptr(self.times), ptr(self.vpeak),
                                                ptr(self.n_samples), ptr(self.obstacles), self.obstacle_radius, dt, n, V, S, margin,
                                                ptr(self.out), poses, stream_ptr()), "chain_traj_check")
        self.launches += 1

    def records(self, ds: DeviceSchedule, obstacles, S: int, margin: float, certify: bool, positions: bool):
        """plan_trajectories' evaluator: (records[n][8 | 12], poses[n][S][A] | None) of one chunk, float32: one launch"""
        n, V = ds.nodes.shape[:2]
        if S % 64 or not (TRAJ_SAMPLES_MIN <= S <= TRAJ_SAMPLES_MAX):
            raise ValueError(f"TrajectoryChecker: S is a multiple of 64 from {TRAJ_SAMPLES_MIN} to {TRAJ_SAMPLES_MAX}: got {S!r}")
        if n * S > self.chunk and n > 1:
            raise ValueError(f"TrajectoryChecker: {n} trajectories at {S} samples exceed the chunk of {self.chunk}")
        if certify and self.reach is None:
            self.reach = torch.from_numpy(reach_table(self.chain)).to(self.dev).contiguous()
            self.guard = certificate_guard(self.chain)
        self._buffers(n, V, S, positions)
        self.load(ds, obstacles, S)
        self.launch(n, V, int(S), float(np.float32(ds.dt)), float(np.float32(margin)), bool(certify), bool(positions))
        floats = TRAJ_CERT_FLOATS if certify else TRAJ_FLOATS
        rec = self._download(self.out.view(-1), n * floats, n, floats)      # (the records lie packed at the buffer's front)
        return rec,(self._download(self.poses, n * S * self.A, n, S, self.A) if positions else None)

    def plan(self, paths, obstacles, vmax, amax, dt: float, certify: bool = False, margin: float = 0.0,
             positions: bool = True) -> Trajectories:
        """paths (JointPaths of N queries), obstacles[N][3], vmax[A], amax[A] -> Trajectories of numpy arrays, float32 where the device's"""
        nodes, count = polyline_nodes(paths)
        ob = np.asarray(obstacles, np.float32).reshape(len(count), 3)
        return plan_trajectories(self, nodes, count, ob, vmax, amax, dt, certify, float(np.float32(margin)), positions, self.chunk)

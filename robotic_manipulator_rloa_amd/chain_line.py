"""LineTracker: the device tracker of environment.line_moves.plan_line_moves (csrc/chain_env.hip, "line moves"). A
chain-model tool in the manner of chain_tools.py — it owns the model's handle and its buffers, needs no agent, no learner and no
graph: per chunk of queries ONE naf_chain_line_track launch, W + 1 nodes and W records of four floats per query back. The verdict,
the collision check of the legs (chain_tools.JointPathChecker.edge_records) and the outcomes are the host's, the same ones the
float64 twin runs.

Every launch goes to the stream torch reports as current. An upload is one copy_ on that stream; a download is the one .cpu() that
waits for the launches in front of it.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _lib
from ._lib import NafHipError, check, ptr, stream_ptr
from .chain_tools import _ChainTool
from .environment.line_moves import TRACK_FLOATS, line_constants, line_updates_ok, line_waypoints_ok

CHAIN_ERR_LDS = -20                   # NAF_CHAIN_ERR_LDS


class LineLdsRefusal(NafHipError):
    """naf_chain_line_track answered NAF_CHAIN_ERR_LDS: the walked joints' records do not fit a workgroup's LDS"""


class LineTracker(_ChainTool):
    """Tracked Cartesian lines on a chain model. A chunk holds at most `chunk` queries; a query's nodes and records do not depend
    on the chunk or the lane it lands in. The buffers are allocated on the first use and again only to grow."""
    CHUNK, CHUNK_MIN, CHUNK_REFUSAL = 16384, 1, "LineTracker: a chunk holds at least one query"

    def __init__(self, chain, obstacle_radius: float = 0.06, chunk: Optional[int] = None, device=None):
        super().__init__(chain, obstacle_radius, chunk, device)
        self.q_start = self.disp = self.nodes = self.out = None
        self.launches = 0

    def _buffers(self, n: int, W: int) -> None:
        if self.q_start is None or len(self.q_start) < n:
            self.q_start, self.disp = self._zeros(n, self.A), self._zeros(n, 3)
        if self.nodes is None or self.nodes.numel() < n * (W + 1) * self.A:
            self.nodes = self._zeros(n * (W + 1) * self.A)
        if self.out is None or self.out.numel() < n * W * TRACK_FLOATS:
            self.out = self._zeros(n * W * TRACK_FLOATS)

    def params(self, constants: dict, tool_axis, tool_normal) -> Tuple["_lib.IkParams", "_lib.IkPoseParams"]:
        """(naf_chain_ik_params_t, naf_chain_ik_pose_params_t) of line_constants' values; iterations and angle_length are not read"""
        f3 = ctypes.c_float * 3
        c = constants
        return (_lib.IkParams(0, c["lam2"], c["e_max"], c["dq_max"]),
                _lib.IkPoseParams(c["weight"], c["w_max"], 1.0, f3(*map(float, tool_axis)), f3(*map(float, tool_normal))))

    def load(self, q_start, disp) -> None:
        """a chunk's queries into the buffers: q_start[n][A], disp[n][3] (float32)"""
        self._upload(self.q_start, q_start)
        self._upload(self.disp, disp)

    def launch(self, n: int, mode: int, W: int, U: int, prm, pose) -> None:
        """the launch of one chunk of n queries already in the buffers, on the current stream"""
        code = self.lib.naf_chain_line_track(self._chain_env, ptr(self.q_start), ptr(self.disp), int(mode), n, W, U, prm, pose,
                                             ptr(self.nodes), ptr(self.out), None, stream_ptr())
        if code == CHAIN_ERR_LDS:
            raise LineLdsRefusal("chain_line_track: the records of this arm's walked joints do not fit a workgroup's LDS")
        check(code, "chain_line_track")
        self.launches += 1

    def track(self, q_start, disp, mode: int, W: int, U: int, constants: Optional[dict] = None, tool_axis=(0.0, 0.0, 1.0),
              tool_normal=(1.0, 0.0, 0.0)) -> Tuple[np.ndarray, np.ndarray]:
        """q_start[N][A] (action order), disp[N][3] -> (nodes[N][W + 1][A], track[N][W][4]), float32, chunked over the queries"""
        if not line_waypoints_ok(W) or not line_updates_ok(W, U):
            raise ValueError(f"LineTracker: W is 1 .. 63 waypoints of U >= 1 updates, W U <= 4096: got {W!r}, {U!r}")
        A, W, U = self.A, int(W), int(U)
        q_start = np.ascontiguousarray(q_start, np.float32).reshape(-1, A)
        N = len(q_start)
        disp = np.ascontiguousarray(disp, np.float32).reshape(N, 3)
        prm, pose = self.params(line_constants(self.chain) if constants is None else constants, tool_axis, tool_normal)
        nodes, track = np.empty((N, W + 1, A), np.float32), np.empty((N, W, TRACK_FLOATS), np.float32)
        for first in range(0, N, self.chunk):
            n = min(self.chunk, N - first)
            sl = slice(first, first + n)
            self._buffers(n, W)
            self.load(q_start[sl], disp[sl])
            self.launch(n, mode, W, U, prm, pose)
            nodes[sl] = self._download(self.nodes, n * (W + 1) * A, n, W + 1, A)
            track[sl] = self._download(self.out, n * W * TRACK_FLOATS, n, W, TRACK_FLOATS)
        return nodes, track

"""PolylineCertifier: the device backend of environment.edge_certificate.certify_polylines (csrc/chain_env.hip, "roadmap edges"; DESIGN
§23). A chain-model tool in the manner of chain_tools.py — it owns the model's handle and its buffers, needs no agent, no learner
and no graph — that certifies the polylines of a JointPaths between their samples: per chunk of whole queries ONE
naf_chain_edge_certify launch over queries x legs, S samples each, twelve floats per leg back; the rounds and the verdicts are the
host's, the same ones the float64 twin runs (certify_polylines_host).

Every launch goes to the stream torch reports as current. An upload is one copy_ on that stream; a download is the one .cpu() that
waits for the launches in front of it.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import NafHipError, check, ptr, stream_ptr
from .chain_tools import _ChainTool
from .environment.edge_certificate import EDGE_CERT_FLOATS, PathCertificates, certify_polylines, polyline_nodes
from .environment.kinematic import PATH_CHUNK, certificate_guard, reach_table

CHAIN_ERR_LDS = -20                   # NAF_CHAIN_ERR_LDS


class PolylineLdsRefusal(NafHipError):
    """naf_chain_edge_certify answered NAF_CHAIN_ERR_LDS: the table and the second reduction row do not fit beside the arm's rows"""


class PolylineCertifier(_ChainTool):
    """Certificates for polylines on a chain model. The model's reach table is uploaded once, when the tool is built (a model with a
    prismatic joint that has no limits is refused there by reach_table); the node, edge, obstacle and record buffers are allocated
    on the first call and again only to grow. A chunk holds at most `chunk` edge-samples (queries x legs x S, whole queries); a
    leg's record does not depend on where in a launch it lies. The evaluator `edge_records` refuses what exceeds the chunk, uploads,
    launches and downloads. The certifying launch keeps the handle's lanes and adds a reduction row and one small table to its
    LDS: an arm with pairs whose rows only just fit a workgroup is refused (PolylineLdsRefusal) and certify_polylines_host answers it."""
    CHUNK, CHUNK_MIN = PATH_CHUNK, 64
    CHUNK_REFUSAL = "PolylineCertifier: a chunk holds at least 64 edge-samples, one leg"

    def __init__(self, chain, obstacle_radius: float = 0.06, chunk: Optional[int] = None, device=None):
        reach = reach_table(chain)                            # (refuses before anything is created on the device)
        super().__init__(chain, obstacle_radius, chunk, device)
        self.reach = torch.from_numpy(reach).to(self.dev).contiguous()
        self.guard = certificate_guard(chain)
        self.nodes = self.edges = self.obstacles = self.out = None
        self.launches = 0

    def _buffers(self, n: int, V: int, E: int) -> None:
        """room for n queries of V nodes and E edges: allocated on the first call, and again only to grow"""
        if self.nodes is None or self.nodes.numel() < n * V * self.A:
            self.nodes = self._zeros(n * V * self.A)
        if self.obstacles is None or len(self.obstacles) < n:
            self.obstacles = self._zeros(n, 3)
        if self.edges is None or len(self.edges) < E:
            self.edges = self._zeros(E, 2, dtype=torch.int32)
        if self.out is None or len(self.out) < n * E:
            self.out = self._zeros(n * E, EDGE_CERT_FLOATS)

    def launch(self, n: int, V: int, E: int, S: int, margin: float) -> None:
        """the certifying launch of one chunk of n polylines already in the buffers, on the current stream"""
        code = self.lib.naf_chain_edge_certify(self._chain_env, ptr(self.nodes), ptr(self.edges), ptr(self.obstacles),
                                               self.obstacle_radius, ptr(self.reach), self.guard, n, V, E, S, margin, ptr(self.out),
                                               None, stream_ptr())
        if code == CHAIN_ERR_LDS:
            raise PolylineLdsRefusal("chain_edge_certify: the table of half-steps and the second reduction row do not fit a "
                                     "workgroup's LDS beside this arm's capsule rows")
        check(code, "chain_edge_certify")
        self.launches += 1

    def edge_records(self, nodes, edges, obstacles, S: int, margin: float) -> np.ndarray:
        """records[n][E][EDGE_CERT_FLOATS] of the polylines nodes[n][K][A] over edges[E][2] in the scenes obstacles[n]: one launch"""
        nodes, edges = np.ascontiguousarray(nodes, np.float32), np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        n, V, E = len(nodes), nodes.shape[1], len(edges)
        if E < 1 or not (np.all(edges[:, 0] >= 0) and np.all(edges[:, 0] < edges[:, 1]) and np.all(edges[:, 1] < V)):
            raise ValueError(f"PolylineCertifier: every leg is (i, j) with 0 <= i < j < {V}")
        if n * E * S > self.chunk:
            raise ValueError(f"PolylineCertifier: one query's {E} legs at {S} samples exceed the chunk of {self.chunk}")
        self._buffers(n, V, E)
        self._upload(self.nodes, nodes.reshape(-1))
        self._upload(self.edges, edges, np.int32)
        self._upload(self.obstacles, np.asarray(obstacles, np.float32).reshape(n, 3))
        self.launch(n, V, E, int(S), float(np.float32(margin)))
        return self._download(self.out, n * E, n, E, EDGE_CERT_FLOATS)

    def certify(self, paths, obstacles, margin: float = 0.0, resolution: float = 0.02) -> PathCertificates:
        """paths (JointPaths of N queries), obstacles[N][3] -> PathCertificates of numpy arrays, float32 where the device's"""
        nodes, count = polyline_nodes(paths)
        ob = np.asarray(obstacles, np.float32).reshape(len(count), 3)

        def run(queries, nodes32, edges, S):
            return self.edge_records(nodes32, edges, ob[queries], S, margin)

        return certify_polylines(run, nodes, count, resolution, self.chunk, np.float32)

"""The K-leg side of chain_tools.DemonstrationWriter (csrc/chain_env.hip, "demonstrations along polylines of any number of legs"):
which of the two entries a plan takes, and the staging and the launch of naf_chain_demo_rows_legs. A mixin: it uses the writer's
handle, its buffers for start poses, scenes, rows and records, and _ChainTool's upload helper, and knows nothing else of chain_tools.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, ptr, stream_ptr
from .environment.kinematic import DEMO_MAX_LEGS


class LegsLaunch:
    legs_actions = legs_ticks = None      # [chunk][K][A] / [chunk][K] on the device: allocated on the first K-leg plan
    legs_launches = 0

    def entry_for(self, plan):
        """(load, launch) for `plan` (environment.kinematic.DemonstrationPlan of N queries), after its refusals. Two legs of at least
        one tick each: the writer's own load and launch, naf_chain_demo_rows as ever. Any other plan of K <= 63 legs
        (demonstration_plan_legs: 0 ticks for the padding behind a query's last leg): load_legs and naf_chain_demo_rows_legs."""
        N, ticks = len(plan.q_start), np.asarray(plan.n_ticks)
        if ticks.ndim == 2 and ticks.shape == (N, 2) and (not N or ticks.min() >= 1):
            return self.load, self.launch
        K = ticks.shape[1] if ticks.ndim == 2 else 0
        if ticks.shape != (N, K) or not 1 <= K <= DEMO_MAX_LEGS or np.asarray(plan.leg_actions).shape != (N, K, self.A):
            raise ValueError(f"DemonstrationWriter: a plan holds n_ticks[N][K] and leg_actions[N][K][A], K from 1 to {DEMO_MAX_LEGS}")
        real = ticks > 0
        if N and (ticks.min() < 0 or not real[:, 0].all() or (real[:, 1:] & ~real[:, :-1]).any()):
            raise ValueError("DemonstrationWriter: every leg of a plan takes at least one tick, and the padding of 0 ticks lies "
                             "behind a query's last leg")
        return self.load_legs, lambda n, T_cap: self.launch_legs(n, K, T_cap)

    def _legs_buffers(self, n: int, K: int) -> None:
        """room for n demonstrations of K legs: allocated on the first K-leg call, and again only to grow"""
        if self.legs_actions is None or self.legs_actions.numel() < n * K * self.A:
            self.legs_actions = self._zeros(n * K * self.A)
        if self.legs_ticks is None or self.legs_ticks.numel() < n * K:
            self.legs_ticks = self._zeros(n * K, dtype=torch.int32)

    def load_legs(self, plan, targets, obstacles, sl: slice) -> int:
        """a chunk's demonstrations of K legs into the buffers, as the writer's load() takes a chunk of two-leg ones"""
        n, K = plan.n_ticks[sl].shape
        self._legs_buffers(n, K)
        self._upload(self.q_start, plan.q_start[sl])
        self._upload(self.legs_actions, np.asarray(plan.leg_actions[sl], np.float32).reshape(-1))
        self._upload(self.legs_ticks, np.asarray(plan.n_ticks[sl], np.int32).reshape(-1), np.int32)
        self._upload(self.targets, targets[sl])
        self._upload(self.obstacles, obstacles[sl])
        return n

    def launch_legs(self, n: int, K: int, T_cap: int) -> None:
        """the launch of one chunk of n demonstrations of K legs already in the legs' buffers, on the current stream"""
        check(self.lib.naf_chain_demo_rows_legs(self._chain_env, ptr(self.q_start), ptr(self.legs_actions), ptr(self.legs_ticks), K,
                                                ptr(self.targets), ptr(self.obstacles), self.obstacle_radius, n, T_cap, ptr(self.rows),
                                                self.row_floats, ptr(self.records), None, stream_ptr()), "chain_demo_rows_legs")
        self.legs_launches += 1

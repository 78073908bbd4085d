"""The per-tick side of chain_tools.DemonstrationWriter (csrc/chain_env.hip, "demonstrations under one action per tick"): the third
entry a plan can take, and the staging and the launch of naf_chain_demo_rows_ticks. A mixin that extends chain_legs.LegsLaunch: a
tick_demo.TickPlan takes this entry, every other plan goes on to the two entries LegsLaunch chooses from. It uses the writer's
handle, its buffers for start poses, scenes, rows and records, and _ChainTool's upload helper, and knows nothing else of chain_tools.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import check, ptr, stream_ptr
from .chain_legs import LegsLaunch
from .environment.tick_demo import is_tick_plan


class TicksLaunch(LegsLaunch):
    tick_actions = tick_counts = None     # [chunk rows][A] / [chunk] on the device: allocated on the first TickPlan
    ticks_launches = 0

    def entry_for(self, plan):
        """(load, launch) for `plan`, after its refusals: a TickPlan takes load_ticks and naf_chain_demo_rows_ticks, any other plan
        what LegsLaunch.entry_for says"""
        if not is_tick_plan(plan):
            return super().entry_for(plan)
        N = len(plan.q_start)
        acts, ticks, rows = np.asarray(plan.actions), np.asarray(plan.planned_ticks), np.asarray(plan.rows)
        if acts.ndim != 3 or acts.shape[0] != N or acts.shape[2] != self.A or ticks.shape != (N,) or rows.shape != (N,):
            raise ValueError(f"DemonstrationWriter: a tick plan holds actions[N][T][{self.A}], planned_ticks[N] and rows[N]")
        if N and (ticks.min() < 1 or np.any(rows > ticks) or rows.max() > acts.shape[1] or not np.all(np.isfinite(acts))):
            raise ValueError("DemonstrationWriter: every demonstration of a tick plan plans at least one tick, its rows are at most "
                             "its planned ticks and the width of the table, and every action is finite")
        return self.load_ticks, self.launch_ticks

    def load_ticks(self, plan, targets, obstacles, sl: slice) -> int:
        """a chunk's demonstrations into the buffers: the table as [n][T_cap][A] with T_cap the chunk's largest row count
        (demonstration_chunks' T_cap), zeros behind a demonstration's own rows"""
        n = sl.stop - sl.start
        T_cap = int(np.max(plan.rows[sl]))
        if self.tick_actions is None:
            self.tick_actions = self._zeros(self.chunk, self.A)
            self.tick_counts = self._zeros(self.chunk, dtype=torch.int32)
        table = np.zeros((n, T_cap, self.A), np.float32)
        width = min(T_cap, plan.actions.shape[1])
        table[:, :width] = np.asarray(plan.actions[sl], np.float32)[:, :width]
        self._upload(self.q_start, plan.q_start[sl])
        self._upload(self.tick_actions, table.reshape(n * T_cap, self.A))
        self._upload(self.tick_counts, np.minimum(np.asarray(plan.planned_ticks[sl], np.int64), 1 << 20).astype(np.int32), np.int32)
        self._upload(self.targets, targets[sl])
        self._upload(self.obstacles, obstacles[sl])
        return n

    def launch_ticks(self, n: int, T_cap: int) -> None:
        """the launch of one chunk of n demonstrations already in the tick buffers, on the current stream"""
        check(self.lib.naf_chain_demo_rows_ticks(self._chain_env, ptr(self.q_start), ptr(self.tick_actions), ptr(self.tick_counts),
                                                 ptr(self.targets), ptr(self.obstacles), self.obstacle_radius, n, T_cap, ptr(self.rows),
                                                 self.row_floats, ptr(self.records), None, stream_ptr()), "chain_demo_rows_ticks")
        self.ticks_launches += 1

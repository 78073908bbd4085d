"""Trajectories as demonstrations, stated once in float64 as environment/kinematic.py states the rest: the table of
one action per tick that drives the arm along a time-parameterised trajectory (environment/trajectory.py) at the environment's own
ticks, and the host's float32 restatement of where the arm then is. numpy only.

THE RULE. Tick i has the time t_i = i DT, DT the environment's tick whatever the trajectory was checked at. Q_i is the float64 law
of the trajectory's schedule at t_i (Trajectories.at); planned_ticks = max(1, ceil(D / DT)), and Q_i = P_K exactly for every
i >= planned_ticks. p_0 = float32(P_0) inside the limits. With feedback the action of tick i aims at Q_{i+1} from where the arm IS:
    a_i = clamp(float32((Q_{i+1} - p_i) / dt32), -1, 1)        p_{i+1} = limits(float32(dt32 a_i + p_i))
dt32 the float32 value the step kernel multiplies by, the sum formed in float64 from the exact product and rounded once — the
fused step of the device (tests/chain_demo_common.poses32). Without feedback a_i = clamp(float32((Q_{i+1} - Q_i) / dt32), -1, 1),
the open-loop form, whose roundings add up. The clamp is the bound of the policy's tanh, not max_velocity.

THE TRACKING BOUND (derived in DESIGN §28). With r = 1/2 ulp32(max |q|) + 1/2 DT ulp32(1): a tick whose action is not clamped ends
within r of Q_{i+1} whatever the error before it; a clamped tick adds at most r to the error before it, because the law moves at
most DT per tick; hence |p_i - Q_i| <= r (1 + the longest run of clamped ticks).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from .urdf_chain import DT


class TickPlan(NamedTuple):
    """One action per tick for N demonstrations: all naf_chain_demo_rows_ticks sees of them, and what the rule measured"""
    q_start: np.ndarray                         # [N][A] float32: the start poses
    actions: np.ndarray                         # [N][T][A] float32: a_i; zeros behind a query's own rows
    planned_ticks: np.ndarray                   # [N] int64: ticks to the trajectory's end, >= 1
    rows: np.ndarray                            # [N] int64: min(planned_ticks, frames)
    tracking_error: Optional[np.ndarray] = None     # [N]: max over the demonstration's ticks and joints of |p_i - Q_i|
    saturated_ticks: Optional[np.ndarray] = None    # [N] int64: ticks with a clamped component
    peak_action: Optional[np.ndarray] = None        # [N]: max |a_i| over the demonstration's ticks
    saturated_run: Optional[np.ndarray] = None      # [N] int64: the longest run of consecutive clamped ticks
    pose_scale: Optional[np.ndarray] = None         # [N]: max |q| over the host recurrence's poses and the law's


def is_tick_plan(plan) -> bool:
    return hasattr(plan, "actions") and hasattr(plan, "planned_ticks")


def tracking_radius(pose_scale) -> np.ndarray:
    """r of the tracking bound for poses up to pose_scale in magnitude: 1/2 ulp32(max |q|) + 1/2 DT ulp32(1)"""
    scale = np.asarray(pose_scale, np.float64).astype(np.float32)
    return 0.5 * np.spacing(np.abs(scale)).astype(np.float64) + 0.5 * DT * float(np.spacing(np.float32(1.0)))


def tracking_bound(plan: TickPlan) -> np.ndarray:
    """[N]: r (1 + the longest saturated run), the bound on plan.tracking_error"""
    return tracking_radius(plan.pose_scale) * (1.0 + np.asarray(plan.saturated_run, np.float64))


def tick_recurrence(q_start, law, limits=None, feedback: bool = True):
    """(actions[N][T][A] float32, poses[N][T + 1][A] float32, clamped[N][T] bool) of the rule above for law[N][T + 1][A] (float64,
    Q_0 .. Q_T) from q_start[N][A]; limits = (lo[A], hi[A]) or None for an arm without"""
    Q = np.asarray(law, np.float64)
    N, T1, A = Q.shape
    T = T1 - 1
    dt32 = np.float64(np.float32(DT))
    lo, hi = (np.full(A, -np.inf, np.float32), np.full(A, np.inf, np.float32)) if limits is None else \
        (np.asarray(limits[0]).astype(np.float32), np.asarray(limits[1]).astype(np.float32))
    p = np.minimum(np.maximum(np.asarray(q_start, np.float32), lo), hi)
    actions, poses, clamped = np.zeros((N, T, A), np.float32), np.empty((N, T1, A), np.float32), np.zeros((N, T), bool)
    poses[:, 0] = p
    for i in range(T):
        raw = ((Q[:, i + 1] - (p.astype(np.float64) if feedback else Q[:, i])) / dt32).astype(np.float32)
        a = np.minimum(np.maximum(raw, np.float32(-1.0)), np.float32(1.0))
        clamped[:, i] = np.any(a != raw, axis=1)
        p = np.minimum(np.maximum((dt32 * a.astype(np.float64) + p.astype(np.float64)).astype(np.float32), lo), hi)
        actions[:, i], poses[:, i + 1] = a, p
    return actions, poses, clamped


def longest_run(flags) -> np.ndarray:
    """[N] int64: the longest run of consecutive True in flags[N][T]"""
    flags = np.asarray(flags, bool)
    best, run = np.zeros(len(flags), np.int64), np.zeros(len(flags), np.int64)
    for i in range(flags.shape[1]):
        run = np.where(flags[:, i], run + 1, 0)
        best = np.maximum(best, run)
    return best


def trajectory_tick_plan(traj, frames: int = 400, feedback: bool = True, limits=None, stand_still=None) -> TickPlan:
    """The TickPlan of `traj` (environment.trajectory.Trajectories of N queries) under the rule above, its diagnostics filled.
    limits = (lo[A], hi[A]) of the arm (a trajectory's nodes lie inside them and a blend stays between its nodes, so the limits
    never clip the law itself); stand_still[A]: where a query without a trajectory (outcome 'none') stands for its one tick at
    action 0 — zeros unless given. Refused by name: a peak velocity above 1 on any joint (the action's bound), frames outside
    1 .. DEMO_MAX_TICKS, and limits or stand_still of another joint count."""
    from .kinematic import DEMO_MAX_TICKS
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or not 1 <= frames <= DEMO_MAX_TICKS:
        raise ValueError(f"frames is a number of steps from 1 to {DEMO_MAX_TICKS}: got {frames!r}")
    count = np.asarray(traj.n_nodes, np.int64)
    N, A = len(count), np.asarray(traj.peak_velocity).shape[-1]
    for name, v in (("limits", None if limits is None else limits[0]), ("stand_still", stand_still)):
        if v is not None and np.asarray(v).shape != (A,):
            raise ValueError(f"{name} holds {np.asarray(v).shape[-1] if np.asarray(v).ndim else 0} joints, the trajectories have {A}")
    has = (count >= 1) & (np.asarray(traj.outcome) != "none")
    peak = np.where(has[:, None], np.asarray(traj.peak_velocity, np.float64), 0.0)
    if N and np.nanmax(peak, initial=0.0) > 1.0 + 1e-9:
        n, m = np.unravel_index(int(np.nanargmax(peak)), peak.shape)
        raise ValueError(f"trajectory_tick_plan: query {int(n)} moves joint {int(m)} at {float(peak[n, m]):.6g} per second, above the "
                         f"unit action: plan the trajectories with max_velocity <= 1")
    D = np.where(has, np.asarray(traj.duration, np.float64), 0.0)
    planned = np.maximum(1, np.ceil(D / DT)).astype(np.int64)
    rows = np.minimum(planned, int(frames))
    T = int(rows.max()) if N else 1
    Q = np.asarray(traj.at(np.arange(T + 1) * DT), np.float64) if N else np.zeros((0, T + 1, A))
    nodes = np.asarray(traj.nodes, np.float64)
    still = np.zeros(A) if stand_still is None else np.asarray(stand_still, np.float32).astype(np.float64)      # (as float32 holds it)
    first = np.where(has[:, None], nodes[np.arange(N), 0] if nodes.shape[1] else still, still)
    last = np.where(has[:, None], nodes[np.arange(N), np.maximum(count - 1, 0)] if nodes.shape[1] else still, still)
    Q = np.where(has[:, None, None], Q, first[:, None, :])
    Q = np.where((np.arange(T + 1)[None, :] >= planned[:, None])[..., None], last[:, None, :], Q)      # P_K exactly at and beyond D
    return tick_plan_from_law(first, Q, planned, rows, limits, feedback)


def tick_plan_from_law(q_start, law, planned, rows, limits=None, feedback: bool = True) -> TickPlan:
    """the TickPlan and its diagnostics for law[N][T + 1][A] (float64: Q_0 .. Q_T, T >= max rows) from q_start[N][A], with
    planned[N] ticks to the law's end and rows[N] = min(planned, frames)"""
    Q = np.asarray(law, np.float64)
    N, T = Q.shape[0], Q.shape[1] - 1
    planned, rows = np.asarray(planned, np.int64), np.asarray(rows, np.int64)
    actions, poses, clamped = tick_recurrence(np.asarray(q_start, np.float32), Q, limits, feedback)
    live = np.arange(T)[None, :] < rows[:, None]
    upto = np.arange(T + 1)[None, :] <= rows[:, None]
    actions = np.where(live[..., None], actions, np.float32(0.0))
    clamped &= live
    err = np.abs(poses.astype(np.float64) - Q).max(axis=2)
    scale = np.maximum(np.abs(poses.astype(np.float64)).max(axis=2), np.abs(Q).max(axis=2))
    return TickPlan(poses[:, 0].copy(), actions, planned, rows, np.where(upto, err, 0.0).max(axis=1), clamped.sum(axis=1),
                    np.abs(actions).max(axis=(1, 2)).astype(np.float64) if T else np.zeros(N), longest_run(clamped),
                    np.where(upto, scale, 0.0).max(axis=1))


def plan_source(plan, frames: int):
    """(planned[N] int64, T_n[N] = min(planned, frames), T = max T_n, actions[N][T][A] float64) of a DemonstrationPlan — the sum of its
    legs' ticks and demo_actions — or of a TickPlan, its own table (0 behind its width: never used): what demonstration_rows_host reads"""
    from .kinematic import demo_actions
    tick = is_tick_plan(plan)
    planned = np.asarray(plan.planned_ticks, np.int64) if tick else np.asarray(plan.n_ticks).astype(np.int64).sum(axis=1)
    Tn = np.minimum(planned, int(frames))
    T = int(Tn.max()) if len(planned) else 1
    if not tick:
        return planned, Tn, T, demo_actions(plan, T)
    table = np.asarray(plan.actions, np.float64)
    actions = np.zeros((table.shape[0], T, table.shape[2]))
    actions[:, :min(T, table.shape[1])] = table[:, :T]
    return planned, Tn, T, actions


def tick_plan_of(plan, T: int) -> TickPlan:
    """the TickPlan that applies, tick by tick, what a DemonstrationPlan of two or K legs applies: demo_actions(plan, T) as float32
    and the sum of its counts"""
    from .kinematic import demo_actions
    ticks = np.asarray(plan.n_ticks, np.int64).sum(axis=1)
    return TickPlan(np.asarray(plan.q_start, np.float32), demo_actions(plan, int(T)).astype(np.float32), ticks, np.minimum(ticks, int(T)))

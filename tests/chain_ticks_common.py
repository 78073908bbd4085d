"""Shared by tests/test_chain_ticks_cpu.py and tests/test_chain_ticks_gpu.py: the cases that hold naf_chain_demo_rows_ticks
(csrc/chain_env.hip) against the float64 rule (environment/tick_demo.py, kinematic.demonstration_rows_host), built with the twin
alone as chain_demo_common builds its own. A case here is a chain_demo_common case in everything its helpers read — `plan`, scenes,
host() — so that rows32, poses32, margins_at, band_of and check_rows serve it as they stand: `plan` is the table seen as a plan of
one leg per tick (demo_actions of it IS the table, and the sum of its counts the planned ticks), and `tick_plan` is the TickPlan the
entry point and the writer are given. The actions are a two-leg blended trajectory's, with feedback."""
import functools

import numpy as np

import chain_demo_common as D
import chain_rollout_common as C

from robotic_manipulator_rloa_amd.environment import tick_demo as K
from robotic_manipulator_rloa_amd.environment import trajectory as T
from robotic_manipulator_rloa_amd.environment.kinematic import (DemonstrationPlan, demo_actions, demonstration_rows_host,
                                                                gather_demonstrations)
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

ORAD, CAP = D.ORAD, D.CAP
AMAX = 16.0                        # rad/s^2 of the cases' blends: a stop costs 15 ticks, so that short budgets still hold whole paths
POOL = D.POOL
# Roles, query n taking role n mod 5: chain_demo_common's four — 0 reach before the last tick, 1 touch mid-path, 2 cut by T_cap,
# 3 run to the end on a joint limit — and 4 LIMIT: the law leaves a joint's limit for several ticks and comes back, so that the
# feedback asks to go further, the clamp holds the joint and its velocity slot reports 0 (an arm without a limited joint runs to
# its end like role 3). Roles are enforced wherever the budget can hold them: from T_cap = lanes - 1 on every role ends as WANT says
# (the limit role may also be cut); only at T_cap = 1, where one tick reaches, touches or ends nothing, is every end code accepted.
# From T_cap = 130 on the limit role's first leg takes about `lanes` ticks, so that the joint is held ON its limit across the
# boundary of the first two passes (asserted by the suites).
ROLES = D.ROLES + ("limit",)
WANT = dict(D.WANT)
WANT[4] = 5
ROLE_TICKS = 63                    # lanes - 1 of every test arm (asserted below): roles are enforced from this budget on
LIMIT_TICKS = 130                  # from this budget on the limit role straddles the first pass boundary


def ends_as_built(role, code):
    """[N] bool: the end code is the role's own; the limit role may also be cut by T_cap (it is about the ticks on the limit)"""
    role, code = np.asarray(role), np.asarray(code)
    return (code == np.array([WANT[r] for r in role])) | ((role == 4) & (code == 0))


def counts_of(model):
    """(N, T_cap) of an arm's cases: every budget — 1, those around a pass (lanes - 1, lanes, lanes + 1), 130, 256 — with every
    count 1, 3, 16"""
    lanes = D.lanes_of(model)
    assert lanes - 1 >= ROLE_TICKS
    return [(N, T) for T in (1, lanes - 1, lanes, lanes + 1, 130, 256) for N in (1, 3, 16)]


NAMES = [name for name in D.ARMS] + [name for name, _, _ in D.EXTRA]
CASES = [(name, N, T) for name in NAMES for N, T in counts_of(D.arm(name)[0]) if T >= 1] + [("iiwa_like7", 2, 1024)]


def leg_per_tick(tick_plan):
    """the TickPlan as a DemonstrationPlan of one leg per tick, for chain_demo_common's helpers: leg k is tick k's action for one
    tick, the last leg of the table takes what is planned beyond it, legs behind the planned ticks are padding"""
    acts, planned = np.asarray(tick_plan.actions, np.float32), np.asarray(tick_plan.planned_ticks, np.int64)
    N, W, _ = acts.shape
    ticks = (np.arange(W)[None, :] < planned[:, None]).astype(np.int64)
    ticks[:, W - 1] += np.maximum(planned - W, 0)
    return DemonstrationPlan(np.asarray(tick_plan.q_start, np.float32), acts, ticks.astype(np.int32), np.asarray(tick_plan.rows, np.int64))


class Case:
    """N demonstrations of one arm under one action per tick at T_cap: tick_plan (TickPlan, table [N, T_cap, A]), law[N, T_cap + 1, A]
    (float64), targets[N, 3], obstacles[N, 3] (float32 values held as float64), role[N], and `plan`, the table as legs"""

    def __init__(self, name, N, T_cap, tick_plan, law, targets, obstacles, role):
        self.name, self.N, self.T_cap = name, N, T_cap
        self.model, self.twin = D.arm(name)
        self.tick_plan, self.law, self.targets, self.obstacles, self.role = tick_plan, law, targets, obstacles, role
        self.plan = leg_per_tick(tick_plan)
        self._host = None

    def take(self, idx):
        idx = np.asarray(idx)
        tp = K.TickPlan(*[None if f is None else np.asarray(f)[idx] for f in self.tick_plan])
        out = Case(self.name, len(idx), self.T_cap, tp, self.law[idx], self.targets[idx], self.obstacles[idx], self.role[idx])
        if self._host is not None:
            _, rec, rows, poses = self._host
            Tm = int(out.plan.rows.max())
            rec, rows, poses = rec[idx], rows[idx, :Tm], poses[idx, :Tm + 1]

            def kept_rows(kept, valid):
                return rows[kept[:, None] & (np.arange(Tm)[None, :] < valid[:, None])].astype(np.float32)
            demos = gather_demonstrations(rec, np.ones(len(idx), bool), kept_rows, False)._replace(action_size=self.model.A)
            out._host = (demos, rec, rows, poses)
        return out

    def sub(self, n):
        return self.take([n])

    def host(self):
        """(demonstrations, records[N, 8], rows[N, T, row floats], poses[N, T + 1, A]): the float64 rule ON THE TICK PLAN"""
        if self._host is None:
            self._host = demonstration_rows_host(self.twin, self.tick_plan, self.targets, self.obstacles, self.T_cap, full=True)
        return self._host


def law_of_polyline(P, T_cap):
    """(law[T_cap + 1, A] float64 at the ticks i DT, planned ticks) of the blended trajectory along P[K + 1, A] at unit speed"""
    A = P.shape[1]
    s = T.blend_schedule(P, np.ones(A), np.full(A, AMAX))
    planned = max(1, int(np.ceil(s["duration"] / DT)))
    Q = T.law_of(s, np.arange(T_cap + 1) * DT)
    Q[min(planned, T_cap + 1):] = s["nodes"][-1]
    return Q, planned


def _polylines(name, model, twin, rng, role, T_cap, lanes):
    """POOL (P[3, A], k) of one role: chain_demo_common's candidates as start -> via -> goal; role 4 leaves a limit and returns"""
    lo, hi = C.limits_of(model)
    room = max(T_cap - 40, 16) if role >= 3 else max(T_cap, 16)      # 'end' and 'limit' run to their last tick: room for three stops
    if role < 4:
        start, via, goal, k = D._candidates(name, model, twin, rng, role, room, lanes)
        return [(np.stack([start[i], via[i], goal[i]]), int(k[i])) for i in range(POOL)]
    start, via, goal, k = D._candidates(name, model, twin, rng, 3, room, lanes)
    limited = [m for m, j in enumerate(model.joints) if j.limited]
    out = []
    for i in range(POOL):
        P = np.stack([start[i], goal[i], 0.5 * (start[i] + goal[i])])
        if T_cap >= LIMIT_TICKS:      # the first leg in about `lanes` ticks: the law's corner, beyond the limit, at the pass boundary
            d = P[1] - P[0]
            P[1] = P[0] + d * ((lanes - 8) * DT / max(np.abs(d).max(), 1e-9))
            P[2] = 0.5 * (P[0] + P[1])
        for m in ([limited[int(rng.integers(len(limited)))]] if limited else []):
            up = abs(hi[m] - start[i, m]) < abs(start[i, m] - lo[m])
            P[0, m] = (hi[m] - 0.05) if up else (lo[m] + 0.05)
            P[1, m] = (hi[m] + 0.04) if up else (lo[m] - 0.04)      # the law's corner lies beyond the limit
            P[2, m] = (hi[m] - 0.03) if up else (lo[m] + 0.03)
        out.append((P, int(k[i])))
    return out


@functools.lru_cache(maxsize=None)
def build_case(name, N, T_cap, seed=0):
    """chain_demo_common.build_case's procedure on tick plans: per query POOL polylines of its role, blended, the table by
    tick_demo.tick_plan_from_law with feedback and the arm's limits, all of the case traced by the twin in one batch; the first
    candidate is taken none of whose ticks lies inside a band and, from T_cap = ROLE_TICKS on, whose demonstration ends as its role
    wants. Target and obstacle are out of the way but for role 0's target and role 1's obstacle, on the end effector of the pose at
    tick k of the float64 recurrence."""
    model, twin = D.arm(name)
    lanes = D.lanes_of(model)
    limits = twin.joint_limits()
    rng = np.random.default_rng(6400 + 977 * N + T_cap + seed)
    tg_away, ob_away = C.away(model)
    picked, todo = {}, list(range(N))
    for attempt in range(8):
        cands = [c for n in todo for c in _polylines(name, model, twin, rng, n % 5, T_cap, lanes)]
        role = np.repeat([n % 5 for n in todo], POOL)
        M = len(role)
        laws = [law_of_polyline(D.f32(P), T_cap) for P, _ in cands]
        law, planned = np.stack([q for q, _ in laws]), np.array([p for _, p in laws])
        k = np.minimum(np.array([kk for _, kk in cands]), np.minimum(planned, T_cap))
        if T_cap < LIMIT_TICKS:      # a short budget: the obstacle on a late pose, or it already touches the arm at its start
            k = np.where(role == 1, np.minimum(planned, T_cap) - rng.integers(0, 3, M), k)
        tp = K.tick_plan_from_law(law[:, 0], law, planned, np.minimum(planned, T_cap), limits, True)
        far = Case(name, M, T_cap, tp, law, np.tile(tg_away, (M, 1)), np.tile(ob_away, (M, 1)), role)
        at = twin.end_effector(D.recurrence64(far)[np.arange(M), k])
        targets = np.where((role == 0)[:, None], at, tg_away)
        obstacles = np.where((role == 1)[:, None], at, ob_away)
        trial = Case(name, M, T_cap, tp, law, D.f32(targets), D.f32(obstacles), role)
        _, rec, _, poses = trial.host()
        live = np.arange(poses.shape[1] - 1)[None, :] < rec[:, :1]
        ok = ~(D.band_of(trial, D.margins_at(trial, poses)) & live).any(axis=1)
        if T_cap >= ROLE_TICKS:
            ok &= ends_as_built(role, rec[:, 1])
            ok &= (role != 0) | (rec[:, 0] < rec[:, 6])
            ok &= (role != 1) | (rec[:, 0] >= 2)
        if T_cap >= LIMIT_TICKS and any(j.limited for j in model.joints):      # on the limit at ticks lanes - 1 and lanes, both live
            held = held_on_limit(trial)
            ok &= (role != 4) | (held[:, lanes - 1] & held[:, lanes] & (rec[:, 0] > lanes + 1))
        for i, n in enumerate(list(todo)):
            good = np.nonzero(ok[i * POOL:(i + 1) * POOL])[0]
            if len(good):
                picked[n] = (trial, i * POOL + int(good[0]))
                todo.remove(n)
        if not todo:
            break
    else:
        raise AssertionError(f"{name} N={N} T_cap={T_cap}: no candidate for queries {todo}")
    parts = [picked[n][0].sub(picked[n][1]) for n in range(N)]
    tp = K.TickPlan(*[None if parts[0].tick_plan[f] is None else np.concatenate([np.asarray(p.tick_plan[f]) for p in parts])
                      for f in range(len(parts[0].tick_plan))])
    return Case(name, N, T_cap, tp, np.concatenate([p.law for p in parts]), np.concatenate([p.targets for p in parts]),
                np.concatenate([p.obstacles for p in parts]), np.arange(N) % 5)


def held_on_limit(case):
    """[N, T_cap] bool: tick k ends with a joint ON its limit while its action still pushes outwards (the host's prediction of the
    device's poses, tick_demo.tick_recurrence)"""
    lo, hi = [v.astype(np.float32) for v in case.twin.joint_limits()]
    acts, poses, _ = K.tick_recurrence(case.tick_plan.q_start, case.law, case.twin.joint_limits(), True)
    return (((poses[:, 1:] == hi) & (acts > 0)) | ((poses[:, 1:] == lo) & (acts < 0))).any(axis=2)


BOUNDARY_NAMES = ("planar3", "iiwa_like7")         # one wave without pairs, and the SC shape


@functools.lru_cache(maxsize=None)
def boundary_case(name, T_cap=130, seed=0):
    """Four demonstrations whose FIRST DONE falls on the boundary of the first two passes: valid rows lanes - 1 (the outcome walked by
    the last lane of pass 0) and lanes (walked by lane 0 of pass 1, whose row takes its action from the carry), once by reaching
    the target and once by touching the obstacle. build_case's procedure with the scene placed at a tick drawn around `lanes`; a
    candidate is taken when the twin counts exactly the wanted rows and no tick lies inside a band."""
    model, twin = D.arm(name)
    lanes, limits = D.lanes_of(model), twin.joint_limits()
    rng = np.random.default_rng(7100 + T_cap + seed)
    tg_away, ob_away = C.away(model)
    want_role, want_valid = np.array([0, 0, 1, 1]), np.array([lanes - 1, lanes, lanes - 1, lanes])
    picked = {}
    for attempt in range(40):
        todo = [n for n in range(4) if n not in picked]
        if not todo:
            break
        cands = [c for n in todo for c in _polylines(name, model, twin, rng, int(want_role[n]), T_cap, lanes)]
        role, want = np.repeat(want_role[todo], POOL), np.repeat(want_valid[todo], POOL)
        M = len(role)
        laws = [law_of_polyline(D.f32(P), T_cap) for P, _ in cands]
        law, planned = np.stack([q for q, _ in laws]), np.array([p for _, p in laws])
        k = np.minimum(want + rng.integers(0, 12, M), np.minimum(planned, T_cap))
        tp = K.tick_plan_from_law(law[:, 0], law, planned, np.minimum(planned, T_cap), limits, True)
        far = Case(name, M, T_cap, tp, law, np.tile(tg_away, (M, 1)), np.tile(ob_away, (M, 1)), role)
        path = D.recurrence64(far)
        for _ in range(3):      # the scene's tick is moved by what the count missed: the done comes some ticks before the pose it sits on
            at = twin.end_effector(path[np.arange(M), k])
            trial = Case(name, M, T_cap, tp, law, D.f32(np.where((role == 0)[:, None], at, tg_away)),
                         D.f32(np.where((role == 1)[:, None], at, ob_away)), role)
            _, rec, _, poses = trial.host()
            k = np.clip(k + (want - rec[:, 0].astype(np.int64)), 1, np.minimum(planned, T_cap))
        live = np.arange(poses.shape[1] - 1)[None, :] < rec[:, :1]
        ok = ~(D.band_of(trial, D.margins_at(trial, poses)) & live).any(axis=1) & (rec[:, 0] == want) & ends_as_built(role, rec[:, 1])
        for i, n in enumerate(todo):
            good = np.nonzero(ok[i * POOL:(i + 1) * POOL])[0]
            if len(good):
                picked[n] = trial.sub(i * POOL + int(good[0]))
    assert len(picked) == 4, f"{name}: no demonstration with a first done at rows {want_valid[[n for n in range(4) if n not in picked]]}"
    parts = [picked[n] for n in range(4)]
    tp = K.TickPlan(*[None if parts[0].tick_plan[f] is None else np.concatenate([np.asarray(p.tick_plan[f]) for p in parts])
                      for f in range(len(parts[0].tick_plan))])
    return Case(name, 4, T_cap, tp, np.concatenate([p.law for p in parts]), np.concatenate([p.targets for p in parts]),
                np.concatenate([p.obstacles for p in parts]), want_role)


def device_tracking_bound(case):
    """[N]: the derived bound on |p_i - Q_i| for the case's poses, tick_demo.tracking_bound. Where the law itself lies outside the
    limits (the limit role) the arm cannot follow it, so the tests apply the bound to clipped_law, the law clipped into them"""
    return K.tracking_bound(case.tick_plan)


def clipped_law(case):
    lo, hi = case.twin.joint_limits()
    return np.minimum(np.maximum(case.law, lo), hi)


def poisoned_table(case, T_cap=None):
    """the table as the GPU tests upload it: [N][T_cap][A] float32 with NaN at every entry k >= T_n, which the kernel never reads"""
    T_cap = case.T_cap if T_cap is None else T_cap
    table = np.full((case.N, T_cap, case.model.A), np.nan, np.float32)
    acts = np.asarray(case.tick_plan.actions, np.float32)
    W = min(T_cap, acts.shape[1])
    table[:, :W] = acts[:, :W]
    table[np.arange(T_cap)[None, :] >= np.asarray(case.tick_plan.rows)[:, None]] = np.nan
    return table


def table_of(plan, T_cap):
    """(table[N][T_cap][A] float32 poisoned behind T_n, counts[N] int32) that feed a two-leg or K-leg plan to the tick entry"""
    ticks = np.asarray(plan.n_ticks, np.int64).sum(axis=1)
    table = demo_actions(plan, T_cap).astype(np.float32)
    table[np.arange(T_cap)[None, :] >= np.minimum(ticks, T_cap)[:, None]] = np.nan
    return table, ticks.astype(np.int32)

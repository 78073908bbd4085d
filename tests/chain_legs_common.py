"""Shared by tests/test_chain_legs_cpu.py and tests/test_chain_legs_gpu.py: the cases that hold naf_chain_demo_rows_legs
(csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (demonstration_plan_legs, demo_actions,
demonstration_rows_host), built with the twin alone as chain_demo_common builds its own. A case here is a chain_demo_common case in
everything its helpers read — plan, scenes, host() — so that rows32, poses32, margins_at, band_of and check_rows serve it as they
stand; what differs is the polyline: nodes[N, K + 1, A] and n_nodes[N] in the place of start, via and goal."""
import functools

import numpy as np

import chain_demo_common as D
import chain_path_common as P
import chain_rollout_common as C

from robotic_manipulator_rloa_amd.environment.kinematic import (demonstration_plan_legs, demonstration_rows_host,
                                                                gather_demonstrations)
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

ORAD = D.ORAD
CAP = D.CAP
# (N, K legs, T_cap): one leg, one demonstration; three legs and a partial last pass; five legs, many passes, every role twice;
# the most legs the entry takes, a switch every tick or two
COUNTS = [(1, 1, 64), (3, 3, 130), (8, 5, 256), (2, 63, 130)]
CASES = [(name, N, K, T) for name in D.ARMS for N, K, T in COUNTS] + [(name, 4, 3, 130) for name, _, _ in D.EXTRA]
POOL = 8
WANT = D.WANT                      # role -> end code: 0 reach -> 1, 1 touch -> 2, 2 cut -> 0, 3 end -> 5


def role_of(n, K):
    """query n takes role n mod 4; the two of a 63-leg case take 'cut' and 'end', which run through every switch of their schedules"""
    return (n + 2) % 4 if K == 63 else n % 4


# The pose bound. test_chain_legs_cpu.test_rehearsal measures, over every pose of every case below, the largest deviation of the
# float32 restatement's recurrence (chain_demo_common.poses32 under demo_actions' K-leg schedule) from the twin's float64 recurrence
# under the same float32 actions:
#     planar3 1.10e-5, iiwa_like7 1.74e-5, long12 1.02e-5, slider4 1.36e-5, iiwa_like7_bare 7.24e-6, planar3_boxes 8.31e-6
#     ->   POSE_DEVIATION = 1.8e-5, rounded up
# — the mechanism is chain_demo_common's: half an ulp of the joint value per tick, leaning one way while a leg repeats one
# increment. More legs change direction more often, so the roundings lean one way for fewer ticks at a time, and the figure came
# out below the two-leg cases' 2.1e-5 at the same tick counts; it is not taken over from there but measured on these cases. The
# bound is 8 x the measured value, the project's margin for another legal rounding of the one fused step, and is never taken from
# the kernel. (check_rows applies chain_demo_common's own, larger bound; the tests here assert this one on the deviation it returns.)
POSE_DEVIATION = 1.8e-5
POSE_BOUND = 8 * POSE_DEVIATION


class Case:
    """N demonstrations of one arm along polylines of at most K legs at T_cap: nodes[N, K + 1, A] (float32 values held as float64, NaN
    behind n_nodes[n]), targets[N, 3], obstacles[N, 3], the plan, and role[N]"""

    def __init__(self, name, N, K, T_cap, nodes, n_nodes, targets, obstacles, role):
        self.name, self.N, self.K, self.T_cap = name, N, K, T_cap
        self.model, self.twin = D.arm(name)
        self.nodes, self.n_nodes, self.targets, self.obstacles, self.role = nodes, n_nodes, targets, obstacles, role
        self.plan = demonstration_plan_legs(nodes, n_nodes, 1.0, T_cap)
        assert self.plan.n_ticks.shape == (N, K)
        self._host = None

    def take(self, idx):
        """the case of the demonstrations idx, in that order; what the twin already said of them is kept"""
        idx = np.asarray(idx)
        out = Case(self.name, len(idx), self.K, self.T_cap, self.nodes[idx], self.n_nodes[idx], self.targets[idx], self.obstacles[idx],
                   self.role[idx])
        if self._host is not None:
            _, rec, rows, poses = self._host
            T = int(out.plan.rows.max())
            rec, rows, poses = rec[idx], rows[idx, :T], poses[idx, :T + 1]

            def kept_rows(kept, valid):
                return rows[kept[:, None] & (np.arange(T)[None, :] < valid[:, None])].astype(np.float32)
            demos = gather_demonstrations(rec, np.ones(len(idx), bool), kept_rows, False)._replace(action_size=self.model.A)
            out._host = (demos, rec, rows, poses)
        return out

    def sub(self, n):
        return self.take([n])

    def host(self):
        """(demonstrations, records[N, 8], rows[N, T, row floats], poses[N, T + 1, A]): the float64 rule"""
        if self._host is None:
            self._host = demonstration_rows_host(self.twin, self.plan, self.targets, self.obstacles, self.T_cap, full=True)
        return self._host


def _between(rng, lo, hi):
    """an integer in lo .. hi - 1, lo where the range is empty"""
    return int(rng.integers(lo, max(hi, lo + 1)))


def schedule(rng, n, K, T_cap, lanes):
    """(ticks per real leg, the legs of zero length) of query n of a case of K legs: what its role and the issue's list ask for.
    A zero-length leg is one tick at action 0; a query may hold fewer than K legs."""
    role = role_of(n, K)
    r = lambda lo=8, hi=36: _between(rng, lo, hi)      # noqa: E731
    if K == 1:
        return [r(20, T_cap - 4)], set()
    if K == 3:
        if role == 0:                                  # a switch strictly inside the first pass
            s, m = _between(rng, 2, lanes - 1), r()
            return [s, m, _between(rng, 8, min(36, T_cap - 6 - s - m))], set()
        if role == 1:                                  # a switch on a pass boundary
            m = r(8, 30)
            return [lanes, m, _between(rng, 4, min(30, T_cap - 4 - lanes - m))], set()
        if role == 2:                                  # T_cap cuts inside leg 1 of 3
            s = r(10, 40)
            return [s, T_cap - s + r(5, 30), 10], set()
        return [r(20, 50), r(20, 50)], set()           # fewer legs than the launch's K; runs to its end
    if K == 5:
        if n == 0:                                     # a leg longer than a pass, then two switches within two ticks, one leg of zero length
            return [lanes + r(5, 20), 1, 1, r(), r()], {1}
        if n == 4:
            return [r(5, 20), min(2 * lanes + 5, 140), 1, 1, r(8, 30)], {3}
        if n == 5:                                     # the first switch on a pass boundary
            return [lanes, r(), 1, 1, r()], {2}
        if role == 1:
            return [r(), r(), r(), r(), r()], set()
        if n == 2:                                     # T_cap cuts inside leg 2 of 5
            a, b = r(20, 60), r(20, 60)
            return [a, b, T_cap - a - b + r(5, 30), r(), r()], set()
        if n == 6:                                     # ... and inside leg 1 of 5
            a = r(20, 60)
            return [a, T_cap - a + r(5, 30), r(), r(), r()], set()
        if n == 3:
            return [r(20, 60), r(20, 60), r(20, 60)], set()
        return [r(20, 50), r(20, 50), 1, r(20, 50)], {2}
    legs = K if role == 2 else 40                      # K = 63: a switch every tick or two; 'cut' with all legs, 'end' with 40
    while True:
        ticks = [int(t) for t in rng.choice([1, 2, 3, 4], legs)]
        if (sum(ticks) >= T_cap + 5 and sum(ticks[:-2]) > T_cap) if role == 2 else 30 <= sum(ticks) <= T_cap - 6:
            ones = [l for l, t in enumerate(ticks) if t == 1 and l > 0]
            return ticks, set(int(l) for l in rng.choice(ones, min(5, len(ones)), replace=False))


def _candidates(model, twin, rng, n, K, T_cap, lanes):
    """POOL (nodes[K + 1, A], n_nodes, k, ticks) of query n: legs from a free pose, each along a max-norm unit direction that leans,
    joint by joint, towards the middle of the limits; k is the tick whose pose places the target (role 0) or the obstacle (role 1)"""
    A = model.A
    lo, hi = C.limits_of(model)
    start = P.IK.free_poses(model, twin, rng, POOL)
    out = []
    for i in range(POOL):
        ticks, still = schedule(rng, n, K, T_cap, lanes)
        d0 = rng.uniform(0.2, 1.0, A) * np.where(start[i] > 0.5 * (lo + hi), -1.0, 1.0)
        d0 /= np.abs(d0).max()
        nodes = np.full((K + 1, A), np.nan)
        nodes[0] = np.clip(start[i], lo, hi)
        for l, t in enumerate(ticks):
            d = d0 if l == 0 else 0.35 * rng.uniform(-1.0, 1.0, A) + 0.65 * d0
            d = d / np.abs(d).max()
            nodes[l + 1] = nodes[l] if l in still else np.clip(nodes[l] + (t - 0.5) * DT * d, lo, hi)      # (ceil gives exactly t)
        total = sum(ticks)
        k = total - _between(rng, 2, 5) if role_of(n, K) == 0 else 2 * total // 3
        out.append((nodes, len(ticks) + 1, k, ticks + [0] * (K - len(ticks))))
    return out


@functools.lru_cache(maxsize=None)
def build_case(name, N, K, T_cap, seed=0):
    """chain_demo_common.build_case's procedure on polylines: per query POOL candidates of its role and schedule, all of the case
    traced by the twin in one batch; the first candidate is taken whose plan holds exactly the scheduled ticks (a clipped node may
    change them), whose demonstration ends as its role wants — role 0 before its last planned tick, role 1 after at least two rows,
    role 2 cut by T_cap, role 3 at its last planned tick — and none of whose ticks lies inside a band. Target and obstacle are out
    of the way but for role 0's target and role 1's obstacle, on the end effector of the pose at tick k along the float64
    recurrence. Queries without an accepted candidate are drawn again."""
    model, twin = D.arm(name)
    lanes = D.lanes_of(model)
    rng = np.random.default_rng(5300 + 977 * N + 31 * K + T_cap + seed)
    tg_away, ob_away = C.away(model)
    picked, todo = {}, list(range(N))
    for attempt in range(8):
        parts = [c for n in todo for c in _candidates(model, twin, rng, n, K, T_cap, lanes)]
        nodes, count = D.f32(np.stack([p[0] for p in parts])), np.array([p[1] for p in parts])
        k, want_ticks = np.array([p[2] for p in parts]), np.array([p[3] for p in parts])
        role = np.repeat([role_of(n, K) for n in todo], POOL)
        M = len(role)
        far = Case(name, M, K, T_cap, nodes, count, np.tile(tg_away, (M, 1)), np.tile(ob_away, (M, 1)), role)
        at = twin.end_effector(D.recurrence64(far)[np.arange(M), np.minimum(k, T_cap)])
        targets = np.where((role == 0)[:, None], at, tg_away)
        obstacles = np.where((role == 1)[:, None], at, ob_away)
        trial = Case(name, M, K, T_cap, nodes, count, D.f32(targets), D.f32(obstacles), role)
        _, rec, _, poses = trial.host()
        live = np.arange(poses.shape[1] - 1)[None, :] < rec[:, :1]
        ok = (rec[:, 1] == np.array([WANT[r] for r in role])) & ~(D.band_of(trial, D.margins_at(trial, poses)) & live).any(axis=1)
        ok &= np.all(trial.plan.n_ticks == want_ticks, axis=1)
        ok &= (role != 0) | (rec[:, 0] < rec[:, 6])
        ok &= (role != 1) | (rec[:, 0] >= 2)
        ok &= (role != 2) | (rec[:, 6] > T_cap)
        ok &= (role != 3) | (rec[:, 6] <= T_cap)
        for i, n in enumerate(list(todo)):
            good = np.nonzero(ok[i * POOL:(i + 1) * POOL])[0]
            if len(good):
                picked[n] = (trial, i * POOL + int(good[0]))
                todo.remove(n)
        if not todo:
            break
    else:
        raise AssertionError(f"{name} N={N} K={K} T_cap={T_cap}: no candidate for queries {todo}")
    trials = {id(t): t for t, _ in picked.values()}
    if len(trials) == 1:
        return next(iter(trials.values())).take([picked[n][1] for n in range(N)])
    cols = [np.stack([getattr(picked[n][0], f)[picked[n][1]] for n in range(N)]) for f in ("nodes", "n_nodes", "targets", "obstacles")]
    return Case(name, N, K, T_cap, *cols, np.array([role_of(n, K) for n in range(N)]))


def features(case):
    """the set of the issue's schedule features that `case` holds, from its plan and what the twin said of it"""
    lanes = D.lanes_of(case.model)
    _, rec, _, _ = case.host()
    found = set()
    for n in range(case.N):
        ticks = case.plan.n_ticks[n].astype(np.int64)
        real = int(np.sum(ticks > 0))
        ends = np.cumsum(ticks[:real])
        T = min(int(ends[-1]), case.T_cap)
        switches = [int(e) for e in ends[:-1] if e <= T]             # tick e is the first of the next leg; pose e is walked
        for e in switches:
            found.add("switch on a pass boundary" if e % lanes == 0 else "switch inside a pass")
        still = [l for l in range(real) if np.all(case.plan.leg_actions[n, l] == 0.0) and ticks[l] == 1]
        for l in range(1, real - 1):
            if ticks[l] == 1 and ticks[l + 1] == 1 and ends[l - 1] // lanes == ends[l + 1] // lanes and ends[l + 1] <= T \
                    and (l in still or l + 1 in still):
                found.add("two switches inside one pass, 1-tick legs, one of zero length")
        if np.any(ticks > lanes):
            found.add("a leg longer than a pass")
        if real < case.K:
            found.add("fewer legs than K")
        if ends[-1] > case.T_cap and case.T_cap not in ends and np.searchsorted(ends, case.T_cap, side="right") < real - 1:
            found.add("T_cap cuts inside a leg that is not the last")
        found.add({1: "reached", 2: "contact", 3: "contact", 4: "contact", 5: "end", 0: "frames"}[int(rec[n, 1])])
    return found


FEATURES = {"switch on a pass boundary", "switch inside a pass", "two switches inside one pass, 1-tick legs, one of zero length",
            "a leg longer than a pass", "fewer legs than K", "T_cap cuts inside a leg that is not the last", "reached", "contact", "end"}


def split_two_leg_plan(plan, K, rng):
    """the two-leg plan as a K-leg plan of the same ticks and actions (K >= 2): each leg cut into consecutive legs of its own
    action, at least one tick each where the leg has that many; what is left over is padding"""
    N, _, A = plan.leg_actions.shape
    ticks, acts = np.zeros((N, K), np.int32), np.zeros((N, K, A), np.float32)
    for n in range(N):
        n1, n2 = (int(t) for t in plan.n_ticks[n])
        k1 = min(n1, max(1, K // 2))
        k2 = min(n2, K - k1)
        pieces = []
        for total, parts, leg in ((n1, k1, 0), (n2, k2, 1)):
            cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
            sizes = np.diff(np.concatenate([[0], cuts, [total]]))
            pieces += [(int(s), leg) for s in sizes]
        for l, (s, leg) in enumerate(pieces):
            ticks[n, l], acts[n, l] = s, plan.leg_actions[n, leg]
    return plan._replace(leg_actions=acts, n_ticks=ticks)

"""Shared by tests/test_oracle_golden.py (G9), tests/test_env_rule_cpu.py and tests/test_env_rule_gpu.py: the reader of fixture G9,
env_oracle's prediction of a G9 scenario's records, and the case builders and checker that hold the host environments and the
kernels to oracle/env_oracle.py. The case table and SEED are fixed here so that the CPU rehearsal and the GPU suite check the
same cases."""
import os
import random

import numpy as np

import g9_scenarios as G9
import scripted_pybullet as SP
from oracle import env_oracle as R

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261                      # of every random draw below


# ---- G9 -----------------------------------------------------------------------------------------------------------------------
_G9 = []


def g9_records():
    """[(scenario, (states, numbers, log, base))] of tests/golden/g9_env.npz, read once"""
    if not _G9:
        _G9.extend(G9.unpack(np.load(os.path.join(HERE, "golden", "g9_env.npz"), allow_pickle=False)))
    return _G9


def _served(d, link, frame, limit=R.MAX_DISTANCE):
    """the scripted simulator's getClosestPoints answer for distance d, as records (scripted_pybullet.make_modules)"""
    if d != d or d > limit:
        return []
    near = (0,) * 8 + (d,)
    return [(0,) * 8 + (d + 0.25,), near, (0,) * 8 + (d + 1.0,)] if (link + frame) % 3 == 0 else [near]


def _reward_record(r):
    return float(r), float(SP.REWARD_INT if isinstance(r, int) else SP.REWARD_FLOAT)


def oracle_records(sc, defect=None):
    """What env_oracle says scenario `sc` records: (states, numbers, log, base) in scripted_pybullet.drive's layout, from the
    scenario's scripted numbers alone."""
    n, ee, involved, fixed = sc["n"], sc["ee"], sc["involved"], sc["fixed"]
    A = len(involved)
    ops = np.asarray(sc["ops"])
    states = np.full((len(ops), 2 * A + 9), np.nan)
    numbers = np.full((len(ops), SP.NUM), np.nan)
    log, base, ticks = [], [], 0

    def seen():
        f = int(np.searchsorted(np.asarray(sc["switch"]).reshape(-1), ticks, side="right"))
        d_obstacle = [R.distance_of(_served(float(sc["obstacle_d"][f, j]), j, f)) for j in range(n)]
        d_target = R.distance_of(_served(float(sc["target_d"][f, ee]), ee, f))
        d_self = [R.distance_of(_served(float(sc["self_d"][f, i, j]), i, f)) for i, j in R.self_pairs(n)]
        state = R.state_of(sc["joints"][f], involved, sc["ee_pos"][f], sc["target"], sc["obstacle"], defect=defect)
        return d_target, d_obstacle, d_self, state

    for k, op in enumerate(ops):
        kind = int(op[0])
        if kind == SP.OP_PROBE:
            d_target, d_obstacle, d_self, states[k] = seen()
            r0, t0 = R.rule(d_target, d_obstacle, d_self, False, defect=defect, involved=involved)
            r1, t1 = R.rule(d_target, d_obstacle, d_self, True, defect=defect, involved=involved)
            le = defect == "le_for_lt"
            flag = d_target <= R.TARGET_THRESHOLD if le else d_target < R.TARGET_THRESHOLD
            numbers[k] = _reward_record(r0) + _reward_record(r1) + (t0, t1, float(flag), d_target - R.TARGET_THRESHOLD)
        elif kind == SP.OP_STEP:
            calls = R.step_calls(involved, fixed, op[1:1 + A], sc["max_force"])
            log.extend(calls.tolist())
            ticks += int(np.sum(calls[:, 0] == R.CALL_TICK))
            d_target, d_obstacle, d_self, states[k] = seen()
            reward, done = R.rule(d_target, d_obstacle, d_self, False, defect=defect, involved=involved)
            numbers[k, :3] = _reward_record(reward) + (done,)
        elif kind == SP.OP_RESET:
            calls = R.reset_calls(n, sc["init"], sc["var"], random.Random(int(op[1])).uniform)
            log.extend(calls.tolist())
            base.append(list(R.BASE_POSE))
            ticks += int(np.sum(calls[:, 0] == R.CALL_TICK))
            states[k] = seen()[3]
    return states, numbers, np.array(log, float).reshape(-1, 6), np.array(base, float).reshape(-1, 7)


def records_differ(got, want):
    """the names of the record parts in which two (states, numbers, log, base) differ (NaN equals NaN)"""
    names = ("states", "numbers", "log", "base")
    return [nm for nm, a, b in zip(names, got, want)
            if np.shape(a) != np.shape(b) or not np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)]


# ---- the kinematic arms: cases built with the twin alone -------------------------------------------------------------------------
# The distances are our own kinematics (KinematicEnvironment, held elsewhere to an independent walk and to brute-force distance
# searches). What is pinned here is the map from those distances to reward, done, outcome and state layout: env_oracle.rule /
# state_of, which G9 pins on the reference.
import functools
from dataclasses import dataclass

E_CASES = 100                     # one full wave and a partial one
ARMS = ("planar3", "iiwa_like7", "slider4")                      # the GPU suite's; the CPU suite adds the two below
CPU_ARMS = ARMS + ("iiwa_like7_noflag", "arm_with_gripper")
# defects that cannot show on an arm, with the structural reason the tests assert:
#   no self-collision pairs in force -> the flag changes nothing;  involved = 0 .. A-1 -> both index rules read the same joints
#   le_for_lt -> nowhere: no computed distance lies ON a threshold (the cases keep delta away from it, and a float32 device is not
#   compared inside its band), so <= and < give every case the same verdict; G9, whose distances are scripted, tells them apart
ON_THRESHOLD_ONLY = {"le_for_lt"}
EQUIVALENT = {
    # (planar3's base capsule is a point ON its first link's axis: no contact is the base's alone)
    "planar3": {"self_without_flag", "self_ignored_with_flag", "joints_at_involved", "contact_on_involved_only"},
    "slider4": {"self_without_flag", "self_ignored_with_flag", "joints_at_involved"},
    "iiwa_like7": {"self_without_flag", "joints_at_involved"},               # compiled WITH the flag: honouring it anyway is the rule
    "iiwa_like7_noflag": {"self_ignored_with_flag", "joints_at_involved"},   # compiled WITHOUT: ignoring it is the rule
    "arm_with_gripper": {"self_without_flag", "self_ignored_with_flag"},
    "synthetic6": {"self_without_flag", "self_ignored_with_flag", "joints_at_involved", "contact_on_involved_only"},
}
EQUIVALENT = {name: defects | ON_THRESHOLD_ONLY for name, defects in EQUIVALENT.items()}
KINDS = ("target_in", "target_out", "obstacle_in", "obstacle_out", "base_in", "self_in", "self_out", "cell_in", "cell_out",
         "reached_obstacle", "reached_self", "reached_cell", "obstacle_self", "free")
PER_KIND = 6                      # cases of every constructed kind; the rest of E_CASES is random filler ("free")


@dataclass
class Arm:
    name: str
    model: object                 # what is stepped
    twin: object                  # KinematicEnvironment(model)
    geometry: object              # the twin whose pairs give the self distances (the flagged compile of the same arm)
    flag: bool                    # consider_autocollision as compiled into `model`
    involved: list                # the involved joints' indices in the URDF
    all_joints: int               # joints the state rule may read: 0 .. max(involved)


@functools.lru_cache(maxsize=None)
def arm_of(name):
    import chain_box_common as X
    import chain_rollout_common as C
    from test_chain_env_cpu import ARMS as TABLE, model_of
    from robotic_manipulator_rloa_amd.environment.kinematic import KinematicEnvironment
    base = "iiwa_like7" if name.startswith("iiwa_like7") else name
    if name == "iiwa_like7":
        model, twin = X.arm("iiwa_like7")
        geometry = twin
    elif name == "iiwa_like7_noflag":
        model = model_of("iiwa_like7", workcell_boxes=X.boxes_of("iiwa_like7"))
        twin, geometry = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), C.ORAD), X.arm("iiwa_like7")[1]
    else:
        model = model_of(name)
        twin = geometry = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), C.ORAD)
    involved = list(TABLE[base][1])
    return Arm(name, model, twin, geometry, bool(model.self_pairs), involved, max(involved) + 1)


def delta_of(model):
    """how far a constructed case lies from its threshold: 16 x the float32 band of the arm's suite (chain_rollout_common.tol_of)"""
    import chain_rollout_common as C
    return 16 * C.tol_of(model)


@dataclass
class Distances:
    """what env_oracle.rule is asked about, per case: float64, from the twin's geometry at the given poses"""
    d_target: np.ndarray          # [E]
    d_links: np.ndarray           # [E, segments (+ 1)]: every capsule's distance to the obstacle sphere; then the workcell clearance
    d_self: np.ndarray            # [E, pairs]: the pair clearances ([E, 0] without pairs)
    moved: list                   # indices into d_links of the capsules a driven joint moves (for the defect contact_on_involved_only)
    ee: np.ndarray                # [E, 3]


def distances(arm, q, target, obstacle):
    import chain_rollout_common as C
    from robotic_manipulator_rloa_amd.environment.kinematic import segment_point_distance2
    q = np.asarray(q, np.float64)
    g = arm.geometry
    ee = g.end_effector(q)
    d_target = np.array([np.linalg.norm(v) for v in (ee - target).reshape(-1, 3)])
    links = [np.sqrt(segment_point_distance2(a, b, np.asarray(obstacle, np.float64))) - r - C.ORAD for a, b, r in g.world_segments(q)]
    moved = [k for k, s in enumerate(arm.model.segments) if s.frame >= 1]
    if arm.model.cell_pairs:
        links.append(arm.twin.cell_clearance(q) + np.zeros(len(q)))
    d_self = g.pair_clearances(q).T if g.model.self_pairs else np.zeros((len(q), 0))
    return Distances(d_target, np.stack(links, axis=1), d_self, moved, ee)


def in_band(arm, dist, tol):
    """[E] bool: a margin inside the band in which a float32 device's class is not compared — the existing chain suites' bands
    (chain_rollout_common.band_of, chain_cell_common.band4): 2 tol on the target distance, the obstacle and the workcell, 4 tol on
    the self-clearance (only where the arm honours it)"""
    band = (np.abs(dist.d_target - R.TARGET_THRESHOLD) <= 2 * tol) | (np.abs(dist.d_links) <= 2 * tol).any(axis=1)
    if arm.flag and dist.d_self.shape[1]:
        band |= (np.abs(dist.d_self) <= 4 * tol).any(axis=1)
    return band


@dataclass
class Census:
    compared: int
    band: int                     # skipped: inside the band
    band_constructed: int         # ... of the constructed cases: must be 0
    band_filler: int
    filler: int
    failures: list
    outcomes: dict


def judge(arm, dist, reward, done, tol, constructed, defect=None, code=None, band_tol=None):
    """THE check, the same for every statement of the rule: env_oracle.rule of the float64 distances against the reported reward[E]
    and done[E] (and outcome code[E] of a rollout: 0 none, 1 reached, 2 / 3 / 4 a contact). done, the outcome's class and the
    values 250 / -1000 must be equal; a shaped reward within tol of the oracle's. Cases inside the band are skipped and counted.
    Nothing is asserted here: the failures are returned, so that the rehearsal can ask for them."""
    band = in_band(arm, dist, tol if band_tol is None else band_tol)
    failures, outcomes = [], {"reached": 0, "contact": 0, "free": 0}
    for e in range(len(reward)):
        if band[e]:
            continue
        want_r, want_d = R.rule(dist.d_target[e], dist.d_links[e], dist.d_self[e], arm.flag, defect=defect, involved=dist.moved)
        kind = "reached" if want_r == R.REACHED_REWARD and isinstance(want_r, int) else \
            ("contact" if want_r == R.CONTACT_REWARD and isinstance(want_r, int) else "free")
        outcomes[kind] += 1
        ok = float(done[e]) == float(want_d)
        if isinstance(want_r, int):
            ok = ok and float(reward[e]) == float(want_r)
        else:
            ok = ok and float(reward[e]) not in (250.0, -1000.0) and abs(float(reward[e]) - want_r) <= tol
        if code is not None:
            ok = ok and {"reached": code[e] == 1, "contact": code[e] in (2, 3, 4), "free": code[e] == 0}[kind]
        if not ok:
            failures.append((e, float(reward[e]), float(done[e]), want_r, want_d, None if code is None else int(code[e])))
    constructed = np.asarray(constructed, bool)
    return Census(int((~band).sum()), int(band.sum()), int((band & constructed).sum()), int((band & ~constructed).sum()),
                  int((~constructed).sum()), failures, outcomes)


def judge_state(arm, q, qd, dist, target, obstacle, state, tol, defect=None):
    """failures of the state layout: state[E, 2A + 9] against env_oracle.state_of of the joint table the reference would read —
    joint j of the URDF holds (q, qd) of its driven joint, (0, 0) if it is a fixed one (:472-476) — the twin's end effector, the
    target and the obstacle. Joint columns within 2^-23 max(1, |q|) (a float32 device), the end effector within tol, the rest
    equal; exact for a float64 statement (tol = 0)."""
    A = arm.model.A
    failures = []
    for e in range(len(state)):
        table = np.zeros((arm.all_joints, 2))
        for k, j in enumerate(arm.involved):
            table[j] = q[e, k], qd[e, k]
        want = R.state_of(table, arm.involved, dist.ee[e], target[e], obstacle[e], defect=defect)
        bound = np.concatenate([2.0 ** -23 * np.maximum(1.0, np.abs(want[:A])), np.zeros(A), np.full(3, tol), np.zeros(6)]) \
            if tol > 0 else np.zeros(2 * A + 9)
        if not np.all(np.abs(np.asarray(state[e], np.float64) - want) <= bound):
            failures.append((e, np.asarray(state[e]), want))
    return failures


@dataclass
class Cases:
    arm: Arm
    kind: np.ndarray              # [E] of KINDS
    q: np.ndarray                 # [E, A] the pose the case is about (float32 values)
    q0: np.ndarray                # [E, A] where the step starts: q0 + DT act = q up to rounding
    act: np.ndarray               # [E, A]
    target: np.ndarray            # [E, 3] float32 values
    obstacle: np.ndarray          # [E, 3]

    @property
    def constructed(self):
        return self.kind != "free"


def _unit(rng, n=None):
    v = rng.normal(size=(3,) if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _crossing(f, base, ends, level, inside):
    """poses on the lines base -> ends at which f crosses `level` downwards, by bisection: the side at or below it (inside) or at or
    above it; NaN rows where f(base) <= level or f(ends) >= level"""
    lo, hi = np.zeros(len(base)), np.ones(len(base))
    ok = (f(base) > level) & (f(ends) < level)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        above = f(base + mid[:, None] * (ends - base)) > level
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    out = base + (hi if inside else lo)[:, None] * (ends - base)
    out[~ok] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def build_cases(name):
    """E_CASES cases of one arm (chain_traj_common's way: a fixed SEED, the table shared by the CPU and the GPU suite):
      target_in / target_out       the target at ee(q) + (0.05 -/+ delta) u; nothing else near
      obstacle_in / obstacle_out   the obstacle centre off the middle of a capsule's axis, perpendicular to it, at capsule radius +
                                   obstacle radius -/+ delta — the twin confirms that no other capsule is nearer
      base_in                      the same on the base's capsule, which no driven joint moves
      self_in / self_out           a fold at which the self-clearance is -/+ delta (arms with pairs), clear of the workcell
      cell_in / cell_out           a pose at which the workcell clearance is -/+ delta (arms with a workcell), clear of itself
      reached_obstacle, reached_self, reached_cell, obstacle_self      two of the above (the `in` sides) at one pose
      free                         random filler: uniform poses, the target within 0.10 of the end effector and the obstacle within
                                   0.05 of touching a capsule, wherever they fall
    delta = 16 tol_of(model): outside every band of the arm's suite by construction, and a threshold off by 1e-3 flips them."""
    import chain_rollout_common as C
    from test_chain_env_cpu import random_q
    from robotic_manipulator_rloa_amd.environment.urdf_chain import DT
    arm = arm_of(name)
    model, g = arm.model, arm.geometry
    A, delta = model.A, delta_of(model)
    rng = np.random.default_rng(SEED + sorted(EQUIVALENT).index(name))
    lo, hi = C.limits_of(model)
    far_t, far_o = C.away(model)
    has_self, has_cell = bool(g.model.self_pairs), bool(model.cell_pairs)
    cell = lambda q: arm.twin.cell_clearance(q) + np.zeros(np.shape(q)[:-1])
    selfc = lambda q: g.self_clearance(q) + np.zeros(np.shape(q)[:-1])

    def pool(n):
        q = np.clip(np.stack([random_q(model, rng) for _ in range(4 * n)]), lo + 0.01, hi - 0.01)
        return q[(selfc(q) > 0.01) & (cell(q) > 0.01)][:n]

    def obstacle_at(q, sign, base=False):
        """an obstacle centre at (capsule radius + obstacle radius + sign delta) off the middle of a capsule of pose q, or None"""
        segs = g.world_segments(q)
        still = [k for k, sg in enumerate(model.segments) if sg.frame == 0]
        moving = [k for k, sg in enumerate(model.segments) if sg.frame >= 1]
        for _ in range(64):
            s = int(rng.choice(still if base else moving))
            a, b, r = segs[s]
            axis = b - a
            n = _unit(rng) if np.linalg.norm(axis) < 1e-9 else np.cross(axis, _unit(rng))
            c = 0.5 * (a + b) + (r + C.ORAD + sign * delta) * n / np.linalg.norm(n)
            if abs(g.clearance(q, c) - C.ORAD - sign * delta) < 1e-9:
                return c
        return None

    free = pool(400)
    folds = {}
    if has_self:
        ends = C.contact_poses(model, g, rng, 400)
        ends = ends[cell(ends) > 0.005]
        n = min(len(ends), len(free))
        for inside in (True, False):
            q = _crossing(selfc, free[:n], ends[:n], -delta if inside else delta, inside)
            q = q[~np.isnan(q).any(axis=1)]
            folds[inside] = list(q[(cell(q) > 0.01) & (np.abs(selfc(q) - (-delta if inside else delta)) < 0.01 * delta)])
    dips = {}
    if has_cell:
        u = np.stack([random_q(model, rng) for _ in range(2000)])
        ends = u[(cell(u) < -0.01) & (selfc(u) > 0.01)][:len(free)]
        n = min(len(ends), len(free))
        for inside in (True, False):
            q = _crossing(cell, free[:n], ends[:n], -delta if inside else delta, inside)
            q = q[~np.isnan(q).any(axis=1)]
            dips[inside] = list(q[(selfc(q) > 0.01) & (np.abs(cell(q) - (-delta if inside else delta)) < 0.01 * delta)])
    free = list(free)
    kinds = [k for k in KINDS[:-1] if ("self" not in k or has_self) and ("cell" not in k or has_cell)]
    rows = []
    for kind in kinds:
        made = 0
        while made < PER_KIND:
            if kind in ("self_in", "reached_self", "obstacle_self"):
                q = folds[True].pop()
            elif kind == "self_out":
                q = folds[False].pop()
            elif kind in ("cell_in", "reached_cell"):
                q = dips[True].pop()
            elif kind == "cell_out":
                q = dips[False].pop()
            else:
                q = free.pop()
            q = C.f32(q)
            tg, ob = far_t, far_o
            if kind in ("target_in", "reached_obstacle", "reached_self", "reached_cell"):
                tg = g.end_effector(q) + (R.TARGET_THRESHOLD - delta) * _unit(rng)
            elif kind == "target_out":
                tg = g.end_effector(q) + (R.TARGET_THRESHOLD + delta) * _unit(rng)
            if kind in ("obstacle_in", "obstacle_out", "base_in", "reached_obstacle", "obstacle_self"):
                ob = obstacle_at(q, 1.0 if kind == "obstacle_out" else -1.0, base=kind == "base_in")
                if ob is None:
                    continue
            rows.append((kind, q, tg, ob))
            made += 1
    while len(rows) < E_CASES:
        q = C.f32(free.pop())
        tg = g.end_effector(q) + rng.uniform(0.0, 0.10) * _unit(rng)
        segs = g.world_segments(q)
        a, b, r = segs[int(rng.integers(0, len(segs)))]
        ob = a + rng.uniform(0.0, 1.0) * (b - a) + (r + C.ORAD + rng.uniform(-0.05, 0.05)) * _unit(rng)
        rows.append(("free", q, tg, ob))
    kind = np.array([r[0] for r in rows])
    q = np.stack([r[1] for r in rows])
    act = rng.uniform(-1.0, 1.0, q.shape)
    q0 = C.f32(np.clip(q - DT * act, lo, hi))
    act = C.f32((q - q0) / DT)
    return Cases(arm, kind, q, q0, act, C.f32(np.stack([r[2] for r in rows])), C.f32(np.stack([r[3] for r in rows])))


# ---- the synthetic stand-in (environment/synthetic.py, csrc/synth_env.hip) --------------------------------------------------------
TOL_SYNTH = 3e-6                  # the stand-in suite's bound on a float32 position (test_agent_gpu: atol 3e-6 on the state)
REWARD_TOL_SYNTH = 1e-5           # ... and on its shaped reward (test_agent_gpu: atol 1e-5)
SYNTH_KINDS = ("target_in", "target_out", "obstacle_in", "obstacle_out", "reached_obstacle", "free")
SYNTH_PER_KIND = 10


def synth_points(q):
    """[E, A, 3] float64: the joint frame origins of the stand-in's chain (alternating z / y revolute joints, link k along the new z)
    — what forward_kinematics / fk_chain walk, restated; the last one is the end effector"""
    from robotic_manipulator_rloa_amd.environment.synthetic import LINKS
    q = np.asarray(q, np.float64)
    E, A = q.shape
    Rm, p = np.broadcast_to(np.eye(3), (E, 3, 3)).copy(), np.zeros((E, 3))
    out = np.empty((E, A, 3))
    for k in range(A):
        c, s = np.cos(q[:, k]), np.sin(q[:, k])
        N = np.empty_like(Rm)
        if k % 2 == 0:
            N[:, :, 0], N[:, :, 1], N[:, :, 2] = Rm[:, :, 0] * c[:, None] + Rm[:, :, 1] * s[:, None], \
                -Rm[:, :, 0] * s[:, None] + Rm[:, :, 1] * c[:, None], Rm[:, :, 2]
        else:
            N[:, :, 0], N[:, :, 1], N[:, :, 2] = Rm[:, :, 0] * c[:, None] - Rm[:, :, 2] * s[:, None], Rm[:, :, 1], \
                Rm[:, :, 0] * s[:, None] + Rm[:, :, 2] * c[:, None]
        Rm = N
        p = p + Rm[:, :, 2] * float(LINKS[k])
        out[:, k] = p
    return out


@functools.lru_cache(maxsize=None)
def synth_arm(A):
    """the stand-in as an Arm for judge(): no pairs, every contact point on an involved joint"""
    model = type("StandIn", (), dict(A=A, self_pairs=[], cell_pairs=[]))()
    return Arm(f"synthetic{A}", model, None, None, False, list(range(A)), A)


def synth_distances(A, q, target, obstacle):
    from robotic_manipulator_rloa_amd.environment.synthetic import OBSTACLE_RADIUS
    pts = synth_points(q)
    ee = pts[:, -1]
    d_target = np.array([np.linalg.norm(v) for v in ee - target])
    d_links = np.linalg.norm(pts - np.asarray(obstacle, np.float64)[:, None, :], axis=-1) - float(OBSTACLE_RADIUS)
    return Distances(d_target, d_links, np.zeros((len(q), 0)), list(range(A)), ee)


@functools.lru_cache(maxsize=None)
def build_synth_cases(A):
    """E_CASES cases of the A-joint stand-in, as build_cases: the target at ee + (0.05 -/+ delta) u, the obstacle centre at
    (0.06 -/+ delta) from a joint frame origin with no other origin nearer, both, and random filler; delta = 16 TOL_SYNTH."""
    import chain_rollout_common as C
    from robotic_manipulator_rloa_amd.environment.synthetic import DT, OBSTACLE_RADIUS
    rng = np.random.default_rng(SEED + 100 + A)
    delta, orad = 16 * TOL_SYNTH, float(OBSTACLE_RADIUS)
    far_t, far_o = np.array([0.0, 0.0, 4.0]), np.array([0.0, 0.0, -4.0])
    rows = []
    for kind in SYNTH_KINDS[:-1]:
        made = 0
        while made < SYNTH_PER_KIND:
            q = C.f32(rng.uniform(-1.5, 1.5, A))
            pts = synth_points(q[None])[0]
            tg, ob = far_t, far_o
            if kind in ("target_in", "reached_obstacle"):
                tg = pts[-1] + (R.TARGET_THRESHOLD - delta) * _unit(rng)
            elif kind == "target_out":
                tg = pts[-1] + (R.TARGET_THRESHOLD + delta) * _unit(rng)
            if kind in ("obstacle_in", "obstacle_out", "reached_obstacle"):
                sign = 1.0 if kind == "obstacle_out" else -1.0
                ob = pts[int(rng.integers(0, A))] + (orad + sign * delta) * _unit(rng)
                if abs(np.min(np.linalg.norm(pts - ob, axis=1)) - orad - sign * delta) > 1e-9:
                    continue
            rows.append((kind, q, tg, ob))
            made += 1
    while len(rows) < E_CASES:
        q = C.f32(rng.uniform(-1.5, 1.5, A))
        pts = synth_points(q[None])[0]
        rows.append(("free", q, pts[-1] + rng.uniform(0.0, 0.10) * _unit(rng),
                     pts[int(rng.integers(0, A))] + (orad + rng.uniform(-0.05, 0.05)) * _unit(rng)))
    kind = np.array([r[0] for r in rows])
    q = np.stack([r[1] for r in rows])
    act = rng.uniform(-1.0, 1.0, q.shape)
    q0 = C.f32(q - float(DT) * act)
    act = C.f32((q - q0) / float(DT))
    return Cases(synth_arm(A), kind, q, q0, act, C.f32(np.stack([r[2] for r in rows])), C.f32(np.stack([r[3] for r in rows])))


# ---- demonstrations: paths through the constructed poses --------------------------------------------------------------------------
DEMO_N, DEMO_T = 8, 16
DEMO_KINDS = ("target_in", "obstacle_in", "self_in", "cell_in", "reached_self", "obstacle_self", "target_out", "self_out")


class DemoCase:
    """what test_chain_demo_gpu.DemoRig and chain_demo_common.rows32 read of a case"""

    def __init__(self, arm, plan, targets, obstacles, tick, kind):
        self.name, self.model, self.twin = arm.name, arm.model, arm.twin
        self.N, self.T_cap, self.plan, self.targets, self.obstacles = len(targets), DEMO_T, plan, targets, obstacles
        self.tick, self.kind = tick, kind           # the row whose step arrives on the constructed pose, and what it was built as


@functools.lru_cache(maxsize=None)
def build_demo_case(legs):
    """DEMO_N demonstrations of iiwa_like7 among its boxes, DEMO_T rows at most: each runs `legs` legs (2 or 3) whose first `legs - 1`
    end exactly on a constructed pose of build_cases("iiwa_like7") — one of every kind of DEMO_KINDS — after 5 ticks (3 + 2 for
    three legs), through poses the twin finds clear of every band, and goes on for 6 ticks behind it."""
    import chain_cell_common as K
    import chain_rollout_common as C
    from robotic_manipulator_rloa_amd.environment.polyline import demonstration_plan_legs
    from robotic_manipulator_rloa_amd.environment.urdf_chain import DT
    cases = build_cases("iiwa_like7")
    arm = cases.arm
    tol = C.tol_of(arm.model)
    rng = np.random.default_rng(SEED + 200 + legs)
    lo, hi = C.limits_of(arm.model)
    nodes, targets, obstacles, kinds = [], [], [], []
    ticks = (5,) if legs == 2 else (3, 2)
    for kind in DEMO_KINDS:
        of_kind = np.nonzero(cases.kind == kind)[0]
        e = int(of_kind[np.argmax(np.minimum(cases.q[of_kind] - lo, hi - cases.q[of_kind]).min(axis=1))])     # the one furthest inside the limits
        q, tg, ob = cases.q[e], cases.target[e], cases.obstacle[e]

        def inward(p):
            """a direction of max norm 0.97 that leads a joint within 0.05 of a limit away from it"""
            d = rng.uniform(-1.0, 1.0, arm.model.A)
            d = np.where(p - lo < 0.05, np.abs(d), np.where(hi - p < 0.05, -np.abs(d), d))
            return 0.97 * d / np.abs(d).max()

        for _ in range(400):
            back = []
            p = q
            for n in reversed(ticks):
                p = p + n * DT * inward(p)
                back.append(p)
            path = back[::-1] + [q, q + 6 * DT * inward(q)]
            if any(np.any(p < lo + 1e-4) or np.any(p > hi - 1e-4) for p in path):
                continue
            path = C.f32(np.stack(path))
            plan = demonstration_plan_legs(path[None], np.array([len(path)]), 1.0, DEMO_T)
            if tuple(plan.n_ticks[0]) != ticks + (6,):
                continue
            # the poses before the constructed one: clear of every band (the twin alone)
            way = np.concatenate([np.linspace(path[k], path[k + 1], n, endpoint=False) for k, n in enumerate(ticks)])
            m = K.margins4(arm.twin, way, tg, np.broadcast_to(ob, (len(way), 3)))
            if np.all(m > 8 * tol):
                break
        else:
            raise AssertionError(f"no clear approach to the {kind} pose")
        nodes.append(path)
        targets.append(tg)
        obstacles.append(ob)
        kinds.append(kind)
    nodes = np.stack(nodes)
    plan = demonstration_plan_legs(nodes, np.full(DEMO_N, nodes.shape[1]), 1.0, DEMO_T)
    return DemoCase(arm, plan, np.stack(targets), np.stack(obstacles), sum(ticks) - 1, np.array(kinds))


def judge_demo_rows(case, rows, tol, defect=None, reward_tol=None):
    """judge() on every written row of rows[N, T, row floats] up to and including the first done of each demonstration: the pose is
    the row's own next_state joint columns, the target distance that of its own end-effector and target columns; the clearances are
    the twin's at that pose. Returns (census, rows judged, whether every constructed row was among them)."""
    from robotic_manipulator_rloa_amd.environment.kinematic import demo_row_layout
    arm = arm_of("iiwa_like7")
    A = arm.model.A
    S, off_s2, off_d, rf = demo_row_layout(A)
    rows = np.asarray(rows, np.float64)
    q, tg, ob, rw, dn, built = [], [], [], [], [], []
    for n in range(case.N):
        for t in range(rows.shape[1]):
            r = rows[n, t]
            if np.isnan(r[0]):
                break
            q.append(r[off_s2:off_s2 + A])
            tg.append(r[off_s2 + 2 * A + 3:off_s2 + 2 * A + 6])
            ob.append(r[off_s2 + 2 * A + 6:off_s2 + S])
            rw.append(r[S + A])
            dn.append(r[off_d])
            built.append(t == case.tick)
            if r[off_d] != 0.0:
                break
    q, tg, ob = np.array(q), np.array(tg), np.array(ob)
    dist = distances(arm, q, tg, ob)
    census = judge(arm, dist, np.array(rw), np.array(dn), tol if reward_tol is None else reward_tol, np.array(built), defect=defect,
                   band_tol=tol)
    return census, len(rw), int(np.sum(built)) == case.N


# ---- hindsight: a synthetic ring with rows put at the threshold --------------------------------------------------------------------
HINDSIGHT_SHAPE, HINDSIGHT_HORIZON, HINDSIGHT_RATIO = (23, 7, 3), 8, 1.0
HINDSIGHT_PER_SIDE = 8


@functools.lru_cache(maxsize=None)
def hindsight_cases():
    """(ring, idx, u, k0, built[n]): hindsight_common's synthetic ring (23, 7, E = 3) and index buffer at horizon 8, ratio 1, with
    2 x HINDSIGHT_PER_SIDE of the gathered rows moved to the threshold: the end effector of such a row's next_state is put at
    (0.05 -/+ delta) from the goal the relabelling will take for it, delta = 16 x the hindsight suite's band (1e-6). Which goal is
    taken depends on tags and contact rewards alone, so the edit changes no choice. built: +1 / -1 for a row put outside / inside,
    0 for the rest (random filler)."""
    import hindsight_common as HC
    from oracle import naf_oracle as O
    from robotic_manipulator_rloa_amd.utils import hindsight as H
    S, A, E = HINDSIGHT_SHAPE
    base = HC.synthetic_ring(S, A, E)
    idx = HC.case_indices(base.size)
    u, k0 = HC.hindsight_draw(HC.SEED, HC.COUNTER, idx.size, HC.ROWS_PER_BATCH, HINDSIGHT_HORIZON)
    _, k = H.relabel_rows(base.deque, idx, u, k0, E, HINDSIGHT_HORIZON, HINDSIGHT_RATIO, S, A)
    ee2 = O.row_offsets(S, A)[2] + 2 * A
    deque = base.deque.copy()
    rng = np.random.default_rng(SEED + 300)
    delta = 16 * HC.BAND
    built = np.zeros(idx.size, np.int64)
    rows_used, sources = set(), set(int(i) + int(kk) * E for i, kk in zip(idx, k) if kk >= 0)
    made = {1: 0, -1: 0}
    for n in rng.permutation(idx.size):
        i, kk = int(idx[n]), int(k[n])
        side = 1 if made[1] <= made[-1] else -1
        if kk <= 0 or i in rows_used or i in sources or made[side] >= HINDSIGHT_PER_SIDE:
            continue
        g = deque[i + kk * E, ee2:ee2 + 3].astype(np.float64)
        deque[i, ee2:ee2 + 3] = (g + (R.TARGET_THRESHOLD + side * delta) * _unit(rng)).astype(np.float32)
        rows_used.add(i)
        built[n] = side
        made[side] += 1
    assert made == {1: HINDSIGHT_PER_SIDE, -1: HINDSIGHT_PER_SIDE}, made
    ring = HC.Ring()
    for name in ("S", "A", "E", "capacity", "size", "rf", "head", "env", "episode", "tick"):
        setattr(ring, name, getattr(base, name))
    ring.deque = deque
    ring.phys = np.roll(deque, ring.head, axis=0)
    return ring, idx, u, k0, built


def judge_hindsight(plain, got, k, built, defect=None):
    """failures and census of relabelled rows got[n, ld] against the plain gather of the same indices: a row the kernel says it
    relabelled (k >= 0) carries env_oracle.relabelled of the distance between its own next_state end-effector and goal columns —
    done and +250 exact, the shaped reward within the hindsight suite's 1e-5 — outside its band |d - 0.05| < 1e-6; every other row,
    the contact rows among them, is the plain gather's byte for byte, and no contact row is relabelled."""
    import hindsight_common as HC
    from oracle import naf_oracle as O
    S, A, _ = HINDSIGHT_SHAPE
    _, off_r, off_s2, off_d = O.row_offsets(S, A)
    ee2, goal = off_s2 + 2 * A, off_s2 + 2 * A + 3
    failures, band, band_built, compared = [], 0, 0, 0
    for n in range(len(got)):
        contact = plain[n, off_r] == np.float32(R.CONTACT_REWARD)
        if k[n] < 0 or contact:
            if k[n] >= 0 or got[n].tobytes() != plain[n].tobytes():
                failures.append((n, "touched", int(k[n]), bool(contact)))
            continue
        d = float(np.linalg.norm(got[n, ee2:ee2 + 3].astype(np.float64) - got[n, goal:goal + 3].astype(np.float64)))
        if abs(d - R.TARGET_THRESHOLD) < HC.BAND:
            band += 1
            band_built += int(built[n] != 0)
            continue
        compared += 1
        want_r, want_d = R.relabelled(d, False) if defect is None else R.rule(d, [R.MAX_DISTANCE], [], False, defect=defect, involved=[0])
        ok = float(got[n, off_d]) == float(want_d) and (float(got[n, off_r]) == want_r if isinstance(want_r, int) else
                                                         got[n, off_r] != 250.0 and abs(float(got[n, off_r]) - want_r) <= 1e-5)
        ok = ok and np.array_equal(got[n, 2 * A + 3:2 * A + 6], got[n, goal:goal + 3])
        if not ok:
            failures.append((n, d, float(got[n, off_r]), float(got[n, off_d]), want_r, want_d))
    return failures, dict(compared=compared, band=band, band_built=band_built)


# ---- the checker's two drivers, shared by the CPU rehearsal (float32 restatements) and the GPU suite (the kernels) -----------------
def run_step(cases, rig, tol, defect=None):
    """One training step of every case through a stepper with chain_limits_common.Restatement's face (read, write_state, step; the row
    offsets): the envs are put on the cases' start poses and scenes by writing env_state, as the existing step tests do, and stepped
    with the cases' actions. The pose judged is the one the ROW reports — its next_state joint slots — and the scene its own
    columns'. Returns (census of reward and done, failures of the next_state's layout, failures of the reported pose itself:
    within 2^-23 max(1, |q|) of q0 + a / 240)."""
    arm = cases.arm
    A, S = arm.model.A, arm.model.state_size
    slot = np.array([j.slot for j in arm.model.joints])
    assert np.all(slot >= 0)
    st, _ = rig.read()
    st[:, :A], st[:, A:A + 3], st[:, A + 3:A + 6] = cases.q0, cases.target, cases.obstacle
    rig.write_state(st)
    row = np.array(rig.step(cases.act.astype(np.float32)))
    s2 = row[:, rig.off_s2:rig.off_s2 + S]
    q, qd = s2[:, slot].astype(np.float64), s2[:, A + slot].astype(np.float64)
    want_q = cases.q0 + DT_F64 * cases.act
    pose = [e for e in range(len(q)) if not np.all(np.abs(q[e] - want_q[e]) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want_q[e])))]
    dist = distances(arm, q, cases.target, cases.obstacle)
    census = judge(arm, dist, row[:, rig.off_r], row[:, rig.off_d], tol, cases.constructed, defect=defect)
    return census, judge_state(arm, q, qd, dist, cases.target, cases.obstacle, s2, tol, defect=defect), pose


DT_F64 = 1.0 / 240.0


def judge_rollout(cases, outs, traj, tol, defect=None):
    """outs: naf_chain_env_rollout_step's outcome[E, 8] after each of T launches (the case's action, then none); traj[T + 1, E, A] the
    recorded poses. Per launch, every env still running is judged at its recorded pose: outcome code (0 none, 1 reached, 2 / 3 / 4 a
    contact), whether it ended, and the score's increment — exact for the first launch (the score starts at 0), within tol plus the
    float32 rounding of the running sum, 2^-23 |score|, afterwards. An env that ended is HELD: its outcome row keeps its bits.
    Returns the per-launch censuses and the envs that were not held."""
    arm = cases.arm
    n = len(cases.q)
    censuses, not_held = [], []
    live = np.ones(n, bool)
    prev = np.zeros((n, 8), np.float32)
    for t, out in enumerate(outs):
        out = np.asarray(out, np.float32)
        not_held += [(t, e) for e in np.nonzero(~live)[0] if out[e].tobytes() != prev[e].tobytes()]
        dist = distances(arm, np.asarray(traj[t + 1], np.float64), cases.target, cases.obstacle)
        inc = out[:, 5].astype(np.float64) - prev[:, 5].astype(np.float64)
        slack = 0.0 if t == 0 else 2.0 ** -23 * np.abs(out[:, 5]).max()
        sub = _take(dist, live)
        c = judge(arm, sub, inc[live], (out[live, 0] != 0).astype(float), tol + slack, cases.constructed[live] & (t == 0),
                  defect=defect, code=out[live, 0].astype(int), band_tol=tol)
        c.failures = [(t,) + f for f in c.failures] + [(t, e, "frames", float(out[e, 1])) for e in np.nonzero(live)[0] if out[e, 1] != t + 1]
        censuses.append(c)
        live = live & (out[:, 0] == 0)
        prev = out
    return censuses, not_held


def _take(dist, mask):
    return Distances(dist.d_target[mask], dist.d_links[mask], dist.d_self[mask], dist.moved, dist.ee[mask])

"""Shared by tests/test_chain_limits_cpu.py and tests/test_chain_limits_gpu.py: the case table that drives every limited joint of
seven arms onto, along and off its position limits (and the unlimited joints of standin8 past +-pi), the float64 statement of the
step's joint rule — q <- clamp(q + a / 240) into the float32 limits the blob carries, a joint its limit stops reports velocity 0 in
its slot — and the check both suites apply to what a stepper returned: a float32 numpy restatement of the step (the CPU rehearsal)
or the kernels of csrc/chain_env.hip (step, tagged step, rollout step, demonstration ticks)."""
import functools

import numpy as np

import chain_ik_common as IK
import chain_rollout_common as C
from oracle import naf_oracle as O
from test_chain_env_cpu import model_of

from robotic_manipulator_rloa_amd.environment.kinematic import PRISMATIC, DemonstrationPlan, KinematicEnvironment
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

ORAD = C.ORAD
T = 3                               # steps of a case's one constant action
CLEARANCE = 0.01                    # self- and workcell clearance every pose of a case keeps: no episode ends, nothing resets
SURE_CONTACT = 0.002                # ... or, in a `contact` case, is inside contact by: every step ends the episode
KINDS = ("stop", "short", "held", "released", "rest")
# the step's rule names joint m's limits, its flag, its type and its slot: the arms that tell these apart
ARMS = ["planar3", "iiwa_like7", "arm_with_gripper", "standin8", "slider4", "slider4_sc", "slider4_cell"]
SLIDER_START = dict(initial_joint_positions=[0.0, 0.2, 0.0, 0.15], initial_positions_variation_range=[0.2, 0.05, 0.2, 0.05])
SLIDER_CELL = dict(floor_height=-0.05, workcell_boxes=[(0.45, 0.0, 0.1, 0.05, 0.3, 0.1)])
# the action schedules a case's poses are kept clear of contact under: the T constant steps, and the two demonstration plans of
# tests/test_chain_limits_gpu.py (leg 1 the action, leg 2 its opposite, leg 3 the action again)
DEMO_TICKS = {2: (2, 2), 3: (2, 2, 1)}


@functools.lru_cache(maxsize=None)
def arm(name):
    """(model, twin): planar3 without pairs; iiwa_like7 with self-collision pairs; arm_with_gripper, whose slots are not its action
    indices and whose last driven joint has none; standin8, eight unlimited joints; slider4 (two prismatic joints) bare, with
    pairs, and with pairs, a floor and a box."""
    if name == "slider4":
        return IK.slider()
    if name == "slider4_sc":
        model = model_of("slider4", consider_autocollision=True, **SLIDER_START)
    elif name == "slider4_cell":
        model = model_of("slider4", consider_autocollision=True, **SLIDER_START, **SLIDER_CELL)
    else:
        model = model_of(name, consider_autocollision=(name == "iiwa_like7"))
    return model, KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)


def limits32(model):
    """(lower[A], upper[A]): the float32 values the blob carries, as float64; -inf / +inf for a joint without limits"""
    lo = np.array([float(np.float32(j.lower)) if j.limited else -np.inf for j in model.joints])
    hi = np.array([float(np.float32(j.upper)) if j.limited else np.inf for j in model.joints])
    return lo, hi


# ---- the float64 rule ------------------------------------------------------------------------------------------------------------
def rule(model, q_prev, act):
    """One step of the joint rule in float64 from float32 joint values q_prev[..., A] and float32 actions act[..., A]:
    (q[..., A] the stepped pose inside the float32 limits, stopped[..., A], edge[..., A]). edge: a limited joint under a non-zero
    action whose unclamped sum lies within 4 * 2^-24 * (|q_prev| + 1/240) of a limit — tests/test_chain_rollout_gpu.py's bound on
    the float32 sum — where a float32 stepper may decide either way. With action 0 the sum is q_prev itself, in every arithmetic."""
    lo, hi = limits32(model)
    q_prev, act = np.asarray(q_prev, np.float64), np.asarray(act, np.float64)
    pre = q_prev + act / 240.0
    stopped = (pre > hi) | (pre < lo)
    bound = 4 * 2.0 ** -24 * (np.abs(q_prev) + 1.0 / 240.0)
    with np.errstate(invalid="ignore"):
        edge = (np.minimum(np.abs(pre - lo), np.abs(pre - hi)) <= bound) & (act != 0.0)
    return np.minimum(np.maximum(pre, lo), hi), stopped, edge


def trace(model, q0, actions):
    """The rule along a schedule actions[F, E, A] from q0[E, A], every pose rounded to float32 as a device holds it:
    (poses[F + 1, E, A] float32, stopped[F, E, A], edge[F, E, A])"""
    q = np.asarray(q0, np.float32)
    poses, stopped, edge = [q], [], []
    for a in np.asarray(actions, np.float32):
        q64, s, e = rule(model, q, a)
        q = q64.astype(np.float32)
        poses.append(q)
        stopped.append(s)
        edge.append(e)
    return np.stack(poses), np.stack(stopped), np.stack(edge)


def demo_plan(table, legs):
    """The demonstration plan of the table's cases: leg 1 the case's action, leg 2 its opposite, leg 3 (legs = 3) the action again,
    DEMO_TICKS[legs] ticks each — a stop, a release and a move back that ends one tick short of the limit."""
    ticks = DEMO_TICKS[legs]
    acts = np.stack([table.act if l % 2 == 0 else -table.act for l in range(legs)], axis=1).astype(np.float32)
    n = np.tile(np.array(ticks, np.int32), (table.E, 1))
    return DemonstrationPlan(table.q0.copy(), acts, n, np.full(table.E, sum(ticks)))


def schedules(q0, act):
    """{name: actions[F, E, A]}: every schedule the tests drive a case under"""
    out = {"steps": np.repeat(act[None], T, axis=0)}
    for legs, ticks in DEMO_TICKS.items():
        out[f"legs{legs}"] = np.concatenate([np.repeat((act if l % 2 == 0 else -act)[None], n, axis=0) for l, n in enumerate(ticks)])
    return out


def clearances(twin, poses, largest=False):
    """[E]: the smallest (largest) over each case's poses[F, E, A] of the pose's clearance, the smaller of its self- and workcell
    clearance (+inf without pairs and workcell)"""
    q = np.asarray(poses, np.float64)
    zero = np.zeros(q.shape[:-1])
    c = np.minimum(twin.self_clearance(q) + zero, twin.cell_clearance(q) + zero)
    return np.max(c, axis=0) if largest else np.min(c, axis=0)


# ---- the table --------------------------------------------------------------------------------------------------------------------
class Table:
    """E cases of one arm: q0[E, A] and act[E, A] float32, target[E, 3] and obstacle[E, 3] (float32 values as float64), kind[E],
    joint[E] (-1: every limited joint), side[E] (+1 upper, -1 lower, 0 mixed), want[T, E, A]: whether the step stops the joint, as
    the kind was built — not computed by the rule — and contact[E]: the cases no pose of which can be clear (build_table)."""

    def __init__(self, name, q0, act, kind, joint, side, want, contact):
        self.name, self.E = name, len(q0)
        self.model, self.twin = arm(name)
        self.q0, self.act, self.kind, self.joint, self.side, self.want, self.contact = q0, act, kind, joint, side, want, contact
        tg, ob = C.away(self.model)
        self.target, self.obstacle = np.tile(C.f32(tg), (self.E, 1)), np.tile(C.f32(ob), (self.E, 1))

    def take(self, idx):
        idx = np.asarray(idx)
        return Table(self.name, self.q0[idx], self.act[idx], [self.kind[i] for i in idx], self.joint[idx], self.side[idx],
                     self.want[:, idx], self.contact[idx])

    def first_stop(self):
        """the table of one case: the first `stop` (standin8, which has none: its first case)"""
        return self.take([self.kind.index("stop") if "stop" in self.kind else 0])

    def steps(self):
        """actions[T, E, A]: the case's constant action"""
        return np.repeat(self.act[None], T, axis=0)


def _draw(model, rng, kind, m, side, n):
    """n candidates (q0[n, A], act[n, A], want[T, n, A]) of one table entry. Every joint starts in the interior — 15 % of its range
    from either limit, or anywhere in +-pi without limits — under an action in [-1, 1]; then joint m (every limited joint for
    `all`) is placed by its kind, u and |a| drawn per candidate."""
    A = model.A
    lo, hi = limits32(model)
    limited = np.array([j.limited for j in model.joints])
    w = np.where(limited, hi - lo, 0.0)
    q = np.where(limited, rng.uniform(np.where(limited, lo, 0.0) + 0.15 * w, np.where(limited, hi, 0.0) - 0.15 * w, (n, A)),
                 rng.uniform(-np.pi, np.pi, (n, A)))
    a = rng.uniform(-1.0, 1.0, (n, A))
    want = np.zeros((T, n, A), bool)

    def place(j, s, k):
        """joint j of the candidates, side s[n] (+-1), kind k"""
        mag = rng.uniform(0.25, 1.0, n)
        lim = np.where(s > 0, hi[j], lo[j])
        if k in ("stop", "short"):
            u = rng.uniform(0.25, 0.75, n) + (1.0 if k == "short" else 0.0)
            q[:, j], a[:, j] = lim - s * u * mag / 240.0, s * mag
            want[(1 if k == "short" else 0):, :, j] = True
        elif k == "held":
            q[:, j], a[:, j] = lim, s * mag
            want[:, :, j] = True
        elif k == "released":
            q[:, j], a[:, j] = lim, -s * mag
        elif k == "rest":
            q[:, j], a[:, j] = lim, 0.0
        else:                                         # free: no limits, |q| beyond pi, outward
            q[:, j], a[:, j] = s * rng.uniform(3.2, 6.9, n), s * mag

    if kind == "all":
        sides = rng.choice([-1.0, 1.0], (n, int(limited.sum())))
        sides[np.all(sides == sides[:, :1], axis=1), 0] *= -1.0      # mixed: never every joint on the same side
        for k, j in enumerate(np.nonzero(limited)[0]):
            place(j, sides[:, k], "stop")
    else:
        place(m, np.full(n, float(side)), kind)
    return q.astype(np.float32), a.astype(np.float32), want


@functools.lru_cache(maxsize=None)
def build_table(name):
    """One case per limited joint, side and kind of KINDS, three `all` cases, and for standin8 one `free` case per joint and side.
    With pairs or a workcell a case is the first of a pool of candidates (1024 at the most) all of whose poses, under every
    schedule of `schedules` and by the twin alone, keep CLEARANCE of self- and workcell clearance: no episode ends. Where the pool
    has none — slider4 with pairs touches itself wherever its lift is within 1 cm of its lower limit, whatever the other joints do
    (test_chain_limits_cpu.test_census states it) — the case stays, marked `contact`: the first candidate every stepped pose of
    which is IN contact by SURE_CONTACT or more, so that the step's -1000 / done is as certain as its absence elsewhere."""
    model, twin = arm(name)
    rng = np.random.default_rng(9100 + ARMS.index(name))
    limited = [m for m, j in enumerate(model.joints) if j.limited]
    entries = [(kind, m, side) for m in limited for side in (1, -1) for kind in KINDS]
    entries += [("all", -1, 0)] * (3 if limited else 0)
    if name == "standin8":
        entries += [("free", m, side) for m in range(model.A) for side in (1, -1)]
    guarded = bool(model.self_pairs or model.cell_pairs)
    q0, act, want, contact = [], [], [], []
    for kind, m, side in entries:
        touching = None
        for attempt in range(16):
            q, a, w = _draw(model, rng, kind, m, side, 64 if guarded else 1)
            ok, sure = np.ones(len(q), bool), np.ones(len(q), bool)
            if guarded:
                for sched in schedules(q, a).values():
                    poses = trace(model, q, sched)[0]
                    ok &= clearances(twin, poses) >= CLEARANCE
                    sure &= -clearances(twin, poses[1:], largest=True) >= SURE_CONTACT
            if ok.any():
                i = int(np.argmax(ok))
                q0.append(q[i]), act.append(a[i]), want.append(w[:, i]), contact.append(False)
                break
            if sure.any() and touching is None:
                i = int(np.argmax(sure))
                touching = (q[i], a[i], w[:, i])
        else:
            assert touching is not None, f"{name}: no candidate of {(kind, m, side)} is clear, or in contact, throughout"
            q0.append(touching[0]), act.append(touching[1]), want.append(touching[2]), contact.append(True)
    return Table(name, np.stack(q0), np.stack(act), [e[0] for e in entries], np.array([e[1] for e in entries]),
                 np.array([e[2] for e in entries]), np.stack(want, axis=1), np.array(contact))


# ---- the check of a stepper's answer, the restatement's or a kernel's ---------------------------------------------------------------
class Counts:
    def __init__(self):
        self.stops = self.free = self.edge = 0
        self.worst = 0.0              # largest position error of a free joint over its bound

    def __repr__(self):
        return f"stops {self.stops} free {self.free} edge {self.edge} worst position error {self.worst:.2f} of its bound"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_limits(model, q_prev, act, q_next, obs, counts, want=None, loose=None):
    """One step of a stepper — q_next[E, A] its joint values and obs[E, 2A + 9] its observation after the step, both float32 —
    against the rule from the stepper's own previous joint values q_prev[E, A] under act[E, A]. Nothing here is measured:
      a stopped joint : its joint value, and its position slot if it has one, bit-equal to the float32 limit; its velocity slot 0
      any other joint : its velocity slot bit-equal to the action; its joint value within 2^-23 max(1, |q|) of the float64 sum
                        (one rounding of the sum, tests/test_chain_env_gpu.py's bound), bit-equal to q_prev under action 0; its
                        position slot bit-equal to its joint value
      a joint with slot -1 changes nothing in the observation (the constants' slots are check_step's).
    An `edge` entry may go either way and is counted; the callers hold the count. want[E, A]: the verdicts the cases were built
    for, which the rule must give from the stepper's values too — but for the entries of `loose`[E, A], which the caller expects
    at an edge. Returns (stopped, edge)."""
    A = model.A
    q_prev, act, q_next, obs = (np.asarray(v, np.float32) for v in (q_prev, act, q_next, obs))
    assert q_next.shape == q_prev.shape == act.shape and obs.shape == q_prev.shape[:-1] + (2 * A + 9,)
    q64, stopped, edge = rule(model, q_prev, act)
    if want is not None:
        skip = edge if loose is None else edge | loose
        assert np.array_equal(stopped | skip, want | skip), np.argwhere((stopped != want) & ~skip)
    lo, hi = limits32(model)
    pre = q_prev.astype(np.float64) + act.astype(np.float64) / 240.0
    lim = np.where(np.abs(pre - lo) <= np.abs(pre - hi), lo, hi).astype(np.float32)      # the float32 limit a stop puts the joint on
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(q64))
    err = np.abs(q_next.astype(np.float64) - q64)
    as_stopped = bits(q_next) == bits(lim)
    as_free = (err <= bound) & ((act != 0.0) | (bits(q_next) == bits(q_prev)))
    vel_zero, vel_act = np.zeros_like(as_free), np.zeros_like(as_free)
    pos_ok = np.ones_like(as_free)
    for m, j in enumerate(model.joints):
        if j.slot >= 0:
            pos_ok[..., m] = bits(obs[..., j.slot]) == bits(q_next[..., m])
            vel_zero[..., m] = obs[..., A + j.slot] == 0.0
            vel_act[..., m] = bits(obs[..., A + j.slot]) == bits(act[..., m])
        else:
            vel_zero[..., m] = vel_act[..., m] = True
    good_stop, good_free = as_stopped & vel_zero & pos_ok, as_free & vel_act & pos_ok
    ok = np.where(edge, good_stop | good_free, np.where(stopped, good_stop, good_free))
    assert np.all(ok), [(tuple(i), bool(stopped[tuple(i)]), float(q_prev[tuple(i)]), float(act[tuple(i)]), float(q_next[tuple(i)]),
                         float(q64[tuple(i)])) for i in np.argwhere(~ok)[:4]]
    # a slot that reports a joint reports this one: every driven slot was compared above, through its joint
    assert sorted(j.slot for j in model.joints if j.slot >= 0) == [k for k, (src, _) in enumerate(model.slots) if src >= 0]
    sure = ~edge
    counts.stops += int(np.sum(stopped & sure))
    counts.free += int(np.sum(~stopped & sure))
    counts.edge += int(np.sum(edge))
    if np.any(~stopped & sure):
        counts.worst = max(counts.worst, float(np.max((err / bound)[~stopped & sure])))
    return stopped, edge


# ---- the float32 restatement of the step ---------------------------------------------------------------------------------------------
DEFECTS = ("velocity_kept", "wrong_slot", "one_side", "flag_ignored", "clamp_after_walk", "neighbour_limits", "prismatic_as_revolute")


def walk32(model, q, prismatic_as_revolute=False):
    """the end effector at q[E, A], every operation in float32 (chain_ik_common.walk32's walk, over the joints before the
    end-effector frame)"""
    f = np.float32
    q = np.asarray(q, f)
    R, p = np.broadcast_to(np.eye(3, dtype=f), q.shape[:-1] + (3, 3)), np.zeros(q.shape[:-1] + (3,), f)
    for m, j in enumerate(model.joints[:model.ee_frame]):
        p = p + R @ j.pre_xyz.astype(f)
        R = R @ j.pre_rot.astype(f)
        if j.type == PRISMATIC and not prismatic_as_revolute:
            p = p + (R @ j.axis.astype(f)) * q[..., m, None]
        else:
            x, y, z = (f(v) for v in j.axis)
            s, c = np.sin(q[..., m]), np.cos(q[..., m])
            v = f(1.0) - c
            rot = np.stack([np.stack([f(1.0) - v * (y * y + z * z), v * x * y - s * z, v * x * z + s * y], -1),
                            np.stack([v * x * y + s * z, f(1.0) - v * (x * x + z * z), v * y * z - s * x], -1),
                            np.stack([v * x * z - s * y, v * y * z + s * x, f(1.0) - v * (x * x + y * y)], -1)], -2)
            R = R @ rot
    out = p + R @ model.ee_point.astype(f)
    assert out.dtype == f
    return out




class Restatement:
    """The step in float32 numpy behind the face `drive` asks for (m, E, A, S, the row offsets, read, write_state, step): one fused
    q + a / 240 (the float64 sum of the exact product rounded once), the clamp into the blob's float32 limits, a float32 walk,
    reward and done by the twin's clearances at the stepped pose, and an env whose episode ended back on its initial pose.
    `defect`: one of DEFECTS, planted."""

    def __init__(self, model, twin, E, defect=None):
        assert defect is None or defect in DEFECTS
        self.m, self.twin, self.E, self.A, self.S, self.defect = model, twin, E, model.A, model.state_size, defect
        A = self.A
        self.nst = -(-(-(-(A + 9) // 2) * 2 + 2) // 4) * 4
        _, self.off_r, self.off_s2, self.off_d = O.row_offsets(self.S, A)
        self.rf = 32
        while self.rf < self.off_d + 1:
            self.rf *= 2
        self.st = np.zeros((E, self.nst), np.float32)
        self.obs = np.zeros((E, self.S), np.float32)
        self.st[:, A + 6] = ORAD

    def read(self):
        return self.st.copy(), self.obs.copy()

    def write_state(self, st):
        self.st[:] = st

    def _observe(self, o, q, vel, walked, scene):
        m, A, d = self.m, self.A, self.defect
        for k, j in enumerate(m.joints):
            if d == "wrong_slot":
                o[:, A + k] = vel[:, k]
            elif j.slot >= 0:
                o[:, A + j.slot] = vel[:, k]
            if j.slot >= 0:
                o[:, j.slot] = q[:, k]
        for k, (src, const) in enumerate(m.slots):
            if src < 0:
                o[:, k], o[:, A + k] = const, 0.0
        ee = walk32(m, walked, d == "prismatic_as_revolute")
        o[:, 2 * A:2 * A + 3], o[:, 2 * A + 3:] = ee, scene
        return ee

    def step(self, act):
        m, A, S, E, d = self.m, self.A, self.S, self.E, self.defect
        f = np.float32
        act = np.asarray(act, f)
        blob = [(1.0 if j.limited else 0.0, f(j.lower), f(j.upper)) for j in m.joints]      # flag | lower | upper as packed
        if d == "neighbour_limits":
            blob = blob[1:] + blob[:1]
        pre = (np.float64(f(DT)) * act.astype(np.float64) + self.st[:, :A].astype(np.float64)).astype(f)
        q, vel = pre.copy(), act.copy()
        for k, (flag, lower, upper) in enumerate(blob):
            if flag != 0.0 or d == "flag_ignored":
                over, under = q[:, k] > upper, (q[:, k] < lower) & (d != "one_side")
                q[over, k], q[under, k] = upper, lower
                if d != "velocity_kept":
                    vel[over | under, k] = 0.0
        row = np.zeros((E, self.rf), f)
        row[:, :S], row[:, S:S + A] = self.obs, act
        o2 = row[:, self.off_s2:self.off_s2 + S]
        ee = self._observe(o2, q, vel, pre if d == "clamp_after_walk" else q, self.st[:, A:A + 6])
        delta = ee - self.st[:, A:A + 3]
        dist = np.sqrt(np.sum(delta * delta, axis=1, dtype=f))
        q64 = q.astype(np.float64)
        hit = (clearances(self.twin, q64[None]) < 0.0) | (self.twin.clearance(q64, self.st[:, A + 3:A + 6].astype(np.float64)) < ORAD)
        row[:, self.off_r] = np.where(dist < f(0.05), f(250.0), np.where(hit, f(-1000.0), -(dist - f(0.05))))
        row[:, self.off_d] = over = (dist < f(0.05)) | hit
        self.st[:, :A] = q
        self.st[:, A + 7] += 1.0
        self.obs[:] = o2
        if over.any():
            n = int(over.sum())
            start = np.tile(np.array([j.init for j in m.joints], f), (n, 1))
            self.st[over, :A], self.st[over, A + 7] = start, 0.0
            self.st[over, A + 8] += 1.0
            o = np.zeros((n, S), f)
            self._observe(o, start, np.zeros((n, A), f), start, self.st[over, A:A + 6])
            self.obs[over] = o
        return row


def drive(table, rig, counts, tally, tag=False):
    """The table's T steps through a stepper with Restatement's face, teacher-forced: the scene and q0 are written into env_state as
    the existing step tests write them, and every step is held to the rule from the stepper's OWN previous env_state.
      every case    : check_limits on the row's next_state against the verdicts the case was built for; with `tag`, the row's last
                      float is the episode ordinal (then cleared for the checks below).
      a clear case  : test_chain_env_gpu.check_step on the row (end effector, scene, reward, done, padding, constants' slots); done 0;
                      obs_next is the row's next_state; env_state's joints are those check_limits saw; frame + 1, episodes unchanged.
      a contact case: the row carries the stepped pose — its joints are read from the row's position slots — with the end effector
                      within tol, the scene, -1000 and done 1; the env then starts an episode: frame 0, one more finished, joints
                      inside init +- variation (1e-6, tests/test_chain_cell_gpu.py's), velocity slots 0, position slots env_state's
                      bits. Before its next step its joints are put on the next pose of the rule's own trace."""
    from test_chain_env_gpu import check_step
    model, twin, A, S = table.model, table.twin, table.model.A, table.model.state_size
    tol = 16 * A * 2.0 ** -24 * model.reach
    hit, clear = table.contact, ~table.contact
    n_clear = int(clear.sum())
    sub = type("Clear", (), dict(m=model, A=A, S=S, E=n_clear, off_r=rig.off_r, off_s2=rig.off_s2, off_d=rig.off_d))
    poses = trace(model, table.q0, table.steps())[0]
    init, var = np.array([j.init for j in model.joints]), np.array([j.variation for j in model.joints])
    slot = np.array([j.slot for j in model.joints])
    assert not hit.any() or np.all(slot >= 0)
    for t in range(T):
        prev, _ = rig.read()
        if t == 0:
            prev[:, :A], prev[:, A:A + 3], prev[:, A + 3:A + 6] = table.q0, table.target, table.obstacle
        prev[hit, :A] = poses[t][hit]
        rig.write_state(prev)
        row = np.array(rig.step(table.act))
        now, obs = rig.read()
        if tag:
            assert np.array_equal(row[:, -1], prev[:, A + 8] + 1.0)
            row[:, -1] = 0.0
        s2 = row[:, rig.off_s2:rig.off_s2 + S]
        q_next = now[:, :A].copy()
        q_next[hit] = s2[hit][:, slot]
        check_limits(model, prev[:, :A], table.act, q_next, s2, counts, table.want[t])
        if n_clear:
            check_step(sub, twin, prev[clear, :A], table.act[clear], row[clear], table.target[clear], table.obstacle[clear], tol, tally)
            assert np.all(row[clear, rig.off_d] == 0.0) and np.array_equal(bits(obs[clear]), bits(s2[clear]))
            assert np.array_equal(now[clear, A + 7], prev[clear, A + 7] + 1.0) and np.array_equal(now[clear, A + 8], prev[clear, A + 8])
        if hit.any():
            q = q_next[hit].astype(np.float64)
            assert clearances(twin, q[None]).max() <= -SURE_CONTACT
            assert np.abs(s2[hit, 2 * A:2 * A + 3] - twin.end_effector(q)).max() <= tol
            assert np.array_equal(bits(s2[hit, 2 * A + 3:]), bits(prev[hit, A:A + 6]))
            assert np.array_equal(bits(row[hit, S:S + A]), bits(table.act[hit]))
            assert np.all(row[hit, S + A + 1:rig.off_s2] == 0.0) and np.all(row[hit, rig.off_d + 1:] == 0.0)
            assert np.all(row[hit, rig.off_r] == -1000.0) and np.all(row[hit, rig.off_d] == 1.0)
            assert np.all(now[hit, A + 7] == 0.0) and np.array_equal(now[hit, A + 8], prev[hit, A + 8] + 1.0)
            assert np.all(np.abs(now[hit, :A] - init) <= var + 1e-6)
            assert np.array_equal(bits(obs[hit][:, slot]), bits(now[hit, :A])) and np.all(obs[hit][:, A + slot] == 0.0)
    return counts

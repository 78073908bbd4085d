"""Shared by tests/test_chain_ik_clear_cpu.py and tests/test_chain_ik_clear_gpu.py: the arms and cases that hold naf_chain_ik_clear
(csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (least_test, clearance_gradient, ik_clear_step,
refine_goal_poses), built with the twin alone; a float32 numpy rehearsal of the refinement that stands in for the device on the CPU
— a float32 walk of its own, then the rule's arithmetic (the *_of functions, which compute in the type they are given) on float32
arrays; and the checks both suites apply to what a refiner — that rehearsal, or the kernel — returned."""
import functools

import numpy as np

import chain_box_common as BX
import chain_cell_common as CK
import chain_ik_common as IK
import chain_rollout_common as C
from test_chain_env_cpu import model_of, random_q

from robotic_manipulator_rloa_amd.environment import contact_push as KM
from robotic_manipulator_rloa_amd.environment.kinematic import PRISMATIC, KinematicEnvironment

ORAD = IK.ORAD
K, SETTLE, PUSH_MAX = KM.CLEAR_ITERATIONS, KM.CLEAR_SETTLE, KM.CLEAR_PUSH_MAX
MARGIN = 0.0
GOAL = float(np.float32(MARGIN + KM.CLEAR_GOAL_OVER_MARGIN))
TOLERANCE = IK.TOLERANCE
CAP, FLOOR = C.CAP, C.FLOOR
COUNTS = IK.COUNTS + [(65, 1)]                       # the IK suite's counts, and one candidate in a second wave's first lane
ARMS = ["planar3", "iiwa_bare", "iiwa_like7", "arm_with_gripper", "slider4", "long12"]
CASES = [(name, N, R) for name in ARMS for N, R in IK.COUNTS] + [("iiwa_like7", 65, 1)]

# What test_chain_ik_clear_cpu.test_rehearsal measures over every recorded update of every case, the float32 rehearsal against the
# float64 rule at the same recorded pose (updates whose least and second-least tests lie within BAND of each other left out):
#     single update, max-norm over the joints   planar3 2.1e-5, iiwa_bare 6.8e-5, iiwa_like7 4.7e-5, arm_with_gripper 4.4e-5,
#                                               slider4 7.0e-6, long12 5.1e-5                                  -> STEP_DEVIATION 7e-5
#     gradient gamma, max-norm                  planar3 4.6e-7, iiwa_bare 1.7e-6, iiwa_like7 3.5e-6, arm_with_gripper 1.5e-5,
#                                               slider4 1.5e-6, long12 2.1e-7                                  -> GAMMA_DEVIATION 1.6e-5
#     least clearance c                         planar3 7.3e-8, iiwa_bare 2.1e-7, iiwa_like7 1.3e-7, arm_with_gripper 1.4e-7,
#                                               slider4 9.9e-8, long12 1.1e-7                                  -> CLEAR_DEVIATION 3e-7
# each rounded up. The GPU bounds are 8 x those, the project's convention: a second float32 evaluation of the same expressions differs
# from the first by the same mechanism and no more than a small multiple of it. They come from the rehearsal, never from the kernel.
# (The single update is largest where sigma is small — the push divides by it — and the gradient where the witness distance is
# small: n is a difference of two nearby points over its length.)
STEP_DEVIATION, GAMMA_DEVIATION, CLEAR_DEVIATION = 7e-5, 1.6e-5, 3e-7
STEP_BOUND, GAMMA_BOUND, CLEAR_BOUND = 8 * STEP_DEVIATION, 8 * GAMMA_DEVIATION, 8 * CLEAR_DEVIATION
BAND = 8 * CLEAR_DEVIATION            # least and second-least test closer than this: either may be the device's least, the update is left out
GRADIENT_GAP = 1e-3                   # the CPU gradient check keeps this far from a kink (central differences of step 1e-6 cross none)


def f32(x):
    return C.f32(x)


@functools.lru_cache(maxsize=None)
def arm(name):
    """(model, twin): planar3 and iiwa_bare without pairs or workcell; iiwa_like7 with self-collision among chain_cell_common's
    sphere and floor and three boxes — the table top, the shelf with rounded edges, the post (a capsule: zero half extents across,
    a rounding radius); arm_with_gripper with self-collision and the end effector on joint index 4, so two driven joints and
    the gripper's capsules lie behind the end-effector frame (iiwa_like7's own capsules never come within 14 mm of each other); slider4 (two prismatic joints); long12 on a floor 7 cm below its base."""
    if name == "slider4":
        return IK.slider()
    if name == "long12":      # (with its self pairs every pose near long12's initial one leans on several at once: its own case is the
        model = model_of(name, floor_height=-0.07)      # floor, 7 cm down: the base, which nothing moves, keeps 4 cm, not the goal's 2)
        return model, KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)
    if name == "iiwa_like7":
        boxes = BX.boxes_of(name)
        boxes[1] = boxes[1][:9] + (0.02,)
        model = model_of(name, **dict(CK.workcell_of(name), workcell_boxes=boxes))
    elif name == "arm_with_gripper":
        model = model_of(name, endeffector_index=4, consider_autocollision=True)
    else:
        model = model_of("iiwa_like7" if name == "iiwa_bare" else name)
    return model, KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), ORAD)


def constants(model):
    return IK.constants(model)


def twin_kw(model):
    c = constants(model)
    return dict(lam=c["lam"], e_max=c["e_max"], dq_max=c["dq_max"], clearance_goal=GOAL, iterations=K, settle=SETTLE, push_max=PUSH_MAX)


SEEDS = {}      # (name, N, R) -> a seed other than 0, where a small case drew a kink into its handful of freed candidates


class Case:
    """N queries x R candidates of one arm, float32 values held as float64: targets[N, 3], obstacles[N, 3], q_in[N R, A] the
    candidates' poses — a float64 solve rounded to float32, what the solve launch would hand over."""

    def __init__(self, name, N, R, targets, obstacles, q_in):
        self.name, self.N, self.R, self.targets, self.obstacles, self.q_in = name, N, R, targets, obstacles, q_in
        self.model, self.twin = arm(name)

    @property
    def g(self):
        return np.repeat(self.targets, self.R, axis=0)

    @property
    def ob(self):
        return np.repeat(self.obstacles, self.R, axis=0)

    @functools.lru_cache(maxsize=None)
    def twin_refined(self):
        """refine_goal_poses of the case by the float64 rule, recorded: computed once, shared, never changed"""
        kw = twin_kw(self.model)
        out = KM.refine_goal_poses(self.twin, self.q_in, self.g, self.ob, TOLERANCE, MARGIN, GOAL, K, SETTLE, PUSH_MAX, kw["lam"],
                                   kw["e_max"], kw["dq_max"], record=True)
        for a in out:
            a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def build_case(name, N, R, seed=None):
    """Targets on the end effector of drawn poses; every candidate solved by the float64 rule from a seed near that pose, so most
    converge. Query n's obstacle: n mod 3 == 0 away from the arm; n mod 3 == 1 pressed 2 .. 30 mm into a drawn capsule — one that a joint
    moves — of the pose its restart n mod R solved: that candidate leans on it; n mod 3 == 2 pressed 2 .. 12 mm into one behind the second joint (slider4: 2 .. 5 mm both times), the
    query's seeds 0.05 rad around one pose: every restart solves nearly the same pose and the whole query leans on it. Arms
    with a workcell lean on it by themselves; with pairs every sixth query is solved for a pose that nearly touches itself."""
    model, twin = arm(name)
    rng = np.random.default_rng(9100 + 131 * N + R + SEEDS.get((name, N, R), 0) if seed is None else seed)
    lo, hi = C.limits_of(model)
    q_goal = np.stack([random_q(model, rng) for _ in range(N)])
    spread = np.full(N, 0.4)
    if name == "long12":      # (two queries in three: a pose that leans on the floor or nearly does, and seeds close to it)
        pool = np.stack([random_q(model, rng) for _ in range(400 * N)])
        cc = twin.cell_clearance(pool)
        pool = pool[(cc > -0.02) & (cc < 0.015)]
        rows = np.nonzero(np.arange(N) % 3 != 0)[0][:len(pool)]
        q_goal[rows], spread[rows] = pool[:len(rows)], 0.01
    if name == "planar3":     # (a planar arm folded back lays two links on top of each other: both are then equally far from anything)
        q_goal[:, 1:] = np.clip(q_goal[:, 1:], -1.5, 1.5)
    if model.self_pairs:      # every sixth query: a pose that nearly touches itself, and seeds close to it
        pool = np.stack([random_q(model, rng) for _ in range(400 * N)])
        sc = twin.self_clearance(pool)
        pool = pool[(sc > -0.02) & (sc < 0.015) & (twin.cell_clearance(pool) + np.zeros(len(pool)) > 0.03)]
        rows = np.arange(0, N, 6)[:len(pool)]
        q_goal[rows], spread[rows] = pool[:len(rows)], 0.01
    if name != "long12":
        spread[2::3] = 0.05   # (the queries that lean as a whole: every restart solves nearly the same pose)
    if name == "slider4":     # (one spare degree of freedom frees few candidates: its other pressed queries start close together too)
        spread[1::3] = 0.1
    targets = f32(twin.end_effector(f32(q_goal)))
    seeds = f32(np.clip(q_goal[:, None, :] + spread[:, None, None] * rng.normal(size=(N, R, model.A)), lo, hi))
    q, _ = twin.solve_ik(targets[:, None, :], seeds, iterations=IK.K, **IK.twin_constants(model))
    q_in = f32(q)
    obstacles = np.tile(C.away(model)[1], (N, 1)).astype(np.float64)
    for n in range(N):
        if n % 3 == 0 or name == "long12":      # (long12's links are as short as the obstacle's radius: pressed into one capsule it is
            continue                            # as near to the next, and the case would sit at kinks; its case is the floor)
        segs = [seg for seg, s in zip(twin.world_segments(q_in[n, n % R]), model.segments)
                if s.frame >= (1 if n % 3 == 1 else min(2, model.ee_frame)) and np.any(s.a != s.b)]
        a, b, r = segs[rng.integers(len(segs))]      # (a capsule that a joint moves: against the base's nothing can be done)
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        t, depth = rng.uniform(0.3, 1.0), rng.uniform(0.002, 0.005 if name == "slider4" else (0.03 if n % 3 == 1 else 0.012))
        obstacles[n] = a + t * (b - a) + d * (r + ORAD - depth)
    return Case(name, N, R, targets, f32(obstacles), q_in.reshape(N * R, model.A))


# ---- the float32 rehearsal ---------------------------------------------------------------------------------------------------------
def walk32(model, q):
    """clear_walk in float32 throughout: (ee, axes[..., A, 3], points[..., A, 3], seg_a, seg_b[..., segments, 3])"""
    f = np.float32
    q = np.asarray(q, f)
    lead = q.shape[:-1]
    R, p = np.broadcast_to(np.eye(3, dtype=f), lead + (3, 3)), np.zeros(lead + (3,), f)
    axes, points, frames = [], [], [(R, p)]
    for m, j in enumerate(model.joints):
        p = p + R @ j.pre_xyz.astype(f)
        R = R @ j.pre_rot.astype(f)
        a = R @ j.axis.astype(f)
        axes.append(a)
        points.append(p)
        if j.type == PRISMATIC:
            p = p + a * q[..., m, None]
        else:
            x, y, z = (f(v) for v in j.axis)
            s, c = np.sin(q[..., m]), np.cos(q[..., m])
            v = f(1.0) - c
            rot = np.stack([np.stack([f(1.0) - v * (y * y + z * z), v * x * y - s * z, v * x * z + s * y], -1),
                            np.stack([v * x * y + s * z, f(1.0) - v * (x * x + z * z), v * y * z - s * x], -1),
                            np.stack([v * x * z - s * y, v * y * z + s * x, f(1.0) - v * (x * x + y * y)], -1)], -2)
            R = R @ rot
        frames.append((R, p))
    Re, pe = frames[model.ee_frame]
    seg_a = [frames[s.frame][1] + frames[s.frame][0] @ s.a.astype(f) for s in model.segments]
    seg_b = [frames[s.frame][1] + frames[s.frame][0] @ s.b.astype(f) for s in model.segments]
    out = (pe + Re @ model.ee_point.astype(f), np.stack(axes, -2), np.stack(points, -2), np.stack(seg_a, -2), np.stack(seg_b, -2))
    assert all(a.dtype == f for a in out)
    return out


def refine32(case):
    """What naf_chain_ik_clear returns with its records on, by the rehearsal: dict of q[N R, A], residual[N R], clear[N R, 4],
    iters[K + 1, N R, A], rec[K, N R, A + 2], all float32"""
    f = np.float32
    model, c = case.model, constants(case.model)
    q0 = case.q_in.astype(f)
    g, ob = case.g.astype(f), case.ob.astype(f)
    A, E = model.A, len(q0)
    q, iters, rec = q0, [q0], []
    tol, goal = f(TOLERANCE), f(GOAL)
    for k in range(K + 1):
        ee, axes, points, seg_a, seg_b = walk32(model, q)
        lt = KM.least_test_of(model, seg_a, seg_b, ob, f(ORAD))
        res = np.sqrt(np.sum((g - ee) * (g - ee), axis=-1))
        assert lt.c.dtype == f and res.dtype == f
        key = np.where(res <= tol, np.minimum(lt.c, goal), f(-np.inf))
        if k == 0:
            early = (lt.c >= goal) | (res > tol)
            best_key, best_q, best_res, c0 = key, q0, res, lt.c
            best_c, best_i, best_kind = lt.c, np.zeros(E, f), lt.kind.astype(f)
        else:
            take = (key > best_key) & ~early
            best_key, best_q, best_res = np.where(take, key, best_key), np.where(take[:, None], q, best_q), np.where(take, res, best_res)
            best_c, best_i, best_kind = np.where(take, lt.c, best_c), np.where(take, f(k), best_i), np.where(take, lt.kind.astype(f), best_kind)
        if k == K:
            break
        gamma = KM.clearance_gradient_of(model, axes, points, lt)
        push_on = np.full(E, k < K - SETTLE)
        q_next, _ = KM.clear_update_of(model, q, g, ee, axes, points, gamma, lt.c, push_on, f(c["lam2"]), f(c["e_max"]), f(c["dq_max"]),
                                       goal, f(PUSH_MAX))
        assert gamma.dtype == f and q_next.dtype == f
        row = np.concatenate([gamma, lt.c[:, None], lt.kind[:, None].astype(f)], axis=1)
        rec.append(np.where(early[:, None], np.concatenate([np.zeros((E, A), f), c0[:, None], best_kind[:, None]], axis=1), row))
        q = np.where(early[:, None], q0, q_next)
        iters.append(q)
    return dict(q=best_q, residual=best_res, clear=np.stack([c0, best_c, best_i, best_kind], axis=1), iters=np.stack(iters),
                rec=np.stack(rec))


# ---- the checks of a refiner's answer, the rehearsal's or the kernel's ---------------------------------------------------------------
def early_of(case, got):
    """The candidates that returned after their first walk: the twin's verdict — c >= clearance_goal or residual > tolerance at the
    input — and the refiner's record must show it: no update moved them and gamma is 0. Inside BAND of the goal or 2 tol of the
    tolerance either verdict is right, and the record says which the refiner took."""
    iters, rec = got["iters"], got["rec"]
    A = case.model.A
    still = np.all(iters == iters[0], axis=(0, 2)) & np.all(rec[:, :, :A] == 0.0, axis=(0, 2))
    lt = KM.least_test(case.twin, case.q_in, case.ob)
    res = np.linalg.norm(case.g - case.twin.end_effector(case.q_in), axis=1)
    want = (lt.c >= GOAL) | (res > TOLERANCE)
    near = (np.abs(lt.c - GOAL) <= BAND) | (np.abs(res - TOLERANCE) <= 2 * C.tol_of(case.model))
    assert np.all(still[want & ~near]), np.nonzero(want & ~near & ~still)[0]
    return np.where(near, still, want)


def check_updates(case, got):
    """Test 1, teacher-forced. Every recorded update of a candidate that did not return early is within STEP_BOUND (max-norm over the
    joints) of ik_clear_step applied to the recorded pose before it, and the recorded gamma and c within GAMMA_BOUND and
    CLEAR_BOUND of the twin's at that pose; the limits hold exactly. Left out: updates where the twin's least and second-least
    tests are closer than BAND — at most CAP of the case's updates. Returns the three largest deviations and the share left out."""
    model, twin = case.model, case.twin
    iters, rec = got["iters"], got["rec"]
    A, E = model.A, case.N * case.R
    assert iters.dtype == np.float32 and iters.shape == (K + 1, E, A) and rec.shape == (K, E, A + 2)
    assert np.array_equal(iters[0], case.q_in.astype(np.float32))
    lo = np.array([j.lower if j.limited else -np.inf for j in model.joints]).astype(np.float32)
    hi = np.array([j.upper if j.limited else np.inf for j in model.joints]).astype(np.float32)
    assert np.all(iters >= lo) and np.all(iters <= hi)
    live = ~early_of(case, got)
    kw = twin_kw(model)
    dev = np.zeros(3)
    left_out = 0
    for k in range(K):
        want, gamma, lt, _ = KM.ik_clear_step(twin, iters[k].astype(np.float64), case.g, case.ob, k, **kw)
        keep = live & (lt.second - lt.c >= BAND)
        left_out += int(np.sum(live & ~keep))
        if not keep.any():
            continue
        d = [np.abs(iters[k + 1].astype(np.float64) - want).max(axis=-1), np.abs(rec[k, :, :A].astype(np.float64) - gamma).max(axis=-1),
             np.abs(rec[k, :, A].astype(np.float64) - lt.c)]
        dev = np.maximum(dev, [x[keep].max() for x in d])
        assert np.array_equal(rec[k, :, A + 1][keep], lt.kind[keep].astype(np.float32)), k
    share = left_out / max(1, K * int(live.sum()))
    assert share <= CAP, (left_out, K * int(live.sum()))
    return dev, share, int(live.sum())


def clearances(case, q):
    twin = case.twin
    zero = np.zeros(len(q))
    return twin.clearance(q, case.ob) - ORAD, twin.self_clearance(q) + zero, twin.cell_clearance(q) + zero


def classes(residual, clear3, margin=MARGIN):
    free = (clear3[0] >= margin) & (clear3[1] >= margin) & (clear3[2] >= margin)
    return np.where(np.asarray(residual) <= np.float32(TOLERANCE), np.where(free, 0, 1), 2)


def check_returned(case, got, class_in=None, class_out=None):
    """Test 2, no exclusions, every candidate. The returned pose's class is <= the input pose's (class_in / class_out: the existing
    probes' and selection's verdicts on the device; the twin's where not given); iterate index 0 means the pose's bits equal the
    input's; residual and clear[1] are within the IK suite's soundness bounds (2 tol; 4 tol where the least test is a self pair)
    of the twin at the returned pose; clear[0] likewise at the input pose; the index is a whole number in 0 .. K."""
    model, twin = case.model, case.twin
    tol = C.tol_of(model)
    q_out, q_in = got["q"], case.q_in.astype(np.float32)
    clear = got["clear"].astype(np.float64)
    index = clear[:, 2]
    assert np.all((index >= 0) & (index <= K) & (index == np.round(index)))
    same = index == 0
    assert np.array_equal(q_out[same].view(np.uint32), q_in[same].view(np.uint32))
    q64 = q_out.astype(np.float64)
    true_res = np.linalg.norm(case.g - twin.end_effector(q64), axis=1)
    assert np.abs(got["residual"] - true_res).max() <= 2 * tol
    for col, q in ((0, case.q_in), (1, q64)):
        lt = KM.least_test(twin, q, case.ob)
        bound = np.where(lt.kind == 1, 4 * tol, 2 * tol)
        assert np.all(np.abs(clear[:, col] - lt.c) <= bound), (col, np.abs(clear[:, col] - lt.c).max(), tol)
    if class_in is None:
        res_in = np.linalg.norm(case.g - twin.end_effector(case.q_in), axis=1)
        class_in, class_out = classes(res_in, clearances(case, case.q_in)), classes(true_res, clearances(case, q64))
    assert np.all(class_out <= class_in), np.nonzero(class_out > class_in)[0]
    # never worse than it came in, on the refiner's own numbers
    assert np.all(np.minimum(clear[:, 1], GOAL) >= np.minimum(clear[:, 0], GOAL))
    return class_in, class_out


def check_completeness(case, got, free_out):
    """Test 3. Every candidate that the free-running twin frees with returned clearance >= margin + BAND, and whose twin trajectory
    kept the least-test gap above BAND at every iterate, is free in `free_out` (the refiner's returned poses by the clearances its
    suite trusts). At most 10 % of the twin-freed candidates are left out. Returns (twin-freed, left out, freed by the refiner)."""
    ref = case.twin_refined()
    res_in = np.linalg.norm(case.g - case.twin.end_effector(case.q_in), axis=1)
    freed = (res_in <= TOLERANCE) & (ref.clear[:, 0] < MARGIN) & (ref.clear[:, 1] >= MARGIN) & (ref.residual <= TOLERANCE)
    gap = np.min(ref.second[:-1] - ref.rec[:, :, -2], axis=0)      # (second-least minus least, at every update's walk)
    sure = freed & (ref.clear[:, 1] >= MARGIN + BAND) & (gap > BAND)
    left_out = int(np.sum(freed & ~sure))
    assert left_out <= 0.1 * max(1, int(freed.sum())), (left_out, int(freed.sum()))
    assert np.all(free_out[sure]), np.nonzero(sure & ~free_out)[0]
    return int(freed.sum()), left_out, int(np.sum(free_out & (ref.clear[:, 0] < MARGIN)))

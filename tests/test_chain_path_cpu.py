"""CPU: the joint-path rule of environment/kinematic.py (path_pose, check_joint_path, path_vias, path_samples, select_joint_path,
JointPaths, joint_paths_host), the rehearsal of every case of tests/test_chain_path_gpu.py with a float32 restatement in the kernel's
place, the plumbing of the entry point and the façade."""
import itertools
import os
import re

import numpy as np
import pytest

import chain_box_common as BX
import chain_cell_common as CC
import chain_ik_common as IK
import chain_path_common as P
import chain_rollout_common as C
from conftest import ROOT
from test_chain_env_cpu import ARMS as ARM_TABLE
from test_chain_env_cpu import model_of, path, random_q

from robotic_manipulator_rloa_amd.environment.kinematic import (PATH_SAMPLES_MAX, JointPaths, KinematicEnvironment, check_joint_path,
                                                                joint_distance32, joint_paths_host, path_chunks, path_pose, path_samples,
                                                                path_vias, select_joint_path)


# ---- the poses ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 128, 2048])
def test_path_pose_end_points_spacing_and_limits(S):
    """Sample 0 is the start, sample S / 2 the via and sample S - 1 the goal, exactly; the via is not a sample of leg 1; each leg's
    samples are evenly spaced (to 4 ulp of the leg); with path_vias' clipped vias every sample lies inside the limits (float32's)."""
    model, twin = IK.arm("iiwa_like7")
    rng = np.random.default_rng(S)
    a, b = np.stack([random_q(model, rng) for _ in range(6)]), np.stack([random_q(model, rng) for _ in range(6)])
    vias = path_vias(model, a, b, 8, seed=2).astype(np.float64)
    a, b = C.f32(a)[:, None, :], C.f32(b)[:, None, :]
    h = S // 2
    q = path_pose(a[:, :, None, :], vias[:, :, None, :], b[:, :, None, :], np.arange(S), S)
    assert q.shape == (6, 8, S, 7)
    assert np.array_equal(q[:, :, 0], np.broadcast_to(a, vias.shape)) and np.array_equal(q[:, :, h], vias)
    assert np.array_equal(q[:, :, S - 1], np.broadcast_to(b, vias.shape))
    assert np.array_equal(path_pose(a[0, 0], vias[0, 3], b[0, 0], h, S), vias[0, 3])
    moving = np.abs(vias - a).max(axis=-1) > 0
    assert np.all(np.abs(q[:, :, h - 1] - vias).max(axis=-1)[moving] > 0)
    for leg, n in ((q[:, :, :h + 1], h), (q[:, :, h:], h - 1)):
        step = np.diff(leg, axis=2)
        want = (leg[:, :, -1] - leg[:, :, 0])[:, :, None, :] / n
        assert np.abs(step - want).max() <= 4 * 2.0 ** -52 * 2 * np.pi
    lo, hi = (C.f32(v) for v in twin.joint_limits())                       # the limits as the device holds them
    assert np.all(q >= lo) and np.all(q <= hi)


# ---- the record against brute force ------------------------------------------------------------------------------------------------
def brute_record(twin, a, via, b, ob, S, margin):
    h, clears, first, count, last = S // 2, [], -1, 0, 0
    for i in range(S):
        lo, hi, f = (a, via, i / h) if i < h else (via, b, (i - h) / (h - 1))
        q = hi if f == 1.0 else lo + f * (hi - lo)
        c = (float(twin.clearance(q, ob)) - twin.obstacle_radius, float(twin.self_clearance(q)), float(twin.cell_clearance(q)))
        clears.append(c)
        if min(c) < margin:
            first, count = (i if first < 0 else first), count + 1
            last = 1 if i == S - 1 else last
    m = np.min(clears, axis=0)
    l1, l2 = np.float32(np.abs(np.float32(via) - np.float32(a)).max()), np.float32(np.abs(np.float32(b) - np.float32(via)).max())
    return [m[0], m[1], m[2], first, count, float(l1 + l2), float(max(l1 / np.float32(h), l2 / np.float32(h - 1))), last]


BRUTE = [("planar3", lambda: CC.arm("planar3")), ("iiwa_cell", lambda: CC.arm("iiwa_like7")), ("iiwa_box", lambda: BX.arm("iiwa_like7")),
         ("long12", lambda: IK.arm("long12")), ("slider4", IK.slider)]


@pytest.mark.parametrize("name,make", BRUTE, ids=[n for n, _ in BRUTE])
def test_check_joint_path_against_brute_force(name, make):
    """check_joint_path's eight numbers equal a loop over the samples that asks twin.clearance / self_clearance / cell_clearance one
    pose at a time: the minima to 1e-12 (a batch's sums round as a single pose's do, up to the order numpy takes them in), the
    index, the count and the flag exactly, length and step as float32 forms them. On the walls, the floor and sphere with
    self-collision, the boxes, twelve joints with pairs, and prismatic joints; some candidates free, some blocked."""
    model, twin = make()
    rng = np.random.default_rng(17)
    q = C.f32(np.stack([random_q(model, rng) for _ in range(6)]))
    a, b = q[:3], q[3:]
    vias = path_vias(model, a, b, 3, seed=4).astype(np.float64)
    ob = C.f32(np.stack([twin.end_effector(0.5 * (a[0] + b[0])), C.away(model)[1], C.away(model)[1]]))
    margin = 0.004
    got = check_joint_path(twin, a[:, None, :], vias, b[:, None, :], ob[:, None, :], 64, margin)
    assert got.shape == (3, 3, 8)
    for n in range(3):
        for c in range(3):
            want = brute_record(twin, a[n], vias[n, c], b[n], ob[n], 64, margin)
            inf = np.isposinf(want[:3])
            assert np.array_equal(np.isposinf(got[n, c, :3]), inf)
            assert np.abs(got[n, c, :3][~inf] - np.array(want[:3])[~inf]).max() <= 1e-12
            assert list(got[n, c, 3:]) == want[3:], (n, c)
    assert np.any(got[..., 4] > 0)
    one = check_joint_path(twin, a[0], vias[0, 1], b[0], ob[0], 64, margin)
    assert one.shape == (8,) and np.array_equal(one, got[0, 1])
    for S in (0, 63, 96, 2112, 64.0):
        with pytest.raises(ValueError, match="multiple of 64"):
            check_joint_path(twin, a[0], vias[0, 1], b[0], ob[0], S)


# ---- cases with a known answer ----------------------------------------------------------------------------------------------------------
def test_an_empty_scene_is_straight():
    """No pairs, no workcell, the obstacle away: every query is 'straight', its length the straight length, which is GoalPoses'
    joint_distance of the same poses bit for bit, and nothing is blocked."""
    model = model_of("iiwa_like7")
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), C.ORAD)
    rng = np.random.default_rng(3)
    a, b = (np.stack([random_q(model, rng) for _ in range(12)]) for _ in range(2))
    out = joint_paths_host(twin, a, b, np.tile(C.away(model)[1], (12, 1)), candidates=4, resolution=0.05)
    assert isinstance(out, JointPaths) and np.all(out.outcome == "straight") and np.all(out.candidate == 0)
    jd = joint_distance32(C.f32(b), C.f32(a))
    assert np.array_equal(out.length, out.straight_length) and np.array_equal(out.straight_length, jd.astype(np.float64))
    assert np.all(out.straight_first_blocked == -1) and np.all(np.isposinf(out.min_self_clearance))
    assert np.all(out.sample_step <= 0.05) and np.all(out.samples % 64 == 0)
    w = out.waypoints(9)
    assert w.shape == (12, 9, 7) and np.array_equal(w[:, 0], C.f32(a)) and np.array_equal(w[:, -1], C.f32(b))
    assert np.abs(w[:, 4] - 0.5 * (C.f32(a) + C.f32(b))).max() <= 1e-6


def test_planar3_around_an_obstacle_on_the_straight_line():
    """planar3 sweeps its first joint by 2 rad with the others held: the obstacle sits where the tip passes at 40 % of the sweep, so
    the straight candidate is blocked at a sample index inside the interval the geometry gives — the tip's capsule (radius 0.03)
    and the obstacle (0.06) overlap while the tip is within 0.09 of the centre, an arc of at most asin(0.09 / r) either side — and
    at least one via candidate is free; the chosen path is that one's."""
    model = model_of("planar3")
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), C.ORAD)
    a, b = C.f32(np.array([-1.0, 0.3, 0.3])), C.f32(np.array([1.0, 0.3, 0.3]))
    ob = C.f32(twin.end_effector(a + 0.4 * (b - a)))
    r = float(np.linalg.norm(ob[:2]))
    half = np.arcsin(min(1.0, (0.03 + C.ORAD) / r)) / 2.0                     # as a fraction of the 2 rad sweep
    out = joint_paths_host(twin, a[None], b[None], ob[None], candidates=32, resolution=0.01, seed=1)
    S = int(out.samples[0])
    first = int(out.straight_first_blocked[0])
    # the links behind the tip pass the obstacle later than the tip does, never earlier than its first touch
    assert (0.4 - half) * S - 2 <= first <= 0.4 * S, (first, S, half)
    assert out.outcome[0] == "via" and out.candidate[0] >= 1 and out.length[0] > out.straight_length[0]
    assert out.min_clearance[0] >= 0.0 and not np.any(np.isnan(out.via[0]))
    rec = check_joint_path(twin, a, out.via[0], b, ob, S)
    assert rec[4] == 0 and rec[0] == out.min_clearance[0]
    w = out.waypoints(50)
    assert np.all(twin.clearance(w[0], ob) - C.ORAD >= -0.01)


def test_start_and_goal_poses_in_contact():
    """A start pose in contact gives 'start', a goal pose in contact 'goal', both 'start'; their numbers are the straight line's
    and there is no path: candidate -1, NaN length, via and waypoints."""
    model = model_of("planar3")
    twin = KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), C.ORAD)
    free, other = C.f32(np.array([0.2, 0.4, -0.3])), C.f32(np.array([1.5, -0.4, 0.5]))
    ob_free, ob_other = C.f32(twin.end_effector(free)), C.f32(twin.end_effector(other))
    a = np.stack([free, other, free])
    b = np.stack([other, free, other])
    ob = np.stack([ob_free, ob_free, C.f32(0.5 * (ob_free + ob_other))])
    out = joint_paths_host(twin, a, b, ob, candidates=4, resolution=0.05)
    assert list(out.outcome[:2]) == ["start", "goal"] and out.outcome[2] in ("straight", "via", "blocked")
    assert np.all(out.candidate[:2] == -1) and np.all(np.isnan(out.length[:2])) and np.all(np.isnan(out.via[:2]))
    assert out.straight_first_blocked[0] == 0 and out.straight_first_blocked[1] > 0 and np.all(out.min_clearance[:2] < 0.0)
    assert np.all(np.isnan(out.waypoints(4)[:2]))
    both = joint_paths_host(twin, free[None], free[None], ob_free[None], candidates=2)
    assert both.outcome[0] == "start"


# ---- vias, samples, selection ---------------------------------------------------------------------------------------------------------
def test_path_vias():
    """Deterministic per seed; candidate 0 is the midpoint; every via lies inside the limits as float32 holds them; an unlimited joint
    is not clipped (its vias reach beyond +-pi); the widths cycle 0.5, 1, 2 x max(D, 0.5)."""
    model, _ = IK.arm("iiwa_like7")
    rng = np.random.default_rng(6)
    a, b = (C.f32(np.stack([random_q(model, rng) for _ in range(40)])) for _ in range(2))
    v = path_vias(model, a, b, 16, seed=9)
    assert v.shape == (40, 16, 7) and v.dtype == np.float32
    assert np.array_equal(v, path_vias(model, a, b, 16, seed=9)) and not np.array_equal(v, path_vias(model, a, b, 16, seed=10))
    assert np.array_equal(v[:, 0], (0.5 * (a + b)).astype(np.float32))
    assert np.array_equal(path_vias(model, a, b, 1, seed=9)[:, 0], v[:, 0])
    lo = np.array([j.lower for j in model.joints]).astype(np.float32)
    hi = np.array([j.upper for j in model.joints]).astype(np.float32)
    assert all(j.limited for j in model.joints) and np.all(v >= lo) and np.all(v <= hi)
    assert np.any(v == lo) and np.any(v == hi)
    free_model = model_of("planar3")                                          # continuous joints
    spin = [m for m, j in enumerate(free_model.joints) if not j.limited]
    a3, b3 = np.full((200, 3), 3.0), np.full((200, 3), 3.1)
    v3 = path_vias(free_model, a3, b3, 4, seed=0)
    if spin:
        assert np.abs(v3[:, 3, spin]).max() > np.pi
    u = np.random.default_rng(0).random((200, 3, 3))
    want = 3.05 + (2.0 * u - 1.0) * (0.5 * 2.0 ** np.arange(3))[None, :, None] * 0.5
    unclipped = np.array([not j.limited for j in free_model.joints])
    assert np.array_equal(v3[:, 1:][:, :, unclipped], want.astype(np.float32)[:, :, unclipped])


def test_path_samples_and_chunks_at_the_boundaries():
    assert path_samples([0.0], 0.02) == 64 and path_samples([], 0.02) == 64
    assert path_samples([31 * 0.02], 0.02) == 64 and path_samples([31 * 0.02 + 1e-9], 0.02) == 128
    assert path_samples([0.1, 63 * 0.02, 0.3], 0.02) == 128 and path_samples([63 * 0.02 + 1e-9], 0.02) == 192
    assert path_samples([1023 * 0.02 - 1e-9], 0.02) == PATH_SAMPLES_MAX == 2048 and path_samples([991 * 0.02], 0.02) == 1984
    assert path_samples([1e9], 0.02) == 2048
    for S in range(64, 2049, 64):
        L = 0.02 * (S // 2 - 1)
        assert path_samples([L * (1 - 1e-12)], 0.02) == S
    legs = np.zeros((5, 3, 2))
    legs[:, 0, 0] = [0.1, 0.1, 2.0, 0.1, 0.1]
    assert path_chunks(legs, 3, 0.02) == [(0, 5, 256)]
    assert path_chunks(legs, 3, 0.02, budget=2 * 3 * 64) == [(0, 2, 64), (2, 1, 256), (3, 2, 64)]
    assert path_chunks(legs, 3, 0.02, budget=64) == [(k, 1, 256 if k == 2 else 64) for k in range(5)]


def brute_select(rec):
    out = []
    for r in rec:
        if r[0][3] == 0:
            out.append(("start", -1))
        elif r[0][7] == 1:
            out.append(("goal", -1))
        else:
            free = [c for c in range(len(r)) if r[c][4] == 0]
            if not free:
                out.append(("blocked", -1))
            elif 0 in free:
                out.append(("straight", 0))
            else:
                best = min(free, key=lambda c: (r[c][5], c))
                out.append(("via", best))
    return out


def test_selection_against_brute_force_over_all_orderings_and_ties():
    """Every assignment of {free, blocked} x three lengths (two of them equal) to C = 3 candidates, with and without a blocked
    start and goal: the outcome and the candidate equal a loop's. A free candidate 0 wins whatever the float32 lengths say —
    no polyline is shorter than the straight line, and a via's L1 + L2 may round an ulp below it."""
    rows = []
    for blocked in itertools.product((0, 3), repeat=3):
        for lengths in itertools.product((1.0, 1.5, 1.5000001), repeat=3):
            for first0, goal in ((-1, 0), (0, 0), (5, 1), (0, 1)):
                rec = np.zeros((3, 8), np.float32)
                rec[:, 4], rec[:, 5] = blocked, lengths
                rec[:, 3] = np.where(np.array(blocked) > 0, 7, -1)
                if first0 >= 0:
                    rec[0, 3], rec[0, 4] = first0, max(rec[0, 4], 1)
                if goal:
                    rec[:, 7], rec[:, 4] = 1, np.maximum(rec[:, 4], 1)
                    rec[:, 3] = np.where(rec[:, 3] < 0, 127, rec[:, 3])
                rows.append(rec)
    rec = np.stack(rows)
    outcome, cand = select_joint_path(rec)
    want = brute_select(rec)
    assert [(o, int(c)) for o, c in zip(outcome, cand)] == want
    assert {o for o, _ in want} == {"start", "goal", "straight", "via", "blocked"}
    o64, c64 = select_joint_path(rec.astype(np.float64))
    assert np.array_equal(o64, outcome) and np.array_equal(c64, cand)
    shorter = np.zeros((1, 2, 8), np.float32)
    shorter[0, :, 3] = -1
    shorter[0, :, 5] = [1.0, np.nextafter(np.float32(1.0), np.float32(0.0))]
    assert select_joint_path(shorter)[0][0] == "straight"


# ---- the rehearsal ------------------------------------------------------------------------------------------------------------------------
REHEARSED = [(name, N, Cn, S) for name in P.ARMS for N, Cn, S in P.COUNTS] + P.EXTRA
MEASURED = {}


@pytest.mark.parametrize("name,N,Cn,S", REHEARSED)
def test_rehearsal(name, N, Cn, S):
    """Every GPU case with the float32 restatement in the kernel's place: the case builds (the twin alone meets the 1 % cap and the
    floors, reseeded until it does), and the restatement's records and poses pass every check the kernel's will; the pose
    deviation is measured."""
    case = P.build_case(name, N, Cn, S)
    out, poses = P.record32(case)
    dev, census = P.check_records(case, out, poses)
    MEASURED[(name, N, Cn, S)] = dev
    lo = np.array([j.lower if j.limited else -np.inf for j in case.model.joints]).astype(np.float32)
    hi = np.array([j.upper if j.limited else np.inf for j in case.model.joints]).astype(np.float32)
    assert np.all(poses >= lo) and np.all(poses <= hi)                         # reset_given will not move a recorded pose


def test_the_measured_deviation_is_the_constant():
    """POSE_DEVIATION is the rehearsal's largest measured deviation rounded up (by no more than a quarter), and the bound 8 x it"""
    if len(MEASURED) < len(REHEARSED):
        for args in REHEARSED:
            case = P.build_case(*args)
            MEASURED[args] = P.check_records(case, *P.record32(case))[0]
    worst = max(MEASURED.values())
    print({k: f"{v:.2e}" for k, v in MEASURED.items()})
    assert worst <= P.POSE_DEVIATION <= 1.25 * worst, (worst, P.POSE_DEVIATION)
    assert P.POSE_BOUND == 8 * P.POSE_DEVIATION


# ---- plumbing --------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_abi_and_argument_errors():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40 and re.search(r"^#define NAF_CHAIN_PATH_FLOATS 8$", text, re.M)
    name = "naf_chain_path_check"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 13
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40
    # argument errors are host code and launch nothing: a fake non-null handle is never dereferenced before they answer
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    call = lambda h=p, a=p, b=p, v=p, o=p, rad=0.06, N=1, Cn=1, S=64, margin=0.0, out=p: lib.naf_chain_path_check(   # noqa: E731
        h, a, b, v, o, rad, N, Cn, S, margin, out, None, None)
    for kw in (dict(h=None), dict(a=None), dict(b=None), dict(v=None), dict(o=None), dict(out=None), dict(N=0), dict(N=-2), dict(Cn=0),
               dict(Cn=65), dict(S=0), dict(S=32), dict(S=96), dict(S=2112), dict(S=-64), dict(margin=float("nan")),
               dict(margin=float("inf")), dict(rad=float("nan")), dict(rad=float("inf")), dict(rad=-0.01), dict(N=1 << 29, Cn=4)):
        assert call(**kw) == -1, kw


# ---- through the façade -------------------------------------------------------------------------------------------------------------------
def framework(**kw):
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    ee, involved, fixed, init, var = ARM_TABLE["iiwa_like7"]
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(path("iiwa_like7"), ee, fixed, involved, [0.45, 0.3, 0.6], [0.35, 0.2, 0.45], init, var,
                                       link_radius=0.03, obstacle_radius=0.07, consider_autocollision=True, **kw)
    return f


def test_plan_joint_paths_on_the_host_and_its_refusals(caplog):
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized,
                                                               InvalidEnvironmentParameter)
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.plan_joint_paths([0.4, 0.2, 0.5])
    f.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="PyBullet and the synthetic stand-in have no chain model to solve on"):
        f.plan_joint_paths([0.4, 0.2, 0.5])
    f = framework(workcell_boxes=BX.boxes_of("iiwa_like7"))
    twin = f.env
    rng = np.random.default_rng(2)
    goals = IK.free_poses(twin.model, twin, rng, 6)
    start = np.tile(twin.initial_joint_positions, (6, 1))
    kw = dict(candidates=4, resolution=0.05, seed=5, on_device=False)
    out = f.plan_joint_paths(goal_joint_positions=goals, **kw)                      # needs no agent
    want = joint_paths_host(twin, start, goals, np.tile(twin.obstacle_pos, (6, 1)), candidates=4, resolution=0.05, seed=5)
    assert isinstance(out, JointPaths) and out.outcome.shape == (6,) and out.via.shape == (6, 7)
    for name, a, b in zip(out._fields, out, want):
        assert np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b), name
    one = f.plan_joint_paths(goal_joint_positions=goals[0], **kw)
    assert one.outcome.shape == (1,) and one.outcome[0] == out.outcome[0]
    # by targets: the goal poses are solve_goal_poses' with the same seed; an unreachable target ends 'goal' with NaN numbers
    targets = np.concatenate([twin.end_effector(goals[:3]), [[0.0, 0.0, 1.1 * twin.model.reach]]])
    by_target = f.plan_joint_paths(targets, **kw)
    goal = f.solve_goal_poses(targets, seed=5, on_device=False)
    assert list(goal.reachable) == [True, True, True, False]
    direct = joint_paths_host(twin, start[:3], goal.joint_positions[:3], np.tile(twin.obstacle_pos, (3, 1)), candidates=4,
                              resolution=0.05, seed=5)
    for name, a, b in zip(out._fields, by_target, direct):
        assert np.array_equal(a[:3], b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a[:3], b), name
    assert by_target.outcome[3] == "goal" and by_target.candidate[3] == -1 and by_target.samples[3] == 0
    assert np.isnan(by_target.length[3]) and np.isnan(by_target.min_clearance[3]) and np.all(np.isnan(by_target.via[3]))
    # a margin no pose keeps blocks the start pose of every query
    assert np.all(f.plan_joint_paths(goal_joint_positions=goals, clearance_margin=5.0, **kw).outcome == "start")
    # the 2048-sample cap: one warning, with the step it got
    caplog.clear()
    with caplog.at_level("WARNING"):
        coarse = f.plan_joint_paths(goal_joint_positions=goals, candidates=2, resolution=1e-4, on_device=False)
        f.plan_joint_paths(goal_joint_positions=goals[:1], candidates=2, resolution=1e-4, on_device=False)
    said = [r for r in caplog.records if "2048" in r.getMessage()]
    assert np.all(coarse.samples == 2048) and np.all(coarse.sample_step > 1e-4)
    if caplog.records:                                     # (the project's logger may not propagate to caplog's handler)
        assert len(said) == 1 and f"{float(coarse.sample_step.max()):.4g}" in said[0].getMessage()
    for args, match in ((dict(), "exactly one"), (dict(targets=np.zeros((2, 3)), goal_joint_positions=goals[:2]), "exactly one"),
                        (dict(targets=np.zeros((4, 2))), "targets"), (dict(targets=[0.0, np.nan, 0.0]), "not finite"),
                        (dict(targets=np.zeros((4, 3)), obstacles=np.zeros((2, 3))), "obstacles"),
                        (dict(goal_joint_positions=goals, obstacles=np.zeros((2, 3))), "obstacles"),
                        (dict(goal_joint_positions=goals, initial_joint_positions=np.zeros(6)), "initial_joint"),
                        (dict(goal_joint_positions=goals, initial_joint_positions=np.full(7, 9.0)),
                         r"initial_joint_positions of query 0: joint 0 \(involved_joints\[0\]\)"),
                        (dict(goal_joint_positions=np.zeros((3, 6))), r"goal_joint_positions is \[N\]\[7\]"),
                        (dict(goal_joint_positions=np.full((3, 7), np.nan)), "not finite"),
                        (dict(goal_joint_positions=np.concatenate([goals[:2], np.full((1, 7), 9.0)])),
                         r"goal_joint_positions of query 2: joint 0 \(involved_joints\[0\]\)"),
                        (dict(goal_joint_positions=goals, candidates=0), "candidates"),
                        (dict(goal_joint_positions=goals, candidates=65), "candidates"),
                        (dict(goal_joint_positions=goals, candidates=4.0), "candidates"),
                        (dict(goal_joint_positions=goals, resolution=0.0), "resolution"),
                        (dict(goal_joint_positions=goals, resolution=float("nan")), "resolution"),
                        (dict(goal_joint_positions=goals, clearance_margin=float("inf")), "clearance_margin"),
                        (dict(goal_joint_positions=goals, seed=-1), "seed"), (dict(goal_joint_positions=goals, seed=1.5), "seed")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.plan_joint_paths(on_device=False, **args)


def test_reach_targets_with_joint_paths_against_a_stub_agent(monkeypatch):
    import torch
    from robotic_manipulator_rloa_amd.engine import ReachResult
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # goal poses and paths come from the twin
    f = framework()
    twin = f.env
    rng = np.random.default_rng(4)
    N, F = 6, 5
    goals = IK.free_poses(twin.model, twin, rng, N)
    targets = twin.end_effector(goals)
    start = np.tile(twin.initial_joint_positions, (N, 1))

    class Agent:                      # returns a straight joint path to the goal pose in F frames for every query but one
        state_size, action_size, seed, world_size = 23, 7, 0, 1
        calls = []

        def rollout_vectorized(self, chain, targets, obstacles, q0, **kw):
            self.calls.append(kw)
            z = np.zeros(N, np.float32)
            s = np.linspace(0.0, 1.0, F + 1)[None, :, None]
            paths = (q0[:, None, :] + s * (goals - q0)[:, None, :]).astype(np.float32)
            outcome = np.array(["reached"] * N)
            outcome[1] = "frames"
            return ReachResult(outcome, np.full(N, F), z, z, z, z, paths, z, z, z, z, z)

    f.naf_agent = Agent()
    plain = f.reach_targets(targets, initial_joint_positions=start, frames=F)
    assert plain.goal is None and plain.path is None and plain.planned_ratio is None
    with_goal = f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True)
    assert with_goal.goal is not None and with_goal.path is None and with_goal.planned_ratio is None
    out = f.reach_targets(targets, initial_joint_positions=start, frames=F, joint_paths=True)
    assert Agent.calls[-1] == Agent.calls[0]                                 # the rollout is called as it was
    for a, b in zip(out.goal, with_goal.goal):                               # joint_paths implies goal_poses
        assert np.array_equal(a, b)
    assert np.array_equal(out.path_ratio, with_goal.path_ratio, equal_nan=True)
    want = f.plan_joint_paths(targets, initial_joint_positions=start)
    for name, a, b in zip(want._fields, out.path, want):
        assert np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b), name
    length = np.abs(goals - start).max(axis=1)
    ok = out.path.candidate >= 0
    ok[1] = False
    assert np.all(np.isnan(out.planned_ratio[~ok])) and ok.sum() >= 2
    assert np.abs(out.planned_ratio[ok] - length[ok] / out.path.length[ok]).max() <= 1e-5
    for field in ("outcome", "frames", "joint_positions", "score"):
        assert np.array_equal(getattr(out, field), getattr(plain, field))

"""CPU (`-m "not gpu"`): the rule of time-parameterised trajectories in environment/trajectory.py (blend_schedule, trajectory_law,
check_trajectory, plan_trajectories) against properties and closed forms of its own; the rehearsal of every GPU case of
tests/test_chain_traj_gpu.py with a float32 restatement in the kernel's place, which measures the pose bound the GPU tests use; the
façade's arguments and refusals; and the plumbing of naf_chain_traj_check / naf_chain_traj_certify."""
import os
import re

import numpy as np
import pytest

import chain_ik_common as IK
import chain_roadmap_common as R
import chain_traj_common as X
from test_chain_ik_cpu import framework

from robotic_manipulator_rloa_amd.environment import trajectory as T
from robotic_manipulator_rloa_amd.environment.edge_certificate import certify_polylines_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAF_ERR_ARG = -1
_REHEARSED = {}

# what both entry points refuse with NAF_ERR_ARG (stated against a launch of N = 1, V = 2, S = 64; the GPU suite runs them on a handle)
nan, inf = float("nan"), float("inf")
ARGUMENT_ERRORS = ([{k: None} for k in ("h", "nodes", "n_nodes", "times", "vpeak", "n_samples", "o", "out")] +
                   [dict(N=0), dict(N=-2), dict(V=1), dict(V=65), dict(S=0), dict(S=63), dict(S=96), dict(S=8256), dict(S=16384),
                    dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf), dict(margin=nan), dict(margin=inf), dict(rad=nan),
                    dict(rad=-0.01), dict(rad=inf)])
CERTIFY_ERRORS = [dict(reach=None), dict(guard=-1e-6), dict(guard=nan), dict(guard=inf)]


def rehearse(case_id):
    """one case with the restatement in the kernel's place: computed once, shared by the tests below"""
    if case_id not in _REHEARSED:
        case = X.build(*case_id)
        out, poses = X.record32(case)
        _REHEARSED[case_id] = (case, out, poses, X.check_poses(case, poses), X.check_records(case, out, poses))
    return _REHEARSED[case_id]


@pytest.mark.parametrize("name,N,L,S", X.CASES)
def test_rehearsal(name, N, L, S):
    """Every case of the GPU suite with the float32 restatement (chain_traj_common.law32, record32) in the kernel's place: the same
    checks, so the pose bound, the band shares and the populated verdicts hold before a GPU is involved; a case of 64 is built with
    the seed the table names. Every case holds a trajectory with S_n = S, one with S_n = S - 63 (2 at S = 64) and one of one sample."""
    case, out, poses, dev, census = rehearse((name, N, L, S))
    if N >= 64:
        assert case.seed == X.SEED[(name, N, L, S)], case.seed
    ns = case.ds.n_samples
    assert ns[0] == S and ns[1] == (S - 63 if S > 64 else 2) and ns[2] == 1 and case.ds.n_nodes[2] == 1
    assert case.ds.n_nodes[0] == L + 1 and case.V == max(L + 1, 2)
    plain, _ = X.record32(case, certify=False)
    assert np.array_equal(plain.view(np.uint32), out[:, :8].view(np.uint32))
    X.check_records(case, plain, poses, certify=False)


def test_the_measured_deviation_is_the_constant():
    """POSE_DEVIATION is the largest deviation the rehearsal measures over all its cases, rounded up by at most a quarter; the GPU
    bound is 4 x it."""
    dev = max(rehearse(c)[3] for c in X.CASES)
    print(f"largest deviation of the restatement from the float64 law {dev:.3e}; POSE_DEVIATION {X.POSE_DEVIATION:.3e}")
    assert 0.75 * X.POSE_DEVIATION <= dev <= X.POSE_DEVIATION and X.POSE_BOUND == 4 * X.POSE_DEVIATION


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def _random_polyline(rng, short=False):
    A, L = int(rng.integers(1, 8)), int(rng.integers(1, 8))
    P = rng.uniform(-2.0, 2.0, (L + 1, A))
    if short:
        P[1:] = P[:-1] + rng.uniform(-0.01, 0.01, (L, A))
    return P, rng.uniform(0.5, 2.0, A), rng.uniform(1.0, 10.0, A)


def test_limits_blends_ends_and_derivative_on_random_polylines():
    """300 random polylines on 1 .. 7 joints with 1 .. 7 legs, every fifth with very short legs: on a grid of 4000 intervals both
    limits hold (the acceleration as the difference quotient of the velocity), the blends do not overlap, q(0) = P_0 and
    q(D) = q(D + 1) = P_K exactly, the velocity is continuous (its jumps between grid points stay within amax h) and equals the
    central difference of q to amax h; the trajectory starts and ends at rest."""
    rng = np.random.default_rng(0)
    ratios = []
    for it in range(300):
        P, vmax, amax = _random_polyline(rng, it % 5 == 0)
        s = T.blend_schedule(P, vmax, amax)
        D, tau, Tl = s["duration"], s["blend_times"], s["leg_times"]
        assert np.all((tau[:-1] + tau[1:]) / 2 <= Tl * (1 + 1e-12)) and np.all(Tl > 0)
        assert np.isclose(D, 0.5 * tau[0] + Tl.sum() + 0.5 * tau[-1], rtol=1e-14)
        t = np.linspace(0.0, D, 4001)
        h = D / 4000
        q, qd = T.law_of(s, t), T.law_of(s, t, derivative=True)
        end = T.law_of(s, [0.0, D, D + 1.0])
        assert np.array_equal(end[0], P[0]) and np.array_equal(end[1], P[-1]) and np.array_equal(end[2], P[-1])
        assert not qd[0].any() and np.abs(qd[-1]).max() <= 1e-9
        assert np.all(np.abs(qd) <= vmax * (1 + 1e-9))
        assert np.all(np.abs(np.diff(qd, axis=0)) <= amax * h * (1 + 1e-6))            # continuous, and within the acceleration limit
        central = (q[2:] - q[:-2]) / (2 * h)
        assert np.all(np.abs(central - qd[1:-1]) <= amax * h)
        ratios.append(D / T.rest_to_rest_duration(P, vmax, amax))
    print(f"duration over rest-to-rest: median {np.median(ratios):.3f}, worst {max(ratios):.3f}, best {min(ratios):.3f}")
    assert np.median(ratios) < 1.0 < max(ratios) < 1.5                                 # usually, not always, the faster one


def test_special_polylines():
    """A collinear polyline with equal leg velocities has tau = 0 at its interior nodes and stays on its line; K = 1 is a trapezoid or
    a triangle with the closed-form duration; duplicate nodes are merged; one node is D = 0 and S = 1; and a polyline on which the
    uniform scaling fires still keeps limits and blends."""
    d = np.array([0.3, -0.2, 0.1])
    P = np.array([0.1, 0.2, 0.3]) + np.arange(5)[:, None] * d
    s = T.blend_schedule(P, np.full(3, 1.0), np.full(3, 4.0))
    assert np.all(s["blend_times"][1:-1] <= 1e-15) and s["blend_times"][0] > 0 and s["rounds"] == 0 and s["scaled"] == 1.0
    q = T.law_of(s, np.linspace(0, s["duration"], 500)) - P[0]
    along = q @ d / (d @ d)
    assert np.abs(q - along[:, None] * d).max() <= 1e-14 and np.all(np.diff(along) >= -1e-15) and np.isclose(along[-1], 4.0)
    for dist, v, a, closed in ((2.0, 1.0, 4.0, 2.0 / 1.0 + 1.0 / 4.0), (0.1, 1.0, 4.0, 2.0 * np.sqrt(0.1 / 4.0))):
        s = T.blend_schedule(np.array([[0.0], [dist]]), [v], [a])
        assert np.isclose(s["duration"], closed, rtol=1e-5) and np.isclose(T.rest_to_rest_duration([[0.0], [dist]], [v], [a]), closed)
        peak = np.abs(T.law_of(s, np.linspace(0, s["duration"], 2001), derivative=True)).max()
        assert np.isclose(peak, min(v, np.sqrt(dist * a)), rtol=1e-3)
    dup = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 0.5], [1.0, 0.5], [1.0, 0.5], [0.0, 1.0]])
    merged = T.blend_schedule(dup, [1.0, 1.0], [3.0, 3.0])
    assert np.array_equal(merged["nodes"], dup[[0, 2, 5]])
    assert merged["duration"] == T.blend_schedule(dup[[0, 2, 5]], [1.0, 1.0], [3.0, 3.0])["duration"]
    one = T.blend_schedule(np.ones((4, 3)), np.ones(3), np.ones(3))
    assert one["duration"] == 0.0 and len(one["nodes"]) == 1
    ds = T.device_schedule([one], X.DT)
    assert ds.n_samples.tolist() == [1] and ds.n_nodes.tolist() == [1] and ds.nodes.shape == (1, 2, 3)
    assert np.array_equal(T.trajectory_poses(ds, 64), np.ones((1, 64, 3)))
    rng = np.random.default_rng(3)
    fired = 0
    for _ in range(400):
        P = np.cumsum(rng.uniform(-1, 1, (8, 2)) * rng.choice([1e-3, 1.0], (8, 1)), axis=0)
        s = T.blend_schedule(P, [1.0, 1.0], [2.0, 2.0])
        if s["scaled"] > 1.0:
            fired += 1
            tau, Tl = s["blend_times"], s["leg_times"]
            assert np.all((tau[:-1] + tau[1:]) / 2 <= Tl) and s["rounds"] == T.TRAJ_ROUNDS
            qd = T.law_of(s, np.linspace(0, s["duration"], 3001), derivative=True)
            assert np.all(np.abs(qd) <= 1.0 + 1e-9) and np.all(np.abs(np.diff(qd, axis=0)) <= 2.0 * s["duration"] / 3000 * (1 + 1e-6))
    print(f"the uniform scaling fired on {fired} of 400 polylines with legs of mixed lengths")
    assert fired >= 1


def _paths(nodes):
    """hand-made polylines as plan_trajectories reads them: (nodes[N][Kmax][A] NaN-padded, n_nodes[N])"""
    Kmax = max(len(p) for p in nodes)
    out = np.full((len(nodes), max(Kmax, 2), len(nodes[0][0])), np.nan)
    for n, p in enumerate(nodes):
        if len(p):
            out[n, :len(p)] = p
    return out, np.array([len(p) for p in nodes])


def test_plan_trajectories_on_the_twin():
    """The control flow with the twin as its backend, on planar3: corner_deviation is the measured distance from q(t_k) to P_k; a
    query without a path is 'none' and never reaches the backend; positions are NaN behind each query's own end and are the law at
    the ticks; at() and velocities() are the float64 law; every tick is a legal action under the default limits; chunking does not
    change a result."""
    model, twin = R.arm("planar3")
    rng = np.random.default_rng(5)
    q = IK.free_poses(model, twin, rng, 9)
    nodes, count = _paths([q[0:3], [], q[3:5], q[5:9], q[8:9]])
    ob = np.tile(X.C.away(model)[1], (5, 1))
    vmax, amax = np.full(3, 1.0), np.full(3, 5.0)
    tr = T.plan_trajectories(T._TwinTrajectories(twin), nodes, count, ob, vmax, amax, X.DT, certify=True)
    assert isinstance(tr, T.Trajectories) and tr.outcome[1] == "none" and tr.n_samples.tolist()[1] == 0 and np.isnan(tr.duration[1])
    assert tr.outcome[4] in ("certified", "sampled") and tr.duration[4] == 0.0 and tr.n_samples[4] == 1
    assert set(tr.outcome) <= set(T.TRAJECTORY_OUTCOMES) and np.array_equal(tr.certified, tr.outcome == "certified")
    has = tr.outcome != "none"
    # S_n = ceil(D / dt) + 1, of the float32 schedule's D and dt: within one of the float64 schedule's
    assert np.all(np.abs(tr.n_samples[has] - (np.ceil(tr.duration[has] / X.DT) + 1)) <= 1)
    for n in np.flatnonzero(has):
        S_n = tr.n_samples[n]
        assert not np.isnan(tr.positions[n, :S_n]).any() and np.isnan(tr.positions[n, S_n:]).all()
        ticks = np.arange(S_n) * X.DT
        assert np.abs(tr.at(ticks)[n] - tr.positions[n, :S_n]).max() <= 2e-6
        step = np.abs(np.diff(tr.positions[n, :S_n], axis=0))
        # |action| <= 1 at the environment's tick: a step is at most vmax times the distance of two ticks, each (float)i dt rounded once
        assert step.size == 0 or step.max() <= 1.0 * (X.DT + 2.0 ** -23 * tr.duration[n])
        assert np.array_equal(tr.positions[n, 0], nodes[n, 0].astype(np.float32)) and np.array_equal(tr.positions[n, S_n - 1], nodes[n, count[n] - 1].astype(np.float32))
        s = T.blend_schedule(nodes[n, :count[n]].astype(np.float32).astype(np.float64), vmax, amax)
        if count[n] > 2:
            apex = T.law_of(s, s["node_times"][1:-1])
            measured = np.abs(apex - s["nodes"][1:-1]).max(axis=1).max()
            assert np.isclose(tr.corner_deviation[n], measured, rtol=1e-9) and measured > 1e-4
        else:
            assert tr.corner_deviation[n] == 0.0
        assert np.all(tr.peak_velocity[n] <= vmax * (1 + 1e-12)) and np.all(tr.peak_acceleration[n] <= amax * (1 + 1e-9))
        assert np.isclose(tr.duration[n], s["duration"]) and tr.rest_to_rest_duration[n] == T.rest_to_rest_duration(s["nodes"], vmax, amax)
    v = tr.velocities()
    assert v.shape == (5, tr.n_samples.max(), 3) and np.isnan(v[1]).all() and not v[0, 0].any() and np.nanmax(np.abs(v)) <= 1.0 + 1e-9
    small = T.plan_trajectories(T._TwinTrajectories(twin), nodes, count, ob, vmax, amax, X.DT, certify=True, budget=64)
    for name, a, b in zip(tr._fields, tr, small):
        assert (a is None and b is None) or np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f"), name
    plain = T.plan_trajectories(T._TwinTrajectories(twin), nodes, count, ob, vmax, amax, X.DT, positions=False)
    assert plain.positions is None and plain.slack is None and plain.certified is None
    assert np.array_equal(plain.outcome == "blocked", tr.outcome == "blocked") and set(plain.outcome) <= {"free", "blocked", "none"}
    with pytest.raises(ValueError, match=r"query \d lasts .* ticks at dt=1e-05: a trajectory holds at most 8192; dt >= \S+ fits"):
        T.plan_trajectories(T._TwinTrajectories(twin), nodes, count, ob, vmax, amax, 1e-5)
    try:
        T.plan_trajectories(T._TwinTrajectories(twin), nodes, count, ob, vmax, amax, 1e-5)
    except ValueError as err:
        fits = float(re.search(r"dt >= (\S+) fits", str(err)).group(1))
    assert T.plan_trajectories(T._TwinTrajectories(twin), nodes, count, ob, vmax, amax, fits * 1.001, positions=False).n_samples.max() <= 8192


def test_chunks_hold_whole_queries_of_similar_lengths():
    """trajectory_chunks: every query in exactly one chunk; a chunk's S is a multiple of 64 that holds its longest trajectory and is
    at most twice its shortest one's; queries x S within the budget unless the chunk is one query."""
    rng = np.random.default_rng(2)
    ns = np.concatenate([[1, 64, 65, 8192], rng.integers(1, 8193, 200)])
    for budget in (64, 1 << 14, 1 << 23):
        chunks = T.trajectory_chunks(ns, budget)
        assert sorted(np.concatenate([q for q, _ in chunks]).tolist()) == list(range(len(ns)))
        for q, S in chunks:
            up = -(-ns[q] // 64) * 64
            assert S % 64 == 0 and 64 <= S <= 8192 and S == up.max() and S <= 2 * up.min() and (len(q) == 1 or len(q) * S <= budget)
    assert [(q.tolist(), S) for q, S in T.trajectory_chunks([100, 1, 130, 64], 1 << 20)] == [([1, 3, 0], 128), ([2], 192)]


def test_dead_samples_count_in_nothing():
    """chain_traj_common.dead_end_case through the twin's record and the restatement's: the last node is below the margin, every
    live sample before the last is free — ONE blocked sample, the last live one, where a launch that counted its dead samples would
    report 97 of them; the same trajectory with the obstacle away is free."""
    case = X.dead_end_case()
    S_n = int(case.ds.n_samples[0])
    want = T.check_trajectory(case.twin, case.ds, case.obstacles, case.S, case.margin, certify=True)
    out, poses = X.record32(case)
    for rec in (want, out):
        assert rec[0, 3] == S_n - 1 and rec[0, 4] == 1 and rec[0, 7] == 1 and rec[0, 11] >= 0
        assert rec[1, 3] == -1 and rec[1, 4] == 0 and rec[1, 7] == 0
    m = X.margins_at(case, poses)[0, 0]
    assert np.all(np.any(m[S_n - 1:] < case.margin, axis=-1)) and not np.any(m[:S_n - 1] < case.margin) and case.S - S_n == 96
    X.check_poses(case, poses)
    X.check_records(case, out, poses)


def test_a_blended_corner_leaves_its_certified_polyline():
    """chain_traj_common.corner_scene on the twin: the two-leg polyline is certified at the margin; blended at full speed the
    trajectory runs into the sphere beside the corner and is 'blocked'; at a fifth of the speed the deviation is 25 x smaller and
    the trajectory is 'certified'. This is why the trajectory is checked again."""
    model, twin, paths, ob = X.corner_scene()
    c = X.CORNER
    assert certify_polylines_host(twin, paths, ob, c["margin"], 0.02).outcome.tolist() == ["certified"]
    fast, slow = (T.trajectories_host(twin, paths, ob, np.full(3, v), np.full(3, c["amax"]), X.DT, True, c["margin"], positions=False)
                  for v in (c["fast"], c["slow"]))
    print(f"fast: {fast.outcome[0]}, deviation {fast.corner_deviation[0]:.3f} rad, clearance {fast.min_clearance[0]:.4f}; "
          f"slow: {slow.outcome[0]}, deviation {slow.corner_deviation[0]:.3f} rad, slack {slow.slack[0]:.4f}")
    assert fast.outcome.tolist() == ["blocked"] and slow.outcome.tolist() == ["certified"]
    assert np.isclose(fast.corner_deviation[0], 0.5) and np.isclose(slow.corner_deviation[0], 0.02)
    assert fast.first_blocked[0] > 0 and np.isclose(fast.first_blocked_time[0], fast.first_blocked[0] * np.float32(X.DT))


# ---- the façade -------------------------------------------------------------------------------------------------------------------
def test_facade_on_the_host_and_its_refusals():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized,
                                                               InvalidEnvironmentParameter)
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.plan_trajectories(None, max_acceleration=1.0)
    f.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="PyBullet and the synthetic stand-in have no chain model"):
        f.plan_trajectories(None, max_acceleration=1.0)
    f = framework()
    twin = f.env
    rng = np.random.default_rng(4)
    goals = IK.free_poses(twin.model, twin, rng, 6)
    ob = np.tile(twin.obstacle_pos, (6, 1)).astype(np.float64)
    ob[1::2] = twin.end_effector(0.5 * (np.asarray(twin.initial_joint_positions) + goals))[1::2]
    paths = f.plan_joint_paths(goal_joint_positions=goals, obstacles=ob, candidates=4, resolution=0.05, seed=2, roadmap=6, shortcut=8,
                               on_device=False)
    base = dict(paths=paths, obstacles=ob, max_acceleration=4.0, on_device=False)
    tr = f.plan_trajectories(**base)
    has = np.isfinite(np.asarray(paths.length, np.float64))
    print(dict(zip(*np.unique(paths.outcome, return_counts=True))), dict(zip(*np.unique(tr.outcome, return_counts=True))))
    assert isinstance(tr, T.Trajectories) and np.array_equal(tr.outcome != "none", has) and has.any()
    assert "trajectories" not in f.arm_planner.tools and tr.positions.shape[:1] == (6,) and tr.positions.shape[2] == 7
    assert set(tr.outcome) <= {"free", "blocked", "none"} and tr.slack is None
    cert = f.plan_trajectories(**dict(base, certify=True, max_velocity=np.full(7, 0.5), positions=False, clearance_margin=0.001))
    assert set(cert.outcome) <= {"certified", "sampled", "blocked", "none"} and cert.positions is None and cert.slack.shape == (6,)
    assert np.all(cert.duration[has] > tr.duration[has]) and np.nanmax(cert.peak_velocity) <= 0.5 * (1 + 1e-12)
    moves = f.plan_linear_moves(goals[:2], [0.0, 0.0, 0.04], waypoints=8, updates=4, on_device=False)
    lin = f.plan_trajectories(moves.as_joint_paths(), max_acceleration=4.0, on_device=False)
    assert np.array_equal(lin.outcome != "none", moves.outcome == "tracked") and np.array_equal(lin.n_nodes > 0, moves.outcome == "tracked")
    for kw, match in ((dict(paths=tr), "paths is the JointPaths"), (dict(paths=None), "paths is the JointPaths"),
                      (dict(max_acceleration=None), "max_acceleration has no default"),
                      (dict(max_acceleration=0.0), "max_acceleration is positive and finite"),
                      (dict(max_acceleration=[1.0, 2.0]), r"max_acceleration is a positive number, or \[7\]"),
                      (dict(max_acceleration="fast"), "max_acceleration is a positive number"),
                      (dict(max_velocity=-1.0), "max_velocity is positive and finite"), (dict(max_velocity=np.full(7, nan)), "max_velocity"),
                      (dict(max_velocity=True), "max_velocity is a positive number"),
                      (dict(dt=0.0), "dt is a positive time"), (dict(dt=nan), "dt is a positive time"), (dict(dt=True), "dt is a positive"),
                      (dict(certify=1), "certify is a bool"), (dict(positions=1), "positions is a bool"),
                      (dict(clearance_margin=nan), "clearance_margin is a finite length"), (dict(obstacles=np.zeros((2, 3))), "obstacles"),
                      (dict(dt=1e-6), r"plan_trajectories: query \d lasts .* holds at most 8192; dt >= \S+ fits")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.plan_trajectories(**dict(base, **kw))
    assert f.plan_trajectories(paths, ob, 1.0, 4.0, on_device=False).outcome.tobytes() == tr.outcome.tobytes()      # positional


# ---- the plumbing -----------------------------------------------------------------------------------------------------------------
def test_header_symbols_and_argument_errors():
    """The header's "Trajectories" block restates the rule and names the float64 statement; both entry points are exported with the
    header's argument counts within ABI 40; every refusal answers NAF_ERR_ARG from host code, before the handle is dereferenced."""
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40
    for name, count in (("naf_chain_traj_check", 16), ("naf_chain_traj_certify", 18)):
        assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == count
    block = text.split("/* Trajectories (an addition within ABI 40)")[1].split("*/")[0]
    for words in ("environment/trajectory.py", "LEAVES the polyline", "(float)i * dt", "COUNTS IN NOTHING", "64 .. 8192", "2 .. 64",
                  "vpeak_m dt", "NAF_CHAIN_ERR_LDS", "NAF_CHAIN_EDGE_CERT_FLOATS", "t_0 = tau_0 / 2", "exactly"):
        assert words in block, words
    assert T.TRAJ_FLOATS == 8 and T.TRAJ_CERT_FLOATS == 12 and (T.TRAJ_SAMPLES_MIN, T.TRAJ_SAMPLES_MAX, T.TRAJ_NODES_MAX) == (64, 8192, 64)
    declared = re.findall(r"^[a-z][\w \*]*?\b(naf_\w+)\(", text, re.M)      # README's count is the header's, whatever it is
    assert sorted(declared) == sorted(_lib.EXPORTED_SYMBOLS)
    assert f"{len(declared)} entry points" in open(os.path.join(ROOT, "README.md")).read()
    lib = _lib.load()
    assert hasattr(lib, "naf_chain_traj_check") and hasattr(lib, "naf_chain_traj_certify") and lib.naf_hip_abi_version() == 40
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    names = ("h", "nodes", "n_nodes", "times", "vpeak", "n_samples", "o", "rad", "reach", "guard", "dt", "N", "V", "S", "margin", "out")
    good = dict(h=p, nodes=p, n_nodes=p, times=p, vpeak=p, n_samples=p, o=p, rad=0.06, reach=p, guard=1e-4, dt=X.DT, N=1, V=2, S=64,
                margin=0.0, out=p)
    for change in ARGUMENT_ERRORS + CERTIFY_ERRORS:
        a = dict(good, **change)
        assert lib.naf_chain_traj_certify(*[a[k] for k in names], None, None) == NAF_ERR_ARG, change
        if change not in CERTIFY_ERRORS:
            assert lib.naf_chain_traj_check(*[a[k] for k in names if k not in ("reach", "guard")], None, None) == NAF_ERR_ARG, change
    assert not buf.any()

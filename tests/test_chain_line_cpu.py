"""CPU (`-m "not gpu"`): the rule of line moves in environment/line_moves.py (track_line, line_verdict, line_outcomes,
gather_linear_moves, plan_line_moves, LinearMoves.as_joint_paths) against references of its own making; the rehearsal of every GPU
case of tests/test_chain_line_gpu.py with a float32 restatement in the kernel's place, which measures the bounds the GPU tests use;
the façade's arguments and refusals; and the plumbing of naf_chain_line_track."""
import ctypes
import os
import re

import numpy as np
import pytest

import chain_ik_common as IK
import chain_line_common as L
import chain_rollout_common as C
from test_chain_ik_cpu import framework

from robotic_manipulator_rloa_amd.environment import line_moves as LM
from robotic_manipulator_rloa_amd.environment.edge_certificate import polyline_nodes
from robotic_manipulator_rloa_amd.environment.kinematic import EDGE_FLOATS, JointPaths
from robotic_manipulator_rloa_amd.environment.polyline import polyline_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAF_ERR_ARG = -1
_REHEARSED = {}


def rehearse(name, N, W, U, mode):
    """one case with the restatement in the kernel's place: computed once, shared by the tests below"""
    key = (name, N, W, U, mode)
    if key not in _REHEARSED:
        case = L.build_case(*key)
        got = L.track32(case)
        dev, out = L.check_iterations(case, got["iters"], got["nodes"])
        _REHEARSED[key] = (case, got, dev, out, L.check_records(case, got["nodes"], got["track"]))
    return _REHEARSED[key]


@pytest.mark.parametrize("name,N,W,U,mode", L.CASES)
def test_rehearsal(name, N, W, U, mode):
    """Every case of the GPU suite with the float32 restatement (chain_line_common.track32) in the kernel's place: the same checks,
    so the band shares and the populated verdicts hold before a GPU is involved. It measures the single-update deviation,
    teacher-forced over all W U updates, and the deviation of the record floats: the constants of chain_line_common."""
    case, got, dev, out, (res_dev, angle_dev, mid_dev) = rehearse(name, N, W, U, mode)
    print(f"{name} N={N} W={W} U={U} mode={mode}: single-update deviation {dev:.2e} (STEP_DEVIATION {L.STEP_DEVIATION:.2e}), left out "
          f"{out:.4f}, record deviations {res_dev:.2e} / {angle_dev:.2e} / {mid_dev:.2e}")
    assert out == 0.0                                         # the orientation held is the start's own: nothing is near half a turn
    assert dev <= L.STEP_DEVIATION and res_dev <= L.RESIDUAL_DEVIATION and angle_dev <= L.ANGLE_DEVIATION and mid_dev <= L.MID_DEVIATION
    census = L.check_verdict(case, got["track"])
    print(f"    {census}")


def test_the_measured_deviations_are_the_constants():
    """The four constants are the largest values the rehearsal measures over all its cases, rounded up by at most a quarter; the GPU
    bounds are 8 x them."""
    measured = {c: rehearse(*c) for c in L.CASES}
    step = max(v[2] for v in measured.values())
    res, angle, mid = (max(v[4][k] for v in measured.values()) for k in range(3))
    print(f"step {step:.3e} residual {res:.3e} angle {angle:.3e} mid-leg {mid:.3e}")
    for got, const in ((step, L.STEP_DEVIATION), (res, L.RESIDUAL_DEVIATION), (angle, L.ANGLE_DEVIATION), (mid, L.MID_DEVIATION)):
        assert 0.75 * const <= got <= const, (got, const)
    assert (L.STEP_BOUND, L.RESIDUAL_BOUND, L.ANGLE_BOUND, L.MID_BOUND) == tuple(
        8 * v for v in (L.STEP_DEVIATION, L.RESIDUAL_DEVIATION, L.ANGLE_DEVIATION, L.MID_DEVIATION))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_track_line_is_the_existing_updates_and_holds_what_it_is_told():
    """Node i is U of the twin's own updates from node i - 1 towards p0 + (i / W) disp; the goal is the start's own orientation; a
    short line is tracked in every mode and the held quantity stays put while the free one moves."""
    model, twin = IK.arm("iiwa_like7")
    rng = np.random.default_rng(1)
    q0 = C.f32(np.clip(np.array([j.init for j in model.joints]) + 0.1 * rng.normal(size=(6, model.A)), *C.limits_of(model)))
    disp = C.f32(0.04 * np.array([[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0], [0.6, 0.6, 0.0], [0, 0.7, 0.7]]))
    c = LM.line_constants(model)
    W, U = 8, 4
    R0, p0 = twin.end_effector_frame(q0)
    for mode in L.MODES:
        nodes, track, iters = LM.track_line(twin, q0, disp, mode, W, U, c, L.TOOL_AXIS, L.TOOL_NORMAL, record=True)
        assert nodes.shape == (6, W + 1, model.A) and track.shape == (6, W, 4) and iters.shape == (W * U + 1, 6, model.A)
        assert np.array_equal(nodes[:, 0], q0) and np.array_equal(iters[::U], nodes.transpose(1, 0, 2))
        q = q0
        for k in range(W * U):
            g = p0 + ((k // U + 1) / W) * disp
            q = twin.ik_step(q, g, c["lam"], c["e_max"], c["dq_max"]) if mode == LM.HOLD_POSITION else \
                twin.ik_pose_step(q, g, mode, R0 if mode == LM.HOLD_FULL else R0 @ L.TOOL_AXIS, c["lam"], c["e_max"], c["dq_max"],
                                  c["weight"], c["w_max"], L.TOOL_AXIS, L.TOOL_NORMAL)
            assert np.array_equal(q, iters[k + 1])
        K, first_lost = LM.line_verdict(track, 1e-3, 1e-3)
        assert np.all(K == W) and np.all(first_lost == -1)
        R_end, ee_end = twin.end_effector_frame(nodes[:, -1])
        assert np.abs(ee_end - (p0 + disp)).max() <= 1e-4
        turned = np.linalg.norm(R_end - R0, axis=(1, 2))
        tilt = np.linalg.norm(R_end @ L.TOOL_AXIS - R0 @ L.TOOL_AXIS, axis=1)
        if mode == LM.HOLD_FULL:
            assert turned.max() <= 2e-4 and not track[:, :, 1].max() > 1e-4
        elif mode == LM.HOLD_AXIS:
            assert tilt.max() <= 2e-4
        else:
            assert not track[:, :, 1].any() and turned.max() > 1e-3      # nothing holds the orientation
        # the mid-leg distance is an upper bound of the perpendicular deviation there, and small for short legs
        assert track[:, :, 3].max() <= 1e-3 and np.all(track[:, :, 2] > 0.0)
    for bad in (dict(W=0), dict(W=64), dict(U=0), dict(W=63, U=66), dict(mode=3)):
        kw = dict(dict(mode=0, W=4, U=2), **bad)
        with pytest.raises(ValueError):
            LM.track_line(twin, q0, disp, kw["mode"], kw["W"], kw["U"])


def _records(W, blocked=(), first_sample=None):
    """edge records [1][W][8] of free legs, the legs in `blocked` with 3 blocked samples from sample 5 (or first_sample)"""
    rec = np.zeros((1, W, EDGE_FLOATS))
    rec[:, :, :3] = 0.1
    rec[:, :, 3] = -1
    for l in blocked:
        rec[0, l, 3], rec[0, l, 4] = (5 if first_sample is None else first_sample), 3
    return rec


def test_verdict_and_outcomes_on_hand_made_records():
    """line_verdict: K counts the LEADING tracked waypoints — a waypoint back inside the tolerances behind a missed one does not
    count; either tolerance misses; the comparison is <=. line_outcomes: every outcome and the priority start > blocked > lost >
    tracked; a blocked leg behind the tracked prefix does not count; fraction = min(K, first blocked leg) / W."""
    W = 6
    track = np.zeros((5, W, 4))
    track[:, :, 0], track[:, :, 1] = 5e-4, 5e-4
    track[1, 3, 0] = 2e-3                                     # position missed at waypoint 4, tracked again behind it
    track[2, 0, 1] = 2e-3                                     # orientation missed at waypoint 1
    track[3, 5, 0] = 1e-3                                     # exactly the tolerance: tracked
    track[4, 5, 1] = np.nextafter(1e-3, 1.0)                  # one ulp above: lost at the last waypoint
    K, first_lost = LM.line_verdict(track, 1e-3, 1e-3)
    assert K.tolist() == [6, 3, 0, 6, 5] and first_lost.tolist() == [-1, 4, 1, -1, 6]
    one = lambda K, rec: tuple(v[0] for v in LM.line_outcomes(np.array([K]), rec, W))      # noqa: E731
    assert one(6, _records(W)) == ("tracked", -1, 1.0)
    assert one(3, _records(W)) == ("lost", -1, 0.5)
    assert one(0, _records(W)) == ("lost", -1, 0.0)
    assert one(6, _records(W, blocked=[4, 2])) == ("blocked", 2, 2 / 6)
    assert one(3, _records(W, blocked=[2])) == ("blocked", 2, 2 / 6)          # blocked before lost
    assert one(3, _records(W, blocked=[3, 5])) == ("lost", -1, 0.5)           # legs behind the tracked prefix do not count
    assert one(6, _records(W, blocked=[0])) == ("blocked", 0, 0.0)            # leg 0 blocked from sample 5: not the start pose
    assert one(6, _records(W, blocked=[0, 3], first_sample=0)) == ("start", 0, 0.0)
    assert one(0, _records(W, blocked=[0], first_sample=0)) == ("start", 0, 0.0)      # start before lost


def _moves(reverse=False, N=4, W=5, A=3, K=(5, 2, 5, 0)):
    rng = np.random.default_rng(3)
    nodes = rng.uniform(-1, 1, (N, W + 1, A)).astype(np.float32)
    track = np.full((N, W, 4), 1e-4, np.float32)
    track[:, :, 2] = np.abs(nodes[:, 1:] - nodes[:, :-1]).max(axis=-1)
    rec = np.repeat(_records(W), N, axis=0).astype(np.float32)
    rec[:, :, 5] = track[:, :, 2]
    rec[:, :, 6] = rec[:, :, 5] / 63
    rec[2, 3, 3], rec[2, 3, 4] = 7, 1                         # query 2: leg 3 blocked
    p0, disp = rng.uniform(-1, 1, (N, 3)).astype(np.float32), rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    return nodes, LM.gather_linear_moves(nodes, track, rec, 64, np.array(K), p0, disp, W, reverse)


def test_gather_reverse_and_as_joint_paths():
    """gather_linear_moves: the fields of a tracked, a lost, a blocked and an entirely lost query; reverse flips the tracked prefix's
    nodes and swaps start and goal while first_lost and first_blocked_leg keep counting from the given pose; as_joint_paths() gives
    the tracked queries a polyline that polyline_nodes and polyline_plan read as they read a 'roadmap' one, the others none."""
    nodes, mv = _moves()
    W = 5
    assert mv.outcome.tolist() == ["tracked", "lost", "blocked", "lost"] and mv.n_nodes.tolist() == [6, 3, 6, 1]
    assert mv.first_lost.tolist() == [-1, 3, -1, 1] and mv.first_blocked_leg.tolist() == [-1, -1, 3, -1]
    assert np.allclose(mv.fraction, [1.0, 0.4, 0.6, 0.0])
    assert np.array_equal(mv.start, nodes[:, 0]) and np.array_equal(mv.goal, nodes[np.arange(4), [5, 2, 5, 0]])
    assert np.array_equal(mv.nodes[1, :3], nodes[1, :3]) and np.isnan(mv.nodes[1, 3:]).all() and np.isnan(mv.nodes[3, 1:]).all()
    assert np.isnan(mv.position_error[3]) and np.isnan(mv.min_clearance[3]) and mv.position_error[0] == np.float32(1e-4)
    assert mv.joint_step[1] == np.abs(nodes[1, 1:] - nodes[1, :-1]).max() and mv.samples.tolist() == [64] * 4
    _, rv = _moves(reverse=True)
    for a, b in zip(mv, rv):
        if a is not mv.nodes and a is not mv.start and a is not mv.goal:
            assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    assert np.array_equal(rv.start, mv.goal) and np.array_equal(rv.goal, mv.start)
    for n, K in enumerate([5, 2, 5, 0]):
        assert np.array_equal(rv.nodes[n, :K + 1], mv.nodes[n, :K + 1][::-1]) and np.isnan(rv.nodes[n, K + 1:]).all()
    for moves in (mv, rv):
        paths = moves.as_joint_paths()
        assert isinstance(paths, JointPaths) and paths.outcome.tolist() == ["line", "blocked", "blocked", "blocked"]
        assert paths.n_nodes.tolist() == [W + 1, 0, 0, 0] and np.all(paths.candidate == -1) and np.isnan(paths.via).all()
        legs = np.abs(np.diff(moves.nodes[0], axis=0)).max(axis=-1)
        want = np.float32(0)
        for v in legs:
            want = want + v
        assert paths.length[0] == want and np.isnan(paths.length[1:]).all()
        assert paths.straight_length[0] == np.abs(moves.goal[0] - moves.start[0]).max()
        got, count = polyline_nodes(paths)
        assert count.tolist() == [W + 1, 0, 0, 0] and np.array_equal(got[0], moves.nodes[0].astype(np.float64))
        plan = polyline_plan(paths, np.asarray(paths.start, np.float64), np.asarray(paths.start, np.float64),
                             np.asarray(paths.goal, np.float64), 1.0, 400)
        assert plan.leg_actions.shape[:2] == (4, W) and np.all(np.asarray(plan.n_ticks)[0] >= 1)
        assert np.asarray(plan.n_ticks)[1:].tolist() == [[1] + [0] * (W - 1)] * 3      # no path: one tick standing still


# ---- the façade -------------------------------------------------------------------------------------------------------------------
def test_plan_linear_moves_on_the_host_end_to_end():
    """solve_goal_poses(approach_directions=[0, 0, -1]) then the 8 cm retreat straight up at W = 16, U = 4 through the twin: every
    line is 'tracked' with the twin's own margins — measured when the case was written: position error 1.1e-5 m, angle error 1.5e-5
    rad, mid-leg deviation 8.2e-6 m, joint step 0.022 rad — the certificate and the demonstration take as_joint_paths() unchanged,
    and reverse=True ends at the given poses. The 25 cm move with the orientation held loses queries to limits and reach."""
    f = framework()
    twin = f.env
    rng = np.random.default_rng(8)
    N = 8
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.1, 0.1, (N, 3))
    goal = f.solve_goal_poses(targets, approach_directions=[0, 0, -1], iterations=64, seed=3, on_device=False)
    assert goal.reachable.all()
    q = goal.joint_positions
    mv = f.plan_linear_moves(q, [0, 0, 0.08], waypoints=16, updates=4, on_device=False)
    assert isinstance(mv, LM.LinearMoves) and mv.outcome.tolist() == ["tracked"] * N and np.all(mv.fraction == 1.0)
    assert np.all(mv.first_lost == -1) and np.all(mv.first_blocked_leg == -1) and np.all(mv.n_nodes == 17)
    assert mv.position_error.max() <= 5e-5 and mv.angle_error.max() <= 5e-5 and mv.line_deviation.max() <= 5e-5
    assert 0.005 <= mv.joint_step.max() <= 0.05 and np.all(mv.min_clearance > 0.0) and np.all(mv.samples == 64)
    assert np.array_equal(mv.start, C.f32(q)) and np.array_equal(mv.nodes[:, 0], mv.start) and np.array_equal(mv.nodes[:, -1], mv.goal)
    R0, p0 = twin.end_effector_frame(mv.start)
    R1, p1 = twin.end_effector_frame(mv.goal)
    assert np.abs(p1 - (p0 + [0, 0, 0.08])).max() <= 5e-5 and np.abs(R1 - R0).max() <= 5e-5
    assert np.allclose(mv.end_effector_start, p0) and np.allclose(mv.displacement, [0, 0, 0.08])
    # every sampled pose of every leg stays near the line: the joint-linear legs bend away from it by less than the mid-leg bound
    t = np.linspace(0, 1, 5)[None, None, :, None]
    poses = mv.nodes[:, :-1, None, :] * (1 - t) + mv.nodes[:, 1:, None, :] * t
    ee = twin.end_effector(poses)
    off = ee - p0[:, None, None, :]
    assert np.abs(off[..., :2]).max() <= 1e-4
    rv = f.plan_linear_moves(q, [0, 0, 0.08], waypoints=16, updates=4, on_device=False, reverse=True)
    assert np.array_equal(rv.goal, mv.start) and np.array_equal(rv.start, mv.goal) and np.array_equal(rv.nodes, mv.nodes[:, ::-1])
    paths = rv.as_joint_paths()
    cert = f.certify_joint_paths(paths, clearance_margin=0.002, on_device=False)
    assert "none" not in cert.outcome.tolist() and cert.certified.all()
    demos = f.demonstrate_joint_paths(paths, polylines=True, on_device=False)
    assert demos.outcome.tolist() == ["reached"] * N
    # position hold leaves the orientation free; axis hold keeps the tool pointing down
    ax = f.plan_linear_moves(q[:3], [0.03, 0, 0.05], hold="axis", waypoints=8, updates=4, on_device=False)
    assert ax.outcome.tolist() == ["tracked"] * 3
    R2, _ = twin.end_effector_frame(ax.goal)
    assert np.abs((R2 - R0[:3]) @ np.array([0, 0, 1.0])).max() <= 5e-5
    po = f.plan_linear_moves(q[:3], [0.03, 0, 0.05], hold="position", waypoints=8, updates=4, on_device=False)
    assert po.outcome.tolist() == ["tracked"] * 3 and not po.angle_error.any()
    far = f.plan_linear_moves(q, [0, 0, 0.25], waypoints=32, updates=2, on_device=False)
    lost = far.outcome == "lost"
    assert lost.any() and np.all(far.first_lost[lost] >= 1) and np.all(far.fraction[lost] < 1.0)
    assert np.array_equal(far.n_nodes[lost], far.first_lost[lost]) and far.as_joint_paths().n_nodes[lost].max() == 0
    # an obstacle on the line blocks it, and one on the given pose is reported as 'start'
    hit = f.plan_linear_moves(q[:2], [0, 0, -0.06], obstacles=p0[:2] + [0, 0, -0.15], waypoints=16, updates=4, on_device=False)
    assert hit.outcome.tolist() == ["blocked"] * 2 and np.all(hit.first_blocked_leg >= 1) and np.all(hit.fraction < 1.0)
    at = f.plan_linear_moves(q[:2], [0, 0, 0.08], obstacles=p0[:2], waypoints=16, updates=4, on_device=False)
    assert at.outcome.tolist() == ["start"] * 2 and not at.fraction.any()


def test_facade_refusals():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized,
                                                               InvalidEnvironmentParameter)
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.plan_linear_moves(np.zeros(7), [0, 0, 0.1])
    f.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="PyBullet and the synthetic stand-in have no chain model"):
        f.plan_linear_moves(np.zeros(7), [0, 0, 0.1])
    f = framework()
    q = np.tile(f.env.initial_joint_positions, (4, 1))
    base = dict(joint_positions=q, displacements=[0, 0, 0.05], waypoints=2, updates=1, on_device=False)
    assert f.plan_linear_moves(**base).outcome.shape == (4,) and f.plan_linear_moves(**dict(base, joint_positions=q[0])).outcome.shape == (1,)
    for kw, match in ((dict(joint_positions=np.zeros((4, 6))), r"joint_positions is \[N\]\[7\]"),
                      (dict(joint_positions="pose"), "joint_positions is not an array"),
                      (dict(joint_positions=np.where(np.arange(28).reshape(4, 7) == 9, np.nan, q)), r"joint_positions\[1\] is not finite"),
                      (dict(joint_positions=np.where(np.arange(28).reshape(4, 7) == 14, 9.0, q)),
                       r"joint_positions of query 2: joint 0 \(involved_joints\[0\]\).*outside its limits"),
                      (dict(displacements=np.zeros((3, 3)) + 0.1), r"displacements is \[N\]\[3\] with N = 4"),
                      (dict(displacements=[0, 0.1]), "displacements is"),
                      (dict(displacements=[[0, 0, 0.1]] * 3 + [[0, np.inf, 0]]), r"displacements\[3\] is not finite"),
                      (dict(displacements=[[0, 0, 0.1], [0, 0, 0], [0, 0, 0.1], [0, 0, 0.1]]), r"displacements\[1\] has length 0"),
                      (dict(waypoints=0), "waypoints is a number of waypoints from 1 to 63"), (dict(waypoints=64), "waypoints"),
                      (dict(waypoints=2.0), "waypoints"), (dict(waypoints=True), "waypoints"),
                      (dict(updates=0), "updates is a positive number"), (dict(updates=1.5), "updates"),
                      (dict(waypoints=63, updates=66), r"waypoints x updates <= 4096"),
                      (dict(hold="roll"), "hold is one of 'orientation', 'axis', 'position'"), (dict(hold=0), "hold is one of"),
                      (dict(hold="axis", tool_axis=[0, 0, 0]), "tool_axis has length 0"), (dict(tool_axis=[1, 0]), r"tool_axis is \[3\]"),
                      (dict(tolerance=0.0), "tolerance is a positive length"), (dict(tolerance=float("nan")), "tolerance"),
                      (dict(orientation_tolerance=-1.0), "orientation_tolerance is a positive angle"),
                      (dict(orientation_tolerance=float("inf")), "orientation_tolerance"),
                      (dict(resolution=0.0), "resolution"), (dict(clearance_margin=float("nan")), "clearance_margin"),
                      (dict(reverse=1), "reverse is a bool"), (dict(obstacles=np.zeros((2, 3))), "obstacles")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.plan_linear_moves(**dict(base, **kw))


# ---- the plumbing -----------------------------------------------------------------------------------------------------------------
def test_header_symbol_and_argument_errors():
    """The header's "Line moves" block restates the rule and names the float64 statement; the entry point is exported with the
    header's argument count within ABI 40; every refusal answers NAF_ERR_ARG from host code, before the handle is dereferenced."""
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40
    name = "naf_chain_line_track"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 13
    assert re.search(r"^#define NAF_CHAIN_TRACK_FLOATS 4$", text, re.M) and LM.TRACK_FLOATS == 4
    block = text.split("/* Line moves (an addition within ABI 40)")[1].split("*/")[0]
    for words in ("environment/line_moves.py", "formed ONCE", "W U <= 4096", "1 .. 63", "(float)i / (float)W", "0.5f", "line_verdict",
                  "params.iterations and pose_params.angle_length are not read", "pose_params is not read in mode 2", "NAF_CHAIN_ERR_LDS"):
        assert words in block, words
    declared = re.findall(r"^[a-z][\w \*]*?\b(naf_\w+)\(", text, re.M)      # README's count is the header's, whatever it is
    assert sorted(declared) == sorted(_lib.EXPORTED_SYMBOLS)
    assert f"{len(declared)} entry points" in open(os.path.join(ROOT, "README.md")).read()
    lib = _lib.load()
    assert hasattr(lib, name) and lib.naf_hip_abi_version() == 40
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    f3 = ctypes.c_float * 3
    nan, inf = float("nan"), float("inf")
    ok, pose = _lib.IkParams(0, 0.01, 0.3, 0.5), _lib.IkPoseParams(0.2, 0.5, nan, f3(0, 0, 1), f3(1, 0, 0))
    names = ("h", "q_start", "disp", "mode", "N", "W", "U", "prm", "pose", "nodes", "track")
    good = dict(h=p, q_start=p, disp=p, mode=0, N=1, W=1, U=1, prm=ok, pose=pose, nodes=p, track=p)
    bad = [{k: None} for k in ("h", "q_start", "disp", "nodes", "track")]
    bad += [dict(N=0), dict(N=-3), dict(W=0), dict(W=64), dict(U=0), dict(W=63, U=66), dict(mode=3), dict(mode=-1)]
    bad += [dict(prm=_lib.IkParams(9, *v)) for v in ((nan, 0.3, 0.5), (0.0, 0.3, 0.5), (0.01, inf, 0.5), (0.01, 0.0, 0.5), (0.01, 0.3, -1.0),
                                                     (0.01, 0.3, nan))]
    bad += [dict(mode=2, prm=_lib.IkParams(9, 0.01, 0.3, 0.0))]
    for mode in (0, 1):
        for v in ((0.0, 0.5), (nan, 0.5), (0.2, 0.0), (0.2, inf), (-0.2, 0.5)):
            bad.append(dict(mode=mode, pose=_lib.IkPoseParams(*v, 1.0, f3(0, 0, 1), f3(1, 0, 0))))
        bad.append(dict(mode=mode, pose=_lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, nan, 1), f3(1, 0, 0))))
        bad.append(dict(mode=mode, pose=_lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, 0, 1), f3(1, inf, 0))))
    for change in bad:
        a = dict(good, **change)
        assert lib.naf_chain_line_track(*[a[k] for k in names], None, None) == NAF_ERR_ARG, change
    assert not buf.any()

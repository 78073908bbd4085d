"""GPU (`-m gpu`): naf_chain_line_track (csrc/chain_env.hip) against the float64 rule of environment/line_moves.py through the C
ABI; chain_line.LineTracker and ManipulatorFramework.plan_linear_moves against that path; the certificate and the demonstration of
tracked lines; and that nothing else in the process changes. tests/test_chain_line_cpu.py rehearses every case with a float32
restatement, which is where the bounds come from."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_ik_common as IK
import chain_line_common as L
import chain_rollout_common as C
from test_chain_env_gpu import _agent
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment import line_moves as LM

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAF_ERR_ARG = -1
PAD = 3                        # queries' worth of rows behind the N queries' that no lane may write


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def line_params(lib_module, model, tool_axis=L.TOOL_AXIS, tool_normal=L.TOOL_NORMAL):
    """(naf_chain_ik_params_t, naf_chain_ik_pose_params_t); iterations and angle_length, which are not read, hold refusable values"""
    c = L.constants(model)
    f3 = ctypes.c_float * 3
    return (lib_module.IkParams(0, c["lam2"], c["e_max"], c["dq_max"]),
            lib_module.IkPoseParams(c["weight"], c["w_max"], float("nan"), f3(*map(float, tool_axis)), f3(*map(float, tool_normal))))


class LineRig:
    """The tracking launch of one case through the C ABI; every output has poisoned rows behind the queries'."""

    def __init__(self, case):
        from robotic_manipulator_rloa_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.case = case
        model, N, W, U = case.model, case.N, case.W, case.U
        self.N, self.W, self.U, self.A = N, W, U, model.A
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.q_start, self.disp = dev(case.q_start), dev(case.disp)
        nan = dict(fill_value=float("nan"), device=DEV)
        self.nodes = torch.full((N + PAD, W + 1, self.A), **nan)
        self.track = torch.full((N + PAD, W, LM.TRACK_FLOATS), **nan)
        self.iters = torch.full((W * U + 2, N, self.A), **nan)
        self.prm, self.pose = line_params(_lib, model)

    def call(self, iters=True, stream=None, **change):
        a = dict(h=self.h, q_start=self.q_start.data_ptr(), disp=self.disp.data_ptr(), mode=self.case.mode, N=self.N, W=self.W, U=self.U,
                 prm=self.prm, pose=self.pose, nodes=self.nodes.data_ptr(), track=self.track.data_ptr(),
                 iters=self.iters.data_ptr() if iters else None,
                 st=torch.cuda.current_stream().cuda_stream if stream is None else stream)
        a.update(change)
        return self.lib.naf_chain_line_track(*[a[k] for k in ("h", "q_start", "disp", "mode", "N", "W", "U", "prm", "pose", "nodes", "track",
                                                              "iters", "st")])

    def poisoned(self):
        N, W, U = self.N, self.W, self.U
        return bool(torch.isnan(self.nodes[N:]).all() and torch.isnan(self.track[N:]).all() and torch.isnan(self.iters[W * U + 1]).all())

    def run(self, iters=True, stream=None):
        assert self.call(iters, stream) == 0
        torch.cuda.synchronize()
        assert self.poisoned()
        N, W, U = self.N, self.W, self.U
        return dict(nodes=self.nodes[:N].cpu().numpy(), track=self.track[:N].cpu().numpy(), iters=self.iters[:W * U + 1].cpu().numpy())

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


@pytest.mark.parametrize("name,N,W,U,mode", L.CASES)
def test_line_track_against_the_rule(name, N, W, U, mode):
    """One case through the C ABI, iters_out on. (1) Teacher-forced: every recorded update within chain_line_common.STEP_BOUND (8 x
    the float32 restatement's measured single-update deviation) of the twin's step at the recorded pose towards its waypoint's line
    point; the limits hold exactly; iters_out[0] is q_start and iters_out[i U] equals nodes_out[:, i] bit for bit. (2) Soundness,
    independent of the twin's tracker: the residual, the angle and the mid-leg distance within 8 x their measured deviations of
    line_record at the returned nodes, the joint step bit for bit the float32 difference of the nodes; every waypoint of a tracked
    prefix within tolerance + 2 tol_of(model) of its line point and orientation_tolerance + ANGLE_BOUND of the held orientation, by
    the twin. (3) Completeness: K per query equals the twin's; no query is without room to spare, by construction; with N >= 64
    both verdicts are populated (slider4 holds no orientation along a drawn line: all 'lost'). The poisoned rows behind nodes_out
    and track_out and the iters_out rows beyond W U + 1 keep their poison."""
    case = L.build_case(name, N, W, U, mode)
    rig = LineRig(case)
    got = rig.run()
    rig.close()
    dev, out = L.check_iterations(case, got["iters"], got["nodes"])
    res_dev, angle_dev, mid_dev = L.check_records(case, got["nodes"], got["track"])
    census = L.check_verdict(case, got["track"])
    print(f"{name} N={N} W={W} U={U} mode={mode}: teacher-forced deviation {dev:.2e} (bound {L.STEP_BOUND:.2e}), left out {out:.4f}, record "
          f"deviations {res_dev:.2e} / {angle_dev:.2e} / {mid_dev:.2e} (bounds {L.RESIDUAL_BOUND:.1e} / {L.ANGLE_BOUND:.1e} / "
          f"{L.MID_BOUND:.1e}), {census}")
    assert dev <= L.STEP_BOUND, (dev, L.STEP_BOUND)
    assert res_dev <= L.RESIDUAL_BOUND and angle_dev <= L.ANGLE_BOUND and mid_dev <= L.MID_BOUND, (res_dev, angle_dev, mid_dev)


@pytest.mark.parametrize("mode", L.MODES)
def test_placement_independence_through_the_c_abi(mode):
    """Query 64 of the 65-query case alone (N = 1: lane 0 of the only wave) gives the bits it gives among the 65 (lane 0 of the
    second wave), and query 37 alone the bits of lane 37; a run without iters_out and one on a side stream give the bits of the first."""
    case = L.build_case("iiwa_like7", 65, 8, 4, mode)
    rig = LineRig(case)
    full = rig.run()
    plain = rig.run(iters=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = rig.run(iters=False, stream=side.cuda_stream)
    rig.close()
    for k in ("nodes", "track"):
        assert np.array_equal(bits(full[k]), bits(plain[k])) and np.array_equal(bits(full[k]), bits(on_side[k])), k
    for i in (64, 37):
        one = LineRig(case.sub(np.array([i])))
        alone = one.run()
        one.close()
        for k in ("nodes", "track"):
            assert np.array_equal(bits(full[k][i:i + 1]), bits(alone[k])), (k, i)
        assert np.array_equal(bits(full["iters"][:, i:i + 1]), bits(alone["iters"]))


def test_argument_errors_return_err_arg_without_a_launch():
    """Every refusal of naf_chain_line_track with a real handle and real buffers: NAF_ERR_ARG, and the poisoned outputs keep their
    poison — nothing was launched. What is not read is not refused: iterations = 0, angle_length = NaN, and in mode 2 pose
    parameters that modes 0 / 1 refuse."""
    from robotic_manipulator_rloa_amd import _lib
    case = L.build_case("slider4", 5, 16, 2, LM.HOLD_AXIS)
    rig = LineRig(case)
    c = L.constants(case.model)
    nan, inf = float("nan"), float("inf")
    f3 = ctypes.c_float * 3
    axis, normal = f3(0, 0, 1), f3(1, 0, 0)
    bad = [{k: None} for k in ("h", "q_start", "disp", "nodes", "track")]
    bad += [dict(N=0), dict(N=-1), dict(W=0), dict(W=64), dict(U=0), dict(U=-2), dict(W=63, U=66), dict(mode=3), dict(mode=-1)]
    bad += [dict(prm=_lib.IkParams(32, *v)) for v in ((0.0, c["e_max"], c["dq_max"]), (nan, c["e_max"], c["dq_max"]),
                                                      (c["lam2"], inf, c["dq_max"]), (c["lam2"], -1.0, c["dq_max"]),
                                                      (c["lam2"], c["e_max"], 0.0), (c["lam2"], c["e_max"], nan))]
    bad += [dict(mode=2, prm=_lib.IkParams(32, c["lam2"], c["e_max"], 0.0))]
    poses = [_lib.IkPoseParams(*v, 1.0, axis, normal) for v in ((0.0, 0.5), (-1.0, 0.5), (0.2, nan), (0.2, inf), (0.2, 0.0))]
    poses += [_lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, nan, 1), normal), _lib.IkPoseParams(0.2, 0.5, 1.0, axis, f3(inf, 0, 0))]
    bad += [dict(mode=mode, pose=pose) for mode in (0, 1) for pose in poses]
    for change in bad:
        assert rig.call(iters=False, **change) == NAF_ERR_ARG, change
    torch.cuda.synchronize()
    assert torch.isnan(rig.nodes).all() and torch.isnan(rig.track).all() and torch.isnan(rig.iters).all()
    for pose in poses:                                        # mode 2 does not read them
        assert rig.call(iters=False, mode=2, pose=pose) == 0
    torch.cuda.synchronize()
    assert rig.poisoned() and not torch.isnan(rig.track[:rig.N]).any()
    rig.close()


@pytest.mark.parametrize("name,N,W,U,mode,chunk", [("iiwa_like7", 65, 8, 4, LM.HOLD_FULL, 16), ("long12", 5, 16, 2, LM.HOLD_AXIS, 2),
                                                   ("slider4", 65, 8, 4, LM.HOLD_POSITION, None)])
def test_line_tracker_equals_the_c_abi_path(name, N, W, U, mode, chunk):
    """chain_line.LineTracker against the C-ABI launch, bit for bit, with a chunk that splits N (65 = 4 x 16 + 1, 5 = 2 + 2 + 1)
    and with the default one; its buffers do not exist before the first call."""
    from robotic_manipulator_rloa_amd.chain_line import LineTracker
    case = L.build_case(name, N, W, U, mode)
    rig = LineRig(case)
    want = rig.run(iters=False)
    rig.close()
    tracker = LineTracker(case.model, L.ORAD, chunk=chunk)
    assert tracker.nodes is None and tracker.out is None and tracker.q_start is None
    nodes, track = tracker.track(case.q_start, case.disp, mode, W, U, L.constants(case.model), L.TOOL_AXIS, L.TOOL_NORMAL)
    assert tracker.launches == (1 if chunk is None else -(-N // chunk))
    assert nodes.dtype == track.dtype == np.float32
    assert np.array_equal(bits(nodes), bits(want["nodes"])) and np.array_equal(bits(track), bits(want["track"]))


def _framework():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(**IIWA_RANGED)
    return f


def _approach_poses(f, N, on_device=None):
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.1, 0.1, (N, 3))
    goal = f.solve_goal_poses(targets, approach_directions=[0, 0, -1], iterations=64, seed=3, on_device=on_device)
    return goal


@pytest.mark.parametrize("hold,disp,W,U", [("orientation", [0.0, 0.0, 0.25], 32, 2), ("position", [0.1, 0.0, 0.1], 8, 4)])
def test_plan_linear_moves_equals_tracker_edge_records_and_the_verdict(scratch_cwd, hold, disp, W, U):
    """plan_linear_moves on the device against LineTracker + JointPathChecker.edge_records + the shared verdict and gather, field for
    field and bit for bit; the 25 cm move with the orientation held populates 'lost' beside 'tracked'."""
    from robotic_manipulator_rloa_amd.chain_line import LineTracker
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    from robotic_manipulator_rloa_amd.environment.kinematic import edge_samples, joint_distance32, tool_normal_of
    f = _framework()
    env = f.env
    N = 24
    goal = _approach_poses(f, N)
    q = goal.joint_positions[goal.reachable]
    n = len(q)
    obstacles = np.tile(np.asarray(env.obstacle_centre, np.float32), (n, 1))
    got = f.plan_linear_moves(q, disp, hold=hold, waypoints=W, updates=U, reverse=True)
    mode = LM.HOLD_MODES[hold]
    axis = np.array([0.0, 0.0, 1.0], np.float32)
    tracker, checker = LineTracker(env.model, env.obstacle_radius), JointPathChecker(env.model, env.obstacle_radius)
    d = np.tile(np.asarray(disp, np.float32), (n, 1))
    nodes, track = tracker.track(q, d, mode, W, U, LM.line_constants(env.model), axis, tool_normal_of(axis.astype(np.float64)).astype(np.float32))
    K, _ = LM.line_verdict(track, np.float32(1e-3), np.float32(1e-3))
    S = edge_samples(joint_distance32(nodes[:, 1:], nodes[:, :-1]), 0.02)
    edges = np.stack([np.arange(W), np.arange(1, W + 1)], axis=1).astype(np.int32)
    rec = checker.edge_records(nodes, edges, obstacles, S, 0.0)
    want = LM.gather_linear_moves(nodes, track, rec, S, K, env.end_effector(q.astype(np.float64)).astype(np.float32), d, W, True)
    for name, a, b in zip(want._fields, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    census = dict(zip(*np.unique(got.outcome, return_counts=True)))
    print(hold, disp, census)
    if hold == "orientation":
        assert census.get("lost", 0) >= 1 and census.get("tracked", 0) >= 1


def test_framework_retreat_end_to_end(scratch_cwd):
    """IIWA_RANGED, N = 24: solve_goal_poses(approach_directions=[0, 0, -1]) then the 8 cm line straight up at W = 16, U = 4 with
    reverse=True. The device's outcomes equal the twin's (on_device=False) for every query whose twin records have room to spare;
    the tracked lines are straight and upright by the twin; certify_joint_paths and demonstrate_joint_paths(polylines=True) take
    as_joint_paths() and report no 'none' for a 'tracked' query; demonstrations of certified lines show no contact drop."""
    f = _framework()
    twin = f.env
    N = 24
    goal = _approach_poses(f, N)
    ok = goal.reachable
    assert ok.mean() >= 0.75
    q = goal.joint_positions[ok]
    kw = dict(waypoints=16, updates=4, reverse=True)
    mv = f.plan_linear_moves(q, [0, 0, 0.08], **kw)
    host = f.plan_linear_moves(q, [0, 0, 0.08], on_device=False, **kw)
    assert mv.nodes.dtype == np.float32 and host.nodes.dtype == np.float64
    # the twin's records with room to spare: errors of the tracked prefix within a quarter of the tolerances, clearances off the margin
    clear = np.minimum(np.minimum(host.min_clearance, host.min_self_clearance), host.min_cell_clearance)
    sure = (host.outcome == "tracked") & (host.position_error <= 2.5e-4) & (host.angle_error <= 2.5e-4) & (clear > 8 * C.tol_of(twin.model))
    print(dict(zip(*np.unique(mv.outcome, return_counts=True))), int(sure.sum()), len(q))
    assert sure.sum() >= len(q) - 2 and np.array_equal(mv.outcome[sure], host.outcome[sure])
    tracked = mv.outcome == "tracked"
    assert np.array_equal(mv.goal[tracked], q[tracked]) and np.all(mv.n_nodes[tracked] == 17)
    R0, p0 = twin.end_effector_frame(mv.goal.astype(np.float64))
    R1, p1 = twin.end_effector_frame(mv.start.astype(np.float64))
    assert np.abs(p1 - (p0 + [0, 0, 0.08]))[tracked].max() <= 1e-3 + 2 * C.tol_of(twin.model)
    assert np.abs((R1 - R0) @ np.array([0, 0, 1.0]))[tracked].max() <= 1e-3 + L.ANGLE_BOUND
    assert np.abs(mv.position_error - host.position_error)[sure].max() <= 1e-4
    paths = mv.as_joint_paths()
    assert np.array_equal(paths.outcome == "line", tracked) and np.array_equal(paths.n_nodes >= 2, tracked)
    cert = f.certify_joint_paths(paths, clearance_margin=0.002)
    demos = f.demonstrate_joint_paths(paths, polylines=True)
    assert not np.any(cert.outcome[tracked] == "none") and not np.any(demos.outcome[tracked] == "none")
    assert np.all(cert.outcome[~tracked] == "none") and np.all(demos.outcome[~tracked] == "none")
    certified = np.asarray(cert.certified, bool)
    assert certified.any()
    contact = np.isin(demos.outcome, ("obstacle", "self", "workcell"))
    assert not contact[certified].any(), demos.outcome[certified]
    # the joint-space path to the far end of the approach: reverse=True makes `start` the pregrasp pose
    to_pregrasp = f.plan_joint_paths(goal_joint_positions=mv.start[tracked])
    assert to_pregrasp.outcome.shape == (int(tracked.sum()),)


def test_off_means_off(scratch_cwd):
    """A fixed-seed DeviceEnvLoop stream (test_chain_rollout_gpu's) hashes the same before and after line moves have been planned in
    the same process, and solve_goal_poses with and without an orientation goal returns the bits it returned before them."""
    model, _ = C.arm("iiwa_like7", True)
    agent = _agent(model)
    before = _training_stream_digest(agent, model, False)
    f = _framework()
    rng = np.random.default_rng(3)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.1, 0.1, (16, 3))
    plain, down = f.solve_goal_poses(targets, seed=5), f.solve_goal_poses(targets, approach_directions=[0, 0, -1], seed=5)
    for hold in LM.HOLD_MODES:
        mv = f.plan_linear_moves(down.joint_positions, [0, 0, 0.08], hold=hold, waypoints=16, updates=4)
        assert mv.outcome.shape == (16,)
    assert f.arm_planner.tools["line_moves"][1].launches == 3
    assert _training_stream_digest(agent, model, False) == before
    plain2, down2 = f.solve_goal_poses(targets, seed=5), f.solve_goal_poses(targets, approach_directions=[0, 0, -1], seed=5)
    for a, b in ((plain, plain2), (down, down2)):
        for name, x, y in zip(a._fields, a, b):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert plain2.angle_residual is None and down.angle_residual.tobytes() == down2.angle_residual.tobytes()

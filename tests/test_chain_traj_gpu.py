"""GPU (`-m gpu`): naf_chain_traj_check and naf_chain_traj_certify (csrc/chain_env.hip) against the float64 rule of
environment/trajectory.py (trajectory_law, check_trajectory) through the C ABI; chain_traj.TrajectoryChecker and
ManipulatorFramework.plan_trajectories against the float64 twin; the scene in which a blended corner is blocked where its polyline
is certified; and that a session which never asks for a trajectory never launches one. tests/test_chain_traj_cpu.py rehearses every
case with a float32 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_edgecert_common as E
import chain_roadmap_common as R
import chain_rollout_common as C
import chain_traj_common as X
from test_chain_rollout_gpu import IIWA_RANGED
from test_chain_traj_cpu import ARGUMENT_ERRORS, CERTIFY_ERRORS

from robotic_manipulator_rloa_amd.environment import trajectory as T
from robotic_manipulator_rloa_amd.environment.kinematic import certificate_guard, reach_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 3                        # trajectories' worth of records and poses behind the N of the launch that no lane may write


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class TrajRig:
    """The two trajectory launches of one case through the C ABI; out and poses_out have PAD poisoned items behind the launch's."""

    def __init__(self, case, orad=X.ORAD):
        from robotic_manipulator_rloa_amd import _lib
        self.lib, self.case, self.orad = _lib.load(), case, float(np.float32(orad))
        model, ds = case.model, case.ds
        self.N, self.S, self.A = case.N, case.S, model.A
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a, t=np.float32: torch.from_numpy(np.ascontiguousarray(a, t)).to(DEV)      # noqa: E731
        self.nodes, self.times, self.vpeak, self.obstacles = dev(ds.nodes), dev(ds.times), dev(ds.vpeak), dev(case.obstacles)
        self.n_nodes, self.n_samples = dev(ds.n_nodes, np.int32), dev(ds.n_samples, np.int32)
        self.reach, self.guard = dev(reach_table(model)), certificate_guard(model)
        nan = dict(fill_value=float("nan"), device=DEV)
        self.out = torch.full((self.N + PAD, 12), **nan)
        self.poses = torch.full((self.N + PAD, self.S, self.A), **nan)

    def call(self, certify=True, poses=True, **over):
        """the entry point's return code, with the case's arguments but for `over`"""
        p = lambda t: t.data_ptr()      # noqa: E731
        case = self.case
        a = dict(h=self.h, nodes=p(self.nodes), n_nodes=p(self.n_nodes), times=p(self.times), vpeak=p(self.vpeak),
                 n_samples=p(self.n_samples), o=p(self.obstacles), rad=self.orad, reach=p(self.reach), guard=self.guard, dt=case.dt,
                 N=case.N, V=case.V, S=case.S, margin=case.margin, out=p(self.out))
        a.update(over)
        tail = (a["dt"], a["N"], a["V"], a["S"], a["margin"], a["out"], p(self.poses) if poses else None,
                torch.cuda.current_stream().cuda_stream)
        head = (a["h"], a["nodes"], a["n_nodes"], a["times"], a["vpeak"], a["n_samples"], a["o"], a["rad"])
        if certify:
            return self.lib.naf_chain_traj_certify(*head, a["reach"], a["guard"], *tail)
        return self.lib.naf_chain_traj_check(*head, *tail)

    def run(self, certify=True, poses=True):
        """returns (out[N, 12 | 8], poses[N, S, A]) as numpy copies"""
        floats = 12 if certify else 8
        self.out.fill_(float("nan"))
        self.poses.fill_(float("nan"))
        assert self.call(certify, poses) == 0
        torch.cuda.synchronize()
        flat = self.out.view(-1)
        assert torch.isnan(flat[self.N * floats:]).all() and torch.isnan(self.poses[self.N:]).all()
        return flat[:self.N * floats].view(self.N, floats).cpu().numpy(), self.poses[:self.N].cpu().numpy()

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


@pytest.mark.parametrize("name,N,L,S", X.CASES)
def test_trajectory_launches_against_the_rule(name, N, L, S):
    """One case through the C ABI (the case is the one the CPU rehearsal verified with the twin; the cap and the floors are asserted
    again here, at the recorded poses). Poses: within POSE_BOUND of the float64 law at every live sample, the rows i >= S_n the
    last node bit for bit, the PAD rows poisoned. Records, teacher-forced at the recorded poses (chain_traj_common.check_records),
    for the certifying launch and for the plain one, whose eight floats are the certifying launch's to the bit on the same poses. A
    run without poses_out gives the same bits. The arms between them launch all twelve instantiations."""
    case = X.build(name, N, L, S, verify=False)
    rig = TrajRig(case)
    out, poses = rig.run()
    quiet, none = rig.run(poses=False)
    plain, poses8 = rig.run(certify=False)
    rig.close()
    assert np.isnan(none).all() and np.array_equal(bits(out), bits(quiet))
    X.check_poses(case, poses)
    X.check_records(case, out, poses)
    assert np.array_equal(bits(poses), bits(poses8)) and np.array_equal(bits(out[:, 5:8]), bits(plain[:, 5:8]))
    X.check_records(case, plain, poses8, certify=False)
    tol = C.tol_of(case.model)
    for k in range(3):
        got, want = out[:, k].astype(np.float64), plain[:, k].astype(np.float64)
        both_inf = np.isposinf(got) & np.isposinf(want)
        assert np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want)).max() <= tol, k


def test_dead_samples_count_in_nothing():
    """chain_traj_common.dead_end_case on the device: the last node is below the margin and three quarters of the launch evaluate
    to it, yet ONE sample is blocked — the last live one, which [7] reports; the same trajectory with the obstacle away is free."""
    case = X.dead_end_case()
    rig = TrajRig(case)
    out, poses = rig.run()
    rig.close()
    S_n = int(case.ds.n_samples[0])
    print(out.tolist())
    assert out[0, 3] == S_n - 1 and out[0, 4] == 1 and out[0, 7] == 1 and out[0, 11] >= 0
    assert out[1, 3] == -1 and out[1, 4] == 0 and out[1, 7] == 0
    X.check_poses(case, poses)
    X.check_records(case, out, poses)


def test_refusals_launch_nothing():
    """Every NAF_ERR_ARG case on a real handle, for both entry points: the return code, and the poisoned buffers stay poisoned."""
    rig = TrajRig(X.build("planar3", 5, 2, 128, verify=False))
    for kw in ARGUMENT_ERRORS + CERTIFY_ERRORS:
        assert rig.call(True, **{**dict(N=1, V=2, S=64), **kw}) == -1, kw
        if kw not in CERTIFY_ERRORS:
            assert rig.call(False, **{**dict(N=1, V=2, S=64), **kw}) == -1, kw
    torch.cuda.synchronize()
    assert torch.isnan(rig.out).all() and torch.isnan(rig.poses).all()
    out, _ = rig.run()
    rig.close()
    assert not np.isnan(out).any()


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
def _against_the_twin(model, twin, paths, ob, margin, vmax, amax, orad):
    """TrajectoryChecker.plan against trajectories_host, certify on: the schedule's fields are equal outright (they are the host's);
    the device's clearances and slacks lie within w = 4 tol + 2^-20 beta + 2 POSE_BOUND reach of the twin's, so every verdict lies
    between the twin's at margin - w and margin + w: where those two twin runs agree, the outcome and the first blocked tick are
    the twin's at the margin."""
    from robotic_manipulator_rloa_amd.chain_traj import TrajectoryChecker
    w = 4 * C.tol_of(model) + 2.0 ** -20 * 0.25 + 2 * X.POSE_BOUND * model.reach
    tool = TrajectoryChecker(model, orad)
    dev = tool.plan(paths, ob, vmax, amax, X.DT, True, margin)
    m32 = float(np.float32(margin))
    host, below, above = (T.trajectories_host(twin, paths, ob, vmax, amax, X.DT, True, m32 + d) for d in (0.0, -w, w))
    sure = (below.outcome == above.outcome) & (below.first_blocked == above.first_blocked)
    print(f"outcomes {dict(zip(*np.unique(dev.outcome, return_counts=True)))}, {int(sure.sum())} of {len(sure)} queries sure, "
          f"{tool.launches} launches, ticks {dev.n_samples.tolist()}")
    assert isinstance(dev, T.Trajectories) and sure.sum() >= len(sure) // 2
    assert np.array_equal(dev.outcome[sure], host.outcome[sure]) and np.array_equal(dev.first_blocked[sure], host.first_blocked[sure])
    assert np.array_equal(dev.outcome == "none", host.outcome == "none")
    for f in ("duration", "rest_to_rest_duration", "n_samples", "corner_deviation", "peak_velocity", "leg_times", "blend_times", "n_nodes"):
        assert np.array_equal(getattr(dev, f), getattr(host, f), equal_nan=True), f
    has = host.outcome != "none"
    assert dev.min_clearance.dtype == np.float32 and dev.positions.dtype == np.float32 and dev.slack.dtype == np.float32
    assert np.all(np.abs(dev.min_clearance[has].astype(np.float64) - host.min_clearance[has]) <= w)
    both = has & np.isfinite(host.slack)
    assert np.all(np.abs(dev.slack[both].astype(np.float64) - host.slack[both]) <= w)
    assert dev.positions.shape == host.positions.shape and np.array_equal(np.isnan(dev.positions), np.isnan(host.positions))
    assert np.nanmax(np.abs(dev.positions.astype(np.float64) - host.positions)) <= X.POSE_BOUND
    quiet = tool.plan(paths, ob, vmax, amax, X.DT, True, margin, positions=False)
    assert quiet.positions is None and quiet.outcome.tobytes() == dev.outcome.tobytes() and quiet.slack.tobytes() == dev.slack.tobytes()
    return dev, host, tool


def test_trajectory_checker_end_to_end_against_the_twin():
    """On the 24-query iiwa_like7 set planned with roadmap=14 and shortcut=16, and on tracked Cartesian lines handed on by
    as_joint_paths(): outcomes equal wherever no tick is in a band, durations equal, 'none' where there is no path; a chunk of one
    launch's worth per trajectory gives the same bytes; a trajectory of too many ticks is refused by name."""
    from robotic_manipulator_rloa_amd.chain_traj import TrajectoryChecker
    from robotic_manipulator_rloa_amd.environment.line_moves import _TwinLines, plan_line_moves
    model, twin = R.arm("iiwa_like7")
    paths, ob, margin = E.polyline_paths("iiwa_like7", E.SHORTCUT, R.IIWA_CUT)
    vmax, amax = np.full(model.A, 3.0), np.full(model.A, 12.0)      # (a few hundred ticks per query: the twin runs them three times)
    dev, host, tool = _against_the_twin(model, twin, paths, ob, margin, vmax, amax, R.ORAD)
    assert (dev.outcome == "none").any() or np.all(np.isfinite(np.asarray(paths.length, np.float64)))
    assert len(set(dev.outcome) - {"none"}) >= 2
    small = TrajectoryChecker(model, R.ORAD, chunk=64).plan(paths, ob, vmax, amax, X.DT, True, margin)
    for name, a, b in zip(dev._fields, dev, small):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), name
    with pytest.raises(ValueError, match=r"query \d+ lasts .* holds at most 8192; dt >= \S+ fits"):
        tool.plan(paths, ob, vmax, amax, 1e-5)
    rng = np.random.default_rng(6)
    q = R.IK.free_poses(model, twin, rng, 6)
    far = np.tile(C.away(model)[1], (6, 1))
    moves = plan_line_moves(_TwinLines(twin), q, np.tile([0.0, 0.0, 0.04], (6, 1)), far, 0, 8, 4)
    lines = moves.as_joint_paths()
    dev2, _, _ = _against_the_twin(model, twin, lines, far, margin, vmax, amax, R.ORAD)
    assert np.array_equal(dev2.outcome != "none", moves.outcome == "tracked") and (moves.outcome == "tracked").any()


def test_a_blended_corner_leaves_its_certified_polyline():
    """chain_traj_common.corner_scene on the device: PolylineCertifier certifies the two-leg polyline at the margin;
    TrajectoryChecker finds the trajectory blended at full speed 'blocked' and the one at a fifth of the speed 'certified'."""
    from robotic_manipulator_rloa_amd.chain_certify import PolylineCertifier
    from robotic_manipulator_rloa_amd.chain_traj import TrajectoryChecker
    model, twin, paths, ob = X.corner_scene()
    c = X.CORNER
    assert PolylineCertifier(model, c["orad"]).certify(paths, ob, c["margin"], 0.02).outcome.tolist() == ["certified"]
    tool = TrajectoryChecker(model, c["orad"])
    fast, slow = (tool.plan(paths, ob, np.full(3, v), np.full(3, c["amax"]), X.DT, True, c["margin"]) for v in (c["fast"], c["slow"]))
    print(f"fast: {fast.outcome[0]} at tick {fast.first_blocked[0]}, clearance {fast.min_clearance[0]:.4f}; slow: {slow.outcome[0]}, "
          f"slack {slow.slack[0]:.4f}, {slow.n_samples[0]} ticks")
    assert fast.outcome.tolist() == ["blocked"] and slow.outcome.tolist() == ["certified"] and slow.n_samples[0] > 2048


# ---- the façade ----------------------------------------------------------------------------------------------------------------------
def test_framework_plan_trajectories_and_off_means_off(monkeypatch, scratch_cwd):
    """plan_trajectories on the device equals TrajectoryChecker of the same paths byte for byte and the twin (on_device=False) in
    its outcomes wherever no tick is in a band; a second call reuses the cached tool; plan_joint_paths' results and the
    training-state digest are what they are without the call; and a session that never calls the method never creates the tool
    and never calls either entry point (monkeypatched to raise)."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_traj import TrajectoryChecker
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    env = f.env
    before = f.naf_agent.training_state_digest()
    rng = np.random.default_rng(8)
    N = 12
    goals = R.IK.free_poses(env.model, env, rng, N)
    start = np.tile(env.initial_joint_positions, (N, 1))
    ob = np.tile(env.obstacle_centre if env.scene_ranges_on else env.obstacle_pos, (N, 1)).astype(np.float64)
    ob[1::2] = env.end_effector(0.5 * (start + goals))[1::2]
    kw = dict(goal_joint_positions=goals, obstacles=ob, candidates=1, resolution=0.05, seed=3, roadmap=R.ROADMAP, shortcut=E.SHORTCUT)
    paths = f.plan_joint_paths(**kw)
    assert "trajectories" not in f.arm_planner.tools
    tkw = dict(obstacles=ob, max_velocity=3.0, max_acceleration=12.0, certify=True, clearance_margin=0.002)
    got = f.plan_trajectories(paths, **tkw)
    tool = f.arm_planner.tools["trajectories"][1]
    want = TrajectoryChecker(env.model, env.obstacle_radius).plan(paths, ob, np.full(7, 3.0), np.full(7, 12.0), 1.0 / 240.0, True, 0.002)
    print({o: int(np.sum(got.outcome == o)) for o in sorted(set(got.outcome))}, "of", {o: int(np.sum(paths.outcome == o)) for o in sorted(set(paths.outcome))})
    for name, x, y in zip(got._fields, got, want):
        assert np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
    w = 4 * C.tol_of(env.model) + 2.0 ** -20 * 0.25 + 2 * X.POSE_BOUND * env.model.reach
    below, above = (f.plan_trajectories(paths, **dict(tkw, clearance_margin=0.002 + d, on_device=False, positions=False)) for d in (-w, w))
    host = f.plan_trajectories(paths, **dict(tkw, on_device=False, positions=False))
    sure = below.outcome == above.outcome
    assert sure.sum() >= N // 2 and np.array_equal(got.outcome[sure], host.outcome[sure])
    assert np.array_equal(got.duration.astype(np.float32), host.duration.astype(np.float32))
    assert np.array_equal(got.outcome == "none", (paths.candidate < 0) & (paths.n_nodes < 2)) and (got.outcome != "none").any()
    again = f.plan_trajectories(paths, **tkw)
    assert f.arm_planner.tools["trajectories"][1] is tool and again.outcome.tobytes() == got.outcome.tobytes()
    assert f.naf_agent.training_state_digest() == before
    replanned = f.plan_joint_paths(**kw)
    for name, x, y in zip(paths._fields, replanned, paths):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name

    def boom(*args):
        raise AssertionError("a trajectory launch without plan_trajectories")
    monkeypatch.setattr(_lib.load(), "naf_chain_traj_check", boom)
    monkeypatch.setattr(_lib.load(), "naf_chain_traj_certify", boom)
    g = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    fresh = g.naf_agent.training_state_digest()
    quiet = g.plan_joint_paths(**kw)
    g.certify_joint_paths(quiet, obstacles=ob, clearance_margin=0.002, resolution=0.05)
    g.demonstrate_joint_paths(quiet, obstacles=ob, polylines=True)
    assert quiet.outcome.tobytes() == paths.outcome.tobytes() and "trajectories" not in g.arm_planner.tools
    assert g.naf_agent.training_state_digest() == fresh

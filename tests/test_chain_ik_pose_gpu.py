"""GPU (`-m gpu`): naf_chain_ik_solve_pose (csrc/chain_env.hip) against the float64 rule of environment/kinematic.py
(orientation_error, ik_pose_step, solve_ik_pose), through the C ABI, with naf_chain_ik_select fed its merit; chain_tools.GoalPoseSolver
and ManipulatorFramework.solve_goal_poses / plan_joint_paths with orientation goals against that path; and that without orientation
arguments every launch and every bit is what it was. tests/test_chain_ik_pose_cpu.py rehearses every case with a float32 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_ik_common as IK
import chain_ik_pose_common as P
import chain_rollout_common as C
from test_chain_env_gpu import _agent
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment.kinematic import (ORIENT_AXIS, ORIENT_FULL, gather_goal_poses, ik_seeds,
                                                                orientation_goal)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAF_ERR_ARG = -1
PAD = 28                       # rows behind the N R candidates that no lane may write


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pose_params(lib_module, model, tool_axis=P.TOOL_AXIS, tool_normal=P.TOOL_NORMAL, angle_length=P.ANGLE_LENGTH):
    c = P.constants(model)
    f3 = ctypes.c_float * 3
    return lib_module.IkPoseParams(c["weight"], c["w_max"], angle_length, f3(*map(float, tool_axis)), f3(*map(float, tool_normal)))


class PoseRig:
    """The oriented goal-pose launches of one case through the C ABI; every output has PAD poisoned rows behind the candidates'."""

    def __init__(self, case):
        from robotic_manipulator_rloa_amd import _lib
        self._lib = _lib
        self.lib = _lib.load()
        self.case = case
        model, N, R = case.model, case.N, case.R
        self.N, self.R, self.A, self.E = N, R, model.A, N * R
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.targets, self.q_start, self.goals = dev(case.targets), dev(case.q_start), dev(case.goals)
        self.seeds = dev(case.seeds.reshape(self.E, self.A))
        self.scene = dev(np.repeat(np.concatenate([case.targets, case.obstacles], axis=1), R, axis=0))
        nan = dict(fill_value=float("nan"), device=DEV)
        E = self.E
        self.q = torch.full((E + PAD, self.A), **nan)
        self.residual, self.angle, self.merit = (torch.full((E + PAD,), **nan) for _ in range(3))
        self.iters = torch.full((P.K + 2, E, self.A), **nan)
        self.st = torch.full((E + PAD, self.lib.naf_chain_env_state_floats(self.h)), **nan)
        self.obs = torch.full((E + PAD, 2 * self.A + 9), **nan)
        self.probe = torch.full((E + PAD, 5), **nan)
        self.cell = torch.full((E + PAD,), **nan)
        self.jd = torch.full((E + PAD,), **nan)
        self.choice = torch.full((N + PAD,), -7, dtype=torch.int32, device=DEV)
        self.cls = torch.full((N + PAD,), -7, dtype=torch.int32, device=DEV)
        self.has_cell = bool(model.cell_pairs)
        c = P.constants(model)
        self.prm = _lib.IkParams(P.K, c["lam2"], c["e_max"], c["dq_max"])
        self.pose = pose_params(_lib, model)

    def run(self, iters=True, stream=None):
        """solve_pose -> reset_given -> probe(s) -> select on merit; returns the numpy copies of what the candidates' rows hold"""
        lib, st = self.lib, torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        assert lib.naf_chain_ik_solve_pose(self.h, p(self.targets), p(self.goals), self.case.mode, p(self.q_start), p(self.seeds), self.N,
                                           self.R, self.prm, self.pose, p(self.q), p(self.residual), p(self.angle), p(self.merit),
                                           p(self.iters) if iters else None, st) == 0
        assert lib.naf_chain_env_reset_given(self.h, p(self.st), p(self.obs), self.E, p(self.q), p(self.scene), P.ORAD, st) == 0
        assert lib.naf_chain_env_probe(self.h, p(self.st), p(self.probe), self.E, st) == 0
        if self.has_cell:
            assert lib.naf_chain_env_probe_cell(self.h, p(self.st), p(self.cell), self.E, st) == 0
        assert lib.naf_chain_ik_select(self.h, p(self.q), p(self.q_start), p(self.merit), p(self.probe),
                                       p(self.cell) if self.has_cell else None, self.N, self.R, P.TOLERANCE, self.case.margin,
                                       p(self.choice), p(self.cls), p(self.jd), st) == 0
        torch.cuda.synchronize()
        E, N = self.E, self.N
        for t in (self.q, self.residual, self.angle, self.merit, self.probe, self.jd):
            assert torch.isnan(t[E:]).all()
        assert torch.isnan(self.iters[P.K + 1]).all() and (self.choice[N:] == -7).all() and (self.cls[N:] == -7).all()
        cell = self.cell[:E].cpu().numpy() if self.has_cell else np.full(E, np.inf, np.float32)
        out = {k: getattr(self, k)[:E].cpu().numpy() for k in ("q", "residual", "angle", "merit", "probe", "jd")}
        out.update(iters=self.iters[:P.K + 1].cpu().numpy(), cell=cell, choice=self.choice[:N].cpu().numpy().astype(np.int64),
                   cls=self.cls[:N].cpu().numpy().astype(np.int64))
        return out

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


@pytest.mark.parametrize("name,N,R,mode", P.CASES)
def test_solve_pose_and_select_against_the_rule(name, N, R, mode):
    """One case through the C ABI, iters_out on. (1) Teacher-forced: every recorded update within chain_ik_pose_common.STEP_BOUND
    (8 x the float32 restatement's measured single-step deviation) of ik_pose_step applied to the recorded pose before it, max-norm
    over the joints; left out are the updates whose twin pose has quaternion w < 1e-3 (full) or |t x d| < 1e-2 with t . d < 0
    (axis), at most 1 % of the case's. (2) Soundness, every candidate: residual_out within 2 tol, angle_out within ANGLE_BOUND
    (8 x the measured deviation) and merit_out within the larger of the two of the twin's numbers at q_out; merit_out is
    max(residual_out, angle_out angle_length) bit for bit; a query reported reachable has position and angle within their
    tolerances plus that slack. (3) Completeness: every query the twin solves at a quarter of both tolerances from the same seeds
    is reported reachable (no query of a case lies between that and tolerance), every 1.1-reach query unreachable. (4) choice,
    class and joint_distance equal select_goal_pose fed merit_out and the probes' outputs, bit for bit; with N R >= 64 every class
    is populated. The PAD rows behind every output, and the iters_out rows beyond K + 1, keep their poison."""
    case = P.build_case(name, N, R, mode)
    rig = PoseRig(case)
    got = rig.run()
    rig.close()
    dev, out = P.check_iterations(case, got["iters"])
    print(f"{name} N={N} R={R} mode={mode}: largest teacher-forced deviation {dev:.2e} (bound {P.STEP_BOUND:.2e}), left out {out:.4f}")
    assert dev <= P.STEP_BOUND, (dev, P.STEP_BOUND)
    assert np.array_equal(bits(got["iters"][P.K]), bits(got["q"]))
    P.check_solution(case, got, got["probe"], got["cell"], got["choice"], got["cls"], got["jd"])


@pytest.mark.parametrize("mode", P.MODES)
def test_placement_independence_through_the_c_abi(mode):
    """Query 37 of the 64 x 8 case alone (N = 1, lanes 0 .. 7 of one wave) gives the bits it gives among the 64 (lanes 40 .. 47 of
    the fifth wave); a run without iters_out and one on a side stream give the bits of the first."""
    case = P.build_case("iiwa_like7", 64, 8, mode)
    rig = PoseRig(case)
    all64 = rig.run()
    plain = rig.run(iters=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = rig.run(iters=False, stream=side.cuda_stream)
    rig.close()
    keys = ("q", "residual", "angle", "merit", "probe", "cell", "jd")
    for k in keys:
        assert np.array_equal(bits(all64[k]), bits(plain[k])) and np.array_equal(bits(all64[k]), bits(on_side[k])), k
    i, R = 37, case.R
    one = PoseRig(case.sub(np.array([i])))
    alone = one.run()
    one.close()
    rows = slice(i * R, (i + 1) * R)
    for k in keys:
        assert np.array_equal(bits(all64[k][rows]), bits(alone[k])), k
    assert np.array_equal(bits(all64["iters"][:, rows]), bits(alone["iters"]))
    assert all64["choice"][i] == alone["choice"][0] and all64["cls"][i] == alone["cls"][0]


def test_argument_errors_return_err_arg_without_a_launch():
    """Every refusal of naf_chain_ik_solve_pose with a real handle and real buffers: NAF_ERR_ARG, and the poisoned outputs keep
    their poison — nothing was launched."""
    from robotic_manipulator_rloa_amd import _lib
    case = P.build_case("slider4", 8, 4, ORIENT_AXIS)
    rig = PoseRig(case)
    lib, p, st = rig.lib, (lambda t: t.data_ptr()), torch.cuda.current_stream().cuda_stream
    good = dict(h=rig.h, targets=p(rig.targets), goals=p(rig.goals), mode=1, q_start=p(rig.q_start), seeds=p(rig.seeds), N=rig.N, R=rig.R,
                prm=rig.prm, pose=rig.pose, q=p(rig.q), residual=p(rig.residual), angle=p(rig.angle), merit=p(rig.merit), iters=None, st=st)
    c = P.constants(case.model)
    bad = [dict(h=None)] + [{k: None} for k in ("targets", "goals", "q_start", "seeds", "q", "residual", "angle", "merit")]
    bad += [dict(N=0), dict(R=3), dict(R=128), dict(mode=2), dict(mode=-1)]
    bad += [dict(prm=_lib.IkParams(*v)) for v in ((0, c["lam2"], c["e_max"], c["dq_max"]), (P.K, 0.0, c["e_max"], c["dq_max"]),
                                                  (P.K, c["lam2"], float("nan"), c["dq_max"]), (P.K, c["lam2"], c["e_max"], float("inf")))]
    f3 = ctypes.c_float * 3
    axis, normal = f3(0, 0, 1), f3(1, 0, 0)
    for v in ((0.0, 0.5, 1.0), (-1.0, 0.5, 1.0), (0.2, float("nan"), 1.0), (0.2, 0.5, float("inf")), (0.2, 0.5, 0.0)):
        bad.append(dict(pose=_lib.IkPoseParams(*v, axis, normal)))
    bad.append(dict(pose=_lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, float("nan"), 1), normal)))
    bad.append(dict(pose=_lib.IkPoseParams(0.2, 0.5, 1.0, axis, f3(float("inf"), 0, 0))))
    for change in bad:
        a = dict(good, **change)
        rc = lib.naf_chain_ik_solve_pose(a["h"], a["targets"], a["goals"], a["mode"], a["q_start"], a["seeds"], a["N"], a["R"], a["prm"],
                                         a["pose"], a["q"], a["residual"], a["angle"], a["merit"], a["iters"], a["st"])
        assert rc == NAF_ERR_ARG, (change, rc)
    torch.cuda.synchronize()
    for t in (rig.q, rig.residual, rig.angle, rig.merit):
        assert torch.isnan(t).all()
    rig.close()


@pytest.mark.parametrize("name,N,R,chunk,mode", [("iiwa_like7", 17, 4, 64, ORIENT_FULL), ("iiwa_like7", 17, 4, 64, ORIENT_AXIS),
                                                 ("long12", 5, 4, None, ORIENT_FULL), ("long12", 5, 4, None, ORIENT_AXIS)])
def test_goal_pose_solver_equals_the_c_abi_path(name, N, R, chunk, mode):
    """chain_tools.GoalPoseSolver with orientation goals, with the seeds it draws, against the C-ABI launches fed ik_seeds of the
    same seed and orientation_goal's float32 goals: every field of GoalPoses and angle_residual bit for bit. Chunks of 64
    candidates: 17 x 4 is a chunk of 16 queries and one of a single query; None: the default chunk."""
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    rng = np.random.default_rng(5)
    base = P.build_case(name, 5, 4, mode)
    rows = np.arange(N) % base.N
    twin = base.twin
    frames, _ = twin.end_effector_frame(np.stack([P.random_q(base.model, rng) for _ in range(N)]))
    if mode == ORIENT_FULL:
        quats = rng.normal(size=(N, 4))
        kw = dict(orientations=quats)
    else:
        kw = dict(approach_directions=3.0 * (frames @ P.TOOL_AXIS))      # (any length: it is scaled to a unit direction)
    og = orientation_goal(N, tolerance=P.TOLERANCE, orientation_tolerance=P.ORIENTATION_TOLERANCE, **kw)
    assert og.mode == mode and og.goals.dtype == np.float32 and og.angle_length == P.ANGLE_LENGTH
    seeds = ik_seeds(base.model, N, R, seed=11).astype(np.float64)
    case = P.PoseCase(name, N, R, mode, base.q_start[rows], base.targets[rows], og.goals.astype(np.float64), base.obstacles[rows], seeds,
                      base.want[rows])
    rig = PoseRig(case)
    got = rig.run(iters=False)
    rig.close()
    A = case.model.A
    sh = lambda k: got[k].reshape(N, R)      # noqa: E731
    want = gather_goal_poses(got["choice"], got["cls"], got["q"].reshape(N, R, A), sh("residual"), got["probe"][:, 3].reshape(N, R),
                             got["probe"][:, 4].reshape(N, R), sh("cell"), sh("jd"), np.float32(P.TOLERANCE), sh("angle"), sh("merit"))
    solver = GoalPoseSolver(case.model, P.ORAD, chunk=chunk)
    assert solver.goals is None and solver.angle is None and solver.merit is None      # not allocated before they are needed
    out = solver.solve(case.q_start, case.targets, case.obstacles, restarts=R, iterations=P.K, tolerance=P.TOLERANCE, seed=11,
                       orientation_tolerance=P.ORIENTATION_TOLERANCE, **kw)
    for f, a, b in zip(want._fields, out, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert out.angle_residual.dtype == np.float32 and out.angle_residual.tobytes() == want.angle_residual.tobytes()
    assert np.array_equal(out.reachable, np.maximum(out.residual, out.angle_residual * np.float32(P.ANGLE_LENGTH)) <= np.float32(P.TOLERANCE))


def test_framework_approach_from_above_end_to_end(scratch_cwd):
    """solve_goal_poses(approach_directions=[0, 0, -1]) on iiwa_like7 returns poses whose twin tool axis is within
    orientation_tolerance (plus the measured float32 slack) of straight down and whose twin end effector is on the target;
    plan_joint_paths(targets, approach_directions=...) plans to exactly those poses; a full quaternion goal is met the same way;
    the host twin under the same rule agrees on reachability wherever it converges with room to spare."""
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    N = 24
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.1, 0.1, (N, 3))
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(**IIWA_RANGED)
    twin = f.env
    down = [0.0, 0.0, -1.0]
    goal = f.solve_goal_poses(targets, approach_directions=down, iterations=64, seed=3)
    assert goal.angle_residual is not None and goal.reachable.mean() >= 0.75
    ok = goal.reachable
    R_ee, ee = twin.end_effector_frame(goal.joint_positions.astype(np.float64))
    t = R_ee @ np.array([0.0, 0.0, 1.0])
    angle = np.arctan2(np.linalg.norm(np.cross(t, down), axis=1), t @ np.array(down))
    assert np.all(angle[ok] <= 1e-3 + P.ANGLE_BOUND), angle[ok].max()
    assert np.all(np.linalg.norm(ee - targets.astype(np.float32), axis=1)[ok] <= 1e-3 + 2 * C.tol_of(twin.model))
    assert np.abs(goal.angle_residual - angle).max() <= P.ANGLE_BOUND
    host = f.solve_goal_poses(targets, approach_directions=down, iterations=64, seed=3, on_device=False)
    merit = np.maximum(host.residual, host.angle_residual)
    sure = (merit <= 1e-3 / 4) | (merit > 4e-3)
    assert sure.sum() >= N - 3 and np.array_equal(goal.reachable[sure], host.reachable[sure])
    # the paths lead to the poses solve_goal_poses returns with its defaults and the same seed
    default = f.solve_goal_poses(targets, approach_directions=down, seed=3)
    paths = f.plan_joint_paths(targets, approach_directions=down, seed=3)
    ok = default.reachable
    assert ok.any() and np.array_equal(paths.outcome == "goal", ~ok)
    assert np.array_equal(bits(paths.goal[ok]), bits(default.joint_positions[ok]))
    # a full orientation: the frame of a known pose, as a quaternion
    q_known = np.clip(twin.initial_joint_positions + 0.2 * rng.normal(size=(N, twin.n)), *C.limits_of(twin.model))
    R_known, t_known = twin.end_effector_frame(q_known)
    quat = np.stack([_quaternion_of(R) for R in R_known])
    full = f.solve_goal_poses(t_known, orientations=quat, iterations=64, seed=3)
    assert full.reachable.mean() >= 0.75
    R_got, _ = twin.end_effector_frame(full.joint_positions.astype(np.float64))
    E = R_known @ np.swapaxes(R_got, -1, -2)
    theta = np.arccos(np.clip((np.trace(E, axis1=-2, axis2=-1) - 1.0) / 2.0, -1.0, 1.0))
    assert np.all(theta[full.reachable] <= 1e-3 + 1e-4)      # (arccos near 0 resolves 1e-8 in its argument to 1e-4 rad)


def _quaternion_of(R):
    """(x, y, z, w) of a rotation matrix by its largest component"""
    tr = np.trace(R)
    forms = [np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + tr]),
             np.array([1.0 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]]),
             np.array([R[0, 1] + R[1, 0], 1.0 + R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]]),
             np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]])]
    quat = forms[int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))]
    return quat / np.linalg.norm(quat)


def test_off_means_off(scratch_cwd):
    """Without orientation arguments solve_goal_poses returns the bits of the old C-ABI path (naf_chain_ik_solve, never the pose
    kernel) with angle_residual None and the solver's pose buffers unallocated; and a fixed-seed DeviceEnvLoop stream
    (test_chain_rollout_gpu's) hashes the same before and after oriented goal poses have been solved in the same process."""
    from test_chain_ik_gpu import IkRig
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    model, _ = C.arm("iiwa_like7", True)
    agent = _agent(model)
    before = _training_stream_digest(agent, model, False)
    rng = np.random.default_rng(3)
    N = 64
    solver = GoalPoseSolver(model, IK.ORAD)
    q0 = np.tile([j.init for j in model.joints], (N, 1))
    out = solver.solve(q0, rng.uniform(-0.5, 0.5, (N, 3)), rng.uniform(-0.5, 0.5, (N, 3)), approach_directions=[0, 0, -1])
    assert out.angle_residual is not None and solver.goals is not None
    assert _training_stream_digest(agent, model, False) == before
    # the positional call through the facade against the positional C-ABI launches
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(**IIWA_RANGED)
    env = f.env
    n, R = 16, 8
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.15, 0.15, (n, 3))
    got = f.solve_goal_poses(targets, seed=5)
    assert got.angle_residual is None and f.arm_planner.tools["goal_poses"][1].goals is None
    start = np.tile(env.initial_joint_positions, (n, 1))
    case = IK.Case("iiwa_like7", n, R, C.f32(start), C.f32(targets), C.f32(np.tile(env.obstacle_centre, (n, 1))),
                   ik_seeds(env.model, n, R, seed=5).astype(np.float64), np.zeros(n, np.int64))
    case.model, case.twin = env.model, env
    rig = IkRig(case)
    rig.prm = rig._lib.IkParams(32, float(0.05 * env.model.reach) ** 2, float(0.25 * env.model.reach), 0.5)
    rig.iters = torch.full((IK.K + 2, rig.E, rig.A), float("nan"), device=DEV)
    old = rig.run(iters=False)
    rig.close()
    A = env.model.A
    sh = lambda a: a.reshape(n, R)      # noqa: E731
    want = gather_goal_poses(old["choice"], old["cls"], old["q"].reshape(n, R, A), sh(old["residual"]), sh(old["probe"][:, 3]),
                             sh(old["probe"][:, 4]), sh(old["cell"]), sh(old["jd"]), np.float32(1e-3))
    for name, a, b in zip(want._fields, got, want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name

"""GPU (`-m gpu`): naf_chain_ik_solve / naf_chain_ik_select (csrc/chain_env.hip) against the float64 rule of environment/kinematic.py,
through the C ABI; chain_tools.GoalPoseSolver, ManipulatorFramework.solve_goal_poses and reach_targets(goal_poses=True) against that
path; and that training launches are untouched. tests/test_chain_ik_cpu.py rehearses every case with a float32 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_ik_common as IK
import chain_rollout_common as C
from test_chain_env_gpu import _agent
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment.kinematic import ik_seeds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 28                       # rows behind the N R candidates that no lane may write


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class IkRig:
    """The goal-pose launches of one case through the C ABI; every output has PAD poisoned rows behind the candidates'."""

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
        self.targets, self.q_start = dev(case.targets), dev(case.q_start)
        self.seeds = dev(case.seeds.reshape(self.E, self.A))
        self.scene = dev(np.repeat(np.concatenate([case.targets, case.obstacles], axis=1), R, axis=0))
        nan = dict(fill_value=float("nan"), device=DEV)
        E = self.E
        self.q = torch.full((E + PAD, self.A), **nan)
        self.residual = torch.full((E + PAD,), **nan)
        self.iters = torch.full((IK.K + 2, E, self.A), **nan)
        self.st = torch.full((E + PAD, self.lib.naf_chain_env_state_floats(self.h)), **nan)
        self.obs = torch.full((E + PAD, 2 * self.A + 9), **nan)
        self.probe = torch.full((E + PAD, 5), **nan)
        self.cell = torch.full((E + PAD,), **nan)
        self.jd = torch.full((E + PAD,), **nan)
        self.choice = torch.full((N + PAD,), -7, dtype=torch.int32, device=DEV)
        self.cls = torch.full((N + PAD,), -7, dtype=torch.int32, device=DEV)
        self.has_cell = bool(model.cell_pairs)
        c = IK.constants(model)
        self.prm = _lib.IkParams(IK.K, c["lam2"], c["e_max"], c["dq_max"])

    def run(self, iters=True, stream=None):
        """solve -> reset_given -> probe(s) -> select; returns the numpy copies of what the candidates' rows hold"""
        lib, st = self.lib, torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        assert lib.naf_chain_ik_solve(self.h, p(self.targets), p(self.q_start), p(self.seeds), self.N, self.R, self.prm, p(self.q),
                                      p(self.residual), p(self.iters) if iters else None, st) == 0
        assert lib.naf_chain_env_reset_given(self.h, p(self.st), p(self.obs), self.E, p(self.q), p(self.scene), IK.ORAD, st) == 0
        assert lib.naf_chain_env_probe(self.h, p(self.st), p(self.probe), self.E, st) == 0
        if self.has_cell:
            assert lib.naf_chain_env_probe_cell(self.h, p(self.st), p(self.cell), self.E, st) == 0
        assert lib.naf_chain_ik_select(self.h, p(self.q), p(self.q_start), p(self.residual), p(self.probe),
                                       p(self.cell) if self.has_cell else None, self.N, self.R, IK.TOLERANCE, self.case.margin,
                                       p(self.choice), p(self.cls), p(self.jd), st) == 0
        torch.cuda.synchronize()
        E, N = self.E, self.N
        for t in (self.q, self.residual, self.probe, self.jd):
            assert torch.isnan(t[E:]).all()
        assert torch.isnan(self.iters[IK.K + 1]).all() and (self.choice[N:] == -7).all() and (self.cls[N:] == -7).all()
        cell = self.cell[:E].cpu().numpy() if self.has_cell else np.full(E, np.inf, np.float32)
        return dict(q=self.q[:E].cpu().numpy(), residual=self.residual[:E].cpu().numpy(), iters=self.iters[:IK.K + 1].cpu().numpy(),
                    probe=self.probe[:E].cpu().numpy(), cell=cell, jd=self.jd[:E].cpu().numpy(),
                    choice=self.choice[:N].cpu().numpy().astype(np.int64), cls=self.cls[:N].cpu().numpy().astype(np.int64))

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


CASES = [(name, N, R) for name in IK.ARMS for N, R in IK.COUNTS] + [("long32", 4, 4), ("slider4", 8, 4), ("iiwa_like7", 65, 1)]


@pytest.mark.parametrize("name,N,R", CASES)
def test_solve_and_select_against_the_rule(name, N, R):
    """One case through the C ABI, iters_out on. (1) Teacher-forced: every recorded update within chain_ik_common.STEP_BOUND (8 x the
    float32 restatement's measured single-step deviation, 1.5e-5 rad) of ik_step applied to the recorded pose before it, max-norm
    over the joints, every candidate and every k; the recorded start is the seed (the start pose for restart 0), the limits hold
    as float32 comparisons. (2) Soundness, every candidate: |residual_out - |g - ee_twin(q_out)|| <= 2 tol, and a query reported
    reachable has |g - ee_twin(chosen pose)| <= tolerance + 2 tol. (3) Completeness: every query for which the twin from the same
    seeds has a candidate at or below tolerance / 4 is reported reachable (at most 1 % of the queries lie between tolerance / 4 and
    tolerance and are left out); every query at 1.1 reach is reported unreachable. (4) choice, class and joint_distance equal
    select_goal_pose fed residual_out and the probes' outputs, bit for bit; with N R >= 64 each class ends at least 8 queries.
    (5) The probes at q_out within tol / 2 tol / 4 tol / 2 tol of the twin's end effector, clearance, self-clearance and workcell
    clearance; `free` agrees with the twin outside 8 tol of the margin (at most 1 % of the candidates inside). The PAD rows behind
    the candidates keep their poison."""
    case = IK.build_case(name, N, R)
    rig = IkRig(case)
    got = rig.run()
    rig.close()
    dev = IK.check_iterations(case, got["iters"])
    print(f"{name} N={N} R={R}: largest teacher-forced deviation {dev:.2e} (bound {IK.STEP_BOUND:.2e})")
    assert dev <= IK.STEP_BOUND, (dev, IK.STEP_BOUND)
    assert np.array_equal(bits(got["iters"][IK.K]), bits(got["q"]))
    IK.check_solution(case, got["q"], got["residual"], got["choice"], got["cls"], got["jd"], got["probe"], got["cell"])


def test_margin_moves_the_free_class():
    """The same case with a clearance margin no pose keeps (10 m): the poses, residuals and probes keep their bits, no query is
    free any more, every query that was reachable still is, and the selection equals select_goal_pose on the device's numbers."""
    from robotic_manipulator_rloa_amd.environment.kinematic import select_goal_pose
    base = IK.build_case("iiwa_like7", 64, 8)
    margin = 10.0
    case = IK.Case(base.name, base.N, base.R, base.q_start, base.targets, base.obstacles, base.seeds, base.want, margin=margin)
    rig = IkRig(case)
    got = rig.run(iters=False)
    rig.close()
    zero = IkRig(base)
    ref = zero.run(iters=False)
    zero.close()
    for k in ("q", "residual", "probe", "cell", "jd"):
        assert np.array_equal(bits(got[k]), bits(ref[k])), k
    assert np.sum(ref["cls"] == 0) >= IK.FLOOR and not np.any(got["cls"] == 0)
    assert np.array_equal(got["cls"] <= 1, ref["cls"] <= 1) and np.array_equal(got["cls"] == 2, ref["cls"] == 2)
    N, R = case.N, case.R
    choice, cls = select_goal_pose(got["residual"].reshape(N, R), got["jd"].reshape(N, R), got["probe"][:, 3].reshape(N, R),
                                   got["probe"][:, 4].reshape(N, R), got["cell"].reshape(N, R), np.float32(IK.TOLERANCE), np.float32(margin))
    assert np.array_equal(choice, got["choice"]) and np.array_equal(cls, got["cls"])


def test_placement_independence_through_the_c_abi():
    """Query 37 of the 64 x 8 case alone (N = 1) gives the bits it gives among the 64; launches on a side stream give the bits of the
    current stream's; a run without iters_out gives the bits of one with."""
    case = IK.build_case("iiwa_like7", 64, 8)
    rig = IkRig(case)
    all64 = rig.run()
    plain = rig.run(iters=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = rig.run(iters=False, stream=side.cuda_stream)
    rig.close()
    for k in ("q", "residual", "probe", "cell", "jd"):
        assert np.array_equal(bits(all64[k]), bits(plain[k])) and np.array_equal(bits(all64[k]), bits(on_side[k])), k
    for k in ("choice", "cls"):
        assert np.array_equal(all64[k], plain[k]) and np.array_equal(all64[k], on_side[k]), k
    i, R = 37, case.R
    one_case = IK.Case(case.name, 1, R, case.q_start[i:i + 1], case.targets[i:i + 1], case.obstacles[i:i + 1], case.seeds[i:i + 1],
                       case.want[i:i + 1])
    one = IkRig(one_case)
    alone = one.run()
    one.close()
    rows = slice(i * R, (i + 1) * R)
    for k in ("q", "residual", "probe", "cell", "jd"):
        assert np.array_equal(bits(all64[k][rows]), bits(alone[k])), k
    assert np.array_equal(bits(all64["iters"][:, rows]), bits(alone["iters"]))
    assert all64["choice"][i] == alone["choice"][0] and all64["cls"][i] == alone["cls"][0]


@pytest.mark.parametrize("name,N,R,chunk", [("iiwa_like7", 65, 1, 64), ("iiwa_like7", 17, 4, 64), ("long12", 5, 4, None)])
def test_goal_pose_solver_equals_the_c_abi_path(name, N, R, chunk):
    """chain_tools.GoalPoseSolver end to end, with the seeds it draws, against the C-ABI launches fed ik_seeds of the same seed: every
    field of GoalPoses bit for bit. Chunks of 64 candidates: N R = 65 is one more than a chunk, 17 x 4 a chunk of 16 queries and one
    of a single query."""
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    from robotic_manipulator_rloa_amd.environment.kinematic import gather_goal_poses
    base = IK.build_case(name, N, R)
    seeds = ik_seeds(base.model, N, R, seed=11).astype(np.float64)
    case = IK.Case(name, N, R, base.q_start, base.targets, base.obstacles, seeds, base.want)
    rig = IkRig(case)
    got = rig.run(iters=False)
    rig.close()
    A = case.model.A
    want = gather_goal_poses(got["choice"], got["cls"], got["q"].reshape(N, R, A), got["residual"].reshape(N, R),
                             got["probe"][:, 3].reshape(N, R), got["probe"][:, 4].reshape(N, R), got["cell"].reshape(N, R),
                             got["jd"].reshape(N, R), np.float32(IK.TOLERANCE))
    solver = GoalPoseSolver(case.model, IK.ORAD, chunk=chunk)
    out = solver.solve(case.q_start, case.targets, case.obstacles, restarts=R, iterations=IK.K, tolerance=IK.TOLERANCE, seed=11)
    for f, a, b in zip(want._fields, out, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert np.array_equal(out.reachable, out.residual <= np.float32(IK.TOLERANCE)) and out.joint_distance.dtype == np.float32


def test_framework_goal_poses_end_to_end(scratch_cwd):
    """solve_goal_poses on the device equals GoalPoseSolver on the same queries and needs no agent; reach_targets(goal_poses=True) on a
    freshly initialised agent returns that `goal`, every other field bit-equal to the call without the argument, path_ratio from
    the recorded paths; neither call changes the training-state digest; the host twin under the same rule agrees on reachability
    wherever it converges with room to spare."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    N, F = 48, 20
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.15, 0.15, (N, 3))
    targets[-1] = [0.0, 0.0, 2.0]                                      # out of reach
    bare = ManipulatorFramework()
    bare.initialize_kinematic_environment(**IIWA_RANGED)
    alone = bare.solve_goal_poses(targets, seed=3)                     # no agent
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    before = f.naf_agent.training_state_digest()
    goal = f.solve_goal_poses(targets, seed=3)
    assert f.naf_agent.training_state_digest() == before
    env = f.env
    start = np.tile(env.initial_joint_positions, (N, 1))
    direct = GoalPoseSolver(env.model, env.obstacle_radius).solve(start, targets, np.tile(env.obstacle_centre, (N, 1)), seed=3)
    for name, a, b, c in zip(goal._fields, goal, direct, alone):
        assert a.tobytes() == b.tobytes() == c.tobytes(), name
    assert goal.reachable[:-1].mean() >= 0.9 and not goal.reachable[-1] and np.all(goal.free <= goal.reachable)
    host = f.solve_goal_poses(targets, seed=3, on_device=False)
    sure = (host.residual <= IK.TOLERANCE / 4) | (host.residual > 4 * IK.TOLERANCE)
    assert sure.sum() >= N - 2 and np.array_equal(goal.reachable[sure], host.reachable[sure])
    plain = f.reach_targets(targets, frames=F)
    assert plain.goal is None and plain.path_ratio is None
    out = f.reach_targets(targets, frames=F, goal_poses=True)
    assert f.naf_agent.training_state_digest() == before
    default = f.solve_goal_poses(targets)
    for name, a, b in zip(default._fields, out.goal, default):
        assert a.tobytes() == b.tobytes(), name
    for name in ("outcome", "frames", "final_distance", "min_clearance", "min_self_clearance", "score", "joint_positions",
                 "start_distance", "start_clearance", "start_self_clearance", "min_cell_clearance", "start_cell_clearance"):
        a, b = getattr(out, name), getattr(plain, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    length = np.abs(np.diff(out.joint_positions.astype(np.float64), axis=1)).max(axis=2).sum(axis=1)
    ok = (out.outcome == "reached") & out.goal.free
    assert out.path_ratio.shape == (N,) and np.all(np.isnan(out.path_ratio[~ok]))
    assert np.array_equal(out.path_ratio[ok], length[ok] / out.goal.joint_distance[ok].astype(np.float64))


def test_off_means_off():
    """A fixed-seed DeviceEnvLoop stream (test_chain_rollout_gpu's: 100 steps, E = 64, iiwa_like7 with self-collision) hashes the
    same before and after goal poses have been solved for the same model in the same process."""
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    model, _ = C.arm("iiwa_like7", True)
    agent = _agent(model)
    before = _training_stream_digest(agent, model, False)
    rng = np.random.default_rng(3)
    N = 64
    out = GoalPoseSolver(model, IK.ORAD).solve(np.tile([j.init for j in model.joints], (N, 1)), rng.uniform(-0.5, 0.5, (N, 3)),
                                               rng.uniform(-0.5, 0.5, (N, 3)))
    assert out.reachable.any()
    assert _training_stream_digest(agent, model, False) == before

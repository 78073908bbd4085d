"""GPU (`-m gpu`): naf_chain_path_check (csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (path_pose,
check_joint_path) and against the existing launches at the same poses, through the C ABI; chain_tools.JointPathChecker,
ManipulatorFramework.plan_joint_paths and reach_targets(joint_paths=True) against that path; and that training launches are
untouched. tests/test_chain_path_cpu.py rehearses every case with a float32 restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_path_common as P
import chain_rollout_common as C
from test_chain_env_gpu import _agent
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment.kinematic import (check_joint_path, gather_joint_paths, path_chunks, path_leg_lengths,
                                                                path_vias)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 5                        # candidates behind the N C of the launch that no lane may write


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class PathRig:
    """The path launch of one case through the C ABI; out and poses_out have PAD poisoned candidates behind the launch's."""

    def __init__(self, case):
        from robotic_manipulator_rloa_amd import _lib
        self.lib = _lib.load()
        self.case = case
        model = case.model
        self.K, self.S, self.A = case.N * case.C, case.S, model.A
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.q_start, self.q_goal, self.obstacles = dev(case.q_start), dev(case.q_goal), dev(case.obstacles)
        self.vias = dev(case.vias.reshape(self.K, self.A))
        nan = dict(fill_value=float("nan"), device=DEV)
        self.out = torch.full((self.K + PAD, 8), **nan)
        self.poses = torch.full((self.K + PAD, self.S, self.A), **nan)
        self.has_cell = bool(model.cell_pairs)

    def run(self, poses=True, stream=None):
        """returns (out[N C, 8], poses[N C, S, A]) as numpy copies"""
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        case = self.case
        self.out.fill_(float("nan"))
        assert self.lib.naf_chain_path_check(self.h, p(self.q_start), p(self.q_goal), p(self.vias), p(self.obstacles), P.ORAD, case.N,
                                             case.C, case.S, case.margin, p(self.out), p(self.poses) if poses else None, st) == 0
        torch.cuda.synchronize()
        assert torch.isnan(self.out[self.K:]).all() and torch.isnan(self.poses[self.K:]).all()
        return self.out[:self.K].cpu().numpy(), self.poses[:self.K].cpu().numpy()

    def probes(self, poses):
        """(clearance - radius, self-clearance, workcell clearance)[N C, S] of reset_given -> probe -> probe_cell at poses[N C, S, A]"""
        lib, case, E = self.lib, self.case, self.K * self.S
        p = lambda t: t.data_ptr()      # noqa: E731
        q0 = torch.from_numpy(np.ascontiguousarray(poses.reshape(E, self.A))).to(DEV)
        ob = np.repeat(np.repeat(case.obstacles, case.C, axis=0), self.S, axis=0)
        scene = torch.from_numpy(np.concatenate([np.zeros((E, 3)), ob], axis=1).astype(np.float32)).to(DEV)
        st = torch.zeros(E, lib.naf_chain_env_state_floats(self.h), device=DEV)
        obs = torch.zeros(E, 2 * self.A + 9, device=DEV)
        probe, cell = torch.zeros(E, 5, device=DEV), torch.full((E,), float("inf"), device=DEV)
        s = torch.cuda.current_stream().cuda_stream
        assert lib.naf_chain_env_reset_given(self.h, p(st), p(obs), E, p(q0), p(scene), P.ORAD, s) == 0
        assert lib.naf_chain_env_probe(self.h, p(st), p(probe), E, s) == 0
        if self.has_cell:
            assert lib.naf_chain_env_probe_cell(self.h, p(st), p(cell), E, s) == 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(st[:, :self.A].cpu().numpy()), bits(poses.reshape(E, self.A)))      # no limit moved a pose
        probe = probe.cpu().numpy()
        return (probe[:, 3].reshape(self.K, self.S), probe[:, 4].reshape(self.K, self.S), cell.cpu().numpy().reshape(self.K, self.S))

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


CASES = [(name, N, Cn, S) for name in P.ARMS for N, Cn, S in P.COUNTS] + P.EXTRA


@pytest.mark.parametrize("name,N,Cn,S", CASES)
def test_path_check_against_the_rule_and_the_probes(name, N, Cn, S):
    """One case through the C ABI, poses_out on. Teacher-forced: every recorded pose within chain_path_common.POSE_BOUND (8 x the
    float32 restatement's measured deviation) of path_pose; the twin AT THE RECORDED POSES gives the three minima within 2 tol /
    4 tol / 2 tol, [5] bit for bit, [6] within an ulp, and [3], [4], [7] wherever no sample lies inside a band (at most 1 % do;
    chain_path_common.check_records). Parity: the three minima within 1 tol of the minima over the samples of what reset_given ->
    probe -> probe_cell return at the recorded poses, which the existing launches took bit for bit (asserted) — not to the bit: the
    same source expressions are contracted and packed differently in a kernel of another shape (NOTEBOOK §22). A run without
    poses_out gives the same bits, and the PAD rows keep their poison."""
    case = P.build_case(name, N, Cn, S)
    rig = PathRig(case)
    out, poses = rig.run()
    plain, _ = rig.run(poses=False)
    clear, self_clear, cell = rig.probes(poses)
    rig.close()
    assert np.array_equal(bits(out), bits(plain))
    P.check_records(case, out, poses)
    tol, exact = C.tol_of(case.model), []
    for k, per_sample in enumerate((clear, self_clear, cell)):
        got, want = out[:, k].astype(np.float64), per_sample.min(axis=1).astype(np.float64)
        both_inf = np.isposinf(got) & np.isposinf(want)
        err = float(np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want)).max())
        exact.append(np.array_equal(bits(out[:, k]), bits(per_sample.min(axis=1))))
        print(f"{name} N={N} C={Cn} S={S}: minimum {k} against the probes: {'bit-equal' if exact[-1] else f'{err:.2e}'} (tol {tol:.2e})")
        assert err <= tol, (k, err, tol)


def test_placement_independence_through_the_c_abi():
    """Candidate (8, 9) of the 16 x 16 case gives the same eight floats and the same poses alone at index 0 of a launch of one, deep
    inside the launch of 256, and as candidate 2 of 3 in a launch with another C; a launch on a side stream gives the current
    stream's bits."""
    case = P.build_case("iiwa_like7", 16, 16, 256)
    rig = PathRig(case)
    big, big_poses = rig.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side, _ = rig.run(stream=side.cuda_stream)
    rig.close()
    assert np.array_equal(bits(big), bits(on_side))
    n, c = 8, 9
    one = PathRig(case.sub(n, c))
    alone, alone_poses = one.run()
    one.close()
    assert np.array_equal(bits(big[n * 16 + c]), bits(alone[0])) and np.array_equal(bits(big_poses[n * 16 + c]), bits(alone_poses[0]))
    three = P.Case(case.name, 1, 3, case.S, case.q_start[n:n + 1], case.q_goal[n:n + 1], case.vias[n:n + 1, [0, 4, c]],
                   case.obstacles[n:n + 1], case.margin)
    rig3 = PathRig(three)
    out3, _ = rig3.run()
    rig3.close()
    assert np.array_equal(bits(out3[2]), bits(alone[0])) and np.array_equal(bits(out3[0]), bits(big[n * 16]))


@pytest.mark.parametrize("name,N,Cn,chunk", [("iiwa_like7", 5, 4, 2 * 4 * 64), ("long12", 3, 5, 5 * 64), ("slider4", 9, 16, None)])
def test_joint_path_checker_equals_the_c_abi_path_across_chunks(name, N, Cn, chunk):
    """chain_tools.JointPathChecker end to end, with the vias it draws, against the C-ABI launch fed path_vias of the same seed, and in
    chunks of two queries / one query against one chunk: every field of JointPaths bit for bit. resolution = 1 rad puts every chunk
    at S = 64, so that the chunks sample as the one launch does."""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    base = P.build_case(name, N, Cn, 64)
    vias = path_vias(base.model, base.q_start, base.q_goal, Cn, seed=11)
    assert path_chunks(path_leg_lengths(vias, base.q_start, base.q_goal), Cn, 1.0) == [(0, N, 64)]
    case = P.Case(name, N, Cn, 64, base.q_start, base.q_goal, vias.astype(np.float64), base.obstacles, base.margin)
    rig = PathRig(case)
    out, _ = rig.run(poses=False)
    rig.close()
    want = gather_joint_paths(out.reshape(N, Cn, 8), vias, base.q_start.astype(np.float32), base.q_goal.astype(np.float32), np.full(N, 64))
    kw = dict(candidates=Cn, resolution=1.0, margin=case.margin, seed=11)
    whole = JointPathChecker(case.model, P.ORAD).check(case.q_start, case.q_goal, case.obstacles, **kw)
    parts = JointPathChecker(case.model, P.ORAD, chunk=chunk).check(case.q_start, case.q_goal, case.obstacles, **kw)
    for f, a, b, c in zip(want._fields, whole, parts, want):
        assert a.shape == b.shape == c.shape and a.dtype == b.dtype == c.dtype, f
        assert a.tobytes() == b.tobytes() == c.tobytes(), f
    assert whole.length.dtype == np.float32 and np.all(whole.samples == 64)


def test_framework_joint_paths_end_to_end(scratch_cwd):
    """plan_joint_paths on the device against on_device=False with the same seeds: the same samples, vias and lengths, and the
    same outcome for every query none of whose samples lies inside a band (found with the twin); it needs no agent.
    reach_targets(joint_paths=True) on a freshly initialised agent returns `path` and `planned_ratio`, every rollout number bit-equal
    to the call without the argument; no call changes the training-state digest."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    N, F = 24, 20
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.15, 0.15, (N, 3))
    targets[-1] = [0.0, 0.0, 2.0]                                      # out of reach
    bare = ManipulatorFramework()
    bare.initialize_kinematic_environment(**IIWA_RANGED)
    alone = bare.plan_joint_paths(targets, candidates=8, seed=3)       # no agent
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    before = f.naf_agent.training_state_digest()
    dev = f.plan_joint_paths(targets, candidates=8, seed=3)
    assert f.naf_agent.training_state_digest() == before
    for name, a, b in zip(dev._fields, dev, alone):
        assert a.tobytes() == b.tobytes(), name
    assert dev.outcome[-1] == "goal" and np.isnan(dev.length[-1]) and dev.candidate[-1] == -1
    goal = f.solve_goal_poses(targets, seed=3)
    env = f.env
    # the host twin, from the DEVICE's goal poses (its own iteration's differ in the last bits): the same vias, samples and lengths
    ok = goal.reachable
    start = np.tile(env.initial_joint_positions, (N, 1))
    host = f.plan_joint_paths(goal_joint_positions=goal.joint_positions[ok], initial_joint_positions=start[ok], candidates=8, seed=3,
                              on_device=False)
    again = f.plan_joint_paths(goal_joint_positions=goal.joint_positions[ok], initial_joint_positions=start[ok], candidates=8, seed=3)
    assert np.array_equal(again.samples, host.samples) and np.array_equal(again.straight_length, host.straight_length.astype(np.float32))
    for name, a, b in zip(dev._fields, again, dev):
        assert np.array_equal(a, b[ok], equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b[ok]), name
    differ = np.nonzero(again.outcome != host.outcome)[0]
    tol = C.tol_of(env.model)
    obstacle = C.f32(np.tile(env.obstacle_centre if env.scene_ranges_on else env.obstacle_pos, (N, 1)))[ok]
    vias = path_vias(env.model, start[ok], goal.joint_positions[ok], 8, 3).astype(np.float64)
    for n in differ:                                                   # (few, if any: each must have a sample inside a band)
        S = int(host.samples[n])
        near = [check_joint_path(env, C.f32(start[ok][n]), vias[n], C.f32(goal.joint_positions[ok][n]), obstacle[n], S, margin=m)
                for m in (-4 * tol, 4 * tol)]
        assert not np.array_equal(near[0][:, [3, 4, 7]], near[1][:, [3, 4, 7]]), n
    same = again.outcome == host.outcome
    found = same & (again.candidate >= 0) & (again.candidate == host.candidate)
    assert np.array_equal(again.length[found], host.length[found].astype(np.float32))
    plain = f.reach_targets(targets, frames=F)
    assert plain.path is None and plain.planned_ratio is None
    out = f.reach_targets(targets, frames=F, joint_paths=True)
    assert f.naf_agent.training_state_digest() == before
    for name in ("outcome", "frames", "final_distance", "min_clearance", "min_self_clearance", "score", "joint_positions",
                 "start_distance", "start_clearance", "start_self_clearance", "min_cell_clearance", "start_cell_clearance"):
        a, b = getattr(out, name), getattr(plain, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    default = f.plan_joint_paths(targets)
    for name, a, b in zip(default._fields, out.path, default):
        assert a.tobytes() == b.tobytes(), name
    assert out.goal is not None and out.path_ratio is not None
    length = np.abs(np.diff(out.joint_positions.astype(np.float64), axis=1)).max(axis=2).sum(axis=1)
    good = (out.outcome == "reached") & (out.path.candidate >= 0)
    assert out.planned_ratio.shape == (N,) and np.all(np.isnan(out.planned_ratio[~good]))
    assert np.array_equal(out.planned_ratio[good], length[good] / out.path.length[good].astype(np.float64))


def test_off_means_off():
    """A fixed-seed DeviceEnvLoop stream (test_chain_rollout_gpu's: 100 steps, E = 64, iiwa_like7 with self-collision) hashes the
    same before and after joint paths have been checked for the same model in the same process."""
    from robotic_manipulator_rloa_amd.chain_tools import JointPathChecker
    model, twin = C.arm("iiwa_like7", True)
    agent = _agent(model)
    before = _training_stream_digest(agent, model, False)
    rng = np.random.default_rng(3)
    N = 32
    q = P.IK.free_poses(model, twin, rng, 2 * N)
    out = JointPathChecker(model, P.ORAD).check(q[:N], q[N:], rng.uniform(-0.5, 0.5, (N, 3)))
    assert (out.candidate >= 0).any()
    assert _training_stream_digest(agent, model, False) == before

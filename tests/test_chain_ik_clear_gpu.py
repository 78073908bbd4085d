"""GPU (`-m gpu`): naf_chain_ik_clear (csrc/chain_env.hip) against the float64 rule of environment/contact_push.py, through the C ABI
with poisoned PAD rows; chain_tools.GoalPoseSolver(avoid_contact=True) and the three framework methods against that path; that
without the argument every launch, buffer and field is what it was; and what the argument is for: fewer queries of
plan_joint_paths end 'goal'. tests/test_chain_ik_clear_cpu.py rehearses every case with a float32 stand-in and measures the bounds."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chain_ik_clear_common as CC
import chain_ik_common as IK
import chain_rollout_common as C
from test_chain_env_gpu import _agent
from test_chain_rollout_gpu import IIWA_RANGED, _training_stream_digest

from robotic_manipulator_rloa_amd.environment.kinematic import gather_goal_poses, ik_seeds, note_pushed, select_goal_pose

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 28                       # rows behind the N R candidates that no lane may write
K = CC.K


@pytest.fixture()
def scratch_cwd(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class ClearRig:
    """naf_chain_ik_clear on one case's candidates, then the existing reset_given -> probe(s) -> select, through the C ABI; every
    output has PAD poisoned rows behind the candidates'."""

    def __init__(self, case, margin=CC.MARGIN):
        from robotic_manipulator_rloa_amd import _lib
        self.lib = _lib.load()
        self.case, self.margin = case, margin
        model, N, R = case.model, case.N, case.R
        self.N, self.R, self.A, self.E = N, R, model.A, N * R
        blob = np.ascontiguousarray(model.pack())
        self.h = ctypes.c_void_p()
        assert self.lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(self.h)) == 0
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
        self.targets, self.obstacles, self.q_in = dev(case.targets), dev(case.obstacles), dev(case.q_in)
        self.q_start = dev(np.zeros((N, self.A)))
        self.scene = dev(np.repeat(np.concatenate([case.targets, case.obstacles], axis=1), R, axis=0))
        nan = dict(fill_value=float("nan"), device=DEV)
        E = self.E
        self.q, self.work = torch.full((E + PAD, self.A), **nan), torch.full((E + PAD, self.A), **nan)
        self.residual, self.clear = torch.full((E + PAD,), **nan), torch.full((E + PAD, 4), **nan)
        self.iters, self.rec = torch.full((K + 2, E, self.A), **nan), torch.full((K + 1, E, self.A + 2), **nan)
        self.st = torch.full((E + PAD, self.lib.naf_chain_env_state_floats(self.h)), **nan)
        self.obs = torch.full((E + PAD, 2 * self.A + 9), **nan)
        self.probe, self.cell, self.jd = torch.full((E + PAD, 5), **nan), torch.full((E + PAD,), **nan), torch.full((E + PAD,), **nan)
        self.choice = torch.full((N + PAD,), -7, dtype=torch.int32, device=DEV)
        self.cls = torch.full((N + PAD,), -7, dtype=torch.int32, device=DEV)
        self.has_cell = bool(model.cell_pairs)
        c = CC.constants(model)
        self.prm = _lib.IkParams(K, c["lam2"], c["e_max"], c["dq_max"])
        self.cp = _lib.IkClearParams(CC.SETTLE, CC.TOLERANCE, CC.GOAL, CC.PUSH_MAX, CC.ORAD)

    def probes(self, q, st):
        """the existing clearances and selection at the poses q (a device tensor [E + PAD][A]): (probe, cell, class per candidate)"""
        lib, p = self.lib, (lambda t: t.data_ptr())
        assert lib.naf_chain_env_reset_given(self.h, p(self.st), p(self.obs), self.E, p(q), p(self.scene), CC.ORAD, st) == 0
        assert lib.naf_chain_env_probe(self.h, p(self.st), p(self.probe), self.E, st) == 0
        if self.has_cell:
            assert lib.naf_chain_env_probe_cell(self.h, p(self.st), p(self.cell), self.E, st) == 0
        torch.cuda.synchronize()
        E = self.E
        cell = self.cell[:E].cpu().numpy() if self.has_cell else np.full(E, np.inf, np.float32)
        return self.probe[:E].cpu().numpy(), cell

    def run(self, record=True, stream=None):
        lib, st = self.lib, torch.cuda.current_stream().cuda_stream if stream is None else stream
        p = lambda t: t.data_ptr()      # noqa: E731
        E, N = self.E, self.N
        self.q[:E] = self.q_in                                     # the class of the input poses, by the existing launches
        probe_in, cell_in = self.probes(self.q, st)
        self.q[:E] = float("nan")
        assert lib.naf_chain_ik_clear(self.h, p(self.targets), p(self.obstacles), p(self.q_in), self.N, self.R, self.prm, self.cp,
                                      p(self.q), p(self.work), p(self.residual), p(self.clear), p(self.iters) if record else None,
                                      p(self.rec) if record else None, st) == 0
        probe, cell = self.probes(self.q, st)
        assert lib.naf_chain_ik_select(self.h, p(self.q), p(self.q_start), p(self.residual), p(self.probe),
                                       p(self.cell) if self.has_cell else None, self.N, self.R, CC.TOLERANCE, self.margin,
                                       p(self.choice), p(self.cls), p(self.jd), st) == 0
        torch.cuda.synchronize()
        for t in (self.q, self.work, self.residual, self.clear):
            assert torch.isnan(t[E:]).all()
        if record:
            assert torch.isnan(self.iters[K + 1]).all() and torch.isnan(self.rec[K]).all()
        assert (self.choice[N:] == -7).all() and (self.cls[N:] == -7).all()
        return dict(q=self.q[:E].cpu().numpy(), residual=self.residual[:E].cpu().numpy(), clear=self.clear[:E].cpu().numpy(),
                    iters=self.iters[:K + 1].cpu().numpy(), rec=self.rec[:K].cpu().numpy(), probe=probe, cell=cell,
                    probe_in=probe_in, cell_in=cell_in, jd=self.jd[:E].cpu().numpy(),
                    choice=self.choice[:N].cpu().numpy().astype(np.int64), cls=self.cls[:N].cpu().numpy().astype(np.int64))

    def close(self):
        torch.cuda.synchronize()
        assert self.lib.naf_chain_env_destroy(self.h) == 0


def device_classes(residual, probe, cell, margin=CC.MARGIN):
    """a candidate's class by the existing probes' float32 numbers, as naf_chain_ik_select forms it"""
    m = np.float32(margin)
    free = (probe[:, 3] >= m) & (probe[:, 4] >= m) & (cell >= m)
    return np.where(residual <= np.float32(CC.TOLERANCE), np.where(free, 0, 1), 2)


@pytest.mark.parametrize("name,N,R", CC.CASES)
def test_clear_against_the_rule(name, N, R):
    """One case through the C ABI, records on. (1) Teacher-forced: every recorded update of a refined candidate within STEP_BOUND
    (8 x the rehearsal's 7e-5) of ik_clear_step applied to the recorded pose before it, the recorded gamma and c within GAMMA_BOUND
    and CLEAR_BOUND (8 x 1.6e-5, 8 x 3e-7) of the twin's at that pose, the kind equal; left out, at most 1 % of the case's updates:
    those where the twin's least and second-least tests are closer than BAND = 8 x 3e-7. (2) No exclusions, every candidate: the
    returned pose's class by the existing probe + select numbers on the device is <= the input pose's; iterate index 0 means the
    pose's bits equal the input's; residual_out and clear_out[1] within 2 tol (4 tol on a self pair) of the twin at the returned
    pose; a returned pose with a residual to spare and clear_out[1] clear of the margin by BAND is free by the probes. (3)
    Completeness: every candidate the free-running twin frees with clearance >= margin + BAND and its trajectory's least-test
    gap above BAND throughout is free by the device's probes (at most 10 % of the twin-freed left out); the device's free count is
    >= the count before. The PAD rows keep their poison."""
    case = CC.build_case(name, N, R)
    rig = ClearRig(case)
    got = rig.run()
    rig.close()
    dev, share, live = CC.check_updates(case, got)
    print(f"{name} N={N} R={R}: {live} refined candidates; deviation of one update {dev[0]:.2e} (bound {CC.STEP_BOUND:.1e}), of gamma "
          f"{dev[1]:.2e} ({CC.GAMMA_BOUND:.1e}), of c {dev[2]:.2e} ({CC.CLEAR_BOUND:.1e}); {share:.4f} of the updates inside the band")
    assert dev[0] <= CC.STEP_BOUND and dev[1] <= CC.GAMMA_BOUND and dev[2] <= CC.CLEAR_BOUND, dev
    res_in = np.linalg.norm(case.g - case.twin.end_effector(case.q_in), axis=1).astype(np.float32)
    class_in = device_classes(res_in, got["probe_in"], got["cell_in"])
    class_out = device_classes(got["residual"], got["probe"], got["cell"])
    # (the input's residual is the twin's, rounded: a candidate within 2 tol of the tolerance may be of either class going in)
    near = np.abs(res_in - np.float32(CC.TOLERANCE)) <= 2 * C.tol_of(case.model)
    class_in = np.where(near & (class_in < 2), np.maximum(class_in, class_out), class_in)
    CC.check_returned(case, got, class_in, class_out)
    least = np.minimum(np.minimum(got["probe"][:, 3], got["probe"][:, 4]), got["cell"])
    tol = C.tol_of(case.model)
    assert np.all(np.abs(least - got["clear"][:, 1]) <= np.where(got["clear"][:, 3] == 1, 8 * tol, 4 * tol))
    free_out, free_in = class_out == 0, class_in == 0
    freed, left_out, freed_dev = CC.check_completeness(case, got, free_out)
    print(f"    twin-freed candidates {freed}, left out {left_out}, freed by the device {freed_dev}; free before {int(free_in.sum())}, "
          f"after {int(free_out.sum())}")
    assert free_out.sum() >= free_in.sum()
    # the selection on the refined numbers is the existing rule's, bit for bit
    want_choice, want_cls = select_goal_pose(got["residual"].reshape(N, R), got["jd"].reshape(N, R), got["probe"][:, 3].reshape(N, R),
                                             got["probe"][:, 4].reshape(N, R), got["cell"].reshape(N, R), np.float32(CC.TOLERANCE),
                                             np.float32(CC.MARGIN))
    assert np.array_equal(got["choice"], want_choice) and np.array_equal(got["cls"], want_cls)


def test_placement_independence_through_the_c_abi():
    """Query 37 of the 64 x 8 case alone (N = 1) gives the bits it gives among the 64 (chunk); the 65 x 1 case's candidate 64, the
    first lane of a second wave, gives the bits it gives alone in lane 0 (lane); a launch on a side stream and one without the
    records give the bits of the recorded launch on the current stream; and q_out may be q_in itself."""
    case = CC.build_case("iiwa_like7", 64, 8)
    rig = ClearRig(case)
    all64 = rig.run()
    plain = rig.run(record=False)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    on_side = rig.run(record=False, stream=side.cuda_stream)
    side.synchronize()
    # in place: q_out is q_in's buffer
    p = lambda t: t.data_ptr()      # noqa: E731
    buf = rig.q_in.clone()
    assert rig.lib.naf_chain_ik_clear(rig.h, p(rig.targets), p(rig.obstacles), p(buf), rig.N, rig.R, rig.prm, rig.cp, p(buf), p(rig.work),
                                      p(rig.residual), p(rig.clear), None, None, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    in_place = dict(q=buf.cpu().numpy(), residual=rig.residual[:rig.E].cpu().numpy(), clear=rig.clear[:rig.E].cpu().numpy())
    rig.close()
    for k in ("q", "residual", "clear"):
        assert np.array_equal(bits(all64[k]), bits(plain[k])) and np.array_equal(bits(all64[k]), bits(on_side[k])), k
        assert np.array_equal(bits(all64[k]), bits(in_place[k])), k
    for i, (big, R) in ((37, (case, 8)), (64, (CC.build_case("iiwa_like7", 65, 1), 1))):
        whole = all64 if big is case else None
        if whole is None:
            r = ClearRig(big)
            whole = r.run()
            r.close()
        rows = slice(i * R, (i + 1) * R)
        one_case = CC.Case(big.name, 1, R, big.targets[i:i + 1], big.obstacles[i:i + 1], big.q_in[rows])
        one = ClearRig(one_case)
        alone = one.run()
        one.close()
        for k in ("q", "residual", "clear"):
            assert np.array_equal(bits(whole[k][rows]), bits(alone[k])), (i, k)
        assert np.array_equal(bits(whole["iters"][:, rows]), bits(alone["iters"])) and np.array_equal(bits(whole["rec"][:, rows]), bits(alone["rec"]))


@pytest.mark.parametrize("name,N,R,chunk", [("iiwa_like7", 65, 1, 64), ("iiwa_like7", 17, 4, 64), ("long12", 5, 4, None)])
def test_goal_pose_solver_equals_the_c_abi_path(name, N, R, chunk):
    """chain_tools.GoalPoseSolver(avoid_contact=True) end to end against the C-ABI launches — solve, clear in place, reset_given,
    probe(s), select — fed ik_seeds of the same seed: every field of GoalPoses bit for bit, pushed and input_clearance too. Chunks of
    64 candidates: N R = 65 is one more than a chunk, 17 x 4 a chunk of 16 queries and one of a single query."""
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    model, twin = CC.arm(name)
    rng = np.random.default_rng(21)
    lo, hi = C.limits_of(model)
    q_goal = np.clip(np.array([j.init for j in model.joints]) + 0.5 * rng.normal(size=(N, model.A)), lo, hi)
    targets = C.f32(twin.end_effector(q_goal))
    q_start = C.f32(np.clip(q_goal + 0.3 * rng.normal(size=q_goal.shape), lo, hi))
    obstacles = C.f32(targets + 0.1 * rng.normal(size=(N, 3)))                 # near the end effector: many candidates lean on it
    seeds = ik_seeds(model, N, R, seed=11)
    lib, E, A = _lib.load(), N * R, model.A
    blob = np.ascontiguousarray(model.pack())
    h = ctypes.c_void_p()
    assert lib.naf_chain_env_create(blob.ctypes.data, int(blob.size), ctypes.byref(h)) == 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)      # noqa: E731
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    p = lambda t: t.data_ptr()      # noqa: E731
    t_, o_, s_, qs_ = dev(targets), dev(obstacles), dev(seeds.reshape(E, A)), dev(q_start)
    scene = dev(np.repeat(np.concatenate([targets, obstacles], axis=1), R, axis=0))
    q, work, res, clear, st = z(E, A), z(E, A), z(E), z(E, 4), z(E, lib.naf_chain_env_state_floats(h))
    obs, probe, cell, jd = z(E, 2 * A + 9), z(E, 5), torch.full((E,), float("inf"), device=DEV), z(E)
    choice, cls = torch.zeros(N, dtype=torch.int32, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
    c = CC.constants(model)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.naf_chain_ik_solve(h, p(t_), p(qs_), p(s_), N, R, _lib.IkParams(IK.K, c["lam2"], c["e_max"], c["dq_max"]), p(q), p(res), None,
                                  stream) == 0
    assert lib.naf_chain_ik_clear(h, p(t_), p(o_), p(q), N, R, _lib.IkParams(K, c["lam2"], c["e_max"], c["dq_max"]),
                                  _lib.IkClearParams(CC.SETTLE, CC.TOLERANCE, CC.GOAL, CC.PUSH_MAX, CC.ORAD), p(q), p(work), p(res), p(clear),
                                  None, None, stream) == 0
    assert lib.naf_chain_env_reset_given(h, p(st), p(obs), E, p(q), p(scene), CC.ORAD, stream) == 0
    assert lib.naf_chain_env_probe(h, p(st), p(probe), E, stream) == 0
    has_cell = bool(model.cell_pairs)
    if has_cell:
        assert lib.naf_chain_env_probe_cell(h, p(st), p(cell), E, stream) == 0
    assert lib.naf_chain_ik_select(h, p(q), p(qs_), p(res), p(probe), p(cell) if has_cell else None, N, R, CC.TOLERANCE, CC.MARGIN,
                                   p(choice), p(cls), p(jd), stream) == 0
    torch.cuda.synchronize()
    n = lambda t, *s: t.cpu().numpy().reshape(*s) if s else t.cpu().numpy()      # noqa: E731
    pr = n(probe, N, R, 5)
    want = note_pushed(gather_goal_poses(n(choice), n(cls), n(q, N, R, A), n(res, N, R), pr[:, :, 3], pr[:, :, 4], n(cell, N, R), n(jd, N, R),
                                         np.float32(CC.TOLERANCE)), n(clear, N, R, 4))
    assert lib.naf_chain_env_destroy(h) == 0
    solver = GoalPoseSolver(model, CC.ORAD, chunk=chunk)
    assert solver.q_work is None and solver.clear is None
    out = solver.solve(q_start, targets, obstacles, restarts=R, iterations=IK.K, tolerance=CC.TOLERANCE, seed=11, avoid_contact=True)
    for f, a, b in zip(want._fields, out, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f
    assert out.pushed.tobytes() == want.pushed.tobytes() and out.input_clearance.tobytes() == want.input_clearance.tobytes()
    assert solver.q_work is not None


def test_framework_methods_end_to_end(scratch_cwd):
    """solve_goal_poses(avoid_contact=True) on the device equals GoalPoseSolver on the same queries and needs no agent; it never
    loses a free query of the call without the argument; reach_targets(goal_poses=True, avoid_contact=True) returns that `goal` and
    every rollout field of the call without; plan_joint_paths(targets, avoid_contact=True) leads to those poses; none of the calls
    changes the training-state digest; the refusal with an orientation goal comes before any launch."""
    from chain_resume_worker import make_framework
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    N, F = 48, 20
    rng = np.random.default_rng(8)
    targets = np.array(IIWA_RANGED["target_position"]) + rng.uniform(-0.2, 0.2, (N, 3))
    bare = ManipulatorFramework()
    bare.initialize_kinematic_environment(**IIWA_RANGED)
    alone = bare.solve_goal_poses(targets, seed=3, avoid_contact=True)                    # no agent
    f = make_framework(IIWA_RANGED, checkpoint_frequency=64, save=False)
    before = f.naf_agent.training_state_digest()
    plain = f.solve_goal_poses(targets, seed=3)
    goal = f.solve_goal_poses(targets, seed=3, avoid_contact=True)
    env = f.env
    start = np.tile(env.initial_joint_positions, (N, 1))
    direct = GoalPoseSolver(env.model, env.obstacle_radius).solve(start, targets, np.tile(env.obstacle_centre, (N, 1)), seed=3,
                                                                  avoid_contact=True, clearance_goal=None, push_iterations=16)
    for name, a, b, c in zip(goal._fields, goal, direct, alone):
        assert a.tobytes() == b.tobytes() == c.tobytes(), name
    assert goal.pushed.tobytes() == direct.pushed.tobytes() and plain.pushed is None
    assert np.all(goal.free >= plain.free) and np.array_equal(goal.reachable, plain.reachable)
    with pytest.raises(InvalidEnvironmentParameter, match="position only"):
        f.solve_goal_poses(targets, avoid_contact=True, approach_directions=[0, 0, -1])
    base = f.reach_targets(targets, frames=F, goal_poses=True)
    out = f.reach_targets(targets, frames=F, goal_poses=True, avoid_contact=True)
    default = f.solve_goal_poses(targets, avoid_contact=True)
    for name, a, b in zip(default._fields, out.goal, default):
        assert a.tobytes() == b.tobytes(), name
    for name in ("outcome", "frames", "final_distance", "min_clearance", "min_self_clearance", "score", "joint_positions"):
        a, b = getattr(out, name), getattr(base, name)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
    paths = f.plan_joint_paths(targets, seed=3, avoid_contact=True)
    ok = goal.reachable
    assert np.array_equal(paths.goal[ok], goal.joint_positions[ok]) and np.array_equal(paths.outcome == "goal", ~ok | ~goal.free)
    assert f.naf_agent.training_state_digest() == before


def test_off_means_off():
    """Without avoid_contact: GoalPoseSolver allocates none of the step's buffers and its fields' bytes are those of a solver that
    has never run the step, before and after another solver of the same model has run it in this process; GoalPoses.pushed is None;
    and a fixed-seed DeviceEnvLoop stream (test_chain_rollout_gpu's) hashes the same before and after the step has run."""
    from robotic_manipulator_rloa_amd.chain_tools import GoalPoseSolver
    model, _ = C.arm("iiwa_like7", True)
    agent = _agent(model)
    before = _training_stream_digest(agent, model, False)
    rng = np.random.default_rng(3)
    N = 64
    q0, t = np.tile([j.init for j in model.joints], (N, 1)), rng.uniform(-0.5, 0.5, (N, 3))
    o = t + 0.1 * rng.normal(size=(N, 3))                 # (an obstacle beside every target: the twin pushes a third of the chosen poses)
    first = GoalPoseSolver(model, IK.ORAD)
    a = first.solve(q0, t, o)
    assert first.q_work is None and first.clear is None and first.obstacles is None and a.pushed is None and a.input_clearance is None
    pushed = GoalPoseSolver(model, IK.ORAD).solve(q0, t, o, avoid_contact=True)
    assert pushed.pushed.any() and np.all(pushed.free >= a.free)
    b = first.solve(q0, t, o)
    other = GoalPoseSolver(model, IK.ORAD)
    other.solve(q0, t, o, avoid_contact=True)
    c = other.solve(q0, t, o)                                                      # the same solver, after it has run the step
    for name, x, y, z in zip(a._fields, a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes(), name
    assert c.pushed is None
    assert _training_stream_digest(agent, model, False) == before


def test_fewer_queries_end_goal_on_the_boxed_cell(scratch_cwd):
    """What the argument is for. plan_joint_paths(targets, avoid_contact=True) on iiwa_like7 among its boxes, spheres and floor ends
    fewer queries 'goal' than the call without, loses none, and every query it newly answers has a goal pose the existing probes
    call free: solve_goal_poses().free of the same call, taken by reset_given + probe + probe_cell, and the path's own last sample."""
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    f = ManipulatorFramework()
    fixed = {k: v for k, v in IIWA_RANGED.items() if k != "target_range"}      # (the nominal scene: no target box for the cell to stay out of)
    f.initialize_kinematic_environment(**dict(fixed, consider_autocollision=True, floor_height=0.0,
                                              workcell_spheres=[(0.62, 0.45, 0.75, 0.1), (-0.4, -0.4, 0.5, 0.1)],
                                              workcell_boxes=[(0.58, -0.45, 0.19, 0.32, 0.2, 0.026, 0.0, 0.0, 0.3),
                                                              (-0.13, 0.64, 0.77, 0.26, 0.064, 0.19, 0.4, -0.3, 0.8),
                                                              (0.0, -0.58, 0.9, 0.0, 0.0, 0.38, 1.2, 0.2, 0.0, 0.05)]))
    rng = np.random.default_rng(5)
    n = 128      # targets just above the table top, just above the floor and around the shelf: the twin frees 3 + 5 + 3 queries more
    targets = np.concatenate([np.stack([rng.uniform(0.35, 0.75, n), rng.uniform(-0.6, -0.3, n), rng.uniform(0.26, 0.36, n)], 1),
                              np.stack([rng.uniform(0.3, 0.7, n), rng.uniform(-0.1, 0.5, n), rng.uniform(0.04, 0.12, n)], 1),
                              np.array([-0.13, 0.64, 0.77]) + rng.uniform(-0.3, 0.3, (n, 3))])
    N = len(targets)
    base = f.plan_joint_paths(targets, seed=2, candidates=4)
    out = f.plan_joint_paths(targets, seed=2, candidates=4, avoid_contact=True)
    goal = f.solve_goal_poses(targets, seed=2, avoid_contact=True)
    was, now = base.outcome == "goal", out.outcome == "goal"
    print(f"queries ending 'goal': {int(was.sum())} without, {int(now.sum())} with avoid_contact, of {N}")
    assert now.sum() < was.sum() and not np.any(now & ~was)
    new = was & ~now
    assert np.all(goal.free[new]) and np.all(goal.pushed[new])
    assert np.all(np.minimum(np.minimum(goal.clearance, goal.self_clearance), goal.cell_clearance)[new] >= 0.0)

"""CPU: the float64 rule of planned joint paths as demonstrations (environment/kinematic.py: demonstration_plan,
demonstration_rows_host), the rehearsal of every GPU case of tests/test_chain_demo_gpu.py with a float32 restatement in the kernel's
place (chain_demo_common), keep / drop and the masks, and the host plumbing: header, symbol, ABI, argument errors, the façade on the
host twin and every refusal's message."""
import os
import re
import types

import numpy as np
import pytest

import chain_box_common as BX
import chain_demo_common as D
import chain_ik_common as IK
import chain_rollout_common as C
from conftest import ROOT
from test_chain_path_cpu import framework

from robotic_manipulator_rloa_amd.environment.kinematic import (DEMO_MAX_TICKS, Demonstrations, demo_actions, demo_row_layout,
                                                                demonstration_plan, demonstration_rows_host, joint_distance32,
                                                                path_vias)
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT


# ---- the plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", [1.0, 0.5, 0.13])
def test_plan_tick_counts_actions_and_the_straight_halves(speed):
    """n_k = max(1, ceil(L_k / (speed DT))) from joint_distance32, up to the one tick more that keeps the rounded action inside
    the speed; n_k DT a_k is the leg within float32 rounding; |a|_inf <= speed; a straight path (path_vias' candidate 0) is two
    collinear halves; a zero-length leg is one tick at action 0."""
    model, twin = D.arm("iiwa_like7")
    rng = np.random.default_rng(5)
    N = 40
    q = IK.free_poses(model, twin, rng, 2 * N)
    a, b = q[:N], q[N:]
    vias = path_vias(model, a, b, 3, seed=1).astype(np.float64)
    for c in range(3):
        via = vias[:, c].copy()
        via[0] = a[0]                                          # a zero-length first leg
        plan = demonstration_plan(a, via, b, speed, 400)
        assert plan.n_ticks.dtype == np.int32 and plan.leg_actions.dtype == np.float32 and plan.q_start.dtype == np.float32
        for k, (lo, hi) in enumerate(((a, via), (via, b))):
            L = joint_distance32(hi, lo).astype(np.float64)
            n = np.maximum(1, np.ceil(L / (speed * DT)))
            assert np.all((plan.n_ticks[:, k] == n) | (plan.n_ticks[:, k] == n + 1))
            assert np.mean(plan.n_ticks[:, k] == n) > 0.9
            moved = plan.n_ticks[:, k, None] * DT * plan.leg_actions[:, k].astype(np.float64)
            assert np.abs(moved - (C.f32(hi) - C.f32(lo))).max() <= 4e-7 * max(1.0, float(np.abs(hi - lo).max()))
        assert np.abs(plan.leg_actions).max() <= np.float32(speed)
        assert plan.n_ticks[0, 0] == 1 and np.all(plan.leg_actions[0, 0] == 0.0)
        assert np.array_equal(plan.rows, np.minimum(plan.n_ticks.sum(axis=1), 400))
        if c == 0:                                             # the straight line: the halves are collinear and equally long
            a1, a2 = plan.leg_actions[1:, 0].astype(np.float64), plan.leg_actions[1:, 1].astype(np.float64)
            assert np.abs(a1 - a2).max() <= 2e-2 * speed       # (the tick counts of the halves differ by at most one)
            assert np.abs(plan.n_ticks[1:, 0] - plan.n_ticks[1:, 1]).max() <= 1
    for bad in (0.0, -1.0, 1.5, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="speed"):
            demonstration_plan(a, vias[:, 0], b, bad, 400)
    for bad in (0, DEMO_MAX_TICKS + 1, 2.0, True):
        with pytest.raises(ValueError, match="frames"):
            demonstration_plan(a, vias[:, 0], b, 1.0, bad)


# ---- the twin against trace ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar3", "iiwa_like7"])
def test_the_twin_is_trace_under_the_plans_actions(name):
    """demonstration_rows_host against KinematicEnvironment.trace and step(), query by query: the poses are trace's, every row is
    what step() returns from the pose before (state, reward, done, velocities), the count and the code are trace's cut at T_n."""
    case = D.build_case(name, 3, 130)
    twin, plan, T = case.twin, case.plan, case.T_cap
    demos, rec, rows, poses = case.host()
    A = case.model.A
    S, off_s2, off_d, rf = demo_row_layout(A)
    for n in range(case.N):
        Tn = int(plan.rows[n])
        act = demo_actions(plan, Tn)[n]
        tr = twin.trace(plan.q_start[n].astype(np.float64), act, case.targets[n], case.obstacles[n], Tn)
        valid = int(tr.frames)
        assert rec[n, 0] == valid and np.array_equal(poses[n, :valid + 1], tr.joint_positions[:valid + 1])
        assert rec[n, 1] == (int(tr.code) if tr.code != 0 else (0 if Tn < plan.n_ticks[n].sum() else 5))
        assert rec[n, 2] == tr.final_distance and rec[n, 3] == tr.min_clearance and rec[n, 6] == plan.n_ticks[n].sum()
        assert np.all(np.isnan(rows[n, valid:]))
        # step() from the recorded pose: the row
        twin.target_pos, twin.obstacle_pos = case.targets[n].copy(), case.obstacles[n].copy()
        twin.q, twin.qd = poses[n, 0].copy(), np.zeros(A)
        for t in range(valid):
            before = twin.get_state()
            state, reward, done = twin.step(act[t])
            row = rows[n, t]
            assert np.array_equal(row[:S], before) and np.array_equal(row[S:S + A], act[t]) and np.array_equal(row[off_s2:off_s2 + S], state)
            assert row[S + A] == reward and row[off_d] == done and np.all(row[off_d + 1:] == 0.0) and np.all(row[S + A + 1:off_s2] == 0.0)
        assert done == (tr.code != 0)
    assert demos.rows.dtype == np.float32 and demos.rows.shape == (demos.rows_total, rf)


# ---- the rehearsal ---------------------------------------------------------------------------------------------------------------
REHEARSED = [(name, N, T) for name in D.ARMS for N, T in D.COUNTS] + D.EXTRA
MEASURED = {}


@pytest.mark.parametrize("name,N,T_cap", REHEARSED)
def test_rehearsal(name, N, T_cap):
    """Every GPU case with the float32 restatement in the kernel's place: the case builds (every demonstration ends as its role
    wants and the twin alone keeps every tick outside the bands), the roles are what chain_demo_common says, and the restatement's
    rows, records and poses pass every check the kernel's will; the pose deviation and the band share are measured."""
    case = D.build_case(name, N, T_cap)
    lanes = D.lanes_of(case.model)
    _, rec, _, _ = case.host()
    ticks = case.plan.n_ticks
    for n in range(N):
        role = n % 4
        assert rec[n, 1] == D.WANT[role]
        if role == 0:
            assert rec[n, 0] < rec[n, 6] and np.array_equal(case.q_start[n], case.vias[n]) and ticks[n, 0] == 1
        if role == 1:
            assert ticks[n, 0] % lanes != 0 and rec[n, 0] >= 2
        if role == 2:
            assert ticks[n, 0] % lanes == 0 and ticks[n].sum() > T_cap and rec[n, 0] == T_cap
        if role == 3:
            limits = np.stack(case.twin.joint_limits()).astype(np.float32)
            limited = any(j.limited for j in case.model.joints)
            assert not limited or np.any(case.q_goal[n].astype(np.float32) == limits)
    dev, inside, total = D.check_rows(case, *D.rows32(case))
    MEASURED[(name, N, T_cap)] = dev
    assert inside <= D.CAP * total


def test_the_measured_deviation_is_the_constant():
    """POSE_DEVIATION is the rehearsal's largest measured deviation rounded up (by no more than a quarter), and the bound 8 x it"""
    if len(MEASURED) < len(REHEARSED):
        for args in REHEARSED:
            case = D.build_case(*args)
            MEASURED[args] = D.check_rows(case, *D.rows32(case))[0]
    worst = max(MEASURED.values())
    print({k: f"{v:.2e}" for k, v in MEASURED.items()})
    assert worst <= D.POSE_DEVIATION <= 1.25 * worst, (worst, D.POSE_DEVIATION)
    assert D.POSE_BOUND == 8 * D.POSE_DEVIATION


# ---- keep / drop and the masks -----------------------------------------------------------------------------------------------------
def test_keep_drop_and_the_masks():
    """Demonstrations that end 'reached', 'frames' or 'end' are kept, one that touches anything is dropped whole unless
    keep_contact; a query without a path is 'none' with no rows; the kept rows are in query order, then tick order."""
    case = D.build_case("iiwa_like7", 16, 256)
    twin, plan = case.twin, case.plan
    demos, rec, rows, _ = case.host()
    assert set(demos.outcome) == {"reached", "obstacle", "frames", "end"}
    assert np.array_equal(demos.kept, demos.outcome != "obstacle") and demos.rows_total == int(demos.frames[demos.kept].sum())
    want = np.concatenate([rows[n, :int(rec[n, 0])] for n in range(case.N) if demos.kept[n]]).astype(np.float32)
    assert np.array_equal(demos.rows, want)
    sub = case.take(np.arange(4))
    has = np.array([True, True, False, True])
    kw = dict(frames=sub.T_cap, has_path=has)
    with_contact = demonstration_rows_host(twin, sub.plan, sub.targets, sub.obstacles, keep_contact=True, **kw)
    without = demonstration_rows_host(twin, sub.plan, sub.targets, sub.obstacles, **kw)
    assert list(with_contact.outcome) == ["reached", "obstacle", "none", "end"] and list(with_contact.kept) == [True, True, False, True]
    assert list(without.kept) == [True, False, False, True] and without.frames[2] == 0 and without.planned_ticks[2] == 0
    assert np.isnan(without.final_distance[2]) and np.isnan(without.min_clearance[2])
    assert with_contact.rows_total == without.rows_total + int(rec[1, 0]) == len(with_contact.rows)
    assert without.action_size == case.model.A and isinstance(without, Demonstrations)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def test_header_symbol_abi_and_argument_errors():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40
    assert re.search(r"^#define NAF_CHAIN_DEMO_FLOATS 8$", text, re.M) and re.search(r"^#define NAF_CHAIN_DEMO_MAX_TICKS 1024$", text, re.M)
    name = "naf_chain_demo_rows"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 14
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40
    # argument errors are host code and launch nothing: the fake handle is a zeroed buffer, read (A = 0) only by the row-width check
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    rf0 = lib.naf_replay_row_floats(9, 0)
    call = lambda h=p, q=p, a=p, n=p, t=p, o=p, rad=0.06, N=1, T=64, rows=p, rf=rf0, rec=p: lib.naf_chain_demo_rows(   # noqa: E731
        h, q, a, n, t, o, rad, N, T, rows, rf, rec, None, None)
    for kw in (dict(h=None), dict(q=None), dict(a=None), dict(n=None), dict(t=None), dict(o=None), dict(rows=None), dict(rec=None),
               dict(N=0), dict(N=-3), dict(T=0), dict(T=1025), dict(T=-64), dict(rf=rf0 + 1), dict(rf=0), dict(rad=float("nan")),
               dict(rad=float("inf")), dict(rad=-0.01)):
        assert call(**kw) == -1, kw


def stub_agent(A=7, buffer_size=1000, world_size=1):
    """an object with what NAFAgent.add_demonstrations touches, its replay ring a list"""
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    S, _, _, rf = demo_row_layout(A)
    added = []
    memory = types.SimpleNamespace(A=A, S=S, row_floats=rf, buffer_size=buffer_size, device="cpu", flush=lambda: None,
                                   add_rows_device=lambda rows, n: added.append(rows[:n].numpy().copy()))
    agent = types.SimpleNamespace(world_size=world_size, memory=memory, state_size=S, action_size=A, added=added)
    agent.add_demonstrations = types.MethodType(NAFAgent.add_demonstrations, agent)
    agent._demonstration_refusals = types.MethodType(NAFAgent._demonstration_refusals, agent)
    return agent


def test_demonstrate_joint_paths_on_the_host_and_every_refusal():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized,
                                                               InvalidEnvironmentParameter, InvalidNAFAgentParameter)
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.demonstrate_joint_paths(None)
    f.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="PyBullet and the synthetic stand-in have no chain model to drive"):
        f.demonstrate_joint_paths(None)
    synthetic = f
    f = framework(workcell_boxes=BX.boxes_of("iiwa_like7"))
    twin = f.env
    rng = np.random.default_rng(2)
    goals = IK.free_poses(twin.model, twin, rng, 5)
    goals = twin.initial_joint_positions + 0.25 * (goals - twin.initial_joint_positions)      # short paths: the twin is slow
    targets = np.concatenate([twin.end_effector(goals[:4]), [[0.0, 0.0, 1.1 * twin.model.reach]]])
    paths = f.plan_joint_paths(targets, candidates=4, resolution=0.05, seed=5, on_device=False)
    assert paths.candidate[4] == -1 and (paths.candidate[:4] >= 0).all()
    demos = f.demonstrate_joint_paths(paths, frames=300, on_device=False)                      # needs no agent
    assert isinstance(demos, Demonstrations) and isinstance(demos.rows, np.ndarray) and demos.rows.dtype == np.float32
    assert demos.outcome[4] == "none" and not demos.kept[4] and demos.frames[4] == 0
    plan = demonstration_plan(paths.start[:4], paths.via[:4], paths.goal[:4], 1.0, 300)
    want = demonstration_rows_host(twin, plan, twin.end_effector(C.f32(paths.goal[:4])), np.tile(twin.obstacle_pos, (4, 1)), 300)
    assert np.array_equal(demos.rows, want.rows) and list(demos.outcome[:4]) == list(want.outcome)
    assert np.array_equal(demos.planned_ticks[:4], plan.n_ticks.sum(axis=1)) and demos.rows_total == len(demos.rows)
    # targets=None is the end effector of the goal pose: a path that arrives reaches it, before its last tick (0.05 short of it)
    assert np.all(demos.outcome[:4][demos.kept[:4]] == "reached") and demos.kept[:4].any()
    assert np.all(demos.frames[:4][demos.kept[:4]] < demos.planned_ticks[:4][demos.kept[:4]])
    slow = f.demonstrate_joint_paths(paths, speed=0.5, frames=300, on_device=False)
    assert np.all(slow.planned_ticks[:4] >= 2 * demos.planned_ticks[:4] - 2)
    given = f.demonstrate_joint_paths(paths, targets=targets, obstacles=[2.0, 2.0, 2.0], frames=300, on_device=False)
    assert given.outcome[4] == "none" and len(given.outcome) == 5
    for args, match in ((dict(paths=None), "JointPaths"), (dict(paths=paths._replace(start=None)), "JointPaths"),
                        (dict(speed=0.0), "speed"), (dict(speed=1.01), "speed"), (dict(speed=float("nan")), "speed"),
                        (dict(frames=0), "frames"), (dict(frames=1025), "frames"), (dict(frames=10.0), "frames"),
                        (dict(targets=np.zeros((5, 2))), "targets"), (dict(targets=np.zeros((3, 3))), "number of paths"),
                        (dict(targets=np.full((5, 3), np.nan)), "not finite"), (dict(obstacles=np.zeros((2, 3))), "obstacles")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.demonstrate_joint_paths(**{"paths": paths, "on_device": False, **args})
    # ---- the ring: add_demonstrations on a stub agent whose ring is a list
    agent = stub_agent()
    f.naf_agent = agent
    stats = f.add_demonstrations(demos)
    assert stats == dict(demonstration_rows=demos.rows_total, demonstrations_kept=int(demos.kept.sum()),
                         demonstrations_dropped_contact=int(np.sum(np.isin(demos.outcome, ("obstacle", "self", "workcell")) & ~demos.kept)))
    assert len(agent.added) == 1 and np.array_equal(agent.added[0], demos.rows)
    with pytest.raises(ValueError, match="more than the replay buffer holds"):
        stub_agent(buffer_size=demos.rows_total - 1).add_demonstrations(demos)
    with pytest.raises(ValueError, match=r"a row is 32 floats wide, the agent's replay ring holds rows of 64"):
        agent.add_demonstrations(demos._replace(rows=demos.rows[:, :32]))
    with pytest.raises(ValueError, match="an arm of 6 joints, the agent's has 7"):
        agent.add_demonstrations(demos._replace(action_size=6))
    with pytest.raises(ValueError, match="rows_total"):
        agent.add_demonstrations(demos._replace(rows_total=demos.rows_total + 1))
    with pytest.raises(ValueError, match="data-parallel"):
        stub_agent(world_size=2).add_demonstrations(demos)
    with pytest.raises(InvalidNAFAgentParameter, match="demonstrate_joint_paths"):
        f.add_demonstrations(demos.rows)
    # ---- run_training / run_vectorized: every refusal names its reason
    for kw, match in ((dict(chain=None, resume=False, hs=None, E=16), "the stand-in, PyBullet"),
                      (dict(chain=twin.model, resume=False, hs=None, E=1), "n_envs > 1"),
                      (dict(chain=twin.model, resume=True, hs=None, E=16), "already in the training state"),
                      (dict(chain=twin.model, resume=False, hs=(0.5, 10), E=16), "ring filled by this run alone")):
        with pytest.raises(ValueError, match=match):
            agent._demonstration_refusals(**kw)
    with pytest.raises(ValueError, match="data-parallel"):
        stub_agent(world_size=2)._demonstration_refusals(chain=twin.model, resume=False, hs=None, E=16)
    agent._demonstration_refusals(chain=twin.model, resume=False, hs=None, E=16)
    with pytest.raises(ValueError, match="n_envs > 1"):
        f.run_training(2, 10, n_envs=1, demonstrations=demos)
    with pytest.raises(ValueError, match="n_envs > 1"):
        f.run_training(2, 10, demonstrations=demos)
    with pytest.raises(InvalidNAFAgentParameter, match="demonstrate_joint_paths"):
        f.run_training(2, 10, n_envs=16, demonstrations=demos.rows)
    with pytest.raises(ValueError, match="already in the training state"):
        f.resume_training(1, 2, 10, n_envs=16, demonstrations=demos)
    synthetic.naf_agent = agent
    with pytest.raises(ValueError, match="synthetic stand-in and PyBullet have no planned joint paths"):
        synthetic.run_training(2, 10, n_envs=16, demonstrations=demos)

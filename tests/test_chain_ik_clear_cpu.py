"""CPU (`-m "not gpu"`): the rule of goal poses pushed out of contact (environment/contact_push.py: least_test, clearance_gradient,
ik_clear_step, refine_goal_poses) against the twin's existing clearances and references of its own making; the rehearsal of every
GPU case of tests/test_chain_ik_clear_gpu.py with a float32 stand-in in the kernel's place, which measures the bounds the GPU tests
use; the plumbing of naf_chain_ik_clear; and the façade's arguments and refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

import chain_ik_clear_common as CC
import chain_ik_common as IK
import chain_rollout_common as C
from test_chain_env_cpu import random_q
from test_chain_ik_cpu import framework

from robotic_manipulator_rloa_amd.environment import contact_push as CP
from robotic_manipulator_rloa_amd.environment.kinematic import (goal_poses_host, segment_box_distance, segment_point_distance2,
                                                                segment_segment_distance2)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAF_ERR_ARG = -1


def poses_and_obstacles(name, n, seed=0):
    model, twin = CC.arm(name)
    rng = np.random.default_rng(500 + seed)
    q = np.stack([random_q(model, rng) for _ in range(n)])
    return model, twin, q, 0.5 * model.reach * rng.normal(size=(n, 3))


def least_of_existing(twin, q, ob):
    zero = np.zeros(len(q))
    return np.minimum(np.minimum(twin.clearance(q, ob) - twin.obstacle_radius, twin.self_clearance(q) + zero), twin.cell_clearance(q) + zero)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_witnesses_attain_the_existing_distances():
    """For every kind, |x - nearest point| equals the existing distance function's distance: point, pair (crossing, parallel and
    zero-length segments among them) and box (rounded, zero-extent, a segment through the box)."""
    rng = np.random.default_rng(1)
    a, b, c, d = (rng.normal(size=(400, 3)) for _ in range(4))
    b[:20] = a[:20]                                       # zero-length
    d[20:40] = c[20:40] + (b - a)[20:40]                  # parallel
    x, dist = CP.segment_point_witness(a, b, c)
    assert np.abs(dist - np.sqrt(segment_point_distance2(a, b, c))).max() <= 1e-12
    t = np.sum((x - a) * (b - a), axis=1) / np.maximum(np.sum((b - a) ** 2, axis=1), 1e-300)
    assert np.all((t >= -1e-12) & (t <= 1 + 1e-12))
    x, y, dist = CP.segment_segment_witness(a, b, c, d)
    assert np.abs(dist - np.sqrt(segment_segment_distance2(a, b, c, d))).max() <= 1e-12
    assert np.abs(np.sqrt(segment_point_distance2(a, b, x))).max() <= 1e-12 and np.abs(np.sqrt(segment_point_distance2(c, d, y))).max() <= 1e-12
    half = np.abs(rng.normal(size=(400, 3))) * 0.3
    half[:50, :2] = 0.0                                   # the "capsule" box
    tb, near, dist = CP.segment_box_witness(a * 0.5, b * 0.5, half)
    assert np.abs(dist - segment_box_distance(a * 0.5, b * 0.5, half)).max() <= 1e-12
    assert np.all(np.abs(near) <= half + 1e-15) and np.all((tb >= 0) & (tb <= 1)) and np.sum(dist == 0.0) >= 10


@pytest.mark.parametrize("name", CC.ARMS)
def test_least_test_is_the_least_of_the_existing_clearances(name):
    """c equals min(clearance - obstacle radius, self_clearance, cell_clearance) of the twin; the witness lies on the capsule it
    names and, for an obstacle test, |x - centre| - radii is that clearance; `second` is never below c."""
    model, twin, q, ob = poses_and_obstacles(name, 300)
    lt = CP.least_test(twin, q, ob)
    assert np.abs(lt.c - least_of_existing(twin, q, ob)).max() <= 1e-12
    assert np.all(lt.second >= lt.c) and np.all((lt.kind >= 0) & (lt.kind <= 2))
    obst = lt.test == 0
    r = np.array([s.radius for s in model.segments])
    frames = np.array([s.frame for s in model.segments])
    d = np.linalg.norm(lt.x - ob, axis=1)[obst]
    # the capsule of the witness: the one of its frame whose axis holds x
    w = CP.clear_walk(twin, q)
    on = np.stack([np.sqrt(segment_point_distance2(w.seg_a[:, s], w.seg_b[:, s], lt.x)) for s in range(len(r))], axis=1)
    on = np.where(frames[None, :] == lt.frame[:, None], on, np.inf)
    assert on.min(axis=1).max() <= 1e-12
    assert np.abs(d - r[on.argmin(axis=1)][obst] - twin.obstacle_radius - lt.c[obst]).max() <= 1e-12
    assert np.all(np.abs(np.linalg.norm(lt.n, axis=1) - 1.0)[lt.c > -0.02] <= 1e-9)


@pytest.mark.parametrize("name", CC.ARMS)
def test_gradient_against_central_differences(name):
    """gamma against central differences (step 1e-6) of the twin's existing clearance / self_clearance / cell_clearance, at poses at
    least GRADIENT_GAP = 1 mm from a kink (two least tests equal) and with a direction (an axis inside a box has none): the
    envelope derivative of the least clearance, within 1e-7 — the differences' own truncation. At least 50 poses an arm."""
    model, twin, q, ob = poses_and_obstacles(name, 300, seed=1)
    gamma, lt = CP.clearance_gradient(twin, q, ob)
    h = 1e-6
    num = np.zeros_like(gamma)
    for m in range(model.A):
        d = np.zeros(model.A)
        d[m] = h
        num[:, m] = (least_of_existing(twin, q + d, ob) - least_of_existing(twin, q - d, ob)) / (2 * h)
    ok = (lt.second - lt.c >= CC.GRADIENT_GAP) & np.any(lt.n != 0.0, axis=1)
    assert ok.sum() >= 50, int(ok.sum())
    assert np.abs(gamma - num)[ok].max() <= 1e-7, np.abs(gamma - num)[ok].max()
    # joints behind the witness frame (and, for a pair, before both frames' common part) do not move the test
    m = np.arange(model.A)
    still = (m[None, :] >= np.maximum(lt.frame, lt.frame2)[:, None])
    assert np.all(gamma[still] == 0.0)


@pytest.mark.parametrize("name", CC.ARMS)
def test_the_push_is_projected_off_the_task(name):
    """J h ~ 0 relative to lam: h = gamma - J^T (J J^T + lam^2 I)^-1 J gamma leaves |J h| <= lam^2 |z| with z = M^-1 J gamma, exactly;
    joints behind the end-effector frame keep gamma; and without a push (c >= clearance_goal, or the settling updates) the update
    is ik_step's."""
    model, twin, q, ob = poses_and_obstacles(name, 200, seed=2)
    kw = CC.twin_kw(model)
    g = twin.end_effector(q) + 1e-4
    w = CP.clear_walk(twin, q)
    lt = CP.least_test(twin, q, ob, w)
    gamma = CP.clearance_gradient_of(model, w.axes, w.points, lt)
    _, h = CP.clear_update_of(model, q, g, w.ee, w.axes, w.points, gamma, lt.c, np.ones(len(q), bool), kw["lam"] ** 2, kw["e_max"],
                              kw["dq_max"], CC.GOAL, CC.PUSH_MAX)
    _, J = twin.jacobian(q)
    Jh = np.einsum("nij,nj->ni", J, h)
    Jg = np.einsum("nij,nj->ni", J, gamma)
    M = J @ np.swapaxes(J, -1, -2) + kw["lam"] ** 2 * np.eye(3)
    z = np.linalg.solve(M, Jg[..., None])[..., 0]
    assert np.abs(Jh - kw["lam"] ** 2 * z).max() <= 1e-12
    assert np.all(np.linalg.norm(Jh, axis=1) <= kw["lam"] * np.linalg.norm(gamma, axis=1) + 1e-12)
    assert np.array_equal(h[:, model.ee_frame:], gamma[:, model.ee_frame:])
    step = twin.ik_step(q, g, kw["lam"], kw["e_max"], kw["dq_max"])
    settled, _, _, _ = CP.ik_clear_step(twin, q, g, ob, CC.K - CC.SETTLE, **kw)
    assert np.abs(settled - step).max() <= 1e-13
    pushed, _, lt, _ = CP.ik_clear_step(twin, q, g, ob, 0, **kw)
    kept = lt.c >= CC.GOAL
    assert kept.any() and np.abs(pushed - step)[kept].max() <= 1e-13 and np.abs(pushed - step).max() <= CC.PUSH_MAX + 1e-12


@pytest.mark.parametrize("name,N,R", CC.CASES)
def test_refinement_is_monotone_and_returns_early_inputs_bit_for_bit(name, N, R):
    """The twin on every case: the returned pose is never worse than the input (min(c, goal) does not fall, the class by the twin's
    existing clearances does not rise); an input at c >= clearance_goal and a non-converged input are returned bit for bit, index 0;
    the returned residual of a refined candidate is within tolerance."""
    case = CC.build_case(name, N, R)
    ref = case.twin_refined()
    c0, c1, index = ref.clear[:, 0], ref.clear[:, 1], ref.clear[:, 2]
    res_in = np.linalg.norm(case.g - case.twin.end_effector(case.q_in), axis=1)
    early = (c0 >= CC.GOAL) | (res_in > CC.TOLERANCE)
    assert np.array_equal(ref.q[early], case.q_in[early]) and np.all(index[early] == 0) and np.array_equal(c1[early], c0[early])
    assert np.array_equal(ref.q[index == 0], case.q_in[index == 0])
    assert np.all(np.minimum(c1, CC.GOAL) >= np.minimum(c0, CC.GOAL))
    assert np.all(ref.residual[~early] <= CC.TOLERANCE)
    cls_in, cls_out = CC.classes(res_in, CC.clearances(case, case.q_in)), CC.classes(ref.residual, CC.clearances(case, ref.q))
    assert np.all(cls_out <= cls_in)
    assert np.all(np.all(ref.iters[:, early] == case.q_in[early], axis=0))


def test_census_of_the_case_table():
    """Every kind of test — obstacle, self pair, sphere, half-space, box — is the least one for at least FLOOR candidates that the
    refinement works on, over the case table; and in every case of 64 or more candidates at least FLOOR queries change class 1 -> 0
    under the twin."""
    census = np.zeros(5, np.int64)
    for name, N, R in CC.CASES:
        case = CC.build_case(name, N, R)
        lt = CP.least_test(case.twin, case.q_in, case.ob)
        census += np.bincount(lt.test[lt.c < CC.GOAL], minlength=5)
        if N * R >= 64:
            ref = case.twin_refined()
            res_in = np.linalg.norm(case.g - case.twin.end_effector(case.q_in), axis=1)
            before = CC.classes(res_in, CC.clearances(case, case.q_in)).reshape(N, R).min(axis=1)
            after = CC.classes(ref.residual, CC.clearances(case, ref.q)).reshape(N, R).min(axis=1)
            freed = int(np.sum((before == 1) & (after == 0)))
            print(f"{name} N={N} R={R}: queries 1 -> 0: {freed}")
            assert freed >= CC.FLOOR, (name, N, R, freed)
    print(dict(zip(CP.CLEAR_TESTS, census)))
    assert census.min() >= CC.FLOOR, dict(zip(CP.CLEAR_TESTS, census))


# ---- the rehearsal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,R", CC.CASES)
def test_rehearsal(name, N, R):
    """Every GPU case with the float32 rehearsal in the kernel's place, through the checks the GPU suite applies. It MEASURES the
    teacher-forced single-update deviation, the gradient deviation and the clearance deviation (printed; the largest over the cases,
    rounded up, are chain_ik_clear_common's STEP_ / GAMMA_ / CLEAR_DEVIATION) and asserts that they stay within those constants,
    that at most CAP of the case's updates lie inside BAND of a kink with the twin alone, and that the rehearsal passes the no-
    exclusions statement and the completeness statement (at most 10 % of the twin-freed candidates left out)."""
    case = CC.build_case(name, N, R)
    got = CC.refine32(case)
    dev, share, live = CC.check_updates(case, got)
    print(f"{name} N={N} R={R}: {live} refined candidates; deviation of one update {dev[0]:.2e}, of gamma {dev[1]:.2e}, of c {dev[2]:.2e}; "
          f"{share:.4f} of the updates inside the band")
    assert dev[0] <= CC.STEP_DEVIATION and dev[1] <= CC.GAMMA_DEVIATION and dev[2] <= CC.CLEAR_DEVIATION, dev
    CC.check_returned(case, got)
    q64 = got["q"].astype(np.float64)
    free_out = CC.classes(np.linalg.norm(case.g - case.twin.end_effector(q64), axis=1), CC.clearances(case, q64)) == 0
    freed, left_out, freed32 = CC.check_completeness(case, got, free_out)
    print(f"    twin-freed candidates {freed}, left out {left_out}, freed by the rehearsal {freed32}")


def test_tie_rule_of_the_second_least_test():
    """LeastTest.second does not count the same contact seen through two capsules that share an end point: an obstacle nearest to a
    joint of planar3 has two tests with the same x and n, and `second` is the next different one."""
    model, twin = CC.arm("planar3")
    q = np.array([[0.3, 0.8, -0.5]])
    segs = twin.world_segments(q[0])
    (a1, joint, _), (_, b2, _) = segs[1], segs[2]         # link 1 ends where link 2 starts
    u1, u2 = (joint - a1) / np.linalg.norm(joint - a1), (b2 - joint) / np.linalg.norm(b2 - joint)
    d = (u1 - u2) / np.linalg.norm(u1 - u2)               # beyond the end of link 1 and before the start of link 2: outside the elbow
    lt = CP.least_test(twin, q, (joint + 0.2 * d)[None])
    assert np.abs(lt.x[0] - joint).max() <= 1e-12 and lt.second[0] - lt.c[0] > 1e-3


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def test_header_symbol_struct_and_argument_errors():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40
    name = "naf_chain_ik_clear"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 15
    assert ctypes.sizeof(_lib.IkClearParams) == 20 and re.search(r"\}\s*naf_chain_ik_clear_params_t;", text)
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40
    # argument errors are host code and launch nothing: a fake non-null handle is never dereferenced before they answer
    buf, other = np.zeros(64, np.float32), np.zeros(64, np.float32)
    p, w = buf.ctypes.data, other.ctypes.data
    ok, clear = _lib.IkParams(16, 0.01, 0.3, 0.5), _lib.IkClearParams(4, 1e-3, 0.02, 0.1, 0.06)
    names = ("h", "targets", "obstacles", "q_in", "N", "R", "prm", "clear", "q", "work", "residual", "out", "iters", "rec")
    good = dict(h=p, targets=p, obstacles=p, q_in=p, N=1, R=1, prm=ok, clear=clear, q=p, work=w, residual=p, out=p, iters=None, rec=None)
    bad = [{k: None} for k in ("h", "targets", "obstacles", "q_in", "q", "work", "residual", "out")]
    bad += [dict(iters=p), dict(rec=p), dict(work=p), dict(N=0), dict(N=-3), dict(R=0), dict(R=3), dict(R=128)]
    bad += [dict(prm=_lib.IkParams(*v)) for v in ((0, 0.01, 0.3, 0.5), (-2, 0.01, 0.3, 0.5), (16, float("nan"), 0.3, 0.5),
                                                  (16, 0.0, 0.3, 0.5), (16, 0.01, float("inf"), 0.5), (16, 0.01, 0.3, -1.0))]
    inf, nan = float("inf"), float("nan")
    bad += [dict(clear=_lib.IkClearParams(*v)) for v in ((-1, 1e-3, 0.02, 0.1, 0.06), (17, 1e-3, 0.02, 0.1, 0.06),
                                                        (4, nan, 0.02, 0.1, 0.06), (4, -1e-3, 0.02, 0.1, 0.06), (4, inf, 0.02, 0.1, 0.06),
                                                        (4, 1e-3, nan, 0.1, 0.06), (4, 1e-3, inf, 0.1, 0.06), (4, 1e-3, 0.02, 0.0, 0.06),
                                                        (4, 1e-3, 0.02, nan, 0.06), (4, 1e-3, 0.02, inf, 0.06), (4, 1e-3, 0.02, 0.1, -0.1),
                                                        (4, 1e-3, 0.02, 0.1, nan))]
    for change in bad:
        a = dict(good, **change)
        assert lib.naf_chain_ik_clear(*[a[k] for k in names], None) == NAF_ERR_ARG, change
    assert not buf.any() and not other.any()
    # the twin refuses the same constants
    for kw in (dict(push_iterations=0), dict(push_iterations=8, push_settle=9), dict(push_settle=-1), dict(push_max=0.0),
               dict(push_max=nan), dict(clearance_goal=inf)):
        with pytest.raises(ValueError):
            CP.clear_defaults(0.0, **kw)


def test_no_kernel_of_the_new_launch_spills():
    """both instantiations of chain_ik_clear_kernel: no scratch, as the build's resource report has it"""
    import json
    from robotic_manipulator_rloa_amd import _lib
    usage = json.load(open(_lib.USAGE_PATH))
    mine = {k: v for k, v in usage.items() if "chain_ik_clear_kernel" in k}
    assert len(mine) == 2 and all(v["scratch_bytes_per_lane"] == 0 and v["vgpr_spills"] == 0 for v in mine.values()), mine


# ---- through the façade ---------------------------------------------------------------------------------------------------------------
def test_facade_arguments_and_refusals():
    """solve_goal_poses / plan_joint_paths(avoid_contact=True) on the host twin equal goal_poses_host with the same arguments, fill
    pushed and input_clearance, never lose a free query, and free some; without the argument the two fields are None and every
    other field is what it was; the refusals, the one with an orientation goal among them."""
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    f = framework(workcell_boxes=IK.BX.boxes_of("iiwa_like7"))
    twin = f.env
    rng = np.random.default_rng(12)
    N = 24
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (N, 3))
    plain = f.solve_goal_poses(targets, restarts=4, seed=5, on_device=False)
    out = f.solve_goal_poses(targets, restarts=4, seed=5, on_device=False, avoid_contact=True)
    want = goal_poses_host(twin, np.tile(twin.initial_joint_positions, (N, 1)), targets, np.tile(twin.obstacle_pos, (N, 1)), restarts=4,
                           seed=5, avoid_contact=True)
    for a, b in zip(out, want):
        assert np.array_equal(a, b)
    assert plain.pushed is None and plain.input_clearance is None
    assert out.pushed.dtype == bool and np.array_equal(out.pushed, want.pushed) and np.array_equal(out.input_clearance, want.input_clearance)
    assert np.all(out.free >= plain.free) and np.array_equal(out.reachable, plain.reachable) and out.free.sum() > plain.free.sum()
    least = np.minimum(np.minimum(out.clearance, out.self_clearance), out.cell_clearance)
    assert np.all(least[out.pushed] > out.input_clearance[out.pushed])
    other = f.solve_goal_poses(targets, restarts=4, seed=5, on_device=False, avoid_contact=True, clearance_goal=0.05, push_iterations=8)
    assert np.all(other.free >= plain.free)
    paths = f.plan_joint_paths(targets, seed=5, candidates=2, resolution=0.1, on_device=False, avoid_contact=True)
    base = f.plan_joint_paths(targets, seed=5, candidates=2, resolution=0.1, on_device=False)
    assert np.sum(paths.outcome == "goal") <= np.sum(base.outcome == "goal")
    args = dict(targets=targets[:4], on_device=False, avoid_contact=True)
    for kw, match in ((dict(approach_directions=[0, 0, -1]), "position only"), (dict(orientations=[0, 0, 0, 1]), "position only"),
                      (dict(avoid_contact="yes"), "avoid_contact is a bool"), (dict(clearance_goal=float("nan")), "clearance_goal is"),
                      (dict(clearance_goal="far"), "clearance_goal is"), (dict(push_iterations=0), "push_iterations is"),
                      (dict(push_iterations=3), "push_iterations is"), (dict(push_iterations=2.5), "push_iterations is")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.solve_goal_poses(**dict(args, **kw))
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.plan_joint_paths(**dict(args, **kw))
    with pytest.raises(InvalidEnvironmentParameter, match="goal_joint_positions=.* is given the goal poses themselves"):
        f.plan_joint_paths(goal_joint_positions=np.tile(twin.initial_joint_positions, (2, 1)), avoid_contact=True, on_device=False)
    # the push's arguments without avoid_contact ask for nothing
    quiet = f.solve_goal_poses(targets, restarts=4, seed=5, on_device=False, clearance_goal=0.05, push_iterations=8)
    for a, b in zip(quiet, plain):
        assert np.array_equal(a, b)
    assert quiet.pushed is None


def test_reach_targets_with_the_push_against_a_stub_agent(monkeypatch):
    import torch
    from robotic_manipulator_rloa_amd.engine import ReachResult
    from robotic_manipulator_rloa_amd.utils.exceptions import ConfigurationIncomplete, InvalidEnvironmentParameter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # the goal poses come from the twin
    f = framework(workcell_boxes=IK.BX.boxes_of("iiwa_like7"))
    twin = f.env
    rng = np.random.default_rng(4)
    N, F = 6, 5
    targets = np.array([0.45, 0.3, 0.6]) + rng.uniform(-0.25, 0.25, (N, 3))
    start = np.tile(twin.initial_joint_positions, (N, 1))

    class Agent:
        state_size, action_size, seed, world_size = 23, 7, 0, 1
        calls = []

        def rollout_vectorized(self, chain, targets, obstacles, q0, **kw):
            self.calls.append(kw)
            z = np.zeros(N, np.float32)
            paths = np.repeat(q0[:, None, :], F + 1, axis=1).astype(np.float32)
            return ReachResult(np.array(["frames"] * N), np.full(N, F), z, z, z, z, paths, z, z, z, z, z)

    f.naf_agent = Agent()
    with pytest.raises(InvalidEnvironmentParameter, match="needs goal_poses=True or\\s+joint_paths=True|needs goal_poses=True or joint_paths=True"):
        f.reach_targets(targets, initial_joint_positions=start, frames=F, avoid_contact=True)
    with pytest.raises(InvalidEnvironmentParameter, match="position only"):
        f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True, avoid_contact=True, approach_directions=[0, 0, -1])
    assert not Agent.calls                                                   # refused before the rollout
    plain = f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True)
    out = f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True, avoid_contact=True)
    assert Agent.calls[-1] == Agent.calls[-2] and plain.goal.pushed is None
    want = f.solve_goal_poses(targets, initial_joint_positions=start, avoid_contact=True)
    for a, b in zip(out.goal, want):
        assert np.array_equal(a, b)
    assert np.array_equal(out.goal.pushed, want.pushed)
    both = f.reach_targets(targets, initial_joint_positions=start, frames=F, joint_paths=True, avoid_contact=True)
    ok = want.reachable
    assert np.array_equal(both.path.goal[ok], C.f32(want.joint_positions[ok]))
    # the stand-in and PyBullet are refused as solve_goal_poses refuses them
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    g = ManipulatorFramework()
    g.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="kinematic environment"):
        g.solve_goal_poses([0.4, 0.2, 0.5], avoid_contact=True)

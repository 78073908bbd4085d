"""CPU: the goal-pose rule of environment/kinematic.py (jacobian, ik_step, solve_ik, select_goal_pose), the rehearsal of every case of
tests/test_chain_ik_gpu.py with a float32 restatement in the kernel's place, the plumbing of the two entry points and the façade."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest

import chain_ik_common as IK
import chain_rollout_common as C
from conftest import ROOT
from test_chain_env_cpu import ARMS as ARM_TABLE
from test_chain_env_cpu import model_of, path, random_q

from robotic_manipulator_rloa_amd.environment.kinematic import (GoalPoses, KinematicEnvironment, goal_poses_host, ik_seeds,
                                                                joint_distance32, select_goal_pose, spd3_solve)


def twin_of(name):
    if name == "slider4":
        return IK.slider()
    model = model_of(name)
    return model, KinematicEnvironment(model, (0, 0, 0), (0, 0, 0), IK.ORAD)


# ---- the Jacobian ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ARM_TABLE))                    # (slider4 among them)
def test_jacobian_against_central_differences(name):
    """J's column m against (ee(q + h e_m) - ee(q - h e_m)) / 2h, h = 1e-6: the difference quotient's own error is h^2 |ee'''| / 6 +
    2^-52 reach / h <= 1e-9 reach; 1e-7 reach is asserted. The end effector returned is end_effector's."""
    model, twin = twin_of(name)
    rng = np.random.default_rng(5)
    q = np.stack([random_q(model, rng) for _ in range(200)])
    ee, J = twin.jacobian(q)
    assert J.shape == (200, 3, model.A) and np.abs(ee - twin.end_effector(q)).max() <= 1e-12 * model.reach
    h = 1e-6
    for m in range(model.A):
        step = h * np.eye(model.A)[m]
        num = (twin.end_effector(q + step) - twin.end_effector(q - step)) / (2 * h)
        assert np.abs(J[..., m] - num).max() <= 1e-7 * model.reach, (m, np.abs(J[..., m] - num).max())
    one_ee, one_J = twin.jacobian(q[3])                      # a single pose: no leading axis
    assert np.array_equal(one_J, J[3]) and np.array_equal(one_ee, ee[3])


def test_jacobian_of_a_prismatic_joint_is_its_axis_and_columns_behind_the_end_effector_are_zero():
    model, twin = IK.slider()
    assert [j.type for j in model.joints] == [0, 1, 0, 1]
    rng = np.random.default_rng(6)
    q = np.stack([random_q(model, rng) for _ in range(50)])
    _, J = twin.jacobian(q)
    assert np.allclose(np.linalg.norm(J[..., 1], axis=-1), 1.0) and np.allclose(J[..., 1], [0.0, 0.0, 1.0])    # the lift, along world z
    assert np.allclose(np.linalg.norm(J[..., 3], axis=-1), 1.0)
    # iiwa_like7 with the end effector on its fourth link: joints 4 .. 6 are behind it
    short = model_of("iiwa_like7", endeffector_index=3)
    assert short.A == 7 and short.ee_frame == 4
    tw = KinematicEnvironment(short, (0, 0, 0), (0, 0, 0))
    q = np.stack([random_q(short, rng) for _ in range(50)])
    ee, J = tw.jacobian(q)
    assert np.all(J[..., 4:] == 0.0) and np.all(np.abs(J[..., :2]).max(axis=(0, 1)) > 0.1)
    moved = q.copy()
    moved[:, 4:] += 0.3
    assert np.array_equal(tw.end_effector(moved), ee)
    out = tw.ik_step(q, ee + 0.05, **tw.ik_defaults())
    assert np.array_equal(out[:, 4:], q[:, 4:])              # and the iteration leaves them where they are


# ---- one update ------------------------------------------------------------------------------------------------------------------
def test_spd3_solve_against_numpy():
    rng = np.random.default_rng(8)
    B = rng.normal(size=(500, 3, 5))
    M = B @ np.swapaxes(B, -1, -2) + 0.01 * np.eye(3)
    e = rng.normal(size=(500, 3))
    want = np.linalg.solve(M, e[..., None])[..., 0]
    assert np.abs(spd3_solve(M, e) - want).max() <= 1e-10 * np.abs(want).max()


def test_ik_step_scalings_clamp_zero_error_and_singular_pose():
    model, twin = twin_of("planar3")
    k = twin.ik_defaults()
    lam, e_max, dq_max = k["lam"], k["e_max"], k["dq_max"]
    assert (lam, e_max, dq_max) == (0.05 * model.reach, 0.25 * model.reach, 0.5)
    q = np.array([0.3, -0.4, 0.5])
    ee, J = twin.jacobian(q)

    def by_hand(q, g, e_max=e_max, dq_max=dq_max):
        ee, J = twin.jacobian(q)
        e = g - ee
        if np.linalg.norm(e) > e_max:
            e = e * e_max / np.linalg.norm(e)
        dq = J.T @ np.linalg.solve(J @ J.T + lam ** 2 * np.eye(3), e)
        if np.abs(dq).max() > dq_max:
            dq = dq * dq_max / np.abs(dq).max()
        return q + dq, e, dq
    # a short error: neither scaling acts
    g = ee + np.array([0.01, -0.02, 0.0])
    want, e, dq = by_hand(q, g)
    assert np.linalg.norm(e) < e_max and np.abs(dq).max() < dq_max
    assert np.abs(twin.ik_step(q, g, lam, e_max, dq_max) - want).max() <= 1e-12
    # a long error is cut to e_max: the step is the one towards the point e_max along it
    g_far = ee + np.array([0.0, 3.0 * e_max, 0.0])
    assert np.abs(twin.ik_step(q, g_far, lam, e_max, dq_max) - twin.ik_step(q, ee + np.array([0.0, e_max, 0.0]), lam, e_max, dq_max)).max() <= 1e-12
    assert np.abs(twin.ik_step(q, g_far, lam, e_max, dq_max) - by_hand(q, g_far)[0]).max() <= 1e-12
    # a joint update above dq_max scales the whole of dq
    raw = by_hand(q, g_far, dq_max=np.inf)[2]
    small = 0.25 * np.abs(raw).max()
    got = twin.ik_step(q, g_far, lam, e_max, small) - q
    assert np.abs(np.abs(got).max() - small) <= 1e-12 and np.abs(got / np.abs(got).max() - raw / np.abs(raw).max()).max() <= 1e-9
    # the clamp: a limited joint is stopped at its limit, the others move as they would
    hi = model.joints[2].upper
    q_edge = np.array([0.3, -0.4, hi - 1e-4])
    g_up = twin.end_effector(np.array([0.3, -0.4, hi])) + np.array([-0.05, 0.05, 0.0])
    want = by_hand(q_edge, g_up)[0]
    assert want[2] > hi
    got = twin.ik_step(q_edge, g_up, lam, e_max, dq_max)
    assert got[2] == hi and np.abs(got[:2] - want[:2]).max() <= 1e-12
    # an arm without limits is not clamped
    free, ftwin = twin_of("standin8")
    unlimited = [m for m, j in enumerate(free.joints) if not j.limited]
    if unlimited:
        qf = np.zeros(free.A)
        qf[unlimited[0]] = 3.1
        assert np.all(np.isfinite(ftwin.ik_step(qf, ftwin.end_effector(qf) + 0.1, **ftwin.ik_defaults())))
    # a zero-length error: nothing moves, nothing divides by zero
    with np.errstate(all="raise"):
        assert np.array_equal(twin.ik_step(q, ee, lam, e_max, dq_max), q)
    # fully stretched: J J^T is singular (every column is normal to the arm), lam alone keeps M regular
    straight = np.zeros(3)
    ee0, J0 = twin.jacobian(straight)
    assert np.linalg.matrix_rank(J0 @ J0.T, tol=1e-12) == 1
    out = twin.ik_step(straight, ee0 * 0.5, lam, e_max, dq_max)           # a pull along the arm: no joint can follow it
    assert np.all(np.isfinite(out)) and np.abs(out - straight).max() <= 1e-12
    side = twin.ik_step(straight, ee0 + np.array([0.0, 0.05, 0.0]), lam, e_max, dq_max)
    assert np.all(np.isfinite(side)) and np.abs(side).max() > 1e-3


# ---- whole solves -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,autocollision", C.ARMS)
def test_solve_ik_converges_on_reachable_targets_and_not_beyond_reach(name, autocollision):
    """256 targets, each the end effector of a pose uniform inside the limits, R = 8 seeds (the initial pose and 7 uniform), K = 32:
    every query has a converged candidate except at most 1 %. Targets at 1.1 reach from the base: none converges."""
    model, twin = C.arm(name, autocollision)
    rng = np.random.default_rng(0)
    N, R = 256, 8
    g = twin.end_effector(np.stack([random_q(model, rng) for _ in range(N)]))
    seeds = np.stack([[random_q(model, rng) for _ in range(R)] for _ in range(N)])
    seeds[:, 0] = [j.init for j in model.joints]
    q, res = twin.solve_ik(g[:, None, :], seeds)
    assert q.shape == (N, R, model.A) and res.shape == (N, R)
    lo, hi = twin.joint_limits()
    assert np.all(q >= lo) and np.all(q <= hi)
    assert np.abs(res - np.linalg.norm(g[:, None, :] - twin.end_effector(q), axis=-1)).max() <= 1e-12
    missed = int(np.sum(~(res <= 1e-3).any(axis=1)))
    print(f"{name}: {N - missed} of {N} queries converge, restart 0 alone {np.mean(res[:, 0] <= 1e-3):.3f}")
    assert missed <= 0.01 * N, missed
    d = rng.normal(size=(N, 3))
    if name == "planar3":
        d[:, 2] = 0.0
    far = 1.1 * model.reach * d / np.linalg.norm(d, axis=1, keepdims=True)
    _, res_far = twin.solve_ik(far[:, None, :], seeds)
    print(f"{name}: smallest residual at 1.1 reach {res_far.min():.3f}")
    assert not np.any(res_far <= 1e-3) and res_far.min() > 0.05 * model.reach


# ---- selection ----------------------------------------------------------------------------------------------------------------------
def brute_force(res, jd, clear, self_clear, cell_clear, tolerance, margin):
    """the rule read literally, candidate by candidate"""
    best = None
    for r in range(len(res)):
        conv = res[r] <= tolerance
        free = clear[r] >= margin and self_clear[r] >= margin and cell_clear[r] >= margin
        cls = 2 if not conv else (0 if free else 1)
        key = (cls, res[r] if cls == 2 else jd[r], r)
        if best is None or key < best:
            best = key
    return best[2], best[0]


def test_selection_against_brute_force_over_all_orderings():
    inf = np.inf
    # (residual, joint distance, clearance, self-clearance, workcell clearance): two free and converged (a tie in joint distance),
    # two converged in contact (one by the workcell, one by itself, a tie again), three that missed (a tie in residual)
    table = [(2e-4, 0.7, 0.1, inf, inf), (5e-4, 0.7, 0.2, inf, 0.3), (1e-4, 0.2, 0.1, inf, -0.01), (3e-4, 0.2, 0.1, -0.002, inf),
             (0.02, 0.1, 0.1, inf, inf), (0.02, 0.9, -0.1, inf, inf), (0.3, 0.0, 0.5, inf, inf)]
    tol = 1e-3
    seen = set()
    for size in (1, 2, 3, 4):
        for rows in itertools.permutations(range(len(table)), size):
            t = np.array([table[i] for i in rows])
            want = brute_force(*t.T, tol, 0.0)
            got = select_goal_pose(t[None, :, 0], t[None, :, 1], t[None, :, 2], t[None, :, 3], t[None, :, 4], tol, 0.0)
            assert (int(got[0][0]), int(got[1][0])) == want, (rows, got, want)
            seen.add(want[1])
    assert seen == {0, 1, 2}
    # all orderings of the whole table at once, batched, and with a margin that turns the first two into contacts
    perms = np.array(list(itertools.permutations(range(len(table)))))
    t = np.array(table)[perms]                                    # [5040, 7, 5]
    for margin in (0.0, 0.15, 0.25):
        choice, cls = select_goal_pose(t[..., 0], t[..., 1], t[..., 2], t[..., 3], t[..., 4], tol, margin)
        for i in range(0, len(perms), 97):
            assert (int(choice[i]), int(cls[i])) == brute_force(*t[i].T, tol, margin)
    # the tie goes to the lowest r
    assert select_goal_pose([[2e-4, 2e-4]], [[0.5, 0.5]], [[1.0, 1.0]], [[inf, inf]], [[inf, inf]], tol)[0][0] == 0
    # joint_distance is formed in float32
    q, q0 = np.array([[0.1, 0.7000001]]), np.array([[0.0, 0.2]])
    jd = joint_distance32(q, q0)
    assert jd.dtype == np.float32 and jd[0] == np.float32(np.float32(0.7000001) - np.float32(0.2))


def test_goal_poses_host_and_seeds():
    model, twin = IK.arm("iiwa_like7")
    seeds = ik_seeds(model, 5, 8, seed=3)
    lo, hi = C.limits_of(model)
    assert seeds.shape == (5, 8, model.A) and seeds.dtype == np.float32 and np.all(seeds[:, 0] == 0.0)
    assert np.all(seeds[:, 1:] >= lo.astype(np.float32)) and np.all(seeds[:, 1:] <= hi.astype(np.float32))
    assert np.array_equal(seeds, ik_seeds(model, 5, 8, seed=3)) and not np.array_equal(seeds, ik_seeds(model, 5, 8, seed=4))
    assert ik_seeds(model, 3, 1, seed=0).shape == (3, 1, model.A)
    case = IK.build_case("iiwa_like7", 6, 4)
    out = goal_poses_host(twin, case.q_start, case.targets, case.obstacles, restarts=4, iterations=IK.K, tolerance=IK.TOLERANCE, seed=1)
    assert isinstance(out, GoalPoses) and out.joint_positions.shape == (6, model.A) and out.joint_distance.dtype == np.float32
    assert np.array_equal(out.reachable, out.residual <= IK.TOLERANCE)
    assert np.all(out.free <= out.reachable) and np.all(out.converged_restarts[~out.reachable] == 0)
    res = np.linalg.norm(case.targets - twin.end_effector(out.joint_positions), axis=1)
    assert np.abs(res - out.residual).max() <= 1e-12
    assert np.all(out.converged_restarts <= 4) and np.all((out.restart >= 0) & (out.restart < 4))


# ---- the rehearsal of tests/test_chain_ik_gpu.py -----------------------------------------------------------------------------------
REHEARSED = [(name, N, R) for name in IK.ARMS for N, R in IK.COUNTS] + [("long32", 4, 4), ("slider4", 8, 4), ("iiwa_like7", 65, 1)]


@functools.lru_cache(maxsize=None)
def rehearse(name, N, R):
    """(case, the restatement's q_out, residual, iters and its largest single-step deviation from ik_step): computed once"""
    case = IK.build_case(name, N, R)
    q_out, residual, iters = IK.solve32(case)
    return case, q_out, residual, iters, IK.check_iterations(case, iters)


@pytest.mark.parametrize("name,N,R", REHEARSED)
def test_rehearsal(name, N, R):
    """Every case of the GPU suite with the float32 restatement (chain_ik_common.ik_step32) in the kernel's place and the twin's
    clearances rounded to float32 in the probes': the same checks, so the band shares (<= 1 %) and the floors (8 queries per
    class where N R >= 64) hold before a GPU is involved, and every query ends in the class it was built for."""
    case, q_out, residual, iters, dev = rehearse(name, N, R)
    print(f"{name} N={N} R={R}: largest single-step deviation of the float32 restatement {dev:.2e} (STEP_DEVIATION {IK.STEP_DEVIATION:.2e})")
    assert dev <= IK.STEP_DEVIATION, dev
    probe, cell = IK.probes32(case, q_out)
    jd = joint_distance32(q_out.reshape(N, R, -1), case.q_start[:, None, :]).reshape(-1)
    choice, cls = select_goal_pose(residual.reshape(N, R), jd.reshape(N, R), probe[:, 3].reshape(N, R), probe[:, 4].reshape(N, R),
                                   cell.reshape(N, R), np.float32(IK.TOLERANCE), np.float32(case.margin))
    IK.check_solution(case, q_out, residual, choice, cls, jd, probe, cell)
    assert np.array_equal(cls, case.want), (cls, case.want)
    # the float32 iteration flips no query's reachability
    _, res_twin = case.twin_solution()
    assert np.array_equal((residual.reshape(N, R) <= IK.TOLERANCE).any(axis=1), (res_twin <= IK.TOLERANCE).any(axis=1))


def test_the_measured_deviation_is_the_constant():
    """chain_ik_common.STEP_DEVIATION is the largest single-step deviation the rehearsal measures over all its cases, rounded up
    by at most a quarter; the teacher-forced bound of the GPU test is 8 x it."""
    measured = {c: rehearse(*c)[4] for c in REHEARSED}
    worst = max(measured.values())
    print({c: f"{v:.2e}" for c, v in measured.items()})
    assert 0.75 * IK.STEP_DEVIATION <= worst <= IK.STEP_DEVIATION, (worst, measured)
    assert IK.STEP_BOUND == 8 * IK.STEP_DEVIATION


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def test_header_symbols_abi_and_argument_errors():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40
    for name in ("naf_chain_ik_solve", "naf_chain_ik_select"):
        assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
        assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1
    assert ctypes.sizeof(_lib.IkParams) == 16 and re.search(r"\}\s*naf_chain_ik_params_t;", text)
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40
    # argument errors are host code and launch nothing: a fake non-null handle is never dereferenced before they answer
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    ok = _lib.IkParams(32, 0.01, 0.3, 0.5)
    solve = lambda h=p, t=p, q=p, s=p, N=1, R=1, prm=ok, out=p, res=p: lib.naf_chain_ik_solve(h, t, q, s, N, R, prm, out, res, None, None)   # noqa: E731
    for kw in (dict(h=None), dict(t=None), dict(q=None), dict(s=None), dict(out=None), dict(res=None), dict(N=0), dict(N=-3),
               dict(R=0), dict(R=3), dict(R=12), dict(R=128), dict(prm=_lib.IkParams(0, 0.01, 0.3, 0.5)),
               dict(prm=_lib.IkParams(32, float("nan"), 0.3, 0.5)), dict(prm=_lib.IkParams(32, 0.0, 0.3, 0.5)),
               dict(prm=_lib.IkParams(32, 0.01, float("inf"), 0.5)), dict(prm=_lib.IkParams(32, 0.01, 0.3, -1.0)),
               dict(prm=_lib.IkParams(32, 0.01, 0.3, float("nan")))):
        assert solve(**kw) == -1, kw
    select = lambda h=p, q=p, q0=p, res=p, pr=p, N=1, R=1, tol=1e-3, margin=0.0, ch=p, cl=p, jd=p: lib.naf_chain_ik_select(   # noqa: E731
        h, q, q0, res, pr, None, N, R, tol, margin, ch, cl, jd, None)
    for kw in (dict(h=None), dict(q=None), dict(q0=None), dict(res=None), dict(pr=None), dict(ch=None), dict(cl=None), dict(jd=None),
               dict(N=0), dict(R=0), dict(R=6), dict(R=128), dict(tol=float("nan")), dict(tol=-1.0), dict(tol=float("inf")),
               dict(margin=float("nan")), dict(margin=float("inf"))):
        assert select(**kw) == -1, kw


# ---- through the façade ---------------------------------------------------------------------------------------------------------------
def framework(**kw):
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    ee, involved, fixed, init, var = ARM_TABLE["iiwa_like7"]
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(path("iiwa_like7"), ee, fixed, involved, [0.45, 0.3, 0.6], [0.35, 0.2, 0.45], init, var,
                                       link_radius=0.03, obstacle_radius=0.07, consider_autocollision=True, **kw)
    return f


def test_solve_goal_poses_on_the_host_and_its_refusals():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized,
                                                               InvalidEnvironmentParameter)
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.solve_goal_poses([0.4, 0.2, 0.5])
    f.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="PyBullet and the synthetic stand-in have no chain model"):
        f.solve_goal_poses([0.4, 0.2, 0.5])
    f = framework(workcell_boxes=IK.BX.boxes_of("iiwa_like7"))
    twin = f.env
    rng = np.random.default_rng(2)
    targets = np.concatenate([twin.end_effector(IK.free_poses(twin.model, twin, rng, 9)), [[0.0, 0.0, 1.1 * twin.model.reach]]])
    out = f.solve_goal_poses(targets, restarts=4, seed=5, on_device=False)            # needs no agent
    assert isinstance(out, GoalPoses) and out.reachable.shape == (10,) and out.joint_positions.shape == (10, 7)
    assert out.reachable[:9].sum() >= 8 and not out.reachable[9] and not out.free[9]
    want = goal_poses_host(twin, np.tile(twin.initial_joint_positions, (10, 1)), targets, np.tile(twin.obstacle_pos, (10, 1)),
                           restarts=4, seed=5)
    for a, b in zip(out, want):
        assert np.array_equal(a, b)
    assert np.array_equal(out.clearance, twin.clearance(out.joint_positions, C.f32(np.tile(twin.obstacle_pos, (10, 1)))) - twin.obstacle_radius)
    one = f.solve_goal_poses(targets[0], restarts=4, seed=5, on_device=False)
    assert one.reachable.shape == (1,)
    # a wider margin frees no pose, and one that no pose keeps leaves none free
    assert not f.solve_goal_poses(targets, restarts=4, seed=5, clearance_margin=5.0, on_device=False).free.any()
    for kw, match in ((dict(targets=np.zeros((4, 2))), "targets"), (dict(targets=[0.0, np.nan, 0.0]), "not finite"),
                      (dict(obstacles=np.zeros((2, 3))), "obstacles"), (dict(initial_joint_positions=np.zeros(6)), "initial_joint"),
                      (dict(initial_joint_positions=np.full(7, 9.0)), r"query 0: joint 0 \(involved_joints\[0\]\)"),
                      (dict(restarts=3), "power of two"), (dict(restarts=128), "power of two"), (dict(restarts=0), "power of two"),
                      (dict(restarts=2.0), "power of two"), (dict(iterations=0), "iterations"), (dict(tolerance=0.0), "tolerance"),
                      (dict(tolerance=float("nan")), "tolerance"), (dict(clearance_margin=float("inf")), "clearance_margin"),
                      (dict(seed=-1), "seed"), (dict(seed=1.5), "seed")):
        args = dict(targets=np.zeros((4, 3)), on_device=False)
        args.update(kw)
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.solve_goal_poses(**args)


def test_reach_targets_with_goal_poses_against_a_stub_agent(monkeypatch):
    import torch
    from robotic_manipulator_rloa_amd.engine import ReachResult
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # the goal poses come from the twin
    f = framework()
    twin = f.env
    rng = np.random.default_rng(4)
    N, F = 6, 5
    goals = IK.free_poses(twin.model, twin, rng, N)
    targets = twin.end_effector(goals)
    start = np.tile(twin.initial_joint_positions, (N, 1))

    class Agent:                      # returns a straight joint path to the goal pose in F frames for every query but two
        state_size, action_size, seed, world_size = 23, 7, 0, 1
        calls = []

        def rollout_vectorized(self, chain, targets, obstacles, q0, **kw):
            self.calls.append(kw)
            z = np.zeros(N, np.float32)
            s = np.linspace(0.0, 1.0, F + 1)[None, :, None]
            paths = (q0[:, None, :] + s * (goals - q0)[:, None, :]).astype(np.float32) if kw["trajectories"] else None
            outcome = np.array(["reached"] * N)
            outcome[1] = "frames"
            return ReachResult(outcome, np.full(N, F), z, z, z, z, paths, z, z, z, z, z)

    f.naf_agent = Agent()
    plain = f.reach_targets(targets, initial_joint_positions=start, frames=F)
    assert plain.goal is None and plain.path_ratio is None
    assert Agent.calls[-1] == dict(frames=F, noise_scale=0.0, n_envs=None, trajectories=True, scene={"obstacle_radius": 0.07})
    out = f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True)
    assert Agent.calls[-1] == Agent.calls[-2]                                # the rollout is called as it was
    want = f.solve_goal_poses(targets, initial_joint_positions=start)
    for a, b in zip(out.goal, want):
        assert np.array_equal(a, b)
    length = np.abs(goals - start).max(axis=1)                               # a straight path's length is its ends' distance
    ok = out.goal.free.copy()
    ok[1] = False
    assert np.all(np.isnan(out.path_ratio[~ok])) and ok.sum() >= 3
    assert np.abs(out.path_ratio[ok] - length[ok] / out.goal.joint_distance[ok]).max() <= 1e-5
    for field in ("outcome", "frames", "joint_positions", "score"):
        assert np.array_equal(getattr(out, field), getattr(plain, field))
    with pytest.raises(InvalidEnvironmentParameter, match="trajectories"):
        f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True, trajectories=False)

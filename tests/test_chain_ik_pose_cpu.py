"""CPU (`-m "not gpu"`): the rule of oriented goal poses in environment/kinematic.py (end_effector_frame, orientation_error, spd6_solve,
ik_pose_step, solve_ik_pose, orientation_goal, goal_poses_host) against references of its own making; the rehearsal of every GPU
case of tests/test_chain_ik_pose_gpu.py with a float32 restatement in the kernel's place, which measures the bounds the GPU tests use;
the façade's arguments and refusals; and the plumbing of naf_chain_ik_solve_pose."""
import ctypes
import os
import re

import numpy as np
import pytest

import chain_ik_common as IK
import chain_ik_pose_common as P
import chain_rollout_common as C
from test_chain_env_cpu import random_q
from test_chain_ik_cpu import framework

from robotic_manipulator_rloa_amd.environment.kinematic import (ORIENT_AXIS, ORIENT_FULL, GoalPoses, gather_goal_poses, goal_poses_host,
                                                                ik_seeds, joint_distance32, orientation_error, orientation_goal,
                                                                quaternion_matrix, select_goal_pose, spd6_solve, tool_normal_of)
from robotic_manipulator_rloa_amd.environment.urdf_chain import axis_rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAF_ERR_ARG = -1
ANGLES = [0.0, 1e-7, np.pi / 2, np.pi - 1e-3, np.pi]


def random_rotation(rng):
    return axis_rotation(unit(rng.normal(size=3)), rng.uniform(0.0, np.pi))      # (float64: orthonormal to rounding)


def unit(v):
    return v / np.linalg.norm(v)


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", ANGLES)
def test_orientation_error_recovers_a_composed_rotation_vector(theta):
    """full: R_goal = exp([theta u]) R_ee gives e_w = theta u (at pi: either sign); axis: d = exp([theta u]) t with u perpendicular
    to t gives e_w = theta u; antiparallel (theta = pi): half a turn about R_ee tool_normal, whatever u was."""
    rng = np.random.default_rng(int(theta * 1e6) % 1000)
    for _ in range(20):
        R_ee, u = random_rotation(rng), unit(rng.normal(size=3))
        w = orientation_error(R_ee, ORIENT_FULL, axis_rotation(u, theta) @ R_ee)
        bound = 1e-12 if theta < 3.0 else 1e-9
        if theta == np.pi:
            assert min(np.abs(w - theta * u).max(), np.abs(w + theta * u).max()) <= 1e-7
            assert abs(np.linalg.norm(w) - np.pi) <= 1e-12
        else:
            assert np.abs(w - theta * u).max() <= bound, (theta, w, theta * u)
        # nine values row-major are the same goal
        assert np.array_equal(orientation_error(R_ee, ORIENT_FULL, (axis_rotation(u, theta) @ R_ee).reshape(9)), w)
        axis = unit(rng.normal(size=3))
        normal = tool_normal_of(axis)
        assert abs(normal @ axis) <= 1e-15 and abs(np.linalg.norm(normal) - 1.0) <= 1e-15
        t = R_ee @ axis
        u = unit(np.cross(t, rng.normal(size=3)))
        d = -t if theta == np.pi else axis_rotation(u, theta) @ t
        w = orientation_error(R_ee, ORIENT_AXIS, d, axis, normal)
        if theta == np.pi:
            assert np.abs(w - np.pi * (R_ee @ normal)).max() <= 1e-15 and abs(w @ t) <= 1e-12
        else:
            assert np.abs(w - theta * u).max() <= 1e-12, (theta, w, theta * u)
    # batches broadcast
    R = np.stack([random_rotation(rng) for _ in range(6)]).reshape(2, 3, 3, 3)
    G = np.stack([random_rotation(rng) for _ in range(6)]).reshape(2, 3, 3, 3)
    both = orientation_error(R, ORIENT_FULL, G)
    assert both.shape == (2, 3, 3) and np.array_equal(both[1, 2], orientation_error(R[1, 2], ORIENT_FULL, G[1, 2]))


def test_orientation_error_is_well_conditioned_near_pi():
    """At pi - 1e-6 a float32-sized perturbation of R_goal (1e-7) moves e_w by about as much, not by 1e-7 / sin(theta)"""
    rng = np.random.default_rng(1)
    for _ in range(20):
        R_ee, u = random_rotation(rng), unit(rng.normal(size=3))
        theta = np.pi - 1e-6
        G = axis_rotation(u, theta) @ R_ee
        w = orientation_error(R_ee, ORIENT_FULL, G)
        w2 = orientation_error(R_ee, ORIENT_FULL, G + 1e-7 * rng.uniform(-1, 1, (3, 3)))
        assert np.abs(w - theta * u).max() <= 1e-9 and min(np.abs(w2 - w).max(), np.abs(w2 + w).max()) <= 2e-6


@pytest.mark.parametrize("name", P.ARMS)
def test_jacobian6_against_central_differences(name):
    """Column m of [Jp ; Ja] is the derivative of (ee, rotation vector of R_ee(q + h) R_ee(q - h)^T / 2h) by q_m; a prismatic joint's
    angular rows and every row behind the end-effector frame are 0."""
    model, twin = IK.arm(name)
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(4):
        q = random_q(model, rng)
        ee, R_ee, Jp, Ja = twin.jacobian6(q)
        R0, ee0 = twin.end_effector_frame(q)
        assert np.array_equal(ee, ee0) and np.array_equal(R_ee, R0) and np.array_equal(Jp, twin.jacobian(q)[1])
        assert np.abs(ee - twin.end_effector(q)).max() <= 1e-15
        for m, j in enumerate(model.joints):
            dq = np.zeros(model.A)
            dq[m] = h
            (Rp, ep), (Rm, em) = twin.end_effector_frame(q + dq), twin.end_effector_frame(q - dq)
            assert np.abs((ep - em) / (2 * h) - Jp[:, m]).max() <= 1e-8 * max(1.0, model.reach)
            assert np.abs(orientation_error(Rm, ORIENT_FULL, Rp) / (2 * h) - Ja[:, m]).max() <= 1e-8
            if m >= model.ee_frame or j.type == P.PRISMATIC:
                assert not Ja[:, m].any()
    if name == "slider4":
        assert sum(j.type == P.PRISMATIC for j in model.joints) == 2


def test_spd6_solve_against_numpy():
    rng = np.random.default_rng(4)
    B = rng.normal(size=(50, 6, 9))
    M = B @ np.swapaxes(B, -1, -2) + 1e-4 * np.eye(6)
    e = rng.normal(size=(50, 6))
    want = np.linalg.solve(M, e[..., None])[..., 0]
    got = spd6_solve(M, e)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    lower = M.copy()
    lower[..., np.tril_indices(6, -1)[0], np.tril_indices(6, -1)[1]] = np.nan      # only the upper triangle is read
    assert np.array_equal(spd6_solve(lower, e), got)
    # nearly singular: rank 2 plus the damping alone
    B = rng.normal(size=(6, 2))
    M = B @ B.T + 1e-4 * np.eye(6)
    assert np.abs(M @ spd6_solve(M, e[0]) - e[0]).max() <= 1e-9


@pytest.mark.parametrize("name", P.ARMS)
def test_weight_to_zero_reproduces_ik_step(name):
    """With L -> 0 the angular rows vanish from J6 and e6: the update is ik_step's to rounding"""
    model, twin = IK.arm(name)
    rng = np.random.default_rng(5)
    q = np.stack([random_q(model, rng) for _ in range(16)])
    R_goal, g = twin.end_effector_frame(np.stack([random_q(model, rng) for _ in range(16)]))
    c = IK.twin_constants(model)
    want = twin.ik_step(q, g, **c)
    for mode, goal in ((ORIENT_FULL, R_goal), (ORIENT_AXIS, R_goal @ P.TOOL_AXIS)):
        got = twin.ik_pose_step(q, g, mode, goal, weight=1e-12, w_max=0.5, **c)
        assert np.abs(got - want).max() <= 1e-10, np.abs(got - want).max()


def test_quaternion_matrix_and_orientation_goal():
    rng = np.random.default_rng(6)
    for _ in range(10):
        u, theta = unit(rng.normal(size=3)), rng.uniform(0, np.pi)
        quat = 2.5 * np.concatenate([np.sin(theta / 2) * u, [np.cos(theta / 2)]])      # (x, y, z, w), any length
        R = quaternion_matrix(quat)
        assert R.dtype == np.float32 and np.abs(R - axis_rotation(u, theta)).max() <= 1e-7
    assert np.array_equal(quaternion_matrix([0, 0, 0, 1]), np.eye(3, dtype=np.float32))
    assert orientation_goal(3) is None
    og = orientation_goal(3, approach_directions=[0, 0, -2.0], tolerance=1e-3, orientation_tolerance=2e-3)
    assert og.mode == ORIENT_AXIS and og.goals.dtype == np.float32 and np.array_equal(og.goals, np.tile([0, 0, -1], (3, 1)))
    assert og.angle_length == 0.5 and np.array_equal(og.tool_axis, [0, 0, 1]) and abs(float(og.tool_normal @ og.tool_axis)) == 0.0
    og = orientation_goal(2, orientations=[[0, 0, 0, 1], [0, 0, np.sin(0.3), np.cos(0.3)]])
    assert og.mode == ORIENT_FULL and og.goals.shape == (2, 9) and np.array_equal(og.goals[0], np.eye(3).reshape(9))
    assert np.abs(og.goals[1].reshape(3, 3) - axis_rotation(np.array([0, 0, 1.0]), 0.6)).max() <= 1e-7
    for kw, match in ((dict(orientations=[0, 0, 0, 1], approach_directions=[0, 0, 1]), "one of them"),
                      (dict(orientations=np.zeros((2, 4))), "got shape"), (dict(orientations=np.zeros((3, 3))), "got shape"),
                      (dict(approach_directions=np.zeros(4)), "got shape"), (dict(approach_directions=np.zeros((2, 3))), "got shape"),
                      (dict(orientations=[[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 0]]), r"orientations\[2\] has length 0"),
                      (dict(approach_directions=[[0, 0, 1], [0, np.nan, 0], [0, 0, 1]]), r"approach_directions\[1\] is not finite"),
                      (dict(approach_directions=[0, 0, 0]), r"approach_directions\[0\] has length 0"),
                      (dict(approach_directions="down"), "not an array of numbers"),
                      (dict(approach_directions=[0, 0, 1], tool_axis=[0, 0, 0]), r"tool_axis\[0\] has length 0"),
                      (dict(approach_directions=[0, 0, 1], tool_axis=[0, 0, np.inf]), "tool_axis.* is not finite"),
                      (dict(approach_directions=[0, 0, 1], tool_axis=[0, 1]), r"tool_axis is \[3\]"),
                      (dict(approach_directions=[0, 0, 1], orientation_tolerance=0.0), "orientation_tolerance"),
                      (dict(approach_directions=[0, 0, 1], orientation_tolerance=float("nan")), "orientation_tolerance")):
        with pytest.raises(ValueError, match=match):
            orientation_goal(3, **kw)


def test_selection_on_merit_against_brute_force():
    """select_goal_pose fed merit in the place of residual against a loop that spells the rule out"""
    rng = np.random.default_rng(7)
    N, R, tol = 200, 8, np.float32(1e-3)
    residual = (10.0 ** rng.uniform(-5, -1, (N, R))).astype(np.float32)
    angle = (10.0 ** rng.uniform(-5, -1, (N, R))).astype(np.float32)
    merit = np.maximum(residual, angle * np.float32(P.ANGLE_LENGTH))
    jd = rng.uniform(0, 2, (N, R)).astype(np.float32)
    jd[:, 3] = jd[:, 1]                                          # ties go to the lower r
    clear, self_clear, cell = (rng.uniform(-0.05, 0.2, (N, R)).astype(np.float32) for _ in range(3))
    choice, cls = select_goal_pose(merit, jd, clear, self_clear, cell, tol)
    for n in range(N):
        keys = []
        for r in range(R):
            conv = residual[n, r] <= tol and angle[n, r] * np.float32(P.ANGLE_LENGTH) <= tol
            free = clear[n, r] >= 0 and self_clear[n, r] >= 0 and cell[n, r] >= 0
            k = (0 if free else 1) if conv else 2
            keys.append((k, float(merit[n, r]) if k == 2 else float(jd[n, r]), r))
        best = min(keys)
        assert (choice[n], cls[n]) == (best[2], best[0])
    assert set(np.unique(cls)) == {0, 1, 2}
    out = gather_goal_poses(choice, cls, np.zeros((N, R, 3)), residual, clear, self_clear, cell, jd, tol, angle, merit)
    assert np.array_equal(out.converged_restarts, np.sum(merit <= tol, axis=1))
    assert np.array_equal(out.angle_residual, angle[np.arange(N), choice]) and np.array_equal(out.reachable, cls <= 1)
    assert out._replace(restart=out.restart).angle_residual is out.angle_residual


# ---- the rehearsal: the float32 restatement in the kernel's place ---------------------------------------------------------------------
_REHEARSED = {}


def rehearse(name, N, R, mode):
    """(case, the restatement's answer, largest single-step deviation, share left out, largest angle deviation over every recorded
    pose); computed once per case"""
    key = (name, N, R, mode)
    if key not in _REHEARSED:
        case = P.build_case(name, N, R, mode)
        got = P.solve32(case)
        dev, out = P.check_iterations(case, got["iters"])
        g, goal = P.goals_of(case)
        angle_dev = 0.0
        for q in got["iters"]:
            _, a32, _ = P.errors32(case.model, q, g, mode, goal)
            _, a64 = case.twin.pose_errors(q.astype(np.float64), g, mode, goal, P.TOOL_AXIS, P.TOOL_NORMAL)
            angle_dev = max(angle_dev, float(np.abs(a32 - a64).max()))
        _REHEARSED[key] = (case, got, dev, out, angle_dev)
    return _REHEARSED[key]


@pytest.mark.parametrize("name,N,R,mode", P.CASES)
def test_rehearsal(name, N, R, mode):
    """Every case of the GPU suite with the float32 restatement (chain_ik_pose_common.ik_pose_step32) in the kernel's place and the
    twin's clearances rounded to float32 in the probes': the same checks, so the band shares and the populated classes hold before
    a GPU is involved, and every query ends in the class it was built for."""
    case, got, dev, out, angle_dev = rehearse(name, N, R, mode)
    print(f"{name} N={N} R={R} mode={mode}: single-step deviation {dev:.2e} (STEP_DEVIATION {P.STEP_DEVIATION:.2e}), left out {out:.4f}, "
          f"angle deviation {angle_dev:.2e} (ANGLE_DEVIATION {P.ANGLE_DEVIATION:.2e})")
    assert dev <= P.STEP_DEVIATION and angle_dev <= P.ANGLE_DEVIATION and out <= P.CAP
    probe, cell = IK.probes32(case, got["q"])
    jd = joint_distance32(got["q"].reshape(N, R, -1), case.q_start[:, None, :]).reshape(-1)
    choice, cls = select_goal_pose(got["merit"].reshape(N, R), jd.reshape(N, R), probe[:, 3].reshape(N, R), probe[:, 4].reshape(N, R),
                                   cell.reshape(N, R), np.float32(P.TOLERANCE), np.float32(case.margin))
    P.check_solution(case, got, probe, cell, choice, cls, jd)
    assert np.array_equal(cls, case.want), (cls, case.want)
    _, _, _, twin_merit = case.twin_solution()
    assert np.array_equal((got["merit"].reshape(N, R) <= P.TOLERANCE).any(axis=1), (twin_merit <= P.TOLERANCE).any(axis=1))
    assert not ((twin_merit.min(axis=1) > P.TOLERANCE / 4) & (twin_merit.min(axis=1) <= P.TOLERANCE)).any()      # the recorded share: 0


def test_the_measured_deviations_are_the_constants():
    """STEP_DEVIATION and ANGLE_DEVIATION are the largest values the rehearsal measures over all its cases, rounded up by at most a
    quarter; the GPU bounds are 8 x them."""
    measured = {c: rehearse(*c)[2:] for c in P.CASES}
    step, angle = max(v[0] for v in measured.values()), max(v[2] for v in measured.values())
    print({c: (f"{v[0]:.2e}", f"{v[2]:.2e}") for c, v in measured.items()})
    assert 0.75 * P.STEP_DEVIATION <= step <= P.STEP_DEVIATION, step
    assert 0.75 * P.ANGLE_DEVIATION <= angle <= P.ANGLE_DEVIATION, angle
    assert P.STEP_BOUND == 8 * P.STEP_DEVIATION and P.ANGLE_BOUND == 8 * P.ANGLE_DEVIATION


# ---- the host path ----------------------------------------------------------------------------------------------------------------
def test_goal_poses_host_with_and_without_an_orientation_goal():
    """Without orientation arguments goal_poses_host is what it was, field for field, with angle_residual None; with them it is
    solve_ik_pose on the float32 goal, selected on merit, and the chosen poses point the tool where they were told to."""
    model, twin = IK.arm("iiwa_like7")
    rng = np.random.default_rng(8)
    N, R = 12, 8
    q_goal = IK.free_poses(model, twin, rng, N)
    R_goal, targets = twin.end_effector_frame(q_goal)
    q0 = np.tile([j.init for j in model.joints], (N, 1))
    obstacles = np.tile(C.away(model)[1], (N, 1))
    plain = goal_poses_host(twin, q0, targets, obstacles, restarts=R, seed=2)
    assert isinstance(plain, GoalPoses) and plain.angle_residual is None and len(plain) == 10 and len(GoalPoses._fields) == 10
    # today's path, spelled out
    q32, t32, o32 = C.f32(q0), C.f32(targets), C.f32(obstacles)
    seeds = ik_seeds(model, N, R, 2).astype(np.float64)
    seeds[:, 0] = q32
    q, residual = twin.solve_ik(t32[:, None, :], seeds, iterations=32)
    ob = np.broadcast_to(o32[:, None, :], q.shape[:-1] + (3,))
    clear = twin.clearance(q, ob) - twin.obstacle_radius
    self_clear, cell_clear = twin.self_clearance(q) + 0 * clear, twin.cell_clearance(q) + 0 * clear
    jd = joint_distance32(q, q32[:, None, :])
    choice, cls = select_goal_pose(residual, jd, clear, self_clear, cell_clear, 1e-3, 0.0)
    want = gather_goal_poses(choice, cls, q, residual, clear, self_clear, cell_clear, jd, 1e-3)
    for f, a, b in zip(GoalPoses._fields, plain, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), f
    for kw, mode, goal in ((dict(orientations=np.stack([quat_of(Rg) for Rg in R_goal])), ORIENT_FULL, None),
                           (dict(approach_directions=R_goal @ np.array([0.0, 1.0, 0.0]), tool_axis=[0, 2.0, 0]), ORIENT_AXIS, None)):
        out = goal_poses_host(twin, q0, targets, obstacles, restarts=R, iterations=64, seed=2, **kw)
        assert out.angle_residual is not None and out.reachable.mean() >= 0.75
        og = orientation_goal(N, tolerance=1e-3, orientation_tolerance=1e-3, **kw)
        assert og.mode == mode
        q, residual, angle, merit = twin.solve_ik_pose(t32[:, None, :], mode, og.goals.astype(np.float64)[:, None, :], seeds, og.angle_length,
                                                       tool_axis=og.tool_axis.astype(np.float64),
                                                       tool_normal=og.tool_normal.astype(np.float64), iterations=64)
        clear = twin.clearance(q, ob) - twin.obstacle_radius
        self_clear, cell_clear = twin.self_clearance(q) + 0 * clear, twin.cell_clearance(q) + 0 * clear
        jd = joint_distance32(q, q32[:, None, :])
        choice, cls = select_goal_pose(merit, jd, clear, self_clear, cell_clear, 1e-3, 0.0)
        want = gather_goal_poses(choice, cls, q, residual, clear, self_clear, cell_clear, jd, 1e-3, angle, merit)
        for f, a, b in zip(GoalPoses._fields, out, want):
            assert np.array_equal(a, b), f
        assert np.array_equal(out.angle_residual, want.angle_residual)
        R_got, ee = twin.end_effector_frame(out.joint_positions)
        ok = out.reachable
        assert np.all(np.linalg.norm(ee - t32, axis=1)[ok] <= 1e-3) and np.all(out.angle_residual[ok] <= 1e-3)
        if mode == ORIENT_FULL:
            assert np.abs(R_got - R_goal)[ok].max() <= 2e-3
        else:
            t, d = R_got @ np.array([0.0, 1.0, 0.0]), R_goal @ np.array([0.0, 1.0, 0.0])
            assert np.all(np.arccos(np.clip(np.sum(t * d, axis=1), -1, 1))[ok] <= 1e-3 + 1e-6)


def quat_of(R):
    """(x, y, z, w) of a rotation matrix by its largest component"""
    tr = np.trace(R)
    forms = [np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], 1.0 + tr]),
             np.array([1.0 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]]),
             np.array([R[0, 1] + R[1, 0], 1.0 + R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]]),
             np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]])]
    quat = forms[int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))]
    return quat / np.linalg.norm(quat)


# ---- through the façade ---------------------------------------------------------------------------------------------------------------
def test_facade_orientation_arguments_and_refusals():
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    f = framework(workcell_boxes=IK.BX.boxes_of("iiwa_like7"))
    twin = f.env
    rng = np.random.default_rng(9)
    N = 6
    q_goal = IK.free_poses(twin.model, twin, rng, N)
    R_goal, targets = twin.end_effector_frame(q_goal)
    directions = R_goal @ np.array([0.0, 0.0, 1.0])
    out = f.solve_goal_poses(targets, approach_directions=directions, restarts=4, iterations=64, seed=5, on_device=False)
    want = goal_poses_host(twin, np.tile(twin.initial_joint_positions, (N, 1)), targets, np.tile(twin.obstacle_pos, (N, 1)), restarts=4,
                           iterations=64, seed=5, approach_directions=directions)
    for a, b in zip(out, want):
        assert np.array_equal(a, b)
    assert out.angle_residual is not None and np.array_equal(out.angle_residual, want.angle_residual) and out.reachable.sum() >= 4
    assert f.solve_goal_poses(targets, restarts=4, seed=5, on_device=False).angle_residual is None
    one = f.solve_goal_poses(targets[0], orientations=[0, 0, 0, 1], restarts=2, iterations=4, on_device=False)
    assert one.angle_residual.shape == (1,)
    # the paths lead to the poses the oriented solve returns with its defaults
    default = f.solve_goal_poses(targets, approach_directions=directions, seed=5, on_device=False)
    paths = f.plan_joint_paths(targets, approach_directions=directions, seed=5, candidates=2, resolution=0.1, on_device=False)
    ok = default.reachable
    assert ok.any() and np.array_equal(paths.outcome == "goal", ~ok) and np.array_equal(paths.goal[ok], C.f32(default.joint_positions[ok]))
    base = dict(targets=np.zeros((4, 3)) + [0.4, 0.2, 0.5], on_device=False)
    for kw, match in ((dict(orientations=[0, 0, 0, 1], approach_directions=[0, 0, 1]), "one of them"),
                      (dict(orientations=np.zeros((4, 3))), "orientations is"), (dict(orientations=np.ones((3, 4))), "orientations is"),
                      (dict(approach_directions=np.ones((4, 4))), "approach_directions is"),
                      (dict(approach_directions=np.ones(2)), "approach_directions is"),
                      (dict(orientations=[[0, 0, 0, 1]] * 3 + [[0, np.inf, 0, 1]]), r"orientations\[3\] is not finite"),
                      (dict(approach_directions=[[0, 0, 1]] * 2 + [[np.nan, 0, 1]] + [[0, 0, 1]]), r"approach_directions\[2\] is not finite"),
                      (dict(orientations=[[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1]]), r"orientations\[1\] has length 0"),
                      (dict(approach_directions=[0, 0, 0]), r"approach_directions\[0\] has length 0"),
                      (dict(approach_directions=[0, 0, 1], tool_axis=[0, 0, 0]), "tool_axis.*length 0"),
                      (dict(approach_directions=[0, 0, 1], tool_axis=[1, 0]), r"tool_axis is \[3\]"),
                      (dict(approach_directions=[0, 0, 1], orientation_tolerance=0.0), "orientation_tolerance is a positive angle"),
                      (dict(approach_directions=[0, 0, 1], orientation_tolerance="fine"), "orientation_tolerance"),
                      (dict(approach_directions=[0, 0, 1], orientation_weight=-1.0), "orientation_weight"),
                      (dict(approach_directions=[0, 0, 1], orientation_weight=float("nan")), "orientation_weight")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.solve_goal_poses(**dict(base, **kw))
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.plan_joint_paths(**dict(base, **kw))
    with pytest.raises(InvalidEnvironmentParameter, match="goal_joint_positions=.* is given the goal poses themselves"):
        f.plan_joint_paths(goal_joint_positions=q_goal, approach_directions=[0, 0, -1], on_device=False)
    # orientation arguments that ask for nothing are no orientation goal
    assert f.plan_joint_paths(goal_joint_positions=q_goal[:2], tool_axis=[1, 0, 0], candidates=1, resolution=0.2,
                              on_device=False).outcome.shape == (2,)


def test_reach_targets_with_an_orientation_goal_against_a_stub_agent(monkeypatch):
    import torch
    from robotic_manipulator_rloa_amd.engine import ReachResult
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # the goal poses come from the twin
    f = framework()
    twin = f.env
    rng = np.random.default_rng(4)
    N, F = 4, 5
    goals = IK.free_poses(twin.model, twin, rng, N)
    R_goal, targets = twin.end_effector_frame(goals)
    directions = R_goal @ np.array([0.0, 0.0, 1.0])
    start = np.tile(twin.initial_joint_positions, (N, 1))

    class Agent:
        state_size, action_size, seed, world_size = 23, 7, 0, 1
        calls = []

        def rollout_vectorized(self, chain, targets, obstacles, q0, **kw):
            self.calls.append(kw)
            z = np.zeros(N, np.float32)
            s = np.linspace(0.0, 1.0, F + 1)[None, :, None]
            paths = (q0[:, None, :] + s * (goals - q0)[:, None, :]).astype(np.float32)
            return ReachResult(np.array(["reached"] * N), np.full(N, F), z, z, z, z, paths, z, z, z, z, z)

    f.naf_agent = Agent()
    with pytest.raises(InvalidEnvironmentParameter, match="needs goal_poses=True or joint_paths=True"):
        f.reach_targets(targets, initial_joint_positions=start, frames=F, approach_directions=directions)
    assert not Agent.calls
    with pytest.raises(InvalidEnvironmentParameter, match=r"approach_directions\[1\] is not finite"):
        f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True,
                        approach_directions=[[0, 0, 1], [0, np.nan, 1], [0, 0, 1], [0, 0, 1]])
    assert not Agent.calls                                                   # refused before the rollout
    plain = f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True)
    out = f.reach_targets(targets, initial_joint_positions=start, frames=F, goal_poses=True, approach_directions=directions)
    assert Agent.calls[-1] == Agent.calls[-2]                                # the rollout is called as it was: its outcome is positional
    assert np.array_equal(out.outcome, plain.outcome) and plain.goal.angle_residual is None
    want = f.solve_goal_poses(targets, initial_joint_positions=start, approach_directions=directions)
    for a, b in zip(out.goal, want):
        assert np.array_equal(a, b)
    assert np.array_equal(out.goal.angle_residual, want.angle_residual)
    both = f.reach_targets(targets, initial_joint_positions=start, frames=F, joint_paths=True, approach_directions=directions)
    ok = want.reachable
    assert np.array_equal(both.path.goal[ok], C.f32(want.joint_positions[ok]))      # (a path's poses are float32 values)


# ---- plumbing --------------------------------------------------------------------------------------------------------------------
def test_header_symbol_struct_and_argument_errors():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40
    name = "naf_chain_ik_solve_pose"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h,", text, re.M) and name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 16
    assert ctypes.sizeof(_lib.IkPoseParams) == 36 and re.search(r"\}\s*naf_chain_ik_pose_params_t;", text)
    assert "Orientation is no goal;" not in text
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40
    # argument errors are host code and launch nothing: a fake non-null handle is never dereferenced before they answer
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    f3 = ctypes.c_float * 3
    ok, pose = _lib.IkParams(64, 0.01, 0.3, 0.5), _lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, 0, 1), f3(1, 0, 0))
    names = ("h", "targets", "goals", "mode", "q_start", "seeds", "N", "R", "prm", "pose", "q", "residual", "angle", "merit")
    good = dict(h=p, targets=p, goals=p, mode=0, q_start=p, seeds=p, N=1, R=1, prm=ok, pose=pose, q=p, residual=p, angle=p, merit=p)
    bad = [{k: None} for k in ("h", "targets", "goals", "q_start", "seeds", "q", "residual", "angle", "merit")]
    bad += [dict(N=0), dict(N=-3), dict(R=0), dict(R=3), dict(R=128), dict(mode=2), dict(mode=-1)]
    bad += [dict(prm=_lib.IkParams(*v)) for v in ((0, 0.01, 0.3, 0.5), (64, float("nan"), 0.3, 0.5), (64, 0.0, 0.3, 0.5),
                                                  (64, 0.01, float("inf"), 0.5), (64, 0.01, 0.3, -1.0))]
    for v in ((0.0, 0.5, 1.0), (float("nan"), 0.5, 1.0), (0.2, 0.0, 1.0), (0.2, float("inf"), 1.0), (0.2, 0.5, 0.0), (0.2, 0.5, -1.0),
              (0.2, 0.5, float("nan"))):
        bad.append(dict(pose=_lib.IkPoseParams(*v, f3(0, 0, 1), f3(1, 0, 0))))
    bad.append(dict(pose=_lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, float("nan"), 1), f3(1, 0, 0))))
    bad.append(dict(pose=_lib.IkPoseParams(0.2, 0.5, 1.0, f3(0, 0, 1), f3(1, float("inf"), 0))))
    for change in bad:
        a = dict(good, **change)
        assert lib.naf_chain_ik_solve_pose(*[a[k] for k in names], None, None) == NAF_ERR_ARG, change
    assert not buf.any()

"""CPU (`-m "not gpu"`): trajectories as demonstrations. The rule of environment/tick_demo.py on random polylines
against its derived tracking bound; kinematic.demonstration_rows_host generalised over the action source, bit-equal on every old
case; the tick cases of chain_ticks_common rehearsed with chain_demo_common's float32 restatement; the refusals, and
plan_trajectories -> demonstrate_trajectories through the twin."""
import json
import os
import re

import numpy as np
import pytest

import chain_demo_common as D
import chain_legs_common as L
import chain_ticks_common as X
import chain_traj_common as TC
from test_chain_ik_cpu import framework

from robotic_manipulator_rloa_amd.environment import tick_demo as K
from robotic_manipulator_rloa_amd.environment.edge_certificate import polyline_nodes
from robotic_manipulator_rloa_amd.environment import trajectory as T
from robotic_manipulator_rloa_amd.environment.kinematic import DEMO_MAX_TICKS, demonstration_rows_host, reach_table
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_LEG_CASES = [(name, N, T_cap) for name in D.ARMS for N, T_cap in D.COUNTS] + D.EXTRA      # test_chain_demo_gpu.CASES
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_ticks_refusals.json")
ARGUMENT_ERRORS = (dict(h=None), dict(q=None), dict(a=None), dict(n=None), dict(t=None), dict(o=None), dict(rows=None), dict(rec=None),
                   dict(N=0), dict(N=-3), dict(T=0), dict(T=1025), dict(T=-64), dict(rf=None), dict(rf=0), dict(rad=float("nan")),
                   dict(rad=float("inf")), dict(rad=-0.01))


class _NoCheck:
    """plan_trajectories' backend for trajectories nobody checks: the schedule is all the rule reads"""
    dtype = np.float64

    def records(self, ds, obstacles, S, margin, certify, positions):
        rec = np.zeros((len(ds.n_nodes), T.TRAJ_CERT_FLOATS if certify else T.TRAJ_FLOATS))
        rec[:, 3] = -1
        return rec, None


def random_trajectories(speed, count=300, seed=0):
    """Trajectories of `count` random polylines of 1 .. 5 legs in +-2.5 rad on 1 .. 7 joints (test_chain_traj_cpu's generator with
    the issue's ranges), grouped by joint count; max_velocity = speed, max_acceleration 4"""
    rng = np.random.default_rng(seed)
    polys = {}
    for _ in range(count):
        A, legs = int(rng.integers(1, 8)), int(rng.integers(1, 6))
        polys.setdefault(A, []).append(rng.uniform(-2.5, 2.5, (legs + 1, A)))
    out = []
    for A, ps in sorted(polys.items()):
        nodes, n_nodes = np.full((len(ps), 6, A), np.nan), np.array([len(p) for p in ps])
        for n, p in enumerate(ps):
            nodes[n, :len(p)] = p
        out.append(T.plan_trajectories(_NoCheck(), nodes, n_nodes, np.zeros((len(ps), 3)), np.full(A, speed), np.full(A, 4.0), 1.0 / 40.0,
                                       positions=False))
    return out


def independent_bound_and_error(traj, plan):
    """(bound[N], error[N]) formed HERE from the law and the table alone, not from the plan's diagnostics: the float32 recurrence
    under plan.actions restated (chain_demo_common.poses32's step), a tick counted as clamped iff the unclamped quotient
    (Q_{i+1} - p_i) / dt32 leaves [-1, 1], max |q| over the recurrence's poses and the law's, r = 1/2 ulp32(max |q|) + 1/2 DT ulp32(1)"""
    N, T, A = plan.actions.shape
    Q = np.asarray(traj.at(np.arange(T + 1) * DT), np.float64)
    last = np.asarray(traj.nodes, np.float64)[np.arange(N), np.asarray(traj.n_nodes) - 1]
    Q = np.where((np.arange(T + 1)[None, :] >= plan.planned_ticks[:, None])[..., None], last[:, None, :], Q)
    dt32 = np.float64(np.float32(DT))
    p = plan.q_start.copy()
    err, scale = np.abs(p - Q[:, 0]).max(axis=1), np.maximum(np.abs(p).max(axis=1), np.abs(Q[:, 0]).max(axis=1))
    run, longest = np.zeros(N, np.int64), np.zeros(N, np.int64)
    for i in range(T):
        live = i < plan.rows
        want = ((Q[:, i + 1] - p.astype(np.float64)) / dt32).astype(np.float32)
        run = np.where(live & (np.abs(want) > 1.0).any(axis=1), run + 1, 0)
        longest = np.maximum(longest, run)
        p = (dt32 * plan.actions[:, i].astype(np.float64) + p.astype(np.float64)).astype(np.float32)
        err = np.where(live, np.maximum(err, np.abs(p - Q[:, i + 1]).max(axis=1)), err)
        scale = np.where(live, np.maximum(scale, np.maximum(np.abs(p).max(axis=1), np.abs(Q[:, i + 1]).max(axis=1))), scale)
    r = 0.5 * np.spacing(scale.astype(np.float32)).astype(np.float64) + 0.5 * DT * float(np.spacing(np.float32(1.0)))
    return r * (1.0 + longest), err


# ---- 1. the rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("speed", [0.5, 1.0])
def test_tick_plan_tracks_within_the_derived_bound(speed):
    """300 random polylines at max_velocity 0.5 and 1.0, frames = 1024: per query tracking_error <= r (1 + longest saturated run),
    r = 1/2 ulp32(max |q|) + 1/2 DT ulp32(1); no saturated tick at 0.5; |a| <= 1 everywhere; the open-loop form is worse than the
    feedback on every query at 0.5. Measured here (NOTEBOOK §42): at 0.5 no saturated tick, worst error 1.19e-7, open loop 1.2e-4;
    at 1.0 the cruise ticks saturate (at unit speed any lag behind the law asks for more than 1), runs up to 509, worst
    error 5.7e-6, open loop 7.8e-5."""
    worst = dict(feedback=0.0, open_loop=0.0, share=0.0, saturated=0, run=0, ticks=0)
    for traj in random_trajectories(speed):
        fb, ol = K.trajectory_tick_plan(traj, DEMO_MAX_TICKS, True), K.trajectory_tick_plan(traj, DEMO_MAX_TICKS, False)
        bound, err = independent_bound_and_error(traj, fb)
        assert np.all(err <= bound), float((err / bound).max())
        assert np.array_equal(err, fb.tracking_error) and np.all(K.tracking_bound(fb) == bound)      # ... and the plan reports the same
        assert np.abs(fb.actions).max() <= 1.0 and np.abs(ol.actions).max() <= 1.0 and np.all(fb.peak_action <= 1.0)
        assert np.array_equal(fb.planned_ticks, np.maximum(1, np.ceil(traj.duration / DT))) and np.array_equal(fb.rows, np.minimum(fb.planned_ticks, 1024))
        assert np.array_equal(fb.q_start, traj.nodes[:, 0].astype(np.float32))
        if speed == 0.5:
            assert not fb.saturated_ticks.any() and np.all(ol.tracking_error > fb.tracking_error)
        worst["feedback"], worst["open_loop"] = max(worst["feedback"], fb.tracking_error.max()), max(worst["open_loop"], ol.tracking_error.max())
        worst["share"] = max(worst["share"], float((fb.tracking_error / bound).max()))
        worst["saturated"] += int(fb.saturated_ticks.sum())
        worst["run"], worst["ticks"] = max(worst["run"], int(fb.saturated_run.max())), worst["ticks"] + int(fb.rows.sum())
    print(f"max_velocity {speed}: worst tracking error {worst['feedback']:.3g} ({worst['share']:.3f} of its bound), open loop "
          f"{worst['open_loop']:.3g}; {worst['saturated']} of {worst['ticks']} ticks saturated, longest run {worst['run']}")


def test_tick_plan_ends_none_queries_and_refusals():
    """Q at and beyond D is P_K: a trajectory shorter than the budget arrives and stays (the last actions are 0 to a rounding); a
    query without a trajectory stands still for one tick; the refusals name what they refuse."""
    model, twin = D.arm("planar3")
    nodes = np.full((3, 3, 3), np.nan)
    nodes[0, :3] = [[0.0, 0.1, 0.2], [0.3, 0.5, 0.1], [0.2, 0.2, 0.2]]
    nodes[2, :1] = [[0.1, 0.1, 0.1]]
    traj = T.plan_trajectories(_NoCheck(), nodes, np.array([3, 0, 1]), np.zeros((3, 3)), np.ones(3), np.full(3, 4.0), DT, positions=False)
    plan = K.trajectory_tick_plan(traj, 400, True, twin.joint_limits(), np.array([0.5, 0.4, 0.3]))
    assert plan.planned_ticks.tolist() == [int(np.ceil(traj.duration[0] / DT)), 1, 1] and plan.rows.tolist() == plan.planned_ticks.tolist()
    assert np.array_equal(plan.q_start[1], np.float32([0.5, 0.4, 0.3])) and not plan.actions[1:].any()
    assert plan.tracking_error[0] <= K.tracking_bound(plan)[0] and plan.tracking_error[1] == 0.0
    short = K.trajectory_tick_plan(traj, 7)
    assert short.rows.tolist() == [7, 1, 1] and short.actions.shape == (3, 7, 3) and short.planned_ticks[0] == plan.planned_ticks[0]
    for kw, match in ((dict(frames=0), "frames is a number of steps from 1 to 1024"), (dict(frames=1025), "frames is a number"),
                      (dict(frames=True), "frames is a number"), (dict(limits=(np.zeros(2), np.ones(2))), "limits holds 2 joints"),
                      (dict(stand_still=np.zeros(4)), "stand_still holds 4 joints")):
        with pytest.raises(ValueError, match=match):
            K.trajectory_tick_plan(traj, **kw)
    fast = T.plan_trajectories(_NoCheck(), nodes, np.array([3, 0, 1]), np.zeros((3, 3)), np.array([1.0, 1.5, 1.0]), np.full(3, 4.0), DT,
                               positions=False)
    with pytest.raises(ValueError, match=r"query 0 moves joint 1 at 1\.\d+ per second, above the unit action"):
        K.trajectory_tick_plan(fast, 400)


# ---- 2. one body for both action sources -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [("demo",) + c for c in TWO_LEG_CASES] + [("legs",) + c for c in L.CASES])
def test_rows_host_is_the_same_for_a_tick_plan_of_the_same_actions(case_id):
    """On every case of chain_demo_common and chain_legs_common, demonstration_rows_host of the TickPlan that holds
    demo_actions(plan, T_cap) and the sum of the counts gives records, rows and poses bit-equal to the plan's own call."""
    case = D.build_case(*case_id[1:]) if case_id[0] == "demo" else L.build_case(*case_id[1:])
    want = case.host()
    got = demonstration_rows_host(case.twin, K.tick_plan_of(case.plan, case.T_cap), case.targets, case.obstacles, case.T_cap, full=True)
    for a, b in zip(want[0][:8], got[0][:8]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert want[0].rows.tobytes() == got[0].rows.tobytes() and want[0].rows_total == got[0].rows_total
    for a, b in zip(want[1:], got[1:]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 3. the tick cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,T_cap", X.CASES)
def test_rehearsal(name, N, T_cap):
    """Every tick case through chain_demo_common's float32 restatement and its checks against the float64 rule (check_rows): at
    most CAP of the case's ticks inside a band ON THE RESTATEMENT, so that the GPU test's cap is one the oracle itself keeps; the
    restatement's poses are bit for bit the poses the rule predicted when it formed the actions, and within the derived tracking
    bound of the law clipped into the limits; from T_cap = lanes - 1 on every role ends as it is built to — a reach before the last
    planned tick, a touch after at least two rows, a cut, an end — and a limited arm's limit role holds a joint ON its limit for
    several ticks with the action still pushing; from T_cap = 130 on it does so at ticks lanes - 1 and lanes, across the boundary
    of the first two passes."""
    case = X.build_case(name, N, T_cap)
    rows, rec, poses = D.rows32(case)
    dev, inside, total = D.check_rows(case, rows, rec, poses)
    assert inside <= D.CAP * total
    tp = case.tick_plan
    _, want_poses, _ = K.tick_recurrence(tp.q_start, case.law, case.twin.joint_limits(), True)
    upto = np.arange(T_cap + 1)[None, :] <= tp.rows[:, None]
    assert np.array_equal(D.bits(np.where(upto[..., None], poses, 0)), D.bits(np.where(upto[..., None], want_poses, 0)))
    err = np.where(upto, np.abs(poses.astype(np.float64) - X.clipped_law(case)).max(axis=2), 0.0).max(axis=1)
    bound = X.device_tracking_bound(case)
    print(f"{name} N={N} T_cap={T_cap}: tracking error {err.max():.3g} (bound {bound.max():.3g}), saturated ticks {tp.saturated_ticks.tolist()}")
    assert np.all(err <= bound)
    assert np.array_equal(rec[:, 6], tp.planned_ticks) and np.abs(tp.actions).max() <= 1.0
    if T_cap >= X.ROLE_TICKS:
        assert np.all(X.ends_as_built(case.role, rec[:, 1]))
        assert np.all((rec[:, 0] < rec[:, 6])[case.role == 0]) and np.all(rec[:, 0][case.role == 1] >= 2)
        lanes = D.lanes_of(case.model)
        lo, hi = [v.astype(np.float32) for v in case.twin.joint_limits()]
        for n in np.flatnonzero(case.role == 4):
            if not any(j.limited for j in case.model.joints):
                continue
            held = ((poses[n, 1:] == hi) & (tp.actions[n] > 0)) | ((poses[n, 1:] == lo) & (tp.actions[n] < 0))
            live = np.arange(T_cap) < rec[n, 0]
            assert (held.any(axis=1) & live).sum() >= 3, (name, n)
            if T_cap >= X.LIMIT_TICKS:
                on = held.any(axis=1) & live
                assert on[lanes - 1] and on[lanes] and np.array_equal(on, X.held_on_limit(case)[n] & live), (name, n)


@pytest.mark.parametrize("name", X.BOUNDARY_NAMES)
def test_rehearsal_of_a_first_done_on_the_pass_boundary(name):
    """chain_ticks_common.boundary_case through the restatement: the four demonstrations end by reaching and by touching with
    exactly lanes - 1 and lanes valid rows — the first done walked by the last lane of pass 0 and by lane 0 of pass 1 — and no tick
    inside a band, so the device has to count the same."""
    case = X.boundary_case(name)
    lanes = D.lanes_of(case.model)
    rows, rec, poses = D.rows32(case)
    _, inside, _ = D.check_rows(case, rows, rec, poses)
    assert inside == 0 and rec[:, 0].tolist() == [lanes - 1, lanes, lanes - 1, lanes] and rec[:, 1].tolist() == [1, 1, 2, 2]


# ---- 4. refusals, and the twin end to end --------------------------------------------------------------------------------------------
def refusals(f, traj):
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    out = {}
    for key, kw in (("not trajectories", dict(trajectories=None)), ("frames 0", dict(frames=0)), ("frames 1025", dict(frames=1025)),
                    ("keep_contact", dict(keep_contact=1)), ("feedback", dict(feedback="yes")),
                    ("targets count", dict(targets=np.zeros((2, 3)))), ("obstacles", dict(obstacles=np.zeros((2, 3))))):
        with pytest.raises(InvalidEnvironmentParameter) as err:
            f.demonstrate_trajectories(**dict(dict(trajectories=traj, on_device=False), **kw))
            pytest.fail(f"{key}: not refused")
        out[key] = str(err.value)
    return out


def test_facade_on_the_host_and_its_refusals():
    """The facade's refusals are the golden strings; plan_trajectories -> demonstrate_trajectories(on_device=False) on the iiwa: a
    Demonstrations with the new trailing fields, 'none' where the trajectory is, planned_ticks = ceil(D / DT), tracking errors
    within the bound's order, and demonstrate_joint_paths leaves the new fields None."""
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.utils.exceptions import (ConfigurationIncomplete, EnvironmentNotInitialized,
                                                               InvalidEnvironmentParameter)
    f = ManipulatorFramework()
    with pytest.raises(EnvironmentNotInitialized):
        f.demonstrate_trajectories(None)
    f.initialize_synthetic_environment()
    with pytest.raises(ConfigurationIncomplete, match="PyBullet and the synthetic stand-in have no chain model"):
        f.demonstrate_trajectories(None)
    f = framework()
    twin = f.env
    rng = np.random.default_rng(4)
    goals = TC.IK.free_poses(twin.model, twin, rng, 3)
    paths = f.plan_joint_paths(goal_joint_positions=goals, candidates=4, resolution=0.05, seed=2, on_device=False)
    # paths planned without a roadmap hold no n_nodes: edge_certificate.polyline_nodes raised on them (IndexError) before this change
    assert paths.n_nodes is None and polyline_nodes(paths)[1].tolist() == np.where(paths.candidate >= 0, 3, 0).tolist()
    traj = f.plan_trajectories(paths, max_velocity=0.5, max_acceleration=4.0, on_device=False, positions=False)
    demos = f.demonstrate_trajectories(traj, frames=400, on_device=False)
    has = traj.outcome != "none"
    assert np.array_equal(demos.outcome == "none", ~has) and has.any() and "demonstrations" not in f.arm_planner.tools
    assert np.array_equal(demos.planned_ticks[has], np.ceil(traj.duration[has] / DT).astype(np.int64))
    assert demos.tracking_error.shape == demos.saturated_ticks.shape == demos.peak_action.shape == (3,)
    assert np.all(demos.tracking_error[has] <= 4e-7) and not demos.saturated_ticks.any() and np.all(demos.peak_action[has] <= 0.5 + float(np.spacing(np.float32(2.0))) / DT)      # (the feedback adds at most an ulp32 of a pose below 4 rad, per tick)
    assert demos.rows.dtype == np.float32 and demos.rows_total == demos.rows.shape[0] == int(demos.frames[demos.kept].sum())
    reached = demos.outcome == "reached"
    assert np.all(demos.frames[reached] <= demos.planned_ticks[reached]) and set(demos.outcome) <= {"reached", "end", "frames", "obstacle", "self", "workcell", "none"}
    old = f.demonstrate_joint_paths(paths, on_device=False)
    assert old.tracking_error is None and old.saturated_ticks is None and old.peak_action is None
    fast = f.plan_trajectories(paths, max_velocity=1.5, max_acceleration=4.0, on_device=False, positions=False)
    with pytest.raises(InvalidEnvironmentParameter, match="above the unit action"):
        f.demonstrate_trajectories(fast, on_device=False)
    with open(GOLDEN) as src:      # written by tests/golden/make_chain_ticks_refusals.py
        assert refusals(f, traj) == json.load(src)


def corner_framework():
    """planar3 without pairs or workcell behind the facade, a sphere of 1 cm: (framework, paths, obstacle[1, 3]) of a two-leg corner
    P_0 -> P_1 -> P_2 whose base joint sweeps 0.8 rad while the elbow folds to 1.0 rad and unfolds, given by hand as the JointPaths a
    one-via query returns. The sphere sits on the end effector of a pose MORE folded than any of the path (elbow 1.38 rad): the
    polyline keeps 2.5 cm from it and so does every blend, which is less folded than the corner. At 1 rad/s and 4 rad/s^2 the
    trajectory lasts 1.05 s, 253 ticks; at 0.5 rad/s 415 — both inside DEMO_MAX_TICKS, unlike chain_traj_common.corner_scene's slow
    one (3889)."""
    from test_chain_ik_cpu import ARM_TABLE, path
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.environment.kinematic import JointPaths
    ee, involved, fixed, init, var = ARM_TABLE["planar3"]
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(path("planar3"), ee, fixed, involved, [0.0, 0.0, 5.0], [0.0, 0.0, -5.0], init, var, link_radius=0.03,
                                       obstacle_radius=0.01, consider_autocollision=False)
    P = np.float32([[-0.4, 0.6, 0.0], [0.0, 1.0, 0.0], [0.4, 0.6, 0.0]]).astype(np.float64)
    nan, zero = np.full(1, np.nan), np.zeros(1, np.int64)
    paths = JointPaths(np.array(["via"]), zero, P[None, 1], nan, nan, nan, nan, nan, zero - 1, nan, zero, P[None, 0], P[None, 2],
                       np.zeros(1, bool), nan, zero)
    return f, paths, f.env.end_effector(np.array([0.0, 1.38, 0.0]))[None]


@pytest.mark.parametrize("speed", [1.0, 0.5])
def test_a_certified_corner_hands_its_minima_to_its_demonstration(speed):
    """plan_trajectories(certify=True) -> demonstrate_trajectories(on_device=False) on corner_framework, the target out of reach so
    that the demonstration runs to its last planned tick: the trajectory is 'certified', the demonstration ends 'end', is kept, and
    its minimum obstacle clearance is the trajectory's own to within (tracking bound + the trajectory's own pose bound) x the reach
    table's gain — the demonstration visits the law's ticks, where the trajectory took its minimum. The second term is
    chain_traj_common.POSE_BOUND: the trajectory evaluates its law on the float32 schedule at float32 tick times, the demonstration
    on the float64 law. Unconditional: nothing here depends on how the demonstration ended."""
    f, paths, ob = corner_framework()
    traj = f.plan_trajectories(paths, obstacles=ob, max_velocity=speed, max_acceleration=4.0, certify=True, clearance_margin=0.002,
                               on_device=False, positions=False)
    demos = f.demonstrate_trajectories(traj, targets=[0.0, 0.0, 5.0], obstacles=ob, frames=DEMO_MAX_TICKS, on_device=False)
    assert traj.outcome.tolist() == ["certified"] and traj.corner_deviation[0] == pytest.approx(speed ** 2 / 8.0, rel=1e-6)
    assert demos.outcome.tolist() == ["end"] and demos.kept.tolist() == [True]
    assert demos.frames[0] == demos.planned_ticks[0] == int(np.ceil(traj.duration[0] / DT)) <= DEMO_MAX_TICKS
    gain = float(reach_table(f.env.model).sum(axis=0).max())
    run = 0 if speed < 1.0 else int(demos.saturated_ticks[0])      # (the longest clamped run is at most the clamped ticks)
    slack = (float(K.tracking_radius(1.0)) * (1 + run) + TC.POSE_BOUND) * gain
    print(f"speed {speed}: clearance {demos.min_clearance[0]:.8f} against {traj.min_clearance[0]:.8f} (slack {slack:.3g}), tracking error "
          f"{demos.tracking_error[0]:.3g}, clamped ticks {int(demos.saturated_ticks[0])}")
    assert demos.tracking_error[0] <= float(K.tracking_radius(1.0)) * (1 + run)
    assert abs(demos.min_clearance[0] - traj.min_clearance[0]) <= slack
    assert np.isposinf(demos.min_self_clearance[0]) and np.isposinf(demos.min_cell_clearance[0])
    assert np.isposinf(traj.min_self_clearance[0]) and np.isposinf(traj.min_cell_clearance[0])


def test_a_blocked_corner_is_driven_into_the_sphere_and_dropped():
    """chain_traj_common.corner_scene blended at full speed: the trajectory is 'blocked', and its demonstration drives the law into
    the sphere beside the corner, ends 'obstacle' and is dropped whole."""
    model, twin, paths, ob = TC.corner_scene()
    c = TC.CORNER
    traj = T.trajectories_host(twin, paths, ob, np.full(3, c["fast"]), np.full(3, c["amax"]), DT, True, c["margin"], positions=False)
    plan = K.trajectory_tick_plan(traj, DEMO_MAX_TICKS, True, twin.joint_limits())
    target = twin.end_effector(np.asarray(traj.nodes[0, traj.n_nodes[0] - 1], np.float32).astype(np.float64))[None]
    demos = demonstration_rows_host(twin, plan, target, ob, DEMO_MAX_TICKS)
    assert traj.outcome.tolist() == ["blocked"] and demos.outcome.tolist() == ["obstacle"] and not demos.kept[0] and demos.rows_total == 0
    assert demos.frames[0] < demos.planned_ticks[0]


def test_header_symbol_and_writer_branch():
    """include/naf_hip.h declares the entry point in a block that names the rule; _lib binds it with the legs entry's arguments but
    K; README counts 109 entry points; DemonstrationWriter chooses the tick entry for a TickPlan only."""
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_ticks import TicksLaunch
    with open(os.path.join(ROOT, "include", "naf_hip.h")) as f:
        header = f.read()
    block = re.search(r"/\* Demonstrations under per-tick actions.*?naf_chain_demo_rows_ticks\(.*?\);", header, re.S).group(0)
    assert "environment/tick_demo.py" in block and "never read" in block and "NAF_CHAIN_ERR_LDS" in block
    legs = list(_lib._PROTOS["naf_chain_demo_rows_legs"])
    del legs[4]
    assert _lib._PROTOS["naf_chain_demo_rows_ticks"] == legs and len(_lib.EXPORTED_SYMBOLS) == 109
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "109 entry points, ABI 40" in f.read()

    class Writer(TicksLaunch):
        A = 3
        load = launch = load_legs = launch_legs = None
    w = Writer()
    case = D.build_case("planar3", 3, 130)
    assert w.entry_for(case.plan) == (None, None)
    tp = K.tick_plan_of(case.plan, 130)
    assert w.entry_for(tp) == (w.load_ticks, w.launch_ticks)
    for bad, match in ((tp._replace(planned_ticks=tp.planned_ticks * 0), "plans at least one tick"),
                       (tp._replace(actions=tp.actions[:, :5]), "the width of the table"),
                       (tp._replace(actions=tp.actions[..., :2]), r"actions\[N\]\[T\]\[3\]")):
        with pytest.raises(ValueError, match=match):
            w.entry_for(bad)

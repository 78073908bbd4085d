"""CPU: demonstrations along polylines of any number of legs and the shortcut round, through the twin alone — the K-leg plan and
demo_actions (environment/kinematic.py: demonstration_plan_legs), the rehearsal of every GPU case of tests/test_chain_legs_gpu.py
with chain_demo_common's float32 restatement in the kernel's place, the header / symbol / ABI / argument errors of
naf_chain_demo_rows_legs, shortcut_nodes and shortcut_round on chain_roadmap_common's value sets, and the façade on the host."""
import os
import re

import numpy as np
import pytest

import chain_demo_common as D
import chain_legs_common as L
import chain_roadmap_common as R
import chain_rollout_common as C
from conftest import ROOT
from test_chain_roadmap_cpu import planar_framework, same_paths

from robotic_manipulator_rloa_amd.environment.kinematic import (DEMO_MAX_LEGS, DemonstrationPlan, demo_actions, demonstration_plan,
                                                                demonstration_plan_legs, joint_distance32, joint_paths_host,
                                                                shortcut_nodes)
from robotic_manipulator_rloa_amd.environment.urdf_chain import DT


# ---- the plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,T_cap", [("iiwa_like7", 16, 256), ("planar3", 3, 130), ("slider4", 16, 256)])
def test_three_nodes_are_demonstration_plan_to_the_byte(name, N, T_cap):
    """demonstration_plan_legs on the three nodes start, via, goal is demonstration_plan on chain_demo_common's cases, field by field"""
    case = D.build_case(name, N, T_cap)
    for speed, frames in ((1.0, T_cap), (0.37, 400)):
        want = demonstration_plan(case.q_start, case.vias, case.q_goal, speed, frames)
        got = demonstration_plan_legs(np.stack([case.q_start, case.vias, case.q_goal], axis=1), np.full(N, 3), speed, frames)
        for f, a, b in zip(want._fields, got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f


def test_plan_of_polylines_padding_speed_and_rows():
    """legs behind a query's last are 0 ticks at action 0, every real leg takes at least one tick under the per-leg rule, a
    zero-length leg is one tick at action 0, |a|_inf <= speed, rows = min(sum, frames); the refusals"""
    rng = np.random.default_rng(11)
    N, K, A = 12, 7, 5
    nodes = np.cumsum(rng.uniform(-0.3, 0.3, (N, K, A)), axis=1).astype(np.float32)
    count = rng.integers(2, K + 1, N)
    count[0], count[1] = 2, K
    nodes[2, 1] = nodes[2, 0]                                  # a zero-length first leg
    padded = nodes.copy()
    padded[np.arange(K)[None, :] >= count[:, None]] = np.nan
    for speed, frames in ((1.0, 400), (0.5, 64)):
        plan = demonstration_plan_legs(padded, count, speed, frames)
        assert isinstance(plan, DemonstrationPlan) and plan.n_ticks.dtype == np.int32 and plan.leg_actions.dtype == np.float32
        assert plan.n_ticks.shape == (N, K - 1) and plan.leg_actions.shape == (N, K - 1, A) and plan.q_start.dtype == np.float32
        real = np.arange(K - 1)[None, :] < count[:, None] - 1
        assert np.all(plan.n_ticks[real] >= 1) and np.all(plan.n_ticks[~real] == 0) and np.all(plan.leg_actions[~real] == 0.0)
        assert np.abs(plan.leg_actions).max() <= np.float32(speed) and np.all(np.isfinite(plan.leg_actions))
        assert plan.n_ticks[2, 0] == 1 and np.all(plan.leg_actions[2, 0] == 0.0)
        assert np.array_equal(plan.rows, np.minimum(plan.n_ticks.sum(axis=1), frames)) and np.array_equal(plan.q_start, nodes[:, 0])
        for l in range(K - 1):
            L_l = joint_distance32(nodes[:, l + 1], nodes[:, l]).astype(np.float64)
            n = np.maximum(1, np.ceil(L_l / (speed * DT)))
            got = plan.n_ticks[:, l]
            assert np.all(((got == n) | (got == n + 1))[real[:, l]])
            moved = got[:, None] * DT * plan.leg_actions[:, l].astype(np.float64)
            assert np.abs(moved - (nodes[:, l + 1].astype(np.float64) - nodes[:, l]))[real[:, l]].max() <= 4e-7
        # what lies behind n_nodes is not read: other values there give the same plan
        again = demonstration_plan_legs(nodes, count, speed, frames)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan, again))
    assert DEMO_MAX_LEGS == 63
    for bad in (np.full(N, 1), np.full(N, K + 1), np.full(N, 2.0), np.full(N - 1, 2)):
        with pytest.raises(ValueError, match="n_nodes"):
            demonstration_plan_legs(padded, bad, 1.0, 400)
    with pytest.raises(ValueError, match="n_nodes"):
        demonstration_plan_legs(np.zeros((1, 66, A), np.float32), np.array([65]), 1.0, 400)
    assert demonstration_plan_legs(np.zeros((1, 66, A), np.float32), np.array([64]), 1.0, 400).n_ticks.sum() == 63
    with pytest.raises(ValueError, match="speed"):
        demonstration_plan_legs(padded, count, 0.0, 400)
    with pytest.raises(ValueError, match="frames"):
        demonstration_plan_legs(padded, count, 1.0, 1025)
    with pytest.raises(ValueError, match="not finite"), np.errstate(invalid="ignore"):
        demonstration_plan_legs(padded, np.full(N, K), 1.0, 400)          # a NaN node inside n_nodes


def test_demo_actions_follows_the_cumulative_ends():
    """On two-leg plans demo_actions is what it was — leg 1 for t < n1, leg 2 after, past the end too; on a K-leg plan tick t takes
    leg min(K_n - 1, #{l : e_l <= t}): several switches within a few ticks, and the padding is never taken"""
    case = D.build_case("iiwa_like7", 16, 256)
    plan, T = case.plan, 300
    first = (np.arange(T)[None, :] < plan.n_ticks[:, :1])[..., None]
    old = np.where(first, plan.leg_actions[:, None, 0, :], plan.leg_actions[:, None, 1, :]).astype(np.float64)
    got = demo_actions(plan, T)
    assert got.dtype == np.float64 and got.tobytes() == old.tobytes()
    A = 2
    acts = np.arange(1, 13, dtype=np.float32).reshape(1, 6, 2) / 16
    acts = np.concatenate([acts, acts], axis=0)
    ticks = np.array([[3, 1, 1, 2, 0, 0], [1, 1, 1, 1, 1, 4]], np.int32)
    acts[0, 4:] = 0.0
    plan = DemonstrationPlan(np.zeros((2, A), np.float32), acts, ticks, ticks.sum(axis=1))
    legs0 = [0, 0, 0, 1, 2, 3, 3, 3, 3, 3, 3, 3]               # past the last tick: the last REAL leg, not the padding
    legs1 = [0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 5, 5]
    got = demo_actions(plan, 12)
    assert got.shape == (2, 12, A)
    assert np.array_equal(got[0], acts[0, legs0].astype(np.float64)) and np.array_equal(got[1], acts[1, legs1].astype(np.float64))
    assert demo_actions(plan, 0).shape == (2, 0, A)


# ---- the cases and the rehearsal -------------------------------------------------------------------------------------------------
MEASURED = {}


@pytest.mark.parametrize("name,N,K,T_cap", L.CASES)
def test_rehearsal(name, N, K, T_cap):
    """Every GPU case with the float32 restatement in the kernel's place: the case builds with the twin alone — every demonstration
    ends as its role wants, no tick of it inside a band — and chain_demo_common's rows32 passes its check_rows as both stand; the
    deviation of the restatement's poses from the twin's stays within this module's own bound."""
    case = L.build_case(name, N, K, T_cap)
    _, rec, _, _ = case.host()
    assert case.plan.n_ticks.shape == (N, K) and np.all(case.plan.n_ticks[:, 0] >= 1)
    assert np.array_equal(rec[:, 1], [L.WANT[L.role_of(n, K)] for n in range(N)])
    dev, inside, total = D.check_rows(case, *D.rows32(case))
    MEASURED[(name, N, K, T_cap)] = dev
    assert inside == 0 and dev <= L.POSE_BOUND


def test_the_cases_hold_what_the_schedule_can_get_wrong():
    """Between them the cases hold: a switch strictly inside a pass and one on a pass boundary (lanes_of), two switches inside one
    pass with 1-tick legs one of which has zero length, a leg longer than a pass, a query of fewer legs than the launch's K, T_cap
    cutting inside a leg that is not the last, and demonstrations that end 'reached', in contact and 'end'; every one of the six
    kernel instantiations has a case."""
    found = set()
    for args in L.CASES:
        f = L.features(L.build_case(*args))
        print(args, sorted(f))
        found |= f
    assert found >= L.FEATURES, L.FEATURES - found
    assert {args[0] for args in L.CASES} == set(D.ARMS) | {name for name, _, _ in D.EXTRA} and len(D.ARMS) + len(D.EXTRA) == 6
    for name in D.ARMS:                                       # per arm: both kinds of switch, whatever its lanes
        per_arm = set().union(*(L.features(L.build_case(*a)) for a in L.CASES if a[0] == name))
        assert {"switch on a pass boundary", "switch inside a pass", "a leg longer than a pass"} <= per_arm, (name, per_arm)


def test_the_measured_deviation_is_the_constant():
    """POSE_DEVIATION is the rehearsal's largest measured deviation rounded up (by no more than a quarter), and the bound 8 x it"""
    for args in L.CASES:
        if args not in MEASURED:
            case = L.build_case(*args)
            MEASURED[args] = D.check_rows(case, *D.rows32(case))[0]
    worst = max(MEASURED.values())
    per_arm = {name: max(v for k, v in MEASURED.items() if k[0] == name) for name in sorted({k[0] for k in MEASURED})}
    print({k: f"{v:.2e}" for k, v in per_arm.items()})
    assert worst <= L.POSE_DEVIATION <= 1.25 * worst, (worst, L.POSE_DEVIATION)
    assert L.POSE_BOUND == 8 * L.POSE_DEVIATION


def test_split_two_leg_plan_keeps_the_actions():
    """the bench's and the GPU suite's way of turning a two-leg plan into K legs gives the same action at every tick"""
    case = D.build_case("iiwa_like7", 16, 256)
    rng = np.random.default_rng(0)
    for K in (2, 3, 8, 63):
        split = L.split_two_leg_plan(case.plan, K, rng)
        assert split.n_ticks.shape == (16, K) and np.array_equal(split.n_ticks.sum(axis=1), case.plan.n_ticks.sum(axis=1))
        assert demo_actions(split, 256).tobytes() == demo_actions(case.plan, 256).tobytes()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
# every refusal of naf_chain_demo_rows_legs that include/naf_hip.h names: naf_chain_demo_rows' and K outside 1 .. 63
ARGUMENT_ERRORS = (dict(h=None), dict(q=None), dict(a=None), dict(n=None), dict(t=None), dict(o=None), dict(rows=None), dict(rec=None),
                   dict(K=0), dict(K=64), dict(K=-1), dict(N=0), dict(N=-3), dict(T=0), dict(T=1025), dict(T=-64), dict(rf=None),
                   dict(rf=0), dict(rad=float("nan")), dict(rad=float("inf")), dict(rad=-0.01))


def test_header_symbol_abi_and_argument_errors():
    import ctypes as ct
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40 and re.search(r"^#define NAF_CHAIN_DEMO_MAX_LEGS 63$", text, re.M)
    name = "naf_chain_demo_rows_legs"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h, const float\* q_start_dev, const float\* leg_actions_dev", text, re.M)
    assert name in _lib.EXPORTED_SYMBOLS
    declared = re.sub(r"/\*.*?\*/", "", text.split(f"int {name}(")[1].split(")")[0], flags=re.S)
    assert len(_lib._PROTOS[name]) == declared.count(",") + 1 == 15
    assert _lib._PROTOS[name] == [ct.c_void_p] * 4 + [ct.c_int] + [ct.c_void_p] * 2 + [ct.c_float] + [ct.c_int] * 2 + [ct.c_void_p] + \
        [ct.c_int] + [ct.c_void_p] * 3
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40 and hasattr(lib, name)
    # argument errors are host code and launch nothing: the fake handle is a zeroed buffer, read (A = 0) only by the row-width check
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    rf0 = lib.naf_replay_row_floats(9, 0)
    call = lambda h=p, q=p, a=p, n=p, K=2, t=p, o=p, rad=0.06, N=1, T=64, rows=p, rf=rf0, rec=p: lib.naf_chain_demo_rows_legs(   # noqa: E731
        h, q, a, n, K, t, o, rad, N, T, rows, rf0 + 1 if rf is None else rf, rec, None, None)
    for kw in ARGUMENT_ERRORS:
        assert call(**kw) == -1, kw


# ---- the shortcut ----------------------------------------------------------------------------------------------------------------
def test_shortcut_nodes():
    """node 0 the start and node 1 the goal; nodes 2 .. in path order, the corners among them as they are; W - K points handed to
    the longest pieces, the lowest leg among equals, placed at a + (i / (c + 1)) (b - a); W <= K leaves the corners only"""
    poly = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 1.0], [4.0, 3.0]], np.float32)      # legs of max-norm length 4, 1, 2
    for W in (0, 3, 4):
        out = shortcut_nodes(poly, W)
        assert out.dtype == np.float32 and np.array_equal(out, poly[[0, 3, 1, 2]])
    out = shortcut_nodes(poly, 8)
    # 4 points: leg 0 (4), then leg 0 again (2 = leg 2's 2: the lowest leg), then leg 2 (2), then leg 0 (4/3)
    want = [[0, 0], [4, 3], [1, 0], [2, 0], [3, 0], [4, 0], [4, 1], [4, 2]]
    assert out.shape == (8, 2) and np.array_equal(out, np.array(want, np.float32))
    rng = np.random.default_rng(3)
    for K, W in ((3, 16), (5, 16), (7, 64), (2, 4)):
        poly = np.cumsum(rng.uniform(-1.0, 1.0, (K, 6)), axis=0).astype(np.float32)
        out = shortcut_nodes(poly, W)
        assert out.shape == (W, 6) and np.array_equal(out[0], poly[0]) and np.array_equal(out[1], poly[-1])
        path = np.concatenate([out[:1], out[2:], out[1:2]])
        at = [int(np.nonzero(np.all(path == c, axis=1))[0][0]) for c in poly]      # the corners, kept to the bit and in order
        assert at == sorted(at) and at[0] == 0 and at[-1] == W - 1
        # in path order: along each old leg the points run from a to b, uniformly
        for l in range(K - 1):
            a, b, c = poly[l].astype(np.float64), poly[l + 1].astype(np.float64), at[l + 1] - at[l] - 1
            for i in range(1, c + 1):
                assert np.array_equal(path[at[l] + i], (a + (i / (c + 1)) * (b - a)).astype(np.float32))
        lengths = joint_distance32(poly[1:], poly[:-1]).astype(np.float64)
        pieces = lengths / np.diff(at)
        assert pieces.max() <= (lengths / np.maximum(np.diff(at) - 1, 1)).min() + 1e-12      # greedy: no piece could have used a point better
        old = np.float64(lengths.sum())
        assert abs(joint_distance32(path[1:], path[:-1]).astype(np.float64).sum() - old) <= 1e-5 * old


RECORDED = {"planar3": {27: (3, 4), 33: (3, 4), 36: (3, 4)}, "iiwa_like7": {3: (4, 4), 14: (5, 4), 16: (4, 3)}}


@pytest.mark.parametrize("name,cut", [("planar3", None), ("iiwa_like7", R.IIWA_CUT)])
def test_the_shortcut_round_shortens_roadmap_paths_and_touches_nothing_else(name, cut):
    """joint_paths_host(roadmap=14, shortcut=16) on chain_roadmap_common's sets through the twin: every query that is not 'roadmap' is
    byte-equal to the call without shortcut, no 'roadmap' length grows, roadmap_length holds the old lengths, at least 2 of the 4
    'roadmap' queries get strictly shorter (recorded: 3 of 4 in both sets — planar3 27, 33, 36 to 1.09 x, 1.00 x, 1.19 x the straight
    line from 1.55 x, 1.38 x, 1.65 x; iiwa_like7 3, 14, 16 to 1.21 x, 1.27 x, 1.15 x from 2.27 x, 3.25 x, 2.35 x; the fourth of each
    is already as long as the straight line), and every edge of every polyline is free at the twin's sure samples."""
    q0, q1, ob, margin = R.value_queries(name, cut)
    base = R.value_paths(name, R.ROADMAP, cut)
    twin = R.arm(name)[1]
    out = joint_paths_host(twin, q0, q1, ob, margin=margin, roadmap=R.ROADMAP, shortcut=16, **R.VALUE_KW)
    rm = base.outcome == "roadmap"
    assert rm.sum() == 4 and np.array_equal(out.outcome, base.outcome)
    for field, x, y in zip(base._fields, out, base):
        assert x.dtype == y.dtype and x[~rm].tobytes() == y[~rm].tobytes(), field
    assert np.array_equal(out.n_nodes[~rm], base.n_nodes[~rm]) and np.all(np.isnan(out.nodes[~rm]))
    assert np.array_equal(out.roadmap_free_edges, base.roadmap_free_edges)
    assert np.array_equal(out.roadmap_length[rm], base.length[rm]) and np.all(np.isnan(out.roadmap_length[~rm]))
    assert out.roadmap_length.dtype == base.length.dtype and out.shortcut_free_edges.dtype == np.int64
    assert np.all(out.shortcut_free_edges[~rm] == -1) and np.all(out.shortcut_free_edges[rm] >= 1)
    # (no polyline is shorter than the straight line; a float32 sum over up to 15 edges may round half an ulp below it per edge)
    assert np.all(out.length[rm] <= base.length[rm]) and np.all(out.length[rm] >= out.straight_length[rm] * (1 - 16 * 2.0 ** -24))
    shorter = rm & (out.length < base.length)
    ratio = lambda p: (p.length / p.straight_length)[rm]      # noqa: E731
    print(name, "roadmap", np.nonzero(rm)[0], "x straight", np.round(ratio(base), 2), "->", np.round(ratio(out), 2), "nodes",
          base.n_nodes[rm], "->", out.n_nodes[rm], "free", out.shortcut_free_edges[rm])
    assert shorter.sum() >= 2
    assert {int(q): (int(base.n_nodes[q]), int(out.n_nodes[q])) for q in np.nonzero(shorter)[0]} == RECORDED[name]
    for q in np.nonzero(rm & ~shorter)[0]:                     # a polyline that is kept is kept whole
        assert out.n_nodes[q] == base.n_nodes[q] and out.nodes[q, :out.n_nodes[q]].tobytes() == base.nodes[q, :base.n_nodes[q]].tobytes()
        assert all(getattr(out, f)[q] == getattr(base, f)[q] for f in ("length", "samples", "sample_step", "min_clearance"))
    for q in np.nonzero(shorter)[0]:                           # a new one runs start .. goal over shortcut_nodes of the old
        poly, pool = out.nodes[q, :out.n_nodes[q]], shortcut_nodes(base.nodes[q, :base.n_nodes[q]], 16).astype(np.float64)
        assert np.array_equal(poly[0], C.f32(q0[q])) and np.array_equal(poly[-1], C.f32(q1[q]))
        assert all(np.any(np.all(pool == x, axis=1)) for x in poly)
        total = np.float32(0.0)
        for x in joint_distance32(poly[1:], poly[:-1]):
            total = np.float32(total + x)
        assert out.length[q] == total and out.sample_step[q] <= R.VALUE_KW["resolution"]
    assert out.nodes.shape == (len(q0), out.n_nodes.max(), q0.shape[1])
    assert R.edges_free_at_sure_samples(name, out, ob, margin) == int((out.n_nodes[rm] - 1).sum())
    w = out.waypoints(5)
    assert np.all(np.isfinite(w[rm])) and out._replace(length=out.length).roadmap_length is out.roadmap_length


def test_shortcut_off_is_off_and_the_refusals():
    q0, q1, ob, margin = R.value_queries("planar3")
    twin = R.arm("planar3")[1]
    base = R.value_paths("planar3", R.ROADMAP)
    off = joint_paths_host(twin, q0, q1, ob, margin=margin, roadmap=R.ROADMAP, shortcut=0, **R.VALUE_KW)
    same_paths(off, base)
    assert off.roadmap_length is None and off.shortcut_free_edges is None and base.roadmap_length is None
    few = (q0[:2], q1[:2], ob[:2])
    with pytest.raises(ValueError, match="shortcut > 0 needs roadmap > 0"):
        joint_paths_host(twin, *few, shortcut=16)
    for bad in (3, 65, True, 16.0, -4, "16"):
        with pytest.raises(ValueError, match="shortcut is a number of nodes, 0 or from 4 to 64"):
            joint_paths_host(twin, *few, roadmap=4, shortcut=bad)
    assert joint_paths_host(twin, *few, roadmap=2, shortcut=4, **R.VALUE_KW).shortcut_free_edges.shape == (2,)


# ---- the façade on the host ------------------------------------------------------------------------------------------------------
def test_the_facade_on_the_host_and_its_refusals():
    """plan_joint_paths(roadmap=, shortcut=) is joint_paths_host's; demonstrate_joint_paths(polylines=True) gives every 'roadmap'
    query an outcome other than 'none' with the plan's ticks, the one-via queries the default call's numbers, and a query with no
    path 'none'; without polylines a 'roadmap' query is still 'none'. The refusals, in arm_planner's words."""
    from robotic_manipulator_rloa_amd.environment.kinematic import demonstration_rows_host
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    f = planar_framework()
    q0, q1, ob, margin = R.value_queries("planar3")
    kw = dict(goal_joint_positions=q1, initial_joint_positions=q0, obstacles=ob, clearance_margin=margin, on_device=False, **R.VALUE_KW)
    out = f.plan_joint_paths(roadmap=R.ROADMAP, shortcut=16, **kw)
    twin = R.arm("planar3")[1]
    want = joint_paths_host(twin, q0, q1, ob, margin=margin, roadmap=R.ROADMAP, shortcut=16, **R.VALUE_KW)
    same_paths(out, want)
    for name in ("roadmap_length", "shortcut_free_edges"):
        assert getattr(out, name).tobytes() == getattr(want, name).tobytes()
    plain = f.plan_joint_paths(roadmap=R.ROADMAP, **kw)
    same_paths(plain, R.value_paths("planar3", R.ROADMAP))
    assert plain.roadmap_length is None and plain.shortcut_free_edges is None
    rm, via, none = out.outcome == "roadmap", out.candidate >= 0, (out.candidate < 0) & (out.outcome != "roadmap")
    assert rm.sum() == 4 and via.sum() >= 8 and none.sum() >= 1
    default = f.demonstrate_joint_paths(out, on_device=False)
    assert np.all(default.outcome[rm] == "none")
    demos = f.demonstrate_joint_paths(out, polylines=True, on_device=False)
    assert np.all(demos.outcome[rm] != "none") and np.all(demos.outcome[none] == "none") and np.all(demos.planned_ticks[none] == 0)
    for q in np.nonzero(rm)[0]:
        plan = demonstration_plan_legs(out.nodes[q:q + 1, :out.n_nodes[q]], out.n_nodes[q:q + 1], 1.0, 400)
        assert demos.planned_ticks[q] == plan.n_ticks.sum() and demos.frames[q] >= 1
        one = demonstration_rows_host(f.env, plan, f.env.end_effector(C.f32(out.goal[q:q + 1])), ob[q:q + 1], 400)
        assert one.outcome[0] == demos.outcome[q] and one.frames[0] == demos.frames[q]
        assert one.final_distance[0] == demos.final_distance[q]
    print("roadmap queries", np.nonzero(rm)[0], demos.outcome[rm], demos.frames[rm], "of", demos.planned_ticks[rm])
    for field in ("outcome", "frames", "final_distance", "min_clearance", "min_self_clearance", "min_cell_clearance", "planned_ticks",
                  "kept"):
        a, b = getattr(demos, field), getattr(default, field)
        assert a.dtype == b.dtype and a[via].tobytes() == b[via].tobytes(), field
    rows_of = lambda d, mask: int(d.frames[mask & d.kept].sum())      # noqa: E731
    assert demos.rows_total == rows_of(default, via) + rows_of(demos, rm) == len(demos.rows)
    # by targets: a query without a reachable goal pose is padded in the new attributes too
    targets = np.concatenate([f.env.end_effector(q1[:3]), [[0.0, 0.0, 5.0]]])
    by_target = f.plan_joint_paths(targets, initial_joint_positions=q0[:4], obstacles=ob[:4], on_device=False, roadmap=4, shortcut=6,
                                   **R.VALUE_KW)
    assert by_target.outcome[3] == "goal" and by_target.shortcut_free_edges[3] == -1 and np.isnan(by_target.roadmap_length[3])
    assert by_target.roadmap_length.shape == by_target.shortcut_free_edges.shape == (4,) and len(by_target) == 16
    few = dict(kw, goal_joint_positions=q1[:2], initial_joint_positions=q0[:2], obstacles=ob[:2])
    for bad in (3, 65, True, 16.0):
        with pytest.raises(InvalidEnvironmentParameter) as err:
            f.plan_joint_paths(roadmap=4, shortcut=bad, **few)
        assert err.value.message == f"shortcut is a number of nodes, 0 (no shortcut round) or from 4 to 64: got {bad!r}"
    with pytest.raises(InvalidEnvironmentParameter) as err:
        f.plan_joint_paths(shortcut=16, **few)
    assert err.value.message == "plan_joint_paths(shortcut=16) shortens 'roadmap' polylines: it needs roadmap=M with M > 0"
    with pytest.raises(InvalidEnvironmentParameter) as err:
        f.demonstrate_joint_paths(out, polylines=1, on_device=False)
    assert err.value.message == "polylines is a bool: got 1"
    f.naf_agent = object()
    with pytest.raises(InvalidEnvironmentParameter) as err:
        f.reach_targets(targets, joint_paths=True, shortcut=16)
    assert err.value.message == "reach_targets(shortcut=16) shortens 'roadmap' polylines: it needs roadmap=M with M > 0"
    with pytest.raises(InvalidEnvironmentParameter, match="shortcut is a number of nodes"):
        f.reach_targets(targets, joint_paths=True, roadmap=4, shortcut=2)

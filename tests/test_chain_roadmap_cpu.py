"""CPU: the roadmap rule of environment/kinematic.py (roadmap_milestones, edge_pose, check_joint_edge, roadmap_edges, roadmap_search,
joint_paths_host(roadmap=M), JointPaths' nodes), the rehearsal of every case of tests/test_chain_roadmap_gpu.py with a float32
restatement in the kernel's place, what the roadmap is worth on two scenes, the plumbing of the entry point and the façade."""
import dataclasses
import itertools
import os
import re

import numpy as np
import pytest

import chain_cell_common as CC
import chain_ik_common as IK
import chain_roadmap_common as R
import chain_rollout_common as C
from conftest import ROOT
from test_chain_env_cpu import ARMS as ARM_TABLE
from test_chain_env_cpu import path, random_q

from robotic_manipulator_rloa_amd.environment.kinematic import (PRISMATIC, ROADMAP_MAX, JointPaths, check_joint_edge, check_joint_path,
                                                                edge_pose, edge_samples, joint_distance32, joint_paths_host,
                                                                path_pose, roadmap_chunks, roadmap_edges, roadmap_milestones,
                                                                roadmap_nodes, roadmap_search)


# ---- the poses and the record, pinned against the one-via rule -----------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 128, 1024])
def test_edge_pose_is_leg_two_of_a_path_that_stands_still_first(S):
    """The poses of a -> b at S samples equal leg 2 of a -> a -> b at 2 S samples, index by index and bit for bit; sample 0 is a,
    sample S - 1 is b, exactly."""
    model, _ = IK.arm("iiwa_like7")
    rng = np.random.default_rng(S)
    a, b = (C.f32(np.stack([random_q(model, rng) for _ in range(5)])) for _ in range(2))
    q = edge_pose(a[:, None, :], b[:, None, :], np.arange(S), S)
    leg2 = path_pose(a[:, None, :], a[:, None, :], b[:, None, :], S + np.arange(S), 2 * S)
    assert q.shape == (5, S, 7) and np.array_equal(q, leg2)
    assert np.array_equal(q[:, 0], a) and np.array_equal(q[:, -1], b)
    assert np.array_equal(edge_pose(a[0], b[0], 3, S), q[0, 3])


@pytest.mark.parametrize("name", ["planar3", "iiwa_like7", "slider4"])
def test_check_joint_edge_is_check_joint_path_on_that_path(name):
    """check_joint_edge(a, b, S) against check_joint_path(a, a, b, 2 S): the three minima, the length and the step bit for bit (the S
    copies of the start pose add nothing to a minimum), the first blocked index shifted by S, the count equal — less the S copies
    of the start pose where the start pose is blocked, whose first index is 0 in both. Free and blocked edges, and blocked starts."""
    model, twin = R.arm(name)
    rng = np.random.default_rng(5)
    q = IK.free_poses(model, twin, rng, 16)
    a, b = q[:8], q[8:]
    b[::3] = a[::3] + 0.15 * (b - a)[::3]                                 # short edges beside free poses: some of them are free
    a, b = C.f32(a), C.f32(b)
    ob = np.tile(C.away(model)[1], (8, 1))
    ob[1::2] = twin.end_effector(0.5 * (a + b))[1::2]
    ob[6] = twin.end_effector(a[6])                                       # a blocked start pose
    ob = C.f32(ob)
    S, margin = 64, R.MARGINS.get(name, 0.0)
    got = check_joint_edge(twin, a, b, ob, S, margin)
    want = check_joint_path(twin, a, a, b, ob, 2 * S, margin)
    assert got.shape == (8, 8)
    assert np.array_equal(got[:, :3], want[:, :3]) and np.array_equal(got[:, 5:7], want[:, 5:7]) and np.all(got[:, 7] == 0)
    assert np.array_equal(got[:, 5], joint_distance32(b, a).astype(np.float64))
    start = want[:, 3] == 0
    assert start[6] and np.array_equal(got[start, 3], want[start, 3]) and np.array_equal(got[start, 4], want[start, 4] - S)
    moved = np.where(want[~start, 3] < 0, -1, want[~start, 3] - S)
    assert np.array_equal(got[~start, 3], moved) and np.array_equal(got[~start, 4], want[~start, 4])
    assert np.any(got[:, 4] == 0) and np.any(got[~start, 4] > 0)
    for bad in (0, 63, 96, 2112, 64.0):
        with pytest.raises(ValueError, match="multiple of 64"):
            check_joint_edge(twin, a[0], b[0], ob[0], bad)


def test_edge_samples_and_chunks_at_the_boundaries():
    assert edge_samples([0.0], 0.05) == 64 and edge_samples([], 0.05) == 64
    assert edge_samples([63 * 0.05], 0.05) == 64 and edge_samples([63 * 0.05 + 1e-9], 0.05) == 128
    assert edge_samples([1e9], 0.05) == 2048 and edge_samples([2047 * 0.05 - 1e-9], 0.05) == 2048
    for S in range(64, 2049, 64):
        assert edge_samples([0.05 * (S - 1) * (1 - 1e-12)], 0.05) == S
    lengths = np.full((5, 3), 0.1)
    lengths[2, 1] = 10.0
    assert roadmap_chunks(lengths, 0.05) == [(0, 5, 256)]
    assert roadmap_chunks(lengths, 0.05, budget=2 * 3 * 64) == [(0, 2, 64), (2, 1, 256), (3, 2, 64)]
    assert roadmap_edges(2).tolist() == [[0, 1]] and roadmap_edges(4).tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert roadmap_edges(64).shape == (2016, 2) and roadmap_edges(64).dtype == np.int32


# ---- the search -----------------------------------------------------------------------------------------------------------------------
def records_of(V, usable, weights):
    edges = roadmap_edges(V)
    rec = np.zeros((1, len(edges), 8), np.float32)
    rec[0, :, 4] = np.where(usable, 0, 3)
    rec[0, :, 5] = weights
    return rec, edges


def brute_shortest(V, edges, usable, weights):
    """the least float64 sum over all simple paths from node 0 to node 1 over the usable edges, None: there is none"""
    w = {}
    for (i, j), u, x in zip(edges.tolist(), usable, weights):
        if u:
            w[(i, j)] = w[(j, i)] = float(x)
    best = None
    for k in range(V - 1):
        for mid in itertools.permutations(range(2, V), k):
            nodes = (0,) + mid + (1,)
            if all(p in w for p in zip(nodes[:-1], nodes[1:])):
                total = sum(w[p] for p in zip(nodes[:-1], nodes[1:]))
                best = total if best is None or total < best else best
    return best


def test_roadmap_search_against_brute_force_over_all_simple_paths():
    """Random graphs on V = 2 .. 7 nodes, each edge usable with probability 0.45, weights multiples of 1 / 8 up to 8 (dyadic: every
    float32 sum is exact, so the lengths are compared exactly): the length is the least over all simple paths, the returned nodes
    are a path over usable edges from 0 to 1 whose weights sum to it, and the float64 copy of the records gives the same answer.
    Without a usable edge (0, 1) — with one the straight line wins, which the next test holds."""
    rng = np.random.default_rng(12)
    reached = unreached = 0
    for trial in range(300):
        V = int(rng.integers(2, 8))
        edges = roadmap_edges(V)
        usable = rng.random(len(edges)) < 0.45
        usable[0] = False if V > 2 and trial % 2 else usable[0]
        weights = rng.integers(1, 65, len(edges)) / 8.0
        if usable[0]:
            weights[0] = 0.125                                # (a usable straight line is the shortest path: no refinement at work)
        rec, _ = records_of(V, usable, weights)
        n_nodes, index, length = roadmap_search(rec, edges, V)
        n64, i64, l64 = roadmap_search(rec.astype(np.float64), edges, V)
        assert np.array_equal(n_nodes, n64) and np.array_equal(index, i64) and np.array_equal(length, l64, equal_nan=True)
        assert length.dtype == np.float32 and index.shape == (1, V)
        want = brute_shortest(V, edges, usable, weights)
        if want is None:
            unreached += 1
            assert n_nodes[0] == 0 and np.isnan(length[0]) and np.all(index[0] == -1)
            continue
        reached += 1
        nodes = index[0, :n_nodes[0]].tolist()
        assert float(length[0]) == want and nodes[0] == 0 and nodes[-1] == 1 and len(set(nodes)) == len(nodes)
        assert np.all(index[0, n_nodes[0]:] == -1)
        w = {tuple(e): x for e, u, x in zip(edges.tolist(), usable, weights) if u}
        assert sum(w[(min(p), max(p))] for p in zip(nodes[:-1], nodes[1:])) == want
    assert reached >= 80 and unreached >= 40


def test_roadmap_search_rules():
    """The straight line wins outright, though a float32 sum comes out an ulp below it; ties go to the lowest predecessor; an
    unreachable goal and V = 2; a batch is searched query by query; an edge outside 0 <= i < j < V is refused."""
    one = np.float32(1.0)
    below = np.nextafter(one, np.float32(0.0)) / np.float32(2.0)
    rec, edges = records_of(3, [True, True, True], [one, below, below])       # (0,1) 1 | (0,2) + (1,2) = 1 - 2^-24
    n_nodes, index, length = roadmap_search(rec, edges, 3)
    assert n_nodes[0] == 2 and index[0].tolist() == [0, 1, -1] and length[0] == one
    rec[0, 0, 4] = 1                                                        # ... and without it the two edges are the path
    n_nodes, index, length = roadmap_search(rec, edges, 3)
    assert n_nodes[0] == 3 and index[0].tolist() == [0, 2, 1] and length[0] == below + below
    # node 1 through node 2 and through node 3 at the same length, and node 4 through both of them: the lowest predecessor
    usable = [False, True, True, True, True, True, False, True, True, False]      # (0,1) (0,2) (0,3) (0,4) (1,2) (1,3) (1,4) (2,3) ..
    rec, edges = records_of(5, usable, [9, 1, 1, 9, 2, 2, 9, 9, 9, 9])
    n_nodes, index, length = roadmap_search(rec, edges, 5)
    assert index[0, :3].tolist() == [0, 2, 1] and length[0] == 3 and n_nodes[0] == 3
    rec[0, 1, 5] = 1.5                                                      # through node 3 is now strictly shorter
    assert roadmap_search(rec, edges, 5)[1][0, :3].tolist() == [0, 3, 1]
    # a chain 0 - 4 - 3 - 2 - 1 needs all V - 1 rounds
    usable = [False, False, False, True, True, False, False, True, False, True]
    rec, edges = records_of(5, usable, [1] * 10)
    n_nodes, index, length = roadmap_search(rec, edges, 5)
    assert index[0].tolist() == [0, 4, 3, 2, 1] and length[0] == 4
    # unreachable: node 1 has no usable edge; V = 2, free and blocked
    rec, edges = records_of(4, [False, True, True, False, False, True], [1] * 6)
    n_nodes, index, length = roadmap_search(rec, edges, 4)
    assert n_nodes[0] == 0 and np.isnan(length[0]) and np.all(index[0] == -1)
    for usable, want in ((True, ([2], [[0, 1]], [0.75])), (False, ([0], [[-1, -1]], [np.nan]))):
        rec, edges = records_of(2, [usable], [0.75])
        n_nodes, index, length = roadmap_search(rec, edges, 2)
        assert n_nodes.tolist() == want[0] and index.tolist() == want[1] and np.array_equal(length, np.float32(want[2]), equal_nan=True)
    # a batch, and a subset of the edges
    a, edges = records_of(3, [False, True, True], [1, 2, 3])
    b, _ = records_of(3, [True, False, False], [1, 2, 3])
    n_nodes, index, length = roadmap_search(np.concatenate([a, b, a]), edges, 3)
    assert n_nodes.tolist() == [3, 2, 3] and index.tolist() == [[0, 2, 1], [0, 1, -1], [0, 2, 1]] and length.tolist() == [5, 1, 5]
    assert roadmap_search(a[:, 1:], edges[1:], 3)[1].tolist() == [[0, 2, 1]]
    assert roadmap_search(np.zeros((0, 3, 8), np.float32), edges, 3)[0].shape == (0,)
    for bad in ([[1, 0]], [[0, 3]], [[-1, 2]], [[2, 2]]):
        with pytest.raises(ValueError, match="0 <= i < j < 3"):
            roadmap_search(a[:, :1], bad, 3)


# ---- the milestones -------------------------------------------------------------------------------------------------------------------
def test_roadmap_milestones():
    """Inside the limits as float32 holds them; deterministic per seed, another seed gives others, and not path_vias' draws; the
    first ceil(M / 2) follow the vias' rule around the midpoint, the rest are uniform over the limits (+-pi for an unlimited
    revolute joint); a query's milestones are the same whichever other queries of the call are blocked — they are drawn for all N
    and indexed; a prismatic joint without limits is refused by name."""
    model, twin = IK.arm("iiwa_like7")
    rng = np.random.default_rng(6)
    a, b = (C.f32(np.stack([random_q(model, rng) for _ in range(40)])) for _ in range(2))
    m = roadmap_milestones(model, a, b, 15, seed=9)
    assert m.shape == (40, 15, 7) and m.dtype == np.float32
    assert np.array_equal(m, roadmap_milestones(model, a, b, 15, seed=9))
    assert np.mean(m != roadmap_milestones(model, a, b, 15, seed=10)) > 0.9          # (all but those clipped onto the same limit)
    lo, hi = (np.array([getattr(j, k) for j in model.joints]).astype(np.float32) for k in ("lower", "upper"))
    assert all(j.limited for j in model.joints) and np.all(m >= lo) and np.all(m <= hi)
    u = np.random.default_rng([9, 0x726F6164]).random((40, 15, 7))
    lo64, hi64 = (np.array([getattr(j, k) for j in model.joints]) for k in ("lower", "upper"))
    far = lo64 + u[:, 8:] * (hi64 - lo64)
    assert np.array_equal(m[:, 8:], np.clip(far.astype(np.float32), lo, hi))
    mid, D = 0.5 * (a + b), np.abs(b - a).max(axis=-1)
    near = mid[:, None, :] + (2.0 * u[:, :8] - 1.0) * (0.5 * 2.0 ** (np.arange(8) % 3))[None, :, None] * np.maximum(D, 0.5)[:, None, None]
    assert np.array_equal(m[:, :8], np.clip(near.astype(np.float32), lo, hi))
    # the uniform ones cover the range, the near ones stay around the midpoint unless their width is large
    assert np.all((m[:, 8:].max(axis=(0, 1)) - m[:, 8:].min(axis=(0, 1))) > 0.9 * (hi - lo))
    assert roadmap_milestones(model, a, b, 1, seed=9).shape == (40, 1, 7) and roadmap_milestones(model, a, b, 0, seed=9).shape == (40, 0, 7)
    assert roadmap_milestones(model, a[:0], b[:0], 4, seed=9).shape == (0, 4, 7)
    # planar3's joints have no limits: +-pi, and the near ones are not clipped
    free_model = R.arm("planar3")[0]
    spin = [k for k, j in enumerate(free_model.joints) if not j.limited]
    m3 = roadmap_milestones(free_model, np.full((300, 3), 3.0), np.full((300, 3), 3.1), 6, seed=0)
    if spin:
        assert np.abs(m3[:, 3:][:, :, spin]).max() <= np.float32(np.pi) and np.abs(m3[:, 3:][:, :, spin]).max() > 3.0
        assert m3[:, :3][:, :, spin].max() > np.pi
    # which queries are blocked does not enter: joint_paths_host hands every query the milestones of its index in the call
    _, twin3 = R.arm("planar3")
    q0, q1, ob, margin = R.value_queries("planar3")
    out = R.value_paths("planar3", R.ROADMAP)
    all_m = roadmap_milestones(twin3.model, q0, q1, R.ROADMAP, R.VALUE_KW["seed"])
    pool = {n: {tuple(x) for x in np.concatenate([C.f32(q0[n:n + 1]), C.f32(q1[n:n + 1]), all_m[n]]).tolist()} for n in range(len(q0))}
    for n in np.nonzero(out.outcome == "roadmap")[0]:
        assert all(tuple(x) in pool[n] for x in out.nodes[n, :out.n_nodes[n]].tolist())
    # an unlimited prismatic joint
    slider, _ = IK.slider()
    k = next(k for k, j in enumerate(slider.joints) if j.type == PRISMATIC)
    joints = list(slider.joints)
    joints[k] = dataclasses.replace(joints[k], limited=False)
    broken = dataclasses.replace(slider, joints=joints)
    with pytest.raises(ValueError, match=rf"joint {k} \(involved_joints\[{k}\]\) is a prismatic joint without limits"):
        roadmap_milestones(broken, np.zeros((2, 4)), np.zeros((2, 4)), 4, seed=0)
    assert roadmap_milestones(slider, np.zeros((2, 4)), np.zeros((2, 4)), 4, seed=0).shape == (2, 4, 4)


# ---- waypoints -----------------------------------------------------------------------------------------------------------------------
def test_waypoints_on_a_three_edge_polyline():
    """A 'roadmap' polyline of three edges with max-norm lengths 1, 2 and 1: waypoints(9) are uniform in its length — the nodes
    themselves at 0, 1/4, 3/4 and 1 — beside a 'via' query resampled as before and a query without a path (NaN)."""
    nodes = np.array([[0.0, 0.0], [1.0, 0.5], [1.0, -1.5], [2.0, -1.0]])
    start = np.array([nodes[0], [0.0, 0.0], [0.0, 0.0]])
    goal = np.array([nodes[-1], [2.0, 0.0], [1.0, 1.0]])
    nan = np.full(3, np.nan)
    via = np.array([[np.nan, np.nan], [1.0, 1.0], [np.nan, np.nan]])
    paths = JointPaths(np.array(["roadmap", "via", "blocked"]), np.array([-1, 3, -1]), via, np.array([4.0, 2.0, np.nan]), nan, nan, nan,
                       nan, np.full(3, -1), nan, np.full(3, 64), start, goal, np.zeros(3, bool), nan, np.zeros(3, np.int64))
    assert paths.nodes is None and paths.n_nodes is None and paths.roadmap_free_edges is None
    plain = paths.waypoints(9)
    assert np.all(np.isnan(plain[0])) and np.all(np.isnan(plain[2])) and np.array_equal(plain[1][[0, 4, 8]], [[0, 0], [1, 1], [2, 0]])
    paths.nodes = np.full((3, 4, 2), np.nan)
    paths.nodes[0] = nodes
    paths.n_nodes, paths.roadmap_free_edges = np.array([4, 0, 0]), np.array([5, -1, 2])
    w = paths.waypoints(9)
    assert w.shape == (3, 9, 2) and np.array_equal(w[1], plain[1]) and np.all(np.isnan(w[2]))
    assert np.array_equal(w[0][[0, 2, 6, 8]], nodes)
    assert np.allclose(w[0][[1, 3, 4, 5, 7]], [[0.5, 0.25], [1.0, 0.0], [1.0, -0.5], [1.0, -1.0], [1.5, -1.25]], atol=1e-15)
    kept = paths._replace(start=start + 0.0)
    assert kept.nodes is paths.nodes and kept.n_nodes is paths.n_nodes and JointPaths._fields == paths._fields and len(paths) == 16
    with pytest.raises(ValueError, match="at least 2"):
        paths.waypoints(1)


# ---- the rehearsal -------------------------------------------------------------------------------------------------------------------
REHEARSED = [(name, N, V, S) for name in R.ARMS for N, V, S in R.COUNTS] + R.EXTRA
MEASURED = {}


@pytest.mark.parametrize("name,N,V,S", REHEARSED)
def test_rehearsal(name, N, V, S):
    """Every GPU case with the float32 restatement in the kernel's place: the case builds (the twin alone meets the 1 % cap and the
    floors, reseeded until it does — at the attempt chain_roadmap_common.ATTEMPT records, which the GPU suite builds unverified),
    and the restatement's records and poses pass every check the kernel's will; the pose deviation is measured."""
    case = R.build_case(name, N, V, S)
    assert case.attempt == R.ATTEMPT[(name, N, V, S)]
    again = R.build_case(name, N, V, S, verify=False)
    assert np.array_equal(again.nodes, case.nodes) and np.array_equal(again.obstacles, case.obstacles)
    out, poses = R.record32(case)
    MEASURED[(name, N, V, S)] = R.check_records(case, out, poses)[0]


def test_the_measured_deviation_is_the_constant():
    """POSE_DEVIATION is the rehearsal's largest measured deviation rounded up (by no more than a quarter), and the bound 8 x it"""
    for args in REHEARSED:
        if args not in MEASURED:
            case = R.build_case(*args)
            MEASURED[args] = R.check_records(case, *R.record32(case))[0]
    worst = max(MEASURED.values())
    print({k: f"{v:.2e}" for k, v in MEASURED.items()})
    assert worst <= R.POSE_DEVIATION <= 1.25 * worst, (worst, R.POSE_DEVIATION)
    assert R.POSE_BOUND == 8 * R.POSE_DEVIATION


# ---- what the roadmap is worth -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.VALUE))
def test_the_roadmap_rescues_blocked_queries_and_touches_nothing_else(name):
    """Through the twin alone, on chain_roadmap_common's query sets (iiwa_like7 among its boxes, 96 queries, margin 0.005; planar3
    between its walls, 48; resolution 0.05, 16 candidates, M = 14): joint_paths_host(roadmap=14) turns at least 4 / at least 1 of
    the 'blocked' queries into 'roadmap'; every other query's fields are bit-equal to the call without roadmap, and so are a
    rescued query's untouched fields; every edge of every returned polyline is free at all its samples (checked again, edge by
    edge, from the returned nodes); length, minima, step and samples are the edges'."""
    q0, q1, ob, margin = R.value_queries(name)
    base, out = R.value_paths(name, 0), R.value_paths(name, R.ROADMAP)
    census = lambda p: {o: int(np.sum(p.outcome == o)) for o in sorted(set(p.outcome))}      # noqa: E731
    print(name, census(base), "->", census(out))
    assert base.nodes is None and base.n_nodes is None and base.roadmap_free_edges is None
    was_blocked, rescued = base.outcome == "blocked", out.outcome == "roadmap"
    assert np.all(was_blocked[rescued]) and rescued.sum() >= R.VALUE[name]["floor"], (int(was_blocked.sum()), int(rescued.sum()))
    assert np.array_equal(out.outcome[~rescued], base.outcome[~rescued])
    for field, x, y in zip(base._fields, out, base):
        keep = ~rescued if field in ("outcome", "length", "min_clearance", "min_self_clearance", "min_cell_clearance", "sample_step",
                                     "samples") else np.ones(len(rescued), bool)
        assert x.dtype == y.dtype and x[keep].tobytes() == y[keep].tobytes(), field
    assert np.all(out.candidate[rescued] == -1) and np.all(np.isnan(out.via[rescued]))
    assert np.array_equal(out.n_nodes > 0, rescued) and np.all(out.n_nodes[rescued] >= 3) and out.nodes.shape == (len(q0), out.n_nodes.max(), q0.shape[1])
    assert np.array_equal(out.roadmap_free_edges >= 0, was_blocked) and np.all(out.roadmap_free_edges[rescued] >= 2)
    assert R.edges_free_at_sure_samples(name, out, ob, margin, blocked_only=False) == int((out.n_nodes[rescued] - 1).sum())
    twin = R.arm(name)[1]
    graph = roadmap_nodes(q0, q1, roadmap_milestones(twin.model, q0, q1, R.ROADMAP, R.VALUE_KW["seed"])).astype(np.float64)
    for q in np.nonzero(rescued)[0]:
        poly = out.nodes[q, :out.n_nodes[q]]
        assert np.array_equal(poly[0], C.f32(q0[q])) and np.array_equal(poly[-1], C.f32(q1[q]))
        # an edge is sampled from its lower node to its higher one, whichever way the polyline runs along it
        index = [int(np.nonzero(np.all(graph[q] == x, axis=1))[0][0]) for x in poly]
        lower = np.array([graph[q, min(i, j)] for i, j in zip(index[:-1], index[1:])])
        upper = np.array([graph[q, max(i, j)] for i, j in zip(index[:-1], index[1:])])
        rec = check_joint_edge(twin, lower, upper, ob[q], int(out.samples[q]), margin)
        assert np.all(rec[:, 4] == 0) and out.samples[q] >= edge_samples(rec[:, 5], R.VALUE_KW["resolution"])
        total = np.float32(0.0)
        for x in rec[:, 5].astype(np.float32):
            total = np.float32(total + x)
        assert out.length[q] == total and out.length[q] >= out.straight_length[q]
        assert out.min_clearance[q] == rec[:, 0].min() and out.min_self_clearance[q] == rec[:, 1].min()
        assert out.min_cell_clearance[q] == rec[:, 2].min() and out.sample_step[q] == rec[:, 6].max() <= R.VALUE_KW["resolution"]
        w = out.waypoints(5)[q]
        assert np.array_equal(w[0], poly[0]) and np.array_equal(w[-1], poly[-1])
    assert np.all(np.isnan(out.waypoints(3)[out.outcome == "blocked"]))
    with pytest.raises(ValueError, match="roadmap is a number of milestones from 0 to 62"):
        joint_paths_host(twin, q0[:1], q1[:1], ob[:1], roadmap=63)
    with pytest.raises(ValueError, match="at their samples only"):
        joint_paths_host(twin, q0[:1], q1[:1], ob[:1], roadmap=2, certify=True)


def test_the_cut_of_the_end_to_end_test_holds_rescued_queries():
    """The GPU suite's end-to-end test plans the first IIWA_CUT queries of the iiwa_like7 set as a call of their own (their
    milestones are then that call's): the twin shows at least 2 of them rescued."""
    out = R.value_paths("iiwa_like7", R.ROADMAP, R.IIWA_CUT)
    print({o: int(np.sum(out.outcome == o)) for o in sorted(set(out.outcome))})
    assert np.sum(out.outcome == "roadmap") >= 2


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def test_header_symbol_abi_and_argument_errors():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40 and re.search(r"^#define NAF_CHAIN_EDGE_FLOATS 8$", text, re.M)
    name = "naf_chain_edge_check"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h, const float\* nodes_dev, const int32_t\* edges_dev,", text, re.M)
    assert name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 13
    import ctypes as ct
    assert _lib._PROTOS[name] == [ct.c_void_p] * 4 + [ct.c_float] + [ct.c_int] * 4 + [ct.c_float] + [ct.c_void_p] * 3
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40 and hasattr(lib, name)
    # argument errors are host code and launch nothing: a fake non-null handle is never dereferenced before they answer
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    call = lambda h=p, nodes=p, edges=p, o=p, rad=0.06, N=1, V=2, E=1, S=64, margin=0.0, out=p: lib.naf_chain_edge_check(   # noqa: E731
        h, nodes, edges, o, rad, N, V, E, S, margin, out, None, None)
    for kw in ARGUMENT_ERRORS:
        assert call(**kw) == -1, kw


# every refusal of naf_chain_edge_check that include/naf_hip.h names (tests/test_chain_roadmap_gpu.py runs them with a real handle)
ARGUMENT_ERRORS = (dict(h=None), dict(nodes=None), dict(edges=None), dict(o=None), dict(out=None), dict(N=0), dict(N=-2), dict(V=1),
                   dict(V=65), dict(V=0), dict(E=0), dict(E=2), dict(V=5, E=11), dict(E=-1), dict(N=1 << 20, V=64, E=2016), dict(S=0),
                   dict(S=32), dict(S=96), dict(S=2112), dict(S=-64), dict(margin=float("nan")), dict(margin=float("inf")),
                   dict(rad=float("nan")), dict(rad=float("inf")), dict(rad=-0.01))


# ---- through the façade --------------------------------------------------------------------------------------------------------------
def planar_framework():
    """planar3 between chain_cell_common's walls, as chain_roadmap_common's twin of it"""
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    ee, involved, fixed, init, var = ARM_TABLE["planar3"]
    f = ManipulatorFramework()
    f.initialize_kinematic_environment(path("planar3"), ee, fixed, involved, [0.45, 0.3, 0.0], [5.0, 5.0, 5.0], init, var,
                                       link_radius=0.03, obstacle_radius=R.ORAD, **CC.workcell_of("planar3"))
    return f


def same_paths(a, b):
    for field, x, y in zip(a._fields, a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), field
    for field in ("nodes", "n_nodes", "roadmap_free_edges"):
        x, y = getattr(a, field), getattr(b, field)
        assert (x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()), field


def test_plan_joint_paths_with_a_roadmap_on_the_host_and_its_refusals():
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    f = planar_framework()
    q0, q1, ob, margin = R.value_queries("planar3")
    kw = dict(goal_joint_positions=q1, initial_joint_positions=q0, obstacles=ob, clearance_margin=margin, on_device=False, **R.VALUE_KW)
    out = f.plan_joint_paths(roadmap=R.ROADMAP, **kw)
    same_paths(out, R.value_paths("planar3", R.ROADMAP))
    assert np.sum(out.outcome == "roadmap") >= 1 and out.nodes.shape[0] == len(q0) and out.n_nodes.shape == (len(q0),)
    for off in (dict(), dict(roadmap=0)):
        plain = f.plan_joint_paths(**kw, **off)
        same_paths(plain, R.value_paths("planar3", 0))
        assert plain.nodes is None and plain.n_nodes is None and plain.roadmap_free_edges is None
    # a 'roadmap' query has no start -> via -> goal: demonstrate_joint_paths reports 'none' for it
    rescued = out.outcome == "roadmap"
    demos = f.demonstrate_joint_paths(out, on_device=False)
    assert np.all(demos.outcome[rescued] == "none") and np.any(demos.outcome[out.candidate >= 0] != "none")
    for bad in (63, -1, 1.5, True, "14", None):
        with pytest.raises(InvalidEnvironmentParameter, match=r"roadmap is a number of milestones from 0 to 62"):
            f.plan_joint_paths(roadmap=bad, **kw)
    with pytest.raises(InvalidEnvironmentParameter, match=r"roadmap=14, certify=True\): roadmap edges are checked at their samples only"):
        f.plan_joint_paths(roadmap=14, certify=True, **kw)
    f.plan_joint_paths(roadmap=0, certify=True, **dict(kw, goal_joint_positions=q1[:2], initial_joint_positions=q0[:2], obstacles=ob[:2]))
    assert ROADMAP_MAX == 62 and f.plan_joint_paths(roadmap=62, **dict(kw, goal_joint_positions=q1[:1], initial_joint_positions=q0[:1],
                                                                      obstacles=ob[:1])).n_nodes.shape == (1,)
    # by targets: a query without a reachable goal pose is padded in the new attributes too
    targets = np.concatenate([f.env.end_effector(q1[:3]), [[0.0, 0.0, 5.0]]])
    by_target = f.plan_joint_paths(targets, initial_joint_positions=q0[:4], obstacles=ob[:4], on_device=False, roadmap=4, **R.VALUE_KW)
    assert by_target.outcome[3] == "goal" and by_target.n_nodes[3] == 0 and by_target.roadmap_free_edges[3] == -1
    assert by_target.nodes.shape[0] == 4 and by_target.nodes.shape[2] == 3 and len(by_target) == 16


def test_reach_targets_with_a_roadmap_against_a_stub_agent(monkeypatch):
    import torch
    from robotic_manipulator_rloa_amd.engine import ReachResult
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)          # goal poses and paths come from the twin
    f = planar_framework()
    q0, q1, ob, margin = R.value_queries("planar3")
    N, F = len(q0), 4
    targets = f.env.end_effector(q1)

    class Agent:                      # returns a straight joint path to the goal pose in F frames for every query but one
        state_size, action_size, seed, world_size = 15, 3, 0, 1

        def rollout_vectorized(self, chain, targets, obstacles, q0, **kw):
            z = np.zeros(N, np.float32)
            s = np.linspace(0.0, 1.0, F + 1)[None, :, None]
            paths = (q0[:, None, :] + s * (q1 - q0)[:, None, :]).astype(np.float32)
            outcome = np.array(["reached"] * N)
            outcome[1] = "frames"
            return ReachResult(outcome, np.full(N, F), z, z, z, z, paths, z, z, z, z, z)

    f.naf_agent = Agent()
    asked = []
    planned = R.value_paths("planar3", R.ROADMAP)

    def paths_to_goals(goal, start, obstacles, kw):
        asked.append(kw)
        return planned

    monkeypatch.setattr(f.arm_planner, "paths_to_goals", paths_to_goals)
    out = f.reach_targets(targets, obstacles=ob, initial_joint_positions=q0, frames=F, joint_paths=True, roadmap=R.ROADMAP)
    plain = f.reach_targets(targets, obstacles=ob, initial_joint_positions=q0, frames=F, joint_paths=True)
    assert asked == [{"roadmap": R.ROADMAP}, {}] and out.path is planned
    rescued = planned.outcome == "roadmap"
    reached = np.asarray(out.outcome) == "reached"
    has = np.isfinite(planned.length)
    assert rescued.sum() >= 1 and np.array_equal(has, rescued | (planned.candidate >= 0))
    walked = np.abs(C.f32(q1) - C.f32(q0)).max(axis=1)
    assert np.all(np.isnan(out.planned_ratio[~(has & reached)]))
    assert np.all(np.isfinite(out.planned_ratio[rescued & reached])) and np.any(rescued & reached)
    assert np.abs(out.planned_ratio[has & reached] - (walked / planned.length)[has & reached]).max() <= 1e-5
    assert np.all(out.planned_ratio[rescued & reached] <= 1.0 + 1e-5)
    for args, match in ((dict(joint_paths=True, roadmap=63), "roadmap is a number of milestones from 0 to 62"),
                        (dict(joint_paths=True, roadmap=2.0), "roadmap is a number of milestones"),
                        (dict(joint_paths=True, roadmap=True), "roadmap is a number of milestones"),
                        (dict(joint_paths=True, roadmap=3, certify=True), "roadmap edges are checked at their samples only"),
                        (dict(roadmap=3), "needs joint_paths=True")):
        with pytest.raises(InvalidEnvironmentParameter, match=match):
            f.reach_targets(targets, obstacles=ob, initial_joint_positions=q0, frames=F, **args)

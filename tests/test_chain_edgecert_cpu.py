"""CPU: the certificate of roadmap edges and polylines of environment/edge_certificate.py (edge_half_steps, certify_joint_edge,
polyline_nodes, certify_polylines, certify_polylines_host), the rehearsal of every case of tests/test_chain_edgecert_gpu.py with a
float32 restatement in the kernel's place, the soundness of a certificate against densely sampled poses, the rounds against a fake
evaluator, and the plumbing and refusals of ManipulatorFramework.certify_joint_paths."""
import os
import re

import numpy as np
import pytest

import chain_edgecert_common as E
import chain_roadmap_common as R
import chain_rollout_common as C
from conftest import ROOT
from test_chain_roadmap_cpu import ARGUMENT_ERRORS, planar_framework

from robotic_manipulator_rloa_amd.environment import kinematic as KIN
from robotic_manipulator_rloa_amd.environment.edge_certificate import (EDGE_CERT_FLOATS, PathCertificates, certify_joint_edge,
                                                                       certify_polylines, certify_polylines_host, edge_half_steps,
                                                                       polyline_nodes)
from robotic_manipulator_rloa_amd.environment.kinematic import JointPaths, check_joint_edge, edge_pose, reach_table


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planar3", "iiwa_like7", "slider4"])
def test_edge_half_steps_against_a_loop_written_out(name):
    """Per segment and per pair: beta = 1/2 sum_m |b_m - a_m| / (S - 1) R[m][.] over the joints that move the segment against the
    world, or the pair's far segment against its near one. slider4: a prismatic joint's reach is 1, so a segment that only
    prismatic joints carry travels |dq| / (2 (S - 1)) per joint."""
    model, twin = R.arm(name)
    rng = np.random.default_rng(3)
    lo, hi = C.limits_of(model)
    a, b = rng.uniform(lo, hi, (5, model.A)), rng.uniform(lo, hi, (5, model.A))
    S, Rt = 192, reach_table(model).astype(np.float64)
    got = edge_half_steps(model, a, b, S)
    n_seg = len(model.segments)
    assert got.shape == (5, n_seg + len(model.self_pairs))
    for k in range(5):
        for s, seg in enumerate(model.segments):
            want = sum(0.5 * abs(b[k, m] - a[k, m]) / (S - 1) * Rt[m, s] for m in range(min(seg.frame, model.A)))
            assert abs(got[k, s] - want) <= 1e-15 + 1e-12 * want
        for p, (s, t) in enumerate(model.self_pairs):
            want = sum(0.5 * abs(b[k, m] - a[k, m]) / (S - 1) * Rt[m, t] for m in range(model.segments[s].frame, model.segments[t].frame))
            assert abs(got[k, n_seg + p] - want) <= 1e-15 + 1e-12 * want
    assert np.array_equal(got, edge_half_steps(model, b, a, S))                      # an edge's table does not depend on its direction
    if name == "slider4":
        prismatic = np.array([j.type == KIN.PRISMATIC for j in model.joints])
        assert prismatic.any()
        for s, seg in enumerate(model.segments):
            moved = np.arange(model.A) < seg.frame
            if moved.any() and prismatic[moved].all():
                assert np.allclose(got[:, s], np.abs(b - a)[:, moved].sum(axis=1) / (2 * (S - 1)), rtol=1e-12, atol=0)
        assert np.all(Rt[prismatic][:, :][Rt[prismatic] > 0] == 1.0)


def test_certify_joint_edge_record_and_direction():
    """[0 .. 7] are check_joint_edge's exactly; [8 .. 10] are the minima of path_slacks with the one table; [11] names the first low
    sample; a kind without tests reads +inf; reversed, the minima are the same and the indices count from the other end."""
    model, twin = R.arm("iiwa_like7")
    case = R.build_case("iiwa_like7", 3, 5, 128, verify=False)
    a, b = case.ends()
    rec = certify_joint_edge(twin, a, b, case.obstacles[:, None, :], 128, case.margin)
    assert rec.shape == (3, 10, EDGE_CERT_FLOATS) and EDGE_CERT_FLOATS == 12
    assert np.array_equal(rec[..., :8], check_joint_edge(twin, a, b, case.obstacles[:, None, :], 128, case.margin))
    s = E.slacks_at(case, edge_pose(a[:, :, None, :], b[:, :, None, :], np.arange(128), 128))
    assert np.array_equal(rec[..., 8:11], s.min(axis=2))
    low = np.any(s < case.margin, axis=-1)
    assert np.array_equal(rec[..., 11], np.where(low.any(axis=-1), np.argmax(low, axis=-1), -1))
    assert np.all(rec[..., 4][rec[..., 11] == -1] == 0) and np.all(rec[..., 8:11] < rec[..., 0:3])
    back = certify_joint_edge(twin, b, a, case.obstacles[:, None, :], 128, case.margin)
    assert np.allclose(back[..., 8:11], rec[..., 8:11], rtol=0, atol=1e-12) and np.array_equal(back[..., 11] == -1, rec[..., 11] == -1)
    bare = R.arm("slider4")[1]
    q = np.zeros((2, bare.model.A))
    assert np.all(np.isposinf(certify_joint_edge(bare, q[0], q[1], [5.0, 5.0, 5.0], 64)[[9, 10]]))
    forced = certify_joint_edge(twin, a, b, case.obstacles[:, None, :], 128, case.margin, poses=R.edge_pose32(a, b, 128).astype(np.float64))
    assert np.array_equal(forced[..., :8], rec[..., :8]) and np.abs(forced[..., 8:11] - rec[..., 8:11]).max() < 1e-5


# ---- the float32 rehearsal -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,V,S", E.CASES)
def test_rehearsal(name, N, V, S):
    """Every GPU case with the float32 restatement in the kernel's place: the case builds (the twin alone meets the 1 % cap and, from
    64 edges up, the floors of certified, blocked and free-yet-uncertified edges — at the seed chain_edgecert_common.SEED records,
    which the GPU suite builds unverified), beta32 lies within 2^-20 of the rule's table, and the restatement's twelve floats pass
    the check_records the kernel's will."""
    case = E.build(name, N, V, S)
    if N * case.E >= 64:
        assert case.seed == E.SEED[(name, N, V, S)]
        again = E.build(name, N, V, S, verify=False)
        assert np.array_equal(again.nodes, case.nodes) and np.array_equal(again.obstacles, case.obstacles)
    b32, b64 = E.beta32(case).astype(np.float64), E.betas_of(case)
    assert np.all(np.abs(b32 - b64) <= 2.0 ** -20 * b64.max(axis=-1, keepdims=True))
    out, poses = E.record32(case)
    E.check_records(case, out, poses)


# ---- soundness: what the feature exists for -----------------------------------------------------------------------------------------
# The margins of the soundness test. At chain_path_common.MARGINS' margin (0.005 for iiwa_like7, 0 for planar3) the twin certifies
# EVERY 'roadmap' polyline of the committed query sets, shortened or not, after 0 to 3 refinements — no mix, and a lower margin
# only certifies more. The mix therefore comes from a second, HIGHER margin per set, chosen on the CPU with the twin alone between
# the smallest and the largest sampled minimum clearance of the sets' 'roadmap' polylines (min over the three kinds, in mm):
#   planar3    : 7.5, 21.5, 22.6, 42.5  |  with shortcut 7.2, 7.3, 7.5, 22.6   ->  margin 0.015: 3 certified + 1 blocked | 1 + 3
#   iiwa_like7 : 8.7, 13.3, 30.5, 34.8  |  with shortcut 8.6, 13.9, 17.7, 30.5 ->  margin 0.020: 2 certified + 2 blocked | 1 + 3
# A polyline with a sample below the margin is 'blocked'; one that keeps a centimetre more than the margin is certified once its
# half-steps, which halve with every refinement, are small enough.
RAISED = {"planar3": 0.015, "iiwa_like7": 0.020}
DENSE = 4096


@pytest.mark.parametrize("name,cut", [("planar3", None), ("iiwa_like7", R.IIWA_CUT)])
@pytest.mark.parametrize("shortcut", [0, E.SHORTCUT])
def test_a_certified_polyline_keeps_the_margin_at_every_pose(name, cut, shortcut):
    """For every polyline certify_polylines_host certifies on chain_roadmap_common's query sets (value_paths(name, ROADMAP, cut)),
    without and with shortcut=16, of every kind at the planning margin and the 'roadmap' ones at the raised margin: the twin's three
    clearances at 4096 uniformly spaced poses of every leg are all >= the margin. Vacuous, and failing, unless over the two margins
    at least one 'roadmap' polyline is certified and at least one ends otherwise."""
    twin = R.arm(name)[1]
    paths, ob, margin = E.polyline_paths(name, shortcut, cut)
    nodes, count = polyline_nodes(paths)
    roadmap = paths.outcome == "roadmap"
    certified_roadmaps = other_roadmaps = 0
    for m, which in ((margin, np.ones(len(count), bool)), (RAISED[name], roadmap)):
        cert = certify_polylines_host(twin, paths, ob, m, R.VALUE_KW["resolution"])
        print(name, "shortcut", shortcut, "margin", m, {o: int(np.sum(cert.outcome[roadmap] == o)) for o in sorted(set(cert.outcome[roadmap]))},
              "of the roadmaps;", {o: int(np.sum(cert.outcome == o)) for o in sorted(set(cert.outcome))}, "of all; refinements",
              cert.refinements[roadmap].tolist())
        certified_roadmaps += int(np.sum(cert.certified & roadmap))
        other_roadmaps += int(np.sum(~cert.certified & roadmap))
        assert np.array_equal(cert.outcome == "none", count < 2) and np.array_equal(cert.certified, cert.outcome == "certified")
        assert np.all(cert.slack[cert.certified] >= m)
        for q in np.nonzero(cert.certified & which)[0]:
            poly = C.f32(nodes[q, :count[q]])
            dense = E.dense_leg_margins(twin, poly, C.f32(ob[q]), DENSE)
            assert dense.min() >= m, (q, float(dense.min()), m)
            assert dense.min() >= cert.slack[q]                 # (the slack is a lower bound on what any pose keeps)
    assert certified_roadmaps >= 1 and other_roadmaps >= 1, (certified_roadmaps, other_roadmaps)


def test_the_missed_contact():
    """chain_edgecert_common.missed_contact: the obstacle midway between samples 10 and 11 of one planar3 edge at S = 64.
    check_joint_edge says free, certify_joint_edge names a sample, and certify_polylines_host never answers 'certified': at every
    S the pose the obstacle sits on is in the edge, so either a sample sees it ('blocked') or none is certified."""
    case, orad = E.missed_contact()
    a, b = case.nodes[0, 0], case.nodes[0, 1]
    assert check_joint_edge(case.twin, a, b, case.obstacles[0], 64, case.margin)[4] == 0
    rec = certify_joint_edge(case.twin, a, b, case.obstacles[0], 64, case.margin)
    assert rec[4] == 0 and rec[3] == -1 and rec[11] >= 0 and rec[8] < case.margin and rec[6] >= 0.05
    N = 1
    paths = JointPaths(np.array(["roadmap"]), np.full(N, -1), np.full((N, 3), np.nan), np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N),
                       np.zeros(N), np.full(N, -1), np.zeros(N), np.full(N, 64), a[None], b[None], np.zeros(N, bool), np.zeros(N),
                       np.zeros(N, np.int64))
    paths.nodes, paths.n_nodes = np.stack([a, b])[None], np.array([2])
    cert = certify_polylines_host(case.twin, paths, case.obstacles, case.margin, resolution=1.0)
    print(cert.outcome, cert.samples, cert.refinements, cert.slack)
    assert cert.outcome[0] in ("blocked", "sampled") and not cert.certified[0]
    dense = E.dense_leg_margins(case.twin, case.nodes[0], case.obstacles[0], 4096)
    assert dense.min() < case.margin


# ---- the rounds ----------------------------------------------------------------------------------------------------------------------
def test_rounds_with_a_fake_evaluator():
    """Groups are formed before they run; an open query is doubled once per round and all its legs with it; a blocked query is never
    reopened; 'none' queries are never passed to run; S stops at 2048 and the query is then 'sampled'."""
    A = 2
    nodes = np.full((6, 4, A), np.nan)
    count = np.array([2, 3, 0, 4, 2, 3])
    for q, k in enumerate(count):
        nodes[q, :k] = np.linspace(0.0, 0.4 + 0.1 * q, k)[:, None] if k else np.nan
    calls = []
    # query 0: certified at once | 1: certified at 4 x its first S | 2: none | 3: blocked in round 2 | 4: never certified | 5: blocked at once
    first = {}

    def run(queries, nodes32, edges, S):
        assert nodes32.dtype == np.float32 and edges.dtype == np.int32 and np.array_equal(edges[:, 1], edges[:, 0] + 1)
        calls.append((tuple(int(q) for q in queries), nodes32.shape[1], int(S)))
        out = np.zeros((len(queries), len(edges), 12))
        out[..., 8:11], out[..., 11], out[..., 6] = 1.0, -1.0, 1.0 / S
        for k, q in enumerate(queries):
            first.setdefault(int(q), int(S))
            assert not np.isnan(nodes32[k]).any()
            if q == 1 and S < 4 * first[1]:
                out[k, 1, 11], out[k, 1, 8] = 5.0, -0.25
            if q == 3:
                out[k, 0, 11] = 7.0
                if S > first[3]:
                    out[k, 2, 4], out[k, 2, 3] = 2.0, 9.0
            if q == 4:
                out[k, 0, 11], out[k, 0, 9] = 0.0, -0.5
            if q == 5:
                out[k, 1, 4], out[k, 1, 11] = 1.0, 3.0
        return out

    cert = certify_polylines(run, nodes, count, 0.02, 1 << 23, np.float64)
    assert isinstance(cert, PathCertificates) and cert._fields == (
        "outcome", "certified", "slack", "leg_slack", "weakest_leg", "min_clearance", "min_self_clearance", "min_cell_clearance",
        "samples", "sample_step", "refinements")
    assert cert.outcome.tolist() == ["certified", "certified", "none", "blocked", "sampled", "blocked"]
    assert cert.refinements.dtype == np.int64 and cert.refinements.tolist() == [0, 2, 0, 1, 5, 0]
    assert cert.samples.tolist() == [64, 256, 0, 128, 2048, 64] and cert.certified.tolist() == [True, True, False, False, False, False]
    assert not any(2 in qs for qs, _, _ in calls)
    seen = {q: [S for qs, _, S in calls if q in qs] for q in (0, 1, 3, 4, 5)}
    assert seen == {0: [64], 1: [64, 128, 256], 3: [64, 128], 4: [64, 128, 256, 512, 1024, 2048], 5: [64]}
    # the first round's groups: (K, S) in order, all formed from the state before any ran — queries 0 and 4 share one launch
    assert calls[:3] == [((0, 4), 2, 64), ((1, 5), 3, 64), ((3,), 4, 64)]
    assert calls[3:6] == [((4,), 2, 128), ((1,), 3, 128), ((3,), 4, 128)]
    assert np.isnan(cert.slack[2]) and cert.weakest_leg.tolist() == [0, 0, -1, 0, 0, 0] and cert.leg_slack.shape == (6, 3)
    assert cert.slack[4] == -0.5 and np.isnan(cert.leg_slack[0, 1:]).all() and np.isnan(cert.sample_step[2])
    # a budget of one query's legs at a time cuts a group into chunks; nothing else changes
    calls.clear()
    small = certify_polylines(run, nodes, count, 0.02, 64, np.float32)
    assert calls[:2] == [((0,), 2, 64), ((4,), 2, 64)] and small.outcome.tolist() == cert.outcome.tolist() and small.slack.dtype == np.float32


def test_polyline_nodes_reads_a_joint_paths_as_polyline_plan_does():
    paths, ob, margin = E.polyline_paths("planar3", 0)
    nodes, count = polyline_nodes(paths)
    has, roadmap = paths.candidate >= 0, paths.outcome == "roadmap"
    assert np.array_equal(count, np.where(roadmap, paths.n_nodes, np.where(has, 3, 0))) and nodes.shape[1] == max(count.max(), 2)
    q = int(np.nonzero(has)[0][0])
    assert np.array_equal(nodes[q, :3], np.stack([paths.start[q], paths.via[q], paths.goal[q]])) and np.isnan(nodes[q, 3:]).all()
    r = int(np.nonzero(roadmap)[0][0])
    assert np.array_equal(nodes[r, :count[r]], paths.nodes[r, :count[r]])
    from robotic_manipulator_rloa_amd.environment.polyline import polyline_plan
    plan = polyline_plan(paths, np.asarray(paths.start, float), np.where(has[:, None], paths.via, paths.start),
                         np.where((has | roadmap)[:, None], paths.goal, paths.start), 1.0, 400)
    legs = np.sum(np.asarray(plan.n_ticks) > 0, axis=1)
    assert np.array_equal(legs[count >= 2], count[count >= 2] - 1)


# ---- plumbing and refusals -----------------------------------------------------------------------------------------------------------
def test_header_symbol_and_abi():
    from robotic_manipulator_rloa_amd import _lib
    text = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    assert _lib.header_abi_version() == 40 and re.search(r"^#define NAF_CHAIN_EDGE_CERT_FLOATS 12$", text, re.M)
    name = "naf_chain_edge_certify"
    assert re.search(rf"^int {name}\(naf_chain_env_t\* h, const float\* nodes_dev, const int32_t\* edges_dev,", text, re.M)
    assert name in _lib.EXPORTED_SYMBOLS
    assert len(_lib._PROTOS[name]) == text.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == 15
    lib = _lib.load()
    assert lib.naf_hip_abi_version() == 40 and hasattr(lib, name)
    # argument errors are host code and launch nothing: a fake non-null handle is never dereferenced before they answer
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data
    call = lambda h=p, nodes=p, edges=p, o=p, rad=0.06, reach=p, guard=0.0, N=1, V=2, E=1, S=64, margin=0.0, out=p: (   # noqa: E731
        lib.naf_chain_edge_certify(h, nodes, edges, o, rad, reach, guard, N, V, E, S, margin, out, None, None))
    for kw in ARGUMENT_ERRORS + EXTRA_ERRORS:
        assert call(**kw) == -1, kw


# what naf_chain_edge_certify refuses beyond naf_chain_edge_check's list
EXTRA_ERRORS = (dict(reach=None), dict(guard=-1e-6), dict(guard=float("nan")), dict(guard=float("inf")))


def test_certify_joint_paths_on_the_host_and_its_refusals():
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    f = planar_framework()
    paths, ob, margin = E.polyline_paths("planar3", E.SHORTCUT)
    got = f.certify_joint_paths(paths, obstacles=ob, clearance_margin=RAISED["planar3"], resolution=R.VALUE_KW["resolution"], on_device=False)
    want = certify_polylines_host(R.arm("planar3")[1], paths, ob, RAISED["planar3"], R.VALUE_KW["resolution"])
    assert isinstance(got, PathCertificates)
    for name, x, y in zip(got._fields, got, want):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    assert got.certified.any() and (got.outcome[paths.outcome == "roadmap"] != "certified").any()
    ok = dict(obstacles=ob, on_device=False)
    for bad in (None, "paths", tuple(paths), paths._replace(start=None)):
        with pytest.raises(InvalidEnvironmentParameter, match=r"paths is the JointPaths that plan_joint_paths\(\) returned"):
            f.certify_joint_paths(bad, **ok)
    wide = paths._replace(start=np.zeros((len(ob), 4)), goal=np.zeros((len(ob), 4)))
    with pytest.raises(InvalidEnvironmentParameter, match=r"paths holds poses of 4 joints, the environment's arm has 3"):
        f.certify_joint_paths(wide, **ok)
    with pytest.raises(InvalidEnvironmentParameter, match=rf"obstacles is \[N\]\[3\] with N = {len(ob)}"):
        f.certify_joint_paths(paths, obstacles=ob[:5], on_device=False)
    for bad in (float("nan"), float("inf"), "0", None):
        with pytest.raises(InvalidEnvironmentParameter, match=r"clearance_margin is a finite length"):
            f.certify_joint_paths(paths, clearance_margin=bad, **ok)
    for bad in (0.0, -0.02, float("nan"), True, None):
        with pytest.raises(InvalidEnvironmentParameter, match=r"resolution is a positive joint-space distance"):
            f.certify_joint_paths(paths, resolution=bad, **ok)
    # plan_joint_paths(roadmap=, certify=True) is still refused with today's words
    q0, q1, _, _ = R.value_queries("planar3")
    with pytest.raises(InvalidEnvironmentParameter, match=r"roadmap=14, certify=True\): roadmap edges are checked at their samples only, "
                                                          r"and nothing certifies a 'roadmap' path between them"):
        f.plan_joint_paths(goal_joint_positions=q1, initial_joint_positions=q0, obstacles=ob, roadmap=14, certify=True, on_device=False)
    # an arm with a prismatic joint that has no limits: reach_table's message, by name
    g = planar_framework()
    joint = next(j for j in g.env.model.joints)
    object.__setattr__(joint, "type", KIN.PRISMATIC)
    object.__setattr__(joint, "limited", False)
    with pytest.raises(InvalidEnvironmentParameter, match=rf"reach_table: prismatic joint {joint.index} has no limits"):
        g.certify_joint_paths(paths, **ok)


def test_the_lds_refusal_points_to_the_twin(monkeypatch):
    """NAF_CHAIN_ERR_LDS from the launch leaves the facade as InvalidEnvironmentParameter whose message names on_device=False
    (the device tool is replaced by one that raises what PolylineCertifier.launch raises for that code)."""
    from robotic_manipulator_rloa_amd import arm_certify, chain_certify
    from robotic_manipulator_rloa_amd.utils.exceptions import InvalidEnvironmentParameter
    f = planar_framework()
    paths, ob, _ = E.polyline_paths("planar3", 0)

    class Refusing:
        def certify(self, *a):
            raise chain_certify.PolylineLdsRefusal("chain_edge_certify: the table does not fit")

    monkeypatch.setattr(f.arm_planner, "tool", lambda kind, factory: Refusing() if kind == "polyline_certificates" else None)
    with pytest.raises(InvalidEnvironmentParameter, match=r"NAF_CHAIN_ERR_LDS\); on_device=False answers this arm"):
        arm_certify.certify_joint_paths(f.arm_planner, paths, ob, 0.0, 0.05, True)

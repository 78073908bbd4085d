"""Shared by tests/test_chain_roadmap_cpu.py and tests/test_chain_roadmap_gpu.py: the arms and cases that hold naf_chain_edge_check
(csrc/chain_env.hip) against the float64 rule of environment/kinematic.py (edge_pose, check_joint_edge), built with the twin alone;
a float32 numpy restatement of the sample poses that stands in for the device in the CPU rehearsal; the checks both suites apply to
what a checker — that restatement, or the kernel — returned; and the query sets of the value test and the end-to-end test."""
import functools

import numpy as np

import chain_ik_common as IK
import chain_path_common as P
import chain_rollout_common as C

from robotic_manipulator_rloa_amd.environment.kinematic import (edge_pose, joint_distance32, joint_paths_host, roadmap_edges,
                                                                roadmap_milestones, roadmap_nodes)

ORAD = C.ORAD
CAP = C.CAP                        # the project's band rule: at most 1 % of a case's samples inside a band
COUNTS = [(1, 2, 64), (3, 5, 128), (8, 16, 256)]      # (N, V, S): one edge, one pass; odd counts, 10 edges, two passes; 960 workgroups
ARMS = P.ARMS                      # planar3 (no pairs, CELL), iiwa_like7 (pairs, CELL + BOX), long12 (pairs, CELL), slider4 (bare)
EXTRA = [("iiwa_like7_bare", 4, 6, 128), ("planar3_boxes", 4, 6, 128)]      # the other two of the six instantiations
MARGINS = P.MARGINS
arm = P.arm


def floor_of(items):
    """edges a case must hold free, and as many blocked: the project's FLOOR of 8 from 64 edges up, a third of them below"""
    return C.FLOOR if items >= 64 else items // 3


# The pose bound. test_chain_roadmap_cpu.test_rehearsal measures, over every sample of every case below, the largest deviation of the
# float32 restatement's pose (edge_pose32: f = float32(i) / float32(S - 1), d = b - a, then f d + a rounded to float32) from
# edge_pose at the same float32 nodes:
#     planar3 3.76e-7, iiwa_like7 4.22e-7, long12 2.04e-7, slider4 3.70e-7, iiwa_like7_bare 4.64e-7, planar3_boxes 4.24e-7
#     ->   POSE_DEVIATION = 5.0e-7, rounded up
# — the rounding of f (2^-24 relative) times the edge's span in a joint, the rounding of d likewise, and half an ulp of the joint
# value itself. An edge between two uniform milestones may span a joint's whole range where §16's legs span a few rad, so
# chain_path_common's constant is not taken over: this one is measured on these cases (it came out no larger). The bound is 8 x
# the measured value, the project's margin for another legal rounding of the one fmaf (numpy has none; the restatement rounds the
# exact product's float64 sum a second time). It is taken from the restatement, never from the kernel.
POSE_DEVIATION = 5.0e-7
POSE_BOUND = 8 * POSE_DEVIATION


def f32(x):
    return C.f32(x)


def edge_pose32(a, b, S):
    """[..., S, A] float32: every sample's pose as the device forms it, from a, b [..., A]"""
    f = np.float32
    a, b = np.asarray(a, f)[..., None, :], np.asarray(b, f)[..., None, :]
    frac = (np.arange(S).astype(f) / f(S - 1)).astype(f)[:, None]
    d = b - a
    assert d.dtype == f and frac.dtype == f
    return (frac.astype(np.float64) * d.astype(np.float64) + a.astype(np.float64)).astype(f)      # (the product is exact in float64)


class Case:
    """N roadmaps of V nodes of one arm, the E edges they share, at S samples; all float32 values held as float64: nodes[N, V, A],
    obstacles[N, 3], margin; edges[E, 2] int32"""

    def __init__(self, name, N, V, S, nodes, obstacles, margin=0.0, edges=None):
        self.name, self.N, self.V, self.S, self.margin = name, N, V, S, margin
        self.model, self.twin = arm(name)
        self.nodes, self.obstacles = nodes, obstacles
        self.edges = roadmap_edges(V) if edges is None else np.asarray(edges, np.int32).reshape(-1, 2)
        self.E = len(self.edges)

    def ends(self):
        """(a, b)[N, E, A]: the end poses of every edge"""
        return self.nodes[:, self.edges[:, 0]], self.nodes[:, self.edges[:, 1]]

    def sub(self, n, edges):
        """the case of query n alone with the given edge list"""
        return Case(self.name, 1, self.V, self.S, self.nodes[n:n + 1], self.obstacles[n:n + 1], self.margin, edges)


def margins_at(case, poses):
    """[N, E, S, 3] float64: the twin's three clearances (the obstacle's minus its radius) at poses[N, E, S, A]"""
    twin = case.twin
    q = np.asarray(poses, np.float64)
    clear = twin.clearance(q, case.obstacles[:, None, None, :]) - ORAD
    zero = np.zeros(clear.shape)
    return np.stack([clear, twin.self_clearance(q) + zero, twin.cell_clearance(q) + zero], axis=-1)


def band_of(case, margins):
    """[N, E, S] bool: a sample one of whose twin clearances lies within the pinned tolerance of the margin — 2 tol for the obstacle
    and the workcell, 4 tol for the pairs (chain_rollout_common.tol_of) — where the device's verdict is not compared"""
    tol = C.tol_of(case.model)
    with np.errstate(invalid="ignore"):
        return np.any(np.abs(margins - case.margin) <= np.array([2 * tol, 4 * tol, 2 * tol]), axis=-1)


# Which reseeding attempt build_case accepted for each case: test_chain_roadmap_cpu.test_rehearsal finds it with the twin (verify=True)
# and holds this table to it, so that the GPU suite can build the same case without evaluating the twin at every sample a second
# time — check_records asserts the cap and the floors again, at the recorded poses.
ATTEMPT = {("planar3", 1, 2, 64): 0, ("planar3", 3, 5, 128): 1, ("planar3", 8, 16, 256): 0,
           ("iiwa_like7", 1, 2, 64): 0, ("iiwa_like7", 3, 5, 128): 2, ("iiwa_like7", 8, 16, 256): 0,
           ("long12", 1, 2, 64): 0, ("long12", 3, 5, 128): 4, ("long12", 8, 16, 256): 0,
           ("slider4", 1, 2, 64): 0, ("slider4", 3, 5, 128): 0, ("slider4", 8, 16, 256): 0,
           ("iiwa_like7_bare", 4, 6, 128): 0, ("planar3_boxes", 4, 6, 128): 0}


@functools.lru_cache(maxsize=None)
def build_case(name, N, V, S, seed=0, verify=True):
    """Nodes 0 and 1 of every query are seeded free poses (chain_ik_common.free_poses), the others roadmap_milestones' (none at
    V = 2). Every second query's obstacle, from query 0 on, sits on the end effector of the straight line's middle pose — edge
    (0, 1) runs into it, and so do the edges that pass nearby; the other queries' is out of the way, where the workcell and the arm
    itself are what blocks; for an arm without a workcell, which little else blocks, it sits on the end effector of node 2, the first
    milestone, and blocks every edge into that node. The margin is chain_path_common.MARGINS'. Reseeded until the twin alone meets
    the cap and the floors at the restatement's poses; verify=False builds ATTEMPT's without asking the twin."""
    model, twin = arm(name)
    for attempt in range(60) if verify else [ATTEMPT[(name, N, V, S)]]:
        rng = np.random.default_rng(9300 + 977 * N + 31 * V + S + 10007 * attempt + seed)
        q = IK.free_poses(model, twin, rng, 2 * N)
        a, b = q[:N], q[N:]
        nodes = roadmap_nodes(a, b, roadmap_milestones(model, a, b, V - 2, seed=int(rng.integers(1 << 30)))).astype(np.float64)
        ob = np.tile(C.away(model)[1], (N, 1))
        mid = twin.end_effector(0.5 * (nodes[:, 0] + nodes[:, 1]))
        ob[0::2] = mid[0::2]
        if not model.cell_pairs:
            ob[1::2] = twin.end_effector(nodes[:, min(2, V - 1)])[1::2]
        case = Case(name, N, V, S, nodes, f32(ob), margin=MARGINS.get(name, 0.0))
        case.attempt = attempt
        if not verify:
            return case
        m = margins_at(case, edge_pose32(*case.ends(), S))
        blocked = np.any(m < case.margin, axis=-1).any(axis=-1)
        enough = min(int(blocked.sum()), int((~blocked).sum())) >= floor_of(N * case.E)
        if band_of(case, m).sum() <= CAP * N * case.E * S and enough:
            return case
    raise AssertionError(f"{name} N={N} V={V} S={S}: no seed meets the cap and the floors")


def record32(case):
    """What naf_chain_edge_check returns, by the restatement: (out[N E, 8] float32, poses[N E, S, A] float32) — the twin's
    clearances at edge_pose32's poses, rounded to float32"""
    N, E, S = case.N, case.E, case.S
    a, b = case.ends()
    poses = edge_pose32(a, b, S)
    m = margins_at(case, poses).astype(np.float32)
    blocked = np.any(m < np.float32(case.margin), axis=-1)
    length = joint_distance32(b, a)
    out = np.empty((N, E, 8), np.float32)
    out[..., :3] = m.min(axis=2)
    out[..., 3] = np.where(blocked.any(axis=-1), np.argmax(blocked, axis=-1), -1)
    out[..., 4] = blocked.sum(axis=-1)
    out[..., 5] = length
    out[..., 6] = length / np.float32(S - 1)
    out[..., 7] = 0.0
    return out.reshape(N * E, 8), poses.reshape(N * E, S, -1)


def check_records(case, out, poses, floors=True):
    """The teacher-forced test and the verdicts on one case, in the manner of chain_path_common.check_records. poses[N E, S, A]
    within POSE_BOUND of edge_pose; then, with the twin evaluated AT THE RECORDED POSES: the three minima within 2 tol / 4 tol /
    2 tol (+inf where the model has no pairs / no workcell), [5] bit-equal to joint_distance32, [6] within 1 ulp, [7] zero; [3] and
    [4] the twin's for every edge whose samples all lie outside the bands, and bracketed by the twin's sure and possible samples
    where some lie inside (at most CAP of the case's). Returns (largest pose deviation, census)."""
    model, N, E, S = case.model, case.N, case.E, case.S
    tol = C.tol_of(model)
    assert out.dtype == np.float32 and out.shape == (N * E, 8) and poses.dtype == np.float32 and poses.shape == (N * E, S, model.A)
    a, b = case.ends()
    want_pose = edge_pose(a[:, :, None, :], b[:, :, None, :], np.arange(S), S)
    dev = float(np.abs(poses.reshape(N, E, S, -1).astype(np.float64) - want_pose).max())
    print(f"{case.name} N={N} V={case.V} S={S}: largest pose deviation {dev:.2e} (bound {POSE_BOUND:.2e})")
    assert dev <= POSE_BOUND, (dev, POSE_BOUND)
    m = margins_at(case, poses.reshape(N, E, S, -1))
    rec = out.reshape(N, E, 8)
    for k, bound in ((0, 2 * tol), (1, 4 * tol), (2, 2 * tol)):
        got, want = rec[..., k].astype(np.float64), m[..., k].min(axis=2)
        both_inf = np.isposinf(got) & np.isposinf(want)
        err = np.abs(np.where(both_inf, 0.0, got) - np.where(both_inf, 0.0, want))
        assert np.all(err <= bound), (k, float(err.max()), bound)
    if not model.self_pairs:
        assert np.all(np.isposinf(rec[..., 1]))
    if not model.cell_pairs:
        assert np.all(np.isposinf(rec[..., 2]))
    length = joint_distance32(b, a)
    assert np.array_equal(length.view(np.uint32), rec[..., 5].view(np.uint32))
    step = length / np.float32(S - 1)
    assert np.all(np.abs(rec[..., 6] - step) <= np.spacing(step))
    assert np.all(rec[..., 7] == 0)
    # the verdicts
    band = band_of(case, m)
    blocked = np.any(m < case.margin, axis=-1)
    sure, maybe = blocked & ~band, blocked | band
    assert band.sum() <= CAP * N * E * S, (int(band.sum()), N * E * S)
    first_of = lambda x: np.where(x.any(axis=-1), np.argmax(x, axis=-1), S)      # noqa: E731
    got_first = np.where(rec[..., 3] < 0, S, rec[..., 3]).astype(np.int64)
    assert np.all((first_of(maybe) <= got_first) & (got_first <= first_of(sure)))
    assert np.all((sure.sum(axis=-1) <= rec[..., 4]) & (rec[..., 4] <= maybe.sum(axis=-1)))
    clean = ~band.any(axis=-1)
    assert np.array_equal(rec[..., 3][clean], np.where(blocked.any(axis=-1), np.argmax(blocked, axis=-1), -1)[clean])
    assert np.array_equal(rec[..., 4][clean], blocked.sum(axis=-1)[clean])
    census = dict(free=int(np.sum(rec[..., 4] == 0)), blocked=int(np.sum(rec[..., 4] > 0)), in_band=int(band.sum()))
    print(f"{case.name} N={N} V={case.V} S={S}: {census}")
    if floors:
        assert min(census["free"], census["blocked"]) >= floor_of(N * E), f"vacuous: {census}"
    return dev, census


# ---- the value test's query sets ---------------------------------------------------------------------------------------------------
VALUE = {"iiwa_like7": dict(N=96, seed=0, floor=4), "planar3": dict(N=48, seed=0, floor=1)}
VALUE_KW = dict(candidates=16, resolution=0.05, seed=1)
ROADMAP = 14
IIWA_CUT = 24                      # the end-to-end test's cut of the iiwa_like7 set: its first 24 queries, planned as a call of their own


@functools.lru_cache(maxsize=None)
def value_queries(name, cut=None):
    """(q_start[N, A], q_goal[N, A], obstacles[N, 3], margin): seeded free start / goal pairs of `name` (iiwa_like7 among
    chain_box_common's boxes, planar3 between chain_cell_common's walls), every second obstacle on the end effector of the straight
    line's middle pose, the others out of the way; the first `cut` of them"""
    model, twin = arm(name)
    N = VALUE[name]["N"]
    rng = np.random.default_rng(VALUE[name]["seed"])
    q = IK.free_poses(model, twin, rng, 2 * N)
    a, b = q[:N], q[N:]
    ob = np.tile(C.away(model)[1], (N, 1))
    ob[1::2] = twin.end_effector(0.5 * (a + b))[1::2]
    n = N if cut is None else cut
    return a[:n], b[:n], f32(ob)[:n], MARGINS.get(name, 0.0)


@functools.lru_cache(maxsize=None)
def value_paths(name, roadmap, cut=None):
    """joint_paths_host of value_queries(name, cut), with `roadmap` milestones"""
    a, b, ob, margin = value_queries(name, cut)
    return joint_paths_host(arm(name)[1], a, b, ob, margin=margin, roadmap=roadmap, **VALUE_KW)


def edges_free_at_sure_samples(name, paths, obstacles, margin, blocked_only=True):
    """for every 'roadmap' query of `paths`: every edge of its polyline, sampled at the query's S by edge_pose, has no sample
    that the twin shows blocked outside the bands (with blocked_only=False: no blocked sample at all). Returns how many edges."""
    model, twin = arm(name)
    tol, count = C.tol_of(model), 0
    for q in np.nonzero(paths.outcome == "roadmap")[0]:
        poly = np.asarray(paths.nodes[q, :paths.n_nodes[q]], np.float64)
        S = int(paths.samples[q])
        case = Case(name, 1, len(poly), S, poly[None], np.asarray(obstacles, np.float64)[q:q + 1], margin,
                    [(k, k + 1) for k in range(len(poly) - 1)])
        a, b = case.ends()
        m = margins_at(case, edge_pose(a[:, :, None, :], b[:, :, None, :], np.arange(S), S))
        blocked = np.any(m < margin, axis=-1)
        if blocked_only:
            blocked &= ~band_of(case, m)
        assert not blocked.any(), (q, np.argwhere(blocked)[:4])
        assert not np.any(np.isnan(poly)) and np.all(np.isnan(paths.nodes[q, paths.n_nodes[q]:]))
        count += len(poly) - 1
    return count

"""The certificate of straight joint-space edges and of the polylines made of them, between their samples, stated once
in float64 as environment/kinematic.py states the rest: the one table of half-steps an edge has (edge_half_steps), the record of a
certified edge (certify_joint_edge), a JointPaths read as polylines (polyline_nodes), and the ONE control flow that certifies
polylines after the fact, for the device and the twin alike (certify_polylines; certify_polylines_host is its twin backend). It
serves every kind of path plan_joint_paths returns: 'straight', 'via', 'sampled', 'roadmap', shortened or not. numpy only.

kinematic.py takes these names in at its end; this module therefore takes what it needs of kinematic.py inside its functions, not
while it is imported.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np

from .urdf_chain import ChainModel

EDGE_CERT_FLOATS = 12                 # NAF_CHAIN_EDGE_CERT_FLOATS
CERTIFICATE_OUTCOMES = ("certified", "sampled", "blocked", "none")


def edge_half_steps(model: ChainModel, a, b, S: int, reach=None) -> np.ndarray:
    """[..., n_seg + P] float64: the ONE table of half-steps of the straight edges a -> b [..., A] at S samples. An edge has S samples
    at f = i / (S - 1), both ends included, so S - 1 intervals, all with the joint displacement (b - a) / (S - 1). Entry s < n_seg:
    beta[s] = 1/2 sum_m |b_m - a_m| / (S - 1) R[m][s], how far a point of capsule s can travel over half an interval. Entry
    n_seg + p, pair p = (s, t) with frames f_s <= f_t: the same sum over m = f_s .. f_t - 1 with R[m][t] — path_half_steps' span
    rule. Every sample of the edge uses this table; it does not depend on the edge's direction. R is reach_table's, as float32
    holds it."""
    from .kinematic import reach_table
    R = (reach_table(model) if reach is None else np.asarray(reach)).astype(np.float64)
    a, b = np.asarray(a, float), np.asarray(b, float)
    n_seg = len(model.segments)
    W = np.zeros((model.A, n_seg + len(model.self_pairs)))
    W[:, :n_seg] = R
    for p, (s, t) in enumerate(model.self_pairs):
        f_s, f_t = model.segments[s].frame, model.segments[t].frame
        W[f_s:f_t, n_seg + p] = R[f_s:f_t, t]
    return 0.5 * (np.abs(b - a) / (int(S) - 1)) @ W


def certify_joint_edge(twin, a, b, obstacle, S: int, margin: float = 0.0, poses=None, reach=None,
                       guard: Optional[float] = None) -> np.ndarray:
    """[..., EDGE_CERT_FLOATS] float64: [0 .. 7] exactly check_joint_edge's record | [8] [9] [10] the minima over the samples of
    (clearance - beta - guard) per test: the obstacle's (its radius subtracted), the pairs', the workcell's, +inf for a kind without
    tests | [11] the index of the first sample one of whose slacks is < margin, -1: none. The edge is CERTIFIED iff [11] == -1.
    COVERAGE: a pose of an interval is at most half the interval's joint displacement away from the nearer of its two end samples,
    and over half an interval no point of the tested capsule (or pair) travels farther than its beta; so if every test at every
    sample keeps margin + beta (+ guard, what float32 may cost), every pose of the edge keeps margin. It implies [4] == 0. A
    polyline's corner is the last sample of one leg and the first of the next, and each leg tests it with its own beta. An edge's
    certificate does not depend on its direction ([3] and [11] count from a). poses[..., S, A]: evaluate the slacks there instead of
    at edge_pose's (the tests' teacher forcing); [0 .. 7] are edge_pose's in either case."""
    from .kinematic import EDGE_FLOATS, certificate_guard, check_joint_edge, edge_pose, path_slacks
    out = np.empty(np.broadcast_shapes(np.shape(a)[:-1], np.shape(b)[:-1]) + (EDGE_CERT_FLOATS,))
    out[..., :EDGE_FLOATS] = check_joint_edge(twin, a, b, obstacle, S, margin)
    a, b = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float))
    obstacle = np.broadcast_to(np.asarray(obstacle, float), a.shape[:-1] + (3,))
    if poses is None:
        poses = edge_pose(a[..., None, :], b[..., None, :], np.arange(S), S)
    guard = certificate_guard(twin.model) if guard is None else float(guard)
    beta = edge_half_steps(twin.model, a, b, S, reach)
    slack = path_slacks(twin, poses, obstacle, (beta, beta, beta), guard)      # (one table: whichever the sample picks, it is this)
    low = np.any(slack < margin, axis=-1)
    out[..., 8:11] = slack.min(axis=-2)
    out[..., 11] = np.where(low.any(axis=-1), np.argmax(low, axis=-1), -1)
    return out


class PathCertificates(NamedTuple):
    """What certify_polylines says about the polylines of N queries (ManipulatorFramework.certify_joint_paths). Where `certified`,
    no pose of the polyline, between the samples included, brings a capsule closer than the margin to anything the samples are
    tested against. The certificate is about the capsule model and the polyline; a controller's tracking error is not in it."""
    outcome: np.ndarray             # [N] str: 'certified' | 'sampled' (free at the last round's samples, not certified at 2048) |
                                    # 'blocked' (a sample is below the margin) | 'none' (the query has no path)
    certified: np.ndarray           # [N] bool
    slack: np.ndarray               # [N]: the least of all legs' three slacks at the last round; NaN for 'none'
    leg_slack: np.ndarray           # [N][Kmax - 1]: the least of each leg's three slacks, NaN-padded
    weakest_leg: np.ndarray         # [N] int: the leg with the least slack, the first of equals; -1 for 'none'
    min_clearance: np.ndarray       # [N]: least obstacle clearance over the samples of all legs; NaN for 'none'
    min_self_clearance: np.ndarray  # [N]: ... self-clearance, +inf without pairs
    min_cell_clearance: np.ndarray  # [N]: ... workcell clearance, +inf without a workcell
    samples: np.ndarray             # [N] int: S, the samples per leg at the last round; 0 for 'none'
    sample_step: np.ndarray         # [N]: the largest max-norm distance between neighbouring samples; NaN for 'none'
    refinements: np.ndarray         # [N] int64: how often the query's samples were doubled


def polyline_nodes(paths) -> Tuple[np.ndarray, np.ndarray]:
    """(nodes[N][Kmax][A] float64, NaN-padded, n_nodes[N] int64) of a JointPaths, as polyline.polyline_plan reads it: a one-via
    query (candidate >= 0) gives start, via, goal; a 'roadmap' query gives nodes[:n_nodes]; a query with neither has no path and
    0 nodes. Kmax is at least 2."""
    start = np.asarray(paths.start, np.float64)
    N, A = start.shape
    has = np.asarray(paths.candidate) >= 0
    roadmap = np.asarray(paths.n_nodes) >= 2 if paths.n_nodes is not None else np.zeros(N, bool)
    count = np.where(has, 3, 0).astype(np.int64)
    if roadmap.any():                                         # (paths planned without a roadmap hold no n_nodes at all)
        count[roadmap] = np.asarray(paths.n_nodes)[roadmap]
    nodes = np.full((N, max(int(count.max()) if N else 2, 2), A), np.nan)
    if has.any():
        nodes[has, 0], nodes[has, 1] = start[has], np.asarray(paths.via, np.float64)[has]
        nodes[has, 2] = np.asarray(paths.goal, np.float64)[has]
    for q in np.nonzero(roadmap)[0]:
        nodes[q] = np.nan
        nodes[q, :count[q]] = np.asarray(paths.nodes, np.float64)[q, :count[q]]
    return nodes, count


def certify_polylines(run, nodes, n_nodes, resolution: float, budget: int, dtype) -> PathCertificates:
    """The ONE control flow of certificates for polylines, run by the device (chain_certify.PolylineCertifier) and by the twin
    (certify_polylines_host) alike. nodes[N][Kmax][A] (taken as float32 holds them), n_nodes[N]; run(queries[n], nodes[n][K][A]
    float32, edges[K - 1][2] int32, S) -> records[n][K - 1][EDGE_CERT_FLOATS] checks the given queries (an index array into the
    call's N) at S samples per leg — roadmap_round's evaluator signature. Query n has the legs (l, l + 1), l < K_n - 1, and starts
    at S = edge_samples(its longest leg, resolution). A round groups the open queries by (K, S) and cuts each group into chunks of
    at most `budget` edge-samples (queries x legs x S; a chunk holds at least one query); the groups are formed before any of them
    runs. After a round a query is 'blocked' if a leg has [4] > 0 — final, a sample is below the margin; 'certified' if every leg
    has [11] == -1; otherwise open while S < 2048, to be run again with all its legs at min(2 S, 2048); otherwise 'sampled'.
    Queries with fewer than 2 nodes are 'none' and are never passed to run."""
    from .kinematic import PATH_SAMPLES_MAX, edge_samples, joint_distance32
    nodes32, count = np.asarray(nodes, np.float32), np.asarray(n_nodes, np.int64)
    N, legs_max = len(count), max(nodes32.shape[1] - 1, 1)
    records = np.full((N, legs_max, EDGE_CERT_FLOATS), np.nan, dtype)
    samples, refinements = np.zeros(N, np.int64), np.zeros(N, np.int64)
    outcome = np.full(N, "none", "<U9")
    open_ = count >= 2
    for q in np.nonzero(open_)[0]:
        poly = nodes32[q, :count[q]]
        samples[q] = edge_samples(joint_distance32(poly[1:], poly[:-1]), resolution)
    while open_.any():
        # the round's groups are formed before any of them runs: a query doubled in this round is looked at again in the next one
        groups = [(int(K), int(S), np.flatnonzero(open_ & (count == K) & (samples == S)))
                  for K, S in sorted({(int(k), int(s)) for k, s in zip(count[open_], samples[open_])})]
        for K, S, idx in groups:
            edges = np.stack([np.arange(K - 1), np.arange(1, K)], axis=1).astype(np.int32)
            per = max(1, int(budget) // ((K - 1) * S))
            for k in range(0, len(idx), per):
                part = idx[k:k + per]
                records[part, :K - 1] = run(part, nodes32[part, :K], edges, S)
        for K, S, idx in groups:
            rec = records[idx, :K - 1]
            blocked, certified = np.any(rec[..., 4] > 0, axis=1), np.all(rec[..., 11] == -1, axis=1)
            again = ~blocked & ~certified & (S < PATH_SAMPLES_MAX)
            outcome[idx] = np.where(blocked, "blocked", np.where(certified, "certified", "sampled"))
            open_[idx] = again
            samples[idx[again]] = min(2 * S, PATH_SAMPLES_MAX)
            refinements[idx[again]] += 1
    has = count >= 2
    with np.errstate(invalid="ignore"):
        leg_slack = np.where(np.isnan(records[..., 8]), np.nan, records[..., 8:11].min(axis=-1)).astype(dtype)
    filled = np.where(np.isnan(leg_slack), np.inf, leg_slack)
    nan = lambda x: np.where(has, x, np.nan).astype(dtype)      # noqa: E731
    low = lambda k: nan(np.where(np.isnan(records[..., k]), np.inf, records[..., k]).min(axis=1))      # noqa: E731
    step = np.where(np.isnan(records[..., 6]), -np.inf, records[..., 6]).max(axis=1)
    return PathCertificates(outcome, outcome == "certified", nan(filled.min(axis=1)), leg_slack,
                            np.where(has, np.argmin(filled, axis=1), -1).astype(np.int64), low(0), low(1), low(2), samples, nan(step),
                            refinements)


def certify_polylines_host(twin, paths, obstacles, margin: float = 0.0, resolution: float = 0.02,
                           chunk: Optional[int] = None) -> PathCertificates:
    """certify_polylines through the twin alone, under the device's rule and on the values the device is given: the polylines of
    `paths` (polyline_nodes) and obstacles[N][3] rounded to float32, the poses and the slacks in float64 (certify_joint_edge), a few
    edges at a time as _TwinPaths.edge_records takes them. chunk: the budget of edge-samples per evaluator call (PATH_CHUNK). An arm
    with a prismatic joint that has no limits is refused by name (reach_table)."""
    from .kinematic import PATH_CHUNK, certificate_guard, reach_table
    nodes, count = polyline_nodes(paths)
    ob = np.asarray(obstacles, np.float64).astype(np.float32).astype(np.float64).reshape(len(count), 3)
    reach, guard = reach_table(twin.model), certificate_guard(twin.model)

    def run(queries, nodes32, edges, S):
        q = nodes32.astype(np.float64)
        out = np.empty((len(q), len(edges), EDGE_CERT_FLOATS))
        block = max(1, 65536 // S)
        for n in range(len(q)):
            for k in range(0, len(edges), block):
                e = edges[k:k + block]
                out[n, k:k + block] = certify_joint_edge(twin, q[n, e[:, 0]], q[n, e[:, 1]], ob[queries[n]], S, margin, reach=reach,
                                                         guard=guard)
        return out

    return certify_polylines(run, nodes, count, resolution, PATH_CHUNK if chunk is None else int(chunk), np.float64)

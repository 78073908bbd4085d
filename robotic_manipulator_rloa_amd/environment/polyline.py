"""Polylines of any number of legs, stated once in float64 as environment/kinematic.py states the rest: the time
parametrisation of a polyline (demonstration_plan_legs; demonstration_plan is its case of three nodes), the action of every tick
under a plan (demo_actions), the shortcut round over a 'roadmap' polyline's own subdivided nodes (shortcut_nodes, shortcut_round),
and what the facade needs to turn JointPaths into polylines. numpy only.

kinematic.py takes these names in at its end, so that `kinematic.demo_actions`, `kinematic.shortcut_round` and the others are where
the rest of the rule is; this module therefore takes what it needs of kinematic.py inside its functions, not while it is imported.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from .urdf_chain import DT

DEMO_MAX_LEGS = 63                    # NAF_CHAIN_DEMO_MAX_LEGS: a polyline of at most 64 nodes
SHORTCUT_MIN, SHORTCUT_MAX = 4, 64    # W, the nodes of a shortcut round: 0 is off


# ---- the plan of a polyline ------------------------------------------------------------------------------------------------------
def leg_ticks_and_action(lo, hi, speed) -> Tuple[np.ndarray, np.ndarray]:
    """(n[N] int64, action[N][A] float32) of the legs lo[N][A] -> hi[N][A] (float32), the per-leg rule: a leg of length
    L = joint_distance32 takes n = max(1, ceil(L / (speed DT))) ticks (float64) at the constant action (hi - lo) / (n DT), formed in
    float64 from the float32 end poses and rounded to float32; |a|_inf <= speed (a leg whose rounded action would exceed it — L rounds
    the exact max difference, and the action rounds again — gets one tick more). A leg of length 0 is one tick at action 0."""
    from .kinematic import joint_distance32
    L = joint_distance32(hi, lo).astype(np.float64)
    n = np.maximum(1, np.ceil(L / (float(speed) * DT))).astype(np.int64)
    d = hi.astype(np.float64) - lo.astype(np.float64)
    act = (d / (n * DT)[:, None]).astype(np.float32)
    over = np.max(np.abs(act), axis=-1) > np.float32(speed) if len(lo) else np.zeros(0, bool)
    n = n + over
    return n, np.where(over[:, None], (d / (n * DT)[:, None]).astype(np.float32), act)


def demonstration_plan_legs(nodes, n_nodes, speed: float = 1.0, frames: int = 400):
    """nodes [N][K][A] (taken as float32 holds them, NaN behind n_nodes[n]), n_nodes [N] in 2 .. 64 -> the DemonstrationPlan of the
    polylines: leg l of query n runs nodes[n][l] -> nodes[n][l + 1] under leg_ticks_and_action, for l < n_nodes[n] - 1; the legs
    behind a query's last are padding, 0 ticks at action 0. n_ticks is [N][K - 1] and leg_actions [N][K - 1][A]; every real leg
    takes at least one tick; rows = min(sum of the ticks, frames)."""
    from .kinematic import DEMO_MAX_TICKS, DemonstrationPlan, demonstration_speed_ok
    if not demonstration_speed_ok(speed):
        raise ValueError(f"speed is a share of the unit action, 0 < speed <= 1: got {speed!r}")
    if isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or not 1 <= frames <= DEMO_MAX_TICKS:
        raise ValueError(f"frames is a number of steps from 1 to {DEMO_MAX_TICKS}: got {frames!r}")
    nodes = np.asarray(nodes, np.float32)
    if nodes.ndim != 3:
        raise ValueError(f"nodes is [N][K][A]: got shape {nodes.shape}")
    N, K, A = nodes.shape
    count = np.asarray(n_nodes)
    if count.shape != (N,) or not np.issubdtype(count.dtype, np.integer) or (N and (count.min() < 2 or count.max() > min(K, DEMO_MAX_LEGS + 1))):
        raise ValueError(f"n_nodes is [N] node counts from 2 to {DEMO_MAX_LEGS + 1}, within the K = {K} nodes given: got {n_nodes!r}")
    legs = max(K - 1, 1)
    ticks, acts = np.zeros((N, legs), np.int64), np.zeros((N, legs, A), np.float32)
    for l in range(K - 1):
        real = count - 1 > l
        ticks[real, l], acts[real, l] = leg_ticks_and_action(nodes[real, l], nodes[real, l + 1], speed)
    if N and (ticks.max() > 1 << 20 or not np.all(np.isfinite(acts))):
        raise ValueError("demonstration_plan: a leg is too long for this speed, or a pose is not finite")
    return DemonstrationPlan(nodes[:, 0].copy(), acts, ticks.astype(np.int32), np.minimum(ticks.sum(axis=1), int(frames)))


def demo_actions(plan, T: int) -> np.ndarray:
    """[N][T][A] float64: a_t of every demonstration — tick t takes leg min(K_n - 1, #{l : e_l <= t}), e_l the cumulative tick
    counts and K_n the query's real legs (those up to its last count above 0). For two legs: leg 1's action for t < n1, leg 2's
    after (also past the last planned tick: never used)"""
    ticks = np.asarray(plan.n_ticks, np.int64)
    ends = np.cumsum(ticks, axis=1)
    real = np.maximum(ticks.shape[1] - np.argmax(ticks[:, ::-1] > 0, axis=1), 1)
    leg = np.minimum(np.sum(ends[:, None, :] <= np.arange(T)[None, :, None], axis=2), real[:, None] - 1)
    return np.take_along_axis(np.asarray(plan.leg_actions), leg[:, :, None], axis=1).astype(np.float64)


# ---- the shortcut round: a roadmap polyline searched again over its own subdivided nodes -----------------------------------------
def shortcut_size_ok(W) -> bool:
    return isinstance(W, (int, np.integer)) and not isinstance(W, bool) and (W == 0 or SHORTCUT_MIN <= W <= SHORTCUT_MAX)


def check_shortcut(prefix: str, shortcut, roadmap) -> None:
    """plan_paths' refusals of `shortcut`, in the backend's words"""
    if not shortcut_size_ok(shortcut):
        raise ValueError(f"{prefix}shortcut is a number of nodes, 0 or from {SHORTCUT_MIN} to {SHORTCUT_MAX}: got {shortcut!r}")
    if shortcut and not roadmap:
        raise ValueError(f"{prefix}shortcut shortens 'roadmap' polylines: shortcut > 0 needs roadmap > 0")


def shortcut_nodes(polyline, W: int) -> np.ndarray:
    """[max(W, K)][A] float32: the nodes of the shortcut round of polyline[K][A] (float32 values), in roadmap_search's convention —
    node 0 the start, node 1 the goal — and nodes 2 .. in path order: the polyline's K - 2 corners and, between them, W - K
    subdivision points. The points are handed out one at a time to the leg l whose current piece L_l / (c_l + 1) is longest
    (L_l = joint_distance32, c_l the points it holds so far; the lowest l among equals) and lie at a + (i / (c_l + 1)) (b - a),
    i = 1 .. c_l, formed in float64 from the float32 nodes and rounded to float32. W <= K leaves the corners only."""
    from .kinematic import joint_distance32
    poly = np.asarray(polyline, np.float32)
    K = len(poly)
    L = joint_distance32(poly[1:], poly[:-1]).astype(np.float64)
    c = np.zeros(K - 1, np.int64)
    for _ in range(max(int(W) - K, 0)):
        c[int(np.argmax(L / (c + 1)))] += 1                  # (argmax: the first of equal maxima, the lowest l)
    inner = []
    for l in range(K - 1):
        a, b = poly[l].astype(np.float64), poly[l + 1].astype(np.float64)
        inner += [(a + (i / (c[l] + 1)) * (b - a)).astype(np.float32) for i in range(1, c[l] + 1)]
        if l < K - 2:
            inner.append(poly[l + 1])
    return np.stack([poly[0], poly[-1]] + inner).astype(np.float32)


def shortcut_round(base, W: int, resolution: float, budget: int, run, dtype):
    """The shortcut round behind roadmap_round's `base` (JointPaths), on the device and through the twin alike, for its 'roadmap'
    queries and no others; W = 0: `base` as it is. shortcut_nodes of each polyline, all pairs of them as edges (roadmap_edges), the
    chunks of roadmap_chunks and run(queries[n], nodes[n][V][A] float32, edges, S) -> records[n][E][EDGE_FLOATS] per chunk —
    roadmap_round's evaluator — then roadmap_search. A polyline is replaced iff a path was found whose float32 length is strictly
    below the old one (max-norm ties are common, and a tie keeps the old polyline with its fewer nodes; so does a polyline already as
    short as the straight line); length, the three minima, sample_step, samples, nodes and n_nodes are then its new edges', as
    gather_roadmap_paths sets them, and the outcome stays 'roadmap'. Queries whose polylines have more than W nodes are searched
    over their own nodes, grouped by node count. Sets roadmap_length and shortcut_free_edges. One round."""
    from .kinematic import EDGE_FLOATS, roadmap_chunks, roadmap_edge_lengths, roadmap_edges, roadmap_search
    if not W:
        return base
    N, A = len(base.outcome), np.asarray(base.start).shape[1]
    todo = np.nonzero(np.asarray(base.outcome) == "roadmap")[0]
    old_nodes, count = np.asarray(base.nodes), np.array(base.n_nodes)
    fields = {name: np.array(getattr(base, name)) for name in ("length", "min_clearance", "min_self_clearance", "min_cell_clearance",
                                                               "sample_step", "samples")}
    before, free_edges = np.full(N, np.nan, fields["length"].dtype), np.full(N, -1, np.int64)
    before[todo] = fields["length"][todo]
    polylines = {q: old_nodes[q, :count[q]] for q in todo}
    sizes = np.maximum(int(W), count[todo])
    for V in np.unique(sizes):
        group = todo[sizes == V]
        edges = roadmap_edges(V)
        edge_of = {(int(i), int(j)): e for e, (i, j) in enumerate(edges)}
        nodes = np.stack([shortcut_nodes(polylines[q], int(W)) for q in group])
        records, samples = np.empty((len(group), len(edges), EDGE_FLOATS), dtype), np.zeros(len(group), np.int64)
        for first, n, S in roadmap_chunks(roadmap_edge_lengths(nodes, edges), resolution, budget):
            records[first:first + n], samples[first:first + n] = run(group[first:first + n], nodes[first:first + n], edges, S), S
        found, index, length = roadmap_search(records, edges, int(V))
        free_edges[group] = np.sum(records[..., 4] == 0, axis=1)
        for k in np.nonzero(found > 0)[0]:
            q, path = group[k], index[k, :found[k]]
            # No polyline is shorter than the straight line (the triangle inequality); one that is as long as it already cannot be
            # shortened, though a float32 sum over more edges may come out an ulp below it: roadmap_search's refinement.
            old = np.float32(fields["length"][q])
            if not np.float32(length[k]) < old or old <= np.float32(base.straight_length[q]):
                continue
            rows = records[k, [edge_of[(min(i, j), max(i, j))] for i, j in zip(path[:-1], path[1:])]]
            count[q], polylines[q] = found[k], nodes[k, path]
            fields["length"][q], fields["samples"][q] = length[k], samples[k]
            fields["min_clearance"][q], fields["min_self_clearance"][q] = rows[:, 0].min(), rows[:, 1].min()
            fields["min_cell_clearance"][q], fields["sample_step"][q] = rows[:, 2].min(), rows[:, 6].max()
    out = base._replace(**fields)
    K = int(count.max()) if N else 0
    out.nodes = np.full((N, K, A), np.nan, old_nodes.dtype)
    for q, poly in polylines.items():
        out.nodes[q, :len(poly)] = poly
    out.n_nodes, out.roadmap_length, out.shortcut_free_edges = count, before, free_edges
    return out


# ---- JointPaths as polylines: what arm_planner.ArmPlanner asks ---------------------------------------------------------------------
def roadmap_arguments(roadmap, shortcut) -> dict:
    """the keywords plan_joint_paths takes for them, none that is off"""
    return {k: int(v) for k, v in (("roadmap", roadmap), ("shortcut", shortcut)) if v}


def pad_shortcut(out, found, ok, kind, shortcut) -> None:
    """the shortcut round's attributes of `found` (JointPaths of the queries ok[N], or None) into `out` of all N, padded as nodes is"""
    if shortcut:
        N = len(ok)
        out.roadmap_length, out.shortcut_free_edges = np.full(N, np.nan, kind), np.full(N, -1, np.int64)
        if found is not None:
            out.roadmap_length[ok], out.shortcut_free_edges[ok] = found.roadmap_length, found.shortcut_free_edges


def roadmap_queries(paths, polylines) -> np.ndarray:
    """[N] bool: the queries of `paths` whose path is a 'roadmap' polyline, none unless polylines are asked for"""
    N = len(paths.candidate)
    return np.asarray(paths.n_nodes) >= 2 if polylines and paths.n_nodes is not None else np.zeros(N, bool)


def polyline_plan(paths, start, via, goal, speed: float, frames: int):
    """the plan of every query of `paths` as a polyline: start, via, goal of a one-via query (candidate >= 0), the nodes of a
    'roadmap' query; one without either stands still at its start pose, two nodes"""
    has, roadmap = np.asarray(paths.candidate) >= 0, roadmap_queries(paths, True)
    count = np.where(has, 3, 2).astype(np.int64)
    count[roadmap] = np.asarray(paths.n_nodes)[roadmap]
    N, A = start.shape
    nodes = np.full((N, int(count.max()) if N else 2, A), np.nan)
    nodes[:, 0], nodes[:, 1] = start, start
    if has.any():
        nodes[has, 1], nodes[has, 2] = via[has], goal[has]
    for q in np.nonzero(roadmap)[0]:
        nodes[q, :count[q]] = np.asarray(paths.nodes, np.float64)[q, :count[q]]
    return demonstration_plan_legs(nodes, count, speed, frames)

"""The certificate of a joint path between its samples, stated once in float64 as environment/kinematic.py states the rest (DESIGN
§18): how far a joint can carry a capsule (reach_table), the half-steps of a start -> via -> goal polyline (path_half_steps), the
slacks at its samples (path_slacks, certify_joint_path), the choice among certified candidates and the refinement rounds
(select_certified_path, certify_rounds). environment/edge_certificate.py builds the certificate of roadmap edges on it. numpy only.

kinematic.py takes these names in at its end, so that `kinematic.reach_table`, `kinematic.certify_rounds` and the others are where
they were; this module therefore takes what it needs of kinematic.py inside its functions, not while it is imported.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from .urdf_chain import PRISMATIC, ChainModel


# ---- certified joint paths: the samples, and a statement about the poses between them (include/naf_hip.h) --------------------------
def _round_up32(x) -> np.ndarray:
    """float32 values none of which is below the float64 x"""
    x = np.asarray(x, np.float64)
    y = x.astype(np.float32)
    return np.where(y.astype(np.float64) < x, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


def reach_table(model: ChainModel) -> np.ndarray:
    """[A][n_seg] float32: R[m][s] bounds, at every pose inside the limits, the distance from joint m's axis to any point of capsule
    s's axis — so a point of capsule s moves at most |dq_m| R[m][s] when joint m alone turns by dq_m. 0 where joint m does not move
    segment s (m >= its frame); 1 for a prismatic joint m (every point it carries moves by |dq_m| exactly); for a revolute joint m
        R[m][s] = max(|a_s|, |b_s|) + sum_{k = m+1 .. frame_s - 1} (|pre_xyz_k| + ext_k),   ext_k = max(|lower_k|, |upper_k|)
    for a prismatic joint k and 0 otherwise. Proof: joint m's axis passes through the origin o_{m+1} of frame m + 1 (a revolute
    joint leaves its frame's origin where it is). A point x of the capsule's axis is o_f + R_f c with c on the segment a_s b_s,
    f = frame_s, and o_{k+1} = o_k + R_k pre_xyz_k + (prismatic k: its unit axis times q_k), so by the triangle inequality
    |x - o_{m+1}| <= sum_k (|pre_xyz_k| + |q_k| [prismatic]) + |c|, |c| <= max(|a_s|, |b_s|) on a segment, |q_k| <= ext_k inside
    the limits; the distance to the axis is at most the distance to a point on it. The capsule's radius plays no part: the capsule
    moves with its axis. Formed in float64, every entry rounded UP to float32. A model with an unlimited prismatic joint is
    refused: its ext is unbounded."""
    A, segs = model.A, model.segments
    ext = np.zeros(A)
    for k, j in enumerate(model.joints):
        if j.type == PRISMATIC:
            if not j.limited or not np.isfinite([j.lower, j.upper]).all():
                raise ValueError(f"reach_table: prismatic joint {j.index} has no limits, so no bound on how far it carries its links")
            ext[k] = max(abs(j.lower), abs(j.upper))
    hop = np.array([np.linalg.norm(j.pre_xyz) for j in model.joints]) + ext
    R = np.zeros((A, len(segs)))
    for s, g in enumerate(segs):
        tip = max(np.linalg.norm(g.a), np.linalg.norm(g.b))
        for m in range(min(g.frame, A)):
            R[m, s] = 1.0 if model.joints[m].type == PRISMATIC else tip + hop[m + 1:g.frame].sum()
    return _round_up32(R)


def certificate_guard(model: ChainModel) -> float:
    """The length taken off every certified slack, on the device and in the twin alike: 8 x the project's bound 16 A 2^-24 reach on
    a float32 walk. 4 of them is the widest band in which a float32 clearance is left uncompared with the twin's; the rest covers
    the float32 rounding of a half-step, (A + 2) 2^-24 relative on centimetres. A float32 certificate is then still a statement
    about the exact geometry. A float32 value."""
    return float(np.float32(8 * 16 * model.A * 2.0 ** -24 * model.reach))


def path_half_steps(model: ChainModel, q_start, via, q_goal, S: int, reach=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(beta_1, beta_2, beta_via), each [..., n_seg + P] float64, of the polylines q_start -> via -> q_goal [..., A] at S samples:
    with h = S / 2, leg 1 has n_1 = h intervals and leg 2 n_2 = h - 1, all of a leg with the joint displacement (b - a) / n. Entry
    s < n_seg: beta[s] = 1/2 sum_m |b_m - a_m| / n R[m][s], how far a point of capsule s can travel over half an interval. Entry
    n_seg + p, pair p = (s, t) with frames f_s <= f_t: the same sum over m = f_s .. f_t - 1 with R[m][t] — only the joints between
    the two links move one relative to the other. beta_via is the larger of the two, entry by entry: the via sample ends leg 1's
    last interval and begins leg 2's first. R is reach_table's, as float32 holds it."""
    R = (reach_table(model) if reach is None else np.asarray(reach)).astype(np.float64)
    a, v, b = np.asarray(q_start, float), np.asarray(via, float), np.asarray(q_goal, float)
    h = int(S) // 2
    n_seg = len(model.segments)
    W = np.zeros((model.A, n_seg + len(model.self_pairs)))
    W[:, :n_seg] = R
    for p, (s, t) in enumerate(model.self_pairs):
        f_s, f_t = model.segments[s].frame, model.segments[t].frame
        W[f_s:f_t, n_seg + p] = R[f_s:f_t, t]
    b1 = 0.5 * (np.abs(v - a) / h) @ W
    b2 = 0.5 * (np.abs(b - v) / (h - 1)) @ W
    return b1, b2, np.maximum(b1, b2)


def path_slacks(twin: KinematicEnvironment, q, obstacle, betas, guard: float) -> np.ndarray:
    """[..., S, 3] float64: the three slacks at the poses q[..., S, A] of polylines whose half-steps are betas = (beta_1, beta_2,
    beta_via) [..., n_seg + P], in the scenes obstacle[..., 3]: per sample the minimum over its tests of (clearance - beta - guard),
    beta the tested capsule's or pair's entry of the sample's table — leg 1's for i < h, leg 2's for i > h, the via's for i == h.
    [0] the obstacle's, its radius subtracted | [1] the pairs', +inf without pairs | [2] the workcell's, +inf without one."""
    from .kinematic import segment_point_distance2
    model = twin.model
    q = np.asarray(q, float)
    S, n_seg = q.shape[-2], len(model.segments)
    h = S // 2
    i = np.arange(S)[:, None]
    b1, b2, bv = (np.asarray(x, float)[..., None, :] for x in betas)
    beta = np.where(i < h, b1, np.where(i == h, bv, b2))                      # [..., S, n_seg + P]
    beta = np.broadcast_to(beta, q.shape[:-1] + beta.shape[-1:])
    c = np.asarray(obstacle, float)[..., None, :]
    segs = twin.world_segments(q)
    out = np.full(q.shape[:-1] + (3,), np.inf)
    out[..., 0] = np.min([np.sqrt(segment_point_distance2(a, b, c)) - r - beta[..., s] for s, (a, b, r) in enumerate(segs)],
                         axis=0) - twin.obstacle_radius - guard
    if model.self_pairs:
        out[..., 1] = np.min(twin.pair_clearances(q) - np.moveaxis(beta[..., n_seg:], -1, 0), axis=0) - guard
    if model.cell_pairs:
        of = np.array([s for s, _ in model.cell_pairs])
        out[..., 2] = np.min(twin.cell_clearances(q) - np.moveaxis(beta[..., of], -1, 0), axis=0) - guard
    return out


def certify_joint_path(twin: KinematicEnvironment, q_start, via, q_goal, obstacle, S: int, margin: float = 0.0, poses=None,
                       reach=None, guard: Optional[float] = None) -> np.ndarray:
    """[..., PATH_CERT_FLOATS] float64: [0 .. 7] exactly check_joint_path's record | [8] [9] [10] the minima over the samples of
    path_slacks' three | [11] the index of the first sample one of whose slacks is < margin, -1: none. A candidate is CERTIFIED iff
    [11] == -1: every test at every sample keeps margin + beta + guard, each sample's tests cover the half intervals on both its
    sides (a point of the tested capsule travels at most beta over one), and the h intervals of leg 1 and the h - 1 of leg 2 are
    each covered, half and half, by the samples at their two ends — so no pose of the polyline is closer than margin to anything
    that is tested. It implies [4] == 0. poses[..., S, A]: evaluate the slacks there instead of at path_pose's (the tests' teacher
    forcing); [0 .. 7] are path_pose's in either case."""
    from .kinematic import PATH_CERT_FLOATS, PATH_FLOATS, check_joint_path, path_pose
    out = np.empty(np.broadcast_shapes(np.shape(q_start)[:-1], np.shape(via)[:-1], np.shape(q_goal)[:-1]) + (PATH_CERT_FLOATS,))
    out[..., :PATH_FLOATS] = check_joint_path(twin, q_start, via, q_goal, obstacle, S, margin)
    q_start, via, q_goal = np.broadcast_arrays(np.asarray(q_start, float), np.asarray(via, float), np.asarray(q_goal, float))
    obstacle = np.broadcast_to(np.asarray(obstacle, float), via.shape[:-1] + (3,))
    if poses is None:
        poses = path_pose(q_start[..., None, :], via[..., None, :], q_goal[..., None, :], np.arange(S), S)
    guard = certificate_guard(twin.model) if guard is None else float(guard)
    slack = path_slacks(twin, poses, obstacle, path_half_steps(twin.model, q_start, via, q_goal, S, reach), guard)
    low = np.any(slack < margin, axis=-1)
    out[..., 8:11] = slack.min(axis=-2)
    out[..., 11] = np.where(low.any(axis=-1), np.argmax(low, axis=-1), -1)
    return out


def select_certified_path(records, samples) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(outcome[N] str, candidate[N] int, open[N] bool) from records[N][C][PATH_CERT_FLOATS] taken at samples[N]. A candidate is
    certified iff [11] == -1 and free iff [4] == 0. The certified candidate with the smallest length [5] wins, ties to the lowest c,
    and a certified candidate 0 — the straight line, which no polyline is shorter than — wins outright: 'straight' or 'via'.
    Without a certified candidate the shortest free one, by the same order, is reported as 'sampled'; 'blocked': none is free.
    'start' before 'goal' before the rest, as select_joint_path has them; candidate is -1 wherever no path is returned.
    open: the query is worth another round at twice the samples — samples < PATH_SAMPLES_MAX, and it has no certified candidate,
    or a candidate that is free, uncertified and shorter than its best certified one (candidate 0 counts as the shortest). A
    'start' or 'goal' query is never open: samples 0 and S - 1 are the same two poses at every S, so no round changes its outcome."""
    from .kinematic import PATH_SAMPLES_MAX
    rec = np.asarray(records)
    free = rec[..., 4] == 0
    cert = rec[..., 11] == -1

    def shortest(ok):
        length = np.where(ok, rec[..., 5].astype(np.float64), np.inf)
        length[..., 0] = np.where(ok[..., 0], -np.inf, np.inf)
        best = np.argmin(length, axis=-1)
        return best, np.take_along_axis(length, best[..., None], axis=-1)[..., 0], length

    best_c, len_c, _ = shortest(cert)
    best_f, _, len_f = shortest(free & ~cert)
    found, any_free = cert.any(axis=-1), free.any(axis=-1)
    outcome = np.where(found, np.where(best_c == 0, "straight", "via"), np.where(any_free, "sampled", "blocked")).astype("<U8")
    outcome = np.where(rec[..., 0, 7] == 1, "goal", outcome)
    outcome = np.where(rec[..., 0, 3] == 0, "start", outcome)
    shorter = np.any(len_f < len_c[..., None], axis=-1)                      # (inf < inf is False: no free-uncertified candidate)
    open_ = (np.asarray(samples) < PATH_SAMPLES_MAX) & (~found | shorter) & (outcome != "start") & (outcome != "goal")
    has = (outcome == "straight") | (outcome == "via") | (outcome == "sampled")
    return outcome, np.where(has, np.where(found, best_c, best_f), -1), open_


def gather_certified_paths(records, vias, q_start, q_goal, samples, refinements) -> JointPaths:
    """JointPaths, its last three fields filled, from the last round's records[N][C][PATH_CERT_FLOATS]"""
    from .kinematic import JointPaths, _gather_paths
    rec = np.asarray(records)
    outcome, cand, _ = select_certified_path(rec, samples)
    fields, row = _gather_paths(rec, vias, q_start, q_goal, samples, outcome, cand)
    return JointPaths(*fields, (cand >= 0) & (row[:, 11] == -1), row[:, 8:11].min(axis=1), np.asarray(refinements, np.int64))


def certify_rounds(run, leg_lengths, candidates: int, resolution: float, budget: int, dtype) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(records[N][C][PATH_CERT_FLOATS], samples[N], refinements[N]): the refinement rounds, the same for the device and the twin.
    run(queries, S) -> [len(queries)][C][PATH_CERT_FLOATS] checks the given queries (an index array, within the budget of
    candidate-samples) with all their candidates at S samples. The first round is path_chunks' — consecutive queries, S from their
    legs; every further one takes the open queries (select_certified_path) again with the same vias at min(2 S, PATH_SAMPLES_MAX)
    and replaces their records, until none is open: from 64 samples at most five more rounds."""
    from .kinematic import PATH_CERT_FLOATS, PATH_SAMPLES_MAX, path_chunks
    N, C = len(leg_lengths), int(candidates)
    records = np.empty((N, C, PATH_CERT_FLOATS), dtype)
    samples, refinements = np.empty(N, np.int64), np.zeros(N, np.int64)
    for first, n, S in path_chunks(leg_lengths, C, resolution, budget):
        records[first:first + n] = run(np.arange(first, first + n), S)
        samples[first:first + n] = S
    while True:
        open_ = select_certified_path(records, samples)[2]
        if not open_.any():
            return records, samples, refinements
        # the round's groups are formed before any of them runs: a query doubled in this round is looked at again in the next one
        for S, idx in [(int(S), np.flatnonzero(open_ & (samples == S))) for S in np.unique(samples[open_])]:
            S2 = min(2 * S, PATH_SAMPLES_MAX)
            per = max(1, budget // (C * S2))
            for k in range(0, len(idx), per):
                records[idx[k:k + per]] = run(idx[k:k + per], S2)
            samples[idx] = S2
            refinements[idx] += 1

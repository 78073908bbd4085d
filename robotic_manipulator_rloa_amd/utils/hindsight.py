"""Hindsight goals in the replay gather, stated in float64 numpy (csrc/replay.hip, replay_gather_rows_hindsight_kernel;
include/naf_hip.h, "Hindsight goals"), and the place of the episode tag in a ring row. Importable without a GPU.

A stored transition of the kinematic arm environment is replayed as if its goal had been a point the end effector reached later
in the same episode. The ring row holds all the reward rule needs (the end effector of state and next_state, the target), so the
relabelling is a transformation of the gather: `relabel_rows` is what the kernel computes, with the Philox uniforms as inputs.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

MAX_HORIZON = 1024              # NAF_HINDSIGHT_MAX_HORIZON
REACHED = 0.05                  # the reward rule's threshold (csrc/chain_env.hip)
CONTACT_REWARD = -1000.0


def _round_up(x: int, m: int) -> int:
    return -(-x // m) * m


def row_floats(S: int, A: int) -> int:
    """naf_replay_row_floats: the used row padded to a power of two floats, at least 32"""
    need, rf = _round_up(S + A + 1, 4) + S + 1, 32
    while rf < need:
        rf *= 2
    return rf


def batch_row_floats(S: int, A: int) -> int:
    """naf_replay_batch_row_floats: the leading floats of a row the learner reads"""
    off_s2 = _round_up(S + A + 1, 4)
    k4 = (S + 3) // 4
    k4d = 6 if k4 <= 6 else (8 if k4 <= 8 else k4)
    return min(_round_up(max(off_s2 + S + 1, off_s2 + 4 * k4d), 4), row_floats(S, A))


def tag_column(S: int, A: int) -> Optional[int]:
    """The float of a ring row that carries the episode tag — the row's last one — or None for an arm whose minibatch row reaches
    it (A = 1, 2, 8, 21 and 47 among the chain environment's S = 2 A + 9 up to 64 joints: the used row fills the power of two)."""
    col = row_floats(S, A) - 1
    return col if col >= batch_row_floats(S, A) else None


def check_arguments(ratio: float, horizon: int) -> None:
    if not (0.0 <= float(ratio) <= 1.0):
        raise ValueError(f"hindsight: ratio {ratio!r} is outside [0, 1]")
    if isinstance(horizon, bool) or int(horizon) != horizon or not (1 <= int(horizon) <= MAX_HORIZON):
        raise ValueError(f"hindsight: horizon {horizon!r} is outside [1, {MAX_HORIZON}]")


def require_tag_column(S: int, A: int) -> int:
    col = tag_column(S, A)
    if col is None:
        raise ValueError(f"hindsight: an arm of {A} joints (state size {S}) has no spare row float for the episode tag — its "
                         f"minibatch row takes all {batch_row_floats(S, A)} of the ring row's {row_floats(S, A)} floats")
    return col


def candidates(k0, horizon: int) -> np.ndarray:
    """[.., J] the halving candidates k0 >> j, j = 0 .. ceil(log2 horizon); the last one is 0 (k0 < horizon)"""
    J = max(0, int(horizon) - 1).bit_length() + 1
    return np.asarray(k0, np.int64)[..., None] >> np.arange(J)


def relabel_rows(rows_in_deque_order, idx, relabel_u, k0, stride: int, horizon: int, ratio: float, S: int, A: int
                 ) -> Tuple[np.ndarray, np.ndarray]:
    """rows_in_deque_order: [size, row_floats] float32 ring rows, oldest first. idx [n]: deque positions. relabel_u [n]: the
    uniforms naf_u01(word 0) of the rows' draws; k0 [n]: (uint64(word 1) * horizon) >> 32.
    Returns (rows [n, row_floats] float32: rows[idx] with goal, reward and done rewritten where a candidate was taken; k [n] int:
    -1 not drawn, -2 drawn and no candidate valid, else the k taken). The distance is float64, the goal is copied exactly."""
    check_arguments(ratio, horizon)
    rows = np.asarray(rows_in_deque_order, np.float32)
    idx = np.asarray(idx, np.int64)
    size, rf = rows.shape
    if S != 2 * A + 9:
        raise ValueError("hindsight: the row is not the kinematic arm environment's (S = 2 A + 9)")
    if rf != row_floats(S, A):
        raise ValueError(f"hindsight: rows of {rf} floats, an arm of S = {S}, A = {A} has rows of {row_floats(S, A)}")
    if int(stride) < 1 or np.asarray(relabel_u).shape != idx.shape or np.asarray(k0).shape != idx.shape:
        raise ValueError("hindsight: stride is positive, relabel_u and k0 hold one value per index")
    if idx.size and (idx.min() < 0 or idx.max() >= size):
        raise ValueError("hindsight: an index outside the ring")
    col = rf - 1             # the kernel's rule at the kernel's column; whether an arm may USE it is tag_column's verdict
    off_r, off_s2 = S + A, _round_up(S + A + 1, 4)
    off_d, ee2 = off_s2 + S, off_s2 + 2 * A
    out = rows[idx].copy()
    n = idx.size
    k = np.full(n, -1, np.int64)
    drawn = np.asarray(relabel_u, np.float32) < np.float32(ratio)
    cand = candidates(np.asarray(k0, np.int64), horizon)                       # [n, J]
    pos = idx[:, None] + cand * int(stride)
    inside = pos < size
    safe = np.where(inside, pos, idx[:, None])
    tag_i = rows[idx, col]
    valid = inside & (tag_i[:, None] >= 1.0) & (rows[safe, col] == tag_i[:, None]) & (rows[safe, off_r] != np.float32(CONTACT_REWARD))
    first = np.argmax(valid, axis=1)
    any_valid = np.any(valid, axis=1)
    k[drawn] = np.where(any_valid, cand[np.arange(n), first], -2)[drawn]
    take = np.nonzero(k >= 0)[0]
    src = idx[take] + k[take] * int(stride)
    g = rows[src, ee2:ee2 + 3]
    out[take, 2 * A + 3:2 * A + 6] = g
    out[take, off_s2 + 2 * A + 3:off_s2 + 2 * A + 6] = g
    d = np.linalg.norm(rows[idx[take], ee2:ee2 + 3].astype(np.float64) - g.astype(np.float64), axis=1)
    reached = d < REACHED
    out[take, off_r] = np.where(reached, 250.0, -(d - REACHED)).astype(np.float32)
    out[take, off_d] = reached.astype(np.float32)
    return out, k


def shares(k, k0, done) -> dict:
    """What a sample of gathered rows says about the relabelling: k = k_out, k0 = the drawn k0 where known (None: the shortened
    share is left out), done = the rows' done column."""
    k = np.asarray(k).reshape(-1)
    done = np.asarray(done).reshape(-1)
    taken = k >= 0
    n_taken = max(1, int(taken.sum()))
    out = {"hindsight_relabelled_share": float(taken.mean()) if k.size else 0.0,
           "hindsight_reached_share": float(np.sum(done[taken] != 0)) / n_taken}
    if k0 is not None:
        out["hindsight_shortened_share"] = float(np.sum(k[taken] < np.asarray(k0).reshape(-1)[taken])) / n_taken
    return out

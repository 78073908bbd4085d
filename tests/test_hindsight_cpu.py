"""No GPU: hindsight goals in the replay gather — the float64 statement (utils/hindsight.relabel_rows) held to its properties on
synthetic rings, a rehearsal that the GPU cases are not vacuous, the tag column, and every argument check and refusal that needs
no device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
from hindsight_common import (BAND, ENVS, HORIZONS, RATIOS, SHAPES, UNTAGGED, case_indices, cases, distance, hindsight_draw, in_band,
                              synthetic_ring, twin_case)
from oracle import naf_oracle as O

from robotic_manipulator_rloa_amd.utils import hindsight as H


def _cols(S, A):
    _, off_r, off_s2, off_d = O.row_offsets(S, A)
    return off_r, off_s2, off_d, np.r_[2 * A + 3:2 * A + 6, off_s2 + 2 * A + 3:off_s2 + 2 * A + 6]


@pytest.mark.parametrize("E", ENVS)
@pytest.mark.parametrize("S,A", SHAPES)
def test_the_builder_builds_what_it_says(S, A, E):
    ring = synthetic_ring(S, A, E)
    off_r, off_s2, off_d, _ = _cols(S, A)
    assert ring.head != 0 and ring.size == ring.capacity and ring.phys.shape == (ring.capacity, H.row_floats(S, A))
    assert np.array_equal(ring.phys[(ring.head + np.arange(ring.size)) % ring.capacity], ring.deque)
    tag = ring.deque[:, -1]
    assert np.all(tag[:UNTAGGED] == 0) and np.all(tag[UNTAGGED:] >= 1)
    # rows i and i + E are the same env one tick apart; tags equal exactly inside an episode
    i = np.arange(UNTAGGED, ring.size - E)
    assert np.all(ring.env[i] == ring.env[i + E]) and np.all(ring.tick[i] + 1 == ring.tick[i + E])
    assert np.array_equal(tag[i] == tag[i + E], ring.episode[i] == ring.episode[i + E])
    r, d = ring.deque[:, off_r], ring.deque[:, off_d]
    assert np.sum(r == 250) >= 5 and np.sum(r == -1000) >= 5 and np.all((d == 1) == ((r == 250) | (r == -1000)))
    # the frame limit ends episodes too: a tag changes behind a row that is not done
    assert np.sum((tag[i] != tag[i + E]) & (d[i] == 0)) >= 5
    # k = 1 .. 12 ticks straddle the threshold
    ee2 = ring.deque[:, off_s2 + 2 * A:off_s2 + 2 * A + 3].astype(np.float64)
    for k, side in ((1, "below"), (12, "above")):
        j = np.arange(UNTAGGED, ring.size - k * E)
        dist = np.linalg.norm(ee2[j] - ee2[j + k * E], axis=1)[ring.episode[j] == ring.episode[j + k * E]]
        assert dist.size == 0 or (np.mean(dist < 0.05) > 0.5 if side == "below" else np.mean(dist > 0.05) > 0.5), (k, dist.mean())


@pytest.mark.parametrize("S,A,E,horizon,ratio", cases())
def test_relabel_rows_properties_and_rehearsal(S, A, E, horizon, ratio):
    ring, idx, u, k0, rows, k = twin_case(S, A, E, horizon, ratio)
    off_r, off_s2, off_d, goal = _cols(S, A)
    src = ring.deque[idx]
    if ratio == 0.0:
        assert rows.tobytes() == src.tobytes() and np.all(k == -1)
        return
    assert np.all(k >= -2) and np.array_equal(k == -1, ~(u < np.float32(ratio)))
    untagged, contact = src[:, -1] == 0, src[:, off_r] == -1000
    assert untagged.sum() >= 40 and np.all(k[untagged] < 0) and np.all(k[contact] < 0)
    same = k < 0
    assert rows[same].tobytes() == src[same].tobytes()
    t = np.nonzero(k >= 0)[0]
    far = idx[t].astype(np.int64) + k[t] * E
    assert np.all(far < ring.size)
    assert np.array_equal(ring.episode[far], ring.episode[idx[t]]) and np.array_equal(ring.env[far], ring.env[idx[t]])
    assert np.all(ring.tick[far] == ring.tick[idx[t]] + k[t])
    assert np.all(ring.deque[far, off_r] != -1000)
    zero = t[k[t] == 0]
    assert np.all(rows[zero, off_r] == 250) and np.all(rows[zero, off_d] == 1)
    touched = np.zeros(ring.rf, bool)
    touched[np.r_[goal, off_r, off_d]] = True
    assert rows[:, ~touched].tobytes() == src[:, ~touched].tobytes()
    g = ring.deque[far, off_s2 + 2 * A:off_s2 + 2 * A + 3]
    assert rows[t][:, goal].tobytes() == np.concatenate([g, g], axis=1).tobytes()
    d = distance(ring, idx, k)[t]
    assert np.array_equal(rows[t, off_d] == 1, d < 0.05)
    assert np.all(rows[t, off_r] == np.where(d < 0.05, 250.0, -(d - 0.05)).astype(np.float32))
    # a reached row stays reached; a non-terminal row whose new goal is far stays non-terminal
    reached = src[:, off_r] == 250
    assert np.all((k[reached] <= 0)) and np.all(rows[reached & (k == 0), off_d] == 1)
    # brute force over the halving candidates: the taken k is the first valid one, -2 means none is
    J = max(0, horizon - 1).bit_length() + 1
    for r in np.nonzero(k != -1)[0]:
        i, first = int(idx[r]), -2
        for j in range(J):
            c = int(k0[r]) >> j
            p = i + c * E
            if ring.deque[i, -1] >= 1 and p < ring.size and ring.deque[p, -1] == ring.deque[i, -1] and ring.deque[p, off_r] != -1000:
                first = c
                break
        assert k[r] == first, (r, k[r], first)
    assert (int(k0.max()) >> (J - 1)) == 0
    # rehearsal of the GPU case: not vacuous, and the band the GPU comparison leaves out is thin — by the twin alone
    n_rel = int(np.sum(k >= 0))
    assert n_rel >= 30, n_rel
    if horizon > 1:
        assert np.sum(k[t] < k0[t]) >= 5 and np.sum(k == -2) >= 5, (int(np.sum(k[t] < k0[t])), int(np.sum(k == -2)))
    assert in_band(ring, idx, k).sum() <= 0.01 * n_rel and BAND == 1e-6


def test_the_draw_is_keyed_as_the_header_says():
    u, k0 = hindsight_draw(7, (1 << 64) - 2, 6, 2, 1024)       # minibatches at 2^64 - 2, 2^64 - 1 and 0: the counter wraps
    v = O.philox4x32_10(np.uint32(0), np.uint32(0), np.uint32(1), np.uint32(0x48494E44), 7, 0)
    assert k0[5] == (int(v[1]) * 1024) >> 32 and 0 <= k0.min() and k0.max() < 1024
    v = O.philox4x32_10(np.uint32(0xFFFFFFFE), np.uint32(0xFFFFFFFF), np.uint32(0), np.uint32(0x48494E44), 7, 0)
    assert u[0] == np.float32((float(int(v[0]) >> 8) + 0.5) * 2.0 ** -24)
    assert hindsight_draw(7, 0, 4, 2, 1)[1].tolist() == [0, 0, 0, 0]
    assert H.candidates([5, 1023], 1024).tolist() == [[5, 2, 1, 0, 0, 0, 0, 0, 0, 0, 0], [1023, 511, 255, 127, 63, 31, 15, 7, 3, 1, 0]]
    assert H.candidates([0], 1).tolist() == [[0]] and H.candidates([7], 8).tolist() == [[7, 3, 1, 0]]


def test_tag_column():
    lib_formula = {}
    for name, A in (("planar3", 3), ("iiwa_like7", 7), ("long12", 12)):
        S = 2 * A + 9
        col = H.tag_column(S, A)
        assert col == H.row_floats(S, A) - 1 and col >= H.batch_row_floats(S, A), name
        lib_formula[A] = col
    assert lib_formula == {3: 63, 7: 63, 12: 127}
    for A in (21, 47):
        assert H.tag_column(2 * A + 9, A) is None
        with pytest.raises(ValueError, match=rf"{A} joints.*{H.row_floats(2 * A + 9, A)} floats"):
            H.require_tag_column(2 * A + 9, A)
    # the rule, not a list: wherever the minibatch row reaches the ring row's last float there is no column
    for A in range(1, 65):
        S = 2 * A + 9
        assert (H.tag_column(S, A) is None) == (H.row_floats(S, A) - 1 < H.batch_row_floats(S, A))
    assert (H.row_floats(21, 6), H.batch_row_floats(21, 6)) == (64, 52) and (H.row_floats(23, 7), H.batch_row_floats(23, 7)) == (64, 56)


def test_the_library_formulas_agree_with_the_host_ones():
    from robotic_manipulator_rloa_amd import _lib
    lib = _lib.load()
    for A in range(1, 65):
        S = 2 * A + 9
        assert lib.naf_replay_row_floats(S, A) == H.row_floats(S, A) and lib.naf_replay_batch_row_floats(S, A) == H.batch_row_floats(S, A)
    assert lib.naf_hip_abi_version() == 40
    assert {"naf_replay_gather_rows_hindsight", "naf_chain_env_step_tagged"} <= set(_lib.EXPORTED_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    for name in ("naf_replay_gather_rows_hindsight", "naf_chain_env_step_tagged"):
        assert re.search(rf"^int {name}\(", hdr, re.M) and len(_lib._PROTOS[name]) == hdr.split(f"int {name}(")[1].split(")")[0].count(",") + 1
    assert ctypes.sizeof(_lib.Hindsight) == 64 and _lib.Hindsight.k_out.offset == 48 and _lib.Hindsight.counter_off.offset == 32
    # no device is touched by an argument error: NULL handles and descriptors are refused before any launch
    assert lib.naf_replay_gather_rows_hindsight(None, None, None, 0, 0, 0, None, None) == -2
    assert lib.naf_chain_env_step_tagged(None, None, None, None, None, 1, 0, None, 0, None, 0, None) == -1


def test_argument_checks():
    ring = synthetic_ring(23, 7, 3)
    idx = case_indices(ring.size)
    u, k0 = hindsight_draw(1, 0, idx.size, 100, 8)
    ok = dict(stride=3, horizon=8, ratio=0.5, S=23, A=7)
    H.relabel_rows(ring.deque, idx, u, k0, **ok)
    for bad, what in ((dict(ratio=-0.1), "ratio"), (dict(ratio=1.5), "ratio"), (dict(ratio=float("nan")), "ratio"),
                      (dict(horizon=0), "horizon"), (dict(horizon=1025), "horizon"), (dict(horizon=2.5), "horizon"),
                      (dict(stride=0), "stride"), (dict(S=22, A=7), "S = 2 A"), (dict(S=33, A=12), "rows of 64 floats")):
        with pytest.raises(ValueError, match=what):
            H.relabel_rows(ring.deque, idx, u, k0, **dict(ok, **bad))
    with pytest.raises(ValueError, match="one value per index"):
        H.relabel_rows(ring.deque, idx, u[:-1], k0, **ok)
    with pytest.raises(ValueError, match="outside the ring"):
        H.relabel_rows(ring.deque, np.array([ring.size]), u[:1], k0[:1], **ok)
    H.check_arguments(0.0, 1)
    H.check_arguments(1.0, 1024)
    s = H.shares([-1, -2, 0, 3, 5], [-1, 9, 4, 3, 9], [0, 1, 1, 0, 0])
    assert s == {"hindsight_relabelled_share": 0.6, "hindsight_reached_share": 1 / 3, "hindsight_shortened_share": 2 / 3}


def test_refusals_that_need_no_gpu():
    from robotic_manipulator_rloa_amd import ManipulatorFramework
    from robotic_manipulator_rloa_amd.naf_components.naf_algorithm import NAFAgent
    me = types.SimpleNamespace(world_size=1, state_size=23, action_size=7, memory=[])
    args = NAFAgent._hindsight_arguments
    chain = object()
    assert args(me, 0.0, None, 400, chain, False) is None and args(me, 0.0, 8, 400, None, False) is None
    assert args(me, 0.8, None, 400, chain, False) == (0.8, 400) and args(me, 0.8, None, 5000, chain, False) == (0.8, 1024)
    assert args(me, 0.8, 16, 400, chain, False) == (0.8, 16)
    for ratio, horizon, what in ((1.2, None, "ratio"), (-0.5, None, "ratio"), (0.5, 0, "horizon"), (0.5, 1025, "horizon"),
                                 (0.0, 2000, "horizon")):
        with pytest.raises(ValueError, match=what):
            args(me, ratio, horizon, 400, chain, False)
    with pytest.raises(ValueError, match="chain model"):
        args(me, 0.5, None, 400, None, False)
    with pytest.raises(ValueError, match="data-parallel"):
        args(types.SimpleNamespace(**dict(vars(me), world_size=2)), 0.5, None, 400, chain, False)
    with pytest.raises(ValueError, match="21 joints"):
        args(types.SimpleNamespace(**dict(vars(me), state_size=51, action_size=21)), 0.5, None, 400, chain, False)
    full = types.SimpleNamespace(**dict(vars(me), memory=[0] * 7))
    with pytest.raises(ValueError, match="already holds 7 rows"):
        args(full, 0.5, None, 400, chain, False)
    assert args(full, 0.5, None, 400, chain, True) == (0.5, 400)          # a resume continues its own ring
    # the framework: the one-env loop, the stand-in and (any env that is not the kinematic one) refuse by name
    f = ManipulatorFramework()
    f.initialize_synthetic_environment(6, [0.3, 0.47, 0.61], [0.25, 0.27, 0.5], [0., 1., 0., -2.3, 0., 0.], [0, 0, 0, 0.3, 1, 1])
    assert f._hindsight_arguments(0.0, None, 64) == {}
    for E in (64, None, 1):
        with pytest.raises(ValueError, match="kinematic arm environment"):
            f._hindsight_arguments(0.5, None, E)
    with pytest.raises(ValueError, match="ratio"):
        f._hindsight_arguments(2.0, None, 64)
    with pytest.raises(ValueError, match="horizon"):
        f._hindsight_arguments(0.5, 4096, 64)

"""The case table of the float64 learn() checks (tests/test_learn_f64_gpu.py on the HIP learner, test_host_cpu.py's checker
calibration on the float32 oracle in test_oracle_golden.py): the shapes where the three chains of learn() keep their edge handling, and data that
drives the clip into both regimes and layer 1's statistics into cancellation. Inputs come from synth_data.make_transitions and
torch's nn.Linear init only."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import naf_oracle as O


@dataclass(frozen=True)
class Case:
    name: str
    S: int
    A: int
    H: int
    B: int
    p_mode: int
    chain: str                   # the chain the learner must pick: rows | columns | unfused
    fuse: str | None = None      # Learner(fuse=...): None = the per-shape default
    pad: bool = True             # Learner(pad_layer=...)
    data: str = "plain"          # plain | rare (+-250 / -1000 rewards) | small (gradient norm < 1) | cancel (layer-1 inputs 3 +- 0.1)
    n_upd: int = 4
    drop: frozenset = field(default_factory=frozenset)   # launches the chain's fuse set must lack ("l1", "gb", ...)
    why: str = ""


CASES = [
    # ---- row-split chain (csrc/big_batch.hip, fused_layers.hip, gemm_bundle.hip) ---------------------------------------
    Case("rows_b16_m1", 21, 6, 256, 16, 1, "rows", why="one 16-row group, L L^T head"),
    Case("rows_b17", 21, 6, 256, 17, 0, "rows", data="rare", why="a one-row partial group"),
    Case("rows_b65", 21, 6, 256, 65, 0, "rows", data="small", why="a one-row partial 64-row block, clip inactive"),
    Case("rows_b100_m1", 25, 8, 256, 100, 1, "rows", why="partial block and group at 8 joints"),
    Case("rows_b320", 21, 6, 256, 320, 0, "rows", data="cancel", why="K ranges with a tail chunk; moments under cancellation"),
    Case("rows_b1040", 21, 6, 256, 1040, 0, "rows", data="rare", why="a 16-row K tail"),
    Case("rows_b2047", 23, 7, 256, 2047, 0, "rows", why="partial block at the last 16-row-per-workgroup size"),
    Case("rows_b2048_m1", 27, 9, 256, 2048, 1, "rows", why="9 joints, L L^T: ReLU inputs within rounding of 0"),
    Case("rows_b2100", 21, 6, 256, 2100, 0, "rows", data="rare", why="32 rows per workgroup, partial"),
    Case("rows_b4096", 21, 6, 256, 4096, 0, "rows", why="the largest row-split batch"),
    Case("rows_s32_b512", 32, 8, 256, 512, 0, "rows", data="rare", why="state size 32: layer 1's whole K"),
    Case("rows_j9_b256_m1", 27, 9, 256, 256, 1, "rows", why="one sample per 16-lane group"),
    Case("rows_j10_b1000_m1", 29, 10, 256, 1000, 1, "rows", data="rare", why="10 joints, partial block"),
    Case("rows_j11_b2048", 31, 11, 256, 2048, 0, "rows", why="11 joints at 16 rows per workgroup"),
    Case("rows_j11_b3000", 31, 11, 256, 3000, 0, "rows", why="11 joints beyond 2048 (Hadamard only)"),
    Case("rows_h128_b256", 21, 6, 128, 256, 0, "rows", data="rare", why="128 stored zero-padded to 256"),
    Case("rows_h320_b48", 21, 6, 320, 48, 0, "rows", why="320 stored zero-padded to 512"),
    Case("rows_h384_b2048", 21, 6, 384, 2048, 0, "rows", data="rare", why="384 padded to 512 at 16 rows per workgroup"),
    Case("rows_h512_b1024_m1", 23, 7, 512, 1024, 1, "rows", why="two 256-column halves, L L^T head"),
    Case("rows_h512_j9_b256", 27, 9, 512, 256, 0, "rows", why="two halves at 9 joints"),
    # ---- column-tile chain (csrc/fused_layers.hip) ------------------------------------------------------------------------
    Case("cols_b9", 21, 6, 256, 9, 0, "columns", data="small", drop=frozenset({"gb"}), why="below 16 rows, clip inactive"),
    Case("cols_b33_m1", 21, 6, 256, 33, 1, "columns", fuse="columns", data="cancel", drop=frozenset({"gb"}),
         why="forced; moments-free layer 1 under cancellation"),
    Case("cols_s40_b32", 40, 4, 256, 32, 0, "columns", data="rare", drop=frozenset({"l1"}), why="state size 40: no l1"),
    Case("cols_s26_b300_m1", 26, 8, 256, 300, 1, "columns", fuse="columns", drop=frozenset({"l1", "gb"}),
         why="state 26 beyond 256 rows: no l1"),
    Case("cols_h200_b100", 21, 6, 200, 100, 0, "columns", pad=False, drop=frozenset({"gb", "s3"}), why="unpadded 200: no gb"),
    # ---- unfused chain (torch GEMMs + csrc/bn_relu.hip, naf_head*.hip) -------------------------------------------------
    Case("unf_b1024_m1", 21, 6, 256, 1024, 1, "unfused", fuse="unfused", why="forced"),
    Case("unf_b5000", 21, 6, 256, 5000, 0, "unfused", data="rare", why="beyond the row-split chain: streamed BatchNorm"),
    Case("unf_a12_b64_m1", 30, 12, 256, 64, 1, "unfused", why="12 joints"),
    Case("unf_a17_b64", 43, 17, 256, 64, 0, "unfused", data="rare", why="17 joints"),
    Case("unf_a32_b100_m1", 73, 32, 256, 100, 1, "unfused", why="32 joints, L L^T"),
    Case("unf_a64_b32", 137, 64, 256, 32, 0, "unfused", why="the wide head beyond 32 joints"),
    Case("unf_b20000", 21, 6, 256, 20000, 0, "unfused", n_upd=2, why="a batch beyond the sampler's 4096"),
]


def init_state(case: Case, seed=3):
    """The reference's state_dict at torch's nn.Linear init (tests/test_learner_gpu.py _random_init_sd); "small" scales the
    three heads' weights and biases by 1e-2."""
    import torch
    import torch.nn as nn
    S, A, H = case.S, case.A, case.H
    torch.manual_seed(seed)
    T = A * (A + 1) // 2
    lin = {"input_layer": nn.Linear(S, H), "hidden_layer": nn.Linear(H, H), "action_values": nn.Linear(H, A),
           "value": nn.Linear(H, 1), "matrix_entries": nn.Linear(H, T)}
    sd = {}
    for k, l in lin.items():
        sd[f"{k}.weight"], sd[f"{k}.bias"] = l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()
    for b in ("bn1", "bn2"):
        sd[f"{b}.weight"], sd[f"{b}.bias"] = np.ones(H, np.float32), np.zeros(H, np.float32)
        sd[f"{b}.running_mean"], sd[f"{b}.running_var"] = np.zeros(H, np.float32), np.ones(H, np.float32)
        sd[f"{b}.num_batches_tracked"] = np.array(0)
    if case.data == "small":
        for k in ("action_values", "value", "matrix_entries"):
            sd[f"{k}.weight"] *= np.float32(1e-2)
            sd[f"{k}.bias"] *= np.float32(1e-2)
    return sd


# (mean 3, spread 0.1: layer 1's z - mean loses 30x the rounding of plain inputs. At spread 0.01 the float32 oracle's own
#  layer 1 — z = W x in float32, then z - mean — misses the 1e-4 gradient bound by up to 24x: the test would then reject honest
#  float32 arithmetic rather than a defect)
CANCEL_SPREAD = 0.1


def transitions(case: Case, seed=21):
    """(states, actions (truncated toward zero, as the gather leaves them), rewards, next_states, dones) for n_upd minibatches.
    small: rewards x 1e-3 and every action inside (-1, 1) (truncated to 0), so the TD errors and the gradient are small.
    cancel: state and next-state columns 3 + CANCEL_SPREAD x N(0, 1), column 0 the constant 3 across the minibatch (the
    moments-based statistics of layer 1, csrc/moments_body.h, and the two-pass variances under cancellation)."""
    from synth_data import make_transitions
    n = case.n_upd * case.B
    st, ac, rw, ns, dn = make_transitions(n, case.S, case.A, seed=seed, rare_events=case.data == "rare",
                                          structured_reward=case.data != "rare")
    if case.data == "small":
        rw = (rw * 1e-3).astype(np.float32)
        ac = (ac * 0.5).astype(np.float32)
    if case.data == "cancel":
        st = (3.0 + CANCEL_SPREAD * st).astype(np.float32)
        ns = (3.0 + CANCEL_SPREAD * ns).astype(np.float32)
        st[:, 0] = ns[:, 0] = np.float32(3.0)
    return st, np.trunc(ac).astype(np.float32), rw, ns, dn


def state_of_oracle(o: O.LearnerOracle) -> dict:
    """check_update's state dict of a LearnerOracle (copies)."""
    return {"main": {k: v.copy() for k, v in o.main.items()}, "target": {k: v.copy() for k, v in o.target.items()},
            "m": {k: v.copy() for k, v in o.m.items()}, "v": {k: v.copy() for k, v in o.v.items()}, "t": o.t}

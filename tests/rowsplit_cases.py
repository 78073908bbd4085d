"""The case table and the starting state of the per-launch checks of the row-split learn() chain
(tests/test_rowsplit_launches_gpu.py on the HIP learner, tests/test_rowsplit_launches_cpu.py on the float32 stand-in of
oracle/launch_check.py): the smallest batch at which each branch of the chain's five launches is taken, and a state in which
main and target network differ in every weight and no BatchNorm parameter or running statistic sits at its default.
CPU only: numpy, torch's nn.Linear init and learn_cases.transitions."""
from __future__ import annotations

import numpy as np

from learn_cases import Case, transitions
from oracle import naf_oracle as O


def _c(S, A, H, B, p_mode=0, data="plain", n_upd=1, why=""):
    name = f"s{S}_a{A}_h{H}_b{B}" + ("_m1" if p_mode else "") + ("_rare" if data == "rare" else "")
    return Case(name, S, A, H, B, p_mode, "rows", data=data, n_upd=n_upd, why=why)


# `why` names the line of the branch the size is there for. The counts were confirmed with chain_plan.plan_chain
# (test_rowsplit_launches_cpu.py::test_the_table_reaches_the_branches_it_names holds them).
CASES = [
    _c(21, 6, 256, 16, 1, why="one 16-row group, one workgroup of launch 3 (big_batch.hip naf_bb_layer2_head: rows == 16, "
                              "FULL = false), L L^T head"),
    _c(21, 6, 256, 17, 0, "rare", why="a one-row partial group: ns_ = 1 in bb_layer2_head_kernel, Bp = 32, TAIL form of the bundle "
                                      "(gemm_bundle.hip: rows past the batch in the last 32-row block)"),
    _c(21, 6, 256, 65, 0, why="one whole statistics block and a one-row block: bb_fold_stats<false>'s n_last = 1, Chan's fold of "
                              "unequal blocks; valid = 1 in bb_linear_stats16_kernel"),
    _c(25, 8, 256, 100, 1, why="partial block (36 rows) and partial group (4 rows) at 8 joints: NHP = 48, KP = 32"),
    _c(21, 6, 256, 256, 0, "rare", n_upd=2, why="the benchmark's shape: four whole blocks (FULL forms), one K range; the second "
                                                "update starts from running statistics the first one moved"),
    _c(21, 6, 256, 576, 0, why="nine statistics blocks: launch 3 folds them once into records (naf_bb_layer2_head: bb_blocks(B) > 8); "
                               "GEMM 2 on 64 x 32 tiles (bb_linear_stats_kernel beyond B = 512); XH1 not kept (chain_plan keep_xhat1)"),
    _c(21, 6, 256, 1040, 0, "rare", why="a 16-row tail of the last statistics block; Bp = 1088 in four split-K ranges of 272 rows"),
    _c(21, 6, 256, 2100, 0, "rare", why="32 rows per workgroup of launch 3 (naf_bb_layer2_head_rows: B > 2048), partial; "
                                        "66 dA1 blocks: the BIG form of the finish launch; six K ranges"),
    _c(27, 9, 256, 64, 1, why="9 joints: one sample per 16-lane group, NHP = 64 (BB_FK_WIDE), kp = 32, L L^T"),
    _c(31, 11, 256, 48, 0, why="11 joints: NHP = 80, kp = 32, a 48-row block"),
    _c(32, 8, 256, 128, 0, "rare", why="K = 32 fills the whole kp: no zero column in the moments record or the P slabs"),
    _c(21, 6, 320, 48, 0, why="320 stored zero-padded to 512: two 256-column halves of launch 3 meeting in `exchange` (HALVES = 2), "
                              "192 pad columns"),
    _c(21, 6, 512, 64, 1, why="512 unpadded: two halves, L L^T head, one whole block"),
    _c(21, 6, 128, 32, 0, "rare", why="128 stored zero-padded to 256 (layout.NetLayout): 128 pad columns that stay exactly 0"),
]
BY_NAME = {c.name: c for c in CASES}

# ---- the vacuity guard -------------------------------------------------------------------------------------------------
# A check of a ReLU mask, of a target network's head or of a BatchNorm affine step says nothing where the mask is all one way, the
# head's output is negligible beside Q, or a column is dead. For every case, in float64 at launch_state / transitions:
MIN_ACTIVE, MAX_ACTIVE = 0.10, 0.90      # share of positive layer-1 and layer-2 activations of each network
MAX_DEAD_COLUMNS = 0.05                  # share of a layer's columns with no positive activation in the batch
MIN_VNEXT_REL = 0.1                      # max |V'(s')| of the target network / max |Q| of the main network

# the seed for which the float64 oracle alone meets the guard in every case (the first tried; no device involved):
# test_rowsplit_launches_cpu.py::test_the_state_is_not_vacuous holds it. A case that needs another gets an entry in SEEDS.
SEEDS = {}
DEFAULT_SEED = 1


def _linears(S, A, H, seed):
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    T = A * (A + 1) // 2
    lin = {"input_layer": nn.Linear(S, H), "hidden_layer": nn.Linear(H, H), "action_values": nn.Linear(H, A),
           "value": nn.Linear(H, 1), "matrix_entries": nn.Linear(H, T)}
    sd = {}
    for k, l in lin.items():
        sd[f"{k}.weight"], sd[f"{k}.bias"] = l.weight.detach().numpy().copy(), l.bias.detach().numpy().copy()
    return sd


def launch_state(case: Case, seed: int | None = None, value_scale: float = 1.0):
    """(main, target): two state dicts in the reference's layout (width case.H, as learn_cases.init_state) from DIFFERENT seeds —
    every weight differs — whose four BatchNorm layers each have their own draws of weight ~ U(0.5, 1.5), bias ~ N(0, 0.3),
    running_mean ~ N(0, 0.3), running_var ~ U(0.5, 2) (as test_policy_act_one_launch_matches_seven_launch_path draws them).
    value_scale: both networks' value.weight and value.bias times this power of two (tests/tilechain_cases.py: with many joints
    the quadratic term of Q dwarfs V at torch's init, and a check of the target's V' would pass because V' is negligible)."""
    seed = SEEDS.get(case.name, DEFAULT_SEED) if seed is None else seed
    out = []
    for net in (0, 1):
        sd = _linears(case.S, case.A, case.H, 1000 * seed + 17 * net + 3)
        rng = np.random.default_rng(1000 * seed + net)
        for b in ("bn1", "bn2"):
            sd[f"{b}.weight"] = rng.uniform(0.5, 1.5, case.H).astype(np.float32)
            sd[f"{b}.bias"] = rng.normal(0, 0.3, case.H).astype(np.float32)
            sd[f"{b}.running_mean"] = rng.normal(0, 0.3, case.H).astype(np.float32)
            sd[f"{b}.running_var"] = rng.uniform(0.5, 2.0, case.H).astype(np.float32)
            sd[f"{b}.num_batches_tracked"] = np.array(0)
        if value_scale != 1.0:
            sd["value.weight"] = (sd["value.weight"] * np.float32(value_scale)).astype(np.float32)
            sd["value.bias"] = (sd["value.bias"] * np.float32(value_scale)).astype(np.float32)
        out.append(sd)
    return out[0], out[1]


def vacuity(case: Case, main: dict, target: dict, batch) -> dict:
    """The guard's figures for one minibatch (states, actions, rewards, next_states), in float64."""
    st, ac, rw, ns = batch
    fm, _ = O.net_forward_train(O.cast_params(main, np.float64), st, ac, case.p_mode)
    ft, _ = O.net_forward_train(O.cast_params(target, np.float64), ns, None, case.p_mode)
    acts = [f[a] > 0 for f in (fm, ft) for a in ("a1", "a2")]
    return {"active_min": min(float(m.mean()) for m in acts), "active_max": max(float(m.mean()) for m in acts),
            "dead_columns": max(float((~m.any(axis=0)).mean()) for m in acts),
            "vnext_rel": float(np.abs(ft["V"]).max() / np.abs(fm["Q"]).max())}


def vacuity_ok(v: dict) -> bool:
    return (MIN_ACTIVE <= v["active_min"] and v["active_max"] <= MAX_ACTIVE and v["dead_columns"] <= MAX_DEAD_COLUMNS and
            v["vnext_rel"] >= MIN_VNEXT_REL)


def minibatches(case: Case):
    """[(states, actions, rewards, next_states)] per update, from learn_cases.transitions."""
    st, ac, rw, ns, _ = transitions(case)
    B = case.B
    return [(st[k * B:(k + 1) * B], ac[k * B:(k + 1) * B], rw[k * B:(k + 1) * B], ns[k * B:(k + 1) * B]) for k in range(case.n_upd)]


def dims(case: Case):
    """oracle.launch_check.Dims of a case, from chain_plan.plan_chain (host arithmetic: no GPU)."""
    from oracle.launch_check import Dims
    from robotic_manipulator_rloa_amd.chain_plan import plan_chain
    from robotic_manipulator_rloa_amd.layout import NetLayout
    plan = plan_chain(case.S, case.A, case.H, case.B, p_mode=case.p_mode, env={})
    assert plan.chain == "rows", (case.name, plan.chain)
    return Dims.of(plan, NetLayout(case.S, case.A, case.H), case.B, case.p_mode)

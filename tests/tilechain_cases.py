"""The case table and the starting state of the per-launch checks of the column-tile and the unfused learn() chains
(tests/test_tilechain_launches_gpu.py on the HIP learner, tests/test_tilechain_launches_cpu.py on the float32 stand-in of
oracle/launch_check.py): the smallest shape at which each branch of Learner._learn_rows_tiles and of the non-row-split half of
Learner.forward_train is taken. State, minibatches and the vacuity guard are tests/rowsplit_cases.py's, unchanged: main and target
network differ in every weight and no BatchNorm parameter or running statistic sits at its default.
CPU only: numpy, torch's nn.Linear init and learn_cases.transitions."""
from __future__ import annotations

from learn_cases import Case
from rowsplit_cases import (MAX_ACTIVE, MAX_DEAD_COLUMNS, MIN_ACTIVE, MIN_VNEXT_REL, launch_state, minibatches, vacuity,  # noqa: F401
                            vacuity_ok)

ALL4 = frozenset({"l1", "b2", "gb", "s3"})


def _c(S, A, H, B, p_mode=0, fuse=None, pad=True, data="plain", n_upd=1, chain="columns", tags=(), why=""):
    name = (f"s{S}_a{A}_h{H}_b{B}" + ("_m1" if p_mode else "") + ("_rare" if data == "rare" else "") +
            ({"columns": "_cols", "unfused": "_unf", None: ""}[fuse]) + ("" if pad else "_nopad"))
    return Case(name, S, A, H, B, p_mode, chain, fuse=fuse, pad=pad, data=data, n_upd=n_upd, drop=ALL4 - frozenset(tags), why=why)


# `why` names the branch the size is there for (file and function). `drop` is what the chain's fuse set lacks; chain, tags, the
# slab count of the split-K heads and fold_norm were confirmed with chain_plan.plan_chain(..., env={})
# (test_tilechain_launches_cpu.py::test_the_table_reaches_the_branches_it_names holds them).
CASES = [
    # ---- column-tile chain (csrc/fused_layers.hip) -----------------------------------------------------------------------------
    _c(21, 6, 256, 2, tags=("l1", "b2", "s3"),
       why="the smallest batch BatchNorm takes (unbiased variance B / (B - 1) = 2); chain_plan._choose: B % 16 != 0 drops gb, so "
           "torch.mm dWh / dW2 / dA1 and naf_grad_norm_partials"),
    _c(21, 6, 256, 9, tags=("l1", "b2", "s3"), why="below 16: one partial row phase of the 8 x 64 tile (fused_layers.hip RPT = 2)"),
    _c(21, 6, 256, 15, 1, data="rare", tags=("l1", "b2", "s3"),
       why="the last size before the row-split chain (chain_plan._choose: bb_ok from 16); L L^T head"),
    _c(21, 6, 256, 16, fuse="columns", tags=ALL4,
       why="the first size with the backward bundle (gemm_bundle.hip, plain three-product form) and folded norm partials "
           "(chain_plan.plan_chain: fold)"),
    _c(21, 6, 256, 512, 1, fuse="columns", data="rare", tags=ALL4,
       why="8 rows per thread (fused_layers.hip RPT_DISPATCH: RPT = 8, the last staged size), the chain's largest batch"),
    _c(26, 8, 256, 256, 1, fuse="columns", tags=ALL4,
       why="K = 26 at 4 rows per thread: the last size that keeps l1 (chain_plan._choose: S > 24 and B > 256); 8 joints, NHP = 48"),
    _c(26, 8, 256, 272, 1, fuse="columns", tags=("b2", "gb", "s3"),
       why="one step further: l1 dropped — torch.bmm layer 1 + naf_bn_relu_fwd_train(1), naf_bn_relu_bwd(1) + torch.mm dW1"),
    _c(40, 4, 256, 32, data="rare", tags=("b2", "gb", "s3"), why="state size 40 (chain_plan._choose: S > 32): no l1; NHP = 16"),
    _c(11, 1, 256, 64, 1, fuse="columns", tags=ALL4, why="one joint: A = T = 1, NHP = 16, K = 11"),
    _c(21, 6, 128, 48, fuse="columns", pad=False, tags=ALL4,
       why="unpadded 128: the other slab count of the split-K head (naf_head_fwd_bwd_mse_splitk: n_slabs = 16)"),
    _c(21, 6, 200, 100, pad=False, tags=("l1", "b2"),
       why="unpadded 200: H % 16 != 0 drops gb, H not in (128, 256) drops s3 — torch.bmm heads + naf_head_fwd_bwd_mse"),
    _c(21, 6, 640, 32, tags=("l1", "b2", "gb"), why="a layer wider than 512 (bb_ok false): 80 column tiles, no s3"),
    # ---- unfused chain (torch GEMMs + csrc/bn_relu.hip, naf_head.hip, naf_head_wide.hip) ----------------------------------------
    _c(21, 6, 256, 64, 1, fuse="unfused", n_upd=2, chain="unfused", tags=("gb",),
       why="8 x 64 BatchNorm tile (bn_relu.hip BN_DISPATCH: B <= 512); the second update starts from running statistics the "
           "first one moved"),
    _c(21, 6, 256, 513, fuse="unfused", data="rare", chain="unfused",
       why="first size on the 8 x 128 tile (BN_DISPATCH: B > 512), one row in its last phase; B % 16 != 0: torch backward GEMMs"),
    _c(21, 6, 256, 528, fuse="unfused", chain="unfused", tags=("gb",), why="8 x 128 tile with the bundle"),
    _c(21, 6, 256, 2049, fuse="unfused", data="rare", chain="unfused",
       why="first streamed BatchNorm size (bn_relu.hip: B > BN_MAX_B = 2048), forward and backward, both layers"),
    _c(21, 6, 256, 2064, 1, fuse="unfused", chain="unfused", tags=("gb",), why="streamed BatchNorm with the bundle, L L^T"),
    _c(30, 12, 256, 32, 1, chain="unfused", tags=("gb",),
       why="12 joints (chain_plan._choose: A > 8 off the row-split chain): naf_head_wide.hip, 16-lane groups"),
    _c(43, 17, 256, 33, data="rare", chain="unfused", why="17 joints: naf_head_wide.hip 32-lane groups, odd batch"),
    _c(75, 33, 256, 16, chain="unfused", tags=("gb",), why="33 joints: 64-lane groups, first size; 4 samples per loss partial"),
    _c(73, 32, 256, 48, 1, chain="unfused", tags=("gb",), why="32 joints: the last 32-lane size, L L^T"),
    _c(137, 64, 256, 32, chain="unfused", tags=("gb",), why="the widest head: 64 joints, NHP = 2160"),
]
BY_NAME = {c.name: c for c in CASES}

# With many joints the quadratic term dominates Q at torch's init: at seed 1 max|V'| / max|Q| is 0.028 (32 joints), 0.038
# (64 joints) and 0.090 (8 joints, L L^T, B = 256), below the guard's 0.1. Both networks' value.weight / value.bias times this
# power of two (rowsplit_cases.launch_state), chosen on the CPU in float64 alone as the smallest power of two that meets the
# guard; max|V'| / max|Q| with it: 0.116, 0.143, 0.177
# (test_tilechain_launches_cpu.py::test_the_state_is_not_vacuous holds the guard, ::test_value_scales_are_the_smallest the choice).
VALUE_SCALE = {"s73_a32_h256_b48_m1": 4.0, "s137_a64_h256_b32": 4.0, "s26_a8_h256_b256_m1_cols": 2.0}


def tile_state(case: Case):
    """(main, target) of a case: rowsplit_cases.launch_state at the default seed, with the case's value scale."""
    return launch_state(case, value_scale=VALUE_SCALE.get(case.name, 1.0))


def plan_of(case: Case):
    from robotic_manipulator_rloa_amd.chain_plan import plan_chain
    return plan_chain(case.S, case.A, case.H, case.B, p_mode=case.p_mode, fuse=case.fuse, pad_layer=case.pad, env={})


def dims(case: Case):
    """oracle.launch_check.Dims of a case, from chain_plan.plan_chain (host arithmetic: no GPU)."""
    from oracle.launch_check import Dims
    from robotic_manipulator_rloa_amd.layout import NetLayout
    plan = plan_of(case)
    assert plan.chain == case.chain and "bb" not in plan.fuse, (case.name, plan.chain, plan.fuse)
    return Dims.of(plan, NetLayout(case.S, case.A, case.H, pad_layer=case.pad), case.B, case.p_mode)

"""Which chain of launches a shape's learn() runs, and every integer that follows from the choice: plan_chain() -> ChainPlan.

Pure host arithmetic: no tensor, no HIP call, no GPU needed (the library's host-only integer helpers are asked for the constants the
kernels own). Learner.__init__ (learner.py) takes the plan and allocates by it; tests/test_chain_plan_cpu.py holds it to a recorded
table (tests/golden/chain_plan.json).

    python -m robotic_manipulator_rloa_amd.chain_plan S A H B [p_mode]        prints the plan's fields, one per line
"""
from __future__ import annotations

import os
from dataclasses import dataclass, fields
from typing import FrozenSet, Mapping, Optional, Tuple

from . import _lib
from .layout import BB_MAX_JOINTS, BB_MAX_STATE, NetLayout


@dataclass(frozen=True)
class ChainPlan:
    """What Learner's constructor derives from the shape and the rest of the class consumes. The row-split extras are None off that
    chain, the column-tile extras None without the split-K heads ("s3")."""
    # the choice and the layout
    chain: str                      # "rows" | "columns" | "unfused"
    fuse: FrozenSet[str]            # the tags forward_train / learn_rows read
    bb_ok: bool                     # the shape fits the row-split chain
    Bp: int                         # rows of the work buffers
    hk_rows: Optional[int]          # rows per block of the fused layer-2 launch's backward partials
    # the optimizer
    fold_norm: bool                 # the gradient's producers leave its sum-of-squares partials
    defer_ok: bool                  # the optimizer step may ride on the next update's first two launches
    # the norm partials
    n_partials_norm: int
    n_partials_fold: int
    n_partials: int
    # block counts
    gb_blocks: int                  # dWh + dW2 blocks of the backward bundle
    gb_wh_blocks: int
    ft_blocks: int                  # workgroups of the column-tile kernels
    n_loss_wg: int
    # the row-split chain
    nb: Optional[int]               # 64-row statistics blocks
    nb1: Optional[int]              # 32-row blocks of the bundle's dA1 product
    kp: Optional[int]
    mom_floats: Optional[int]
    ks_w2: Optional[int]            # split-K ranges of the bundle's dW2 | dWh products
    ks_wh: Optional[int]
    keep_xhat1: bool                # layer 1's xhat kept by the forward pass (XH1)
    exchange_floats: Optional[int]  # where the two halves of an H = 512 layer-2 launch meet (None at H = 256)
    # the column-tile chain's split-K heads
    n_slabs: Optional[int]
    slab_stride: Optional[int]
    warning: Optional[str]          # what the constructor warns with
    act_fused: bool                 # ActPath: one launch for the whole act()


# Three chains of launches implement one learn(); `fuse` (a set of tags, read by forward_train / learn_rows) says which:
#   "rows"     {bb, gb, hk, ep, s2}: the ROW-SPLIT chain of csrc/big_batch.hip — 64-row blocks over the whole chip, two-stage
#              BatchNorm statistics, GEMM 2 on f32 MFMA, layer 2 + heads + NAF head + first backward stage in one launch
#              (hk), the backward GEMMs as one launch (gb) that also carries the second stage of layer 2's BatchNorm
#              backward as its prologue (s2) and the batch pass of layer 1's backward as its epilogue (ep), a finish
#              launch — 5 launches per update in a chain of updates. Needs 16 <= B <= 4096 (any size in it), H = 256 | 512, S <= 32,
#              A <= 8 (A <= 11 up to B = 2048).
#              Default wherever the shape fits (measured at the end of round 3, updates/s, column-tile | row-split: B = 64:
#              32.3k | 36.0k, 128: 30.7k | 35.4k, 192: 25.8k | 34.0k, 256: 25.7k | 34.7k, 512: 20.3k | 30.9k; until then the
#              column-tile chain led below B = 256 — 32.5k | 29.3k at 64 in round 2).
#   "columns"  {l1, b2, gb, s3}: the COLUMN-TILE chain of csrc/fused_layers.hip — a workgroup owns 8 feature columns x all
#              B rows (ceil(B/64) <= 8 rows per thread in registers), the K = state-size and N = heads GEMMs folded into
#              the BatchNorm kernels, 8 launches per update. B <= 512. Default below B = 16 (and up to 512 where H or S
#              do not fit the row-split chain). (B = 16 ... 63 moved to the row-split chain in round 4: one partial
#              block — 37.1k against 31.0k updates/s at B = 32, 36.5k against 21.1k at 63.)
#   "unfused"  {gb} or {}: torch (rocBLAS) GEMMs + the BatchNorm / head kernels of csrc/bn_relu.hip, naf_head.hip, with
#              the backward GEMM bundle where its shapes allow (B, H multiples of 16) — any shape up to B = 4096; 14
#              launches per update (round 1's chain: 12.7k updates/s at B = 1024).
# NAF_FUSE = rows | columns | unfused overrides the choice (a chain whose shape limits are not met falls to the next).
#
# The reference takes any positive batch_size (rl_framework.py:186-189). Here: every size up to 4096 trains — 16 ... 4096
# on the row-split chain, smaller ones on the column-tile chain, other layer / state sizes on the unfused chain (beyond 2048
# with the streamed BatchNorm kernels of csrc/bn_relu.hip) with a warning that names the row-split chain's range. 4096 is
# the replay sampler's limit (one workgroup draws a minibatch without replacement in LDS, csrc/replay.hip).
def _choose(lay: NetLayout, B: int, p_mode: int, fuse: Optional[str], env: Mapping[str, str]) -> Tuple[str, set, bool, Optional[str]]:
    """(chain, fuse tags, bb_ok, warning) of a shape. The `fuse` argument wins over NAF_FUSE."""
    if B < 1 or B > (1 << 20):
        raise ValueError(f"batch_size {B}: 1 <= batch_size <= 1,048,576 (the replay sampler's table, csrc/replay.hip)")
    # (round 4: ANY batch size from 16 to 4096 — the last 64-row block of layer 1 / GEMM 2, the last 16-row workgroup of the fused
    #  layer-2 + head launch and the last block of the bundle's dA1 product may be partial: rows past the batch read as zeros, are
    #  never stored and stay out of every statistic and sum. The work buffers hold Bp = the next multiple of 16 rows (of 32 beyond
    #  B = 2048, where the fused layer-2 + head launch runs 32 rows per workgroup),
    #  zero-initialised: the weight-gradient products walk Bp rows as their K dimension, and a row past the batch is a zero in at
    #  least one operand of each — dH and dY2 rows the head body never writes, A1 rows layer 1 never stores.)
    # (round 6, late: state sizes up to 32 — the layer-1 kernels' K — and 9 .. 11 joints: the fused layer-2 launch then holds one
    #  sample per 16-lane group and a Wh tile of 64 | 80 rows, 16 rows per workgroup only, hence B <= 2048; csrc/big_batch.hip.
    #  The reference's state is 9 + 2 A floats, environment.py:261: 27 | 29 | 31 at 9 | 10 | 11 joints)
    #  (beyond 2048 — 32 rows per workgroup — with the reference's Hadamard head only: the matmul mode's L tiles do not fit there)
    bb_ok = (16 <= B <= 4096 and lay.H in (256, 512) and lay.S <= BB_MAX_STATE and
             (lay.A <= 8 or (lay.A <= BB_MAX_JOINTS and (B <= 2048 or p_mode == _lib.P_HADAMARD))))
    want = (fuse or env.get("NAF_FUSE", "default")).lower()
    if want not in ("default", "rows", "columns", "unfused"):
        raise ValueError(f"NAF_FUSE / fuse = {want!r}: one of default, rows, columns, unfused")
    if want == "default":
        want = "rows" if bb_ok else ("columns" if B <= 512 else "unfused")
    if want == "rows" and not bb_ok:
        want = "columns" if B <= 512 else "unfused"
    if lay.A > 8 and want != "rows":
        want = "unfused"                   # (9 .. 16 joints: the column-tile kernels hold one sample per 8-lane group)
    if want == "rows":
        tags = {"bb", "gb", "hk", "ep", "s2"}
    elif want == "columns" and B <= 512:
        tags = {"l1", "b2", "gb", "s3"}
        if lay.S > 32 or (lay.S > 24 and B > 256):
            tags -= {"l1"}                 # (K = 25 .. 32: the layer-1 backward tile holds at most 4 rows per thread)
        if lay.H not in (128, 256):
            tags -= {"s3"}
    else:
        want = "unfused"
        tags = {"gb"}
    if (B % 16 != 0 and want != "rows") or lay.H % 16 != 0:
        tags -= {"gb"}                     # the MFMA kernels take whole 16 x 16 x 16 steps: M, N, K % 16 == 0
    warning = None
    if lay.A > 8 and want != "rows":
        warning = (f"action_size {lay.A} at batch_size {B}, state_size {lay.S} runs the unfused chain: the row-split "
                   f"chain takes up to {BB_MAX_JOINTS} joints at 16 <= batch_size <= 4096 (2048 with p_mode matmul), state_size <= {BB_MAX_STATE} "
                   f"(every arm the reference ships has 6 or 7: KUKA / xArm, Panda)")
    elif B > 512 and want != "rows":
        # (a performance cliff, not an error: say so once, with the sizes that avoid it)
        warning = (f"batch_size {B} at H = {lay.H}, S = {lay.S} runs the unfused chain (about half the updates/s of the "
                   f"row-split chain): the row-split kernels need 16 <= batch_size <= 4096, layer_size <= 512 and "
                   f"state_size <= {BB_MAX_STATE}")
    return want, tags, bb_ok, warning


def _k_ranges(Bp: int, target: int, most: int) -> int:
    """largest number of equal K ranges <= most, each whole 16-k steps and at least `target` rows long"""
    return max([d for d in range(1, most + 1) if Bp % d == 0 and (Bp // d) % 16 == 0 and Bp // d >= target] or [1])


def _bundle_blocks(M: int, N: int, k_split: int) -> int:
    """32 x 32 blocks of one product of the bundle (csrc/gemm_bundle.hip)"""
    return ((M + 31) // 32) * ((N + 31) // 32) * k_split


def _split_k(lay: NetLayout, Bp: int) -> Tuple[int, int]:
    """(ks_w2, ks_wh): into how many K ranges the row-split chain's bundle cuts its two weight-gradient products."""
    # The weight gradients reduce over K = B. Cut K into ranges, one grid of blocks each, writing partial slabs that
    # the layer-1 finish launch adds in slab order (and takes the norm partials of): 256-row ranges — with every launch
    # of the chain working by eighths of the batch (csrc/big_batch.hip, bb_place_rows) a 256-row range is what one XCD
    # (or two) already holds of dY2, Z2 and A1. For dW2 twice as long (512 rows) where the launch would otherwise not fit
    # the chip at once — more than the 1024 blocks the four-wave form of the bundle has room for: B = 2048 (1096 blocks
    # with eight ranges, 840 with four). Updates/s with 256- | 512-row ranges, A/B/A/B on one box at the end of round 3:
    # B = 1024 28.0k | 27.0k, 1536 22.7k | 22.0k, 2048 20.9k | 21.3k. (Round 2 had it the other way round at 1024 — 420
    # blocks in one round of the eight-wave form against 548 — before the rows went to the XCDs by eighths.) Batch sizes
    # that are not multiples of 256: as many equal ranges (<= 8, whole 64-row blocks) as divide B / 64.
    H, HP, NHP = lay.H, lay.HP, lay.NHP
    ks = Bp // 256 if (Bp % 256 == 0 and Bp <= 2048) else _k_ranges(Bp, 256, 8)      # (at most 8 slabs: csrc/big_batch.hip)
    ks_w2 = ks_wh = ks
    # (round 4's LDS-DMA ring form of this launch measured slower at every size: benchmarks/experimental/gemm_ring.h)
    if _bundle_blocks(Bp, H, 1) + _bundle_blocks(H, H, ks) + _bundle_blocks(NHP, HP, ks) + 8 > 1024 and ks % 2 == 0 and \
            (Bp // (ks // 2)) % 256 == 0:
        ks_w2 = ks // 2
    return ks_w2, ks_wh


FINISH_SMALL_NB1, FINISH_SMALL_SLABS = 16, 2      # BF_SMALL_NB1, BF_SMALL_SLABS of csrc/big_batch.hip


def finish_small(nb1: int, nb: int, n_slabs, push: bool = False, merge: bool = False) -> bool:
    """Whether the finish launch of the row-split chain takes its small form when the library chooses (csrc/big_batch.hip,
    bb_finish_launch, whose rule this restates): no gradient exchange rides on it, at most 16 blocks of the dA1 product (B <= 512),
    at most 64 statistics blocks of layer 2's bias gradient, at most 2 slabs in every slab segment (n_slabs: one count per segment)."""
    return (not push and not merge and nb1 <= FINISH_SMALL_NB1 and nb <= 64 and
            all(n <= FINISH_SMALL_SLABS for n in n_slabs))


def plan_chain(state_size: int, action_size: int, layer_size: int, batch_size: int, p_mode: int = _lib.P_HADAMARD,
               world_size: int = 1, fuse: Optional[str] = None, pad_layer: bool = True, force_allreduce: bool = False,
               fold_norm: bool = True, env: Mapping[str, str] = os.environ) -> ChainPlan:
    """The plan of Learner(state_size, action_size, layer_size, batch_size, ...): see ChainPlan and the comment above _choose.
    fuse: "rows" | "columns" | "unfused" | None (= NAF_FUSE or the per-shape default). force_allreduce / fold_norm: Learner's
    test-only arguments. env: where NAF_FUSE and NAF_DEFER_ADAM are read.
    World sizes beyond 1 change three fields and nothing else: fold_norm is False, n_partials is n_partials_norm (until the
    exchange form is set, Learner._set_exchange), and defer_ok is `"bb" in fuse and NAF_DEFER_ADAM != "0"`."""
    lib = _lib.load()
    lay = NetLayout(state_size, action_size, layer_size, pad_layer=pad_layer)
    B, world_size = int(batch_size), int(world_size)
    chain, tags, bb_ok, warning = _choose(lay, B, int(p_mode), fuse, env)
    bb = "bb" in tags
    # with every gradient element produced by one of our own kernels, those kernels also emit its sum-of-squares partial:
    # the separate grad-norm launch disappears. Data-parallel runs keep it (the norm is taken on the all-reduced gradient).
    fold = bool(({"l1", "b2", "gb"} <= tags or {"bb", "gb"} <= tags) and world_size == 1 and not force_allreduce and fold_norm)
    P, H, HP, NHP = lay.P, lay.H, lay.HP, lay.NHP
    # rows of the work buffers: whole 16-row groups on the row-split chain (see bb_ok above), B everywhere else
    # (beyond B = 256 whole 64-row blocks: the K ranges of the weight-gradient products then divide as they do for the next
    #  multiple of 64 — B = 1000 runs the products of B = 1024 with 24 zero rows, four 256-row ranges instead of three of 336)
    pad_rows = (lib.naf_bb_layer2_head_rows(B) if B <= 256 else 64) if bb else 1
    Bp = -(-B // pad_rows) * pad_rows
    ft_tx = lib.naf_fused_tile_cols()
    ft_blocks = (H + ft_tx - 1) // ft_tx                               # workgroups of the column-tile kernels
    gb_wh_blocks = ((NHP + 31) // 32) * ((HP + 31) // 32)
    gb_blocks = gb_wh_blocks + ((H + 31) // 32) ** 2                   # dWh + dW2 blocks of the bundle
    n_partials_norm = (P + _lib.NORM_CHUNK - 1) // _lib.NORM_CHUNK
    # folded norm partials: the bundle's dWh + dW2 blocks, then the column-tile kernels (two launches of ft_blocks) or,
    # in the large-batch chain, the workgroups of the layer-1 finish kernel (two columns each)
    n_partials_fold = gb_blocks + 2 * ft_blocks
    if bb:
        n_partials_fold = lib.naf_bb_layer1_bwd_finish_blocks(H) + (H * H + 1023) // 1024 + (NHP * HP + 1023) // 1024
    # the optimizer step of update k carried by the first two launches of update k + 1 (csrc/adam_body.h): the row-split
    # chain on one rank, gradient norm folded into the producers. NAF_DEFER_ADAM=0 keeps the launch of its own.
    # Data parallel over peer memory: the one-shot all-reduce launch leaves the norm partials and the step count exactly
    # as the folded producers do on one rank, so the step can ride there too (the RCCL path keeps its two launches).
    # The collective path (RCCL, or the test-only forced all-reduce): the norm must be taken on the REDUCED gradient, so a norm
    # launch stays behind the collective — and the optimizer step rides on the next update behind it all the same (round 4:
    # one launch and one boundary less per update there too; before, that path kept both launches).
    defer_ok = bool(bb and env.get("NAF_DEFER_ADAM", "1") != "0" and
                    ((fold and world_size == 1) or world_size > 1 or force_allreduce))
    rows = dict(nb=None, nb1=None, kp=None, mom_floats=None, ks_w2=None, ks_wh=None, exchange_floats=None)
    if bb:
        ks_w2, ks_wh = _split_k(lay, Bp)
        rows = dict(
            nb=-(-B // 64),                                      # 64-row statistics blocks (the last may hold 16, 32 or 48 rows)
            nb1=-(-Bp // 32),                                    # 32-row blocks of the bundle's dA1 product (M = Bp rows)
            kp=lib.naf_bb_layer1_bwd_kp(lay.S), mom_floats=lib.naf_bb_moments_floats(lay.S), ks_w2=ks_w2, ks_wh=ks_wh,
            # (H = 512: the fused layer-2 launch runs two workgroups per row block, one per 256-column half; their partial heads meet here)
            exchange_floats=max(4, lib.naf_bb_layer2_head_exchange_floats(B, NHP)) if H > 256 else None)
    s3 = "s3" in tags
    return ChainPlan(
        chain=chain, fuse=frozenset(tags), bb_ok=bb_ok, Bp=Bp, hk_rows=lib.naf_bb_layer2_head_rows(B) if bb else None,
        fold_norm=fold, defer_ok=defer_ok,
        n_partials_norm=n_partials_norm, n_partials_fold=n_partials_fold, n_partials=n_partials_fold if fold else n_partials_norm,
        gb_blocks=gb_blocks, gb_wh_blocks=gb_wh_blocks, ft_blocks=ft_blocks,
        # loss partials per update: one per workgroup of the head launch (8 samples each; 4 beyond 32 joints, csrc/naf_head_wide.hip)
        n_loss_wg=(B + 7) // 8 if lay.A <= 32 else (B + 3) // 4,
        # (xhat of layer 1 kept by the forward pass for the epilogue up to B = 512 — one round of blocks, where recomputing it
        # sat on the critical path: updates/s 36.0k -> 36.8k at B = 64, 35.2k -> 36.0k at 128, 34.6k -> 35.1k at 256, 31.25k ->
        # 31.5k at 512; beyond that the recomputation hides and the extra B x H floats each way do not: 28.3k -> 27.7k at 1024)
        keep_xhat1=bb and B <= 512,
        # split-K heads: one [B, NHP] slab per 8-column workgroup of layer 2's BN kernel (+ the target's V column)
        # slabs 256 B further apart than their size: the H/8 pieces of one row, read together by the head kernel,
        # then sit in different L2 channels instead of one (32-KB stride: 6.6 us per head launch, padded: see DESIGN)
        n_slabs=H // 8 if s3 else None, slab_stride=B * NHP + 64 if s3 else None,
        warning=warning,
        # one launch for the whole act() (csrc/policy_act.hip) when the shapes are the framework's (H = 256, S <= 32);
        # other shapes take the seven-launch path (3 GEMMs, 2 BN kernels, noise, counter)
        # (round 6: up to 11 joints — the state's group in the noise body is then 16 lanes wide)
        #  and layer sizes up to 512 — stored as 512: policy_act_512_kernel)
        act_fused=lay.H in (256, 512) and lay.S <= 32 and lay.A <= BB_MAX_JOINTS, **rows)


if __name__ == "__main__":
    import sys
    plan = plan_chain(*[int(a) for a in sys.argv[1:6]])
    for f in fields(plan):
        v = getattr(plan, f.name)
        print(f"{f.name}: {','.join(sorted(v)) if isinstance(v, frozenset) else v}")

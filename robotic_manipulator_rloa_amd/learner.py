"""Flat-buffer NAF learner: the MI355X implementation of NAFAgent.learn() + soft_update
(reference naf_components/naf_algorithm.py:180-226) and of NAF.forward's training pass
(naf_components/naf_neural_network.py:76-115).

Design:
  * all learner state lives in a few flat f32 HBM allocations: theta2[2, P] (row 0 = main net, row 1 = target
    net), grad[P], adam m[P], v[P]; parameters of the nn.Module facades are views into them.
  * the big trunk GEMMs stay on PyTorch-ROCm (torch.bmm / torch.mm with out=; rocBLAS kernels picked by the shipped
    TunableOp results); main and target forward share every launch (batch-2 bmm, 2-net BN kernel).
  * everything else is libnaf_hip.so: bias+BatchNorm+ReLU fwd/bwd (with the K=21 and N=32 GEMMs folded in), the
    fused NAF head (fwd + TD target + MSE + bwd), the backward GEMM bundle on f32 MFMA, grad-norm partials,
    clip+Adam+Polyak in one pass.
  * the three head Linears are one GEMM against Wh[NHP, H+8]: column H of Wh is the bias and the activation
    buffer carries a constant-1 column there, so bias add and bias gradient ride inside the GEMMs.
  * no host sync anywhere: step count, clip factor, replay size and sampler counters live on the device, so a
    chunk of U updates (sample -> gather -> U x learn) is captured once as a HIP graph and replayed.
"""
from __future__ import annotations

import os

import numpy as np
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .chain_plan import finish_small, plan_chain
from .layout import NetLayout
from .parallel import XgmiAllReduce, all_reduce_flat_grad

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
MAX_GRAD_NORM = 1.0


_BLAS_CONFIGURED = False
TUNING_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuning", "tunableop_gfx950.csv")


def configure_blas() -> str:
    """Pick the GEMM kernels PyTorch-ROCm will use for the (tiny) trunk GEMMs.
    Measured on MI355X (benchmarks/gemm_probe.py, B=256): hipBLASLt's default heuristic runs the 256x256x256 f32
    GEMMs as ONE 256x256 macro-tile on one CU (63 us each, 239 us for the 8 GEMMs of an update); rocBLAS takes
    42 us for the 8; with the shipped TunableOp results (best rocBLAS/hipBLASLt solution per shape) 26 us.
    Env: NAF_BLAS_DEFAULT=1 leaves torch's BLAS settings untouched; NAF_BLAS_TUNING_FILE overrides the results file
    ('none' disables it)."""
    global _BLAS_CONFIGURED
    if _BLAS_CONFIGURED or os.environ.get("NAF_BLAS_DEFAULT") == "1":
        _BLAS_CONFIGURED = True
        return "default"
    _BLAS_CONFIGURED = True
    torch.backends.cuda.preferred_blas_library("cublas")           # = rocBLAS on ROCm
    path = os.environ.get("NAF_BLAS_TUNING_FILE", TUNING_FILE)
    if path != "none" and os.path.exists(path):
        try:
            torch.cuda.tunable.enable(True)
            torch.cuda.tunable.tuning_enable(False)                # look up only: never tune inside a training run
            torch.cuda.tunable.read_file(path)
            return "rocblas+tunableop"
        except Exception:                                          # results from another library build: ignore them
            torch.cuda.tunable.enable(False)
    return "rocblas"


PARAM_ORDER = ["input_layer.weight", "input_layer.bias", "bn1.weight", "bn1.bias", "hidden_layer.weight",
               "hidden_layer.bias", "bn2.weight", "bn2.bias", "action_values.weight", "action_values.bias",
               "value.weight", "value.bias", "matrix_entries.weight", "matrix_entries.bias"]


class Learner:
    """Owns the flat learner state of one agent (main + target) and enqueues learn() updates on the current
    stream. Everything is asynchronous; nothing here calls .item()/.cpu()."""

    def __init__(self, state_size: int, action_size: int, layer_size: int, batch_size: int, learning_rate: float,
                 tau: float, gamma: float, device: torch.device, p_mode: int = _lib.P_HADAMARD,
                 world_size: int = 1, process_group=None, fuse: Optional[str] = None, _force_allreduce: bool = False,
                 _fold_norm: bool = True, pad_layer: bool = True, _xgmi=None, _finish_form: int = _lib.FINISH_AUTO):
        """fuse: "rows" | "columns" | "unfused" | None (= NAF_FUSE or the per-shape default, see chain_plan.py). The underscore
        arguments are for tests: run the gradient all-reduce at world size 1 / keep the separate grad-norm launch; _finish_form
        (tests and A/B runs): the form of the row-split chain's finish launch, _lib.FINISH_AUTO | FINISH_GENERAL | FINISH_SMALL.
        pad_layer: a layer_size below 256 is stored zero-padded to 256 (NetLayout) and runs the kernels built for that width;
        False: its own width on the column-tile / unfused chains (tests compare the two).
        Which chain of launches the shape gets, and every count that follows from it, is chain_plan.plan_chain's to say (self.plan);
        the methods below allocate by it."""
        _lib.require_gpu()
        self.lib = self._f = _lib.load()
        self.blas = configure_blas()
        self.dev = torch.device(device)
        self.plan = plan = plan_chain(state_size, action_size, layer_size, batch_size, p_mode=p_mode, world_size=world_size,
                                      fuse=fuse, pad_layer=pad_layer, force_allreduce=_force_allreduce, fold_norm=_fold_norm)
        if plan.warning:
            import warnings
            warnings.warn(plan.warning, stacklevel=3)
        self.lay = NetLayout(state_size, action_size, layer_size, pad_layer=pad_layer)
        self.B = int(batch_size)
        self.lr, self.tau, self.gamma = float(learning_rate), float(tau), float(gamma)
        self.p_mode = int(p_mode)
        self.world_size = int(world_size)
        self.pg = process_group
        self._force_allreduce = bool(_force_allreduce)
        self._finish_form = int(_finish_form)
        # what the launch methods, engine.py and the benchmarks read of the plan: plain attributes, copied once
        self.chain, self.fuse, self.bb_ok, self.Bp, self.hk_rows = plan.chain, plan.fuse, plan.bb_ok, plan.Bp, plan.hk_rows
        self.fold_norm, self.defer_ok = plan.fold_norm, plan.defer_ok
        self.n_partials, self.n_partials_fold, self.n_partials_norm = plan.n_partials, plan.n_partials_fold, plan.n_partials_norm
        self.n_loss_wg = plan.n_loss_wg
        self._nb1, self._gb_blocks, self._ft_blocks, self._gb_wh_blocks = plan.nb1, plan.gb_blocks, plan.ft_blocks, plan.gb_wh_blocks
        self.mom_floats, self.n_slabs, self.slab_stride = plan.mom_floats, plan.n_slabs, plan.slab_stride
        self._f32 = dict(dtype=torch.float32, device=self.dev)
        self._open_exchange(_xgmi)
        self._alloc_state()
        self._alloc_work_buffers()
        if "s3" in self.fuse:
            self._alloc_head_slabs()
        self._make_gemm_views()
        if "bb" in self.fuse:
            self._alloc_row_split()
        if self.world_size > 1:
            self._pick_exchange()

    def _open_exchange(self, _xgmi) -> None:
        """The gradient exchange's communicator (data parallel), before anything is sized by it."""
        # Data parallel inside one node — three forms of the one exchange (the sum of the flat gradient over the ranks, where
        # loss.backward() -> clip_grad_norm_ sit in the reference, naf_algorithm.py:207-210):
        #   "oneshot"  the one-shot peer-memory all-reduce as a launch of its own behind the finish launch (csrc/xgmi_reduce.hip; the
        #              finish launch pushes 91 % of the bytes early)
        #   "merged"   the whole exchange INSIDE the finish launch of the row-split chain (csrc/big_batch.hip, bb_finish_exchange):
        #              five launches per update as on one GPU
        #   "rccl"     torch.distributed's all-reduce (RCCL over xGMI) captured in the graph + a norm launch
        # The peer-memory forms exist when every rank could map every peer and the exact self-test passed on all of them
        # (XgmiAllReduce.try_create is collective; NAF_XGMI=0 skips it). WHICH form runs is measured where the job runs:
        # autotune_exchange() (end of the constructor) times them on this node and every rank takes the collectively fastest —
        # the one-GPU rehearsal ranks them oneshot < merged < collective, real xGMI may not (a peer's slab is not behind the
        # writer's L2 there). NAF_DP_EXCHANGE = oneshot | merged | rccl pins the form instead.
        P = self.lay.P
        self.xgmi = None
        self._xg = None                    # the communicator the CURRENT form uses (None: the collective)
        self.xgmi_merged = False
        self.exchange = "none" if self.world_size == 1 else "rccl"
        self.exchange_autotune = None      # {form: us per update ..., "chosen": form} once autotune_exchange() has run
        self._exchange_pick = "auto"
        self._push_desc = None
        if _xgmi is not None:
            # a communicator handed in (XgmiAllReduce.local_group: the in-process rehearsal of world sizes beyond what a one-GPU
            # box hosts as processes); the exchange form must then be pinned — nothing here is collective
            if _xgmi.world != self.world_size or _xgmi.n != P or os.environ.get("NAF_DP_EXCHANGE", "auto") not in ("oneshot", "merged"):
                raise ValueError("Learner(_xgmi=...): a communicator of this world size and length, NAF_DP_EXCHANGE = oneshot | merged")
            self.xgmi = _xgmi
        elif self.world_size > 1 and os.environ.get("NAF_XGMI", "1") != "0":
            self.xgmi = XgmiAllReduce.try_create(P, self.dev, self.pg)

    def _alloc_state(self) -> None:
        """Persistent state: parameters, gradient, optimizer state, BatchNorm statistics, norm partials."""
        P, H, dev, f32 = self.lay.P, self.lay.H, self.dev, self._f32
        self.theta2 = torch.zeros(2, P, **f32)             # [main; target]
        self.grad = torch.zeros(P, **f32)
        self.adam_m = torch.zeros(P, **f32)
        self.adam_v = torch.zeros(P, **f32)
        # BN running statistics [net][rm1, rv1, rm2, rv2][H]; not in theta: soft_update copies parameters() only
        self.bn_stats = torch.zeros(2, 4, H, **f32)
        self.bn_stats[:, 1].fill_(1.0)
        self.bn_stats[:, 3].fill_(1.0)
        # what the row-split chain reads and advances: the public buffers themselves — except while a pipelined per-timestep chunk
        # (engine.TrainChunk) captures its graphs, whose chains work on copies of their own that the chunk's last launch commits
        self.bn_live = self.bn_stats
        self._gen = 0              # bumped by every method that changes parameters, optimizer state, statistics or the gradient
                                   # when CALLED (graph replays do not count): a pipelined chunk's pending gradient is void then
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)   # optimizer steps taken
        self.step_live = self.step_dev
        n_partials_most = max(self.n_partials_fold + 1, self.n_partials_norm, self.n_partials)
        if self.xgmi is not None:
            n_partials_most = max(n_partials_most, self.xgmi.n_partials)
        self.partials = torch.zeros(n_partials_most + 1, **f32)
        self.adam_bc = torch.zeros(8, **f32)     # the next step's bias corrections, left by the riding optimizer workgroups
        self._adam_args = _lib.AdamArgs(
            ptr(self.theta2[0]), ptr(self.grad), ptr(self.adam_m), ptr(self.adam_v), ptr(self.theta2[1]), ptr(self.partials),
            self.n_partials, MAX_GRAD_NORM, self.lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, self.tau, float(1.0 - self.tau),
            ptr(self.step_dev), 1.0 / self.world_size, P, self.lay.seg["W2"].offset, ptr(self.adam_bc))
        # a poll inside a fused launch that gave up on the folded records and folded for itself (csrc/bn2bwd_fold.h) bumps this
        # pinned HOST word; fold_fallbacks reads it without synchronising
        self.err_host = torch.zeros(8, dtype=torch.int64).pin_memory()

    def _alloc_work_buffers(self) -> None:
        """Work buffers for one minibatch: Bp rows (chain_plan.py says why), zero-initialised."""
        lay, B, Bp, f32 = self.lay, self.B, self.Bp, self._f32
        H, HP, NHP = lay.H, lay.HP, lay.NHP
        self.G1 = torch.zeros(2, Bp, H, **f32)
        self.A1 = torch.zeros(2, Bp, H, **f32)
        self.G2 = torch.zeros(2, Bp, H, **f32)
        self.A2 = torch.zeros(2, Bp, HP, **f32)
        self.A2[:, :, H] = 1.0                               # the constant-1 column that carries the head biases
        self.Gh = torch.zeros(2, Bp, NHP, **f32)
        self.dH = torch.zeros(Bp, NHP, **f32)
        self.dA2 = torch.zeros(Bp, HP, **f32)
        self.dZ2 = torch.zeros(Bp, H, **f32)
        self.dA1 = torch.zeros(Bp, H, **f32)
        self.dZ1 = torch.zeros(Bp, H, **f32)
        self.save_mean = torch.empty(2, 2, H, **f32)         # [layer][net][H]
        self.save_invstd = torch.empty(2, 2, H, **f32)
        self.q_out = torch.empty(B, **f32)

    def _alloc_head_slabs(self) -> None:
        """The column-tile chain's split-K heads: n_slabs slabs of [B, NHP], slab_stride floats apart (chain_plan.py)."""
        self.heads_partial = torch.zeros(self.n_slabs * self.slab_stride, **self._f32)
        self.vnext_partial = torch.zeros(self.n_slabs, self.B, **self._f32)

    def _make_gemm_views(self) -> None:
        """GEMM operand views (built once: no per-call tensor construction on the hot path) and the backward bundle of the
        column-tile / unfused chains."""
        lay, B = self.lay, self.B
        seg, H, HP, NHP = lay.seg, lay.H, lay.HP, lay.NHP
        t2 = self.theta2
        self.W1T2 = t2[:, seg["W1"].offset:seg["W1"].offset + seg["W1"].numel].view(2, H, lay.S).transpose(1, 2)
        self.W2T2 = t2[:, seg["W2"].offset:seg["W2"].offset + seg["W2"].numel].view(2, H, H).transpose(1, 2)
        self.WhT2 = t2[:, seg["Wh"].offset:seg["Wh"].offset + seg["Wh"].numel].view(2, NHP, HP).transpose(1, 2)
        # (running the weight-gradient GEMMs on a forked branch of the captured graph was measured SLOWER — 8.0k vs
        # 12.7k updates/s: hipGraph cross-stream edges cost more than the serial launches they hide — so the update is
        # one linear chain of launches)
        self.W2_main = lay.view(t2[0], "W2")
        self.Wh_main = lay.view(t2[0], "Wh")
        self.gW1 = lay.view(self.grad, "W1")
        self.gW2 = lay.view(self.grad, "W2")
        self.gWh = lay.view(self.grad, "Wh")
        D = _lib.GemmDesc
        pp = self.partials.data_ptr()
        sq_wh = pp if self.fold_norm else None
        sq_w2 = pp + 4 * self._gb_wh_blocks if self.fold_norm else None
        self._bundle = (D * 3)(
            D(ptr(self.dH), ptr(self.A2[0]), ptr(self.gWh), sq_wh, NHP, HP, B, NHP, HP, HP, 1, 1),          # dWh
            D(ptr(self.dZ2), ptr(self.A1[0]), ptr(self.gW2), sq_w2, H, H, B, H, H, H, 1, 1),                  # dW2
            D(ptr(self.dZ2), ptr(self.W2_main), ptr(self.dA1), None, B, H, H, H, H, H, 0, 1))                 # dA1
        self._bb_segs, self._bb_nsegs = None, 0

    def _alloc_row_split(self) -> None:
        """The row-split chain's own buffers and the descriptors of its backward bundle (prologue s2, epilogue ep); the counts are
        the plan's."""
        plan, lay, B, Bp, dev, f32 = self.plan, self.lay, self.B, self.Bp, self.dev, self._f32
        H, HP, NHP, kp = lay.H, lay.HP, lay.NHP, plan.kp
        ks_w2, ks_wh = plan.ks_w2, plan.ks_wh
        # moments record of one minibatch's layer-1 inputs, [net][Sx | C]: everything layer 1's BatchNorm needs from
        # the batch dimension (TrainChunk computes the records of all its minibatches in one launch behind the gather)
        self.bb_mom = torch.zeros(2, self.mom_floats, **f32)
        self.bb_wc = torch.zeros(H, kp, **f32)               # w_c C of the main net, forward -> finish
        self.bb_st2 = torch.zeros(2, plan.nb, H, 2, **f32)   # layer-2 statistics partials per 64-row block: (sum, M2)
        self.bb_bw2 = torch.zeros(Bp // self.hk_rows, H, 2, **f32)   # backward partials of layer 2: (sum dy, sum dy*xhat)
        self.bb_bw1 = torch.zeros(self._nb1, H, 2, **f32)    # backward partials of layer 1, per 32-row block of the bundle
        self.bb_dw1 = torch.zeros(self._nb1, H, kp, **f32)   # per-block shares of P = dY1^T X
        # the split-K slabs of the two weight-gradient products, added in slab order by the finish launch
        self.bb_slab_w2 = torch.zeros(ks_w2, H * H, **f32)
        self.bb_slab_wh = torch.zeros(ks_wh, NHP * HP, **f32)
        t2p_, seg_, gp_ = self.theta2.data_ptr(), lay.seg, self.grad.data_ptr()
        # ep: the batch pass of layer 1's backward as the epilogue of the dA1 blocks (x / ldx: set per minibatch)
        # (xhat of layer 1 kept by the forward pass for the epilogue where the plan says so: keep_xhat1)
        self.XH1 = torch.zeros(Bp, H, **f32) if plan.keep_xhat1 else None
        self._epi = _lib.GemmL1Bwd(None, t2p_ + 4 * seg_["W1"].offset, t2p_ + 4 * seg_["b1"].offset, ptr(self.A1[0]),
                                   ptr(self.save_mean[0, 0]), ptr(self.save_invstd[0, 0]), ptr(self.bb_bw1), ptr(self.bb_dw1),
                                   0, lay.S, kp, H, ptr(self.XH1),
                                   t2p_ + 4 * seg_["g1"].offset, t2p_ + 4 * seg_["be1"].offset, B)
        # s2: dY2 -> dZ2 while the two products that read it stage their A panels; the block sums folded once per launch
        # by the bundle's first workgroups and handed on as tagged records (csrc/gemm_bundle.hip, gemm_bn2bwd_fold_block)
        self.bb_cst = torch.zeros(H, 4, **f32)                                        # per-column constants of the launch
        self.bb_fold_flag = torch.ones(1, dtype=torch.int32, device=dev)              # launch number: finish advances it; never restored
        self._pro = _lib.GemmBn2Bwd(ptr(self.G2[0]), ptr(self.bb_bw2), t2p_ + 4 * seg_["g2"].offset, ptr(self.save_mean[1, 0]),
                                    ptr(self.save_invstd[1, 0]), gp_ + 4 * seg_["g2"].offset, gp_ + 4 * seg_["be2"].offset,
                                    Bp // self.hk_rows, B, H, ptr(self.bb_cst), ptr(self.bb_fold_flag), self.err_host.data_ptr())
        pro_ = _lib.C.addressof(self._pro)
        # layer 2's forward statistics folded once per launch too where a workgroup would pull more than 16 blocks of them
        # (B > 1024; the library decides): records of their own, the same launch counter and error word
        self.bb_stat_rec = torch.zeros(2 * H, 4, **f32)
        # (H = 512: the two workgroups of a row block of the fused layer-2 launch meet here)
        self.bb_exchange = torch.zeros(plan.exchange_floats, **f32) if plan.exchange_floats is not None else None
        self._stats_once_s = _lib.BbStatsOnce(ptr(self.bb_stat_rec), ptr(self.bb_fold_flag), self.err_host.data_ptr(),
                                              ptr(self.bb_exchange))
        self._stats_once = _lib.C.byref(self._stats_once_s)
        # dA1 FIRST: its blocks carry the layer-1 epilogue and run longest; dispatched first, the short weight-gradient
        # blocks fill in behind them instead of the other way round
        D = _lib.GemmDesc
        self._bundle = (D * 3)(
            D(ptr(self.dZ2), ptr(self.W2_main), None, None, Bp, H, H, H, H, H, 0, 1, 1, 0, _lib.C.addressof(self._epi), pro_),
            D(ptr(self.dZ2), ptr(self.A1[0]), ptr(self.bb_slab_w2), None, H, H, Bp, H, H, H, 1, 1, ks_w2, H * H, None, pro_),
            D(ptr(self.dH), ptr(self.A2[0]), ptr(self.bb_slab_wh), None, NHP, HP, Bp, NHP, HP, HP, 1, 1, ks_wh, NHP * HP))
        SS = _lib.SlabSeg
        self._bb_segs = (SS * 2)(SS(ptr(self.bb_slab_w2), ptr(self.gW2), H * H, H * H, ks_w2),
                                 SS(ptr(self.bb_slab_wh), ptr(self.gWh), NHP * HP, NHP * HP, ks_wh))
        self._bb_nsegs = 2

    def _pick_exchange(self) -> None:
        """Which form the gradient exchange takes (data parallel): the pinned one, or the fastest measured here."""
        want_x = os.environ.get("NAF_DP_EXCHANGE", "auto").lower()
        if want_x not in ("auto", "fastest", "oneshot", "merged", "rccl"):
            raise ValueError(f"NAF_DP_EXCHANGE = {want_x!r}: one of auto, fastest, oneshot, merged, rccl")
        forms = self.exchange_forms()
        self._exchange_pick = want_x
        if want_x in ("auto", "fastest"):
            self._set_exchange(forms[0])
            if len(forms) > 1:
                self.autotune_exchange()
        else:
            if want_x not in forms:
                raise _lib.NafHipError(f"NAF_DP_EXCHANGE={want_x}: not available here (forms: {forms})")
            self._set_exchange(want_x)

    # ---- data parallel: the form of the gradient exchange -------------------------------------------------------------
    def exchange_forms(self):
        """The forms this learner can run, fastest-in-the-rehearsal first: see the constructor."""
        if self.world_size == 1:
            return ["none"]
        forms = []
        if self.xgmi is not None:
            forms.append("oneshot")
            if "bb" in self.fuse and self.lay.ends_with_wh:
                forms.append("merged")
        return forms + ["rccl"]

    def _set_exchange(self, form: str) -> None:
        """Switch the exchange of every learn_rows() enqueued (or captured) from now on. Collective in effect: every rank must make
        the same switch between the same two updates."""
        if form not in self.exchange_forms():
            raise ValueError(f"exchange form {form!r} not available (forms: {self.exchange_forms()})")
        self.exchange = form
        self._xg = self.xgmi if form in ("oneshot", "merged") else None
        self.xgmi_merged = form == "merged"
        if self.world_size > 1:
            # who leaves the sum-of-squares partials of the REDUCED gradient, and how many
            self.n_partials = {"oneshot": self.xgmi.n_partials if self.xgmi is not None else 0,
                               "merged": self.n_partials_fold + 1,       # (+ the layer-1 / BatchNorm ranges' entry of the last workgroup)
                               "rccl": self.n_partials_norm}[form]
            self._adam_args.n_partials = self.n_partials

    def autotune_exchange(self, updates: int = 200, chunk: int = 8, verbose: bool = False) -> dict:
        """Time `updates` graph-replayed learn() calls under every available form of the exchange ON THIS NODE, agree on the
        fastest (every rank's time, MAX over the ranks, then the smallest: all ranks see the same three numbers and make the same
        choice) and switch to it. Collective: every rank of the group calls it at the same point — the constructor does. The
        learner's state is put back afterwards bit for bit. Returns {form: us per update, ..., "chosen": form} (also kept as
        self.exchange_autotune; bench.py prints it in its `preflight` object)."""
        import time
        import torch.distributed as dist
        forms = self.exchange_forms()
        lay, B, dev = self.lay, self.B, self.dev
        saved = [(t, t.clone()) for t in (self.theta2, self.grad, self.adam_m, self.adam_v, self.bn_stats, self.step_dev,
                                          self.partials, self.adam_bc)]
        g = torch.Generator(device=dev).manual_seed(1234)          # (the same rows on every rank: timing, not learning)
        rows = torch.randn(chunk, B, lay.batch_row_floats, generator=g, device=dev)
        rows[:, :, lay.S:lay.S + lay.A].clamp_(-1, 1).trunc_()
        store = torch.zeros(chunk * B * lay.batch_row_floats + 64, device=dev)
        store[:rows.numel()].copy_(rows.view(-1))
        rows = store[:rows.numel()].view(chunk, B, lay.batch_row_floats)
        d = self.defer_ok
        nccl = dist.get_backend(self.pg) == "nccl"

        def body():
            for k in range(chunk):
                self.learn_rows(rows[k], pending=d and k > 0, defer=d and k < chunk - 1)

        def restore():
            for live, keep in saved:
                live.copy_(keep)

        # two passes over the forms, the faster reading of each: the first launches of a process read five times too long
        # (clocks, first-touch, code objects) — with one pass the first form timed paid for all of that
        from .parallel import _agree
        times, errors = {}, {}
        for form in forms + forms:
            if form in errors:
                continue
            self._set_exchange(form)
            graph, err = None, None
            capturable = form != "rccl" or nccl              # (gloo, the one-GPU rehearsal's control plane, cannot be captured)
            # A form that cannot be warmed or captured HERE (a collective that refuses stream capture, a mapping that faults) must
            # cost this node that form, not the job: the attempt is fenced, and the ranks agree on its outcome before anyone times
            # anything (a rank that went on alone would wait at the barrier below for ever).
            try:
                body()                                       # warm the launch paths (and the collective's communicator)
                torch.cuda.synchronize(dev)
                if capturable:
                    graph = torch.cuda.CUDAGraph()
                    with _lib.graph_capture(graph):
                        body()
                    torch.cuda.synchronize(dev)
            except Exception as e:                           # noqa: BLE001
                err, graph = f"{type(e).__name__}: {e}"[:300], None
                try:
                    torch.cuda.synchronize(dev)
                except Exception:                            # noqa: BLE001
                    pass
            if not _agree(err is None, dev, self.pg):
                errors[form] = err or "failed on another rank"
                times[form] = float("inf")
                restore()
                continue
            run = graph.replay if graph is not None else body
            reps = max(1, updates // chunk) if graph is not None else max(1, updates // (4 * chunk))
            run()
            torch.cuda.synchronize(dev)
            dist.barrier(group=self.pg)
            t0 = time.perf_counter()
            for _ in range(reps):
                run()
            torch.cuda.synchronize(dev)
            took = (time.perf_counter() - t0) / (reps * chunk) * 1e6
            if verbose:
                import sys
                print(f"[autotune rank {dist.get_rank(self.pg)}] {form}: {took:.1f} us per update ({reps} x {chunk}, graph={graph is not None}, "
                      f"fold fallbacks {self.fold_fallbacks})", file=sys.stderr, flush=True)
            times[form] = min(times.get(form, 1e30), took)
            del graph
            restore()
            torch.cuda.synchronize(dev)
        # ONE reduction carries everything the ranks must agree on before they choose: each form's time (the slowest rank bounds a
        # lock-step update) AND the count of peer waits that timed out while the forms were being timed — that count is per rank (a
        # late rank A makes rank B give up while A then finds B's flags in place), and ranks that decided on their own counts would
        # part: one in an RCCL all-reduce without a partner, the other in peer waits
        my_timeouts = float(self.xgmi.status()[1]) if self.xgmi is not None else 0.0
        t = torch.tensor([times[f] for f in forms] + [my_timeouts], dtype=torch.float64, device=dev if nccl else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.pg)
        *tt, timeouts = t.tolist()
        timeouts = int(timeouts)
        agreed = {f: (round(float(v), 2) if v != float("inf") else None) for f, v in zip(forms, tt)}
        usable = [f for f in forms if agreed[f] is not None] or forms[:1]
        # the peer-memory forms sum in RANK order, RCCL in ring order: the same job gives the same bits from launch to launch only
        # if warm-up noise cannot move it between the two families — `auto` therefore chooses among the rank-ordered forms and
        # keeps RCCL as the fall-back (none of them usable, or one of them lost a wait while being timed);
        # NAF_DP_EXCHANGE=fastest lets the clock decide among all of them
        ordered = [f for f in usable if f != "rccl"]
        pool = usable if (self._exchange_pick == "fastest" or not ordered) else ordered
        best = min(pool, key=lambda f: (agreed[f] if agreed[f] is not None else 0.0, forms.index(f)))
        if timeouts and best != "rccl":                      # a peer-memory form that lost a wait while being timed is not trusted
            best = "rccl"
        self._set_exchange(best)
        self.exchange_autotune = dict(agreed, chosen=best, updates_timed=updates, xgmi_timed_out_waits=int(timeouts))
        if errors:
            self.exchange_autotune["errors"] = errors
        if dist.get_rank(self.pg) == 0:
            import sys
            print("[naf] gradient exchange on this node, us per update: " +
                  ", ".join(f"{f} {agreed[f]:.1f}" if agreed[f] is not None else f"{f} unavailable ({errors.get(f, '?')})" for f in forms) +
                  f" -> {best}", file=sys.stderr, flush=True)
        return self.exchange_autotune

    # ---- parameters in / out ----------------------------------------------------------------------------
    def main_views(self) -> Dict[str, torch.Tensor]:
        return self.lay.param_views(self.theta2[0])

    def target_views(self) -> Dict[str, torch.Tensor]:
        return self.lay.param_views(self.theta2[1])

    def bn_views(self, net: int) -> Dict[str, torch.Tensor]:
        s, h = self.bn_stats[net], self.lay.H_ref
        return {"bn1.running_mean": s[0][:h], "bn1.running_var": s[1][:h], "bn2.running_mean": s[2][:h], "bn2.running_var": s[3][:h]}

    def load_params(self, net: int, sd: Dict[str, torch.Tensor]) -> None:
        self._gen += 1
        views = self.lay.param_views(self.theta2[net])
        with torch.no_grad():
            for k, v in views.items():
                v.copy_(torch.as_tensor(sd[k]).to(self.dev, torch.float32).reshape(v.shape))
            for k, v in self.bn_views(net).items():
                if k in sd:
                    v.copy_(torch.as_tensor(sd[k]).to(self.dev, torch.float32))

    def reset_optimizer(self) -> None:
        self._gen += 1
        self.adam_m.zero_()
        self.adam_v.zero_()
        self.step_dev.zero_()

    def raise_on_device_error(self) -> None:
        """Host-side check of what the kernels can only flag: a bounded wait on a PEER that expired (the one-shot all-reduce).
        Reads a pinned host word the kernel bumps — a load, never a synchronisation; the value lags the stream by whatever is
        still queued. Called before every chunk of updates and every learn(). (The waits INSIDE a launch — the records of the
        BatchNorm folds — cannot fail: a thread that waits too long folds for itself, see fold_fallbacks.)"""
        if self._xg is not None:
            self._xg.raise_on_timeout()

    @property
    def fold_fallbacks(self) -> int:
        """How many polls inside the fused launches gave up on the folded records after 20 us and folded for themselves (same
        bits either way: csrc/bn2bwd_fold.h). Zero when the process has the GPU to itself; a count that grows means the GPU is
        shared or over-subscribed. Read from pinned host memory without a synchronisation."""
        return int(self.err_host[0])

    # ---- one learn() on the current stream --------------------------------------------------------------
    def _x2(self, rows: torch.Tensor) -> torch.Tensor:
        """[2, B, S] view of a [B, ld] minibatch: net 0 reads `state`, net 1 reads `next_state`."""
        lay = self.lay
        return rows.as_strided((2, self.B, lay.S), (lay.off_s2, rows.stride(0), 1), rows.storage_offset())

    def moments(self, rows: torch.Tensor, out: torch.Tensor, n_batches: int = 1) -> None:
        """Moments records of n_batches minibatches stored back to back in `rows` ([n_batches * B, ld]) -> out
        [n_batches, 2, mom_floats]: one launch (row-split chain only)."""
        lay = self.lay
        ld = rows.stride(-2)
        check(self._f.naf_bb_moments(rows.data_ptr(), self.B * ld, lay.off_s2, ld, lay.S, ptr(out), self.B, int(n_batches), 2,
                                     stream_ptr()), "bb_moments")

    def layer1_args(self, rows: torch.Tensor, moments: torch.Tensor) -> "_lib.BbLayer1":
        """The arguments of the row-split chain's first launch (layer 1 of both networks from the minibatch's moments record) as a
        structure: naf_adam_polyak_act_layer1 runs that launch's body in extra workgroups of the per-timestep path's first launch
        (csrc/step_path.hip), and learn_rows(..., l1_done=True) then starts the chain at GEMM 2. Reads the working BatchNorm
        statistics (bn_live) as they are set when it is called."""
        lay, H, P = self.lay, self.lay.H, self.lay.P
        seg, t2p, bnp = lay.seg, self.theta2.data_ptr(), self.bn_live.data_ptr()
        return _lib.BbLayer1(rows.data_ptr(), lay.off_s2, rows.stride(0), lay.S, t2p + 4 * seg["W1"].offset, t2p + 4 * seg["b1"].offset,
                             t2p + 4 * seg["g1"].offset, t2p + 4 * seg["be1"].offset, P, ptr(moments), bnp, bnp + 4 * H, 4 * H,
                             ptr(self.A1), self.Bp * H, H, ptr(self.save_mean[0]), ptr(self.save_invstd[0]), ptr(self.bb_wc),
                             ptr(self.XH1), self.B, H, 2, BN_MOMENTUM, BN_EPS)

    def forward_train(self, rows: torch.Tensor, heads_gemm: bool = True, moments: Optional[torch.Tensor] = None,
                      adam_pending: bool = False, l1_done: bool = False) -> None:
        """Both networks' training-mode forward up to the second hidden activation A2 (and, with heads_gemm, the
        heads pre-activations Gh). Main net sees `state`, target net sees `next_state` (naf_algorithm.py:194-202);
        both use batch statistics and both update their running statistics (the reference never calls .eval() on the
        target). adam_pending: the optimizer step of the previous update was deferred (learn_rows(defer=True)) and rides
        on the first two launches here. Row-split chain: stops behind GEMM 2 — layer 2 from Z2 on is inside
        naf_bb_layer2_head (learn_rows)."""
        lay, B, st = self.lay, self.B, stream_ptr()
        seg, P, H = lay.seg, lay.P, lay.H
        t2p = self.theta2.data_ptr()
        bnp = self.bn_stats.data_ptr()
        if "bb" in self.fuse:
            bnp = self.bn_live.data_ptr()      # (the row-split chain's statistics: bn_stats itself unless a pipelined chunk says otherwise)
            ld = rows.stride(0)
            if moments is None:      # a minibatch that came without its moments (learn_rows called directly): one launch more
                self.moments(rows, self.bb_mom)
                moments = self.bb_mom
            self._mom = moments
            # layer 1: batch statistics from the moments, z, normalise, ReLU — one launch for both nets
            # (adam_pending: the previous update's clip + Adam + Polyak ride on these two launches — extra workgroups of
            # the first step everything behind the layer-1 segment while its own workgroups evaluate the layer-1
            # parameters as the step will leave them, extra workgroups of the second step the layer-1 segment)
            adam = _lib.C.byref(self._adam_args) if adam_pending else None
            if l1_done:
                # (layer 1 of this minibatch rode on the per-timestep path's first launch, naf_adam_polyak_act_layer1: layer1_args)
                if adam_pending:
                    raise ValueError("forward_train: l1_done with a pending optimizer step (that step rides on layer 1's launch)")
            else:
                check(self._f.naf_bb_layer1_adam(
                    rows.data_ptr(), lay.off_s2, ld, lay.S, t2p + 4 * seg["W1"].offset, t2p + 4 * seg["b1"].offset,
                    t2p + 4 * seg["g1"].offset, t2p + 4 * seg["be1"].offset, P, ptr(moments), bnp, bnp + 4 * H, 4 * H,
                    ptr(self.A1), self.Bp * H, H, ptr(self.save_mean[0]), ptr(self.save_invstd[0]), ptr(self.bb_wc), ptr(self.XH1), B, H,
                    2, BN_MOMENTUM, BN_EPS, adam, st), "bb_layer1")
            # GEMM 2 of both nets on f32 MFMA, bias added, statistics partials from the epilogue
            check(self._f.naf_bb_linear_stats_adam(ptr(self.A1), self.Bp * H, H, t2p + 4 * seg["W2"].offset,
                                                   t2p + 4 * seg["b2"].offset, P, ptr(self.G2), self.Bp * H, H, ptr(self.bb_st2), B, H,
                                                   H, 2, adam, st), "bb_linear_stats")
            return
        if "l1" in self.fuse:
            # layer 1 (K = state size): GEMM + bias + BN + ReLU of both nets in one launch, straight off the rows
            check(self._f.naf_linear_bn_relu_fwd_train(
                rows.data_ptr(), lay.off_s2, rows.stride(0), lay.S, t2p + 4 * seg["W1"].offset, t2p + 4 * seg["b1"].offset,
                t2p + 4 * seg["g1"].offset, t2p + 4 * seg["be1"].offset, P, bnp, bnp + 4 * H, 4 * H, ptr(self.A1), B * H, H,
                ptr(self.save_mean[0]), ptr(self.save_invstd[0]), B, H, 2, BN_MOMENTUM, BN_EPS, st), "linear_bn_relu_fwd_train")
        else:
            torch.bmm(self._x2(rows), self.W1T2, out=self.G1)
            check(self._f.naf_bn_relu_fwd_train(
                ptr(self.G1), B * H, H, t2p + 4 * seg["b1"].offset, t2p + 4 * seg["g1"].offset, t2p + 4 * seg["be1"].offset, P,
                bnp, bnp + 4 * H, 4 * H, ptr(self.A1), B * H, H, ptr(self.save_mean[0]), ptr(self.save_invstd[0]),
                B, H, 2, BN_MOMENTUM, BN_EPS, st), "bn_relu_fwd_train(1)")
        torch.bmm(self.A1, self.W2T2, out=self.G2)
        if heads_gemm and "s3" in self.fuse:
            # layer-2 BN + ReLU and, on the same tile, this workgroup's K-slice of the heads GEMM (no heads launch)
            check(self._f.naf_bn_relu_fwd_heads_partial(
                ptr(self.G2), B * H, H, t2p + 4 * seg["b2"].offset, t2p + 4 * seg["g2"].offset, t2p + 4 * seg["be2"].offset,
                P, bnp + 8 * H, bnp + 12 * H, 4 * H, ptr(self.A2), B * lay.HP, lay.HP, ptr(self.save_mean[1]),
                ptr(self.save_invstd[1]), t2p + 4 * seg["Wh"].offset, P, lay.HP, lay.NHP, lay.A + lay.T,
                ptr(self.heads_partial), self.slab_stride, ptr(self.vnext_partial), B, H, BN_MOMENTUM, BN_EPS, st),
                "bn_relu_fwd_heads_partial")
            return
        check(self._f.naf_bn_relu_fwd_train(
            ptr(self.G2), B * H, H, t2p + 4 * seg["b2"].offset, t2p + 4 * seg["g2"].offset, t2p + 4 * seg["be2"].offset, P,
            bnp + 8 * H, bnp + 12 * H, 4 * H, ptr(self.A2), B * lay.HP, lay.HP, ptr(self.save_mean[1]),
            ptr(self.save_invstd[1]), B, H, 2, BN_MOMENTUM, BN_EPS, st), "bn_relu_fwd_train(2)")
        if heads_gemm:
            torch.bmm(self.A2, self.WhT2, out=self.Gh)

    def learn_rows(self, rows: torch.Tensor, loss_partials: Optional[torch.Tensor] = None,
                   moments: Optional[torch.Tensor] = None, pending: bool = False, defer: bool = False, l1_done: bool = False) -> None:
        """Enqueue one full NAFAgent.learn() (naf_algorithm.py:180-215) + soft_update (:217-226) on the minibatch
        `rows` [B, ld] in the transition-row layout, ld = rows.stride(0) >= lay.batch_row_floats (actions already
        truncated by the gather if the reference's `.long()` is mimicked).
        loss_partials: optional [n_loss_wg] f32 receiving the per-workgroup parts of the MSE loss.
        moments: optional [2, mom_floats] record of this minibatch (row-split chain; Learner.moments); computed here when
        missing.
        defer / pending (only where self.defer_ok; a chain of updates, engine.TrainChunk): defer = leave this update's
        optimizer step (clip + Adam + Polyak) to the NEXT learn_rows call, which must then say pending = True and whose
        first two launches carry it — one launch less per update. Between the two calls the parameter buffers still hold
        the values from before this update; the chain ends with a call that does not defer.
        l1_done (row-split chain): layer 1 of this minibatch has run already — in the extra workgroups of the per-timestep path's
        first launch (layer1_args, naf_adam_polyak_act_layer1) — and the chain starts at GEMM 2."""
        self._gen += 1
        if (pending or defer) and not self.defer_ok:
            raise ValueError("learn_rows: a deferred optimizer step needs the row-split chain with the gradient norm left by the "
                             "producers or by the one-shot all-reduce (Learner.defer_ok)")
        if not pending:
            self.raise_on_device_error()
        lay, B, st = self.lay, self.B, stream_ptr()
        seg, P, H, HP, NHP = lay.seg, lay.P, lay.H, lay.HP, lay.NHP
        f = self._f
        t2p, gp = self.theta2.data_ptr(), self.grad.data_ptr()
        rp, ld = rows.data_ptr(), rows.stride(0)
        if rows.shape[0] != B or rows.stride(1) != 1 or ld < lay.batch_row_floats or ld % 4 or rp % 16:
            raise ValueError(f"learn_rows: need [B={B}, >={lay.batch_row_floats}] f32 rows, 16-B aligned, row stride % 4 == 0")
        lp = ptr(loss_partials) if loss_partials is not None else None
        if l1_done and ("bb" not in self.fuse or pending or moments is None):
            raise ValueError("learn_rows: l1_done needs the row-split chain, the minibatch's moments and no pending optimizer step")
        if "bb" in self.fuse:
            self._learn_rows_split(rows, lp, moments, pending, l1_done)
        else:
            self._learn_rows_tiles(rows, lp)
        if self.world_size > 1 or self._force_allreduce:
            # data parallel: one sum all-reduce of the flat gradient over RCCL/xGMI; the 1/W is folded into the
            # clip scale of the optimizer kernel (the clip acts on the averaged gradient)
            if self._xg is not None:
                # push + rank-ordered reduce in one launch, which also leaves the sum-of-squares partials and the step count
                # (merged: the finish launch of the row-split chain has done all of that already)
                if not (self.xgmi_merged and "bb" in self.fuse):
                    self._xg.all_reduce(self.grad, self.grad, self.partials, self.step_live, pushed_lo=self._pushed_lo,
                                         pushed_also=self._pushed_also)
                if not defer:
                    self.optimizer_step(norm_ready=True)
                return
            all_reduce_flat_grad(self.grad, self.pg)
            if defer:
                # the step rides on the next update; the sum-of-squares partials of the reduced gradient (and the step count) it
                # reads are left by this launch
                check(self._f.naf_grad_norm_partials(ptr(self.grad), P, ptr(self.partials), ptr(self.step_live), st), "grad_norm")
                return
        if defer:
            return                       # the next learn_rows(pending=True) carries the step
        self.optimizer_step(norm_ready=self.fold_norm)

    def _learn_rows_split(self, rows: torch.Tensor, lp, moments, pending: bool, l1_done: bool = False) -> None:
        """The row-split chain (csrc/big_batch.hip + gemm_bundle.hip): layer 1 | GEMM 2 | layer 2 + heads + head + first
        backward stage | backward GEMM bundle with its prologue and epilogue | finish."""
        lay, B, st = self.lay, self.B, stream_ptr()
        seg, P, H, HP, NHP = lay.seg, lay.P, lay.H, lay.HP, lay.NHP
        f = self._f
        t2p, gp, bnp = self.theta2.data_ptr(), self.grad.data_ptr(), self.bn_live.data_ptr()
        rp, ld = rows.data_ptr(), rows.stride(0)
        self._pushed_lo = self._pushed_also = None
        self.forward_train(rows, moments=moments, adam_pending=pending, l1_done=l1_done)
        # BN2 + ReLU + heads (MFMA) + NAF head + dA2 (MFMA) + ReLU mask + backward block sums: one launch
        check(f.naf_bb_layer2_head(
            ptr(self.G2), self.Bp * H, H, t2p + 4 * seg["g2"].offset, t2p + 4 * seg["be2"].offset, P, ptr(self.bb_st2),
            bnp + 8 * H, bnp + 12 * H, 4 * H, ptr(self.A2[0]), HP, ptr(self.save_mean[1]), ptr(self.save_invstd[1]),
            t2p + 4 * seg["Wh"].offset, P, HP, NHP, rp + 4 * lay.off_u, ld, rp + 4 * lay.off_r, ld, self.gamma,
            ptr(self.q_out), ptr(self.dH), lp, ptr(self.dZ2), H, ptr(self.bb_bw2), B, H, lay.A, self.p_mode, BN_MOMENTUM,
            BN_EPS, self._stats_once, st), "bb_layer2_head")
        # dWh = dH^T A2, dW2 = dZ2^T A1, dA1 = dZ2 W2: one launch of MFMA tiles; dY2 becomes dZ2 while it is staged, the
        # dA1 blocks run layer 1's backward batch pass on their tile (this minibatch's rows: z recomputed from them)
        self._epi.x, self._epi.ldx = rp, ld
        check(f.naf_gemm_bundle(self._bundle, 3, st), "gemm_bundle")
        # finish: everything added in block order, the xhat term from the moments, the bundle's split-K slabs, the norm
        # partials (nb = 0: the layer-2 bias gradient is written as the 0 it identically is). Data parallel over peer memory:
        # the workgroups that add the slabs of dW2 and dWh (91 % of the flat gradient) store them to the peers as well, so the
        # all-reduce launch behind this one sends only the layer-1 / BatchNorm segments before it raises its flags
        push = None
        merged = False
        if self._xg is not None and lay.ends_with_wh:                             # (Wh ends the buffer: no pad behind it)
            if self._push_desc is None:
                self._push_desc = self._xg.push_desc()
            push = _lib.C.byref(self._push_desc)
            self._pushed_lo = seg["Wh"].offset                                         # Wh is the last segment: [Wh, P)
            self._pushed_also = (seg["W2"].offset, seg["W2"].offset + H * H)
            merged = self.xgmi_merged
        elif self.xgmi_merged:
            raise _lib.NafHipError("merged gradient exchange: the flat layout must end with the Wh segment")
        self._launch_finish(push, merged, self._finish_form)

    @property
    def finish_small(self) -> bool:
        """Whether this learner's finish launch takes the small form when the library chooses (chain_plan.finish_small)."""
        return "bb" in self.fuse and finish_small(self._nb1, 0, (self.plan.ks_w2, self.plan.ks_wh),
                                                  push=self._xg is not None and self.lay.ends_with_wh, merge=self.xgmi_merged)

    def _launch_finish(self, push, merged: bool, form: int) -> None:
        """The row-split chain's finish launch on the learner's buffers, in the given form (learn_rows: self._finish_form)."""
        lay, B, st = self.lay, self.B, stream_ptr()
        seg, P, H = lay.seg, lay.P, lay.H
        t2p, gp = self.theta2.data_ptr(), self.grad.data_ptr()
        norm_here = self.fold_norm or merged
        args = (ptr(self.bb_dw1), lay.S, ptr(self.bb_bw1), self._nb1, None, 0,
                ptr(self._mom), ptr(self.bb_wc), t2p + 4 * seg["g1"].offset, ptr(self.save_invstd[0, 0]),
                gp + 4 * seg["W1"].offset, gp + 4 * seg["g1"].offset, gp + 4 * seg["be1"].offset, gp + 4 * seg["b1"].offset,
                gp + 4 * seg["b2"].offset, gp + 4 * seg["g2"].offset, gp + 4 * seg["be2"].offset,
                ptr(self.partials) if norm_here else None, ptr(self.step_live) if norm_here else None, B, H,
                self._bb_segs, self._bb_nsegs, ptr(self.bb_fold_flag), push, gp if push is not None else None, P if merged else 0)
        if form == _lib.FINISH_AUTO:         # (the entry every caller but a test or an A/B run uses)
            check(self._f.naf_bb_layer1_bwd_finish(*args, st), "bb_layer1_bwd_finish")
        else:
            check(self._f.naf_bb_layer1_bwd_finish_form(*args, form, st), "bb_layer1_bwd_finish_form")

    def _learn_rows_tiles(self, rows: torch.Tensor, lp) -> None:
        """The column-tile chain (csrc/fused_layers.hip) and the unfused chain (torch GEMMs + csrc/bn_relu.hip), by `fuse`."""
        lay, B, st = self.lay, self.B, stream_ptr()
        seg, P, H, HP, NHP = lay.seg, lay.P, lay.H, lay.HP, lay.NHP
        f = self._f
        t2p, gp = self.theta2.data_ptr(), self.grad.data_ptr()
        rp, ld = rows.data_ptr(), rows.stride(0)
        self._pushed_lo = self._pushed_also = None
        self.forward_train(rows)
        if "s3" in self.fuse:
            # the head adds the split-K slabs (H/8 of them) while staging its rows
            check(f.naf_head_fwd_bwd_mse_splitk(
                ptr(self.heads_partial), self.slab_stride, ptr(self.vnext_partial), self.n_slabs, NHP, rp + 4 * lay.off_u,
                ld, rp + 4 * lay.off_r, ld, self.gamma, ptr(self.q_out), ptr(self.dH), lp, B, lay.A, self.p_mode,
                st), "head_fwd_bwd_mse_splitk")
        else:
            # y = r + gamma * V'(s') ; Q ; loss ; d loss / d heads_pre — one launch
            check(f.naf_head_fwd_bwd_mse(
                ptr(self.Gh[0]), NHP, rp + 4 * lay.off_u, ld, rp + 4 * lay.off_r, ld,
                self.Gh[1].data_ptr() + 4 * (lay.A + lay.T), NHP, self.gamma, ptr(self.q_out), ptr(self.dH), lp, B, lay.A,
                self.p_mode, st), "head_fwd_bwd_mse")
        # heads GEMM backward: weight+bias gradient in one GEMM thanks to the ones column
        gb = "gb" in self.fuse
        if not gb:
            torch.mm(self.dH.t(), self.A2[0], out=self.gWh)
        if "b2" in self.fuse:
            # dA2 = dH @ Wh (K = NHP) folded into the ReLU/BN backward of layer 2
            check(f.naf_heads_bwd_bn_relu_bwd(
                ptr(self.dH), NHP, t2p + 4 * seg["Wh"].offset, HP, ptr(self.G2[0]), H, t2p + 4 * seg["b2"].offset,
                ptr(self.A2[0]), HP, t2p + 4 * seg["g2"].offset, ptr(self.save_mean[1, 0]), ptr(self.save_invstd[1, 0]),
                ptr(self.dZ2), H, gp + 4 * seg["g2"].offset, gp + 4 * seg["be2"].offset, gp + 4 * seg["b2"].offset,
                self.partials.data_ptr() + 4 * (self._gb_blocks + self._ft_blocks) if self.fold_norm else None, B, H, st),
                "heads_bwd_bn_relu_bwd")
        else:
            torch.mm(self.dH, self.Wh_main, out=self.dA2)
            check(f.naf_bn_relu_bwd(
                ptr(self.dA2), HP, ptr(self.G2[0]), H, t2p + 4 * seg["b2"].offset, ptr(self.A2[0]), HP,
                t2p + 4 * seg["g2"].offset, ptr(self.save_mean[1, 0]), ptr(self.save_invstd[1, 0]), ptr(self.dZ2), H,
                gp + 4 * seg["g2"].offset, gp + 4 * seg["be2"].offset, gp + 4 * seg["b2"].offset, B, H, st), "bn_relu_bwd(2)")
        if gb:
            # dWh = dH^T A2, dW2 = dZ2^T A1, dA1 = dZ2 W2: one launch of MFMA tiles
            check(f.naf_gemm_bundle(self._bundle, 3, st), "gemm_bundle")
        else:
            torch.mm(self.dZ2.t(), self.A1[0], out=self.gW2)
            torch.mm(self.dZ2, self.W2_main, out=self.dA1)
        if "l1" in self.fuse:
            # ReLU/BN backward of layer 1 + dW1 = dZ1^T X in one launch (dZ1 never written). Data parallel over peer
            # memory: everything but layer 1's gradient is final by now (segments W2 .. Wh of the flat buffer) and goes
            # to the peers from extra workgroups of this very launch, so its wire time runs under the kernel
            push = None
            if self._xg is not None:
                if self._push_desc is None:
                    self._push_desc = self._xg.push_desc()
                push, self._pushed_lo = _lib.C.byref(self._push_desc), seg["W2"].offset
            check(f.naf_bn_relu_bwd_wgrad_push(
                ptr(self.dA1), H, rp, ld, lay.S, t2p + 4 * seg["W1"].offset, t2p + 4 * seg["b1"].offset,
                ptr(self.A1[0]), H, t2p + 4 * seg["g1"].offset, ptr(self.save_mean[0, 0]), ptr(self.save_invstd[0, 0]),
                gp + 4 * seg["g1"].offset, gp + 4 * seg["be1"].offset, gp + 4 * seg["b1"].offset, gp + 4 * seg["W1"].offset,
                self.partials.data_ptr() + 4 * self._gb_blocks if self.fold_norm else None,
                ptr(self.step_dev) if self.fold_norm else None, B, H, push, gp if push is not None else None,
                self._pushed_lo or 0, P if push is not None else 0, st), "bn_relu_bwd_wgrad")
        else:
            check(f.naf_bn_relu_bwd(
                ptr(self.dA1), H, ptr(self.G1[0]), H, t2p + 4 * seg["b1"].offset, ptr(self.A1[0]), H,
                t2p + 4 * seg["g1"].offset, ptr(self.save_mean[0, 0]), ptr(self.save_invstd[0, 0]), ptr(self.dZ1), H,
                gp + 4 * seg["g1"].offset, gp + 4 * seg["be1"].offset, gp + 4 * seg["b1"].offset, B, H, st), "bn_relu_bwd(1)")
            torch.mm(self.dZ1.t(), self._x2(rows)[0], out=self.gW1)

    def optimizer_step(self, norm_ready: Optional[bool] = None) -> None:
        """clip_grad_norm_(params, 1) + Adam.step() + soft_update on the flat buffers: 2 launches (1 when the
        producers of the gradient already left its sum-of-squares partials)."""
        self._gen += 1
        st, P = stream_ptr(), self.lay.P
        f = self._f
        if norm_ready is None:
            norm_ready = self.fold_norm
        if not norm_ready:
            check(f.naf_grad_norm_partials(ptr(self.grad), P, ptr(self.partials), ptr(self.step_dev), st), "grad_norm")
        check(f.naf_adam_polyak_fused(
            ptr(self.theta2[0]), ptr(self.grad), ptr(self.adam_m), ptr(self.adam_v), ptr(self.theta2[1]),
            ptr(self.partials), self.n_partials if norm_ready else self.n_partials_norm, MAX_GRAD_NORM, self.lr,
            ADAM_BETA1, ADAM_BETA2, ADAM_EPS, self.tau, float(1.0 - self.tau), ptr(self.step_dev), 1.0 / self.world_size, P, st), "adam_polyak")

    def soft_update(self) -> None:
        """Standalone NAFAgent.soft_update(main, target) (naf_algorithm.py:217-226) over the flat buffers."""
        self._gen += 1
        check(self._f.naf_polyak_update(ptr(self.theta2[1]), ptr(self.theta2[0]), self.tau, float(1.0 - self.tau),
                                        self.lay.P, stream_ptr()), "polyak")


class ActPath:
    """Eval-mode policy forward for E states at once (NAFAgent.act, naf_algorithm.py:158-178): running-stat BN
    (main net only), mu = tanh, exploration noise clamp(mu + P^-1/2 z) — noise is drawn on EVERY call exactly as
    the reference's forward does (naf_neural_network.py:119-121), unless noise_scale = 0."""

    def __init__(self, learner: Learner, n_states: int, seed: int, host_io: bool = False):
        """host_io: `obs` and `actions` live in pinned HOST memory that the one-launch kernel reads and writes directly
        (84 B in, 24 B out per state): the per-call H2D / D2H copies of NAFAgent.act() disappear, the caller fills
        `obs_np`, enqueues act(), synchronises the stream and reads `actions_np`. Only with the fused kernel."""
        self.L = learner
        lay, dev = learner.lay, learner.dev
        self.E = int(n_states)
        f32 = dict(dtype=torch.float32, device=dev)
        E, H, HP, NHP = self.E, lay.H, lay.HP, lay.NHP
        self.obs = torch.zeros(E, lay.S, **f32)
        self.G1 = torch.empty(E, H, **f32)
        self.A1 = torch.empty(E, H, **f32)
        self.G2 = torch.empty(E, H, **f32)
        self.A2 = torch.zeros(E, HP, **f32)
        self.A2[:, H] = 1.0
        self.Gh = torch.empty(E, NHP, **f32)
        self.actions = torch.zeros(E, lay.A, **f32)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)   # noise stream position (uint64 on device)
        # one launch for the whole act() (csrc/policy_act.hip) where the plan says the shape takes it (chain_plan.py: act_fused);
        # other shapes take the seven-launch path (3 GEMMs, 2 BN kernels, noise, counter)
        self.fused = learner.plan.act_fused
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.host_io = bool(host_io) and self.fused
        if self.host_io:
            self.obs = torch.zeros(E, lay.S, dtype=torch.float32).pin_memory()
            self.actions = torch.zeros(E, lay.A, dtype=torch.float32).pin_memory()
            self.obs_np, self.actions_np = self.obs.numpy(), self.actions.numpy()
        self.W1T = learner.W1T2[0]
        self.W2T = learner.W2T2[0]
        self.WhT = learner.WhT2[0]
        # ONE state on the row-split chain: the optimizer step of the update in front can take this act() along
        # (naf_adam_polyak_act, csrc/step_path.hip: the workgroups that step the weights multiply them with the policy's
        # activations) — NAFAgent.step's graph then ends with one launch instead of two. `seq` (pinned host): the launch's ordinal,
        # written behind the action: a host that polls it reads the action without synchronising the stream.
        seg = lay.seg
        self.can_ride = (self.fused and E == 1 and learner.defer_ok and lay.NHP <= 80 and
                         [seg[k].offset for k in ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "Wh")] ==
                         [0, H * lay.S, H * lay.S + H, H * lay.S + 2 * H, H * lay.S + 3 * H, H * lay.S + 3 * H + H * H,
                          H * lay.S + 4 * H + H * H, H * lay.S + 5 * H + H * H, H * lay.S + 6 * H + H * H] and
                         lay.P == H * lay.S + 6 * H + H * H + lay.NHP * lay.HP)
        self.sync = self.seq = self.seq_np = self.ordinal_np = None
        if self.can_ride:
            self.sync = torch.zeros(learner.lib.naf_adam_polyak_act_sync_ints(), dtype=torch.int32, device=dev)
            self.seq = torch.zeros(2, dtype=torch.int32).pin_memory()
            self.seq_np = self.seq.numpy()
            # the action as the launch hands it to a host that does not synchronise the stream: three (9 .. 11 joints: four) 16-byte
            # chunks {a[3j], a[3j + 1], a[3j + 2], ordinal}, one store each (naf_adam_polyak_act: action_rec); `ordinal_np` = chunk 0's
            self.act_rec = torch.zeros(16, dtype=torch.int32).pin_memory()
            self.rec_np = self.act_rec.numpy()
            self.rec_f = self.rec_np.view(np.float32)
            self.ordinal_np = self.rec_np[3:4]
            self._rec_words = [w for w in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13)][:lay.A]
            self._rec_ords = [4 * j + 3 for j in range((lay.A + 2) // 3)]
            bnp = learner.bn_stats.data_ptr()
            self._net = _lib.ActNet(lay.S, lay.A, H, lay.NHP, lay.HP, *[seg[k].offset for k in
                                    ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "Wh")],
                                    bnp, bnp + 4 * H, bnp + 8 * H, bnp + 12 * H, BN_EPS)

    def act_with_optimizer_step(self, noise_scale: float = 1.0, obs_ptr: Optional[int] = None, prefetch=None,
                                obs_system_scope: bool = False, adam_args=None, net=None, layer1=None) -> torch.Tensor:
        """The pending optimizer step of the learner (a learn_rows(defer=True) in front) and act() on the parameters it leaves, in
        one launch. Same parameters as Learner.optimizer_step() and the same action as act() behind it, bit for bit.
        obs_ptr: where the observation lies instead of self.obs (device-visible, S floats). prefetch: a _lib.StepPrefetch — one
        more workgroup of the launch draws the NEXT timestep's minibatch (engine.TrainChunk). obs_system_scope: the observation
        lies in device memory the host stores into. adam_args / net: the structures to pass instead of the learner's / this path's
        own (the pipelined chunk's: optimizer step count and BatchNorm statistics of its working state). layer1: a _lib.BbLayer1
        (Learner.layer1_args) — layer 1 of the NEXT update's chain rides on the launch (naf_adam_polyak_act_layer1); the caller then
        runs that chain with learn_rows(..., l1_done=True)."""
        L = self.L
        if layer1 is not None:
            check(L.lib.naf_adam_polyak_act_layer1(
                _lib.C.byref(adam_args if adam_args is not None else L._adam_args), _lib.C.byref(net if net is not None else self._net),
                obs_ptr or ptr(self.obs), ptr(self.Gh), ptr(self.actions), self.seed, ptr(self.counter), float(noise_scale), L.p_mode,
                # (no `host_seq` word here: the pipelined timestep's host takes the action from the self-validating chunks of act_rec
                #  alone, and the launch's last workgroup would wait a microsecond for the action's stores to cross PCIe before it
                #  stores that word — at the very end of the kernel the chain is queued behind)
                ptr(self.sync), L.err_host.data_ptr() + 8, None, ptr(self.act_rec),
                _lib.C.byref(prefetch) if prefetch is not None else None, int(bool(obs_system_scope)), _lib.C.byref(layer1),
                stream_ptr()), "adam_polyak_act_layer1")
            return self.actions
        check(L.lib.naf_adam_polyak_act(_lib.C.byref(adam_args if adam_args is not None else L._adam_args),
                                        _lib.C.byref(net if net is not None else self._net), obs_ptr or ptr(self.obs), ptr(self.Gh),
                                        ptr(self.actions), self.seed, ptr(self.counter), float(noise_scale), L.p_mode,
                                        ptr(self.sync), L.err_host.data_ptr() + 8, ptr(self.seq), ptr(self.act_rec),
                                        _lib.C.byref(prefetch) if prefetch is not None else None, int(bool(obs_system_scope)),
                                        stream_ptr()), "adam_polyak_act")
        return self.actions

    @property
    def act_timeouts(self) -> int:
        """Polls inside naf_adam_polyak_act whose 2-ms bound ran out (pinned host word; 0 on a healthy GPU): the action of such a
        launch is NaN."""
        return int(self.L.err_host[1])

    def heads(self) -> None:
        L, lay, E, st = self.L, self.L.lay, self.E, stream_ptr()
        seg, H = lay.seg, lay.H
        t2p, bnp = L.theta2.data_ptr(), L.bn_stats.data_ptr()
        f = L.lib
        torch.mm(self.obs, self.W1T, out=self.G1)
        check(f.naf_bn_relu_fwd_eval(ptr(self.G1), H, t2p + 4 * seg["b1"].offset, t2p + 4 * seg["g1"].offset,
                                     t2p + 4 * seg["be1"].offset, bnp, bnp + 4 * H, ptr(self.A1), H, E, H, BN_EPS, st),
              "bn_relu_fwd_eval(1)")
        torch.mm(self.A1, self.W2T, out=self.G2)
        check(f.naf_bn_relu_fwd_eval(ptr(self.G2), H, t2p + 4 * seg["b2"].offset, t2p + 4 * seg["g2"].offset,
                                     t2p + 4 * seg["be2"].offset, bnp + 8 * H, bnp + 12 * H, ptr(self.A2), lay.HP, E, H,
                                     BN_EPS, st), "bn_relu_fwd_eval(2)")
        torch.mm(self.A2, self.WhT, out=self.Gh)

    def act(self, noise_scale: float = 1.0) -> torch.Tensor:
        """obs (already in self.obs) -> self.actions; advances the noise counter on the device."""
        L, lay, st = self.L, self.L.lay, stream_ptr()
        if self.fused:
            seg, H = lay.seg, lay.H
            t2p, bnp = L.theta2.data_ptr(), L.bn_stats.data_ptr()
            off = lambda name: t2p + 4 * seg[name].offset          # noqa: E731
            check(L.lib.naf_policy_act(
                ptr(self.obs), lay.S, lay.S, off("W1"), off("b1"), off("g1"), off("be1"), off("W2"), off("b2"), off("g2"),
                off("be2"), off("Wh"), lay.HP, lay.NH, bnp, bnp + 4 * H, bnp + 8 * H, bnp + 12 * H, BN_EPS, H, ptr(self.Gh),
                lay.NHP, ptr(self.actions), self.seed, ptr(self.counter), ptr(self._ticket), float(noise_scale), self.E,
                lay.A, L.p_mode, st), "policy_act")
            return self.actions
        self.heads()
        check(L.lib.naf_act_noise(ptr(self.Gh), lay.NHP, ptr(self.actions), self.seed, ptr(self.counter), 0,
                                  float(noise_scale), self.E, lay.A, L.p_mode, st), "act_noise")
        check(L.lib.naf_counter_add(ptr(self.counter), 1, st), "counter_add")
        return self.actions

    def act_env_append(self, noise_scale: float, env: "_lib.VecEnv") -> torch.Tensor:
        """act(), the stand-in envs' step on the actions, the step counter and the append of the rows, in ONE launch
        (naf_vec_act_env_append, csrc/vector_step.hip): the same bits in every word as the four launches. Only with the fused
        kernel (engine.DeviceEnvLoop decides)."""
        L, lay, st = self.L, self.L.lay, stream_ptr()
        seg, H = lay.seg, lay.H
        t2p, bnp = L.theta2.data_ptr(), L.bn_stats.data_ptr()
        off = lambda name: t2p + 4 * seg[name].offset          # noqa: E731
        check(L.lib.naf_vec_act_env_append(
            ptr(self.obs), lay.S, off("W1"), off("b1"), off("g1"), off("be1"), off("W2"), off("b2"), off("g2"), off("be2"),
            off("Wh"), lay.HP, lay.NH, bnp, bnp + 4 * H, bnp + 8 * H, bnp + 12 * H, BN_EPS, H, ptr(self.Gh), lay.NHP,
            ptr(self.actions), self.seed, ptr(self.counter), ptr(self._ticket), float(noise_scale), self.E, lay.A, L.p_mode,
            _lib.C.byref(env), st), "vec_act_env_append")
        return self.actions

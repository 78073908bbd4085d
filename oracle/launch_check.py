"""
oracle/launch_check.py — TEST INFRASTRUCTURE ONLY. The five launches of the row-split learn() chain (csrc/big_batch.hip, the
prologue and epilogue of csrc/gemm_bundle.hip, the finish launch; contracts in include/naf_hip.h), each checked against float64
computed from THE DEVICE VALUES THAT LAUNCH READ: after one Learner.learn_rows() every intermediate of every launch is still in
the learner's buffers, and the parameters and statistics the launches read are the ones read back before the call. No error
propagates from launch to launch and no ReLU element has to be guessed across launches.

check_launches() is the whole comparison. tests/test_rowsplit_launches_gpu.py feeds it the HIP learner's buffers,
tests/test_rowsplit_launches_cpu.py feeds it f32_standin() — a float32 numpy chain built from oracle/naf_oracle.py's functions
that fills the same dictionary — to show that every bound admits honest float32 arithmetic and rejects the planted DEFECTS. The
two share this file and tests/rowsplit_cases.py so that they cannot drift apart.

The other two chains — column-tile and unfused — are held the same way by check_tile_launches() and f32_standin_tiles() in the
second half of this file (their dictionary, their n and c and their defects are stated there; tests/tilechain_cases.py,
tests/test_tilechain_launches_{cpu,gpu}.py). The rules (1) - (3) below and the constants of (2) serve both.

Everything is in the STORED layout (layout.NetLayout): H is the stored width (a layer of 128 | 320 is stored zero-padded to
256 | 512), h the reference's; the three heads are one matrix Wh [NHP][HP] whose column H is the bias.

    pre    {"net": [main, target] each {"W1","b1","g1","be1","W2","b2","g2","be2","Wh"}, "bn": [2][rm1, rv1, rm2, rv2][H],
            "step": int, "flag": int}                                       what the launches read
    batch  (states, actions (truncated), rewards, next_states)              the minibatch rows
    dev    what the update left, by the Learner's buffer: A1 [2][Bp][H], XH1 [Bp][H] | None, save_mean / save_invstd
           [layer][net][H], bn, mom [2][kp + kp kp], wc [H][kp], G2 [2][Bp][H], st2 [2][nb][H][2], A2 [Bp][HP] (main), q [B],
           loss (the summed loss partials), dH [Bp][NHP], dY2 [Bp][H] (the dZ2 buffer: launch 4 forms dZ2 in registers only),
           bw2 [Bp / hk_rows][H][2], bw1 [nb1][H][2], dw1 [nb1][H][kp], slab_w2 [ks_w2][H][H], slab_wh [ks_wh][NHP][HP],
           grad {as pre["net"][0]}, sumsq (the summed norm partials), step, flag

THE BOUNDS. None is tuned on a device. U = 2^-24, the unit roundoff of float32.

(1) Dot products. A float32 sum of n products, in any order, with c further roundings per term, lies within
    (n + c) U sum_i |a_i| |b_i| of the exact one (first order). Per output, n and c:
      wc          n = S           c = 2    row c of W1 C, C from the launch's own moments record
      G2          n = H           c = 2    the bias add and the store
      st2 sum     n = rows of the 64-row block            c = 2
      st2 M2      (n + 4) U M2 + 2 (n + 2) U sum|g - m| mean|g|: each squared deviation rounds thrice and carries the block mean's
                  own error (n + 2) U mean|g| times 2 |g - m|; n = rows of the block
      dY2         n = NHP         c = 2    dH Wh; an element the mask removes is exactly 0
      bw2         n = hk_rows     c = 2 (sum dy) | 4 (sum dy xhat: xhat = (z - mean) invstd rounds twice, the product once more)
      g2, be2     n = Bp / hk_rows blocks   c = 1
      dZ2 (never in memory; the scale of one element's error, for the three products that read it):
                  M_dz = |k1| (|dy| + sum|block sum dy| / B + |xhat| sum|block sum dy xhat| / B), c_dz = Bp / hk_rows + 10 roundings —
                  the two folds of the block sums, k1 = gamma invstd, the divisions by B, k1 c1, invstd k1 c2, z - mean, two products,
                  two subtractions
      slab_w2     n = Bp / ks_w2  c = c_dz      scale M_dz^T |A1|
      slab_wh     n = Bp / ks_wh  c = 2         scale |dH|^T |A2|
      bw1 sum dy  n = H + 32      c = c_dz      scale sum over the block's unmasked rows of M_dA1 = M_dz |W2|
      bw1 sum dy xhat   the same with c = c_dz + 4 and |xhat|; where XH1 is not kept the epilogue recomputes xhat from the
                  minibatch rows: + sum |dy| (S + 4) U invstd (|x| |W1|^T + |b1| + |mean|)
      dw1         n = H + 32      c = c_dz + 1  scale (M_dA1 masked)^T |x|
      finish W1   n = nb1         c = 10        scale |g1 invstd| (sum|P blocks| + sum|dy blocks| |Sx| / B + sum|dy xhat blocks| |invstd wc| / B)
      finish g1, be1    n = nb1   c = 1
(2) Behind a division, a square root, tanh or exp: the tolerance the suite already applies to the same quantity, unchanged.
      test_bn_relu_train_fwd_bwd_vs_oracle (tests/test_kernels_gpu.py):
          normalised activations (A1, XH1, A2)  rtol = atol = 5e-5        save_mean      rtol 1e-5, atol 1e-5
          save_invstd   rtol 1e-4               running_mean  rtol 1e-5, atol 1e-6       running_var  rtol 1e-4, atol 1e-6
      test_head_both_modes_vs_oracle_f64 (tests/test_kernels_gpu.py):
          q  rtol 3e-5, atol 3e-5      d_mu, d_l  rtol 3e-4, atol 1e-6 x 10 max|dq| + 1e-7      d_V  rtol 1e-5, atol 1e-8
          loss  rtol 1e-4
      That test hands its kernel the heads' pre-activations and V'(s') exactly. Launch 3 forms them itself — H-term float32 dot
      products of normalised activations — so its d_V = 2 (Q - r - gamma V') / B carries the rounding of Q and V' where Q - y
      cancels: against 2 (Q64 - y64) / B the float32 stand-in reaches 1.39 x the head test's d_V tolerance (s21_a6_h512_b64_m1;
      0.97 x at s31_a11_h256_b48), so that comparison would reject honest float32. Teacher-forced like everything else here, the
      d_V column is compared with 2 (q_dev - y64) / B — on the launch's own q_out, which the q check pins — at the head test's
      tolerance plus what V' brings in: (2 / B) gamma times the dot-product bound of V' (n = H, c = 8: the normalisation's four
      roundings, the statistics', the bias, the store). d_mu and d_l are compared with head_backward at the launch's own dq (its
      d_V column) at the head test's tolerance as it is.
      The folded norm partials: rtol 1e-5 on sum(partials) against ||grad||^2, the suite's tolerance for folded norm partials
      (learn_check.NORM_SELF_RTOL).
(3) Anything left — check (b) of the finish launch, launches 4 and 5 together against the direct BatchNorm backward dz1^T X,
    per block in norm: 8 x the largest error of f32_standin() against the same float64 reference over the table of
    tests/rowsplit_cases.py (the project's margin for "another legal float32 evaluation", chain_ik_common.STEP_BOUND).
    Measured on the CPU, never against the kernel (tests/test_rowsplit_launches_cpu.py recomputes it and fails if the table has
    outgrown it): see MEASURED_FINISH_B below.
ReLU kinks (launch 4's epilogue, check (b)): the reference mask is A1_dev > 0. An element whose float64 pre-activation lies
within naf_oracle.relu_kink_tau of 0 may go either way in an epilogue that recomputes it; those elements are counted
(meta["ambiguous"]; the tests bound the count) and a block sum gets the slack of exactly its ambiguous elements.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import naf_oracle as O
from .learn_check import BIAS0_REL, NORM_SELF_RTOL, SUM_ABS_RTOL, Report

U = 2.0 ** -24
BN_MOMENTUM = O.BN_MOMENTUM

# (2) — test_bn_relu_train_fwd_bwd_vs_oracle
ACT_TOL = 5e-5
MEAN_RTOL, MEAN_ATOL = 1e-5, 1e-5
INVSTD_RTOL = 1e-4
RM_RTOL, RM_ATOL = 1e-5, 1e-6
RV_RTOL, RV_ATOL = 1e-4, 1e-6
# (2) — test_head_both_modes_vs_oracle_f64
Q_RTOL, Q_ATOL = 3e-5, 3e-5
DHEAD_RTOL, DHEAD_ATOL_SCALE, DHEAD_ATOL = 3e-4, 1e-6 * 10, 1e-7
DV_RTOL, DV_ATOL = 1e-5, 1e-8
LOSS_RTOL = 1e-4
# (3) — largest ||f32_standin - float64|| / ||float64|| of d_W1 | d_g1 | d_be1 in check (b) over tests/rowsplit_cases.py:
# W1 5.01e-7 (s21_a6_h256_b2100_rare), g1 5.25e-7, be1 5.47e-7 (both s21_a6_h256_b1040_rare)  ->  5.5e-7, rounded up
MEASURED_FINISH_B = 5.5e-7
FINISH_B_RTOL = 8 * MEASURED_FINISH_B

PARAMS = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "Wh")
DEFECTS = ("target_bn2_from_main", "target_w2_from_main", "mask_no_beta1", "k1_no_gamma", "biased_running_var",
           "momentum_on_old", "target_stats_in_main_slots", "batch_mean_partials", "dw1_no_invstd", "slabs_reversed")
ADMITTED_AT_INIT = DEFECTS[:3]        # move nothing where the target equals the main network and beta = 0


@dataclass(frozen=True)
class Dims:
    S: int
    A: int
    H: int
    h: int
    B: int
    Bp: int
    HP: int
    NHP: int
    kp: int
    nb: int
    nb1: int
    hk_rows: int
    ks_w2: int
    ks_wh: int
    keep_xhat1: bool
    p_mode: int
    gamma: float = 0.99
    fuse: frozenset = frozenset()       # the column-tile / unfused chains (check_tile_launches): the plan's tags,
    n_slabs: int | None = None          # the slab count of the split-K heads (s3)
    fold_norm: bool = False             # and whether the gradient's producers leave the norm partials

    @property
    def T(self):
        return self.A * (self.A + 1) // 2

    @classmethod
    def of(cls, plan, lay, B, p_mode, gamma=0.99):
        """From a chain_plan.ChainPlan and its layout.NetLayout."""
        return cls(lay.S, lay.A, lay.H, lay.H_ref, int(B), plan.Bp, lay.HP, lay.NHP, plan.kp, plan.nb, plan.nb1, plan.hk_rows,
                   plan.ks_w2, plan.ks_wh, bool(plan.keep_xhat1), int(p_mode), float(gamma), frozenset(plan.fuse), plan.n_slabs,
                   bool(plan.fold_norm))


def stored_state(main: dict, target: dict, d: Dims) -> dict:
    """`pre` of two state dicts in the reference's layout, as Learner.load_params stores them in a fresh learner."""
    A, T, H, h = d.A, d.T, d.H, d.h
    nets = []
    bn = np.zeros((2, 4, H), np.float32)
    bn[:, 1], bn[:, 3] = 1.0, 1.0
    for n, sd in enumerate((main, target)):
        p = {"W1": np.zeros((H, d.S), np.float32), "W2": np.zeros((H, H), np.float32), "Wh": np.zeros((d.NHP, d.HP), np.float32)}
        p["W1"][:h] = sd["input_layer.weight"]
        p["W2"][:h, :h] = sd["hidden_layer.weight"]
        for k, src in (("b1", "input_layer.bias"), ("g1", "bn1.weight"), ("be1", "bn1.bias"), ("b2", "hidden_layer.bias"),
                       ("g2", "bn2.weight"), ("be2", "bn2.bias")):
            p[k] = np.zeros(H, np.float32)
            p[k][:h] = sd[src]
        for r0, r1, name in ((0, A, "action_values"), (A, A + T, "matrix_entries"), (A + T, A + T + 1, "value")):
            p["Wh"][r0:r1, :h] = sd[f"{name}.weight"]
            p["Wh"][r0:r1, H] = sd[f"{name}.bias"]
        nets.append(p)
        for i, k in enumerate(("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")):
            bn[n, i, :h] = sd[k]
    return {"net": nets, "bn": bn, "step": 0, "flag": 1}


def _f64(a):
    return np.asarray(a, np.float64)


def _blocks(n_rows, rows, B):
    """[(first row, end row clipped to B)] of the blocks of `rows` rows that cover n_rows buffer rows"""
    return [(r0, max(r0, min(B, r0 + rows))) for r0 in range(0, n_rows, rows)]


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def slab_sum_f32(slabs):
    """the float32 sum of split-K slabs in slab order, as the finish launch adds them"""
    acc = np.array(slabs[0], np.float32)
    for s in range(1, len(slabs)):
        acc = (acc + np.asarray(slabs[s], np.float32)).astype(np.float32)
    return acc


def _check_stats(rep, check, smean, sinv, bn1, layer, net, cache, rm, rv):
    """(2): what one BatchNorm launch saved and left in ITS slots — layer `layer` (0 | 1) of network `net` — against float64."""
    rep.add(f"{check}.mean", np.abs(smean[layer, net] - cache["mean"]), MEAN_RTOL * np.abs(cache["mean"]) + MEAN_ATOL,
            f"save_mean layer {layer + 1} net {net}")
    rep.add(f"{check}.invstd", np.abs(sinv[layer, net] - cache["invstd"]), INVSTD_RTOL * cache["invstd"],
            f"save_invstd layer {layer + 1} net {net}")
    rep.add(f"{check}.rm", np.abs(bn1[net, 2 * layer] - rm), RM_RTOL * np.abs(rm) + RM_ATOL, f"bn{layer + 1} running_mean net {net}")
    rep.add(f"{check}.rv", np.abs(bn1[net, 2 * layer + 1] - rv), RV_RTOL * np.abs(rv) + RV_ATOL, f"bn{layer + 1} running_var net {net}")


def _check_head(rep, pfx, d, mu_pre, l_pre, V, vn, vn_tol, ac, rw, q_dev, loss_dev, dH):
    """(2): the NAF head of one launch — q, the loss and d_heads [Bp][NHP] — against float64 from the heads' pre-activations and the
    target's V'(s') (float64 arrays); vn_tol: what V' carries of its own rounding. The d_V column is teacher-forced on the
    launch's own q_out (the header says why)."""
    A, T, B = d.A, d.T, d.B
    u, r = _f64(ac), _f64(rw).reshape(-1)
    Q = O.head_forward(mu_pre, l_pre, V, u, d.p_mode)["Q"]
    y = r + d.gamma * vn
    q = _f64(q_dev).reshape(-1)[:B]
    rep.add(f"{pfx}.q", np.abs(q - Q), Q_RTOL * np.abs(Q) + Q_ATOL, "q_out")
    loss64 = float(((Q - y) ** 2).mean())
    rep.add(f"{pfx}.loss", abs(float(loss_dev) - loss64), LOSS_RTOL * abs(loss64), "summed loss partials")
    dq_dev = dH[:B, A + T]
    dq_ref = 2.0 * (q - y) / B
    rep.add(f"{pfx}.dv", np.abs(dq_dev - dq_ref), DV_RTOL * np.abs(dq_ref) + DV_ATOL + (2.0 / B) * d.gamma * vn_tol, "d_heads, V column")
    d_mu, d_l, _ = O.head_backward(mu_pre, l_pre, u, dq_dev, d.p_mode)
    atol = DHEAD_ATOL_SCALE * np.abs(dq_dev).max() + DHEAD_ATOL
    rep.add(f"{pfx}.dmu", np.abs(dH[:B, :A] - d_mu), DHEAD_RTOL * np.abs(d_mu) + atol, "d_heads, mu columns")
    rep.add(f"{pfx}.dl", np.abs(dH[:B, A:A + T] - d_l), DHEAD_RTOL * np.abs(d_l) + atol, "d_heads, L columns")
    rep.add(f"{pfx}.pad", 0.0 if (not dH[B:].any() and not dH[:, A + T + 1:].any()) else 1.0, 0.5,
            "d_heads rows past the batch and pad columns")


# ------------------------------------------------------------------------------------------------------------------------
def check_launches(pre: dict, batch, dev: dict, d: Dims) -> Report:
    """Every launch of one update of the row-split chain against float64 from the values it read. Returns a learn_check.Report:
    .failures is empty when every check holds, .ratios has the largest error / tolerance per check, .meta["ambiguous"] the
    number of layer-1 ReLU elements within rounding of 0, .meta["finish_b"] the relative errors of check (b)."""
    rep = Report()
    S, A, T, H, h, B, Bp, HP, NHP, kp = d.S, d.A, d.T, d.H, d.h, d.B, d.Bp, d.HP, d.NHP, d.kp
    st, ac, rw, ns = batch
    x = [_f64(st), _f64(ns)]
    P = [{k: _f64(v) for k, v in pre["net"][n].items()} for n in (0, 1)]
    bn0, bn1 = _f64(pre["bn"]), _f64(dev["bn"])
    A1, G2, A2, dH, dY2 = _f64(dev["A1"]), _f64(dev["G2"]), _f64(dev["A2"]), _f64(dev["dH"]), _f64(dev["dY2"])
    smean, sinv = _f64(dev["save_mean"]), _f64(dev["save_invstd"])
    kept = dev.get("XH1") is not None
    assert kept == d.keep_xhat1, "XH1 is kept exactly where the plan says so"

    def exact(check, cond, what):
        rep.add(check, 0.0 if bool(cond) else 1.0, 0.5, what)

    def stats(check, layer, net, cache, rm, rv):
        _check_stats(rep, check, smean, sinv, bn1, layer, net, cache, rm, rv)

    # ---- launch 1: naf_bb_layer1_adam ---------------------------------------------------------------------------------
    c1 = []
    y1 = []
    for net in (0, 1):
        p = P[net]
        z = x[net] @ p["W1"].T + p["b1"]
        y, cache, rm, rv = O.bn_train_forward(z, p["g1"], p["be1"], bn0[net, 0], bn0[net, 1])
        ref = np.maximum(y, 0)
        rep.add("l1.a1", np.abs(A1[net, :B] - ref), ACT_TOL * ref + ACT_TOL, f"A1 net {net}")
        stats("l1", 0, net, cache, rm, rv)
        c1.append(cache)
        y1.append(y)
    exact("l1.pad_rows", not A1[:, B:].any(), "A1 rows past the batch")
    mom = _f64(dev["mom"])
    Cm = mom[0, kp:].reshape(kp, kp)[:S, :S]
    rep.add("l1.wc", np.abs(_f64(dev["wc"])[:, :S] - P[0]["W1"] @ Cm), (S + 2) * U * (np.abs(P[0]["W1"]) @ np.abs(Cm)), "bb_wc")
    if kept:
        XH1 = _f64(dev["XH1"])
        rep.add("l1.xh1", np.abs(XH1[:B] - c1[0]["xhat"]), ACT_TOL * np.abs(c1[0]["xhat"]) + ACT_TOL, "XH1")
        exact("l1.pad_rows", not XH1[B:].any(), "XH1 rows past the batch")

    # ---- launch 2: naf_bb_linear_stats_adam -----------------------------------------------------------------------------
    st2 = _f64(dev["st2"])
    for net in (0, 1):
        p = P[net]
        a = A1[net, :B]
        rep.add("l2.g2", np.abs(G2[net, :B] - (a @ p["W2"].T + p["b2"])), (H + 2) * U * (np.abs(a) @ np.abs(p["W2"]).T + np.abs(p["b2"])),
                f"G2 net {net}")
        for blk, (r0, r1) in enumerate(_blocks(64 * d.nb, 64, B)):
            g, n = G2[net, r0:r1], r1 - r0
            s, ga = g.sum(0), np.abs(g).sum(0)
            dl = g - s / n
            m2 = (dl * dl).sum(0)
            rep.add("l2.sum", np.abs(st2[net, blk, :, 0] - s), (n + 2) * U * ga, f"bb_st2 sum net {net} block {blk}")
            rep.add("l2.m2", np.abs(st2[net, blk, :, 1] - m2), (n + 4) * U * m2 + 2 * (n + 2) * U * np.abs(dl).sum(0) * ga / n,
                    f"bb_st2 M2 net {net} block {blk}")
    exact("l2.pad_rows", not G2[:, B:].any(), "G2 rows past the batch")

    # ---- launch 3: naf_bb_layer2_head, from G2_dev ------------------------------------------------------------------------
    c2, y2 = [], []
    for net in (0, 1):
        p = P[net]
        y, cache, rm, rv = O.bn_train_forward(G2[net, :B], p["g2"], p["be2"], bn0[net, 2], bn0[net, 3])
        stats("l3", 1, net, cache, rm, rv)
        c2.append(cache)
        y2.append(y)
    ref = np.maximum(y2[0], 0)
    rep.add("l3.a2", np.abs(A2[:B, :H] - ref), ACT_TOL * ref + ACT_TOL, "A2")
    exact("l3.a2_ones", (A2[:, H] == 1).all() and not A2[:, H + 1:].any(), "A2's constant-1 column and the zeros behind it")
    Whm, Wht = P[0]["Wh"], P[1]["Wh"]
    heads = A2[:B, :H] @ Whm[:, :H].T + Whm[:, H]
    mu_pre, l_pre, V = heads[:, :A], heads[:, A:A + T], heads[:, A + T]
    a2t = np.maximum(y2[1], 0)
    vn = a2t @ Wht[A + T, :H] + Wht[A + T, H]
    vn_tol = (H + 8) * U * (a2t @ np.abs(Wht[A + T, :H]) + abs(Wht[A + T, H]))
    _check_head(rep, "l3", d, mu_pre, l_pre, V, vn, vn_tol, ac, rw, dev["q"], dev["loss"], dH)
    on2 = A2[:B, :H] > 0
    rep.add("l3.dy2", np.abs(dY2[:B] - (dH[:B] @ Whm[:, :H]) * on2), (NHP + 2) * U * (np.abs(dH[:B]) @ np.abs(Whm[:, :H])) * on2, "dY2")
    exact("l3.pad", not dY2[B:].any(), "dY2 rows past the batch")
    xh2 = (G2[0, :B] - smean[1, 0]) * sinv[1, 0]
    bw2 = _f64(dev["bw2"])
    hk = d.hk_rows
    assert bw2.shape[0] == Bp // hk
    for blk, (r0, r1) in enumerate(_blocks(Bp, hk, B)):
        dy, n = dY2[r0:r1], r1 - r0
        rep.add("l3.bw2", np.abs(bw2[blk, :, 0] - dy.sum(0)), (n + 2) * U * np.abs(dy).sum(0), f"bb_bw2 sum dy block {blk}")
        rep.add("l3.bw2", np.abs(bw2[blk, :, 1] - (dy * xh2[r0:r1]).sum(0)), (n + 4) * U * np.abs(dy * xh2[r0:r1]).sum(0),
                f"bb_bw2 sum dy xhat block {blk}")

    # ---- launch 4: naf_gemm_bundle with prologue and epilogue ---------------------------------------------------------------
    npb = Bp // hk
    grad = {k: _f64(dev["grad"][k]) for k in PARAMS}
    S1, S2, S1a, S2a = bw2[:, :, 0].sum(0), bw2[:, :, 1].sum(0), np.abs(bw2[:, :, 0]).sum(0), np.abs(bw2[:, :, 1]).sum(0)
    rep.add("l4.be2", np.abs(grad["be2"] - S1), (npb + 1) * U * S1a, "grad be2")
    rep.add("l4.g2", np.abs(grad["g2"] - S2), (npb + 1) * U * S2a, "grad g2")
    k1 = P[0]["g2"] * sinv[1, 0]
    dz = k1 * (dY2[:B] - S1 / B - xh2 * (S2 / B))
    Mdz = np.abs(k1) * (np.abs(dY2[:B]) + S1a / B + np.abs(xh2) * (S2a / B))
    cdz = npb + 10
    a1m = A1[0, :B]
    for name, ks, lhs, lhs_abs, rhs, c in (("slab_w2", d.ks_w2, dz, Mdz, a1m, cdz), ("slab_wh", d.ks_wh, dH[:B], np.abs(dH[:B]), A2[:B], 2)):
        slabs = _f64(dev[name]).reshape(ks, lhs.shape[1], rhs.shape[1])
        n = Bp // ks
        for s in range(ks):
            r0, r1 = min(B, s * n), min(B, (s + 1) * n)
            rep.add(f"l4.{name}", np.abs(slabs[s] - lhs[r0:r1].T @ rhs[r0:r1]), (n + c) * U * (lhs_abs[r0:r1].T @ np.abs(rhs[r0:r1])),
                    f"{name} {s}")
    dA1 = dz @ P[0]["W2"]
    MdA = Mdz @ np.abs(P[0]["W2"])
    mask = a1m > 0
    p0 = P[0]
    fwd = {"x": x[0], "a1": np.maximum(y1[0], 0), "c1": c1[0], "c2": c2[0]}
    pk = {"bn1.weight": p0["g1"], "bn1.bias": p0["be1"], "input_layer.weight": p0["W1"], "input_layer.bias": p0["b1"],
          "bn2.weight": p0["g2"], "bn2.bias": p0["be2"], "hidden_layer.weight": p0["W2"], "hidden_layer.bias": p0["b2"]}
    tau1, _ = O.relu_kink_tau(pk, fwd)
    amb = np.abs(y1[0]) <= tau1
    amb[:, h:] = False                         # (a pad column's pre-activation is exactly 0 on both sides)
    flips = mask != (y1[0] > 0)
    rep.add("l1.mask", np.abs(y1[0][flips]), tau1[flips], "A1's mask unlike float64's beyond rounding")
    rep.meta["ambiguous"] = int(amb.sum())
    zabs = np.abs(x[0]) @ np.abs(p0["W1"]).T + np.abs(p0["b1"]) + np.abs(smean[0, 0])
    if kept:
        xh1, xh_err = XH1[:B], np.zeros_like(zabs)
    else:
        xh1 = (x[0] @ p0["W1"].T + p0["b1"] - smean[0, 0]) * sinv[0, 0]
        xh_err = (S + 4) * U * zabs * sinv[0, 0]
    dy1 = dA1 * mask
    bw1, dw1 = _f64(dev["bw1"]), _f64(dev["dw1"])
    assert bw1.shape[0] == d.nb1 and dw1.shape[0] == d.nb1
    ax = np.abs(x[0])
    for blk, (r0, r1) in enumerate(_blocks(32 * d.nb1, 32, B)):
        sl = slice(r0, r1)
        Mm, da_amb = MdA[sl] * mask[sl], np.abs(dA1[sl]) * amb[sl]
        rep.add("l4.bw1", np.abs(bw1[blk, :, 0] - dy1[sl].sum(0)), (H + cdz + 32) * U * Mm.sum(0) + da_amb.sum(0), f"bb_bw1 sum dy block {blk}")
        rep.add("l4.bw1", np.abs(bw1[blk, :, 1] - (dy1[sl] * xh1[sl]).sum(0)),
                (H + cdz + 36) * U * (Mm * np.abs(xh1[sl])).sum(0) + (np.abs(dy1[sl]) * xh_err[sl]).sum(0) +
                (da_amb * np.abs(xh1[sl])).sum(0), f"bb_bw1 sum dy xhat block {blk}")
        rep.add("l4.dw1", np.abs(dw1[blk, :, :S] - dy1[sl].T @ x[0][sl]), (H + cdz + 33) * U * (Mm.T @ ax[sl]) + da_amb.T @ ax[sl],
                f"bb_dw1 block {blk}")

    # ---- launch 5 (a): naf_bb_layer1_bwd_finish from its own inputs -------------------------------------------------------------
    Pt, Pa = dw1[:, :, :S].sum(0), np.abs(dw1[:, :, :S]).sum(0)
    sdy, sdx, sdya, sdxa = bw1[:, :, 0].sum(0), bw1[:, :, 1].sum(0), np.abs(bw1[:, :, 0]).sum(0), np.abs(bw1[:, :, 1]).sum(0)
    Sx, wc, inv, g1 = mom[0, :S], _f64(dev["wc"])[:, :S], sinv[0, 0], p0["g1"]
    iw = inv[:, None] * wc
    refW = (g1 * inv)[:, None] * (Pt - (sdy / B)[:, None] * Sx[None] - (sdx / B)[:, None] * iw)
    tolW = (d.nb1 + 10) * U * np.abs(g1 * inv)[:, None] * (Pa + (sdya / B)[:, None] * np.abs(Sx)[None] + (sdxa / B)[:, None] * np.abs(iw))
    rep.add("l5.w1", np.abs(grad["W1"] - refW), tolW, "grad W1 by the header's formula")
    rep.add("l5.g1", np.abs(grad["g1"] - sdx), (d.nb1 + 1) * U * sdxa, "grad g1")
    rep.add("l5.be1", np.abs(grad["be1"] - sdy), (d.nb1 + 1) * U * sdya, "grad be1")
    exact("l5.bias0", not grad["b1"].any() and not grad["b2"].any(), "grad b1 = grad b2 = 0 exactly")
    exact("l5.slabs", _bits_equal(dev["grad"]["W2"], slab_sum_f32(dev["slab_w2"]).reshape(H, H)), "grad W2 = the slabs added in order, to the bit")
    exact("l5.slabs", _bits_equal(dev["grad"]["Wh"], slab_sum_f32(dev["slab_wh"]).reshape(NHP, HP)), "grad Wh = the slabs added in order, to the bit")
    g2n = float(sum((grad[k] ** 2).sum() for k in PARAMS))
    rep.add("l5.sumsq", abs(float(dev["sumsq"]) - g2n), NORM_SELF_RTOL * g2n, "sum(partials) against ||grad||^2")
    exact("l5.step", int(dev["step"]) == int(pre["step"]) + 1, "step_live advanced by exactly 1")
    exact("l5.flag", int(dev["flag"]) == int(pre["flag"]) + 1, "bb_fold_flag advanced by exactly 1")

    # ---- launch 5 (b): launches 4 and 5 together against the direct BatchNorm backward dz1^T X ------------------------------------
    dz1, dg1, dbe1 = O.bn_train_backward(dy1, c1[0], g1)
    refs = {"W1": dz1.T @ x[0], "g1": dg1, "be1": dbe1}
    slack = {k: 0.0 for k in refs}
    xh64, inv64 = c1[0]["xhat"], c1[0]["invstd"]
    for rr, cc in np.argwhere(amb):
        v = dA1[rr, cc]
        dgm = v * xh64[rr, cc]
        col = -v / B - xh64[:, cc] * (dgm / B)
        col[rr] += v
        slack["W1"] += float(np.linalg.norm((g1[cc] * inv64[cc] * col) @ x[0]))
        slack["g1"] += abs(dgm)
        slack["be1"] += abs(v)
    rel = {}
    for k, rf in refs.items():
        e, nrm = float(np.linalg.norm(grad[k] - rf)), float(np.linalg.norm(rf))
        rel[k] = e / nrm
        rep.add(f"l5b.{k}", e, FINISH_B_RTOL * nrm + slack[k], f"grad {k} against the direct BatchNorm backward")
    rep.meta["finish_b"] = rel

    # ---- padding: the pad columns of a layer stored padded stay exactly 0 in every output ----------------------------------------
    if h != H:
        zero = [A1[:, :, h:], G2[:, :, h:], A2[:, h:H], dY2[:, h:], _f64(dev["wc"])[h:, :S], st2[:, :, h:], bw2[:, h:], bw1[:, h:],
                dw1[:, h:, :S], _f64(dev["slab_w2"]).reshape(-1, H, H)[:, h:], _f64(dev["slab_w2"]).reshape(-1, H, H)[:, :, h:],
                _f64(dev["slab_wh"]).reshape(-1, NHP, HP)[:, :, h:H], grad["W1"][h:], grad["g1"][h:], grad["be1"][h:], grad["W2"][h:],
                grad["W2"][:, h:], grad["g2"][h:], grad["be2"][h:], grad["Wh"][:, h:H]]
        if kept:
            zero.append(XH1[:, h:])
        exact("pad_cols", not any(z.any() for z in zero), "pad columns of a layer stored padded")
    return rep


# ------------------------------------------------------------------------------------------------------------------------
def f32_standin(pre: dict, batch, d: Dims, defect: str | None = None) -> dict:
    """What check_launches() reads from a device, computed in float32 numpy from the same state, launch after launch, each
    from the previous one's float32 output — honest float32 in another order of operations than the kernels' (direct batch
    statistics instead of the moments and block folds). defect: None or one of DEFECTS, a chain that is wrong in one way:
      target_bn2_from_main        launch 3 normalises the target network with the main network's gamma2 / beta2
      target_w2_from_main         launch 2 multiplies the target network's A1 with the main network's W2
      mask_no_beta1               the epilogue's ReLU mask is xhat gamma > 0 instead of fma(xhat, gamma, beta) > 0
      k1_no_gamma                 the prologue's k1 = invstd instead of gamma invstd
      biased_running_var          running_var takes the biased variance
      momentum_on_old             running statistics = momentum x old + (1 - momentum) x batch
      target_stats_in_main_slots  both networks write their running statistics to the main network's slots
      batch_mean_partials         bb_st2's second component about the batch mean instead of the block mean
      dw1_no_invstd               the finish launch's c2 term of d_W1 without its invstd
      slabs_reversed              the finish launch adds the split-K slabs last to first"""
    assert defect is None or defect in DEFECTS, defect
    f = np.float32
    S, A, T, H, B, Bp, HP, NHP, kp = d.S, d.A, d.T, d.H, d.B, d.Bp, d.HP, d.NHP, d.kp
    st, ac, rw, ns = batch
    xs = [np.asarray(st, f), np.asarray(ns, f)]
    P = [{k: np.asarray(v, f) for k, v in pre["net"][n].items()} for n in (0, 1)]
    bn0 = np.asarray(pre["bn"], f)
    bn = bn0.copy()
    mom_, one = f(BN_MOMENTUM), f(1.0)

    def bn_fwd(z, gamma, beta, net, layer):
        y, cache, rm, rv = O.bn_train_forward(z, gamma, beta, bn0[net, 2 * layer], bn0[net, 2 * layer + 1])
        var = ((z - cache["mean"]) ** 2).mean(axis=0)
        if defect == "biased_running_var":
            rv = ((one - mom_) * bn0[net, 2 * layer + 1] + mom_ * var).astype(f)
        if defect == "momentum_on_old":
            rm = (mom_ * bn0[net, 2 * layer] + (one - mom_) * cache["mean"]).astype(f)
            rv = (mom_ * bn0[net, 2 * layer + 1] + (one - mom_) * var * f(B / (B - 1))).astype(f)
        slot = 0 if defect == "target_stats_in_main_slots" else net
        bn[slot, 2 * layer], bn[slot, 2 * layer + 1] = rm, rv
        return y, cache

    out = {"save_mean": np.zeros((2, 2, H), f), "save_invstd": np.zeros((2, 2, H), f)}
    # launch 1
    A1 = np.zeros((2, Bp, H), f)
    mom = np.zeros((2, kp + kp * kp), f)
    c1 = []
    for net in (0, 1):
        p = P[net]
        y, cache = bn_fwd(xs[net] @ p["W1"].T + p["b1"], p["g1"], p["be1"], net, 0)
        A1[net, :B] = np.maximum(y, 0)
        out["save_mean"][0, net], out["save_invstd"][0, net] = cache["mean"], cache["invstd"]
        c1.append(cache)
        X = xs[net].astype(np.float64)
        Cf = np.zeros((kp, kp))
        Cf[:S, :S] = (X - X.mean(0)).T @ (X - X.mean(0))
        mom[net, :S], mom[net, kp:] = X.sum(0), Cf.reshape(-1)
    XH1 = np.zeros((Bp, H), f)
    XH1[:B] = c1[0]["xhat"]
    wc = np.zeros((H, kp), f)
    wc[:, :S] = P[0]["W1"] @ mom[0, kp:].reshape(kp, kp)[:S, :S]
    # launch 2
    G2 = np.zeros((2, Bp, H), f)
    st2 = np.zeros((2, d.nb, H, 2), f)
    for net in (0, 1):
        W2 = P[0]["W2"] if (net == 1 and defect == "target_w2_from_main") else P[net]["W2"]
        G2[net, :B] = A1[net, :B] @ W2.T + P[net]["b2"]
        for blk, (r0, r1) in enumerate(_blocks(64 * d.nb, 64, B)):
            g = G2[net, r0:r1]
            s = g.sum(0)
            m = G2[net, :B].mean(0) if defect == "batch_mean_partials" else s / f(r1 - r0)
            st2[net, blk, :, 0], st2[net, blk, :, 1] = s, ((g - m) ** 2).sum(0)
    # launch 3
    c2, a2 = [], []
    for net in (0, 1):
        src = P[0] if (net == 1 and defect == "target_bn2_from_main") else P[net]
        y, cache = bn_fwd(G2[net, :B], src["g2"], src["be2"], net, 1)
        out["save_mean"][1, net], out["save_invstd"][1, net] = cache["mean"], cache["invstd"]
        c2.append(cache)
        a2.append(np.maximum(y, 0))
    A2 = np.zeros((Bp, HP), f)
    A2[:, H] = 1.0
    A2[:B, :H] = a2[0]
    Whm, Wht = P[0]["Wh"], P[1]["Wh"]
    heads = a2[0] @ Whm[:, :H].T + Whm[:, H]
    vn = a2[1] @ Wht[A + T, :H] + Wht[A + T, H]
    mu_pre, l_pre, V = heads[:, :A], heads[:, A:A + T], heads[:, A + T]
    u, r = np.asarray(ac, f), np.asarray(rw, f).reshape(-1)
    Q = O.head_forward(mu_pre, l_pre, V, u, d.p_mode)["Q"]
    y_td = r + f(d.gamma) * vn
    err = Q - y_td
    dq = (f(2.0) * err / f(B)).astype(f)
    d_mu, d_l, d_V = O.head_backward(mu_pre, l_pre, u, dq, d.p_mode)
    dH = np.zeros((Bp, NHP), f)
    dH[:B, :A], dH[:B, A:A + T], dH[:B, A + T] = d_mu, d_l, d_V
    dY2 = np.zeros((Bp, H), f)
    dY2[:B] = (dH[:B] @ Whm[:, :H]) * (a2[0] > 0)
    xh2 = c2[0]["xhat"]
    hk = d.hk_rows
    bw2 = np.zeros((Bp // hk, H, 2), f)
    for blk, (r0, r1) in enumerate(_blocks(Bp, hk, B)):
        bw2[blk, :, 0], bw2[blk, :, 1] = dY2[r0:r1].sum(0), (dY2[r0:r1] * xh2[r0:r1]).sum(0)
    # launch 4
    grad = {k: np.zeros_like(P[0][k]) for k in PARAMS}
    S1, S2 = bw2[:, :, 0].sum(0), bw2[:, :, 1].sum(0)
    grad["be2"], grad["g2"] = S1, S2
    inv2 = c2[0]["invstd"]
    k1 = inv2 if defect == "k1_no_gamma" else P[0]["g2"] * inv2
    dz = k1 * (dY2[:B] - S1 / f(B) - xh2 * (S2 / f(B)))
    slab_w2, slab_wh = np.zeros((d.ks_w2, H * H), f), np.zeros((d.ks_wh, NHP * HP), f)
    for slabs, ks, lhs, rhs in ((slab_w2, d.ks_w2, dz, A1[0, :B]), (slab_wh, d.ks_wh, dH[:B], A2[:B])):
        n = Bp // ks
        for s in range(ks):
            r0, r1 = min(B, s * n), min(B, (s + 1) * n)
            slabs[s] = (lhs[r0:r1].T @ rhs[r0:r1]).reshape(-1)
    dA1 = dz @ P[0]["W2"]
    xh1 = c1[0]["xhat"]
    mask = (xh1 * P[0]["g1"] > 0) if defect == "mask_no_beta1" else (A1[0, :B] > 0)
    dy1 = dA1 * mask
    bw1, dw1 = np.zeros((d.nb1, H, 2), f), np.zeros((d.nb1, H, kp), f)
    for blk, (r0, r1) in enumerate(_blocks(32 * d.nb1, 32, B)):
        bw1[blk, :, 0], bw1[blk, :, 1] = dy1[r0:r1].sum(0), (dy1[r0:r1] * xh1[r0:r1]).sum(0)
        dw1[blk, :, :S] = dy1[r0:r1].T @ xs[0][r0:r1]
    # launch 5
    Pt, sdy, sdx = dw1[:, :, :S].sum(0), bw1[:, :, 0].sum(0), bw1[:, :, 1].sum(0)
    inv1, g1 = c1[0]["invstd"], P[0]["g1"]
    iw = wc[:, :S] if defect == "dw1_no_invstd" else inv1[:, None] * wc[:, :S]
    grad["W1"] = ((g1 * inv1)[:, None] * (Pt - (sdy / f(B))[:, None] * mom[0, :S][None] - (sdx / f(B))[:, None] * iw)).astype(f)
    grad["g1"], grad["be1"] = sdx, sdy
    order = slice(None, None, -1) if defect == "slabs_reversed" else slice(None)
    grad["W2"] = slab_sum_f32(slab_w2[order]).reshape(H, H)
    grad["Wh"] = slab_sum_f32(slab_wh[order]).reshape(NHP, HP)
    for k, v in grad.items():
        assert v.dtype == f, k
    out.update(A1=A1, XH1=XH1 if d.keep_xhat1 else None, bn=bn, mom=mom, wc=wc, G2=G2, st2=st2, A2=A2, q=Q,
               loss=float((err.astype(np.float64) ** 2).mean()), dH=dH, dY2=dY2, bw2=bw2, bw1=bw1, dw1=dw1, slab_w2=slab_w2,
               slab_wh=slab_wh, grad=grad, sumsq=float(f(sum(float((v.astype(np.float64) ** 2).sum()) for v in grad.values()))),
               step=int(pre["step"]) + 1, flag=int(pre["flag"]) + 1)
    return out


# ========================================================================================================================
# The column-tile and the unfused chain: Learner._learn_rows_tiles and the non-row-split half of Learner.forward_train
# (csrc/fused_layers.hip, bn_relu.hip, naf_head.hip, naf_head_wide.hip, the plain three-product form of gemm_bundle.hip, torch
# GEMMs). The same convention: every launch against float64 from the device values it read. What differs from the row-split chain:
# G1 / G2 are the bare products (the BatchNorm kernels add the bias themselves), A2 exists for both networks, every backward kernel
# takes its ReLU mask from the stored activation (`out > 0`), so no mask has to be guessed, and Bp = B.
#
#     dev    A1 [2][B][H], G1 [2][B][H] | None (l1: layer 1's product never leaves the launch), G2 [2][B][H], A2 [2][B][HP],
#            save_mean / save_invstd [layer][net][H], bn, heads_partial [n_slabs][B][NHP] + vnext_partial [n_slabs][B] (s3) | Gh
#            [2][B][NHP], q [B], loss, dH [B][NHP], dA2 [B][HP] | None (b2), dZ2 [B][H], dA1 [B][H], dZ1 [B][H] | None (l1),
#            grad {as pre["net"][0]}, sumsq (the summed norm partials), step
#
# THE BOUNDS, by the header's rules; n and c per output (U = 2^-24):
# (1)   G1          n = S        c = 2    torch.bmm (rocBLAS): the product and the store
#       G2          n = H        c = 2    torch.bmm
#       heads       n = H + 1    c = 2    the slab-order float32 sum of heads_partial (H products and the bias, n_slabs adds of 8-term
#                                         slabs: any order of H + 1 terms) against A2_dev[0] Wh_main^T; vnext the same with the target's row
#       Gh          n = HP       c = 2    torch.bmm over the stored width (the ones column carries the bias)
#       dA2         n = NHP      c = 2    torch.mm; inside naf_heads_bwd_bn_relu_bwd the same product stays in registers and its bound
#                                         E_dy = (NHP + 2) U |dH| |Wh| (masked) is carried into everything below
#       xhat        3 roundings (g + b, - mean, x invstd), each at most U (|g| + |b| + |mean|) invstd: xh_err. Where layer 1's z is
#                   recomputed from the rows (naf_bn_relu_bwd_wgrad_push): (S + 4) U (|x| |W1|^T + |b1| + |mean|) invstd, as the
#                   row-split epilogue's
#       sum dy      n = B        c = 2    + sum E_dy                                   (d_beta; E_S1)
#       sum dy xhat n = B        c = 4    + sum (E_dy |xhat| + |dy| xh_err)            (d_gamma; E_S2)
#       dZ          |k1| (E_dy + E_S1 / B + |xhat| E_S2 / B + xh_err |S2| / B) + C_DZ U M_dz, M_dz = |k1| (|dy| + |S1| / B + |xhat| |S2| / B),
#                   C_DZ = 8 roundings: k1 = gamma invstd, 1 / B, the two products with it, xhat x (.), two subtractions, k1 x (.)
#       gWh         n = B        c = 2    dH_dev^T A2_dev[0], the ones column (the head biases) included
#       gW2         n = B        c = 2    dZ2_dev^T A1_dev[0]
#       dA1         n = H        c = 2    dZ2_dev W2_main
#       gW1         n = B        c = 2    dZ1_dev^T X where dZ1 is in memory; else scale |dZ1|^T |X| plus the dZ bound above times |X|
# (2)   activations, saved and running statistics, q, loss, d_heads: the constants above, unchanged — the streamed BatchNorm
#       (B > 2048) at the same ones as the tiled. The heads' pre-activations and V' are the device's own (the slab-order sum is
#       the head launch's own order, csrc/naf_head.hip: to the bit), so V' brings no tolerance of its own here.
#       d_b1, d_b2 (identically 0 in exact arithmetic): max(BIAS0_REL ||grad||, SUM_ABS_RTOL sum|dZ|), learn_check's bound.
#       The norm: NORM_SELF_RTOL on sum(partials) against ||grad||^2, folded or from naf_grad_norm_partials.
# (3)   nothing is left to it: every output of these two chains is a dot product, sits behind (2), or is the BatchNorm backward
#       whose bound is derived above. No constant of these checks is measured.
C_DZ = 8
TILE_DEFECTS = ("target_bn2_from_main", "target_w2_from_main", "target_vrow_from_main", "mask_no_beta1", "mask_no_beta2",
                "k1_no_gamma", "vnext_from_state", "bn2_stats_in_layer1_slots", "target_stats_in_main_slots", "biased_running_var",
                "momentum_on_old", "gwh_no_bias_column", "slab_twice", "last_phase_dropped")
# move nothing where the target equals the main network, gamma = 1 and beta = 0. vnext_from_state is NOT among them: state and next_state
# differ at any state of the networks, and the layer-1 check of the target rejects it at the init state too.
TILE_ADMITTED_AT_INIT = TILE_DEFECTS[:6]


def bn_row_phases(B: int) -> int:
    """Row phases of the BatchNorm tile a batch takes (csrc/bn_relu.hip, BN_DISPATCH and BN_MAX_B): 64 up to B = 512, 128 beyond —
    held in registers up to 2048 rows, streamed beyond."""
    return 64 if B <= 512 else 128


def _kink_tau(gamma, beta, cache, zabs):
    """naf_oracle.relu_kink_tau's scale for one layer in the stored layout"""
    g = np.abs(gamma)
    return O.KINK_KAPPA * U * (g * cache["invstd"] * zabs + g * np.abs(cache["xhat"]) + np.abs(beta))


def _bn_bwd_ref(dy, E_dy, xh, xh_err, k1, B):
    """float64 BatchNorm backward of one layer from the launch's own inputs and the first-order bounds of the header:
    (S1, S2, E_S1, E_S2, dz, tol_dz)"""
    S1, S2 = dy.sum(0), (dy * xh).sum(0)
    E1 = (B + 2) * U * np.abs(dy).sum(0) + E_dy.sum(0)
    E2 = (B + 4) * U * np.abs(dy * xh).sum(0) + (E_dy * np.abs(xh) + np.abs(dy) * xh_err).sum(0)
    dz = k1 * (dy - S1 / B - xh * (S2 / B))
    Mdz = np.abs(k1) * (np.abs(dy) + np.abs(S1) / B + np.abs(xh) * (np.abs(S2) / B))
    tol = np.abs(k1) * (E_dy + E1 / B + np.abs(xh) * (E2 / B) + xh_err * (np.abs(S2) / B)) + C_DZ * U * Mdz
    return S1, S2, E1, E2, dz, tol


def check_tile_launches(pre: dict, batch, dev: dict, d: Dims) -> Report:
    """Every launch of one update of the column-tile | unfused chain (d.fuse says which launches ran) against float64 from the
    values it read. Returns a learn_check.Report as check_launches does; .meta["ambiguous"]: ReLU elements of the main network
    (both layers) within rounding of 0."""
    rep = Report()
    S, A, T, H, h, B, HP, NHP = d.S, d.A, d.T, d.H, d.h, d.B, d.HP, d.NHP
    assert d.Bp == B and "bb" not in d.fuse
    l1, b2, gb, s3 = ("l1" in d.fuse), ("b2" in d.fuse), ("gb" in d.fuse), ("s3" in d.fuse)
    st, ac, rw, ns = batch
    x = [_f64(st), _f64(ns)]
    P = [{k: _f64(v) for k, v in pre["net"][n].items()} for n in (0, 1)]
    bn0, bn1 = _f64(pre["bn"]), _f64(dev["bn"])
    A1, G2, A2, dH, dZ2, dA1 = (_f64(dev[k]) for k in ("A1", "G2", "A2", "dH", "dZ2", "dA1"))
    smean, sinv = _f64(dev["save_mean"]), _f64(dev["save_invstd"])
    assert (dev.get("G1") is None) == l1 and (dev.get("dZ1") is None) == l1 and (dev.get("dA2") is None) == b2
    assert (dev.get("heads_partial") is not None) == s3 and (dev.get("Gh") is None) == s3
    assert A1.shape == (2, B, H) and G2.shape == (2, B, H) and A2.shape == (2, B, HP) and dH.shape == (B, NHP)

    def exact(check, cond, what):
        rep.add(check, 0.0 if bool(cond) else 1.0, 0.5, what)

    # ---- layer 1, both nets: naf_linear_bn_relu_fwd_train | torch.bmm + naf_bn_relu_fwd_train(1) ------------------------------------
    c1, amb = [], 0
    for net in (0, 1):
        p = P[net]
        zabs = np.abs(x[net]) @ np.abs(p["W1"]).T
        if l1:
            z = x[net] @ p["W1"].T + p["b1"]
        else:
            G1 = _f64(dev["G1"])[net]
            rep.add("f1.g1", np.abs(G1 - x[net] @ p["W1"].T), (S + 2) * U * zabs, f"G1 net {net}")
            z, zabs = G1 + p["b1"], np.abs(G1)
        y, cache, rm, rv = O.bn_train_forward(z, p["g1"], p["be1"], bn0[net, 0], bn0[net, 1])
        ref = np.maximum(y, 0)
        rep.add("f1.a1", np.abs(A1[net] - ref), ACT_TOL * ref + ACT_TOL, f"A1 net {net}")
        _check_stats(rep, "f1", smean, sinv, bn1, 0, net, cache, rm, rv)
        c1.append(cache)
        if net == 0:
            tau = _kink_tau(p["g1"], p["be1"], cache, zabs + np.abs(p["b1"]) + np.abs(cache["mean"]))
            flips = (A1[0] > 0) != (y > 0)
            rep.add("f1.mask", np.abs(y[flips]), tau[flips], "A1's mask unlike float64's beyond rounding")
            amb += int((np.abs(y)[:, :h] <= tau[:, :h]).sum())

    # ---- GEMM 2, both nets: torch.bmm, each from its own W2 and its own A1 -----------------------------------------------------------
    for net in (0, 1):
        a, w = A1[net], P[net]["W2"]
        rep.add("g2.g2", np.abs(G2[net] - a @ w.T), (H + 2) * U * (np.abs(a) @ np.abs(w).T), f"G2 net {net}")

    # ---- layer 2, both nets: naf_bn_relu_fwd_heads_partial | naf_bn_relu_fwd_train(2) + torch.bmm ---------------------------------------
    c2 = []
    for net in (0, 1):
        p = P[net]
        y, cache, rm, rv = O.bn_train_forward(G2[net] + p["b2"], p["g2"], p["be2"], bn0[net, 2], bn0[net, 3])
        ref = np.maximum(y, 0)
        rep.add("f2.a2", np.abs(A2[net, :, :H] - ref), ACT_TOL * ref + ACT_TOL, f"A2 net {net}")
        _check_stats(rep, "f2", smean, sinv, bn1, 1, net, cache, rm, rv)
        c2.append(cache)
        if net == 0:
            tau = _kink_tau(p["g2"], p["be2"], cache, np.abs(G2[0]) + np.abs(p["b2"]) + np.abs(cache["mean"]))
            flips = (A2[0, :, :H] > 0) != (y > 0)
            rep.add("f2.mask", np.abs(y[flips]), tau[flips], "A2's mask unlike float64's beyond rounding")
            amb += int((np.abs(y)[:, :h] <= tau[:, :h]).sum())
    rep.meta["ambiguous"] = amb
    exact("f2.ones", (A2[:, :, H] == 1).all() and not A2[:, :, H + 1:].any(), "A2's constant-1 column and the zeros behind it")
    Whm, Wht = P[0]["Wh"], P[1]["Wh"]
    v = A + T
    if s3:
        hp, vp = np.asarray(dev["heads_partial"], np.float32), np.asarray(dev["vnext_partial"], np.float32)
        assert hp.shape == (d.n_slabs, B, NHP) and vp.shape == (d.n_slabs, B) and d.n_slabs == H // 8
        heads, vn = _f64(slab_sum_f32(hp)), _f64(slab_sum_f32(vp))
        a2m, a2t = A2[0, :, :H], A2[1, :, :H]
        rep.add("f2.heads", np.abs(heads - (a2m @ Whm[:, :H].T + Whm[:, H])), (H + 3) * U * (a2m @ np.abs(Whm[:, :H]).T + np.abs(Whm[:, H])),
                "the slab-order sum of heads_partial")
        rep.add("f2.vnext", np.abs(vn - (a2t @ Wht[v, :H] + Wht[v, H])), (H + 3) * U * (a2t @ np.abs(Wht[v, :H]) + abs(Wht[v, H])),
                "the slab-order sum of vnext_partial against the TARGET's value row")
    else:
        Gh = _f64(dev["Gh"])
        assert Gh.shape == (2, B, NHP)
        for net in (0, 1):
            w = P[net]["Wh"]
            rep.add("f2.gh", np.abs(Gh[net] - A2[net] @ w.T), (HP + 2) * U * (np.abs(A2[net]) @ np.abs(w).T), f"Gh net {net}")
        heads, vn = Gh[0], Gh[1][:, v]

    # ---- head: naf_head_fwd_bwd_mse_splitk | naf_head_fwd_bwd_mse (naf_head_wide.hip beyond 8 joints) -----------------------------------
    _check_head(rep, "hd", d, heads[:, :A], heads[:, A:v], heads[:, v], vn, 0.0, ac, rw, dev["q"], dev["loss"], dH)

    # ---- layer 2 backward: naf_heads_bwd_bn_relu_bwd | torch.mm + naf_bn_relu_bwd(2) ------------------------------------------------------
    grad = {k: _f64(dev["grad"][k]) for k in PARAMS}
    gnorm2 = float(sum((g ** 2).sum() for g in grad.values()))
    gnorm = gnorm2 ** 0.5
    on2 = A2[0, :, :H] > 0
    if b2:
        dy2 = (dH @ Whm[:, :H]) * on2
        E_dy = (NHP + 2) * U * (np.abs(dH) @ np.abs(Whm[:, :H])) * on2
    else:
        dA2 = _f64(dev["dA2"])
        assert dA2.shape == (B, HP)
        rep.add("b2.da2", np.abs(dA2 - dH @ Whm), (NHP + 2) * U * (np.abs(dH) @ np.abs(Whm)), "dA2")
        dy2, E_dy = dA2[:, :H] * on2, np.zeros((B, H))
    mean2, inv2, b2v = smean[1, 0], sinv[1, 0], P[0]["b2"]
    xh2 = (G2[0] + b2v - mean2) * inv2
    xe2 = 3 * U * (np.abs(G2[0]) + np.abs(b2v) + np.abs(mean2)) * inv2
    S1, S2, E1, E2, dz2, tz2 = _bn_bwd_ref(dy2, E_dy, xh2, xe2, P[0]["g2"] * inv2, B)
    rep.add("b2.dz2", np.abs(dZ2 - dz2), tz2, "dZ2")
    rep.add("b2.g2", np.abs(grad["g2"] - S2), E2, "grad g2")
    rep.add("b2.be2", np.abs(grad["be2"] - S1), E1, "grad be2")
    rep.add("b2.bias0", np.abs(grad["b2"]), np.maximum(BIAS0_REL * gnorm, SUM_ABS_RTOL * np.abs(dZ2).sum(0)), "grad b2 = 0 to rounding")

    # ---- the bundle (naf_gemm_bundle, three products) | three torch.mm ----------------------------------------------------------------------
    rep.add("gb.gwh", np.abs(grad["Wh"] - dH.T @ A2[0]), (B + 2) * U * (np.abs(dH).T @ np.abs(A2[0])), "grad Wh, the bias column included")
    rep.add("gb.gw2", np.abs(grad["W2"] - dZ2.T @ A1[0]), (B + 2) * U * (np.abs(dZ2).T @ np.abs(A1[0])), "grad W2")
    rep.add("gb.da1", np.abs(dA1 - dZ2 @ P[0]["W2"]), (H + 2) * U * (np.abs(dZ2) @ np.abs(P[0]["W2"])), "dA1")

    # ---- layer 1 backward: naf_bn_relu_bwd_wgrad_push (push = None) | naf_bn_relu_bwd(1) + torch.mm -----------------------------------------
    p0 = P[0]
    mean1, inv1 = smean[0, 0], sinv[0, 0]
    dy1 = dA1 * (A1[0] > 0)
    if l1:
        z1 = x[0] @ p0["W1"].T + p0["b1"]
        xe1 = (S + 4) * U * (np.abs(x[0]) @ np.abs(p0["W1"]).T + np.abs(p0["b1"]) + np.abs(mean1)) * inv1
    else:
        G1m = _f64(dev["G1"])[0]
        z1 = G1m + p0["b1"]
        xe1 = 3 * U * (np.abs(G1m) + np.abs(p0["b1"]) + np.abs(mean1)) * inv1
    xh1 = (z1 - mean1) * inv1
    S1, S2, E1, E2, dz1, tz1 = _bn_bwd_ref(dy1, np.zeros((B, H)), xh1, xe1, p0["g1"] * inv1, B)
    rep.add("b1.g1", np.abs(grad["g1"] - S2), E2, "grad g1")
    rep.add("b1.be1", np.abs(grad["be1"] - S1), E1, "grad be1")
    ax = np.abs(x[0])
    if l1:
        rep.add("b1.gw1", np.abs(grad["W1"] - dz1.T @ x[0]), (B + 2) * U * (np.abs(dz1).T @ ax) + tz1.T @ ax, "grad W1")
        dz1_abs = np.abs(dz1)
    else:
        dZ1 = _f64(dev["dZ1"])
        rep.add("b1.dz1", np.abs(dZ1 - dz1), tz1, "dZ1")
        rep.add("b1.gw1", np.abs(grad["W1"] - dZ1.T @ x[0]), (B + 2) * U * (np.abs(dZ1).T @ ax), "grad W1")
        dz1_abs = np.abs(dZ1)
    rep.add("b1.bias0", np.abs(grad["b1"]), np.maximum(BIAS0_REL * gnorm, SUM_ABS_RTOL * dz1_abs.sum(0)), "grad b1 = 0 to rounding")

    # ---- the norm partials (folded into the producers | naf_grad_norm_partials) and the step count --------------------------------------------
    rep.add("nm.sumsq", abs(float(dev["sumsq"]) - gnorm2), NORM_SELF_RTOL * gnorm2, "sum(partials) against ||grad||^2")
    exact("nm.step", int(dev["step"]) == int(pre["step"]) + 1, "the step count advanced by exactly 1")

    # ---- padding: the pad columns of a layer stored padded stay exactly 0 in every output -------------------------------------------------------
    if h != H:
        zero = [A1[:, :, h:], G2[:, :, h:], A2[:, :, h:H], dZ2[:, h:], dA1[:, h:], grad["W1"][h:], grad["g1"][h:], grad["be1"][h:],
                grad["b1"][h:], grad["W2"][h:], grad["W2"][:, h:], grad["g2"][h:], grad["be2"][h:], grad["b2"][h:], grad["Wh"][:, h:H]]
        zero += [_f64(dev[k])[..., h:H] for k in ("G1", "dZ1", "dA2") if dev.get(k) is not None]
        exact("pad_cols", not any(z.any() for z in zero), "pad columns of a layer stored padded")
    return rep


def f32_standin_tiles(pre: dict, batch, d: Dims, defect: str | None = None) -> dict:
    """What check_tile_launches() reads from a device, computed in float32 numpy from the same state, launch after launch, each
    from the previous one's float32 output. defect: None or one of TILE_DEFECTS, a chain that is wrong in one way:
      target_bn2_from_main        layer 2 normalises the target network with the main network's gamma2 / beta2
      target_w2_from_main         GEMM 2 multiplies the target network's A1 with the main network's W2
      target_vrow_from_main       V' from the main network's value row (and bias) on the target's A2
      mask_no_beta1 | 2           the backward's ReLU mask of that layer is xhat gamma > 0 instead of the stored activation > 0
      vnext_from_state            the target network reads `state` instead of `next_state`
      k1_no_gamma                 layer 2's backward with k1 = invstd instead of gamma invstd
      bn2_stats_in_layer1_slots   layer 2 writes its running statistics into layer 1's slots
      target_stats_in_main_slots  both networks write their running statistics to the main network's slots
      biased_running_var          running_var takes the biased variance
      momentum_on_old             running statistics = momentum x old + (1 - momentum) x batch
      gwh_no_bias_column          grad Wh without its column H (the head biases)
      slab_twice                  the split-K head adds slab 1 twice (s3 only)
      last_phase_dropped          the batch mean's sum leaves out the rows of the last, partial pass over the row phases"""
    assert defect is None or defect in TILE_DEFECTS, defect
    f = np.float32
    S, A, T, H, B, HP, NHP = d.S, d.A, d.T, d.H, d.B, d.HP, d.NHP
    l1, b2, s3 = ("l1" in d.fuse), ("b2" in d.fuse), ("s3" in d.fuse)
    st, ac, rw, ns = batch
    xs = [np.asarray(st, f), np.asarray(st if defect == "vnext_from_state" else ns, f)]
    P = [{k: np.asarray(v, f) for k, v in pre["net"][n].items()} for n in (0, 1)]
    bn0 = np.asarray(pre["bn"], f)
    bn = bn0.copy()
    mom_, one, eps = f(BN_MOMENTUM), f(1.0), f(O.BN_EPS)
    out = {"save_mean": np.zeros((2, 2, H), f), "save_invstd": np.zeros((2, 2, H), f)}

    def bn_fwd(z, gamma, beta, net, layer):
        if defect == "last_phase_dropped":
            mean = (z[:((B - 1) // bn_row_phases(B)) * bn_row_phases(B)].sum(0) / f(B)).astype(f)
        else:
            mean = z.mean(axis=0)
        var = ((z - mean) ** 2).mean(axis=0)
        invstd = (one / np.sqrt(var + eps)).astype(f)
        xhat = (z - mean) * invstd
        y = xhat * gamma + beta
        unb = var if (defect == "biased_running_var" or B == 1) else var * f(B / (B - 1))
        old_m, old_v = bn0[net, 2 * layer], bn0[net, 2 * layer + 1]
        if defect == "momentum_on_old":
            rm, rv = mom_ * old_m + (one - mom_) * mean, mom_ * old_v + (one - mom_) * unb
        else:
            rm, rv = (one - mom_) * old_m + mom_ * mean, (one - mom_) * old_v + mom_ * unb
        slot = 0 if defect == "target_stats_in_main_slots" else net
        ls = 0 if defect == "bn2_stats_in_layer1_slots" else layer
        bn[slot, 2 * ls], bn[slot, 2 * ls + 1] = rm.astype(f), rv.astype(f)
        out["save_mean"][layer, net], out["save_invstd"][layer, net] = mean, invstd
        assert y.dtype == f
        return y, {"mean": mean, "invstd": invstd, "xhat": xhat}

    G1, A1, G2, A2 = np.zeros((2, B, H), f), np.zeros((2, B, H), f), np.zeros((2, B, H), f), np.zeros((2, B, HP), f)
    A2[:, :, H] = 1.0
    c1, c2 = [], []
    for net in (0, 1):
        p = P[net]
        G1[net] = xs[net] @ p["W1"].T
        y, cache = bn_fwd(G1[net] + p["b1"], p["g1"], p["be1"], net, 0)
        A1[net] = np.maximum(y, 0)
        c1.append(cache)
    for net in (0, 1):
        W2 = P[0]["W2"] if (net == 1 and defect == "target_w2_from_main") else P[net]["W2"]
        G2[net] = A1[net] @ W2.T
        src = P[0] if (net == 1 and defect == "target_bn2_from_main") else P[net]
        y, cache = bn_fwd(G2[net] + P[net]["b2"], src["g2"], src["be2"], net, 1)
        A2[net, :, :H] = np.maximum(y, 0)
        c2.append(cache)
    Whm = P[0]["Wh"]
    Wv = (P[0] if defect == "target_vrow_from_main" else P[1])["Wh"][A + T]
    if s3:
        n = H // 8
        hp, vp = np.zeros((n, B, NHP), f), np.zeros((n, B), f)
        for w in range(n):
            c = slice(8 * w, 8 * w + 8)
            hp[w] = A2[0][:, c] @ Whm[:, c].T + (Whm[:, H] if w == 0 else f(0))
            vp[w] = A2[1][:, c] @ Wv[c] + (Wv[H] if w == 0 else f(0))
        out.update(heads_partial=hp, vnext_partial=vp, Gh=None)
        heads = slab_sum_f32(np.concatenate([hp[:2], hp[1:]]) if defect == "slab_twice" else hp)
        vn = slab_sum_f32(vp)
    else:
        Gh = np.stack([A2[net] @ P[net]["Wh"].T for net in (0, 1)]).astype(f)
        Gh[1][:, A + T] = A2[1] @ Wv
        out.update(heads_partial=None, vnext_partial=None, Gh=Gh)
        heads, vn = Gh[0], Gh[1][:, A + T]
    mu_pre, l_pre, V = heads[:, :A], heads[:, A:A + T], heads[:, A + T]
    u, r = np.asarray(ac, f), np.asarray(rw, f).reshape(-1)
    Q = O.head_forward(mu_pre, l_pre, V, u, d.p_mode)["Q"]
    err = Q - (r + f(d.gamma) * vn)
    dq = (f(2.0) * err / f(B)).astype(f)
    d_mu, d_l, d_V = O.head_backward(mu_pre, l_pre, u, dq, d.p_mode)
    dH = np.zeros((B, NHP), f)
    dH[:, :A], dH[:, A:A + T], dH[:, A + T] = d_mu, d_l, d_V
    grad = {k: np.zeros_like(P[0][k]) for k in PARAMS}
    grad["Wh"] = dH.T @ A2[0]
    if defect == "gwh_no_bias_column":
        grad["Wh"][:, H] = 0
    dA2 = dH @ Whm

    def bn_bwd(d_out, act, cache, gamma, no_beta, no_gamma=False):
        mask = (cache["xhat"] * gamma > 0) if no_beta else (act > 0)
        dy = d_out * mask
        s1, s2 = dy.sum(0), (dy * cache["xhat"]).sum(0)
        k1 = cache["invstd"] if no_gamma else gamma * cache["invstd"]
        dz = (k1 * (dy - s1 / f(B) - cache["xhat"] * (s2 / f(B)))).astype(f)
        return dz, s2, s1, dz.sum(0)

    dZ2, grad["g2"], grad["be2"], grad["b2"] = bn_bwd(dA2[:, :H], A2[0][:, :H], c2[0], P[0]["g2"], defect == "mask_no_beta2",
                                                      defect == "k1_no_gamma")
    grad["W2"] = dZ2.T @ A1[0]
    dA1 = dZ2 @ P[0]["W2"]
    dZ1, grad["g1"], grad["be1"], grad["b1"] = bn_bwd(dA1, A1[0], c1[0], P[0]["g1"], defect == "mask_no_beta1")
    grad["W1"] = dZ1.T @ xs[0]
    for k, v in grad.items():
        assert v.dtype == f and v.shape == P[0][k].shape, k
    out.update(A1=A1, G1=None if l1 else G1, G2=G2, A2=A2, bn=bn, q=Q, loss=float((err.astype(np.float64) ** 2).mean()), dH=dH,
               dA2=None if b2 else dA2, dZ2=dZ2, dA1=dA1, dZ1=None if l1 else dZ1, grad=grad,
               sumsq=float(f(sum(float((v.astype(np.float64) ** 2).sum()) for v in grad.values()))), step=int(pre["step"]) + 1)
    return out

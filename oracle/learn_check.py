"""
oracle/learn_check.py — TEST INFRASTRUCTURE ONLY. One learn() update of an implementation against a float64 oracle
started from that implementation's own state before the update (teacher forcing: errors never compound).

check_update() is the whole comparison; tests/test_learn_f64_gpu.py feeds it the HIP learner, tests/test_oracle_golden.py
feeds it the float32 numpy oracle (f32_standin) to show that the tolerances admit honest float32 arithmetic and reject
planted defects. The two tests share this function so that they cannot drift apart.

States are dicts in the reference's layout (naf_neural_network.py:37-54):
    {"main": {param and BatchNorm buffer name: array}, "target": {...}, "m": {param: array}, "v": {...}, "t": int}
"""
from __future__ import annotations

import numpy as np

from . import naf_oracle as O

# Tolerances: 2 - 100x the float32 numpy oracle's error on the case table of tests/learn_cases.py (test_oracle_golden.py
# checks that it passes them all):
Q_RTOL, Q_ATOL_REL = 1e-4, 1e-4          # per sample, atol relative to max |Q|
LOSS_RTOL = 1e-5
BN_RTOL, BN_ATOL = 1e-4, 1e-5            # running mean / var of both nets (f32 sums over up to 4096 rows)
GRAD_RTOL = 1e-4                         # per block, in norm, + 1.01 x the ReLU-kink slack of the block
KINK_SLACK_FACTOR = 1.01
BIAS0_REL = 1e-5                         # the two biases BatchNorm cancels: |g| <= 1e-5 ||g_total||
SUM_ABS_RTOL = 1e-5                      # ... or, for any bias block (a sum over rows), <= 1e-5 x the sum of its terms' magnitudes
NORM_SELF_RTOL = 1e-5                    # sqrt(sum of the norm partials) vs the norm of the gradient they cover
NORM_RTOL = 1e-4                         # ... vs the oracle's norm (+ the total kink slack)
THETA_ULPS, THETA_LR = 2.0, 1e-5         # theta and target: 2 ulp of theta + 1e-5 lr
MV_RTOL = 1e-5                           # m, v: relative to the magnitude of the terms that make them
ZERO_BIASES = ("input_layer.bias", "hidden_layer.bias")


def _spacing(*xs):
    """float32 ulp of the largest magnitude among xs (elementwise)"""
    a = np.max(np.stack([np.abs(np.asarray(x, np.float64)) for x in xs]), axis=0)
    return np.spacing(a.astype(np.float32)).astype(np.float64)


class Report:
    def __init__(self):
        self.ratios = {}          # check -> largest error / tolerance
        self.failures = []        # (check, message)
        self.meta = {}

    def add(self, check, err, tol, what=""):
        err, tol = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(tol, np.float64))
        r = err / np.maximum(tol, 1e-300)
        worst = float(r.max()) if r.size else 0.0
        if not np.isfinite(worst):
            worst = float("inf")
        self.ratios[check] = max(self.ratios.get(check, 0.0), worst)
        if worst > 1.0:
            i = int(np.argmax(r)) if r.size else 0
            self.failures.append((check, f"{check} {what}: error {float(err.ravel()[i]):.3e} > tolerance "
                                         f"{float(tol.ravel()[i]):.3e} (ratio {worst:.3g}, {int((r > 1).sum())} of {r.size})"))

    def failed(self, *checks):
        return any(c in checks for c, _ in self.failures)


def check_update(pre: dict, batch, dev: dict, lr=1e-3, tau=1e-3, gamma=0.99, p_mode=O.P_HADAMARD) -> Report:
    """pre: the implementation's state before the update. batch: (states, actions, rewards, next_states) of the minibatch as
    the implementation read them. dev: what the update left — "q" (B,), "loss" (the summed loss partials), "grad" {param: the
    gradient before the clip}, "norm" (sqrt of the summed norm partials) and the state after it ("main", "target", "m", "v",
    "t"). Returns a Report; report.failures is empty when every check holds."""
    rep = Report()
    st, ac, rw, ns = batch
    o = O.LearnerOracle.from_state(pre["main"], pre["target"], pre["m"], pre["v"], pre["t"], lr=lr, tau=tau, gamma=gamma,
                                   p_mode=p_mode, dtype=np.float64)
    loss64 = o.learn(st, ac, rw, ns)
    last = o.last
    p64, fwd, inter, g64 = last["params"], last["fwd"], last["inter"], last["grads"]
    tau1, tau2 = O.relu_kink_tau(p64, fwd)
    n_amb = int((np.abs(fwd["y1"]) <= tau1).sum() + (np.abs(fwd["y2"]) <= tau2).sum())
    # the implementation's ReLU masks, where it reports its activations: a mask unlike the oracle's only within tau of 0, and
    # the slack then covers exactly the elements masked the other way (without them: every element within tau of 0)
    flips = {}
    for a, y, t in (("a1", fwd["y1"], tau1), ("a2", fwd["y2"], tau2)):
        if a in dev:
            flips[a] = (np.asarray(dev[a]) > 0) != (y > 0)
            rep.add("mask", np.abs(y[flips[a]]), t[flips[a]], f"{a} mask unlike the oracle's")
    slack, n_slack = O.relu_kink_slack(p64, fwd, inter, tau1, tau2, flips.get("a1"), flips.get("a2"))
    rep.meta.update(ambiguous=n_amb, flipped=n_slack if flips else None, norm64=last["grad_norm"])

    # ---- 1. forward -------------------------------------------------------------------------------------------------
    Q = last["Q"]
    q = np.asarray(dev["q"], np.float64).reshape(-1)
    rep.add("q", np.abs(q - Q), Q_RTOL * np.abs(Q) + Q_ATOL_REL * np.abs(Q).max(), "q_out")
    rep.add("loss", abs(float(dev["loss"]) - loss64), LOSS_RTOL * abs(loss64), "summed loss")
    for net, ref in (("main", o.main), ("target", o.target)):
        for k in ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var"):
            got = np.asarray(dev[net][k], np.float64)
            rep.add("bn", np.abs(got - ref[k]), BN_RTOL * np.abs(ref[k]) + BN_ATOL, f"{net} {k}")

    # ---- 2. the gradient before the clip ------------------------------------------------------------------------------
    gd = {k: np.asarray(dev["grad"][k], np.float64).reshape(g64[k].shape) for k in O.PARAM_ORDER}
    gnorm_dev = float(np.sqrt(sum(float((gd[k] ** 2).sum()) for k in O.PARAM_ORDER)))
    # the blocks that are column sums over the minibatch rows: their terms' magnitudes (a sum that cancels to near 0 — the value
    # bias when the TD errors balance, the two biases BatchNorm cancels — is only known to f32 rounding of those magnitudes)
    m1, m2 = fwd["a1"] > 0, fwd["a2"] > 0
    abs_terms = {"input_layer.bias": np.abs(inter["dz1"]).sum(0), "hidden_layer.bias": np.abs(inter["dz2"]).sum(0),
                 "bn1.bias": np.abs(inter["d_a1"] * m1).sum(0), "bn2.bias": np.abs(inter["d_a2"] * m2).sum(0),
                 "action_values.bias": np.abs(inter["d_mu"]).sum(0), "matrix_entries.bias": np.abs(inter["d_l"]).sum(0),
                 "value.bias": np.abs(inter["d_V"]).sum(keepdims=True)}
    for k in O.PARAM_ORDER:
        if k in ZERO_BIASES:      # identically 0 in exact arithmetic: BatchNorm removes the bias again
            rep.add("bias0", np.abs(gd[k]), np.maximum(BIAS0_REL * last["grad_norm"], SUM_ABS_RTOL * abs_terms[k]), k)
            continue
        tol = GRAD_RTOL * np.linalg.norm(g64[k]) + KINK_SLACK_FACTOR * slack[k]
        if k in abs_terms:
            tol = max(tol, SUM_ABS_RTOL * float(np.linalg.norm(abs_terms[k])) + KINK_SLACK_FACTOR * slack[k])
        if k == "input_layer.weight":
            # dz1^T x = dz1^T (x - mean x) + (sum of dz1) mean x, and the sum of dz1 is 0 only to f32 rounding of its terms:
            # inputs far from 0 (tests/learn_cases.py, data "cancel") carry that rounding times their mean
            tol += SUM_ABS_RTOL * float(np.linalg.norm(abs_terms["input_layer.bias"]) * np.linalg.norm(fwd["x"].mean(0)))
        rep.add("grad", np.linalg.norm(gd[k] - g64[k]), tol, k)
    norm_dev = float(dev["norm"])
    rep.add("norm_self", abs(norm_dev - gnorm_dev), NORM_SELF_RTOL * gnorm_dev, "sqrt(sum partials) vs ||grad||")
    rep.add("norm", abs(norm_dev - last["grad_norm"]),
            NORM_RTOL * last["grad_norm"] + KINK_SLACK_FACTOR * sum(slack.values()), "sqrt(sum partials) vs oracle")

    # ---- 3. the optimizer step on the implementation's own gradient ---------------------------------------------------
    th, tg, m1, v1, t1, _, coef = O.optimizer_step(pre["main"], pre["target"], pre["m"], pre["v"], pre["t"], gd, lr=lr, tau=tau)
    rep.meta["clip"] = coef
    b2 = 0.999
    for k in O.PARAM_ORDER:
        shp = th[k].shape
        th0 = np.asarray(pre["main"][k], np.float64).reshape(shp)
        tg0 = np.asarray(pre["target"][k], np.float64).reshape(shp)
        thd = np.asarray(dev["main"][k], np.float64).reshape(shp)
        tgd = np.asarray(dev["target"][k], np.float64).reshape(shp)
        rep.add("theta", np.abs(thd - th[k]), THETA_ULPS * _spacing(th0, th[k]) + THETA_LR * lr, f"main {k}")
        rep.add("theta", np.abs(tgd - tg[k]), THETA_ULPS * _spacing(tg0, tg[k]) + THETA_LR * lr, f"target {k}")
        gs = gd[k] * coef
        m0 = np.asarray(pre["m"][k], np.float64).reshape(shp)
        v0 = np.asarray(pre["v"][k], np.float64).reshape(shp)
        # (scale: the terms m and v are made of — m can cancel to 0; a float32 v below the normal range may be flushed)
        rep.add("m", np.abs(np.asarray(dev["m"][k], np.float64).reshape(shp) - m1[k]),
                MV_RTOL * (np.abs(m1[k]) + 0.9 * np.abs(m0) + 0.1 * np.abs(gs)) + 1e-37, f"adam m {k}")
        rep.add("v", np.abs(np.asarray(dev["v"][k], np.float64).reshape(shp) - v1[k]),
                MV_RTOL * (v1[k] + b2 * v0 + (1 - b2) * gs * gs) + 1e-37, f"adam v {k}")
    rep.add("step", abs(int(dev["t"]) - t1), 0.5, "step count")
    return rep


def f32_standin(pre: dict, batch, lr=1e-3, tau=1e-3, gamma=0.99, p_mode=O.P_HADAMARD, defect=None) -> dict:
    """What check_update() reads from a device, computed by the float32 numpy oracle from the same state. defect: None or one
    of "drop_row" (the last minibatch row left out of hidden_layer.weight's gradient), "ktail_twice" (the last 64-row K chunk
    of hidden_layer.weight's gradient added twice), "scale_block" (action_values.weight's gradient x (1 + 1e-3)),
    "zero_column" (one column of hidden_layer.weight's gradient zeroed), "norm" (the norm partials 1 % high, and the clip
    taken with that norm) — the optimizer step then runs on the defective gradient / norm, as a device's would."""
    st, ac, rw, ns = batch
    o = O.LearnerOracle.from_state(pre["main"], pre["target"], pre["m"], pre["v"], pre["t"], lr=lr, tau=tau, gamma=gamma,
                                   p_mode=p_mode, dtype=np.float32)
    loss = o.learn(st, ac, rw, ns)
    last = o.last
    g = {k: v.copy() for k, v in last["grads"].items()}
    dz2, a1 = last["inter"]["dz2"], last["fwd"]["a1"]
    f32 = np.float32
    if defect == "drop_row":
        g["hidden_layer.weight"] -= np.outer(dz2[-1], a1[-1]).astype(f32)
    elif defect == "ktail_twice":
        k0 = (dz2.shape[0] - 1) // 64 * 64
        g["hidden_layer.weight"] += (dz2[k0:].T @ a1[k0:]).astype(f32)
    elif defect == "scale_block":
        g["action_values.weight"] *= f32(1 + 1e-3)
    elif defect == "zero_column":
        g["hidden_layer.weight"][:, g["hidden_layer.weight"].shape[1] // 2] = 0
    elif defect is not None:
        assert defect == "norm", defect
    norm = float(f32(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))))
    if defect == "norm":
        norm *= 1.01
    th, tg, m1, v1, t1, _, _ = O.optimizer_step(last["params"], pre["target"], pre["m"], pre["v"], pre["t"], g, lr=lr, tau=tau,
                                                dtype=np.float32, norm=norm if defect == "norm" else None)
    main = dict(th, **{k: o.main[k] for k in ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")})
    target = dict(tg, **{k: o.target[k] for k in ("bn1.running_mean", "bn1.running_var", "bn2.running_mean", "bn2.running_var")})
    return {"q": last["Q"], "loss": loss, "grad": g, "norm": norm, "main": main, "target": target, "m": m1, "v": v1, "t": t1,
            "a1": last["fwd"]["a1"], "a2": last["fwd"]["a2"]}

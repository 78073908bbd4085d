"""
oracle/optim_check.py — TEST INFRASTRUCTURE ONLY. One optimizer step (clip by global norm + Adam + Polyak) on flat
float32 buffers against a float64 statement of naf_algorithm.py:209-213, 217-226, at the level of the C ABI
(naf_grad_norm_partials + naf_adam_polyak_fused), for ANY hyperparameters, optimizer age and buffer length.

check_optimizer_step() is the whole comparison. tests/test_optim_kernels_gpu.py feeds it the HIP kernels,
tests/test_optim_cases_cpu.py feeds it f32_standin() — a float32 numpy restatement of the kernels' arithmetic — to show that
the bounds admit honest float32 and reject planted defects. The two share this file and tests/optim_cases.py so that they
cannot drift apart.

A state is a dict of flat arrays {"theta", "target" (or None: no Polyak), "m", "v"}; the step count t is 1-based (the count
of the step being taken, what *step_dev holds when naf_adam_polyak_fused reads it).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import naf_oracle as O
from .learn_check import Report

U32 = 2.0 ** -24                     # unit roundoff of float32
NORM_CHUNK = 4096                    # NAF_NORM_CHUNK: gradient elements per norm partial
PREFETCHED_PARTIALS = 256            # NAF_MAX_NORM_PARTIALS: partials beyond these are folded by a loop of their own
GRID_SPAN = 4 * 2048 * 256           # elements one trip of adam_block's grid-stride loop covers (float4 x blocks x threads)

# ---- the bounds -----------------------------------------------------------------------------------------------------------
# Errors are counted in units of U32 x a per-element scale:
#     m       K_M  x U32 x (|m'| + |m| + |clip g|)
#     v       K_V  x U32 x |v'|
#     theta   K_TH x U32 x (|theta'| + 8 |theta' - theta|)
#     target  K_TG x U32 x (|target'| + |tau theta'| + |(1 - tau) target| + 8 tau |theta' - theta|)
#             (theta's form with the Polyak terms: the two products and their sum round once each, and the stepped theta
#              enters with weight tau, so its own bound does too)
# MEASURED_* are the largest error / scale of f32_standin() — honest float32 in the kernels' operation order, both with the
# kernel's multiply by 1/sqrt(1 - beta2^t) and with O.adam_step's division by sqrt(1 - beta2^t) — against optimizer_step_f64
# over the whole table of tests/optim_cases.py (tests/test_optim_cases_cpu.py recomputes them and fails if the table has
# outgrown them). K_* = 4 x measured, rounded up: the factor covers a device's different but legal rounding of sqrtf, of the
# division and of the double-to-float conversions of the two bias corrections. They are not tuned on any device result.
# Measured (24 cases x 3 steps x both forms): m 0.954 (n1021_frozen_t1048576_w1), v 6.49 (n1048579_slow_t0_w8),
# theta 25.8 (n2200003_copy_t9_w8), target 17.2 (n2200003_copy_t9_w8).
MEASURED_M, MEASURED_V, MEASURED_TH, MEASURED_TG = 0.954, 6.49, 25.8, 17.2
K_M, K_V, K_TH, K_TG = 4.0, 26.0, 104.0, 69.0
# The norm is not measured but bounded a priori: a partial is a sum of 4096 squares, all >= 0, and an element passes through
# at most 1 (square) + 3 (the float4's adds) + 4 (accumulator) + 6 (wave) + 4 (workgroup) = 18 roundings on its way into it, so
# the partial is within 18 U32 of its exact value, relative, in any legal order; the checker folds the partials in float64
# and the square root halves the relative error. 9 U32 (1 + 18 U32) < 9.001 U32.
K_NORM = 9.001


@dataclass(frozen=True)
class Hyper:
    lr: float = 1e-3
    tau: float = 1e-3
    max_norm: float = 1.0
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    polyak: bool = True              # False: theta_target = NULL


def kernel_scalars(h: Hyper, world: int) -> dict:
    """The float32-rounded scalars the kernel receives through the C ABI, as Python floats."""
    f = lambda x: float(np.float32(x))
    return dict(lr=f(h.lr), beta1=f(h.beta1), beta2=f(h.beta2), eps=f(h.eps), tau=f(h.tau), one_minus_tau=f(1.0 - h.tau),
                max_norm=f(h.max_norm), inv_world=f(1.0 / world))


def optimizer_step_f64(pre: dict, g, hyper: Hyper, t: int, world: int = 1, norm: float | None = None) -> dict:
    """naf_algorithm.py:209-213 (clip_grad_norm_ with its + 1e-6; Adam.step()) and :217-226 (soft_update with the freshly
    stepped parameters) on flat buffers, in float64 from the float32-rounded scalars of kernel_scalars(). g: this rank's
    summed gradient; the clip and the step see g / world. norm: the total norm (of g / world) the clip uses instead of the
    gradient's own — the device's, so that its float32 rounding is checked once and not in every element.
    Returns theta, target, m, v, gs (the clipped averaged gradient), norm (of g / world, always the gradient's own), clip."""
    s = kernel_scalars(hyper, world)
    g = np.asarray(g, np.float64)
    own = float(np.sqrt((g * g).sum())) * s["inv_world"]
    total = own if norm is None else float(norm)
    clipped, _ = O.clip_grad_norm({"g": g * s["inv_world"]}, s["max_norm"])      # (coefficient: min(1, max_norm / (norm + 1e-6)))
    clip = min(1.0, s["max_norm"] / (total + 1e-6))
    gs = clipped["g"] if norm is None else g * s["inv_world"] * clip
    th0, m0, v0 = (np.asarray(pre[k], np.float64) for k in ("theta", "m", "v"))
    th, m, v = O.adam_step(th0, gs, m0, v0, int(t), s["lr"], s["beta1"], s["beta2"], s["eps"])
    tg = None
    if hyper.polyak:
        tg0 = np.asarray(pre["target"], np.float64)
        tg = s["tau"] * th + s["one_minus_tau"] * tg0        # (O.polyak with the kernel's own float32(1 - tau))
    return dict(theta=th, target=tg, m=m, v=v, gs=gs, norm=own, clip=clip)


def check_optimizer_step(pre: dict, dev: dict, g, hyper: Hyper, t: int, world: int = 1, constants=None) -> Report:
    """pre: the buffers before the step (float32). dev: what the two launches left — "theta", "target" (None without Polyak),
    "m", "v", "partials" (the norm partials, all of them) and "t" (the step count after naf_grad_norm_partials).
    g: the gradient both launches read. constants: (k_m, k_v, k_th, k_tg) instead of K_M, K_V, K_TH, K_TG.
    Returns a Report; report.failures is empty when every check holds."""
    k_m, k_v, k_th, k_tg = (K_M, K_V, K_TH, K_TG) if constants is None else constants
    rep = Report()
    s = kernel_scalars(hyper, world)
    g32 = np.asarray(g, np.float32)
    n = g32.size
    parts = np.asarray(dev["partials"], np.float64)
    rep.add("partials", abs(parts.size - (n + NORM_CHUNK - 1) // NORM_CHUNK), 0.5, "number of norm partials")
    norm_dev = float(np.sqrt(parts.sum())) * s["inv_world"]
    want = optimizer_step_f64(pre, g32, hyper, t, world, norm=norm_dev)
    rep.meta.update(clip=want["clip"], norm64=want["norm"], norm_dev=norm_dev)
    rep.add("norm", abs(norm_dev - want["norm"]), K_NORM * U32 * want["norm"], "sqrt(sum partials) / world vs float64")
    rep.add("step", abs(int(dev["t"]) - int(t)), 0.5, "step count")

    th0, m0, v0 = (np.asarray(pre[k], np.float64) for k in ("theta", "m", "v"))
    thd, md, vd = (np.asarray(dev[k], np.float64) for k in ("theta", "m", "v"))
    th, m, v, gs = want["theta"], want["m"], want["v"], want["gs"]
    moved = np.abs(th - th0)
    rep.add("m", np.abs(md - m), k_m * U32 * (np.abs(m) + np.abs(m0) + np.abs(gs)), "adam m")
    rep.add("v", np.abs(vd - v), k_v * U32 * np.abs(v), "adam v")
    rep.add("theta", np.abs(thd - th), k_th * U32 * (np.abs(th) + 8 * moved), "theta")
    # the smallest magnitude float32 has to hold: the table stays clear of subnormals (flushing is out of scope)
    small = [np.abs(x[x != 0]).min() for x in (gs, v, (1.0 - s["beta2"]) * gs * gs) if (x != 0).any()]
    rep.meta["smallest"] = float(min(small)) if small else 1.0

    # padding and Hadamard-dead weights: no gradient, no moments -> nothing moves, and the target is the plain soft update
    dead = (g32 == 0) & (np.asarray(pre["m"]) == 0) & (np.asarray(pre["v"]) == 0)
    rep.meta["dead"] = int(dead.sum())
    for k in ("theta", "m", "v"):
        a, b = np.asarray(dev[k], np.float32)[dead], np.asarray(pre[k], np.float32)[dead]
        rep.add("dead", float((a.view(np.uint32) != b.view(np.uint32)).sum()), 0.5, f"{k} of elements with g = m = v = 0 moved")
    if hyper.polyak:
        tg0 = np.asarray(pre["target"], np.float64)
        tgd = np.asarray(dev["target"], np.float64)
        tg = want["target"]
        rep.add("target", np.abs(tgd - tg),
                k_tg * U32 * (np.abs(tg) + np.abs(s["tau"] * th) + np.abs(s["one_minus_tau"] * tg0) + 8 * s["tau"] * moved), "target")
        exp = O.polyak(np.asarray(pre["target"], np.float32)[dead], np.asarray(pre["theta"], np.float32)[dead], hyper.tau)
        got = np.asarray(dev["target"], np.float32)[dead]
        rep.add("dead", float((got.view(np.uint32) != exp.view(np.uint32)).sum()), 0.5, "target of dead elements is not O.polyak's bits")
    else:
        rep.add("target", 0.0 if dev.get("target") is None else 1.0, 0.5, "a target came back without Polyak")
    return rep


def error_units(rep: Report) -> dict:
    """Largest error / (U32 x scale) of m, v, theta and target in a report made with the default constants: what K_* are
    measured in."""
    return {k: rep.ratios.get(k, 0.0) * c for k, c in (("m", K_M), ("v", K_V), ("theta", K_TH), ("target", K_TG))}


# ---- float32 stand-in of the two kernels ------------------------------------------------------------------------------------
DEFECTS = ("bc_t_minus_1", "bc2_without_sqrt", "eps_before_bc", "polyak_from_old_theta", "tau_swapped", "clip_not_clamped",
           "max_norm_one", "inv_world_dropped", "tail_untouched", "second_trip_untouched", "partials_beyond_256_ignored")


def _tree64(x):
    """sum over the last axis (64 lanes) by halving: a fixed-order lane sum in float32"""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def standin_partials(g: np.ndarray) -> np.ndarray:
    """grad_norm_partials_kernel in float32 numpy: per 4096-element chunk, 256 threads x 4 float4 in its order."""
    f32 = np.float32
    n = g.size
    nb = (n + NORM_CHUNK - 1) // NORM_CHUNK
    x = np.zeros(nb * NORM_CHUNK, f32)
    x[:n] = g
    x = x.reshape(nb, NORM_CHUNK // 1024, 256, 4)
    sq = x * x
    e = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3]          # [nb, 4, 256]
    acc = np.zeros((nb, 256), f32)
    for k in range(e.shape[1]):
        acc = acc + e[:, k]
    w = _tree64(acc.reshape(nb, 4, 64))                                  # [nb, 4 waves]
    s = np.zeros(nb, f32)
    for k in range(4):
        s = s + w[:, k]
    return s.astype(f32)


def _ipow(b: float, t: int) -> float:
    r = 1.0
    while t > 0:
        if t & 1:
            r *= b
        b *= b
        t >>= 1
    return r


def f32_standin(pre: dict, g, hyper: Hyper, t: int, world: int = 1, defect: str | None = None, divide: bool = False) -> dict:
    """What check_optimizer_step() reads from a device, by float32 numpy in the operation order of adam_derive / adam_one
    (csrc/adam_body.h). divide: sqrt(v) / sqrt(bc2) as O.adam_step writes it, not the kernel's multiply by the reciprocal.
    defect: None or one of DEFECTS — a kernel that is wrong in that one way."""
    assert defect is None or defect in DEFECTS, defect
    f32 = np.float32
    s = {k: f32(x) for k, x in kernel_scalars(hyper, world).items()}
    g = np.asarray(g, f32)
    n = g.size
    parts = standin_partials(g)
    # adam_derive: lane-major fold of the partials, 64 lanes
    use = parts[:PREFETCHED_PARTIALS] if defect == "partials_beyond_256_ignored" else parts
    lanes = np.zeros(64 * ((use.size + 63) // 64), f32)
    lanes[:use.size] = use
    lanes = lanes.reshape(-1, 64)
    acc = np.zeros(64, f32)
    for j in range(lanes.shape[0]):
        acc = acc + lanes[j]
    ssum = _tree64(acc)
    inv_world = f32(1.0) if defect == "inv_world_dropped" else s["inv_world"]
    max_norm = f32(1.0) if defect == "max_norm_one" else s["max_norm"]
    total = np.sqrt(ssum, dtype=f32) * inv_world
    clip = max_norm / (total + f32(1e-6))
    if defect != "clip_not_clamped":
        clip = min(f32(1.0), clip)
    clip_scale = f32(clip) * inv_world
    tb = t - 1 if defect == "bc_t_minus_1" else t
    bc1 = 1.0 - _ipow(float(s["beta1"]), tb)
    bc2 = 1.0 - _ipow(float(s["beta2"]), tb)
    with np.errstate(divide="ignore", invalid="ignore"):
        bc1, bc2 = np.float64(bc1), np.float64(bc2)                 # (a zero divides to inf, as on the device)
        step_size = f32(np.float64(s["lr"]) / bc1)
        if defect == "bc2_without_sqrt":
            inv_bc2_sqrt, bc2_sqrt = f32(1.0 / bc2), f32(bc2)
        else:
            inv_bc2_sqrt, bc2_sqrt = f32(1.0 / np.sqrt(bc2)), f32(np.sqrt(bc2))
        th0, m0, v0 = (np.asarray(pre[k], f32) for k in ("theta", "m", "v"))
        gs = g * clip_scale
        m = m0 + (gs - m0) * (f32(1.0) - s["beta1"])
        v = v0 * s["beta2"] + ((f32(1.0) - s["beta2"]) * gs) * gs
        rt = np.sqrt(v)
        if defect == "eps_before_bc":
            denom = (rt + s["eps"]) * inv_bc2_sqrt
        elif divide:
            denom = rt / bc2_sqrt + s["eps"]
        else:
            denom = rt * inv_bc2_sqrt + s["eps"]
        th = th0 - step_size * (m / denom)
        tg = None
        if hyper.polyak:
            tg0 = np.asarray(pre["target"], f32)
            a, b = (s["one_minus_tau"], s["tau"]) if defect == "tau_swapped" else (s["tau"], s["one_minus_tau"])
            tg = a * (th0 if defect == "polyak_from_old_theta" else th) + b * tg0
    out = dict(theta=th, m=m, v=v, target=tg)
    keep = slice(0, 0)
    if defect == "tail_untouched":
        keep = slice(n - n % 4, n)
    elif defect == "second_trip_untouched":
        keep = slice(min(n, GRID_SPAN), n)
    for k, old in (("theta", th0), ("m", m0), ("v", v0)) + ((("target", tg0),) if hyper.polyak else ()):
        out[k] = out[k].astype(f32)
        out[k][keep] = old[keep]
    out.update(partials=parts, t=t)
    return out

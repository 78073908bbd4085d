"""The case table of the optimizer-step checks at the C ABI (tests/test_optim_kernels_gpu.py on naf_grad_norm_partials +
naf_adam_polyak_fused, tests/test_optim_cases_cpu.py on the float32 stand-in of oracle/optim_check.py): buffer lengths where
the kernels keep their edge handling, hyperparameters away from the reference's defaults, and optimizers of every age.

Lengths: 4 and 7 (one float4, with and without the n % 4 tail), 1021, 4096 and 4099 (one norm partial exactly, two with a
tail of 3), 83264 (the reference's parameter count, padded), 1,048,579 (257 norm partials: one beyond the prefetched 256,
covering a tail of 3) and 2,200,003 (538 partials, a tail of 3 and a second trip of the update's grid-stride loop, which
one trip covers up to 2,097,152 elements).
A small cross: every value of every axis occurs, not the full product."""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from oracle.optim_check import Hyper

HYPERS = {
    "default": Hyper(),                                               # the control
    "slow": Hyper(lr=1e-4, tau=0.05, max_norm=0.1),
    "copy": Hyper(lr=3e-2, tau=1.0, max_norm=1e9),                    # never clips; the target becomes the stepped theta
    "frozen": Hyper(tau=0.0, beta1=0.5, beta2=0.9, eps=1e-3),         # the target comes back bit-equal
    "nopolyak": Hyper(polyak=False),                                  # theta_target = NULL
}
NS = (4, 7, 1021, 4096, 4099, 83264, 1_048_579, 2_200_003)
AGES = (0, 1, 9, 999, 6930, 1_048_576)        # beta2^6930 ~ 1e-3 at beta2 = 0.999
WORLDS = (1, 8)
N_STEPS = 3


@dataclass(frozen=True)
class Case:
    n: int
    hyper: str
    t0: int                      # steps already taken; 0 = a new optimizer (zero moments), otherwise aged moments
    gscale: float                # overall gradient scale: puts the clip into either regime
    world: int = 1
    loud_tail: bool = False      # the elements of the last norm partial carry gradients of scale 30 x gscale

    @property
    def name(self):
        return f"n{self.n}_{self.hyper}_t{self.t0}_w{self.world}"


# (norm of the averaged gradient ~ 0.16 sqrt(n) gscale / world)
CASES = [
    Case(4, "default", 0, 1.0),
    Case(4, "copy", 9, 1.0, world=8),
    Case(7, "slow", 1, 1.0),
    Case(7, "frozen", 0, 1e-2, world=8),
    Case(7, "nopolyak", 999, 1.0),
    Case(1021, "default", 6930, 1.0),
    Case(1021, "copy", 0, 1.0, world=8),
    Case(1021, "frozen", 1_048_576, 1.0),
    Case(4096, "slow", 9, 1e-3),
    Case(4096, "nopolyak", 0, 1.0),
    Case(4099, "default", 999, 1e-2),
    Case(4099, "frozen", 6930, 1.0, world=8),
    Case(4099, "copy", 1, 1.0),
    Case(83264, "default", 0, 1.0),
    Case(83264, "slow", 6930, 1.0, world=8),
    Case(83264, "copy", 1_048_576, 1.0),
    Case(83264, "frozen", 9, 1e-3),
    Case(83264, "default", 1, 0.01, world=8),            # the clip idle at world 8: inv_world shows in every element
    Case(83264, "nopolyak", 6930, 1.0),
    Case(1_048_579, "default", 999, 1.0, loud_tail=True),
    Case(1_048_579, "slow", 0, 1.0, world=8, loud_tail=True),
    Case(2_200_003, "default", 6930, 1.0),
    Case(2_200_003, "copy", 9, 1.0, world=8),
    Case(2_200_003, "frozen", 1, 1e-3),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def _rng(case: Case, what: int):
    return np.random.default_rng([zlib.crc32(case.name.encode()), what])


def dead_mask(case: Case) -> np.ndarray:
    """10 % of the elements are padding / Hadamard-dead weights: no gradient ever, no moments."""
    return _rng(case, 100).random(case.n) < 0.1


def initial_state(case: Case) -> dict:
    """theta and target ~ 0.05 N(0, 1), independent. Age 0: zero moments. Aged: v log-uniform in [1e-16, 1e-2],
    m = sqrt(v) U(-1, 1), both 0 on the dead elements; no subnormals."""
    rng = _rng(case, 101)
    n = case.n
    f32 = np.float32
    theta = (0.05 * rng.standard_normal(n)).astype(f32)
    target = (0.05 * rng.standard_normal(n)).astype(f32)
    if case.t0 == 0:
        m, v = np.zeros(n, f32), np.zeros(n, f32)
    else:
        v = np.exp(rng.uniform(np.log(1e-16), np.log(1e-2), n))
        u = rng.uniform(-1.0, 1.0, n)
        u = np.where(np.abs(u) < 1e-6, 1e-6, u)
        m = (np.sqrt(v) * u).astype(f32)
        v = v.astype(f32)
        dead = dead_mask(case)
        m[dead] = 0
        v[dead] = 0
    return dict(theta=theta, target=target, m=m, v=v)


def gradient(case: Case, k: int) -> np.ndarray:
    """This rank's summed gradient of step k: N(0, 1) x a per-element log-uniform scale in [1e-6, 1] x gscale x world, 30 %
    exact zeros (and every dead element). |N| is kept above 1e-3 so that no square lands in the subnormal range."""
    rng = _rng(case, k)
    n = case.n
    z = rng.standard_normal(n)
    z = np.where(np.abs(z) < 1e-3, np.copysign(1e-3, z), z)
    scale = np.exp(rng.uniform(np.log(1e-6), 0.0, n))
    zero = rng.random(n) < 0.3
    if case.loud_tail:
        tail = np.arange(n) >= n - n % 4096
        scale[tail] = 30.0
        zero[tail] = False
    g = z * scale * case.gscale * case.world
    g[zero | dead_mask(case)] = 0.0
    return g.astype(np.float32)

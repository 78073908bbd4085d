"""CPU rehearsal of the optimizer-step check (oracle/optim_check.py) on the float32 numpy stand-in of the two kernels, over
the case table the GPU test runs (tests/optim_cases.py): the bounds admit honest float32 arithmetic — their constants are
4 x what it measures here — and reject a kernel that is wrong in any one of the ways of optim_check.DEFECTS."""
import math

import numpy as np
import pytest

from oracle import optim_check as C
from optim_cases import AGES, CASES, HYPERS, NS, N_STEPS, WORLDS, gradient, initial_state

KEEP_BELOW = 100_000          # the honest chain's states are kept for the defect runs below this length (memory)


def _next(dev, case):
    pre = {k: dev[k] for k in ("theta", "target", "m", "v")}
    if pre["target"] is None:
        pre["target"] = initial_state(case)["target"]
    return pre


@pytest.fixture(scope="module")
def honest():
    """The stand-in over the whole table, teacher-forced on itself: per case the reports, the measured error units (both forms
    of the division by sqrt(1 - beta2^t)) and, for the shorter buffers, the state before each step."""
    out = {}
    for c in CASES:
        h = HYPERS[c.hyper]
        reps, units, pres = [], [], []
        for divide in (False, True):
            pre = initial_state(c)
            for k in range(N_STEPS):
                g, t = gradient(c, k), c.t0 + k + 1
                dev = C.f32_standin(pre, g, h, t, c.world, divide=divide)
                reps.append(C.check_optimizer_step(pre, dev, g, h, t, c.world))
                units.append(C.error_units(reps[-1]))
                if not divide and (k == 0 or c.n < KEEP_BELOW):
                    pres.append(pre)
                pre = _next(dev, c)
        out[c.name] = (reps, units, pres)
    return out


def test_the_table_has_every_value_of_every_axis():
    assert {c.n for c in CASES} == set(NS) and {c.t0 for c in CASES} == set(AGES)
    assert {c.hyper for c in CASES} == set(HYPERS) and {c.world for c in CASES} == set(WORLDS)
    assert len(CASES) <= 36
    # the three paths no smaller buffer reaches
    assert any(c.n % 4 for c in CASES)
    assert any(c.n > C.GRID_SPAN and c.n % 4 for c in CASES)
    assert any(C.PREFETCHED_PARTIALS < (c.n + C.NORM_CHUNK - 1) // C.NORM_CHUNK for c in CASES)
    for c in CASES:
        st = initial_state(c)
        assert (c.t0 == 0) == (not st["m"].any() and not st["v"].any())
        for a in list(st.values()) + [gradient(c, 0)]:
            nz = np.abs(a[a != 0])
            assert a.dtype == np.float32 and (nz.size == 0 or nz.min() >= np.finfo(np.float32).tiny)


def test_float32_standin_passes_the_whole_table(honest):
    clips = []
    for c in CASES:
        reps, _, _ = honest[c.name]
        for k, rep in enumerate(reps):
            assert not rep.failures, f"{c.name} step {k % N_STEPS}:\n  " + "\n  ".join(m for _, m in rep.failures)
            # (flush-to-zero is out of scope: the smallest magnitude float32 has to hold stays 2^10 above its normal range's end)
            assert rep.meta["smallest"] > 1024 * np.finfo(np.float32).tiny, (c.name, rep.meta)
            clips.append(rep.meta["clip"])
    assert any(x < 1.0 for x in clips) and any(x == 1.0 for x in clips)
    assert any(rep.meta["dead"] > 0 for c in CASES for rep in honest[c.name][0])


def test_the_constants_are_four_times_what_float32_measures(honest):
    worst = {}
    for c in CASES:
        for u in honest[c.name][1]:
            for k, x in u.items():
                worst[k] = max(worst.get(k, 0.0), x)
    print("[optim f32 stand-in] largest error / (2^-24 scale):", {k: round(x, 3) for k, x in worst.items()})
    for k, meas, const in (("m", C.MEASURED_M, C.K_M), ("v", C.MEASURED_V, C.K_V), ("theta", C.MEASURED_TH, C.K_TH),
                           ("target", C.MEASURED_TG, C.K_TG)):
        # the recorded figure is this table's (rounded up in its third digit), and the constant is 4 x it, rounded up to an integer
        assert 0.98 * meas <= worst[k] <= meas, (k, worst[k], meas)
        assert const == math.ceil(4 * meas), (k, const)


def _applies(defect, c):
    h = HYPERS[c.hyper]
    return {"tail_untouched": c.n % 4 != 0, "second_trip_untouched": c.n > C.GRID_SPAN,
            "partials_beyond_256_ignored": c.n > C.PREFETCHED_PARTIALS * C.NORM_CHUNK,
            "inv_world_dropped": c.world != 1, "max_norm_one": h.max_norm != 1.0,
            "polyak_from_old_theta": h.polyak, "tau_swapped": h.polyak}.get(defect, True)


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_the_checker_rejects_a_planted_defect(honest, defect):
    """From the honest chain's states: the defective stand-in fails a check that the honest one passed in that same step."""
    caught = []
    for c in sorted(CASES, key=lambda c: c.n):
        if not _applies(defect, c):
            continue
        h = HYPERS[c.hyper]
        reps, _, pres = honest[c.name]
        for k, pre in enumerate(pres):
            g, t = gradient(c, k), c.t0 + k + 1
            rep = C.check_optimizer_step(pre, C.f32_standin(pre, g, h, t, c.world, defect=defect), g, h, t, c.world)
            if rep.failures and not reps[k].failures:
                caught.append((c.name, k, sorted({chk for chk, _ in rep.failures})))
        if len(caught) >= 2:
            break
    print(f"[optim defect] {defect}: {caught}")
    assert caught, f"no case of the table tells {defect} from honest float32"


def test_a_null_target_and_a_frozen_target_are_checked_to_the_bit():
    c = next(c for c in CASES if c.hyper == "frozen" and c.n >= 1021)
    h, pre, g = HYPERS[c.hyper], initial_state(c), gradient(c, 0)
    dev = C.f32_standin(pre, g, h, c.t0 + 1, c.world)
    assert np.array_equal(dev["target"].view(np.uint32), pre["target"].view(np.uint32))       # tau = 0
    c = next(c for c in CASES if c.hyper == "copy" and c.n >= 1021)
    h, pre, g = HYPERS[c.hyper], initial_state(c), gradient(c, 0)
    dev = C.f32_standin(pre, g, h, c.t0 + 1, c.world)
    assert np.array_equal(dev["target"], dev["theta"])                                        # tau = 1
    c = next(c for c in CASES if c.hyper == "nopolyak")
    h, pre, g = HYPERS[c.hyper], initial_state(c), gradient(c, 0)
    dev = C.f32_standin(pre, g, h, c.t0 + 1, c.world)
    assert dev["target"] is None and not C.check_optimizer_step(pre, dev, g, h, c.t0 + 1, c.world).failures
    dev["target"] = pre["target"]
    assert C.check_optimizer_step(pre, dev, g, h, c.t0 + 1, c.world).failed("target")

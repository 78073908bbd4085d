"""CPU rehearsal of the per-launch checks of the row-split learn() chain (oracle/launch_check.py) on its float32 numpy stand-in,
over the case table the GPU test runs (tests/rowsplit_cases.py): every bound admits honest float32 arithmetic, every planted
defect of launch_check.DEFECTS is rejected at the two-net trained state — and the first three of them pass at
learn_cases.init_state, where every whole-update test of the suite starts: the gap these checks close, shown here."""
import numpy as np
import pytest

from learn_cases import init_state
from oracle import launch_check as C
from rowsplit_cases import (BY_NAME, CASES, MAX_DEAD_COLUMNS, MIN_ACTIVE, MAX_ACTIVE, MIN_VNEXT_REL, dims, launch_state, minibatches,
                            vacuity, vacuity_ok)

MAX_AMBIGUOUS = 32            # as tests/test_learn_f64_gpu.py scales it: per update and per 4096 x 256 elements of a layer
# the defects run where they can show: small shapes, two statistics blocks of unequal size, three or more split-K slabs
DEFECT_CASES = ["s21_a6_h256_b16_m1", "s21_a6_h256_b65", "s21_a6_h128_b32_rare", "s21_a6_h256_b1040_rare"]


def most_ambiguous(case):
    return MAX_AMBIGUOUS * max(1.0, case.B * case.H / (4096 * 256))


def _run(case, main, target, defect=None):
    d = dims(case)
    pre = C.stored_state(main, target, d)
    reps = []
    for batch in minibatches(case):
        dev = C.f32_standin(pre, batch, d, defect)
        reps.append(C.check_launches(pre, batch, dev, d))
        pre = dict(pre, bn=dev["bn"], step=dev["step"], flag=dev["flag"])       # (the optimizer step is not these checks' subject)
    return reps


@pytest.fixture(scope="module")
def honest():
    return {c.name: _run(c, *launch_state(c)) for c in CASES}


def test_the_table_reaches_the_branches_it_names():
    """The counts each case's `why` relies on, from chain_plan.plan_chain."""
    want = {   # name: (Bp, nb, nb1, kp, hk_rows, ks_w2, keep_xhat1, H stored, NHP)
        "s21_a6_h256_b16_m1": (16, 1, 1, 24, 16, 1, True, 256, 32), "s21_a6_h256_b17_rare": (32, 1, 1, 24, 16, 1, True, 256, 32),
        "s21_a6_h256_b65": (80, 2, 3, 24, 16, 1, True, 256, 32), "s25_a8_h256_b100_m1": (112, 2, 4, 32, 16, 1, True, 256, 48),
        "s21_a6_h256_b256_rare": (256, 4, 8, 24, 16, 1, True, 256, 32), "s21_a6_h256_b576": (576, 9, 18, 24, 16, 2, False, 256, 32),
        "s21_a6_h256_b1040_rare": (1088, 17, 34, 24, 16, 4, False, 256, 32),
        "s21_a6_h256_b2100_rare": (2112, 33, 66, 24, 32, 6, False, 256, 32), "s27_a9_h256_b64_m1": (64, 1, 2, 32, 16, 1, True, 256, 64),
        "s31_a11_h256_b48": (48, 1, 2, 32, 16, 1, True, 256, 80), "s32_a8_h256_b128_rare": (128, 2, 4, 32, 16, 1, True, 256, 48),
        "s21_a6_h320_b48": (48, 1, 2, 24, 16, 1, True, 512, 32), "s21_a6_h512_b64_m1": (64, 1, 2, 24, 16, 1, True, 512, 32),
        "s21_a6_h128_b32_rare": (32, 1, 1, 24, 16, 1, True, 256, 32)}
    assert set(want) == set(BY_NAME)
    for c in CASES:
        d = dims(c)              # (asserts the row-split chain)
        assert (d.Bp, d.nb, d.nb1, d.kp, d.hk_rows, d.ks_w2, d.keep_xhat1, d.H, d.NHP) == want[c.name], c.name
        assert d.ks_wh == d.ks_w2 and c.why
    assert sum(c.n_upd for c in CASES) == len(CASES) + 1 and BY_NAME["s21_a6_h256_b256_rare"].n_upd == 2
    assert {c.data for c in CASES} == {"plain", "rare"} and {c.p_mode for c in CASES} == {0, 1}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_state_is_not_vacuous(case):
    """The guard of tests/rowsplit_cases.py in float64, and the state's own premises: the two networks differ in every weight and
    no BatchNorm parameter or statistic is at its default."""
    main, target = launch_state(case)
    for batch in minibatches(case):
        v = vacuity(case, main, target, batch)
        assert vacuity_ok(v), (case.name, v, (MIN_ACTIVE, MAX_ACTIVE, MAX_DEAD_COLUMNS, MIN_VNEXT_REL))
    for k, w in main.items():
        if "num_batches" not in k:
            assert (np.asarray(w) != np.asarray(target[k])).all(), k
    for sd in (main, target):
        for b in ("bn1", "bn2"):
            assert (sd[f"{b}.weight"] != 1).all() and (sd[f"{b}.bias"] != 0).all()
            assert (sd[f"{b}.running_mean"] != 0).all() and (sd[f"{b}.running_var"] != 1).all()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_float32_standin_passes_every_check(case, honest):
    for k, rep in enumerate(honest[case.name]):
        assert not rep.failures, f"{case.name} update {k}:\n  " + "\n  ".join(m for _, m in rep.failures)
        assert rep.meta["ambiguous"] <= most_ambiguous(case), (case.name, k, rep.meta["ambiguous"])
        # every check ran (a check that never ran rejects nothing)
        for chk in ("l1.a1", "l1.wc", "l2.g2", "l2.sum", "l2.m2", "l3.a2", "l3.q", "l3.loss", "l3.dv", "l3.dmu", "l3.dl", "l3.dy2",
                    "l3.bw2", "l4.g2", "l4.be2", "l4.slab_w2", "l4.slab_wh", "l4.bw1", "l4.dw1", "l5.w1", "l5.g1", "l5.be1", "l5.bias0",
                    "l5.slabs", "l5.sumsq", "l5.step", "l5.flag", "l5b.W1", "l5b.g1", "l5b.be1"):
            assert chk in rep.ratios, (case.name, chk)
        assert ("l1.xh1" in rep.ratios) == dims(case).keep_xhat1
        assert ("pad_cols" in rep.ratios) == (case.H in (128, 320))


def test_measured_constant_covers_the_table(honest):
    """launch_check.MEASURED_FINISH_B is the float32 stand-in's largest relative error in check (b) over the table (the bound is 8 x
    it); a table that has outgrown it fails here, not on a device."""
    worst = {}
    for name, reps in honest.items():
        for rep in reps:
            for k, v in rep.meta["finish_b"].items():
                if v > worst.get(k, (0.0,))[0]:
                    worst[k] = (v, name)
    print("[launch] check (b), float32 stand-in against float64: " + ", ".join(f"{k} {v:.3g} ({n})" for k, (v, n) in sorted(worst.items())))
    top = max(v for v, _ in worst.values())
    assert top <= C.MEASURED_FINISH_B, worst
    assert top >= 0.5 * C.MEASURED_FINISH_B, ("the constant is stale: measure again", worst)
    assert C.FINISH_B_RTOL == 8 * C.MEASURED_FINISH_B


@pytest.mark.parametrize("defect", C.DEFECTS)
def test_planted_defect_is_rejected(defect):
    caught = {}
    for name in DEFECT_CASES:
        case = BY_NAME[name]
        rep = _run(case, *launch_state(case), defect=defect)[0]
        if rep.failures:
            caught[name] = sorted({c for c, _ in rep.failures})
    print(f"[launch] {defect}: rejected by {caught}")
    assert caught, defect
    # where the defect sits is where it shows: the launch's own check, not only a later one
    first = {"target_bn2_from_main": "l3.", "target_w2_from_main": "l2.g2", "mask_no_beta1": "l4.bw1", "k1_no_gamma": "l4.slab_w2",
             "biased_running_var": "l1.rv", "momentum_on_old": "l1.rm", "target_stats_in_main_slots": "l1.rm",
             "batch_mean_partials": "l2.m2", "dw1_no_invstd": "l5.w1", "slabs_reversed": "l5.slabs"}[defect]
    assert any(c.startswith(first) for cs in caught.values() for c in cs), (defect, caught)


@pytest.mark.parametrize("defect", C.ADMITTED_AT_INIT)
def test_defect_passes_at_the_init_state(defect):
    """At learn_cases.init_state — BatchNorm weight 1, bias 0, the target loaded from the main network's state dict — the same
    defect changes nothing any check can see: no test that starts there can reject it."""
    for name in DEFECT_CASES:
        case = BY_NAME[name]
        sd = init_state(case)
        rep = _run(case, sd, sd, defect=defect)[0]
        assert not rep.failures, (defect, name, rep.failures[:3])
        assert _run(case, *launch_state(case), defect=defect)[0].failures, (defect, name)

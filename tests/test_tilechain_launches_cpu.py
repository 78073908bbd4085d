"""CPU rehearsal of the per-launch checks of the column-tile and the unfused learn() chains (oracle/launch_check.py,
check_tile_launches) on their float32 numpy stand-in, over the case table the GPU test runs (tests/tilechain_cases.py): every bound
admits honest float32 arithmetic, every planted defect of launch_check.TILE_DEFECTS is rejected by the check of the launch it sits in
at the two-net trained state — and the first six of them pass at learn_cases.init_state, where every whole-update test of the suite
starts: the gap these checks close, shown here."""
import numpy as np
import pytest

from learn_cases import init_state
from oracle import launch_check as C
from rowsplit_cases import launch_state
from tilechain_cases import (ALL4, BY_NAME, CASES, MAX_ACTIVE, MAX_DEAD_COLUMNS, MIN_ACTIVE, MIN_VNEXT_REL, VALUE_SCALE, dims, minibatches,
                             plan_of, tile_state, vacuity, vacuity_ok)

MAX_AMBIGUOUS = 32            # as tests/test_learn_f64_gpu.py scales it: per update, per layer and per 4096 x 256 elements
# the defects run where they can show: the split-K heads at both slab counts, the heads GEMM, torch's layer 1 and dA2, a last
# row phase of one row on the 8 x 128 tile and in the streamed form, the wide head with its scaled value row
DEFECT_CASES = ["s21_a6_h256_b9", "s21_a6_h128_b48_cols_nopad", "s21_a6_h200_b100_nopad", "s40_a4_h256_b32_rare",
                "s21_a6_h256_b513_rare_unf", "s21_a6_h256_b2049_rare_unf", "s73_a32_h256_b48_m1"]
# the check of the launch each defect sits in
FIRST = {"target_bn2_from_main": ("f2.a2",), "target_w2_from_main": ("g2.g2",), "target_vrow_from_main": ("f2.vnext", "f2.gh"),
         "mask_no_beta1": ("b1.",), "mask_no_beta2": ("b2.",), "vnext_from_state": ("f1.a1", "f1.g1"), "k1_no_gamma": ("b2.dz2",),
         "bn2_stats_in_layer1_slots": ("f2.rm",), "target_stats_in_main_slots": ("f1.rm",), "biased_running_var": ("f1.rv",),
         "momentum_on_old": ("f1.rm",), "gwh_no_bias_column": ("gb.gwh",), "slab_twice": ("hd.q",), "last_phase_dropped": ("f1.mean",)}


def most_ambiguous(case):
    return 2 * MAX_AMBIGUOUS * max(1.0, case.B * case.H / (4096 * 256))


def applies(defect, case):
    """slab_twice needs the split-K heads; the last row phase is a partial pass only where the batch is no multiple of the phases;
    the biased variance moves running_var by momentum / (B - 1) of the batch variance, which the suite's RV_RTOL resolves at small
    batches only (taken here with a factor 2 in hand: B <= 500)"""
    if defect == "biased_running_var":
        return C.BN_MOMENTUM / (case.B - 1) > 2 * C.RV_RTOL
    if defect == "slab_twice":
        return "s3" not in case.drop
    if defect == "last_phase_dropped":
        return case.B % C.bn_row_phases(case.B) != 0
    return True


def _run(case, main, target, defect=None):
    d = dims(case)
    pre = C.stored_state(main, target, d)
    reps = []
    for batch in minibatches(case):
        dev = C.f32_standin_tiles(pre, batch, d, defect)
        reps.append(C.check_tile_launches(pre, batch, dev, d))
        pre = dict(pre, bn=dev["bn"], step=dev["step"])       # (the optimizer step is not these checks' subject)
    return reps


@pytest.fixture(scope="module")
def honest():
    return {c.name: _run(c, *tile_state(c)) for c in CASES}


def test_the_table_reaches_the_branches_it_names():
    """Chain, tags, slab count of the split-K heads and fold_norm of every case, from chain_plan.plan_chain."""
    want = {   # name: (chain, tags, n_slabs, fold_norm, H stored, NHP)
        "s21_a6_h256_b2": ("columns", "l1 b2 s3", 32, False, 256, 32), "s21_a6_h256_b9": ("columns", "l1 b2 s3", 32, False, 256, 32),
        "s21_a6_h256_b15_m1_rare": ("columns", "l1 b2 s3", 32, False, 256, 32),
        "s21_a6_h256_b16_cols": ("columns", "l1 b2 gb s3", 32, True, 256, 32),
        "s21_a6_h256_b512_m1_rare_cols": ("columns", "l1 b2 gb s3", 32, True, 256, 32),
        "s26_a8_h256_b256_m1_cols": ("columns", "l1 b2 gb s3", 32, True, 256, 48),
        "s26_a8_h256_b272_m1_cols": ("columns", "b2 gb s3", 32, False, 256, 48),
        "s40_a4_h256_b32_rare": ("columns", "b2 gb s3", 32, False, 256, 16), "s11_a1_h256_b64_m1_cols": ("columns", "l1 b2 gb s3", 32, True, 256, 16),
        "s21_a6_h128_b48_cols_nopad": ("columns", "l1 b2 gb s3", 16, True, 128, 32),
        "s21_a6_h200_b100_nopad": ("columns", "l1 b2", None, False, 200, 32), "s21_a6_h640_b32": ("columns", "l1 b2 gb", None, True, 640, 32),
        "s21_a6_h256_b64_m1_unf": ("unfused", "gb", None, False, 256, 32), "s21_a6_h256_b513_rare_unf": ("unfused", "", None, False, 256, 32),
        "s21_a6_h256_b528_unf": ("unfused", "gb", None, False, 256, 32), "s21_a6_h256_b2049_rare_unf": ("unfused", "", None, False, 256, 32),
        "s21_a6_h256_b2064_m1_unf": ("unfused", "gb", None, False, 256, 32), "s30_a12_h256_b32_m1": ("unfused", "gb", None, False, 256, 96),
        "s43_a17_h256_b33_rare": ("unfused", "", None, False, 256, 176), "s75_a33_h256_b16": ("unfused", "gb", None, False, 256, 608),
        "s73_a32_h256_b48_m1": ("unfused", "gb", None, False, 256, 576), "s137_a64_h256_b32": ("unfused", "gb", None, False, 256, 2160)}
    assert set(want) == set(BY_NAME) and len(CASES) == 22
    for c in CASES:
        plan, d = plan_of(c), dims(c)
        assert (plan.chain, " ".join(t for t in ("l1", "b2", "gb", "s3") if t in plan.fuse), plan.n_slabs, plan.fold_norm, d.H,
                d.NHP) == want[c.name], c.name
        assert plan.chain == c.chain and plan.fuse == ALL4 - c.drop and c.why and plan.Bp == c.B and d.h == d.H
        assert d.fuse == plan.fuse and d.n_slabs == plan.n_slabs and d.fold_norm == plan.fold_norm
    assert sum(c.n_upd for c in CASES) == len(CASES) + 1 and BY_NAME["s21_a6_h256_b64_m1_unf"].n_upd == 2
    assert {c.data for c in CASES} == {"plain", "rare"} and {c.p_mode for c in CASES} == {0, 1}
    assert max(c.B for c in CASES) == 2064 and min(c.B for c in CASES) == 2


def test_the_batchnorm_form_each_size_takes():
    """csrc/bn_relu.hip's rule restated (BN_DISPATCH, BN_MAX_B): 8 x 64 row phases up to B = 512, 8 x 128 up to 2048 with the rows held
    in registers, streamed beyond. The unfused cases sit on both sides of both thresholds; 513 and 2049 leave one row in the last pass."""
    def form(B):
        return "8x64" if B <= 512 else ("8x128" if B <= 16 * 128 else "streamed")
    got = {c.B: form(c.B) for c in CASES if c.chain == "unfused" and c.A == 6}
    assert got == {64: "8x64", 513: "8x128", 528: "8x128", 2049: "streamed", 2064: "streamed"}
    for B in got:
        assert C.bn_row_phases(B) == (64 if got[B] == "8x64" else 128)
    assert 513 % 128 == 1 and 2049 % 128 == 1
    # the column-tile kernels hold ceil(B / 64) <= 8 rows per thread (fused_layers.hip): the chain ends at 512
    assert max(c.B for c in CASES if c.chain == "columns") == 512 and all(plan_of(c).chain == "columns" for c in CASES if c.chain == "columns")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_state_is_not_vacuous(case):
    """The guard of tests/rowsplit_cases.py in float64, bounds unchanged, and the state's own premises."""
    main, target = tile_state(case)
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


def test_value_scales_are_the_smallest():
    """Each entry of VALUE_SCALE is the smallest power of two at which float64 alone meets the guard: half of it does not."""
    assert (MIN_ACTIVE, MAX_ACTIVE, MAX_DEAD_COLUMNS, MIN_VNEXT_REL) == (0.10, 0.90, 0.05, 0.1)
    for name, scale in VALUE_SCALE.items():
        case = BY_NAME[name]
        assert scale in (2.0, 4.0, 8.0)
        half = launch_state(case, value_scale=scale / 2)
        assert not all(vacuity_ok(vacuity(case, *half, b)) for b in minibatches(case)), name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_float32_standin_passes_every_check(case, honest):
    tags = ALL4 - case.drop
    for k, rep in enumerate(honest[case.name]):
        assert not rep.failures, f"{case.name} update {k}:\n  " + "\n  ".join(m for _, m in rep.failures)
        assert rep.meta["ambiguous"] <= most_ambiguous(case), (case.name, k, rep.meta["ambiguous"])
        # every check ran (a check that never ran rejects nothing), and the optional ones exactly where their launch did
        for chk in ("f1.a1", "f1.mean", "f1.invstd", "f1.rm", "f1.rv", "f1.mask", "g2.g2", "f2.a2", "f2.mean", "f2.invstd", "f2.rm", "f2.rv",
                    "f2.mask", "f2.ones", "hd.q", "hd.loss", "hd.dv", "hd.dmu", "hd.dl", "hd.pad", "b2.dz2", "b2.g2", "b2.be2", "b2.bias0",
                    "gb.gwh", "gb.gw2", "gb.da1", "b1.gw1", "b1.g1", "b1.be1", "b1.bias0", "nm.sumsq", "nm.step"):
            assert chk in rep.ratios, (case.name, chk)
        assert ("f1.g1" in rep.ratios) == ("b1.dz1" in rep.ratios) == ("l1" not in tags)
        assert ("f2.heads" in rep.ratios) == ("f2.vnext" in rep.ratios) == ("s3" in tags) and ("f2.gh" in rep.ratios) == ("s3" not in tags)
        assert ("b2.da2" in rep.ratios) == ("b2" not in tags)
        assert "pad_cols" not in rep.ratios          # (no case of this table is stored padded)


def test_no_bound_of_these_checks_is_measured(honest):
    """Every tolerance of check_tile_launches follows from rule (1) or (2) of launch_check's header: the module has no measured
    constant for it, and the honest float32 stand-in stays below half of every bound over the whole table — a derived worst-case
    bound that honest arithmetic nearly fills would be a sign that an n or c is short."""
    worst = {}
    for name, reps in honest.items():
        for rep in reps:
            for k, r in rep.ratios.items():
                if r > worst.get(k, (0.0,))[0]:
                    worst[k] = (r, name)
    for k, (r, name) in sorted(worst.items()):
        print(f"[tiles] {k:10s} float32 stand-in, largest error / tolerance {r:.3g} ({name})")
    assert C.C_DZ == 8 and not [n for n in dir(C) if n.startswith("MEASURED_") and n != "MEASURED_FINISH_B"]
    assert max(r for r, _ in worst.values()) <= 0.5, worst


@pytest.mark.parametrize("defect", C.TILE_DEFECTS)
def test_planted_defect_is_rejected(defect):
    """Wherever the defect applies it is rejected, and by the check of the launch it sits in, not only by a later one."""
    ran = 0
    for name in DEFECT_CASES:
        case = BY_NAME[name]
        if not applies(defect, case):
            continue
        ran += 1
        rep = _run(case, *tile_state(case), defect=defect)[0]
        caught = sorted({c for c, _ in rep.failures})
        print(f"[tiles] {defect} at {name}: rejected by {caught}")
        assert any(c.startswith(f) for c in caught for f in FIRST[defect]), (defect, name, caught)
    assert ran >= 2, defect


@pytest.mark.parametrize("defect", C.TILE_DEFECTS)
def test_which_defects_pass_at_the_init_state(defect):
    """At learn_cases.init_state — BatchNorm weight 1, bias 0, the target loaded from the main network's state dict — the defects of
    TILE_ADMITTED_AT_INIT change nothing any check can see: no test that starts there can reject them. Every other one is rejected
    there too (vnext_from_state among them: state and next_state differ whatever the networks hold)."""
    assert C.TILE_ADMITTED_AT_INIT == ("target_bn2_from_main", "target_w2_from_main", "target_vrow_from_main", "mask_no_beta1",
                                       "mask_no_beta2", "k1_no_gamma")
    for name in DEFECT_CASES:
        case = BY_NAME[name]
        if not applies(defect, case):
            continue
        sd = init_state(case)
        rep = _run(case, sd, sd, defect=defect)[0]
        if defect in C.TILE_ADMITTED_AT_INIT:
            assert not rep.failures, (defect, name, rep.failures[:3])
        else:
            assert rep.failures, (defect, name)

"""GPU: every launch of the row-split learn() chain (csrc/big_batch.hip, the prologue and epilogue of csrc/gemm_bundle.hip, the
finish launch) against float64 computed from the device values that launch read, at a state where main and target network
differ in every weight and no BatchNorm parameter or running statistic is at its default (tests/rowsplit_cases.py). After one
Learner.learn_rows() every intermediate is still in the learner's buffers; oracle/launch_check.check_launches holds each to its
launch's contract (include/naf_hip.h). tests/test_rowsplit_launches_cpu.py runs the same checker on a float32 numpy stand-in: the
bounds admit honest float32 arithmetic and reject the planted defects, three of which no test that starts at the init state can see."""
import numpy as np
import pytest
import torch

from learn_cases import transitions
from oracle import launch_check as C
from oracle import naf_oracle as O
from rowsplit_cases import CASES, dims, launch_state

pytestmark = pytest.mark.gpu

MAX_AMBIGUOUS = 32          # as tests/test_learn_f64_gpu.py scales it: per update and per 4096 x 256 elements of a layer
_RATIOS = {}                # check -> (largest error / tolerance, case, update)
_SEEN = {}                  # case -> [ambiguous elements] per update


def _np(t):
    return t.detach().cpu().numpy().copy()


def _pre(L):
    """What the launches of the next update will read."""
    return {"net": [{k: _np(L.lay.view(L.theta2[n], k)) for k in C.PARAMS} for n in (0, 1)], "bn": _np(L.bn_stats),
            "step": int(L.step_live.item()), "flag": int(L.bb_fold_flag.item())}


def _dev(L, lp):
    """What the update left in the learner's buffers."""
    B = L.B
    return {"A1": _np(L.A1), "XH1": _np(L.XH1) if L.XH1 is not None else None, "save_mean": _np(L.save_mean),
            "save_invstd": _np(L.save_invstd), "bn": _np(L.bn_stats), "mom": _np(L.bb_mom), "wc": _np(L.bb_wc), "G2": _np(L.G2),
            "st2": _np(L.bb_st2), "A2": _np(L.A2[0]), "q": _np(L.q_out[:B]), "loss": float(lp.double().sum()), "dH": _np(L.dH),
            "dY2": _np(L.dZ2), "bw2": _np(L.bb_bw2), "bw1": _np(L.bb_bw1), "dw1": _np(L.bb_dw1), "slab_w2": _np(L.bb_slab_w2),
            "slab_wh": _np(L.bb_slab_wh), "grad": {k: _np(L.lay.view(L.grad, k)) for k in C.PARAMS},
            "sumsq": float(L.partials[:L.n_partials].double().sum()), "step": int(L.step_live.item()),
            "flag": int(L.bb_fold_flag.item())}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_launch_vs_f64_from_its_own_inputs(case, monkeypatch):
    monkeypatch.delenv("NAF_FUSE", raising=False)
    monkeypatch.delenv("NAF_DEFER_ADAM", raising=False)
    from robotic_manipulator_rloa_amd.learner import Learner
    main, target = launch_state(case)
    st, ac, rw, ns, dn = transitions(case)
    L = Learner(case.S, case.A, case.H, case.B, 1e-3, 1e-3, 0.99, torch.device("cuda"), p_mode=case.p_mode)
    L.load_params(0, main)
    L.load_params(1, target)
    assert L.chain == "rows", (case.name, case.why, L.chain)
    d = C.Dims.of(L.plan, L.lay, case.B, case.p_mode, L.gamma)
    assert d == dims(case)
    B = case.B
    rows = torch.from_numpy(O.pack_rows(st, ac, rw, ns, dn, L.lay.row_floats)).cuda()
    lp = torch.zeros(case.n_upd, L.n_loss_wg, device="cuda")
    seen = _SEEN.setdefault(case.name, [])
    for k in range(case.n_upd):
        sl = slice(k * B, (k + 1) * B)
        torch.cuda.synchronize()
        pre = _pre(L)
        if k == 0:
            # the learner stores the two state dicts as the CPU rehearsal assumed (launch_check.stored_state), to the bit
            ref = C.stored_state(main, target, d)
            assert all(np.array_equal(pre["net"][n][p], ref["net"][n][p]) for n in (0, 1) for p in C.PARAMS)
            assert np.array_equal(pre["bn"], ref["bn"]) and (pre["step"], pre["flag"]) == (ref["step"], ref["flag"])
        L.learn_rows(rows[sl], lp[k])
        torch.cuda.synchronize()
        dev = _dev(L, lp[k])
        rep = C.check_launches(pre, (st[sl], ac[sl], rw[sl], ns[sl]), dev, d)
        seen.append(rep.meta["ambiguous"])
        for chk, r in rep.ratios.items():
            if r > _RATIOS.get(chk, (-1.0,))[0]:
                _RATIOS[chk] = (r, case.name, k)
        assert not rep.failures, f"{case.name} ({case.why}) update {k}:\n  " + "\n  ".join(m for _, m in rep.failures)
        assert rep.meta["ambiguous"] <= MAX_AMBIGUOUS * max(1.0, case.B * case.H / (4096 * 256)), (case.name, k, rep.meta)
    if L.lay.H != L.lay.H_ref:
        # the gaps and pad regions of the flat gradient (a layer stored zero-padded) stay exactly zero
        mask = torch.ones(L.lay.P, dtype=torch.bool, device="cuda")
        for v in L.lay.param_views(torch.arange(L.lay.P, device="cuda", dtype=torch.float32)).values():
            mask[v.reshape(-1).long()] = False
        assert (L.grad[mask] == 0).all()


def test_zz_largest_error_over_tolerance_per_check():
    """Runs after the table (file order): prints the largest error / tolerance of every check and the case that had it."""
    for chk, (r, name, k) in sorted(_RATIOS.items()):
        print(f"[launch] {chk:12s} largest error / tolerance {r:.3g} ({name}, update {k})")
    updates = [u for v in _SEEN.values() for u in v]
    print(f"[launch] updates {len(updates)}, layer-1 ReLU elements within rounding of 0: {sum(updates)} (most in one update {max(updates, default=0)})")
    assert all(r <= 1.0 for r, _, _ in _RATIOS.values())

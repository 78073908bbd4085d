"""GPU: every learn() update of the three chains, teacher-forced against a float64 oracle at the shapes where their edge
handling lives (tests/learn_cases.py). Before each update the learner's whole state is read back and seeds the oracle, so
errors never compound; oracle/learn_check.check_update then pins the forward (Q, loss, BatchNorm running statistics), the
gradient before the clip block by block (with the slack of the ReLU elements within float32 rounding of 0), the folded norm
partials, and the optimizer step (clip + Adam + Polyak) on the learner's own gradient. test_oracle_golden.py runs the same checker
on the float32 numpy oracle: the tolerances admit honest float32 arithmetic and reject planted defects."""
import warnings

import numpy as np
import pytest
import torch

from oracle import learn_check as C
from oracle import naf_oracle as O
from learn_cases import CASES, init_state, transitions

pytestmark = pytest.mark.gpu

ROWS, COLUMNS = {"bb", "gb", "hk", "ep", "s2"}, {"l1", "b2", "gb", "s3"}
# ReLU elements within float32 rounding of 0 (relu_kink_tau), per update and per 4096 x 256 elements of a layer: the threshold
# stays narrow. The slack itself covers only those the learner masked the other way (its A1 / A2 against the oracle's y).
MAX_AMBIGUOUS = 32
MAX_FLIPPED = 4


def _most_ambiguous(case):
    return MAX_AMBIGUOUS * max(1.0, case.B * case.H / (4096 * 256))
_SEEN = {}                  # case -> [(clip coefficient, ambiguous count)] per update
_RATIOS = {}                # check -> (largest error / tolerance, case, update)


def _state(L):
    lay = L.lay
    out = {}
    for net, name in ((0, "main"), (1, "target")):
        sd = {k: v.detach().cpu().numpy().copy() for k, v in lay.param_views(L.theta2[net]).items()}
        sd.update({k: v.cpu().numpy().copy() for k, v in L.bn_views(net).items()})
        out[name] = sd
    out["m"] = {k: v.cpu().numpy().copy() for k, v in lay.param_views(L.adam_m).items()}
    out["v"] = {k: v.cpu().numpy().copy() for k, v in lay.param_views(L.adam_v).items()}
    out["t"] = int(L.step_dev.item())
    return out


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_learn_update_vs_f64_oracle(case, monkeypatch):
    monkeypatch.delenv("NAF_FUSE", raising=False)
    monkeypatch.delenv("NAF_DEFER_ADAM", raising=False)
    from robotic_manipulator_rloa_amd.learner import Learner
    sd = init_state(case)
    st, ac, rw, ns, dn = transitions(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (the unfused chain beyond B = 512 / 8 joints says so)
        L = Learner(case.S, case.A, case.H, case.B, 1e-3, 1e-3, 0.99, torch.device("cuda"), p_mode=case.p_mode,
                    fuse=case.fuse, pad_layer=case.pad)
    L.load_params(0, sd)
    L.load_params(1, sd)
    assert L.chain == case.chain, (case.name, L.chain)
    if case.chain == "rows":
        assert L.fuse == ROWS
    elif case.chain == "columns":
        assert L.fuse == COLUMNS - case.drop
    else:
        assert "bb" not in L.fuse and not (L.fuse & {"l1", "b2", "s3"})
    B, h = case.B, L.lay.H_ref
    rows = torch.from_numpy(O.pack_rows(st, ac, rw, ns, dn, L.lay.row_floats)).cuda()
    lp = torch.zeros(case.n_upd, L.n_loss_wg, device="cuda")
    seen = _SEEN.setdefault(case.name, [])
    for k in range(case.n_upd):
        sl = slice(k * B, (k + 1) * B)
        torch.cuda.synchronize()
        pre = _state(L)
        L.learn_rows(rows[sl], lp[k])
        torch.cuda.synchronize()
        dev = _state(L)
        dev.update(q=L.q_out[:B].cpu().numpy(), loss=float(lp[k].double().sum()),
                   grad={kk: v.cpu().numpy() for kk, v in L.lay.param_views(L.grad).items()},
                   norm=float(np.sqrt(L.partials[:L.n_partials].double().sum().item())),
                   a1=L.A1[0, :B, :h].cpu().numpy(), a2=L.A2[0, :B, :h].cpu().numpy())
        rep = C.check_update(pre, (st[sl], ac[sl], rw[sl], ns[sl]), dev, p_mode=case.p_mode)
        seen.append((rep.meta["clip"], rep.meta["ambiguous"] <= _most_ambiguous(case), rep.meta["flipped"]))
        for chk, r in rep.ratios.items():
            if r > _RATIOS.get(chk, (-1.0,))[0]:
                _RATIOS[chk] = (r, case.name, k)
        assert not rep.failures, f"{case.name} ({case.why}) update {k}:\n  " + "\n  ".join(m for _, m in rep.failures)
        assert rep.meta["ambiguous"] <= _most_ambiguous(case) and rep.meta["flipped"] <= MAX_FLIPPED, (case.name, k, rep.meta)
    if L.lay.H != h:
        # pad regions of the flat buffers (a layer stored zero-padded) stay exactly zero
        mask = torch.ones(L.lay.P, dtype=torch.bool, device="cuda")
        for v in L.lay.param_views(torch.arange(L.lay.P, device="cuda", dtype=torch.float32)).values():
            mask[v.reshape(-1).long()] = False
        for buf in (L.grad, L.theta2[0], L.theta2[1], L.adam_m, L.adam_v):
            assert (buf[mask] == 0).all()


def test_zz_the_table_covered_both_clip_regimes_and_few_kinks():
    """Runs after the table (file order): the clip was active (norm > 1) and inactive somewhere, and no update had more
    ReLU elements within rounding of 0 or masked the other way than the bounds above. Prints the largest error ratio of
    every check."""
    for chk, (r, name, k) in sorted(_RATIOS.items()):
        print(f"[f64] {chk:10s} largest error / tolerance {r:.3g} ({name}, update {k})")
    updates = [u for v in _SEEN.values() for u in v]
    print(f"[f64] updates {len(updates)}, clip active in {sum(c < 1.0 for c, _, _ in updates)}, masks flipped "
          f"{sum(f for _, _, f in updates)}")
    assert all(few and f <= MAX_FLIPPED for _, few, f in updates)
    if len(_SEEN) == len(CASES):
        assert any(c < 1.0 for c, _, _ in updates) and any(c == 1.0 for c, _, _ in updates)

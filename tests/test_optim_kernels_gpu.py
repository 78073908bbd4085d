"""GPU: the optimizer and TD-target kernels away from the reference's default values, through the C ABI.

test_optimizer_step_vs_f64_oracle   naf_grad_norm_partials + naf_adam_polyak_fused over tests/optim_cases.py: five sets of
                                    hyperparameters, optimizers aged 0 .. 1M steps with moments spread over 14 decades, buffer
                                    lengths with an n % 4 tail, beyond 256 norm partials and beyond one trip of the update's
                                    grid-stride loop — every element against float64 (oracle/optim_check.py, whose bounds
                                    tests/test_optim_cases_cpu.py rehearses on a float32 stand-in with planted defects).
test_polyak_bit_exact_any_tau       naf_polyak_update == O.polyak in float32, to the bit.
test_td_target_follows_gamma_and_strides, test_first_update_loss_follows_gamma
                                    y = r + gamma V' at other gammas and at the strides the learner passes."""
import warnings

import numpy as np
import pytest
import torch

from oracle import naf_oracle as O
from oracle import optim_check as C
from learn_cases import Case as LearnCase, init_state, transitions
from optim_cases import CASES, HYPERS, N_STEPS, gradient, initial_state

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 8                      # floats behind every buffer, filled with SENTINEL: nothing may be written there
_RATIOS = {}                 # check -> (largest error / tolerance, case, step)
_CLIPS = {}                  # case -> [clip coefficient per step]


@pytest.fixture(scope="module")
def lib():
    from robotic_manipulator_rloa_amd import _lib
    _lib.require_gpu()
    return _lib.load(allow_build=False)


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to("cuda", dtype)


def padded(x, n):
    """x (n floats) on the device with PAD sentinels behind it"""
    d = torch.full((n + PAD,), SENTINEL, device="cuda")
    d[:n] = dev(x)
    return d


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------
# clip + Adam + Polyak
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_optimizer_step_vs_f64_oracle(lib, case):
    """Three consecutive steps, teacher-forced: the buffers are read back before each step and seed the float64 oracle, so
    nothing compounds. Step count, number of norm partials and everything behind the buffers' ends are pinned exactly."""
    h, n, world = HYPERS[case.hyper], case.n, case.world
    init = initial_state(case)
    buf = {k: padded(init[k], n) for k in ("theta", "target", "m", "v")}
    nparts = (n + C.NORM_CHUNK - 1) // C.NORM_CHUNK
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in range(N_STEPS):
        t0 = case.t0 + k
        pre = {name: b[:n].cpu().numpy() for name, b in buf.items()}
        g = gradient(case, k)
        gd = padded(g, n)
        parts = torch.full((nparts + PAD,), SENTINEL, device="cuda")
        step.fill_(t0)
        assert lib.naf_grad_norm_partials(gd.data_ptr(), n, parts.data_ptr(), step.data_ptr(), st()) == 0
        assert lib.naf_adam_polyak_fused(buf["theta"].data_ptr(), gd.data_ptr(), buf["m"].data_ptr(), buf["v"].data_ptr(),
                                         buf["target"].data_ptr() if h.polyak else None, parts.data_ptr(), nparts, h.max_norm,
                                         h.lr, h.beta1, h.beta2, h.eps, h.tau, float(1.0 - h.tau), step.data_ptr(), 1.0 / world,
                                         n, st()) == 0
        torch.cuda.synchronize()
        assert int(step.item()) == t0 + 1
        pn = parts.cpu().numpy()
        assert (pn[nparts:] == SENTINEL).all() and (pn[:nparts] != SENTINEL).all(), "norm partials: not exactly ceil(n / 4096)"
        for name, b in list(buf.items()) + [("grad", gd)]:
            assert (b[n:] == SENTINEL).all(), f"{name}: written beyond n"
        assert np.array_equal(gd[:n].cpu().numpy(), g)
        out = {name: b[:n].cpu().numpy() for name, b in buf.items()}
        if not h.polyak:
            assert np.array_equal(bits(out["target"]), bits(pre["target"])), "a target that was not passed was written"
            out["target"] = None
        out.update(partials=pn[:nparts], t=int(step.item()))
        rep = C.check_optimizer_step(pre, out, g, h, t0 + 1, world)
        for chk, r in rep.ratios.items():
            if r > _RATIOS.get(chk, (-1.0,))[0]:
                _RATIOS[chk] = (r, case.name, k)
        _CLIPS.setdefault(case.name, []).append(rep.meta["clip"])
        assert not rep.failures, f"{case.name} step {k}:\n  " + "\n  ".join(m for _, m in rep.failures)
        if h.polyak and h.tau == 0.0:
            assert np.array_equal(bits(out["target"]), bits(pre["target"])), "tau = 0 moved the target"
        if h.polyak and h.tau == 1.0:
            assert np.array_equal(bits(out["target"]), bits(out["theta"])), "tau = 1: the target is not the stepped theta"


def test_zz_the_optimizer_table_covered_both_clip_regimes():
    """Runs after the table (file order): prints the largest error / tolerance of every check; the clip was active in some
    steps and idle in others."""
    for chk, (r, name, k) in sorted(_RATIOS.items()):
        print(f"[optim f64] {chk:9s} largest error / tolerance {r:.3g} ({name}, step {k})")
    clips = [c for v in _CLIPS.values() for c in v]
    print(f"[optim f64] steps {len(clips)}, clip active in {sum(c < 1.0 for c in clips)}")
    if len(_CLIPS) == len(CASES):
        assert any(c < 1.0 for c in clips) and any(c == 1.0 for c in clips)


@pytest.mark.parametrize("n", [1, 3, 5, 1023, 2_200_003])
def test_polyak_bit_exact_any_tau(lib, n):
    rng = np.random.default_rng(n)
    main, tgt = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    md = padded(main, n)
    for tau in (0.0, 1e-3, 0.05, 0.5, 1.0):
        td = padded(tgt, n)
        assert lib.naf_polyak_update(td.data_ptr(), md.data_ptr(), tau, float(1.0 - tau), n, st()) == 0
        got = td.cpu().numpy()
        exp = O.polyak(tgt, main, tau)      # f32: fl(fl(tau*main) + fl((1-tau)*target)), exactly the reference's expression
        assert np.array_equal(bits(got[:n]), bits(exp)), tau
        assert (got[n:] == SENTINEL).all() and (md[n:] == SENTINEL).all()
        if tau == 0.0:
            assert np.array_equal(bits(got[:n]), bits(tgt))
        if tau == 1.0:
            assert np.array_equal(bits(got[:n]), bits(main))
    assert np.array_equal(md[:n].cpu().numpy(), main)


# ------------------------------------------------------------------------------------------------------------
# y = r + gamma V'
# ------------------------------------------------------------------------------------------------------------
GAMMAS = (0.0, 0.5, 0.9, 1.0)
LOSS_RTOL = 1e-4             # test_head_both_modes_vs_oracle_f64's tolerance of the summed loss
R_STRIDE = 52                # the minibatch row stride the learner passes for r


def head_inputs(A, B, mode):
    """Pre-activations, actions and rewards as test_head_both_modes_vs_oracle_f64 draws them. V' is drawn positive and as
    large as the advantage term (which grows with the joint count and would otherwise bury gamma V' below the loss's
    tolerance): y then lies on the other side of 0 from Q, so Q - y does not cancel and gamma shows in every sample."""
    rng = np.random.default_rng(1000 * A + 10 * B + mode)
    T = A * (A + 1) // 2
    x = dict(mu=rng.standard_normal((B, A)), l=rng.standard_normal((B, T)), V=rng.standard_normal(B),
             u=np.trunc(rng.uniform(-1.5, 1.5, (B, A))), r=rng.standard_normal(B))
    adv = O.head_forward(x["mu"], x["l"], np.zeros(B), x["u"], mode)["Q"]
    sigma = max(1.0, float(np.sqrt((adv ** 2).mean())))
    x["vn"] = sigma * (1.0 + np.abs(rng.standard_normal(B)))
    return x


def head_oracle(x, gamma, mode):
    """(Q, loss, d_mu, d_l, d_V) in float64"""
    B = x["V"].shape[0]
    f = O.head_forward(x["mu"], x["l"], x["V"], x["u"], mode)
    y = x["r"] + gamma * x["vn"]
    dq = 2 * (f["Q"] - y) / B
    return (f["Q"], ((f["Q"] - y) ** 2).mean(), dq) + tuple(O.head_backward(x["mu"], x["l"], x["u"], dq, mode))


def gamma_shows_in_the_loss(loss_at, rtol):
    """Vacuity guard, in the oracle alone: the loss at every gamma differs from the loss at 0.99 by more than the tolerance."""
    return all(abs(loss_at[g] - loss_at[0.99]) > rtol * max(abs(loss_at[g]), abs(loss_at[0.99])) for g in loss_at if g != 0.99)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("A,B", [(6, 256), (1, 5), (8, 100), (9, 256), (17, 64), (33, 50)])
def test_td_target_follows_gamma_and_strides(lib, mode, A, B):
    """naf_head_fwd_bwd_mse against O.head_forward / O.head_backward in float64 at gamma 0, 0.5, 0.9 and 1 — with r and V' at
    stride 1, and with r at the minibatch row stride and V' as the value column of the target net's padded head rows, as the
    learner passes them. Up to 8 joints: naf_head_fwd_bwd_mse_splitk on slabs is the unsplit kernel bit for bit at each gamma."""
    x = head_inputs(A, B, mode)
    T = A * (A + 1) // 2
    ldh = (A + T + 1 + 7) // 8 * 8
    ref = {g: head_oracle(x, g, mode) for g in GAMMAS + (0.99,)}
    assert gamma_shows_in_the_loss({g: ref[g][1] for g in ref}, LOSS_RTOL)
    nwg = (B + 7) // 8 if A <= 32 else (B + 3) // 4
    h = dev(np.concatenate([np.asarray(x["mu"]), x["l"], x["V"][:, None], np.zeros((B, ldh - A - T - 1))], axis=1))
    ud = dev(x["u"])
    r1, vn1 = dev(x["r"]), dev(x["vn"])
    rows = torch.full((B, R_STRIDE), 3.0, device="cuda")                 # r inside minibatch rows
    rows[:, 27] = r1
    hn = torch.full((B, ldh), -2.0, device="cuda")                       # V' inside the target net's head rows
    hn[:, A + T] = vn1
    layouts = {"unit": (r1.data_ptr(), 1, vn1.data_ptr(), 1),
               "learner": (rows.data_ptr() + 4 * 27, R_STRIDE, hn.data_ptr() + 4 * (A + T), ldh)}
    for gamma in GAMMAS:
        Q, loss, dq, d_mu, d_l, d_V = ref[gamma]
        res = {}
        for name, (rp, ldr, vp, ldv) in layouts.items():
            q = torch.empty(B, device="cuda")
            dh = torch.empty(B, ldh, device="cuda")
            lp = torch.zeros(nwg, device="cuda")
            assert lib.naf_head_fwd_bwd_mse(h.data_ptr(), ldh, ud.data_ptr(), A, rp, ldr, vp, ldv, gamma, q.data_ptr(),
                                            dh.data_ptr(), lp.data_ptr(), B, A, mode, st()) == 0
            torch.cuda.synchronize()
            res[name] = (q, dh, lp)
            # (the tolerances of test_head_both_modes_vs_oracle_f64, unchanged)
            np.testing.assert_allclose(q.cpu().numpy(), Q, rtol=3e-5, atol=3e-5)
            dhn = dh.cpu().numpy()
            scale = np.abs(dq).max() * 10
            np.testing.assert_allclose(dhn[:, :A], d_mu, rtol=3e-4, atol=1e-6 * scale + 1e-7, err_msg=f"{name} gamma {gamma}")
            np.testing.assert_allclose(dhn[:, A:A + T], d_l, rtol=3e-4, atol=1e-6 * scale + 1e-7, err_msg=f"{name} gamma {gamma}")
            np.testing.assert_allclose(dhn[:, A + T], d_V, rtol=1e-5, atol=1e-8, err_msg=f"{name} gamma {gamma}")
            np.testing.assert_allclose(lp.sum().item(), loss, rtol=LOSS_RTOL, err_msg=f"{name} gamma {gamma}")
        for a, b in zip(res["unit"], res["learner"]):                    # same values through other strides: same bits
            assert torch.equal(a, b), gamma
        assert (rows[:, :27] == 3.0).all() and (rows[:, 28:] == 3.0).all() and (hn[:, :A + T] == -2.0).all()
    if A > 8:
        return
    # split-K slabs whose slab-ordered float32 sum is the unsplit kernel's input
    rng = np.random.default_rng(A + B)
    n_slabs, NHP = 16, (A + T + 1 + 15) // 16 * 16
    stride = B * NHP + 64
    hp = torch.zeros(n_slabs, stride, device="cuda")
    part = np.zeros((n_slabs, B, NHP), np.float32)
    part[:, :, :A + T + 1] = rng.standard_normal((n_slabs, B, A + T + 1)) / 4.0
    hp[:, :B * NHP] = dev(part.reshape(n_slabs, -1))
    vp = dev(rng.standard_normal((n_slabs, B)) / 4.0)
    heads, vn = hp[0, :B * NHP].reshape(B, NHP).clone(), vp[0].clone()
    for w in range(1, n_slabs):
        heads += hp[w, :B * NHP].reshape(B, NHP)
        vn += vp[w]
    first_lp = None
    for gamma in GAMMAS:
        res = []
        for split in (False, True):
            q, dH = torch.empty(B, device="cuda"), torch.empty(B, NHP, device="cuda")
            lp = torch.zeros((B + 7) // 8, device="cuda")
            if split:
                assert lib.naf_head_fwd_bwd_mse_splitk(hp.data_ptr(), stride, vp.data_ptr(), n_slabs, NHP, ud.data_ptr(), A,
                                                       rows.data_ptr() + 4 * 27, R_STRIDE, gamma, q.data_ptr(), dH.data_ptr(),
                                                       lp.data_ptr(), B, A, mode, st()) == 0
            else:
                assert lib.naf_head_fwd_bwd_mse(heads.data_ptr(), NHP, ud.data_ptr(), A, rows.data_ptr() + 4 * 27, R_STRIDE,
                                                vn.data_ptr(), 1, gamma, q.data_ptr(), dH.data_ptr(), lp.data_ptr(), B, A, mode,
                                                st()) == 0
            torch.cuda.synchronize()
            res.append((q, dH, lp))
        for a, b in zip(res[0], res[1]):
            assert torch.equal(a, b), gamma
        if first_lp is None:
            first_lp = res[0][2].clone()
        else:
            assert not torch.equal(res[0][2], first_lp)                  # (gamma reached the kernel)


FIRST_UPDATE_RTOL = 2e-4     # the suite's tolerance of a first update's loss against the float32 oracle
FIRST_UPDATES = [("rows", 21, 6, 256), ("rows", 27, 9, 256), ("rows", 21, 6, 2500), ("columns", 21, 6, 64), ("unfused", 30, 12, 64)]


def first_update_oracle_losses(chain, S, A, B, gammas):
    case = LearnCase("first", S, A, 256, B, 0, chain, n_upd=1)
    sd = init_state(case)
    st_, ac, rw, ns, dn = transitions(case)
    return case, sd, (st_, ac, rw, ns, dn), {g: float(O.LearnerOracle(sd, gamma=g, dtype=np.float32).learn(st_, ac, rw, ns))
                                              for g in gammas}


@pytest.mark.parametrize("chain,S,A,B", FIRST_UPDATES, ids=[f"{c}_{s}_{a}_{b}" for c, s, a, b in FIRST_UPDATES])
def test_first_update_loss_follows_gamma(chain, S, A, B, monkeypatch):
    """One learn_rows from the same initial state at gamma 0.5 and 1.0 on each chain: the loss against the float32 oracle at
    that gamma (the only place that reaches the gamma of the fused layer-2 + head launch of the row-split chain)."""
    monkeypatch.delenv("NAF_FUSE", raising=False)
    monkeypatch.delenv("NAF_DEFER_ADAM", raising=False)
    from robotic_manipulator_rloa_amd.learner import Learner
    case, sd, (st_, ac, rw, ns, dn), want = first_update_oracle_losses(chain, S, A, B, (0.5, 1.0, 0.99))
    assert gamma_shows_in_the_loss(want, FIRST_UPDATE_RTOL)
    for gamma in (0.5, 1.0):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            L = Learner(S, A, 256, B, 1e-3, 1e-3, gamma, torch.device("cuda"), fuse=chain)
        L.load_params(0, sd)
        L.load_params(1, sd)
        assert L.chain == chain
        rows = torch.from_numpy(O.pack_rows(st_, ac, rw, ns, dn, L.lay.row_floats)).cuda()
        lp = torch.zeros(L.n_loss_wg, device="cuda")
        L.learn_rows(rows, lp)
        torch.cuda.synchronize()
        got = float(lp.double().sum())
        print(f"[gamma] {chain} ({S}, {A}, {B}) gamma {gamma}: loss {got:.8g}, oracle {want[gamma]:.8g}, "
              f"relative error {abs(got - want[gamma]) / abs(want[gamma]):.2e}")
        np.testing.assert_allclose(got, want[gamma], rtol=FIRST_UPDATE_RTOL)

"""GPU: the two forms of the row-split chain's finish launch (csrc/big_batch.hip, bb_finish_block<.., SMALL>;
naf_bb_layer1_bwd_finish_form) leave the same bits. One learn_rows() at the two-net trained state of tests/rowsplit_cases.py fills the
learner's buffers up to the bundle; the finish launch then runs in the general and in the small form on the same inputs, and
everything it writes — the whole flat gradient, every sum-of-squares partial, the step count, the launch number — must be equal,
entries neither form writes included (they keep a sentinel). Then three whole updates with each form forced: parameters, Adam state
and BatchNorm buffers equal. The shapes are the smallest at which each branch of the small form can go wrong."""
import pytest
import torch

from learn_cases import Case, transitions
from oracle import naf_oracle as O
from rowsplit_cases import launch_state

pytestmark = pytest.mark.gpu

SENTINEL = -7.25            # what no sum of squares is and no gradient element of these cases happens to be
N_UPD = 3


def _case(S, A, H, B, p_mode=0, why=""):
    return Case(f"s{S}_a{A}_h{H}_b{B}" + ("_m1" if p_mode else ""), S, A, H, B, p_mode, "rows", n_upd=N_UPD, why=why)


SMALL_CASES = [
    _case(21, 6, 256, 16, why="NB1 = 1: three of the four quarters empty"),
    _case(21, 6, 256, 48, why="a partial 64-row block (NB1 = 2, Q = 1)"),
    _case(21, 6, 256, 64, why="one whole block, NB1 = 2"),
    _case(21, 6, 256, 160, why="NB1 = 5: Q = 2, the third quarter one block short, the fourth past the end of p_slabs"),
    _case(21, 6, 256, 256, why="the benchmark's shape: NB1 = 8, Q = 2, one slab"),
    _case(21, 6, 256, 256, 1, why="the benchmark's batch with the L L^T head"),
    _case(21, 6, 256, 512, why="the largest small shape: NB1 = 16, Q = 4, two slabs per segment"),
    _case(32, 8, 256, 128, why="kp = 32 (naf_bb_layer1_bwd_kp): every k lane loads, NHP = 48"),
    _case(21, 6, 512, 64, 1, why="H = 512: 256 finish workgroups, block stride H * KP of 48 KB"),
]
GENERAL_CASE = _case(21, 6, 256, 576, why="NB1 = 18: the first shape outside the small form's conditions")


def _learner(case, form):
    from robotic_manipulator_rloa_amd.learner import Learner
    main, target = launch_state(case)
    L = Learner(case.S, case.A, case.H, case.B, 1e-3, 1e-3, 0.99, torch.device("cuda"), p_mode=case.p_mode, _finish_form=form)
    L.load_params(0, main)
    L.load_params(1, target)
    assert L.chain == "rows" and L.fold_norm and L.defer_ok, (case.name, L.chain)
    return L


def _rows(case, L):
    st, ac, rw, ns, dn = transitions(case)
    return torch.from_numpy(O.pack_rows(st, ac, rw, ns, dn, L.lay.row_floats)).cuda()


def _finish_outputs(L, form, grad_in):
    """One finish launch in `form` on the buffers the chain left; what it wrote, over sentinels."""
    L.grad.copy_(grad_in)
    L.partials.fill_(SENTINEL)
    L.step_live.fill_(5)
    L.bb_fold_flag.fill_(9)
    L._launch_finish(None, False, form)
    torch.cuda.synchronize()
    return {"grad": L.grad.clone(), "sumsq_partials": L.partials.clone(), "step_dev": L.step_live.clone(),
            "bb_fold_flag": L.bb_fold_flag.clone()}


def _up_to_the_bundle(case):
    """A learner whose buffers hold what the finish launch reads, and the gradient with every element the launch writes replaced
    by the sentinel (layer 2's BatchNorm gradient, which it reads, kept)."""
    from robotic_manipulator_rloa_amd import _lib
    L = _learner(case, _lib.FINISH_AUTO)
    rows = _rows(case, L)
    lp = torch.zeros(L.n_loss_wg, device="cuda")
    L.learn_rows(rows[:case.B], lp, defer=True)          # (deferred: no optimizer step — the parameters the launch reads stay)
    torch.cuda.synchronize()
    grad_in = L.grad.clone()
    for k in ("W1", "b1", "g1", "be1", "W2", "b2", "Wh"):
        L.lay.view(grad_in, k).fill_(SENTINEL)
    # the inputs are not vacuous: the block shares and sums the launch folds are there
    assert L.bb_dw1.abs().max() > 0 and L.bb_bw1.abs().max() > 0 and L.bb_slab_w2.abs().max() > 0
    return L, grad_in


@pytest.mark.parametrize("case", SMALL_CASES, ids=[c.name for c in SMALL_CASES])
def test_small_form_leaves_the_general_forms_bits(case):
    from robotic_manipulator_rloa_amd import _lib
    L, grad_in = _up_to_the_bundle(case)
    assert L.finish_small, (case.name, case.why)
    out = {f: _finish_outputs(L, f, grad_in) for f in (_lib.FINISH_GENERAL, _lib.FINISH_SMALL, _lib.FINISH_AUTO)}
    gen = out[_lib.FINISH_GENERAL]
    # the launch wrote: every element of its segments (pad regions of a padded layer aside) and one partial per workgroup
    for k in ("W1", "g1", "be1", "b1", "b2", "W2", "Wh"):
        assert not (L.lay.view(gen["grad"], k) == SENTINEL).any(), k
    assert L.lay.view(gen["grad"], "W1").abs().max() > 0 and L.lay.view(gen["grad"], "g1").abs().max() > 0
    assert not (gen["sumsq_partials"][:L.n_partials_fold] == SENTINEL).any()
    assert (gen["sumsq_partials"][L.n_partials_fold:] == SENTINEL).all()
    assert int(gen["step_dev"]) == 6 and int(gen["bb_fold_flag"]) == 10
    for form in (_lib.FINISH_SMALL, _lib.FINISH_AUTO):
        for name, t in out[form].items():
            assert torch.equal(t, gen[name]), (case.name, case.why, form, name,
                                                int((t != gen[name]).sum()) if t.shape == gen[name].shape else "shape")
    # three whole updates with each form forced
    state = {}
    for form in (_lib.FINISH_GENERAL, _lib.FINISH_SMALL):
        Lf = _learner(case, form)
        rows = _rows(case, Lf)
        lp = torch.zeros(N_UPD, Lf.n_loss_wg, device="cuda")
        for k in range(N_UPD):
            Lf.learn_rows(rows[k * case.B:(k + 1) * case.B], lp[k])
        torch.cuda.synchronize()
        assert int(Lf.step_dev) == N_UPD
        state[form] = {"theta2": Lf.theta2.clone(), "adam_m": Lf.adam_m.clone(), "adam_v": Lf.adam_v.clone(),
                       "bn_stats": Lf.bn_stats.clone(), "loss": lp.clone()}
    assert state[_lib.FINISH_GENERAL]["adam_v"].abs().max() > 0
    for name, t in state[_lib.FINISH_SMALL].items():
        assert torch.equal(t, state[_lib.FINISH_GENERAL][name]), (case.name, case.why, name)


def test_first_shape_outside_the_conditions_runs_general_and_refuses_small():
    from robotic_manipulator_rloa_amd import _lib
    case = GENERAL_CASE
    L, grad_in = _up_to_the_bundle(case)
    assert L.plan.nb1 == 18 and not L.finish_small
    auto, gen = _finish_outputs(L, _lib.FINISH_AUTO, grad_in), _finish_outputs(L, _lib.FINISH_GENERAL, grad_in)
    for name, t in auto.items():
        assert torch.equal(t, gen[name]), name
    assert not (L.lay.view(gen["grad"], "W1") == SENTINEL).any()
    before = {k: v.clone() for k, v in gen.items()}
    with pytest.raises(_lib.NafHipError, match="error -1"):          # NAF_ERR_ARG: nothing launched
        L._launch_finish(None, False, _lib.FINISH_SMALL)
    torch.cuda.synchronize()
    assert torch.equal(L.grad, before["grad"]) and torch.equal(L.partials, before["sumsq_partials"])
    assert int(L.step_live) == 6 and int(L.bb_fold_flag) == 10

"""The forms of the finish launch without a GPU: the header declares naf_bb_layer1_bwd_finish_form as naf_bb_layer1_bwd_finish plus
`form` and the binding agrees, the ABI number stands, chain_plan.finish_small — the launcher's rule restated (csrc/big_batch.hip,
bb_finish_launch) — holds over the shapes tests/test_finish_forms_gpu.py runs plus the two forms of the gradient exchange, and the
library refuses the small form, before anything is launched, wherever that rule says no."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


def _args(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.M)     # (comments hold ';' and ',')
    assert m, f"include/naf_hip.h does not declare {name}"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_header_and_binding_agree_on_the_entry_and_the_abi_number_stands():
    from robotic_manipulator_rloa_amd import _lib
    header = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    args, args0 = _args(header, "naf_bb_layer1_bwd_finish_form"), _args(header, "naf_bb_layer1_bwd_finish")
    assert args[-2] == "int form" and args[:-2] + args[-1:] == args0
    proto, proto0 = _lib._PROTOS["naf_bb_layer1_bwd_finish_form"], _lib._PROTOS["naf_bb_layer1_bwd_finish"]
    assert len(proto) == len(args) and proto[-2] is C.c_int and proto[:-2] + proto[-1:] == proto0
    for name, value in (("AUTO", _lib.FINISH_AUTO), ("GENERAL", _lib.FINISH_GENERAL), ("SMALL", _lib.FINISH_SMALL)):
        assert re.search(r"^#define NAF_FINISH_%s %d$" % (name, value), header, re.M), name
    assert _lib.header_abi_version() == 40
    assert _lib.load().naf_hip_abi_version() == 40
    assert hasattr(_lib.load(), "naf_bb_layer1_bwd_finish_form")


# (B, small) at S = 21, A = 6, H = 256: what tests/test_finish_forms_gpu.py runs, and where the rule turns
TABLE = [(16, True), (48, True), (64, True), (160, True), (256, True), (512, True), (576, False), (1024, False), (2100, False)]


@pytest.mark.parametrize("B,small", TABLE)
def test_the_rule_over_the_shapes(B, small):
    from robotic_manipulator_rloa_amd.chain_plan import finish_small, plan_chain
    plan = plan_chain(21, 6, 256, B, env={})
    assert plan.chain == "rows"
    slabs = (plan.ks_w2, plan.ks_wh)
    assert finish_small(plan.nb1, 0, slabs) is small
    # a gradient exchange riding on the launch (push, or push + merge) takes the general form at every size
    assert not finish_small(plan.nb1, 0, slabs, push=True) and not finish_small(plan.nb1, 0, slabs, push=True, merge=True)


def test_the_rule_at_its_edges():
    from robotic_manipulator_rloa_amd.chain_plan import finish_small
    assert finish_small(16, 64, (2, 2)) and finish_small(1, 0, (1, 1)) and finish_small(16, 0, ())
    assert not finish_small(17, 0, (1, 1)) and not finish_small(16, 65, (1, 1))
    assert not finish_small(16, 0, (3, 1)) and not finish_small(16, 0, (1, 3))
    src = open(os.path.join(ROOT, "robotic_manipulator_rloa_amd", "csrc", "big_batch.hip")).read()
    from robotic_manipulator_rloa_amd import chain_plan
    assert int(re.search(r"^#define BF_SMALL_NB1 (\d+)", src, re.M).group(1)) == chain_plan.FINISH_SMALL_NB1
    assert int(re.search(r"^#define BF_SMALL_SLABS (\d+)", src, re.M).group(1)) == chain_plan.FINISH_SMALL_SLABS
    assert "chain_plan.finish_small" in src          # the launcher's comment names its restatement


def _call(lib, nb1, n_slabs, form, nb=0):
    """naf_bb_layer1_bwd_finish_form on made-up device addresses (the launcher reads none of them; only `segs` is host memory)."""
    from robotic_manipulator_rloa_amd import _lib
    a = 1 << 20                                        # a 16-byte aligned stand-in for every device pointer
    segs = (_lib.SlabSeg * 2)(_lib.SlabSeg(a, a, 1024, 1024, n_slabs[0]), _lib.SlabSeg(a, a, 1024, 1024, n_slabs[1]))
    return lib.naf_bb_layer1_bwd_finish_form(a, 21, a, nb1, a if nb else None, nb, a, a, a, a, a, a, a, a, a, a, a, a, a, 32 * nb1,
                                             256, segs, 2, a, None, None, 0, form, None)


@pytest.mark.parametrize("nb1,n_slabs,nb", [(17, (1, 1), 0), (18, (2, 2), 0), (64, (4, 4), 0), (16, (3, 1), 0), (16, (2, 3), 0),
                                            (8, (1, 8), 0)])
def test_small_form_on_a_shape_outside_its_conditions_is_an_argument_error(nb1, n_slabs, nb):
    from robotic_manipulator_rloa_amd import _lib
    from robotic_manipulator_rloa_amd.chain_plan import finish_small
    assert not finish_small(nb1, nb, n_slabs)
    assert _call(_lib.load(), nb1, n_slabs, _lib.FINISH_SMALL, nb) == -1        # NAF_ERR_ARG, before any launch


@pytest.mark.parametrize("form", [-1, 3, 7])
def test_a_form_the_library_does_not_have_is_an_argument_error(form):
    from robotic_manipulator_rloa_amd import _lib
    assert _call(_lib.load(), 8, (1, 1), form) == -1

"""naf_bb_layer1_adam_tile without a GPU: the header declares it, the library refuses a tile width it does not have before anything
else is looked at, and the entry came without an ABI bump."""
import os
import re

import pytest

from conftest import ROOT


def test_header_declares_the_tile_entry_and_the_abi_number_stands():
    from robotic_manipulator_rloa_amd import _lib
    header = open(os.path.join(ROOT, "include", "naf_hip.h")).read()
    m = re.search(r"^int naf_bb_layer1_adam_tile\(([^;]*)\);", header, re.M)
    assert m, "include/naf_hip.h does not declare naf_bb_layer1_adam_tile"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert "int cols" in args
    # the same arguments as naf_bb_layer1_adam plus the width, and the binding has as many
    m0 = re.search(r"^int naf_bb_layer1_adam\(([^;]*)\);", header, re.M)
    args0 = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m0.group(1), flags=re.S).split(",")]
    assert [a for a in args if a != "int cols"] == args0
    assert len(_lib._PROTOS["naf_bb_layer1_adam_tile"]) == len(args) == len(_lib._PROTOS["naf_bb_layer1_adam"]) + 1
    assert _lib.header_abi_version() == 40
    assert _lib.load().naf_hip_abi_version() == 40


@pytest.mark.parametrize("cols", [-16, 1, 8, 17, 24, 48, 63, 65, 128])
def test_a_width_the_library_does_not_have_is_an_argument_error(cols):
    from robotic_manipulator_rloa_amd import _lib
    lib = _lib.load()
    nul = None
    rc = lib.naf_bb_layer1_adam_tile(nul, 0, 24, 21, nul, nul, nul, nul, 0, nul, nul, nul, 0, nul, 0, 256, nul, nul, nul, nul, 64, 256,
                                     2, 0.1, 1e-5, cols, nul, nul)
    assert rc == -1          # NAF_ERR_ARG

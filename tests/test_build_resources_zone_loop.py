"""The zone loop and the centre deficits (trx_cells.hpp) are compile-time restricted to the one-row stencil
likelihood instantiations of cells_kernel -- <MODE_LNL, STEP, fp64 | fp32, LONG, ST, !PRUNE, WT both ways> --: those keep
four waves per SIMD, no scratch and sixteen workgroups' LDS per CU; every other instantiation compiles to the registers,
scratch and static LDS it had in the commit before the change (the figures below are from a build of that commit with
build()'s flags).  No GPU needed."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib

# template arguments <MODE, STEP, FP32, LONG, ST, PRUNE, WT> as they are mangled
ZONE = ("ILi0ELb1ELb0ELb1ELb1ELb0ELb0EE", "ILi0ELb1ELb0ELb1ELb1ELb0ELb1EE",
        "ILi0ELb1ELb1ELb1ELb1ELb0ELb0EE", "ILi0ELb1ELb1ELb1ELb1ELb0ELb1EE")
# (VGPRs, SGPRs, bytes of scratch a lane, bytes of static LDS) of libtrx.so's other instantiations, parent commit
PARENT = {
    "ILi0ELb0ELb0ELb0ELb0ELb0ELb0EE": (95, 106, 0, 0),
    "ILi0ELb0ELb0ELb1ELb0ELb0ELb0EE": (113, 106, 0, 0),
    "ILi0ELb0ELb0ELb1ELb1ELb0ELb0EE": (124, 106, 0, 0),
    "ILi0ELb1ELb0ELb0ELb0ELb0ELb0EE": (95, 106, 0, 0),
    "ILi0ELb1ELb0ELb0ELb0ELb0ELb1EE": (95, 106, 0, 0),
    "ILi0ELb1ELb0ELb0ELb0ELb1ELb0EE": (93, 106, 0, 720),
    "ILi0ELb1ELb0ELb1ELb0ELb0ELb0EE": (115, 106, 0, 0),
    "ILi0ELb1ELb0ELb1ELb0ELb0ELb1EE": (119, 106, 0, 0),
    "ILi0ELb1ELb0ELb1ELb0ELb1ELb0EE": (120, 106, 0, 0),
    "ILi0ELb1ELb1ELb0ELb0ELb0ELb0EE": (67, 106, 0, 0),
    "ILi0ELb1ELb1ELb0ELb0ELb0ELb1EE": (68, 106, 0, 0),
    "ILi0ELb1ELb1ELb0ELb0ELb1ELb0EE": (76, 106, 0, 720),
    "ILi0ELb1ELb1ELb1ELb0ELb0ELb0EE": (98, 106, 0, 0),
    "ILi0ELb1ELb1ELb1ELb0ELb0ELb1EE": (103, 104, 0, 0),
    "ILi0ELb1ELb1ELb1ELb0ELb1ELb0EE": (102, 106, 0, 0),
    "ILi1ELb0ELb0ELb0ELb0ELb0ELb0EE": (96, 105, 0, 0),
    "ILi1ELb0ELb0ELb1ELb0ELb0ELb0EE": (111, 106, 0, 0),
    "ILi1ELb0ELb0ELb1ELb1ELb0ELb0EE": (117, 106, 0, 0),
    "ILi1ELb1ELb0ELb0ELb0ELb0ELb0EE": (96, 106, 0, 0),
    "ILi1ELb1ELb0ELb1ELb0ELb0ELb0EE": (113, 106, 0, 0),
    "ILi1ELb1ELb0ELb1ELb1ELb0ELb0EE": (121, 106, 0, 0),
    "ILi1ELb1ELb1ELb0ELb0ELb0ELb0EE": (69, 106, 0, 0),
    "ILi1ELb1ELb1ELb1ELb0ELb0ELb0EE": (93, 106, 0, 0),
    "ILi1ELb1ELb1ELb1ELb1ELb0ELb0EE": (110, 106, 0, 0),
}


def _args(name):
    return name[name.index("cells_kernel") + len("cells_kernel"):].split("EvNS_")[0]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    return {_args(name): r for name, r in instantiations(kernel_resources(_lib.LIB_PATH), "cells_kernel").items()}


def test_zone_instantiations_keep_four_waves_no_scratch_and_their_lds(built):
    for args in ZONE:
        vgprs, _, scratch, static_lds = built[args]
        assert vgprs <= 128 and scratch == 0 and static_lds == 0, (args, built[args])
    assert _lib.lib().trx_debug_cells_lds_one_row() == 10240          # (the testing library: tests/conftest.py)


def test_every_other_instantiation_compiles_to_what_it_did(built):
    assert set(built) == set(PARENT) | set(ZONE), sorted(set(built) ^ (set(PARENT) | set(ZONE)))
    moved = {args: (PARENT[args], built[args]) for args in PARENT if built[args] != PARENT[args]}
    assert not moved, moved

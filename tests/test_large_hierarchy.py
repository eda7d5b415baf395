"""Host side of the global-row form of the tree-rule kernels (csrc/rules_global.h): the large fixtures lie where the LDS
form refuses, the new C symbols and Python switches exist, and the restated automatic choice (fits -> LDS, else global)
agrees with tests/_tree_shapes.describe on every shape.  No GPU."""
import ctypes
import os
import re

import pytest

import _large_tree_cases as L
import _tree_shapes as S
import nbdt_path
from nbdt import _C, ops
from nbdt.tree import Tree

_flats = {}


@pytest.fixture(scope="module")
def shapes_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("large_hierarchy")


def _described(name, directory):
    if name not in _flats:
        pg, pw, leaves = (L.build if name in L.LARGE else S.build)(name, directory)
        flat = Tree(None, path_graph=pg, path_wnids=pw, classes=leaves).flat
        _flats[name] = (flat, S.describe(flat))
    return _flats[name]


@pytest.mark.parametrize("name", list(L.LARGE))
def test_large_shapes_lie_where_the_lds_form_refuses(name, shapes_dir):
    flat, d = _described(name, shapes_dir)
    assert flat.num_classes == L.LARGE[name][1][0]
    flat.require_single_path()
    for entry in L.ENTRY_POINTS:
        assert d["staged"][entry] is None, (name, entry)
        assert L.expected_path(flat, entry, d) == "global"
    assert d["staged"]["tree_stats"] is None                  # and the diagnostics, which keep refusing
    assert d["tps"] == 1024
    if name == "star6000":
        assert list(L.wide_nodes(flat)) == [0] and d["max_fanout"] == 6000
    else:
        assert len(L.wide_nodes(flat)) == 0
    if name == "kary21841_2":
        assert d["longest_slot"] > 10000                      # one ordered chain of ~11k logits
        assert L.row_floats(flat) * 4 < 0.65 * 2 ** 20         # "0.6 MB at 21,841 classes"


@pytest.mark.parametrize("name", list(S.SHAPES) + list(L.LARGE))
def test_restated_choice_agrees_with_describe(name, shapes_dir):
    flat, d = _described(name, shapes_dir)
    for entry in L.ENTRY_POINTS:
        refused = d["staged"][entry] is None
        assert L.takes_global(flat, entry, d["sched_len"]) == refused, (name, entry)
        assert L.expected_path(flat, entry, d) == ("global" if refused else "lds" if d["staged"][entry] else "lds-unstaged")
    if name in S.SHAPES:      # automatic mode never selects new code on anything the LDS form runs
        assert all(d["staged"][e] is not None for e in L.ENTRY_POINTS)


def test_new_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(nbdt_path.ROOT, "include", "nbdt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+nbdt_set_rules_path\s*\(\s*int\s+mode\s*\)\s*;", code)
    assert re.search(r"\bint\s+nbdt_get_rules_path\s*\(\s*void\s*\)\s*;", code)
    assert re.search(r"\bconst\s+char\s*\*\s*nbdt_debug_last_rules_path\s*\(\s*void\s*\)\s*;", code)
    assert _C.SIGNATURES["nbdt_set_rules_path"] == (ctypes.c_int, [ctypes.c_int])
    assert _C.SIGNATURES["nbdt_get_rules_path"] == (ctypes.c_int, [])
    assert _C.SIGNATURES["nbdt_debug_last_rules_path"] == (ctypes.c_char_p, [])
    if not os.path.exists(_C.libpath()):
        from nbdt import _build
        _build.build()
    exported = set(_C.exported_symbols())
    assert {"nbdt_set_rules_path", "nbdt_get_rules_path", "nbdt_debug_last_rules_path"} <= exported
    assert _C.lib().nbdt_version() >= 127


def test_rules_path_switch_is_host_only():
    """Default automatic; "global" and back; unknown names and modes are refused and leave the switch alone."""
    assert ops.rules_path() == "auto" and _C.lib().nbdt_get_rules_path() == 0
    try:
        ops.set_rules_path("global")
        assert ops.rules_path() == "global" and _C.lib().nbdt_get_rules_path() == 1
        for bad in ("lds", "Global", "", None, 1):
            with pytest.raises(ValueError, match="unknown rules path"):
                ops.set_rules_path(bad)
        assert ops.rules_path() == "global"
        assert _C.lib().nbdt_set_rules_path(2) == -1 and b"rules path" in _C.lib().nbdt_last_error()
        assert _C.lib().nbdt_set_rules_path(-1) == -1
        assert ops.rules_path() == "global"
    finally:
        ops.set_rules_path("auto")
    assert ops.rules_path() == "auto"
    assert _C.last_rules_path() in ("", "lds", "lds-unstaged", "global")      # "" until this thread launches


@pytest.mark.parametrize("name", ["kary243_3", "kary600_70", "kary2560_2"])
def test_sparse_references_are_soft_target_ref(name, shapes_dir):
    """_large_tree_cases.ref_soft_losses / ref_hard_loss (sparse membership, one path product for several targets) give
    the numbers of _soft_target_ref.soft_loss / hard_loss, which build the dense matrix."""
    import numpy as np
    import torch
    import _soft_target_ref as R
    flat, _ = _described(name, shapes_dir)
    C = flat.num_classes
    z, y = L.logits_for(C), L.labels_for(C)
    t = torch.softmax(torch.randn(L.B, C, generator=torch.Generator().manual_seed(1)), 1).numpy()
    cases = [(y, 0.0), (y, 0.1), (t, 0.0), (t, 0.1)]
    for (target, eps), (loss, dz) in zip(cases, L.ref_soft_losses(flat, z, cases, 0.5, 10.0)):
        want_loss, want_dz = R.soft_loss(flat, z, target, eps, 0.5, 10.0)
        assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
        np.testing.assert_allclose(dz, want_dz, rtol=1e-9, atol=1e-15)
    for eps in (0.0, 0.1):
        loss, dz = L.ref_hard_loss(flat, z, y, eps, 0.5, 200.0 / flat.num_inodes)
        want_loss, want_dz = R.hard_loss(flat, z, y, eps, 0.5, 200.0 / flat.num_inodes)
        assert abs(loss - want_loss) <= 1e-12 * abs(want_loss)
        np.testing.assert_allclose(dz, want_dz, rtol=1e-9, atol=1e-15)

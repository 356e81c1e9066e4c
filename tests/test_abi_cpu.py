"""CPU: the C-ABI library builds, loads, and exports every entry point include/*.h declares
(no compute calls without a GPU); the ctypes binding covers the same set."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    names = set()
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h.endswith(".h"):
            src = open(os.path.join(ROOT, "include", h)).read()
            src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
            names |= set(re.findall(r"\b(cpt_[a-z0-9_]+)\s*\(", src))
    return sorted(names)


def test_header_symbols_exported():
    from cpt_amd import build, _lib
    build.build(verbose=False)
    names = _declared()
    assert len(names) >= 15
    lib = _lib.lib()                                  # dlopen: every undefined symbol would fail here
    for n in names:
        assert hasattr(lib, n), "libcpt_hip.so does not export %s" % n
    assert set(_lib.exported_symbols()) == set(names), set(_lib.exported_symbols()) ^ set(names)
    assert lib.cpt_version() == 8
    assert isinstance(lib.cpt_last_error(), bytes)


def test_struct_layouts_match_header():
    from cpt_amd import _lib as L
    assert ctypes.sizeof(L.Dims) == 12 * 4 + 2 * 4
    assert ctypes.sizeof(L.Layer) == 12 * 8
    assert ctypes.sizeof(L.Batch) == 3 * 4 + 4 + 7 * 8 + 4 + 4 + 8     # 3 ints, padding, 7 pointers, n_rows, padding, row_seq (ABI 5)
    assert ctypes.sizeof(L.Outputs) == 8 * 8
    assert L.Model.layers.offset == ctypes.sizeof(L.Dims) + 9 * 8


def test_product_path_has_no_cpu_fallback():
    """Model on CPU tensors must raise, and nothing under cpt_amd imports the oracle."""
    import torch
    from cpt_amd import config as cfgmod
    from cpt_amd.modeling_rec import REC_MLM_CPT
    m = REC_MLM_CPT(cfgmod.tiny())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, dtype=torch.long))
    for dp, _, files in os.walk(os.path.join(ROOT, "cpt_amd")):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.replace("# noqa", ""), "%s mentions the oracle" % f


def test_switch_table_and_header_key_list_agree():
    """The kernel-variant switches are written down once, in the table of cpt_amd/csrc/switches.h; the comment of cpt_set_tuning in
    include/cpt_hip_debug.h describes the same keys to a caller.  Both name every key exactly once, and no source file defines a switch
    of its own beside the table."""
    csrc = os.path.join(ROOT, "cpt_amd", "csrc")
    table = open(os.path.join(csrc, "switches.h")).read()
    rows = re.findall(r"^\s*X\(\s*(-?\d+)\s*,\s*(\w+)\s*,", table, flags=re.M)
    keys = [int(k) for k, _ in rows]
    names = [n for _, n in rows]
    assert len(keys) >= 10
    assert len(set(keys)) == len(keys), "a key appears twice in the switch table: %s" % sorted(k for k in keys if keys.count(k) > 1)
    assert len(set(names)) == len(names), "a variable appears twice in the switch table"
    assert all(k >= 0 and k != 8 for k in keys), "-1 (reset) and 8 (trace filter) are not switches"
    header = open(os.path.join(ROOT, "include", "cpt_hip_debug.h")).read()
    doc = [int(k) for k in re.findall(r"^ \*\s+key\s+(-?\d+)\b", header, flags=re.M)]
    assert len(set(doc)) == len(doc), "a key is described twice in cpt_hip_debug.h: %s" % sorted(k for k in doc if doc.count(k) > 1)
    assert sorted(doc) == sorted(keys), "switches.h and cpt_hip_debug.h disagree on keys %s" % sorted(set(doc) ^ set(keys))
    assert "switches.h" in header                      # the header says which file is authoritative
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip") or f.endswith(".cpp"):
            assert "CPT_SWITCH(" not in open(os.path.join(csrc, f)).read(), "%s defines a switch outside the table" % f

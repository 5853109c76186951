"""CPU checks of the colour classes on a KmerSetSet index (ksh_kss_color_classes): the version, the exported and
declared name, the route bit, the Python layer, the header's list of calls that leave plans exact, and every refusal
that is made before the index is dereferenced -- KSH_INVALID_ARGUMENT with a message that names the field.  (The
refusals that read the index are in tests/test_gpu_classes.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

from kmersets import capi


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_the_classes(lib):
    assert lib.ksh_version() >= 9
    assert "ksh_kss_color_classes" in capi.exported_symbols()
    assert hasattr(lib, "ksh_kss_color_classes")
    assert capi.QROUTE_CLASS_SPILL == 128
    for name in ("color_classes", "class_matrix"):
        assert callable(getattr(capi.KssIndex, name)), name


def test_header_declares_the_call_and_the_route_bit():
    text = open(capi.HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int\s+ksh_kss_color_classes\s*\(([^)]*)\)", code)
    assert decl, "the header declares the call"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const int32_t* cols", "int32_t n_cols", "ksh_kss_index* idx", "int64_t capacity",
                      "uint64_t* rows", "int64_t* counts", "int64_t* n_classes"]
    assert "KSH_QROUTE_CLASS_SPILL = 1 << 7" in text
    assert "KSH_QROUTE_PAIR_SPLIT = 1 << 5" in text and "KSH_QROUTE_PAIR_FLUSH = 1 << 6" in text  # keep their bits


def test_header_lists_the_call_among_those_that_leave_plans_exact():
    text = open(capi.HEADER).read()
    plans = text[text.index("Every other call leaves every pending plan exact"):text.index("A failed plan ends")]
    assert "ksh_kss_color_classes" in plans


def test_class_matrix():
    rows = np.array([[0, 0], [5, 0], [1 << 63, 1], [(1 << 64) - 1, (1 << 64) - 1]], dtype=np.uint64)
    m = capi.KssIndex.class_matrix(rows, 128)
    assert m.dtype == bool and m.shape == (4, 128)
    assert not m[0].any() and m[3].all()
    assert np.flatnonzero(m[1]).tolist() == [0, 2] and np.flatnonzero(m[2]).tolist() == [63, 64]
    assert capi.KssIndex.class_matrix(rows[:2], 3).tolist() == [[False] * 3, [True, False, True]]
    assert capi.KssIndex.class_matrix(np.zeros((0, 2), dtype=np.uint64), 5).shape == (0, 5)


def refused(lib, rc, word):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"
    assert word in lib.ksh_last_error(), (word, lib.ksh_last_error())


def test_refusals_before_the_index(lib):
    fake = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    cols = (C.c_int32 * 2)(0, 1)
    many = (C.c_int32 * 129)(*range(129))
    rows = (C.c_uint64 * 8)(*([0xA5] * 8))
    counts = (C.c_int64 * 4)(*([0xA5] * 4))
    n = C.c_int64(-7)
    call = lib.ksh_kss_color_classes
    refused(lib, call(cols, 2, None, 4, rows, counts, C.byref(n)), b"idx")
    refused(lib, call(cols, 2, fake, 4, None, counts, C.byref(n)), b"rows")
    refused(lib, call(cols, 2, fake, 4, rows, None, C.byref(n)), b"counts")
    refused(lib, call(cols, 2, fake, 4, rows, counts, None), b"n_classes")
    refused(lib, call(None, 0, None, 4, rows, counts, C.byref(n)), b"idx")
    for capacity in (0, -1, (1 << 24) + 1, 1 << 40, -(1 << 40)):
        refused(lib, call(cols, 2, fake, capacity, rows, counts, C.byref(n)), b"capacity")
        refused(lib, call(None, 0, fake, capacity, rows, counts, C.byref(n)), b"capacity")
    for n_cols in (0, -1, 129, 1 << 20):
        refused(lib, call(many, n_cols, fake, 4, rows, counts, C.byref(n)), b"n_cols")
    # nothing was written by a refused call
    assert list(rows) == [0xA5] * 8 and list(counts) == [0xA5] * 4 and n.value == -7

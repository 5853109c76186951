"""CPU checks of the class id per selected k-mer (ksh_kss_select_class_ids): the version, the exported name and its
parameter list, the Python layer, the header's list of calls that leave plans exact, and every refusal that is made
before the index is dereferenced -- KSH_INVALID_ARGUMENT with a message that names the field, and nothing written.
(The refusals that read the index are in tests/test_gpu_class_ids.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

from kmersets import capi

SENTINEL = -777


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_the_call(lib):
    assert lib.ksh_version() >= 10
    assert "ksh_kss_select_class_ids" in capi.exported_symbols()
    assert hasattr(lib, "ksh_kss_select_class_ids")
    assert capi.CLASS_NONE == 0xFFFFFFFF
    for name in ("select_class_ids", "select_classes"):
        assert callable(getattr(capi.KssIndex, name)), name


def test_header_declares_the_call():
    text = open(capi.HEADER).read()
    decl = re.search(r"\bint\s+ksh_kss_select_class_ids\s*\(([^)]*)\)\s*;", text)
    assert decl, "ksh_kss_select_class_ids is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const ksh_kss_selection* sel", "ksh_kss_index* idx", "const uint64_t* rows",
                      "int64_t n_classes", "const int64_t* d_offsets", "int64_t n_keys", "void* d_keys",
                      "uint32_t* d_class_ids", "int64_t* n_unmatched"]
    assert re.search(r"#define\s+KSH_CLASS_NONE\s+0xFFFFFFFFu", text)


def test_header_lists_the_call_among_those_that_leave_plans_exact():
    text = open(capi.HEADER).read()
    plans = text[text.index("Every other call leaves every pending plan exact"):text.index("A failed plan ends")]
    assert "ksh_kss_select_class_ids" in plans
    routes = text[text.index("The routes the last query"):text.index("enum {", text.index("The routes the last query"))]
    assert "ksh_kss_select_class_ids" in routes


# ---- the request of tests/test_select_cpu.py (copied: importing a test module would collect its tests twice) -------
def selection(cols=(0, 1), n_cols=None, min_count=1, max_count=0, require=(), n_require=None, exclude=(),
              n_exclude=None, struct_size=None):
    def ids(x):
        return None if x is None else (C.c_int32 * max(len(x), 1))(*x)
    c, r, e = ids(cols), ids(require), ids(exclude)
    sel = capi.Selection(C.sizeof(capi.Selection) if struct_size is None else struct_size, c,
                         (len(cols) if cols is not None else 0) if n_cols is None else n_cols, min_count, max_count, r,
                         (len(require) if require is not None else 0) if n_require is None else n_require, e,
                         (len(exclude) if exclude is not None else 0) if n_exclude is None else n_exclude)
    sel._keep = (c, r, e)
    return sel


MANY = tuple(range(129))
BAD_REQUESTS = [
    (dict(struct_size=0), b"struct_size"),
    (dict(struct_size=C.sizeof(capi.Selection) - 8), b"struct_size"),
    (dict(n_cols=0), b"n_cols"),
    (dict(n_cols=-1), b"n_cols"),
    (dict(cols=MANY), b"n_cols"),
    (dict(cols=MANY, n_cols=1 << 20), b"n_cols"),
    (dict(min_count=0), b"min_count"),
    (dict(min_count=-3), b"min_count"),
    (dict(max_count=-1), b"max_count"),
    (dict(min_count=2, max_count=1), b"max_count"),
    (dict(n_require=-1), b"n_require"),
    (dict(n_exclude=-1), b"n_exclude"),
    (dict(require=None, n_require=1), b"require"),
    (dict(exclude=None, n_exclude=2), b"exclude"),
]
GOOD_ROWS = [1, 0, 2, 0, 3, 0]  # three classes of two columns


def call(lib, sel, idx, rows, n_classes, d_offsets, n_keys, d_keys, d_ids, with_unmatched=False):
    """The C call; asserts that a refusal left the host's table and *n_unmatched as they were."""
    table = None if rows is None else np.array(rows, dtype=np.uint64)
    before = None if table is None else table.copy()
    missing = C.c_int64(SENTINEL)
    rc = lib.ksh_kss_select_class_ids(sel, idx, None if table is None else table.ctypes.data_as(C.POINTER(C.c_uint64)),
                                      n_classes, d_offsets, n_keys, d_keys, d_ids,
                                      C.byref(missing) if with_unmatched else None)
    assert missing.value == SENTINEL
    assert table is None or np.array_equal(table, before)
    return rc


def refused(lib, rc, word):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"
    assert word in lib.ksh_last_error(), (word, lib.ksh_last_error())


@pytest.mark.parametrize("fields,word", BAD_REQUESTS,
                         ids=[w.decode() + str(i) for i, (_, w) in enumerate(BAD_REQUESTS)])
def test_requests_refused_before_the_index(lib, fields, word):
    fake = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    sel = selection(**fields)
    for with_unmatched in (False, True):
        refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, fake, 0, fake, fake, with_unmatched), word)
    if "cols" not in fields and "n_cols" not in fields:  # the same with cols = NULL (all nodes)
        sel = selection(**dict(fields, cols=None))
        refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, fake, 0, fake, fake), word)


def test_null_arguments_refused_before_the_index(lib):
    fake = C.c_void_p(8)
    sel = selection()
    refused(lib, call(lib, None, fake, GOOD_ROWS, 3, fake, 0, fake, fake), b"sel")
    refused(lib, call(lib, C.byref(sel), None, GOOD_ROWS, 3, fake, 0, fake, fake), b"idx")
    refused(lib, call(lib, C.byref(sel), fake, None, 3, fake, 0, fake, fake), b"rows")
    refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, None, 0, fake, fake), b"d_offsets")
    refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, fake, 5, fake, None), b"d_class_ids")
    # (d_keys may be NULL: the ids alone are missed)
    refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, fake, 5, None, None), b"d_class_ids")
    refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, fake, -1, fake, fake), b"n_keys")
    refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, 3, fake, -1, fake, fake, True), b"n_keys")


@pytest.mark.parametrize("n_classes", [0, -1, (1 << 24) + 1])
def test_class_count_refused_before_the_index(lib, n_classes):
    fake = C.c_void_p(8)
    sel = selection()
    refused(lib, call(lib, C.byref(sel), fake, GOOD_ROWS, n_classes, fake, 0, fake, fake), b"n_classes")


@pytest.mark.parametrize("rows,at", [
    ([1, 0, 2, 0, 2, 0], b"rows[2]"),           # equal
    ([1, 0, 3, 0, 2, 0, 4, 0], b"rows[2]"),     # descending
    ([3, 0, 1, 0], b"rows[1]"),                 # descending at once
    ([0, 1, 1, 0], b"rows[1]"),                 # ascending by the low word only: the high word decides
    ([1, 0, 0, 1, 2, 0], b"rows[2]"),           # ... and again behind an ascending step
    ([5, 7, 5, 7], b"rows[1]"),                 # equal in both words
])
def test_unsorted_rows_refused_before_the_index(lib, rows, at):
    fake = C.c_void_p(8)
    sel = selection()
    for with_unmatched in (False, True):
        rc = call(lib, C.byref(sel), fake, rows, len(rows) // 2, fake, 0, fake, fake, with_unmatched)
        refused(lib, rc, b"rows")
        assert at in lib.ksh_last_error() and b"ascending" in lib.ksh_last_error()

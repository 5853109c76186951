"""CPU checks of the painting of sequences with colour classes (ksh_seq_class_runs): the version, the exported name
and its parameter list, the request struct, the Python layer, the header's list of calls that leave plans exact, and
every refusal that is made before the index is dereferenced -- KSH_INVALID_ARGUMENT with a message that names the
field, and nothing written.  (The refusals that read the index are in tests/test_gpu_paint.py.)"""
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
    assert lib.ksh_version() >= 11
    assert "ksh_seq_class_runs" in capi.exported_symbols()
    assert hasattr(lib, "ksh_seq_class_runs")
    for name in ("class_runs", "paint"):
        assert callable(getattr(capi.KssIndex, name)), name


def test_header_declares_the_call():
    text = open(capi.HEADER).read()
    decl = re.search(r"\bint\s+ksh_seq_class_runs\s*\(([^)]*)\)\s*;", text)
    assert decl, "ksh_seq_class_runs is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const ksh_spss_view* seqs", "ksh_kss_index* idx", "const ksh_seq_paint* req",
                      "int64_t capacity", "int64_t* d_run_offsets", "uint32_t* d_run_start",
                      "uint32_t* d_run_class", "int64_t* n_runs", "int64_t* n_unmatched"]


def test_struct_mirrors_the_header():
    text = open(capi.HEADER).read()
    body = re.search(r"typedef\s+struct\s+ksh_seq_paint\s*\{(.*?)\}\s*ksh_seq_paint\s*;", text, flags=re.S)
    assert body, "ksh_seq_paint is not declared"
    plain = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    members = [" ".join(m.split()) for m in plain.split(";") if m.strip()]
    assert members == ["size_t struct_size", "const int32_t* cols", "int32_t n_cols", "int32_t canonicalize",
                       "const uint64_t* rows", "int64_t n_classes", "int32_t route", "int64_t pass_positions"]
    assert [f[0] for f in capi.SeqPaint._fields_] == [m.split()[-1] for m in members]
    assert C.sizeof(capi.SeqPaint) == 56  # 8 + 8 + 4 + 4 + 8 + 8 + 4 (+ 4 of padding) + 8


def test_header_lists_the_call_among_those_that_leave_plans_exact():
    text = open(capi.HEADER).read()
    plans = text[text.index("Every other call leaves every pending plan exact"):text.index("A failed plan ends")]
    assert "ksh_seq_class_runs" in plans
    routes = text[text.index("The routes the last query"):text.index("enum {", text.index("The routes the last query"))]
    assert "ksh_seq_class_runs" in routes


GOOD_ROWS = [1, 0, 2, 0, 3, 0]  # three classes of two columns
FAKE = 8  # a pointer that is never dereferenced: the arguments are refused first


def call(lib, rows=GOOD_ROWS, n_classes=None, cols=(0, 1), n_cols=None, struct_size=None, route=0, pass_positions=0,
         n_strings=3, n_bases=90, words=FAKE, lens=FAKE, capacity=0, off=FAKE, start=FAKE, cls=FAKE, seqs=True,
         idx=FAKE, req=True, runs=True, with_unmatched=False):
    """The C call; asserts that it left *n_runs, *n_unmatched and the host's table as they were."""
    table = None if rows is None else np.array(rows, dtype=np.uint64)
    before = None if table is None else table.copy()
    ids = None if cols is None else (C.c_int32 * max(len(cols), 1))(*cols)
    paint = capi.SeqPaint(C.sizeof(capi.SeqPaint) if struct_size is None else struct_size, ids,
                          (0 if cols is None else len(cols)) if n_cols is None else n_cols, 1,
                          None if table is None else table.ctypes.data_as(C.POINTER(C.c_uint64)),
                          (0 if table is None else table.size // 2) if n_classes is None else n_classes, route,
                          pass_positions)
    view = capi.SpssView(words, lens, n_strings, n_bases)
    n_runs, missing = C.c_int64(SENTINEL), C.c_int64(SENTINEL)
    rc = lib.ksh_seq_class_runs(C.byref(view) if seqs else None, idx, C.byref(paint) if req else None, capacity, off,
                                start, cls, C.byref(n_runs) if runs else None,
                                C.byref(missing) if with_unmatched else None)
    assert n_runs.value == SENTINEL and missing.value == SENTINEL
    assert table is None or np.array_equal(table, before)
    return rc


def refused(lib, rc, word):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"
    assert word in lib.ksh_last_error(), (word, lib.ksh_last_error())


MANY = tuple(range(129))
BAD = [
    (dict(seqs=False), b"seqs"),
    (dict(idx=None), b"idx"),
    (dict(req=False), b"req"),
    (dict(runs=False), b"n_runs"),
    (dict(struct_size=0), b"struct_size"),
    (dict(struct_size=48), b"struct_size"),
    (dict(n_strings=-1), b"negative size"),
    (dict(n_bases=-5), b"negative size"),
    (dict(pass_positions=-1), b"pass_positions"),
    (dict(route=3), b"route"),
    (dict(route=-1), b"route"),
    (dict(words=None), b"NULL"),
    (dict(lens=None), b"NULL"),
    (dict(rows=None, n_classes=3), b"rows"),
    (dict(n_classes=0), b"n_classes"),
    (dict(n_classes=-1), b"n_classes"),
    (dict(n_classes=(1 << 24) + 1), b"n_classes"),
    (dict(n_cols=0), b"n_cols"),
    (dict(n_cols=-1), b"n_cols"),
    (dict(cols=MANY), b"n_cols"),
    (dict(cols=MANY, n_cols=1 << 20), b"n_cols"),
    (dict(capacity=-1), b"capacity"),
    (dict(capacity=5, start=None), b"d_run_start"),
    (dict(capacity=5, cls=None), b"d_run_class"),
    (dict(capacity=1, start=None, cls=None, off=None), b"d_run_start"),
]


@pytest.mark.parametrize("fields,word", BAD, ids=["%s%d" % (w.decode().replace(" ", "_"), i)
                                                  for i, (_, w) in enumerate(BAD)])
def test_refused_before_the_index(lib, fields, word):
    for with_unmatched in (False, True):
        refused(lib, call(lib, with_unmatched=with_unmatched, **fields), word)
    if "cols" not in fields and "n_cols" not in fields:  # the same with cols = NULL (all nodes)
        refused(lib, call(lib, **dict(fields, cols=None)), word)


@pytest.mark.parametrize("rows,at", [
    ([1, 0, 2, 0, 2, 0], b"rows[2]"),           # equal
    ([1, 0, 3, 0, 2, 0, 4, 0], b"rows[2]"),     # descending
    ([3, 0, 1, 0], b"rows[1]"),                 # descending at once
    ([0, 1, 1, 0], b"rows[1]"),                 # ascending by the low word only: the high word decides
    ([1, 0, 0, 1, 2, 0], b"rows[2]"),           # ... and again behind an ascending step
    ([5, 7, 5, 7], b"rows[1]"),                 # equal in both words
])
def test_unsorted_rows_refused_before_the_index(lib, rows, at):
    for with_unmatched in (False, True):
        for capacity in (0, 7):
            refused(lib, call(lib, rows=rows, capacity=capacity, with_unmatched=with_unmatched), b"rows")
            assert at in lib.ksh_last_error() and b"ascending" in lib.ksh_last_error()

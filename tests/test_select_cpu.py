"""CPU checks of the selections on a KmerSetSet index (ksh_kss_select_count, ksh_kss_select_keys): the version, the
exported names, the Python layer, the header's list of calls that leave plans exact, and every refusal that is made
before the index is dereferenced -- KSH_INVALID_ARGUMENT with a message that names the field.  (The refusals that
read the index are in tests/test_gpu_select.py.)"""
import ctypes as C

import pytest

from kmersets import capi


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_the_selections(lib):
    assert lib.ksh_version() >= 8
    for name in ("ksh_kss_select_count", "ksh_kss_select_keys"):
        assert name in capi.exported_symbols()
        assert hasattr(lib, name)
    for name in ("select", "spectrum", "select_count", "select_write"):
        assert callable(getattr(capi.KssIndex, name)), name


def test_header_lists_the_calls_among_those_that_leave_plans_exact():
    text = open(capi.HEADER).read()
    plans = text[text.index("Every other call leaves every pending plan exact"):text.index("A failed plan ends")]
    assert "ksh_kss_select_count" in plans and "ksh_kss_select_keys" in plans
    assert "ksh_kss_select_count, ksh_kss_select_keys: some bucket" in text  # KSH_QROUTE_PAIR_SPLIT is theirs too


def test_struct_matches_the_header():
    """The ctypes struct has the header's members in the header's order."""
    text = open(capi.HEADER).read()
    body = text[text.index("typedef struct ksh_kss_selection {"):text.index("} ksh_kss_selection;")]
    at = [body.index(" %s" % name) for name, _ in capi.Selection._fields_]
    assert at == sorted(at)
    assert C.sizeof(capi.Selection) == 64  # (LP64: 8, 8, 3 x 4 + 4 of padding, 8, 4 + 4, 8, 4 + 4)


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


def refused(lib, rc, word):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"
    assert word in lib.ksh_last_error(), (word, lib.ksh_last_error())


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


@pytest.mark.parametrize("fields,word", BAD_REQUESTS, ids=[w.decode() + str(i) for i, (_, w) in enumerate(BAD_REQUESTS)])
def test_requests_refused_before_the_index(lib, fields, word):
    fake = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    n = C.c_int64()
    sel = selection(**fields)
    refused(lib, lib.ksh_kss_select_count(C.byref(sel), fake, fake, C.byref(n), None), word)
    refused(lib, lib.ksh_kss_select_keys(C.byref(sel), fake, fake, 0, fake), word)
    sel = selection(**dict(fields, cols=None)) if "cols" not in fields and "n_cols" not in fields else None
    if sel is not None:  # the same with cols = NULL (all nodes)
        refused(lib, lib.ksh_kss_select_count(C.byref(sel), fake, fake, C.byref(n), None), word)


def test_null_arguments_refused_before_the_index(lib):
    fake = C.c_void_p(8)
    n = C.c_int64()
    spec = (C.c_int64 * 3)()
    sel = selection()
    refused(lib, lib.ksh_kss_select_count(None, fake, fake, C.byref(n), spec), b"sel")
    refused(lib, lib.ksh_kss_select_count(C.byref(sel), None, fake, C.byref(n), spec), b"idx")
    refused(lib, lib.ksh_kss_select_count(C.byref(sel), fake, None, None, None), b"spectrum")
    refused(lib, lib.ksh_kss_select_keys(None, fake, fake, 0, fake), b"sel")
    refused(lib, lib.ksh_kss_select_keys(C.byref(sel), None, fake, 0, fake), b"idx")
    refused(lib, lib.ksh_kss_select_keys(C.byref(sel), fake, None, 0, fake), b"d_offsets")
    refused(lib, lib.ksh_kss_select_keys(C.byref(sel), fake, fake, -1, fake), b"n_keys")
    refused(lib, lib.ksh_kss_select_keys(C.byref(sel), fake, fake, 5, None), b"d_keys")

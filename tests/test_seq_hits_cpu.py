"""CPU checks of the sequence queries on a KmerSetSet index (ksh_seq_hits): the version, the exported name, the new
route bit, and the entry refusing NULL arguments, negative sizes and bad routes with KSH_INVALID_ARGUMENT and a
message before it touches a device or the index."""
import ctypes as C

import pytest

from kmersets import capi


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_seq_hits(lib):
    assert lib.ksh_version() >= 6
    assert "ksh_seq_hits" in capi.exported_symbols()
    assert hasattr(lib, "ksh_seq_hits")
    assert capi.QROUTE_SEQ_PASSES == 16
    assert callable(capi.KssIndex.seq_hits)


def refused(lib, rc, word=None):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"
    if word:
        assert word in lib.ksh_last_error()


def test_seq_hits_refuses_null(lib):
    view = capi.SpssView(8, 8, 1, 23)
    fake = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    refused(lib, lib.ksh_seq_hits(None, fake, 1, 0, 0, fake), b"NULL")
    refused(lib, lib.ksh_seq_hits(C.byref(view), None, 1, 0, 0, fake), b"NULL")
    refused(lib, lib.ksh_seq_hits(C.byref(view), fake, 1, 0, 0, None), b"NULL")


def test_seq_hits_refuses_bad_sizes_before_the_index(lib):
    fake = C.c_void_p(8)
    for view in (capi.SpssView(8, 8, -1, 23), capi.SpssView(8, 8, 1, -23)):
        refused(lib, lib.ksh_seq_hits(C.byref(view), fake, 1, 0, 0, fake), b"negative")
    view = capi.SpssView(8, 8, 1, 23)
    refused(lib, lib.ksh_seq_hits(C.byref(view), fake, 1, 0, -1, fake), b"pass_positions")
    for route in (-1, 3):
        refused(lib, lib.ksh_seq_hits(C.byref(view), fake, 1, route, 0, fake), b"route")
    for view in (capi.SpssView(None, 8, 1, 23), capi.SpssView(8, None, 1, 23)):
        refused(lib, lib.ksh_seq_hits(C.byref(view), fake, 1, 0, 0, fake), b"NULL")


def test_header_lists_the_call_among_those_that_leave_plans_exact():
    text = open(capi.HEADER).read()
    plans = text[text.index("Every other call leaves every pending plan exact"):text.index("A failed plan ends")]
    assert "ksh_seq_hits" in plans

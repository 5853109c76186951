"""CPU checks of the pairwise intersection counts on a KmerSetSet index (ksh_kss_pair_counts): the version, the
exported name, the two new route bits, and the entry refusing NULL arguments, a column count outside [1, 128] and a
negative flush_rows with KSH_INVALID_ARGUMENT and a message before it touches a device or the index.  (The refusals
that read the index -- an id out of range, a repeated id, NULL cols on more than 128 nodes -- are in
tests/test_gpu_pair_counts.py.)"""
import ctypes as C

import pytest

from kmersets import capi


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_pair_counts(lib):
    assert lib.ksh_version() >= 7
    assert "ksh_kss_pair_counts" in capi.exported_symbols()
    assert hasattr(lib, "ksh_kss_pair_counts")
    assert capi.QROUTE_PAIR_SPLIT == 32 and capi.QROUTE_PAIR_FLUSH == 64
    assert callable(capi.KssIndex.pair_counts) and callable(capi.KssIndex.jaccard)


def test_header_has_the_route_bits():
    text = open(capi.HEADER).read()
    assert "KSH_QROUTE_PAIR_SPLIT = 1 << 5" in text and "KSH_QROUTE_PAIR_FLUSH = 1 << 6" in text


def refused(lib, rc, word=None):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"
    if word:
        assert word in lib.ksh_last_error()


def test_pair_counts_refuses_before_the_index(lib):
    fake = C.c_void_p(8)  # never dereferenced: the arguments are refused first
    cols = (C.c_int32 * 2)(0, 1)
    refused(lib, lib.ksh_kss_pair_counts(cols, 2, None, 0, fake, None), b"NULL")
    refused(lib, lib.ksh_kss_pair_counts(cols, 2, fake, 0, None, None), b"NULL")
    refused(lib, lib.ksh_kss_pair_counts(None, 0, None, 0, fake, None), b"NULL")
    many = (C.c_int32 * 129)(*range(129))
    for n_cols in (0, -1, 129, 1 << 20):
        refused(lib, lib.ksh_kss_pair_counts(many, n_cols, fake, 0, fake, None), b"n_cols")
    for flush_rows in (-1, -(1 << 40)):
        refused(lib, lib.ksh_kss_pair_counts(cols, 2, fake, flush_rows, fake, None), b"flush_rows")
        refused(lib, lib.ksh_kss_pair_counts(None, 0, fake, flush_rows, fake, None), b"flush_rows")


def test_header_lists_the_call_among_those_that_leave_plans_exact():
    text = open(capi.HEADER).read()
    plans = text[text.index("Every other call leaves every pending plan exact"):text.index("A failed plan ends")]
    assert "ksh_kss_pair_counts" in plans

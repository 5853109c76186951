"""CPU checks of the path cover from caller-supplied unitigs (ksh_spss_cover_*): the test-side oracle shim
agrees with the oracle's own C API, and the C ABI refuses bad arguments before it touches a device."""
import ctypes as C

import numpy as np
import pytest

import cover_oracle
import oracle_lib as ol
from kmersets import capi, synth


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_cover(lib):
    assert lib.ksh_version() >= 3
    for name in ("ksh_spss_cover_plan", "ksh_spss_cover_write", "ksh_spss_cover_stats", "ksh_spss_cover_release"):
        assert name in capi.exported_symbols()


def test_cover_refuses_bad_arguments(lib):
    g = capi.geom(9, 10)
    v = capi.SpssView(None, None, 0, 0)
    ns, nb = C.c_int64(), C.c_int64()
    assert lib.ksh_spss_cover_plan(None, C.byref(g), C.byref(v), 1, 1, C.byref(ns), C.byref(nb)) == \
        capi.KSH_INVALID_ARGUMENT
    assert b"NULL" in lib.ksh_last_error()
    assert lib.ksh_spss_cover_write(None, None, None) == capi.KSH_INVALID_ARGUMENT
    st = (C.c_int64 * 4)()
    assert lib.ksh_spss_cover_stats(None, st) == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_spss_cover_release(None) == capi.KSH_OK


@pytest.mark.parametrize("k", [5, 9, 15])
def test_shim_matches_oracle_capi(k):
    """cover_shim.cc's fast canonical cover == ko_spss_from_unitigs, on the oracle's unitigs shuffled and
    half reverse-complemented; on the unitigs as the oracle orders them, all three variants == the set-based
    oracle (ko_spss_canonical / ko_spss_variant)."""
    kmers = synth.random_read_kmers(k, 150 if k == 5 else 3000, seed=k, canonical=True)
    oset = ol.Set.from_kmers(k, min(10, 2 * k - 4), 4, kmers)
    u = oset.unitigs()
    assert cover_oracle.cover(u, k) == oset.spss()
    assert cover_oracle.cover(u, k, fast=False) == oset.spss_slow()
    assert cover_oracle.cover(oset.unitigs_directed(), k, canonical=False) == oset.spss_directed()
    mixed = cover_oracle.shuffled(u, seed=k)
    assert cover_oracle.cover(mixed, k) == cover_oracle.oracle_capi_cover(mixed, k)
    assert cover_oracle.cover([], k) == []

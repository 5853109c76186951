"""CPU checks of the KmerSetSet membership index (ksh_kss_index_*): the version and the exported names, and every
entry refusing NULL arguments with KSH_INVALID_ARGUMENT and a message before it touches a device."""
import ctypes as C

import pytest

from kmersets import capi

NAMES = ("ksh_kss_index_from_kss", "ksh_kss_index_create", "ksh_kss_index_query", "ksh_kss_index_info",
         "ksh_kss_index_routes", "ksh_kss_index_destroy")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_version_has_index(lib):
    assert lib.ksh_version() >= 4
    for name in NAMES:
        assert name in capi.exported_symbols()
        assert hasattr(lib, name)


def refused(lib, rc):
    assert rc == capi.KSH_INVALID_ARGUMENT
    assert lib.ksh_last_error(), "a refusal comes with a message"


def test_index_refuses_null(lib):
    h = C.c_void_p()
    refused(lib, lib.ksh_kss_index_from_kss(None, C.byref(h)))
    assert b"NULL" in lib.ksh_last_error()
    refused(lib, lib.ksh_kss_index_from_kss(C.c_void_p(8), None))
    g = capi.geom(23, 14)
    views = (capi.SpssView * 1)(capi.SpssView(None, None, 0, 0))
    offs = (C.c_int64 * 2)(0, 0)
    refused(lib, lib.ksh_kss_index_create(None, C.byref(g), views, 1, offs, None, 1, C.byref(h)))
    refused(lib, lib.ksh_kss_index_create(C.c_void_p(8), None, views, 1, offs, None, 1, C.byref(h)))
    refused(lib, lib.ksh_kss_index_create(C.c_void_p(8), C.byref(g), None, 1, offs, None, 1, C.byref(h)))
    refused(lib, lib.ksh_kss_index_create(C.c_void_p(8), C.byref(g), views, 1, None, None, 1, C.byref(h)))
    refused(lib, lib.ksh_kss_index_create(C.c_void_p(8), C.byref(g), views, 1, offs, None, 1, None))
    refused(lib, lib.ksh_kss_index_query(None, None, 0, 1, 0, None))
    n, w, b = C.c_int32(), C.c_int32(), C.c_int64()
    refused(lib, lib.ksh_kss_index_info(None, C.byref(n), C.byref(w), C.byref(b)))
    bits = C.c_uint32()
    refused(lib, lib.ksh_kss_index_routes(None, C.byref(bits)))
    refused(lib, lib.ksh_kss_index_destroy(None))


def _create(lib, n_nodes, offs, ids, g=None):
    g = g or capi.geom(23, 14)
    views = (capi.SpssView * max(n_nodes, 1))(*[capi.SpssView(None, None, 0, 0) for _ in range(max(n_nodes, 1))])
    o = (C.c_int64 * len(offs))(*offs)
    i = (C.c_int32 * max(len(ids), 1))(*(ids or [0]))
    h = C.c_void_p()
    # the context pointer is never dereferenced: the DAG and the arguments are refused first
    return lib.ksh_kss_index_create(C.c_void_p(8), C.byref(g), views, n_nodes, o, i, 1, C.byref(h))


def test_create_refuses_bad_dags_before_the_device(lib):
    refused(lib, _create(lib, 2, [0, 1, 1], [5]))            # child out of range
    assert b"outside" in lib.ksh_last_error()
    refused(lib, _create(lib, 2, [0, 1, 1], [0]))            # self edge
    assert b"self edge" in lib.ksh_last_error()
    refused(lib, _create(lib, 3, [0, 1, 2, 3], [1, 2, 0]))   # cycle
    assert b"cycle" in lib.ksh_last_error()
    refused(lib, _create(lib, 0, [0], []))                   # no nodes
    refused(lib, _create(lib, 1025, [0] * 1026, []))        # rows wider than 16 words
    assert b"1024" in lib.ksh_last_error()
    refused(lib, _create(lib, 1, [0, 0], [], g=capi.Geom(23, 14, 2, 0)))  # key bits do not fit the key type


def test_create_checks_every_offset_before_reading_edges(lib):
    """Offsets that rise and fall again ([0, 5, 0]) with no child_ids: refused, never read through NULL."""
    g = capi.geom(23, 14)
    views = (capi.SpssView * 2)(capi.SpssView(None, None, 0, 0), capi.SpssView(None, None, 0, 0))
    h = C.c_void_p()
    for offs in ([0, 5, 0], [0, 0, 3]):
        o = (C.c_int64 * 3)(*offs)
        refused(lib, lib.ksh_kss_index_create(C.c_void_p(8), C.byref(g), views, 2, o, None, 1, C.byref(h)))
    assert b"child_ids is NULL" in lib.ksh_last_error()

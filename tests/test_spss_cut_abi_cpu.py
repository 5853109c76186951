"""ksh_spss_cut through the layers that need no GPU: the header's declaration, the built library's export, the ctypes
signature, the Python wrappers, and the plan protocol's table staying complete without a new row (the call takes the
sequences first, as ksh_seq_hits does, and is neither a plan nor a write)."""
import ctypes as C
import inspect
import re

import plan_protocol_cases as cases
import test_plan_protocol_cpu as protocol
from kmersets import capi


def test_header_declares_the_call_with_the_sequences_first():
    decl = protocol.declarations()
    assert decl.get("ksh_spss_cut")[0] == "const ksh_spss_view* seqs"
    assert "ksh_spss_cut" in capi.exported_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(capi.HEADER).read(), flags=re.S)
    params = re.search(r"\bint\s+ksh_spss_cut\s*\(([^)]*)\)", text).group(1)
    types = [" ".join(p.split()[:-1]) for p in params.split(",")]
    assert types == ["const ksh_spss_view*", "ksh_ctx*", "const ksh_geom*", "const int64_t*", "const uint32_t*",
                     "int64_t", "uint64_t*", "uint32_t*", "int64_t*"]


def test_library_exports_it_with_a_signature():
    lib = capi.lib()
    assert hasattr(lib, "ksh_spss_cut")
    fn = lib.ksh_spss_cut
    assert fn.restype is C.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[0] is C.POINTER(capi.SpssView) and fn.argtypes[5] is C.c_int64


def test_host_refusals_need_no_device():
    """What is refused before anything touches a device."""
    lib = capi.lib()
    g = capi.geom(23, 14)
    view = capi.SpssView(None, None, 0, 0)
    n = C.c_int64(-1)
    fake = C.c_void_p(64)  # (never dereferenced: every call below is refused before)
    assert lib.ksh_spss_cut(None, fake, C.byref(g), None, None, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"seqs" in lib.ksh_last_error()
    assert lib.ksh_spss_cut(C.byref(view), None, C.byref(g), None, None, 0, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"ctx" in lib.ksh_last_error()
    assert lib.ksh_spss_cut(C.byref(view), fake, None, None, None, 0, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"g is NULL" in lib.ksh_last_error()
    tiny = capi.geom(3, 5)
    assert lib.ksh_spss_cut(C.byref(view), fake, C.byref(tiny), None, None, 0, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"K >= 4" in lib.ksh_last_error()
    assert lib.ksh_spss_cut(C.byref(view), fake, C.byref(g), None, None, -1, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"n_runs" in lib.ksh_last_error()
    assert lib.ksh_spss_cut(C.byref(view), fake, C.byref(g), None, None, 2, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"n_runs" in lib.ksh_last_error()  # runs without strings
    negative = capi.SpssView(None, None, -1, 0)
    assert lib.ksh_spss_cut(C.byref(negative), fake, C.byref(g), None, None, 0, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"negative" in lib.ksh_last_error()
    some = capi.SpssView(fake, fake, 3, 100)
    assert lib.ksh_spss_cut(C.byref(some), fake, C.byref(g), fake, fake, 2, fake, fake, None) == capi.KSH_INVALID_ARGUMENT
    assert b"n_runs = 2" in lib.ksh_last_error() and b"n_strings = 3" in lib.ksh_last_error()
    for at, name in ((3, b"d_run_offsets"), (4, b"d_run_start"), (6, b"d_words"), (7, b"d_lens")):
        args = [C.byref(some), fake, C.byref(g), fake, fake, 3, fake, fake, None]
        args[at] = None
        assert lib.ksh_spss_cut(*args) == capi.KSH_INVALID_ARGUMENT and name in lib.ksh_last_error()
    # no strings: served on the host, the size reported
    assert lib.ksh_spss_cut(C.byref(view), fake, C.byref(g), None, None, 0, None, None, C.byref(n)) == capi.KSH_OK
    assert n.value == 0


def test_python_wrappers_exist():
    assert callable(capi.Context.spss_cut) and callable(capi.KssIndex.colored_unitigs)
    assert list(inspect.signature(capi.Context.spss_cut).parameters) == ["self", "seqs", "run_offsets", "run_start"]
    sig = inspect.signature(capi.KssIndex.colored_unitigs)
    assert list(sig.parameters) == ["self", "cols", "mode", "route", "pass_positions"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 0, 0, 0]


def test_plan_protocol_table_is_unchanged_and_complete():
    """The call is no plan and no write, so the table has no row for it; it takes a context behind its request, so it
    is an intruder column on the victim's context and on the second one, it ends no plan, and every check of
    tests/test_plan_protocol_cpu.py holds."""
    mine = [c for c in cases.INTRUDERS if "ksh_spss_cut" in c["symbols"]]
    assert {c["where"] for c in mine} == {"own", "second"} and "ksh_spss_cut" not in cases.EXCLUDED
    assert all(c["refuses"] == () for c in mine) and any(not c["op"].startswith("fail:") for c in mine)
    protocol.test_every_plan_write_pair_is_a_victim()
    protocol.test_every_context_entry_point_is_an_intruder()
    protocol.test_refusals_only_where_the_contract_permits()

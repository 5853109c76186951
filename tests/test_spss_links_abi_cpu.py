"""ksh_spss_links through the layers that need no GPU: the header's declaration, the built library's export, the
ctypes signature, every host refusal, the no-strings answer, the Python wrappers, and the plan protocol's table staying
complete without a new row (the call takes the sequences first, as ksh_spss_cut does, and is neither a plan nor a
write)."""
import ctypes as C
import inspect
import re

import plan_protocol_cases as cases
import test_plan_protocol_cpu as protocol
from kmersets import capi


def test_header_declares_the_call_with_the_sequences_first():
    decl = protocol.declarations()
    assert decl.get("ksh_spss_links")[0] == "const ksh_spss_view* seqs"
    assert "ksh_spss_links" in capi.exported_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(capi.HEADER).read(), flags=re.S)
    params = re.search(r"\bint\s+ksh_spss_links\s*\(([^)]*)\)", text).group(1)
    types = [" ".join(p.split()[:-1]) for p in params.split(",")]
    assert types == ["const ksh_spss_view*", "ksh_ctx*", "const ksh_geom*", "int", "int64_t", "int64_t*", "int64_t*",
                     "int64_t*"]
    assert not "ksh_spss_links".endswith(("_plan", "_write"))


def test_library_exports_it_with_a_signature():
    lib = capi.lib()
    assert hasattr(lib, "ksh_spss_links")
    fn = lib.ksh_spss_links
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert fn.argtypes[0] is C.POINTER(capi.SpssView) and fn.argtypes[3] is C.c_int and fn.argtypes[4] is C.c_int64
    assert fn.argtypes[7] is C.POINTER(C.c_int64)


def test_host_refusals_need_no_device():
    """What is refused before anything touches a device."""
    lib = capi.lib()
    g = capi.geom(23, 14)
    view = capi.SpssView(None, None, 0, 0)
    n = C.c_int64(-1)
    fake = C.c_void_p(64)  # (never dereferenced: every call below is refused before, or served on the host)
    call = lib.ksh_spss_links
    assert call(None, fake, C.byref(g), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"seqs" in lib.ksh_last_error()
    assert call(C.byref(view), None, C.byref(g), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"ctx" in lib.ksh_last_error()
    assert call(C.byref(view), fake, None, 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"g is NULL" in lib.ksh_last_error()
    assert call(C.byref(view), fake, C.byref(g), 1, 0, None, None, None) == capi.KSH_INVALID_ARGUMENT
    assert b"n_links" in lib.ksh_last_error()
    tiny = capi.geom(3, 5)
    assert call(C.byref(view), fake, C.byref(tiny), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"K >= 4" in lib.ksh_last_error()
    broken = capi.Geom(23, 14, 3, 0)  # (no key has three bytes: what check_geom refuses)
    assert call(C.byref(view), fake, C.byref(broken), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"key_bytes" in lib.ksh_last_error()
    assert call(C.byref(view), fake, C.byref(g), 1, -1, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"capacity" in lib.ksh_last_error()
    assert call(C.byref(view), fake, C.byref(g), 0, 5, fake, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"d_link_to" in lib.ksh_last_error() and b"capacity = 5" in lib.ksh_last_error()
    negative = capi.SpssView(None, None, -1, 0)
    assert call(C.byref(negative), fake, C.byref(g), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"negative" in lib.ksh_last_error()
    for words, lens in ((None, fake), (fake, None)):  # strings without arrays (seq_check_request)
        some = capi.SpssView(words, lens, 3, 100)
        assert call(C.byref(some), fake, C.byref(g), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
        assert b"NULL" in lib.ksh_last_error()
    bases = capi.SpssView(None, None, 0, 7)  # no strings but bases
    assert call(C.byref(bases), fake, C.byref(g), 1, 0, None, None, C.byref(n)) == capi.KSH_INVALID_ARGUMENT
    assert b"n_bases" in lib.ksh_last_error()
    assert n.value == -1  # no refusal has written it
    # no strings: served on the host, in both modes, counting or with a capacity
    for canonical, capacity, to in ((1, 0, None), (0, 0, None), (1, 4, fake)):
        n.value = -1
        assert call(C.byref(view), fake, C.byref(g), canonical, capacity, None, to, C.byref(n)) == capi.KSH_OK
        assert n.value == 0


def test_python_wrappers_exist():
    assert callable(capi.Context.spss_links) and callable(capi.KssIndex.colored_graph)
    sig = inspect.signature(capi.Context.spss_links)
    assert list(sig.parameters) == ["self", "seqs", "canonical"] and sig.parameters["canonical"].default is True
    sig = inspect.signature(capi.KssIndex.colored_graph)
    assert list(sig.parameters) == ["self", "cols", "route", "pass_positions"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 0, 0]
    sig = inspect.signature(capi.gfa_lines)
    assert list(sig.parameters) == ["strings", "k", "link_offsets", "link_to", "string_class"]
    assert sig.parameters["string_class"].default is None
    assert list(inspect.signature(capi.write_gfa).parameters) == ["path"] + list(sig.parameters)
    assert "twins" in capi.gfa_lines.__doc__
    assert capi.gfa_lines(["ACGTA", "CGTAC"], 5, [0, 1, 1, 1, 2], [2, 1], [3, 4]) == [
        "H\tVN:Z:1.0", "S\t0\tACGTA\tCL:i:3", "S\t1\tCGTAC\tCL:i:4", "L\t0\t+\t1\t+\t4M", "L\t1\t-\t0\t-\t4M"]


def test_plan_protocol_table_is_unchanged_and_complete():
    """The call is no plan and no write, so the table has no row for it; it takes a context behind its request, so it
    is an intruder column on the victim's context and on the second one, it ends no plan, and every check of
    tests/test_plan_protocol_cpu.py holds."""
    mine = [c for c in cases.INTRUDERS if "ksh_spss_links" in c["symbols"]]
    assert {c["where"] for c in mine} == {"own", "second"} and "ksh_spss_links" not in cases.EXCLUDED
    assert all(c["refuses"] == () for c in mine) and any(not c["op"].startswith("fail:") for c in mine)
    protocol.test_every_plan_write_pair_is_a_victim()
    protocol.test_every_context_entry_point_is_an_intruder()
    protocol.test_refusals_only_where_the_contract_permits()

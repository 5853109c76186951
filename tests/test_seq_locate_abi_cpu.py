"""ksh_seq_locate through the layers that need no GPU: the header's declaration with the request as its only
parameter, the built library's export, the struct's layout, every host refusal with pointers that are never
dereferenced, the no-strings answer, the Python wrappers' signatures, and the plan protocol's table staying as it is
(no parameter of the call is a handle: the context is a field of the request)."""
import ctypes as C
import inspect
import re

import test_plan_protocol_cpu as protocol
from kmersets import capi

NAME = "ksh_seq_locate"


def test_header_declares_the_call_with_one_parameter():
    decl = protocol.declarations()
    assert decl.get(NAME) == ["const ksh_seq_locate_req* req"]
    assert NAME in capi.exported_symbols() and not NAME.endswith(("_plan", "_write"))
    assert not protocol.takes_a_context(decl[NAME])  # no parameter is a handle
    text = re.sub(r"/\*.*?\*/", "", open(capi.HEADER).read(), flags=re.S)
    fields = re.search(r"typedef struct ksh_seq_locate_req \{(.*?)\} ksh_seq_locate_req;", text, flags=re.S).group(1)
    members = [" ".join(f.split()) for f in fields.split(";") if f.strip()]
    assert members == ["size_t struct_size", "ksh_ctx* ctx", "const ksh_geom* g", "const ksh_spss_view* strings",
                       "const ksh_spss_view* reference", "int32_t canonical", "int64_t* d_where", "uint32_t* d_count",
                       "int64_t* n_located"]
    assert [m.split()[-1] for m in members] == [name for name, _ in capi.LocateReq._fields_]
    assert not re.match(r"ksh_(ctx|kss)", "ksh_seq_locate_req")
    header = open(capi.HEADER).read()
    assert "ends no pending plan" in header.split("ksh_seq_locate_req {")[0].rsplit("/* ----", 1)[1]


def test_library_exports_it_with_a_signature():
    lib = capi.lib()
    assert hasattr(lib, NAME)
    fn = lib.ksh_seq_locate
    assert fn.restype is C.c_int and fn.argtypes == [C.POINTER(capi.LocateReq)]
    assert C.sizeof(capi.LocateReq) == 72
    offsets = {name: getattr(capi.LocateReq, name).offset for name, _ in capi.LocateReq._fields_}
    assert offsets == {"struct_size": 0, "ctx": 8, "g": 16, "strings": 24, "reference": 32, "canonical": 40,
                       "d_where": 48, "d_count": 56, "n_located": 64}


def test_host_refusals_need_no_device():
    """What is refused before anything touches a device."""
    lib = capi.lib()
    fake = 64  # (never dereferenced: every call below is refused before, or served on the host)
    size = C.sizeof(capi.LocateReq)
    located = C.c_int64(-7)
    good_g = capi.geom(23, 14)

    def view(n=3, bases=100, words=fake, lens=fake):
        return capi.SpssView(words, lens, n, bases)

    def request(ctx=fake, g=good_g, strings=None, reference=None, where=fake, count=fake, struct_size=size):
        strings = view() if strings is None else strings
        reference = view(2, 80) if reference is None else reference
        return capi.LocateReq(struct_size, ctx, C.pointer(g) if g else None,
                              C.pointer(strings) if strings else None, C.pointer(reference) if reference else None,
                              1, where, count, C.pointer(located))

    def refused(word, req):
        rc = lib.ksh_seq_locate(C.byref(req) if req is not None else None)
        assert rc == capi.KSH_INVALID_ARGUMENT, (word, rc)
        assert word.encode() in lib.ksh_last_error(), (word, lib.ksh_last_error())

    refused("req is NULL", None)
    refused("req->struct_size = 64", request(struct_size=size - 8))
    refused("req->struct_size = 0", request(struct_size=0))
    refused("req->ctx is NULL", request(ctx=None))
    refused("req->g is NULL", request(g=False))
    refused("key_bytes", request(g=capi.Geom(23, 14, 3, 0)))          # a geometry no call accepts
    refused("req->g: k = 3", request(g=capi.Geom(3, 2, 2, 0)))
    refused("req->strings is NULL", request(strings=False))
    refused("req->strings: negative size: -1 strings", request(strings=view(n=-1)))
    refused("req->strings: negative size: 3 strings, -5 bases", request(strings=view(bases=-5)))
    refused("req->reference: negative size: -2 strings", request(reference=view(n=-2)))
    refused("req->reference: negative size: 2 strings, -1 bases", request(reference=view(2, -1)))
    refused("req->reference is NULL with 3 strings", request(reference=False))
    refused("req->strings: NULL words or lens", request(strings=view(words=None)))
    refused("req->strings: NULL words or lens", request(strings=view(lens=None)))
    refused("req->reference: NULL words or lens", request(reference=view(2, 80, lens=None)))
    refused("req->d_where is NULL with 3 strings", request(where=None))
    refused("req->d_count is NULL with 3 strings", request(count=None))
    refused("req->strings: sum(lens + K) = 0 but n_bases = 9", request(strings=view(0, 9)))
    refused("req->reference: sum(lens + K) = 0 but n_bases = 4", request(reference=view(0, 4)))
    assert located.value == -7  # no refusal has written it
    # no strings: served on the host, whatever else is missing
    for req in (request(strings=view(0, 0)), request(strings=view(0, 0, None, None), reference=False, where=None,
                                                     count=None)):
        located.value = -7
        assert lib.ksh_seq_locate(C.byref(req)) == capi.KSH_OK and located.value == 0
    req = request(strings=view(0, 0))
    req.n_located = None
    assert lib.ksh_seq_locate(C.byref(req)) == capi.KSH_OK


def test_python_wrappers_exist():
    sig = inspect.signature(capi.Context.seq_locate)
    assert list(sig.parameters) == ["self", "strings", "reference", "canonical"]
    assert sig.parameters["canonical"].default is True
    assert list(inspect.signature(capi.Context.seq_locate_raw).parameters)[:4] == ["self", "strings", "reference",
                                                                                  "canonical"]
    sig = inspect.signature(capi.KssIndex.colored_variants)
    assert list(sig.parameters)[:4] == ["self", "reference", "cols", "max_arm"]
    assert [sig.parameters[p].default for p in ("cols", "max_arm")] == [None, 8]
    sig = inspect.signature(capi.place_bubbles)
    assert list(sig.parameters) == ["strings", "k", "ends", "arm_offsets", "arm_strings", "where", "count",
                                    "ref_strings", "arm_rows", "n_cols"]
    assert list(inspect.signature(capi.vcf_lines).parameters) == ["records", "ref_names", "ref_lengths",
                                                                  "sample_names"]
    assert list(inspect.signature(capi.write_vcf).parameters) == ["path", "records", "ref_names", "ref_lengths",
                                                                  "sample_names"]


def test_plan_protocol_table_is_unchanged_and_complete():
    """The call has no handle among its parameters, so the closed table of tests/plan_protocol_cases.py neither
    lists it nor misses it, and every check of tests/test_plan_protocol_cpu.py holds with it declared."""
    import plan_protocol_cases as cases

    assert NAME not in cases.NEW_SYMBOLS and NAME not in cases.EXCLUDED
    assert not any(NAME in c["symbols"] for c in cases.INTRUDERS)
    protocol.test_every_plan_write_pair_is_a_victim()
    protocol.test_every_context_entry_point_is_an_intruder()

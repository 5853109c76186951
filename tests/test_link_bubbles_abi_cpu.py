"""ksh_link_bubbles through the layers that need no GPU: the header's declaration with the graph first, the built
library's export, the ctypes signature, every host refusal with pointers that are never dereferenced, the no-strings
answer, the Python wrappers' signatures, and the plan protocol's table staying complete without a new row (the call
takes the graph first and is neither a plan nor a write)."""
import ctypes as C
import inspect
import re

import plan_protocol_cases as cases
import test_plan_protocol_cpu as protocol
from kmersets import capi

NAME = "ksh_link_bubbles"


def test_header_declares_the_call_with_the_graph_first():
    decl = protocol.declarations()
    assert decl.get(NAME)[0] == "const ksh_link_graph* graph"
    assert NAME in capi.exported_symbols()
    text = re.sub(r"/\*.*?\*/", "", open(capi.HEADER).read(), flags=re.S)
    params = re.search(r"\bint\s+ksh_link_bubbles\s*\(([^)]*)\)", text).group(1)
    types = [" ".join(p.split()[:-1]) for p in params.split(",")]
    assert types == ["const ksh_link_graph*", "ksh_ctx*", "int32_t", "int64_t", "int64_t", "int64_t*", "int64_t*",
                     "int64_t*", "uint64_t*", "int64_t*", "int64_t*"]
    assert not NAME.endswith(("_plan", "_write"))
    assert re.search(r"#define\s+KSH_BUBBLE_MAX_ARM\s+64\b", text)
    fields = re.search(r"typedef struct ksh_link_graph \{(.*?)\} ksh_link_graph;", text, flags=re.S).group(1)
    assert [f.split()[-1] for f in fields.split(";") if f.strip()] == [name for name, _ in capi.LinkGraph._fields_]
    header = open(capi.HEADER).read()
    assert "CANONICAL" in header and "NOT A CARRIER" in header


def test_library_exports_it_with_a_signature():
    lib = capi.lib()
    assert hasattr(lib, NAME)
    fn = lib.ksh_link_bubbles
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[0] is C.POINTER(capi.LinkGraph) and fn.argtypes[2] is C.c_int32
    assert fn.argtypes[3] is C.c_int64 and fn.argtypes[4] is C.c_int64
    assert fn.argtypes[9] is C.POINTER(C.c_int64) and fn.argtypes[10] is C.POINTER(C.c_int64)
    assert C.sizeof(capi.LinkGraph) == 64


def test_host_refusals_need_no_device():
    """What is refused before anything touches a device."""
    lib = capi.lib()
    fake = 64  # (never dereferenced: every call below is refused before, or served on the host)
    ctx = C.c_void_p(fake)
    nb, na = C.c_int64(-1), C.c_int64(-1)
    rows = (C.c_uint64 * 4)(1, 0, 3, 0)
    size = C.sizeof(capi.LinkGraph)

    def graph(n=3, off=fake, to=fake, links=4, cls=None, table=None, n_classes=0, struct_size=size):
        return capi.LinkGraph(struct_size, n, off, to, links, cls, table, n_classes)

    def refused(word, g=None, ctx=ctx, max_arm=8, capacity=0, arm_capacity=0, outs=(None, None, None, None),
                counts=None):
        g = graph() if g is None else g
        counts = (C.byref(nb), C.byref(na)) if counts is None else counts
        rc = lib.ksh_link_bubbles(C.byref(g) if g else None, ctx, max_arm, capacity, arm_capacity, *outs, *counts)
        assert rc == capi.KSH_INVALID_ARGUMENT, (word, rc)
        assert word.encode() in lib.ksh_last_error(), (word, lib.ksh_last_error())

    refused("graph is NULL", g=False)
    refused("ctx is NULL", ctx=None)
    refused("n_bubbles is NULL", counts=(None, C.byref(na)))
    refused("n_arm_strings is NULL", counts=(C.byref(nb), None))
    refused("struct_size", g=graph(struct_size=size - 8))
    refused("n_strings = -1 is negative", g=graph(n=-1))
    refused("n_links = -2 is negative", g=graph(links=-2))
    refused("d_link_offsets is NULL", g=graph(off=None))
    refused("d_link_to is NULL", g=graph(to=None))
    refused("n_links = 25", g=graph(links=25))  # (more than 8 n)
    refused("n_links = 1", g=graph(n=0, off=None, links=1))
    for max_arm in (0, -1, 65):
        refused("max_arm = %d" % max_arm, max_arm=max_arm)
    refused("capacity = -1 is negative", capacity=-1)
    refused("arm_capacity = -3 is negative", arm_capacity=-3)
    refused("d_bubble_ends is NULL", capacity=2, arm_capacity=4, outs=(None, fake, fake, None))
    refused("d_arm_offsets is NULL", capacity=2, arm_capacity=4, outs=(fake, None, fake, None))
    refused("d_arm_strings is NULL with arm_capacity = 4", capacity=2, arm_capacity=4, outs=(fake, fake, None, None))
    refused("both or neither (rows is NULL)", g=graph(cls=fake))
    refused("both or neither (d_string_class is NULL)", g=graph(table=rows, n_classes=2))
    for n_classes in (0, -1, (1 << 24) + 1):
        refused("n_classes = %d" % n_classes, g=graph(cls=fake, table=rows, n_classes=n_classes))
    refused("d_arm_rows is given", outs=(None, None, None, fake))
    refused("d_arm_rows is NULL with classes", g=graph(cls=fake, table=rows, n_classes=2), capacity=2, arm_capacity=4,
            outs=(fake, fake, fake, None))
    assert (nb.value, na.value) == (-1, -1)  # no refusal has written them
    # no strings: served on the host when it only counts, with or without classes
    for g in (graph(n=0, off=None, to=None, links=0), graph(n=0, off=fake, to=fake, links=0),
              graph(n=0, off=None, to=None, links=0, cls=fake, table=rows, n_classes=2)):
        nb.value = na.value = -1
        assert lib.ksh_link_bubbles(C.byref(g), ctx, 8, 0, 0, None, None, None, None, C.byref(nb),
                                    C.byref(na)) == capi.KSH_OK
        assert (nb.value, na.value) == (0, 0)


def test_python_wrappers_exist():
    assert callable(capi.Context.link_bubbles) and callable(capi.KssIndex.colored_bubbles)
    sig = inspect.signature(capi.Context.link_bubbles)
    assert list(sig.parameters) == ["self", "link_offsets", "link_to", "max_arm", "string_class", "rows"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [8, None, None]
    raw = inspect.signature(capi.Context.link_bubbles_raw)
    assert list(raw.parameters)[:6] == ["self", "link_offsets", "link_to", "max_arm", "capacity", "arm_capacity"]
    sig = inspect.signature(capi.KssIndex.colored_bubbles)
    assert list(sig.parameters) == ["self", "cols", "max_arm", "route", "pass_positions"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None, 8, 0, 0]
    sig = inspect.signature(capi.bubble_alleles)
    assert list(sig.parameters) == ["strings", "k", "ends", "arm_offsets", "arm_strings"]
    lines = inspect.signature(capi.bubble_lines)
    assert list(lines.parameters)[:5] == list(sig.parameters)
    assert list(inspect.signature(capi.write_bubbles).parameters) == ["path"] + list(lines.parameters)
    assert "not a carrier" in capi.Context.link_bubbles.__doc__
    # TTACGTA -> {ACGTAC | ACGTAG} ... -> the sink, K = 5: strings 1 and 2 are the arms, string 2 reversed
    strings = ["TTACGT", "ACGTAGGCA", "TGCCGACGT", "GGCAT"]
    assert capi.bubble_alleles(strings, 5, [[0, 6]], [0, 1, 2], [2, 5]) == [(0, 6, "ACGTAGGCA", "ACGTCGGCA")]
    assert capi.bubble_lines(strings, 5, [[0, 6]], [0, 1, 2], [2, 5], [[5, 0], [0, 1]], 128) == [
        "0\t6\tACGTAGGCA\tACGTCGGCA\t0,2\t64"]
    assert capi.bubble_lines(strings, 5, [[0, 6]], [0, 1, 2], [2, 5], [[2, 0], [0, 0]], 3)[0].endswith("\t1\t.")


def test_plan_protocol_table_is_unchanged_and_complete():
    """The call is no plan and no write, so the table has no row for it; it takes a context behind its request, so it
    is an intruder column on the victim's context and on the second one, it ends no plan, and every check of
    tests/test_plan_protocol_cpu.py holds."""
    mine = [c for c in cases.INTRUDERS if NAME in c["symbols"]]
    assert {c["where"] for c in mine} == {"own", "second"} and NAME not in cases.EXCLUDED
    assert all(c["refuses"] == () for c in mine) and any(not c["op"].startswith("fail:") for c in mine)
    protocol.test_every_plan_write_pair_is_a_victim()
    protocol.test_every_context_entry_point_is_an_intruder()
    protocol.test_refusals_only_where_the_contract_permits()

"""The case table of the plan / write protocol tests (no GPU needed): victims, intruders and every cell's outcome.

A *victim* is one plan / write pair of the C ABI with a plan pending; an *intruder* is whatever a caller may issue
between the plan and its write.  include/kmersets_hip.h ("Plans") states the contract: the write is then either
`exact` (KSH_OK and the true result) or `refused` (KSH_FAILED_PRECONDITION naming the missing plan, no output
touched, the context usable), and it may be refused only after a plan of the victim's own group, a composite call
that plans on the context itself, or a release.  tests/test_plan_protocol_cpu.py guards this table against the
header's exported symbols and against that rule; tests/test_gpu_plan_protocol.py runs every cell.

The outcome of a cell is written column-wise: every intruder lists the victim kinds whose pending plan it ends
(`refuses`); every other victim's write is `exact`.  The header's table mirrors the columns."""

EXACT, REFUSED = "exact", "refused"

# ---- victims ---------------------------------------------------------------------------------------------------
# kind -> (plan symbol, write symbol, group)
KINDS = {
    "pair": ("ksh_pair_plan", "ksh_pair_write", "pair"),
    "union": ("ksh_set_union_plan", "ksh_set_union_write", "pair"),
    "decode": ("ksh_spss_decode_plan", "ksh_spss_decode_write", "decode"),
    "count": ("ksh_spss_decode_plan", "ksh_kmer_count_write", "decode"),
    "encode": ("ksh_spss_encode_plan", "ksh_spss_encode_write", "encode"),
    "cover": ("ksh_spss_cover_plan", "ksh_spss_cover_write", "encode"),
    "from_text": ("ksh_spss_from_text_plan", "ksh_spss_from_text_write", "text"),
    "fasta": ("ksh_fasta_plan", "ksh_fasta_write", "text"),
}
# The writes that name no input have two forms (the header's "Plans"): the plain one is the victim's `_write`
# symbol itself, the `_for` one states the plan it means.  Both are victims, with the same table.
NAMELESS = ("encode", "cover", "from_text", "fasta")
GROUPS = {}
for _kind, (_p, _w, _group) in KINDS.items():
    GROUPS.setdefault(_group, []).append(_kind)

# (k, N, device key bytes): the three key widths the suite uses at N = 14, and the wide decode route (N > 14)
NARROW = [(15, 14, 2), (23, 14, 4), (31, 14, 8)]
WIDE = [(23, 16, 4), (31, 20, 8)]
EMPTY_GEOM = (23, 14, 4)
VICTIM_KMERS = 20000
LARGE_KMERS = 2000000


def _victims():
    rows = []
    for kind in KINDS:
        for plain in ((False, True) if kind in NAMELESS else (False,)):
            for geom in NARROW:
                rows.append({"kind": kind, "geom": geom, "empty": False, "plain": plain})
            if kind in ("decode", "count"):
                for geom in WIDE:
                    rows.append({"kind": kind, "geom": geom, "empty": False, "plain": plain})
            rows.append({"kind": kind, "geom": EMPTY_GEOM, "empty": True, "plain": plain})
    for r in rows:
        r["id"] = "%s-k%d-N%d-u%d%s%s" % ((r["kind"],) + r["geom"][:2] + (
            8 * r["geom"][2], "-empty" if r["empty"] else "", "-plain" if r["plain"] else ""))
    return rows


VICTIMS = _victims()


def other_geom(geom):
    """The intruder geometry "at another key width": the next of the three widths at N = 14."""
    kb = geom[2]
    return {2: NARROW[1], 4: NARROW[2], 8: NARROW[0]}[kb]


# ---- intruders -------------------------------------------------------------------------------------------------
# op -> the exported entry points it calls
OPS = {
    "hash": ("ksh_set_hash",),
    "contains": ("ksh_set_contains",),
    "kmers": ("ksh_set_kmers",),
    "diff": ("ksh_set_diff",),
    "weights": ("ksh_pair_weights",),
    "algebra": ("ksh_pair_algebra",),
    "batch": ("ksh_pair_algebra_batch",),
    "dsu": ("ksh_dsu_components",),
    "svb": ("ksh_svb_encode_0124", "ksh_svb_decode_0124"),
    "size": ("ksh_spss_size",),
    "to_text": ("ksh_spss_to_text",),
    "copies": ("ksh_ctx_memcpy_h2d", "ksh_ctx_memcpy_d2h", "ksh_ctx_memcpy_d2d"),
    "ctx_misc": ("ksh_ctx_sync", "ksh_ctx_enable_timing", "ksh_ctx_timing_reset", "ksh_ctx_timing_read",
                 "ksh_ctx_timing_units", "ksh_ctx_timing_wall", "ksh_ctx_mem_stats"),
    "reserve": ("ksh_ctx_reserve", "ksh_ctx_mem_stats"),
    "lanes": ("ksh_ctx_set_lanes",),
    "release:encode": ("ksh_spss_encode_release",),
    "release:cover": ("ksh_spss_cover_release",),
    "fail:decode": ("ksh_spss_decode_plan",),    # a view that declares more bases than its strings hold
    "fail:cover": ("ksh_spss_cover_plan",),      # the same view
    "fail:from_text": ("ksh_spss_from_text_plan",),  # a byte outside ACGT and '\n'
    "fail:fasta": ("ksh_fasta_plan",),           # an odd number of lines
    "fail:encode": ("ksh_spss_encode_plan",),    # an even-k canonical set with a self-reverse-complement k-mer
    "kss_build:lanes1": ("ksh_ctx_set_lanes", "ksh_kss_build", "ksh_kss_size", "ksh_kss_node", "ksh_kss_children",
                         "ksh_kss_meta", "ksh_kss_trace", "ksh_kss_initial_weights", "ksh_kss_stats",
                         "ksh_kss_encode_counts", "ksh_kss_weighed_counts", "ksh_kss_phase_seconds",
                         "ksh_kss_node_holder", "ksh_kss_comm_stats"),
    "kss_build:default": ("ksh_ctx_set_lanes", "ksh_kss_build", "ksh_kss_size", "ksh_kss_node", "ksh_kss_stats"),
    "kss_get": ("ksh_kss_get",),
    # the two indexes stay open in the row's state for the columns behind them: the owned one (it decodes its nodes) ...
    "kss_index_create": ("ksh_kss_index_create", "ksh_kss_index_info", "ksh_kss_index_query", "ksh_kss_index_routes"),
    # ... and the one that borrows the node sets of the build before it
    "kss_index_query": ("ksh_kss_index_from_kss", "ksh_kss_index_info", "ksh_kss_index_query", "ksh_kss_index_routes"),
    "kss_index_close": ("ksh_kss_index_destroy",),
    "kss_destroy": ("ksh_kss_destroy",),
    # the calls that take their request first and an index or a context behind it.  Each op calls these symbols and
    # nothing else: offsets, run lists and graphs come from the host references, not from a sibling call
    "seq_hits": ("ksh_seq_hits",),
    "pair_counts": ("ksh_kss_pair_counts",),
    "select": ("ksh_kss_select_count", "ksh_kss_select_keys"),
    "classes": ("ksh_kss_color_classes",),
    "class_ids": ("ksh_kss_select_class_ids",),
    "class_runs": ("ksh_seq_class_runs",),
    "cut": ("ksh_spss_cut",),
    "links": ("ksh_spss_links",),
    "bubbles": ("ksh_link_bubbles",),
    "fail:select_keys": ("ksh_kss_select_keys",),   # the offsets of another request
    "fail:cut": ("ksh_spss_cut",),                   # run offsets that descend
    "fail:links_end": ("ksh_spss_links",),           # a container with a repeated end k-mer
    "fail:links_capacity": ("ksh_spss_links",),      # capacity one short of n_links
    "fail:bubbles": ("ksh_link_bubbles",),           # a link that has no twin
    # ~2 * 10^6 k-mers, so that scratch the context owns must grow while the victim's plan is pending
    # (asserted through ksh_ctx_mem_stats): the arena ...
    "large:arena": ("ksh_pair_algebra", "ksh_spss_to_text", "ksh_ctx_mem_stats"),
    # ... and ctx->plan, the decode slot and the text slot
    "large:plans": ("ksh_pair_plan", "ksh_pair_write", "ksh_spss_decode_plan", "ksh_spss_decode_write",
                    "ksh_spss_from_text_plan", "ksh_spss_from_text_write_for", "ksh_ctx_mem_stats"),
}
for _kind, (_p, _w, _group) in KINDS.items():
    if _kind in NAMELESS:  # the wrappers write with the `_for` form; plain:<kind> is the three-argument write
        OPS["plain:" + _kind] = (_p, _w)
        _w = _w + "_for"
    OPS["full:" + _kind] = (_p, _w) + {"encode": ("ksh_spss_encode_stats", "ksh_spss_encode_routes"),
                                       "cover": ("ksh_spss_cover_stats",)}.get(_kind, ())
    OPS["abandon:" + _kind] = (_p,)

# What an op does to the pending plans of the context it runs on: op -> (victim kinds refused afterwards, reason).
# reason: "group" (it holds a plan of that group), "composite" (it plans on the context for itself), "release".
# Ops that are not listed end nothing.  ksh_ctx_set_lanes and ksh_kss_index_query may end plans by the contract
# and do not.
ENDS = {
    "release:encode": (("encode", "cover"), "release"),
    "release:cover": (("encode", "cover"), "release"),
    "fail:decode": (("decode", "count"), "group"),
    "fail:cover": (("encode", "cover"), "group"),
    "fail:from_text": (("from_text", "fasta"), "group"),
    "fail:fasta": (("from_text", "fasta"), "group"),
    "fail:encode": (("encode", "cover"), "group"),
    # the build runs pair plans, decodes and encodes; which of them on the context itself depends on the lanes and
    # the memory, so it ends all three groups when it starts
    "kss_build:lanes1": (("pair", "union", "decode", "count", "encode", "cover"), "composite"),
    "kss_build:default": (("pair", "union", "decode", "count", "encode", "cover"), "composite"),
    "kss_get": (("pair", "union"), "composite"),               # union plans
    "kss_index_create": (("decode", "count"), "composite"),    # decodes
    "large:plans": (("pair", "union", "decode", "count", "from_text", "fasta"), "group"),
}
for _kind, (_p, _w, _group) in KINDS.items():
    ENDS["full:" + _kind] = (tuple(GROUPS[_group]), "group")
    ENDS["abandon:" + _kind] = (tuple(GROUPS[_group]), "group")
    if _kind in NAMELESS:
        ENDS["plain:" + _kind] = (tuple(GROUPS[_group]), "group")

COMPOSITE_SYMBOLS = ("ksh_kss_build", "ksh_kss_build_sharded", "ksh_kss_build_owned", "ksh_kss_get",
                     "ksh_kss_index_create", "ksh_kss_index_query")
RELEASE_SYMBOLS = ("ksh_spss_encode_release", "ksh_spss_cover_release", "ksh_ctx_set_lanes")

# The ten entry points whose context or index is not their first parameter, as ops: those that read an index ...
INDEX_OPS = ["seq_hits", "pair_counts", "select", "classes", "class_ids", "class_runs"]
# ... and those that take the context itself (the bubbles have no key width: each width has a graph of its own)
STRING_OPS = ["cut", "links", "bubbles"]
NEW_SYMBOLS = ("ksh_seq_hits", "ksh_kss_pair_counts", "ksh_kss_select_count", "ksh_kss_select_keys",
               "ksh_kss_color_classes", "ksh_kss_select_class_ids", "ksh_seq_class_runs", "ksh_spss_cut",
               "ksh_spss_links", "ksh_link_bubbles")
NEW_FAILING = ["fail:select_keys", "fail:cut", "fail:links_end", "fail:links_capacity", "fail:bubbles"]

# ops issued at the victim's geometry and at another key width (on data other than the victim's)
_TWO_WIDTHS = ["hash", "contains", "kmers", "diff", "weights", "algebra", "batch", "size", "to_text"] + STRING_OPS + \
              ["%s:%s" % (how, kind) for how in ("full", "abandon") for kind in KINDS] + \
              ["plain:" + kind for kind in NAMELESS]
# ops without a key width, or with a geometry of their own
_ONE = ["dsu", "svb", "copies", "ctx_misc", "reserve", "lanes", "release:encode", "release:cover", "fail:decode",
        "fail:cover", "fail:from_text", "fail:fasta", "fail:encode", "fail:cut", "fail:links_end",
        "fail:links_capacity", "fail:bubbles"]


def _kss(widths):
    """The columns that need a built structure, in this order: the later ones use what the earlier ones left in the
    row's state.  A build, the index that borrows its sets and the index that decodes the node containers, per width
    (an index must exist before the victim plans: ksh_kss_index_create ends decode plans by contract, which would
    mask what the calls on the index do); every index op on both indexes; the indexes closed, the builds destroyed;
    then the build with the default lanes."""
    cols = []
    for width in widths:
        cols += [("kss_build:lanes1", width), ("kss_index_query", width)]
        cols += [("kss_get", width)] if width == "same" else []
        cols += [("kss_index_create", width)]
    cols += [(op, width) for op in INDEX_OPS for width in widths] + [("fail:select_keys", "same")]
    cols += [("kss_index_close", width) for width in widths] + [("kss_destroy", width) for width in widths]
    return cols + [("kss_build:default", "same"), ("kss_get", "same"), ("kss_destroy", "same")]


def _intruders():
    cols = []

    def add(op, width, where):
        ends, why = ENDS.get(op, ((), None))
        if where == "second":  # nothing done on another context touches this one's plans
            ends, why = (), None
        cols.append({"op": op, "width": width, "where": where, "refuses": tuple(ends), "why": why,
                     "symbols": OPS[op]})

    for op in _TWO_WIDTHS:
        add(op, "same", "own")
        add(op, "other", "own")
    for op in _ONE:
        add(op, "same", "own")
    add("large:arena", "same", "own")
    add("large:plans", "same", "own")
    for op, width in _kss(("same", "other")):
        add(op, width, "own")
    # the same intruders on a second context (one width)
    for op in _TWO_WIDTHS + _ONE:
        add(op, "same", "second")
    for op, width in _kss(("same",)):
        add(op, width, "second")
    seen = {}
    for c in cols:
        base = "%s@%s%s" % (c["op"], c["width"], "" if c["where"] == "own" else "/ctx2")
        seen[base] = seen.get(base, 0) + 1
        c["id"] = base if seen[base] == 1 else "%s#%d" % (base, seen[base])
    return cols


INTRUDERS = _intruders()


def outcome(victim, intruder):
    """The expected outcome of the victim's write after the intruder."""
    return REFUSED if victim["kind"] in intruder["refuses"] else EXACT


TABLE = {(v["id"], c["id"]): outcome(v, c) for v in VICTIMS for c in INTRUDERS}

# Exported entry points that take a context, a KmerSetSet or an index and that no intruder calls, with the reason
EXCLUDED = {
    "ksh_ctx_create": "takes no context: it makes one (every row and the second context go through it)",
    "ksh_ctx_destroy": "ends the context and every plan in it; there is no write to judge afterwards",
    "ksh_kss_build_sharded": "multi-rank build: needs ranks and an all-gather",
    "ksh_kss_build_owned": "multi-rank build: needs ranks and a communicator",
    "ksh_comm_create_rccl": "needs ranks (one process per GPU)",
    "ksh_comm_create_custom": "needs ranks and a transport",
}


# ---- the inputs and the truth of the index and string ops --------------------------------------------------------
# Host only, made once per geometry and shared by tests/test_plan_protocol_cpu.py (which asserts that none of the
# expected values is vacuous) and tests/test_gpu_plan_protocol.py (which uploads them).  The truth is numpy set algebra
# and the tests' own references -- index_reference, paint_reference, spss_cut_reference, spss_links_reference,
# link_bubbles_reference -- never the library.
KSS_SETS, KSS_KMERS = 4, 3000
COLS = [2, 0, 3, 1]                         # the columns of every index op: the four inputs, permuted
REQUEST_A = dict(cols=COLS, min_count=2)    # the selection the table's columns make
REQUEST_B = dict(cols=[1, 3], max_count=1)  # another request on the same index (other columns)
COLS_B = [1, 3]
_MADE = {}


def _once(key, make):
    if key not in _MADE:
        _MADE[key] = make()
    return _MADE[key]


def kss_sets(k):
    """The four input sets of the table's KmerSetSet builds, sorted uint64 arrays."""
    def make():
        import numpy as np
        from kmersets import synth

        sets = [np.asarray(s, dtype=np.uint64) for s in synth.phylogeny_sets(k, KSS_SETS, KSS_KMERS, seed=77 + k)]
        assert all((s[1:] > s[:-1]).all() for s in sets)
        return sets
    return _once(("sets", k), make)


def kss_strings(k):
    """The oracle's SPSS strings of every input set."""
    def make():
        import geometry_families as gf
        import oracle_lib as ol

        return [ol.Set.from_kmers(k, *gf.ref_geom(k), s).spss() for s in kss_sets(k)]
    return _once(("strings", k), make)


def sequences(k):
    """A dozen strings of 200 to 300 bases: two windows of every input's strings, the second reverse-complemented
    (their k-mers hit), and four random ones (theirs miss)."""
    def make():
        from index_reference import revcomp_string
        from kmersets import synth

        out = []
        for i, strings in enumerate(kss_strings(k)):
            text = max(strings, key=len)
            assert len(text) >= 1500
            out += [text[100 * i:100 * i + 300], revcomp_string(text[700 + 90 * i:950 + 97 * i])]
        out += [synth.string_of_bases(synth.random_genome(200 + 17 * j, 0xC0FFEE + 31 * k + j)) for j in range(4)]
        return out
    return _once(("sequences", k), make)


def index_case(geom):
    """The truth of the six index ops at one geometry.  The reference is the membership matrix of the four inputs
    without a DAG: that is the owned index of the table (four nodes, no children), and over the columns 0..3 it is
    the index that borrows a built structure too -- Get(i) of an input is the input, and a build holds no k-mer that
    no input holds, so the counts of the whole structure (n_distinct, spectrum[0], the zero row) agree as well."""
    def make():
        import numpy as np

        import paint_reference as pr
        from index_reference import IndexReference

        k, n, kb = geom
        sets = kss_sets(k)
        ref = IndexReference(k, sets, [[] for _ in sets])
        strings = sequences(k)
        rows, counts = ref.color_classes(COLS)
        table = pr.with_zero_row(rows)
        case = {"ref": ref, "strings": strings, "hits": ref.seq_hits(strings, True), "pairs": ref.pair_table(COLS),
                "n_distinct": ref.n_distinct, "rows": rows, "counts": counts, "table": table, "select": {},
                "runs": {}, "spectrum": {}, "class_ids": {}}
        for name, request in (("A", REQUEST_A), ("B", REQUEST_B)):
            kmers = ref.select(**request)
            case["select"][name] = (kmers,) + ref.bucketed(kmers, n, kb)
            case["spectrum"][name] = ref.spectrum(request["cols"])
            # the union of the request's columns with the class of every k-mer, over the request's own table
            own_rows = ref.color_classes(request["cols"])[0]
            own_rows = own_rows[own_rows.any(axis=1)]  # (a k-mer of the union is in some column)
            kmers, ids = ref.class_ids(own_rows, cols=request["cols"])
            case["class_ids"][name] = (own_rows, kmers) + ref.bucketed(kmers, n, kb) + (ids.astype(np.int32),)
            cols = request["cols"]
            own_table = pr.with_zero_row(ref.color_classes(cols)[0])
            case["runs"][name] = (own_table,) + pr.class_runs(ref, strings, cols, own_table, True)
        return case
    return _once(("index", geom), make)


def cut_case(k):
    """(strings, run offsets, run starts) of the cut op: the seeded random case of spss_cut_cases at this K, or, where
    the designed cases have no such K, one made by their builder."""
    def make():
        import spss_cut_cases as cc

        found = [c for c in cc.CASES if c["id"] == "random_p0.02-k%d" % k]
        if found:
            return found[0]
        return cc.make_case("protocol", k, [50, 1, 40, 30, 1, 60, 200, 2],
                            [[10, 20, 30], [], [5], [7, 9, 11], [], [1], [64, 65, 150], []], [cc.HAS_CUT], 900 + k)
    return _once(("cut", k), make)


def descending_offsets(case):
    """The cut case's run offsets with off[3] above off[4] ("string 3 has no run")."""
    bad = case["offsets"].copy()
    bad[3] = bad[4] + 1
    return bad


def links_case(k, which="A"):
    """The strings of the links op.  A: the seeded random case of spss_links_cases at this K, the orientations case
    where there is no random one, else a chain made by their builder on the orientations recipe.  B: another, smaller
    container at the same K."""
    def make():
        import spss_links_cases as lc

        if which == "B":
            return lc.search(lambda seed: lc.chain(k, [4, 2, 3], [0, 1, 0], seed), k, (True, False), 2000 + k)
        for prefix in ("random_1500", "orientations"):
            found = [c for c in lc.CASES if c["id"] == "%s-k%d" % (prefix, k)]
            if found:
                return found[0]["strings"]
        sizes, flips = [7, 5, 6, 4, 9, 1, 8, 1, 6], [0, 0, 1, 1, 0, 0, 0, 1, 1]
        return lc.search(lambda seed: lc.chain(k, sizes, flips, seed), k, (True, False), 400 + k)
    return _once(("links", k, which), make)


def repeated_end(k):
    """The links container with one more string, which begins with the first k-mer of string 1."""
    def make():
        from kmersets import synth

        strings = list(links_case(k))
        tail = synth.string_of_bases(synth.random_genome(30, 0xE2D + k))
        return strings + [strings[1][:k] + tail]
    return _once(("repeated_end", k), make)


BUBBLE_GRAPHS = {2: "family-11", 4: "back-to-back", 8: "family-12"}  # key bytes -> a case of link_bubbles_cases


def bubbles_case(kb):
    """(off, to, max_arm, string_class, rows) of the bubbles op: a graph has no key width, so each width takes a graph
    of its own from link_bubbles_cases, with classes."""
    def make():
        import link_bubbles_cases as bc

        name = BUBBLE_GRAPHS[kb]
        if name.startswith("family"):
            f = next(f for f in bc.families() if f["id"] == name)
            return f["off"], f["to"], f["max_arm"], f["string_class"], f["rows"]
        c = next(c for c in bc.CASES if c["id"] == name)
        return c["off"], c["to"], c["max_arm"], bc.classes_of(c["n"]), bc.ROWS
    return _once(("bubbles", kb), make)


BUBBLES_MAX_ARM_B = 1  # request B of the bubbles: the same graph with another max_arm


def no_twin(kb):
    """The bubbles graph with the first link of its first two-link row turned to the other orientation."""
    off, to = bubbles_case(kb)[:2]
    row = next(v for v in range(len(off) - 1) if off[v + 1] - off[v] == 2)
    bad = to.copy()
    bad[off[row]] ^= 1
    return bad

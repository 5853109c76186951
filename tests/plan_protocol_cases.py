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
    "kss_index_create": ("ksh_kss_index_create", "ksh_kss_index_info", "ksh_kss_index_destroy"),
    "kss_index_query": ("ksh_kss_index_from_kss", "ksh_kss_index_query", "ksh_kss_index_routes",
                        "ksh_kss_index_destroy"),
    "kss_destroy": ("ksh_kss_destroy",),
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

# ops issued at the victim's geometry and at another key width (on data other than the victim's)
_TWO_WIDTHS = ["hash", "contains", "kmers", "diff", "weights", "algebra", "batch", "size", "to_text"] + \
              ["%s:%s" % (how, kind) for how in ("full", "abandon") for kind in KINDS] + \
              ["plain:" + kind for kind in NAMELESS]
# ops without a key width, or with a geometry of their own
_ONE = ["dsu", "svb", "copies", "ctx_misc", "reserve", "lanes", "release:encode", "release:cover", "fail:decode",
        "fail:cover", "fail:from_text", "fail:fasta", "fail:encode"]
# in this order: the later ones use the structure the build left on the context
_KSS = ["kss_build:lanes1", "kss_index_query", "kss_get", "kss_index_create", "kss_destroy", "kss_build:default",
        "kss_get", "kss_destroy"]


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
    for op in _KSS:
        add(op, "same", "own")
    # the same intruders on a second context (one width)
    for op in _TWO_WIDTHS + _ONE + _KSS:
        add(op, "same", "second")
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

# Exported entry points whose first parameter is a context or a KmerSetSet and that no intruder calls, with the reason
EXCLUDED = {
    "ksh_ctx_create": "takes no context: it makes one (every row and the second context go through it)",
    "ksh_ctx_destroy": "ends the context and every plan in it; there is no write to judge afterwards",
    "ksh_kss_build_sharded": "multi-rank build: needs ranks and an all-gather",
    "ksh_kss_build_owned": "multi-rank build: needs ranks and a communicator",
    "ksh_comm_create_rccl": "needs ranks (one process per GPU)",
    "ksh_comm_create_custom": "needs ranks and a transport",
}

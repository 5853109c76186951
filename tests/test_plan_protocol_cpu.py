"""Guards the plan / write protocol table (tests/plan_protocol_cases.py) against the header: no GPU needed.

The table decides which sequences tests/test_gpu_plan_protocol.py issues and what it expects of each; these checks
keep it complete (every two-call pair is a victim, every entry point that takes a context is an intruder) and
honest (a refusal only where include/kmersets_hip.h, "Plans", permits one; at most half of a victim's cells)."""
import re

import numpy as np
import pytest

import plan_protocol_cases as cases
from kmersets import capi


def declarations():
    """name -> the types and names of all its parameters (a list of str), for every function the header declares."""
    text = open(capi.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(ksh_[a-z0-9_]+)\s*\(([^()]*)\)", text):
        out[name] = [" ".join(p.split()) for p in params.split(",")]
    return out


HANDLE = re.compile(r"^(const )?ksh_(ctx|kss|kss_index)\s*\*")


def takes_a_context(params):
    """Is any parameter a (const) ksh_ctx*, ksh_kss* or ksh_kss_index*?  (Whichever position: the calls added behind
    the index take their request first.)"""
    return any(HANDLE.match(p) for p in params)


def test_every_plan_write_pair_is_a_victim():
    symbols = capi.exported_symbols()
    two_call = {s for s in symbols if s.endswith("_plan") or s.endswith("_write")}
    in_table = {s for plan, write, _ in cases.KINDS.values() for s in (plan, write)}
    assert two_call == in_table
    assert len(cases.KINDS) == 8 and sorted(cases.GROUPS) == ["decode", "encode", "pair", "text"]
    assert all(len(kinds) == 2 for kinds in cases.GROUPS.values())


def test_victim_rows():
    """The eight pairs at the three key widths, the decode and the count on the wide route too, each pair once
    with an empty input."""
    rows = cases.VICTIMS
    assert len({r["id"] for r in rows}) == len(rows)
    for kind in cases.KINDS:
        mine = [r for r in rows if r["kind"] == kind]
        assert {r["geom"] for r in mine if not r["empty"]} >= set(cases.NARROW), kind
        assert {r["geom"][2] for r in mine if not r["empty"]} == {2, 4, 8}, kind
        forms = {r["plain"] for r in mine}
        assert forms == ({False, True} if kind in cases.NAMELESS else {False}), kind
        for plain in forms:  # every form of the write: the three widths and one empty input
            of_form = [r for r in mine if r["plain"] == plain]
            assert {r["geom"][2] for r in of_form if not r["empty"]} == {2, 4, 8}, kind
            assert sum(r["empty"] for r in of_form) == 1, kind
    for kind in ("decode", "count"):
        wide = {r["geom"] for r in rows if r["kind"] == kind and r["geom"][1] > 14}
        assert wide == {(23, 16, 4), (31, 20, 8)}
    for k, n, kb in cases.NARROW + cases.WIDE:
        assert capi.geom(k, n).key_bytes == kb
        assert cases.other_geom((k, n, kb))[2] != kb


REQUEST_FIRST = ("ksh_seq_hits", "ksh_kss_pair_counts", "ksh_kss_select_count", "ksh_kss_select_keys",
                 "ksh_kss_color_classes", "ksh_kss_select_class_ids", "ksh_seq_class_runs", "ksh_spss_cut",
                 "ksh_spss_links", "ksh_link_bubbles")


def test_every_context_entry_point_is_an_intruder():
    decl = declarations()
    assert set(decl) == set(capi.exported_symbols())
    takes_ctx = {name for name, params in decl.items() if takes_a_context(params)}
    assert "ksh_pair_plan" in takes_ctx and "ksh_kss_get" in takes_ctx and "ksh_kss_index_query" in takes_ctx
    assert "ksh_malloc" not in takes_ctx and "ksh_last_error" not in takes_ctx
    # the calls whose handle is their second or third parameter: whatever becomes of the rule, these stay in
    assert set(REQUEST_FIRST) <= takes_ctx, set(REQUEST_FIRST) - takes_ctx
    assert not any(HANDLE.match(decl[name][0]) for name in REQUEST_FIRST)
    assert len(cases.EXCLUDED) == 6  # (the list of what no intruder calls does not grow)
    called = {s for c in cases.INTRUDERS for s in c["symbols"]}
    assert called <= set(decl), called - set(decl)
    missing = takes_ctx - called - set(cases.EXCLUDED)
    assert not missing, "%d entry points take a context and are no intruder: %s" % (len(missing), ", ".join(sorted(missing)))
    for name, reason in cases.EXCLUDED.items():
        assert name in decl and name not in called and reason
    assert set(cases.NEW_SYMBOLS) == set(REQUEST_FIRST) and len(cases.NEW_SYMBOLS) == 10


def test_intruder_columns():
    cols = cases.INTRUDERS
    assert len({c["id"] for c in cols}) == len(cols)
    ops = {(c["op"], c["width"], c["where"]) for c in cols}
    for kind in cases.KINDS:  # each victim kind as a full plan + write and as an abandoned plan, at both widths
        for how in ("full", "abandon"):
            for width in ("same", "other"):
                assert ("%s:%s" % (how, kind), width, "own") in ops
    for op in ("fail:decode", "fail:from_text", "fail:fasta", "fail:encode", "kss_build:lanes1", "kss_build:default",
               "kss_get", "kss_index_create", "kss_index_query", "reserve", "large:arena", "large:plans",
               "kss_index_close") + tuple(cases.INDEX_OPS + cases.STRING_OPS + cases.NEW_FAILING):
        assert any(c["op"] == op and c["where"] == "own" for c in cols), op
    # the ten calls added behind the index: at both key widths on the victim's context, and on the second one; their
    # failing variants on both contexts; none of them ends a plan
    for op in cases.INDEX_OPS + cases.STRING_OPS:
        for width, where in (("same", "own"), ("other", "own"), ("same", "second")):
            assert (op, width, where) in ops, (op, width, where)
    for op in cases.NEW_FAILING:
        assert (op, "same", "own") in ops and (op, "same", "second") in ops, op
    for c in cols:
        if c["op"] in cases.INDEX_OPS + cases.STRING_OPS + cases.NEW_FAILING:
            assert c["refuses"] == () and set(c["symbols"]) <= set(cases.NEW_SYMBOLS), c["id"]
    assert {s for op in cases.INDEX_OPS + cases.STRING_OPS for s in cases.OPS[op]} == set(cases.NEW_SYMBOLS)
    assert not set(cases.INDEX_OPS + cases.STRING_OPS + cases.NEW_FAILING) & set(cases.ENDS)
    # an index op runs behind the columns that open its indexes and before the one that closes them, per context
    for where in ("own", "second"):
        order = [(c["op"], c["width"]) for c in cols if c["where"] == where]
        for op, width in order:
            if op in cases.INDEX_OPS + ["fail:select_keys"]:
                at = order.index((op, width))
                for opener in ("kss_build:lanes1", "kss_index_query", "kss_index_create"):
                    assert order.index((opener, width)) < at < order.index(("kss_index_close", width)), (op, width)
                assert order.index(("kss_index_close", width)) < order.index(("kss_destroy", width))
    # whatever is issued on the victim's context is issued on a second one too
    own = {c["op"] for c in cols if c["where"] == "own" and not c["op"].startswith("large:")}
    assert own == {c["op"] for c in cols if c["where"] == "second"}
    assert cases.LARGE_KMERS >= 100 * cases.VICTIM_KMERS


def permitted(victim_kind, col):
    """May this intruder end the victim's pending plan?  (include/kmersets_hip.h, "Plans": a plan of the same
    group, a composite call, a release or ksh_ctx_set_lanes -- and only on the victim's own context.)"""
    if col["where"] != "own":
        return False
    group = cases.KINDS[victim_kind][2]
    same_group_plans = {cases.KINDS[k][0] for k in cases.GROUPS[group]}
    syms = set(col["symbols"])
    return bool(syms & same_group_plans or syms & set(cases.COMPOSITE_SYMBOLS) or syms & set(cases.RELEASE_SYMBOLS))


def test_refusals_only_where_the_contract_permits():
    by_id = {c["id"]: c for c in cases.INTRUDERS}
    assert set(cases.TABLE.values()) == {cases.EXACT, cases.REFUSED}
    assert len(cases.TABLE) == len(cases.VICTIMS) * len(cases.INTRUDERS)
    for v in cases.VICTIMS:
        for cid, col in by_id.items():
            if cases.TABLE[(v["id"], cid)] == cases.REFUSED:
                assert permitted(v["kind"], col), (v["id"], cid)
                assert col["why"] in ("group", "composite", "release")
    # the listed reason is the true one
    for col in cases.INTRUDERS:
        for kind in col["refuses"]:
            group = cases.KINDS[kind][2]
            if col["why"] == "group":
                assert set(col["symbols"]) & {cases.KINDS[k][0] for k in cases.GROUPS[group]}, col["id"]
            elif col["why"] == "composite":
                assert set(col["symbols"]) & set(cases.COMPOSITE_SYMBOLS), col["id"]
            else:
                assert col["why"] == "release" and set(col["symbols"]) & set(cases.RELEASE_SYMBOLS), col["id"]
    # a release ends the plans of the encode / cover slot and nothing else
    for col in cases.INTRUDERS:
        if col["why"] == "release":
            assert set(col["refuses"]) == {"encode", "cover"}


def test_at_least_half_of_every_victims_cells_are_exact():
    for v in cases.VICTIMS:
        cells = [cases.TABLE[(v["id"], c["id"])] for c in cases.INTRUDERS]
        assert 2 * cells.count(cases.EXACT) >= len(cells), (v["id"], cells.count(cases.EXACT), len(cells))


def test_split_wrappers_exist():
    """capi.Context has a plan-only and a write-only method for every pair; the one-shot wrappers stay."""
    for name in ("pair_plan", "pair_write", "set_union_plan", "set_union_write", "spss_decode_plan",
                 "spss_decode_write", "kmer_count_write", "spss_encode_plan", "spss_encode_write", "spss_cover_plan",
                 "spss_cover_write", "spss_from_text_plan", "spss_from_text_write", "fasta_plan", "fasta_write",
                 "pair_algebra", "set_union", "spss_decode", "kmer_count", "spss_encode", "spss_cover",
                 "spss_from_text", "fasta_fragments"):
        assert callable(getattr(capi.Context, name)), name


# ---- the expected values of the index and string ops are not vacuous (the references alone) ----------------------
GEOMS = cases.NARROW + cases.WIDE  # every geometry an op runs at: the victims' (other_geom maps into NARROW)
KS = sorted({g[0] for g in GEOMS})


def test_the_new_ops_run_at_these_geometries():
    assert {v["geom"] for v in cases.VICTIMS} | {cases.other_geom(v["geom"]) for v in cases.VICTIMS} == set(GEOMS)
    assert {g[2] for g in GEOMS} == set(cases.BUBBLE_GRAPHS)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "k%d-N%d-u%d" % (g[0], g[1], 8 * g[2]))
def test_index_truths_are_not_vacuous(geom):
    k, n, kb = geom
    ic = cases.index_case(geom)
    ref, cols = ic["ref"], cases.COLS
    assert ref.n_nodes == cases.KSS_SETS and sorted(cols) == list(range(ref.n_nodes)) and cols != sorted(cols)
    # seq_hits: the windows cut from input i hit (input i at every position), the random strings miss
    hits, strings = ic["hits"], ic["strings"]
    assert len(strings) == 12 and all(200 <= len(s) <= 300 for s in strings)
    assert hits.shape == (12, 4) and (hits[:8] > 0).all() and not hits[8:].any()
    for i in range(4):  # (another input misses some position of the two windows together)
        own = hits[2 * i:2 * i + 2, i]
        assert own.tolist() == [len(s) - k + 1 for s in strings[2 * i:2 * i + 2]]
        assert (hits[2 * i:2 * i + 2] < own[:, None]).any()
    # pair_counts: no two columns alike, and the permutation of the columns shows
    pairs = ic["pairs"]
    assert np.array_equal(pairs, pairs.T) and len({tuple(r) for r in pairs.tolist()}) == 4
    assert not np.array_equal(pairs, ref.pair_table(sorted(cols)))
    # every selected column has k-mers of its own, and k-mers it shares
    for c in cols:
        assert ref.select(cols=cols, require=[c], max_count=1).size > 0
        assert ref.select(cols=cols, require=[c], min_count=2).size > 0
    # select: A and B are proper subsets, B is smaller, and their bucket offsets differ (fail:select_keys)
    (a, off_a, keys_a), (b, off_b, keys_b) = ic["select"]["A"], ic["select"]["B"]
    assert 0 < b.size < a.size < ref.n_distinct and not np.array_equal(off_a, off_b)
    assert off_a.size == (1 << n) + 1 and keys_a.dtype.itemsize == kb and (np.diff(off_a) > 0).sum() > 100
    assert ic["spectrum"]["A"].size == 5 and (ic["spectrum"]["A"][1:] > 0).all() and ic["spectrum"]["A"][0] == 0
    # classes: more than one, counts that tell them apart
    assert len(ic["rows"]) > 4 and len(set(ic["counts"].tolist())) > 4 and ic["counts"].sum() == ref.n_distinct
    # class ids: every class of the table is some k-mer's, B's union is smaller than A's
    for name in "AB":
        rows, kmers, off, keys, ids = ic["class_ids"][name]
        assert (ids >= 0).all() and np.unique(ids).size == len(rows) > 1 and kmers.size == off[-1] == keys.size
    assert 0 < ic["class_ids"]["B"][1].size < ic["class_ids"]["A"][1].size
    assert not np.array_equal(ic["class_ids"]["A"][2], ic["class_ids"]["B"][2])
    # class runs: runs inside strings, several classes, no position without one; B has fewer runs than A
    for name in "AB":
        table, off, start, cls, unmatched = ic["runs"][name]
        assert off[-1] == start.size == cls.size > len(strings) and np.unique(cls).size >= 3 and unmatched == 0
        assert (start > 0).any() and off[-1] < sum(len(s) - k + 1 for s in strings)
    assert 0 < ic["runs"]["B"][1][-1] < ic["runs"]["A"][1][-1]


@pytest.mark.parametrize("k", KS)
def test_string_truths_are_not_vacuous(k):
    import spss_links_reference as links_ref
    from spss_cut_reference import cut

    case = cases.cut_case(k)
    assert case["k"] == k and 4 <= len(case["strings"]) <= 300
    out, lens, n_out = cut(case["strings"], k, case["offsets"], case["start"])
    assert len(out) > len(case["strings"]) and max(len(s) for s in out) > k     # some string is cut, some piece is long
    assert any(a != b for a, b in zip(out, case["strings"]))
    with pytest.raises(AssertionError):                                          # (the reference refuses them too)
        cut(case["strings"], k, cases.descending_offsets(case), case["start"])
    a, b = cases.links_case(k), cases.links_case(k, "B")
    assert 3 <= len(b) < len(a) <= 300
    (off_a, to_a), (off_b, to_b) = links_ref.links(a, k, True), links_ref.links(b, k, True)
    assert 1 < to_b.size < to_a.size - 1 and links_ref.twin_symmetric(off_a, to_a)
    assert len(set(to_a.tolist())) > 4 and (np.diff(off_a) == 0).any() and (np.diff(off_a) > 0).any()
    with pytest.raises(ValueError, match="duplicate end: string 1"):
        links_ref.check_container(cases.repeated_end(k), k, True)
    assert cases.repeated_end(k)[:-1] == a


@pytest.mark.parametrize("kb", sorted(cases.BUBBLE_GRAPHS))
def test_bubble_truths_are_not_vacuous(kb):
    import link_bubbles_reference as bubbles_ref

    off, to, max_arm, cls, rows = cases.bubbles_case(kb)
    assert (len(off) - 1) // 2 <= 300 and cases.BUBBLES_MAX_ARM_B != max_arm
    ends, arm_off, arm, arm_rows = bubbles_ref.bubbles(off, to, max_arm, cls, rows)
    assert len(ends) > 0 and len(arm) >= 2 * len(ends) and len({tuple(r) for r in arm_rows.tolist()}) > 1
    ends_b, _, arm_b, _ = bubbles_ref.bubbles(off, to, cases.BUBBLES_MAX_ARM_B, cls, rows)
    assert 0 < len(ends_b) < len(ends) and 0 < len(arm_b) < len(arm)
    with pytest.raises(ValueError, match="has no twin"):
        bubbles_ref.check_graph(off, cases.no_twin(kb), cls, len(rows))


def test_the_table_is_complete():
    """One cell per victim row and column, the new columns all exact."""
    assert len(cases.TABLE) == len(cases.VICTIMS) * len(cases.INTRUDERS)
    new = [c for c in cases.INTRUDERS if set(c["symbols"]) <= set(cases.NEW_SYMBOLS)]
    assert len(new) == 3 * len(cases.INDEX_OPS + cases.STRING_OPS) + 2 * len(cases.NEW_FAILING)
    assert all(cases.TABLE[(v["id"], c["id"])] == cases.EXACT for v in cases.VICTIMS for c in new)

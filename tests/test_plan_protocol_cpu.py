"""Guards the plan / write protocol table (tests/plan_protocol_cases.py) against the header: no GPU needed.

The table decides which sequences tests/test_gpu_plan_protocol.py issues and what it expects of each; these checks
keep it complete (every two-call pair is a victim, every entry point that takes a context is an intruder) and
honest (a refusal only where include/kmersets_hip.h, "Plans", permits one; at most half of a victim's cells)."""
import re

import plan_protocol_cases as cases
from kmersets import capi


def declarations():
    """name -> type of the first parameter, for every function the header declares."""
    text = open(capi.HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, first in re.findall(r"\b(ksh_[a-z0-9_]+)\s*\(\s*([^,)]*)", text):
        out[name] = " ".join(first.split())
    return out


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


def test_every_context_entry_point_is_an_intruder():
    decl = declarations()
    assert set(decl) == set(capi.exported_symbols())
    takes_ctx = {name for name, first in decl.items() if re.search(r"\bksh_(ctx|kss|kss_index)\s*\*", first)}
    assert "ksh_pair_plan" in takes_ctx and "ksh_kss_get" in takes_ctx and "ksh_kss_index_query" in takes_ctx
    assert "ksh_malloc" not in takes_ctx
    called = {s for c in cases.INTRUDERS for s in c["symbols"]}
    assert called <= set(decl), called - set(decl)
    missing = takes_ctx - called - set(cases.EXCLUDED)
    assert not missing, sorted(missing)
    for name, reason in cases.EXCLUDED.items():
        assert name in decl and name not in called and reason


def test_intruder_columns():
    cols = cases.INTRUDERS
    assert len({c["id"] for c in cols}) == len(cols)
    ops = {(c["op"], c["width"], c["where"]) for c in cols}
    for kind in cases.KINDS:  # each victim kind as a full plan + write and as an abandoned plan, at both widths
        for how in ("full", "abandon"):
            for width in ("same", "other"):
                assert ("%s:%s" % (how, kind), width, "own") in ops
    for op in ("fail:decode", "fail:from_text", "fail:fasta", "fail:encode", "kss_build:lanes1", "kss_build:default",
               "kss_get", "kss_index_create", "kss_index_query", "reserve", "large:arena", "large:plans"):
        assert any(c["op"] == op and c["where"] == "own" for c in cols), op
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

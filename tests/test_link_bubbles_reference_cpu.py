"""The host reference of ksh_link_bubbles and its designed cases, without a GPU: every edge class a case lists is a
predicate that holds on it, the hand-worked answers are the reference's, every bubble's twin is a bubble, and on the
two families built from strings every planted substitution that stands alone is found exactly once, with the two
genome windows as alleles and the samples that hold each window whole as carriers.

Seeds checked: the families of link_bubbles_cases.FAMILY_ARGS, seeds 11 (K = 15) and 12 (K = 17).  For both,
test_family_seeds_have_no_repeats holds: no (K - 1)-mer of the samples, up to reverse complement, lies at two
positions of the genome, so no repeat lies near any site, whatever max_arm."""
import numpy as np
import pytest

import link_bubbles_cases as bc
import link_bubbles_reference as ref
import spss_links_reference as links_ref
from kmersets import capi

IDS = [c["id"] for c in bc.CASES]


def found_of(case, max_arm=None):
    """The reported bubbles of a case as (v, w, arm_0, arm_1) tuples."""
    ends, off, arm, _ = ref.bubbles(case["off"], case["to"], case["max_arm"] if max_arm is None else max_arm,
                                    limit=ref.MAX_ARM + 1)
    return [(int(v), int(w), [int(x) for x in arm[off[2 * b]:off[2 * b + 1]]],
             [int(x) for x in arm[off[2 * b + 1]:off[2 * b + 2]]]) for b, (v, w) in enumerate(ends)]


def arm_end(case, x):
    """How the walk of the arm that begins with x ends: (reason, vertex)."""
    off, to = case["off"], case["to"]
    outdeg, indeg = ref.degrees(off)
    steps = 0
    while True:
        if indeg[x] != 1:
            return "in", x
        if outdeg[x] != 1:
            return "out", x
        if steps == case["max_arm"]:
            return "long", x
        steps += 1
        x = int(to[off[x]])
        if indeg[x] == 2:
            return "sink", x
        if indeg[x] != 1:
            return "next_in", x


def arm_ends(case):
    """[(v, end of arm 0, end of arm 1)] of every vertex with two links out."""
    off, to = case["off"], case["to"]
    outdeg, _ = ref.degrees(off)
    return [(v, arm_end(case, int(to[off[v]])), arm_end(case, int(to[off[v] + 1])))
            for v in range(2 * case["n"]) if outdeg[v] == 2]


def lens(found):
    return [(len(a0), len(a1)) for _, _, a0, a1 in found]


def has_ring(case):
    off, to, m = case["off"], case["to"], 2 * case["n"]
    for x in range(m):
        y, steps = x, 0
        while off[y + 1] > off[y] and steps < m:
            y, steps = int(to[off[y]]), steps + 1
            if y == x:
                if steps > 1:
                    return True
                break
    return False


def sinks_differ(case, side_entry):
    outdeg, _ = ref.degrees(case["off"])
    for _, e0, e1 in arm_ends(case):
        if e0[0] == e1[0] == "sink" and e0[1] != e1[1]:
            if not side_entry or 1 in (outdeg[e0[1]], outdeg[e1[1]]):
                return True
    return False


def lost_at(case, max_arm):
    """The bubbles found at max_arm but not at the case's own."""
    have = {(v, w) for v, w, _, _ in found_of(case)}
    return [b for b in found_of(case, max_arm) if (b[0], b[1]) not in have]


def degree_seen(case, which, d):
    return d in ref.degrees(case["off"])[which]


PREDICATES = {
    "arms_1_1": lambda c, f: (1, 1) in lens(f),
    "arms_1_2": lambda c, f: (1, 2) in lens(f) or (2, 1) in lens(f),
    "arms_max_max": lambda c, f: (c["max_arm"], c["max_arm"]) in lens(f),
    "arm_max_plus_1_nothing": lambda c, f: any(max(len(b[2]), len(b[3])) == c["max_arm"] + 1
                                               for b in lost_at(c, c["max_arm"] + 1)),
    "arm_max_plus_1_found": lambda c, f: c["max_arm"] > 1 and any(
        max(ls) == c["max_arm"] for ls in lens(f)) and len(found_of(c, c["max_arm"] - 1)) < len(f),
    "max_arm_1": lambda c, f: c["max_arm"] == 1 and len(f) > 0,
    "max_arm_64": lambda c, f: c["max_arm"] == 64 == ref.MAX_ARM,
    "hairpin": lambda c, f: any(w == v ^ 1 for v, w, _, _ in f),
    "outdeg_3": lambda c, f: degree_seen(c, 0, 3) and not f,
    "outdeg_4": lambda c, f: degree_seen(c, 0, 4) and not f,
    "different_sinks": lambda c, f: sinks_differ(c, False),
    "side_entry": lambda c, f: sinks_differ(c, True),
    "sink_indeg_3": lambda c, f: any("next_in" in (e0[0], e1[0]) for _, e0, e1 in arm_ends(c)) and degree_seen(c, 1, 3),
    "side_exit": lambda c, f: any(e[0] == "out" and ref.degrees(c["off"])[0][e[1]] >= 2
                                  for _, e0, e1 in arm_ends(c) for e in (e0, e1)),
    "tip": lambda c, f: any(e[0] == "out" and ref.degrees(c["off"])[0][e[1]] == 0
                            for _, e0, e1 in arm_ends(c) for e in (e0, e1)),
    "ring": lambda c, f: has_ring(c) and not f,
    "self_link": lambda c, f: any(v in c["to"][c["off"][v]:c["off"][v + 1]] for v in range(2 * c["n"])),
    "back_to_back": lambda c, f: bool({w for _, w, _, _ in f} & {v for v, _, _, _ in f}),
    "twin_low": lambda c, f: any(not v & 1 and not any(x & 1 for x in a0 + a1) for v, _, a0, a1 in f),
    "twin_high": lambda c, f: any(v & 1 and all(x & 1 for x in a0 + a1) for v, _, a0, a1 in f),
    "source_at_0": lambda c, f: any(v == 0 for v, _, _, _ in f),
    "sink_at_2n_1": lambda c, f: any(w == 2 * c["n"] - 1 for _, w, _, _ in f),
    "sources_255_256_257": lambda c, f: {255, 256, 257} <= {v for v, _, _, _ in f},
    "scan_block_edges": lambda c, f: set(bc.EDGE_SOURCES) <= {v for v, _, _, _ in f},
    "many": lambda c, f: len(f) >= 1500,
    "no_strings": lambda c, f: c["n"] == 0 and c["off"].tolist() == [0] and not f,
    "one_string": lambda c, f: c["n"] == 1 and not f,
    "no_links": lambda c, f: c["n"] > 0 and c["to"].size == 0 and not f,
}


def test_every_edge_class_is_listed_and_has_a_predicate():
    listed = {name for c in bc.CASES for name in c["classes"]}
    assert listed == set(PREDICATES)
    assert len(set(IDS)) == len(IDS)
    assert max(c["n"] for c in bc.CASES) < 8000


@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_case_is_what_it_is_there_for(case):
    assert links_ref.twin_symmetric(case["off"], case["to"])
    found = found_of(case)
    assert sorted((v, w, len(a0), len(a1)) for v, w, a0, a1 in found) == case["want"]
    assert [v for v, _, _, _ in found] == sorted({v for v, _, _, _ in found})  # ascending, one bubble a source
    for name in case["classes"]:
        assert PREDICATES[name](case, found), name


def unordered(b):
    return b[0], b[1], tuple(sorted((tuple(b[2]), tuple(b[3]))))


def check_twins(off, to, max_arm):
    every = ref.all_bubbles(off, to, max_arm)
    keys = {unordered(b) for b in every}
    assert len(keys) == len(every)
    for b in every:
        assert unordered(ref.twin_of(b)) in keys
    ends = ref.bubbles(off, to, max_arm)[0]
    reported = {(int(v), int(w)) for v, w in ends}
    for v, w, _, _ in every:  # exactly one of the twins (a hairpin is its own twin)
        assert ((v, w) in reported) + ((w ^ 1, v ^ 1) in reported) == (2 if w == v ^ 1 else 1)
    return len(every)


@pytest.mark.parametrize("case", bc.CASES, ids=IDS)
def test_every_bubble_has_its_twin(case):
    check_twins(case["off"], case["to"], case["max_arm"])


def test_carriers_are_the_and_over_the_arm():
    case = next(c for c in bc.CASES if c["id"] == "back-to-back")
    cls = bc.classes_of(case["n"])
    ends, off, arm, rows = ref.bubbles(case["off"], case["to"], case["max_arm"], cls, bc.ROWS)
    assert rows.shape == (2 * len(ends), 2) and rows.dtype == np.uint64
    several = 0
    for a in range(2 * len(ends)):
        members = [set(ref.carriers(bc.ROWS[cls[x >> 1]])) for x in arm[off[a]:off[a + 1]]]
        assert set(ref.carriers(rows[a])) == set.intersection(*members)
        several += len(members) > 1 and len({frozenset(m) for m in members}) > 1
    assert several  # an arm whose strings have different classes: a set on part of the arm is no carrier
    plain = ref.bubbles(case["off"], case["to"], case["max_arm"])
    assert plain[3] is None and all(np.array_equal(a, b) for a, b in zip(plain[:3], (ends, off, arm)))


def test_check_graph_names_the_smallest_offender():
    case = next(c for c in bc.CASES if c["id"] == "back-to-back")
    off, to = case["off"], case["to"]
    ref.check_graph(off, to, bc.classes_of(case["n"]), len(bc.ROWS))

    def refused(word, off=off, to=to, cls=None):
        with pytest.raises(ValueError, match=word):
            ref.check_graph(off, to, cls, len(bc.ROWS))

    bad = off.copy()
    bad[0] = 1
    refused(r"\[0\] is not 0", off=bad)
    bad = off.copy()
    bad[-1] += 1
    refused(r"\[2 n\] is not n_links", off=bad)
    bad = off.copy()
    bad[3], bad[9] = bad[4] + 1, bad[10] + 2
    refused("descends behind vertex 3$", off=bad)
    refused("the row of vertex 0 has more", off=np.concatenate([[0], np.full(off.size - 1, to.size)]))
    bad = to.copy()
    bad[5], bad[2] = -1, 2 * case["n"]
    refused("the target of link 2 is outside", to=bad)
    wide_off, wide_to = ref.csr(3, [(0, 2), (0, 4), (2, 4)])
    bad = wide_to.copy()
    bad[1] = bad[0]
    refused("the row of vertex 0 repeats", off=wide_off, to=bad)
    one_way_off, one_way_to = ref.csr(3, [(0, 2), (2, 4)], twins=False)
    refused(r"link 0 \(v -> w\) has no twin", off=one_way_off, to=one_way_to)
    cls = bc.classes_of(case["n"])
    cls[4], cls[2] = -1, len(bc.ROWS)
    refused("the class of string 2 is outside", cls=cls)


# ---- the families built from strings -----------------------------------------------------------------------------

FAMILY_IDS = ["family-%d" % args[0] for args in bc.FAMILY_ARGS]


@pytest.fixture(scope="module", params=FAMILY_IDS)
def fam(request):
    f = next(f for f in bc.families() if f["id"] == request.param)
    f = dict(f)
    f["result"] = ref.bubbles(f["off"], f["to"], f["max_arm"], f["string_class"], f["rows"])
    return f


def test_family_seeds_have_no_repeats(fam):
    k = fam["k"]
    where = {}
    for t in fam["samples"]:  # (every sample is a genome or a prefix of one: positions are the genome's)
        for p in range(len(t) - k + 2):
            where.setdefault(links_ref.canon(t[p:p + k - 1]), set()).add(p)
    assert all(len(ps) == 1 for ps in where.values())


def test_family_graph_is_the_colored_graph(fam):
    k, strings = fam["k"], fam["strings"]
    kmers = links_ref.kmers_of(strings, k)
    want = {links_ref.canon(t[p:p + k]) for t in fam["samples"] for p in range(len(t) - k + 1)}
    assert len(kmers) == len(want) and {links_ref.canon(x) for x in kmers} == want
    for t, c in zip(strings, fam["string_class"]):  # one class a string: the samples that hold each of its k-mers
        held = {tuple(i for i, s in enumerate(fam["samples"]) if x in s or links_ref.rc(x) in s)
                for x in links_ref.kmers_of([t], k)}
        assert held == {tuple(ref.carriers(fam["rows"][c]))}
    pairs = set(links_ref.link_pairs(strings, k, fam["off"], fam["to"])) | set(links_ref.inner_pairs(strings, k, True))
    assert pairs == links_ref.graph_edges(kmers, k, True)
    assert links_ref.twin_symmetric(fam["off"], fam["to"])
    check_twins(fam["off"], fam["to"], fam["max_arm"])


def holds(sample, window):
    return window in sample or links_ref.rc(window) in sample


def test_family_sites_are_found_once_with_their_carriers(fam):
    k, strings, samples = fam["k"], fam["strings"], fam["samples"]
    ends, off, arm, rows = fam["result"]
    alleles = capi.bubble_alleles(strings, k, ends, off, arm)
    assert [(v, w) for v, w, _, _ in alleles] == [(int(v), int(w)) for v, w in ends]
    for b, (_, _, a0, a1) in enumerate(alleles):
        assert a0 == ref.spell(strings, k, arm[off[2 * b]:off[2 * b + 1]])
        assert a1 == ref.spell(strings, k, arm[off[2 * b + 1]:off[2 * b + 2]])
    assert len(fam["isolated"]) >= 5 and len(alleles) >= len(fam["isolated"])
    for p in fam["isolated"]:
        windows = {g[p - k + 1:p + k] for g in fam["genomes"]}
        assert len(windows) == 2 and all(len(x) == 2 * k - 1 for x in windows)
        x, y = sorted(windows)
        assert x[:k - 1] == y[:k - 1] and x[k:] == y[k:] and x[k - 1] != y[k - 1]  # the middle base only
        hits = [b for b, (_, _, a0, a1) in enumerate(alleles)
                if {a0, a1} == windows or {links_ref.rc(a0), links_ref.rc(a1)} == windows]
        assert len(hits) == 1, p
        (b,) = hits
        for i, allele in enumerate(alleles[b][2:]):
            window = allele if allele in windows else links_ref.rc(allele)
            assert ref.carriers(rows[2 * b + i], len(samples)) == [s for s, t in enumerate(samples) if holds(t, window)]
            assert ref.carriers(rows[2 * b + i]) == ref.carriers(rows[2 * b + i], len(samples))
    # the partial samples end inside an arm: arms of two strings, found from max_arm = 2 on, and no carriers there
    two = [b for b in range(len(ends)) if 2 in (off[2 * b + 1] - off[2 * b], off[2 * b + 2] - off[2 * b + 1])]
    assert len(two) >= len(fam["partial"])
    fewer = ref.bubbles(fam["off"], fam["to"], 1, fam["string_class"], fam["rows"])[0]
    assert len(fewer) == len(ends) - len(two)
    assert np.array_equal(ref.bubbles(fam["off"], fam["to"], 2, fam["string_class"], fam["rows"])[0], ends)
    for sample, p in fam["partial"]:
        windows = [g[p - k + 1:p + k] for g in fam["genomes"]]
        assert not any(holds(samples[sample], x) for x in windows)
        assert any(samples[sample][-k:] in x for x in windows)  # ... though it holds part of one


def test_bubble_lines_parse_back(fam, tmp_path):
    k, strings = fam["k"], fam["strings"]
    ends, off, arm, rows = fam["result"]
    n_cols = len(fam["samples"])
    lines = capi.bubble_lines(strings, k, ends, off, arm, rows, n_cols)
    parsed = ref.parse_bubble_lines(lines)
    assert len(parsed) == len(ends) > 0
    for b, (v, w, a0, a1, c0, c1) in enumerate(parsed):
        assert (v, w) == (int(ends[b, 0]), int(ends[b, 1]))
        assert a0 == ref.spell(strings, k, arm[off[2 * b]:off[2 * b + 1]])
        assert a1 == ref.spell(strings, k, arm[off[2 * b + 1]:off[2 * b + 2]])
        assert (c0, c1) == (ref.carriers(rows[2 * b]), ref.carriers(rows[2 * b + 1]))
        assert a0[:k - 1] == a1[:k - 1] == ref.oriented(strings, v)[-(k - 1):]
        assert a0[-(k - 1):] == a1[-(k - 1):] == ref.oriented(strings, w)[:k - 1]
    assert any(c == [] for row in parsed for c in row[4:]) or all("." not in line.split("\t")[4:] for line in lines)
    bare = capi.bubble_lines(strings, k, ends, off, arm)
    assert [line.split("\t")[:4] for line in bare] == [line.split("\t")[:4] for line in lines]
    assert all(line.split("\t")[4:] == [".", "."] for line in bare)
    path = tmp_path / "bubbles.tsv"
    assert capi.write_bubbles(str(path), strings, k, ends, off, arm, rows, n_cols) == len(lines)
    assert path.read_text() == "".join(line + "\n" for line in lines)

"""Checks of the host reference of ksh_spss_links (tests/spss_links_reference.py) and of the designed inputs
(tests/spss_links_cases.py): a case worked by hand, the reference against an independent all-pairs comparison of
overlaps, every edge class a case claims asserted by a predicate on the case, the three properties of the contract
(rows of at most four, twin symmetry, completeness against a brute-force edge set) on the oracle's unitigs and on random
cuts of them, and the GFA text parsed back.  No GPU."""
import numpy as np
import pytest

import oracle_lib as ol
import spss_links_cases as lc
import spss_links_reference as ref
from kmersets import capi, synth

IDS = [c["id"] for c in lc.CASES]
MODAL = [(c, m) for c in lc.CASES for m in c["modes"]]
MODAL_IDS = ["%s-%s" % (c["id"], "canonical" if m else "directed") for c, m in MODAL]


def all_pairs(strings, k, canonical):
    """Independent of the reference's dict: the last K - 1 bases of every oriented string against the first K - 1 of
    every oriented string, the skip rule applied, rows ascending by the appended base."""
    n = len(strings)
    vs = [v for v in range(2 * n) if canonical or not v & 1]
    text = {v: ref.oriented(strings, v) for v in vs}
    out = []
    for v in range(2 * n):
        found = []
        if v in text:
            last = text[v][-k:]
            for w in vs:
                if text[w][:k - 1] == last[1:]:
                    y = text[w][:k]
                    if (ref.canon(y) != ref.canon(last)) if canonical else (y != last):
                        found.append(("ACGT".index(y[-1]), w))
        assert len({b for b, _ in found}) == len(found)  # a base reaches at most one string
        out.append([w for _, w in sorted(found)])
    return out


def test_hand_worked():
    """K = 4.  AACCG ends in ACCG; CCGTA begins with CCGT = ACCG[1:] + T: 0 -> 2, and its twin 3 -> 1."""
    off, to = ref.links(["AACCG", "CCGTA"], 4, True)
    assert off.tolist() == [0, 1, 1, 1, 2] and to.tolist() == [2, 1]
    off, to = ref.links(["AACCG", "CCGTA"], 4, False)
    assert off.tolist() == [0, 1, 1, 1, 1] and to.tolist() == [2]
    off, to = ref.links([], 9, True)
    assert off.tolist() == [0] and to.size == 0 and off.dtype == to.dtype == np.int64
    # the loop and the hairpin give nothing; a ring links to itself
    assert ref.links(["AAAAA"], 5, True)[1].size == 0 and ref.links(["AAAAA"], 5, False)[1].size == 0
    assert ref.links(["CACGT"], 5, True)[1].size == 0
    assert ref.rows(*ref.links(["ACGGTACGG"], 5, True)) == [[0], [1]]
    assert ref.rows(*ref.links(["ACGGTACGG"], 5, False)) == [[0], []]
    # refused: ACGTT and AACGT are one canonical k-mer; AACGTT is its own reverse complement; a string ACGGT .. ACGGT
    for bad, k, word in ((["GGACG", "ACGTT", "AACGT"], 5, "duplicate end: string 1"),
                         (["CCCCCA", "AACGTT"], 6, "palindromic end: string 1"),
                         (["ACGGTTTACGGT"], 5, "duplicate end: string 0")):
        with pytest.raises(ValueError, match=word):
            ref.links(bad, k, True)
    # (legal as written: AACGT + T is ACGTT)
    assert ref.rows(*ref.links(["GGACG", "ACGTT", "AACGT"], 5, False)) == [[], [], [], [], [2], []]


@pytest.mark.parametrize("case,canonical", MODAL, ids=MODAL_IDS)
def test_reference_equals_all_pairs(case, canonical):
    k, strings = case["k"], case["strings"]
    if len(strings) > 1200:
        strings = strings[:1200]  # (all pairs: the first 1200 strings of the largest case, a container of its own)
    off, to = ref.links(strings, k, canonical)
    got = ref.rows(off, to)
    assert got == all_pairs(strings, k, canonical)
    assert max([len(r) for r in got] + [0]) <= 4 and off.size == 2 * len(strings) + 1
    if canonical:
        assert ref.twin_symmetric(off, to)
    else:
        assert all(not r for r in got[1::2]) and all(not w & 1 for w in to)


def starts_of(case):
    lens = [len(s) for s in case["strings"]]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def would_link(case, hit):
    """Some (v, base) whose extension y satisfies hit(v, y, first) without the skip rule, and is skipped by it."""
    k, strings = case["k"], case["strings"]
    first = {ref.oriented(strings, v)[:k]: v for v in range(2 * len(strings))}
    for v in range(2 * len(strings)):
        last = ref.oriented(strings, v)[-k:]
        for b in "ACGT":
            y = last[1:] + b
            if ref.canon(y) == ref.canon(last) and y in first and hit(v, last, y, first[y]):
                return True
    return False


def orientation_pairs(case):
    off, to = ref.links(case["strings"], case["k"], True)
    return {(v & 1, w & 1) for v, row in enumerate(ref.rows(off, to)) for w in row}


def entered_both_ways(case):
    off, to = ref.links(case["strings"], case["k"], True)
    singles = {s for s, t in enumerate(case["strings"]) if len(t) == case["k"]}
    return any(2 * s in to and 2 * s + 1 in to for s in singles)


def interior_landing(case):
    k, strings = case["k"], case["strings"]
    inner = {t[i:i + k] for t in strings for i in range(1, len(t) - k)}
    inner |= {ref.rc(x) for x in inner}
    first = {ref.oriented(strings, v)[:k] for v in range(2 * len(strings))}
    return any(ref.oriented(strings, v)[-k:][1:] + b in inner - first for v in range(2 * len(strings)) for b in "ACGT")


def linked_to(case, kmer):
    k, strings = case["k"], case["strings"]
    for canonical in case["modes"]:
        off, to = ref.links(strings, k, canonical)
        if not any(ref.oriented(strings, w)[:k] == kmer and not w & 1 for w in to):
            return False
    return any(t[:k] == kmer or t[-k:] == kmer for t in strings)


PREDICATES = {
    lc.FIRST_STRADDLES: lambda c: any(b % 32 + c["k"] > 32 for b in starts_of(c)[:-1]),
    lc.LAST_STRADDLES: lambda c: any((e - c["k"]) % 32 + c["k"] > 32 for e in starts_of(c)[1:]),
    lc.STARTS_ON_WORD: lambda c: any(b % 32 == 0 for b in starts_of(c)[1:-1]),
    lc.ENDS_PARTIAL: lambda c: starts_of(c)[-1] % 32 != 0,
    lc.ENDS_ON_WORD: lambda c: starts_of(c)[-1] % 32 == 0 and starts_of(c)[-1] > 0,
    lc.SINGLE_BOTH_SIDES: entered_both_ways,
    lc.ALL_A_END: lambda c: linked_to(c, "A" * c["k"]),
    lc.ALL_T_END: lambda c: linked_to(c, "T" * c["k"]),
    lc.FOUR_LINKS: lambda c: all(max(len(r) for r in ref.rows(*ref.links(c["strings"], c["k"], m))) == 4
                                 for m in c["modes"]),
    lc.ALL_ORIENTATIONS: lambda c: orientation_pairs(c) == {(0, 0), (0, 1), (1, 0), (1, 1)},
    lc.CIRCULAR: lambda c: any(v in row and len(c["strings"][v >> 1]) > c["k"]
                               for v, row in enumerate(ref.rows(*ref.links(c["strings"], c["k"], True)))),
    lc.LOOP: lambda c: would_link(c, lambda v, last, y, w: y == last and w == v),
    lc.HAIRPIN: lambda c: would_link(c, lambda v, last, y, w: y == ref.rc(last) and y != last and w == v ^ 1),
    lc.INTERIOR: interior_landing,
    lc.BOTH_MODES: lambda c: c["modes"] == (True, False),
    lc.NO_LINKS: lambda c: len(c["strings"]) > 0 and all(ref.links(c["strings"], c["k"], m)[1].size == 0
                                                         for m in c["modes"]),
    lc.EMPTY: lambda c: len(c["strings"]) == 0,
    lc.SINGLE_STRING: lambda c: len(c["strings"]) == 1,
    lc.OVER_256: lambda c: len(c["strings"]) > 256,
    lc.THOUSANDS: lambda c: len(c["strings"]) >= 3000,
    lc.RANDOM: lambda c: len({len(s) for s in c["strings"]}) > 5,
    lc.HAS_LINKS: lambda c: ref.links(c["strings"], c["k"], True)[1].size > 0,
}


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_case_is_what_it_claims(case):
    k, strings = case["k"], case["strings"]
    assert k in lc.KS and case["covers"] and all(len(s) >= k for s in strings)
    assert sum(len(s) - k + 1 for s in strings) <= 8000
    for m in case["modes"]:
        assert lc.legal(strings, k, m)
    for cover in case["covers"]:
        assert PREDICATES[cover](case), (case["id"], cover)


def test_every_edge_class_is_covered():
    covered = {c for case in lc.CASES for c in case["covers"]}
    assert covered == set(PREDICATES)
    assert {case["k"] for case in lc.CASES} == set(lc.KS)
    assert len(set(IDS)) == len(IDS)
    assert sum(lc.RANDOM in case["covers"] for case in lc.CASES) == 2
    # both modes at every K
    assert {(case["k"], m) for case in lc.CASES for m in case["modes"]} == {(k, m) for k in lc.KS for m in (True, False)}


def kmer_text(x, k):
    return "".join("ACGT"[(int(x) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def random_cut(strings, k, rng, p):
    out = []
    for t in strings:
        n = len(t) - k + 1
        at = [0] + [int(x) for x in 1 + np.flatnonzero(rng.random(n - 1) < p)] + [n]
        out += [t[a:e + k - 1] for a, e in zip(at[:-1], at[1:])]
    return out


def three_properties(strings, kmers, k, canonical):
    off, to = ref.links(strings, k, canonical)
    got = ref.rows(off, to)
    assert max(len(r) for r in got) <= 4
    if canonical:
        assert ref.twin_symmetric(off, to)
    else:
        assert all(not r for r in got[1::2])
    between = ref.link_pairs(strings, k, off, to)
    inside = ref.inner_pairs(strings, k, canonical)
    assert len(set(between)) == len(between) and len(set(inside)) == len(inside)
    assert not set(between) & set(inside)
    assert set(between) | set(inside) == ref.graph_edges(kmers, k, canonical)
    return len(between)


GEOMS = [(5, 3, 1), (9, 10, 1), (23, 14, 4), (31, 14, 8)]


@pytest.mark.parametrize("geom", GEOMS, ids=["k%d" % g[0] for g in GEOMS])
@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "directed"])
def test_three_properties_on_oracle_unitigs(geom, canonical):
    """The oracle's unitigs of a k-mer set, and random cuts of them: the links and the pairs inside the strings are
    the set's de Bruijn edges, each once."""
    k, n, kb = geom
    links_seen = 0
    for seed in range(3):
        length = {5: 150, 9: 1500}.get(k, 3000)
        bases = synth.plant_repeats(synth.random_genome(length, 40 + seed), 4, 3, 50 + seed, min_len=k, max_len=3 * k)
        kmers = synth.canonical_set_of_bases(bases, k) if canonical else np.unique(synth.kmers_of_bases(bases, k))
        oset = ol.Set.from_kmers(k, n, kb, kmers)
        text = [kmer_text(x, k) for x in oset.kmers()]
        unitigs = oset.unitigs() if canonical else oset.unitigs_directed()
        assert sorted(ref.canon(x) if canonical else x for x in ref.kmers_of(unitigs, k)) == sorted(text)
        links_seen += three_properties(unitigs, text, k, canonical)
        rng = np.random.default_rng(60 + seed)
        for p in (0.05, 0.5):
            pieces = random_cut(unitigs, k, rng, p)
            assert len(pieces) > len(unitigs)
            links_seen += three_properties(pieces, text, k, canonical)
    assert links_seen > 0


@pytest.mark.parametrize("case,canonical", [(c, m) for c, m in MODAL if len(c["strings"]) <= 400],
                         ids=[i for (c, m), i in zip(MODAL, MODAL_IDS) if len(c["strings"]) <= 400])
def test_gfa_parses_back(case, canonical, tmp_path):
    k, strings = case["k"], case["strings"]
    off, to = ref.links(strings, k, canonical)
    classes = [(7 * r) % 5 for r in range(len(strings))]
    lines = capi.gfa_lines(strings, k, off, to, classes)
    segments, ls = ref.parse_gfa(lines)
    assert segments == {str(r): (s, c) for r, (s, c) in enumerate(zip(strings, classes))}
    assert len(ls) == to.size and len(lines) == 1 + len(strings) + to.size
    pairs = ref.gfa_links_verify(lines, k)
    assert pairs == [(v, w) for v, row in enumerate(ref.rows(off, to)) for w in row]
    plain = capi.gfa_lines(strings, k, off.tolist(), to.tolist())
    assert ref.parse_gfa(plain)[0] == {str(r): (s, None) for r, s in enumerate(strings)}
    assert ref.parse_gfa(plain)[1] == ls
    path = tmp_path / "graph.gfa"
    assert capi.write_gfa(str(path), strings, k, off, to, classes) == len(lines)
    assert path.read_text() == "\n".join(lines) + "\n"
    with pytest.raises(ValueError):
        capi.gfa_lines(strings, k, off[:-1] if off.size > 1 else [0, 0], to)

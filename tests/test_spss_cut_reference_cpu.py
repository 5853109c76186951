"""Checks of the host reference of ksh_spss_cut (tests/spss_cut_reference.py) and of the designed inputs
(tests/spss_cut_cases.py): a case worked by hand, the k-mers staying what and where they were, the closed form of
n_bases_out, a cut made from ids through paint_reference.runs_of_ids and back through expand, and every edge class a
case claims asserted by a predicate on the case.  No GPU."""
import math

import numpy as np
import pytest

import paint_reference as pr
import spss_cut_cases as cc
from spss_cut_reference import cut, out_bases
from kmersets import synth

IDS = [c["id"] for c in cc.CASES]


def kmers_in_order(strings, k):
    parts = [synth.kmers_of_bases(synth.bases_of_string(s), k) for s in strings]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def test_hand_worked():
    """K = 4.  ACGTACG has positions 0..3; cut at 1 and 3: ACGT | CGTAC | TACG.  TTTT has one position."""
    out, lens, n = cut(["ACGTACG", "TTTT"], 4, [0, 3, 4], [0, 1, 3, 0])
    assert out == ["ACGT", "CGTAC", "TACG", "TTTT"] and lens.tolist() == [0, 1, 0, 0] and n == 17
    assert lens.dtype == np.uint32 and n == 11 + (4 - 2) * 3
    b, shift = out_bases(["ACGTACG", "TTTT"], 4, [0, 3, 4], [0, 1, 3, 0])
    assert b.tolist() == [0, 4, 9, 13, 17] and shift.tolist() == [0, 3, 6, 6]
    nothing = cut([], 9, [0], [])
    assert nothing[0] == [] and nothing[1].size == 0 and nothing[2] == 0
    assert cut(["ACGTACG"], 4, [0, 1], [0])[0] == ["ACGTACG"]


@pytest.mark.parametrize("case", cc.CASES, ids=IDS)
def test_same_kmers_and_closed_form(case):
    k, strings = case["k"], case["strings"]
    out, lens, n_out = cut(strings, k, case["offsets"], case["start"])
    assert np.array_equal(kmers_in_order(out, k), kmers_in_order(strings, k))
    n_runs = int(case["offsets"][-1])
    assert len(out) == n_runs == case["start"].size and lens.size == n_runs
    assert n_out == sum(len(s) for s in strings) + (n_runs - len(strings)) * (k - 1)
    assert all(len(x) == int(l) + k for x, l in zip(out, lens))
    b, shift = out_bases(strings, k, case["offsets"], case["start"])
    assert b[-1] == n_out and np.array_equal(np.diff(b), lens.astype(np.int64) + k)
    flat_in, flat_out = "".join(strings), "".join(out)
    for r in range(0, n_runs, max(1, n_runs // 50)):  # the shift identity, on a sample of the strings
        assert flat_out[b[r]:b[r + 1]] == flat_in[b[r] - shift[r]:b[r + 1] - shift[r]]


@pytest.mark.parametrize("case", cc.CASES, ids=IDS)
def test_a_cut_made_from_ids_round_trips(case):
    """Ids that change exactly at the case's cuts: runs_of_ids gives the case's run list back, and every string of the
    cut has one id; the ids of the cut strings, expanded, are the ids of the input."""
    k, strings, off, start = case["k"], case["strings"], case["offsets"], case["start"]
    sizes = [len(s) - k + 1 for s in strings]
    ids = []
    for s, n in enumerate(sizes):
        a, b = int(off[s]), int(off[s + 1])
        ends = np.concatenate([start[a + 1:b], [n]]).astype(np.int64)
        ids.append(np.repeat((np.arange(b - a) + s) % 3, ends - start[a:b]).astype(np.int64))
    got_off, got_start, cls = pr.runs_of_ids(ids)
    assert np.array_equal(got_off, off) and np.array_equal(got_start, start)
    out, lens, _ = cut(strings, k, got_off, got_start)
    one_each = np.arange(len(out) + 1, dtype=np.int64)
    back = pr.expand(one_each, np.zeros(len(out), dtype=np.int32), cls, lens.astype(np.int64) + 1)
    flat = np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)
    assert np.array_equal(np.concatenate(back) if back else flat, flat)
    uncut = pr.expand(got_off, got_start, cls, sizes)  # ... as are the runs of the uncut strings, expanded
    assert np.array_equal(np.concatenate(uncut) if uncut else flat, flat)


# ---- the edge classes, by predicate -------------------------------------------------------------------------------
def facts(case):
    k, strings = case["k"], case["strings"]
    out, lens, n_out = cut(strings, k, case["offsets"], case["start"])
    b, shift = out_bases(strings, k, case["offsets"], case["start"])
    first_runs = case["offsets"][:-1]
    in_start = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)[:-1]
    return dict(k=k, strings=strings, out=out, lens=lens, n_out=n_out, b=b, shift=shift, first_runs=first_runs,
                in_start=in_start, n_runs=len(out), in_lens=np.array([len(s) - k for s in strings], dtype=np.int64))


def boundaries(f):
    """Per output string the number of output word boundaries strictly inside it."""
    b = f["b"]
    return (b[1:] - 1) // 32 - b[:-1] // 32


def between_long(f):
    l = f["in_lens"]
    return any(l[s] == 0 and l[:s].max(initial=0) >= 64 and l[s + 1:].max(initial=0) >= 64 for s in range(l.size))


def reachable_shifts(k):
    return set(range(0, 32, math.gcd(k - 1, 32)))


PREDICATES = {
    cc.NO_CUT: lambda f: f["n_runs"] == len(f["strings"]) >= 1,
    cc.EVERY_POSITION: lambda f: f["n_runs"] > len(f["strings"]) and not f["lens"].any(),
    cc.EIGHT_IN_A_WORD: lambda f: f["k"] == 4 and np.bincount(f["b"][:-1] // 32).max() == 8,
    cc.PIECE_IN_WORD: lambda f: bool((boundaries(f) == 0).any()),
    cc.PIECE_ONE_BOUNDARY: lambda f: bool((boundaries(f) == 1).any()),
    cc.PIECE_THREE_BOUNDARIES: lambda f: bool((boundaries(f) >= 3).any()),
    cc.EVERY_SHIFT: lambda f: len(f["strings"]) == 1 and set((f["shift"] % 32).tolist()) == reachable_shifts(f["k"]),
    cc.EVERY_PHASE: lambda f: len(f["strings"]) == 1 and set((f["b"][:-1] % 32).tolist()) == set(range(32)),
    cc.EMPTY_LENS_BETWEEN_LONG: between_long,
    cc.BOUNDARY_ON_INPUT_WORD: lambda f: bool((f["in_start"][1:] % 32 == 0).any()),
    cc.BOUNDARY_ON_OUTPUT_WORD: lambda f: bool(((f["b"][f["first_runs"][1:]] % 32 == 0)
                                                 & (f["in_start"][1:] % 32 != 0)).any()),
    cc.OUT_MULTIPLE: lambda f: f["n_out"] > 0 and f["n_out"] % 32 == 0,
    cc.OUT_MULTIPLE_PLUS: lambda f: f["n_out"] % 32 == 1,
    cc.OUT_MULTIPLE_MINUS: lambda f: f["n_out"] % 32 == 31,
    cc.SINGLE: lambda f: len(f["strings"]) == 1 and f["n_runs"] == 1,
    cc.EMPTY: lambda f: len(f["strings"]) == 0 and f["n_runs"] == 0 and f["n_out"] == 0,
    cc.RANDOM: lambda f: len(f["strings"]) == 200 and f["in_lens"].max() > 3 * np.median(f["in_lens"]),
    cc.HAS_CUT: lambda f: f["n_runs"] > len(f["strings"]),
    cc.HAS_LONG_PIECE: lambda f: bool(f["lens"].any()),
}


@pytest.mark.parametrize("case", cc.CASES, ids=IDS)
def test_a_case_is_what_it_claims(case):
    f = facts(case)
    assert case["covers"]
    for name in case["covers"]:
        assert PREDICATES[name](f), name
    assert case["k"] in cc.KS and sum(len(s) - case["k"] + 1 for s in case["strings"]) < 10000


def test_the_list_covers_every_edge_class():
    assert set(PREDICATES) == set(cc.EDGE_CLASSES)
    covered = {}
    for case in cc.CASES:
        for name in case["covers"]:
            covered.setdefault(name, set()).add(case["k"])
    assert set(covered) == set(cc.EDGE_CLASSES)
    for name, ks in covered.items():  # at every K, but for the two that one K settles
        assert ks == ({4} if name == cc.EIGHT_IN_A_WORD else {23} if name == cc.EMPTY else set(cc.KS)), name
    assert len({c["id"] for c in cc.CASES}) == len(cc.CASES)
    # every shift 0..31 where K - 1 is odd, and the two cut probabilities of the random cases tell in the run counts
    assert reachable_shifts(4) == reachable_shifts(16) == set(range(32))
    for k in cc.KS:
        sparse, dense = (next(c for c in cc.CASES if c["id"] == "random_p%s-k%d" % (p, k)) for p in ("0.02", "0.5"))
        positions = sum(len(s) - k + 1 for s in dense["strings"])
        few = sum(len(s) - k + 1 for s in sparse["strings"])  # (200 runs and about 0.02 cuts per further position)
        assert 200 < sparse["start"].size < 200 + 0.04 * few and dense["start"].size > positions // 3

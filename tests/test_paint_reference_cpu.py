"""Checks of the numpy reference of ksh_seq_class_runs (tests/paint_reference.py) itself: a case worked by hand, the
runs expanded back to ids, adjacent runs differing, the runs summed per column against IndexReference.seq_hits, and
on a small structure built by the oracle against Get(i).Contains of every position.  No GPU."""
import numpy as np

import oracle_lib as ol
import paint_reference as pr
from paint_reference import with_zero_row
from index_reference import IndexReference, class_matrix, revcomp_string
from kmersets import synth

U = np.uint64


def kmers(*words):
    return np.unique(np.array([synth.kmers_of_bases(synth.bases_of_string(w), len(w))[0] for w in words], dtype=U))


def test_hand_worked():
    """K = 4, two nodes without edges, k-mers as written (not canonicalised).
    AACCGG     : AACC in node 0, ACCG in both, CCGG in node 1           -> rows 1, 3, 2
    AACCAACCT  : AACC, then ACCA CCAA CAAC in no node, AACC, ACCT none  -> rows 1, 0, 0, 0, 1, 0
    AACC       : one position."""
    ref = IndexReference(4, [kmers("AACC", "ACCG"), kmers("ACCG", "CCGG")], [[], []])
    strings = ["AACCGG", "AACCAACCT", "AACC"]
    table = np.array([[1, 0], [2, 0], [3, 0]], dtype=U)
    off, start, cls, missing = pr.class_runs(ref, strings, [0, 1], table, False)
    assert off.tolist() == [0, 3, 7, 8]
    assert start.tolist() == [0, 1, 2, 0, 1, 4, 5, 0]
    assert cls.tolist() == [0, 2, 1, 0, -1, 0, -1, 0]
    assert missing == 4
    assert off.dtype == np.int64 and start.dtype == np.int32 and cls.dtype == np.int32
    # with the zero row in the table every id moves up by one and nothing is unmatched
    off, start, cls, missing = pr.class_runs(ref, strings, [0, 1], with_zero_row(table), False)
    assert cls.tolist() == [1, 3, 2, 1, 0, 1, 0, 1] and missing == 0 and start.tolist() == [0, 1, 2, 0, 1, 4, 5, 0]
    # the columns the other way round: rows 1 and 2 change places; one column: ACCG joins its neighbour
    assert pr.class_runs(ref, strings, [1, 0], table, False)[2].tolist() == [1, 2, 0, 1, -1, 1, -1, 1]
    off, start, cls, missing = pr.class_runs(ref, strings, [0], np.array([[0, 0], [1, 0]], dtype=U), False)
    assert off.tolist() == [0, 2, 6, 7] and start.tolist() == [0, 2, 0, 1, 4, 5, 0] and cls.tolist() == [1, 0, 1, 0, 1, 0, 1]
    # canonicalised: GGTT is AACC read from the other strand
    assert pr.class_runs(ref, ["GGTT"], [0, 1], table, True)[2].tolist() == [0]
    assert pr.class_runs(ref, ["GGTT"], [0, 1], table, False)[2].tolist() == [-1]
    assert pr.class_runs(ref, [], [0, 1], table, True)[0].tolist() == [0]


def fabricated(seed, k=9, n_nodes=5, size=300):
    rng = np.random.default_rng(seed)
    genome = synth.random_genome(4 * size, seed)
    pool = synth.canonical_set_of_bases(genome, k)
    node_sets = [np.unique(rng.choice(pool, size=size)) for _ in range(n_nodes)]
    children = [[1, 2], [3], [3], [], []]
    strings = [synth.string_of_bases(genome[a:a + n]) for a, n in ((0, 200), (150, k), (400, 333), (900, k + 1))]
    strings += [revcomp_string(strings[0])]
    return IndexReference(k, node_sets, children), strings


def test_runs_expand_to_the_ids_and_adjacent_runs_differ():
    ref, strings = fabricated(5)
    for cols in ([0, 1, 2, 3, 4], [4, 1], None):
        rows, _ = ref.color_classes(cols)
        for table in (with_zero_row(rows), rows[1::2]):
            for canon in (False, True):
                ids = pr.position_ids(ref, strings, cols, table, canon)
                off, start, cls, missing = pr.class_runs(ref, strings, cols, table, canon)
                lengths = [len(s) - ref.k + 1 for s in strings]
                back = pr.expand(off, start, cls, lengths)
                assert all(np.array_equal(a, b) for a, b in zip(ids, back))
                assert missing == sum(int((i == -1).sum()) for i in ids)
                assert off[-1] == start.size == cls.size and off.size == len(strings) + 1
                for s in range(len(strings)):
                    a, b = off[s], off[s + 1]
                    assert b > a and start[a] == 0 and (np.diff(start[a:b]) > 0).all()
                    assert (np.diff(cls[a:b]) != 0).all()
    # the case has something to show: several runs in a string, and a mirrored string with the mirrored runs
    rows = with_zero_row(ref.color_classes(None)[0])
    off, start, cls, _ = pr.class_runs(ref, strings, None, rows, True)
    assert off[1] > 3
    first, last = slice(off[0], off[1]), slice(off[-2], off[-1])
    assert np.array_equal(cls[first][::-1], cls[last])


def test_a_single_kmer_paints_with_its_class_id():
    """A K-long string of k-mer q has one run, and its class is IndexReference.class_ids of q under the union
    selection (-1 where the table does not hold q's row, or no column holds q): the two references agree."""
    ref, _ = fabricated(7)
    k = ref.k
    absent = np.setdiff1d(synth.canonical(np.arange(5000, 5040, dtype=U), k), ref.kmers)[:5]
    assert absent.size == 5
    for cols in (None, [4, 1], [2, 0, 3]):
        rows, _ = ref.color_classes(cols)
        for table in (rows, rows[1::2], with_zero_row(rows)):
            kmers, ids = ref.class_ids(table, cols)
            some = np.concatenate([ref.kmers[::7], absent])
            strings = ["".join("ACGT"[(int(q) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for q in some]
            off, start, cls, missing = pr.class_runs(ref, strings, cols, table, True)
            assert off.tolist() == list(range(len(strings) + 1)) and not start.any()
            at = np.minimum(np.searchsorted(kmers, some), kmers.size - 1)
            selected = kmers[at] == some  # (in some column: the union selection holds it)
            assert selected[:-5].any() and not selected[-5:].any()
            assert np.array_equal(cls[selected], ids[at[selected]])
            zero = [c for c, r in enumerate(table.tolist()) if r == [0, 0]]
            assert (cls[~selected] == (zero[0] if zero else -1)).all()
            assert missing == int((cls == -1).sum())


def test_runs_summed_per_column_are_seq_hits():
    ref, strings = fabricated(6)
    for cols in ([0, 1, 2, 3, 4], [3, 0]):
        table = with_zero_row(ref.color_classes(cols)[0])
        for canon in (False, True):
            off, start, cls, missing = pr.class_runs(ref, strings, cols, table, canon)
            assert missing == 0
            bits = class_matrix(table, len(cols)).astype(np.int64)
            hits = np.zeros((len(strings), len(cols)), dtype=np.int64)
            for s, text in enumerate(strings):
                a, b = off[s], off[s + 1]
                ends = np.concatenate([start[a + 1:b], [len(text) - ref.k + 1]])
                hits[s] = ((ends - start[a:b])[:, None] * bits[cls[a:b]]).sum(axis=0)
            want = ref.seq_hits(strings, canon)[:, cols]
            assert want.any() and np.array_equal(hits, want)


def test_against_the_oracle_position_by_position():
    """A structure the oracle builds; Get(i) of the oracle is column i (an IndexReference of the Get(i) as nodes
    without edges has exactly that membership matrix).  Every position of every string: the class the runs give it
    has bit i iff the oracle's Get(i) contains the canonical k-mer."""
    k, n, kb, n_sets, size = 15, 10, 2, 4, 400
    sets = synth.phylogeny_sets(k, n_sets, size, seed=3)
    okss = ol.KmerSetSet([ol.Set.from_kmers(k, n, kb, s).compact() for s in sets], synth.sample_bucket_ids(n, seed=4))
    n_nodes = okss.size()
    gets = [okss.get(i) for i in range(n_nodes)]
    ref = IndexReference(k, [g.kmers() for g in gets], [[] for _ in range(n_nodes)])
    strings = okss.node(0).strings()[:6] + okss.node(n_nodes - 1).strings()[:3]
    strings += [revcomp_string(s) for s in strings[:2]] + ["ACGT" * 8]
    cols = list(range(n_nodes))[:128]
    table = with_zero_row(ref.color_classes(cols)[0])
    off, start, cls, missing = pr.class_runs(ref, strings, cols, table, True)
    assert missing == 0
    ids = pr.expand(off, start, cls, [len(s) - k + 1 for s in strings])
    bits = class_matrix(table, len(cols))
    seen = set()
    for s, text in enumerate(strings):
        x = synth.canonical(synth.kmers_of_bases(synth.bases_of_string(text), k), k)
        for p, q in enumerate(x):
            want = [bool(gets[c].contains(int(q))) for c in cols]
            assert bits[ids[s][p]].tolist() == want, (s, p)
            seen.add(int(ids[s][p]))
    assert len(seen) > 2

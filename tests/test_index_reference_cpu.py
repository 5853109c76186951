"""The numpy reference of the index geometry sweep (tests/index_reference.py) against brute force with Python sets on
tiny structures, and the sweep's fabricated structures (tests/index_geometry_cells.py): every case must discriminate
-- several colour classes of distinct sizes, k-mers of one column only and of all non-empty columns, a pair count
that is no trivial value, selections that are neither empty nor everything, class-id requests that select three
classes or more of which none holds more than half of the selection -- so that a wrong answer on the GPU
cannot hide in an empty or a total result.  The route models the GPU test asserts are computed and sanity-checked
here too.  No GPU."""
import collections

import numpy as np
import pytest

import index_geometry_cells as cells
from index_reference import IndexReference, class_matrix, pack_rows, reachable, revcomp_string
from kmersets import synth

U = np.uint64
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def value_of(s):
    v = 0
    for ch in s:
        v = v * 4 + "ACGT".index(ch)
    return v


def brute_canonical(v, k):
    s = cells.kmer_strings([v], k)[0]
    return min(v, value_of("".join(COMP[ch] for ch in reversed(s))))


TINY = [
    # (k, node sets as sets of ints drawn below, children): a DAG with a shared child and an empty node
    (3, 5, [[2, 3], [3], [4], [], []], 1),
    (5, 7, [[4, 5], [4, 6], [5], [], [6], [], []], 2),
    (5, 6, [[1], [2], [3], [], [3, 5], []], 3),  # a chain into a shared sink, ids not in topological order below
]


def tiny_structure(k, n_nodes, seed):
    rng = np.random.default_rng(seed)
    space = 4 ** k
    sets = []
    for j in range(n_nodes):
        if j == n_nodes - 2:
            sets.append(set())  # the empty node
        else:
            sets.append({int(v) for v in rng.choice(space, size=min(space // 3, 40), replace=False)})
    return sets


@pytest.mark.parametrize("k,n_nodes,children,seed", TINY)
def test_reference_equals_brute_force(k, n_nodes, children, seed):
    sets = tiny_structure(k, n_nodes, seed)
    ref = IndexReference(k, [np.array(sorted(s), dtype=U) for s in sets], children)

    def get(i, seen=None):  # the union of node i's set and those of every node reachable from it
        seen = set() if seen is None else seen
        if i in seen:
            return set()
        seen.add(i)
        out = set(sets[i])
        for c in children[i]:
            out |= get(c, seen)
        return out

    gets = [get(i) for i in range(n_nodes)]
    every = sorted(set().union(*sets))
    assert ref.kmers.tolist() == every and ref.n_distinct == len(every)
    assert ref.M.tolist() == [[q in gets[i] for i in range(n_nodes)] for q in every]
    assert reachable(children).tolist() == [[j == i or bool(gets_reach(children, i, j)) for j in range(n_nodes)]
                                            for i in range(n_nodes)]
    # query rows: members, absent k-mers, patterns with a high bit; as written and canonicalised
    patterns = list(range(4 ** k)) + [every[0] | 1 << (2 * k), every[-1] | 1 << 63, 1 << (2 * k)]
    for canon in (False, True):
        want = []
        for z in patterns:
            if z >> (2 * k):
                want.append([False] * n_nodes)
            else:
                q = brute_canonical(z, k) if canon else z
                want.append([q in gets[i] for i in range(n_nodes)])
        assert ref.query_rows(np.array(patterns, dtype=U), canon).tolist() == want
    # seq_hits: positions counted per string, no window across strings
    rng = np.random.default_rng(seed + 10)
    strings = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=n)) for n in (k, k + 1, 40, k, 3 * k)]
    strings.append(cells.kmer_strings(every[:1], k)[0] * 3)
    for canon in (False, True):
        want = []
        for s in strings:
            row = [0] * n_nodes
            for p in range(len(s) - k + 1):
                q = value_of(s[p:p + k])
                q = brute_canonical(q, k) if canon else q
                for i in range(n_nodes):
                    row[i] += q in gets[i]
            want.append(row)
        assert ref.seq_hits(strings, canon).tolist() == want
    assert ref.seq_hits([revcomp_string(s) for s in strings], True).tolist() == ref.seq_hits(strings, True).tolist()
    # pair table, spectrum, selections, classes over all columns and a permuted subset
    for cols in (None, [n_nodes - 1, 0, n_nodes - 2, 1]):
        ids = list(range(n_nodes)) if cols is None else cols
        assert ref.pair_table(cols).tolist() == [[len(gets[a] & gets[b]) for b in ids] for a in ids]
        count = {q: sum(q in gets[c] for c in ids) for q in every}
        assert ref.spectrum(cols).tolist() == [sum(1 for q in every if count[q] == m) for m in range(len(ids) + 1)]
        requests = [dict(min_count=len(ids)), dict(require=[ids[1]], max_count=1),
                    dict(require=[ids[0], ids[1]], exclude=[ids[3]]), dict(min_count=2, max_count=3)]
        for r in requests:
            want = [q for q in every
                    if r.get("min_count", 1) <= count[q] <= r.get("max_count", len(ids))
                    and all(q in gets[x] for x in r.get("require", ()))
                    and not any(q in gets[x] for x in r.get("exclude", ()))]
            assert ref.select(cols, **r).tolist() == want
        tally = collections.Counter(sum((q in gets[c]) << a for a, c in enumerate(ids)) for q in every)
        rows, counts = ref.color_classes(cols)
        assert rows[:, 1].tolist() == [0] * len(tally)
        assert list(zip(rows[:, 0].tolist(), counts.tolist())) == sorted(tally.items())
        assert np.array_equal(pack_rows(class_matrix(rows, len(ids))), rows)
        # class ids: a dict from the row as an integer to its position in the table, asked per selected k-mer; the
        # whole table, every second row of it and the rows above the first, with and without require / exclude
        value = {q: sum((q in gets[c]) << a for a, c in enumerate(ids)) for q in every}
        for r in requests + [dict(), dict(exclude=[ids[2]])]:
            chosen = ref.select(cols, **r).tolist()
            for table in (rows, rows[::2], rows[1:]):
                at = {int(low): c for c, (low, high) in enumerate(table.tolist())}
                kmers, got = ref.class_ids(table, cols, **r)
                assert kmers.tolist() == chosen and got.dtype == np.int64
                assert got.tolist() == [at.get(value[q], -1) for q in chosen]
        kmers, got = ref.class_ids(rows, cols)
        assert (got >= 0).all() and len(set(got.tolist())) > 2
        assert np.bincount(got, minlength=len(tally)).tolist() == [0 if v == 0 else n for v, n in sorted(tally.items())]
        assert (ref.class_ids(rows[::2], cols)[1] < 0).any()
    # the bucketed form of a selection at two geometries
    sel = ref.select(None)
    for n_bits, kb in ((1, 2), (2 * k - 1, 4)):
        off, keys = ref.bucketed(sel, n_bits, kb)
        assert np.array_equal(synth.from_bucketed(off, keys, k, n_bits), sel) and keys.dtype.itemsize == kb
        want_off, want_keys = synth.to_bucketed(sel, k, n_bits, kb)
        assert np.array_equal(off, want_off) and np.array_equal(keys, want_keys)


def gets_reach(children, i, j):
    todo, seen = [i], set()
    while todo:
        cur = todo.pop()
        if cur in seen:
            continue
        seen.add(cur)
        todo.extend(children[cur])
    return j in seen


def test_packed_rows_use_both_words():
    bits = np.zeros((3, 70), dtype=bool)
    bits[0, 0] = bits[1, 63] = bits[2, 69] = True
    assert pack_rows(bits).tolist() == [[1, 0], [1 << 63, 0], [0, 1 << 5]]


def test_cells_and_variants():
    """The sweep holds every cell of the geometry sweep, the extra cells, and the plain variant where the issue of
    the all-ones key is: at the full-width keys of both widths that have them, and once per key width."""
    from test_gpu_geometry import CELLS

    canon = [c for c, plain in cells.CASES if not plain]
    plain = [c for c, p in cells.CASES if p]
    assert set(CELLS) <= set(canon) and len(set(cells.CASES)) == len(cells.CASES)
    assert set(cells.EXTRA) <= set(plain) and {cells.WIDEST, cells.ONE_BIT_WIDE} <= set(canon)
    assert {kb for k, n, kb in cells.FULL_WIDTH} == {2, 4} and set(cells.FULL_WIDTH) <= set(plain)
    assert {kb for k, n, kb in plain} == {2, 4, 8}
    assert {c[0] for c in cells.K3_CELLS} == {3} and len(cells.K3_CELLS) == 2
    assert set(cells.BORROWED_CELLS) <= set(CELLS)
    for k, n, kb in canon + plain:
        assert 2 * k - n <= 8 * kb and n < 2 * k and n <= 24, (k, n, kb)


MODELS = {}


@pytest.mark.parametrize("case", cells.CASES, ids=[cells.case_id(c) for c in cells.CASES])
def test_fixture_discriminates(case):
    cell, plain = case
    k, n, kb = cell
    node_sets = cells.fabricate(case)
    assert len(node_sets) == cells.N_NODES and node_sets[cells.EMPTY_NODE].size == 0
    a, b = cells.TWINS
    assert np.array_equal(node_sets[a], node_sets[b]) and node_sets[a].size
    whole = node_sets[cells.WHOLE]
    assert all(np.isin(s, whole).all() for s in node_sets)
    key_bits = 2 * k - n
    if plain:  # key 0 and the all-ones key, in the first and in the last bucket, in every non-empty node
        for s in (node_sets[i] for i in ([cells.WHOLE] if cell == cells.DENSE else cells.NONEMPTY)):
            assert np.isin(cells.plain_sentinels(k, n), s).all()
        keys = whole & U((1 << key_bits) - 1)
        assert keys.min() == 0 and keys.max() == (1 << key_bits) - 1
        assert (whole >> U(key_bits)).min() == 0 and (whole >> U(key_bits)).max() == (1 << n) - 1
    else:
        assert np.array_equal(synth.canonical(whole, k), whole)
    ref = IndexReference(k, node_sets, cells.CHILDREN)
    assert ref.n_distinct == whole.size
    # at least three colour classes with pairwise distinct counts, none of them the zero row
    rows, counts = ref.color_classes()
    assert rows.any(axis=1).all() and len(set(counts.tolist())) >= 3, counts
    assert counts.sum() == ref.n_distinct
    # a k-mer of one column only, and one of all non-empty columns (no column but the empty node's is empty)
    per_row = ref.M.sum(axis=1)
    empty_cols = [i for i in range(cells.N_NODES) if not ref.M[:, i].any()]
    assert empty_cols == [cells.EMPTY_NODE]
    assert (per_row == 1).any() and (per_row == cells.N_NODES - 1).any()
    # an off-diagonal pair count that is neither 0 nor a diagonal value
    table = ref.pair_table()
    off = table[~np.eye(cells.N_NODES, dtype=bool)]
    assert ((off != 0) & ~np.isin(off, np.diag(table))).any()
    sub = ref.pair_table(cells.PERMUTED)
    assert np.array_equal(sub, table[np.ix_(cells.PERMUTED, cells.PERMUTED)])
    # every select request: neither empty nor everything
    for request in cells.SELECTS:
        got = ref.select(**request)
        assert 0 < got.size < ref.n_distinct, request
    # every class-id request: at least three distinct ids against the full table of its columns, and no id on more
    # than half of the selection -- a constant id array, or ids that left their keys, cannot pass
    for request, distinct, largest in zip(cells.CLASS_REQUESTS, (6, 4, 4) if k >= 4 else (5, 3, 3), (0.38, 0.38, 0.5)):
        kmers, ids = ref.class_ids(ref.color_classes(request["cols"])[0], **request)
        assert np.array_equal(kmers, ref.select(**request)) and (ids >= 0).all(), request
        share = np.bincount(ids) / ids.size
        assert (share > 0).sum() >= 3 and share.max() <= 0.5, (request, share)
        if cell != cells.DENSE:  # the dealing of PART_OF_RANK: the same classes at every geometry
            assert (share > 0).sum() == distinct and share.max() <= largest + 0.005, (request, share)
        # neighbouring keys have different classes somewhere in every bucket that holds several k-mers of several
        # classes: an id that left its key in a tile's sort shows
        assert (np.diff(ids) != 0).mean() > 0.3, request
    q = cells.queries_of(ref, plain, seed=k * 31 + n)
    hit = ref.query_rows(q, not plain).any(axis=1)
    assert hit[:ref.n_distinct].all() and not hit[-3:].any()
    if k >= 4:
        seqs = cells.sequences_of(ref, plain, seed=k * 31 + n)
        hits = ref.seq_hits(seqs, not plain)
        assert all(len(s) >= k for s in seqs) and len(seqs[-1]) == 3 * k
        assert hits[-1, cells.WHOLE] >= 3 and hits[:16, cells.WHOLE].tolist() == [1] * 16
        assert not hits[:, cells.EMPTY_NODE].any()
    # the route model
    model = cells.route_model(case, node_sets)
    MODELS[case] = model
    assert model["total_entries"] == sum(s.size for s in node_sets)
    assert model["largest_slice_bytes"] <= kb * model["largest_bucket"] <= kb * model["total_entries"]
    if n >= cells.LARGE_N:  # 16 workgroups or more for the walk of 2^N mostly empty buckets
        assert model["total_entries"] >= cells.LARGE_N_MIN_ENTRIES
    if case == (cells.DENSE, True):
        # the closed forms of the moduli: Get(0) = multiples of 2, 7 or 5; Get(1) of 3, 7 or 5; Get(4) of 7 or 5; ...
        space = 4 ** k
        union = [[2, 7, 5], [3, 7, 5], [5], [1], [7, 5], [], [5]]
        want = [cells.count_multiples(m, space) if m else 0 for m in union]
        assert np.diag(table).tolist() == want and want[3] == space == ref.n_distinct
        assert ref.select(**cells.SELECTS[0]).size == cells.count_multiples([5], space)
        # private to 0 among {0, 1, 2}: the even numbers that 3, 5 and 7 do not divide
        private = cells.count_multiples([2], space) - count_even_multiples([3, 5, 7], space)
        assert ref.select(**cells.SELECTS[1]).size == private
        # Get(0) & Get(3) \ Get(4): the even numbers that 5 and 7 do not divide
        assert ref.select(**cells.SELECTS[2]).size == cells.count_multiples([2], space) - count_even_multiples([5, 7], space)
        only_whole = space - cells.count_multiples([2, 3, 5, 7], space)
        assert int(counts[(rows[:, 0] == 1 << cells.WHOLE)][0]) == only_whole
        assert model["largest_slice_bytes"] == 2 * 32768 and model["oversize"] and model["pair_split"]


def count_even_multiples(moduli, limit):
    """|{even x in [0, limit): some m of the odd moduli divides x}|."""
    return cells.count_multiples([2 * m for m in moduli], limit)


def test_route_models_cover_both_sides():
    """Per key width the cases reach a cut bucket and an uncut one, a slice above the join's LDS stage and one
    below: what the GPU test's route table asserts it saw."""
    assert len(MODELS) == len(cells.CASES), "the fixture checks did not run"
    for kb in (2, 4, 8):
        mine = [m for ((k, n, b), plain), m in MODELS.items() if b == kb]
        assert {m["pair_split"] for m in mine} == {True, False}, kb
        assert {m["oversize"] for m in mine} == {True, False}, kb

"""The five calls that read a KssIndex -- query, seq_hits, pair_counts, select / spectrum and color_classes -- at every
class of bucket geometry and key width of tests/test_gpu_geometry.py, plus three cells of their own, against one
numpy reference (tests/index_reference.py): the membership matrix of a fabricated structure of seven nodes.

What changes with (k, N, key bytes) in these kernels: the tile walk of csrc/ksh_rowtile.h cuts every bucket by key
range at small N and strides over millions of empty buckets at large N; the all-ones key of a full-width key type
sits next to the walk's empty-slot sentinel; the query splits a pattern by the key bits and reads keys in the key
type; the join stages a node's slice of a bucket in 32 KiB of LDS, which is another number of keys per key width;
keys wider than the minimum take another instantiation of every kernel.  Every result is compared for equality, and
every case asserts the routes it must have taken from a model computed on the CPU (tests/index_geometry_cells.py),
so that no case drifts silently to the other route.  tests/test_index_reference_cpu.py checks the reference against
brute force and that every structure used here discriminates."""
import numpy as np
import pytest
import torch

import geometry_families as gf
import index_geometry_cells as cells
from index_reference import IndexReference, class_matrix, revcomp_string
from kmersets import capi, synth

pytestmark = pytest.mark.gpu
U = np.uint64
TABLE = {}


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def encode_nodes(ctx, g, node_sets, plain):
    return [ctx.spss_encode(capi.DeviceSet.from_kmers(g, s, ctx.device), mode=0, canonical=not plain)
            for s in node_sets]


def check_query(idx, ref, plain, model, seed):
    q = cells.queries_of(ref, plain, seed)
    want = ref.query_rows(q, not plain)
    assert want[:ref.n_distinct].any(axis=1).all() and not want[-3:].any()
    seen = 0
    for route in (1, 2, 0):
        got = idx.query(q, canonicalize=not plain, route=route)
        routes = idx.routes()
        assert np.array_equal(got, want), "route %d" % route
        if route == 2:
            assert routes & capi.QROUTE_JOIN and not routes & capi.QROUTE_SEARCH
            # k_query_join stages a slice of len <= kSliceBytes / sizeof(KeyT) keys; every non-empty bucket is asked
            assert bool(routes & capi.QROUTE_OVERSIZE) == model["oversize"], model
        else:  # (auto joins only above 256 MiB of resident keys)
            assert routes & capi.QROUTE_SEARCH and not routes & (capi.QROUTE_JOIN | capi.QROUTE_OVERSIZE)
        seen |= routes
    return seen


def check_walk_route(idx, model):
    """pc_tile_cut sets the flag iff a bucket's first tile finds more than kTile entries left."""
    routes = idx.routes()
    assert bool(routes & capi.QROUTE_PAIR_SPLIT) == model["pair_split"], model
    return routes


def check_pair_counts(idx, ref, model, sub, all_columns=True):
    """-> the GPU's tables over all columns and over `sub`, and the routes seen."""
    table, seen = None, 0
    if all_columns:
        table, n_distinct = idx.pair_counts(with_distinct=True)
        seen = check_walk_route(idx, model)
        assert np.array_equal(table, ref.pair_table()) and n_distinct == ref.n_distinct
    part, n_distinct = idx.pair_counts(cols=sub, flush_rows=1, with_distinct=True)
    seen |= check_walk_route(idx, model)
    assert np.array_equal(part, ref.pair_table(sub)) and n_distinct == ref.n_distinct
    return table, part, seen


def check_select(ctx, idx, ref, model, requests, probe):
    """-> the GPU's spectrum per request."""
    g = idx.g
    spectra = []
    for request in requests:
        want = ref.select(**request)
        assert 0 < want.size < ref.n_distinct, request
        want_off, want_keys = ref.bucketed(want, g.n_bucket_bits, g.key_bytes)
        off, n_keys, spec = idx.select_count(spectrum=True, **request)
        check_walk_route(idx, model)
        assert n_keys == want.size, request
        assert np.array_equal(off.cpu().numpy(), want_off), request
        assert np.array_equal(spec, ref.spectrum(request["cols"])), request
        spectra.append(spec)
        # the keys, as KssIndex.select writes them: the result is an ordinary set at this geometry
        with torch.cuda.stream(ctx.stream):
            keys = torch.empty(max(n_keys * g.key_bytes, 16), dtype=torch.uint8, device=ctx.device)
        idx.select_write(off, n_keys, keys, **request)
        check_walk_route(idx, model)
        d = capi.DeviceSet(g, off, keys, n_keys)
        assert np.array_equal(d.to_numpy()[1], want_keys), request
        assert np.array_equal(ctx.set_kmers(d), want), request
        assert ctx.set_hash(d) == int(np.bitwise_xor.reduce(want)), request
        assert np.array_equal(ctx.set_contains(d, probe), np.isin(probe, want)), request
    return spectra


def check_classes(idx, ref, model, cols, table, spectrum):
    """Rows and counts equal the reference; their marginals equal the GPU's own spectrum and pair table."""
    rows, counts = idx.color_classes(cols)
    check_walk_route(idx, model)
    want_rows, want_counts = ref.color_classes(cols)
    assert rows.shape == want_rows.shape and np.array_equal(rows, want_rows)
    assert np.array_equal(counts, want_counts) and counts.sum() == ref.n_distinct
    n_cols = len(ref.cols_of(cols))
    m = class_matrix(rows, n_cols).astype(np.int64)
    by_popcount = np.zeros(n_cols + 1, dtype=np.int64)
    np.add.at(by_popcount, m.sum(axis=1), counts)
    assert np.array_equal(by_popcount, spectrum)
    assert np.array_equal(m.T @ (m * counts[:, None]), table)


def check_seq_hits(ctx, idx, ref, plain, own_strings, seed):
    g = idx.g
    few = cells.sequences_of(ref, plain, seed)
    seqs = list(own_strings) + [revcomp_string(s) for s in own_strings] + few
    want = ref.seq_hits(seqs, not plain)
    assert want.any() and (want.sum(axis=0) > 0).sum() >= 2
    dseqs = capi.DeviceSpss.from_strings(g, seqs, ctx.device)
    for route in (0, 1, 2):
        got = idx.seq_hits(dseqs, canonicalize=not plain, route=route)
        routes = idx.routes()
        assert np.array_equal(got, want), "route %d" % route
        assert routes & (capi.QROUTE_JOIN if route == 2 else capi.QROUTE_SEARCH)
        assert not routes & capi.QROUTE_SEQ_PASSES
    # passes of seven positions: every string longer than that is split across passes and its counts add up
    got = idx.seq_hits(few, canonicalize=not plain, route=1, pass_positions=7)
    assert idx.routes() & capi.QROUTE_SEQ_PASSES
    assert np.array_equal(got, want[-len(few):])


def check_all(ctx, idx, ref, plain, model, own_strings, seed, sub, requests, all_columns=True):
    """All five calls on one index; -> the routes seen.  all_columns=False leaves out the passes over all columns
    and all but the last request (the borrowed index at N = 24: each pass walks 2^24 buckets)."""
    k = ref.k
    seen = check_query(idx, ref, plain, model, seed)
    table, part, walk = check_pair_counts(idx, ref, model, sub, all_columns)
    seen |= walk
    probe = np.concatenate([ref.kmers[::max(1, ref.n_distinct // 2000)], cells.absent_kmers(ref, 500, not plain, seed)])
    spectra = check_select(ctx, idx, ref, model, requests if all_columns else requests[-1:], probe)
    assert requests[-1]["cols"] == sub
    check_classes(idx, ref, model, sub, part, spectra[-1])
    if all_columns:
        check_classes(idx, ref, model, None, table, idx.spectrum(None))
    if k >= 4:
        check_seq_hits(ctx, idx, ref, plain, own_strings, seed)
    else:  # documented in include/kmersets_hip.h: ksh_seq_hits needs K >= 4; the index still serves
        with pytest.raises(capi.KshError) as e:
            idx.seq_hits(["ACGT"], canonicalize=not plain)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and "K >= 4" in str(e.value)
        q = cells.queries_of(ref, plain, seed + 1)
        assert np.array_equal(idx.query(q, canonicalize=not plain), ref.query_rows(q, not plain))
    return seen


@pytest.mark.parametrize("case", cells.CASES, ids=[cells.case_id(c) for c in cells.CASES])
def test_index_cell(ctx, case):
    (k, n, kb), plain = case
    g = capi.geom(k, n, kb)
    assert g.key_bytes == kb
    node_sets = cells.fabricate(case)
    ref = IndexReference(k, node_sets, cells.CHILDREN)
    model = cells.route_model(case, node_sets)
    comps = encode_nodes(ctx, g, node_sets, plain)
    idx = capi.KssIndex.from_nodes(ctx, comps, cells.CHILDREN, canonical=not plain)
    assert idx.n_nodes == cells.N_NODES
    seen = check_all(ctx, idx, ref, plain, model, comps[0].to_strings(), k * 31 + n, cells.PERMUTED, cells.SELECTS)
    idx.close()
    TABLE[case] = (model, seen)


@pytest.mark.parametrize("cell", cells.K3_CELLS, ids=["k%d-N%d-u%d" % (k, n, 8 * kb) for k, n, kb in cells.K3_CELLS])
def test_k3_cells_ran_the_refusal(cell):
    """The k = 3 cells of the sweep took the seq_hits refusal and served a query after it (check_all)."""
    assert cell[0] < 4 and (cell, False) in TABLE, "the k = 3 cells did not run"


def test_dense_cell_closed_forms(ctx):
    """(8, 1) dense and plain: the GPU's numbers against the closed forms of the moduli (the reference's own are
    pinned to them in tests/test_index_reference_cpu.py)."""
    case = (cells.DENSE, True)
    k, n, kb = cells.DENSE
    g = capi.geom(k, n, kb)
    comps = encode_nodes(ctx, g, cells.fabricate(case), True)
    idx = capi.KssIndex.from_nodes(ctx, comps, cells.CHILDREN, canonical=False)
    space = 4 ** k
    union = [[2, 7, 5], [3, 7, 5], [5], [1], [7, 5], [], [5]]  # Get(i) = the multiples of any of these
    table, n_distinct = idx.pair_counts(with_distinct=True)
    assert n_distinct == space and idx.routes() & capi.QROUTE_PAIR_SPLIT
    assert np.diag(table).tolist() == [cells.count_multiples(m, space) if m else 0 for m in union]
    assert table[0, 1] == cells.count_multiples([6, 7, 5], space)  # the multiples of 2 and 3, or of 7, or of 5
    _, n_core, spec = idx.select_count(spectrum=True, offsets=False, **cells.SELECTS[0])
    assert n_core == cells.count_multiples([5], space) == spec[6]
    assert spec[0] == 0 and spec[1] == space - cells.count_multiples([2, 3, 5, 7], space)
    rows, counts = idx.color_classes()
    assert counts[rows[:, 0] == 1 << cells.WHOLE].tolist() == [space - cells.count_multiples([2, 3, 5, 7], space)]
    # all 8-mers and nothing else: every query hits column 3, on the join's HBM route too
    q = np.arange(space + 3, dtype=U)
    got = idx.query(q, canonicalize=False, route=2)
    assert idx.routes() & capi.QROUTE_OVERSIZE
    assert got[:space, cells.WHOLE].all() and not got[space:].any()
    assert np.array_equal(got[:space, 2], q[:space] % U(5) == 0)
    idx.close()


def borrowed_inputs(k, n):
    """Four sets of the cell's pool that share three eighths of it and hold an eighth each of their own."""
    # (at N >= 22 a larger pool, as in index_geometry_cells.pool_size: the built nodes hold every k-mer once, and the
    # walk starts a workgroup per 8192 of them)
    pool = cells.pool_of(k, n) if n < cells.LARGE_N else gf.family("genome", k, 2 * cells.LARGE_N_POOL, seed=cells.FAMILY_SEED + k)
    h = synth.mix64(np.arange(pool.size, dtype=U) + U(77 * k + n)) % U(8)
    sets = [pool[(h < 3) | (h == 3 + i)] for i in range(4)]
    if n <= 8:
        ids = np.arange(1 << n, dtype=np.int32)  # (a sample of 2^N / 50 buckets would be empty or nearly)
    else:
        ids = np.unique(synth.mix64(np.arange((1 << n) // 50, dtype=U) + U(5)) % U(1 << n)).astype(np.int32)
    return sets, ids


@pytest.mark.parametrize("cell", cells.BORROWED_CELLS,
                         ids=["k%d-N%d-u%d" % (k, n, 8 * kb) for k, n, kb in cells.BORROWED_CELLS])
def test_borrowed_index(ctx, cell):
    """A built DeviceKmerSetSet at three geometries: the index that borrows its resident node sets and the one that
    decodes its node containers both give the reference's answers, the reference being computed from the nodes and
    children the build left.  The only part of this module that runs the build."""
    k, n, kb = cell
    g = capi.geom(k, n, kb)
    sets, ids = borrowed_inputs(k, n)
    inputs = encode_nodes(ctx, g, sets, False)
    dkss = capi.DeviceKmerSetSet(ctx, inputs, ids)
    n_nodes = dkss.size()
    children = [dkss.children(i) for i in range(n_nodes)]
    node_sets = [dkss.node_kmers(i) for i in range(n_nodes)]
    print("nodes: %d, sizes %s, children %s" % (n_nodes, [s.size for s in node_sets], children))
    assert n_nodes > 4 and any(children), "the build merged nothing: no DAG to close"
    ref = IndexReference(k, node_sets, children)
    for i, s in enumerate(sets):  # Get(i) of the built structure is input i
        assert np.array_equal(ref.kmers[ref.M[:, i]], s), i
    model = cells.route_model(((k, n, kb), False), node_sets)
    if n >= cells.LARGE_N:
        assert model["total_entries"] >= cells.LARGE_N_MIN_ENTRIES
    sub = [n_nodes - 1, 2, 0, n_nodes - 2]
    requests = [dict(cols=[0, 1, 2, 3], min_count=4), dict(cols=[0, 1, 2, 3], require=[0], max_count=1),
                dict(cols=sub, require=[0], exclude=[2])]
    strings = [dkss.node_strings(i) for i in range(n_nodes)]
    borrowed = capi.KssIndex.from_kss(dkss)
    owned = capi.KssIndex.from_nodes(ctx, [capi.DeviceSpss.from_strings(g, s, ctx.device) for s in strings], children)
    for idx in (borrowed, owned):
        assert idx.n_nodes == n_nodes
        check_all(ctx, idx, ref, False, model, strings[0], k * 31 + n, sub, requests, all_columns=n < cells.LARGE_N)
    owned.close()
    borrowed.close()
    dkss.close()


def test_route_table():
    """The case -> routes table (run with -s to see it): per key width a cut bucket and an uncut one, a slice above
    the join's LDS stage and one below, the join and the search."""
    assert len(TABLE) == len(cells.CASES), "the cases did not run"
    print("\n%-22s %9s %9s %12s  %s" % ("case", "entries", "bucket", "slice bytes", "routes"))
    names = [(capi.QROUTE_SEARCH, "search"), (capi.QROUTE_JOIN, "join"), (capi.QROUTE_OVERSIZE, "oversize"),
             (capi.QROUTE_PAIR_SPLIT, "split")]
    for case, (model, seen) in sorted(TABLE.items(), key=lambda t: (t[0][0][1], t[0][0][0], t[0][0][2], t[0][1])):
        print("%-22s %9d %9d %12d  %s" % (cells.case_id(case), model["total_entries"], model["largest_bucket"],
                                          model["largest_slice_bytes"],
                                          " ".join(name for bit, name in names if seen & bit)))
    for kb in (2, 4, 8):
        mine = [seen for ((k, n, b), plain), (model, seen) in TABLE.items() if b == kb]
        for bit, name in names:
            assert any(s & bit for s in mine), (kb, name)
        for bit in (capi.QROUTE_OVERSIZE, capi.QROUTE_PAIR_SPLIT):
            assert any(not s & bit for s in mine), (kb, bit)

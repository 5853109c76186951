"""The seven calls that read a KssIndex -- query, seq_hits, pair_counts, select / spectrum, color_classes,
select_class_ids and class_runs -- at every class of bucket geometry and key width of tests/test_gpu_geometry.py, plus
three cells of their own, against one numpy reference (tests/index_reference.py, and tests/paint_reference.py on top
of it): the membership matrix of a fabricated structure of seven nodes.

What changes with (k, N, key bytes) in these kernels: the tile walk of csrc/ksh_rowtile.h cuts every bucket by key
range at small N and strides over millions of empty buckets at large N; the all-ones key of a full-width key type
sits next to the walk's empty-slot sentinel; the query splits a pattern by the key bits and reads keys in the key
type; the join stages a node's slice of a bucket in 32 KiB of LDS, which is another number of keys per key width;
keys wider than the minimum take another instantiation of every kernel.  The class-id walk keeps a tile's selected
keys in 64-bit LDS words beside their ids, pads its sort with the sentinel, narrows the keys on the way out and
places a bucket's tiles one after the other; the painting's own kernels depend on the pass cuts and on the route that
filled the rows.  Every result is compared for equality, and every case asserts the routes it must have taken from a
model computed on the CPU (tests/index_geometry_cells.py), so that no case drifts silently to the other route.
tests/test_index_reference_cpu.py checks the reference against brute force and that every structure used here
discriminates."""
import numpy as np
import pytest
import torch

import geometry_families as gf
import index_geometry_cells as cells
import paint_reference as pr
from paint_reference import with_zero_row
from index_reference import IndexReference, class_matrix, revcomp_string
from kmersets import capi, synth

pytestmark = pytest.mark.gpu
U = np.uint64
TABLE = {}
TAIL, PATTERN, KEY_BYTE = 64, 0x5A5A5A5A, 0xA5  # the elements behind every result buffer and what they are filled with


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


def fresh_ids(ctx, g, n_keys):
    """Key and id buffers of n_keys + TAIL elements, prefilled."""
    with torch.cuda.stream(ctx.stream):
        return (torch.full(((n_keys + TAIL) * g.key_bytes,), KEY_BYTE, dtype=torch.uint8, device=ctx.device),
                torch.full((n_keys + TAIL,), PATTERN, dtype=torch.int32, device=ctx.device))


def host_keys(g, keys, n_keys):
    """(the first n_keys keys in the key type, whether every byte behind them is still the pattern)"""
    raw = keys.cpu().numpy()
    cut = n_keys * g.key_bytes
    return raw[:cut].view({2: np.uint16, 4: np.uint32, 8: np.uint64}[g.key_bytes]), bool((raw[cut:] == KEY_BYTE).all())


def host_class_ids(ids, n_keys):
    raw = ids.cpu().numpy()
    return raw[:n_keys].astype(np.int64), bool((raw[n_keys:] == PATTERN).all())


def check_class_ids(ctx, idx, ref, model, requests):
    """select_class_ids per request against IndexReference.class_ids, key by key and id by id, the table being the
    reference's; once per case without keys, with every second row of the table, and the refusal of that table."""
    g = idx.g
    seen = 0
    for at, request in enumerate(requests):
        cols = request["cols"]
        table, counts = ref.color_classes(cols)
        want_kmers, want_ids = ref.class_ids(table, **request)
        want_off, want_keys = ref.bucketed(want_kmers, g.n_bucket_bits, g.key_bytes)
        n_keys = int(want_kmers.size)
        assert (want_ids >= 0).all() and np.unique(want_ids).size >= 3, request
        off, got_n, _ = idx.select_count(**request)
        assert got_n == n_keys and np.array_equal(off.cpu().numpy(), want_off), request
        keys, ids = fresh_ids(ctx, g, n_keys)
        assert idx.select_class_ids(off, n_keys, table, keys, ids, **request) is None
        seen |= check_walk_route(idx, model)
        got_keys, keys_tail = host_keys(g, keys, n_keys)
        got_ids, ids_tail = host_class_ids(ids, n_keys)
        assert np.array_equal(got_keys, want_keys), request
        assert np.array_equal(got_ids, want_ids), request
        assert keys_tail and ids_tail, request
        if request == dict(cols=None):  # the union over all nodes: every k-mer of the structure, class by class
            assert np.array_equal(np.bincount(got_ids, minlength=counts.size), counts)
        if at == 0 and len(requests) > 1:  # d_keys = NULL: the same ids (not where one request alone is run: N = 24)
            _, alone = fresh_ids(ctx, g, n_keys)
            idx.select_class_ids(off, n_keys, table, None, alone, **request)
            check_walk_route(idx, model)
            got_ids, ids_tail = host_class_ids(alone, n_keys)
            assert np.array_equal(got_ids, want_ids) and ids_tail
        if request is requests[min(1, len(requests) - 1)]:  # every second row of the table (request (b))
            reduced = table[::2]
            _, partial = ref.class_ids(reduced, **request)
            assert (partial < 0).any() and (partial >= 0).any(), request
            keys, ids = fresh_ids(ctx, g, n_keys)
            missing = idx.select_class_ids(off, n_keys, reduced, keys, ids, allow_unmatched=True, **request)
            check_walk_route(idx, model)
            got_ids, ids_tail = host_class_ids(ids, n_keys)
            assert np.array_equal(got_ids, partial) and ids_tail and missing == int((partial < 0).sum())
            assert np.array_equal(ids.cpu().numpy()[:n_keys].view(np.uint32) == capi.CLASS_NONE, partial < 0)
            assert np.array_equal(host_keys(g, keys, n_keys)[0], want_keys)
            with pytest.raises(capi.KshError) as e:
                idx.select_class_ids(off, n_keys, reduced, keys, ids, **request)
            assert e.value.code == capi.KSH_FAILED_PRECONDITION and "rows" in str(e.value)
            keys, ids = fresh_ids(ctx, g, n_keys)  # ... and the index serves the full table again
            idx.select_class_ids(off, n_keys, table, keys, ids, **request)
            assert np.array_equal(host_class_ids(ids, n_keys)[0], want_ids)
            assert np.array_equal(host_keys(g, keys, n_keys)[0], want_keys)
    return seen


def paint_call(ctx, idx, dseqs, table, want, **kw):
    """One ksh_seq_class_runs call with run buffers of capacity + TAIL prefilled elements, the capacity being the
    reference's number of runs (a call that makes more is refused) -> the result on the host; the tail is intact."""
    capacity = int(want[0][-1])
    with torch.cuda.stream(ctx.stream):
        off = torch.full((dseqs.n_strings + 1,), -5, dtype=torch.int64, device=ctx.device)
        start = torch.full((capacity + TAIL,), PATTERN, dtype=torch.int32, device=ctx.device)
        cls = torch.full((capacity + TAIL,), PATTERN, dtype=torch.int32, device=ctx.device)
    rc, n_runs, missing = idx.class_runs_raw(dseqs, table, capacity, off, start, cls, **kw)
    assert rc == capi.KSH_OK, capi.lib().ksh_last_error().decode()
    assert n_runs == capacity
    start, cls = start.cpu().numpy(), cls.cpu().numpy()
    assert (start[capacity:] == PATTERN).all() and (cls[capacity:] == PATTERN).all()
    return off.cpu().numpy(), start[:capacity], cls[:capacity], missing


def same_runs(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]


def check_class_runs(ctx, idx, ref, plain, model, whole_strings, seed, column_lists):
    """class_runs per column list against paint_reference.class_runs on the three routes, with the table as the
    reference gives it (positions without a class), and in passes of 7 and 257 positions; -> the routes the join
    took."""
    g = idx.g
    canon = not plain
    strings = cells.paint_strings(whole_strings, ref, plain, seed)
    few = cells.paint_strings_for_passes(whole_strings, ref, plain, seed)
    dseqs = capi.DeviceSpss.from_strings(g, strings, ctx.device)
    dfew = capi.DeviceSpss.from_strings(g, few, ctx.device)
    assert sum(len(s) - ref.k + 1 for s in few) > 257
    join = 0
    for at, cols in enumerate(column_lists):
        bare = ref.color_classes(cols)[0]
        table = with_zero_row(bare)
        want = pr.class_runs(ref, strings, cols, table, canon)
        # the reference's answer discriminates: runs inside strings, several classes, a run of several positions
        lengths = [len(s) - ref.k + 1 for s in strings]
        assert want[0][-1] > len(strings) and np.unique(want[2]).size >= 3 and want[3] == 0, cols
        assert want[0][-1] < sum(lengths), cols
        for route in (1, 2, 0):
            got = paint_call(ctx, idx, dseqs, table, want, cols=cols, canonicalize=canon, route=route)
            routes = idx.routes()
            assert same_runs(got, want), (cols, route)
            assert not routes & capi.QROUTE_SEQ_PASSES
            if route == 2:
                assert routes & capi.QROUTE_JOIN and not routes & capi.QROUTE_SEARCH
                assert model["oversize"] or not routes & capi.QROUTE_OVERSIZE, model  # (not every bucket is asked)
                join |= routes
            else:  # (auto joins only above 256 MiB of resident keys)
                assert routes & capi.QROUTE_SEARCH and not routes & (capi.QROUTE_JOIN | capi.QROUTE_OVERSIZE)
        # the table without the zero row: the positions of k-mers that no column holds have no class
        want = pr.class_runs(ref, strings, cols, bare, canon)
        got = paint_call(ctx, idx, dseqs, bare, want, cols=cols, canonicalize=canon, route=1 + at % 2)
        assert same_runs(got, want), cols
        assert np.array_equal(got[2].view(np.uint32) == capi.CLASS_NONE, want[2] < 0)
        # passes: every string longer than a pass is cut, and a run goes on from one pass into the next
        want = pr.class_runs(ref, few, cols, table, canon)
        for pass_positions, route in ((7, 1), (257, 2 - at % 2)):
            got = paint_call(ctx, idx, dfew, table, want, cols=cols, canonicalize=canon, route=route,
                             pass_positions=pass_positions)
            assert same_runs(got, want), (cols, pass_positions, route)
            assert idx.routes() & capi.QROUTE_SEQ_PASSES
    return join


def check_all(ctx, idx, ref, plain, model, own_strings, seed, sub, requests, class_requests, paint_from,
              all_columns=True):
    """All seven calls on one index; -> the routes seen, those of the class-id walk and those of the painting on the
    join.  all_columns=False leaves out the passes over all columns and all but the last request, and of the
    class-id requests all but the one over `sub` (the borrowed index at N = 24: each pass walks 2^24 buckets)."""
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
    assert class_requests[1]["cols"] == sub
    walk = check_class_ids(ctx, idx, ref, model, class_requests if all_columns else class_requests[1:2])
    join = 0
    if k >= 4:
        join = check_class_runs(ctx, idx, ref, plain, model, paint_from, seed, (None, sub))
    else:  # ksh_seq_class_runs needs K >= 4 as ksh_seq_hits does; the index still serves
        with pytest.raises(capi.KshError) as e:
            idx.class_runs(["ACGT"], ref.color_classes(sub)[0], sub, canonicalize=not plain)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and "K >= 4" in str(e.value)
        q = cells.queries_of(ref, plain, seed + 2)
        assert np.array_equal(idx.query(q, canonicalize=not plain), ref.query_rows(q, not plain))
    return seen, walk, join


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
    seen, walk, join = check_all(ctx, idx, ref, plain, model, comps[0].to_strings(), k * 31 + n, cells.PERMUTED,
                                 cells.SELECTS, cells.CLASS_REQUESTS, comps[cells.WHOLE].to_strings())
    idx.close()
    TABLE[case] = (model, seen, walk, join)


@pytest.mark.parametrize("cell", cells.K3_CELLS, ids=["k%d-N%d-u%d" % (k, n, 8 * kb) for k, n, kb in cells.K3_CELLS])
def test_k3_cells_ran_the_refusal(cell):
    """The k = 3 cells of the sweep took the refusals of seq_hits and class_runs and served a query after each, and
    ran the class ids (check_all)."""
    assert cell[0] < 4 and (cell, False) in TABLE, "the k = 3 cells did not run"
    assert TABLE[(cell, False)][3] == 0  # (nothing was painted)


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
    # the class ids of the union over all nodes.  A multiple of 5 is in every non-empty node; any other multiple of 7
    # in nodes 0, 1, 3 and 4; any other x in node 3, in node 0 if it is even and in node 1 if 3 divides it: six
    # classes, and the keys with id c are exactly the x whose divisibility by (2, 3, 5, 7) is that of row c
    x = np.arange(space, dtype=np.int64)
    row_of = np.where(x % 5 == 0, 0x5F, np.where(x % 7 == 0, 0x1B, 8 + (x % 2 == 0) + 2 * (x % 3 == 0)))
    want_rows = np.array([[8, 0], [9, 0], [10, 0], [11, 0], [0x1B, 0], [0x5F, 0]], dtype=U)
    assert np.array_equal(rows, want_rows)
    off, n_keys, _ = idx.select_count()
    assert n_keys == space and off.cpu().numpy().tolist() == [0, space // 2, space]
    keys, ids = fresh_ids(ctx, g, n_keys)
    idx.select_class_ids(off, n_keys, want_rows, keys, ids)
    assert idx.routes() & capi.QROUTE_PAIR_SPLIT
    got_keys, keys_tail = host_keys(g, keys, n_keys)
    got_ids, ids_tail = host_class_ids(ids, n_keys)
    assert keys_tail and ids_tail
    assert np.array_equal(got_keys, (x % (space // 2)).astype(np.uint16))  # 15 key bits: consecutive keys, twice
    assert np.array_equal(got_ids, np.searchsorted(want_rows[:, 0], row_of.astype(U)))
    both = cells.count_multiples([5, 7], space)
    assert np.bincount(got_ids, minlength=6).tolist() == [
        space - cells.count_multiples([2, 3, 5, 7], space),
        cells.count_multiples([2, 5, 7], space) - cells.count_multiples([6, 5, 7], space),
        cells.count_multiples([3, 5, 7], space) - cells.count_multiples([6, 5, 7], space),
        cells.count_multiples([6, 5, 7], space) - both,
        both - cells.count_multiples([5], space),
        cells.count_multiples([5], space)]
    assert counts.tolist() == np.bincount(got_ids, minlength=6).tolist()
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
    try:  # (a structure must not outlive its context: a failing check leaves none behind for the collector)
        check_borrowed(ctx, g, cell, sets, dkss)
    finally:
        dkss.close()


def check_borrowed(ctx, g, cell, sets, dkss):
    k, n, kb = cell
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
    # (c) here: what input 1 does not hold.  The own eighths of inputs 0, 2 and 3 are three classes whatever the
    # build made of them (Get(i) is input i), where require=[0] would select two, the shared part and input 0's own
    class_requests = [dict(cols=None), dict(cols=sub), dict(cols=None, exclude=[1])]
    strings = [dkss.node_strings(i) for i in range(n_nodes)]
    # the strings to paint are those of all distinct k-mers together, as node WHOLE's are on the fabricated structures:
    # a node's own strings are of one class each, these pass from the k-mers of one node into those of another
    union = capi.DeviceSet.from_kmers(g, ref.kmers, ctx.device)
    every_string = ctx.spss_encode(union, mode=0, canonical=True).to_strings()
    borrowed = capi.KssIndex.from_kss(dkss)
    owned = capi.KssIndex.from_nodes(ctx, [capi.DeviceSpss.from_strings(g, s, ctx.device) for s in strings], children)
    try:
        for idx in (borrowed, owned):
            assert idx.n_nodes == n_nodes
            check_all(ctx, idx, ref, False, model, strings[0], k * 31 + n, sub, requests, class_requests,
                      every_string, all_columns=n < cells.LARGE_N)
    finally:
        owned.close()
        borrowed.close()


def test_route_table():
    """The case -> routes table (run with -s to see it): per key width a cut bucket and an uncut one, a slice above
    the join's LDS stage and one below, the join and the search; the class-id walk with and without a cut bucket,
    the painting on the join with and without a slice above the stage."""
    assert len(TABLE) == len(cells.CASES), "the cases did not run"
    print("\n%-22s %9s %9s %12s  %s" % ("case", "entries", "bucket", "slice bytes", "routes"))
    names = [(capi.QROUTE_SEARCH, "search"), (capi.QROUTE_JOIN, "join"), (capi.QROUTE_OVERSIZE, "oversize"),
             (capi.QROUTE_PAIR_SPLIT, "split")]
    by_n = sorted(TABLE.items(), key=lambda t: (t[0][0][1], t[0][0][0], t[0][0][2], t[0][1]))
    for case, (model, seen, walk, join) in by_n:
        print("%-22s %9d %9d %12d  %s | ids: %s | paint: %s" % (
            cells.case_id(case), model["total_entries"], model["largest_bucket"], model["largest_slice_bytes"],
            " ".join(name for bit, name in names if seen & bit), " ".join(name for bit, name in names if walk & bit),
            " ".join(name for bit, name in names if join & bit)))
    for kb in (2, 4, 8):
        mine = [seen for ((k, n, b), plain), (model, seen, walk, join) in TABLE.items() if b == kb]
        walks = [walk for ((k, n, b), plain), (model, seen, walk, join) in TABLE.items() if b == kb]
        joins = [join for ((k, n, b), plain), (model, seen, walk, join) in TABLE.items() if b == kb and k >= 4]
        assert {bool(w & capi.QROUTE_PAIR_SPLIT) for w in walks} == {True, False}, kb
        assert all(j & capi.QROUTE_JOIN for j in joins), kb
        assert {bool(j & capi.QROUTE_OVERSIZE) for j in joins} == {True, False}, kb
        for bit, name in names:
            assert any(s & bit for s in mine), (kb, name)
        for bit in (capi.QROUTE_OVERSIZE, capi.QROUTE_PAIR_SPLIT):
            assert any(not s & bit for s in mine), (kb, bit)

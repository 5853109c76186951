"""Encode, decode and set operations at every class of bucket geometry and key width, against one oracle run per
family (the strings do not depend on the geometry: tests/test_oracle_geometry_cpu.py pins that) and numpy.

The GPU path changes shape across (k, N, key bytes): the decode takes the wide route above N = 14 with a u16, u32
or u64 composite; the encode stages its neighbour probe (k_rc_*, k_adj_rc1 / k_adj_rc, k_adj_fwd_targets) only
for N <= 14, enough key bits and groups at most four windows long, and probes in place (k_adjacency) otherwise;
the rc kernels' thread count follows n / 2^N.  Each cell below belongs to one or more classes, and every cell
asserts which probe route it took, so that no cell drifts silently to the other one."""
import numpy as np
import pytest

import geometry_families as gf
import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu
U = np.uint64

# (k, N, device key bytes): the classes each cell stands for are in the comments
CELLS = [
    (7, 1, 2), (15, 1, 4), (23, 1, 8),                 # N = 1: one bucket
    (8, 2, 2), (16, 2, 4), (25, 2, 8),                 # N = 2 (even k: canonical sets without self-rc k-mers)
    (7, 7, 2), (9, 8, 2), (19, 8, 4), (27, 8, 8),      # N = 7, 8: one-level scatter (7 key bits: in place)
    (11, 13, 2), (15, 14, 2), (19, 13, 4), (23, 14, 4), (27, 13, 8), (31, 14, 8),  # N = 13, 14; 16 / 32 key bits
    (15, 15, 2), (16, 16, 2), (17, 18, 2), (19, 17, 4), (23, 20, 4), (25, 18, 4), (31, 20, 8),  # N = 15 .. 20
    (19, 22, 2), (13, 24, 2), (27, 22, 4), (23, 24, 4), (31, 24, 8),  # N = 22, 24
    (3, 5, 2), (3, 5, 4), (7, 13, 2), (9, 17, 2), (11, 21, 2), (11, 21, 8),  # one key bit
    (15, 14, 4), (15, 14, 8), (23, 14, 8), (19, 22, 4), (25, 18, 8),  # keys wider than the minimum
]
SIZE = {15: 70000, 23: 50000}  # N = 1 past the staged probe's four windows; other k: 20 000
FAMILY_SEED = 500
COUNT_CELLS = {(25, 18, 4), (27, 22, 4)}  # the u32 -> u64 composite route of the counter
TABLE = {}


def size_of(k):
    return SIZE.get(k, 20000)


def staged_model(k, n_bits, kb, n):
    """The encode plan's test for the staged probe (csrc/ksh_encode.hip): N <= 14, 2K >= N + 4, key bits >= N + 2
    + (N & 1), and a bucket at most four LDS windows of (78 KB - 64) / (key bytes + 6) records."""
    key_bits = 2 * k - n_bits
    return (n_bits <= 14 and 2 * k >= n_bits + 4 and key_bits >= n_bits + 2 + (n_bits & 1)
            and n >> n_bits <= 4 * ((78 * 1024 - 4 * 16) // (kb + 6)))


def rc_threads(n, n_bits):
    per_group = n >> n_bits
    return "rc_1024" if per_group > 4096 else "rc_512" if per_group > 1024 else "rc_256" if per_group > 256 else "rc_64"


def composite(k, n_bits, kb):
    """The wide decode's composite type (csrc/ksh_decode.hip, decode_write_t): None on the narrow route."""
    if n_bits <= 14:
        return None
    cbits = 2 * k - 14
    return "u%d" % (8 * max(2 if cbits <= 16 else 4 if cbits <= 32 else 8, kb))


def test_cells_cover_the_classes():
    """Every class of the sweep is present for every key width it allows (CPU arithmetic on the cell list)."""
    for k, n, kb in CELLS:
        assert 2 * k - n <= 8 * kb and n < 2 * k and n <= 24, (k, n, kb)
    widths = lambda pred: {kb for k, n, kb in CELLS if pred(k, n, kb)}  # noqa: E731
    for ns in ({1}, {2}, {7, 8}, {13, 14}, {15, 16, 17, 20}, {22, 24}):
        assert widths(lambda k, n, kb: n in ns) == {2, 4, 8}, ns
    for n in (15, 16, 17, 20, 22, 24):
        assert any(c[1] == n for c in CELLS), n
    assert {(k, n) for k, n, kb in CELLS if 2 * k - n == 1} == {(3, 5), (7, 13), (9, 17), (11, 21)}
    assert widths(lambda k, n, kb: 2 * k - n == 1) == {2, 4, 8}
    full = {(kb, n <= 14) for k, n, kb in CELLS if 2 * k - n == 8 * kb}
    assert {(2, True), (2, False), (4, True), (4, False)} <= full
    minimal = lambda k, n: capi.geom(k, n).key_bytes  # noqa: E731
    wider = {(minimal(k, n), kb) for k, n, kb in CELLS if kb > minimal(k, n)}
    assert {(2, 4), (2, 8), (4, 8)} <= wider
    comps = {(kb, composite(k, n, kb)) for k, n, kb in CELLS}
    assert {(2, "u32"), (4, "u64")} <= comps


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def families():
    """Per k: each family's k-mers, the oracle's strings (one run, at the reference geometry) and the k-mers that
    decoding those strings gives, canonical and as written."""
    cache = {}

    def get(k):
        if k not in cache:
            out = {}
            for name in gf.FAMILIES:
                x = gf.family(name, k, size_of(k), seed=FAMILY_SEED + k)
                want = gf.oracle_answers(ol, name, k, x)
                lines = want["spss_directed" if name == "directed" else "spss"]
                out[name] = {"kmers": x, "want": want, "lines": lines,
                             "dec_canon": gf.kmers_of_strings(lines, k, canonical=True),
                             "dec_fwd": gf.kmers_of_strings(lines, k, canonical=False)}
            cache[k] = out
        return cache[k]

    return get


def check_bucketed(d, kmers):
    g = d.g
    want_off, want_keys = synth.to_bucketed(kmers, g.k, g.n_bucket_bits, g.key_bytes)
    off, keys = d.to_numpy()
    assert d.n_keys == kmers.size
    assert np.array_equal(off, want_off)
    assert np.array_equal(keys, want_keys)


def contains_queries(x, k, seed):
    mask = U((1 << (2 * k)) - 1)
    some = x[:: max(1, x.size // 500)]
    nexts = np.concatenate([((some << U(2)) & mask) | U(c) for c in range(4)])
    prevs = np.concatenate([(some >> U(2)) | U(a << (2 * k - 2)) for a in range(4)])
    rnd = synth.mix64(np.arange(2000, dtype=U) + U(seed)) & mask
    high = np.concatenate([some[:64] | U(1 << (2 * k)), some[:64] | U(1 << 63), synth.mix64(np.arange(64, dtype=U) + U(seed + 1))])
    return np.concatenate([some, nexts, prevs, rnd, high])


def reads_of(k, seed):
    """Overlapping reads of a 3000-base genome (each k-mer seen about four times) plus unique random reads."""
    bases = synth.random_genome(3000, 0x5EED0000 + seed)
    starts = (synth.mix64(np.arange(100, dtype=U) + U(seed)) % U(bases.size - 120)).astype(np.int64)
    reads = [synth.string_of_bases(bases[p:p + 120]) for p in starts]
    noise = synth.random_genome(40 * 60, seed + 1)
    reads += [synth.string_of_bases(noise[i:i + 60]) for i in range(0, noise.size, 60)]
    return reads


@pytest.mark.parametrize("cell", CELLS, ids=["k%d-N%d-u%d" % (k, n, 8 * kb) for k, n, kb in CELLS])
def test_geometry_cell(ctx, families, cell):
    k, n, kb = cell
    g = capi.geom(k, n, kb)
    assert g.key_bytes == kb
    fams = families(k)
    routes_seen = set()
    row = {"staged": set()}
    for i, name in enumerate(gf.FAMILIES):
        f = fams[name]
        x = f["kmers"]
        canon = name != "directed"
        d = capi.DeviceSet.from_kmers(g, x, ctx.device)
        assert d.n_keys == x.size
        # encode: every mode against the oracle's strings, and the round trip
        modes = ((0, "spss"), (1, "unitigs"), (2, "spss_slow")) if canon else ((0, "spss_directed"), (1, "unitigs_directed"))
        for mode, variant in modes:
            sp = ctx.spss_encode(d, mode=mode, canonical=canon)
            routes = ctx.spss_encode_routes()
            routes_seen |= routes
            staged = canon and staged_model(k, n, kb, x.size)
            assert ("probe_staged" in routes) == staged, (name, mode, sorted(routes))
            if canon:
                row["staged"].add(staged)
            if staged:
                assert rc_threads(x.size, n) in routes and "rc1_streamed" in routes, (name, sorted(routes))
            got = sp.to_strings()
            assert got == f["want"][variant], (name, variant)
            if mode == 0:
                back = ctx.spss_decode(sp, canonical=canon)
                assert back.n_keys == d.n_keys and ctx.set_diff(back, d) == 0, name
        # decode of the oracle's strings, canonical and as written
        lines = capi.DeviceSpss.from_strings(g, f["lines"], ctx.device)
        check_bucketed(ctx.spss_decode(lines, canonical=True), f["dec_canon"])
        check_bucketed(ctx.spss_decode(lines, canonical=False), f["dec_fwd"])
        # hash, contains
        assert ctx.set_hash(d) == (int(np.bitwise_xor.reduce(x)) if x.size else 0)
        q = contains_queries(x, k, seed=k * 31 + n + i)
        assert np.array_equal(ctx.set_contains(d, q), np.isin(q, x)), name
        # set algebra with the next family
        y = fams[gf.FAMILIES[(i + 1) % len(gf.FAMILIES)]]["kmers"]
        e = capi.DeviceSet.from_kmers(g, y, ctx.device)
        inter, amb, bma = ctx.pair_algebra(d, e)
        assert np.array_equal(ctx.set_kmers(inter), np.intersect1d(x, y))
        assert np.array_equal(ctx.set_kmers(amb), np.setdiff1d(x, y))
        assert np.array_equal(ctx.set_kmers(bma), np.setdiff1d(y, x))
        assert np.array_equal(ctx.set_kmers(ctx.set_union(d, e)), np.union1d(x, y))
        assert ctx.set_diff(d, e) == np.setdiff1d(x, y).size + np.setdiff1d(y, x).size
    if k % 2 == 0:
        # refused on purpose: an even-k canonical set with a self-reverse-complement k-mer
        x = fams["genome"]["kmers"]
        h = x[:1] >> U(k)  # the top k / 2 bases of a member, then their reverse complement
        pal = (h << U(k)) | synth.revcomp(h, k // 2)
        assert gf.self_rc(pal, k).all()
        bad = np.union1d(x, pal)
        with pytest.raises(capi.KshError, match="own reverse"):
            ctx.spss_encode(capi.DeviceSet.from_kmers(g, bad, ctx.device), mode=0)
    if cell in COUNT_CELLS:
        reads = reads_of(k, seed=n)
        frags = capi.DeviceSpss.from_strings(g, reads, ctx.device)
        allk = np.concatenate([synth.canonical(synth.kmers_of_bases(synth.bases_of_string(r), k), k) for r in reads])
        uniq, cnt = np.unique(allk, return_counts=True)
        for cutoff in (1, 2, 3):
            got, n_cut = ctx.kmer_count(frags, cutoff)
            assert n_cut == int((cnt < cutoff).sum())
            check_bucketed(got, uniq[cnt >= cutoff])
        assert 0 < (cnt >= 3).sum() < uniq.size
    TABLE[cell] = (sorted(row["staged"]), composite(k, n, kb),
                   sorted(r for r in routes_seen if r.startswith("rc_") or r in ("rc1_streamed", "tgt_parts")))


def test_group_probe_one_key_bit(ctx):
    """Regression: at N = 2K - 1 the four k-mers Next(x, A..T) span two buckets (one key bit), and
    DevSet::for_group4 searched only the first -- the edges to Next(x, G) and Next(x, T) were seen from one side
    only, which broke the encode (a GPU memory fault at (3, 5)); k_edges read the last base as key & 3.  Every edge
    of this genome set whose group straddles a bucket boundary must come out as the oracle's strings, in every mode."""
    k, n = 7, 13
    kmers = synth.phylogeny_sets(k, 1, 300, seed=3)[0]
    mask = U((1 << (2 * k)) - 1)
    nxt = np.concatenate([((kmers << U(2)) & mask) | U(c) for c in (2, 3)])
    assert np.isin(synth.canonical(nxt, k), kmers).sum() > 20  # edges into the second bucket of a group
    g = capi.geom(k, n)
    d = capi.DeviceSet.from_kmers(g, kmers, ctx.device)
    o = ol.Set.from_kmers(k, n, 2, kmers)
    assert ctx.spss_encode(d, mode=0).to_strings() == o.spss()
    assert ctx.spss_encode(d, mode=1).to_strings() == o.unitigs()
    assert ctx.spss_encode(d, mode=2).to_strings() == o.spss_slow()
    assert ctx.spss_encode(d, mode=0, canonical=False).to_strings() == o.spss_directed()
    assert ctx.spss_encode(d, mode=1, canonical=False).to_strings() == o.unitigs_directed()


def test_route_table():
    """The cell -> routes table (run with -s to see it); both probe routes and the wide composites occur."""
    assert TABLE, "the cells did not run"
    print("\n%-14s %-16s %-10s %s" % ("cell", "probe", "composite", "rc / target routes"))
    for (k, n, kb), (staged, comp, rc) in sorted(TABLE.items(), key=lambda t: (t[0][1], t[0][0], t[0][2])):
        probe = "+".join("staged" if s else "in-place" for s in staged)
        print("%-14s %-16s %-10s %s" % ("(%d,%d,u%d)" % (k, n, 8 * kb), probe, comp or "-", " ".join(rc)))
    staged = {s for v in TABLE.values() for s in v[0]}
    assert staged == {True, False}
    comps = {(kb, v[1]) for (k, n, kb), v in TABLE.items()}
    assert {(2, "u32"), (4, "u64")} <= comps

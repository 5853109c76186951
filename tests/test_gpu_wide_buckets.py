"""GPU tests for 2^15 .. 2^24 buckets: the decode's wide route (ksh_decode.hip, N > 14: counting, scatter and
sort on 2^14 coarse buckets with composite keys, then fine offsets and narrowing), the counter's cutoff path on
it, and everything that decodes or works on such sets (encode round trip, pair algebra and weights, Contains,
KmerSetSet).  N <= 20 against the oracle; N = 22 and 24 against numpy (the sorted unique canonical k-mers split
into bucket and key), where the oracle's 2^N per-bucket tables are too large."""
import numpy as np
import pytest

import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

U = np.uint64


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def kb_of(k, n):
    return capi.geom(k, n).key_bytes


def genome_strings(k, size, seed, pieces=3):
    """A random genome of about `size` k-mers cut into `pieces` overlapping strings, and its canonical k-mers."""
    bases = synth.random_genome(size + k - 1, seed)
    cut = np.linspace(0, bases.size, pieces + 1).astype(int)
    strings = [synth.string_of_bases(bases[max(0, a - k + 1):b]) for a, b in zip(cut[:-1], cut[1:])]
    return [s for s in strings if len(s) >= k], synth.canonical_set_of_bases(bases, k)


def decode(ctx, k, n, strings, canonical=True):
    g = capi.geom(k, n)
    return ctx.spss_decode(capi.DeviceSpss.from_strings(g, strings, ctx.device), canonical=canonical)


def check_against_numpy(ctx, d, kmers):
    """offsets, keys, size and hash of the decoded set d == the bucketed sorted unique k-mers."""
    g = d.g
    want_off, want_keys = synth.to_bucketed(kmers, g.k, g.n_bucket_bits, g.key_bytes)
    off, keys = d.to_numpy()
    assert d.n_keys == kmers.size
    assert np.array_equal(off, want_off)
    assert np.array_equal(keys, want_keys)
    assert ctx.set_hash(d) == ctx.set_hash(capi.DeviceSet.from_kmers(g, kmers, ctx.device))


def check_against_oracle(ctx, d, oset):
    check_against_numpy(ctx, d, oset.kmers())
    assert ctx.set_hash(d) == oset.hash()


ORACLE_GEOMS = [(21, 15, 4), (23, 16, 4), (23, 20, 4), (31, 18, 8), (15, 16, 2), (17, 18, 2), (9, 16, 2)]


@pytest.mark.parametrize("geom", ORACLE_GEOMS)
def test_decode_vs_oracle(ctx, geom):
    k, n, kb = geom
    assert kb_of(k, n) == kb
    size = 150 if k == 9 else 20000
    genome = synth.phylogeny_sets(k, 1, size, seed=k + n)[0]
    rnd = synth.uniform_pair(k, min(size, 4 ** k // 8), 0.0, seed=k * n)[0]
    for kmers in (genome, rnd):
        o = ol.Set.from_kmers(k, n, kb, kmers)
        lines = o.spss()
        d = decode(ctx, k, n, lines)
        check_against_oracle(ctx, d, ol.Set.from_spss(lines, k, n, kb))
        assert np.array_equal(d.kmers(), kmers)


@pytest.mark.parametrize("geom", [(31, 24, 8), (19, 22, 2), (23, 22, 4)])
def test_decode_vs_numpy(ctx, geom):
    k, n, kb = geom
    assert kb_of(k, n) == kb
    strings, want = genome_strings(k, 200000, seed=n)
    check_against_numpy(ctx, decode(ctx, k, n, strings), want)


@pytest.mark.parametrize("geom", [(23, 16, 4), (17, 18, 2), (31, 24, 8)])
def test_decode_large_two_level(ctx, geom):
    """Over 2^20 k-mers: the coarse scatter takes the two-level route (k_decode_l1 / l2)."""
    k, n, _ = geom
    strings, want = genome_strings(k, 1200000, seed=3 * n, pieces=40)
    check_against_numpy(ctx, decode(ctx, k, n, strings), want)


@pytest.mark.parametrize("geom", [(23, 16, 4), (19, 22, 2), (31, 24, 8)])
def test_decode_empty_one_bucket_last_bucket(ctx, geom):
    k, n, kb = geom
    # the empty set
    d = decode(ctx, k, n, [])
    assert d.n_keys == 0 and not d.offsets.cpu().numpy().any()
    key_bits = 2 * k - n
    rnd = synth.mix64(np.arange(3000, dtype=U) + U(77 * n)) & U((1 << key_bits) - 1)
    for bucket in (0, 5, (1 << n) - 1):
        # k-mers as-is (not canonical: the last bucket's T... k-mers never are), one string each
        kmers = np.unique((U(bucket) << U(key_bits)) | rnd)
        strings = [ol.kmer_str(int(x), k) for x in kmers]
        d = decode(ctx, k, n, strings, canonical=False)
        check_against_numpy(ctx, d, kmers)
        off = d.offsets.cpu().numpy()
        assert off[bucket + 1] - off[bucket] == kmers.size


@pytest.mark.parametrize("geom", [(23, 16, 4), (31, 18, 8), (17, 18, 2)])
def test_decode_oversize_coarse_bucket(ctx, geom):
    """25 000 k-mers under one 14-bit prefix, spread over its fine buckets: the coarse bucket exceeds the sort's
    LDS window (15 872 four-byte, 7 936 eight-byte composites) and takes the partition-first path."""
    k, n, kb = geom
    low = 2 * k - 14
    rnd = synth.mix64(np.arange(25000, dtype=U) + U(1000 + n)) & U((1 << low) - 1)
    kmers = np.unique((U(0x1234) << U(low)) | rnd)
    strings = [ol.kmer_str(int(x), k) for x in kmers]
    d = decode(ctx, k, n, strings, canonical=False)
    check_against_oracle(ctx, d, ol.Set.from_spss(strings, k, n, kb, canonical=False))
    off = d.offsets.cpu().numpy()
    first = 0x1234 << (n - 14)
    assert np.count_nonzero(np.diff(off)[first:first + (1 << (n - 14))]) > 1


@pytest.mark.parametrize("geom", [(23, 16, 4), (17, 18, 2), (31, 20, 8)])
def test_decode_drops_repeated_kmers(ctx, geom):
    """A hand-written SPSS with k-mers repeated within and across strings (also reverse complemented):
    duplicates dropped, offsets rewritten -- in place (4-byte composites in 4-byte keys) and through the wider
    scratch (2-byte keys at K = 17)."""
    k, n, kb = geom
    strings, _ = genome_strings(k, 6000, seed=n + 5, pieces=2)
    s = strings[0]
    rc = synth.string_of_bases(3 - synth.bases_of_string(s)[::-1])
    lines = [s, s[10:300], rc, strings[1], s[: k + 3], s]
    o = ol.Set.from_spss(lines, k, n, kb)
    d = decode(ctx, k, n, lines)
    assert d.n_keys < sum(len(x) - k + 1 for x in lines)
    check_against_oracle(ctx, d, o)


def reads_fasta(k, seed):
    bases = synth.random_genome(4000, seed)
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, bases.size - 120, size=200)
    reads = [synth.string_of_bases(bases[p:p + 120]) for p in starts]
    return "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)).encode()


@pytest.mark.parametrize("geom", [(23, 16, 4), (17, 18, 2)])
def test_kmer_count_cutoff(ctx, geom):
    import torch

    k, n, kb = geom
    g = capi.geom(k, n)
    text = reads_fasta(k, seed=n)
    frags = ctx.fasta_fragments(g, torch.frombuffer(bytearray(text), dtype=torch.uint8).to(ctx.device))
    for cutoff in (1, 3):
        oc = ol.Counter(k, n, kb)
        assert oc.from_fasta(text) == 0
        want, want_cut = oc.to_set(cutoff)
        got, n_cut = ctx.kmer_count(frags, cutoff)
        assert n_cut == want_cut
        check_against_oracle(ctx, got, want)
        if cutoff == 3:
            assert 0 < got.n_keys < oc.size() and n_cut > 0


@pytest.mark.parametrize("geom", [(23, 16, 4), (31, 20, 8)])
def test_encode_decode_round_trip(ctx, geom):
    k, n, kb = geom
    kmers = synth.phylogeny_sets(k, 1, 30000, seed=n + 31)[0]
    o = ol.Set.from_kmers(k, n, kb, kmers)
    d = capi.DeviceSet.from_kmers(capi.geom(k, n), kmers, ctx.device)
    sp = ctx.spss_encode(d, mode=0)
    assert sp.to_strings() == o.spss()
    back = ctx.spss_decode(sp)
    check_against_oracle(ctx, back, o)


def test_pair_ops_and_contains(ctx):
    k, n, kb = 23, 18, 4
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 4, 20000, seed=61)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets[:2])
    oa, ob = (ol.Set.from_kmers(k, n, kb, s) for s in sets[:2])
    oi = oa.intersection(ob)
    inter, amb, bma = ctx.pair_algebra(a, b)
    assert np.array_equal(inter.kmers(), oi.kmers())
    assert np.array_equal(amb.kmers(), oa.copy().sub_set(oi).kmers())
    assert np.array_equal(bma.kmers(), ob.copy().sub_set(oi).kmers())
    assert ctx.set_diff(a, b) == oa.diff(ob)
    assert ctx.set_hash(inter) == oi.hash()
    # Contains: members, their Next k-mers, random patterns
    mask = U((1 << (2 * k)) - 1)
    some = sets[0][::40]
    nexts = np.concatenate([((some << U(2)) & mask) | U(c) for c in range(4)])
    rnd = synth.mix64(np.arange(2000, dtype=U) + U(9)) & mask
    q = np.concatenate([some, nexts, rnd])
    assert np.array_equal(ctx.set_contains(a, q), np.array([bool(oa.contains(int(x))) for x in q]))
    # pair weights over the 2^18 / 50 sampled buckets
    ids = synth.sample_bucket_ids(n, seed=62)
    kss = ol.KmerSetSet([ol.Set.from_kmers(k, n, kb, s).compact() for s in sets], ids, max_iterations=0)
    dsets = [capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets]
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    got = ctx.pair_weights(dsets, ids, pairs)
    assert np.array_equal(got, kss.initial_weights(4)) and got.sum() > 0


def test_kmer_set_set_vs_oracle(ctx):
    k, n, kb, n_sets = 23, 16, 4, 8
    sets = synth.phylogeny_sets(k, n_sets, 20000, seed=71)
    ocomp = [ol.Set.from_kmers(k, n, kb, s).compact() for s in sets]
    ids = synth.sample_bucket_ids(n, seed=72)
    okss = ol.KmerSetSet(ocomp, ids)
    g = capi.geom(k, n)
    dkss = capi.DeviceKmerSetSet(ctx, [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocomp], ids)
    it = dkss.trace()[0]
    assert np.array_equal(it, okss.iterations()) and len(it) > 0
    assert dkss.meta() == okss.meta()
    for i in range(okss.size()):
        assert dkss.node_strings(i) == okss.node(i).strings(), "node %d" % i
    for i in range(n_sets):
        got = dkss.get_kmers(i)
        assert np.array_equal(got, sets[i]) and np.array_equal(got, okss.get(i).kmers())
    dkss.close()


def test_kmer_set_set_n22(ctx):
    """8 small sets at N = 22 (83 886 sampled buckets): Get(i) gives every input back."""
    k, n, n_sets = 23, 22, 8
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, n_sets, 5000, seed=81)
    inputs = []
    for s in sets:
        d = capi.DeviceSet.from_kmers(g, s, ctx.device)
        inputs.append(ctx.spss_encode(d, mode=0))
    ids = synth.sample_bucket_ids(n, seed=82)
    dkss = capi.DeviceKmerSetSet(ctx, inputs, ids)
    assert dkss.size() >= n_sets
    for i in range(n_sets):
        got = dkss.get_kmers(i)
        assert np.array_equal(got, sets[i]), "set %d" % i
        size, h = dkss.get_size_and_hash(i)
        assert size == sets[i].size
        assert h == ctx.set_hash(capi.DeviceSet.from_kmers(g, sets[i], ctx.device))
    dkss.close()


def test_pair_weights_chunked_n24(ctx):
    """16 sets at N = 24: 120 pairs x 335 544 sampled buckets = 4 x 10^7 segments, over the bound above which the pair
    list goes in chunks; every weight == the common k-mers in sampled buckets (numpy)."""
    k, n, n_sets = 23, 24, 16
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, n_sets, 3000, seed=91)
    ids = synth.sample_bucket_ids(n, seed=92)
    dsets = [capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets]
    pairs = [(i, j) for i in range(n_sets) for j in range(i + 1, n_sets)]
    assert len(pairs) * ids.size > 1 << 25
    got = ctx.pair_weights(dsets, ids, pairs)
    shift = U(2 * k - n)
    want = [np.count_nonzero(np.isin((np.intersect1d(sets[i], sets[j]) >> shift).astype(np.int64), ids))
            for i, j in pairs]
    assert np.array_equal(got, np.array(want)) and got.sum() > 0

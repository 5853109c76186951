"""GPU parity tests for the path cover from caller-supplied unitigs (ksh_spss_cover_plan / _write,
Context.spss_cover): GetSPSSCanonical(unitigs, prefixes, suffixes, fast) and GetSPSS(unitigs, prefixes)
(lib/core/spss.h:697-1014, :1039-1829) against the oracle, string for string and in order."""
import numpy as np
import pytest

import cover_oracle
import oracle_lib as ol
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

GEOMS = [(9, 10, 1), (15, 14, 2), (23, 14, 4), (31, 14, 8)]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def cover(ctx, k, n, strings, canonical=True, fast=True):
    sp = capi.DeviceSpss.from_strings(capi.geom(k, n), strings, ctx.device)
    return ctx.spss_cover(sp, canonical=canonical, fast=fast)


def check_all(ctx, k, n, kb, kmers):
    """The oracle's unitigs through every cover == the oracle's SPSS of the same set."""
    oset = ol.Set.from_kmers(k, n, kb, kmers)
    u = oset.unitigs()
    out = cover(ctx, k, n, u)
    want = oset.spss()
    assert out.to_strings() == want
    assert out.n_strings == len(want) and out.n_bases == sum(len(s) for s in want)
    assert ctx.spss_size(out) == oset.size()
    st = ctx.spss_cover_stats()
    assert st["unitigs"] == len(u) and st["strings"] == len(want) and st["bases"] == out.n_bases
    assert cover(ctx, k, n, u, fast=False).to_strings() == oset.spss_slow()
    ud = oset.unitigs_directed()
    assert cover(ctx, k, n, ud, canonical=False).to_strings() == oset.spss_directed()
    return oset


def read_shaped(k, which, seed):
    if which == 0:
        return synth.random_read_kmers(k, 150 if k < 7 else 6000, seed=seed, canonical=True)
    if which == 1:
        return synth.phylogeny_sets(k, 1, 20000, seed=seed)[0]
    return synth.genome_with_tips(k, 20000, seed, every=97)


# ------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("which", [0, 1, 2])
def test_cover_oracle_unitigs(ctx, geom, which):
    k, n, kb = geom
    check_all(ctx, k, n, kb, read_shaped(k, which, seed=k + which))


# ------------------------------------------------------------------------------ 2. any order / orientation
@pytest.mark.parametrize("geom", GEOMS)
def test_cover_any_order_and_orientation(ctx, geom):
    k, n, kb = geom
    oset = ol.Set.from_kmers(k, n, kb, read_shaped(k, 2, seed=3 * k))
    mixed = cover_oracle.shuffled(oset.unitigs(), seed=k)
    assert cover(ctx, k, n, mixed).to_strings() == cover_oracle.oracle_capi_cover(mixed, k)
    assert cover(ctx, k, n, mixed, fast=False).to_strings() == cover_oracle.cover(mixed, k, fast=False)
    ud = cover_oracle.shuffled(oset.unitigs_directed(), seed=k + 1, flip=False)
    assert cover(ctx, k, n, ud, canonical=False).to_strings() == cover_oracle.cover(ud, k, canonical=False)


# ------------------------------------------------------------------------------ 3. loops, dense graphs
def test_cover_loops_and_dense_graphs(ctx):
    for seed in range(20):
        k = [5, 7, 9, 11][seed % 4]
        km = synth.circular_with_tails(k, 20 + (seed * 7) % 150, seed % 5, 1 + seed % 4, seed)
        check_all(ctx, k, min(10, 2 * k - 4), 4, km)
    rng = np.random.default_rng(23)
    for trial in range(16):
        k = 5 if trial % 2 == 0 else 7
        m = int(rng.integers(1, 4 ** k))
        km = np.unique(synth.canonical(rng.integers(0, 4 ** k, size=m, dtype=np.uint64), k))
        oset = check_all(ctx, k, min(10, 2 * k - 4), 4, km)
        mixed = cover_oracle.shuffled(oset.unitigs(), seed=trial)
        n = min(10, 2 * k - 4)
        assert cover(ctx, k, n, mixed).to_strings() == cover_oracle.oracle_capi_cover(mixed, k)
        assert cover(ctx, k, n, mixed, fast=False).to_strings() == cover_oracle.cover(mixed, k, fast=False)


# ------------------------------------------------------------------------------ 4. small shapes
def test_cover_small_shapes(ctx):
    k, n = 9, 10
    for canonical, fast in ((True, True), (True, False), (False, True)):
        out = cover(ctx, k, n, [], canonical, fast)
        assert out.n_strings == 0 and out.n_bases == 0 and out.to_strings() == []
        one = ["ACGTTGCATGCA"]
        assert cover(ctx, k, n, one, canonical, fast).to_strings() == cover_oracle.cover(one, k, canonical, fast)
    # only K-long strings: distinct canonical k-mers, some of them adjacent
    g = synth.string_of_bases(synth.random_genome(400, 5))
    short = [g[i:i + k] for i in range(0, 300, 3)]
    short = cover_oracle.shuffled(short, seed=1)
    for fast in (True, False):
        assert cover(ctx, k, n, short, fast=fast).to_strings() == cover_oracle.cover(short, k, fast=fast)
    assert cover(ctx, k, n, short, canonical=False).to_strings() == cover_oracle.cover(short, k, canonical=False)
    # a single non-branching loop: one unitig, it stays one string
    km = synth.circular_with_tails(k, 80, 0, 1, 4)
    oset = check_all(ctx, k, n, 4, km)
    assert len(oset.unitigs()) == 1
    # even k, canonical, no palindromic end k-mers (the palindromes are taken out of the set)
    for k in (6, 8, 12):
        km = synth.random_read_kmers(k, min(3000, 4 ** k // 3), seed=k, canonical=True)
        km = km[km != synth.revcomp(km, k)]
        oset = ol.Set.from_kmers(k, min(10, 2 * k - 4), 4, km)
        u = cover_oracle.shuffled(oset.unitigs(), seed=k)
        got = cover(ctx, k, min(10, 2 * k - 4), u).to_strings()
        assert got == cover_oracle.oracle_capi_cover(u, k)
        assert cover(ctx, k, min(10, 2 * k - 4), oset.unitigs()).to_strings() == oset.spss()


# ------------------------------------------------------------------------------ 5. refusals
def test_cover_refusals(ctx):
    k, n = 9, 10
    oset = ol.Set.from_kmers(k, n, 4, read_shaped(k, 0, seed=2))
    u = oset.unitigs()

    def refused(strings, match, k=k, n=n, canonical=True):
        with pytest.raises(capi.KshError, match=match) as e:
            cover(ctx, k, n, strings, canonical=canonical)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT

    refused(u + [u[3]], "another string too")
    refused(u[:5] + [cover_oracle.revcomp_string(u[1])], "another string too")
    refused(u[:5] + ["AAAAAAAAAAAA"], "longer than K")
    refused(["AAAAATTTTT"], "longer than K")  # first k-mer = rc(last k-mer)
    refused(["ACGCGTAAC", "TTTTTTG"], "own reverse complement", k=6, n=8)
    refused(["TTTTTTG", "CAACGCGT"], "own reverse complement", k=6, n=8)
    refused(["ACGTACGTATT", "ACGTACGTACC"], "repeated first k-mer", canonical=False)
    refused(["TTACGTACGTA", "CCACGTACGTA"], "repeated last k-mer", canonical=False)
    # a string and its reverse complement are fine for the non-canonical cover (its rule is as-is)
    pair = ["ACGTTGCATGCAA", cover_oracle.revcomp_string("ACGTTGCATGCAA")]
    assert cover(ctx, k, n, pair, canonical=False).to_strings() == cover_oracle.cover(pair, k, canonical=False)
    # lens that do not add up to n_bases
    sp = capi.DeviceSpss.from_strings(capi.geom(k, n), u, ctx.device)
    bad = capi.DeviceSpss(sp.g, sp.words, sp.lens, sp.n_strings, sp.n_bases - 1)
    with pytest.raises(capi.KshError, match="add up"):
        ctx.spss_cover(bad)
    # and the context is still usable afterwards
    assert cover(ctx, k, n, u).to_strings() == oset.spss()


# ------------------------------------------------------------------------------ 6. identity at scale
def _same(a, b):
    assert a.n_strings == b.n_strings and a.n_bases == b.n_bases
    nw = (a.n_bases + 31) // 32
    assert bool((a.words[:nw] == b.words[:nw]).all())
    assert bool((a.lens[:a.n_strings] == b.lens[:b.n_strings]).all())


@pytest.mark.parametrize("geom,size", [((23, 14, 4), 100_000_000), ((31, 14, 8), 20_000_000)])
def test_cover_identity_at_scale(ctx, geom, size):
    """GetSPSSCanonical(set) = GetSPSSCanonical(GetUnitigsCanonical(set), ...) (spss.h:1835-1858), on the device."""
    import torch

    from kmersets import synth_torch

    k, n, _ = geom
    g = capi.geom(k, n)
    s = synth_torch.device_set(g, synth_torch.phylogeny_sets(k, 1, size, seed=k, device=ctx.device)[0])
    unitigs = ctx.spss_encode(s, mode=1)
    want = ctx.spss_encode(s, mode=0)
    got = ctx.spss_cover(unitigs)
    _same(got, want)
    assert ctx.spss_cover_stats()["unitigs"] == unitigs.n_strings
    del got, want, unitigs, s
    torch.cuda.empty_cache()


def test_cover_slow_identity(ctx):
    from kmersets import synth_torch

    for k, n in ((23, 14), (31, 14)):
        g = capi.geom(k, n)
        s = synth_torch.device_set(g, synth_torch.genome_with_tips(k, 1_000_000, k, ctx.device))
        unitigs = ctx.spss_encode(s, mode=1)
        _same(ctx.spss_cover(unitigs, fast=False), ctx.spss_encode(s, mode=2))
        _same(ctx.spss_cover(ctx.spss_encode(s, mode=1, canonical=False), canonical=False),
              ctx.spss_encode(s, mode=0, canonical=False))


# ------------------------------------------------------------------------------ 7. FASTA route
def test_cover_from_fasta(ctx):
    import torch

    k, n, kb = 23, 14, 4
    oset = ol.Set.from_kmers(k, n, kb, read_shaped(k, 2, seed=7))
    u = oset.unitigs()
    text = "".join(">u%d\n%s\n" % (i, s) for i, s in enumerate(u)).encode()
    t = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(ctx.device)
    frags = ctx.fasta_fragments(capi.geom(k, n), t)
    assert frags.to_strings() == u
    assert ctx.spss_cover(frags).to_strings() == oset.spss()


# ------------------------------------------------------------------------------ 8. plan interplay
def test_cover_and_encode_share_the_plan_slot(ctx):
    k, n, kb = 15, 14, 2
    km = read_shaped(k, 1, seed=11)
    oset = ol.Set.from_kmers(k, n, kb, km)
    d = capi.DeviceSet.from_kmers(capi.geom(k, n), km, ctx.device)
    u = capi.DeviceSpss.from_strings(capi.geom(k, n), oset.unitigs(), ctx.device)
    want = oset.spss()
    assert ctx.spss_cover(u).to_strings() == want
    assert ctx.spss_encode(d).to_strings() == want
    assert ctx.spss_cover(u).to_strings() == want
    assert ctx.spss_encode(d).to_strings() == want
    assert ctx.spss_cover(u).to_strings() == want
    # a write of the other kind is refused, not mis-served
    import ctypes as C

    assert capi.lib().ksh_spss_encode_write(ctx.h, None, None) == capi.KSH_FAILED_PRECONDITION
    ctx.spss_encode(d)
    assert capi.lib().ksh_spss_cover_write(ctx.h, None, None) == capi.KSH_FAILED_PRECONDITION
    st = (C.c_int64 * 4)()
    assert capi.lib().ksh_spss_cover_stats(ctx.h, st) == capi.KSH_FAILED_PRECONDITION

"""Sequence queries on a KmerSetSet index (ksh_seq_hits, capi.KssIndex.seq_hits): for every sequence and node, the
number of the sequence's k-mer positions whose k-mer is in Get(i) (lib/core/kmer_set_set.h:433-454), against the
oracle's Get(i) with a numpy sliding window, numpy closures of fabricated DAGs, torch.isin on device families, and
the column sums of KssIndex.query on the explicitly cut k-mers; passes, edges, refusals, and pending plans of the
context staying exact across the call."""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from kmersets import capi, synth, synth_torch

pytestmark = pytest.mark.gpu

ROUTES = (1, 2, 0)
CASES = [(9, 10, 1, 6, 3000, 11), (15, 14, 2, 8, 20000, 3), (23, 14, 4, 8, 30000, 5), (31, 14, 8, 4, 20000, 7)]
COMP = str.maketrans("ACGT", "TGCA")


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


# ---- recipes of tests/test_gpu_kss_index.py (copied: importing a test module would collect its tests twice) ----
def build_both(ctx, k, n, kb, n_sets, size, seed, max_iterations=-1):
    sets = synth.phylogeny_sets(k, n_sets, size, seed=seed)
    osets = [ol.Set.from_kmers(k, n, kb, s) for s in sets]
    ocompacts = [s.compact() for s in osets]
    ids = synth.sample_bucket_ids(n, seed=seed + 1)
    okss = ol.KmerSetSet(ocompacts, ids, max_iterations=max_iterations)
    g = capi.geom(k, n)
    dcompacts = [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocompacts]
    dkss = capi.DeviceKmerSetSet(ctx, dcompacts, ids, max_iterations=max_iterations)
    return sets, ocompacts, okss, dkss


def closure(n, children):
    anc = np.eye(n, dtype=bool)  # anc[j, i]: j reachable from i
    indeg = [0] * n
    for i in range(n):
        for c in children[i]:
            indeg[c] += 1
    order = [i for i in range(n) if indeg[i] == 0]
    for p in order:
        for c in children[p]:
            anc[c] |= anc[p]
            indeg[c] -= 1
            if indeg[c] == 0:
                order.append(c)
    return anc


def kmer_strings(kmers, k):
    return ["".join("ACGT"[(int(x) >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in kmers]


def fabricated(ctx, n_nodes, seed, k=15, n=10, per_node=12, empty_every=0):
    rng = np.random.default_rng(seed)
    g = capi.geom(k, n)
    pool = np.unique(synth.canonical(rng.integers(0, 1 << (2 * k), size=n_nodes * per_node, dtype=np.uint64), k))
    node_sets, comps = [], []
    for i in range(n_nodes):
        s = np.unique(rng.choice(pool, size=per_node)) if not (empty_every and i % empty_every == 0) else \
            np.zeros(0, dtype=np.uint64)
        node_sets.append(s.astype(np.uint64))
        comps.append(capi.DeviceSpss.from_strings(g, kmer_strings(s, k), ctx.device))
    children = [[] for _ in range(n_nodes)]
    for i in range(n_nodes - 1):
        for c in rng.choice(np.arange(i + 1, n_nodes), size=min(2, n_nodes - 1 - i), replace=False):
            children[i].append(int(c))
    return g, pool, node_sets, comps, children


def device_family(ctx, k, n, n_sets, size, seed):
    g = capi.geom(k, n)
    sets = synth_torch.phylogeny_sets(k, n_sets, size, seed, ctx.device)
    comps = [ctx.spss_encode(synth_torch.device_set(g, s), mode=0) for s in sets]
    return g, sets, comps


# ---- the numpy reference -------------------------------------------------------------------------------------
def cut(seqs, k):
    """(k-mers of all sequences as given, concatenated in order; the sequence of each; positions per sequence)."""
    parts = [synth.kmers_of_bases(synth.bases_of_string(s), k) for s in seqs]
    counts = np.array([p.size for p in parts], dtype=np.int64)
    kmers = np.concatenate(parts).astype(np.uint64) if parts else np.zeros(0, dtype=np.uint64)
    return kmers, np.repeat(np.arange(len(seqs)), counts), counts


def segment_sums(member, owner, n_seqs):
    """member[position, node] (bool) -> hits[sequence, node]."""
    out = np.zeros((n_seqs, member.shape[1]), dtype=np.int64)
    np.add.at(out, owner, member.astype(np.int64))
    return out


def expected_hits(gets, seqs, k, canonicalize):
    kmers, owner, counts = cut(seqs, k)
    q = synth.canonical(kmers, k).astype(np.uint64) if canonicalize else kmers
    member = np.stack([np.isin(q, s) for s in gets], axis=1)
    return segment_sums(member, owner, len(seqs)), counts


def revcomp_string(s):
    return s.translate(COMP)[::-1]


def case_sequences(ocompacts, k, seed):
    """Per input set the 20 longest and 5 shortest strings of its oracle SPSS; the reverse complement of every third
    of those; every second of them with one base changed every 2K bases from K/2 on; half as many random strings of
    K .. 199 bases.  Returns the sequences and (index of a string, index of its reverse complement) pairs."""
    rng = np.random.default_rng(seed)
    mem = []
    for c in ocompacts:
        strings = sorted(c.strings(), key=len)
        mem += strings[-20:] + strings[:5]
    rc = [revcomp_string(s) for s in mem[::3]]
    mut = []
    for s in mem[::2]:
        b = list(s)
        for j in range(k // 2, len(b), 2 * k):
            b[j] = "ACGT"[("ACGT".index(b[j]) + 1) % 4]
        mut.append("".join(b))
    n_rnd = (len(mem) + len(rc) + len(mut)) // 2
    rnd = ["".join("ACGT"[c] for c in rng.integers(0, 4, size=int(ln))) for ln in rng.integers(k, 200, size=n_rnd)]
    pairs = [(3 * j, len(mem) + j) for j in range(len(rc))]
    return mem + rc + mut + rnd, pairs


@pytest.fixture(scope="module")
def built(ctx):
    """case -> (structure, the oracle's Get(i) sets, the case's sequences on the host and on the device, the reverse
    complement pairs, the expected tables): made once per case, shared by the tests and left unchanged."""
    made = {}

    def get(case):
        if case not in made:
            k, n, kb, n_sets, size, seed = case
            sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
            gets = [okss.get(i).kmers() for i in range(okss.size())]
            seqs, pairs = case_sequences(ocompacts, k, seed)
            dseqs = capi.DeviceSpss.from_strings(capi.geom(k, n), seqs, ctx.device)
            want = {canon: expected_hits(gets, seqs, k, canon) for canon in (True, False)}
            made[case] = (dkss, gets, seqs, dseqs, pairs, want)
        return made[case]

    yield get
    for dkss, *_ in made.values():
        dkss.close()


@pytest.mark.parametrize("case", CASES)
def test_seq_hits_vs_oracle(ctx, built, case):
    """hits[s, i] == the number of positions of s whose k-mer the oracle's Get(i) holds, canonicalised or as given,
    on routes 1, 2 and auto; == the column sums of idx.query on the cut k-mers; a string and its reverse complement
    give equal rows when canonicalised."""
    k = case[0]
    dkss, gets, seqs, dseqs, pairs, want = built(case)
    idx = capi.KssIndex.from_kss(dkss)
    n_nodes = len(gets)
    assert idx.n_nodes == n_nodes
    # the expected table itself: a wrong answer cannot hide in an all-zero or all-full table
    table, counts = want[True]
    cells = float(table.size)
    zero, full = (table == 0).sum() / cells, (table == counts[:, None]).sum() / cells
    partial = ((table > 0) & (table < counts[:, None])).sum() / cells
    print("expected table: %.1f %% zero, %.1f %% partial, %.1f %% full" % (100 * zero, 100 * partial, 100 * full))
    assert zero >= 0.15 and partial >= 0.30 and full >= 0.02
    kmers, owner, _ = cut(seqs, k)
    for canon in (True, False):
        for route in ROUTES:
            got = idx.seq_hits(dseqs, canonicalize=canon, route=route)
            assert got.dtype == np.uint32 and got.shape == (len(seqs), n_nodes)
            assert np.array_equal(got.astype(np.int64), want[canon][0]), (canon, route)
            bits = idx.routes()
            assert bits & (capi.QROUTE_SEARCH if route == 1 else capi.QROUTE_JOIN if route == 2 else 3)
            assert not bits & capi.QROUTE_SEQ_PASSES
            if canon:
                a, b = zip(*pairs)
                assert np.array_equal(got[list(a)], got[list(b)])
        rows = idx.query(kmers, canonicalize=canon, route=0)
        assert np.array_equal(segment_sums(rows, owner, len(seqs)), want[canon][0]), canon
    # a list of str is uploaded by the call; a device result holds the same counts
    few = seqs[:7]
    assert np.array_equal(idx.seq_hits(few), want[True][0][:7].astype(np.uint32))
    dev = idx.seq_hits(dseqs, device=True)
    assert dev.device.type == "cuda" and np.array_equal(dev.cpu().numpy().view(np.uint32).astype(np.int64), table)
    idx.close()


@pytest.mark.parametrize("pass_positions", [1, 7, 4096])
def test_passes(ctx, built, pass_positions):
    """Passes of 1, 7 and 4096 positions against sequences of up to about 3 * 10^4 bases: the same table as the
    default pass gives, and the route bits say that there were several passes.  (Passes of 4096 on the join too; a
    pass of the join costs a dozen launches and a synchronisation, so the tiny ones run on the search only.)"""
    dkss, gets, seqs, dseqs, pairs, want = built(CASES[2])
    assert max(len(s) for s in seqs) > 4 * 4096
    idx = capi.KssIndex.from_kss(dkss)
    one = idx.seq_hits(dseqs, pass_positions=0)
    assert np.array_equal(one.astype(np.int64), want[True][0])
    assert not idx.routes() & capi.QROUTE_SEQ_PASSES
    for route in ((0, 1, 2) if pass_positions == 4096 else (0,)):
        got = idx.seq_hits(dseqs, pass_positions=pass_positions, route=route)
        assert np.array_equal(got, one), route
        assert idx.routes() & capi.QROUTE_SEQ_PASSES
    idx.close()


@pytest.mark.parametrize("n_nodes", [150, 700])
def test_edges(ctx, n_nodes):
    """W = 3 and 11 words per row on fabricated DAGs, against a numpy closure: strings of exactly K bases, 33 of them
    in a row (their starts fall on every 2-bit offset of a word), one string of 5 * 10^4 bases, the empty batch, and
    two adjacent strings whose straddling window is a member k-mer."""
    k = 15
    g, pool, node_sets, comps, children = fabricated(ctx, n_nodes, n_nodes, k=k, empty_every=37)
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    anc = closure(n_nodes, children)
    rng = np.random.default_rng(2)
    rnd = rng.integers(0, 1 << (2 * k), size=40, dtype=np.uint64)
    short = kmer_strings(np.concatenate([pool[:26], rnd[:7]]), k)  # 33 strings of K bases: starts at 15 j mod 32
    assert len(short) == 33 and {(15 * j) % 32 for j in range(33)} == set(range(32))
    picks = pool[rng.integers(0, pool.size, size=50000 // k + 1)]  # members back to back (some twice), random joints
    long = "".join(kmer_strings(picks, k))[:50000]
    m = kmer_strings(node_sets[1][:1], k)[0]  # a member, cut in two: the window across A | B spells it
    a = "".join("ACGT"[c] for c in rng.integers(0, 4, size=k)) + m[:7]
    b = m[7:] + "".join("ACGT"[c] for c in rng.integers(0, 4, size=k))
    seqs = short + [long] + kmer_strings(rnd[7:], k) + [a, b, a + b] + short
    ia = len(short) + 1 + 33
    assert seqs[ia] == a and seqs[ia + 2] == a + b

    kmers, owner, counts = cut(seqs, k)
    direct = np.stack([np.isin(kmers, s) for s in node_sets], axis=1)  # [position, j]
    member = (direct.astype(np.float32) @ anc.astype(np.float32)) > 0   # OR over j of anc[j] (sums <= 700: exact)
    want = segment_sums(member, owner, len(seqs))
    # the straddling window is a member somewhere: joined, A + B has more hits than A and B apart
    assert (want[ia + 2] - want[ia] - want[ia + 1]).max() >= 1
    assert want[len(short)].max() > 20 and counts[len(short)] == 50000 - k + 1
    dseqs = capi.DeviceSpss.from_strings(g, seqs, ctx.device)
    for route in ROUTES:
        for pass_positions in (0, 1000):
            got = idx.seq_hits(dseqs, canonicalize=False, route=route, pass_positions=pass_positions)
            assert np.array_equal(got.astype(np.int64), want), (route, pass_positions)
    empty = idx.seq_hits([])
    assert empty.shape == (0, n_nodes) and empty.dtype == np.uint32
    assert idx.seq_hits(capi.DeviceSpss.from_strings(g, [], ctx.device), route=2).shape == (0, n_nodes)
    idx.close()


def test_all_nodes_empty(ctx):
    g, pool, node_sets, comps, children = fabricated(ctx, 4, 5)
    empty = [capi.DeviceSpss.from_strings(g, [], ctx.device) for _ in range(3)]
    idx = capi.KssIndex.from_nodes(ctx, empty, [[1], [2], []])
    seqs = kmer_strings(pool[:20], g.k) + ["".join(kmer_strings(pool[:40], g.k))]
    for route in ROUTES:
        got = idx.seq_hits(seqs, route=route)
        assert got.shape == (21, 3) and not got.any()
    idx.close()


def test_wide_buckets(ctx):
    """(23, 18, 4): 2^18 buckets, 3 sets of 2 * 10^5 k-mers made on the device, 2000 sequences, against torch.isin."""
    k, n = 23, 18
    g, sets, comps = device_family(ctx, k, n, 3, 200000, 22)
    children = [[2], [2], []]
    idx = capi.KssIndex.from_nodes(ctx, comps, children)
    rng = np.random.default_rng(3)
    seqs = []
    for c in comps:
        seqs += [s[:300] for s in c.to_strings()[:400]]
    seqs += ["".join("ACGT"[c] for c in rng.integers(0, 4, size=int(ln)))
             for ln in rng.integers(k, 200, size=2000 - len(seqs))]
    assert len(seqs) == 2000
    kmers, owner, counts = cut(seqs, k)
    q = torch.from_numpy(kmers.view(np.int64)).to(ctx.device)
    qc = torch.minimum(q, synth_torch.revcomp(q, k))
    anc = torch.from_numpy(closure(3, children)).to(ctx.device)
    direct = torch.stack([torch.isin(qc, s) for s in sets], dim=1)
    member = (direct.to(torch.float32) @ anc.to(torch.float32)) > 0
    want = torch.zeros((len(seqs), 3), dtype=torch.int64, device=ctx.device)
    want.index_add_(0, torch.from_numpy(owner).to(ctx.device), member.to(torch.int64))
    want = want.cpu().numpy()
    assert (want > 0).any() and (want == 0).any()
    dseqs = capi.DeviceSpss.from_strings(g, seqs, ctx.device)
    for route in ROUTES:
        assert np.array_equal(idx.seq_hits(dseqs, route=route).astype(np.int64), want), route
        assert not idx.routes() & capi.QROUTE_OVERSIZE
    idx.close()


def test_refusals(ctx):
    """n_bases off by one and a length of UINT32_MAX are KSH_INVALID_ARGUMENT, a borrowed index whose structure is
    closed is KSH_FAILED_PRECONDITION; after each refusal the context still serves a correct call."""
    k, n = 15, 14
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, 2, 3, 5000, 13)
    gets = [okss.get(i).kmers() for i in range(okss.size())]
    seqs = sorted(ocompacts[0].strings(), key=len)[-10:] + kmer_strings(sets[1][:10], k)
    want = expected_hits(gets, seqs, k, True)[0]
    g = capi.geom(k, n)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(okss.size())]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(okss.size())])
    idx = capi.KssIndex.from_kss(dkss)
    dseqs = capi.DeviceSpss.from_strings(g, seqs, ctx.device)
    assert np.array_equal(idx.seq_hits(dseqs).astype(np.int64), want)

    for delta in (1, -1):
        bad = capi.DeviceSpss(g, dseqs.words, dseqs.lens, dseqs.n_strings, dseqs.n_bases + delta)
        with pytest.raises(capi.KshError) as e:
            idx.seq_hits(bad)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and "n_bases" in str(e.value)
        assert np.array_equal(idx.seq_hits(dseqs, route=2).astype(np.int64), want)
    lens = dseqs.lens.clone()
    lens[3] = -1  # UINT32_MAX
    with pytest.raises(capi.KshError) as e:
        idx.seq_hits(capi.DeviceSpss(g, dseqs.words, lens, dseqs.n_strings, dseqs.n_bases))
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "lens[3]" in str(e.value)
    assert np.array_equal(owned.seq_hits(dseqs).astype(np.int64), want)
    with pytest.raises(capi.KshError) as e:
        idx.seq_hits(dseqs, route=3)
    assert e.value.code == capi.KSH_INVALID_ARGUMENT

    dkss.close()
    with pytest.raises(capi.KshError) as e:
        idx.seq_hits(dseqs)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION
    assert idx.h is None
    for route in ROUTES:  # the index that owns its sets goes on serving
        assert np.array_equal(owned.seq_hits(dseqs, route=route).astype(np.int64), want)
    owned.close()


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, ksh_seq_hits on a structure of the same context (on the join, which
    resets the arena, in several passes, and on the search), then the write: served, and equal to a fresh plan +
    write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca, cb = ctx.spss_encode(a, mode=0), ctx.spss_encode(b, mode=0)
    idx = capi.KssIndex.from_nodes(ctx, [ca, cb], [[1], []])
    seqs = sorted(ca.to_strings(), key=len)[-30:] + sorted(cb.to_strings(), key=len)[-30:]
    dseqs = capi.DeviceSpss.from_strings(g, seqs, ctx.device)
    both = np.union1d(sets[0], sets[1]).astype(np.uint64)
    want = expected_hits([both, np.asarray(sets[1], dtype=np.uint64)], seqs, k, True)[0]

    def intrude():
        assert np.array_equal(idx.seq_hits(dseqs, route=2, pass_positions=1000).astype(np.int64), want)
        assert np.array_equal(idx.seq_hits(dseqs, route=1).astype(np.int64), want)

    intrude()
    # pair
    fresh = [s.kmers() for s in ctx.pair_algebra(a, b)]
    outs = [capi.DeviceSet.empty_like_offsets(g, 0, ctx.device) for _ in range(3)]
    totals = ctx.pair_plan(a, b, *outs)
    for o, t in zip(outs, totals):
        o.n_keys = t
        o.keys = torch.empty(max(t * g.key_bytes, 16), dtype=torch.uint8, device=ctx.device)
    intrude()
    ctx.pair_write(a, b, *outs)
    assert all(np.array_equal(o.kmers(), f) for o, f in zip(outs, fresh))
    # decode
    fresh = ctx.spss_decode(ca).kmers()
    plan = ctx.spss_decode_plan(ca)
    intrude()
    assert np.array_equal(ctx.spss_decode_write(plan).kmers(), fresh) and np.array_equal(fresh, np.sort(sets[0]))
    # encode
    fresh = ctx.spss_encode(a, mode=0).to_strings()
    plan = ctx.spss_encode_plan(a, mode=0)
    intrude()
    assert ctx.spss_encode_write(plan).to_strings() == fresh
    # text
    text = ctx.spss_to_text(ca)
    fresh = ctx.spss_from_text(g, text).to_strings()
    plan = ctx.spss_from_text_plan(g, text)
    intrude()
    assert ctx.spss_from_text_write(plan).to_strings() == fresh == ca.to_strings()
    idx.close()

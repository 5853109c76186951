"""ksh_spss_links (capi.Context.spss_links) against the host reference of tests/spss_links_reference.py on the designed
inputs of tests/spss_links_cases.py, in every mode a case is legal for: offsets and targets, the write guard behind both
outputs, count-only / exact capacity / too small a capacity, the call repeated, every device-side refusal with the
outputs untouched and the context still serving, and pending plans of every group staying exact across a call.  Every
comparison is array or string equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import spss_links_cases as lc
import spss_links_reference as ref
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
GUARD = 64
MODAL = [(c, m) for c in lc.CASES for m in c["modes"]]
MODAL_IDS = ["%s-%s" % (c["id"], "canonical" if m else "directed") for c, m in MODAL]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """The reference's answer per case and mode, computed once; it has something to show."""
    out = {(c["id"], m): ref.links(c["strings"], c["k"], m) for c, m in MODAL}
    assert sum(to.size > 0 for _, to in out.values()) * 2 > len(out)
    return out


def geom_of(k):
    return capi.geom(k, 10 if k > 5 else 4)


def upload(ctx, strings, k):
    return capi.DeviceSpss.from_strings(geom_of(k), strings, ctx.device)


def prefilled(ctx, n_strings, n_links):
    return (torch.full((2 * n_strings + 1 + GUARD,), PATTERN, dtype=torch.int64, device=ctx.device),
            torch.full((n_links + GUARD,), PATTERN, dtype=torch.int64, device=ctx.device))


@pytest.mark.parametrize("case,canonical", MODAL, ids=MODAL_IDS)
def test_links_vs_reference(ctx, want, case, canonical):
    want_off, want_to = want[(case["id"], canonical)]
    n, n_links = len(case["strings"]), int(want_to.size)
    seqs = upload(ctx, case["strings"], case["k"])
    off, to = ctx.spss_links(seqs, canonical=canonical)
    assert off.dtype == to.dtype == torch.int64 and off.is_cuda and to.is_cuda
    assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(to.cpu().numpy(), want_to)
    # count only: the offsets whole, the targets not asked for
    g_off, g_to = prefilled(ctx, n, n_links)
    rc, got = ctx.spss_links_raw(seqs, canonical, 0, g_off)
    assert rc == capi.KSH_OK and got == n_links
    assert np.array_equal(g_off[:2 * n + 1].cpu().numpy(), want_off) and bool((g_off[2 * n + 1:] == PATTERN).all())
    rc, got = ctx.spss_links_raw(seqs, canonical, 0)  # (no offsets either)
    assert rc == capi.KSH_OK and got == n_links
    # the exact capacity, and the guard behind both outputs
    if n_links:
        g_off, g_to = prefilled(ctx, n, n_links)
        rc, got = ctx.spss_links_raw(seqs, canonical, n_links, g_off, g_to)
        assert rc == capi.KSH_OK and got == n_links
        assert bool((g_off[2 * n + 1:] == PATTERN).all()) and bool((g_to[n_links:] == PATTERN).all())
        assert np.array_equal(g_off[:2 * n + 1].cpu().numpy(), want_off)
        assert np.array_equal(g_to[:n_links].cpu().numpy(), want_to)
        again_off, again_to = prefilled(ctx, n, n_links)  # the call made twice
        assert ctx.spss_links_raw(seqs, canonical, n_links, again_off, again_to) == (capi.KSH_OK, n_links)
        assert torch.equal(again_off, g_off) and torch.equal(again_to, g_to)
        r_off, r_to = prefilled(ctx, n, n_links)  # more room than needed: the same, nothing behind n_links
        assert ctx.spss_links_raw(seqs, canonical, n_links + 7, r_off, r_to[:n_links + 7]) == (capi.KSH_OK, n_links)
        assert torch.equal(r_off, g_off) and torch.equal(r_to, g_to)
    # too small a capacity: the true number, and nothing written
    if n_links > 1:
        g_off, g_to = prefilled(ctx, n, n_links)
        rc, got = ctx.spss_links_raw(seqs, canonical, n_links - 1, None, g_to)
        message = capi.lib().ksh_last_error().decode()
        assert rc == capi.KSH_FAILED_PRECONDITION and got == n_links
        assert "capacity = %d" % (n_links - 1) in message and "n_links = %d" % n_links in message
        assert bool((g_to == PATTERN).all())
        rc, got = ctx.spss_links_raw(seqs, canonical, 1, g_off, g_to)
        assert rc == capi.KSH_FAILED_PRECONDITION and got == n_links and bool((g_to == PATTERN).all())
        assert bool((g_off[2 * n + 1:] == PATTERN).all())


def test_device_refusals_touch_nothing(ctx):
    k = 23
    strings = lc.search(lambda s: lc.chain(k, [50, 1, 40, 30, 1, 60], [0, 1, 0, 1, 0, 0], s, gaps=(3,)), k,
                        (True, False), 77)
    n = len(strings)
    want = {m: ref.links(strings, k, m) for m in (True, False)}
    assert want[True][1].size > 4 and want[False][1].size > 0
    seqs = upload(ctx, strings, k)
    # (30 bases that repeat no k-mer of the container when they follow string 1's k-mer: the first such seed)
    tails = (synth.string_of_bases(synth.random_genome(30, s)) for s in range(78, 98))
    tail = next(t for t in tails if lc.legal(strings[:4] + [ref.rc(strings[1][:k]) + t] + strings[5:], k, False))

    def serves():
        for m in (True, False):
            off, to = ctx.spss_links(seqs, canonical=m)
            assert np.array_equal(off.cpu().numpy(), want[m][0]) and np.array_equal(to.cpu().numpy(), want[m][1])

    def refused(bad, canonical, word, size):
        g_off, g_to = prefilled(ctx, n, size)
        rc, _ = ctx_raw(ctx, bad, canonical, size, g_off, g_to)
        message = capi.lib().ksh_last_error().decode()
        assert rc == capi.KSH_INVALID_ARGUMENT and word in message, (word, rc, message)
        assert bool((g_off == PATTERN).all()) and bool((g_to == PATTERN).all()), word
        serves()

    def with_string(at, text):
        edited = list(strings)
        edited[at] = text
        return edited

    serves()
    # an end shared by two strings: string 4 begins with the reverse complement of string 1's first k-mer (one
    # canonical k-mer, two k-mers as written), or with that k-mer itself
    twin = with_string(4, ref.rc(strings[1][:k]) + tail)
    assert lc.legal(twin, k, False) and not lc.legal(twin, k, True)
    refused(upload(ctx, twin, k), True, "string 1 ", 16)
    off, to = ctx.spss_links(upload(ctx, twin, k), canonical=False)  # (as written they are distinct: served)
    assert np.array_equal(to.cpu().numpy(), ref.links(twin, k, False)[1])
    assert np.array_equal(off.cpu().numpy(), ref.links(twin, k, False)[0])
    same = with_string(4, strings[1][:k] + tail)
    for m in (True, False):
        refused(upload(ctx, same, k), m, "string 1 ", 16)
    # a long string whose first and last k-mer coincide
    ring = with_string(2, strings[2][:k] + tail + strings[2][:k])
    for m in (True, False):
        refused(upload(ctx, ring, k), m, "string 2 ", 16)
    flipped = with_string(2, strings[2][:k] + tail + ref.rc(strings[2][:k]))  # ... after canonicalisation only
    refused(upload(ctx, flipped, k), True, "string 2 ", 16)
    # the container's own sizes
    bad_lens = seqs.lens.clone()
    bad_lens[3] = -1  # UINT32_MAX
    for m in (True, False):
        refused(capi.DeviceSpss(seqs.g, seqs.words, bad_lens, n, seqs.n_bases), m, "lens[3]", 16)
        refused(capi.DeviceSpss(seqs.g, seqs.words, seqs.lens, n, seqs.n_bases + 1), m, "n_bases", 16)
        refused(capi.DeviceSpss(seqs.g, seqs.words, seqs.lens, n, seqs.n_bases - 1), m, "n_bases", 0)
    # K = 4, canonical: the end ACGT is its own reverse complement; as written the container is served
    small = ["AACCG", "ACGTA", "GGAT"]
    assert lc.legal(small, 4, False) and not lc.legal(small, 4, True)
    d_small = upload(ctx, small, 4)
    g_off, g_to = prefilled(ctx, 3, 8)
    rc, _ = ctx_raw(ctx, d_small, True, 8, g_off, g_to)
    message = capi.lib().ksh_last_error().decode()
    assert rc == capi.KSH_INVALID_ARGUMENT and "string 1 " in message and "reverse complement" in message
    assert bool((g_off == PATTERN).all()) and bool((g_to == PATTERN).all())
    off, to = ctx.spss_links(d_small, canonical=False)
    assert np.array_equal(off.cpu().numpy(), ref.links(small, 4, False)[0])
    assert np.array_equal(to.cpu().numpy(), ref.links(small, 4, False)[1])
    serves()


def ctx_raw(ctx, seqs, canonical, capacity, off, to):
    """ksh_spss_links with every return code handed back."""
    view, n = seqs.view(), C.c_int64(-7)
    with torch.cuda.stream(ctx.stream):
        rc = capi.lib().ksh_spss_links(C.byref(view), ctx.h, C.byref(seqs.g), int(canonical), capacity, off.data_ptr(),
                                       to.data_ptr() if capacity else None, C.byref(n))
    return rc, n.value


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, a links call on the same context, then the write: served, and equal to a
    fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca = ctx.spss_encode(a, mode=0)
    uncut = ca.to_strings()
    # the unitigs of the union of the two sets: they branch where the sets differ
    both = capi.DeviceSet.from_kmers(g, np.union1d(sets[0], sets[1]), ctx.device)
    cu = ctx.spss_encode(both, mode=1)
    want_off, want_to = ref.links(cu.to_strings(), k, True)
    assert want_to.size > 0 and ref.twin_symmetric(want_off, want_to)

    def intrude():
        off, to = ctx.spss_links(cu)
        assert np.array_equal(off.cpu().numpy(), want_off) and np.array_equal(to.cpu().numpy(), want_to)

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
    assert ctx.spss_from_text_write(plan).to_strings() == fresh == uncut

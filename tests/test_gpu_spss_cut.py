"""ksh_spss_cut (capi.Context.spss_cut) against the string-slicing reference of tests/spss_cut_reference.py on the
designed inputs of tests/spss_cut_cases.py, the write guard behind both outputs, every device-side refusal with the
outputs untouched and the context still serving, and pending plans of every group staying exact across a cut.  Every
comparison is array or string equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import spss_cut_cases as cc
from spss_cut_reference import cut
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

U = np.uint64
PATTERN = 0x5A5A5A5A
GUARD = 64


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """The reference's answer per case, computed once.  Before any comparison: where a case says it cuts, the
    reference has more output strings than input strings, and where it says a piece is long, a string longer than K --
    and most cases say both."""
    out = {}
    both = 0
    for case in cc.CASES:
        strings, lens, n_out = cut(case["strings"], case["k"], case["offsets"], case["start"])
        if cc.HAS_CUT in case["covers"]:
            assert len(strings) > len(case["strings"]), case["id"]
        if cc.HAS_LONG_PIECE in case["covers"]:
            assert max(len(s) for s in strings) > case["k"], case["id"]
        both += cc.HAS_CUT in case["covers"] and cc.HAS_LONG_PIECE in case["covers"]
        out[case["id"]] = (strings, lens, n_out)
    assert 2 * both > len(cc.CASES)
    return out


def upload(ctx, case):
    g = capi.geom(case["k"], 10 if case["k"] > 5 else 4)
    seqs = capi.DeviceSpss.from_strings(g, case["strings"], ctx.device)
    off = torch.from_numpy(case["offsets"].copy()).to(ctx.device)
    start = torch.from_numpy(case["start"].copy()).to(ctx.device)
    return seqs, off, start


def masked_words(words, n_bases):
    """The first ceil(n_bases / 32) words as uint64, the bits behind the last base cleared."""
    n_words = (n_bases + 31) // 32
    w = words[:n_words].cpu().numpy().view(U).copy()
    if n_bases % 32:
        w[-1] &= ~U(0) << U(64 - 2 * (n_bases % 32))
    return w


@pytest.mark.parametrize("case", cc.CASES, ids=[c["id"] for c in cc.CASES])
def test_cut_vs_reference(ctx, want, case):
    strings, lens, n_out = want[case["id"]]
    seqs, off, start = upload(ctx, case)
    got = ctx.spss_cut(seqs, off, start)
    assert got.n_strings == len(strings) and got.n_bases == n_out
    assert np.array_equal(got.lens[:got.n_strings].cpu().numpy().view(np.uint32), lens)
    assert got.to_strings() == strings
    assert np.array_equal(masked_words(got.words, n_out), synth.pack_strings(strings, case["k"])[0])
    if cc.NO_CUT in case["covers"]:  # nothing moves: the stream is the input's
        assert np.array_equal(masked_words(got.words, n_out), masked_words(seqs.words, seqs.n_bases))
    again = ctx.spss_cut(seqs, off, start.view(torch.uint32) if start.numel() else start)  # (uint32 starts as well)
    assert torch.equal(again.words[:(n_out + 31) // 32], got.words[:(n_out + 31) // 32])


def raw_cut(ctx, seqs, off, start, n_runs, words, lens):
    view, n = seqs.view(), C.c_int64(-7)
    with torch.cuda.stream(ctx.stream):
        rc = capi.lib().ksh_spss_cut(C.byref(view), ctx.h, C.byref(seqs.g), off.data_ptr(), start.data_ptr(), n_runs,
                                     words.data_ptr(), lens.data_ptr(), C.byref(n))
    return rc, n.value


def prefilled(ctx, n_words, n_runs):
    return (torch.full((n_words + GUARD,), PATTERN, dtype=torch.int64, device=ctx.device),
            torch.full((n_runs + GUARD,), PATTERN, dtype=torch.int32, device=ctx.device))


@pytest.mark.parametrize("which", ["one_long-k4", "every_position-k4", "stream_edge+0-k16", "stream_edge+1-k23",
                                   "stream_edge-1-k31", "random_p0.5-k9", "single-k31"])
def test_write_guard(ctx, want, which):
    case = next(c for c in cc.CASES if c["id"] == which)
    strings, lens_want, n_out = want[which]
    seqs, off, start = upload(ctx, case)
    n_words, n_runs = (n_out + 31) // 32, len(strings)
    words, lens = prefilled(ctx, n_words, n_runs)
    rc, n = raw_cut(ctx, seqs, off, start, n_runs, words, lens)
    assert rc == capi.KSH_OK and n == n_out
    assert bool((words[n_words:] == PATTERN).all()) and bool((lens[n_runs:] == PATTERN).all())
    assert np.array_equal(masked_words(words, n_out), synth.pack_strings(strings, case["k"])[0])
    assert np.array_equal(lens[:n_runs].cpu().numpy().view(np.uint32), lens_want)


def test_device_refusals_touch_nothing(ctx):
    k = 23
    sizes = [50, 1, 40, 30, 1, 60]
    case = cc.make_case("refusals", k, sizes, [[10, 20, 30], [], [5], [7, 9, 11], [], [1]], [cc.HAS_CUT], 911)
    strings, lens_want, n_out = cut(case["strings"], k, case["offsets"], case["start"])
    assert len(strings) > len(sizes) and max(len(s) for s in strings) > k
    seqs, off, start = upload(ctx, case)
    n, n_runs, n_words = len(sizes), len(strings), (n_out + 31) // 32
    o = case["offsets"]

    def edited(t, at, value):
        t = t.clone()
        t[at] = value
        return t

    bad_lens = edited(seqs.lens, 3, -1)  # UINT32_MAX
    malformed = [
        (seqs, edited(off, 0, 1), start, "d_run_offsets[0]"),
        (seqs, edited(off, n, n_runs + 1), start, "d_run_offsets[%d]" % n),
        (seqs, edited(off, n, n_runs - 1), start, "d_run_offsets[%d]" % n),
        (seqs, edited(off, 2, int(o[1])), start, "string 1 has no run"),
        (seqs, edited(off, 3, int(o[4]) + 1), start, "string 3 has no run"),  # (descending)
        (seqs, off, edited(start, int(o[3]), 1), "string 3 does not start at position 0"),
        (seqs, off, edited(start, int(o[3]) + 2, 7), "d_run_start[%d] is not above" % (int(o[3]) + 2)),
        (seqs, off, edited(start, int(o[0]) + 2, 5), "d_run_start[%d] is not above" % (int(o[0]) + 2)),  # (descending)
        (seqs, off, edited(start, int(o[3]) - 1, sizes[2]), "d_run_start[%d] is beyond" % (int(o[3]) - 1)),
        (seqs, off, edited(start, n_runs - 1, 2 ** 31 - 1), "d_run_start[%d] is beyond" % (n_runs - 1)),
        (capi.DeviceSpss(seqs.g, seqs.words, bad_lens, n, seqs.n_bases), off, start, "lens[3]"),
        (capi.DeviceSpss(seqs.g, seqs.words, seqs.lens, n, seqs.n_bases + 1), off, start, "n_bases"),
        (capi.DeviceSpss(seqs.g, seqs.words, seqs.lens, n, seqs.n_bases - 1), off, start, "n_bases"),
    ]
    for bad_seqs, bad_off, bad_start, word in malformed:
        words, lens = prefilled(ctx, n_words, n_runs)
        rc, _ = raw_cut(ctx, bad_seqs, bad_off, bad_start, n_runs, words, lens)
        message = capi.lib().ksh_last_error().decode()
        assert rc == capi.KSH_INVALID_ARGUMENT and word in message, (word, rc, message)
        assert bool((words == PATTERN).all()) and bool((lens == PATTERN).all()), word
        assert ctx.spss_cut(seqs, off, start).to_strings() == strings  # still serving
    with pytest.raises(capi.KshError) as e:  # fewer runs than strings: refused on the host
        ctx.spss_cut(seqs, off, start[:n - 1])
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "n_runs" in str(e.value)
    assert ctx.spss_cut(seqs, off, start).to_strings() == strings


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, a cut on the same context, then the write: served, and equal to a fresh
    plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca = ctx.spss_encode(a, mode=0)
    uncut = ca.to_strings()
    rng = np.random.default_rng(18)
    sizes = [len(s) - k + 1 for s in uncut]
    starts = [[0] + [int(x) for x in 1 + np.flatnonzero(rng.random(p - 1) < 0.05)] for p in sizes]
    off_h = np.concatenate([[0], np.cumsum([len(x) for x in starts])]).astype(np.int64)
    start_h = np.array([x for row in starts for x in row], dtype=np.int32)
    want, _, _ = cut(uncut, k, off_h, start_h)
    assert len(want) > len(uncut) and max(len(s) for s in want) > k
    off, start = torch.from_numpy(off_h).to(ctx.device), torch.from_numpy(start_h).to(ctx.device)

    def intrude():
        assert ctx.spss_cut(ca, off, start).to_strings() == want

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
    # the cut strings hold the same set
    assert np.array_equal(ctx.spss_decode(ctx.spss_cut(ca, off, start)).kmers(), np.sort(sets[0]))

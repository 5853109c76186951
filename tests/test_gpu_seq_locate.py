"""ksh_seq_locate (capi.Context.seq_locate) against the host reference of tests/seq_locate_reference.py on the designed
containers of tests/seq_locate_cases.py in both modes: both outputs with a write guard of 64 elements behind each, the
call made twice, every device-side refusal with the outputs untouched and the context still serving, and every plan /
write pair of the plan protocol staying exact across the call and across a refused call, on the victim's context and
on a second one.  Every comparison is array equality."""
import numpy as np
import pytest
import torch

import plan_protocol_cases as protocol
import seq_locate_cases as cases
import seq_locate_reference as ref
import test_gpu_plan_protocol as pp
from kmersets import capi

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN_WHERE, PATTERN_COUNT = 0x5A5A5A5A5A5A, 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """The reference's answer per case and mode, computed once."""
    return {(c["id"], m): ref.locate(c["strings"], c["reference"], c["k"], m) for c in cases.CASES
            for m in (True, False)}


def prefilled(ctx, n):
    with torch.cuda.stream(ctx.stream):
        return (torch.full((2 * n + GUARD,), PATTERN_WHERE, dtype=torch.int64, device=ctx.device),
                torch.full((2 * n + GUARD,), PATTERN_COUNT, dtype=torch.int32, device=ctx.device))


def untouched(bufs):
    return bool((bufs[0] == PATTERN_WHERE).all()) and bool((bufs[1] == PATTERN_COUNT).all())


def equal_to(bufs, answer):
    where, count = bufs[0].cpu().numpy(), bufs[1].cpu().numpy().view(np.uint32)
    m = answer[0].size
    return (np.array_equal(where[:m], answer[0]) and np.array_equal(count[:m], answer[1])
            and bool((where[m:] == PATTERN_WHERE).all()) and bool((count[m:] == PATTERN_COUNT).all()))


def geom_of(k):
    return capi.geom(k, 14)


@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "directed"])
@pytest.mark.parametrize("case", cases.CASES, ids=[c["id"] for c in cases.CASES])
def test_locate_vs_reference(ctx, want, case, canonical):
    answer = want[(case["id"], canonical)]
    g = geom_of(case["k"])
    strings = capi.DeviceSpss.from_strings(g, case["strings"], ctx.device)
    reference = capi.DeviceSpss.from_strings(g, case["reference"], ctx.device)
    n = len(case["strings"])
    located = int((answer[1] > 0).sum())
    bufs = prefilled(ctx, n)
    assert ctx.seq_locate_raw(strings, reference, canonical, *bufs) == (capi.KSH_OK, located)
    assert equal_to(bufs, answer), case["edge"]
    again = prefilled(ctx, n)  # the call made twice
    assert ctx.seq_locate_raw(strings, reference, canonical, *again) == (capi.KSH_OK, located)
    assert torch.equal(again[0], bufs[0]) and torch.equal(again[1], bufs[1])
    assert ctx.seq_locate_raw(strings, reference, canonical, *again, want_located=False)[0] == capi.KSH_OK
    assert equal_to(again, answer)
    # the wrapper
    where, count = ctx.seq_locate(strings, reference, canonical=canonical)
    assert where.dtype == torch.int64 and count.dtype == torch.uint32 and where.is_cuda and count.is_cuda
    assert where.shape == count.shape == (2 * n,)
    assert np.array_equal(where.cpu().numpy(), answer[0]) and np.array_equal(count.cpu().numpy(), answer[1])


def overdeclared(ctx, g, strings, extra):
    """A view that declares `extra` bases more than its strings hold; the words are there (zero) for the declared
    count, so whatever reads by n_bases stays inside the buffer."""
    sp = capi.DeviceSpss.from_strings(g, strings, ctx.device)
    with torch.cuda.stream(ctx.stream):
        w = torch.zeros((sp.n_bases + extra + 31) // 32 + 1, dtype=torch.int64, device=ctx.device)
        w[: sp.words.numel()] = sp.words
    return capi.DeviceSpss(g, w, sp.lens, sp.n_strings, sp.n_bases + extra)


def with_huge_lens(ctx, sp, at):
    with torch.cuda.stream(ctx.stream):
        lens = sp.lens.clone()
        lens[at] = -1  # UINT32_MAX
    return capi.DeviceSpss(sp.g, sp.words, lens, sp.n_strings, sp.n_bases)


def test_device_refusals_touch_nothing(ctx):
    case = next(c for c in cases.CASES if c["id"] == "duplicate-ends-k23")
    k, g = 23, geom_of(23)
    answer = ref.locate(case["strings"], case["reference"], k, True)
    n = len(case["strings"])
    strings = capi.DeviceSpss.from_strings(g, case["strings"], ctx.device)
    reference = capi.DeviceSpss.from_strings(g, case["reference"], ctx.device)
    lens = lambda c: [len(t) - k for t in c]  # noqa: E731

    def serves():
        bufs = prefilled(ctx, n)
        assert ctx.seq_locate_raw(strings, reference, True, *bufs)[0] == capi.KSH_OK
        assert equal_to(bufs, answer)

    def refused(word, s=strings, r=reference, s_lens=None, r_lens=None):
        with pytest.raises(ValueError) as host:  # the reference refuses it too, in the same words
            ref.check_request(lens(case["strings"]) if s_lens is None else s_lens, s.n_bases,
                              lens(case["reference"]) if r_lens is None else r_lens, r.n_bases, k)
        assert word in str(host.value)
        bufs = prefilled(ctx, n)
        rc, located = ctx.seq_locate_raw(s, r, True, *bufs)
        message = capi.lib().ksh_last_error().decode()
        assert rc == capi.KSH_INVALID_ARGUMENT and located == -1 and word in message, message
        assert untouched(bufs), word
        serves()

    serves()
    huge = lens(case["strings"])
    huge[1] = huge[3] = ref.UINT32_MAX
    bad = with_huge_lens(ctx, with_huge_lens(ctx, strings, 3), 1)
    refused("req->strings: lens[1] = UINT32_MAX", s=bad, s_lens=huge)
    refused("req->strings: sum(lens + K) = %d but n_bases = %d" % (strings.n_bases, strings.n_bases + 40),
            s=overdeclared(ctx, g, case["strings"], 40))
    huge = lens(case["reference"])
    huge[0] = ref.UINT32_MAX
    refused("req->reference: lens[0] = UINT32_MAX", r=with_huge_lens(ctx, reference, 0), r_lens=huge)
    refused("req->reference: sum(lens + K) = %d but n_bases = %d" % (reference.n_bases, reference.n_bases + 7),
            r=overdeclared(ctx, g, case["reference"], 7))
    # both containers malformed: the strings are named
    refused("req->strings: sum(lens + K)", s=overdeclared(ctx, g, case["strings"], 40),
            r=with_huge_lens(ctx, reference, 0), r_lens=huge)
    # the host's refusals leave the outputs alone as well
    bufs = prefilled(ctx, n)
    assert ctx.seq_locate_raw(strings, reference, True, bufs[0], None)[0] == capi.KSH_INVALID_ARGUMENT
    assert ctx.seq_locate_raw(strings, None, True, *bufs)[0] == capi.KSH_INVALID_ARGUMENT
    assert ctx.seq_locate_raw(strings, reference, True, *bufs, struct_size=8)[0] == capi.KSH_INVALID_ARGUMENT
    assert untouched(bufs)
    serves()


def test_more_than_one_pass_of_workgroups(ctx):
    """A reference of a few workgroups of positions in sequences of uneven lengths against reads cut from it and
    reverse-complemented ones: every end is found where the reference finds it."""
    k, g = 31, geom_of(31)
    rng = np.random.default_rng(77)
    reference = [cases.rnd(rng, int(n)) for n in rng.integers(k, 900, size=max(40, 3 * cases.BLOCK // 300))]
    assert sum(len(t) - k + 1 for t in reference) > 3 * cases.BLOCK
    reads = []
    for i in range(300):
        t = reference[int(rng.integers(0, len(reference)))]
        if len(t) > k + 1:
            a = int(rng.integers(0, len(t) - k))
            b = int(rng.integers(a + k, len(t) + 1))
            reads.append(ref.rc(t[a:b]) if i % 3 == 0 else t[a:b])
    reads += [cases.rnd(rng, k + 5) for _ in range(20)]
    for canonical in (True, False):
        answer = ref.locate(reads, reference, k, canonical)
        assert 0 < int((answer[1] == 0).sum()) < answer[1].size and (answer[0][answer[0] >= 0] & 1).any() == canonical
        bufs = prefilled(ctx, len(reads))
        rc, located = ctx.seq_locate_raw(capi.DeviceSpss.from_strings(g, reads, ctx.device),
                                         capi.DeviceSpss.from_strings(g, reference, ctx.device), canonical, *bufs)
        assert (rc, located) == (capi.KSH_OK, int((answer[1] > 0).sum())) and equal_to(bufs, answer)


def test_plans_stay_exact(gpu):
    """Every plan / write pair of the protocol's table with the call, and a refused call, between its plan and its
    write, issued on the victim's context and on a second one: the write is served and exact (include/kmersets_hip.h,
    "Plans": the call ends no pending plan)."""
    geom = (23, 14, 4)
    data = pp.Data(geom, 1000 + 23 + 14, gpu)
    case = next(c for c in cases.CASES if c["id"] == "both-strands-k23")
    answer = ref.locate(case["strings"], case["reference"], 23, True)
    own, second = capi.Context(0), capi.Context(0)
    try:
        inputs = {}
        for c in (own, second):
            pp.use(c)
            s = capi.DeviceSpss.from_strings(data.g, case["strings"], c.device)
            r = capi.DeviceSpss.from_strings(data.g, case["reference"], c.device)
            inputs[c] = (s, r, overdeclared(c, data.g, case["reference"], 33))

        def intrude(c):
            pp.use(c)
            s, r, bad = inputs[c]
            bufs = prefilled(c, len(case["strings"]))
            assert c.seq_locate_raw(s, r, True, *bufs)[0] == capi.KSH_OK and equal_to(bufs, answer)
            bufs = prefilled(c, len(case["strings"]))
            assert c.seq_locate_raw(s, bad, True, *bufs)[0] == capi.KSH_INVALID_ARGUMENT and untouched(bufs)

        assert sorted(protocol.KINDS) == sorted(["pair", "union", "decode", "count", "encode", "cover", "from_text",
                                                 "fasta"])
        for kind in protocol.KINDS:
            for where in (own, second):
                for plain in ((False, True) if kind in protocol.NAMELESS else (False,)):
                    pp.use(own)
                    v = pp.Victim(kind, data, own, plain=plain)
                    v.plan()
                    intrude(where)
                    pp.use(own)
                    v.write()
                    v.check_exact()
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())
        own.close()
        second.close()

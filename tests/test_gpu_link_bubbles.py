"""ksh_link_bubbles (capi.Context.link_bubbles) against the host reference of tests/link_bubbles_reference.py on the
designed graphs and the two string families of tests/link_bubbles_cases.py, without and with classes: all four
outputs, the write guard of 64 elements behind each, count / exact capacities / room to spare, each capacity too small
in turn, the call repeated, every device-side refusal with the outputs untouched and the context still serving, and
pending plans of every group staying exact across a call.  Every comparison is array equality."""
import numpy as np
import pytest
import torch

import link_bubbles_cases as bc
import link_bubbles_reference as ref
from kmersets import capi, synth

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
GUARD = 64


def _inputs():
    out = []
    for c in bc.CASES:
        out.append((c["id"], c, None, None))
        if c["n"]:  # (no strings, no classes: an array of no classes is no array)
            out.append((c["id"] + "-classes", c, bc.classes_of(c["n"]), bc.ROWS))
    for f in bc.families():
        out.append((f["id"], f, None, None))
        out.append((f["id"] + "-classes", f, f["string_class"], f["rows"]))
    return out


INPUTS = _inputs()


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """The reference's answer per input, computed once; most inputs have something to show."""
    out = {name: ref.bubbles(c["off"], c["to"], c["max_arm"], cls, rows) for name, c, cls, rows in INPUTS}
    assert sum(len(w[0]) > 0 for w in out.values()) * 2 > len(out)
    return out


def dev(ctx, a, dtype=None):
    with torch.cuda.stream(ctx.stream):
        return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device) if dtype is None else torch.from_numpy(
            np.ascontiguousarray(a).astype(dtype)).to(ctx.device)


def prefilled(ctx, nb, na):
    """ends, arm_offsets, arm_strings, arm_rows with GUARD elements behind what nb bubbles and na arm strings take."""
    sizes = (2 * nb, 2 * nb + 1, na, 4 * nb)
    with torch.cuda.stream(ctx.stream):
        return [torch.full((s + GUARD,), PATTERN, dtype=torch.int64, device=ctx.device) for s in sizes]


def untouched(bufs):
    return all(bool((b == PATTERN).all()) for b in bufs)


def equal_to(bufs, answer, with_rows):
    ends, off, arm, rows = answer
    nb, na = len(ends), len(arm)
    got = [b.cpu().numpy() for b in bufs]
    ok = np.array_equal(got[0][:2 * nb], ends.reshape(-1)) and bool((got[0][2 * nb:] == PATTERN).all())
    ok = ok and np.array_equal(got[1][:2 * nb + 1], off) and bool((got[1][2 * nb + 1:] == PATTERN).all())
    ok = ok and np.array_equal(got[2][:na], arm) and bool((got[2][na:] == PATTERN).all())
    if with_rows:
        ok = ok and np.array_equal(got[3][:4 * nb].view(np.uint64), rows.reshape(-1))
        return ok and bool((got[3][4 * nb:] == PATTERN).all())
    return ok and bool((got[3] == PATTERN).all())


@pytest.mark.parametrize("name,case,cls,rows", INPUTS, ids=[i[0] for i in INPUTS])
def test_bubbles_vs_reference(ctx, want, name, case, cls, rows):
    answer = want[name]
    nb, na = len(answer[0]), len(answer[2])
    off, to = dev(ctx, case["off"]), dev(ctx, case["to"])
    kw = dict(string_class=None if cls is None else dev(ctx, cls, np.int32), rows=rows)
    max_arm = case["max_arm"]
    # the wrapper: one call counts, a second one fills
    ends, arm_off, arm, arm_rows = ctx.link_bubbles(off, to, max_arm, **kw)
    assert ends.dtype == arm_off.dtype == arm.dtype == torch.int64 and ends.is_cuda and ends.shape == (nb, 2)
    assert np.array_equal(ends.cpu().numpy(), answer[0]) and np.array_equal(arm_off.cpu().numpy(), answer[1])
    assert np.array_equal(arm.cpu().numpy(), answer[2])
    if cls is None:
        assert arm_rows is None
    else:
        assert arm_rows.dtype == torch.uint64 and arm_rows.shape == (2 * nb, 2)
        assert np.array_equal(arm_rows.cpu().numpy(), answer[3])
    # count only: nothing is written, whether outputs are given or not
    bufs = prefilled(ctx, nb, na)
    assert ctx.link_bubbles_raw(off, to, max_arm, 0, 0, **kw) == (capi.KSH_OK, nb, na)
    assert ctx.link_bubbles_raw(off, to, max_arm, 0, 0, bufs[0], bufs[1], bufs[2], bufs[3] if cls is not None else None,
                                **kw) == (capi.KSH_OK, nb, na)
    assert untouched(bufs)
    outs = lambda b: (b[0], b[1], b[2], b[3] if cls is not None else None)  # noqa: E731
    # the exact capacities (with no strings at all they are 1 and 0: a capacity of 0 only counts)
    cap, arm_cap = max(nb, 1), na
    bufs = prefilled(ctx, nb, na)
    assert ctx.link_bubbles_raw(off, to, max_arm, cap, arm_cap, *outs(bufs), **kw) == (capi.KSH_OK, nb, na)
    assert equal_to(bufs, answer, cls is not None)
    again = prefilled(ctx, nb, na)  # the call made twice
    assert ctx.link_bubbles_raw(off, to, max_arm, cap, arm_cap, *outs(again), **kw) == (capi.KSH_OK, nb, na)
    assert all(torch.equal(a, b) for a, b in zip(again, bufs))
    roomy = prefilled(ctx, nb, na)  # room to spare: the same, nothing behind the counts
    assert ctx.link_bubbles_raw(off, to, max_arm, nb + 5, na + 9, *outs(roomy), **kw) == (capi.KSH_OK, nb, na)
    assert all(torch.equal(a, b) for a, b in zip(roomy, bufs))
    # each capacity too small in turn: the true numbers, and nothing written
    if nb > 1:
        for cap, arm_cap, word in ((nb - 1, na, "capacity = %d but n_bubbles = %d" % (nb - 1, nb)),
                                   (nb, na - 1, "arm_capacity = %d but n_arm_strings = %d" % (na - 1, na)),
                                   (1, na + 3, "capacity = 1 but n_bubbles = %d" % nb)):
            bufs = prefilled(ctx, nb, na)
            got = ctx.link_bubbles_raw(off, to, max_arm, cap, arm_cap, *outs(bufs), **kw)
            message = capi.lib().ksh_last_error().decode()
            assert got == (capi.KSH_FAILED_PRECONDITION, nb, na) and word in message, message
            assert untouched(bufs)


def test_device_refusals_touch_nothing(ctx):
    """One malformed graph per refusal.  Each is refused by the check before any walk; none reads outside its arrays
    (the check bounds every row before it reads it)."""
    case = next(c for c in bc.CASES if c["id"] == "back-to-back")
    off, to, n, max_arm = case["off"], case["to"], case["n"], case["max_arm"]
    cls = bc.classes_of(n)
    answer = ref.bubbles(off, to, max_arm, cls, bc.ROWS)
    nb, na = len(answer[0]), len(answer[2])
    d_cls = dev(ctx, cls, np.int32)

    def serves():
        bufs = prefilled(ctx, nb, na)
        assert ctx.link_bubbles_raw(dev(ctx, off), dev(ctx, to), max_arm, nb, na, *bufs, string_class=d_cls,
                                    rows=bc.ROWS) == (capi.KSH_OK, nb, na)
        assert equal_to(bufs, answer, True)

    def refused(word, off=off, to=to, cls=cls, n_links=None):
        with pytest.raises(ValueError) as host:  # the reference refuses it too, in the same words
            ref.check_graph(off, to if n_links is None else np.resize(to, n_links), cls, len(bc.ROWS))
        assert word in str(host.value)
        bufs = prefilled(ctx, nb, na)
        with pytest.raises(capi.KshError) as err:
            ctx.link_bubbles_raw(dev(ctx, off), dev(ctx, to), max_arm, nb, na, *bufs, string_class=dev(ctx, cls, np.int32),
                                 rows=bc.ROWS, n_links=n_links)
        assert word in str(err.value) and err.value.code == capi.KSH_INVALID_ARGUMENT, str(err.value)
        assert untouched(bufs), word
        serves()

    serves()
    bad = off.copy()
    bad[0] = 1
    refused("d_link_offsets[0] is not 0", off=bad)
    bad = off.copy()
    bad[-1] += 1
    refused("d_link_offsets[2 n] is not n_links", off=bad)
    refused("d_link_offsets[2 n] is not n_links", n_links=to.size - 2)  # offsets beyond n_links
    bad = off.copy()
    bad[3], bad[9] = bad[4] + 1, bad[10] + 2
    refused("descends behind vertex 3", off=bad)
    bad = off.copy()
    bad[1:-1] += 10 ** 12  # offsets far beyond n_links: no row of theirs is read
    refused("descends behind vertex %d" % (2 * n - 1), off=bad)
    refused("the row of vertex 0 has more than four", off=np.concatenate([[0], np.full(off.size - 1, to.size)]))
    bad = to.copy()
    bad[5], bad[2] = -1, 2 * n
    refused("the target of link 2 is outside", to=bad)
    bad = to.copy()
    bad[5] = -1
    refused("the target of link 5 is outside", to=bad)
    row = next(v for v in range(2 * n) if off[v + 1] - off[v] == 2)
    bad = to.copy()
    bad[off[row] + 1] = bad[off[row]]
    refused("the row of vertex %d repeats a target" % row, to=bad)
    bad = to.copy()
    bad[off[row]] ^= 1  # a link to the other orientation: its twin is not there
    refused("has no twin", to=bad)
    bad_cls = cls.copy()
    bad_cls[4], bad_cls[2] = -1, len(bc.ROWS)
    refused("the class of string 2 is outside", cls=bad_cls)
    # the links of non-canonical mode: only the rows 2 s have any
    one_off, one_to = ref.csr(3, [(0, 2), (2, 4)], twins=False)
    with pytest.raises(capi.KshError, match="canonical"):
        ctx.link_bubbles(dev(ctx, one_off), dev(ctx, one_to))
    serves()


def test_plans_stay_exact(ctx):
    """One victim of each plan group: plan, a bubbles call on the same context, then the write: served, and equal to
    a fresh plan + write (include/kmersets_hip.h, "Plans")."""
    k, n = 23, 14
    g = capi.geom(k, n)
    sets = synth.phylogeny_sets(k, 2, 20000, seed=17)
    a, b = (capi.DeviceSet.from_kmers(g, s, ctx.device) for s in sets)
    ca = ctx.spss_encode(a, mode=0)
    uncut = ca.to_strings()
    # the unitigs of the union of the two sets: they branch where the sets differ
    both = capi.DeviceSet.from_kmers(g, np.union1d(sets[0], sets[1]), ctx.device)
    off, to = ctx.spss_links(ctx.spss_encode(both, mode=1))
    answer = ref.bubbles(off.cpu().numpy(), to.cpu().numpy(), 8)
    assert len(answer[0]) > 0

    def intrude():
        got = ctx.link_bubbles(off, to)
        assert got[3] is None and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(got[:3], answer[:3]))

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

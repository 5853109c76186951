"""The byte-stream kernels at every boundary they create: stage_chunk's two staging paths and its global reads at
the span edges (csrc/ksh_bytes.h), the text form in both directions (csrc/ksh_text.hip), the FASTA front end
(csrc/ksh_fasta.hip), StreamVByte (csrc/ksh_svb.hip) and, through it, the four routes of scan_exclusive_i64.

The cases and the expected answers come from tests/byte_stream_cases.py (plain Python / numpy, pinned to the oracle
by tests/test_byte_stream_model_cpu.py).  Every input text is a slice buf[p : p + n] of a device buffer, so that the
pointer the C ABI gets has phase p modulo 16; every output buffer is longer than needed and prefilled with a
sentinel, and what lies behind the expected output must still be the sentinel.  Bit-exact throughout."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import byte_stream_cases as bsc
from kmersets import capi

pytestmark = pytest.mark.gpu

SENT_W = 0x5A5A5A5A5A5A5A5A  # int64 words
SENT_L = 0x5A5A5A5A          # int32 lens
SENT_B = 0xA5                # bytes
GUARD = 64
PHASES = list(range(16))


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def consts():
    return bsc.constants()


Expected = namedtuple("Expected", "verdict n_strings n_bases words lens strings")


def expect(case):
    if case.kind == "text":
        v = bsc.text_verdict(case.raw, case.k)
        lines = bsc.lines_of(case.raw)
        if v != bsc.OK:  # the plan still counts lines and bases of a text whose only fault is a short line
            return Expected(v, len(lines), sum(map(len, lines)), None, None, None)
        strings = lines
    else:
        v = bsc.fasta_verdict(case.raw)
        if v != bsc.OK:
            return Expected(v, 0, 0, None, None, None)
        strings = bsc.fasta_fragments(case.raw, case.k)
    words, lens = bsc.pack(strings, case.k)
    return Expected(v, len(strings), sum(map(len, strings)), words, lens, strings)


@pytest.fixture(scope="module")
def suite(consts):
    """kind -> [(case, expected)]: the references are computed once and shared."""
    return {"text": [(x, expect(x)) for x in bsc.text_cases(consts)],
            "fasta": [(x, expect(x)) for x in bsc.fasta_cases(consts)]}


def use(ctx):
    """torch's fills and copies go to torch's current stream, the library's kernels to the context's."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.set_stream(ctx.stream)


def at_phase(ctx, raw, p):
    """The bytes as buf[p : p + n] of a device buffer: a pointer of phase p modulo 16."""
    import torch

    buf = torch.full((p + len(raw) + 16,), SENT_B, dtype=torch.uint8, device=ctx.device)
    buf[p:p + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(ctx.device)
    text = buf[p:p + len(raw)]
    assert text.data_ptr() % 16 == p
    return text


def sentinel_buffers(ctx, exp):
    import torch

    n_words = (exp.n_bases + 31) // 32
    words = torch.full((n_words + 5,), SENT_W, dtype=torch.int64, device=ctx.device)
    lens = torch.full((exp.n_strings + 7,), SENT_L, dtype=torch.int32, device=ctx.device)
    return words, lens


def check_outputs(name, exp, words, lens):
    """The first ceil(n_bases / 32) words and n_strings lens are the packed reference, the rest is untouched."""
    n_words = (exp.n_bases + 31) // 32
    w = words.cpu().numpy().view(np.uint64)
    ln = lens.cpu().numpy().view(np.uint32)
    assert np.array_equal(w[:n_words], exp.words), name
    assert (w[n_words:] == np.uint64(SENT_W)).all(), name
    assert np.array_equal(ln[:exp.n_strings], exp.lens), name
    assert (ln[exp.n_strings:] == np.uint32(SENT_L)).all(), name


def geom():
    return capi.geom(*bsc.GEOM)


def to_text_at(ctx, g, words, lens, n_strings, n_bases, p):
    """lib().ksh_spss_to_text into out[p : p + n] of a sentinel-filled buffer -> (bytes written, guards intact)."""
    import torch

    n = n_bases + n_strings
    out = torch.full((GUARD + p + n + GUARD + 16,), SENT_B, dtype=torch.uint8, device=ctx.device)
    assert out.data_ptr() % 16 == 0 and GUARD % 16 == 0
    view = capi.SpssView(words.data_ptr(), lens.data_ptr(), n_strings, n_bases)
    capi.check(capi.lib().ksh_spss_to_text(ctx.h, C.byref(g), C.byref(view), out.data_ptr() + GUARD + p))
    host = out.cpu().numpy()
    lo, hi = GUARD + p, GUARD + p + n
    return host[lo:hi].tobytes(), bool((host[:lo] == SENT_B).all() and (host[hi:] == SENT_B).all())


# ---- the two parsers -----------------------------------------------------------------------------------------------------
def run_from_text(ctx, case, exp, p):
    text = at_phase(ctx, case.raw, p)
    g = geom()
    if exp.verdict == bsc.BAD_BYTE:
        with pytest.raises(capi.KshError) as e:
            ctx.spss_from_text_plan(g, text)
        assert e.value.code == 3 and bsc.TEXT_MESSAGE[bsc.BAD_BYTE] in str(e.value), case.name
        return
    plan = ctx.spss_from_text_plan(g, text)
    assert (plan.n_strings, plan.n_bases) == (exp.n_strings, exp.n_bases), case.name
    words, lens = sentinel_buffers(ctx, exp)
    if exp.verdict == bsc.SHORT:
        with pytest.raises(capi.KshError) as e:
            ctx.spss_from_text_write(plan, words=words, lens=lens)
        assert e.value.code == 3 and bsc.TEXT_MESSAGE[bsc.SHORT] % case.k in str(e.value), case.name
        assert (lens[exp.n_strings:] == SENT_L).all() and (words[(exp.n_bases + 31) // 32:] == SENT_W).all(), case.name
        return
    sp = ctx.spss_from_text_write(plan, words=words, lens=lens)
    check_outputs(case.name, exp, words, lens)
    if case.raw.endswith(b"\n"):  # to_text(from_text(t)) == t, written at the same phase
        back, intact = to_text_at(ctx, g, sp.words, sp.lens, sp.n_strings, sp.n_bases, p)
        assert back == case.raw and intact, case.name


def run_fasta(ctx, case, exp, p):
    text = at_phase(ctx, case.raw, p)
    g = geom()
    if exp.verdict != bsc.OK:
        with pytest.raises(capi.KshError) as e:
            ctx.fasta_plan(g, text)
        assert e.value.code == 9 and bsc.FASTA_MESSAGE[exp.verdict] in str(e.value), case.name
        return None
    plan = ctx.fasta_plan(g, text)  # accepted: the verdict is the reference's
    assert (plan.n_strings, plan.n_bases) == (exp.n_strings, exp.n_bases), case.name
    words, lens = sentinel_buffers(ctx, exp)
    frags = ctx.fasta_write(plan, words=words, lens=lens)
    check_outputs(case.name, exp, words, lens)
    return frags


def selected(suite, kind, p):
    """Every case at phase 0; at the other phases the ones that hold the chunk-edge and span-edge classes."""
    return [(x, e) for x, e in suite[kind] if p == 0 or x.phase]


@pytest.mark.parametrize("p", PHASES)
def test_from_text_at_pointer_phase(ctx, suite, p):
    use(ctx)
    chosen = selected(suite, "text", p)
    assert len(chosen) >= 30
    for case, exp in chosen:
        run_from_text(ctx, case, exp, p)
    assert {e.verdict for _, e in chosen} == {bsc.OK, bsc.BAD_BYTE, bsc.SHORT}


@pytest.mark.parametrize("p", PHASES)
def test_fasta_at_pointer_phase(ctx, suite, p):
    use(ctx)
    chosen = selected(suite, "fasta", p)
    assert len(chosen) >= 60
    for case, exp in chosen:
        run_fasta(ctx, case, exp, p)
    assert {e.verdict for _, e in chosen} == {bsc.OK, bsc.ODD, bsc.INVALID}


@pytest.mark.parametrize("p", [0, 7])
def test_fasta_fragments_count_to_the_reference_kmers(ctx, consts, suite, p):
    use(ctx)
    k = bsc.GEOM[0]
    done = 0
    for case, exp in suite["fasta"]:
        if not case.phase or exp.verdict != bsc.OK or len(case.raw) > 2 * consts.span + 200:
            continue
        frags = run_fasta(ctx, case, exp, p)
        got, n_cut = ctx.kmer_count(frags, 1)
        assert n_cut == 0 and np.array_equal(np.sort(got.kmers()), bsc.canonical_kmers_of(exp.strings, k)), case.name
        done += 1
    assert done >= 40


# ---- to_text ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def to_text_inputs(ctx, consts):
    """[(case, device words, device lens, n_bases, expected bytes)], uploaded once."""
    import torch

    use(ctx)
    out = []
    for x in bsc.to_text_cases(consts):
        words, lens = bsc.pack(x.strings, x.k)
        w = torch.from_numpy(words.view(np.int64).copy()).to(ctx.device)
        ln = torch.from_numpy(lens.view(np.int32).copy()).to(ctx.device)
        out.append((x, w, ln, sum(map(len, x.strings)), bsc.text_of(x.strings)))
    return out


@pytest.mark.parametrize("p", PHASES)
def test_to_text_at_output_phase(ctx, to_text_inputs, p):
    use(ctx)
    for x, w, ln, n_bases, want in to_text_inputs:
        g = capi.geom(x.k, 3 if x.k == bsc.K_DENSE else bsc.GEOM[1])
        got, intact = to_text_at(ctx, g, w, ln, len(x.strings), n_bases, p)
        assert got == want, x.name
        assert intact, x.name


def test_to_text_refuses_an_under_declared_view(ctx, consts):
    """A view whose string lengths sum to more than its n_bases is refused, and the context works afterwards.  The
    excess stays at 64 bases at the most: whatever a string end beyond n_bases indexes then lies inside the scratch
    arena's own allocations."""
    import torch

    use(ctx)
    rng = np.random.default_rng(0x0DEC)
    strings = [bsc.acgt(rng, int(v)) for v in rng.integers(bsc.K, 90, size=40)]
    n_bases = sum(map(len, strings))
    words, lens = bsc.pack(strings, bsc.K)
    w = torch.from_numpy(words.view(np.int64).copy()).to(ctx.device)
    ln = torch.from_numpy(lens.view(np.int32).copy()).to(ctx.device)
    g = geom()
    for excess in (1, 33, 64):
        with pytest.raises(capi.KshError) as e:
            to_text_at(ctx, g, w, ln, len(strings), n_bases - excess, 0)
        assert e.value.code == 3, excess
        assert "sum of string lengths (%d) != n_bases (%d)" % (n_bases, n_bases - excess) in str(e.value)
        got, intact = to_text_at(ctx, g, w, ln, len(strings), n_bases, 0)
        assert got == bsc.text_of(strings) and intact, excess


# ---- the FASTA slot's growth -------------------------------------------------------------------------------------------------
def test_fasta_slot_growth_in_both_orders(ctx, consts):
    """One large and one small text on a fresh context, and small first, then large, on another: the large plan
    finds the text slot too small for its fragment arrays either way (3 x 8 bytes per fragment against the 64 KiB
    of slack a slot is given), which is the branch of ksh_fasta_plan that recomputes the two prefix arrays."""
    rng = np.random.default_rng(0x510F)
    recs = []
    while sum(map(len, recs)) < 3 * consts.span - 400:
        read = b"N".join(bsc.acgt(rng, int(v)) for v in rng.integers(1, 13, size=int(rng.integers(1, 40))))
        recs.append(bsc.header(int(rng.integers(2, 12))) + read + b"\n")
    large = b"".join(recs)
    small = bsc.header(7) + bsc.acgt(rng, 30) + b"N" + bsc.acgt(rng, 8) + b"\n"
    assert len(bsc.fasta_runs(large)) > 4000 and len(large) < 50_000
    texts = {"large": bsc.Case("large", "fasta", large, bsc.K, False), "small": bsc.Case("small", "fasta", small, bsc.K, False)}
    exps = {name: expect(x) for name, x in texts.items()}
    assert exps["large"].n_strings > 1000 and exps["small"].n_strings == 1
    try:
        for order in (("large", "small"), ("small", "large")):
            fresh = capi.Context(0)
            try:
                use(fresh)
                for name in order:
                    run_fasta(fresh, texts[name], exps[name], 3)  # check_outputs: all four calls equal the reference
            finally:
                import torch

                torch.cuda.synchronize()
                fresh.close()
    finally:
        use(ctx)


# ---- StreamVByte, and the scan under it --------------------------------------------------------------------------------------
def svb_round_trip(ctx, name, d_in, n, want):
    """encode == reference (the size-only call too), decode(encode(v)) == v, bytes_read == size; nothing is written
    behind either output."""
    L = capi.lib()
    size = C.c_int64(-1)
    capi.check(L.ksh_svb_encode_0124(ctx.h, d_in.data_ptr(), n, None, C.byref(size)))
    assert size.value == want.size, name
    svb_decode_guarded(ctx, name, svb_encode_guarded(ctx, name, d_in, n, want), d_in, n, want)


def svb_encode_guarded(ctx, name, d_in, n, want):
    """One encode into a buffer with a sentinel tail: the reference's bytes, nothing behind them.  Returns the buffer."""
    import torch

    d_out = torch.full((want.size + GUARD,), SENT_B, dtype=torch.uint8, device=ctx.device)
    size = C.c_int64(-1)
    capi.check(capi.lib().ksh_svb_encode_0124(ctx.h, d_in.data_ptr(), n, d_out.data_ptr(), C.byref(size)))
    assert size.value == want.size, name
    host = d_out.cpu().numpy()
    assert np.array_equal(host[:want.size], want), name
    assert (host[want.size:] == SENT_B).all(), name
    return d_out


def svb_decode_guarded(ctx, name, d_out, d_in, n, want):
    """One decode of an encoded buffer: the values that went in, the bytes read, nothing behind the values."""
    import torch

    back = torch.full((n + 8,), SENT_L, dtype=torch.int32, device=ctx.device)
    used = C.c_int64(-1)
    capi.check(capi.lib().ksh_svb_decode_0124(ctx.h, d_out.data_ptr(), n, back.data_ptr(), C.byref(used)))
    assert used.value == want.size, name
    assert torch.equal(back[:n], d_in[:n]) and bool((back[n:] == SENT_L).all()), name


@pytest.mark.parametrize("route", ["small", "chained", "tiled"])
def test_svb_on_the_scan_route(ctx, consts, route):
    import torch

    use(ctx)
    chosen = [x for x in bsc.svb_cases(consts) if bsc.scan_route((x.n + 3) // 4, consts) == route]
    assert len(chosen) >= 8 and {x.n % 4 for x in chosen} == {0, 1, 2, 3}
    assert {x.pattern for x in chosen} == set(bsc.PATTERNS)
    for x in chosen:
        v = bsc.svb_values(x)
        d_in = torch.from_numpy(v.view(np.int32).copy()).to(ctx.device)
        svb_round_trip(ctx, x.name, d_in, x.n, bsc.svb_encode(v))


@pytest.mark.parametrize("which", [0, 1])
def test_svb_on_the_recursion_route(ctx, consts, which):
    """kScanFixMaxBlocks tiles + 1 groups; all values zero but 10^5 scattered ones, placed on the device."""
    import torch

    use(ctx)
    name, n, idx, vals = bsc.svb_sparse_cases(consts)[which]
    assert bsc.scan_route((n + 3) // 4, consts) == "recursion"
    d_in = torch.zeros(n, dtype=torch.int32, device=ctx.device)
    d_in[torch.from_numpy(idx).to(ctx.device)] = torch.from_numpy(vals.view(np.int32).copy()).to(ctx.device)
    svb_round_trip(ctx, name, d_in, n, bsc.svb_encode_sparse(n, idx, vals))

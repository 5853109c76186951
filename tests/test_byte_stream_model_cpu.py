"""CPU checks of the byte-stream sweep (tests/byte_stream_cases.py): the constants and lines read from the kernels'
text, the class list -- which chunk, span and word boundaries the built texts hit, recomputed from their bytes --
and the plain references against the oracle (KmerCounter::FromFASTA's verdict and k-mers, KmerSetCompact's words
and StreamVByte bytes).  tests/test_gpu_byte_streams.py runs the cases."""
import numpy as np
import pytest

import byte_stream_cases as bsc
import oracle_lib as ol


@pytest.fixture(scope="module")
def c():
    return bsc.constants()


@pytest.fixture(scope="module")
def cases(c):
    return {"text": bsc.text_cases(c), "fasta": bsc.fasta_cases(c)}


@pytest.fixture(scope="module")
def case_facts(c, cases):
    return {kind: [bsc.facts(kind, x.raw, x.k, c) for x in cases[kind]] for kind in cases}


def test_constants_read_from_the_kernels(c):
    # the values the cases were laid out for: a changed constant is a reason to look at the cases again
    assert c == bsc.Consts(chunk=64, threads=256, stride=68, span=16384, text_lds=20544, scan_small=4096,
                           scan_tile=2048, fix_blocks=4096, chain_tile=2048, chain_blocks=128)
    assert c.span + c.span // bsc.K_DENSE <= c.text_lds  # the K = 4 span fits k_to_text's LDS, and only just
    assert c.text_lds - (c.span + c.span // bsc.K_DENSE) == 64
    src = bsc.sources()
    # every restated line is needed: without it the constants do not parse
    for name, line, _ in bsc.RESTATED:
        broken = dict(src)
        broken[name] = src[name].replace(line, line[:len(line) // 2] + " /**/ " + line[len(line) // 2:])
        assert broken[name] != src[name]
        with pytest.raises(AssertionError):
            bsc.constants(broken)
    # and every constant is read, not assumed
    for name, const, field in (("bytes", "kChunkBytes", None), ("bytes", "kChunkThreads", None),
                               ("bytes", "kChunkStride", "stride"), ("fasta", "kFaChunk", None),
                               ("fasta", "kFaThreads", None), ("text", "kChunk", None), ("text", "kTextThreads", None),
                               ("core", "kScanSmallMax", "scan_small"), ("core", "kScanItems", "scan_tile"),
                               ("core", "kScanThreads", "scan_tile"), ("core", "kScanFixMaxBlocks", "fix_blocks"),
                               ("scan", "kChainItems", "chain_tile"), ("scan", "kChainThreads", "chain_tile"),
                               ("scan", "kChainMaxBlocks", "chain_blocks")):
        changed = dict(src)
        changed[name], n = bsc.re.subn(r"(constexpr (?:int|int64_t) %s = )(\d+);" % const,
                                       lambda m: "%s%d;" % (m.group(1), 2 * int(m.group(2))), src[name])
        assert n == 1, const
        if field is None:  # the three files must agree on the chunk and the workgroup
            with pytest.raises(AssertionError):
                bsc.constants(changed)
        else:
            assert getattr(bsc.constants(changed), field) == 2 * getattr(c, field), const


@pytest.mark.parametrize("kind", ["text", "fasta"])
def test_every_class_is_hit(kind, c, cases, case_facts):
    names = [x.name for x in cases[kind]]
    assert len(set(names)) == len(names)
    assert all(len(x.raw) <= 3 * c.span + 2 * c.chunk < 50_000 for x in cases[kind])
    have = set().union(*case_facts[kind])
    missing = bsc.required(kind, c) - have
    assert not missing, sorted(missing)
    # the cases that run at every pointer phase hit every chunk-edge and span-edge class
    phased = set().union(*(f for x, f in zip(cases[kind], case_facts[kind]) if x.phase))
    missing = bsc.phase_required(kind, c) - phased
    assert not missing, sorted(missing)
    assert len(bsc.phase_required(kind, c)) >= 15
    # thread 0 of span 1 reads text[b0 - 1] from global memory and it matters: a base continues a line or a
    # fragment there in one phased case, a newline closes one in another
    span_prev = {x.raw[c.span - 1:c.span + 1] for x in cases[kind] if x.phase and len(x.raw) > c.span}
    assert any(p[:1] == b"\n" for p in span_prev) and any(p[:1] in b"ACGT" and p[1:] in b"ACGT" for p in span_prev)
    if kind == "fasta":
        assert any(p[:1] == b"N" and p[1:] in b"ACGT" for p in span_prev)


def test_to_text_classes(c, cases):
    tt = bsc.to_text_cases(c)
    have = set().union(*(bsc.to_text_facts(x.strings, x.k, c) for x in tt))
    assert not bsc.to_text_required(c) - have, sorted(bsc.to_text_required(c) - have)
    assert all(len(s) >= x.k for x in tt for s in x.strings)
    # the accepted, closed text cases run through to_text as well (the round trip of the GPU test)
    closed = [x for x in cases["text"] if bsc.text_verdict(x.raw, x.k) == bsc.OK and x.raw.endswith(b"\n")]
    assert len(closed) > 40
    for x in closed:
        assert bsc.text_of(bsc.lines_of(x.raw)) == x.raw


def test_text_reference_against_the_oracle(c, cases):
    k, n, kb = bsc.GEOM
    for x in cases["text"][::3] + bsc.to_text_cases(c)[:6]:
        strings = x.strings if isinstance(x, bsc.ToText) else bsc.lines_of(x.raw)
        if isinstance(x, bsc.Case) and bsc.text_verdict(x.raw, x.k) != bsc.OK:
            continue
        words, lens = bsc.pack(strings, x.k)
        oc = ol.Compact.from_strings([s.decode() for s in strings], x.k, n, kb)
        assert np.array_equal(oc.words(), words), x.name
        assert np.array_equal(oc.lengths_compressed(), bsc.svb_encode(lens)), x.name
        assert lens.size == len(strings) and words.size == (sum(map(len, strings)) + 31) // 32


def test_fasta_reference_against_the_oracle(c, cases):
    k, n, kb = bsc.GEOM
    code = {bsc.OK: 0, bsc.ODD: 1, bsc.INVALID: 2}
    seen = set()
    for x in cases["fasta"]:
        v = bsc.fasta_verdict(x.raw)
        seen.add(v)
        oc = ol.Counter(k, n, kb)
        assert oc.from_fasta(x.raw) == code[v], x.name
        if v == bsc.OK:
            frags = bsc.fasta_fragments(x.raw, k)
            want = bsc.canonical_kmers_of(frags, k)
            got, n_cut = oc.to_set(1)
            assert n_cut == 0 and np.array_equal(np.sort(got.kmers()), want), x.name
    assert seen == set(code)
    # the order of the checks: a text that is both odd and invalid is odd
    both = b"r1\nACGTA\n>r2\n"
    assert bsc.fasta_verdict(both) == bsc.ODD and ol.Counter(k, n, kb).from_fasta(both) == 1


def test_svb_reference_against_the_oracle(c):
    L = ol.lib()
    small = [x for x in bsc.svb_cases(c) if x.n <= 4 * (c.scan_small + 1)]
    assert {x.pattern for x in small} == set(bsc.PATTERNS) and {x.n % 4 for x in small} == {0, 1, 2, 3}
    for x in small:
        v = bsc.svb_values(x)
        want = np.zeros(int(L.ko_svb_max_compressed_bytes(v.size)), dtype=np.uint8)
        size = int(L.ko_svb_encode_0124(v, v.size, want))
        got = bsc.svb_encode(v)
        assert got.size == size and np.array_equal(got, want[:size]), x.name
        back, used = bsc.svb_decode(got, v.size)
        assert used == size and np.array_equal(back, v), x.name
        # the sparse form of the recursion-route case is the dense one
        idx = np.flatnonzero(v)
        assert np.array_equal(bsc.svb_encode_sparse(v.size, idx, v[idx]), got), x.name
    for x in bsc.svb_cases(c):
        v = bsc.svb_values(x) if x.n <= 70000 else None
        if v is not None and x.pattern == "big":
            assert (v >= 65536).all()
        if v is not None and x.pattern == "widths" and v.size >= 4:
            per = [set(bsc._svb_codes(v[j::4]).tolist()) for j in range(4)]
            assert all(len(p) == 1 for p in per) and set().union(*per) == {0, 1, 2, 3}
        if v is not None and x.pattern == "bounds" and v.size > 1000:
            assert set(bsc.BOUNDS.tolist()) <= set(v.tolist())


def test_svb_sizes_sit_on_the_scan_regimes(c):
    route = lambda ng: bsc.scan_route(ng, c)
    groups = {(x.n + 3) // 4 for x in bsc.svb_cases(c)}
    assert {x.n % 4 for x in bsc.svb_cases(c) if (x.n + 3) // 4 == c.scan_small + 1} == {0, 1, 2, 3}
    top = c.chain_tile * c.chain_blocks
    t = c.chain_tile
    assert {c.scan_small, c.scan_small + 1, t - 1, t, t + 1, 2 * t, top, top + 1} <= groups
    assert (route(c.scan_small), route(c.scan_small + 1)) == ("small", "chained")
    assert (route(top), route(top + 1)) == ("chained", "tiled")
    # a chained workgroup edge inside the chained route, and a tile edge of the tiled route
    assert {3 * t - 1, 3 * t, 3 * t + 1} <= groups and route(3 * t - 1) == "chained"
    above = [g for g in groups if route(g) == "tiled"]
    assert {g % c.scan_tile for g in above} >= {c.scan_tile - 1, 0, 1}
    for _, n, idx, vals in bsc.svb_sparse_cases(c):
        ng = (n + 3) // 4
        assert route(ng) == "recursion" and route(ng - 1) == "tiled" and ng == c.fix_blocks * c.scan_tile + 1
        assert 3.3e7 < n < 3.5e7 and idx.size <= bsc.SPARSE_NONZERO + 4 and set(bsc.BOUNDS[1:].tolist()) <= set(vals.tolist())
        # the scan of the block sums inside the recursion takes the chained route
        assert route((ng + c.scan_tile - 1) // c.scan_tile) == "chained"

"""Cases and plain references for the byte-stream kernels: stage_chunk (csrc/ksh_bytes.h), the SPSS text form
(csrc/ksh_text.hip), the FASTA front end (csrc/ksh_fasta.hip), StreamVByte 0124 (csrc/ksh_svb.hip) and the
exclusive scan they all lean on (scan_exclusive_i64, csrc/ksh_core.hip and ksh_scan.h).

A *case* is one small text (at most 3 spans + 2 chunks) built so that a newline, a line, a fragment, an 'N' or an
invalid byte falls on a boundary the kernels create: the 64-byte chunk of a thread, the 16 KiB span of a workgroup,
the 32-base output word.  The *placers* put a feature at an absolute byte offset: a FASTA header has free length
('>' plus a filler that itself holds A, C, G, T, N and '>' bytes, so that a line-parity error shows); in the text
form earlier lines of length >= K sum to the wanted offset.

The *references* are pure Python / numpy and share no code with the kernels: the text form and its inverse, the
FASTA verdict and fragments (pinned to the oracle in tests/test_byte_stream_model_cpu.py), the ksh_spss_view
packing, and a vectorised StreamVByte 0124 encoder and decoder written from the format description.

What a case is *for* is never taken from its label: facts() recomputes the boundary classes a text hits from its
bytes and the constants, and the CPU test checks the required class lists against that.  The constants themselves
are read from the kernels' text, and the lines the cases rely on must stand there as written, so a changed kernel
fails the CPU test instead of moving the cases off their boundaries silently."""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc")
FILES = {"bytes": "ksh_bytes.h", "text": "ksh_text.hip", "fasta": "ksh_fasta.hip", "core": "ksh_core.hip",
         "scan": "ksh_scan.h", "svb": "ksh_svb.hip"}

K = 9                      # both parsers run at (k, N, key bytes) = GEOM, the oracle's FASTA pin uses the same
GEOM = (9, 10, 4)
K_DENSE = 4                # the smallest K the text kernels take: the densest newlines of k_to_text
OK, ODD, INVALID, BAD_BYTE, SHORT = "ok", "odd", "invalid", "bad_byte", "short"
FASTA_MESSAGE = {ODD: "FASTA files should have an even number of lines", INVALID: "invalid FASTA file"}
TEXT_MESSAGE = {BAD_BYTE: "neither A, C, G, T nor a newline", SHORT: "a line shorter than K = %d"}


# ---- constants from the kernels' text ------------------------------------------------------------------------------
def sources():
    return {name: open(os.path.join(CSRC, f)).read() for name, f in FILES.items()}


# the lines the cases rely on: (file, line, how often it stands there)
RESTATED = (
    ("bytes", "if ((reinterpret_cast<uintptr_t>(text) & 15) == 0) {", 1),
    ("bytes", "else if (b0 > 0) c.prev = text[b0 - 1];", 1),
    ("bytes", "c.next = threadIdx.x + 1 < kChunkThreads ? lds[(threadIdx.x + 1) * kChunkStride] : text[b0 + kChunkBytes];", 1),
    ("bytes", "const int64_t block0 = int64_t(blockIdx.x) * (kChunkThreads * kChunkBytes);", 1),
    ("text", "constexpr int kSpan = kTextThreads * kChunk;", 1),
    ("text", "constexpr int kTextLds = kSpan + kSpan / 4 + 64;", 1),
    ("text", "const int lead = int(base0 & 31);", 1),
    ("text", "const int head = int((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15);", 1),
    ("text", "if (w == 0 || w == n_words - 1) atomicOr(&out[w], x);", 1),
    ("text", "if (g->k < 4) return fail(KSH_INVALID_ARGUMENT, \"the text kernels need K >= 4\");", 1),
    ("text", "if (len < k) {", 1),
    ("fasta", "constexpr int kFaSpan = kFaThreads * kFaChunk;", 1),
    ("fasta", "const int lead = int(base0 & 31);", 1),
    ("fasta", "if (b0 > 0 && r > 0) keep = frag_end[r - 1] > b0 && frag_end[r - 1] - frag_start[r - 1] >= k;", 2),
    ("fasta", "keep = frag_end[r] - frag_start[r] >= k;", 2),
    ("fasta", "if (w == 0 || w == n_words - 1) atomicOr(&out[w], x);", 1),
    ("fasta", "const bool grows = 3 * per_chunk + 3 * per_frag > ctx->slot_bytes[kSlotText];", 1),
    ("core", "constexpr int kScanTile = kScanThreads * kScanItems;", 1),
    ("core", "if (n <= kScanSmallMax) {", 1),
    ("core", "if (scan_exclusive_chained(ctx, LoadArray{d_in}, d_out, n, d_total)) {", 1),
    ("core", "if (blocks <= kScanFixMaxBlocks) {", 1),
    ("scan", "constexpr int kChainTile = kChainThreads * kChainItems;", 1),
    ("scan", "if (n <= 0 || blocks > kChainMaxBlocks || !ctx->scan_state) return false;", 1),
    ("svb", "return v == 0 ? 0 : (v < 256u ? 1 : (v < 65536u ? 2 : 3));", 1),
    ("svb", "const int64_t n_groups = (n + 3) / 4;", 2),
)

Consts = namedtuple("Consts", "chunk threads stride span text_lds scan_small scan_tile fix_blocks chain_tile chain_blocks")


def constants(src=None):
    """The constants of the byte-stream kernels, from their text; the restated lines must stand there as written."""
    src = src or sources()

    def num(name, const):
        m = re.search(r"constexpr (?:int|int64_t) %s = (\d+);" % const, src[name])
        assert m, "%s no longer defines %s as a plain number" % (FILES[name], const)
        return int(m.group(1))

    for name, line, times in RESTATED:
        assert src[name].count(line) == times, "%s no longer has (%d x) the line the cases restate: %s" % (
            FILES[name], times, line)
    chunk, threads, stride = num("bytes", "kChunkBytes"), num("bytes", "kChunkThreads"), num("bytes", "kChunkStride")
    assert (num("fasta", "kFaChunk"), num("fasta", "kFaThreads")) == (chunk, threads), "FASTA and stage_chunk disagree"
    assert (num("text", "kChunk"), num("text", "kTextThreads")) == (chunk, threads), "text and stage_chunk disagree"
    assert stride >= chunk and stride % 4 == 0
    span = chunk * threads
    scan_tile = num("core", "kScanThreads") * num("core", "kScanItems")
    chain_tile = num("scan", "kChainThreads") * num("scan", "kChainItems")
    return Consts(chunk, threads, stride, span, span + span // 4 + 64, num("core", "kScanSmallMax"), scan_tile,
                  num("core", "kScanFixMaxBlocks"), chain_tile, num("scan", "kChainMaxBlocks"))


# ---- references ------------------------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CODE = np.full(256, 255, dtype=np.uint8)
CODE[ACGT] = np.arange(4, dtype=np.uint8)


def text_of(strings):
    """The text form of an SPSS: every string closed by a newline."""
    return b"".join(s + b"\n" for s in strings)


def lines_of(raw):
    """Split on '\\n', dropping the empty piece after a final newline (no bytes: no lines)."""
    parts = raw.split(b"\n")
    if parts[-1] == b"":
        parts.pop()
    return parts


def line_starts(raw):
    out, at = [], 0
    for ln in lines_of(raw):
        out.append(at)
        at += len(ln) + 1
    return out


def text_verdict(raw, k):
    """ok / bad_byte (seen by the plan) / short (seen by the write)."""
    if any(c not in b"ACGT\n" for c in raw):
        return BAD_BYTE
    if any(len(ln) < k for ln in lines_of(raw)):
        return SHORT
    return OK


def fasta_verdict(raw):
    """odd line count, then an invalid header or read byte, else ok (KmerCounter::FromFASTA's order)."""
    lines = lines_of(raw)
    if len(lines) % 2:
        return ODD
    for i, ln in enumerate(lines):
        if i % 2 == 0:
            if not ln or ln[:1] != b">":
                return INVALID
        elif any(c not in b"ACGTN" for c in ln):
            return INVALID
    return OK


def fasta_runs(raw):
    """[start, end) of every maximal ACGT run of the odd lines, in file order."""
    out = []
    for i, (at, ln) in enumerate(zip(line_starts(raw), lines_of(raw))):
        if i % 2:
            out.extend((at + m.start(), at + m.end()) for m in re.finditer(rb"[ACGT]+", ln))
    return out


def fasta_fragments(raw, k):
    return [raw[s:e] for s, e in fasta_runs(raw) if e - s >= k]


def pack(strings, k):
    """Strings over ACGT -> (uint64 words, uint32 len - k) in the ksh_spss_view layout: base i of the stream in
    bits [62 - 2 (i % 32), 63 - 2 (i % 32)] of word i / 32."""
    lens = np.array([len(s) - k for s in strings], dtype=np.int64)
    assert (lens >= 0).all()
    codes = CODE[np.frombuffer(b"".join(strings), dtype=np.uint8)]
    assert (codes < 4).all()
    n_words = (codes.size + 31) // 32
    padded = np.zeros(n_words * 32, dtype=np.uint64)
    padded[:codes.size] = codes
    shifts = (62 - 2 * np.arange(32)).astype(np.uint64)
    words = np.bitwise_or.reduce(padded.reshape(n_words, 32) << shifts, axis=1) if n_words else np.zeros(0, np.uint64)
    return words.astype(np.uint64), lens.astype(np.uint32)


def kmers_of(fragments, k):
    """The distinct k-mers (2 bits per base, first base highest) of a list of strings, ascending."""
    out = set()
    for f in fragments:
        c = CODE[np.frombuffer(f, dtype=np.uint8)].astype(np.uint64)
        if c.size >= k:
            v = np.zeros(c.size - k + 1, dtype=np.uint64)
            for j in range(k):
                v = (v << np.uint64(2)) | c[j:j + v.size]
            out.update(v.tolist())
    return np.array(sorted(out), dtype=np.uint64)


def revcomp(kmers, k):
    x = np.asarray(kmers, dtype=np.uint64)
    out = np.zeros_like(x)
    for _ in range(k):
        out = (out << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x = x >> np.uint64(2)
    return out


def canonical_kmers_of(fragments, k):
    x = kmers_of(fragments, k)
    return np.unique(np.minimum(x, revcomp(x, k)))


# StreamVByte 0124: ceil(n / 4) control bytes, then the data bytes; value i has a 2-bit code in control byte
# i / 4 at bits [2 (i % 4), 2 (i % 4) + 1]; code 0 / 1 / 2 / 3 = 0 / 1 / 2 / 4 little-endian data bytes, the
# smallest width that holds the value.
def _svb_codes(v):
    return ((v > 0).astype(np.uint8) + (v > 255) + (v > 65535)).astype(np.uint8)


def svb_encode(values):
    v = np.ascontiguousarray(values, dtype=np.uint32)
    n_groups = (v.size + 3) // 4
    code = _svb_codes(v)
    quad = np.zeros(n_groups * 4, dtype=np.uint8)
    quad[:v.size] = code
    quad = quad.reshape(n_groups, 4)
    ctrl = quad[:, 0] | (quad[:, 1] << 2) | (quad[:, 2] << 4) | (quad[:, 3] << 6)
    width = np.where(code == 3, 4, code)
    le = v.astype("<u4").view(np.uint8).reshape(v.size, 4)
    data = le[np.arange(4)[None, :] < width[:, None]]  # row-major: value order, low byte first
    return np.concatenate([ctrl.astype(np.uint8), data])


def svb_decode(data, n):
    """-> (values, bytes read)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n_groups = (n + 3) // 4
    code = ((data[:n_groups, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(-1)[:n]
    width = np.where(code == 3, 4, code)
    total = int(width.sum())
    le = np.zeros((n, 4), dtype=np.uint8)
    le[np.arange(4)[None, :] < width[:, None]] = data[n_groups:n_groups + total]
    return le.view("<u4").reshape(-1).astype(np.uint32), n_groups + total


def svb_encode_sparse(n, idx, vals):
    """svb_encode of n values that are zero except vals (non-zero) at the ascending indices idx, without the
    dense array: a zero has code 0 and no data byte."""
    idx = np.asarray(idx, dtype=np.int64)
    vals = np.ascontiguousarray(vals, dtype=np.uint32)
    assert (np.diff(idx) > 0).all() and (vals > 0).all() and (idx.size == 0 or idx[-1] < n)
    ctrl = np.zeros((n + 3) // 4, dtype=np.uint8)
    np.add.at(ctrl, idx // 4, (_svb_codes(vals) << (2 * (idx % 4)).astype(np.uint8)).astype(np.uint8))
    return np.concatenate([ctrl, svb_encode(vals)[(vals.size + 3) // 4:]])


# ---- placers -----------------------------------------------------------------------------------------------------------
FILL = b"ACGTN>NTGCA>GN"


def acgt(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def header(n):
    """A header line of n bytes, '>' and the newline included (n >= 2)."""
    assert n >= 2, n
    return b">" + (FILL * (n // len(FILL) + 1))[:n - 2] + b"\n"


def fa_place(prefix, read, at, off=0):
    """prefix (whole records) + a header + read + newline, with read[off] at absolute byte `at`."""
    return prefix + header(at - off - len(prefix)) + read + b"\n"


def fa_fill(rng, n_bytes):
    """Exactly n_bytes (>= 5) of valid records: reads of 1 to 200 bases with some 'N's, the last one to measure."""
    out, left = [], n_bytes
    while left > 320:
        read = bytearray(acgt(rng, int(rng.integers(1, 200))))
        for _ in range(int(rng.integers(0, 3))):
            p = int(rng.integers(0, len(read)))
            w = int(rng.integers(1, 4))
            read[p:p + w] = b"N" * len(read[p:p + w])
        rec = header(int(rng.integers(2, 30))) + bytes(read) + b"\n"
        out.append(rec)
        left -= len(rec)
    h = min(10, left - 3)
    out.append(header(h) + acgt(rng, left - h - 1) + b"\n")
    raw = b"".join(out)
    assert len(raw) == n_bytes
    return raw


def t_fill(rng, n_bytes, k, n_lines=None):
    """Exactly n_bytes of lines of length >= k, each closed by a newline (n_lines of them if given)."""
    if n_bytes == 0:
        return b""
    assert n_bytes >= k + 1, n_bytes
    if n_lines is None:
        n_lines = max(1, n_bytes // (k + 21))
    extra = n_bytes - n_lines * (k + 1)
    assert extra >= 0, (n_bytes, n_lines)
    cuts = np.sort(rng.integers(0, extra + 1, size=n_lines - 1))
    parts = np.diff(np.concatenate([[0], cuts, [extra]]))
    raw = b"".join(acgt(rng, k + int(e)) + b"\n" for e in parts)
    assert len(raw) == n_bytes
    return raw


def put(raw, pos, byte):
    return raw[:pos] + byte + raw[pos + 1:]


# ---- what a text hits, from its bytes ------------------------------------------------------------------------------------
def sizes(c):
    s = c.span
    return (1, 63, 64, 65, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1)


def bad_positions(kind, raw):
    """Byte positions that make the text invalid (an empty header counts at its newline)."""
    if kind == "text":
        return [i for i, c in enumerate(raw) if c not in b"ACGT\n"]
    out = []
    for i, (at, ln) in enumerate(zip(line_starts(raw), lines_of(raw))):
        if i % 2 == 0:
            if ln[:1] != b">":
                out.append(at)
        else:
            out.extend(at + j for j, c in enumerate(ln) if c not in b"ACGTN")
    return out


def kept_mask(kind, raw, k):
    a = np.frombuffer(raw, dtype=np.uint8)
    if kind == "text":
        return a != 10
    m = np.zeros(a.size, dtype=bool)
    for s, e in fasta_runs(raw):
        if e - s >= k:
            m[s:e] = True
    return m


def verdict(kind, raw, k):
    return text_verdict(raw, k) if kind == "text" else fasta_verdict(raw)


def _where(pos, c):
    """Names of the boundary places an absolute byte position is."""
    out = []
    if pos % c.chunk == 0:
        out.append("chunk0")
    if pos % c.chunk == c.chunk - 1:
        out.append("chunk63")
    if pos == c.span - 1:
        out.append("span0_last")
    if pos == c.span:
        out.append("span1_first")
    return out


def _straddles(start, end, c):
    """(boundary kind, bases before, bases after) of every chunk start inside (start, end)."""
    out = []
    b = (start // c.chunk + 1) * c.chunk
    while b < end:
        out.append(("span" if b % c.span == 0 else "chunk", b - start, end - b))
        b += c.chunk
    return out


def facts(kind, raw, k, c):
    """The boundary classes a text hits, recomputed from its bytes and the constants."""
    f = set()
    n = len(raw)
    a = np.frombuffer(raw, dtype=np.uint8)
    v = verdict(kind, raw, k)
    f.add("verdict=" + v)
    closed = raw[-1:] == b"\n"
    if n in sizes(c):
        f.add("n=%d:%s" % (n, "nl" if closed else "open"))
    for pos in np.flatnonzero(a == 10).tolist():
        f.update("nl@" + w for w in _where(pos, c))
    if not closed and n % c.chunk == 0:
        f.add("open_end@chunk")
    if not closed and n % c.span == 0:
        f.add("open_end@span")
    bad = bad_positions(kind, raw)
    if len(bad) == 1 and v in (BAD_BYTE, INVALID):
        if bad[0] == 0:
            f.add("bad@0")
        f.update("bad@" + w for w in _where(bad[0], c) if w.startswith("span"))
        if n % c.chunk and bad[0] == n // c.chunk * c.chunk:
            f.add("bad@tail_chunk_first")
    if v == OK or (kind == "text" and v == SHORT):
        kept = kept_mask(kind, raw, k)
        cs = np.concatenate([[0], np.cumsum(kept)])
        n_spans = (n + c.span - 1) // c.span
        per = [int(cs[min((s + 1) * c.span, n)] - cs[s * c.span]) for s in range(n_spans)]
        if v == OK:
            if n_spans > 1 and per[1] > 0:
                f.add("lead=%d" % (int(cs[c.span]) & 31))
            for s in range(n_spans):
                if 1 <= per[s] and (int(cs[s * c.span]) & 31) + per[s] <= 32:
                    f.add("one_word_span")
                    if s > 0 and s + 1 < n_spans and per[s + 1] > 0:
                        f.add("one_word_span:middle")
                if per[s] == 0 and sum(per[:s]) > 0 and sum(per[s + 1:]) > 0:
                    f.add("empty_span_between")
    if kind == "text" and v != BAD_BYTE:
        for at, ln in zip(line_starts(raw), lines_of(raw)):
            if len(ln) > c.span:
                f.add("line>span")
            for what, _, _ in _straddles(at, at + len(ln), c):
                if len(ln) == k:
                    f.add("lineK@%s_start" % what)
                if len(ln) == k - 1:
                    f.add("short@%s_start" % what)
    if kind == "fasta":
        lines, starts = lines_of(raw), line_starts(raw)
        for i, (at, ln) in enumerate(zip(starts, lines)):
            if i % 2 == 0:
                if not ln:
                    f.update("empty_header@" + w for w in _where(at, c) + (["byte0"] if at == 0 else []))
                if at == c.span:
                    f.add("header@span1_first:" + ("valid" if ln[:1] == b">" else "invalid" if ln[:1] == b"A" else "other"))
                if len(ln) > c.span and all(ch in ln for ch in b"ACGTN") and kept_mask(kind, raw, k)[:at].any() \
                        and kept_mask(kind, raw, k)[at:].any():
                    f.add("header>span_between_kept")
            else:
                if not ln:
                    f.add("empty_read")
                    f.update("empty_read@" + w for w in _where(at, c))
                for m in re.finditer(rb"N+", ln):
                    s, e = at + m.start(), at + m.end()
                    f.update("N@" + w for p in range(s, min(e, s + 2 * c.chunk)) for w in _where(p, c) if w.startswith("chunk"))
                    if e - s == c.chunk and s % c.chunk == 0:
                        f.add("N64@chunk")
                    if e - s > c.span and (s, e) != (at, at + len(ln)):
                        km = kept_mask(kind, raw, k)
                        if km[at:s].any() and km[e:at + len(ln)].any():
                            f.add("Nrun>span_between_kept")
        runs = fasta_runs(raw)
        if runs and v == OK and not any(e - s >= k for s, e in runs):
            f.add("no_long_fragment")
        for s, e in runs:
            ln = e - s
            if ln > c.span:
                f.add("kept_frag>span")
            if (e - 1) // c.chunk - s // c.chunk >= 2:
                f.add("kept_open3" if ln >= k else "dropped_open3")
            if ln < k and _straddles(s, e, c):
                f.add("dropped_open")
            if ln in (k - 1, k, k + 1):
                tag = "frag%+d" % (ln - k)
                if e % c.chunk == 0:
                    f.add(tag + ":end@chunk63")
                if e == c.span:
                    f.add(tag + ":end@span0_last")
                if s % c.chunk == 0:
                    f.add(tag + ":start@chunk0")
                if s == c.span:
                    f.add(tag + ":start@span1_first")
                for what, before, after in _straddles(s, e, c):
                    f.add("%s:straddle_%s:before%d" % (tag, what, before))
                    f.add("%s:straddle_%s:after%d" % (tag, what, after))
    return f


def to_text_facts(strings, k, c):
    f = set()
    ends = np.cumsum([len(s) for s in strings]) - 1
    n_bases = int(ends[-1]) + 1
    if (ends % c.chunk == 0).any():
        f.add("end@bit0")
    if (ends % c.chunk == c.chunk - 1).any():
        f.add("end@bit63")
    if (ends % c.span == c.span - 1).any():
        f.add("end@span_last")
    if n_bases in (63, 64, 65, c.span, c.span + 1):
        f.add("n_bases=%d" % n_bases)
    if k == K_DENSE and all(len(s) == k for s in strings) and n_bases >= c.span + c.chunk:
        f.add("k4_dense")
        # the densest span: span bases + one newline per 4 of them, which kTextLds must hold
        assert c.span + c.span // k <= c.text_lds
    return f


def straddle_ds(ln, k):
    """(side, d): d bases before / after the boundary, d in {1, K - 1}, where the fragment still straddles."""
    return [(side, d) for side in ("before", "after") for d in sorted({1, k - 1}) if 0 < d < ln]


def required(kind, c, k=K):
    """The classes that must be hit by at least one case of a parser."""
    r = {"n=%d:%s" % (v, t) for v in sizes(c) for t in ("nl", "open")}
    r |= {"nl@chunk0", "nl@chunk63", "nl@span0_last", "nl@span1_first", "open_end@chunk", "open_end@span",
          "one_word_span", "bad@0", "bad@span0_last", "bad@span1_first", "bad@tail_chunk_first"}
    r |= {"lead=%d" % v for v in range(32)}
    if kind == "text":
        r |= {"lineK@chunk_start", "lineK@span_start", "short@chunk_start", "short@span_start", "line>span",
              "verdict=short", "verdict=bad_byte", "verdict=ok"}
    else:
        for ln in (k - 1, k, k + 1):
            tag = "frag%+d" % (ln - k)
            r |= {tag + ":end@chunk63", tag + ":start@chunk0", tag + ":end@span0_last", tag + ":start@span1_first"}
            r |= {"%s:straddle_%s:%s%d" % (tag, what, side, d) for what in ("chunk", "span")
                  for side, d in straddle_ds(ln, k)}
        # (K <= 31 < 64: a dropped fragment touches two chunks at the most, so of the fragments open across three
        # or more chunks only the kept one exists; the dropped one is open across one chunk start)
        r |= {"kept_open3", "dropped_open", "kept_frag>span", "N@chunk0", "N@chunk63", "N64@chunk",
              "Nrun>span_between_kept", "header>span_between_kept", "empty_span_between", "one_word_span:middle",
              "header@span1_first:valid", "header@span1_first:invalid", "empty_read", "empty_read@chunk0",
              "empty_read@chunk63", "empty_read@span0_last", "empty_read@span1_first", "empty_header@byte0",
              "empty_header@chunk0", "empty_header@chunk63", "empty_header@span0_last",
              "empty_header@span1_first", "no_long_fragment", "verdict=ok", "verdict=odd", "verdict=invalid"}
    return r


def phase_required(kind, c, k=K):
    """The chunk-edge and span-edge classes: the cases run at every pointer phase must hit all of them."""
    edge = ("nl@", "open_end@", "bad@", "lineK@", "short@", "frag", "N@", "N64@", "empty_", "header@", "one_word",
            "lead=0", "lead=31", "lead=13")
    return {x for x in required(kind, c, k) if x.startswith(edge)}


TO_TEXT_REQUIRED = {"end@bit0", "end@bit63", "end@span_last", "k4_dense"}


def to_text_required(c):
    return TO_TEXT_REQUIRED | {"n_bases=%d" % v for v in (63, 64, 65, c.span, c.span + 1)}


# ---- the cases -----------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind raw k phase")
ToText = namedtuple("ToText", "name strings k")


def text_cases(c=None):
    c = c or constants()
    rng = np.random.default_rng(0x7E47)
    S, C64, k = c.span, c.chunk, K
    out = []

    def add(name, raw, phase=False):
        assert len(raw) <= 3 * S + 2 * C64, name
        out.append(Case("text-" + name, "text", raw, k, phase))

    for v in sizes(c):
        edge = v in (63, 64, 65, S, S + 1, 2 * S)
        add("n%d-nl" % v, t_fill(rng, v, k) if v > k else b"A" * (v - 1) + b"\n", phase=edge)
        add("n%d-open" % v, t_fill(rng, v - k - 3, k) + acgt(rng, k + 3) if v > 2 * k + 4 else b"A" * v, phase=edge)
    add("nl-chunk63", t_fill(rng, 3 * C64, k) + t_fill(rng, 70, k), phase=True)
    add("nl-chunk0", t_fill(rng, 3 * C64 + 1, k) + t_fill(rng, 70, k), phase=True)
    add("nl-span0-last", t_fill(rng, S, k) + t_fill(rng, 100, k), phase=True)
    add("nl-span1-first", t_fill(rng, S + 1, k) + t_fill(rng, 100, k), phase=True)
    add("open-end-chunk", t_fill(rng, 2 * C64 - 20, k) + acgt(rng, 20), phase=True)
    add("open-end-span", t_fill(rng, 2 * S - 31, k) + acgt(rng, 31), phase=True)
    for lead in range(32):
        n_lines = (-lead) % 32 or 32  # base0 of span 1 = span - newlines before it
        if lead % 2:
            raw = t_fill(rng, S - 5, k, n_lines) + acgt(rng, 20) + b"\n" + t_fill(rng, 150, k)
        else:
            raw = t_fill(rng, S, k, n_lines) + t_fill(rng, 150, k)
        add("lead%d" % lead, raw, phase=lead in (0, 13, 31))
    add("one-word-span", t_fill(rng, S - 8, k, 29) + acgt(rng, 18) + b"\n", phase=True)
    body = t_fill(rng, S - 7, k) + acgt(rng, 30) + b"\n" + t_fill(rng, 200, k)
    add("bad-byte0", put(body, 0, b"N"), phase=True)
    add("bad-span0-last", put(body, S - 1, b"a"), phase=True)
    add("bad-span1-first", put(body, S, b">"), phase=True)
    add("bad-tail-chunk", put(t_fill(rng, 2 * C64 - 5, k) + acgt(rng, 15), 2 * C64, b"\r"), phase=True)
    for what, b in (("chunk", 2 * C64), ("span", S)):
        for ln in (k, k - 1):
            for before in (1, 4, ln - 1):
                add("line%d-%s-start-%d" % (ln, what, before),
                    t_fill(rng, b - before, k) + acgt(rng, ln) + b"\n" + t_fill(rng, 50, k), phase=before != 4)
    add("line-over-span", t_fill(rng, 100, k) + acgt(rng, S + 300) + b"\n" + t_fill(rng, 100, k))
    add("line-over-two-spans", t_fill(rng, 70, k) + acgt(rng, 2 * S + 50) + b"\n" + t_fill(rng, 60, k), phase=True)
    return out


def fasta_cases(c=None):
    c = c or constants()
    rng = np.random.default_rng(0xFA57A)
    S, C64, k = c.span, c.chunk, K
    out = []

    def add(name, raw, phase=False):
        assert len(raw) <= 3 * S + 2 * C64, name
        out.append(Case("fasta-" + name, "fasta", raw, k, phase))

    tail = header(5) + acgt(rng, 30) + b"\n"
    for v in sizes(c):
        edge = v in (63, 64, 65, S, S + 1, 2 * S)
        add("n%d-nl" % v, fa_fill(rng, v) if v >= 5 else b"\n", phase=edge)
        add("n%d-open" % v, fa_fill(rng, v + 1)[:-1] if v >= 5 else b">", phase=edge)
    add("n%d-one-read-nl" % (2 * S), fa_place(b"", acgt(rng, 2 * S - 41), 40))  # one read over two spans
    add("header-nl-chunk63", header(C64) + acgt(rng, 100) + b"\n", phase=True)
    add("header-nl-chunk0", header(C64 + 1) + acgt(rng, 100) + b"\n", phase=True)
    add("read-nl-chunk0", fa_place(b"", acgt(rng, 20), 2 * C64 - 20) + tail, phase=True)
    add("read-nl-chunk63", fa_place(b"", acgt(rng, 20), 2 * C64 - 21) + tail, phase=True)
    add("nl-span0-last", fa_place(fa_fill(rng, S - 300), acgt(rng, 50), S - 51) + tail, phase=True)
    add("nl-span1-first", fa_place(fa_fill(rng, S - 300), acgt(rng, 50), S - 50) + tail, phase=True)
    add("open-end-chunk", fa_place(b"", acgt(rng, 30), 2 * C64 - 30)[:-1], phase=True)
    add("open-end-span", fa_place(fa_fill(rng, S - 400), acgt(rng, 100), S - 100)[:-1], phase=True)
    for lead in range(32):
        first = header(3) + acgt(rng, 32 + lead) + b"\n"
        if lead % 2:  # the read of span 1 starts at its first byte (thread 0 reads the newline before it)
            raw = fa_place(first, acgt(rng, 40), S) + tail
        else:  # a kept fragment straddles the span start: 12 bases before it
            raw = fa_place(first, acgt(rng, 40), S - 12) + tail
        add("lead%d" % lead, raw, phase=lead in (0, 13, 20, 31))
    # a span of 12 kept bases that shares its only word with both neighbours
    raw = fa_place(header(4) + acgt(rng, 40) + b"\n", acgt(rng, 12), S + 100)
    add("one-word-span-middle", fa_place(raw, acgt(rng, 20), 2 * S + 50), phase=True)
    body = fa_place(fa_fill(rng, S - 500), acgt(rng, 60), S - 30) + tail
    add("bad-byte0", put(body, 0, b"A"), phase=True)
    add("bad-span0-last", put(body, S - 1, b"a"), phase=True)
    add("bad-span1-first", put(body, S, b">"), phase=True)
    add("bad-tail-chunk", put(fa_place(b"", acgt(rng, 30), 2 * C64, 5), 2 * C64, b"\r"), phase=True)
    # fragments of K - 1, K, K + 1 between two kept neighbours, slid over the chunk and span edges
    for ln in (k - 1, k, k + 1):
        def read_with():
            return acgt(rng, k + 2) + b"N" + acgt(rng, ln) + b"N" + acgt(rng, k + 1)
        off = k + 3
        for what, b, prefix_len in (("chunk", 2 * C64, 0), ("span", S, S - 600)):
            def place(name, start):
                prefix = fa_fill(rng, prefix_len) if prefix_len else b""
                add("frag%d-%s-%s" % (ln, what, name), fa_place(prefix, read_with(), start, off) + tail, phase=True)
            place("end-at-last", b - ln)
            place("start-at-first", b)
            for side, d in straddle_ds(ln, k):
                place("%s%d" % (side, d), b - d if side == "before" else b - (ln - d))
    add("kept-open-4-chunks", fa_place(b"", acgt(rng, 200), 100) + tail, phase=True)
    add("kept-over-span", fa_place(b"", acgt(rng, S + 500), 300) + tail, phase=True)
    add("N-chunk0", fa_place(b"", acgt(rng, 20) + b"N" + acgt(rng, 20), 2 * C64, 20) + tail, phase=True)
    add("N-chunk63", fa_place(b"", acgt(rng, 20) + b"N" + acgt(rng, 20), 2 * C64 - 1, 20) + tail, phase=True)
    add("N64-on-chunk", fa_place(b"", acgt(rng, 15) + b"N" * C64 + acgt(rng, 15), 2 * C64, 15) + tail, phase=True)
    add("N-run-over-span", fa_place(b"", acgt(rng, 30) + b"N" * (S + 100) + acgt(rng, 30), 50) + tail, phase=True)
    add("header-over-span", header(3) + acgt(rng, 30) + b"\n" + header(S + 200) + acgt(rng, 30) + b"\n", phase=True)
    # a whole span without a kept base between two spans that have some
    add("N-run-over-two-spans", fa_place(b"", acgt(rng, 30) + b"N" * (2 * S + 100) + acgt(rng, 30), 50) + tail, phase=True)
    add("header-over-two-spans", header(3) + acgt(rng, 30) + b"\n" + header(2 * S + 100) + acgt(rng, 30) + b"\n",
        phase=True)
    body = fa_place(fa_fill(rng, S - 300), acgt(rng, 40), S - 41) + header(8) + acgt(rng, 20) + b"\n"
    add("header-at-span1-valid", body, phase=True)
    add("header-at-span1-invalid", put(body, S, b"A"), phase=True)
    add("empty-read", header(5) + b"\n" + header(4) + acgt(rng, 12) + b"\n", phase=True)
    add("no-long-fragment", header(4) + b"ACGTNACGTACGNAC\n" + header(2) + b"NNACGTACG\n", phase=True)
    for name, pos in (("chunk0", 2 * C64), ("chunk63", 2 * C64 - 1), ("span0-last", S - 1), ("span1-first", S)):
        add("empty-read-" + name, fa_place(fa_fill(rng, pos - 40) if pos > 200 else b"", b"", pos) + tail, phase=True)
        add("empty-header-" + name, fa_fill(rng, pos) + b"\n" + acgt(rng, 12) + b"\n" + tail, phase=True)
    add("empty-header-byte0", b"\n" + acgt(rng, 12) + b"\n" + tail, phase=True)
    # an odd line count that hangs on the last line: a header after the last read, closed and open
    add("odd-closed-header-last", fa_place(b"", acgt(rng, 30), 2 * C64 - 31) + header(C64), phase=True)
    add("odd-open-header-last", fa_place(fa_fill(rng, S - 300), acgt(rng, 30), S - 31) + b">", phase=True)
    return out


def to_text_cases(c=None):
    c = c or constants()
    rng = np.random.default_rng(0x707E)
    S, k = c.span, K
    out = []

    def add(name, lens, kk=k):
        out.append(ToText("to-text-" + name, [acgt(rng, int(v)) for v in lens], kk))

    add("end-bit0", [65, 20, 43, 64, 11])
    add("end-bit63", [64, 30, 34, 128, 9])
    for n in (63, 64, 65):
        add("n%d-one" % n, [n])
        add("n%d-many" % n, [k, k + 1, n - 2 * k - 1])
    add("n%d-one" % S, [S])
    add("n%d-one" % (S + 1), [S + 1])
    many = [len(x) for x in lines_of(t_fill(rng, S + S // 20, k, S // 20))]  # S bases in S / 20 strings
    add("n%d-many" % S, many)
    add("n%d-many" % (S + 1), many[:-1] + [many[-1] + 1])
    add("end-span-last", many + [k, 40, k + 2])
    add("k4-dense", [K_DENSE] * ((S + c.chunk) // K_DENSE), K_DENSE)
    add("k4-dense-two-spans", [K_DENSE] * (2 * S // K_DENSE + 5), K_DENSE)
    return out


# ---- StreamVByte ---------------------------------------------------------------------------------------------------------
Svb = namedtuple("Svb", "name n pattern seed")
PATTERNS = ("zeros", "big", "widths", "bounds")
BOUNDS = np.array([0, 1, 255, 256, 65535, 65536, 2 ** 32 - 1], dtype=np.uint32)
SPARSE_NONZERO = 100_000


def scan_route(n, c):
    """The route scan_exclusive_i64 takes for n values."""
    if n <= c.scan_small:
        return "small"
    if (n + c.chain_tile - 1) // c.chain_tile <= c.chain_blocks:
        return "chained"
    if (n + c.scan_tile - 1) // c.scan_tile <= c.fix_blocks:
        return "tiled"
    return "recursion"


def svb_group_counts(c):
    t, top = c.chain_tile, c.chain_tile * c.chain_blocks
    above = (top // c.scan_tile + 1) * c.scan_tile  # the first tile edge of the tiled route past the chained maximum
    return [1, 2, c.scan_small, c.scan_small + 1, t - 1, t, t + 1, 2 * t, 3 * t - 1, 3 * t, 3 * t + 1, top, top + 1,
            above - 1, above, above + 1]


def recursion_groups(c):
    return c.fix_blocks * c.scan_tile + 1


def svb_cases(c=None):
    """The dense cases (values() gives the array); every group count runs with n % 4 = 0, 1, 2, 3, the patterns
    rotating over them."""
    c = c or constants()
    out = []
    for i, ng in enumerate(dict.fromkeys(svb_group_counts(c))):
        for r in range(4):
            n = 4 * ng - r
            if n > 0:
                out.append(Svb("g%d-n%d-%s" % (ng, n, PATTERNS[(i + r) % 4]), n, PATTERNS[(i + r) % 4], 1000 * i + r))
    for j, p in enumerate(PATTERNS):  # every pattern at the two regime edges that matter most
        for ng in (c.scan_small + 1, c.chain_tile * c.chain_blocks + 1):
            out.append(Svb("g%d-n%d-%s-all" % (ng, 4 * ng - j, p), 4 * ng - j, p, 77 + j))
    return out


def svb_values(case):
    rng = np.random.default_rng(case.seed)
    n = case.n
    if case.pattern == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if case.pattern == "big":
        return rng.integers(65536, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    if case.pattern == "widths":  # one width per group position, the assignment turning with the seed
        code = (np.arange(n) + case.seed) % 4
        lo = np.array([0, 1, 256, 65536], dtype=np.uint64)[code]
        hi = np.array([1, 256, 65536, 2 ** 32], dtype=np.uint64)[code]
        return (lo + (rng.integers(0, 2 ** 32, size=n, dtype=np.uint64) % (hi - lo))).astype(np.uint32)
    v = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 32, size=n).astype(np.uint32)
    at = rng.random(n) < 0.5
    v[at] = BOUNDS[rng.integers(0, BOUNDS.size, size=int(at.sum()))]
    return v


def svb_sparse_cases(c=None):
    """(name, n, idx, vals): the recursion route, all values zero but SPARSE_NONZERO scattered ones."""
    c = c or constants()
    out = []
    for r in (0, 3):
        n = 4 * recursion_groups(c) - r
        rng = np.random.default_rng(0x5BA5 + r)
        idx = np.unique(np.concatenate([rng.integers(0, n, size=SPARSE_NONZERO), [0, n - 1, 4 * c.scan_tile - 1,
                                                                                  4 * c.scan_tile]]))
        vals = BOUNDS[1:][rng.integers(0, BOUNDS.size - 1, size=idx.size)].copy()
        some = rng.random(idx.size) < 0.5
        vals[some] = rng.integers(1, 2 ** 32, size=int(some.sum()), dtype=np.uint64).astype(np.uint32)
        out.append(("recursion-n%d" % n, n, idx, vals))
    return out

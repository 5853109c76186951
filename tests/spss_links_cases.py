"""Designed inputs of ksh_spss_links, shared by test_spss_links_reference_cpu.py (which asserts by predicate that each
case is what it claims) and test_gpu_spss_links.py: at most a few thousand k-mer positions each, K in
{4, 5, 9, 16, 23, 31}.

A case is a dict: id, k, strings (ACGT, each at least K long), modes (the values of `canonical` the container is legal
for: its end k-mers distinct, in canonical mode after canonicalisation and none its own reverse complement), and
covers: the edge classes the case is there for, every one of which test_spss_links_reference_cpu.py turns into a
predicate on the case.

Most cases are chains: consecutive stretches of one seeded genome that overlap by K - 1 bases, so that every piece
links to the next, some written reverse-complemented.  Where a short K makes a random genome repeat a k-mer, the
builder tries seeds in order until the reference accepts the container (a fixed, repeatable search)."""
import numpy as np

import spss_links_reference as ref
from kmersets import synth

KS = (4, 5, 9, 16, 23, 31)

FIRST_STRADDLES = "a first k-mer across a 64-bit word boundary"
LAST_STRADDLES = "a last k-mer across a 64-bit word boundary"
STARTS_ON_WORD = "a string other than the first begins exactly on a word boundary"
ENDS_PARTIAL = "the last string ends in a partial final word"
ENDS_ON_WORD = "the last string ends exactly at a word end"
SINGLE_BOTH_SIDES = "a one-k-mer string entered as written and reverse-complemented"
ALL_A_END = "the all-A end k-mer, linked to"
ALL_T_END = "the all-T end k-mer as written, linked to"
FOUR_LINKS = "a side with all four links"
ALL_ORIENTATIONS = "links (+,+), (+,-), (-,+) and (-,-)"
CIRCULAR = "a circular string of two or more k-mers linking to itself"
LOOP = "a one-k-mer loop that gives no link"
HAIRPIN = "a hairpin end x -> rc(x) that gives no link"
INTERIOR = "an extension that lands in the interior of another string: no link"
BOTH_MODES = "the same strings in canonical and non-canonical mode"
NO_LINKS = "strings but no links at all"
EMPTY = "no strings"
SINGLE_STRING = "a single string"
OVER_256 = "more than 256 strings"
THOUSANDS = "several thousand strings"
RANDOM = "seeded random pieces and orientations"
HAS_LINKS = "at least one link"


def legal(strings, k, canonical):
    try:
        ref.check_container(strings, k, canonical)
    except ValueError:
        return False
    kmers = ref.kmers_of(strings, k)
    keys = [ref.canon(x) for x in kmers] if canonical else kmers
    return len(set(keys)) == len(keys)


def chain(k, sizes, flips, seed, gaps=()):
    """Piece i has sizes[i] k-mer positions of one seeded genome; it overlaps piece i - 1 by K - 1 bases unless i is in
    gaps (then K positions are left out between them); flips[i] writes it reverse-complemented."""
    text = synth.string_of_bases(synth.random_genome(sum(sizes) + k * (len(gaps) + 1), seed))
    out, p = [], 0
    for i, size in enumerate(sizes):
        if i in gaps:
            p += k
        piece = text[p:p + size + k - 1]
        out.append(ref.rc(piece) if flips[i] else piece)
        p += size
    return out


def search(build, k, modes, seed):
    """build(seed) for the first seed from `seed` on whose container is legal in every mode."""
    for s in range(seed, seed + 2000):
        strings = build(s)
        if all(legal(strings, k, m) for m in modes):
            return strings
    raise AssertionError("no legal container from seed %d" % seed)


def case(cid, k, strings, modes, covers):
    assert all(legal(strings, k, m) for m in modes), cid
    return {"id": "%s-k%d" % (cid, k), "k": k, "strings": list(strings), "modes": tuple(modes),
            "covers": tuple(covers)}


def _modes(k):
    """Both: where K is even the seed search passes over containers with a palindromic end."""
    return (True, False)


def _word_edges(k, partial):
    """String 1 begins at base 64; string 2 at base 125 (phase 29: its first k-mer crosses into the next word) and its
    last k-mer begins at phase 30; the last string is sized so that the stream ends on a word end, or 5 bases on."""
    sizes = [64 - (k - 1), 61 - (k - 1), 34]
    used = 125 + 34 + k - 1
    size3 = (-(used + k - 1)) % 32
    size3 += 32 if size3 < 2 else 0
    sizes.append(size3 + (5 if partial else 0))
    build = lambda seed: chain(k, sizes, [0, 0, 0, 1], seed)  # noqa: E731
    covers = [FIRST_STRADDLES, LAST_STRADDLES, STARTS_ON_WORD, ENDS_PARTIAL if partial else ENDS_ON_WORD, HAS_LINKS,
              BOTH_MODES]
    return case("word_edges_%s" % ("partial" if partial else "whole"), k, search(build, k, _modes(k), 300 + k),
                _modes(k), covers)


def _orientations(k):
    """A -> B (+,+), B -> C' (+,-), C' -> D' (-,-), D' -> E (-,+), and a one-k-mer string between two long ones, once
    as written and once flipped."""
    sizes = [7, 5, 6, 4, 9, 1, 8, 1, 6]
    flips = [0, 0, 1, 1, 0, 0, 0, 1, 1]
    build = lambda seed: chain(k, sizes, flips, seed)  # noqa: E731
    return case("orientations", k, search(build, k, _modes(k), 400 + k), _modes(k),
                [ALL_ORIENTATIONS, SINGLE_BOTH_SIDES, HAS_LINKS, BOTH_MODES])


def _poly(k, base):
    """... C A^(K-1) | A^K | A^(K-1) C ...: the one-k-mer string A^K is linked to and links on, and follows itself
    (the loop gives no link).  base T: the same strings reverse-complemented as written."""
    a = "A" * k

    def build(seed):
        tail = synth.string_of_bases(synth.random_genome(2 * k + 6, seed))
        strings = [tail[:k + 1] + "C" + a[:k - 1], a, a[:k - 1] + "C" + tail[k + 1:]]
        return [ref.rc(s) for s in strings] if base == "T" else strings

    modes = (True, False)
    return case("poly_%s" % base, k, search(build, k, modes, 500 + k), modes,
                [ALL_A_END if base == "A" else ALL_T_END, LOOP, HAS_LINKS, BOTH_MODES])


def _four_links(k):
    """One string, and four that begin with its last K - 1 bases and one base each."""
    def build(seed):
        t = synth.string_of_bases(synth.random_genome(k + 3 + 4 * 3, seed))
        head = t[:k + 3]
        return [head] + [head[-(k - 1):] + b + t[k + 3 + 3 * i:k + 6 + 3 * i] for i, b in enumerate("ACGT")]

    return case("four_links", k, search(build, k, (True, False), 600 + k), (True, False), [FOUR_LINKS, HAS_LINKS])


def _circular(k):
    def build(seed):
        t = synth.string_of_bases(synth.random_genome(3 * k + 40, seed))
        ring = t[:k + 17]
        return [t[k + 17:2 * k + 30], ring + ring[:k - 1], ref.rc(t[2 * k + 30:])]

    return case("circular", k, search(build, k, _modes(k), 700 + k), _modes(k), [CIRCULAR, HAS_LINKS, BOTH_MODES])


def _hairpin():
    """K = 5: the string ends in CACGT, whose last four bases are their own reverse complement: CACGT + G is
    rc(CACGT), the first k-mer of the reverse-complemented string."""
    return case("hairpin", 5, ["GGACACGT", "TTAGC"], (True,), [HAIRPIN])


def _interior(k):
    """The second string ends in K - 1 bases from the middle of the first: its extension is a k-mer inside."""
    def build(seed):
        t = synth.string_of_bases(synth.random_genome(4 * k + 30, seed))
        long = t[:2 * k + 20]
        at = k // 2 + 3
        return [long, t[2 * k + 20:3 * k + 25] + long[at:at + k - 1], t[3 * k + 25:]]

    return case("interior", k, search(build, k, _modes(k), 800 + k), _modes(k), [INTERIOR, NO_LINKS])


def _no_links(k):
    sizes = [5, 1, 30, 2, 1, 12]
    build = lambda seed: chain(k, sizes, [0, 1, 0, 0, 1, 1], seed, gaps=(1, 2, 3, 4, 5))  # noqa: E731
    return case("no_links", k, search(build, k, _modes(k), 900 + k), _modes(k), [NO_LINKS, BOTH_MODES])


def _single(k):
    build = lambda seed: chain(k, [40], [0], seed)  # noqa: E731
    return case("single", k, search(build, k, _modes(k), 1000 + k), _modes(k), [SINGLE_STRING, NO_LINKS])


def _many(k, n, cid, covers, seed):
    """n pieces of 1 .. 3 positions (a third of them one k-mer long), a gap before every 50th, seeded flips."""
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.integers(1, 4, size=n)]
    flips = [int(x) for x in rng.integers(0, 2, size=n)]
    build = lambda s: chain(k, sizes, flips, s, gaps=tuple(range(50, n, 50)))  # noqa: E731
    return case(cid, k, search(build, k, _modes(k), seed), _modes(k), list(covers) + [HAS_LINKS, BOTH_MODES])


def _random(k, seed):
    rng = np.random.default_rng(seed)
    n = 60 if k <= 9 else 200
    sizes = [int(x) for x in np.minimum(rng.geometric(0.3 if k <= 9 else 0.1, size=n), 60)]
    flips = [int(x) for x in rng.integers(0, 2, size=n)]
    gaps = tuple(int(i) for i in np.flatnonzero(rng.random(n) < 0.15) if i > 0)
    build = lambda s: chain(k, sizes, flips, s, gaps=gaps)  # noqa: E731
    return case("random_%d" % seed, k, search(build, k, _modes(k), seed), _modes(k), [RANDOM, HAS_LINKS, BOTH_MODES])


def _small4():
    """K = 4 leaves 120 canonical k-mers that are not their own reverse complement: a chain of three short pieces."""
    build = lambda seed: chain(4, [3, 1, 2], [0, 1, 0], seed)  # noqa: E731
    return case("chain", 4, search(build, 4, (True, False), 1600), (True, False),
                [SINGLE_BOTH_SIDES, HAS_LINKS, BOTH_MODES])


def _build():
    out = [case("empty", 23, [], (True, False), [EMPTY])]
    for k in (9, 16, 23, 31):
        out += [_word_edges(k, False), _word_edges(k, True)]
    for k in (5, 9, 16, 23, 31):
        out.append(_orientations(k))
    for k in (5, 16, 31):
        out += [_poly(k, "A"), _poly(k, "T")]
    out += [_four_links(5), _four_links(9), _hairpin()]
    for k in (9, 23):
        out += [_circular(k), _interior(k)]
    for k in (9, 31):
        out += [_no_links(k), _single(k)]
    out.append(case("tiny", 4, ["AACCG", "ACCGT"[1:] + "A"], (True, False), [HAS_LINKS, BOTH_MODES]))
    out.append(_small4())
    out.append(_many(23, 300, "many_300", [OVER_256], 1100))
    out.append(_many(31, 3000, "many_3000", [OVER_256, THOUSANDS], 1200))
    out.append(_many(16, 1000, "many_1000", [OVER_256], 1300))
    out += [_random(9, 1400), _random(23, 1500)]
    return out


CASES = _build()

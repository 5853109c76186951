"""Designed inputs of ksh_spss_cut, shared by test_spss_cut_reference_cpu.py (which asserts by predicate that each case
is what it claims) and test_gpu_spss_cut.py: a few thousand k-mer positions each, at K in {4, 9, 16, 23, 31}.

A case is a dict: id, k, strings (ACGT, each at least K long), offsets int64[n + 1] and start int32[n_runs] (a run list
as ksh_seq_class_runs writes it), and covers: the edge classes the case is there for, every one of which
test_spss_cut_reference_cpu.py turns into a predicate on the case.

Terms: output string r begins at output base B[r]; its bases are the input bases at the same index
minus shift[r] = (r - s)(K - 1); a string's phase is B[r] mod 32.  shift[r] mod 32 only takes multiples of
gcd(K - 1, 32), so "every shift" means every such multiple: all of 0..31 at K = 4 and K = 16 (K - 1 odd), the even
values at K = 23 and 31, the multiples of 8 at K = 9."""
import numpy as np

from kmersets import synth

KS = (4, 9, 16, 23, 31)

NO_CUT = "no cut: n_runs == n_strings"
EVERY_POSITION = "every position its own run: all output strings K long"
EIGHT_IN_A_WORD = "eight output strings begin in one word"
PIECE_IN_WORD = "a piece within one output word"
PIECE_ONE_BOUNDARY = "a piece across exactly one output word boundary"
PIECE_THREE_BOUNDARIES = "a piece across three or more output word boundaries"
EVERY_SHIFT = "every reachable shift mod 32"
EVERY_PHASE = "every output phase 0..31"
EMPTY_LENS_BETWEEN_LONG = "strings with lens == 0 between long strings"
BOUNDARY_ON_INPUT_WORD = "a string boundary on an input word boundary"
BOUNDARY_ON_OUTPUT_WORD = "a string boundary on an output word boundary and on no input word boundary"
OUT_MULTIPLE = "n_bases_out a multiple of 32"
OUT_MULTIPLE_PLUS = "n_bases_out a multiple of 32, plus 1"
OUT_MULTIPLE_MINUS = "n_bases_out a multiple of 32, minus 1"
SINGLE = "a single string with a single run"
EMPTY = "no strings"
RANDOM = "200 strings of geometric lengths, seeded cuts"
HAS_CUT = "more output strings than input strings"
HAS_LONG_PIECE = "an output string longer than K"


def _strings(k, sizes, seed):
    """Strings of sizes[s] positions each: consecutive, non-overlapping stretches of one seeded genome."""
    lengths = [int(p) + k - 1 for p in sizes]
    text = synth.string_of_bases(synth.random_genome(sum(lengths), seed))
    ends = np.cumsum(lengths)
    return [text[int(e) - n:int(e)] for e, n in zip(ends, lengths)]


def make_case(cid, k, sizes, cuts, covers, seed):
    """cuts[s]: the ascending positions 1 .. sizes[s] - 1 of string s at which a new run starts."""
    assert len(sizes) == len(cuts)
    for p, c in zip(sizes, cuts):
        assert list(c) == sorted(set(int(x) for x in c)) and all(0 < int(x) < p for x in c)
    starts = [[0] + [int(x) for x in c] for c in cuts]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in starts])]).astype(np.int64)
    start = np.array([x for row in starts for x in row], dtype=np.int32)
    return {"id": "%s-k%d" % (cid, k), "k": k, "strings": _strings(k, sizes, seed), "offsets": offsets, "start": start,
            "covers": tuple(covers)}


def _runs_to_cuts(run_sizes):
    return [int(x) for x in np.cumsum(run_sizes)[:-1]]


def _no_cut(k):
    sizes = [900, 1, 1, 33, 64, 1200, 1, 700, 2, 31]
    return make_case("no_cut", k, sizes, [[] for _ in sizes], [NO_CUT, EMPTY_LENS_BETWEEN_LONG], 100 + k)


def _every_position(k):
    sizes = [700, 1, 1, 900, 2, 400]
    covers = [EVERY_POSITION, HAS_CUT] + ([EIGHT_IN_A_WORD] if k == 4 else [])
    return make_case("every_position", k, sizes, [list(range(1, p)) for p in sizes], covers, 200 + k)


def _one_long(k):
    """One string of about 3000 positions.  Its first run is one position (a piece of K <= 32 bases at phase 0: within
    a word).  Every later run has 1 .. 32 positions, every eighth 100 .. 131 (across three boundaries and more), the
    very number chosen so that the NEXT string's phase is 7 r mod 32: the phases go round all 32 values three times,
    and with more than 32 runs r (K - 1) mod 32 takes every value it can."""
    runs, at = [1], k
    while sum(runs) < 3000:
        r = len(runs)
        least = 100 if r % 8 == 0 else 1
        size = next(n for n in range(least, least + 32) if (at + n + k - 1) % 32 == (7 * (r + 1)) % 32)
        runs.append(size)
        at += size + k - 1
    covers = [PIECE_IN_WORD, PIECE_ONE_BOUNDARY, PIECE_THREE_BOUNDARIES, EVERY_SHIFT, EVERY_PHASE, HAS_CUT,
              HAS_LONG_PIECE]
    return make_case("one_long", k, [sum(runs)], [_runs_to_cuts(runs)], covers, 300 + k)


def _short_between_long(k):
    """long A, three strings of one position, long B, one of one position, long C, two of one position, long D.
    A is 160 bases long, so string 1 begins on an input word boundary.  Three cuts lie before C (two in A, one in B),
    3 (K - 1) is no multiple of 32 at any K of KS, and B's length is chosen so that C begins on an OUTPUT word
    boundary: input start of C + 3 (K - 1) = 0 mod 32."""
    a = 160 - (k - 1)
    assert (3 * (k - 1)) % 32 != 0
    before_b = 160 + 3 * k
    b = next(p for p in range(600, 632) if (before_b + p + k - 1 + k + 3 * (k - 1)) % 32 == 0)
    sizes = [a, 1, 1, 1, b, 1, 700, 1, 1, 900]
    cuts = [[40, 41], [], [], [], [333], [], [5, 64, 65, 300], [], [], [1, 450, 899]]
    covers = [EMPTY_LENS_BETWEEN_LONG, BOUNDARY_ON_INPUT_WORD, BOUNDARY_ON_OUTPUT_WORD, HAS_CUT, HAS_LONG_PIECE]
    return make_case("short_between_long", k, sizes, cuts, covers, 400 + k)


def _stream_edge(k, delta, cover):
    """n_bases_out = a multiple of 32, plus delta: the last string's length settles it."""
    sizes = [500, 1, 800, 77]
    cuts = [[100, 101, 350], [], [400], [10]]
    n_cuts = sum(len(c) for c in cuts)
    fixed = sum(p + k - 1 for p in sizes) + (k - 1) + n_cuts * (k - 1)
    last = next(p for p in range(640, 672) if (fixed + p) % 32 == delta % 32)
    return make_case("stream_edge%+d" % delta, k, sizes + [last], cuts + [[]], [cover, HAS_CUT, HAS_LONG_PIECE], 500 + k)


def _single(k):
    return make_case("single", k, [50], [[]], [SINGLE, NO_CUT], 600 + k)


def _empty(k):
    return {"id": "empty-k%d" % k, "k": k, "strings": [], "offsets": np.zeros(1, dtype=np.int64),
            "start": np.zeros(0, dtype=np.int32), "covers": (EMPTY,)}


def _random(k, p_cut, seed):
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.geometric(1.0 / 15, size=200)]
    cuts = [[int(x) for x in 1 + np.flatnonzero(rng.random(p - 1) < p_cut)] for p in sizes]
    return make_case("random_p%g" % p_cut, k, sizes, cuts, [RANDOM, HAS_CUT, HAS_LONG_PIECE], seed)


def _build():
    out = []
    for k in KS:
        out += [_no_cut(k), _every_position(k), _one_long(k), _short_between_long(k),
                _stream_edge(k, 0, OUT_MULTIPLE), _stream_edge(k, 1, OUT_MULTIPLE_PLUS),
                _stream_edge(k, -1, OUT_MULTIPLE_MINUS), _single(k), _random(k, 0.02, 700 + k),
                _random(k, 0.5, 800 + k)]
    out.append(_empty(23))
    return out


CASES = _build()
EDGE_CLASSES = (NO_CUT, EVERY_POSITION, EIGHT_IN_A_WORD, PIECE_IN_WORD, PIECE_ONE_BOUNDARY, PIECE_THREE_BOUNDARIES,
                EVERY_SHIFT, EVERY_PHASE, EMPTY_LENS_BETWEEN_LONG, BOUNDARY_ON_INPUT_WORD, BOUNDARY_ON_OUTPUT_WORD,
                OUT_MULTIPLE, OUT_MULTIPLE_PLUS, OUT_MULTIPLE_MINUS, SINGLE, EMPTY, RANDOM, HAS_CUT, HAS_LONG_PIECE)

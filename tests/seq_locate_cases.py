"""Designed containers for ksh_seq_locate (csrc/ksh_locate.hip): each case aims at one edge of the scan, of the end
table or of the definition, and lists it.  R (positions per thread of the scan) and the workgroup's size are read
from the kernel's text, so the boundaries move with them.

A case is {"id", "k", "strings", "reference", "edge", "expect"}: expect[canonical][e] = (sequence, position, strand,
count) claimed of end e in that mode, (-1, -1, -1, 0) for an end that is nowhere.  tests/test_seq_locate_model_cpu.py
holds every claim against tests/seq_locate_reference.py; tests/test_gpu_seq_locate.py runs the cases on the device."""
import os
import re

import numpy as np

import hash_table_cases as hc
from seq_locate_reference import rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc", "ksh_locate.hip")
KS = (15, 16, 23, 31)
NOWHERE = (-1, -1, -1, 0)


def kernel_constants(text=None):
    """(R, threads of a workgroup) as csrc/ksh_locate.hip states them, each exactly once."""
    text = open(SOURCE).read() if text is None else text
    out = []
    for name in ("kLocRun", "kLocThreads"):
        found = re.findall(r"^constexpr int %s = (\d+);" % name, text, flags=re.M)
        assert len(found) == 1, "%s is stated %d times" % (name, len(found))
        out.append(int(found[0]))
    return tuple(out)


R, THREADS = kernel_constants()
BLOCK = R * THREADS  # positions per workgroup


def rnd(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def seq_of_positions(rng, k, positions):
    return rnd(rng, positions + k - 1)


def slots_of(n_strings):
    """The end table of n strings: the next power of two >= 4 n."""
    slots = 1
    while slots < 4 * n_strings:
        slots <<= 1
    return slots


def case(cid, k, strings, reference, edge, expect):
    per_mode = bool(expect) and all(isinstance(key, bool) for key in expect)  # (keyed by the canonical flag, or by end)
    both = {m: dict(expect[m] if per_mode else expect) for m in (True, False)}
    return {"id": "%s-k%d" % (cid, k), "k": k, "strings": list(strings), "reference": list(reference), "edge": edge,
            "expect": both}


# ---- where the sequence boundaries fall --------------------------------------------------------------------------
def boundaries(k):
    """Sequences whose first positions are the global positions R - 1, R, R + 1, 256 R - 1, 256 R, 256 R + 1; the
    strings are the sequences themselves, so every sequence is hit at its first and at its last position."""
    rng = np.random.default_rng(100 + k)
    starts = [0, R - 1, R, R + 1, BLOCK - 1, BLOCK, BLOCK + 1, BLOCK + 2 * R + 3]
    counts = np.diff(starts).tolist() + [R + 5]
    reference = [seq_of_positions(rng, k, c) for c in counts]
    expect = {}
    for s, c in enumerate(counts):
        expect[2 * s], expect[2 * s + 1] = (s, 0, 0, 1), (s, c - 1, 0, 1)
    return case("boundaries", k, reference, reference,
                "sequences start at global positions R - 1, R, R + 1, 256 R - 1, 256 R, 256 R + 1; hits at the first "
                "and the last position of every sequence", expect)


def exact_k(k):
    rng = np.random.default_rng(200 + k)
    reference = [rnd(rng, k + 20), rnd(rng, k), rnd(rng, k + 7)]
    return case("exact-k", k, [reference[1]], reference, "a sequence of exactly K bases between two longer ones",
                {0: (1, 0, 0, 1), 1: (1, 0, 0, 1)})


def one_position_runs(k):
    """3 R sequences of one position each behind a sequence of 5 positions: whole runs of the scan start a sequence
    at every position."""
    rng = np.random.default_rng(300 + k)
    reference = [seq_of_positions(rng, k, 5)] + [rnd(rng, k) for _ in range(3 * R)] + [seq_of_positions(rng, k, 4)]
    picks = [1, 2, R, R + 1, 2 * R, 3 * R]
    expect = {}
    for i, r in enumerate(picks):
        expect[2 * i] = expect[2 * i + 1] = (r, 0, 0, 1)
    return case("one-position-runs", k, [reference[r] for r in picks], reference,
                "many one-position sequences in a row inside one run", expect)


def word_edges(k):
    """Hits at the base offsets where a window starts a word, ends one, or just does and does not cross into the
    next: one reference sequence, so the base offset of a position is the position."""
    rng = np.random.default_rng(400 + k)
    reference = [rnd(rng, 150)]
    offsets = sorted({0, 31, 32 - k, 33 - k, 32, 63, 64 - k, 65 - k, 64, 150 - k})
    strings = [reference[0][b:b + k] for b in offsets]
    expect = {}
    for i, b in enumerate(offsets):
        expect[2 * i] = expect[2 * i + 1] = (0, b, 0, 1)
    return case("word-edges", k, strings, reference,
                "hits at base offsets 0, 31, 32 - K, 33 - K (and a word on), and at the last position", expect)


def across_boundary(k):
    rng = np.random.default_rng(500 + k)
    a, b = rnd(rng, k + 11), rnd(rng, k + 9)
    j = k // 2
    planted = a[-j:] + b[:k - j]  # adjacent in the base stream, in no sequence
    return case("across-boundary", k, [planted, a[-k:]], [a, b],
                "an end k-mer that spans a sequence boundary of the base stream must not match",
                {0: NOWHERE, 1: NOWHERE, 2: (0, 11, 0, 1), 3: (0, 11, 0, 1)})


# ---- strands and counts ------------------------------------------------------------------------------------------
def rc_only(k):
    rng = np.random.default_rng(600 + k)
    y = rnd(rng, k)
    reference = [rnd(rng, 37), rnd(rng, 20) + rc(y) + rnd(rng, 13)]
    at = (1, 20, 1, 1)
    return case("rc-only", k, [y], reference, "the end occurs only as its reverse complement: strand 1; in "
                "non-canonical mode it is nowhere", {True: {0: at, 1: at}, False: {0: NOWHERE, 1: NOWHERE}})


def both_strands(k):
    """y first as written and later reverse-complemented; z the other way round."""
    rng = np.random.default_rng(700 + k)
    y, z = rnd(rng, k), rnd(rng, k)
    text = rnd(rng, 9) + y + rnd(rng, 5) + rc(z) + rnd(rng, 17) + rc(y) + rnd(rng, 3) + z + rnd(rng, 8)
    py, prz, pry, pz = 9, 14 + k, 31 + 2 * k, 34 + 3 * k
    assert text[py:py + k] == y and text[prz:prz + k] == rc(z) and text[pry:pry + k] == rc(y) and text[pz:pz + k] == z
    return case("both-strands", k, [y, z], [rnd(rng, k + 2), text],
                "occurrences on both strands, the smaller position on either; the reverse-complement ones vanish in "
                "non-canonical mode",
                {True: {0: (1, py, 0, 2), 1: (1, py, 0, 2), 2: (1, prz, 1, 2), 3: (1, prz, 1, 2)},
                 False: {0: (1, py, 0, 1), 1: (1, py, 0, 1), 2: (1, pz, 0, 1), 3: (1, pz, 0, 1)}})


def homopolymer(k):
    reference = ["A" * (k + 40), "T" * (k + 9)]
    return case("homopolymer", k, ["A" * k, "T" * k, "A" * (k + 3)], reference,
                "a homopolymer reference against the all-A end: the key is 0, the count is the number of positions",
                {True: {0: (0, 0, 0, 51), 1: (0, 0, 0, 51), 2: (0, 0, 1, 51), 3: (0, 0, 1, 51), 4: (0, 0, 0, 51),
                        5: (0, 0, 0, 51)},
                 False: {0: (0, 0, 0, 41), 1: (0, 0, 0, 41), 2: (1, 0, 0, 10), 3: (1, 0, 0, 10), 4: (0, 0, 0, 41),
                         5: (0, 0, 0, 41)}})


def self_rc(k):
    assert k % 2 == 0
    rng = np.random.default_rng(800 + k)
    half = rnd(rng, k // 2)
    y = half + rc(half)
    assert rc(y) == y
    text = rnd(rng, 6) + y + rnd(rng, 21) + y + rnd(rng, 4)
    at = (0, 6, 0, 2)
    return case("self-rc", k, [y, text[:6 + k]], [text], "an end that is its own reverse complement: strand 0, every "
                "occurrence counted once", {0: at, 1: at, 3: at})


def duplicate_ends(k):
    """One-k-mer strings, two strings with the same first k-mer, and an end that is another string's end
    reverse-complemented."""
    rng = np.random.default_rng(900 + k)
    y, z = rnd(rng, k), rnd(rng, k)
    s0 = y                       # one k-mer: both ends are y
    s1 = y + rnd(rng, 6)         # the same first k-mer
    s2 = rnd(rng, 4) + rc(y)     # its last k-mer is rc(y)
    s3 = z + rnd(rng, 3) + z     # first and last k-mer alike
    reference = [rnd(rng, 12) + y + rnd(rng, 9), rnd(rng, 3) + z + rnd(rng, 30)]
    fy, fz = (0, 12, 0, 1), (1, 3, 0, 1)
    return case("duplicate-ends", k, [s0, s1, s2, s3], reference,
                "ends that are not distinct: a one-k-mer string, two strings with one first k-mer, an end that is "
                "another's reverse complement, a string that ends as it starts",
                {True: {0: fy, 1: fy, 2: fy, 5: (0, 12, 1, 1), 6: fz, 7: fz},
                 False: {0: fy, 1: fy, 2: fy, 5: NOWHERE, 6: fz, 7: fz}})


# ---- the end table -----------------------------------------------------------------------------------------------
def smallest_table(k):
    rng = np.random.default_rng(1000 + k)
    s = rnd(rng, k + 25)
    reference = [rnd(rng, 40), s[3:] + rnd(rng, 4), rnd(rng, 8) + s[:k + 2]]
    return case("n1", k, [s], reference, "n = 1: a table of 4 slots", {0: (2, 8, 0, 1), 1: (1, 22, 0, 1)})


def _canonical_pool(k, seed, size=6000):
    """Random k-mers that are their own canonical form, so their key is the same in both modes."""
    rng = np.random.default_rng(seed)
    pool = []
    while len(pool) < size:
        y = rnd(rng, k)
        if y < rc(y):
            pool.append(y)
    return sorted(set(pool))


def _table_case(cid, k, home_of_run, edge, seed):
    """8 one-k-mer strings (32 slots): `run` of them with one home, an absent k-mer of the reference with that home
    too, the others with homes away from the run."""
    n, run = 8, 4
    slots = slots_of(n)
    pool = _canonical_pool(k, seed)
    homes = hc.link_homes(np.array([hc.kmer_int(y) for y in pool], dtype=np.uint64), slots)
    home = home_of_run(homes, slots)
    same = [y for y, h in zip(pool, homes) if h == home]
    assert len(same) >= run + 1
    away = {y for y, h in zip(pool, homes) if (h - home) % slots > run + 2 and (home - h) % slots > n}
    colliding, absent = same[:run], same[run]
    others, seen = [], set()
    for y, h in zip(pool, homes):  # each with a home of its own: nothing else grows the run
        if y in away and h not in seen:
            others.append(y)
            seen.add(int(h))
        if len(others) == n - run:
            break
    strings = colliding + others
    rng = np.random.default_rng(seed + 1)
    reference = [absent] + strings[::-1] + [rnd(rng, 12) + absent + colliding[2] + rnd(rng, 5)]
    expect = {}
    for s in range(n):
        expect[2 * s] = expect[2 * s + 1] = (n - s, 0, 0, 2 if s == 2 else 1)
    c = case(cid, k, strings, reference, edge, expect)
    c["table"] = {"slots": slots, "home": int(home), "run": run, "absent": absent}
    return c


def colliding_run(k):
    return _table_case("colliding-run", k, lambda homes, slots: 5,
                       "four ends with one home and an absent k-mer of the reference behind the full run", 1100 + k)


def wrapping_run(k):
    return _table_case("wrap", k, lambda homes, slots: slots - 1,
                       "four ends whose home is the last slot: the probe wraps to slot 0, an absent k-mer follows it",
                       1200 + k)


# ---- degenerate inputs -------------------------------------------------------------------------------------------
def no_strings(k):
    rng = np.random.default_rng(1300 + k)
    return case("no-strings", k, [], [rnd(rng, 50)], "no strings: nothing is written", {})


def no_reference(k):
    rng = np.random.default_rng(1400 + k)
    strings = [rnd(rng, k + 3), rnd(rng, k)]
    return case("no-reference", k, strings, [], "no reference sequences: -1 and 0 everywhere",
                {e: NOWHERE for e in range(4)})


def no_hit(k):
    rng = np.random.default_rng(1500 + k)
    strings = [rnd(rng, k + i) for i in range(5)]
    return case("no-hit", k, strings, [rnd(rng, 3 * R + k), rnd(rng, k)], "a reference with no hit at all",
                {e: NOWHERE for e in range(10)})


BUILDERS = (boundaries, exact_k, one_position_runs, word_edges, across_boundary, rc_only, both_strands, homopolymer,
            duplicate_ends, smallest_table, colliding_run, wrapping_run, no_strings, no_reference, no_hit)


def _cases():
    out = [build(k) for build in BUILDERS for k in KS]
    out.append(self_rc(16))
    assert len({c["id"] for c in out}) == len(out)
    return out


CASES = _cases()
SMALL = [c for c in CASES if sum(len(t) for t in c["reference"]) <= 400]  # (brute force compares all pairs)

"""Cases for the per-bucket sort of the decode and the k-mer count (k_bucket_sort, csrc/ksh_decode.hip) and a numpy
model of the branches it takes.

A *case* is a multiset of k-mers that aims at one *target* bucket of the sort: its size, the skew of its keys or its
runs of equal keys sit where the kernel takes another branch.  Both neighbouring buckets hold a few distinct keys,
key 0 and the all-ones key among them, so a sort that leaves its range shows as a wrong neighbour.  pack_kmers
turns the multiset into a container of one string of exactly K bases per k-mer, in a seeded shuffled order; decoded
with canonical=False the decoder sees exactly that multiset.  On the wide route (N > kCoarseBits) the sort's bucket is
the coarse bucket (the top kCoarseBits bits of the k-mer) and its key the composite of 2K - kCoarseBits bits, in the
composite's type.

The model (lds_plan, partition_plan, bucket_branches) restates the kernel's arithmetic: it says which branches a
case takes, so that the GPU test (tests/test_gpu_bucket_sort.py) can assert what it is testing and the CPU test
(tests/test_bucket_sort_model_cpu.py) that every branch is reached.  It is never the expected answer: that is
np.unique on the 64-bit k-mers (reference).  The constants are read from the text of ksh_decode.hip, so a changed
constant fails the CPU test instead of moving the cases off the thresholds silently."""
import os
import re
from collections import namedtuple

import numpy as np

from kmersets import synth

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_HIP = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc", "ksh_decode.hip")

BRANCHES = ("regs", "stream", "lds_bitonic", "partition", "part_lds_bitonic", "global_bitonic", "drops",
            "cutoff_straddle", "run_at_end")
CUTOFFS = (0, 1, 2, 3, 255)
ORACLE_MAX = 20000  # occurrences up to which the CPU test feeds a case to the oracle's KmerCounter

Geom = namedtuple("Geom", "route k n kb")
GEOMS = (Geom("plain", 11, 8, 2), Geom("plain", 19, 8, 4), Geom("plain", 23, 14, 4), Geom("plain", 25, 8, 8),
         Geom("plain", 31, 14, 8), Geom("wide", 23, 20, 4), Geom("wide", 17, 20, 2), Geom("wide", 31, 16, 8))
BIG_GEOM = Geom("plain", 31, 14, 8)
FAMILIES = ("uniform", "threshold", "clustered", "heavy", "runs", "reads")

Cfg = namedtuple("Cfg", "kSortLdsBytes kMaxSubBits kSortThreads kSortRegs kCoarseBits sub_limit part_div")


def geom_id(g):
    return "%s-%d-%d-%d" % g


# ---- constants from the kernel's text -------------------------------------------------------------------------------
def constants(text=None):
    """Cfg from ksh_decode.hip; the lines the model restates must stand there as written."""
    if text is None:
        text = open(DECODE_HIP).read()

    def num(pattern):
        m = re.search(pattern, text)
        if m is None:
            raise AssertionError("ksh_decode.hip no longer has what the model reads: " + pattern)
        return int(m.group(1))

    cfg = Cfg(num(r"constexpr int kSortLdsBytes = (\d+);"), num(r"constexpr int kMaxSubBits = (\d+);"),
              num(r"constexpr int kSortThreads = (\d+);"), num(r"constexpr int kSortRegs = (\d+);"),
              num(r"constexpr int kCoarseBits = (\d+);"), num(r"if \(s1 - s0 > (\d+)\) \{"),
              num(r"while \(\(cnt64 >> bits\) > kCap / (\d+) && bits < kMaxSubBits\) bits\+\+;"))
    for line in ("constexpr int kCap = kSortLdsBytes / int(sizeof(KeyT));",
                 "while ((4 << bits) < cnt && bits < kMaxSubBits) bits++;",
                 "if (bits > eff_bits) bits = eff_bits;",
                 "const int shift = eff_bits - bits;",
                 "const bool in_regs = cnt <= kSortRegs * kSortThreads;",
                 "if (cnt64 <= kCap) {",
                 "int bits = 1;",
                 "if (bits > key_bits) bits = key_bits;",
                 "const int shift = key_bits - bits;",
                 "if (pc <= kCap) {",
                 "block_sort_into_lds(tmp + s0, int(pc), shift, lds, &sh);",
                 "const int per = (cnt + kSortThreads - 1) / kSortThreads;",
                 "if (max_bucket > int64_t(kSortLdsBytes / sizeof(KeyT))) {",
                 "const size_t need = cbits <= 16 ? 2 : cbits <= 32 ? 4 : 8;"):
        if line not in text:
            raise AssertionError("ksh_decode.hip no longer has the line the model restates: " + line)
    return cfg


_CFG = []


def cfg():
    if not _CFG:
        _CFG.append(constants())
    return _CFG[0]


def k_cap(sb, c=None):
    """Keys of a type of `sb` bytes that the sort's LDS holds."""
    return (c or cfg()).kSortLdsBytes // sb


# ---- the geometry the sort works on -----------------------------------------------------------------------------------
def sort_bucket_bits(g, c=None):
    return (c or cfg()).kCoarseBits if g.route == "wide" else g.n


def sort_key_bits(g, c=None):
    return 2 * g.k - sort_bucket_bits(g, c)


def sorted_bytes(g, c=None):
    """Size of the type k_bucket_sort is instantiated with: the key on the plain route, the composite on the wide."""
    if g.route != "wide":
        return g.kb
    cbits = sort_key_bits(g, c)
    need = 2 if cbits <= 16 else (4 if cbits <= 32 else 8)
    return max(need, g.kb)


# ---- the model ---------------------------------------------------------------------------------------------------------
def lds_plan(cnt, eff_bits, c=None):
    """block_sort_into_lds: (sub-bin bits, shift) for cnt keys that differ in their low eff_bits bits."""
    c = c or cfg()
    bits = 0
    while (4 << bits) < cnt and bits < c.kMaxSubBits:
        bits += 1
    bits = min(bits, eff_bits)
    return bits, eff_bits - bits


def sub_bin_counts(keys, eff_bits, c=None):
    """Keys per sub-bin of one block_sort_into_lds call."""
    bits, shift = lds_plan(keys.size, eff_bits, c)
    sub = (keys >> U(shift)) & U((1 << bits) - 1)
    return np.bincount(sub.astype(np.int64), minlength=1 << bits)


def partition_plan(cnt, key_bits, sb, c=None):
    """The oversize branch of k_bucket_sort: (bits, shift)."""
    c = c or cfg()
    bits = 1
    while (cnt >> bits) > k_cap(sb, c) // c.part_div and bits < c.kMaxSubBits:
        bits += 1
    bits = min(bits, key_bits)
    return bits, key_bits - bits


def _unique_write(s, c, out):
    """block_unique_write on the sorted keys s of one LDS call: runs of equal keys across the threads' ranges."""
    cnt = s.size
    per = (cnt + c.kSortThreads - 1) // c.kSortThreads
    c0 = np.arange(per, cnt, per)
    if c0.size and (s[c0] == s[c0 - 1]).any():
        out.add("cutoff_straddle")


def _lds_call(keys, eff_bits, c, out, in_part):
    out.add("regs" if keys.size <= c.kSortRegs * c.kSortThreads else "stream")
    if sub_bin_counts(keys, eff_bits, c).max() > c.sub_limit:
        out.add("part_lds_bitonic" if in_part else "lds_bitonic")
    _unique_write(np.sort(keys), c, out)


def bucket_branches(keys, key_bits, sb, cutoff=1, c=None):
    """The branches k_bucket_sort<type of sb bytes> takes on one bucket holding the multiset `keys` (uint64, any
    order) of key_bits bits, called with `cutoff`."""
    c = c or cfg()
    keys = np.asarray(keys, dtype=U)
    cnt = keys.size
    out = set()
    if cnt == 0:
        return out
    cap = k_cap(sb, c)
    if cnt <= cap:
        _lds_call(keys, key_bits, c, out, False)
    else:
        out.add("partition")
        bits, shift = partition_plan(cnt, key_bits, sb, c)
        part = ((keys >> U(shift)) & U((1 << bits) - 1)).astype(np.int64)
        order = np.argsort(part, kind="stable")
        ends = np.cumsum(np.bincount(part, minlength=1 << bits))
        by_part = keys[order]
        for p in np.flatnonzero(np.diff(np.concatenate([[0], ends]))):
            pk = by_part[(ends[p - 1] if p else 0):ends[p]]
            if pk.size <= cap:
                _lds_call(pk, shift, c, out, True)
            else:
                out.add("global_bitonic")
    _, counts = np.unique(keys, return_counts=True)
    kept = int((counts >= max(cutoff, 1)).sum())
    if kept != cnt:
        out.add("drops")
    if int(counts[-1]) in (cutoff - 1, cutoff):
        out.add("run_at_end")
    return out


# ---- the input builder and the reference ---------------------------------------------------------------------------
def pack_kmers(kmers, k):
    """(words, lens) of the container with one string of exactly k bases per k-mer, in the order given."""
    kmers = np.asarray(kmers, dtype=U)
    n = kmers.size
    total = n * k
    codes = np.zeros((total + 31) // 32 * 32, dtype=np.uint8)
    body = codes[:total].reshape(n, k)
    for j in range(k):
        body[:, j] = (kmers >> U(2 * (k - 1 - j))) & U(3)
    quads = codes.reshape(-1, 4)
    packed = (quads[:, 0] << 6) | (quads[:, 1] << 4) | (quads[:, 2] << 2) | quads[:, 3]
    words = np.ascontiguousarray(packed).view(">u8").astype(U)
    return words, np.zeros(n, dtype=np.uint32)


def count_kmers(kmers):
    """(the distinct k-mers, ascending; how often each occurs): np.unique on the full 64-bit k-mers."""
    return np.unique(np.asarray(kmers, dtype=U), return_counts=True)


def reference_at(vals, counts, g, cutoff):
    """From count_kmers' result: (the k-mers seen at least max(cutoff, 1) times, ascending; the number of distinct
    k-mers below the cutoff; the bucket offsets of the kept ones: the cumulative bincount of their top N bits)."""
    keep = counts >= max(cutoff, 1)
    kept = vals[keep]
    offsets = np.zeros((1 << g.n) + 1, dtype=np.int64)
    np.cumsum(np.bincount((kept >> U(2 * g.k - g.n)).astype(np.int64), minlength=1 << g.n), out=offsets[1:])
    return kept, int((~keep).sum()), offsets


def reference(kmers, g, cutoff):
    return reference_at(*count_kmers(kmers), g, cutoff)


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """name, family, geometry, the k-mer occurrences in the order they are packed (uint64), the canonical flag
    they are decoded with, the sort bucket aimed at, the branches the model must (expect) and must not (forbid)
    report for that bucket at `at_cutoff`, and -- reads only -- the strings."""

    def __init__(self, name, family, g, kmers, target, expect, forbid=(), at_cutoff=1, canonical=False, strings=None):
        self.name, self.family, self.g, self.kmers, self.target = name, family, g, kmers, target
        self.expect, self.forbid, self.at_cutoff = frozenset(expect), frozenset(forbid), at_cutoff
        self.canonical, self.strings = canonical, strings

    def counted(self):
        """The multiset the decoder counts: the k-mers as packed, folded when the case is decoded canonically."""
        return synth.canonical(self.kmers, self.g.k) if self.canonical else self.kmers

    def target_keys(self, c=None):
        kbw = sort_key_bits(self.g, c)
        km = self.counted()
        return km[(km >> U(kbw)) == U(self.target)] & U((1 << kbw) - 1)

    def branches(self, cutoff=None, c=None):
        return bucket_branches(self.target_keys(c), sort_key_bits(self.g, c), sorted_bytes(self.g, c),
                               self.at_cutoff if cutoff is None else cutoff, c)


def _distinct(rng, n, lo, hi):
    """n distinct values of [lo, hi), ascending."""
    span = hi - lo
    assert 0 < n <= span
    if span <= 4 * n or span <= 1 << 16:
        return np.sort(rng.permutation(span)[:n].astype(U)) + U(lo)
    got = np.unique(rng.integers(lo, hi, size=n + n // 8 + 16, dtype=np.uint64))
    while got.size < n:
        got = np.unique(np.concatenate([got, rng.integers(lo, hi, size=n, dtype=np.uint64)]))
    return np.sort(rng.permutation(got)[:n])


def _spread(rng, n, lo, hi):
    """n values of [lo, hi): distinct while the range has room for twice as many, else every value of the range
    equally often (a shuffled range, tiled)."""
    span = hi - lo
    if 2 * n <= span:
        return _distinct(rng, n, lo, hi)
    perm = rng.permutation(span).astype(U) + U(lo)
    return np.tile(perm, (n + span - 1) // span)[:n]


def _neighbour_keys(kbw):
    top = (1 << kbw) - 1
    return np.array([0, 1, top // 2, top - 1, top], dtype=U)


def _assemble(name, family, g, keys, pos, expect, forbid=(), at_cutoff=1, seed=0):
    """The case whose target bucket (pos 0: the first, 1: a middle one, 2: the last) holds `keys`."""
    nbw, kbw = sort_bucket_bits(g), sort_key_bits(g)
    last = (1 << nbw) - 1
    target = (0, last // 2 + 3, last)[pos]
    parts = [(U(target) << U(kbw)) | np.asarray(keys, dtype=U)]
    for nb in (target - 1, target + 1):
        if 0 <= nb <= last:
            parts.append((U(nb) << U(kbw)) | _neighbour_keys(kbw))
    kmers = np.concatenate(parts)
    np.random.default_rng(0xB5C0 + seed).shuffle(kmers)
    return Case(name, family, g, kmers, target, expect, forbid, at_cutoff)


def uniform_sizes(g):
    cap = k_cap(sorted_bytes(g))
    return [1, 2, 4, 5, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, cap - 1, cap, cap + 1, 2 * cap + 3, 5 * cap]


def big_size(c=None):
    c = c or cfg()
    return (1 << c.kMaxSubBits) * (k_cap(BIG_GEOM.kb, c) // c.part_div) + 1


def _uniform(g, rng):
    kbw, cap = sort_key_bits(g), k_cap(sorted_bytes(g))
    regs = cfg().kSortRegs * cfg().kSortThreads
    out = []
    for i, cnt in enumerate(uniform_sizes(g)):
        keys = _spread(rng, cnt, 0, 1 << kbw)
        if cnt > cap:
            expect, forbid = {"partition"}, {"global_bitonic", "part_lds_bitonic"}
        else:
            expect, forbid = {"regs" if cnt <= regs else "stream"}, {"partition", "lds_bitonic"}
        if np.unique(keys).size == cnt:
            forbid = set(forbid) | {"drops", "cutoff_straddle"}
        out.append(_assemble("uniform-%d" % cnt, "uniform", g, keys, i % 3, expect, forbid, seed=i))
    return out


def big_case():
    """2^kMaxSubBits * kCap / 4 + 1 distinct keys in one bucket of (31, 14, 8): the partition's bits stop at
    kMaxSubBits and its parts are larger than their target."""
    rng = np.random.default_rng(0xB16)
    keys = _distinct(rng, big_size(), 0, 1 << sort_key_bits(BIG_GEOM))
    return _assemble("uniform-big", "uniform", BIG_GEOM, keys, 1, {"partition"},
                     {"global_bitonic", "part_lds_bitonic", "drops"}, seed=99)


def _threshold(g, rng):
    """1025 keys (9 sub-bin bits): one sub-bin holds exactly `n_in` keys, the other bins at most three each."""
    kbw, lim = sort_key_bits(g), cfg().sub_limit
    cnt = 1025
    bits, shift = lds_plan(cnt, kbw)
    assert bits == 9
    out = []
    for i, n_in in enumerate((lim, lim + 1)):
        for j, full in enumerate((0, (1 << bits) // 2 + 1, (1 << bits) - 1)):
            inside = _spread(rng, n_in, full << shift, (full + 1) << shift)
            others = np.delete(np.arange(1 << bits), full)
            per = np.full(others.size, (cnt - n_in) // others.size)
            per[:(cnt - n_in) - int(per.sum())] += 1
            rest = [_spread(rng, int(m), int(b) << shift, (int(b) + 1) << shift) for b, m in zip(others, per)]
            keys = np.concatenate([inside] + rest)
            assert keys.size == cnt
            expect, forbid = ({"regs"}, {"lds_bitonic", "partition"}) if n_in <= lim else ({"regs", "lds_bitonic"}, {"partition"})
            out.append(_assemble("threshold-%d-bin%d" % (n_in, full), "threshold", g, keys, (i + j) % 3, expect, forbid,
                                 seed=10 * i + j))
    return out


def cluster_bits(g):
    """The low bits the clustered keys differ in: 12, and 3 where the key has no room above 12 bits for two
    clusters to fall into one sub-bin each."""
    return 12 if sort_key_bits(g) >= 20 else 3


def _clustered(g, rng):
    kbw, cap = sort_key_bits(g), k_cap(sorted_bytes(g))
    low = cluster_bits(g)
    out = []
    for i, base in enumerate((0, (1 << kbw) // 3, (1 << kbw) - (1 << low))):
        base = base >> low << low
        keys = _spread(rng, 3000, base, base + (1 << low))
        out.append(_assemble("cluster-3000-at%d" % i, "clustered", g, keys, i, {"regs", "lds_bitonic"}, {"partition"}, seed=i))
    if low < 12:
        # a part's sub-bins of such a short key hold one value each once the part passes 4096 keys; this one holds
        # 3000 keys on 8 values, two values to a sub-bin, and the seven other parts bring the bucket beyond kCap
        part_span = (1 << kbw) // 8
        keys = np.concatenate([_spread(rng, 3000, 5 * part_span + 64, 5 * part_span + 64 + (1 << low))] +
                              [_spread(rng, (cap + 100 - 3000) // 7 + 1, p * part_span, (p + 1) * part_span)
                               for p in range(8) if p != 5])
        out.append(_assemble("cluster-part", "clustered", g, keys, 1, {"partition", "part_lds_bitonic"},
                             {"global_bitonic", "lds_bitonic"}, seed=5))
    total = cap + 100
    for i, (b0, b1) in enumerate(((0, (1 << kbw) - (1 << low)), ((1 << kbw) // 5, (1 << kbw) // 5 * 4))):
        b0, b1 = b0 >> low << low, b1 >> low << low
        assert b0 < (1 << (kbw - 1)) <= b1
        keys = np.concatenate([_spread(rng, total // 2, b0, b0 + (1 << low)),
                               _spread(rng, total - total // 2, b1, b1 + (1 << low))])
        out.append(_assemble("cluster-pair-%d" % i, "clustered", g, keys, 1 + i, {"partition", "part_lds_bitonic"},
                             {"global_bitonic", "lds_bitonic"}, seed=7 + i))
    return out


def heavy_counts(g):
    cap = k_cap(sorted_bytes(g))
    return [65, 254, 255, 256, cap // 4 + 1, cap + 5]


def needs_network(keys, eff_bits, c=None):
    """Some sub-bin of this block_sort_into_lds call overflows AND holds more than one value: the bitonic network
    has work to do (an overflowing sub-bin of one value is in order as it lies)."""
    c = c or cfg()
    bits, shift = lds_plan(keys.size, eff_bits, c)
    sub = ((keys >> U(shift)) & U((1 << bits) - 1)).astype(np.int64)
    over = np.flatnonzero(np.bincount(sub, minlength=1 << bits) > c.sub_limit)
    return any(np.unique(keys[sub == b]).size > 1 for b in over)


def _heavy(g, rng):
    kbw, cap = sort_key_bits(g), k_cap(sorted_bytes(g))
    top = (1 << kbw) - 1
    out = []
    for i, h in enumerate(heavy_counts(g)):
        for j, heavy in enumerate((0, top, top // 2 + 12345 % (top // 2))):
            # three single keys next to the heavy one share its sub-bin: what the network has to put in order
            near = np.array([heavy + d if heavy < top else heavy - d for d in (1, 2, 3)], dtype=U)
            rest = _distinct(rng, 2000, 1, top)
            rest = rest[~np.isin(rest, np.append(near, U(heavy)))]
            keys = np.concatenate([np.full(h, heavy, dtype=U), near, rest])
            if keys.size > cap:
                expect, forbid = {"partition", "global_bitonic", "drops"}, {"lds_bitonic"}
            else:
                fits_regs = keys.size <= cfg().kSortRegs * cfg().kSortThreads
                expect, forbid = {"regs" if fits_regs else "stream", "lds_bitonic", "drops", "cutoff_straddle"}, {"partition"}
            out.append(_assemble("heavy-%d-%s" % (h, ("zero", "ones", "mid")[j]), "heavy", g, keys, (i + j) % 3, expect,
                                 forbid, seed=10 * i + j))
    return out


RUN_PERS = (1, 2, 9)
RUN_LAST = (1, 2, 3, 4, 254, 255, 256)  # cutoff - 1, cutoff and cutoff + 1 occurrences of the last key, cutoffs 2, 3 and 255


def _runs(g, rng):
    """Every key 1 to 4 times; the bucket's size gives block_unique_write `per` keys per thread (an 8-byte type
    holds fewer than 9 x kSortThreads keys in LDS: its per = 9 cases take the partition instead), and the
    largest key of the bucket occurs `last` times."""
    kbw, threads = sort_key_bits(g), cfg().kSortThreads
    top = (1 << kbw) - 1
    out = []
    for i, per in enumerate(RUN_PERS):
        cnt = per * threads - 24
        for j, last in enumerate(RUN_LAST):
            m = rng.integers(1, 5, size=cnt)
            m = m[:int(np.searchsorted(np.cumsum(m), cnt - last, side="right"))]
            body = cnt - last - int(m.sum())
            if body:
                m = np.append(m, body)
            vals = _distinct(rng, m.size, 0, top)
            keys = np.concatenate([np.repeat(vals, m), np.full(last, top, dtype=U)])
            assert keys.size == cnt and (cnt + threads - 1) // threads == per
            at = 255 if last >= 254 else (2 if last <= 2 else 3)
            expect = {"drops"} | ({"cutoff_straddle"} if cnt <= k_cap(sorted_bytes(g)) else {"partition"})
            at_end = {"run_at_end"} if last in (at - 1, at) else set()  # (4 and 256 are cutoff + 1 for 3 and 255)
            out.append(_assemble("runs-per%d-last%d" % (per, last), "runs", g, keys, (i + j) % 3, expect | at_end,
                                 {"run_at_end"} - at_end, at, seed=10 * i + j))
    return out


def _reads(g, rng):
    """Whole reads, decoded canonically: the realistic form of the heavy key (a poly-A tail, a tandem repeat, a
    read seen four times), with string ends and the canonical fold in play."""
    kbw, cap = sort_key_bits(g), k_cap(sorted_bytes(g))
    random_read = synth.string_of_bases(rng.integers(0, 4, size=150).astype(np.uint8))
    out = []
    for name, strings in (("poly-a", ["A" * 150] * 300), ("tandem-ac", ["AC" * 75] * 300), ("read-x4", [random_read] * 4)):
        kmers = np.concatenate([synth.kmers_of_bases(synth.bases_of_string(s), g.k) for s in dict.fromkeys(strings)])
        kmers = np.tile(kmers, len(strings) // len(set(strings)))
        folded = synth.canonical(kmers, g.k)
        buckets, counts = np.unique(folded >> U(kbw), return_counts=True)
        target, cnt = int(buckets[np.argmax(counts)]), int(counts.max())
        if name == "read-x4":
            expect = {"regs", "drops"}
        else:
            expect = {"drops"} | ({"partition", "global_bitonic"} if cnt > cap else {"lds_bitonic"})
        out.append(Case(name, "reads", g, kmers, target, expect, (), 2, canonical=True, strings=strings))
    return out


_BUILDERS = {"uniform": _uniform, "threshold": _threshold, "clustered": _clustered, "heavy": _heavy, "runs": _runs,
             "reads": _reads}
_CASES = {}


def cases(g, family):
    """The cases of one geometry and family, in a fixed order (seeded; built once per process)."""
    if (g, family) not in _CASES:
        rng = np.random.default_rng([0xB50C, g.k, g.n, g.kb, FAMILIES.index(family)])
        _CASES[g, family] = _BUILDERS[family](g, rng)
    return _CASES[g, family]


def all_cases(g):
    return [c for family in FAMILIES for c in cases(g, family)]


def largest_bucket(kmers, k, n):
    """Occurrences in the fullest of the 2^n buckets of a k-mer array."""
    return int(np.bincount((np.asarray(kmers, dtype=U) >> U(2 * k - n)).astype(np.int64)).max())

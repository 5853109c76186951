"""Cases for the front half of the SPSS decode (k_str_bases, k_mark_ends, k_decode<false/true>, k_hist_columns,
k_decode_l1, k_decode_l2 in csrc/ksh_decode.hip, with decode_geometry and the route choice of scatter_sort), a numpy
model of the branches it takes and a numpy reference of what it must compute.

A *case* is a list of ACGT strings with a geometry (k, N, key bytes) and, optionally, the padding bits of the last
word set to all ones.  The strings are laid out so that a string end, a k-mer, a word, a group of words, a tile of
the two-level scatter or the count of k-mers sits on an edge of the kernels' arithmetic.

The reference (walk_reference) is plain numpy on the strings: every k-mer occurrence as a 64-bit value, from a loop
over the k base offsets of the concatenated codes, the positions inside each string's last K - 1 bases masked out.
Expected sets are np.unique with counts of that, cut at the cutoff; tests/test_decode_walk_model_cpu.py ties it to
the oracle on every small case.

The model (geometry, route, valid_positions, l1_tiles, l2_spans, branches) restates the kernels' arithmetic -- the
end-bit window, the groups, the tiles, the super-buckets -- and says which branches a case takes under a given
environment and canonical flag.  It is never the expected answer.  Its constants are read from the text of
ksh_decode.hip, so a changed constant fails the CPU test instead of moving the cases off their edges silently.
Every case declares the branch names it must (expect) and must not (forbid) reach, in the environment and with the
canonical flag it aims at; tests/test_gpu_decode_walk.py asserts them before it runs the case, and the CPU test that
every name of BRANCHES is some case's expectation."""
import os
import re
from collections import namedtuple

import numpy as np

from kmersets import synth

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECODE_HIP = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc", "ksh_decode.hip")

CUTOFFS = (1, 2)
ORACLE_MAX = 20000  # occurrences up to which the CPU test feeds a case to the oracle
PHANTOM_MIN_K = 12  # from here on the windows across a string end or the tail are absent from the real k-mers

# the three processes of the GPU test: what each sets (both switches are read once per process)
ENVS = {"default": {}, "l2min": {"KSH_DECODE_L2_MIN": "1024"}, "direct": {"KSH_DECODE_SCATTER": "direct"}}

Geom = namedtuple("Geom", "k n kb")
Cfg = namedtuple("Cfg", "kDecThreads kDecSgBits kDecL1Threads per_narrow per_wide kDecL2Threads kDecL2Per kColTeams "
                        "kCoarseBits max_groups group_words l2_min_floor l2_min_default_bits max_two_level_bits")
Geometry = namedtuple("Geometry", "n_words n_end_words groups wpg")

WALK_BRANCHES = (
    ["end_mod64_%d" % r for r in (0, 31, 32, 63)] + ["blocked_by_next_end_word"] +
    ["onek_phase_%d" % p for p in range(32)] +
    ["kmer_ends_word", "kmer_crosses_word", "one_word", "tail_0", "tail_1", "tail_31", "tail_1_ones", "tail_31_ones",
     "string_gt_group", "string_gt_l1_tile", "k_2", "k_8", "k_9", "k_16", "k_31", "palindrome", "rc_lt_fw",
     "non_canonical"])
GROUP_BRANCHES = ["groups_1", "groups_2_short_last", "groups_15", "groups_16", "groups_17", "groups_cap_wpg_gt_256",
                  "empty_last_group", "hist_groups_lt_teams", "hist_partial_wave"]
L1_BRANCHES = ["l1_top_lt_64", "l1_top_eq_64", "l1_top_gt_64", "l1_wide_key_tile", "l1_partial_tile", "l1_multi_tile",
               "l1_full_tile_one_sg", "l1_tile_all_sg"]
L2_BRANCHES = ["l2_one_sg", "l2_seam", "l2_far", "l2_first_127", "l2_last_1", "l2_last_full", "l2_lo_bits_1",
               "l2_lo_bits_7", "l2_wide_u16", "l2_wide_u32", "l2_wide_u64"]
ROUTE_BRANCHES = ["route_direct_below_2p20", "route_two_level_at_2p20", "route_direct_small_n", "route_direct_few",
                  "route_direct_forced", "route_two_level_small"]
BRANCHES = tuple(WALK_BRANCHES + GROUP_BRANCHES + L1_BRANCHES + L2_BRANCHES + ROUTE_BRANCHES)


def geom_id(g):
    return "%d-%d-%d" % g


# ---- constants from the kernel's text -------------------------------------------------------------------------------
RESTATED = (
    "*n_words = (s->n_bases + 31) / 32;",
    "*n_end_words = (s->n_bases + 63) / 64 + 1;",
    "if (g < 1) g = 1;",
    "*words_per_group = (*n_words + g - 1) / g;",
    "const int64_t p = str_start[i + 1] - 1;",
    "atomicOr(&end_bits[p >> 6], 1ull << (p & 63));",
    "const uint64_t no_end_mask = (uint64_t(1) << (k - 1)) - 1;  // bits p .. p+K-2 must be clear",
    "const bool valid = (p + k <= n_bases) && (((eb >> j) & no_end_mask) == 0);",
    "const bool valid = (p + k <= n_bases) && (((eb >> jj) & no_end_mask) == 0);",
    "if (esh && ew + 1 < n_end_words) eb |= end_bits[ew + 1] << (64 - esh);",
    "const uint64_t w1 = (w + 1 < n_words) ? words[w + 1] : 0;",
    "const int64_t w_begin = int64_t(blockIdx.x) * words_per_group;",
    "const int64_t w_end = min(w_begin + words_per_group, n_words);",
    "static constexpr int kTile = kDecL1Threads * kPer;",
    "for (int64_t w0i = w_begin; w0i < w_end; w0i += kDecL1Tile / 32) {",
    "const int j0 = (tid % kParts) * kDecL1Per;",
    "const int top = 2 * (j0 + k);  // bits of the window up to and including the k-mer's last base",
    "uint64_t fw = (top <= 64 ? (w0 >> (64 - top)) : ((w0 << (top - 64)) | (w1 >> (128 - top)))) & mask;",
    "constexpr int kDecL2Tile = kDecL2Threads * kDecL2Per;",
    "const int nb = 1 << n_bucket_bits, lo_bits = n_bucket_bits - kDecSgBits;",
    "const uint32_t n_bins = min<uint32_t>(uint32_t(kBins), (2u << lo_bits));",
    "if (tid == 0) s_first = (uint32_t(tmp_b[p0]) >> lo_bits) << lo_bits;  // first bucket of the tile's first super-bucket",
    "if (b - base_b < n_bins) {",
    "const int64_t per_team = (n_groups + kColTeams - 1) / kColTeams;",
    "if (int(blockIdx.x + 1) * 64 <= n_buckets) {  // a full wave (the others returned above: every lane for itself)",
    "return e && std::string(e) == \"direct\";",
    "if (!direct && ctx->dec_kmers >= two_level_min && nbits_w > kDecSgBits && nbits_w <= ",
    "ctx->dec_kmers < int64_t(0xFFFFFFF0)) {",
    "inline bool wide_route(const ksh_geom* g) { return g->n_bucket_bits > kCoarseBits; }",
    "const int kbw = wide ? 2 * g->k - kCoarseBits : key_bits(g);",
    "const size_t need = cbits <= 16 ? 2 : cbits <= 32 ? 4 : 8;",
)


def constants(text=None):
    """Cfg from ksh_decode.hip; the lines the model restates must stand there as written."""
    if text is None:
        text = open(DECODE_HIP).read()

    def nums(pattern):
        m = re.search(pattern, text)
        if m is None:
            raise AssertionError("ksh_decode.hip no longer has what the model reads: " + pattern)
        return [int(x) for x in m.groups()]

    per_wide, per_narrow = nums(r"static constexpr int kPer = sizeof\(KeyT\) == 8 \? (\d+) : (\d+);")
    max_groups, round_up, group_words = nums(r"int64_t g = std::min<int64_t>\((\d+), \(\*n_words \+ (\d+)\) / (\d+)\);")
    if round_up != group_words - 1:
        raise AssertionError("decode_geometry no longer rounds the group count up")
    floor, default_bits = nums(r"return e \? std::max<int64_t>\((\d+), atoll\(e\)\) : int64_t\(1\) << (\d+);")
    cfg = Cfg(nums(r"constexpr int kDecThreads = (\d+);")[0], nums(r"constexpr int kDecSgBits = (\d+);")[0],
              nums(r"constexpr int kDecL1Threads = (\d+);")[0], per_narrow, per_wide,
              nums(r"constexpr int kDecL2Threads = (\d+);")[0], nums(r"constexpr int kDecL2Per = (\d+);")[0],
              nums(r"constexpr int kColTeams = (\d+);")[0], nums(r"constexpr int kCoarseBits = (\d+);")[0],
              max_groups, group_words, floor, default_bits,
              nums(r"nbits_w > kDecSgBits && nbits_w <= (\d+) &&")[0])
    for line in RESTATED:
        if line not in text:
            raise AssertionError("ksh_decode.hip no longer has the line the model restates: " + line)
    return cfg


_CFG = []


def cfg():
    if not _CFG:
        _CFG.append(constants())
    return _CFG[0]


# ---- the model: geometry and route --------------------------------------------------------------------------------------
def geometry(n_bases, c=None):
    """decode_geometry: words, end words, groups and words per group of a container of n_bases bases."""
    c = c or cfg()
    n_words = (n_bases + 31) // 32
    n_end_words = (n_bases + 63) // 64 + 1
    groups = max(1, min(c.max_groups, (n_words + c.group_words - 1) // c.group_words))
    return Geometry(n_words, n_end_words, groups, (n_words + groups - 1) // groups)


def scatter_bucket_bits(g, c=None):
    """The bucket bits the counting pass and the scatter work on: the coarse geometry on the wide route."""
    c = c or cfg()
    return c.kCoarseBits if g.n > c.kCoarseBits else g.n


def scatter_bytes(g, c=None):
    """Size of the type the scatter is instantiated with: the key, or the composite on the wide route."""
    c = c or cfg()
    if g.n <= c.kCoarseBits:
        return g.kb
    cbits = 2 * g.k - c.kCoarseBits
    return max(2 if cbits <= 16 else (4 if cbits <= 32 else 8), g.kb)


def two_level_min(env, c=None):
    c = c or cfg()
    e = env.get("KSH_DECODE_L2_MIN")
    return max(c.l2_min_floor, int(e)) if e is not None else 1 << c.l2_min_default_bits


def route(case, env, c=None):
    """scatter_sort's choice for this case in a process with `env` set: "direct" (k_decode<true>) or "two_level"
    (k_decode_l1 / k_decode_l2)."""
    c = c or cfg()
    nbits_w = scatter_bucket_bits(case.g, c)
    if env.get("KSH_DECODE_SCATTER") == "direct":
        return "direct"
    if (case.n_occ >= two_level_min(env, c) and c.kDecSgBits < nbits_w <= c.max_two_level_bits and
            case.n_occ < 0xFFFFFFF0):
        return "two_level"
    return "direct"


def l1_tile_positions(g, c=None):
    """Positions of one k_decode_l1 tile: kDecL1Threads * kPer."""
    c = c or cfg()
    return c.kDecL1Threads * (c.per_wide if scatter_bytes(g, c) == 8 else c.per_narrow)


# ---- the reference ---------------------------------------------------------------------------------------------------------
_CODE = np.full(256, 255, dtype=np.uint8)
_CODE[[ord(x) for x in "ACGT"]] = (0, 1, 2, 3)


def codes_of(strings):
    """(the 2-bit codes of the concatenated strings, uint8; the lengths, int64)."""
    lens = np.array([len(s) for s in strings], dtype=np.int64)
    codes = _CODE[np.frombuffer("".join(strings).encode(), dtype=np.uint8)]
    assert codes.size == 0 or codes.max() < 4
    return codes, lens


def _windows(codes, k):
    """Forward and reverse-complement value of the window of k codes at every position that has one."""
    n_pos = codes.size - k + 1
    fw = np.zeros(max(n_pos, 0), dtype=U)
    rc = np.zeros(max(n_pos, 0), dtype=U)
    for j in range(k):
        c = codes[j:j + n_pos].astype(U)
        fw = (fw << U(2)) | c
        rc |= (U(3) - c) << U(2 * j)
    return fw, rc


def walk_both(strings, k):
    """(forward, reverse complement) of every k-mer occurrence of the strings, in position order."""
    codes, lens = codes_of(strings)
    assert (lens >= k).all()
    fw, rc = _windows(codes, k)
    keep = np.ones(fw.size, dtype=bool)
    ends = np.cumsum(lens)
    for d in range(1, k):  # the positions inside each string's last K - 1 bases start no k-mer
        at = ends - d
        keep[at[at < keep.size]] = False
    return fw[keep], rc[keep]


def walk_reference(strings, k, canonical):
    """Every k-mer occurrence of the strings as a 64-bit value: the forward k-mer, or the minimum of it and its
    reverse complement."""
    fw, rc = walk_both(strings, k)
    return np.minimum(fw, rc) if canonical else fw


def expected_at(vals, counts, g, cutoff):
    """From np.unique(occurrences, return_counts=True): (the k-mers seen at least `cutoff` times, ascending; how
    many distinct ones are below the cutoff; offsets and keys of the kept ones by synth.to_bucketed)."""
    keep = counts >= max(cutoff, 1)
    kept = vals[keep]
    offsets, keys = synth.to_bucketed(kept, g.k, g.n, g.kb)
    return kept, int((~keep).sum()), offsets, keys


def phantom_windows(case, canonical):
    """The windows the decoder must NOT emit: at every position of the stream that starts no k-mer -- across a
    string end, or across the tail into the padding bits and the zero word behind the last one."""
    codes, lens = codes_of(case.strings)
    k = case.g.k
    pad = np.full(-codes.size % 32, 3 if case.pad_ones else 0, dtype=np.uint8)
    stream = np.concatenate([codes, pad, np.zeros(32, dtype=np.uint8)])
    fw, rc = _windows(stream, k)
    fw, rc = fw[:codes.size], rc[:codes.size]
    keep = np.zeros(codes.size, dtype=bool)
    ends = np.cumsum(lens)
    for d in range(1, k):
        keep[ends - d] = True
    return np.unique(np.minimum(fw[keep], rc[keep]) if canonical else fw[keep])


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """name, family, geometry, the strings, whether the padding bits of the last word are ones, the branch names
    the model must (expect) and must not (forbid) report in environment `env` (a key of ENVS) with the canonical
    flag `canonical`."""

    def __init__(self, name, family, g, strings, expect, forbid=(), env="default", canonical=False, pad_ones=False):
        self.name, self.family, self.g, self.strings = name, family, g, strings
        self.expect, self.forbid, self.env, self.canonical = frozenset(expect), frozenset(forbid), env, canonical
        self.pad_ones = pad_ones
        self.lens = np.array([len(s) for s in strings], dtype=np.int64)
        self.n_bases = int(self.lens.sum())
        self.n_occ = int((self.lens - g.k + 1).sum())
        self._occ, self._counted, self._branches = None, {}, {}
        unknown = (self.expect | self.forbid) - set(BRANCHES)
        assert not unknown, (name, sorted(unknown))

    def words_and_lens(self):
        """The container as the device gets it (synth.pack_strings; the padding bits set when the case says so)."""
        words, lens = synth.pack_strings(self.strings, self.g.k)
        pad = -self.n_bases % 32
        if self.pad_ones and pad:
            words = words.copy()
            words[-1] |= U((1 << (2 * pad)) - 1)
        return words, lens

    def occurrences(self, canonical):
        if self._occ is None:
            self._occ = walk_both(self.strings, self.g.k)
        fw, rc = self._occ
        return np.minimum(fw, rc) if canonical else fw

    def counted(self, canonical):
        """np.unique with counts of the occurrences (computed once per flag)."""
        if canonical not in self._counted:
            self._counted[canonical] = np.unique(self.occurrences(canonical), return_counts=True)
        return self._counted[canonical]

    def branches(self, env=None, canonical=None):
        env = self.env if env is None else env
        canonical = self.canonical if canonical is None else canonical
        if (env, canonical) not in self._branches:
            self._branches[env, canonical] = branches(self, ENVS[env], canonical)
        return self._branches[env, canonical]

    def aims_hold(self):
        got = self.branches()
        return self.expect <= got and not (self.forbid & got)


# ---- the model: the walk, the tiles, the spans ----------------------------------------------------------------------------
def valid_positions(case):
    """The kernels' validity test at every position of every word: p + K <= n_bases and no end bit at p .. p + K - 2
    (end bit: the last base of a string).  Also returns the end-bit prefix sums it was computed from."""
    k, n = case.g.k, case.n_bases
    n_pos = geometry(n).n_words * 32
    marks = np.zeros(n_pos + k + 64, dtype=np.int64)
    marks[np.cumsum(case.lens) - 1] = 1
    cs = np.concatenate([[0], np.cumsum(marks)])
    p = np.arange(n_pos)
    ends_in_window = cs[p + k - 1] - cs[p]
    return (p + k <= n) & (ends_in_window == 0), cs


def l1_tiles(case, c=None):
    """(words per tile, [(group, first word, words, valid positions) for every tile k_decode_l1 takes])."""
    c = c or cfg()
    geo = geometry(case.n_bases, c)
    tile_words = l1_tile_positions(case.g, c) // 32
    valid, _ = valid_positions(case)
    vc = np.concatenate([[0], np.cumsum(valid)])
    tiles = []
    for grp in range(geo.groups):
        w_begin = grp * geo.wpg
        w_end = min(w_begin + geo.wpg, geo.n_words)
        for w0 in range(w_begin, w_end, tile_words):
            w1 = min(w0 + tile_words, w_end)
            tiles.append((grp, w0, w1 - w0, int(vc[32 * w1] - vc[32 * w0])))
    return tile_words, tiles


def l2_spans(sg_counts, c=None):
    """[(first super-bucket, width) for every kDecL2Tile-key tile of the intermediate array], which is sorted by
    super-bucket: width = last super-bucket - first + 1, counted by index as the kernel's window of two
    super-buckets' bins is (an empty super-bucket in between counts)."""
    c = c or cfg()
    tile = c.kDecL2Threads * c.kDecL2Per
    cum = np.cumsum(np.asarray(sg_counts, dtype=np.int64))
    n = int(cum[-1])
    out = []
    for p0 in range(0, n, tile):
        first = int(np.searchsorted(cum, p0, side="right"))
        last = int(np.searchsorted(cum, min(p0 + tile, n) - 1, side="right"))
        out.append((first, last - first + 1))
    return out


def branches(case, env, canonical, c=None):
    """The branch names (BRANCHES) the decode of `case` reaches in a process with `env` set, decoded with the
    canonical flag given."""
    c = c or cfg()
    g, k, n = case.g, case.g.k, case.n_bases
    geo = geometry(n, c)
    out = set()
    # ---- the walk
    valid, cs = valid_positions(case)
    ends = np.cumsum(case.lens) - 1
    starts = ends + 1 - case.lens
    for r in (0, 31, 32, 63):
        if (ends % 64 == r).any():
            out.add("end_mod64_%d" % r)
    p = np.arange(valid.size)
    in_window = cs[p + k - 1] - cs[p]
    next_word = (p // 64 + 1) * 64
    in_own_word = cs[np.minimum(p + k - 1, next_word)] - cs[p]
    if ((p % 64 >= 32) & (p + k <= n) & (in_window > 0) & (in_own_word == 0)).any():
        out.add("blocked_by_next_end_word")
    for ph in np.unique(starts[case.lens == k] % 32):
        out.add("onek_phase_%d" % ph)
    vp = np.flatnonzero(valid)
    assert vp.size == case.n_occ
    if (vp % 32 + k == 32).any():
        out.add("kmer_ends_word")
    if (vp % 32 + k > 32).any():
        out.add("kmer_crosses_word")
    if geo.n_words == 1:
        out.add("one_word")
    if n % 32 in (0, 1, 31):
        out.add("tail_%d%s" % (n % 32, "_ones" if case.pad_ones and n % 32 else ""))
    if (case.lens > geo.wpg * 32).any():
        out.add("string_gt_group")
    if (case.lens > l1_tile_positions(g, c)).any():
        out.add("string_gt_l1_tile")
    if k in (2, 8, 9, 16, 31):
        out.add("k_%d" % k)
    fw, rc = case.occurrences(False), None
    if canonical:
        rc = case._occ[1]
        if (rc == fw).any():
            out.add("palindrome")
        if (rc < fw).any():
            out.add("rc_lt_fw")
    else:
        out.add("non_canonical")
    # ---- groups and k_hist_columns
    last_words = geo.n_words - (geo.groups - 1) * geo.wpg
    if geo.groups in (1, 15, 16, 17):
        out.add("groups_%d" % geo.groups)
    if geo.groups == 2 and 0 < last_words < geo.wpg:
        out.add("groups_2_short_last")
    if geo.groups == c.max_groups and geo.wpg > c.group_words:
        out.add("groups_cap_wpg_gt_256")
    if last_words <= 0:
        out.add("empty_last_group")
    if geo.groups < c.kColTeams:
        out.add("hist_groups_lt_teams")
    nbits_w = scatter_bucket_bits(g, c)
    if (1 << nbits_w) % 64:
        out.add("hist_partial_wave")
    # ---- the route
    how = route(case, env, c)
    default_min = 1 << c.l2_min_default_bits
    if how == "direct":
        if env.get("KSH_DECODE_SCATTER") == "direct":
            out.add("route_direct_forced")
        elif not c.kDecSgBits < nbits_w <= c.max_two_level_bits:
            out.add("route_direct_small_n")
        elif "KSH_DECODE_L2_MIN" in env:
            out.add("route_direct_few")
        elif case.n_occ == default_min - 1:
            out.add("route_direct_below_2p20")
        return out
    if "KSH_DECODE_L2_MIN" not in env and case.n_occ == default_min:
        out.add("route_two_level_at_2p20")
    if case.n_occ < default_min:
        out.add("route_two_level_small")
    # ---- k_decode_l1
    occ = np.minimum(fw, rc) if canonical else fw
    sg = (occ >> U(2 * k - c.kDecSgBits)).astype(np.int64)
    n_sg = 1 << c.kDecSgBits
    sb = scatter_bytes(g, c)
    per = c.per_wide if sb == 8 else c.per_narrow
    tops = {2 * (j0 + k) for j0 in range(0, 32, per)}
    if min(tops) < 64:
        out.add("l1_top_lt_64")
    if 64 in tops:
        out.add("l1_top_eq_64")
    if max(tops) > 64:
        out.add("l1_top_gt_64")
    if sb == 8:
        out.add("l1_wide_key_tile")
    tile_words, tiles = l1_tiles(case, c)
    per_group = np.bincount([t[0] for t in tiles], minlength=geo.groups)
    if per_group.max() > 1:
        out.add("l1_multi_tile")
    at = 0
    for grp, w0, nw, n_valid in tiles:
        if nw < tile_words:
            out.add("l1_partial_tile")
        seen = np.bincount(sg[at:at + n_valid], minlength=n_sg)
        at += n_valid
        if n_valid == tile_words * 32 and (seen > 0).sum() == 1:
            out.add("l1_full_tile_one_sg")
        if (seen > 0).all():
            out.add("l1_tile_all_sg")
    assert at == occ.size
    # ---- k_decode_l2
    l2_tile = c.kDecL2Threads * c.kDecL2Per
    for first, width in l2_spans(np.bincount(sg, minlength=n_sg), c):
        out.add("l2_one_sg" if width == 1 else ("l2_seam" if width == 2 else "l2_far"))
        if first == n_sg - 1:
            out.add("l2_first_127")
    if occ.size % l2_tile == 1:
        out.add("l2_last_1")
    if occ.size % l2_tile == 0:
        out.add("l2_last_full")
    lo_bits = nbits_w - c.kDecSgBits
    if lo_bits in (1, 7):
        out.add("l2_lo_bits_%d" % lo_bits)
    if g.n > c.kCoarseBits:
        out.add("l2_wide_u%d" % (8 * sb))
    return out


# ---- builders ------------------------------------------------------------------------------------------------------------
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def _text(rng, n, alphabet=4):
    return _LETTERS[rng.integers(0, alphabet, size=n)].tobytes().decode()


def _cut(text, lens):
    out, at = [], 0
    for ln in lens:
        out.append(text[at:at + ln])
        at += ln
    assert at == len(text)
    return out


def _palindrome(rng, k):
    """A string of k bases (k even) that equals its own reverse complement."""
    half = _text(rng, k // 2)
    return half + half[::-1].translate(str.maketrans("ACGT", "TGCA"))


def walk_lengths(k, tail, rng, min_occ):
    """String lengths that put last bases on positions 0, 31, 32 and 63 of an end word, a string of exactly K bases
    on every phase of a word, random lengths up to min_occ k-mers, and n_bases % 32 == tail."""
    lens = []
    for r in (0, 31, 32, 63):
        pos = sum(lens)
        lens.append(k + 1 + (r - (pos + k)) % 64)  # last base at pos + len - 1 = r (mod 64)
    for ph in range(32):
        pos = sum(lens)
        lens += [k + 1 + (ph - (pos + k + 1)) % 32, k]
    while sum(lens) - len(lens) * (k - 1) < min_occ:
        lens.append(k + int(rng.integers(0, 80)))
    pos = sum(lens)
    lens.append(k + 1 + (tail - (pos + k + 1)) % 32)
    assert sum(lens) % 32 == tail
    return lens


WALK_GEOMS = (Geom(2, 3, 2), Geom(8, 8, 4), Geom(9, 10, 4), Geom(16, 14, 4), Geom(31, 14, 8))
WIDE_GEOMS = (Geom(15, 20, 2), Geom(16, 20, 2), Geom(23, 20, 4), Geom(31, 20, 8))
TAILS = ((0, False), (1, False), (31, False), (1, True), (31, True))


def _walk_cases():
    out = []
    for g in WALK_GEOMS + (WIDE_GEOMS[0], WIDE_GEOMS[2], WIDE_GEOMS[3]):
        wide = g.n > cfg().kCoarseBits
        rng = np.random.default_rng([0xDEC0, g.k, g.n, g.kb])
        for tail, ones in (TAILS[2:3] if wide else TAILS):
            lens = walk_lengths(g.k, tail, rng, 1500)
            strings = _cut(_text(rng, sum(lens)), lens)
            if g.k % 2 == 0:  # a k-mer that is its own reverse complement, in a string of exactly K bases
                assert lens[5] == g.k
                strings[5] = _palindrome(rng, g.k)
            expect = {"end_mod64_0", "end_mod64_31", "end_mod64_32", "end_mod64_63", "kmer_ends_word",
                      "kmer_crosses_word", "groups_1", "hist_groups_lt_teams", "rc_lt_fw",
                      "tail_%d%s" % (tail, "_ones" if ones else "")}
            expect |= {"onek_phase_%d" % ph for ph in range(32)}
            if g.k > 2:
                expect.add("blocked_by_next_end_word")
            if g.k in (2, 8, 9, 16, 31):
                expect.add("k_%d" % g.k)
            if g.k % 2 == 0:
                expect.add("palindrome")
            if g.n <= cfg().kDecSgBits:
                expect |= {"hist_partial_wave", "route_direct_small_n"}
            else:
                expect |= {"route_two_level_small", "l2_far", "l1_partial_tile"}
                expect.add("l1_wide_key_tile" if scatter_bytes(g) == 8 else "l1_top_lt_64")
                if g.k == 8:
                    expect |= {"l1_top_eq_64", "l2_lo_bits_1"}
                if g.k >= 9:
                    expect.add("l1_top_gt_64")
                if g.n == 14:
                    expect.add("l2_lo_bits_7")
                if wide:
                    expect.add("l2_wide_u%d" % (8 * scatter_bytes(g)))
            forbid = {"l1_top_gt_64", "l1_wide_key_tile"} if g.k == 8 else set()
            name = "walk-%s-tail%d%s" % (geom_id(g), tail, "-ones" if ones else "")
            out.append(Case(name, "walk", g, strings, expect, forbid, env="l2min", canonical=True, pad_ones=ones))
    # one word: w1 is never read
    rng = np.random.default_rng(0x0E)
    out.append(Case("one-word-8", "walk", Geom(8, 8, 4), _cut(_text(rng, 32), [8, 9, 15]),
                    {"one_word", "tail_0", "groups_1", "route_direct_few", "k_8"}, env="l2min"))
    out.append(Case("one-word-2", "walk", Geom(2, 3, 2), ["AC", "GTT", "AT"],
                    {"one_word", "palindrome", "hist_partial_wave", "k_2"}, canonical=True))
    out.append(Case("one-word-31", "walk", Geom(31, 14, 8), [_text(rng, 31)],
                    {"one_word", "tail_31_ones", "k_31", "route_direct_forced"}, env="direct", pad_ones=True))
    return out


def _fill(total, k, rng, lo, hi):
    """Random string lengths in [lo, hi) that sum to `total` (the last two share what is left)."""
    lens = []
    left = total
    while left >= 2 * hi:
        lens.append(int(rng.integers(lo, hi)))
        left -= lens[-1]
    first = left // 2
    lens += [first, left - first]
    assert min(lens) >= k and sum(lens) == total
    return lens


def _group_cases():
    out = []
    # two groups, the last one short; one string longer than a group
    g = Geom(16, 14, 4)
    rng = np.random.default_rng(0x6209)
    n_words = cfg().group_words + 1
    lens = [300, 129 * 32 + 50] + _fill(n_words * 32 - 7 - 300 - (129 * 32 + 50), g.k, rng, 200, 900)
    out.append(Case("groups-2", "groups", g, _cut(_text(rng, sum(lens)), lens),
                    {"groups_2_short_last", "string_gt_group", "hist_groups_lt_teams", "l1_partial_tile", "l2_far",
                     "route_two_level_small"}, {"string_gt_l1_tile"}, env="l2min"))
    # 15 | 16 and 16 | 17 groups
    for n_words, g, groups, more in ((3840, Geom(9, 5, 4), 15, {"hist_partial_wave", "hist_groups_lt_teams", "route_direct_small_n", "k_9"}),
                                     (3841, Geom(16, 14, 4), 16, {"l1_partial_tile", "l1_tile_all_sg", "l2_far"}),
                                     (4096, Geom(31, 14, 8), 16, {"l1_multi_tile", "l1_wide_key_tile", "l1_tile_all_sg", "l2_far"}),
                                     (4097, Geom(16, 14, 4), 17, {"l1_partial_tile", "l1_tile_all_sg", "l2_far"})):
        rng = np.random.default_rng([0x6209, n_words])
        lens = _fill(n_words * 32 - 5, g.k, rng, 500, 4000)
        forbid = {"hist_groups_lt_teams"} if groups >= cfg().kColTeams else set()
        if n_words == 4096:
            forbid.add("l1_partial_tile")
        out.append(Case("groups-%d-words" % n_words, "groups", g, _cut(_text(rng, sum(lens)), lens),
                        {"groups_%d" % groups} | more, forbid, env="l2min"))
    # the group cap: 512 groups of 257 words cover more than 131073 words, so group 511 starts past the end
    g = Geom(23, 14, 4)
    rng = np.random.default_rng(0xCA9)
    n_words = cfg().max_groups * cfg().group_words + 1
    lens = _fill(n_words * 32 - 9, g.k, rng, 2000, 40000)
    out.append(Case("group-cap", "groups", g, _cut(_text(rng, sum(lens)), lens),
                    {"groups_cap_wpg_gt_256", "empty_last_group", "l1_multi_tile", "l1_partial_tile", "l1_tile_all_sg",
                     "l2_one_sg", "l2_seam", "string_gt_l1_tile", "string_gt_group"},
                    {"hist_groups_lt_teams", "route_two_level_small", "l2_far"}))
    return out


def _poly_a_case():
    """A^(8192 + K + 32) at the front of exactly 512 words: two groups of 256 words, and the first tile of the first
    group has all of its 8192 positions valid, all of them the k-mer A^K in super-bucket 0."""
    g = Geom(16, 14, 4)
    rng = np.random.default_rng(0xA)
    tile = l1_tile_positions(g)
    first = tile + g.k + 32
    lens = _fill(2 * tile - first, g.k, rng, 100, 700)
    strings = ["A" * first] + ["C" + s[1:-1] + "G" for s in _cut(_text(rng, sum(lens)), lens)]
    return Case("poly-a-tile", "l1", g, strings,
                {"l1_full_tile_one_sg", "string_gt_l1_tile", "string_gt_group", "tail_0", "l2_one_sg"},
                {"l1_partial_tile", "l1_multi_tile"}, env="l2min", canonical=True)


def prefix_strings(rng, k, parts):
    """Strings of exactly k bases: `count` of each (prefix, count) of parts, the prefix followed by bases drawn
    from A, C and G, in a shuffled order.  Under canonical=False every k-mer lies in its prefix's super-bucket.
    The prefixes used here (CAGT, CATA; TTTA, TTTT) hold the strings' only Ts, so no window across two strings
    starts with one of them; CAGT and CATA are not their own reverse complements either (ACGT is: its windows
    would collide with real k-mers under canonical=True)."""
    strings = []
    for prefix, count in parts:
        tails = _text(rng, count * (k - len(prefix)), alphabet=3)
        strings += [prefix + tails[i * (k - len(prefix)):(i + 1) * (k - len(prefix))] for i in range(count)]
    return [strings[i] for i in rng.permutation(len(strings))]


def _l2_cases():
    out = []
    tile = cfg().kDecL2Threads * cfg().kDecL2Per
    plans = (
        ("one", (("CAGT", 2 * tile + 1),), {"l2_one_sg", "l2_last_1"}, {"l2_seam", "l2_far", "l2_first_127"}),
        ("seam", (("CAGT", tile - 48), ("CATA", tile + 48)), {"l2_one_sg", "l2_seam", "l2_last_full"}, {"l2_far", "l2_first_127"}),
        ("last", (("TTTA", tile + 952), ("TTTT", 2 * tile - 952 - 96)), {"l2_one_sg", "l2_seam", "l2_first_127"}, {"l2_far"}),
    )
    for g in (Geom(16, 14, 4), Geom(16, 8, 4)) + WIDE_GEOMS:
        for name, parts, expect, forbid in plans:
            if g.n > cfg().kCoarseBits and name != "last":
                continue
            rng = np.random.default_rng([0x12, g.k, g.n, len(name)])
            expect = set(expect) | {"route_two_level_small", "non_canonical"}
            if g.n > cfg().kCoarseBits:
                expect.add("l2_wide_u%d" % (8 * scatter_bytes(g)))
            else:
                expect.add("l2_lo_bits_%d" % (g.n - cfg().kDecSgBits))
            out.append(Case("l2-%s-%s" % (name, geom_id(g)), "l2", g, prefix_strings(rng, g.k, parts), expect, forbid,
                            env="l2min"))
    return out


def occurrence_strings(rng, k, n_occ, lo, hi):
    """Random strings with exactly n_occ k-mer occurrences: lengths in [lo, hi), the last one what is left."""
    lens = []
    left = n_occ
    while left >= hi:
        lens.append(int(rng.integers(lo, hi)))
        left -= lens[-1] - k + 1
    lens.append(left + k - 1)
    assert min(lens) >= k
    return _cut(_text(rng, sum(lens)), lens)


def _switch_cases():
    """One k-mer occurrence below the default switch of the two scatters, and exactly on it."""
    g = Geom(23, 14, 4)
    at = 1 << cfg().l2_min_default_bits
    out = []
    for n_occ, expect, forbid in ((at - 1, {"route_direct_below_2p20"}, {"route_two_level_at_2p20"}),
                                  (at, {"route_two_level_at_2p20", "l2_last_full", "l2_one_sg", "l2_seam", "l1_tile_all_sg"},
                                   {"route_direct_below_2p20", "l2_far", "route_two_level_small"})):
        rng = np.random.default_rng(0x5117C4)
        out.append(Case("switch-%d" % n_occ, "switch", g, occurrence_strings(rng, g.k, n_occ, 3000, 30000), expect,
                        forbid, env="default"))
    return out


FAMILIES = ("walk", "groups", "l1", "l2", "switch")
_BUILDERS = {"walk": _walk_cases, "groups": _group_cases, "l1": lambda: [_poly_a_case()], "l2": _l2_cases,
             "switch": _switch_cases}
_CASES = {}


def cases(family):
    """The cases of one family, in a fixed order (seeded; built once per process)."""
    if family not in _CASES:
        _CASES[family] = _BUILDERS[family]()
    return _CASES[family]


def all_cases():
    return [c for family in FAMILIES for c in cases(family)]


def case_named(name):
    (c,) = [c for c in all_cases() if c.name == name]
    return c

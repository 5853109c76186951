"""Cases for the staged neighbour probe of the SPSS encode (csrc/ksh_encode.hip): the rc partition (k_rc_hist,
k_rc_columns, k_rc_scatter, k_rc_scatter_l1 / _l2, k_rc_bounds), the reverse-complement half (k_adj_rc1, k_adj_rc)
and the forward half (k_tgt_bounds, k_tgt_split, k_tgt_subcuts, k_adj_fwd_targets), with a numpy model of what the
encode plan and these kernels compute from (K, N, key bytes, the sorted k-mers).

A *case* is a k-mer set built so that something sits on an edge of that arithmetic: a group with exactly rc1_cap
records, a bucket of exactly `cap` keys, a (K-1)-base prefix run across index 2048, a stream of exactly kStreamMax
k-mers.  The builders start from a base set, add engineered k-mers (crowd_group: k-mers whose record lands in one
group; crowd_prefix: k-mers that start with given bases) and loop on the model until it says the edge is hit.

The model (Plan, Probe) is written from the C++ and never calls the library.  It says which branches a case takes
(Probe.branches) and which routes a run must report under a set of switches (Case.routes), so that the GPU test
(tests/test_gpu_probe.py) can assert what it is testing and the CPU test (tests/test_probe_model_cpu.py) that every
branch is reached.  Its neighbour verdicts follow the definition the oracle restates (lib/core/spss.h:238-272), and
the CPU test derives the unitigs from them and compares with the oracle's: that ties the model to a reference.  The
expected strings of the GPU test are the oracle's, never the model's.  The constants and the restated lines are read
from ksh_encode.hip, so a changed constant fails the CPU test instead of moving the cases off their edges."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from kmersets import synth

U = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODE_HIP = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc", "ksh_encode.hip")

Cfg = namedtuple("Cfg", "rows_max window_bytes segs sg_bits l1_threads l2_tile off_cap rc1_slices_max rc1_lds chunk "
                        "chunk64 span tgt_threads")

# the lines of ksh_encode.hip that the model restates
LINES = (
    "} else if (staged_adjacency() && nbits <= 14 && 2 * g->k >= nbits + 4 &&",
    "key_bits(g) >= nbits + 2 + (nbits & 1) &&",
    "n / nb <= 4 * ((kRcWindowBytes - 4 * kRcSegs) / int64_t(sizeof(KeyT) + 6))) {",
    "const int64_t rows = std::max<int64_t>(1, std::min<int64_t>(kRcRowsMax, (n + 16383) / 16384));",
    "const int64_t per_row = ((n + rows - 1) / rows + 1023) / 1024 * 1024;",
    "const bool two_level = n >= (int64_t(1) << (half_groups ? 12 : 20)) && nbits > kSgBits && nbits <= 16 && !one_level;",
    "const int extra = (half_groups && two_level && nbits == 14 && key_bits(g) >= 2 * ((nbits + 1 + 2 + 1) / 2)) ? 1 : 0;",
    "const int64_t per_group = n / ng;",
    "const int cap = int(std::min<int64_t>((kRcWindowBytes - 4 * kRcSegs) / int64_t(sizeof(KeyT) + 6),",
    "std::max<int64_t>(1024, extra ? per_group * 23 / 20 + 256 : per_group * 5 / 4 + 256))) & ~7;",
    "p->routes |= per_group > 4096 ? KSH_ROUTE_RC_1024 : per_group > 1024 ? KSH_ROUTE_RC_512",
    ": per_group > 256 ? KSH_ROUTE_RC_256 : KSH_ROUTE_RC_64;",
    "const int rc1_cap = rc1_marks ? 0 : int(std::min<int64_t>(Rc1Cfg<KeyT>::kCap, (per_group * 4 / 3 + 263) & ~int64_t(7)));",
    "const int pass1_cap = rc1_marks ? -1 : rc1_cap;",
    "while ((1 << rc1_sbits) < kRc1SlicesMax && (2 << rc1_sbits) <= rc1_cap + 1) rc1_sbits++;",
    "static constexpr int kEntryBytes = kPacked ? 8 : int(sizeof(KeyT)) + 6;",
    "static constexpr int kCap = int((kRc1LdsBytes - kRc1SlicesMax * 4) / kEntryBytes) & ~7;",
    "if (r1 - r0 <= int64_t(pass1_cap)) return;  // a group of at most that many records is k_adj_rc1's, both passes",
    "if (pass1_cap >= 0 && threadIdx.x == 0) *taken = 1;  // (ksh_spss_encode_routes: some group did not fit k_adj_rc1)",
    "if (!batched && r1 - r0 > int64_t(cap)) return;  // k_adj_rc has this group",
    "if (r1 - r0 > int64_t(cap) && threadIdx.x == 0) *took_batches = 1;  // (ksh_spss_encode_routes)",
    "const int rest_bits = 2 * set.k - 4 - gbits;  // bits of a record key between its top base and its last base",
    "const int e_sbits = sbits < rest_bits ? sbits : rest_bits;",
    "const int len = int(len64 < int64_t(cap) + 1 ? len64 : int64_t(cap) + 1);",
    "if (total <= cap) {",
    "const int take = int(avail < int64_t(cap - used) ? avail : int64_t(cap - used));",
    "if (pos < bt.seg_hi[seg]) break;  // the window is full",
    "if (lg > seg_bits - 2) lg = seg_bits - 2 > 0 ? seg_bits - 2 : 0;",
    "const int seg_bits = (pass == 0 ? set.key_bits : set.key_bits - 4) - extra;",
    "const int n_span = int(min<int64_t>(b_last - b_first + 1, kOffCap + 1));",
    "if (g - base_g < n_bins) {",
    "const int first = __ffsll((long long)(m & 0x1Eull)) - 1;  // 1 .. 4 (a prefix has at most four k-mers)",
    "const int64_t m = (stream + stream_max - 1) / stream_max;",
    "if (len > best_len) {",
    "const int64_t pos = lo_c[2 + best] + int64_t((uint64_t(best_len) * uint64_t(t.j)) / uint64_t(t.m));  // (< 2^31 * 2^31)",
    "static constexpr int kStreamMax = 2 * kChunk;",
    "const int64_t n_chunks = (n + kTgtChunk - 1) / kTgtChunk;",
    "my_b = j < kTgtSpan ? int64_t(s_fb[a] + j) : set.bucket_of(int64_t(p32));",
    "if (jw >= 0 && jw < kTgtSpan) {",
    "if (at == p32) continue;  // Next(x, c) == x",
    "if ((((kf >> 2) & hi_mask) << 2 | (kf & 3)) == want && t != uint32_t(i)) {  // (t == i: y = Next(rc(y), c), the k-mer itself)",
    "if ((kf >> 2) == want && t != uint32_t(i)) {  // (t == i: rc(z) = Next(z, c'), the k-mer itself)",
    "if (wlen == 0 || rz < z || z == x) continue;  // not staged now; not canonical (cannot be in the set); x itself",
    "if (d < 4 && p0_win_lo + uint32_t(i) != rr.t) mark_hit(&slots[i], mark);",
    "if (atomicCAS(slot, kNone, v) != kNone) *reinterpret_cast<volatile uint32_t*>(slot) = kMulti;",
    "if (*reinterpret_cast<const int*>(at_tail(offsetof(EncCtl, tgt_extra))) > 0) p->routes |= KSH_ROUTE_TGT_PARTS;",
)


def constants(text=None):
    """Cfg from ksh_encode.hip; the lines the model restates must stand there as written."""
    if text is None:
        text = open(ENCODE_HIP).read()

    def num(pattern):
        m = re.search(pattern, text)
        if m is None:
            raise AssertionError("ksh_encode.hip no longer has what the model reads: " + pattern)
        return int(m.group(1), 0)

    l2 = num(r"constexpr int kL2Threads = (\d+);") * num(r"constexpr int kL2Per = (\d+);")
    cfg = Cfg(num(r"constexpr int64_t kRcRowsMax = (\d+);"), num(r"constexpr int64_t kRcWindowBytes = (\d+) << 10;") << 10,
              num(r"constexpr int kRcSegs = (\d+);"), num(r"constexpr int kSgBits = (\d+);"),
              num(r"constexpr int kL1Threads = (\d+);"), l2, num(r"constexpr int kOffCap = (\d+);"),
              num(r"constexpr int kRc1SlicesMax = (\d+);"), num(r"constexpr int kRc1LdsBytes = (\d+);"),
              num(r"#define KSH_TGT_CHUNK (\d+)"), num(r"#define KSH_TGT_CHUNK64 (\d+)"),
              num(r"constexpr int kTgtSpan = (\d+);"), num(r"#define KSH_TGT_THREADS (\d+)"))
    for line in LINES:
        if line not in text:
            raise AssertionError("ksh_encode.hip no longer has the line the model restates: " + line)
    return cfg


_CFG = []


def cfg():
    if not _CFG:
        _CFG.append(constants())
    return _CFG[0]


# ---- the switch sets -------------------------------------------------------------------------------------------------
ENVS = {
    "default": {},
    "marks": {"KSH_RC1": "marks"},
    "batched": {"KSH_RC1": "batched"},
    "half": {"KSH_RC_GROUPS": "half"},
    "half+direct": {"KSH_RC_GROUPS": "half", "KSH_RC_SCATTER": "direct"},
    "staged": {"KSH_FWD": "staged"},
    "probe": {"KSH_FWD": "probe"},
}


# ---- the plan ----------------------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "k nbits kb n key_bits staged rows per_row two_level extra gbits ng per_group threads cap "
                          "rc1_kcap rc1_cap pass1_cap rc1_mode rc1_sbits rest_bits e_sbits fwd_mode chunk stream_max "
                          "n_chunks rec_bytes")


def rc1_kcap(kb, c=None):
    """Rc1Cfg<KeyT>::kCap."""
    c = c or cfg()
    return ((c.rc1_lds - c.rc1_slices_max * 4) // (8 if kb <= 4 else kb + 6)) & ~7


def plan(k, nbits, kb, n, env=None, c=None):
    """The block after staged_adjacency() of the encode plan, for a canonical set of n k-mers at <K, N, key bytes>
    under the switches env (a dict of environment variables)."""
    c = c or cfg()
    env = env or {}
    key_bits = 2 * k - nbits
    nb = 1 << nbits
    window_keys = (c.window_bytes - 4 * c.segs) // (kb + 6)
    staged = (env.get("KSH_ADJACENCY") != "probe" and nbits <= 14 and 2 * k >= nbits + 4 and
              key_bits >= nbits + 2 + (nbits & 1) and n // nb <= 4 * window_keys)
    rows = max(1, min(c.rows_max, (n + 16383) // 16384))
    per_row = ((n + rows - 1) // rows + 1023) // 1024 * 1024
    half = env.get("KSH_RC_GROUPS") == "half"
    one_level = env.get("KSH_RC_SCATTER") == "direct"
    two_level = n >= (1 << (12 if half else 20)) and nbits > c.sg_bits and nbits <= 16 and not one_level
    extra = 1 if (half and two_level and nbits == 14 and key_bits >= 2 * ((nbits + 1 + 2 + 1) // 2)) else 0
    gbits = nbits + extra
    ng = 1 << gbits
    per_group = n // ng
    threads = 1024 if per_group > 4096 else 512 if per_group > 1024 else 256 if per_group > 256 else 64
    cap = min(window_keys, max(1024, per_group * 23 // 20 + 256 if extra else per_group * 5 // 4 + 256)) & ~7
    rc1_mode = {"marks": "marks", "batched": "batched"}.get(env.get("KSH_RC1"), "default")
    kcap = rc1_kcap(kb, c)
    rc1_cap = 0 if rc1_mode == "marks" else min(kcap, (per_group * 4 // 3 + 263) & ~7)
    pass1_cap = -1 if rc1_mode == "marks" else rc1_cap
    sbits = 6
    while (1 << sbits) < c.rc1_slices_max and (2 << sbits) <= rc1_cap + 1:
        sbits += 1
    rest_bits = 2 * k - 4 - gbits
    fwd_mode = {"probe": "probe", "staged": "staged"}.get(env.get("KSH_FWD"), "targets")
    chunk = c.chunk64 if kb == 8 else c.chunk
    return Plan(k, nbits, kb, n, key_bits, staged, rows, per_row, two_level, extra, gbits, ng, per_group, threads, cap,
                kcap, rc1_cap, pass1_cap, rc1_mode, sbits, rest_bits, min(sbits, rest_bits), fwd_mode, chunk, 2 * chunk,
                (n + chunk - 1) // chunk, 8 if kb <= 4 else 16)


# ---- helpers that older tests share ---------------------------------------------------------------------------------
# Rc1Cfg<KeyT>::kCap (csrc/ksh_encode.hip): (kRc1LdsBytes - kRc1SlicesMax * 4) / entry bytes, a multiple of 8;
# an entry is one 8-byte word for 2- and 4-byte keys, key + 6 bytes for 8-byte keys
RC1_CAP = {2: (81408 - 4096 * 4) // 8 & ~7, 4: (81408 - 4096 * 4) // 8 & ~7, 8: (81408 - 4096 * 4) // 14 & ~7}


def rc_shape(n, nbits, kb):
    """(per_group, threads route, rc1_cap) as the encode plan computes them for a staged probe without half groups."""
    per_group = n >> nbits
    threads = "rc_1024" if per_group > 4096 else "rc_512" if per_group > 1024 else "rc_256" if per_group > 256 else "rc_64"
    return per_group, threads, min(RC1_CAP[kb], (per_group * 4 // 3 + 263) & ~7)


def records_per_group(kmers, k, nbits):
    """How many rc records each group gets: x's record is rc(x), grouped by the nbits below its top base
    (csrc/ksh_encode.hip, k_rc_hist)."""
    return np.bincount(group_of(kmers, k, nbits).astype(np.int64), minlength=1 << nbits)


def group_of(kmers, k, gbits):
    rx = synth.revcomp(kmers, k)
    return (rx >> U(2 * k - 2 - gbits)) & U((1 << gbits) - 1)


def cuts_of(s, k, chunk):
    """(b, v) per cut as k_tgt_bounds finds them: b = the first index >= c * chunk where the prefix changes."""
    pref = s >> U(2)
    n = s.size
    n_chunks = (n + chunk - 1) // chunk
    b, v = [0], [0]
    for c in range(1, n_chunks + 1):
        at = c * chunk
        while at < n and pref[at] == pref[at - 1]:
            at += 1
        if at >= n:
            b.append(n)
            v.append(1 << (2 * k - 2))
        else:
            b.append(at)
            v.append(int(pref[at]))
    return b, v


def cuts_with_first(s, k, chunk):
    """cuts_of, and per cut the offset `first` (1 .. 4) that k_tgt_bounds' ballot finds: the cut lies at index
    c * chunk - 1 + first (0 for cut 0; a cut past the end of the set is clamped to n afterwards)."""
    b, v = cuts_of(s, k, chunk)
    first = [0]
    for c in range(1, len(b)):
        first.append(min(4, max(1, b[c] - (c * chunk - 1))) if c * chunk <= s.size else 1)
    return b, v, first


# ---- the model ---------------------------------------------------------------------------------------------------------
def _lb(km, values):
    """First index of km whose k-mer is >= value (lower_bound_kmer), for Python ints or an array of them."""
    return np.searchsorted(km, np.asarray(values, dtype=U), side="left").astype(np.int64)


def rc_batches(lens, cap):
    """k_adj_rc's batches of one pass over ranges of these lengths: (fits, [(used, {range: take})], take0) -- fits:
    the sixteen lanes lay the one batch out; else plan_serial's batches, and take0: some batch filled the window
    exactly at a range's end, so the next non-empty range got take = 0 there and starts the next batch."""
    total = sum(min(int(x), cap + 1) for x in lens)
    if total <= cap:
        return True, [(total, {s: int(x) for s, x in enumerate(lens) if x})], False
    batches, seg, pos, take0 = [], 0, 0, False
    while seg < len(lens):
        used, takes = 0, {}
        while seg < len(lens):
            avail = int(lens[seg]) - pos
            take = min(avail, cap - used)
            if take == 0 and avail > 0:
                take0 = True
            if take:
                takes[seg] = take
            used += take
            pos += take
            if pos < lens[seg]:
                break
            seg += 1
            pos = 0
        batches.append((used, takes))
    return False, batches, take0


COMBOS = tuple("s%d:d%dr%d" % (s, d, r) for s in (0, 1) for d in (0, 1, 2) for r in (0, 1, 2))


class Probe:
    """What the staged probe does with one canonical set at <K, N, key bytes> under a set of switches."""

    def __init__(self, kmers, k, nbits, kb, env=None):
        self.km = np.ascontiguousarray(kmers, dtype=U)
        assert k <= 31 and (np.diff(self.km.astype(np.int64)) > 0).all(), "an ascending set of k-mers of at most 62 bits"
        self.k, self.nbits, self.kb = k, nbits, kb
        self.n = int(self.km.size)
        self.env = dict(env or {})
        self.plan = plan(k, nbits, kb, self.n, self.env)
        assert self.plan.staged, "the case is outside the staged probe"
        self._groups = self._windows = self._verdicts = None

    # -- item 2: the groups -----------------------------------------------------------------------------------------
    def groups(self):
        """rec[G], p0[G] (pass 0's range: bucket G, or half of it), p1[G][16] (the ranges [c][tb][G])."""
        if self._groups is None:
            p, k = self.plan, self.k
            rec = records_per_group(self.km, k, p.gbits)
            p0 = np.diff(_lb(self.km, np.arange(p.ng + 1, dtype=U) << U(2 * k - p.gbits)))
            p1 = np.diff(_lb(self.km, np.arange(16 * p.ng + 1, dtype=U) << U(2 * k - 4 - p.gbits)))
            self._groups = (rec, p0, p1.reshape(16, p.ng).T.copy())
        return self._groups

    def takers(self):
        """Per group, the kernel that probes it: True = k_adj_rc (records looking for k-mers, marks)."""
        rec = self.groups()[0]
        mode = self.plan.rc1_mode
        if mode == "marks":
            return np.ones(rec.size, dtype=bool)
        if mode == "batched":
            return np.zeros(rec.size, dtype=bool)
        return rec > self.plan.rc1_cap

    def rc_passes(self):
        """For every group of k_adj_rc whose pass does not fit one batch: {(G, pass): rc_batches(...)}."""
        rec, p0, p1 = self.groups()
        cap, by = self.plan.cap, self.takers()
        out = {}
        for g in np.flatnonzero(by & (p0 > cap)):
            out[(int(g), 0)] = rc_batches([p0[g]], cap)
        for g in np.flatnonzero(by & (np.minimum(p1, cap + 1).sum(axis=1) > cap)):
            out[(int(g), 1)] = rc_batches(p1[g].tolist(), cap)
        return out

    # -- item 3: the windows of the forward half ------------------------------------------------------------------------
    def windows(self):
        """The workgroups of k_adj_fwd_targets: a dict of arrays over the parts (a window whose stream is short is
        one part), and per window m and first."""
        if self._windows is None:
            p, k, km = self.plan, self.k, self.km
            b, v, first = cuts_with_first(km, k, p.chunk)
            top = 1 << (2 * k - 2)
            sb = np.stack([_lb(km, [(a * top) + x for x in v]) for a in range(4)], axis=1)  # [cut][a]
            lens = np.diff(sb, axis=0)                                                       # [window][a]
            stream = lens.sum(axis=1)
            m = (stream + p.stream_max - 1) // p.stream_max
            edges, owner, tie, one_top = [], [], [], []
            for c in range(len(b) - 1):
                edges.append(v[c])
                owner.append(c)
                if m[c] > 1:
                    best = int(np.argmax(lens[c]))  # the first of the longest
                    tie.append(int((lens[c] == lens[c][best]).sum()) > 1)
                    one_top.append(int((lens[c] > 0).sum()) == 1)
                    for j in range(1, int(m[c])):
                        pos = int(sb[c][best]) + int(lens[c][best]) * j // int(m[c])
                        edges.append(int(km[pos]) & (top - 1))
                        owner.append(c)
            edges.append(v[-1])
            assert all(x <= y for x, y in zip(edges[:-1], edges[1:]))  # (equal: the cuts past the end of the set)
            V = np.array(edges, dtype=U)
            wlo = _lb(km, [x << 2 for x in edges])
            wlo[-1] = self.n
            slo = np.stack([_lb(km, [(a * top) + x for x in edges]) for a in range(4)], axis=1)
            self._windows = dict(b=b, v=v, first=first, stream=stream, m=m, lens=lens, V=V, owner=np.array(owner),
                                 win_len=np.diff(wlo), win_lo=wlo[:-1], part_lens=np.diff(slo, axis=0), tie=tie,
                                 one_top=one_top)
        return self._windows

    # -- item 4: the verdicts, by the definition ---------------------------------------------------------------------------
    def verdicts(self):
        """Per side (0: left, Prev; 1: right, Next) and k-mer: nd (direct neighbours), nr (through a reverse
        complement), the single neighbour's index and whether it is reached through a reverse complement, and the
        self-hits a k-mer never counts: self_direct (Next(x, c) == x), self_rc (the canonical form of the candidate
        is x itself: x's (K-1)-base prefix, side 0, or suffix, side 1, is its own reverse complement)."""
        if self._verdicts is None:
            km, k, n = self.km, self.k, self.n
            mask = U((1 << (2 * k)) - 1)
            nd = np.zeros((2, n), dtype=np.int64)
            nr = np.zeros((2, n), dtype=np.int64)
            single = np.full((2, n), -1, dtype=np.int64)
            via_rc = np.zeros((2, n), dtype=bool)
            self_direct = np.zeros((2, n), dtype=bool)
            self_rc = np.zeros((2, n), dtype=bool)
            for side in (0, 1):
                for c in range(4):
                    y = (((km << U(2)) & mask) | U(c)) if side else ((km >> U(2)) | (U(c) << U(2 * (k - 1))))
                    z = synth.canonical(y, k)
                    pos = np.minimum(np.searchsorted(km, z), max(n - 1, 0))
                    hit = (km[pos] == z) & (z != km)
                    nd[side] += hit & (z == y)
                    nr[side] += hit & (z != y)
                    single[side] = np.where(hit, pos, single[side])
                    via_rc[side] = np.where(hit, z != y, via_rc[side])
                    self_direct[side] |= y == km
                    self_rc[side] |= (z == km) & (y != km)
            self._verdicts = dict(nd=nd, nr=nr, single=single, via_rc=via_rc, self_direct=self_direct, self_rc=self_rc)
        return self._verdicts

    def combined(self):
        """Per side and k-mer: -1 none, -2 several, else the index of the single neighbour."""
        v = self.verdicts()
        tot = v["nd"] + v["nr"]
        return np.where(tot == 0, -1, np.where(tot > 1, -2, v["single"]))

    def links(self):
        """succ[s] of every state s = 2 t + d (d = 0 leaves through the right side), -1 where the side has no link:
        two k-mers are linked where each is the other's single neighbour on the facing sides."""
        v, n = self.verdicts(), self.n
        comb = self.combined()
        succ = np.full(2 * n, -1, dtype=np.int64)
        for side in (0, 1):
            y = comb[side]
            ok = y >= 0
            ys = np.maximum(y, 0)
            facing = np.where(v["via_rc"][side], side, 1 - side)  # through a reverse complement: the same side of y
            back = comb[facing, ys]
            ok &= back == np.arange(n)
            # the state of y that the walk goes on in: leaving y through the side opposite to the facing one
            nxt = 2 * ys + np.where(facing == 0, 0, 1)
            succ[(0 if side else 1)::2] = np.where(ok, nxt, -1)
        return succ

    def unitig_strings(self):
        """The unitigs that follow from the combined verdicts, in the encode's order (the chain walking, the choice
        of the spelled direction and the order are chain_rank_cases.Profile's, which the chain-ranking sweep ties to
        the oracle; the links are this model's)."""
        import chain_rank_cases as crc

        succ = self.links()
        prof = crc.Profile.__new__(crc.Profile)
        prof.k, prof.canonical, prof.km, prof.n = self.k, True, self.km, self.n
        prof.succ = succ.tolist()
        has_pred = np.zeros(2 * self.n, dtype=bool)
        has_pred[succ[succ >= 0]] = True
        prof.has_pred = has_pred.tolist()
        prof._unitigs()
        return prof.unitig_strings()

    # -- item 5 --------------------------------------------------------------------------------------------------------------
    def branches(self):
        p, k, n = self.plan, self.k, self.n
        c = cfg()
        out = set()
        rec, p0, p1 = self.groups()
        by_rc = self.takers()
        by_rc1 = ~by_rc
        any_range = (p0 > 0) | (p1.sum(axis=1) > 0)
        v = self.verdicts()
        # ---- A: k_adj_rc1 and the split
        if ((rec == 0) & any_range).any():
            out.add("g:no_records_but_ranges")
        if ((rec > 0) & (p0 == 0)).any():
            out.add("g:records_empty_pass0")
        if ((rec > 0) & (p1.sum(axis=1) == 0)).any():
            out.add("g:records_sixteen_empty")
        if p.rc1_mode == "default":
            if (rec == p.rc1_cap).any():
                out.add("split:at_rc1_cap")
            if (rec == p.rc1_cap + 1).any():
                out.add("split:rc1_cap+1")
            out.add("route:rc_marks_groups" if by_rc.any() else "route:no_rc_marks_groups")
        if by_rc1.any():
            r1 = rec[by_rc1]
            for name, want in (("4T-1", 4 * p.threads - 1), ("4T", 4 * p.threads), ("4T+1", 4 * p.threads + 1)):
                if (r1 == want).any():
                    out.add("rc1:records_" + name)
            if (r1 > 0).any():
                out.add("rc1:rest0" if p.rest_bits == 0 else "rc1:rest<sbits" if p.rest_bits < p.rc1_sbits else
                        "rc1:rest>sbits" if p.rest_bits > p.rc1_sbits else "rc1:rest=sbits")
                out.add("rc1:sbits%d" % p.rc1_sbits)
                wide = self.kb > (2 if p.key_bits <= 16 else 4 if p.key_bits <= 32 else 8)
                out.add("rc1:rkey_rt_nxt" if self.kb == 8 else "rc1:packed%d%s" % (self.kb, "_wide" if wide else ""))
                out.add("rc1:T%d:kb%d" % (p.threads, self.kb))
            # one chain walk that returns "several": pass 0, records that differ in their top base only (what reaches
            # side 0 of y through a reverse complement; y's group is its top gbits), pass 1, in their last base only
            g0 = (self.km >> U(2 * k - p.gbits)).astype(np.int64)
            g1 = ((self.km >> U(2 * k - 4 - p.gbits)) & U(p.ng - 1)).astype(np.int64)
            if ((v["nr"][0] >= 2) & by_rc1[g0]).any():
                out.add("rc1:several_top_base")
            if ((v["nr"][1] >= 2) & by_rc1[g1]).any():
                out.add("rc1:several_last_base")
            if p.rc1_mode == "batched":
                nb = (rec + p.rc1_cap - 1) // p.rc1_cap
                if (nb == 2).any():
                    out.add("rc1:batches2")
                if (nb >= 3).any():
                    out.add("rc1:batches3+")
        # ---- B: k_adj_rc
        if by_rc.any():
            cap = p.cap
            out.add("rc:T%d:kb%d" % (p.threads, self.kb))
            q0, q1 = p0[by_rc], p1[by_rc]
            s1 = q1.sum(axis=1)
            fits1 = np.minimum(q1, cap + 1).sum(axis=1) <= cap
            for name, hit in (("rc:p0_at_cap", q0 == cap), ("rc:p0_cap+1", q0 == cap + 1), ("rc:p0_gt_2cap", q0 > 2 * cap),
                              ("rc:p0_fits", q0 <= cap), ("rc:p0_batched", q0 > cap),
                              ("rc:p1_at_cap", s1 == cap), ("rc:p1_cap+1", s1 == cap + 1),
                              ("rc:p1_fits", fits1), ("rc:p1_batched", ~fits1),
                              ("rc:p1_one_full_fifteen_empty", ((q1 > 0).sum(axis=1) == 1) & (q1.max(axis=1) == cap))):
                if hit.any():
                    out.add(name)
            inner = (q1[:, 1:-1] > cap) & (q1[:, :-2] == 0) & (q1[:, 2:] == 0)
            if inner.any():
                out.add("rc:p1_range_split")
            passes = self.rc_passes()
            for (g, ps), (fits, batches, take0) in passes.items():
                if ps == 1 and take0:
                    out.add("rc:p1_batch_ends_at_range_end")
                if ps == 0 and len(batches) >= 3:
                    out.add("rc:p0_three_batches")
                if ps == 0 and len(batches) == 2:
                    out.add("rc:p0_two_batches")
                if self.kb == 2:
                    out.add("rc:kb2_full_window_cap%%16=%d" % (cap % 16))
            out.add("route:rc_batched" if passes else "route:no_rc_batched")
            for ps, lens in ((0, q0), (1, q1)):
                seg_bits = (p.key_bits if ps == 0 else p.key_bits - 4) - p.extra
                if seg_bits - 2 < 0 and (lens >= 1).any():  # (lg = 0 > seg_bits - 2 whatever the range holds)
                    out.add("rc:slice_lg_clamped_to_0")
                lens = np.minimum(lens[lens >= 2], cap)
                if lens.size:
                    lg = np.floor(np.log2(lens)).astype(np.int64)
                    if seg_bits - 2 <= 0:
                        out.add("rc:slice_lg_clamped_to_0")
                    else:
                        if (lg > seg_bits - 2).any():
                            out.add("rc:slice_lg_clamped")
                        if (lg <= seg_bits - 2).any():
                            out.add("rc:slice_lg_unclamped")
            if self.kb == 2:
                out.add("rc:kb2_cap%%16=%d" % (cap % 16))
        elif p.rc1_mode == "batched":
            out.add("route:rc_batched" if (rec > p.rc1_cap).any() else "route:no_rc_batched")
        else:
            out.add("route:no_rc_batched")
        # ---- C: the partition
        out.add("part:two_level" if p.two_level else "part:one_level")
        out.add("part:records%d" % p.rec_bytes)
        if (rec > 0).sum() == 1:
            out.add("part:one_group_has_all")
        if (rec > 0).all():
            out.add("part:every_group_has_records")
        if n % 1024 == 1023:
            out.add("part:n=1024j-1")
        if n % 1024 == 1:
            out.add("part:n=1024j+1")
        for size in (16384, 16385, 32769):
            if n == size:
                out.add("part:n=%d" % size)
        if p.rows >= 2 and n - (p.rows - 1) * p.per_row <= 0:
            out.add("part:empty_last_row")
        if self.env.get("KSH_RC_SCATTER") == "direct":
            out.add("part:direct")
        if p.two_level:
            out.add("part:extra1" if p.extra else "part:extra0")
            out.add("part:two_level_N=14" if self.nbits == 14 else "part:two_level_N<14")
            bucket = (self.km >> U(p.key_bits)).astype(np.int64)
            lo_bits = p.gbits - c.sg_bits
            sg = (group_of(self.km, k, p.gbits) >> U(lo_bits)).astype(np.int64)
            tile1 = c.l1_threads * (4 if p.rec_bytes == 8 else 2)
            for r in range(p.rows):
                t0, t1 = r * p.per_row, min((r + 1) * p.per_row, n)
                if t0 >= t1:
                    continue
                span = bucket[t1 - 1] - bucket[t0] + 1
                out.add("l1:offsets_not_staged" if span > c.off_cap else "l1:offsets_staged")
                if span == 1:
                    out.add("l1:row_in_one_bucket")
                for a in range(t0, t1, tile1):
                    if np.unique(sg[a:min(a + tile1, t1)]).size == 1:
                        out.add("l1:tile_one_super_group")
            order = np.sort(sg, kind="stable")  # the intermediate array: by super-group
            for a in range(0, n, c.l2_tile):
                tile = order[a:a + c.l2_tile]
                base = tile[0]
                kinds = np.unique(tile).size
                if kinds == 1:
                    out.add("l2:tile_one_super_group")
                if kinds == 2 and tile[-1] == base + 1:
                    out.add("l2:tile_at_a_seam")
                if (tile - base >= 2).any():
                    out.add("l2:tile_three_super_groups")
        # ---- D: the forward half
        w = self.windows()
        n_cuts = len(w["b"]) - 1
        for cc in range(1, n_cuts):
            out.add("fwd:first%d" % w["first"][cc])
        for cc in range(n_cuts):
            if w["b"][cc + 1] - w["b"][cc] == p.chunk + 3:
                out.add("fwd:window_chunk+3")
            if cc >= 1 and w["b"][cc] == n:
                out.add("fwd:run_reaches_end")
        for size, name in ((p.chunk, "chunk"), (p.chunk + 1, "chunk+1"), (2 * p.chunk, "2chunk"), (2 * p.chunk + 1, "2chunk+1")):
            if n == size:
                out.add("fwd:n=" + name)
        if n < p.chunk:
            out.add("fwd:one_window")
        if (w["stream"] == p.stream_max).any():
            out.add("fwd:stream_at_max")
        if (w["stream"] == p.stream_max + 1).any():
            out.add("fwd:stream_max+1")
        if (w["m"] == 2).any():
            out.add("fwd:m2")
        if (w["m"] >= 3).any():
            out.add("fwd:m3+")
        out.add("route:tgt_parts" if (w["m"] > 1).any() else "route:no_tgt_parts")
        if any(w["tie"]):
            out.add("fwd:tie_of_longest_ranges")
        if any(w["one_top"]):
            out.add("fwd:one_top_base_streams_all")
        part_stream = w["part_lens"].sum(axis=1)
        split = (w["m"] > 1)[w["owner"]]
        if (split & (w["win_len"] == 0) & (part_stream > 0)).any():
            out.add("fwd:part_empty_window")
        if ((w["win_len"] > 0) & (part_stream == 0)).any():
            out.add("fwd:empty_stream")
        if ((w["win_len"] == 0) & (part_stream == 0)).any():
            out.add("fwd:empty_window_and_stream")
        # buckets: of the window's keys, of the targets (slot jw of the window's table), of the stream's k-mers
        if n:
            key_bits = p.key_bits
            fb_w = ((w["V"][:-1] << U(2)) >> U(key_bits)).astype(np.int64)
            bucket = (self.km >> U(key_bits)).astype(np.int64)
            for i in np.flatnonzero(w["win_len"] > 0):
                lo, hi = int(w["win_lo"][i]), int(w["win_lo"][i] + w["win_len"][i])
                if bucket[hi - 1] == bucket[lo]:
                    out.add("fwd:window_in_one_bucket")
                if bucket[hi - 1] - fb_w[i] >= c.span:
                    out.add("fwd:window_over_span")
            suffix = self.km & U((1 << (2 * k - 2)) - 1)
            part = np.searchsorted(w["V"], suffix, side="right") - 1
            jw = ((suffix << U(2)) >> U(key_bits)).astype(np.int64) - fb_w[part]
            found = v["nd"][1] > 0
            if (found & (jw == c.span - 1)).any():
                out.add("fwd:target_in_slot15")
            if (found & (jw >= c.span)).any():
                out.add("fwd:target_in_slot16+")
            if (found & (jw < c.span - 1)).any():
                out.add("fwd:target_in_table")
            topb = (self.km >> U(2 * k - 2)).astype(np.int64)
            fb_s = (((topb.astype(U) << U(2 * k - 2)) | w["V"][part]) >> U(key_bits)).astype(np.int64)
            out.add("fwd:stream_bucket_searched" if (bucket - fb_s >= c.span).any() else "fwd:stream_buckets_in_table")
        # the verdict classes and the self-hits
        for side in (0, 1):
            d, r = np.minimum(v["nd"][side], 2), np.minimum(v["nr"][side], 2)
            for cls in np.unique(d * 3 + r):
                out.add("s%d:d%dr%d" % (side, cls // 3, cls % 3))
        if v["self_direct"].any():
            out.add("self:next_is_itself")
        if v["self_rc"][0].any():
            out.add("self:prefix_is_its_own_rc")
        if v["self_rc"][1].any():
            out.add("self:suffix_is_its_own_rc")
        return out


A_BRANCHES = ("g:no_records_but_ranges", "g:records_empty_pass0", "g:records_sixteen_empty", "split:at_rc1_cap",
              "split:rc1_cap+1", "rc1:records_4T-1", "rc1:records_4T", "rc1:records_4T+1", "rc1:rest0", "rc1:rest<sbits",
              "rc1:rest>sbits", "rc1:sbits8", "rc1:sbits9", "rc1:sbits10", "rc1:sbits11", "rc1:sbits12", "rc1:packed2",
              "rc1:packed4", "rc1:packed4_wide", "rc1:rkey_rt_nxt", "rc1:several_top_base", "rc1:several_last_base") + \
    tuple("rc1:T%d:kb%d" % (t, kb) for t in (64, 256, 512, 1024) for kb in (2, 4, 8))
B_BRANCHES = ("rc:p0_at_cap", "rc:p0_cap+1", "rc:p0_gt_2cap", "rc:p0_two_batches", "rc:p0_three_batches", "rc:p1_at_cap",
              "rc:p1_cap+1", "rc:p1_batch_ends_at_range_end", "rc:p1_range_split", "rc:p1_one_full_fifteen_empty",
              "rc:slice_lg_clamped_to_0", "rc:slice_lg_clamped", "rc:slice_lg_unclamped", "rc:kb2_cap%16=0",
              "rc:kb2_cap%16=8", "rc:kb2_full_window_cap%16=0", "rc:kb2_full_window_cap%16=8", "rc:T64:kb2", "rc:T64:kb4")
C_BRANCHES = ("part:one_level", "part:two_level", "part:one_group_has_all", "part:every_group_has_records",
              "part:n=1024j-1", "part:n=1024j+1", "part:n=16384", "part:n=16385", "part:n=32769", "part:records8",
              "part:records16", "part:extra1", "part:extra0", "part:two_level_N=14", "part:two_level_N<14", "part:direct",
              "l1:offsets_not_staged", "l1:offsets_staged", "l1:row_in_one_bucket", "l1:tile_one_super_group",
              "l2:tile_one_super_group", "l2:tile_at_a_seam", "l2:tile_three_super_groups")
D_BRANCHES = ("fwd:first1", "fwd:first2", "fwd:first3", "fwd:first4", "fwd:window_chunk+3", "fwd:n=chunk", "fwd:n=chunk+1",
              "fwd:n=2chunk", "fwd:n=2chunk+1", "fwd:run_reaches_end", "fwd:one_window", "fwd:window_in_one_bucket",
              "fwd:window_over_span", "fwd:target_in_slot15", "fwd:target_in_slot16+", "fwd:stream_bucket_searched",
              "fwd:stream_at_max", "fwd:stream_max+1", "fwd:m2", "fwd:m3+", "fwd:part_empty_window", "fwd:empty_stream",
              "fwd:tie_of_longest_ranges", "fwd:one_top_base_streams_all", "self:next_is_itself",
              "self:prefix_is_its_own_rc", "self:suffix_is_its_own_rc") + \
    tuple("s%d:d%dr%d" % (s, d, r) for s in (0, 1) for (d, r) in ((1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (2, 2)))
E_BRANCHES = ("rc1:batches2", "rc1:batches3+")
OPPOSITES = (("rc:p0_fits", "rc:p0_batched"), ("rc:p1_fits", "rc:p1_batched"), ("route:tgt_parts", "route:no_tgt_parts"),
             ("route:rc_marks_groups", "route:no_rc_marks_groups"), ("route:rc_batched", "route:no_rc_batched"))
BRANCHES = A_BRANCHES + B_BRANCHES + C_BRANCHES + D_BRANCHES + E_BRANCHES + tuple(x for pair in OPPOSITES for x in pair)
# What the issue's list names and no input reaches, with the reason.
UNREACHABLE = {
    "a part, cut from a long stream, with a non-empty window and an empty stream":
        "k_tgt_subcuts cuts at the quantiles of the LONGEST stream range, which holds a quarter of more than kStreamMax "
        "k-mers, so every part streams at least floor(best_len / m) >= 1 k-mers of it; a whole window without a stream "
        "is reachable and pinned (fwd:empty_stream)",
}


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """name, (K, N, key bytes), the set (ascending uint64), the branches the model must (expect) and must not
    (forbid) report under the case's home switch set `env` (a key of ENVS), and the other switch sets it runs
    under as well (also)."""

    def __init__(self, name, k, nbits, kb, kmers, expect, forbid=(), env="default", also=()):
        self.name, self.k, self.nbits, self.kb = name, k, nbits, kb
        self.kmers = np.ascontiguousarray(kmers, dtype=U)
        self.expect, self.forbid, self.env, self.also = frozenset(expect), frozenset(forbid), env, tuple(also)
        self._models = {}

    def model(self, env=None):
        env = env or self.env
        if env not in self._models:
            self._models[env] = Probe(self.kmers, self.k, self.nbits, self.kb, ENVS[env])
        return self._models[env]

    def branches(self, env=None):
        return self.model(env).branches()

    def envs(self):
        return (self.env,) + self.also

    def routes(self, env=None):
        """(route names the encode must report, names it must not) under the switch set env."""
        m = self.model(env)
        p, b = m.plan, m.branches()
        must, never = {"probe_staged"}, set()
        for t in (64, 256, 512, 1024):
            (must if t == p.threads else never).add("rc_%d" % t)
        (must if p.two_level else never).add("scatter_two_level")
        (never if p.rc1_mode == "marks" else must).add("rc1_streamed")
        (must if "route:rc_marks_groups" in b else never).add("rc_marks_groups")
        (must if "route:rc_batched" in b else never).add("rc_batched")
        (must if p.fwd_mode == "targets" else never).add("fwd_targets")
        (must if p.fwd_mode == "staged" else never).add("fwd_staged")
        (must if p.fwd_mode == "targets" and "route:tgt_parts" in b else never).add("tgt_parts")
        return must, never


def finish(kmers, k):
    """Canonical forms, without the k-mers that are their own reverse complement, ascending."""
    x = np.asarray(kmers, dtype=U)
    r = synth.revcomp(x, k)
    return np.unique(np.minimum(x, r)[x != r])


def genome(k, size, seed):
    """The canonical k-mers of a random genome (a little under `size` of them): chains with a few branches."""
    return finish(synth.phylogeny_sets(k, 1, size, seed=seed)[0], k)


def dense(k, size, seed):
    """`size` canonical k-mers drawn evenly: at small K a dense graph with every kind of junction."""
    rng = np.random.default_rng([0xD3, k, seed])
    x = finish(rng.integers(0, 4 ** k, size=4 * size + 64, dtype=np.uint64), k)
    return np.sort(rng.permutation(x)[:size]) if x.size > size else x


def trimmed(kmers, size, seed):
    """`size` of the k-mers, ascending."""
    assert kmers.size >= size
    rng = np.random.default_rng([0x7E, seed])
    return np.sort(rng.permutation(kmers)[:size])


def crowd_group(k, gbits, grp, count, rng, avoid=None):
    """`count` canonical k-mers whose record lands in group grp: rc(x) carries grp in the gbits below its top base
    (bases k-1-gbits/2 .. k-2 of x hold grp's reverse complement)."""
    low = 2 * k - 2 - gbits
    out = np.zeros(0, dtype=U)
    for _ in range(64):
        rx = rng.integers(0, 4 ** k, size=4 * count + 64, dtype=np.uint64)
        rx = (rx & ~(U((1 << gbits) - 1) << U(low))) | (U(grp) << U(low))
        x = synth.revcomp(rx, k)
        x = x[x < rx]
        out = np.unique(np.concatenate([out, x]))
        if avoid is not None:
            out = out[~np.isin(out, avoid)]
        if out.size >= count:
            return rng.permutation(out)[:count]
    raise AssertionError("no room in group %d" % grp)


def crowd_prefix(k, bits, prefix, count, rng, avoid=None, lo=None, hi=None):
    """`count` canonical k-mers that start with the `bits` bits of prefix (their rest in [lo, hi) where given)."""
    rest = 2 * k - bits
    lo = 0 if lo is None else lo
    hi = (1 << rest) if hi is None else hi
    out = np.zeros(0, dtype=U)
    for _ in range(64):
        x = (U(prefix) << U(rest)) | rng.integers(lo, hi, size=4 * count + 64, dtype=np.uint64)
        x = x[x < synth.revcomp(x, k)]
        out = np.unique(np.concatenate([out, x]))
        if avoid is not None:
            out = out[~np.isin(out, avoid)]
        if out.size >= count or hi - lo <= out.size:
            break
    if out.size < count:
        raise AssertionError("no room under the prefix")
    return rng.permutation(out)[:count]


def union(*parts):
    return np.unique(np.concatenate([np.asarray(p, dtype=U) for p in parts]))


def grow_to(base, extras, measure, target):
    """base plus the first j of extras, j the smallest at which measure(set) reaches target(set) -- measure must
    not fall as k-mers are added; both are read from the model of the set, and the hit must be exact."""
    def at(j):
        s = union(base, extras[:j])
        return s, measure(s) - target(s)

    lo, hi = 0, len(extras)
    s, d = at(hi)
    assert d >= 0, "not enough engineered k-mers: %d short" % -d
    while lo < hi:
        mid = (lo + hi) // 2
        if at(mid)[1] >= 0:
            hi = mid
        else:
            lo = mid + 1
    s, d = at(lo)
    assert d == 0, "the edge is stepped over: %d" % d
    return s, lo


def place_at(kmers, x, index, k, rng):
    """The set with k-mers dropped or lone random k-mers added below x until x has that index."""
    kmers = np.asarray(kmers, dtype=U)
    at = int(np.searchsorted(kmers, U(x)))
    if at > index:
        below = rng.permutation(at)[:at - index]
        kmers = np.delete(kmers, below)
    elif at < index:
        add = crowd_prefix(k, 0, 0, index - at, rng, avoid=kmers, lo=0, hi=int(x))
        kmers = union(kmers, add)
    assert int(np.searchsorted(kmers, U(x))) == index
    return kmers


def with_branches(kmers, k, count, seed):
    """The set plus all eight candidates (canonical) of `count` of its k-mers: junctions with direct neighbours and
    neighbours through a reverse complement on both sides."""
    rng = np.random.default_rng([0xB2, k, seed])
    pick = kmers[rng.permutation(kmers.size)[:count]]
    mask = U((1 << (2 * k)) - 1)
    cands = []
    for c in range(4):
        cands.append(((pick << U(2)) & mask) | U(c))
        cands.append((pick >> U(2)) | (U(c) << U(2 * (k - 1))))
    extra = np.concatenate(cands)
    keep = rng.random(extra.size) < 0.45
    return union(kmers, finish(extra[keep], k))


def _probe(kmers, k, nbits, kb, env="default"):
    return Probe(kmers, k, nbits, kb, ENVS[env])


def _first(make, seeds=range(24)):
    last = None
    for seed in seeds:
        try:
            return make(seed)
        except AssertionError as e:
            last = e
    raise AssertionError("no seed builds this case: %s" % last)


# ---- A ---------------------------------------------------------------------------------------------------------------------
def _group_counts_case(name, k, nbits, kb, base_size, targets, expect, forbid=(), also=("marks", "batched"), seed=1):
    """A base genome and crowds that bring chosen groups to record counts given as functions of the plan."""
    def make(seed):
        rng = np.random.default_rng([0xA1, k, nbits, seed])
        kmers = genome(k, base_size, seed)
        groups = rng.permutation(1 << nbits)[:len(targets)].tolist()
        for grp, want in zip(groups, targets):
            extras = crowd_group(k, nbits, grp, 12000 if nbits <= 2 else 1400, rng, avoid=kmers)
            kmers, _ = grow_to(kmers, extras, lambda s: int(records_per_group(s, k, nbits)[grp]),
                               lambda s: want(plan(k, nbits, kb, s.size)))
        pl = plan(k, nbits, kb, kmers.size)
        rec = records_per_group(kmers, k, nbits)
        assert [int(rec[g]) for g in groups] == [w(pl) for w in targets], "a later crowd moved the plan"
        return Case(name, k, nbits, kb, kmers, expect, forbid, also=also)

    return _first(make, range(seed, seed + 24))


def a_cases_build():
    out = []
    # groups without records, without a pass-0 range, without any of the sixteen ranges
    def sparse(seed):
        kmers = genome(11, 600, seed)
        c = Case("a-sparse-groups", 11, 8, 2, kmers,
                 {"g:no_records_but_ranges", "g:records_empty_pass0", "g:records_sixteen_empty", "rc1:packed2", "rc1:sbits8",
                  "rc1:T64:kb2"}, {"route:rc_marks_groups"}, also=("marks", "batched"))
        assert c.expect <= c.branches()
        return c
    out.append(_first(sparse))
    # the split between the kernels: rc1_cap records, and one more, on the same base
    at_cap = _group_counts_case("a-group-at-rc1-cap", 15, 8, 4, 6000, [lambda p: p.rc1_cap],
                                {"split:at_rc1_cap", "route:no_rc_marks_groups", "rc1:packed4", "rc1:rest>sbits"},
                                {"route:rc_marks_groups", "split:rc1_cap+1"})
    out.append(at_cap)
    rng = np.random.default_rng(0xA2)
    m = at_cap.model()
    grp = int(np.argmax(m.groups()[0]))
    one = crowd_group(15, 8, grp, 1, rng, avoid=at_cap.kmers)
    out.append(Case("a-group-rc1-cap+1", 15, 8, 4, union(at_cap.kmers, one),
                    {"split:rc1_cap+1", "route:rc_marks_groups", "rc:T64:kb4"}, {"route:no_rc_marks_groups"},
                    also=("marks", "batched")))
    # the four-records-per-thread request loop
    out.append(_group_counts_case("a-records-4T-64", 15, 8, 4, 6000,
                                  [lambda p: 4 * p.threads - 1, lambda p: 4 * p.threads, lambda p: 4 * p.threads + 1],
                                  {"rc1:records_4T-1", "rc1:records_4T", "rc1:records_4T+1", "rc1:T64:kb4"},
                                  {"route:rc_marks_groups"}, seed=3))
    out.append(_group_counts_case("a-records-4T-256", 15, 2, 4, 1200,
                                  [lambda p: 4 * p.threads - 1, lambda p: 4 * p.threads, lambda p: 4 * p.threads + 1],
                                  {"rc1:records_4T-1", "rc1:records_4T", "rc1:records_4T+1", "rc1:T256:kb4"},
                                  {"route:rc_marks_groups"}, seed=5))
    # rest_bits: 0 (2K = N + 4), below and above sbits
    # (2K = N + 4 passes the staged condition -- 2K - N >= N + 2 + (N & 1) -- at N = 2 only: (5, 6) and (9, 14) take
    # the in-place probe, which tests/test_gpu_geometry.py has)
    for k, nbits, size, name in ((3, 2, 28, "rc1:rest0"), (5, 2, 300, "rc1:rest<sbits"), (7, 6, 1500, "rc1:rest<sbits")):
        kmers = dense(k, size, 7)
        out.append(Case("a-rest-bits-k%d-n%d" % (k, nbits), k, nbits, 2, kmers, {name, "rc1:packed2"},
                        {"route:rc_marks_groups"}, also=("marks", "batched")))
    # keys wider than the minimum
    out.append(Case("a-wide-keys-15-14-4", 15, 14, 4, with_branches(genome(15, 5000, 11), 15, 300, 1),
                    {"rc1:packed4_wide", "rc1:rest>sbits", "rc1:sbits8"}, {"route:rc_marks_groups"}, also=("marks", "batched")))
    # sbits 11 (the thread variants below bring 9, 10 and 12, the N = 8 sets 8)
    out.append(Case("a-sbits11", 15, 2, 4, with_branches(genome(15, 6200, 13), 15, 300, 2), {"rc1:sbits11", "rc1:T512:kb4"},
                    also=("marks",)))
    # every thread variant at every key width, at the smallest sets that select it (N = 2)
    for kb, k in ((2, 9), (4, 15), (8, 23)):
        for threads, size in ((64, 1024), (256, 1028), (512, 4100), (1024, 16388)):
            big = dense(k, size + 600, 17) if k == 9 else with_branches(genome(k, size + 300, 17 + kb), k, 200, 3)
            kmers = trimmed(big, size, kb)
            expect = {"rc1:T%d:kb%d" % (threads, kb), "rc1:rkey_rt_nxt" if kb == 8 else "rc1:packed%d" % kb,
                      "rc1:sbits%d" % {64: 9, 256: 9, 512: 10, 1024: 12}[threads]}
            if k == 9 and size >= 4100:
                expect |= {"rc1:several_top_base", "rc1:several_last_base"}
            out.append(Case("a-threads%d-kb%d" % (threads, kb), k, 2, kb, kmers, expect,
                            also=("marks",) + (("batched",) if threads <= 256 else ())))
    return out


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _without_group_ranges(kmers, k, gbits, grp):
    """The k-mers that lie in none of the sixteen ranges [c][tb][grp]."""
    g1 = (kmers >> U(2 * k - 4 - gbits)) & U((1 << gbits) - 1)
    return kmers[g1 != U(grp)]


def b_cases_build():
    out = []
    k, nbits, kb = 15, 8, 4
    rng = np.random.default_rng(0xB1)
    base = with_branches(genome(k, 5000, 21), k, 200, 4)

    def cap_of(s):
        return plan(k, nbits, kb, s.size, ENVS["marks"]).cap

    # pass 0: a bucket of exactly cap keys, one more, and more than twice as many
    bucket = 0b00011011  # A C G T
    extras = crowd_prefix(k, nbits, bucket, 2400, rng, avoid=base)

    def in_bucket(s):
        return int(np.count_nonzero((s >> U(2 * k - nbits)) == U(bucket)))

    at_cap, j = grow_to(base, extras, in_bucket, cap_of)
    out.append(Case("b-pass0-at-cap", k, nbits, kb, at_cap, {"rc:p0_at_cap", "rc:p0_fits", "route:no_rc_batched", "rc:T64:kb4"},
                    {"route:rc_batched", "rc:p0_batched", "rc:p1_batched"}, env="marks", also=("batched",)))
    out.append(Case("b-pass0-cap+1", k, nbits, kb, union(at_cap, extras[j:j + 1]),
                    {"rc:p0_cap+1", "rc:p0_two_batches", "rc:p0_batched", "route:rc_batched"}, {"route:no_rc_batched"},
                    env="marks"))
    out.append(Case("b-pass0-three-batches", k, nbits, kb, union(base, extras[:2300]),
                    {"rc:p0_gt_2cap", "rc:p0_three_batches", "route:rc_batched"}, env="marks"))
    # pass 1: sixteen ranges that hold cap keys together, and one more
    grp = 0b01101100  # C G T A
    pool = []
    for seg in range(16):
        try:
            pool.append(crowd_prefix(k, 4 + nbits, (seg << nbits) | grp, 140, rng, avoid=base))
        except AssertionError:
            pass
    extras = rng.permutation(np.concatenate(pool))

    def in_ranges(s):
        return int(np.count_nonzero(((s >> U(2 * k - 4 - nbits)) & U(255)) == U(grp)))

    at_cap, j = grow_to(base, extras, in_ranges, cap_of)
    out.append(Case("b-pass1-at-cap", k, nbits, kb, at_cap, {"rc:p1_at_cap", "rc:p1_fits", "route:no_rc_batched"},
                    {"route:rc_batched", "rc:p1_batched"}, env="marks", also=("batched",)))
    out.append(Case("b-pass1-cap+1", k, nbits, kb, union(at_cap, extras[j:j + 1]), {"rc:p1_cap+1", "rc:p1_batched", "route:rc_batched"},
                    {"route:no_rc_batched"}, env="marks"))
    # pass 1 with chosen range lengths: the group's ranges hold engineered k-mers only
    clean = _without_group_ranges(base, k, nbits, grp)

    def ranges_case(name, lens, expect, forbid=()):
        """lens: {range: its length as a function of cap}."""
        def make(seed):
            r2 = np.random.default_rng([0xB3, seed])
            s = clean
            for _ in range(4):  # (cap does not move at these sizes; the loop is there for the model to say so)
                cap = cap_of(s)
                parts = [crowd_prefix(k, 4 + nbits, (seg << nbits) | grp, f(cap), r2) for seg, f in lens.items()]
                s = union(clean, *parts)
                if cap_of(s) == cap:
                    break
            got = _probe(s, k, nbits, kb, "marks").groups()[2][grp]
            assert {seg: int(got[seg]) for seg in lens} == {seg: f(cap_of(s)) for seg, f in lens.items()}
            assert int(got.sum()) == sum(f(cap_of(s)) for f in lens.values())
            return Case(name, k, nbits, kb, s, expect, forbid, env="marks")
        return _first(make)

    out.append(ranges_case("b-pass1-batch-ends-at-range-end", {0: lambda c: 600, 1: lambda c: c - 600, 2: lambda c: 100},
                           {"rc:p1_batch_ends_at_range_end", "rc:p1_batched", "route:rc_batched"}))
    out.append(ranges_case("b-pass1-range-split", {5: lambda c: 2 * c + 300},
                           {"rc:p1_range_split", "rc:p1_batched", "route:rc_batched"}))
    out.append(ranges_case("b-pass1-one-full", {6: lambda c: c}, {"rc:p1_one_full_fifteen_empty", "rc:p1_fits"}))
    # slice_lg clamped to 0 at the smallest keys, clamped and unclamped elsewhere
    out.append(Case("b-slices-3-2", 3, 2, 2, dense(3, 30, 3), {"rc:slice_lg_clamped_to_0", "rc:T64:kb2"}, env="marks"))
    out.append(Case("b-slices-4-2", 4, 2, 2, dense(4, 110, 3), {"rc:slice_lg_clamped_to_0", "rc:slice_lg_clamped"}, env="marks"))
    out.append(Case("b-slices-7-6", 7, 6, 2, dense(7, 6000, 5), {"rc:slice_lg_unclamped", "rc:slice_lg_clamped"}, env="marks"))
    # 2-byte keys, every parity of cap that & ~7 allows, with windows filled to the last key
    for size, parity in ((4 * 621, 8), (4 * 628, 0), (31200, 8)):
        kmers = trimmed(dense(9, size + 500, 9), size, size)
        p = plan(9, 2, 2, size, ENVS["marks"])
        assert p.cap % 8 == 0 and p.cap % 16 == parity
        out.append(Case("b-u16-cap%d" % p.cap, 9, 2, 2, kmers,
                        {"rc:kb2_cap%%16=%d" % parity, "rc:kb2_full_window_cap%%16=%d" % parity, "route:rc_batched"},
                        env="marks"))
    # the default route: one group over rc1_cap whose bucket is over cap as well
    def mixed(seed):
        r2 = np.random.default_rng([0xB4, seed])
        s = union(base, crowd_group(k, nbits, bucket, 400, r2, avoid=base), crowd_prefix(k, nbits, bucket, 1150, r2, avoid=base))
        return Case("b-mixed-default", k, nbits, kb, s, {"route:rc_marks_groups", "route:rc_batched", "rc:p0_batched", "rc1:packed4"},
                    also=("batched",))
    out.append(_first(mixed))
    return out


# ---- C ---------------------------------------------------------------------------------------------------------------------
def c_cases_build():
    out = []
    rng = np.random.default_rng(0xC1)
    # one level
    out.append(Case("c-all-in-one-group", 15, 8, 4, union(crowd_group(15, 8, 0b10010011, 3000, rng)),
                    {"part:one_level", "part:one_group_has_all", "route:rc_marks_groups", "part:records8"},
                    also=("marks", "batched")))
    out.append(Case("c-every-group", 11, 6, 2, genome(11, 3000, 31), {"part:one_level", "part:every_group_has_records"}))
    big = with_branches(genome(15, 33500, 33), 15, 500, 5)
    for size, name in ((3071, "part:n=1024j-1"), (3073, "part:n=1024j+1"), (16384, "part:n=16384"), (16385, "part:n=16385"),
                       (32769, "part:n=32769")):
        out.append(Case("c-n%d" % size, 15, 8, 4, trimmed(big, size, size), {name, "part:one_level"}))
    # two levels (KSH_RC_GROUPS=half), and the one-pass form at the same sizes (+ KSH_RC_SCATTER=direct)
    half = dict(env="half", also=("half+direct",))
    out.append(Case("c-half-17-14", 17, 14, 4, with_branches(genome(17, 5000, 35), 17, 200, 6),
                    {"part:two_level", "part:extra1", "part:two_level_N=14", "l1:offsets_not_staged", "l2:tile_three_super_groups",
                     "part:records8"}, **half))
    out.append(Case("c-half-15-14", 15, 14, 2, with_branches(genome(15, 5000, 37), 15, 200, 7),
                    {"part:two_level", "part:extra0", "part:two_level_N=14", "l2:tile_three_super_groups"}, **half))
    out.append(Case("c-half-15-8", 15, 8, 4, with_branches(genome(15, 9000, 39), 15, 200, 8),
                    {"part:two_level", "part:extra0", "part:two_level_N<14", "l1:offsets_staged"}, **half))
    out.append(Case("c-half-25-14-u64", 25, 14, 8, with_branches(genome(25, 5000, 41), 25, 200, 9),
                    {"part:two_level", "part:extra1", "part:records16", "l2:tile_three_super_groups"}, **half))
    out.append(Case("c-half-23-8-u64", 23, 8, 8, with_branches(genome(23, 5000, 43), 23, 200, 10),
                    {"part:two_level", "part:records16", "part:two_level_N<14"}, **half))
    # all records in one super-group; in two neighbouring ones (a level-2 tile at their seam)
    for k, nbits, kb in ((17, 14, 4), (25, 14, 8)):
        gbits = plan(k, nbits, kb, 6000, ENVS["half"]).gbits
        lo_bits = gbits - cfg().sg_bits
        one = union(*[crowd_group(k, gbits, (37 << lo_bits) | int(g), 60, rng) for g in rng.permutation(1 << lo_bits)[:90]])
        two = union(trimmed(one, 3000, 1), *[crowd_group(k, gbits, (38 << lo_bits) | int(g), 60, rng)
                                             for g in rng.permutation(1 << lo_bits)[:50]])
        out.append(Case("c-half-one-super-group-%d" % kb, k, nbits, kb, one,
                        {"part:two_level", "l1:tile_one_super_group", "l2:tile_one_super_group"},
                        {"l2:tile_three_super_groups", "l2:tile_at_a_seam"}, **half))
        out.append(Case("c-half-two-super-groups-%d" % kb, k, nbits, kb, two, {"part:two_level", "l2:tile_at_a_seam"},
                        {"l2:tile_three_super_groups"}, **half))
    # a row inside one bucket
    out.append(Case("c-half-one-bucket", 15, 8, 4, union(crowd_prefix(15, 8, 0b00100111, 4300, rng)),
                    {"part:two_level", "l1:row_in_one_bucket", "l1:offsets_staged"}, **half))
    return out


# ---- D ---------------------------------------------------------------------------------------------------------------------
def _prefix_run(kmers, k, length, rng, lo_frac, hi_frac, has_pred=False):
    """A (K-1)-base prefix with exactly `length` canonical k-mers, none of them in the set yet and no k-mer of the set
    with that prefix, between the k-mers at the given fractions of the set."""
    n = kmers.size
    lo, hi = int(kmers[int(n * lo_frac)]) >> 2, int(kmers[int(n * hi_frac)]) >> 2
    have = set((kmers >> U(2)).tolist())
    for _ in range(2000):
        p = int(rng.integers(lo + 1, hi))
        if p in have:
            continue
        run = finish(np.array([(p << 2) | c for c in range(4)], dtype=U), k)
        run = run[(run >> U(2)) == U(p)]
        if run.size >= length:
            return run[:length]
    raise AssertionError("no prefix with %d canonical k-mers" % length)


def _cut_case(name, k, nbits, kb, size, runs, expect, seed0=1):
    """runs: [(cut index c, run length)]: a prefix run of that many k-mers starting at index c * chunk - 1."""
    def make(seed):
        rng = np.random.default_rng([0xD1, seed])
        kmers = genome(k, size, 50 + seed)
        chunk = plan(k, nbits, kb, kmers.size).chunk
        placed = []
        for c, length in runs:
            frac = (c * chunk) / kmers.size
            run = _prefix_run(kmers, k, length, rng, frac * 0.98, min(frac * 1.02, 0.999))
            kmers = union(kmers, run)
            # (k-mers are dropped or added between the run before this one and this one only)
            floor = int(np.searchsorted(kmers, placed[-1])) + 1 if placed else 0
            at = int(np.searchsorted(kmers, run[0]))
            want = c * chunk - 1
            if at > want:
                drop = floor + rng.permutation(at - floor)[:at - want]
                kmers = np.delete(kmers, drop)
            elif at < want:
                lo_v = int(kmers[floor]) if floor else 0
                kmers = union(kmers, crowd_prefix(k, 0, 0, want - at, rng, avoid=kmers, lo=lo_v + 1, hi=int(run[0])))
            assert int(np.searchsorted(kmers, run[0])) == want
            placed.append(run[-1])
        case = Case(name, k, nbits, kb, kmers, expect, also=("staged", "probe"))
        m = case.model()
        assert case.expect <= m.branches()
        # the k-mer in front of every run has a direct predecessor (a mark that a misplaced cut would lose)
        for c, _ in runs:
            assert m.verdicts()["nd"][0][c * chunk - 2] >= 1
        return case

    return _first(make, range(seed0, seed0 + 40))


def _stream_case(k, nbits, kb, size, seed):
    """A base whose window 0 streams exactly kStreamMax k-mers (engineered: k-mers G s A' with the suffix s in window
    0's prefix range sit far above the window and lengthen its stream only), and the k-mers to add for more."""
    rng = np.random.default_rng([0xD2, seed])
    base = with_branches(genome(k, size, 60 + seed), k, 150, 11)
    p = plan(k, nbits, kb, base.size)
    v1 = cuts_of(base, k, p.chunk)[1][1]
    assert int(np.searchsorted(base, U(2 << (2 * k - 2)))) > 2 * p.chunk  # the G k-mers lie beyond the first cuts
    extras = crowd_prefix(k, 2, 2, 9000, rng, avoid=base, lo=0, hi=v1)

    def stream0(s):
        return int(_probe(s, k, nbits, kb).windows()["stream"][0])

    at_max, j = grow_to(base, extras, stream0, lambda s: plan(k, nbits, kb, s.size).stream_max)
    return base, at_max, extras, j


def d_cases_build():
    out = []
    fwd = dict(also=("staged", "probe"))
    k, nbits, kb = 15, 8, 4
    # the cut offset: a prefix run of 1, 2, 3 and 4 k-mers that starts at index 2047
    for length in (1, 2, 3, 4):
        out.append(_cut_case("d-first%d" % length, k, nbits, kb, 5000, [(1, length)], {"fwd:first%d" % length}, seed0=length))
    out.append(_cut_case("d-window-chunk+3", k, nbits, kb, 11000, [(1, 1), (2, 4)], {"fwd:first1", "fwd:first4", "fwd:window_chunk+3"}))
    # set sizes around the window
    big = with_branches(genome(k, 4500, 71), k, 150, 12)
    for size, name in ((2048, "fwd:n=chunk"), (2049, "fwd:n=chunk+1"), (4096, "fwd:n=2chunk"), (4097, "fwd:n=2chunk+1"),
                       (1500, "fwd:one_window")):
        out.append(Case("d-n%d" % size, k, nbits, kb, trimmed(big, size, size), {name}, **fwd))

    # a prefix run across the last nominal cut that reaches the end of the set: the last window is empty
    def to_end(seed):
        rng = np.random.default_rng([0xD3, seed])
        s = genome(k, 7000, 73 + seed)
        run = _prefix_run(s, k, 4, rng, 0.31, 0.40)
        s = union(s[s < run[0]], run)
        s = place_at(s, int(run[0]), 2046, k, rng)
        c = Case("d-run-reaches-end", k, nbits, kb, s, {"fwd:run_reaches_end", "fwd:empty_window_and_stream"}, **fwd)
        assert c.expect <= c.branches() and s.size == 2050
        return c
    out.append(_first(to_end))
    # buckets: a window inside one bucket; windows over more than kTgtSpan buckets; targets in slot 15 and beyond
    out.append(Case("d-window-in-one-bucket", k, 2, kb, with_branches(genome(k, 9000, 75), k, 200, 13),
                    {"fwd:window_in_one_bucket", "fwd:stream_buckets_in_table"}, **fwd))
    out.append(Case("d-windows-over-span", k, 14, 2, with_branches(genome(k, 5000, 77), k, 200, 14),
                    {"fwd:window_over_span", "fwd:target_in_slot16+", "fwd:stream_bucket_searched"}, **fwd))
    out.append(Case("d-slots-15-16", k, nbits, kb, with_branches(genome(k, 20000, 79), k, 400, 15),
                    {"fwd:window_over_span", "fwd:target_in_slot15", "fwd:target_in_slot16+", "fwd:target_in_table"}, **fwd))
    # streams: exactly kStreamMax and one more on the same base; three parts and more
    base, at_max, extras, j = _stream_case(k, nbits, kb, 12000, 1)
    out.append(Case("d-stream-at-max", k, nbits, kb, at_max, {"fwd:stream_at_max", "route:no_tgt_parts"}, {"route:tgt_parts"}, **fwd))
    out.append(Case("d-stream-max+1", k, nbits, kb, union(at_max, extras[j:j + 1]), {"fwd:stream_max+1", "fwd:m2", "route:tgt_parts"}, {"route:no_tgt_parts"}, **fwd))
    out.append(Case("d-stream-three-parts", k, nbits, kb, union(at_max, extras[j:j + 4200]), {"fwd:m3+"}, **fwd))

    # the engineered stream packed into a gap of window 0's prefixes: parts with an empty window
    def empty_part(seed):
        rng = np.random.default_rng([0xD4, seed])
        p = plan(k, nbits, kb, base.size)
        pref = (base[:p.chunk] >> U(2)).astype(np.int64)
        g = int(np.argmax(np.diff(pref)))
        lo, hi = int(pref[g]) + 1, int(pref[g + 1])
        s = union(base, crowd_prefix(k, 2, 2, 9000, rng, avoid=base, lo=lo, hi=hi))
        c = Case("d-part-with-empty-window", k, nbits, kb, s, {"fwd:part_empty_window", "fwd:m3+"}, **fwd)
        assert c.expect <= c.branches()
        return c
    out.append(_first(empty_part))

    # two longest stream ranges of the same length; a stream that one top base holds alone
    def tie(seed):
        rng = np.random.default_rng([0xD5, seed])
        s = union(at_max, extras[j:j + 2500])
        v1 = cuts_of(s, k, plan(k, nbits, kb, s.size).chunk)[1][1]
        more = crowd_prefix(k, 2, 1, 9000, rng, avoid=s, lo=0, hi=v1)
        assert int(np.searchsorted(s, U(1 << (2 * k - 2)))) > 2200  # the C k-mers lie beyond the first cut

        def c_range(t):
            return int(_probe(t, k, nbits, kb).windows()["lens"][0][1])

        s, _ = grow_to(s, more, c_range, lambda t: int(_probe(t, k, nbits, kb).windows()["lens"][0][2]))
        c = Case("d-tie-of-longest", k, nbits, kb, s, {"fwd:tie_of_longest_ranges", "fwd:m3+"}, **fwd)
        assert c.expect <= c.branches()
        return c
    out.append(_first(tie))

    def one_top(seed):
        s = union(at_max, extras[j:j + 3000])
        for _ in range(12):
            w = _probe(s, k, nbits, kb).windows()
            v1 = w["v"][1]
            suffix = (s & U((1 << (2 * k - 2)) - 1)).astype(np.int64)
            top = (s >> U(2 * k - 2)).astype(np.int64)
            drop = (suffix < v1) & (top != 2)
            if not drop.any():
                break
            s = s[~drop]
        c = Case("d-one-top-base", k, nbits, kb, s, {"fwd:one_top_base_streams_all"}, **fwd)
        assert c.expect <= c.branches()
        return c
    out.append(_first(one_top, range(1)))

    # a window with k-mers and nobody to stream: every k-mer's second base is A, the last window starts with C
    def no_stream(seed):
        rng = np.random.default_rng([0xD6, seed])
        low = crowd_prefix(k, 4, 0, plan(k, nbits, kb, 2054).chunk, rng)  # A A ...: window 0, to its last key
        high = np.concatenate([crowd_prefix(k, 4, 0b0100, 3, rng), crowd_prefix(k, 4, 0b1000, 3, rng)])  # C A ..., G A ...
        s = union(low, high)
        c = Case("d-window-without-stream", k, nbits, kb, s, {"fwd:empty_stream"}, **fwd)
        assert c.expect <= c.branches()
        return c
    out.append(_first(no_stream))
    # every class of direct x through-rc neighbours on both sides, marks over every rc0, at 2-, 4- and 8-byte keys
    combos = set(D_BRANCHES[-14:])
    out.append(Case("d-verdicts-dense-9", 9, 8, 2, dense(9, 30000, 81), combos, **fwd))
    out.append(Case("d-verdicts-dense-11", 11, 2, 4, dense(11, 40000, 83), {x for x in combos if not x.endswith(("d2r2", "d2r1"))}, **fwd))
    out.append(Case("d-verdicts-23", 23, 8, 8, with_branches(genome(23, 6000, 85), 23, 1500, 16),
                    {"s0:d1r0", "s0:d0r1", "s0:d1r1", "s1:d1r0", "s1:d0r1", "s1:d1r1"}, **fwd))
    # the k-mers a probe must not count: poly-A, a (K-1)-base prefix or suffix that is its own reverse complement
    def selfies(k, nbits, kb, size):
        s = genome(k, size, 87) if k >= 9 else dense(k, size, 87)
        if k % 2:
            rng = np.random.default_rng([0xD7, k])
            h = (k - 1) // 2
            w = rng.integers(0, 4 ** h, size=40, dtype=np.uint64)
            pal = (w << U(2 * h)) | synth.revcomp(w, h)          # (K-1)-mers that are their own reverse complement
            mask = U((1 << (2 * k)) - 1)
            cand = [((pal << U(2)) | U(c)) & mask for c in range(4)] + [(U(c) << U(2 * k - 2)) | pal for c in range(4)]
            cand = np.concatenate(cand)
            # and their neighbours, so that the miscount would change a verdict
            more = [((cand << U(2)) & mask) | U(c) for c in range(4)] + [(cand >> U(2)) | (U(c) << U(2 * k - 2)) for c in range(4)]
            keep = rng.random(8 * cand.size) < 0.3
            s = union(s, finish(cand, k), finish(np.concatenate(more)[keep], k))
        s = union(s, finish(np.array([0, 1, 1 << (2 * k - 2)], dtype=U), k))  # A..A, A..AC, CA..A
        return s
    for k, nbits, kb, size in ((3, 2, 2, 24), (15, 8, 4, 4000), (23, 8, 8, 4000), (9, 8, 2, 4000)):
        expect = {"self:next_is_itself"} | ({"self:prefix_is_its_own_rc", "self:suffix_is_its_own_rc"} if k % 2 else set())
        out.append(Case("d-self-hits-k%d" % k, k, nbits, kb, selfies(k, nbits, kb, size), expect, also=("staged", "probe", "marks")))
    return out


FAMILIES = {"a": a_cases_build, "b": b_cases_build, "c": c_cases_build, "d": d_cases_build}


@functools.lru_cache(maxsize=None)
def family(name):
    cases = FAMILIES[name]()
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def all_cases():
    return [c for f in FAMILIES for c in family(f)]


def cases_under(env):
    """The cases that run under the switch set env."""
    return [c for c in all_cases() if env in c.envs()]

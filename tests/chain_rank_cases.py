"""Cases for the middle of the SPSS encode (csrc/ksh_encode.hip): the chain ranking (k_rank_walk, k_rank_heads,
k_ruler_jump, k_l2_walk / _jump / _resolve, k_choose_ends, k_rulers_done), the strings written from the logs of the
ranking walks (emit_logged, emit_ruler_walker, emit_head_walker) and the stamped second pass after a loop, with a
numpy / Python model of the branches a k-mer set takes there.

A *case* is a k-mer set built so that its rulers stand where the kernels take another branch.  The rulers are the
k-mers whose index in the ascending set is a multiple of kRulerEvery, so a case starts from base sequences whose
k-mers form the wanted chains and gets lone filler k-mers -- k-mers without a de Bruijn neighbour in the set -- put
just below a chosen k-mer until its index has the wanted residue (place).  Every (K-1)-mer, in canonical form, occurs
once in a case (Builder), apart from the junctions a case asks for: two k-mers are neighbours only where a sequence
says so, at every K.

The model (Profile) restates the kernels' arithmetic: per walker the steps to its arrival, what it arrives at, the
states it logs, who walks under KSH_RANK_PHASES=2 (first_phase), the level-2 rulers of every chain, the log-fit
rule, and (log_emit) the writing of the strings from the logs.  It says which branches a case takes, so that the GPU
test (tests/test_gpu_chain_rank.py) can assert what it is testing and the CPU test
(tests/test_chain_rank_model_cpu.py) that every branch is reached.  It is never the expected answer: that is the
oracle's strings.  The constants and the restated lines are read from ksh_encode.hip, so a changed constant fails
the CPU test instead of moving the cases off the edges silently."""
import os
import re
from collections import namedtuple

import numpy as np

from kmersets import synth

U = np.uint64
NONE = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENCODE_HIP = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc", "ksh_encode.hip")

Cfg = namedtuple("Cfg", "ruler_shift l2_shift jump_hops mid_rulers mid_heads match_first match_batch l2_floor "
                        "l2_default hash_mul hash_shift")

# the lines of ksh_encode.hip that the model restates
LINES = (
    "constexpr uint32_t kRulerEvery = 1u << kRulerShift;",
    "__device__ __forceinline__ bool sampled_ruler(uint32_t s) { return (s & (2u * kRulerEvery - 2u)) == 0; }",
    "__device__ __forceinline__ uint32_t dense_index(uint32_t s) { return ((s >> (kRulerShift + 1)) << 1) | (s & 1); }",
    "__device__ __forceinline__ bool is_long(uint32_t steps) const { return steps > uint32_t(n_mid + 1) * uint32_t(k); }",
    "if (is_long(steps)) long_walkers[atomicAdd(long_count, 1u)] = uint32_t(w) | long_tag;",
    "if (hdr && j < n_mid) mid[int64_t(j) * n_walkers + w] = state;",
    "if (++since == log.k) {",
    "if (enter_link(own, r) == kNone) log.arrived(i, 0, r);  // a k-mer on its own: no walk arrives at it",
    "if (kPhase == 1 && !first_phase(r)) return;",
    "if (kPhase == 1 && !first_phase(s0)) return;",
    "if (rec_look(rinfo + i) != kRecUnset) return;",
    "if (rec_look(chain_info + t) != kRecUnset) return;",
    "if (log.is_long(steps)) return;  // on the list (WalkLog::arrived)",
    "const int n_passed = int((steps - 1) / uint32_t(k));",
    "if (!sampled_ruler(arrival)) emit(arrival, steps, set.kmer(arrival >> 1));",
    "if (++since == k || step == steps) {",
    "const uint32_t q_u = flip ? (c.len - 1 - c.p) : c.p;",
    "const bool with_string = (u & 1) == (c.d ^ flip);  // the walk ran in string order",
    "const uint32_t q = with_string ? q_u + step : q_u - step;",
    "const uint32_t as_read = with_string ? state : state ^ 1;",
    "if (kLongPass || (i & 1) || log.hdr[i ^ 1] != kRecUnset) return;",
    "const uint32_t u = (own.y == kNone && own.x != kNone) ? 2 * t + 1 : 2 * t;",
    "c.d = (directed || fwd_start >= fwd_end) ? 0u : 1u;",
    "c.cls = (directed || fwd_start == fwd_end) ? uint8_t(0) : uint8_t((c.head_state & 1) == 0 ? 1 : 2);",
    "__device__ __forceinline__ bool is_level2(int64_t i) { return ((i >> 1) & ((1 << kL2Shift) - 1)) == 0; }",
    "if (!kLevel2 && (is_level2(i) || !(rinfo[i ^ 1] & kEndFlag))) return;  // level 2, or something comes before it: that walker passes it",
    "if (is_level2(cur) || steps > n_dense) {",
    "if (st == kRecUnset) return;  // a loop of rulers without a level-2 ruler: stays without an end",
    "const int64_t n_dense = 2 * ((n + kRulerEvery - 1) / kRulerEvery);",
    "const size_t used = (size_t(n_dense) + size_t(n)) * 8;",
    "const size_t log_bytes = size_t(n_dense) * (8 + 4 * kLogMidRulers + 4) + size_t(n_ends) * (8 + 4 * kLogMidHeads + 4) + 64;  // + the long list",
    "if (!emit_by_walking() && used + log_bytes <= size_t(2 * n) * 8) {",
    "const bool two_levels = !stamped && n_dense >= l2_threshold();",
    "const int64_t n_jump = two_levels ? (((n_dense - 1) >> (kL2Shift + 1)) << 1) + 2 : n_dense;",
    "int max_rounds = 3;  // a record's reach grows five-fold per launch (four hops): log5 of the records, and spare",
    "for (int64_t x = n_jump; x > 1; x /= (kJumpHops + 1)) max_rounds++;",
    "for (int hop = 0; hop < kJumpHops && !(mine & kEndFlag); hop++) {",
    "if (!first_pass) {  // the stamping pass after a loop was found: its flags and sums start over",
    "if (accounted == n && *reinterpret_cast<int*>(ctx->h_pinned + 2 + kLenSums) == 0) break;",
    "if (!p->stamped && (lc[0] || lc[1])) p->routes |= KSH_ROUTE_LONG_STRETCHES;",
    "if (p->rounds > kMatchFirst) p->routes |= KSH_ROUTE_MATCH_MORE_ROUNDS;",
    "const int batch = p->rounds ? kMatchBatch : kMatchFirst;",
    "p->rounds += more ? batch : ran + 1;  // (the round that found nothing counts, as before)",
    "store_run<(kRun ? kRun : 4)>(at, o, k, 0);",
    "if (k > kRun) store_run<(kRun ? kRun : 4)>(at, o, k, k - kRun);",
    "if (g->k >= 16)",
    "else if (g->k >= 8)",
    "else if (g->k >= 4)",
)


def constants(text=None):
    """Cfg from ksh_encode.hip; the lines the model restates must stand there as written."""
    if text is None:
        text = open(ENCODE_HIP).read()

    def nums(pattern):
        m = re.search(pattern, text)
        if m is None:
            raise AssertionError("ksh_encode.hip no longer has what the model reads: " + pattern)
        return [int(g, 0) for g in m.groups()]

    mid = nums(r"constexpr int kLogMidRulers = (\d+), kLogMidHeads = (\d+);")
    fp = nums(r"return \(\(\(s >> 1\) \* (0x[0-9A-Fa-f]+)u\) >> (\d+) \^ s\) & 1u;")
    l2 = nums(r"return e \? std::max<int64_t>\((\d+), atoll\(e\)\) : int64_t\(1\) << (\d+);")
    cfg = Cfg(nums(r"#define KSH_RULER_SHIFT (\d+)")[0], nums(r"#define KSH_L2_SHIFT (\d+)")[0],
              nums(r"#define KSH_JUMP_HOPS (\d+)")[0], mid[0], mid[1],
              nums(r"constexpr int kMatchFirst = (\d+);")[0], nums(r"constexpr int kMatchBatch = (\d+);")[0],
              l2[0], 1 << l2[1], fp[0], fp[1])
    for line in LINES:
        if line not in text:
            raise AssertionError("ksh_encode.hip no longer has the line the model restates: " + line)
    return cfg


_CFG = []


def cfg():
    if not _CFG:
        _CFG.append(constants())
    return _CFG[0]


def every(c=None):
    return 1 << (c or cfg()).ruler_shift


def l2_every(c=None):
    c = c or cfg()
    return 1 << (c.ruler_shift + c.l2_shift)


def first_phase(s, c=None):
    c = c or cfg()
    return ((((s >> 1) * c.hash_mul) & 0xFFFFFFFF) >> c.hash_shift ^ s) & 1


def emit_run(k):
    """The run width KSH_EMIT picks for K."""
    return 16 if k >= 16 else (8 if k >= 8 else (4 if k >= 4 else 0))


def n_dense_of(n, c=None):
    e = every(c)
    return 2 * ((n + e - 1) // e)


def logs_fit(n, n_ends, c=None):
    """The log-fit rule of encode_plan_t."""
    c = c or cfg()
    nd = n_dense_of(n, c)
    used = (nd + n) * 8
    log_bytes = nd * (8 + 4 * c.mid_rulers + 4) + n_ends * (8 + 4 * c.mid_heads + 4) + 64
    return used + log_bytes <= 2 * n * 8


def max_ends_that_fit(n, c=None):
    e = 0
    while logs_fit(n, e + 1, c):
        e += 1
    assert logs_fit(n, e, c)
    return e


def jump_rounds(n_jump, c=None):
    c = c or cfg()
    r, x = 3, n_jump
    while x > 1:
        r += 1
        x //= c.jump_hops + 1
    return r


def rounds_needed(records, c=None):
    """Launches of k_ruler_jump / k_l2_jump after which a chain of `records` records has ended, if every launch
    read the records as the launch before left them (launches that read fresher records need no more)."""
    c = c or cfg()
    reach, r = 1, 0  # a record points `reach` records ahead; the last record of the chain holds the end already
    while reach < records - 1:
        reach *= c.jump_hops + 1
        r += 1
    return r


# ---- links ------------------------------------------------------------------------------------------------------------
class Links:
    """succ[s] of every state s = 2 t + d (NONE: the leaving side has no link), and which sides have a link."""

    def __init__(self, kmers, k, canonical=True):
        km = np.ascontiguousarray(kmers, dtype=U)
        n = km.size
        mask = U((1 << (2 * k)) - 1)
        nb = np.full((2, n, 4), NONE, dtype=np.int64)
        same = np.zeros((2, n, 4), dtype=bool)
        for side in (0, 1):  # 0: left, 1: right
            for c in range(4):
                y = (((km << U(2)) & mask) | U(c)) if side else ((km >> U(2)) | (U(c) << U(2 * (k - 1))))
                z = synth.canonical(y, k) if canonical else y
                pos = np.minimum(np.searchsorted(km, z), n - 1)
                hit = (km[pos] == z) & (z != km)
                nb[side, :, c] = np.where(hit, pos, NONE)
                same[side, :, c] = hit & (z != y)
        cnt = (nb >= 0).sum(axis=2)
        first = np.argmax(nb >= 0, axis=2)[..., None]
        sn = np.take_along_axis(nb, first, 2)[..., 0]
        ss = np.take_along_axis(same, first, 2)[..., 0]
        link = np.full((2, n), NONE, dtype=np.int64)
        lsame = np.zeros((2, n), dtype=bool)
        for side in (0, 1):
            facing = np.where(ss[side], side, 1 - side)
            ok = (cnt[side] == 1) & (cnt[facing, np.maximum(sn[side], 0)] == 1)
            link[side] = np.where(ok, sn[side], NONE)
            lsame[side] = ok & ss[side]
        succ = np.full(2 * n, NONE, dtype=np.int64)
        succ[0::2] = np.where(link[1] >= 0, 2 * link[1] + lsame[1], NONE)        # d = 0 leaves through the right side
        succ[1::2] = np.where(link[0] >= 0, 2 * link[0] + (1 - lsame[0]), NONE)  # d = 1 through the left side
        self.n, self.k, self.cnt, self.link, self.succ = n, k, cnt, link, succ
        self.has_pred = np.zeros(2 * n, dtype=bool)
        self.has_pred[0::2] = link[0] >= 0
        self.has_pred[1::2] = link[1] >= 0
        self.ends = np.flatnonzero((link[0] < 0) | (link[1] < 0))  # the end k-mers, ascending (k_end_fill)


# ---- the model ----------------------------------------------------------------------------------------------------------
Walker = namedtuple("Walker", "ruler w u steps arrival kind mid")
# kind: r2r, r2e, h2r, h2e (start -> arrival), lone_sampled, lone_unsampled


def boundary_lengths(k, c=None):
    c = c or cfg()
    top = (c.mid_rulers + 1) * k
    return {"K-1": k - 1, "K": k, "K+1": k + 1, "top-1": top - 1, "top": top, "top+1": top + 1}


def length_names(k, c=None):
    return dict(boundary_lengths(k, c), **{"1": 1, "2K": 2 * k})


KINDS = ("r2r", "r2e", "h2r", "h2e")
LENGTH_NAMES = ("1", "K-1", "K", "K+1", "2K", "top-1", "top", "top+1", "several")
STRETCH_BRANCHES = tuple("%s@%s" % (kind, ln) for kind in KINDS for ln in LENGTH_NAMES)
DIRECTION_BRANCHES = tuple("%s@%s" % (w, ln) for w in ("with", "against") for ln in ("K-1", "K", "K+1", "top-1", "top", "top+1"))
WHO_BRANCHES = ("lone_sampled", "lone_unsampled", "ruler_is_end", "self_only", "ph2:r2r", "ph2:r2e", "ph2:h2r", "ph2:h2e",
                "ph2:race")
L2_BRANCHES = ("l2:none_on_chain", "l2:single_first", "l2:single_last", "l2:single_middle", "l2:gap_gt",
               "l2:first_is_l2", "l2:pow-1", "l2:pow", "l2:pow+1")
JUMP_BRANCHES = ("jump:pow-1", "jump:pow", "jump:pow+1")
LOOP_BRANCHES = ("loop:large", "loop:rulers_with_l2", "loop:rulers_no_l2", "loop:one_sampled", "loop:unsampled",
                 "loop:with_long_and_logs")
ROUTE_BRANCHES = ("route:emit_logs", "route:no_logs", "route:long", "route:no_long", "route:stamped")
WIDTH_BRANCHES = ("run16", "run8", "run4", "run0", "log_emit@run16", "log_emit@run8", "log_emit@run4", "log_emit@run0", "string_K", "string_K+1", "canonical", "directed")
MATCH_BRANCHES = ("rounds>first", "rounds>first+batch")
UNREACHABLE_BRANCHES = {
    "rounds>first+batch": "a side's edges all run through one junction, which has at most four sides a side: every "
                          "live round matches a pair of it, so no set takes more than kMatchFirst + 1 rounds",
    "log_emit@run0": "no set of 3-mers or 2-mers has logs that fit (small_k_unreachable)",
}
BRANCHES = (STRETCH_BRANCHES + DIRECTION_BRANCHES + WHO_BRANCHES + L2_BRANCHES + JUMP_BRANCHES + LOOP_BRANCHES +
            ROUTE_BRANCHES + WIDTH_BRANCHES + MATCH_BRANCHES)


class Profile:
    """What the ranking walks and the log emit do on one set."""

    def __init__(self, kmers, k, canonical=True, c=None):
        self.c = c or cfg()
        self.k, self.canonical = k, canonical
        self.km = np.ascontiguousarray(kmers, dtype=U)
        self.n = self.km.size
        self.links = Links(self.km, k, canonical)
        self.succ = self.links.succ.tolist()
        self.has_pred = self.links.has_pred.tolist()
        self.ends = self.links.ends.tolist()
        self.n_ends = len(self.ends)
        self.n_dense = n_dense_of(self.n, self.c)
        self._walk()
        self._unitigs()

    def sampled(self, s):
        return (s >> 1) % every(self.c) == 0

    def dense(self, s):
        return (((s >> 1) // every(self.c)) << 1) | (s & 1)

    def level2(self, i):
        return ((i >> 1) & ((1 << self.c.l2_shift) - 1)) == 0

    # -- k_rank_walk / k_rank_heads, all walkers ------------------------------------------------------------------
    def _one_walk(self, u, n_mid):
        succ, k = self.succ, self.k
        cur, steps, since, mid = u, 0, 0, []
        while True:
            cur = succ[cur]
            steps += 1
            if self.sampled(cur):
                return steps, cur, mid, True
            since += 1
            if since == k:
                since = 0
                if len(mid) < n_mid:
                    mid.append(cur)
            if succ[cur] == NONE:
                return steps, cur, mid, False

    def _walk(self):
        succ, has_pred = self.succ, self.has_pred
        self.walkers = []      # every walker that may log
        self.ruler_is_end = 0  # sampled states that end their chain at once and are not on their own
        ev = every(self.c)
        for t in range(0, self.n, ev):
            for d in (0, 1):
                r = 2 * t + d
                i = self.dense(r)
                if succ[r] == NONE:
                    if not has_pred[r]:
                        self.walkers.append(Walker(True, i, r, 0, r, "lone_sampled", []))
                    else:
                        self.ruler_is_end += 1
                    continue
                steps, arrival, mid, at_ruler = self._one_walk(r, self.c.mid_rulers)
                self.walkers.append(Walker(True, i, r, steps, arrival, "r2r" if at_ruler else "r2e", mid))
        for e, t in enumerate(self.ends):
            if t % ev == 0:
                continue
            x, y = self.links.link[0][t], self.links.link[1][t]
            if x == NONE and y != NONE:
                s0 = 2 * t
            elif y == NONE and x != NONE:
                s0 = 2 * t + 1
            else:
                self.walkers.append(Walker(False, e, 2 * t, 0, 2 * t, "lone_unsampled", []))
                continue
            steps, arrival, mid, at_ruler = self._one_walk(s0, self.c.mid_heads)
            self.walkers.append(Walker(False, e, s0, steps, arrival, "h2r" if at_ruler else "h2e", mid))
        self.by_start = {w.u: w for w in self.walkers}

    def mirror(self, w):
        """The walker of the mirror image of w's stretch (None for a k-mer on its own or a loop's one ruler)."""
        if w.steps == 0:
            return None
        return self.by_start.get(w.arrival ^ 1)

    def who_walks(self):
        """Under KSH_RANK_PHASES=2: {start state: "walks" | "rests" | "race"} for every walker of a stretch."""
        out = {}
        for w in self.walkers:
            if w.steps == 0:
                out[w.u] = "walks"
                continue
            m = self.mirror(w)
            if m is None or m.u == w.u:
                out[w.u] = "walks"
                continue
            a, b = first_phase(w.u, self.c), first_phase(m.u, self.c)
            out[w.u] = "race" if a == b else ("walks" if a else "rests")
        return out

    # -- the unitigs (k_choose_ends' choice, k_loops) ---------------------------------------------------------------
    def _unitigs(self):
        succ, has_pred, n = self.succ, self.has_pred, self.n
        covered = [False] * n
        found = []  # (class, head k-mer, states in string order)
        for s0 in range(2 * n):
            if has_pred[s0] or (not self.canonical and (s0 & 1)):
                continue
            chain, s = [], s0
            while s != NONE:
                chain.append(s)
                s = succ[s]
            a, b = chain[0] >> 1, chain[-1] >> 1
            if self.canonical and (a < b or (a == b and (s0 & 1))):
                continue  # the mirror image spells it
            assert a != b or len(chain) == 1, "a chain passes a k-mer once"
            cls = 0 if (not self.canonical or a == b) else (1 if (s0 & 1) == 0 else 2)
            found.append((cls, a, chain))
            for s in chain:
                assert not covered[s >> 1]
                covered[s >> 1] = True
        self.loops = []
        for t in range(n):
            if covered[t]:
                continue
            chain, s = [], 2 * t
            while True:
                chain.append(s)
                covered[s >> 1] = True
                s = succ[s]
                assert s != NONE
                if s == 2 * t:
                    break
                assert not covered[s >> 1], "a loop passes a k-mer once"
            found.append((3, t, chain))
            self.loops.append(chain)
        found.sort(key=lambda f: (f[0], f[1]))
        self.unitig_states = [f[2] for f in found]
        self.unitig_class = [f[0] for f in found]
        self.place = {}  # k-mer -> (unitig, position, spelled reverse-complemented)
        for u, chain in enumerate(self.unitig_states):
            for p, s in enumerate(chain):
                self.place[s >> 1] = (u, p, s & 1)

    def oriented(self, s):
        x = int(self.km[s >> 1])
        if s & 1:
            x = int(synth.revcomp(np.array([x], dtype=U), self.k)[0])
        return x

    def kmer_bases(self, s):
        x = self.oriented(s)
        return bytes((x >> (2 * (self.k - 1 - i))) & 3 for i in range(self.k))

    def unitig_strings(self):
        out = []
        for chain in self.unitig_states:
            b = bytearray(self.kmer_bases(chain[0]))
            for s in chain[1:]:
                b.append(self.oriented(s) & 3)
            out.append(bytes(b).translate(bytes.maketrans(b"\x00\x01\x02\x03", b"ACGT")).decode())
        return out

    # -- the strings from the logs (emit_logged, emit_ruler_walker, emit_head_walker) ---------------------------------
    def log_emit(self, policy="all", flip=False, variant=None):
        """The unitigs as the log emit writes them: one bytearray per unitig (0xFF: a slot nothing wrote), or an
        AssertionError where the kernel would read a log entry that no walk wrote.  policy: which walkers walked
        ("all": both mirror images of every stretch; "first" / "second": the walkers KSH_RANK_PHASES=2 lets walk,
        a race won by the mirror image with the smaller / larger start state).  flip: every unitig is placed the
        way the path cover places a flipped one.  variant: None, or one of the deliberately wrong models
        "steps_over_k", "long_ge", "no_arrival" (the CPU test's sensitivity checks)."""
        assert not self.loops, "a set with a loop takes the stamped pass: no log emit"
        k, c = self.k, self.c
        who = self.who_walks()
        walked = {}
        for w in self.walkers:
            verdict = "walks" if policy == "all" else who[w.u]
            if verdict == "race":
                m = self.mirror(w)
                verdict = "walks" if (w.u < m.u) == (policy == "first") else "rests"
            if verdict == "walks":
                walked[(w.ruler, w.w)] = w
        bufs = [bytearray(b"\xff" * (len(ch) + k - 1)) for ch in self.unitig_states]
        lens = [len(ch) for ch in self.unitig_states]

        def is_long(steps, n_mid, where):
            if variant == "long_ge" and where == "emit":
                return steps >= (n_mid + 1) * k
            return steps > (n_mid + 1) * k

        def store(u, q, state):
            assert 0 <= q < lens[u], "a slot outside the unitig"
            new = self.kmer_bases(state)
            old = bufs[u][q:q + k]
            assert all(o == 0xFF or o == b for o, b in zip(old, new)), "two writes disagree"
            bufs[u][q:q + k] = new

        for (is_ruler, _), w in sorted(walked.items()):
            n_mid = c.mid_rulers if is_ruler else c.mid_heads
            u, p, d = self.place[w.u >> 1]
            q_u = lens[u] - 1 - p if flip else p
            with_string = (w.u & 1) == (d ^ int(flip))

            def emit(state, step):
                store(u, q_u + step if with_string else q_u - step, state if with_string else state ^ 1)

            if is_long(w.steps, n_mid, "arrived"):  # from the list: walked once more
                emit(w.u, 0)
                cur, step, since = w.u, 0, 0
                while step < w.steps:
                    cur = self.succ[cur]
                    step += 1
                    since += 1
                    if since == k or step == w.steps:
                        since = 0
                        emit(cur, step)
                continue
            if is_long(w.steps, n_mid, "emit"):
                continue
            emit(w.u, 0)
            if w.steps == 0:
                continue
            n_passed = (w.steps // k) if variant == "steps_over_k" else (w.steps - 1) // k
            for j in range(n_passed):
                assert j < len(w.mid), "a log entry that no walk wrote"
                emit(w.mid[j], (j + 1) * k)
            if not self.sampled(w.arrival) and variant != "no_arrival":
                emit(w.arrival, w.steps)
        # a sampled k-mer neither of whose states walked writes itself
        ev = every(c)
        self.self_only = []
        for t in range(0, self.n, ev):
            i = 2 * (t // ev)
            if (True, i) in walked or (True, i + 1) in walked:
                continue
            u, p, d = self.place[t]
            self.self_only.append(t)
            store(u, lens[u] - 1 - p if flip else p, 2 * t + (d ^ int(flip)))
        return bufs

    def log_emit_strings(self, policy="all", flip=False, variant=None):
        bufs = self.log_emit(policy, flip, variant)
        assert all(0xFF not in b for b in bufs), "a slot nothing wrote"
        return [bytes(b).translate(bytes.maketrans(b"\x00\x01\x02\x03", b"ACGT")).decode() for b in bufs]

    # -- the ruler records of every chain, for the pointer jumping -------------------------------------------------
    def ruler_chains(self):
        """Per chain with ends, in both directions: the dense indices of its sampled states in walking order; and
        the same per loop, from an arbitrary start."""
        chains, loops = [], []
        for cls, states in zip(self.unitig_class, self.unitig_states):
            fwd = [self.dense(s) for s in states if self.sampled(s)]
            back = [self.dense(s ^ 1) for s in reversed(states) if self.sampled(s)]
            if cls == 3:
                loops.append(fwd)
                if self.canonical:
                    loops.append(back)
            else:
                chains.append(fwd)
                if self.canonical:
                    chains.append(back)
        if not self.canonical:  # the d = 1 states walk the same chains backwards
            chains += [[i ^ 1 for i in reversed(ch)] for ch in chains]
            loops += [[i ^ 1 for i in reversed(ch)] for ch in loops]
        return chains, loops

    # -- branches ----------------------------------------------------------------------------------------------------
    def branches(self, rounds=None):
        c, k = self.c, self.k
        out = {"canonical" if self.canonical else "directed", "run%d" % emit_run(k)}
        names = length_names(k, c)
        top = (c.mid_rulers + 1) * k
        who = self.who_walks()
        for w in self.walkers:
            if w.steps == 0:
                out.add(w.kind)
                continue
            for name, v in names.items():
                if w.steps == v:
                    out.add("%s@%s" % (w.kind, name))
            if w.steps >= 2 * top:
                out.add("%s@several" % w.kind)
            if who[w.u] == "race":
                out.add("ph2:race")
            elif who[w.u] == "walks" and not self.loops:
                out.add("ph2:" + w.kind)
                u, p, d = self.place[w.u >> 1]
                for name, v in boundary_lengths(k, c).items():
                    if w.steps == v:
                        out.add("%s@%s" % ("with" if (w.u & 1) == d else "against", name))
        if self.ruler_is_end:
            out.add("ruler_is_end")
        if not self.loops:
            ev = every(c)
            for t in range(0, self.n, ev):
                if all(who.get(2 * t + d, "rests") == "rests" for d in (0, 1)):
                    out.add("self_only")
        lens = [len(ch) for ch in self.unitig_states]
        if 1 in lens:
            out.add("string_K")
        if 2 in lens:
            out.add("string_K+1")
        # routes
        any_long = any(w.steps > ((c.mid_rulers if w.ruler else c.mid_heads) + 1) * k for w in self.walkers)
        fit = logs_fit(self.n, self.n_ends, c)
        if self.loops:
            out.add("route:stamped")
        else:
            out.add("route:emit_logs" if fit else "route:no_logs")
            if fit:
                out.add("log_emit@run%d" % emit_run(k))
            out.add("route:long" if (fit and any_long) else "route:no_long")
        # the ruler records
        chains, loops = self.ruler_chains()
        hops = c.jump_hops + 1
        span = 1 << c.l2_shift
        for ch in chains:
            l2 = [self.level2(i) for i in ch]
            if ch and not any(l2):
                out.add("l2:none_on_chain")
            if ch and l2[0]:
                out.add("l2:first_is_l2")
            if len(ch) >= 3 and sum(l2) == 1:
                out.add("l2:single_first" if l2[0] else ("l2:single_last" if l2[-1] else "l2:single_middle"))
            at = [j for j, v in enumerate(l2) if v]
            if any(b - a - 1 > span for a, b in zip(at, at[1:])):
                out.add("l2:gap_gt")
            for label, count in (("l2", len(at)), ("jump", len(ch))):
                r = 1
                while hops ** (r + 1) <= count + 1:
                    r += 1
                if r >= 3 and abs(count - hops ** r) <= 1:
                    out.add("%s:pow%s" % (label, ("-1", "", "+1")[count - hops ** r + 1]))
        for lp in self.loops:
            rulers = [self.dense(s) for s in lp if self.sampled(s)]
            if len(lp) >= 2000:
                out.add("loop:large")
                if fit and any_long:
                    out.add("loop:with_long_and_logs")
            if len(rulers) == 0:
                out.add("loop:unsampled")
            elif len(rulers) == 1:
                out.add("loop:one_sampled")
            if len(rulers) >= 2:
                out.add("loop:rulers_with_l2" if any(self.level2(i) for i in rulers) else "loop:rulers_no_l2")
        if rounds is not None and rounds > c.match_first:
            out.add("rounds>first")
        if rounds is not None and rounds > c.match_first + c.match_batch:
            out.add("rounds>first+batch")
        return out


def flipped_unitigs(unitigs, spss, k):
    """Which of the unitigs (strings) the path cover's strings hold reverse-complemented."""
    seen = set()
    for x in spss:
        for i in range(len(x) - k + 1):
            seen.add(x[i:i + k])
    rc = str.maketrans("ACGT", "TGCA")
    out = []
    for u in unitigs:
        fwd = u[:k] in seen
        assert fwd or u[:k][::-1].translate(rc) in seen
        out.append(not fwd)
    return out


# ---- building a set --------------------------------------------------------------------------------------------------------
class PlacementError(Exception):
    pass


def _rc_int(x, m):
    out = 0
    for _ in range(m):
        out = (out << 2) | (3 - (x & 3))
        x >>= 2
    return out


_PERMS = [p for p in __import__("itertools").permutations(range(4))]


class Builder:
    """Sequences and lone k-mers over one pool of (K-1)-mers: every (K-1)-mer, in canonical form, is used once (a
    junction that a case asks for apart), none is its own reverse complement, and no k-mer is."""

    def __init__(self, k, canonical, seed):
        self.k, self.canonical = k, canonical
        self.rng = np.random.default_rng([0xC4A1, k, int(canonical), seed])
        self.used = set()
        self.km_mask = (1 << (2 * (k - 1))) - 1
        self.parts = []     # arrays of k-mers in sequence order, as read
        self.status = {}    # k-mer of the set -> (kind, wanted first_phase of the state that runs with its sequence)

    def _sub(self, x):
        """Canonical (K-1)-mer, or None for one that is its own reverse complement."""
        r = _rc_int(x, self.k - 1)
        return None if r == x else min(x, r)

    def grow(self, n_kmers, prefix=None, circular=False):
        """The k-mers (as read) of a fresh sequence of n_kmers k-mers; prefix: the K-1 bases it starts with (a
        junction); circular: the sequence closes on itself (n_kmers k-mers on a loop)."""
        k, rng = self.k, self.rng
        top1, top = 2 * (k - 2), 2 * (k - 1)
        for _ in range(200):
            got, fresh = [], set()
            if prefix is None:
                cur = int(rng.integers(0, 1 << (2 * (k - 1))))
                sub = self._sub(cur)
                if sub is None or sub in self.used:
                    continue
                fresh.add(sub)
            else:
                cur = prefix
            first, rc = cur, _rc_int(cur, k - 1)
            ok = True
            draws = rng.integers(0, 24, size=n_kmers).tolist()
            for step in range(n_kmers - (k - 1) if circular else n_kmers):
                for b in _PERMS[draws[step]]:
                    x = (cur << 2) | b
                    if x == (((3 - b) << top) | rc):
                        continue  # the k-mer is its own reverse complement
                    nxt, nrc = x & self.km_mask, (rc >> 2) | ((3 - b) << top1)
                    sub = min(nxt, nrc)
                    if nxt == nrc or sub in self.used or sub in fresh:
                        continue
                    fresh.add(sub)
                    got.append(x)
                    cur, rc = nxt, nrc
                    break
                else:
                    ok = False
                    break
            if ok and circular:  # close the circle with the first K-1 bases
                for j in range(k - 1):
                    b = (first >> (2 * (k - 2 - j))) & 3
                    x = (cur << 2) | b
                    nxt, nrc = x & self.km_mask, (rc >> 2) | ((3 - b) << top1)
                    sub = min(nxt, nrc)
                    last = j == k - 2
                    if x == (((3 - b) << top) | rc) or (not last and (nxt == nrc or sub in self.used or sub in fresh)):
                        ok = False
                        break
                    if not last:
                        fresh.add(sub)
                    got.append(x)
                    cur, rc = nxt, nrc
            if not ok:
                continue
            self.used |= fresh
            seq = np.array(got, dtype=U)
            self.parts.append(seq)
            return seq
        raise PlacementError("no room for a sequence of %d k-mers" % n_kmers)

    def in_set(self, x):
        """The form in which k-mer x (as read, an int) is in the set, and whether its d = 0 state runs with it."""
        if not self.canonical:
            return x, True
        r = _rc_int(x, self.k)
        return (x, True) if x < r else (r, False)

    def want(self, seq, pos, kind, rightward=None):
        """k-mer `pos` of seq is to be `kind`; rightward (0 / 1): first_phase of its state that runs with seq."""
        v, fwd = self.in_set(int(seq[pos]))
        phase = None if rightward is None else (rightward if fwd else 1 - rightward)
        self.status[v] = (kind, phase)

    def suffix(self, seq):
        return int(seq[-1]) & self.km_mask

    def _lone(self, lo, hi, count, partial=False):
        """`count` lone k-mers with values in (lo, hi); partial: as many of them as there are."""
        k, rng, out = self.k, self.rng, []
        if hi - lo - 1 < count and not partial:
            raise PlacementError("no room below a k-mer")
        if hi - lo - 1 < 1 or count < 1:
            return out
        for attempt in range(40):
            m = 8 * (count - len(out)) + 32
            if hi - lo - 1 <= 4 * m:
                cand = rng.permutation(np.arange(lo + 1, hi, dtype=np.uint64))
            else:
                cand = rng.integers(lo + 1, hi, size=m, dtype=np.uint64)
            if self.canonical:
                cand = cand[cand < synth.revcomp(cand, k)]
            else:
                cand = cand[cand != synth.revcomp(cand, k)]
            for x in cand.tolist():
                a, b = self._sub(x >> 2), self._sub(x & self.km_mask)
                if a is None or b is None or a == b or a in self.used or b in self.used:
                    continue
                self.used.add(a)
                self.used.add(b)
                out.append(x)
                if len(out) == count:
                    return out
            if hi - lo - 1 <= 4 * m:
                break
        if partial:
            return out
        raise PlacementError("no lone k-mers left below a k-mer")

    def place(self, default="none", pad_to=0):
        """The set: the parts' k-mers plus the lone k-mers that give every k-mer its wanted kind.  Kinds: "none"
        (not sampled), "ruler" (sampled, not level 2), "l2", "free" (anything but level 2), "any".  pad_to: lone
        k-mers above the largest until the set holds that many.
        Working upwards, a k-mer gets its lone k-mers just below it; where that gap has too few, the gaps below
        it take the rest, down to the last k-mer that is a ruler or has a wanted phase, and only as many as leave
        the unsampled and "free" k-mers they shift what they are."""
        c = cfg()
        ev, ev2 = every(c), l2_every(c)
        seqs = np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=U)
        base = np.unique(synth.canonical(seqs, self.k) if self.canonical else seqs)
        assert base.size == seqs.size, "the sequences share a k-mer"
        ok = {"none": lambda t: t % ev != 0, "ruler": lambda t: t % ev == 0 and t % ev2 != 0,
              "l2": lambda t: t % ev2 == 0, "free": lambda t: t % ev2 != 0, "any": lambda t: True}
        lone, shift = [], 0
        soft = []  # [value, index, kind] of the "none" / "free" k-mers since the last hard one
        floor = -1  # value of the last hard k-mer
        for j, x in enumerate(base.tolist()):
            kind, phase = self.status.get(x, (default, None))
            if kind == "any" and phase is None:
                continue
            t = j + shift
            placed = False
            add = 0
            for _ in range(6):
                while not (ok[kind](t + add) and (phase is None or first_phase(2 * (t + add), c) == phase)):
                    add += 1
                    if add > 64 * ev2:
                        raise PlacementError("no index for a k-mer")
                if add == 0:
                    placed = True
                    break
                got = self._fill(floor, soft, x, add, ok)
                if got is not None:
                    lone += got
                    shift += add
                    placed = True
                    break
                add += 1
            if not placed:
                raise PlacementError("no lone k-mers left below a k-mer")
            if kind in ("ruler", "l2") or phase is not None:
                soft, floor = [], x
            else:
                soft.append([x, t + add, kind])
        n = base.size + len(lone)
        if pad_to > n:  # above the last k-mer that is a ruler or has a wanted phase
            got = self._fill(floor, soft, 1 << (2 * self.k), pad_to - n, ok)
            if got is None:
                raise PlacementError("no lone k-mers left at the top")
            lone += got
        out = np.unique(np.concatenate([base, np.array(lone, dtype=U)]))
        assert out.size == base.size + len(lone)
        self.lone = np.array(sorted(lone), dtype=U)
        return out

    def _fill(self, floor, soft, x, add, ok):
        """`add` lone k-mers below x: from the gap just below it downwards; None where they do not fit."""
        marks = [floor] + [s[0] for s in soft] + [x]
        got, rest = [], add
        plan = []
        for g in range(len(marks) - 2, -1, -1):  # gap g lies below soft[g] (or below x, the topmost)
            take = self._lone(marks[g], marks[g + 1], rest, partial=True)
            plan.append((g, take))
            rest -= len(take)
            if g >= 1 and not ok[soft[g - 1][2]](soft[g - 1][1] + rest):
                # soft[g - 1] lies below this gap: it is shifted by `rest`; one k-mer less here moves it on
                if not take:
                    rest = -1
                    break
                self._unuse(take.pop())
                rest += 1
                if not ok[soft[g - 1][2]](soft[g - 1][1] + rest):
                    rest = -1
                    break
            if rest == 0:
                break
        if rest != 0:
            for _, take in plan:
                for v in take:
                    self._unuse(v)
            return None
        below = add
        for g, take in plan:  # from the top gap down: soft[g - 1] is shifted by what lies below it
            below -= len(take)
            if g >= 1:
                soft[g - 1][1] += below
            got += take
        return got

    def _unuse(self, x):
        self.used.discard(self._sub(x >> 2))
        self.used.discard(self._sub(x & self.km_mask))


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """name, K, canonical, the set (ascending uint64), the lone k-mers among it, the branches the model must
    (expect) and must not (forbid) report, the environment it needs ("l2": KSH_L2_MIN at its floor) and the
    matching rounds the model counts (None: not asked)."""

    def __init__(self, name, k, canonical, kmers, lone, expect, forbid=(), env=(), want_rounds=False):
        self.name, self.k, self.canonical, self.kmers, self.lone = name, k, canonical, kmers, lone
        self.expect, self.forbid, self.env, self.want_rounds = frozenset(expect), frozenset(forbid), tuple(env), want_rounds
        self._profile = None
        self.rounds = None

    def geom(self):
        """(N, key bytes) of the geometry the case is encoded at."""
        n = min(14, 2 * self.k - 1) if self.k >= 4 else 2 * self.k - 2
        kb = 2 * self.k - n
        return n, (2 if kb <= 16 else 4 if kb <= 32 else 8)

    def profile(self):
        if self._profile is None:
            self._profile = Profile(self.kmers, self.k, self.canonical)
        return self._profile

    def model_rounds(self):
        if self.rounds is None:
            from model_encode import EncodeModel

            m = EncodeModel(self.kmers, self.k)
            m.build_links()
            m.build_unitigs()
            m.build_edges()
            m.greedy_rounds()
            self.rounds = m.rounds
        return self.rounds

    def branches(self):
        return self.profile().branches(self.model_rounds() if self.want_rounds else None)

    def routes(self, l2=False):
        """(route names the encode must report, names it must not) in a process with or without KSH_L2_MIN at its
        floor."""
        b = self.branches()
        c = cfg()
        must, never = set(), set()
        (must if "route:stamped" in b else never).add("rank_stamped")
        (must if "route:emit_logs" in b else never).add("emit_logs")
        (must if "route:long" in b else never).add("long_stretches")
        two = "route:stamped" not in b and self.profile().n_dense >= (c.l2_floor if l2 else c.l2_default)
        (must if two else never).add("jump_two_level")
        if self.want_rounds:
            (must if "rounds>first" in b else never).add("match_more_rounds")
        return must, never


def _try_seeds(make, seeds=range(16)):
    """The first seed at which `make` places its set (deterministic: the rng of a Builder is seeded by the seed)."""
    for seed in seeds:
        try:
            return make(seed)
        except PlacementError:
            continue
    raise PlacementError("no seed places this case")


def _chain(b, stops, rightward=None):
    """A sequence whose k-mers at `stops` ((kind, position), the first and the last k-mer among them) are of that
    kind and all others unsampled; rightward: per stop, first_phase of its state that runs with the sequence --
    under KSH_RANK_PHASES=2 a stretch between two stops is walked with the sequence where both are 1, against it
    where both are 0, and by either or both mirror images where they differ."""
    seq = b.grow(stops[-1][1] + 1)
    for j in range(seq.size):
        b.want(seq, j, "none")
    for j, (kind, pos) in enumerate(stops):
        b.want(seq, pos, kind, None if rightward is None else rightward[j])
    return seq


def _an_arm_is_flipped(kmers, k, arm_kmers):
    from model_encode import EncodeModel

    m = EncodeModel(kmers, k)
    spss = m.spss()
    unitigs = [m.unitig_string(u) for u in range(m.n_unitigs)]
    flipped = flipped_unitigs(unitigs, spss, k)
    return any(f and len(u) == arm_kmers + k - 1 for f, u in zip(flipped, unitigs))


STRETCH_GROUPS = ("short", "K-1", "K", "K+1", "top-1", "top", "top+1", "several")


def group_lengths(k, group):
    c = cfg()
    top = (c.mid_rulers + 1) * k
    if group == "short":
        return {"1": 1, "2K": 2 * k}
    if group == "several":
        return {"several": 2 * top + 3}
    return {group: boundary_lengths(k)[group]}


def stretch_case(k, canonical, group):
    """Items 1, 2, 3 and 7, one case per length g (1 and 2K together): chains with ruler-to-ruler, ruler-to-end,
    head-to-ruler and head-to-end stretches of g steps; at the boundary lengths their walkers under
    KSH_RANK_PHASES=2 are fixed so that each kind runs with the string and against it, a sampled chain end is left
    to itself, and (canonical sets) two arms at a junction hold the length for the path cover to flip.  Chains of
    at most (n_mid + 1) K + 1 k-mers with rulers wherever they fall bring the set to the size at which its logs
    fit."""
    c = cfg()
    top = (c.mid_rulers + 1) * k
    lengths = group_lengths(k, group)
    phased = group in boundary_lengths(k)
    if any(g < 1 for g in lengths.values()):
        return None

    def make(seed, bulk_for=None):
        b = Builder(k, canonical, seed)
        rulers = 0
        if bulk_for is None:
            _, first = make(seed, -1)
            bulk_for = Links(first, k, canonical).ends.size
            return make(seed, bulk_for)
        if bulk_for < 0:
            bulk_for = None
        for g in lengths.values():
            o = (lambda *bits: bits) if phased else (lambda *bits: None)
            # h -g- R -g- R -g- R -g- R -g- e: two stretches with the sequence, a race, two against it
            _chain(b, [("none", 0)] + [("ruler", j * g) for j in range(1, 5)] + [("none", 5 * g)], o(1, 1, 1, 0, 0, 0))
            rulers += 4
            if group == "several":
                _chain(b, [("none", 0), ("none", g)])
                _chain(b, [("ruler", 0), ("none", g)])
                continue
            # h -g- R - R -g- e: the rulers walk to the chain ends
            _chain(b, [("none", 0), ("ruler", g), ("ruler", g + 1), ("none", 2 * g + 1)], o(0, 0, 1, 1))
            # chains without a ruler, walked from either end
            _chain(b, [("none", 0), ("none", g)], o(1, 1))
            _chain(b, [("none", 0), ("none", g)], o(0, 0))
            # a sampled chain end, walked towards from the other end: left to itself
            _chain(b, [("ruler", 0), ("none", g)], o(0, 0))
            rulers += 3
            if canonical and phased:
                # junctions whose arms are chains of g steps without a ruler: the path cover joins an arm to its trunk
                # and flips one of them; the seed is kept only if an arm is flipped (the cover of these unitigs alone
                # orders and matches them as the cover of the whole set does: ids keep their order, edges stay)
                mark = len(b.parts)
                for _ in range(4 if g <= 128 else 2):
                    trunk = b.grow(3)
                    for _ in range(2):
                        arm = b.grow(g + 1, prefix=b.suffix(trunk))
                        for j in range(g + 1):
                            b.want(arm, j, "none")
                if not _an_arm_is_flipped(np.unique(synth.canonical(np.concatenate(b.parts[mark:]), k)), k, g + 1):
                    raise PlacementError("the cover flips no arm")
        base = sum(p.size for p in b.parts)
        piece = min(top + 1, 400)
        if bulk_for is None:  # a first placement without the bulk, to count the end k-mers
            kmers = b.place("any")
            return b, kmers
        ends = int(bulk_for * (1.04 + 0.04 * seed)) + 8
        bulk = max(0, int((8 * ends + 64 - base - ends) / (1 - 16.0 / piece)))
        for _ in range((bulk + piece - 1) // piece):
            b.grow(piece)
        kmers = b.place("any")
        if not logs_fit(kmers.size, Links(kmers, k, canonical).ends.size):
            raise PlacementError("the logs do not fit")
        return b, kmers

    b, kmers = _try_seeds(make)
    names = list(lengths)
    expect = {"canonical" if canonical else "directed", "run%d" % emit_run(k), "route:emit_logs", "lone_sampled",
              "lone_unsampled", "string_K"}
    expect |= {"%s@%s" % (kind, n) for kind in KINDS for n in names} | {"ruler_is_end"}
    forbid = {"route:stamped", "route:no_logs"}
    if phased:
        expect |= {"ph2:" + kind for kind in KINDS} | {"ph2:race", "self_only", "with@" + group, "against@" + group}
    if group in ("top+1", "several"):
        expect.add("route:long")
    else:
        forbid.add("route:long")
    return Case("stretch-k%d-%s-%s" % (k, "canonical" if canonical else "directed", group), k, canonical, kmers, b.lone,
                expect, forbid)


STRETCH_KS = (9, 15, 16, 23, 31)


def stretch_cases(ks=STRETCH_KS):
    out = []
    for k in ks:
        for canonical in (True, False):
            for group in STRETCH_GROUPS:
                case = stretch_case(k, canonical, group)
                if case is not None:
                    out.append(case)
    return out


def short_strings_case(k, canonical):
    """Strings exactly K and K + 1 long, next to a few longer ones: the second store_run starts at K - kRun."""

    def make(seed):
        b = Builder(k, canonical, seed)
        for n in (1, 2, 2, 3, 1, 2, k, k + 1):
            b.grow(n)
        seq = b.grow(2)
        b.want(seq, 0, "ruler")
        seq = b.grow(2)
        b.want(seq, 1, "ruler")
        for _ in range(4):
            b.grow(300)  # the size at which the logs fit
        return b, b.place("any")

    b, kmers = _try_seeds(make)
    return Case("short-strings-k%d-%s" % (k, "canonical" if canonical else "directed"), k, canonical, kmers, b.lone,
                {"string_K", "string_K+1", "run%d" % emit_run(k), "route:emit_logs"}, {"route:stamped"})


def log_fit_cases(k=23, n=24000):
    """Item 6: two sets of n k-mers, one with the most end k-mers whose logs still fit and one with one more: one
    long chain and lone k-mers."""
    e_max = max_ends_that_fit(n)
    out = []
    for name, n_ends in (("fits", e_max), ("over", e_max + 1)):
        def make(seed, n_ends=n_ends):
            b = Builder(k, True, seed)
            b.grow(n - (n_ends - 2))
            return b, b.place("any", pad_to=n)

        b, kmers = _try_seeds(make)
        assert kmers.size == n
        out.append(Case("log-fit-" + name, k, True, kmers, b.lone,
                        {"route:emit_logs", "route:long"} if name == "fits" else {"route:no_logs", "route:no_long"},
                        {"route:no_logs"} if name == "fits" else {"route:emit_logs", "route:long"}))
    return out


def min_l2_kmers():
    """The fewest k-mers whose ruler records reach the floor of KSH_L2_MIN."""
    c = cfg()
    return (c.l2_floor // 2 - 1) * every(c) + 1


def l2_chains_case(k=23):
    """Item 4, per chain: rulers but no level-2 ruler; exactly one, first, last and in the middle; more than
    2^kL2Shift ordinary rulers between two level-2 rulers."""
    c = cfg()
    span = 1 << c.l2_shift

    def make(seed):
        b = Builder(k, True, seed)
        for kinds in (("ruler", "ruler", "ruler"), ("l2", "ruler", "ruler"), ("ruler", "l2", "ruler"),
                      ("l2",) + ("ruler",) * (span + 3) + ("l2",), ("l2", "l2"), ("ruler",)):
            seq = b.grow(5 * len(kinds) + 7)
            for j, kind in enumerate(kinds):
                b.want(seq, 4 + 5 * j, kind)
        _chain(b, [("none", 0), ("none", 12 * k)])  # a long stretch among them
        b.grow(min_l2_kmers() * 7 // 8)
        return b, b.place("free", pad_to=min_l2_kmers())

    b, kmers = _try_seeds(make)
    return Case("l2-chains", k, True, kmers, b.lone,
                {"l2:none_on_chain", "l2:single_first", "l2:single_last", "l2:single_middle", "l2:gap_gt",
                 "l2:first_is_l2"}, {"route:stamped"}, env=("l2",))


def l2_power_case(delta, k=23):
    """Item 4: one chain with (kJumpHops + 1)^r + delta level-2 rulers, r the largest that a set at the floor of
    KSH_L2_MIN holds."""
    c = cfg()
    hops = c.jump_hops + 1
    r = 1
    while hops ** (r + 1) + 1 <= min_l2_kmers() // l2_every(c) + 1:
        r += 1
    count = hops ** r + delta

    def make(seed):
        b = Builder(k, True, seed)
        gap = l2_every(c) - every(c)  # the level-2 rulers by rank in the set: few lone k-mers bring each to its index
        seq = b.grow(gap * count)
        ranked = np.sort(synth.canonical(seq, k))
        for j in range(count):
            b.status[int(ranked[7 + gap * j])] = ("l2", None)
        return b, b.place("free", pad_to=min_l2_kmers())

    b, kmers = _try_seeds(make)
    return Case("l2-power%+d" % delta, k, True, kmers, b.lone, {"l2:pow" + ("-1", "", "+1")[delta + 1]},
                {"route:stamped"}, env=("l2",))


def one_chain_case(delta, k=23):
    """Item 4, single level: the whole set one chain, (kJumpHops + 1)^4 + delta rulers on each mirror chain."""
    c = cfg()
    rulers = (c.jump_hops + 1) ** 4 + delta
    n = (rulers - 1) * every(c) + 1

    def make(seed):
        b = Builder(k, True, seed)
        b.grow(n)
        return b, b.place("any")

    b, kmers = _try_seeds(make)
    assert kmers.size == n
    return Case("one-chain%+d" % delta, k, True, kmers, b.lone, {"jump:pow" + ("-1", "", "+1")[delta + 1]},
                {"route:stamped"})


def loop_case(k=23, l2=False):
    """Item 5: a non-branching loop of a few thousand k-mers in a set with long stretches and logs that would fit;
    loops with exactly one sampled k-mer and with none; with l2, at the floor of KSH_L2_MIN, a loop of rulers that
    holds a level-2 ruler and one that holds none."""
    c = cfg()

    def make(seed):
        b = Builder(k, True, seed)
        big = b.grow(3000, circular=True)
        b.want(big, 100, "l2" if l2 else "ruler")
        small = b.grow(200, circular=True)  # a loop of rulers without a level-2 ruler
        for j in (10, 50, 90):
            b.want(small, j, "ruler")
        one = b.grow(40, circular=True)
        for j in range(40):
            b.want(one, j, "ruler" if j == 7 else "none")
        none = b.grow(30, circular=True)
        for j in range(30):
            b.want(none, j, "none")
        _chain(b, [("none", 0), ("none", 12 * k)])  # a long stretch
        b.grow(min_l2_kmers() * 7 // 8 if l2 else 2000)
        return b, b.place("free", pad_to=min_l2_kmers() if l2 else 0)

    b, kmers = _try_seeds(make)
    expect = {"route:stamped", "loop:large", "loop:with_long_and_logs", "loop:one_sampled", "loop:unsampled",
              "loop:rulers_no_l2"} | ({"loop:rulers_with_l2"} if l2 else set())
    return Case("loops-l2" if l2 else "loops", k, True, kmers, b.lone, expect, (), env=("l2",) if l2 else ())


def junction_case(k=15, full=True):
    """match_more_rounds: junctions of four unitigs that end with a (K-1)-mer and four that start with it.  The
    sides of a junction are matched among themselves alone (a side's edges all run through its junction), every
    edge of the junction's unitig with the smallest id has a smaller priority than every other edge there, so a
    live round matches exactly one pair: the four pairs take four rounds and the empty round after them is the
    fifth, one more than kMatchFirst.  (No junction has more than four sides a side: five is the most rounds any
    set takes, and kMatchFirst + kMatchBatch is out of reach.)"""

    def make(seed):
        b = Builder(k, True, seed)
        for _ in range(3 if full else 0):
            j = int(b.rng.integers(0, 1 << (2 * (k - 1))))
            if b._sub(j) is None or b._sub(j) in b.used:
                raise PlacementError("the junction is taken")
            b.used.add(b._sub(j))
            for _ in range(4):
                b.grow(6, prefix=j)                     # starts with the junction
                b.grow(6, prefix=_rc_int(j, k - 1))     # ends with it, read from the other strand
        b.grow(400)
        return b, b.place("any")

    b, kmers = _try_seeds(make)
    return Case("junctions" if full else "plain-genome", k, True, kmers, b.lone,
                {"rounds>first"} if full else set(), set() if full else {"rounds>first"}, want_rounds=True)


def small_k_case(k, canonical, seed, lengths):
    """A K too small for placed rulers (a K = 5 set has 120 (K-1)-mers to build from: the lone k-mers of a placement
    would take them, and their end k-mers would keep the logs from fitting): chains of the given lengths with the
    rulers where they fall, at a seed found by small_k_search.  The case states no stretch lengths; the model
    reports those it has, and SMALL_K_BRANCHES says what the committed seeds reach together."""
    b = Builder(k, canonical, seed)
    for n in lengths:
        b.grow(n)
    kmers = b.place("any")
    fits = logs_fit(kmers.size, Links(kmers, k, canonical).ends.size)
    name = "small-k%d-%s-%s-seed%d" % (k, "canonical" if canonical else "directed", "+".join(map(str, lengths)), seed)
    return Case(name, k, canonical, kmers, b.lone, {"run%d" % emit_run(k), "route:emit_logs" if fits else "route:no_logs"},
                {"route:stamped"})


SMALL_K_SEARCH_LENGTHS = ((46, 30, 16, 1, 1), (46, 30, 5, 6), (46, 30, 7, 11), (41, 40, 5, 1), (42, 40, 6), (41, 42, 11),
                          (40, 41, 42), (60, 41, 2), (100, 5), (95, 11, 5), (88, 21, 3))


def small_k_search(k, canonical, lengths=SMALL_K_SEARCH_LENGTHS, seeds=range(160)):
    """[(lengths, seed)] picked greedily by the stretch and direction branches they add, among the small_k_cases
    whose logs fit, over a bounded range of chain lengths and seeds (how SMALL_K_SETS was found; the sets with a
    stretch of 2 (n_mid + 1) K steps and more come from the same search over (84, 20), (104,) and (81, 15) up to
    seed 600: a ruler-free chain that long needs a set of at most three sampled indices, 96 k-mers, or luck)."""
    want = set(STRETCH_BRANCHES + DIRECTION_BRANCHES)
    per = {}
    for ln in lengths:
        for seed in seeds:
            try:
                got = small_k_case(k, canonical, seed, ln).branches()
            except PlacementError:
                continue
            if "route:emit_logs" in got:
                per[(ln, seed)] = got & want
    chosen, covered = [], set()
    while per:
        best = max(per, key=lambda key: (len(per[key] - covered), -key[1]))
        if not per[best] - covered:
            break
        chosen.append(best)
        covered |= per[best]
    return chosen


# K = 5: chains with the rulers where they fall, logs in use (small_k_search); K = 3 has six (K-1)-mers to build from
# and no set of 3-mers whose logs fit (see small_k_unreachable)
SMALL_K_SETS = {
    (5, True): (((46, 30, 7, 11), 87), ((42, 40, 6), 60), ((46, 30, 5, 6), 94), ((41, 42, 11), 71), ((60, 41, 2), 3),
                ((100, 5), 84), ((41, 40, 5, 1), 3), ((100, 5), 79), ((100, 5), 4), ((100, 5), 5), ((100, 5), 105),
                ((84, 20), 434)),
    (5, False): (((46, 30, 7, 11), 80), ((46, 30, 5, 6), 31), ((60, 41, 2), 57), ((41, 42, 11), 12), ((42, 40, 6), 5),
                 ((41, 42, 11), 138), ((46, 30, 7, 11), 77), ((100, 5), 146), ((46, 30, 5, 6), 2), ((100, 5), 8),
                 ((42, 40, 6), 27), ((104,), 322), ((81, 15), 86)),
    (3, True): (((4,), 0), ((4,), 1)),
    (3, False): (((4,), 0),),
}
# what the K = 5 sets reach together: every stretch length and kind and both directions at every boundary length
SMALL_K_BRANCHES = {
    (5, True): set(STRETCH_BRANCHES + DIRECTION_BRANCHES) | {"route:emit_logs", "run4"},
    (5, False): set(STRETCH_BRANCHES + DIRECTION_BRANCHES) | {"route:emit_logs", "run4"},
}


def small_k_unreachable():
    """{n: the largest n_ends with which the logs of a set of n k-mers fit (-1: none)} for the n a set of 3-mers can
    have.  No set of 3-mers takes the log emit (the byte-by-byte stores, run0, there): below 30 k-mers the 64 bytes
    of the long list alone keep the logs from fitting a set with the two end k-mers of a chain; a set of n >= 30
    3-mers as read has n edges between sixteen 2-mers, so at least n - 16 of its k-mers leave a 2-mer that another
    one leaves too, which makes each an end k-mer, more than fit; and the canonical sets of 30 to 32 3-mers (there
    are 32 canonical 3-mers) are few enough to count (tests/test_chain_rank_model_cpu.py does both)."""
    return {n: max([e for e in range(0, n + 1) if logs_fit(n, e)], default=-1) for n in range(1, 65)}


def small_k_cases():
    return [small_k_case(k, canonical, seed, lengths) for (k, canonical), sets in SMALL_K_SETS.items()
            for lengths, seed in sets]


_CASES = {}


def _memo(key, fn):
    if key not in _CASES:
        _CASES[key] = fn()
    return _CASES[key]


def small_cases():
    """Items 1, 2, 3, 7 and the matching rounds: a few thousand k-mers each."""
    def build():
        out = stretch_cases()
        out += [short_strings_case(k, canonical) for k in (9, 15, 16, 23, 31) for canonical in (True, False)]
        out += [junction_case(full=True), junction_case(full=False)]
        return out + small_k_cases()
    return _memo("small", build)


def medium_cases():
    """Item 6 and the single-level jumping: a few tens of thousands."""
    return _memo("medium", lambda: log_fit_cases() + [one_chain_case(d) for d in (-1, 0, 1)] + [loop_case(l2=False)])


def l2_cases():
    """Items 4 and 5 under KSH_L2_MIN at its floor: the smallest sets the floor allows."""
    return _memo("l2", lambda: [l2_chains_case()] + [l2_power_case(d) for d in (-1, 0, 1)] + [loop_case(l2=True)])


def all_cases():
    return small_cases() + medium_cases() + l2_cases()

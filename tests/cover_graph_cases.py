"""Designed unitig graphs for the unitig-level stage of the path cover (cover_stage in csrc/ksh_encode.hip: the
greedy matching in batches of rounds, the loop cut, the walks under their round allowance, the string order) and for
the four kernels of csrc/ksh_cover.hip that feed it from caller-supplied strings, with a plain numpy / Python model
of that stage.

ksh_spss_cover_plan takes the caller's strings as the nodes and their end k-mers as the edges, so any unitig graph
can be hand-built from a few short strings and runs through exactly the code the encode runs.  A *family* below is
a list of such inputs, each the smallest shape that reaches one branch of the stage; every case says which model
branches it must (expect) and must not (forbid) reach, and check_case() asserts that -- and that the model's edge
table holds exactly the designed edges -- before anything runs, so a case cannot silently test something else.

The *model* (model()) is written from the contract in include/kmersets_hip.h and the kernels' comments: the edge
table of both rules, the parallel matching round by round with the priorities of slot_priority, the loops of the
matched graph with the node the ascending union-by-rank replay cuts them at, the open paths and the number of
k_walk_jump launches a worst-case schedule needs, the classes, string ids and every unitig's (sid, koff, flip), and
from those the output strings.  It is never the expected answer of a GPU test: that is the oracle
(tests/cover_oracle.py over oracle/ko_spss.h); tests/test_cover_graph_model_cpu.py pins the model to the oracle on
every case.  What the model adds is the things the oracle does not say: round counts, loop lengths, cut nodes,
walk lengths, input phases.

The constants the families are built around are read from the kernels' text; the lines the cases rely on must
stand there as written (constants()), so a changed constant moves the cases or fails the CPU test.

How many matching rounds can an input need?  The sides that share one (k-1)-mer X form one connected component
of the edge table: the sides that look out over X on one hand, those that look out over rc(X) on the other.  Two
sides of the same hand would need end k-mers a.X with the same a, which the preconditions forbid, so a hand holds
at most four sides and the component is a K(a, b) with a, b <= 4 (less the edges from a string to itself; a
complete graph on at most four sides when X is its own reverse complement).  A live round commits at least the
component's edge of smallest priority, a component has at most min(a, b) <= 4 commits, so no input has more than
4 live rounds: the reported count is at most 5 = kMatchFirst + 1, the second batch is entered (by a K(4, 4) whose
predecessors all come before its successors) and never left for a third.  No input needs more than kMatchFirst +
kMatchBatch rounds, and none is faked here."""
import os
import re
from collections import namedtuple

import numpy as np

import cover_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc")
FILES = {"encode": "ksh_encode.hip", "cover": "ksh_cover.hip"}
U = np.uint64
K = 15  # the designed graphs: long enough that a few thousand random strings share no (k-1)-mer by accident
K_LONG = 31  # ... and a few ten thousand


def k_for(length):
    return K if length < 1000 else K_LONG


# ---- constants from the kernels' text --------------------------------------------------------------------------------
def sources():
    return {name: open(os.path.join(CSRC, f)).read() for name, f in FILES.items()}


# anchored patterns with one number each: (constant, file, pattern); each must match exactly once
NUMBERS = (
    ("match_first", "encode", r"^constexpr int kMatchFirst = (\d+);"),
    ("match_batch", "encode", r"^constexpr int kMatchBatch = (\d+);"),
    ("walk_rounds_max", "encode", r"^constexpr int kWalkRoundsMax = (\d+);"),
    ("jump_hops", "encode", r"^#define KSH_JUMP_HOPS (\d+)$"),
    ("walk_rounds_start", "encode", r"^  walk_rounds = (\d+);"),
    ("loop_cut_block", "encode", r"^__global__ __launch_bounds__\((\d+)\) void k_loop_cut\("),
    ("emit_run", "cover", r"^constexpr int kCoverEmitRun = (\d+);"),
    ("table_factor", "encode", r"^  while \(cap < uint64_t\((\d+) \* n\)\) cap <<= 1;"),
)
# the lines the model restates: (file, line, how often it stands there)
RESTATED = (
    ("encode", "#ifndef KSH_JUMP_HOPS", 1),
    ("encode", "constexpr int kJumpHops = KSH_JUMP_HOPS;", 1),
    ("encode", "  for (int64_t x = 2 * n_u; x > 1; x /= (kJumpHops + 1)) walk_rounds++;", 1),
    ("encode", "  walk_rounds = std::min(walk_rounds, kWalkRoundsMax);", 1),
    ("encode", "  if (directed && !(v & 1)) return ~uint64_t(0);", 1),
    ("encode", "  return uint64_t(v >> 1) * 8 + ((v & 1) ? 0 : 4) + uint64_t(c);", 1),
    ("encode", "      const int batch = p->rounds ? kMatchBatch : kMatchFirst;", 1),
    ("encode", "      p->rounds += more ? batch : ran + 1;  // (the round that found nothing counts, as before)", 1),
    ("encode", "    hipLaunchKernelGGL(k_loop_cut, dim3(unsigned((n_u + 63) / 64)), dim3(64), 0, st, p->mate, n_u,", 1),
    ("encode", "  const int64_t cut = 2 * int64_t(root_node) + (directed ? 1 : 0);", 1),
    ("encode", "    if (uint32_t(u) <= far_end) cls = hl ? 1 : 0;", 1),
    ("cover", "  uint64_t h = hash_key(key) & cap_mask;", 2),
    ("cover", "  const int64_t q0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * kCoverEmitRun;", 1),
    ("cover", "    if (u_koff[u] && t < k - 1) continue;", 1),
    ("cover", "  if (off + k > 32 && w + 1 < n_words) x |= words[w + 1] >> (64 - 2 * off);", 1),
)

Consts = namedtuple("Consts", [name for name, _, _ in NUMBERS])


def anchor_counts(src=None):
    """How often every anchor stands in its file: [(what, found, wanted)]."""
    src = src or sources()
    out = [(name, len(re.findall(pat, src[f], flags=re.M)), 1) for name, f, pat in NUMBERS]
    out += [(line, src[f].count(line), times) for f, line, times in RESTATED]
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    out.append(("the build leaves KSH_JUMP_HOPS at its default", makefile.count("KSH_JUMP_HOPS"), 0))
    return out


def constants(src=None):
    src = src or sources()
    for what, found, wanted in anchor_counts(src):
        assert found == wanted, "the kernels' text has %d x (wanted %d x): %s" % (found, wanted, what)
    return Consts(*[int(re.search(pat, src[f], flags=re.M).group(1)) for _, f, pat in NUMBERS])


C = constants()
assert C.loop_cut_block == 64 and C.walk_rounds_start == 3 and C.table_factor == 4


def walk_allowance(n_u, c=C):
    """The host's walk_rounds for n_u unitigs."""
    rounds, x = c.walk_rounds_start, 2 * n_u
    while x > 1:
        x //= c.jump_hops + 1
        rounds += 1
    return min(rounds, c.walk_rounds_max)


_need = {}


def walk_need(length, hops=None):
    """k_walk_jump launches that an open path of `length` states needs under the worst schedule: every hop of a
    launch reads its successor as the launch before left it (any fresher word only reaches further), the launch
    that finds nothing to change included -- the host looks at the last launch's flag."""
    hops = hops or C.jump_hops
    if (length, hops) in _need:
        return _need[(length, hops)]
    # state at distance d from the walk's last state (d = 0: done from the start); span = distance to `next`
    d = np.arange(length, dtype=np.int64)
    done = d == 0
    span = np.where(done, 0, 1).astype(np.int64)
    launches = 0
    while True:
        launches += 1
        if done.all():
            break
        new_done, new_span = done.copy(), span.copy()
        active = ~done
        for _ in range(hops):
            t = d - new_span  # the state `next` points at
            theirs_done, theirs_span = done[t], span[t]
            finish = active & theirs_done
            new_done |= finish
            new_span = np.where(finish, d, np.where(active, new_span + theirs_span, new_span))
            active &= ~finish
        done, span = new_done, new_span
        assert launches < 100
    _need[(length, hops)] = launches
    return launches


# ---- k-mers ----------------------------------------------------------------------------------------------------------
_DIGITS = str.maketrans("ACGT", "0123")
revcomp_string = cover_oracle.revcomp_string


def kmer_of(s):
    return int(s.translate(_DIGITS), 4)


def revcomp_bits(x, k):
    """Reverse complement of 2-bit packed k-mers (uint64 array), base by base."""
    x = np.asarray(x, dtype=U)
    out = np.zeros_like(x)
    for _ in range(k):
        out = (out << U(2)) | (U(3) - (x & U(3)))
        x = x >> U(2)
    return out


def hash_key(x):
    """splitmix64 finaliser, as the end table of k_cover_ends hashes its keys."""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return x ^ (x >> U(31))


def table_cap(n):
    cap = 1
    while cap < C.table_factor * n:
        cap <<= 1
    return cap


# ---- the model -------------------------------------------------------------------------------------------------------
FAST, SLOW, DIRECTED = "fast", "slow", "directed"
ARGS = {FAST: dict(canonical=True, fast=True), SLOW: dict(canonical=True, fast=False),
        DIRECTED: dict(canonical=False, fast=True)}
NONE = -1


def _lookup(keys, q):
    """Index of every q in keys (unique), or NONE."""
    if keys.size == 0:
        return np.full(q.shape, NONE, dtype=np.int64)
    order = np.argsort(keys, kind="stable")
    at = np.minimum(np.searchsorted(keys[order], q), keys.size - 1)
    return np.where(keys[order][at] == q, order[at], NONE)


def meets_preconditions(P, S, lens, k, directed):
    """include/kmersets_hip.h: canonical -- the canonical forms of the end k-mers pairwise distinct across strings,
    first and last of one string equal (in canonical form) only in a K-long string, none its own reverse complement;
    directed -- the first k-mers pairwise distinct, and the last."""
    if directed:
        return np.unique(P).size == P.size and np.unique(S).size == S.size
    rp, rs = revcomp_bits(P, k), revcomp_bits(S, k)
    cp, cs = np.minimum(P, rp), np.minimum(S, rs)
    same = cp == cs
    if (P == rp).any() or (S == rs).any() or (same & (np.array(lens) != k)).any():
        return False
    ends = np.concatenate([cp, cs[~same]])
    return np.unique(ends).size == ends.size


def edge_table(strings, k, directed):
    """edges[2 i + side][c] (side 0 = left, 1 = right): the vertex met, or NONE.  include/kmersets_hip.h: the right
    side of i meets j != i where P_j == Next(S_i, c) (j's left side) or S_j == rc(Next(S_i, c)) (j's right side), the
    left side where S_j == Prev(P_i, c) (right side) or P_j == rc(Prev(P_i, c)) (left side); directed: P_j ==
    Next(S_i, c) only, seen from both of its ends."""
    n = len(strings)
    P = np.array([kmer_of(s[:k]) for s in strings], dtype=U)
    S = np.array([kmer_of(s[len(s) - k:]) for s in strings], dtype=U)
    assert meets_preconditions(P, S, [len(s) for s in strings], k, directed), "not an input ksh_spss_cover_plan takes"
    mask = U((1 << (2 * k)) - 1)
    me = np.arange(n, dtype=np.int64)
    edges = np.full((2 * n, 4), NONE, dtype=np.int64)
    for c in range(4):
        nxt = ((S << U(2)) | U(c)) & mask
        prv = (P >> U(2)) | (U(c) << U(2 * (k - 1)))
        for side, y, as_is, flipped in ((1, nxt, P, S), (0, prv, S, P)):
            j = _lookup(as_is, y)  # the other string continues this one as it stands: its opposite side
            hit = (j != NONE) & (j != me)
            edges[2 * me[hit] + side, c] = 2 * j[hit] + (1 - side)
            if directed:
                continue
            j = _lookup(flipped, revcomp_bits(y, k))  # ... reverse-complemented: its same side
            hit = (j != NONE) & (j != me)
            assert (edges[2 * me[hit] + side, c] == NONE).all(), "two strings behind one candidate: preconditions"
            edges[2 * me[hit] + side, c] = 2 * j[hit] + side
    return edges, P, S


def match_parallel(edges, directed):
    """k_match_best / k_match_commit round by round.  Returns (mate, reported rounds = live rounds + 1)."""
    nv = edges.shape[0]
    inf = np.iinfo(np.int64).max
    v = np.arange(nv, dtype=np.int64)[:, None]
    own = (v >> 1) * 8 + np.where(v & 1, 0, 4) + np.arange(4, dtype=np.int64)[None, :]  # slot_priority
    if directed:
        own = np.where(v & 1, own, inf)
    own = np.where(edges != NONE, own, inf)
    back = np.full(edges.shape, inf, dtype=np.int64)  # the priority of the same edge seen from its other end
    w = np.where(edges != NONE, edges, 0)
    for c2 in range(4):
        back = np.minimum(back, np.where((edges[w, c2] == v) & (edges != NONE), own[w, c2], inf))
    prio = np.minimum(own, back)
    mate = np.full(nv, NONE, dtype=np.int64)
    live = 0
    while True:
        free = (mate == NONE)
        cand = np.where((edges != NONE) & free[:, None] & free[w], prio, inf)
        best = cand.min(axis=1)
        if not (best < inf).any():
            break
        live += 1
        bw = np.where(best < inf, edges[np.arange(nv), cand.argmin(axis=1)], NONE)
        pick = np.where(bw != NONE, bw, 0)
        commit = (bw != NONE) & (bw[pick] == np.arange(nv)) & (best[pick] == best)
        mate[commit] = bw[commit]
        assert live <= 64
    return mate, live + 1


def match_slow(edges):
    """fast = false: from every node without an edge yet, one path extended as far as it goes, through the first
    edge whose far side is free and that does not come back to the start (k_match_slow)."""
    e = edges.tolist()
    n = len(e) // 2
    mate = [NONE] * (2 * n)
    for i in range(n):
        if mate[2 * i] != NONE or mate[2 * i + 1] != NONE:
            continue
        any_l = any(x != NONE for x in e[2 * i])
        any_r = any(x != NONE for x in e[2 * i + 1])
        if not any_l and not any_r:
            continue
        v = 2 * i + (1 if any_r else 0)
        while mate[v] == NONE:
            pick = NONE
            for w in e[v]:
                if w != NONE and (w >> 1) != i and mate[w] == NONE:
                    pick = w
                    break
            if pick == NONE:
                break
            mate[v], mate[pick] = pick, v
            v = pick ^ 1
    return np.array(mate, dtype=np.int64)


Loop = namedtuple("Loop", "length smallest cut flips blocks")


def cut_loops(mate, directed):
    """The loops of the matched graph and the node the reference's serial union-by-rank replay (nodes ascending,
    left edge before right; lower rank, then lower index, becomes the child) leaves as each one's root: its left
    edge (directed: its outgoing edge) is dropped.  Returns the loops; mate is changed in place."""
    n = mate.size // 2
    m = mate.tolist()
    parent, rank = list(range(n)), [0] * n

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    def unite(a, b):
        a, b = find(a), find(b)
        if a == b:
            return
        if rank[a] > rank[b] or (rank[a] == rank[b] and a > b):
            a, b = b, a
        parent[a] = b
        if rank[a] == rank[b]:
            rank[b] += 1

    for i in range(n):
        if not directed and m[2 * i] != NONE:
            unite(i, m[2 * i] >> 1)
        if m[2 * i + 1] != NONE:
            unite(i, m[2 * i + 1] >> 1)
    root_of = [find(i) for i in range(n)]
    open_roots = set()
    for i in range(n):
        if m[2 * i + 1] == NONE or (not directed and m[2 * i] == NONE):
            open_roots.add(root_of[i])
    members = {}
    for i in range(n):
        if root_of[i] not in open_roots:
            members.setdefault(root_of[i], []).append(i)
    loops = []
    for root, nodes in sorted(members.items(), key=lambda kv: kv[1][0]):
        # the lap from the smallest node out of its right side, as k_loop_cut walks it
        cur, going_right, flips, steps = nodes[0], True, 0, 0
        while True:
            w = m[2 * cur + (1 if going_right else 0)]
            assert w != NONE
            flips += int(((w & 1) == 0) != going_right)
            cur, going_right = w >> 1, (w & 1) == 0
            steps += 1
            if cur == nodes[0]:
                break
        assert steps == len(nodes)
        loops.append(Loop(len(nodes), nodes[0], root, flips, len({x // C.loop_cut_block for x in nodes})))
        cut = 2 * root + (1 if directed else 0)
        other = m[cut]
        mate[cut] = NONE
        mate[other] = NONE
    return loops


Result = namedtuple("Result", "strings edges mate rounds loops paths sid koff flip classes out_lens")


def model(strings, k, mode):
    """The unitig-level stage on `strings` under mode FAST, SLOW or DIRECTED."""
    directed = mode == DIRECTED
    n = len(strings)
    edges, _, _ = edge_table(strings, k, directed)
    if mode == SLOW:
        mate, rounds, loops = match_slow(edges), 0, []
    else:
        mate, rounds = match_parallel(edges, directed)
        loops = cut_loops(mate, directed)
    m = mate.tolist()
    u_len = [len(s) - k + 1 for s in strings]

    def walk(start, going_right):
        path, cur = [], start
        while True:
            path.append((cur, not going_right))
            w = m[2 * cur + (1 if going_right else 0)]
            if w == NONE:
                return path
            cur, going_right = w >> 1, (w & 1) == 0
            assert len(path) <= n, "the path cover still holds a loop"

    # the starts, by class: 0 = from a left terminal, 1 = from a right terminal, 2 = isolated
    starts, classes, paths = [[], [], []], {}, []
    for u in range(n):
        hl, hr = m[2 * u] != NONE, m[2 * u + 1] != NONE
        if directed:
            if not hl:
                starts[0].append((u, walk(u, True)))
                classes[u] = 0
                paths.append(len(starts[0][-1][1]))
            continue
        if hl and hr:
            continue
        if not hl and not hr:
            cls, path = 2, [(u, mode == SLOW)]  # fast = false spells an isolated string reverse-complemented
        else:
            cls, path = (0 if not hl else 1), walk(u, not hl)
        if path[0][0] <= path[-1][0]:
            starts[0 if mode == SLOW else cls].append((u, path))
            classes[u] = cls
            paths.append(len(path))
    sid = np.full(n, NONE, dtype=np.int64)
    koff = np.zeros(n, dtype=np.int64)
    flip = np.zeros(n, dtype=np.int64)
    out = []
    for _, path in starts[0] + starts[1] + starts[2]:
        parts, at = [], 0
        for i, (u, flipped) in enumerate(path):
            s = revcomp_string(strings[u]) if flipped else strings[u]
            parts.append(s if i == 0 else s[k - 1:])
            sid[u], koff[u], flip[u] = len(out), at, int(flipped)
            at += u_len[u]
        out.append("".join(parts))
    assert (sid != NONE).all(), "a string that no path holds"
    return Result(out, edges, mate, rounds, loops, paths, sid, koff, flip, classes, [len(s) for s in out])


def edge_pairs(edges):
    v, c = np.nonzero(edges != NONE)
    pairs = {(int(a), int(b)) for a, b in zip(v, edges[v, c])}
    assert all((b, a) in pairs for a, b in pairs), "an edge seen from one end only"
    return {frozenset(p) for p in pairs}


def geometry(strings, k, results):
    """Branches of the cover kernels: the word phases of the end k-mers (k_cover_ends' kmer_at), the table, and what
    the kCoverEmitRun-base runs of k_cover_emit meet under each mode's (koff, flip)."""
    b = set()
    lens = np.array([len(s) for s in strings], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(lens)])
    total = int(start[-1])
    n_words = (total + 31) // 32
    for name, at in (("first", start[:-1]), ("last", start[1:] - k)):
        ph = at % 32
        b |= {"%s_phase=%d" % (name, p) for p in set(ph.tolist())}
        if (ph + k > 32).any():
            b.add(name + "_crosses_word")
        if (((at + k - 1) // 32) == n_words - 1).any():
            b.add(name + "_in_final_word")
    b.add("stream_ends_at_word_end" if total % 32 == 0 else "final_word_partial")
    if ((start[1:] % 32) == 0).any():
        b.add("last_ends_at_word_end")
    n = len(strings)
    b.add("n=%d" % n if n <= 5 else "n>5")
    b.add("cap=%d" % table_cap(n) if n <= 5 else "cap>32")
    owner = np.repeat(np.arange(n), lens)
    run = C.emit_run
    pad = (-total) % run
    own = np.concatenate([owner, np.full(pad, n - 1)]).reshape(-1, run)
    spans = (np.diff(own, axis=1) != 0).sum(axis=1) + 1
    b |= {"run_spans=%d" % s for s in set(spans.tolist())}
    off = np.arange(total) - start[owner]  # source offset within the string
    for r in results:
        t = np.where(r.flip[owner] != 0, lens[owner] - 1 - off, off)
        skipped = (r.koff[owner] != 0) & (t < k - 1)
        flipped = np.concatenate([r.flip[owner] != 0, np.zeros(pad, dtype=bool)]).reshape(-1, run)
        skip = np.concatenate([skipped, np.zeros(pad, dtype=bool)]).reshape(-1, run)
        if ((spans > 1) & flipped.any(axis=1)).any():
            b.add("run_crosses_in_flipped")
        if flipped.any():
            b.add("run_in_flipped")
        if skip.any():
            b.add("run_in_overlap")
        if (skip.any(axis=1) & ~skip.all(axis=1)).any():
            b.add("run_part_overlap")
    return b


def table_wraps(strings, k, directed=False):
    """Does some probe sequence of the end table run past its last slot?  (Which key ends where is a race; which
    slots end up taken is not: linear probing fills the same slots in any order.)"""
    P = np.array([kmer_of(s[:k]) for s in strings], dtype=U)
    S = np.array([kmer_of(s[len(s) - k:]) for s in strings], dtype=U)
    cap = table_cap(len(strings))
    tables = [P, S] if directed else [np.unique(np.concatenate([np.minimum(P, revcomp_bits(P, k)),
                                                                 np.minimum(S, revcomp_bits(S, k))]))]
    wrapped = False
    for keys in tables:
        taken = np.zeros(cap, dtype=bool)
        for h in (hash_key(keys) & U(cap - 1)).tolist():
            while taken[h]:
                h += 1
                if h == cap:
                    h, wrapped = 0, True
            taken[h] = True
    return wrapped


def branches(k, strings, results_by_mode):
    b = set()
    for mode, r in results_by_mode.items():
        if mode != SLOW:
            b.add("rounds=%d" % r.rounds)
            b.add("second_batch" if r.rounds - 1 >= C.match_first else "first_batch_only")
            if r.rounds - 1 == C.match_first - 1:
                b.add("first_batch_full_less_one")
            if r.rounds > C.match_first + C.match_batch:
                b.add("third_batch")
        e = r.edges
        if mode != DIRECTED and ((e != NONE) & ((e & 1) == (np.arange(e.shape[0])[:, None] & 1))).any():
            b.add("same_side_edge")
        tag = "directed_" if mode == DIRECTED else ""
        for lp in r.loops:
            b.add(tag + "loop_len=%d" % lp.length)
            b.add(tag + ("cut_at_smallest" if lp.cut == lp.smallest else "cut_not_smallest"))
            if lp.flips:
                b.add("lap_flips")
            if lp.blocks > 1:
                b.add("loop_spans_blocks")
        b.add(tag + ("loops=%d" % len(r.loops) if len(r.loops) <= 1 else "loops>1"))
        if mode == SLOW:
            b.add("slow")
            if any(c == 2 for c in r.classes.values()):
                b.add("slow_isolated_flipped")
        else:
            b |= {tag + "class%d" % c for c in r.classes.values()}
        for length in r.paths:
            need, allow = walk_need(length), walk_allowance(len(strings))
            assert need <= allow, "a path of %d states needs %d launches, %d strings allow %d" % (
                length, need, len(strings), allow)
            b.add("walk_need=%d" % need)
        if mode == FAST:
            b.add("walk_allow=%d" % walk_allowance(len(strings)))
        if mode == FAST:
            m = r.mate
            n = len(strings)
            hl, hr = m[0::2] != NONE, m[1::2] != NONE
            kept = np.zeros(n, dtype=bool)
            kept[np.array(list(r.classes), dtype=np.int64)] = True
            if ((hl != hr) & ~kept).any():
                b.add("skipped_walk")
            # a path whose two terminals are of one kind: u <= far_end alone decides which of them starts the string
            ends = {}
            for u in np.nonzero(hl != hr)[0].tolist():
                ends.setdefault(int(r.sid[u]), []).append(bool(hl[u]))
            for kinds in ends.values():
                if len(kinds) == 2 and kinds[0] == kinds[1]:
                    b.add("both_right_terminals" if kinds[0] else "both_left_terminals")
    b |= geometry(strings, k, list(results_by_mode.values()))
    return b


# ---- cases -----------------------------------------------------------------------------------------------------------
class Case:
    """One input: the strings, the modes it runs under, the designed edges (vertex pairs of the canonical rule; None:
    not designed, a dense graph), the branches it must and must not reach."""

    def __init__(self, name, family, k, strings, modes, designed=None, expect=(), forbid=(), wraps=False):
        self.name, self.family, self.k, self.strings, self.modes = name, family, k, list(strings), tuple(modes)
        self.designed, self.expect, self.forbid, self.wraps = designed, frozenset(expect), frozenset(forbid), wraps
        self._results = None

    def __repr__(self):
        return self.name

    def results(self):
        if self._results is None:
            self._results = {mode: model(self.strings, self.k, mode) for mode in self.modes}
        return self._results

    def branches(self):
        b = branches(self.k, self.strings, self.results())
        if self.wraps and table_wraps(self.strings, self.k):
            b.add("table_wrap")
        return b


def check_case(case):
    """What the runner asserts before a case runs: the designed edges, expect and forbid.  Returns the model's
    results by mode."""
    res = case.results()
    if case.designed is not None:
        for mode, r in res.items():
            want = case.designed if mode != DIRECTED else {e for e in case.designed if sum(v & 1 for v in e) == 1}
            got = edge_pairs(r.edges)
            assert got == want, "%s (%s): %d edges beside the designed ones, %d designed ones missing" % (
                case.name, mode, len(got - want), len(want - got))
    b = case.branches()
    assert case.expect <= b, "%s does not reach %s" % (case.name, sorted(case.expect - b))
    assert not (case.forbid & b), "%s reaches %s" % (case.name, sorted(case.forbid & b))
    return res


def rand_seq(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8).tobytes().translate(
        bytes.maketrans(b"\x00\x01\x02\x03", b"ACGT")).decode()


def arrange(strings, designed, order, flips):
    """New string j = old string order[j], reverse-complemented where flips[j]; the designed edges follow."""
    new_of = {int(old): j for j, old in enumerate(order)}
    out = [revcomp_string(strings[old]) if f else strings[old] for old, f in zip(order, flips)]
    if designed is None:
        return out, None
    move = lambda v: 2 * new_of[v >> 1] + ((v & 1) ^ int(flips[new_of[v >> 1]]))
    return out, {frozenset(move(v) for v in e) for e in designed}


def shuffled(strings, designed, seed, flip):
    """cover_oracle.shuffled, with the designed edges carried along."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(strings))
    flips = rng.integers(0, 2, size=len(strings)) if flip else np.zeros(len(strings), dtype=np.int64)
    out, moved = arrange(strings, designed, order, flips)
    assert out == cover_oracle.shuffled(strings, seed, flip)
    return out, moved


def presentations(name, family, k, strings, designed, modes, expect=(), forbid=(), loose=(), seed=1, **kw):
    """A case as built, shuffled, and shuffled with a random half reverse-complemented.  `loose`: the part of
    expect that holds for the case as built only (it depends on the order or the orientation)."""
    out = [Case(name, family, k, strings, modes, designed, set(expect) | set(loose), forbid, **kw)]
    s, d = shuffled(strings, designed, seed, False)
    out.append(Case(name + "/shuffled", family, k, s, modes, d, expect, forbid, **kw))
    s, d = shuffled(strings, designed, seed + 1, True)
    out.append(Case(name + "/shuffled+rc", family, k, s, modes, d, expect, forbid, **kw))
    return out


def compose(parts):
    """Several (strings, designed) side by side."""
    strings, designed = [], set()
    for s, d in parts:
        designed |= {frozenset(v + 2 * len(strings) for v in e) for e in d}
        strings += s
    return strings, designed


def valid(strings, k, directed=False):
    P = np.array([kmer_of(s[:k]) for s in strings], dtype=U)
    S = np.array([kmer_of(s[len(s) - k:]) for s in strings], dtype=U)
    return meets_preconditions(P, S, [len(s) for s in strings], k, directed)


def junction(rng, k, ins, outs, filler=6, x=None):
    """Strings that end in a.X for a in `ins` and strings that start with X.b for b in `outs`, X one (k-1)-mer: every
    one of the former meets every one of the latter.  Returns (strings, designed): the `ins` first."""
    x = x or rand_seq(rng, k - 1)
    strings = [rand_seq(rng, filler) + a + x for a in ins] + [x + b + rand_seq(rng, filler) for b in outs]
    designed = {frozenset((2 * i + 1, 2 * (len(ins) + j))) for i in range(len(ins)) for j in range(len(outs))}
    return strings, designed


def path_pieces(rng, k, length, adv=3):
    """A random sequence cut into `length` pieces of adv + k - 1 bases that overlap by k - 1: one open path."""
    while True:  # (among some 10^4 random 15-mers two ends do coincide now and then: draw again)
        seq = rand_seq(rng, length * adv + k - 1)
        strings = [seq[p * adv:p * adv + adv + k - 1] for p in range(length)]
        if valid(strings, k):
            break
    return strings, {frozenset((2 * p + 1, 2 * p + 2)) for p in range(length - 1)}


def cycle_pieces(rng, k, length, adv=3):
    """One circular sequence cut into `length` pieces that overlap by k - 1: a loop with no branch."""
    adv = max(adv, -(-(k + 1) // length))  # (the circle at least k + 1 long: a short one would repeat its k-mers)
    while True:
        circ = rand_seq(rng, length * adv)
        ext = circ + circ[:k - 1]
        strings = [ext[p * adv:p * adv + adv + k - 1] for p in range(length)]
        if valid(strings, k):
            break
    return strings, {frozenset((2 * p + 1, 2 * ((p + 1) % length))) for p in range(length)}


# (family -> the branches, of the kinds the family is about, that its cases reach between them: the CPU test holds
# the model to exactly this list, and each family's docstring ends with it)
FAMILY_BRANCHES = {}
FAMILY_TRACKED = {}


def family(tracked, reached):
    def wrap(fn):
        name = fn.__name__
        FAMILY_TRACKED[name] = re.compile(tracked)
        FAMILY_BRANCHES[name] = frozenset(reached)
        fn.__doc__ += "\n    Branches: " + ", ".join(sorted(reached))
        return fn
    return wrap


ALL = (FAST, SLOW, DIRECTED)
ROUNDS = ["rounds=%d" % r for r in range(1, C.match_first + 2)]


@family(r"rounds=|first_batch|second_batch|third_batch|same_side_edge",
        ROUNDS + ["first_batch_only", "first_batch_full_less_one", "second_batch", "same_side_edge"])
def matching_rounds():
    """Junctions of ends that share one (k-1)-mer.  A K(r, r) whose predecessors all come before its successors
    commits one pair per round: r live rounds, r + 1 reported; r = kMatchFirst - 1 is answered inside the first
    batch, r = kMatchFirst needs the second one.  (No input reaches a third batch: see the module's docstring.)"""
    out = []
    rng = np.random.default_rng(101)
    iso = [rand_seq(rng, K + 2) for _ in range(3)]
    out += presentations("rounds-none", "matching_rounds", K, iso, set(), ALL, expect={"rounds=1", "first_batch_only"})
    for r in range(1, C.match_first + 1):
        s, d = junction(rng, K, "ACGT"[:r], "ACGT"[:r])
        loose = {"rounds=%d" % (r + 1), "second_batch" if r >= C.match_first else "first_batch_only"}
        if r == C.match_first - 1:
            loose.add("first_batch_full_less_one")
        out += presentations("rounds-K%d%d" % (r, r), "matching_rounds", K, s, d, ALL, loose=loose, seed=10 * r,
                             forbid={"third_batch"})
    # the shared (k-1)-mer its own reverse complement: the four ends meet each other, through whichever side
    half = rand_seq(rng, (K - 1) // 2)
    x = half + revcomp_string(half)
    s = [rand_seq(rng, 6) + a + x for a in "AC"] + [x + b + rand_seq(rng, 6) for b in "AC"]
    d = {frozenset((a, b)) for a in (1, 3, 4, 6) for b in (1, 3, 4, 6) if a != b}
    out += presentations("rounds-self-rc", "matching_rounds", K, s, d, (FAST, SLOW), expect={"same_side_edge"}, seed=50)
    # canonical, two-sided: half of either hand stored reverse-complemented (the ends meet as P_j and as rc(S_j))
    s, d = junction(rng, K, "ACGT", "ACGT")
    s2, d2 = arrange(s, d, np.arange(8), [0, 0, 1, 1, 0, 0, 1, 1])
    out += presentations("rounds-two-sided", "matching_rounds", K, s2, d2, (FAST, SLOW), loose={"same_side_edge"},
                         forbid={"third_batch"}, seed=60)
    # many junctions of different depths at once, every junction's predecessors before every successor
    parts = []
    for j in range(240):
        a, b = 1 + j % 4, 1 + (j // 4) % 4
        ins, outs = ("".join(rng.permutation(list("ACGT"))[:m]) for m in (a, b))
        parts.append(junction(rng, K, ins, outs))
    s, d = compose(parts)
    ins = [i for i in range(len(s)) if any(2 * i + 1 in e for e in d)]
    order = ins + [i for i in range(len(s)) if i not in set(ins)]
    s2, d2 = arrange(s, d, order, np.zeros(len(s), dtype=np.int64))
    out += presentations("rounds-many", "matching_rounds", K, s2, d2, ALL, loose={"rounds=%d" % (C.match_first + 1)},
                         seed=70)
    return out


LOOP_LENGTHS = (2, 3, 4, 63, 64, 65, 4096, 10 ** 4 + 1)


@family(r"(directed_)?loop_len=|(directed_)?cut_|lap_flips|loop_spans_blocks|(directed_)?loops(=1|>1)|slow$",
        ["%sloop_len=%d" % (t, n) for t in ("", "directed_") for n in LOOP_LENGTHS + (5, 6, 7)]
        + ["cut_not_smallest", "directed_cut_not_smallest", "lap_flips", "loop_spans_blocks", "slow"]
        + [t + x for t in ("", "directed_") for x in ("loops=1", "loops>1")])
def cover_loops():
    """A cycle of L strings with no branch, for L around the loop cut's block of 64 nodes and far beyond it, the
    loop's smallest node at the first, a middle and the last position of the cycle, all strings forward or a random
    half reverse-complemented (going_right flips along the lap); many loops at once; loops beside open paths and
    isolated strings; every one also under fast = false, which never closes a loop, and the all-forward ones under
    the directed rule.  (The replay's first union makes node 0 of a loop a child: the cut node is never the
    smallest.)"""
    out = []
    rng = np.random.default_rng(202)
    for length in LOOP_LENGTHS:
        k = k_for(length)
        s, d = cycle_pieces(rng, k, length)
        expect = {"loop_len=%d" % length, "loops=1", "cut_not_smallest", "slow"}
        for where, p in (("first", 0), ("middle", length // 2), ("last", length - 1)):
            order = (np.arange(length) + p) % length  # node j is the piece at cycle position j + p: node 0 stands at p
            s2, d2 = arrange(s, d, order, np.zeros(length, dtype=np.int64))
            out.append(Case("loop-%d-%s" % (length, where), "cover_loops", k, s2, ALL, d2,
                            expect | {"directed_loop_len=%d" % length}, {"lap_flips"}))
            flips = rng.integers(0, 2, size=length)
            flips[:2] = (0, 1)
            s3, d3 = arrange(s, d, order, flips)
            out.append(Case("loop-%d-%s-mixed" % (length, where), "cover_loops", k, s3, (FAST, SLOW), d3,
                            expect | {"lap_flips"}))
        s2, d2 = shuffled(s, d, length, False)
        out.append(Case("loop-%d/shuffled" % length, "cover_loops", k, s2, ALL, d2, expect))
        s2, d2 = shuffled(s, d, length + 1, True)
        out.append(Case("loop-%d/shuffled+rc" % length, "cover_loops", k, s2, (FAST, SLOW), d2, expect))
    # 1000 loops of 2 .. 7 strings, interleaved in index order: the scratch cursor hands every loop its own range
    parts = [cycle_pieces(rng, K, 2 + j % 6) for j in range(1000)]
    s, d = compose(parts)
    where = [(p, j) for j, (sj, _) in enumerate(parts) for p in range(len(sj))]
    order = np.array(sorted(range(len(s)), key=lambda i: where[i]))
    s2, d2 = arrange(s, d, order, np.zeros(len(s), dtype=np.int64))
    for c in presentations("loops-1000", "cover_loops", K, s2, d2, ALL, expect={"loops>1", "loop_spans_blocks"},
                           seed=7):
        loops = c.results()[FAST].loops
        assert len(loops) == 1000 and sum(lp.length for lp in loops) == len(s)  # disjoint ranges: all looped nodes
        out.append(c)
    # loops beside open paths and isolated strings
    parts = [cycle_pieces(rng, K, 3 + j) for j in range(5)] + [path_pieces(rng, K, 1 + j) for j in range(5)]
    s, d = compose(parts)
    s2, d2 = shuffled(s, d, 5, False)
    out.append(Case("loops-beside-paths", "cover_loops", K, s2, ALL, d2, {"loops>1", "class0", "class2"}))
    s2, d2 = shuffled(s, d, 6, True)
    out.append(Case("loops-beside-paths+rc", "cover_loops", K, s2, (FAST, SLOW), d2,
                    {"loops>1", "class2", "lap_flips"}))
    return out


def walk_lengths():
    """L with 2 L the largest value below a power of kJumpHops + 1, and the next L, up to the first power above 7e4:
    a path there has about a power of kJumpHops + 1 states in its two directions together."""
    out, p = [], C.jump_hops + 1
    while True:
        out += [(p - 1) // 2, (p - 1) // 2 + 1]
        if p > 7 * 10 ** 4:
            return out
        p *= C.jump_hops + 1


def step_powers():
    """The powers p of kJumpHops + 1 up to the first above 7e4.  The host counts how often x = 2 n_u can be divided
    (rounding down) before it reaches 1 or 0, and 2 p / p = 2 > 1 where (2 p - 2) / p = 1: walk_rounds steps between
    n_u = p - 1 and n_u = p.  The need steps one string later, between L = p and L = p + 1: the first state of a
    path of L strings is L - 1 hops from the last, a record's reach grows (kJumpHops + 1)-fold per launch, p hops
    take one launch more than p - 1."""
    out, p = [], C.jump_hops + 1
    while True:
        out.append(p)
        if p > 7 * 10 ** 4:
            return out
        p *= C.jump_hops + 1


def step_lengths():
    """p - 1 and p for every power (the allowance steps), p + 1 too below 2e4 strings (the need steps)."""
    return [n for p in step_powers() for n in (p - 1, p, p + 1) if n <= p or p < 2 * 10 ** 4]


WALK_SINGLES = sorted(set([1] + walk_lengths() + step_lengths()))
WALK_PAIRS = ((1, 2), (2, 12), (62, 63))
WALK_BESIDE_LOOPS = (2, 63)
WALK_SIZES = WALK_SINGLES + [a + b for a, b in WALK_PAIRS] + [2 * n for n in WALK_BESIDE_LOOPS]


@family(r"walk_need=|walk_allow=", ["walk_need=%d" % walk_need(n) for n in WALK_SINGLES]
        + ["walk_allow=%d" % walk_allowance(n) for n in WALK_SIZES])
def walk_allowance_paths():
    """A single open path of L strings of k + 2 bases: at L = p - 1, p and p + 1 for every power p of kJumpHops + 1
    up to the first above 7e4 -- the host's walk_rounds steps between p - 1 and p strings, the worst-case need between
    p and p + 1 -- and at the L with 2 L just below and just above such a power; each in index order, reversed,
    shuffled, and shuffled with a random half reverse-complemented (beyond 10^4 strings under the fast cover only,
    the index order also directed).  L = 1 and 2; two paths in one input; a path beside a loop of its length.  The
    model shows the allowance to cover the worst schedule for each."""
    out = []
    rng = np.random.default_rng(303)
    for length in WALK_SINGLES:
        k = k_for(length)
        s, d = path_pieces(rng, k, length)
        big = length > 10 ** 4
        expect = {"walk_need=%d" % walk_need(length), "walk_allow=%d" % walk_allowance(length)}
        one = length == 1  # (a single string is isolated: class 2 either way)
        out.append(Case("walk-%d" % length, "walk_allowance_paths", k, s, (FAST, DIRECTED) if big else ALL, d,
                        expect | {"class2" if one else "class0"}, {"class1"}))
        s2, d2 = arrange(s, d, np.arange(length)[::-1], np.zeros(length, dtype=np.int64))
        out.append(Case("walk-%d-reversed" % length, "walk_allowance_paths", k, s2, (FAST,) if big else ALL, d2,
                        expect | {"class2" if one else "class1"}, {"class0"}))
        s2, d2 = shuffled(s, d, length, False)
        out.append(Case("walk-%d/shuffled" % length, "walk_allowance_paths", k, s2, (FAST,) if big else ALL, d2,
                        expect))
        s2, d2 = shuffled(s, d, length + 1, True)
        out.append(Case("walk-%d/shuffled+rc" % length, "walk_allowance_paths", k, s2,
                        (FAST,) if big else (FAST, SLOW), d2, expect))
    for a, b in WALK_PAIRS:
        s, d = compose([path_pieces(rng, K, a), path_pieces(rng, K, b)])
        out += presentations("walk-%d+%d" % (a, b), "walk_allowance_paths", K, s, d, ALL, seed=a,
                             expect={"walk_need=%d" % walk_need(a), "walk_need=%d" % walk_need(b)})
    for length in WALK_BESIDE_LOOPS:
        s, d = compose([path_pieces(rng, K, length), cycle_pieces(rng, K, length)])
        out += presentations("walk-%d-beside-loop" % length, "walk_allowance_paths", K, s, d, ALL, seed=length,
                             expect={"loop_len=%d" % length})
    return out


@family(r"class\d$|skipped_walk|both_|slow_isolated_flipped",
        ["class0", "class1", "class2", "skipped_walk", "both_left_terminals", "both_right_terminals",
         "slow_isolated_flipped"])
def classes_and_order():
    """Strings of class 0 (a kept walk from a left terminal), 1 (from a right terminal) and 2 (isolated) in every
    order of the three by index and interleaved, each class absent in turn, paths whose two terminals are both left
    (both right) terminals so that u <= far_end alone picks the start, isolated strings only, one string; under
    fast = false the strings come in node order and an isolated string is spelled reverse-complemented."""
    out = []
    rng = np.random.default_rng(404)

    def part(kind):
        if kind == 2:
            return path_pieces(rng, K, 1)
        s, d = path_pieces(rng, K, 3)
        if kind == 0:
            return s, d
        if kind == 1:
            return arrange(s, d, [2, 1, 0], [0, 0, 0])
        if kind == "ll":  # the second string reverse-complemented: the two meet right to right, both ends look left
            return arrange(s[:2], {frozenset((1, 2))}, [0, 1], [0, 1])
        return arrange(s[:2], {frozenset((1, 2))}, [0, 1], [1, 0])  # "rr": left to left

    import itertools
    for perm in itertools.permutations((0, 1, 2)):
        s, d = compose([part(kind) for kind in perm for _ in range(2)])
        out.append(Case("classes-%d%d%d" % perm, "classes_and_order", K, s, (FAST, SLOW), d,
                        {"class0", "class1", "class2", "skipped_walk", "slow_isolated_flipped"}))
    s, d = compose([part(kind) for kind in (0, 1, 2, 1, 0, 2, 2, 0, 1)])
    order = np.argsort(np.arange(len(s)) % 4, kind="stable")  # interleaved: the paths' nodes far apart by index
    s2, d2 = arrange(s, d, order, np.zeros(len(s), dtype=np.int64))
    out += presentations("classes-interleaved", "classes_and_order", K, s2, d2, ALL, expect={"class2"},
                         loose={"class0", "class1"}, seed=3)
    for absent in (0, 1, 2):
        kinds = [x for x in (0, 1, 2) if x != absent] * 2
        s, d = compose([part(kind) for kind in kinds])
        out.append(Case("classes-no-%d" % absent, "classes_and_order", K, s, (FAST, SLOW), d,
                        {"class%d" % x for x in kinds}, {"class%d" % absent}))
    s, d = compose([part("ll"), part(2), part("rr"), part("ll"), part("rr")])
    out += presentations("classes-ties", "classes_and_order", K, s, d, (FAST, SLOW), seed=9,
                         expect={"skipped_walk"}, loose={"both_left_terminals", "both_right_terminals"})
    s, d = compose([part(2) for _ in range(3)])
    out += presentations("classes-isolated-only", "classes_and_order", K, s, d, ALL, seed=11, expect={"class2"},
                         forbid={"class1", "skipped_walk"})
    s, d = part(2)
    out.append(Case("classes-one-string", "classes_and_order", K, s, ALL, d, {"class2", "n=1"}, {"class1"}))
    return out


def valid_strings(rng, k, lens, canonical=True, tries=4000):
    """Random strings of the given lengths that meet the preconditions of ksh_spss_cover_plan (as many of them as
    the k-mers of this k allow): pairwise distinct canonical end k-mers, none its own reverse complement, first and
    last of a longer string different; directed: distinct first k-mers, distinct last k-mers."""
    out, used, used_p, used_s = [], set(), set(), set()
    canon = lambda x: min(x, revcomp_string(x))
    for ln in lens:
        for _ in range(tries):
            s = rand_seq(rng, int(ln))
            p, q = s[:k], s[len(s) - k:]
            if canonical:
                if p == revcomp_string(p) or q == revcomp_string(q) or canon(p) in used or canon(q) in used:
                    continue
                if ln > k and canon(p) == canon(q):
                    continue
                used |= {canon(p), canon(q)}
            else:
                if p in used_p or q in used_s:
                    continue
                used_p.add(p)
                used_s.add(q)
            out.append(s)
            break
    return out


PHASE_KS = (2, 3, 16, 17, 31)
PHASES = ["%s_phase=%d" % (e, p) for e in ("first", "last") for p in range(32)]


@family(r"(first|last)_(phase=|crosses_word|in_final_word)|stream_ends|final_word_partial|last_ends_at_word_end|"
        r"run_|n=|cap=|table_wrap",
        PHASES + ["first_crosses_word", "last_crosses_word", "first_in_final_word", "last_in_final_word",
                  "stream_ends_at_word_end", "final_word_partial", "last_ends_at_word_end", "table_wrap",
                  "run_spans=1", "run_spans=2", "run_spans=3", "run_crosses_in_flipped", "run_in_flipped",
                  "run_in_overlap", "run_part_overlap"]
        + ["n=%d" % n for n in range(1, 6)] + ["cap=%d" % c for c in (4, 8, 16, 32)])
def cover_kernels():
    """The four kernels of ksh_cover.hip.  For k in {2, 3, 16, 17, 31}: strings whose first and whose last k-mer
    start at every phase 0 .. 31 of a word, the last k-mer ending exactly at a word end or in the stream's final,
    partly filled word; K-long strings only (a run of kCoverEmitRun bases spans three strings at k = 2); every
    length K .. K + 2 kCoverEmitRun in one input; n = 1 .. 5 strings (tables of 4 .. 32 slots); and one input whose
    end k-mers make a probe sequence wrap past the table's last slot.  (The phase cases come as built only: the order
    and the lengths of their three strings are what puts the k-mers at their phases.)"""
    out = []
    rng = np.random.default_rng(505)
    for k in PHASE_KS:
        for phi in range(32):
            psi = (5 * phi + k) % 32
            l0 = phi if phi >= k else phi + 32
            l1 = k + (psi - phi) % 32
            rest = (-(l0 + l1 + k)) % 32
            l2 = (k + rest, k + rest + 5, k)[phi % 3]
            s = valid_strings(rng, k, [l0, l1, l2])
            assert len(s) == 3
            expect = {"first_phase=%d" % phi, "last_phase=%d" % psi}
            expect.add(("stream_ends_at_word_end", "final_word_partial")[phi % 3 == 1] if phi % 3 < 2 else "n=3")
            out.append(Case("phase-k%d-%d" % (k, phi), "cover_kernels", k, s, ALL, None, expect))
    for k, n in ((2, 6), (3, 20)):
        s = valid_strings(rng, k, [k] * n)
        assert len(s) == n
        out += presentations("klong-k%d" % k, "cover_kernels", k, s, None, ALL, expect={"run_spans=2"}, seed=k)
    s = valid_strings(rng, 2, [2] * 16, canonical=False)
    assert len(s) == 16
    out.append(Case("klong-k2-directed", "cover_kernels", 2, s, (DIRECTED,), None, {"run_spans=2"}))
    s = valid_strings(rng, 2, [5, 2, 2])  # a K-long string at an odd offset: one run of four bases meets three strings
    assert len(s) == 3
    out += presentations("run-of-three-k2", "cover_kernels", 2, s, None, ALL, loose={"run_spans=3"}, seed=2)
    for k in (3, 16, 17, 31):
        s = valid_strings(rng, k, [k + j for j in range(2 * C.emit_run + 1)])
        assert len(s) == 2 * C.emit_run + 1
        out += presentations("lengths-k%d" % k, "cover_kernels", k, s, None, ALL, seed=k)
    for n in range(1, 6):
        s, d = path_pieces(rng, K, n)
        out += presentations("n-%d" % n, "cover_kernels", K, s, d, ALL, seed=n,
                             expect={"n=%d" % n, "cap=%d" % table_cap(n)})
    # a probe sequence that wraps: two end k-mers whose home is the table's last slot
    n = 3000
    cap = table_cap(n)
    homes = []
    while len(homes) < 2:
        e = rand_seq(rng, K)
        x = np.array([kmer_of(min(e, revcomp_string(e)))], dtype=U)
        if int(hash_key(x)[0]) & (cap - 1) == cap - 1:
            homes.append(e)
    s, d = compose([path_pieces(rng, K, 1) for _ in range(n - 2)])
    s = [homes[0] + rand_seq(rng, 2)] + s[:n // 2] + [homes[1] + rand_seq(rng, 2)] + s[n // 2:]
    out += presentations("table-wrap", "cover_kernels", K, s, set(), ALL, seed=8, expect={"table_wrap"}, wraps=True)
    return out


@family(r"slow$", ["slow"])
def dense_fuzz():
    """k in {2, 3, 4, 5}: seeded random string lists that meet the preconditions (canonical without
    self-complementary ends; directed), most of them far from any set's unitigs -- the contract allows that."""
    out = []
    rng = np.random.default_rng(606)
    for k, n_max in ((2, 3), (3, 14), (4, 40), (5, 120)):
        for t in range(50):
            n = int(rng.integers(1, n_max + 1))
            s = valid_strings(rng, k, k + rng.integers(0, 7, size=n) * rng.integers(0, 2, size=n), tries=200)
            out.append(Case("fuzz-k%d-%d" % (k, t), "dense_fuzz", k, s, ALL, None))
        for t in range(30):
            n = int(rng.integers(1, 3 * n_max + 1))
            s = valid_strings(rng, k, k + rng.integers(0, 7, size=n), canonical=False, tries=200)
            out.append(Case("fuzz-directed-k%d-%d" % (k, t), "dense_fuzz", k, s, (DIRECTED,), None))
    return out


def geom_bits(k):
    """Bucket bits the tests run a k at (the cover does not look at them; the encode and the oracle's set do)."""
    return max(1, min(14, 2 * k - 4))


OWN_MAX_STRINGS = 5000  # (the inputs beyond are single paths and loops cut into pieces: one unitig, not theirs)


def own_unitig_set(case):
    """(the oracle's set of the case's k-mers, the k-mers) if the case's strings are exactly that set's unitigs, up
    to orientation, and the set is one the encode takes (no k-mer its own reverse complement); else None."""
    import oracle_lib as ol
    from kmersets import synth

    k = case.k
    if len(case.strings) > OWN_MAX_STRINGS:
        return None
    kmers = np.unique(np.concatenate([synth.canonical_set_of_bases(synth.bases_of_string(s), k) for s in case.strings]))
    if (kmers == revcomp_bits(kmers, k)).any():
        return None
    key_bits = 2 * k - geom_bits(k)
    oset = ol.Set.from_kmers(k, geom_bits(k), 2 if key_bits <= 16 else (4 if key_bits <= 32 else 8), kmers)
    canon = lambda s: min(s, revcomp_string(s))
    same = sorted(canon(s) for s in oset.unitigs()) == sorted(canon(s) for s in case.strings)
    return (oset, kmers) if same else None


# the families some of whose cases are the unitigs of their own k-mer set (cover_loops: a loop's pieces never are)
ENCODED = ("matching_rounds", "walk_allowance_paths", "classes_and_order", "cover_kernels", "dense_fuzz")
FAMILIES = (matching_rounds, cover_loops, walk_allowance_paths, classes_and_order, cover_kernels, dense_fuzz)
_cases = {}


def cases(name):
    """The cases of one family, built once."""
    if name not in _cases:
        fn = {f.__name__: f for f in FAMILIES}[name]
        _cases[name] = fn()
        names = [c.name for c in _cases[name]]
        assert len(set(names)) == len(names)
    return _cases[name]


def tracked_branches(name):
    """The branches, of the kinds the family is about, that its cases reach between them."""
    seen = set()
    for c in cases(name):
        seen |= {b for b in c.branches() if FAMILY_TRACKED[name].match(b)}
    return seen


# ---- refusals --------------------------------------------------------------------------------------------------------
BASES, PALINDROME, SAME_ENDS = "bases", "palindrome", "same_ends"
DUP_END, DUP_FIRST, DUP_LAST = "dup_end", "dup_first", "dup_last"
HOST_ORDER = {True: (BASES, PALINDROME, SAME_ENDS, DUP_END), False: (BASES, DUP_FIRST, DUP_LAST)}
MESSAGE = {BASES: "add up", PALINDROME: "own reverse complement", SAME_ENDS: "longer than K",
           DUP_END: "another string too", DUP_FIRST: "repeated first k-mer", DUP_LAST: "repeated last k-mer"}
REFUSAL_K = 6


def violations(strings, k, canonical):
    """Which strings break which precondition, as k_cover_ends meets them: a string with a palindromic end or with
    equal ends enters no table; a repeated k-mer counts for every string that shares it."""
    out = {}
    canon = lambda x: min(x, revcomp_string(x))
    keys = {}
    for i, s in enumerate(strings):
        p, q = s[:k], s[len(s) - k:]
        if not canonical:
            keys.setdefault((DUP_FIRST, p), []).append(i)
            keys.setdefault((DUP_LAST, q), []).append(i)
        elif p == revcomp_string(p) or q == revcomp_string(q):
            out.setdefault(PALINDROME, set()).add(i)
        elif canon(p) == canon(q) and len(s) > k:
            out.setdefault(SAME_ENDS, set()).add(i)
        else:
            for e in {canon(p), canon(q)}:
                keys.setdefault((DUP_END, e), []).append(i)
    for (kind, _), who in keys.items():
        if len(who) > 1:
            out.setdefault(kind, set()).update(who)
    return out


Refusal = namedtuple("Refusal", "name strings canonical bases_off kind named")


def refusal_inputs():
    """(good strings, refusals): inputs of 14 strings at k = 6 with several violations of one kind (at strings 3, 7
    and 11) or of several kinds; `kind` is what the host's order reports, `named` the strings the message may name:
    the smallest index for a fault a string commits alone, any of the strings that share a repeated k-mer (which of
    them loses the table's atomicCAS is a race)."""
    k = REFUSAL_K
    good = valid_strings(np.random.default_rng(77), k, [k + 2] * 14)

    def planted(at):
        s = list(good)
        for i, x in at.items():
            s[i] = x
        return s

    w = ["ACCGAT", "GGATAC", "CTTAGA"]
    e = "CAGGTA"
    pal = {3: "ACGCGTAA", 7: "TTGAATTC", 11: "AAGCTTCC"}
    same = {3: w[0] + w[0], 7: w[1] + revcomp_string(w[1]), 11: w[2] + w[2]}
    dup = {3: e + "AC", 7: e + "TG", 11: "GA" + revcomp_string(e)}
    out = [Refusal("palindromes", planted(pal), True, 0, PALINDROME, {3}),
           Refusal("same-ends", planted(same), True, 0, SAME_ENDS, {3}),
           Refusal("dup-ends", planted(dup), True, 0, DUP_END, {3, 7, 11}),
           Refusal("dup-firsts", planted({3: e + "AC", 7: e + "TG", 11: e + "CA"}), False, 0, DUP_FIRST, {3, 7, 11}),
           Refusal("dup-lasts", planted({3: "AC" + e, 7: "TG" + e, 11: "CA" + e}), False, 0, DUP_LAST, {3, 7, 11})]
    every = {2: same[3], 5: pal[3], 8: dup[3], 9: dup[7]}
    out += [Refusal("all-kinds-bases-%+d" % off, planted(every), True, off, BASES, None) for off in (-1, 1)]
    out.append(Refusal("all-kinds", planted(every), True, 0, PALINDROME, {5}))
    del every[5]
    out.append(Refusal("same-ends+dup", planted(every), True, 0, SAME_ENDS, {2}))
    del every[2]
    out.append(Refusal("dup-alone", planted(every), True, 0, DUP_END, {8, 9}))
    both = {1: e + "AC", 4: e + "TG", 6: "AC" + w[0], 10: "TG" + w[0]}
    out.append(Refusal("directed-first+last", planted(both), False, 0, DUP_FIRST, {1, 4}))
    del both[4]
    out.append(Refusal("directed-last", planted(both), False, 0, DUP_LAST, {6, 10}))
    out += [Refusal("bases-%+d-%s" % (off, c), good, c, off, BASES, None) for off in (-1, 1) for c in (True, False)]
    return good, out

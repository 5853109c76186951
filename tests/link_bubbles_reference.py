"""The host reference of ksh_link_bubbles (capi.Context.link_bubbles), shared by test_link_bubbles_reference_cpu.py,
test_gpu_link_bubbles.py and test_gpu_colored_bubbles.py: the definition of include/kmersets_hip.h in plain Python
over the CSR arrays.

The graph has n strings and 2 n oriented strings v = 2 s + o; out(v) is the row of v, outdeg(v) its length and
indeg(v) := outdeg(v ^ 1).  The walk of arm i (i = 0, 1, in row order) from a source v with outdeg(v) == 2:

    x = out(v)[i]; arm = []
    loop:
      if indeg(x) != 1 or outdeg(x) != 1 or len(arm) == max_arm: the arm fails
      arm.append(x)
      x = out(x)[0]
      if indeg(x) == 2: sink_i = x; stop

(a next x with indeg 1 is met again at the top of the loop, any other indeg makes the arm fail).  v is the source of a
bubble (v, w, arm_0, arm_1) iff both arms succeed and sink_0 == sink_1 =: w; it is reported iff v <= w ^ 1.  The
carriers of an arm are the AND of rows[string_class[x >> 1]] over its strings."""
import numpy as np

MAX_ARM = 64  # KSH_BUBBLE_MAX_ARM
_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def csr(n_strings, links, twins=True):
    """(link_offsets int64[2 n + 1], link_to int64[n_links]) of a list of directed links (v, w) between oriented
    strings.  twins: every link's twin (w ^ 1, v ^ 1) is added, so that a case can be drawn as a graph, one
    orientation of it.  A row keeps the order in which its links are first listed (twins behind the link that
    brings them); a link listed twice is kept once."""
    rows = [[] for _ in range(2 * n_strings)]
    for v, w in links:
        for a, b in ((v, w), (w ^ 1, v ^ 1)) if twins else ((v, w),):
            if b not in rows[a]:
                rows[a].append(b)
    off = np.zeros(2 * n_strings + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.array([w for r in rows for w in r], dtype=np.int64)


def check_graph(off, to, string_class=None, n_classes=None):
    """What the call refuses on the device, as ValueError with the device's words: each kind names its smallest
    offending vertex or link, the offsets' offences first."""
    off, to = [int(x) for x in off], [int(x) for x in to]
    m, n_links = len(off) - 1, len(to)
    assert m >= 0 and m % 2 == 0
    if off[0] != 0:
        raise ValueError("d_link_offsets[0] is not 0")
    if off[m] != n_links:
        raise ValueError("d_link_offsets[2 n] is not n_links = %d" % n_links)
    for v in range(m):
        if off[v] > off[v + 1]:
            raise ValueError("descends behind vertex %d" % v)
    for v in range(m):
        if off[v + 1] - off[v] > 4:
            raise ValueError("the row of vertex %d has more than four links" % v)
    for e, w in enumerate(to):
        if not 0 <= w < m:
            raise ValueError("the target of link %d is outside" % e)
    for v in range(m):
        row = to[off[v]:off[v + 1]]
        if len(set(row)) != len(row):
            raise ValueError("the row of vertex %d repeats a target" % v)
    for v in range(m):
        for e in range(off[v], off[v + 1]):
            w = to[e] ^ 1
            if v ^ 1 not in to[off[w]:off[w + 1]]:
                raise ValueError("link %d (v -> w) has no twin" % e)
    if string_class is not None:
        for s, c in enumerate(string_class):
            if not 0 <= int(c) < n_classes:
                raise ValueError("the class of string %d is outside" % s)


def degrees(off):
    """(outdeg, indeg) of every oriented string, two lists."""
    out = [int(off[v + 1] - off[v]) for v in range(len(off) - 1)]
    return out, [out[v ^ 1] for v in range(len(out))]


def walk(off, to, outdeg, indeg, x, max_arm):
    """(arm, sink) of the arm that begins with x, or None if it fails."""
    arm = []
    while True:
        if indeg[x] != 1 or outdeg[x] != 1 or len(arm) == max_arm:
            return None
        arm.append(x)
        x = int(to[off[x]])
        if indeg[x] == 2:
            return arm, x
        if indeg[x] != 1:
            return None


def all_bubbles(off, to, max_arm):
    """Every bubble, both twins: a list of (v, w, arm_0, arm_1) ascending by v."""
    assert max_arm >= 1
    outdeg, indeg = degrees(off)
    found = []
    for v in range(len(outdeg)):
        if outdeg[v] != 2:
            continue
        arms = [walk(off, to, outdeg, indeg, int(to[off[v] + i]), max_arm) for i in (0, 1)]
        if arms[0] is None or arms[1] is None or arms[0][1] != arms[1][1]:
            continue
        found.append((v, arms[0][1], arms[0][0], arms[1][0]))
    return found


def twin_of(bubble):
    v, w, a0, a1 = bubble
    return w ^ 1, v ^ 1, [x ^ 1 for x in reversed(a0)], [x ^ 1 for x in reversed(a1)]


def bubbles(off, to, max_arm, string_class=None, rows=None, limit=MAX_ARM):
    """(ends int64[nb, 2], arm_offsets int64[2 nb + 1], arm_strings int64[...], arm_rows uint64[2 nb, 2] or None) of a
    graph that check_graph accepts: the four outputs of the call.  max_arm is in [1, limit], as the call asks (a test
    that looks one string beyond an arm of MAX_ARM raises the limit)."""
    assert (string_class is None) == (rows is None) and 1 <= max_arm <= limit
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    check_graph(off, to, string_class, None if rows is None else len(rows))
    ends, arm_off, arm, arm_rows = [], [0], [], []
    for v, w, a0, a1 in all_bubbles(off, to, max_arm):
        if v > w ^ 1:
            continue
        ends.append((v, w))
        for a in (a0, a1):
            arm += a
            arm_off.append(len(arm))
            if rows is not None:
                r = np.array([~np.uint64(0), ~np.uint64(0)])
                for x in a:
                    r = r & rows[int(string_class[x >> 1])]
                arm_rows.append(r)
    return (np.array(ends, dtype=np.int64).reshape(-1, 2), np.array(arm_off, dtype=np.int64),
            np.array(arm, dtype=np.int64),
            None if rows is None else np.array(arm_rows, dtype=np.uint64).reshape(-1, 2))


def oriented(strings, v):
    s = strings[v >> 1]
    return rc(s) if v & 1 else s


def spell(strings, k, arm):
    """The oriented strings of `arm` joined on their K - 1 overlaps (which are asserted)."""
    text = ""
    for x in arm:
        t = oriented(strings, int(x))
        if text:
            assert text[-(k - 1):] == t[:k - 1], (text, t)
            t = t[k - 1:]
        text += t
    return text


def carriers(row, n_cols=128):
    """The column positions whose bit is set in one arm row (two uint64 words)."""
    bits = int(row[0]) | int(row[1]) << 64
    return [c for c in range(n_cols) if bits >> c & 1]


def parse_bubble_lines(lines):
    """[(v, w, allele_0, allele_1, carriers_0, carriers_1)] of capi.bubble_lines, the carriers as lists of int."""
    out = []
    for line in lines:
        f = line.split("\t")
        assert len(f) == 6 and "\n" not in line
        sets = [[] if c == "." else [int(x) for x in c.split(",")] for c in f[4:]]
        out.append((int(f[0]), int(f[1]), f[2], f[3], sets[0], sets[1]))
    return out

"""The host reference of ksh_spss_links (capi.Context.spss_links), shared by test_spss_links_reference_cpu.py,
test_gpu_spss_links.py and test_gpu_colored_graph.py: the definition of include/kmersets_hip.h in plain Python on the
strings themselves -- a dict of the oriented first k-mers, then the rows.

The oriented string v = 2 s + o is string s as written (o = 0) or its reverse complement (o = 1).  For each base b of
ACGT let y = last(v)[1:] + b; the base is skipped if canon(y) == canon(last(v)) (canonical) or y == last(v) (not
canonical); otherwise v -> w is a link iff first(w) == y.  Not canonical: only o = 0 exists, rows 2 s + 1 are empty."""
import numpy as np

_COMP = str.maketrans("ACGT", "TGCA")


def rc(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    r = rc(s)
    return s if s <= r else r


def oriented(strings, v):
    s = strings[v >> 1]
    return rc(s) if v & 1 else s


def check_container(strings, k, canonical):
    """What the call refuses on the device, as ValueError naming the smallest offending string: two string ends with
    the same end k-mer (the two ends of a one-k-mer string are one end), in canonical mode after canonicalisation, and
    there an end k-mer that is its own reverse complement."""
    seen, dup, palin = {}, [], []
    for s, t in enumerate(strings):
        assert len(t) >= k and set(t) <= set("ACGT"), (s, t)
        for e in ([t[:k]] if len(t) == k else [t[:k], t[-k:]]):
            if canonical and e == rc(e):
                palin.append(s)
            key = canon(e) if canonical else e
            if key in seen:
                dup.append(min(s, seen[key]))
            seen.setdefault(key, s)
    if palin:
        raise ValueError("palindromic end: string %d" % min(palin))
    if dup:
        raise ValueError("duplicate end: string %d" % min(dup))


def links(strings, k, canonical=True):
    """(link_offsets int64[2 n + 1], link_to int64[n_links]) of a container that check_container accepts."""
    check_container(strings, k, canonical)
    n = len(strings)
    first = {}
    for v in range(2 * n):
        if canonical or not v & 1:
            head = oriented(strings, v)[:k]
            assert head not in first
            first[head] = v
    offsets, to = [0], []
    for v in range(2 * n):
        if canonical or not v & 1:
            last = oriented(strings, v)[-k:]
            for b in "ACGT":
                y = last[1:] + b
                if (canon(y) == canon(last)) if canonical else (y == last):
                    continue
                if y in first:
                    to.append(first[y])
        offsets.append(len(to))
    return np.array(offsets, dtype=np.int64), np.array(to, dtype=np.int64)


def rows(offsets, to):
    """The CSR arrays as a list of lists."""
    return [[int(w) for w in to[offsets[v]:offsets[v + 1]]] for v in range(len(offsets) - 1)]


def twin_symmetric(offsets, to):
    """v -> w iff w ^ 1 -> v ^ 1, with multiplicity."""
    pairs = sorted((v, w) for v, row in enumerate(rows(offsets, to)) for w in row)
    return pairs == sorted((w ^ 1, v ^ 1) for v, w in pairs)


def link_pairs(strings, k, offsets, to):
    """The directed k-mer pairs (last(v), first(w)) of the links, a list."""
    return [(oriented(strings, v)[-k:], oriented(strings, w)[:k])
            for v, row in enumerate(rows(offsets, to)) for w in row]


def inner_pairs(strings, k, canonical):
    """The consecutive k-mer pairs inside the oriented strings, a list."""
    out = []
    for v in range(2 * len(strings)):
        if canonical or not v & 1:
            t = oriented(strings, v)
            out += [(t[i:i + k], t[i + 1:i + 1 + k]) for i in range(len(t) - k)]
    return out


def graph_edges(kmers, k, canonical):
    """Brute force: the edges x -> y, y = x[1:] + b, canon(x) != canon(y), of the node-centric de Bruijn graph of a
    k-mer set given as strings (canonical: either orientation of a member is a node; not: the members as given)."""
    nodes = set(kmers)
    if canonical:
        nodes |= {rc(x) for x in kmers}
    out = set()
    for x in nodes:
        for b in "ACGT":
            y = x[1:] + b
            if y in nodes and ((canon(x) != canon(y)) if canonical else (x != y)):
                out.add((x, y))
    return out


def kmers_of(strings, k):
    return [t[i:i + k] for t in strings for i in range(len(t) - k + 1)]


def parse_gfa(lines):
    """(segments {name: (sequence, class or None)}, links [(a, '+'|'-', b, '+'|'-', overlap)]) of GFA 1 lines."""
    assert lines[0] == "H\tVN:Z:1.0"
    segments, out = {}, []
    for line in lines[1:]:
        f = line.split("\t")
        if f[0] == "S":
            assert f[1] not in segments and len(f) in (3, 4)
            cls = None
            if len(f) == 4:
                assert f[3].startswith("CL:i:")
                cls = int(f[3][5:])
            segments[f[1]] = (f[2], cls)
        else:
            assert f[0] == "L" and len(f) == 6 and f[2] in "+-" and f[4] in "+-"
            out.append((f[1], f[2], f[3], f[4], f[5]))
    return segments, out


def gfa_links_verify(lines, k):
    """Every L line textually: the last K - 1 bases of the oriented source are the first K - 1 of the oriented target,
    and the overlap field is (K-1)M.  Returns the links as (v, w) pairs."""
    segments, ls = parse_gfa(lines)
    pairs = []
    for a, oa, b, ob, overlap in ls:
        assert overlap == "%dM" % (k - 1)
        x, y = segments[a][0], segments[b][0]
        x = rc(x) if oa == "-" else x
        y = rc(y) if ob == "-" else y
        assert x[-(k - 1):] == y[:k - 1], (a, oa, b, ob)
        pairs.append((2 * int(a) + (oa == "-"), 2 * int(b) + (ob == "-")))
    return pairs

"""ksh_seq_locate in plain Python (include/kmersets_hip.h, "Where the string ends of one container occur in another").

End e = 2 s is the first k-mer of string s as written, e = 2 s + 1 its last.  The reference's k-mer positions are
numbered in one line, sequence after sequence; a position with k-mer x matches the end k-mer y when x == y (strand 0)
or, in canonical mode only, x == rc(y) (strand 1); a k-mer that is its own reverse complement reads strand 0.
count[e] is the number of matching positions, where[e] = (g << 1) | strand of the one with the smallest global index
g, -1 if there is none.  A dict over the reference's positions; brute() is the same by comparing all pairs."""
import numpy as np

_COMPLEMENT = str.maketrans("ACGT", "TGCA")
UINT32_MAX = 0xFFFFFFFF


def rc(s):
    return s.translate(_COMPLEMENT)[::-1]


def pstart(reference, k):
    """The first global position of every reference sequence, and the number of positions behind them."""
    return np.concatenate([[0], np.cumsum([len(t) - k + 1 for t in reference])]).astype(np.int64)


def end_kmers(strings, k):
    """The 2 n end k-mers as written."""
    out = []
    for t in strings:
        out += [t[:k], t[-k:]]
    return out


def positions(reference, k):
    """{k-mer: [global positions, ascending]} of the reference."""
    at, g = {}, 0
    for t in reference:
        for p in range(len(t) - k + 1):
            at.setdefault(t[p:p + k], []).append(g)
            g += 1
    return at


def locate(strings, reference, k, canonical):
    """(where int64[2 n], count uint32[2 n])."""
    for t in list(strings) + list(reference):
        assert len(t) >= k and set(t) <= set("ACGT")
    at = positions(reference, k)
    where, count = [], []
    for y in end_kmers(strings, k):
        hits = [(g << 1) | 0 for g in at.get(y, ())]
        if canonical and rc(y) != y:
            hits += [(g << 1) | 1 for g in at.get(rc(y), ())]
        where.append(min(hits) if hits else -1)
        count.append(len(hits))
    return np.array(where, dtype=np.int64).reshape(-1), np.array(count, dtype=np.uint32).reshape(-1)


def brute(strings, reference, k, canonical):
    """The same by comparing every end with every window of every sequence."""
    where, count = [], []
    for y in end_kmers(strings, k):
        best, c, g = -1, 0, 0
        for t in reference:
            for p in range(len(t) - k + 1):
                x = t[p:p + k]
                strand = 0 if x == y else 1 if canonical and x == rc(y) else None
                if strand is not None:
                    c += 1
                    if best < 0:
                        best = (g << 1) | strand
                g += 1
        where.append(best)
        count.append(c)
    return np.array(where, dtype=np.int64).reshape(-1), np.array(count, dtype=np.uint32).reshape(-1)


def split(where, reference, k):
    """(sequence, position, strand) per end, (-1, -1, -1) for an end that is nowhere."""
    ps = pstart(reference, k)
    out = []
    for w in where:
        if w < 0:
            out.append((-1, -1, -1))
        else:
            g = int(w) >> 1
            r = int(np.searchsorted(ps, g, side="right")) - 1
            out.append((r, g - int(ps[r]), int(w) & 1))
    return out


def check_container(name, lens, n_bases, k):
    """What the device refuses of one container given as its lens (len - K per string) and its n_bases, in the
    device's order: the first string with lens == UINT32_MAX, then sum(lens + K) != n_bases.  Raises ValueError with
    the words of the library's message."""
    lens = np.asarray(lens, dtype=np.uint64)
    big = np.flatnonzero(lens == UINT32_MAX)
    if big.size:
        raise ValueError("%s: lens[%d] = UINT32_MAX" % (name, big[0]))
    total = int(lens.sum()) + k * int(lens.size)
    if total != int(n_bases):
        raise ValueError("%s: sum(lens + K) = %d but n_bases = %d" % (name, total, n_bases))


def check_request(strings_lens, strings_bases, reference_lens, reference_bases, k):
    """The size refusals of a call with strings in their order: a reference of no sequences that claims bases (on the
    host), then on the device the strings first and the reference second."""
    if not len(reference_lens) and reference_bases != 0:
        raise ValueError("req->reference: sum(lens + K) = 0 but n_bases = %d" % reference_bases)
    check_container("req->strings", strings_lens, strings_bases, k)
    if len(reference_lens):
        check_container("req->reference", reference_lens, reference_bases, k)

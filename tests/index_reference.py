"""One numpy reference for the seven calls that read a KssIndex (query, seq_hits, pair_counts, select / spectrum,
color_classes, select_class_ids and -- through tests/paint_reference.py, which takes an IndexReference -- class_runs),
shared by test_index_reference_cpu.py and test_gpu_index_geometry.py.

Everything derives from the membership matrix M of a structure: one row per distinct k-mer of all node sets, one
column per node, M[q, i] = q in Get(i), where Get(i) is the union of the sets of the nodes reachable from i (i
included).  The matrix does not depend on the bucket geometry; only select's bucket offsets do."""
import numpy as np

from kmersets import synth

U = np.uint64


def reachable(children):
    """bool[n, n]: element [i, j] is True iff node j is reachable from node i (i itself included)."""
    n = len(children)
    reach = np.eye(n, dtype=bool)
    changed = True
    while changed:  # (a handful of nodes: the plain fixpoint, whatever the order of the ids)
        changed = False
        for i in range(n):
            for c in children[i]:
                new = reach[i] | reach[c]
                if not np.array_equal(new, reach[i]):
                    reach[i] = new
                    changed = True
    return reach


def pack_rows(bits):
    """bool[n, n_cols <= 128] -> uint64[n, 2], bit a % 64 of word a // 64 = column a."""
    wide = np.zeros((bits.shape[0], 128), dtype=bool)
    wide[:, :bits.shape[1]] = bits
    return np.packbits(wide, axis=1, bitorder="little").view(U).reshape(-1, 2)


def revcomp_string(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


class IndexReference:
    """k, the node sets (sorted unique uint64 arrays) and the children lists of a structure."""

    def __init__(self, k, node_sets, children):
        self.k = k
        self.n_nodes = len(node_sets)
        node_sets = [np.asarray(s, dtype=U) for s in node_sets]
        for s in node_sets:
            assert s.size < 2 or (s[1:] > s[:-1]).all(), "node sets are sorted and unique"
        self.kmers = np.unique(np.concatenate([np.zeros(0, dtype=U)] + node_sets))
        own = np.stack([np.isin(self.kmers, s, assume_unique=True) for s in node_sets], axis=1) \
            if self.n_nodes else np.zeros((self.kmers.size, 0), dtype=bool)
        reach = reachable(children)
        # M[q, i] = OR over the nodes j reachable from i of own[q, j]
        self.M = (own.astype(np.int64) @ reach.T.astype(np.int64)) > 0
        self.n_distinct = int(self.kmers.size)
        self._classes = {}  # column list -> color_classes of it

    # ---- query -------------------------------------------------------------------------------------------------
    def query_rows(self, patterns, canonicalize):
        """bool[n, n_nodes]: M's row of every pattern; zero for an absent k-mer and for a pattern with bits at or
        above 2K (checked before canonicalising)."""
        z = np.asarray(patterns, dtype=U)
        valid = (z >> U(2 * self.k)) == 0
        z = np.where(valid, z, U(0))
        if canonicalize:
            z = synth.canonical(z, self.k)
        rows = np.zeros((z.size, self.n_nodes), dtype=bool)
        if self.kmers.size:
            at = np.minimum(np.searchsorted(self.kmers, z), self.kmers.size - 1)
            hit = valid & (self.kmers[at] == z)
            rows[hit] = self.M[at[hit]]
        return rows

    # ---- seq_hits ----------------------------------------------------------------------------------------------
    def seq_hits(self, strings, canonicalize):
        """uint32[n_strings, n_nodes]: per string the k-mer positions whose k-mer is in Get(i).  Positions are
        counted, not distinct k-mers; no window crosses from one string into the next."""
        k = self.k
        hits = np.zeros((len(strings), self.n_nodes), dtype=np.uint32)
        if not strings:
            return hits
        x = synth.kmers_of_bases(synth.bases_of_string("".join(strings)), k)
        ends = np.cumsum([len(s) for s in strings])
        start = np.arange(x.size, dtype=np.int64)
        sid = np.searchsorted(ends, start, side="right")
        inside = sid == np.searchsorted(ends, start + k - 1, side="right")
        rows = self.query_rows(x[inside], canonicalize)
        for i in range(self.n_nodes):
            hits[:, i] = np.bincount(sid[inside], weights=rows[:, i], minlength=len(strings)).astype(np.uint32)
        return hits

    # ---- pair_counts -------------------------------------------------------------------------------------------
    def cols_of(self, cols):
        return list(range(self.n_nodes)) if cols is None else [int(c) for c in cols]

    def pair_table(self, cols=None):
        """int64[n_cols, n_cols]: |Get(cols[a]) & Get(cols[b])|."""
        m = self.M[:, self.cols_of(cols)].astype(np.int64)
        return m.T @ m

    # ---- select / spectrum -------------------------------------------------------------------------------------
    def select(self, cols=None, min_count=1, max_count=None, require=(), exclude=()):
        """The selected k-mers, ascending: min_count <= c(q) <= max_count over cols, in Get(r) for every r of
        require and in no Get(x) of exclude."""
        cols = self.cols_of(cols)
        c = self.M[:, cols].sum(axis=1)
        keep = (c >= min_count) & (c <= (len(cols) if max_count is None else max_count))
        for r in require:
            keep &= self.M[:, r]
        for x in exclude:
            keep &= ~self.M[:, x]
        return self.kmers[keep]

    def bucketed(self, kmers, n_bits, key_bytes):
        """(offsets int64[2^N + 1], keys) of ascending k-mers at a geometry, from np.bincount of kmer >> key bits."""
        key_bits = 2 * self.k - n_bits
        counts = np.bincount((kmers >> U(key_bits)).astype(np.int64), minlength=1 << n_bits)
        offsets = np.zeros((1 << n_bits) + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        keys = (kmers & U((1 << key_bits) - 1)).astype({2: np.uint16, 4: np.uint32, 8: np.uint64}[key_bytes])
        return offsets, keys

    def spectrum(self, cols=None):
        """int64[n_cols + 1]: element m = the distinct k-mers of the structure that m of the columns hold."""
        cols = self.cols_of(cols)
        return np.bincount(self.M[:, cols].sum(axis=1), minlength=len(cols) + 1).astype(np.int64)

    # ---- color_classes -----------------------------------------------------------------------------------------
    def color_classes(self, cols=None):
        """(rows uint64[n, 2], counts int64[n]): np.unique of the packed 128-bit rows, ascending by (high, low).
        Computed once per column list and shared: read-only arrays."""
        key = tuple(self.cols_of(cols))
        if key not in self._classes:
            rows = pack_rows(self.M[:, list(key)])
            if rows.shape[0] == 0:
                u, counts = np.zeros((0, 2), dtype=U), np.zeros(0, dtype=np.int64)
            else:
                u, counts = np.unique(rows, axis=0, return_counts=True)
                order = np.lexsort((u[:, 0], u[:, 1]))
                u, counts = u[order], counts[order].astype(np.int64)
            u.flags.writeable = counts.flags.writeable = False
            self._classes[key] = (u, counts)
        return self._classes[key]

    # ---- select_class_ids --------------------------------------------------------------------------------------
    def class_ids(self, rows, cols=None, min_count=1, max_count=None, require=(), exclude=()):
        """(kmers, ids int64): the selected k-mers, ascending, as select() gives them, and for each the position in
        `rows` of its row over cols (pack_rows(M[:, cols])), -1 where `rows` does not hold it.  rows: uint64[n, 2],
        ascending by (high, low) -- color_classes(cols)[0] or an ascending subset of it."""
        rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, 2)
        kmers = self.select(cols, min_count, max_count, require, exclude)
        mine = pack_rows(self.M[np.searchsorted(self.kmers, kmers)][:, self.cols_of(cols)])
        ids = np.full(kmers.size, -1, dtype=np.int64)
        for c in range(rows.shape[0]):  # (a handful of rows; a row is in the table once, so no id is written twice)
            ids[(mine[:, 0] == rows[c, 0]) & (mine[:, 1] == rows[c, 1])] = c
        return kmers, ids


def class_matrix(rows, n_cols):
    """bool[n, n_cols] of packed rows."""
    rows = np.ascontiguousarray(rows, dtype=U).reshape(-1, 2)
    bits = np.unpackbits(rows.view(np.uint8).reshape(rows.shape[0], 16), axis=1, bitorder="little")
    return bits[:, :n_cols].astype(bool)

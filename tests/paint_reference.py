"""The numpy reference of ksh_seq_class_runs (capi.KssIndex.class_runs), shared by test_paint_reference_cpu.py,
test_gpu_paint.py and tools that check a painting: per string the k-mers of its positions, their rows from the
membership matrix of tests/index_reference.py projected onto the columns, their ids from a dict of the table's rows,
and the runs from np.diff of the ids."""
import numpy as np

from index_reference import pack_rows
from kmersets import synth

NONE = -1  # KSH_CLASS_NONE as int32


def with_zero_row(table):
    """The table with the zero row, ascending by (high, low): every position then has a class."""
    t = np.unique(np.concatenate([np.zeros((1, 2), dtype=np.uint64),
                                  np.asarray(table, dtype=np.uint64).reshape(-1, 2)]), axis=0)
    return t[np.lexsort((t[:, 0], t[:, 1]))]


def position_ids(ref, strings, cols, table, canonicalize):
    """Per string the int64 class id of every k-mer position (NONE where the table does not hold the row)."""
    cols = ref.cols_of(cols)
    table = np.ascontiguousarray(table, dtype=np.uint64).reshape(-1, 2)
    at = {(int(r[0]), int(r[1])): c for c, r in enumerate(table)}
    parts = [synth.kmers_of_bases(synth.bases_of_string(s), ref.k) for s in strings]
    assert all(x.size >= 1 for x in parts), "every string is at least K long"
    if not parts:
        return []
    rows = pack_rows(ref.query_rows(np.concatenate(parts), canonicalize)[:, cols])
    distinct, inverse = np.unique(rows, axis=0, return_inverse=True)  # (the dict is asked once per distinct row)
    ids = np.array([at.get((int(r[0]), int(r[1])), NONE) for r in distinct], dtype=np.int64)[inverse.reshape(-1)]
    return np.split(ids, np.cumsum([x.size for x in parts])[:-1])


def runs_of_ids(ids_per_string):
    """(offsets int64[n + 1], start int32[n_runs], cls int32[n_runs]) of per-string id arrays."""
    if not ids_per_string:
        return np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    sizes = np.array([i.size for i in ids_per_string], dtype=np.int64)
    first_of = np.concatenate([[0], np.cumsum(sizes)])  # the first position of every string in one line
    ids = np.concatenate(ids_per_string)
    flag = np.ones(ids.size, dtype=bool)
    flag[1:] = np.diff(ids) != 0
    flag[first_of[:-1]] = True
    at = np.flatnonzero(flag)
    owner = np.searchsorted(first_of, at, side="right") - 1
    offsets = np.searchsorted(at, first_of)  # (every string's first position is flagged)
    return offsets.astype(np.int64), (at - first_of[owner]).astype(np.int32), ids[at].astype(np.int32)


def class_runs(ref, strings, cols, table, canonicalize):
    """-> (offsets, start, cls, n_unmatched) as KssIndex.class_runs returns them (on the host)."""
    ids = position_ids(ref, strings, cols, table, canonicalize)
    offsets, start, cls = runs_of_ids(ids)
    return offsets, start, cls, int(sum(int((i == NONE).sum()) for i in ids))


def expand(offsets, start, cls, lengths):
    """Per string the id of every position, from its runs; lengths[s] = the positions of string s."""
    out = []
    for s, n in enumerate(lengths):
        a, b = int(offsets[s]), int(offsets[s + 1])
        ends = np.concatenate([start[a + 1:b], [n]]).astype(np.int64)
        out.append(np.repeat(cls[a:b].astype(np.int64), ends - start[a:b].astype(np.int64)))
    return out

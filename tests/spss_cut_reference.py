"""The host reference of ksh_spss_cut (capi.Context.spss_cut), shared by test_spss_cut_reference_cpu.py,
test_gpu_spss_cut.py and test_gpu_colored_unitigs.py: Python strings sliced at the runs.  Run r of string s covers
positions start[r] .. e of s (e = the next run's start, or the string's position count), and becomes the string
text[start[r] : e + K - 1]: the K - 1 bases behind a cut are repeated, so the k-mers stay what and where they were."""
import numpy as np


def cut(strings, k, offsets, start):
    """-> (strings_out, lens_out uint32[n_runs], n_bases_out).  offsets int[n + 1], start int[n_runs] as
    KssIndex.class_runs returns them (on the host)."""
    assert len(offsets) == len(strings) + 1 and int(offsets[0]) == 0 and int(offsets[-1]) == len(start)
    out = []
    for s, text in enumerate(strings):
        a, b = int(offsets[s]), int(offsets[s + 1])
        n_pos = len(text) - k + 1
        assert b > a and int(start[a]) == 0 and n_pos >= 1
        ends = [int(x) for x in start[a + 1:b]] + [n_pos]
        for r in range(a, b):
            first, e = int(start[r]), ends[r - a]
            assert first < e <= n_pos
            out.append(text[first:e + k - 1])
    lens_out = np.array([len(x) - k for x in out], dtype=np.int64).astype(np.uint32)
    return out, lens_out, int(sum(len(x) for x in out))


def out_bases(strings, k, offsets, start):
    """(B int64[n_runs + 1], shift int64[n_runs]): output string r begins at output base B[r] (B[n_runs] =
    n_bases_out), and its bases are the input bases at the same index minus shift[r] = (r - s)(K - 1)."""
    sizes = np.array([len(x) - k + 1 for x in strings], dtype=np.int64)
    pstart = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_runs = int(offsets[-1])
    owner = np.searchsorted(offsets, np.arange(n_runs), side="right") - 1
    q = pstart[owner] + np.asarray(start, dtype=np.int64)[:n_runs]
    r = np.arange(n_runs, dtype=np.int64)
    n_out = int(pstart[-1]) + n_runs * (k - 1)
    return np.concatenate([q + r * (k - 1), [n_out]]), (r - owner) * (k - 1)

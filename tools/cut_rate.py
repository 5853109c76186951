"""Cutting the coloured graph of a phylogeny family into coloured unitigs (k = 23, (23, 14, uint32), the family of
tools/paint_rate.py, made as bench.py makes its inputs): the union of the inputs with the class table
(select_classes), its SPSS (spss_encode), the runs of those strings (KssIndex.class_runs), and Context.spss_cut of the
strings at the runs, timed alone: wall clock from a synchronised start to a synchronised end, median of --reps after
one warm-up.  KssIndex.class_runs on the same strings, timed the same way in the same process, is the yardstick: the
cut is the step that follows it.  The bytes the cut moves are the input words, the output words and 12 bytes per run
(a start of 4 bytes read, a place q of 8 bytes written); the rate is those bytes over the wall time, which includes the
call's two synchronisations and its three small kernels.  The sizes of the three forms of the coloured
graph are reported side by side: coloured unitigs (words, lens and 4 bytes of class per string), the run form of
DESIGN.md 3.8g (the uncut strings, 8 bytes per run and an offset per string) and one id per k-mer (3.8f: the uncut
strings and 4 bytes per k-mer).  The tool checks that the cut strings decode to the union and that every string paints
as one run of its own class (the exact comparisons are tests/test_gpu_spss_cut.py and test_gpu_colored_unitigs.py).
Prints one JSON line and a table for DESIGN.md 3.8h, and writes profiles/cut_rate.json.  No rate is a pass condition.

    python tools/cut_rate.py [--sets 8] [--size 1e7] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth_torch  # noqa: E402


def wall_ms(fn, reps):
    fn()  # warm-up: the pool holds the scratch from then on
    times, out = [], None
    for _ in range(reps):
        out = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--size", type=float, default=1e7)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "cut_rate.json"))
    args = ap.parse_args()
    k, nbits = 23, 14
    g = capi.geom(k, nbits)
    ctx = capi.Context(0)
    dev = ctx.device
    kmers = synth_torch.phylogeny_sets(k, args.sets, int(args.size), args.seed, dev)
    compacts = []
    for i, km in enumerate(kmers):
        compacts.append(ctx.spss_encode(synth_torch.device_set(g, km), mode=0))
        kmers[i] = None
    del kmers
    idx = capi.KssIndex.from_nodes(ctx, compacts, [[] for _ in compacts])
    cols = list(range(args.sets))
    union, ids, rows, counts = idx.select_classes(cols)
    spss = ctx.spss_encode(union, mode=0)
    positions = spss.n_bases - spss.n_strings * (k - 1)
    assert positions == union.n_keys

    runs_ms, (off, start, cls, _) = wall_ms(lambda: idx.class_runs(spss, rows, cols, allow_unmatched=False), args.reps)
    n_runs = int(start.numel())
    cut_ms, out = wall_ms(lambda: ctx.spss_cut(spss, off, start), args.reps)
    words_in, words_out = (spss.n_bases + 31) // 32, (out.n_bases + 31) // 32
    moved = 8 * words_in + 8 * words_out + 12 * n_runs
    unitig_bytes = 8 * words_out + 4 * out.n_strings + 4 * out.n_strings
    run_form_bytes = 8 * words_in + 4 * spss.n_strings + 8 * n_runs + 8 * (spss.n_strings + 1)
    per_kmer_bytes = 8 * words_in + 4 * spss.n_strings + 4 * positions
    res = {"tool": "cut_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "classes": int(counts.size), "positions": int(positions), "reps": args.reps,
           "strings_before": spss.n_strings, "bases_before": spss.n_bases, "strings_after": out.n_strings,
           "bases_after": out.n_bases, "runs": n_runs, "cut_wall_ms": round(cut_ms, 3), "bytes_moved": moved,
           "cut_bytes_per_s": round(moved / cut_ms * 1e3), "class_runs_wall_ms": round(runs_ms, 3),
           "cut_over_class_runs": round(cut_ms / runs_ms, 4), "colored_unitig_bytes": unitig_bytes,
           "run_form_bytes": run_form_bytes, "id_per_kmer_bytes": per_kmer_bytes,
           "colored_unitigs_over_run_form": round(unitig_bytes / float(run_form_bytes), 4),
           "colored_unitigs_over_id_per_kmer": round(unitig_bytes / float(per_kmer_bytes), 4),
           "spread_between_runs": "not measured (median of %d)" % args.reps}
    # the cut strings are the union, and every one of them paints as one run of the class its run had
    decoded = ctx.spss_decode(out)
    with torch.cuda.stream(ctx.stream):
        res["same_set"] = bool(decoded.n_keys == union.n_keys and torch.equal(decoded.offsets, union.offsets)
                               and torch.equal(decoded.keys[:union.n_keys * g.key_bytes],
                                               union.keys[:union.n_keys * g.key_bytes]))
    m_off, m_start, m_cls, _ = idx.class_runs(out, rows, cols, allow_unmatched=False)
    with torch.cuda.stream(ctx.stream):
        res["monochromatic"] = bool(m_start.numel() == out.n_strings and not bool(m_start.any())
                                    and torch.equal(m_cls, cls))
    idx.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    print("| strings | bases | runs | cut ms | GB/s moved | class_runs ms | unitig form MB | run form MB | id per k-mer MB |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("| %d -> %d | %d -> %d | %d | %.3f | %.1f | %.3f | %.1f | %.1f | %.1f |"
          % (spss.n_strings, out.n_strings, spss.n_bases, out.n_bases, n_runs, cut_ms, moved / cut_ms / 1e6, runs_ms,
             unitig_bytes / 1e6, run_form_bytes / 1e6, per_kmer_bytes / 1e6))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

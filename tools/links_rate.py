"""The links between the coloured unitigs of a phylogeny family (k = 23, (23, 14, uint32), the family of
tools/cut_rate.py, made as bench.py makes its inputs): the union of the inputs with the class table (select_classes),
its unitigs (spss_encode, mode 1), the runs of those strings (KssIndex.class_runs), the strings cut at the runs
(Context.spss_cut) and Context.spss_links of the cut strings, timed alone: wall clock from a synchronised start to a
synchronised end, median of --reps after one warm-up, the profiler off.  Context.spss_links is two ksh_spss_links calls
(one counts, one fills); the filling call alone is timed as well.  KssIndex.class_runs and Context.spss_cut on the same
unitigs, timed the same way in the same process, are the yardsticks: the links are the step that follows them.

bytes_moved is a count by the design of DESIGN.md 3.8i for ONE ksh_spss_links call that fills, n strings, e end
entries, S table slots, L links: lens 4 n; pstart 16 n (written, scanned in place, read); ends 16 n written and 16 n
read by each of the two row kernels; the table 16 S zeroed, 32 e for the inserts (a slot read and written) and 16 per
look-up of the 8 n candidates of each row kernel that is not skipped (counted as all 8 n); the row counts 16 n written,
scanned in place (32 n) and copied to the caller (32 n); the targets 8 L.  Probes that step past the first slot are
not counted.  The rate is those bytes over the wall time, which includes the call's three synchronisations.

The tool checks twin symmetry of the result on the device (the exact comparisons are tests/test_gpu_spss_links.py and
tests/test_gpu_colored_graph.py).  Prints one JSON line and a table for DESIGN.md 3.8i, and writes
profiles/links_rate.json.  No rate is a pass condition.

    python tools/links_rate.py [--sets 8] [--size 1e7] [--reps 3]
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
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "links_rate.json"))
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
    unitigs = ctx.spss_encode(union, mode=1)
    positions = unitigs.n_bases - unitigs.n_strings * (k - 1)
    assert positions == union.n_keys

    runs_ms, (r_off, r_start, r_cls, _) = wall_ms(
        lambda: idx.class_runs(unitigs, rows, cols, allow_unmatched=False), args.reps)
    cut_ms, cu = wall_ms(lambda: ctx.spss_cut(unitigs, r_off, r_start), args.reps)
    links_ms, (off, to) = wall_ms(lambda: ctx.spss_links(cu, canonical=True), args.reps)
    n, n_links = cu.n_strings, int(to.numel())
    with torch.cuda.stream(ctx.stream):
        f_off = torch.empty_like(off)
        f_to = torch.empty(max(n_links, 1), dtype=torch.int64, device=dev)
    fill_ms, (rc, got) = wall_ms(lambda: ctx.spss_links_raw(cu, True, n_links, f_off, f_to), args.reps)
    assert rc == capi.KSH_OK and got == n_links
    with torch.cuda.stream(ctx.stream):
        same = bool(torch.equal(f_off, off) and torch.equal(f_to[:n_links], to))
        singles = int((cu.lens[:n] == 0).sum())
        entries = 2 * n - singles
        slots = 1
        while slots < 4 * n:
            slots <<= 1
        # twin symmetry: v -> w iff w ^ 1 -> v ^ 1
        src = torch.repeat_interleave(torch.arange(2 * n, dtype=torch.int64, device=dev), off[1:] - off[:-1])
        fwd = torch.sort(src * (2 * n) + to).values
        back = torch.sort((to ^ 1) * (2 * n) + (src ^ 1)).values
        twins = bool(torch.equal(fwd, back)) and bool((fwd[1:] != fwd[:-1]).all())
        max_row = int((off[1:] - off[:-1]).max()) if n else 0
        mixed = int((r_cls[src >> 1] != r_cls[to >> 1]).sum())
    moved = (4 * n + 16 * n + 16 * n + 2 * 16 * n + 16 * slots + 32 * entries + 2 * 16 * 8 * n + 16 * n + 32 * n
             + 32 * n + 8 * n_links)
    res = {"tool": "links_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "classes": int(counts.size), "positions": int(positions), "reps": args.reps,
           "unitigs": unitigs.n_strings, "strings": n, "one_kmer_strings": singles, "table_slots": slots,
           "links": n_links, "links_per_string": round(n_links / float(max(n, 1)), 4), "max_row": max_row,
           "links_between_classes": mixed,
           "links_wall_ms": round(links_ms, 3), "fill_call_wall_ms": round(fill_ms, 3), "bytes_moved_fill_call": moved,
           "fill_call_bytes_per_s": round(moved / fill_ms * 1e3),
           "spss_cut_wall_ms": round(cut_ms, 3), "class_runs_wall_ms": round(runs_ms, 3),
           "links_over_cut": round(links_ms / cut_ms, 4), "links_over_class_runs": round(links_ms / runs_ms, 4),
           "twin_symmetric": twins, "fill_call_equals_wrapper": same,
           "spread_between_runs": "not measured (median of %d)" % args.reps}
    assert twins and same and max_row <= 4
    idx.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    print("| strings | links | links / string | spss_links ms | fill call ms | GB/s moved (fill call) | spss_cut ms | "
          "class_runs ms |")
    print("|---|---|---|---|---|---|---|---|")
    print("| %d | %d | %.3f | %.3f | %.3f | %.1f | %.3f | %.3f |"
          % (n, n_links, n_links / float(max(n, 1)), links_ms, fill_ms, moved / fill_ms / 1e6, cut_ms, runs_ms))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

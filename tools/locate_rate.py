"""The coloured graph of a phylogeny family placed on a reference (k = 23, (23, 14, uint32), the family and the
coloured graph of tools/links_rate.py): the ends of the cut coloured unitigs located among the k-mer positions of the
mode-0 spss_encode strings of input 0 (Context.seq_locate), timed alone: wall clock from a synchronised start to a
synchronised end, median of --reps after one warm-up, the profiler off.  The scan is timed with every run length R
that the library builds (KSH_LOCATE_RUN picks it; the library's own R is the one csrc/ksh_locate.hip states), the
reported rate is that of the library's own.  KssIndex.seq_hits over the same reference container and
Context.spss_links on the same strings, timed the same way in the same process, are the yardsticks.

The tool checks the located ends on the device against the definition where that is cheap (an end that is located has
a position inside the reference, every count is at least 1 exactly where a position is given), places the bubbles of
the graph with capi.place_bubbles on the host and reports them by reason.  Prints one JSON line and a table for
DESIGN.md 3.8m, and writes profiles/locate_rate.json.  No rate is a pass condition.

    python tools/locate_rate.py [--sets 8] [--size 1e7] [--reps 3] [--max-arm 8]
"""
import argparse
import json
import os
import re
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth_torch  # noqa: E402

RUNS = (8, 16, 32, 64)


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


def library_run():
    text = open(os.path.join(capi.CSRC_DIR, "ksh_locate.hip")).read()
    return int(re.search(r"^constexpr int kLocRun = (\d+);", text, flags=re.M).group(1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--size", type=float, default=1e7)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-arm", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "locate_rate.json"))
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
    r_off, r_start, r_cls, _ = idx.class_runs(unitigs, rows, cols, allow_unmatched=False)
    cu = ctx.spss_cut(unitigs, r_off, r_start)
    reference = compacts[0]
    positions = reference.n_bases - reference.n_strings * (k - 1)
    n = cu.n_strings

    links_ms, (off, to) = wall_ms(lambda: ctx.spss_links(cu, canonical=True), args.reps)
    hits_ms, _ = wall_ms(lambda: idx.seq_hits(reference, device=True), args.reps)
    by_run = {}
    for r in RUNS:
        os.environ["KSH_LOCATE_RUN"] = str(r)
        by_run[r], _ = wall_ms(lambda: ctx.seq_locate(cu, reference, canonical=True), args.reps)
    del os.environ["KSH_LOCATE_RUN"]
    own = library_run()
    locate_ms, (where, count) = wall_ms(lambda: ctx.seq_locate(cu, reference, canonical=True), args.reps)
    with torch.cuda.stream(ctx.stream):
        cnt = count.to(torch.int64)
        located = int((cnt > 0).sum())
        consistent = bool(((where >= 0) == (cnt > 0)).all()) and bool(((where >> 1) < positions).all())
        once = int((cnt == 1).sum())
        slots = 1
        while slots < 4 * n:
            slots <<= 1
    ends, arm_off, arm, arm_rows = ctx.link_bubbles(off, to, args.max_arm, string_class=r_cls, rows=rows)
    t0 = time.perf_counter()
    recs = capi.place_bubbles(cu.to_strings(), k, ends, arm_off, arm, where, count, reference.to_strings(), arm_rows,
                              args.sets)
    _, placed = capi.vcf_lines(recs, ["r%d" % i for i in range(reference.n_strings)], [0] * reference.n_strings)
    host_s = time.perf_counter() - t0
    res = {"tool": "locate_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "reps": args.reps, "strings": n, "ends": 2 * n, "table_slots": slots,
           "reference_sequences": reference.n_strings, "reference_positions": int(positions),
           "ends_per_position": round(2 * n / float(positions), 5),
           "run": own, "runs_tried_wall_ms": {str(r): round(ms, 3) for r, ms in by_run.items()},
           "seq_locate_wall_ms": round(locate_ms, 3),
           "positions_per_s": round(positions / locate_ms * 1e3),
           "seq_hits_wall_ms": round(hits_ms, 3), "seq_hits_positions_per_s": round(positions / hits_ms * 1e3),
           "spss_links_wall_ms": round(links_ms, 3),
           "locate_over_seq_hits": round(locate_ms / hits_ms, 4), "locate_over_links": round(locate_ms / links_ms, 4),
           "located_ends": located, "located_share": round(located / float(max(2 * n, 1)), 4),
           "ends_located_once": once, "bubbles": int(ends.shape[0]), "max_arm": args.max_arm,
           "bubbles_by_outcome": placed, "place_bubbles_host_s": round(host_s, 2),
           "where_and_count_agree": consistent, "spread_between_runs": "not measured (median of %d)" % args.reps}
    assert consistent
    idx.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    print("| ends | reference positions | seq_locate ms | positions / s | R = 8 / 16 / 32 / 64 ms | seq_hits ms | "
          "spss_links ms | located ends | placed / bubbles |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("| %d | %d | %.3f | %.3g | %s | %.3f | %.3f | %d (%.1f %%) | %d / %d |"
          % (2 * n, positions, locate_ms, positions / locate_ms * 1e3, " / ".join("%.3f" % by_run[r] for r in RUNS),
             hits_ms, links_ms, located, 100.0 * located / max(2 * n, 1), placed["placed"], int(ends.shape[0])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

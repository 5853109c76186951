"""The bubbles of the coloured graph of a phylogeny family (k = 23, (23, 14, uint32), the family of
tools/links_rate.py, made as bench.py makes its inputs): the union of the inputs with the class table
(select_classes), its unitigs (spss_encode, mode 1), their runs (KssIndex.class_runs), the strings cut at the runs
(Context.spss_cut), their links (Context.spss_links) and Context.link_bubbles of those links with the strings' classes,
timed alone: wall clock from a synchronised start to a synchronised end, median of --reps after one warm-up, the
profiler off.  Context.link_bubbles is two ksh_link_bubbles calls (one counts, one fills); the filling call alone is
timed as well.  Context.spss_links and KssIndex.class_runs, timed the same way in the same process, are the
yardsticks: the bubbles are the step that follows them.

The tool checks on the device that every reported source has two links out, every sink two links in and that
v <= w ^ 1 (the exact comparisons are tests/test_gpu_link_bubbles.py and tests/test_gpu_colored_bubbles.py), and
reports the bubbles, the arm strings per arm and the histogram of arm lengths.  Prints one JSON line and a table for
DESIGN.md 3.8j, and writes profiles/bubbles_rate.json.  No rate is a pass condition.

    python tools/bubbles_rate.py [--sets 8] [--size 1e7] [--reps 3] [--max-arm 8]
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
    ap.add_argument("--max-arm", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "bubbles_rate.json"))
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

    runs_ms, (r_off, r_start, r_cls, _) = wall_ms(
        lambda: idx.class_runs(unitigs, rows, cols, allow_unmatched=False), args.reps)
    cu = ctx.spss_cut(unitigs, r_off, r_start)
    links_ms, (off, to) = wall_ms(lambda: ctx.spss_links(cu, canonical=True), args.reps)
    n, n_links = cu.n_strings, int(to.numel())
    kw = dict(string_class=r_cls, rows=rows)
    bubbles_ms, (ends, arm_off, arm, arm_rows) = wall_ms(
        lambda: ctx.link_bubbles(off, to, args.max_arm, **kw), args.reps)
    nb, na = int(ends.shape[0]), int(arm.numel())
    with torch.cuda.stream(ctx.stream):
        f_ends = torch.empty(2 * max(nb, 1), dtype=torch.int64, device=dev)
        f_off = torch.empty(2 * max(nb, 1) + 1, dtype=torch.int64, device=dev)
        f_arm = torch.empty(max(na, 1), dtype=torch.int64, device=dev)
        f_rows = torch.empty(4 * max(nb, 1), dtype=torch.int64, device=dev)
    fill_ms, got = wall_ms(lambda: ctx.link_bubbles_raw(off, to, args.max_arm, max(nb, 1), na, f_ends, f_off, f_arm,
                                                        f_rows, **kw), args.reps)
    assert got == (capi.KSH_OK, nb, na)
    with torch.cuda.stream(ctx.stream):
        same = bool(torch.equal(f_ends[:2 * nb].reshape(nb, 2), ends) and torch.equal(f_off[:2 * nb + 1], arm_off)
                    and torch.equal(f_arm[:na], arm)
                    and torch.equal(f_rows[:4 * nb], arm_rows.reshape(-1).view(torch.int64)))
        outdeg = off[1:] - off[:-1]
        v, w = ends[:, 0], ends[:, 1]
        sources_ok = bool((outdeg[v] == 2).all())
        sinks_ok = bool((outdeg[w ^ 1] == 2).all())
        once = bool((v <= (w ^ 1)).all()) and bool((v[1:] > v[:-1]).all())
        lens = arm_off[1:] - arm_off[:-1]
        hist = torch.bincount(lens, minlength=2).tolist() if nb else []
        hairpins = int((w == (v ^ 1)).sum())
        no_carrier = int(((arm_rows.view(torch.int64) == 0).all(dim=1)).sum()) if nb else 0
    res = {"tool": "bubbles_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "classes": int(counts.size), "reps": args.reps, "max_arm": args.max_arm, "unitigs": unitigs.n_strings,
           "strings": n, "links": n_links, "bubbles": nb, "arm_strings": na,
           "arm_strings_per_arm": round(na / float(max(2 * nb, 1)), 4), "arm_length_histogram": hist,
           "hairpins": hairpins, "arms_without_carrier": no_carrier,
           "link_bubbles_wall_ms": round(bubbles_ms, 3), "fill_call_wall_ms": round(fill_ms, 3),
           "spss_links_wall_ms": round(links_ms, 3), "class_runs_wall_ms": round(runs_ms, 3),
           "bubbles_over_links": round(bubbles_ms / links_ms, 4),
           "bubbles_over_class_runs": round(bubbles_ms / runs_ms, 4),
           "sources_have_two_out": sources_ok, "sinks_have_two_in": sinks_ok, "each_reported_once": once,
           "fill_call_equals_wrapper": same, "spread_between_runs": "not measured (median of %d)" % args.reps}
    assert sources_ok and sinks_ok and once and same
    idx.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    print("| strings | links | bubbles | arm strings / arm | link_bubbles ms | fill call ms | spss_links ms | "
          "class_runs ms |")
    print("|---|---|---|---|---|---|---|---|")
    print("| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f |"
          % (n, n_links, nb, na / float(max(2 * nb, 1)), bubbles_ms, fill_ms, links_ms, runs_ms))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

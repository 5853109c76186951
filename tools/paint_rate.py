"""Painting the coloured graph of a phylogeny family (k = 23, (23, 14, uint32), inputs made as bench.py makes them):
the union of the inputs with the class of every k-mer (select_classes), its SPSS (spss_encode), and
KssIndex.class_runs of those strings with the full class table -- the runs are the compact colouring, one class per
run of positions where select_classes stores one per k-mer.  On the same sequences and index, in the same process,
KssIndex.seq_hits: it shares the extraction and the look-up, so it is the yardstick.  Both are timed the same way:
wall clock from a synchronised start to a synchronised end, median of --reps after one warm-up.  The context's timers
(kinds 6 and 7) split one further painting into the look-up stages and the two new stages.  The index holds the inputs
as nodes without edges (no KmerSetSet is built: the painting reads only the index).  The tool checks that the runs
cover every position and that the classes counted per position are those of select_classes counted per k-mer (the
exact comparison, k-mer by k-mer, is tests/test_gpu_paint.py).  Prints one JSON line and writes
profiles/paint_rate.json.  No ratio is a pass condition: the figures are what they are.

    python tools/paint_rate.py [--sets 8] [--size 1e7] [--reps 3] [--route 0]
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
    ap.add_argument("--route", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "paint_rate.json"))
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
    res = {"tool": "paint_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "nodes": idx.n_nodes, "words_per_row": idx.words, "classes": int(counts.size), "strings": spss.n_strings,
           "positions": int(positions), "route": args.route, "reps": args.reps}

    with torch.cuda.stream(ctx.stream):
        off = torch.empty(spss.n_strings + 1, dtype=torch.int64, device=dev)
        start = torch.empty(positions, dtype=torch.int32, device=dev)  # (room for a run per position)
        cls = torch.empty(positions, dtype=torch.int32, device=dev)

    def paint():
        rc, n_runs, missing = idx.class_runs_raw(spss, rows, positions, off, start, cls, cols, route=args.route,
                                                 allow_unmatched=False)
        capi.check(rc)
        return n_runs

    paint_ms, n_runs = wall_ms(paint, args.reps)
    routes = idx.routes()
    count_ms, _ = wall_ms(lambda: idx.class_runs_raw(spss, rows, 0, None, None, None, cols, route=args.route), args.reps)
    hits_ms, _ = wall_ms(lambda: idx.seq_hits(spss, route=args.route, device=True), args.reps)
    ctx.enable_timing(True)
    ctx.timing_reset()
    paint()
    (lookup_ms, passes), (new_ms, _) = ctx.timing_read(6), ctx.timing_read(7)
    ctx.enable_timing(False)
    run_bytes = 8 * n_runs + 8 * (spss.n_strings + 1)  # start and class per run, an offset per string
    res.update({"paint_wall_ms": round(paint_ms, 3), "paint_positions_per_s": round(positions / paint_ms * 1e3),
                "count_only_wall_ms": round(count_ms, 3), "seq_hits_wall_ms": round(hits_ms, 3),
                "seq_hits_positions_per_s": round(positions / hits_ms * 1e3), "routes_bits": routes, "passes": passes,
                "timed_lookup_ms": round(lookup_ms, 3), "timed_classify_and_runs_ms": round(new_ms, 3),
                "new_stages_share_of_a_pass": round(new_ms / (lookup_ms + new_ms), 4), "runs": n_runs,
                "runs_per_position": round(n_runs / positions, 6), "run_bytes": run_bytes,
                "bytes_at_4_per_kmer": 4 * positions, "run_bytes_over_4_per_kmer": round(run_bytes / (4.0 * positions), 4),
                "class_bytes_alone_over_4_per_kmer": round(n_runs / float(positions), 4)})
    # the runs say what select_classes says: a class per position, looked up by the position's canonical k-mer
    with torch.cuda.stream(ctx.stream):
        lens = spss.lens[:spss.n_strings].to(torch.int64) + 1
        first = torch.cumsum(lens, 0) - lens
        begin = first.repeat_interleave((off[1:] - off[:-1])) + start[:n_runs].to(torch.int64)
        length = torch.diff(torch.cat([begin, torch.tensor([positions], device=dev)]))
        per_position = cls[:n_runs].repeat_interleave(length)
        decoded = ctx.spss_decode(spss)  # the k-mers of the strings as a set: the union again, keys in its order
        same_set = decoded.n_keys == union.n_keys and bool(torch.equal(decoded.offsets, union.offsets))
        res["runs_cover_every_position"] = bool(per_position.numel() == positions and int(length.min()) >= 1)
        res["class_histogram_equal"] = bool(same_set and torch.equal(
            torch.bincount(per_position.to(torch.int64), minlength=counts.size),
            torch.bincount(ids.to(torch.int64), minlength=counts.size)))
    idx.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

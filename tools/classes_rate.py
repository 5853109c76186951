"""The colour-class table of the bench's KmerSetSet (64 sets of 10^8 k-mers, k = 23, (23, 14, uint32), inputs made
as bench.py makes them), with cols = the inputs: ksh_kss_color_classes against the route to the same table that
exists without it -- select() of the union of the columns, its k-mers (expanded on the device) through
query(packed=True), the columns' bits out of the rows, then unique rows with counts in torch; nothing but the table
itself crosses to the host on either side.  Both sides are timed the same way: wall clock from a
synchronised start to a synchronised end, median of --reps after one warm-up.  The tool checks that both give the
same table.  Prints one JSON line and writes profiles/classes_rate.json.  No ratio is a pass condition: the figures
are what they are.

    python tools/classes_rate.py [--sets 64] [--size 1e8] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth, synth_torch  # noqa: E402


def wall_ms(fn, reps):
    fn()  # warm-up: the pool holds the scratch from then on
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], out


def baseline_classes(ctx, idx, cols, chunk=1 << 24):
    """The table without the call, for at most 64 columns (one row word): the union's k-mers, their rows over all
    nodes in passes of `chunk`, the columns' bits gathered into one word, unique with counts.  Everything stays on
    the device until the table itself: the union's k-mers are expanded there (ksh_set_kmers), the words of the
    passes go into one tensor made ahead, and only the unique rows and their counts come to the host.  The zero row
    (k-mers that only nodes outside cols hold) is what the distinct count of the structure leaves over."""
    assert len(cols) <= 64
    union = idx.select(cols)
    with torch.cuda.stream(ctx.stream):
        n = union.n_keys
        kmers = torch.empty(max(n, 1), dtype=torch.int64, device=ctx.device)
        view = union.view()
        capi.check(capi.lib().ksh_set_kmers(ctx.h, C.byref(union.g), C.byref(view), kmers.data_ptr()))
        kmers = kmers[:n]
        del union
        word = torch.zeros(n, dtype=torch.int64, device=ctx.device)
        for at in range(0, n, chunk):
            rows = idx.query(kmers[at:at + chunk], packed=True)
            part = word[at:at + chunk]
            for a, c in enumerate(cols):
                part |= ((rows[:, c >> 6] >> (c & 63)) & 1) << a
            del rows
        del kmers
        u, cnt = torch.unique(word, return_counts=True)
        u, cnt = u.cpu().numpy().view(np.uint64), cnt.cpu().numpy()
    order = np.argsort(u, kind="stable")
    return u[order], cnt[order].astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--size", type=float, default=1e8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "classes_rate.json"))
    args = ap.parse_args()
    k, nbits = 23, 14
    g = capi.geom(k, nbits)
    ctx = capi.Context(0)
    dev = ctx.device
    ids = synth.sample_bucket_ids(nbits, seed=args.seed + 1)
    kmers = synth_torch.phylogeny_sets(k, args.sets, int(args.size), args.seed, dev)
    compacts = []
    for i, km in enumerate(kmers):
        compacts.append(ctx.spss_encode(synth_torch.device_set(g, km), mode=0))
        kmers[i] = None
    del kmers
    dkss = capi.DeviceKmerSetSet(ctx, compacts, ids)
    idx = capi.KssIndex.from_kss(dkss)
    cols = list(range(args.sets))
    info = idx.info()
    res = {"tool": "classes_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "nodes": idx.n_nodes, "resident_bytes": info["resident_bytes"], "reps": args.reps}

    call_ms, (rows, counts) = wall_ms(lambda: idx.color_classes(cols), args.reps)
    res.update({"classes_wall_ms": round(call_ms, 3), "routes_bits": idx.routes(), "classes": int(counts.size),
                "distinct_kmers": int(counts.sum()), "largest_class": int(counts.max()) if counts.size else 0})
    print(json.dumps(res), file=sys.stderr)
    base_ms, (b_rows, b_counts) = wall_ms(lambda: baseline_classes(ctx, idx, cols), args.reps)
    some = rows[:, 0] != 0  # the baseline sees the union of the columns only: every class but the zero row
    res.update({"baseline_wall_ms": round(base_ms, 3), "baseline_over_classes": round(base_ms / call_ms, 3),
                "same_table": bool(not rows[:, 1].any() and np.array_equal(rows[some, 0], b_rows)
                                   and np.array_equal(counts[some], b_counts))})
    idx.close()
    dkss.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

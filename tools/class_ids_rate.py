"""The class id of every k-mer of the bench's KmerSetSet (64 sets of 10^8 k-mers, k = 23, (23, 14, uint32), inputs
made as bench.py makes them), with cols = the inputs and the union selection: ksh_kss_select_class_ids against the
route to the same ids that exists without it -- select() of the union of the columns, its k-mers (expanded on the
device by ksh_set_kmers) through query(packed=True) over all nodes in chunks, the columns' bits out of the rows, then
torch.unique(..., return_inverse=True); the ids stay on the device on either side.  Both sides are timed the same
way: wall clock from a synchronised start to a synchronised end, median of --reps after one warm-up.  The tool checks
that both give the same ids.  Prints one JSON line and writes profiles/class_ids_rate.json.  No ratio is a pass
condition: the figures are what they are.  A side that cannot run at the given size is recorded as such.

    python tools/class_ids_rate.py [--sets 64] [--size 1e8] [--reps 3]
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

SIGN = -(1 << 63)  # int64 words compare as unsigned once their top bit is flipped


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


def baseline_ids(ctx, idx, cols, chunk=1 << 24):
    """(the union as a DeviceSet, ids, the distinct rows) without the call, for at most 64 columns (one row word):
    the union's k-mers, their rows over all nodes in passes of `chunk`, the columns' bits gathered into one word per
    k-mer, then the distinct words and each k-mer's position among them.  Everything stays on the device."""
    assert len(cols) <= 64
    union = idx.select(cols)
    with torch.cuda.stream(ctx.stream):
        n = union.n_keys
        kmers = torch.empty(max(n, 1), dtype=torch.int64, device=ctx.device)
        view = union.view()
        capi.check(capi.lib().ksh_set_kmers(ctx.h, C.byref(union.g), C.byref(view), kmers.data_ptr()))
        kmers = kmers[:n]
        word = torch.zeros(n, dtype=torch.int64, device=ctx.device)
        for at in range(0, n, chunk):
            rows = idx.query(kmers[at:at + chunk], packed=True)
            part = word[at:at + chunk]
            for a, c in enumerate(cols):
                part |= ((rows[:, c >> 6] >> (c & 63)) & 1) << a
            del rows
        del kmers
        word ^= SIGN
        u, inverse = torch.unique(word, return_inverse=True)
        del word
        return union, inverse, u ^ SIGN


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--size", type=float, default=1e8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "class_ids_rate.json"))
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
    res = {"tool": "class_ids_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "nodes": idx.n_nodes, "resident_bytes": info["resident_bytes"], "reps": args.reps}

    got = None
    try:
        table_ms, (rows, counts) = wall_ms(lambda: idx.color_classes(cols), args.reps)
        res.update({"class_table_wall_ms": round(table_ms, 3), "classes": int(counts.size)})
        whole_ms, got = wall_ms(lambda: idx.select_classes(cols, rows=rows), args.reps)  # count, allocate, the call
        union, ids_call = got[0], got[1]
        n = union.n_keys
        with torch.cuda.stream(ctx.stream):
            again = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        call_ms, _ = wall_ms(lambda: idx.select_class_ids(union.offsets, n, rows, union.keys, again, cols), args.reps)
        ids_only_ms, _ = wall_ms(lambda: idx.select_class_ids(union.offsets, n, rows, None, again, cols), args.reps)
        res.update({"select_classes_wall_ms": round(whole_ms, 3), "call_wall_ms": round(call_ms, 3),
                    "call_ids_only_wall_ms": round(ids_only_ms, 3), "routes_bits": idx.routes(), "selected_kmers": n,
                    "bytes_out_per_kmer": g.key_bytes + 4})
        del again
    except capi.KshError as e:
        res["call_cannot_run"] = str(e)[:300]
    print(json.dumps(res), file=sys.stderr)
    try:
        base_ms, (b_union, b_ids, b_rows) = wall_ms(lambda: baseline_ids(ctx, idx, cols), args.reps)
        res["baseline_wall_ms"] = round(base_ms, 3)
        if got is not None:
            res["baseline_over_select_classes"] = round(base_ms / whole_ms, 3)
            some = rows.any(axis=1)  # the baseline sees the union of the columns only: every class but the zero row
            shift = int(rows.shape[0] - some.sum())  # (the zero row, if there is one, is the table's first)
            same = (not rows[:, 1].any() and np.array_equal(rows[some, 0], b_rows.cpu().numpy().view(np.uint64))
                    and b_union.n_keys == n
                    and torch.equal(b_union.keys[:n * g.key_bytes], union.keys[:n * g.key_bytes])
                    and bool(torch.equal(ids_call.to(torch.int64), b_ids + shift)))
            res["same_ids"] = bool(same)
    except (capi.KshError, RuntimeError) as e:  # (torch reports exhausted memory as a RuntimeError)
        res["baseline_cannot_run"] = str(e)[:300]
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

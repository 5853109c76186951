"""Worker of tests/test_gpu_loop_families.py: ksh_kss_build over every family of tests/loop_families.py (or the
ones named on the command line) in a process of its own -- the switches KSH_KSS_LOOP and KSH_REWEIGH are read
once per process -- each against the oracle with the full comparison (tests/kss_compare.py).

  [KSH_KSS_LOOP=ahead | KSH_REWEIGH=full] python loop_families_worker.py [NAME ...]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
import loop_families as lf  # noqa: E402
import oracle_lib as ol  # noqa: E402
from kmersets import capi  # noqa: E402
from kss_compare import compare  # noqa: E402


def main():
    names = sys.argv[1:] or list(lf.FAMILIES)
    ctx = capi.Context(0)
    for name in names:
        k, n, kb, sets, ids, osets, ocompacts, okss = lf.oracle_build(ol, name)
        g = capi.geom(k, n)
        t0 = time.perf_counter()
        dcompacts = [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocompacts]
        dkss = capi.DeviceKmerSetSet(ctx, dcompacts, ids)
        merges = compare(sets, osets, okss, dkss)
        st = dkss.stats()
        print("%s: %d merges, %d encodes (%d weighed), %.2f s" % (name, merges, st["n_encodes"], st["n_weighed"],
                                                                   time.perf_counter() - t0), flush=True)
        dkss.close()
    ctx.close()
    print("loop families ok %d" % len(names))


if __name__ == "__main__":
    main()

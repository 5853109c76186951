"""Child of tests/test_gpu_decode_walk.py: runs every case of tests/decode_walk_cases.py in this process, whose
environment carries the switch under test (KSH_DECODE_L2_MIN and KSH_DECODE_SCATTER are read once per process).  One
line per case -- its name, the route the model names for it here, the seconds it took -- and a final ok line."""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
sys.path.insert(0, HERE)


def main(env_name):
    from kmersets import capi
    import decode_walk_cases as dw
    import test_gpu_decode_walk as t

    ctx = capi.Context(0)
    n = 0
    for case in dw.all_cases():
        t0 = time.time()
        how = t.check_case(ctx, case, env_name)
        print("case %s %s %.2f s" % (case.name, how, time.time() - t0), flush=True)
        n += 1
    ctx.close()
    print("decode walk ok: %d cases" % n)


if __name__ == "__main__":
    main(sys.argv[1])

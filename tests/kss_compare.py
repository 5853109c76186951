"""The full comparison of a device KmerSetSet with the oracle's, shared by test_gpu_kmer_set_set.py,
test_gpu_loop_families.py and tests/loop_families_worker.py."""
import numpy as np


def compare(sets, osets, okss, dkss):
    n0 = len(sets)
    assert np.array_equal(dkss.initial_weights(), okss.initial_weights(n0))
    it, cp, imp = dkss.trace()
    assert np.array_equal(it, okss.iterations())
    ocp, oimp = okss.checkpoints()
    assert np.array_equal(cp, ocp)
    assert np.array_equal(imp, oimp)            # same float arithmetic, bit for bit
    assert dkss.size() == okss.size()
    assert dkss.meta() == okss.meta()
    st = dkss.stats()
    assert st["initial_total_size"] == okss.stat(0) and st["final_total_size"] == okss.stat(1)
    assert st["initial_spss_weight"] == okss.stat(2) and st["n_processed"] == okss.stat(3)
    for i in range(okss.size()):
        node = okss.node(i)
        assert dkss.node_strings(i) == node.strings(), "node %d" % i
        assert dkss.node_size(i) == node.size()
    for i in range(n0):
        got = dkss.get_kmers(i)
        assert np.array_equal(got, sets[i])      # test/kmer_set_set.cc:30-34
        assert np.array_equal(got, okss.get(i).kmers())
    return len(it)

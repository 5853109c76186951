"""The C++17 host mirror's KmerSetSetIndex::PairCounts (kmer-sets-compression_amd/cpp/core/kmer_set_set.h), driven by
cpp/test/test_pair_counts.cc: on one small family the table of all nodes equals the sizes of the pairwise
Intersection of the mirror's Get(a) and Get(b), and a shuffled list of columns gives the matching sub-table."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_pair_counts_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_pair_counts"])
    out = subprocess.run([os.path.join(CPP, "build", "test_pair_counts")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

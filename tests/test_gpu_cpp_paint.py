"""The C++17 host mirror's KmerSetSetIndex::Paint (kmer-sets-compression_amd/cpp/core/kmer_set_set.h), driven by
cpp/test/test_paint.cc: on one small family the runs of every sequence, expanded to a class per k-mer position, equal
a host loop over the mirror's own Get(i).Contains; a partial table and too small a capacity behave as the header
says."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_paint_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_paint"])
    out = subprocess.run([os.path.join(CPP, "build", "test_paint")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

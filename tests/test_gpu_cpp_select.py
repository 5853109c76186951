"""The C++17 host mirror's KmerSetSetIndex::Select and Spectrum (kmer-sets-compression_amd/cpp/core/kmer_set_set.h),
driven by cpp/test/test_select.cc: on one small family the core, the union, the k-mers private to one input and
(A & B) \\ C equal what the mirror's own Get / Intersection / Add / Sub give, and the spectrum sums to the size of the
union of all nodes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_select_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_select"])
    out = subprocess.run([os.path.join(CPP, "build", "test_select")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

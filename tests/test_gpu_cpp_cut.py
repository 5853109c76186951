"""The C++17 host mirror's KmerSetCompact::Cut and KmerSetSetIndex::ColoredUnitigs
(kmer-sets-compression_amd/cpp/core/), driven by cpp/test/test_cut.cc: a cut worked by hand, and on one small family
the k-mers of the coloured unitigs with the class of their string equal SelectClasses."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_cut_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_cut"])
    out = subprocess.run([os.path.join(CPP, "build", "test_cut")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

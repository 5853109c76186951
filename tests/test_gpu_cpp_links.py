"""The C++17 host mirror's KmerSetCompact::Links and KmerSetSetIndex::ColoredGraph
(kmer-sets-compression_amd/cpp/core/), driven by cpp/test/test_links.cc: links worked by hand in both modes, and on one
small family the coloured graph's links checked textually, twin by twin and against the brute-force de Bruijn edges."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_links_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_links"])
    out = subprocess.run([os.path.join(CPP, "build", "test_links")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

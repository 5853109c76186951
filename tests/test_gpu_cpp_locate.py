"""The C++17 host mirror's KmerSetCompact::Locate (kmer-sets-compression_amd/cpp/core/), driven by
cpp/test/test_locate.cc: ends located by hand in both modes, a malformed reference refused with the context serving
afterwards, and reads cut from a random reference against a brute-force search of all windows."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_locate_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_locate"])
    out = subprocess.run([os.path.join(CPP, "build", "test_locate")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

"""The C++17 host mirror's KmerSetSetIndex::SelectClasses (kmer-sets-compression_amd/cpp/core/kmer_set_set.h), driven
by cpp/test/test_class_ids.cc: on one small family the class id of every k-mer of the inputs equals the one computed
on the host from the mirror's own Get(i), the ids counted per class are ColorClasses, and a foreign table is
refused."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "kmer-sets-compression_amd", "cpp")


def test_cpp_class_ids_mirror(gpu):
    from kmersets import capi

    capi.build()
    subprocess.check_call(["make", "-C", CPP, "-s", "build/test_class_ids"])
    out = subprocess.run([os.path.join(CPP, "build", "test_class_ids")], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    print(out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failed" in out.stdout

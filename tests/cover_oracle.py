"""The oracle's path cover from unitigs on strings in any order (tests/cover_shim.cc over oracle/ko_spss.h),
for the cover tests: GetSPSSCanonical(unitigs, fast) and GetSPSS(unitigs)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def shim():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="cover_shim_"), "libcover_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "oracle"),
                               "-o", out, os.path.join(ROOT, "tests", "cover_shim.cc")])
        L = C.CDLL(out)
        i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
        L.cover_shim_run.restype = C.c_int64
        L.cover_shim_run.argtypes = [C.c_char_p, i64p, C.c_int64, C.c_int, C.c_int]
        L.cover_shim_total.restype = C.c_int64
        L.cover_shim_total.argtypes = []
        L.cover_shim_get.restype = None
        L.cover_shim_get.argtypes = [C.c_char_p, i64p]
        _lib = L
    return _lib


def cover(unitigs, k, canonical=True, fast=True):
    L = shim()
    lens = np.array([len(s) for s in unitigs] or [0], dtype=np.int64)
    n = L.cover_shim_run("".join(unitigs).encode(), lens, len(unitigs), k, (0 if fast else 1) if canonical else 2)
    total = L.cover_shim_total()
    buf = C.create_string_buffer(total + 1)
    out_lens = np.zeros(max(n, 1), dtype=np.int64)
    L.cover_shim_get(buf, out_lens)
    raw = buf.raw[:total].decode()
    out, at = [], 0
    for ln in out_lens[:n]:
        out.append(raw[at:at + int(ln)])
        at += int(ln)
    return out


def oracle_capi_cover(unitigs, k):
    """ko_spss_from_unitigs: the oracle's own C API, canonical and fast."""
    import oracle_lib as ol

    held = ol.Strings.from_list(unitigs)  # (kept alive across the call: its handle is freed with it)
    return ol.Strings(ol.lib().ko_spss_from_unitigs(held.h, k)).to_list()


def revcomp_string(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def shuffled(unitigs, seed, flip=True):
    """The unitigs in a random order, a random half of them reverse-complemented (flip)."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(unitigs))
    out = [unitigs[i] for i in order]
    if flip:
        out = [revcomp_string(s) if f else s for s, f in zip(out, rng.integers(0, 2, size=len(out)))]
    return out

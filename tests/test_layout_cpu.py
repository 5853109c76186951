"""The two-mode bump carver that every stage's scratch layout goes through (csrc/ksh_layout.h), on the CPU:
tests/layout_main.cc, a stand-alone program, is compiled with the address and undefined-behaviour sanitizers and
runs a handful of mixed layouts -- element sizes 1, 2, 4, 8 and 16, counts 0 and 1, pads, an array that is only
sometimes used in both of its states -- once measuring and once on a real block."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer-sets-compression_amd", "csrc")
LAYOUTS = ("every-width", "sometimes-unused", "sometimes-used", "all-empty", "odd-pad")


@pytest.fixture(scope="module")
def report():
    exe = os.path.join(tempfile.mkdtemp(prefix="layout_main_"), "layout_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "layout_main.cc")])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert done.returncode == 0, done.stderr
    out = {"layout": {}, "take": {}, "bind": {}}
    for line in done.stdout.splitlines():
        f = line.split()
        if f[0] == "round":
            out["round"] = [int(x) for x in f[1:]]
        elif f[0] == "layout":
            out["layout"][f[1], f[2]] = (int(f[3]), int(f[4]))
        elif f[0] == "take":
            out["take"].setdefault((f[1], f[2]), []).append((int(f[3]), int(f[4])))
        elif f[0] == "bind":
            out["bind"][f[1]] = [int(x) for x in f[2:]]
    return out


def test_rounding(report):
    assert report["round"] == [0, 256, 256, 256, 512]


def test_the_program_ran_every_layout(report):
    assert {name for name, _ in report["layout"]} == set(LAYOUTS)


@pytest.mark.parametrize("name", LAYOUTS)
def test_measuring_and_binding_agree(report, name):
    measured, block = report["layout"][name, "measure"]
    bound, _ = report["layout"][name, "bind"]
    assert measured == bound == block
    # while measuring every pointer is null; the arrays asked for are the same in both runs
    assert all(off == -1 for off, _ in report["take"][name, "measure"])
    assert [b for _, b in report["take"][name, "measure"]] == [b for _, b in report["take"][name, "bind"]]
    # layout_bind: the block fits, one byte less does not, no block does not
    assert report["bind"][name] == [1, 1, 1]


@pytest.mark.parametrize("name", LAYOUTS)
def test_arrays_are_aligned_inside_and_apart(report, name):
    _, block = report["layout"][name, "bind"]
    end = 0
    for off, need in report["take"][name, "bind"]:
        if off == -1:  # the sometimes-used array, unused
            assert name == "sometimes-unused"
            continue
        assert off % 256 == 0
        assert off >= end and off + need <= block
        end = off + need


def test_an_unused_array_keeps_its_room(report):
    """The block's size does not depend on whether the sometimes-used array is used, nor does any other array's
    place; only its pointer does."""
    assert report["layout"]["sometimes-unused", "bind"] == report["layout"]["sometimes-used", "bind"]
    unused, used = report["take"]["sometimes-unused", "bind"], report["take"]["sometimes-used", "bind"]
    assert [x for i, x in enumerate(unused) if i != 2] == [x for i, x in enumerate(used) if i != 2]
    assert unused[2][0] == -1 and used[2][0] > 0


def test_pads_are_counted(report):
    takes = report["take"]["sometimes-used", "bind"]
    assert takes[1][0] - takes[0][0] == 4096 + 4096  # u32[1000] rounds to 4096, then the pad
    takes = report["take"]["odd-pad", "bind"]
    assert takes[2][0] - takes[1][0] == 512 + 256  # u8[257] rounds to 512; the 24-byte pad costs a whole step
    assert report["layout"]["odd-pad", "bind"][0] == takes[3][0] + 512 + 4096


def test_the_header_is_small_and_host_only():
    text = open(os.path.join(CSRC, "ksh_layout.h")).read()
    lines = text.splitlines()
    assert len(lines) <= 80
    assert [x for x in lines if x.startswith("#include")] == ["#include <cstddef>"]
    assert text.count("#define") == 1 and "virtual" not in text  # (the include guard)

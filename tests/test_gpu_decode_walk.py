"""The front half of the SPSS decode (k_str_bases, k_mark_ends, k_decode<false/true>, k_hist_columns, k_decode_l1,
k_decode_l2 in csrc/ksh_decode.hip, with decode_geometry and the route choice of scatter_sort) over string ends,
word, group and tile edges: the cases of tests/decode_walk_cases.py through ksh_spss_size, ksh_spss_decode_plan /
_write and ksh_kmer_count_write at cutoffs 1 and 2, for both canonical flags, on three routes -- in this process
with no switch set (where the pair of 2^20 - 1 and 2^20 k-mer occurrences falls on both sides of the default
switch), in a child with KSH_DECODE_L2_MIN=1024 and in a child with KSH_DECODE_SCATTER=direct (both switches are read
once per process).  Expected values are np.unique with counts of the numpy reference on the strings (tied to the oracle
on the CPU, tests/test_decode_walk_model_cpu.py); everything is exact.  Before a case runs, the model's branches are
asserted against what the case declares, so a case cannot silently test something else."""
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_walk_cases as dw
from kmersets import capi
from test_gpu_bucket_sort import ascending_in_buckets

pytestmark = pytest.mark.gpu
SWITCHES = ("KSH_DECODE_L2_MIN", "KSH_DECODE_SCATTER")
ALL = dw.all_cases()
_failed_children = []


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def device_spss(ctx, case):
    import torch

    g = capi.geom(case.g.k, case.g.n, case.g.kb)
    assert g.key_bytes == case.g.kb
    words, lens = case.words_and_lens()
    w = torch.from_numpy(words.view(np.int64).copy()).to(ctx.device)
    ln = torch.from_numpy(lens.view(np.int32).copy()).to(ctx.device)
    return capi.DeviceSpss(g, w, ln, len(case.strings), case.n_bases)


def check_set(got, want, want_off, want_keys, what):
    assert got.n_keys == want.size, (what, got.n_keys, want.size)
    off, keys = got.to_numpy()
    assert np.array_equal(off, want_off), what
    assert keys.size == want.size and ascending_in_buckets(off, keys), what
    assert keys.dtype == want_keys.dtype and np.array_equal(keys, want_keys), what
    assert np.array_equal(got.kmers(), want), what


def check_case(ctx, case, env_name):
    """One case in a process whose environment is dw.ENVS[env_name]: the size, the decode, the count at cutoff 1, and
    the plan with the count at cutoff 2 written on it, for both canonical flags.  Returns the route the model names."""
    assert {s: os.environ[s] for s in SWITCHES if s in os.environ} == dw.ENVS[env_name], env_name
    got_branches = case.branches()
    assert case.expect <= got_branches and not (case.forbid & got_branches), (case.name, sorted(got_branches))
    how = dw.route(case, dw.ENVS[env_name])
    sp = device_spss(ctx, case)
    # the plan's count comes from the histogram of the walk: a phantom k-mer across a string end or in the tail shows
    # here even where the set saturates
    assert ctx.spss_size(sp) == case.n_occ, case.name
    for canonical in (False, True):
        what = (case.name, env_name, how, canonical)
        vals, counts = case.counted(canonical)
        want, _, want_off, want_keys = dw.expected_at(vals, counts, case.g, 1)
        check_set(ctx.spss_decode(sp, canonical=canonical), want, want_off, want_keys, what)
        gset, n_cut = ctx.kmer_count(sp, 1, canonical=canonical)
        assert n_cut == 0, what
        check_set(gset, want, want_off, want_keys, what + (1,))
        plan = ctx.spss_decode_plan(sp, canonical)
        assert plan.n_keys == case.n_occ, (what, plan.n_keys, case.n_occ)
        want, want_cut, want_off, want_keys = dw.expected_at(vals, counts, case.g, 2)
        gset, n_cut = ctx.kmer_count_write(plan, 2)
        assert n_cut == want_cut, (what, n_cut, want_cut)
        check_set(gset, want, want_off, want_keys, what + (2,))
    return how


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_decode_walk_default_switches(ctx, case):
    """Every case with no switch set: the direct scatter below 2^20 k-mer occurrences, the two-level one from there."""
    how = check_case(ctx, case, "default")
    assert how == ("two_level" if case.n_occ >= 1 << 20 and 7 < min(case.g.n, 14) else "direct")
    if case.family == "switch":
        assert case.n_occ in ((1 << 20) - 1, 1 << 20) and how == ("direct", "two_level")[case.n_occ - (1 << 20) + 1]


@pytest.mark.parametrize("env_name", ["l2min", "direct"])
def test_decode_walk_child(gpu, env_name):
    """Every case in a fresh process with one switch set (tests/decode_walk_worker.py): KSH_DECODE_L2_MIN=1024 sends
    all but the cases of fewer than 1024 occurrences or N <= 7 through k_decode_l1 / k_decode_l2,
    KSH_DECODE_SCATTER=direct all of them through k_decode<true>."""
    assert not _failed_children, "not started: the child before this one failed (%s)" % _failed_children
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(dw.ENVS[env_name])
    try:
        r = subprocess.run([sys.executable, os.path.join(here, "decode_walk_worker.py"), env_name], env=env,
                           capture_output=True, text=True, timeout=300)
        ok = r.returncode == 0 and ("decode walk ok: %d cases" % len(ALL)) in r.stdout
        report = "%s: exit %d\n%s%s" % (env_name, r.returncode, r.stdout[-3000:], r.stderr[-4000:])
    except subprocess.TimeoutExpired as e:
        ok, report = False, "%s: no end after %d s\n%s" % (env_name, e.timeout, (e.stdout or b"")[-3000:])
    if not ok:
        _failed_children.append(env_name)
    assert ok, report
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("case ")]
    assert [ln[1] for ln in lines] == [c.name for c in ALL]
    assert [ln[2] for ln in lines] == [dw.route(c, dw.ENVS[env_name]) for c in ALL]
    if env_name == "direct":
        assert {ln[2] for ln in lines} == {"direct"}
    else:
        assert sum(ln[2] == "two_level" for ln in lines) >= 40

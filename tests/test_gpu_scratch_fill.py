"""Every stage on poisoned scratch, and the chained scan across its epoch wrap.

The other modules pin each stage's inputs; this one pins the memory the stages work in.  With the scratch fill
(ksh_debug_set_scratch_fill, KSH_SCRATCH_FILL) every block of scratch whose contents are undefined by
contract -- a fresh allocation, a pool block at its rounded size, an arena range, the plan block, a slot at the start of
a plan -- holds one byte value when it is handed out: 0xFF makes every integer -1 and every flag set, 0xA5 a large
unrelated number, 0x00 is the control.  A kernel that reads scratch it never wrote then computes something else.

Nothing here has expected values of its own: (a) runs the columns and victims of the plan-protocol table through
test_gpu_plan_protocol's own run_intruder / Victim and the checks they return, (b) starts the four route-bearing
workers as their own tests start them, under KSH_SCRATCH_FILL=0xFF, (c) calls the sweeps' own test functions with a
context of this module.  The fill counters (ksh_debug_scratch_fill_stats) show that the hook is live where work is
launched.  The epoch test places two 128-workgroup scans at one epoch around the wrap (tests/scan_epoch_cases.py).

One failure that is KSH_INTERNAL or a HIP error ends the module: nothing more is started on the GPU."""
import inspect
import itertools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import byte_stream_cases as bsc
import plan_protocol_cases as cases
import scan_epoch_cases as sec
import test_gpu_bucket_sort
import test_gpu_byte_streams
import test_gpu_chain_rank
import test_gpu_cover_graphs
import test_gpu_decode_walk
import test_gpu_hash_tables
import test_gpu_index_geometry
import test_gpu_link_bubbles
import test_gpu_loop_families
import test_gpu_pair_tiles
import test_gpu_plan_protocol as pp
import test_gpu_probe
import test_gpu_seq_locate
import test_gpu_spss_cut
import test_gpu_spss_links
from kmersets import capi

pytestmark = pytest.mark.gpu

FILLS = (0x00, 0xFF, 0xA5)
POISON = 0xFF
GEOMS = cases.NARROW + cases.WIDE
GEOM_IDS = ["k%d-N%d-u%d" % (k, n, 8 * kb) for k, n, kb in GEOMS]


def filled_context(fill):
    ctx = capi.Context(0)
    if fill is not None:
        ctx.debug_scratch_fill(fill)
        assert ctx.debug_scratch_fill_stats() == (0, 0)
    pp.use(ctx)
    return ctx


def close_context(ctx):
    if not pp.STOP["why"]:
        import torch

        torch.cuda.synchronize()
        ctx.close()


@pytest.fixture(scope="module")
def store(gpu):
    return pp.Store(gpu)


# ---- (a) every entry point ---------------------------------------------------------------------------------------------
# The columns of the table on the context itself at the row's own width: the other width is another geometry's own
# column here, the second context another context's.
COLUMNS = [c for c in cases.INTRUDERS if c["where"] == "own" and c["width"] == "same"]
PARTS = ("calls", "plans", "large", "kss", "victims")

# The ops that take no scratch, with what they do instead (the entry points' own text); every other column must move
# the fill counters.
NO_SCRATCH = {
    "contains": "ksh_set_contains: one kernel from the caller's buffers to the caller's buffer",
    "kmers": "ksh_set_kmers: one kernel from the set to the caller's buffer",
    "copies": "ksh_ctx_memcpy_*: copies between the caller's buffers",
    "ctx_misc": "sync, timing and statistics: no launch",
    "lanes": "ksh_ctx_set_lanes: sets a number",
    "release:encode": "frees the plan's blocks",
    "release:cover": "frees the plan's blocks",
    "kss_index_close": "frees the indexes",
    "kss_destroy": "frees the structure",
}


def part_of(op):
    if op.startswith(("full:", "abandon:", "plain:")):
        return "plans"
    if op.startswith("large:"):
        return "large"
    if op.startswith("kss_") or op in cases.INDEX_OPS or op == "fail:select_keys":
        return "kss"
    return "calls"


def test_the_columns_are_the_tables():
    ops = {c["op"] for c in COLUMNS}
    assert ops == set(cases.OPS) and set(NO_SCRATCH) <= ops
    assert {part_of(c["op"]) for c in COLUMNS} == set(PARTS) - {"victims"}
    assert {"kss_build:lanes1", "kss_build:default"} <= ops


@pytest.mark.parametrize("part", PARTS)
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("fill", FILLS, ids=["fill%02X" % f for f in FILLS])
@pp.stops_module
def test_entry_points_on_filled_scratch(store, fill, geom, part):
    ctx = filled_context(fill)
    state, unmoved = {}, []
    try:
        if part == "victims":
            data = store.get(geom, "victim")
            for kind in cases.KINDS:
                for plain in ((False, True) if kind in cases.NAMELESS else (False,)):
                    before = ctx.debug_scratch_fill_stats()
                    v = pp.Victim(kind, data, ctx, plain=plain)
                    v.plan()
                    v.write()
                    v.check_exact()
                    if not ctx.debug_scratch_fill_stats()[0] > before[0]:
                        unmoved.append("%s%s" % (kind, "-plain" if plain else ""))
        for col in COLUMNS if part != "victims" else ():
            if part_of(col["op"]) != part:
                continue
            before = ctx.debug_scratch_fill_stats()
            pp.run_intruder(col, ctx, store, geom, state)()
            after = ctx.debug_scratch_fill_stats()
            assert after[0] >= before[0] and after[1] >= before[1]
            if col["op"] not in NO_SCRATCH and not (after[0] > before[0] and after[1] > before[1]):
                unmoved.append(col["id"])
            if col["op"] == "kss_build:default":
                print("lanes after %s: %d" % (col["id"], ctx.mem_stats()["n_lanes"]))
        assert not unmoved, "the fill counters did not move over: %s" % ", ".join(unmoved)
    finally:
        if not pp.STOP["why"]:
            import torch

            torch.cuda.synchronize()
            for kind in ("borrowed", "owned", "kss"):  # the indexes before the structures they borrow from
                for key in [key for key in state if isinstance(key, tuple) and key[0] == kind]:
                    state.pop(key).close()
        close_context(ctx)


# ---- (b) the route-bearing sweeps in child processes ---------------------------------------------------------------------
# Each child is started by its own module's test function -- argv, switches, time limit, case list and the coverage
# it asserts are that test's -- with KSH_SCRATCH_FILL in the environment it copies.  One child at a time; none after a
# failed one.
CHILDREN = [("decode_walk:" + name, test_gpu_decode_walk.test_decode_walk_child, name) for name in ("l2min", "direct")] + \
           [("chain_rank:" + knobs, test_gpu_chain_rank.test_other_routes_in_a_child, knobs)
            for knobs in test_gpu_chain_rank.CHILDREN] + \
           [("probe:" + switches, test_gpu_probe.test_other_routes_in_a_child, switches)
            for switches in test_gpu_probe.CHILDREN] + \
           [("loop_families:" + switch, test_gpu_loop_families.test_families_switch, switch)
            for switch in ("KSH_KSS_LOOP=ahead", "KSH_REWEIGH=full")]
_failed_children = []


def test_environment_sets_the_fill_in_a_child(gpu):
    """KSH_SCRATCH_FILL (decimal or 0x..) is read when a process makes its first context: in a child, the arena that
    ksh_ctx_create reserves is filled already; a value that is no byte leaves the fill off, and a fill turned off
    counts nothing."""
    assert not pp.STOP["why"], pp.STOP["why"]
    code = ("import conftest\nfrom kmersets import capi\nc = capi.Context(0)\nprint('fills', *c.debug_scratch_fill_stats())\n"
            "c.debug_scratch_fill(None)\nprint('off', *c.debug_scratch_fill_stats())\nc.svb_encode(__import__('numpy').arange(9, dtype='uint32'))\n"
            "print('off', *c.debug_scratch_fill_stats())\nc.close()\n")
    here = os.path.dirname(os.path.abspath(__file__))
    for value, want in (("0xFF", True), ("165", True), ("", False), ("256", False)):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KSH_SCRATCH_FILL=value), cwd=here,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [ln.split() for ln in r.stdout.splitlines()]
        fills, n_bytes = int(lines[0][1]), int(lines[0][2])
        assert lines[0][0] == "fills" and (fills >= 1 and n_bytes >= 8 << 20) == want and (fills == 0) != want, r.stdout
        assert lines[1] == ["off", "0", "0"] and lines[2] == ["off", "0", "0"], r.stdout  # off: no fill, no count


@pytest.mark.parametrize("name,start,arg", CHILDREN, ids=[c[0] for c in CHILDREN])
def test_worker_on_filled_scratch(gpu, monkeypatch, tmp_path, name, start, arg):
    assert not pp.STOP["why"], pp.STOP["why"]
    assert not _failed_children, "not started: the child before this one failed (%s)" % _failed_children
    capi.Context(0).close()  # (this process has read KSH_SCRATCH_FILL for itself before it is set for the children)
    monkeypatch.setenv("KSH_SCRATCH_FILL", "0x%02X" % POISON)
    kwargs = {"tmp_path": tmp_path} if "tmp_path" in inspect.signature(start).parameters else {}
    t0 = time.time()
    try:
        start(gpu, arg, **kwargs)
    except BaseException:
        _failed_children.append(name)
        raise
    finally:
        print("child %s under KSH_SCRATCH_FILL: %.1f s (its preparation on the host included)" % (name, time.time() - t0))


# ---- (c) the in-process sweeps, on a context filled with 0xFF --------------------------------------------------------------
# (module, its test functions), the four newest stages first.  Each function runs once per parameter set of its own
# module, with that module's fixtures made for this module's context.
SWEEPS = [
    (test_gpu_seq_locate, ["test_locate_vs_reference"]),
    (test_gpu_spss_links, ["test_links_vs_reference"]),
    (test_gpu_link_bubbles, ["test_bubbles_vs_reference"]),
    (test_gpu_spss_cut, ["test_cut_vs_reference"]),
    (test_gpu_hash_tables, ["test_count_side", "test_capacity_below_the_class_count", "test_lookup_side",
                            "test_paint_alternating_rows", "test_links", "test_tile_table"]),
    (test_gpu_pair_tiles, ["test_two_call_form", "test_one_call_form", "test_batch_form", "test_union_and_diff"]),
    (test_gpu_bucket_sort, ["test_bucket_sort_cases"]),
    (test_gpu_cover_graphs, ["test_cover_graphs"]),
    (test_gpu_index_geometry, ["test_index_cell"]),
    (test_gpu_byte_streams, ["test_svb_on_the_scan_route"]),
]


def parameter_sets(fn):
    """[(id, {argument: value})] of a test function, from its own parametrize marks."""
    axes = []
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [s.strip() for s in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        ids = mark.kwargs.get("ids")
        axis = []
        for i, value in enumerate(mark.args[1]):
            values = (value,) if len(names) == 1 else tuple(value)
            label = ids[i] if isinstance(ids, (list, tuple)) else ids(value) if callable(ids) else \
                "-".join(str(v) for v in values) if all(isinstance(v, (str, int, bool)) for v in values) else str(i)
            axis.append((str(label), dict(zip(names, values))))
        axes.append(axis)
    out = []
    for combo in itertools.product(*axes):
        merged = {}
        for _, kw in combo:
            merged.update(kw)
        out.append(("-".join(label for label, _ in combo), merged))
    return out


SWEEP_CALLS = [("%s::%s[%s]" % (mod.__name__[len("test_gpu_"):], name, pid), mod, name, kw)
               for mod, names in SWEEPS for name in names for pid, kw in parameter_sets(getattr(mod, name))]


def kw_id(kw):
    """The case's own id, where the parameter set has one."""
    return kw["name"] if isinstance(kw.get("name"), str) else kw["case"]["id"] if isinstance(kw.get("case"), dict) else None


# The cases with no strings: ksh_seq_locate, ksh_spss_links, ksh_link_bubbles and ksh_spss_cut return on the host
# before they allocate anything (their `n == 0` branches), so these calls take no scratch -- and must not.
NO_INPUT = {(test_gpu_seq_locate, "test_locate_vs_reference", "no-strings-k%d" % k) for k in (15, 16, 23, 31)} | \
           {(test_gpu_spss_links, "test_links_vs_reference", "empty-k23"),
            (test_gpu_link_bubbles, "test_bubbles_vs_reference", "no-strings"),
            (test_gpu_spss_cut, "test_cut_vs_reference", "empty-k23")}


class Fixtures:
    """The module-scoped fixtures of the sweeps' modules, made once for this module's context: `ctx` is the filled
    context, `gpu` its device, every other name the module's own fixture function."""

    def __init__(self, ctx):
        self.ctx, self.made, self.finish = ctx, {}, []

    def get(self, mod, name):
        if name == "ctx":
            return self.ctx
        if name == "gpu":
            return self.ctx.device
        if (mod, name) not in self.made:
            body = getattr(mod, name).__wrapped__
            value = body(*[self.get(mod, p) for p in inspect.signature(body).parameters])
            if inspect.isgenerator(value):
                gen, value = value, next(value)
                self.finish.append(gen)
            self.made[(mod, name)] = value
        return self.made[(mod, name)]

    def close(self):
        for gen in reversed(self.finish):
            next(gen, None)


@pytest.fixture(scope="module")
def poisoned(gpu):
    ctx = filled_context(POISON)
    fx = Fixtures(ctx)
    yield fx
    if not pp.STOP["why"]:
        import torch

        torch.cuda.synchronize()
        fx.close()
    close_context(ctx)


def test_the_sweeps_have_their_cases():
    counts = {}
    for _, mod, name, _ in SWEEP_CALLS:
        counts[(mod.__name__, name)] = counts.get((mod.__name__, name), 0) + 1
    assert len(counts) == sum(len(names) for _, names in SWEEPS) and all(n >= 2 for n in counts.values()), counts
    assert counts[("test_gpu_seq_locate", "test_locate_vs_reference")] == 2 * len(test_gpu_seq_locate.cases.CASES)
    assert counts[("test_gpu_byte_streams", "test_svb_on_the_scan_route")] == 3
    assert NO_INPUT <= {(mod, name, kw_id(kw)) for _, mod, name, kw in SWEEP_CALLS}
    for mod, name, cid in NO_INPUT:  # (they are the cases without strings)
        case = next(kw["case"] for _, m, f, kw in SWEEP_CALLS if (m, f, kw_id(kw)) == (mod, name, cid))
        assert len(case["strings"]) == 0 if "strings" in case else case["n"] == 0
    assert counts[("test_gpu_index_geometry", "test_index_cell")] == len(test_gpu_index_geometry.cells.CASES)


@pytest.mark.parametrize("mod,name,kw", [c[1:] for c in SWEEP_CALLS], ids=[c[0] for c in SWEEP_CALLS])
@pp.stops_module
def test_sweep_on_filled_scratch(poisoned, mod, name, kw):
    ctx = poisoned.ctx
    pp.use(ctx)
    fn = getattr(mod, name)
    args = {p: kw[p] if p in kw else poisoned.get(mod, p) for p in inspect.signature(fn).parameters}
    before = ctx.debug_scratch_fill_stats()
    keep = dict(test_gpu_index_geometry.TABLE)  # (test_index_cell notes its routes there for its own module's table)
    try:
        fn(**args)
    finally:
        test_gpu_index_geometry.TABLE.clear()
        test_gpu_index_geometry.TABLE.update(keep)
    after = ctx.debug_scratch_fill_stats()
    if (mod, name, kw_id(kw)) in NO_INPUT:
        assert after == before
    else:
        assert after[0] > before[0] and after[1] > before[1], "the sweep took no scratch"


# ---- the epoch wrap ----------------------------------------------------------------------------------------------------------
_EPOCH = {}


def epoch_inputs():
    """(n, values, reference bytes) of the big zero encode, the big mixed one and the small one, made once."""
    if not _EPOCH:
        c = bsc.constants()
        big, blocks_big, small, blocks_small = sec.geometry(c)
        assert (blocks_big, blocks_small) == (c.chain_blocks, 3)
        zeros = np.zeros(4 * big, dtype=np.uint32)
        mixed = bsc.svb_values(bsc.Svb("epoch-big", 4 * big, "widths", 5))
        little = bsc.svb_values(bsc.Svb("epoch-small", 4 * small - 1, "widths", 6))
        for v in (mixed, little):  # 0-, 1-, 2- and 4-byte values
            assert {int(x) for x in np.unique(np.where(v == 0, 0, np.where(v < 256, 1, np.where(v < 65536, 2, 4))))} == {0, 1, 2, 4}
        for name, v in (("zeros", zeros), ("mixed", mixed), ("small", little)):
            assert bsc.scan_route((v.size + 3) // 4, c) == "chained"
            _EPOCH[name] = (v.size, v, bsc.svb_encode(v))
    return _EPOCH


@pytest.mark.parametrize("fill", [None, POISON], ids=["no-fill", "fillFF"])
@pp.stops_module
def test_scan_epoch_wrap(gpu, fill):
    """A 128-workgroup encode of zeros at epoch E (every published sum is 0: a stale prefix can only be too small, and
    a broken wrap writes wrong bytes inside the buffer, never past it); the epoch set to just below 0xFFFF; the smallest
    chained encodes across the wrap up to E - 1; the 128-workgroup encode of mixed values at E, and its decode."""
    import torch

    bs = test_gpu_byte_streams
    inputs = epoch_inputs()
    ctx = filled_context(fill)
    try:
        dev = {name: torch.from_numpy(v.view(np.int32).copy()).to(ctx.device) for name, (_, v, _) in inputs.items()}

        def encode(name):
            n, _, want = inputs[name]
            return bs.svb_encode_guarded(ctx, name, dev[name], n, want)

        def decode(name, d_out):
            n, _, want = inputs[name]
            bs.svb_decode_guarded(ctx, name, d_out, dev[name], n, want)

        # how many chained scans an encode and a decode take: read, not assumed
        e0 = ctx.debug_scan_epoch()
        d_out = encode("small")
        e1 = ctx.debug_scan_epoch()
        decode("small", d_out)
        e2 = ctx.debug_scan_epoch()
        per_encode, per_decode = e1 - e0, e2 - e1
        assert per_encode >= 1 and per_decode >= 1, "the encode or the decode did not take the chained scan"
        encode("zeros")
        epoch_big = ctx.debug_scan_epoch() - per_encode + 1  # the epoch of its first scan
        assert epoch_big == e2 + 1
        seen = []
        for step in sec.plan(epoch_big, per_encode):
            if step[0] == "set":
                assert ctx.debug_scan_epoch(set_to=step[1]) == step[1]
            elif step[0] == "small":
                encode("small")
                seen.append(ctx.debug_scan_epoch())
            else:
                assert sec.next_epoch(ctx.debug_scan_epoch())[0] == epoch_big, "the second big encode is not at E"
                d_out = encode("mixed")
                assert ctx.debug_scan_epoch() == epoch_big + per_encode - 1
                decode("mixed", d_out)
        # the wrap happened, once, between the two big launches
        drops = [i for i in range(1, len(seen)) if seen[i] < seen[i - 1]]
        assert len(drops) == 1 and seen[drops[0] - 1] > sec.EPOCH_MASK - per_encode and seen[drops[0]] <= per_encode, seen
        assert seen[-1] == epoch_big - 1
        if fill is not None:
            assert ctx.debug_scratch_fill_stats()[0] > 0
    finally:
        close_context(ctx)

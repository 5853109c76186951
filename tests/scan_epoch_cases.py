"""The epoch of the chained scan (csrc/ksh_scan.h) across its wrap, as a model and a launch plan (no GPU needed).

scan_exclusive_chained never clears ctx->scan_state: a published sum carries the launch's 16-bit epoch, and after
65 535 launches the epoch wraps; the launch that would take epoch 0 clears the array and takes 1.  If that clear were
missing, or ordered wrongly on the stream, a launch at epoch E after the wrap would accept what a launch at epoch E
before the wrap left in the slots nobody has written since.  plan() places two launches of kChainMaxBlocks workgroups
so: the first at E, the epoch then set (ksh_debug_scan_epoch) to just below 0xFFFF, launches of as few workgroups as a
chained scan can have across the wrap and up to E - 1, the second at E.

The public operation over the scan is ksh_svb_encode_0124 / ksh_svb_decode_0124: (n + 3) / 4 groups, one value of
the scan per group, kChainTile groups per workgroup.  Up to kScanSmallMax values scan_exclusive_i64 takes its
one-workgroup kernel, which has no epoch: the smallest chained scan has kScanSmallMax + 1 values, that is
SMALL_BLOCKS = 3 workgroups, and leaves the slots from SMALL_BLOCKS on as they were.

tests/test_scan_epoch_model_cpu.py asserts what the plan claims; tests/test_gpu_scratch_fill.py runs it."""
import byte_stream_cases as bsc

EPOCH_MASK = 0xFFFF
BEFORE_WRAP = 2  # launches between the set epoch and 0xFFFF, the one at 0xFFFF included


def next_epoch(e):
    """(the epoch the next chained launch runs at, whether it clears the state first): scan_exclusive_chained."""
    e = (e + 1) & EPOCH_MASK
    return (1, True) if e == 0 else (e, False)


def geometry(c=None):
    """(groups of the big launch, its workgroups, groups of the small launch, its workgroups)."""
    c = c or bsc.constants()
    big = c.chain_tile * c.chain_blocks
    small = c.scan_small + 1
    blocks = lambda groups: (groups + c.chain_tile - 1) // c.chain_tile  # noqa: E731
    assert bsc.scan_route(big, c) == "chained" and bsc.scan_route(small, c) == "chained"
    assert bsc.scan_route(small - 1, c) == "small"
    return big, blocks(big), small, blocks(small)


def plan(epoch_big, scans_per_encode=1):
    """The steps behind the first big encode, which ran its (last) scan at epoch_big: ("set", epoch), ("small",) --
    one encode of the small size -- and, last, ("big",).  An encode takes scans_per_encode chained scans, the last
    big one must run its first at epoch_big again."""
    assert 1 <= epoch_big < EPOCH_MASK - BEFORE_WRAP * scans_per_encode and scans_per_encode >= 1
    # (whole encodes from the set epoch to epoch_big - 1: the launches up to 0xFFFF and the epoch_big - 1 behind it)
    steps = [("set", EPOCH_MASK - BEFORE_WRAP * scans_per_encode - (1 - epoch_big) % scans_per_encode)]
    e = steps[0][1]
    wrapped = False
    while True:
        # the epochs the next encode would take
        took, x = [], e
        for _ in range(scans_per_encode):
            x, cleared = next_epoch(x)
            took.append((x, cleared))
        if took[0][0] == epoch_big and (wrapped or took[0][1]):
            break
        assert not wrapped or took[-1][0] < epoch_big, "the small encodes step over the epoch of the big one"
        steps.append(("small",))
        wrapped = wrapped or any(cleared for _, cleared in took)
        e = x
    steps.append(("big",))
    return steps


def replay(epoch_big, steps, blocks_big, blocks_small, scans_per_encode=1):
    """The launches of the plan as (epoch, workgroups, cleared first), the first big encode's last scan in front."""
    launches = [(epoch_big, blocks_big, False)]
    e = epoch_big
    for step in steps:
        if step[0] == "set":
            e = step[1]
            continue
        for _ in range(scans_per_encode):
            e, cleared = next_epoch(e)
            launches.append((e, blocks_big if step[0] == "big" else blocks_small, cleared))
    return launches

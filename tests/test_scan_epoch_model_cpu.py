"""The launch plan of tests/scan_epoch_cases.py against the rule of scan_exclusive_chained (csrc/ksh_scan.h), which it
restates: two launches of kChainMaxBlocks workgroups at one epoch, one on either side of exactly one wrap, and between
them only launches of the fewest workgroups a chained scan can have -- so that the second finds, in every slot from
there on, what the first published, unless the wrap cleared it."""
import os
import re

import pytest

import byte_stream_cases as bsc
import scan_epoch_cases as sec

SCAN_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kmer-sets-compression_amd", "csrc", "ksh_scan.h")


def test_the_rule_is_the_kernel_text():
    """next = (e + 1) & 0xFFFF; 0 -> clear, 1: the lines of scan_exclusive_chained, and the tag's 16 bits."""
    text = open(SCAN_H).read()
    for line in ("ctx->scan_epoch = (ctx->scan_epoch + 1) & 0xFFFF;", "if (ctx->scan_epoch == 0) {",
                 "ctx->scan_epoch = 1;", "constexpr int kChainValueBits = 48;"):
        assert text.count(line) == 1, line
    clear = re.search(r"hipMemsetAsync\(ctx->scan_state, 0, size_t\(2 \* kChainMaxBlocks\) \* sizeof\(unsigned long long\), "
                      r"ctx->stream\);\s*ctx->scan_epoch = 1;", text)
    assert clear, "the wrap no longer clears the whole state on the context's stream"
    assert text.index("ctx->scan_epoch == 0") < clear.start() < text.index("hipLaunchKernelGGL((k_scan_chained")
    assert sec.EPOCH_MASK == (1 << (64 - 48)) - 1
    assert sec.next_epoch(0) == (1, False) and sec.next_epoch(5) == (6, False)
    assert sec.next_epoch(0xFFFE) == (0xFFFF, False) and sec.next_epoch(0xFFFF) == (1, True)
    seen, e = set(), 0
    for _ in range(sec.EPOCH_MASK):  # 65 535 launches take 65 535 different epochs, never 0
        e, _ = sec.next_epoch(e)
        seen.add(e)
    assert len(seen) == sec.EPOCH_MASK and 0 not in seen and sec.next_epoch(e) == (1, True)


def test_geometry_from_the_kernel_text():
    c = bsc.constants()
    text = open(SCAN_H).read()
    num = lambda name: int(re.search(r"constexpr (?:int|int64_t) %s = (\d+);" % name, text).group(1))  # noqa: E731
    assert c.chain_tile == num("kChainThreads") * num("kChainItems") and c.chain_blocks == num("kChainMaxBlocks")
    big, blocks_big, small, blocks_small = sec.geometry(c)
    assert blocks_big == c.chain_blocks == 128 and big == 128 * 2048
    # a scan of one workgroup's worth of values never reaches the chained kernel: the fewest workgroups are 3
    assert bsc.scan_route(c.chain_tile, c) == "small" and blocks_small == 3 < blocks_big


@pytest.mark.parametrize("scans", [1, 2])
@pytest.mark.parametrize("epoch_big", [1, 2, 3, 7, 200])
def test_plan_puts_both_big_launches_at_one_epoch_around_one_wrap(epoch_big, scans):
    _, blocks_big, _, blocks_small = sec.geometry()
    steps = sec.plan(epoch_big, scans)
    assert steps[0][0] == "set" and steps[-1] == ("big",) and all(s == ("small",) for s in steps[1:-1])
    launches = sec.replay(epoch_big, steps, blocks_big, blocks_small, scans)
    first, second = launches[0], launches[-scans]
    assert first[:2] == second[:2] == (epoch_big, blocks_big)
    between = launches[1:-scans]
    assert between and all(blocks == blocks_small for _, blocks, _ in between)
    assert sum(cleared for _, _, cleared in launches) == 1 and sum(cleared for _, _, cleared in between) == (epoch_big > 1)
    epochs = [e for e, _, _ in launches[1:]]
    assert sec.EPOCH_MASK in epochs and epochs[epochs.index(sec.EPOCH_MASK) + 1] == 1  # the wrap itself
    # no launch between the two wrote a slot from blocks_small on, and none of them ran at the big one's epoch
    assert all(e != epoch_big for e, _, _ in between)
    # (epoch_big == 1: the second big launch is the clearing one -- the clear is then ordered before it on the stream)
    assert second[2] == (epoch_big == 1)

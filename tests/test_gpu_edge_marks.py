"""GPU parity tests for the edge search of the SPSS encode (k_edges, csrc/ksh_encode.hip): a unitig side that never
had a neighbour stores its four `none` without a search, told from a side whose link k_link_cut took away by the cut
marks.  Every set of tests/edge_marks_cases.py is encoded twice -- by default, and with KSH_EDGES=search (every side
searches, no marks kept) -- and both give the oracle's strings, string for string and in order.  The library reads
the switch once, so each value runs in a fresh child process that encodes all the sets."""
import json
import os
import subprocess
import sys

import pytest

import edge_marks_cases as emc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_CHILD = (
    "import json, sys\n"
    "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import edge_marks_cases as emc\n"
    "from kmersets import capi\n"
    "ctx = capi.Context(0)\n"
    "out = {}\n"
    "for (name, k, n, kb, kmers, canonical, mode, _) in emc.cases():\n"
    "    d = capi.DeviceSet.from_kmers(capi.geom(k, n), kmers, ctx.device)\n"
    "    assert d.g.key_bytes == kb, (name, d.g.key_bytes)\n"
    "    out[name] = ctx.spss_encode(d, mode=mode, canonical=canonical).to_strings()\n"
    "ctx.close()\n"
    "json.dump(out, open(sys.argv[1], 'w'))\n"
    "print('edge marks ok')\n"
) % (os.path.join(_HERE, "..", "kmer-sets-compression_amd"), _HERE)

_CASES = emc.cases()
_SWITCHES = ("default", "search")


@pytest.fixture(scope="module")
def encoded(gpu, tmp_path_factory):
    """{switch: {case: strings}}: one child process per value of KSH_EDGES."""
    got = {}
    for switch in _SWITCHES:
        path = str(tmp_path_factory.mktemp("edge_marks") / (switch + ".json"))
        env = {key: v for key, v in os.environ.items() if key != "KSH_EDGES"}
        if switch == "search":
            env["KSH_EDGES"] = "search"
        r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "edge marks ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
        with open(path) as f:
            got[switch] = json.load(f)
    return got


@pytest.fixture(scope="module")
def oracle():
    """{case: the oracle's strings}, computed once."""
    want = {}
    for (name, k, n, kb, kmers, canonical, mode, method) in _CASES:
        want[name] = getattr(ol.Set.from_kmers(k, n, kb, kmers), method)()
    return want


@pytest.mark.parametrize("switch", _SWITCHES)
@pytest.mark.parametrize("name", [c[0] for c in _CASES])
def test_edges_with_and_without_the_search(encoded, oracle, name, switch):
    want = oracle[name]
    assert len(want) >= 1
    assert encoded[switch][name] == want, (name, switch)


def test_cases_cover_the_issue():
    """Chains, forks, remainder and intersection at the three key widths; the loop, a directed set and fast = false."""
    names = [c[0] for c in _CASES]
    assert len(set(names)) == len(names) == 19
    assert {(c[1], c[2], c[3]) for c in _CASES[:15]} == {(23, 14, 4), (15, 14, 2), (31, 14, 8)}
    assert all(2000 <= c[4].size <= 20000 for c in _CASES)
    assert sum(not c[5] for c in _CASES) == 1 and sum(c[6] == 2 for c in _CASES) == 2

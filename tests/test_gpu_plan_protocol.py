"""The protocol between a `*_plan` call and its `*_write` under interleaved calls (include/kmersets_hip.h, "Plans").

Every cell of tests/plan_protocol_cases.py runs the same way: plan the victim, fill its output buffers with a
sentinel byte, run the intruder, write, check.  An `exact` cell asserts KSH_OK and the full outputs; a `refused`
cell asserts KSH_FAILED_PRECONDITION, a message that names the missing plan, every sentinel byte intact, and then
the truth from a fresh plan + write on the same context.  In both, what the intruder produced is checked after the
victim's write.  The truth never comes from the library: numpy set operations with synth.to_bucketed, the oracle's
strings, geometry_families.kmers_of_strings, np.unique, Python string joins and splits.  Bit-exact throughout.

The columns include the ten calls that take their request first and an index or the context behind it (sequence
hits, pair counts, selections, colour classes, class ids, class runs, cut, links, bubbles), on the index that borrows
a built structure and on the one that owns its sets, with their failing variants; their truth is
tests/index_reference.py, tests/paint_reference.py and the references of the cut, the links and the bubbles.
test_two_call_requests_keep_no_state shows beside the table that the count / fill forms of those calls keep nothing
in the library between the two calls.

One context serves a victim row (accumulated state is the point); once any call returns KSH_INTERNAL or a HIP
error shows, every remaining cell fails without touching the GPU."""
import ctypes as C
import time

import numpy as np
import pytest

import geometry_families as gf
import link_bubbles_reference as bubbles_ref
import oracle_lib as ol
import plan_protocol_cases as cases
import spss_cut_reference as cut_ref
import spss_links_reference as links_ref
from kmersets import capi, synth

pytestmark = pytest.mark.gpu
U = np.uint64
SENTINEL = 0xA5
TAIL = 64            # sentinel bytes behind every output buffer: a write sized by another plan shows there too
STOP = {"why": None}  # set once: KSH_INTERNAL or a HIP error anywhere ends the module
OUTCOMES = {}        # (victim id, intruder id) -> observed outcome
WALL = {}
T0 = time.time()


def guard():
    if STOP["why"]:
        pytest.fail("stopped: " + STOP["why"])


def stop_on_internal(exc):
    if isinstance(exc, capi.KshError):
        if exc.code == capi.KSH_INTERNAL:
            STOP["why"] = str(exc)
    elif not isinstance(exc, AssertionError) and ("HIP" in str(exc) or "hip" in str(exc)):
        STOP["why"] = str(exc)


def stops_module(test):
    """For the tests beside the table: whatever they raise goes through stop_on_internal, so that a KSH_INTERNAL or
    a HIP error met in a bare plan, write or check ends the module as one met in a table cell does."""
    import functools

    @functools.wraps(test)
    def wrapped(*args, **kwargs):
        guard()
        try:
            return test(*args, **kwargs)
        except BaseException as e:  # noqa: B902
            stop_on_internal(e)
            raise
    return wrapped


# ---- data ------------------------------------------------------------------------------------------------------
def fasta_of(reads):
    return "".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads))


def reads_with_n(k, seed, n_reads=120):
    """Reads over ACGTN from a small genome (every k-mer seen several times), some fragments shorter than K."""
    bases = synth.random_genome(3000, 0x5EED0000 + seed)
    starts = (synth.mix64(np.arange(n_reads, dtype=U) + U(seed)) % U(bases.size - 150)).astype(np.int64)
    reads = []
    for i, p in enumerate(starts):
        r = synth.string_of_bases(bases[p:p + 150])
        if i % 3 == 0:
            cut = 20 + (i * 7) % 100
            r = r[:cut] + "N" + r[cut + 1:]
        if i % 10 == 0:
            r = r[:5] + "N" + r[6:]  # a leading fragment shorter than K
        reads.append(r)
    return reads


class Data:
    """Host truth and device inputs of one geometry: a pair of sets, the oracle's strings and unitigs of the first,
    reads, text and FASTA.  Made once per (geometry, seed); the device tensors are shared by all contexts."""

    def __init__(self, geom, seed, device, size=cases.VICTIM_KMERS, empty=False):
        import torch

        k, n, kb = geom
        self.geom, self.k, self.g = geom, k, capi.geom(k, n, kb)
        assert self.g.key_bytes == kb
        if empty:
            a = np.zeros(0, dtype=U)
            b = synth.phylogeny_sets(k, 1, size, seed=seed)[0]
            self.spss, self.unitigs, reads = [], [], []
        else:
            a, b = synth.phylogeny_sets(k, 2, size, seed=seed, rate=0.02)
            oset = ol.Set.from_kmers(k, *gf.ref_geom(k), a)
            self.spss, self.unitigs = oset.spss(), oset.unitigs()
            reads = reads_with_n(k, seed)
        self.a, self.b = np.asarray(a, dtype=U), np.asarray(b, dtype=U)
        self.dA = capi.DeviceSet.from_kmers(self.g, self.a, device)
        self.dB = capi.DeviceSet.from_kmers(self.g, self.b, device)
        self.sp = capi.DeviceSpss.from_strings(self.g, self.spss, device)
        self.dU = capi.DeviceSpss.from_strings(self.g, self.unitigs, device)
        self.dec_truth = gf.kmers_of_strings(self.spss, k, canonical=True)
        # reads -> fragments (split at N, at least K long) -> counted canonical k-mers
        self.reads = reads
        self.frags = [f for r in reads for f in r.split("N") if len(f) >= k]
        self.dF = capi.DeviceSpss.from_strings(self.g, self.frags, device)
        if self.frags:
            allk = np.concatenate([synth.canonical(synth.kmers_of_bases(synth.bases_of_string(f), k), k) for f in self.frags])
            self.uniq, self.cnt = np.unique(allk, return_counts=True)
        else:
            self.uniq, self.cnt = np.zeros(0, dtype=U), np.zeros(0, dtype=np.int64)
        self.text = "".join(s + "\n" for s in self.spss)
        self.fasta = fasta_of(reads)
        to_dev = lambda s: torch.from_numpy(np.frombuffer(s.encode(), dtype=np.uint8).copy()).to(device)  # noqa: E731
        self.d_text, self.d_fasta = to_dev(self.text), to_dev(self.fasta)
        torch.cuda.synchronize()


def upload(a, device, dtype=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).copy()).to(device)


class IndexData:
    """The host truth of the index ops at one geometry (cases.index_case) and their device inputs: the sequences, and
    the bucket offsets of both requests as the reference gives them."""

    def __init__(self, geom, device):
        import torch

        k, n, kb = geom
        self.geom, self.k, self.g, self.h = geom, k, capi.geom(k, n, kb), cases.index_case(geom)
        self.dseqs = capi.DeviceSpss.from_strings(self.g, self.h["strings"], device)
        self.select_off = {name: upload(self.h["select"][name][1], device) for name in "AB"}
        self.ids_off = {name: upload(self.h["class_ids"][name][2], device) for name in "AB"}
        torch.cuda.synchronize()


class StringData:
    """The containers, run lists and graphs of the cut, links and bubbles ops at one geometry, their malformed
    variants, and the references' answers."""

    def __init__(self, geom, device):
        import torch

        k, n, kb = geom
        self.geom, self.k, self.g = geom, k, capi.geom(k, n, kb)
        c = cases.cut_case(k)
        self.cut = {"seqs": capi.DeviceSpss.from_strings(self.g, c["strings"], device),
                    "off": upload(c["offsets"], device), "start": upload(c["start"], device),
                    "bad_off": upload(cases.descending_offsets(c), device),
                    "want": cut_ref.cut(c["strings"], k, c["offsets"], c["start"])}
        self.cut["words"] = synth.pack_strings(self.cut["want"][0], k)[0]
        self.links = {}
        for which in "AB":
            strings = cases.links_case(k, which)
            self.links[which] = {"seqs": capi.DeviceSpss.from_strings(self.g, strings, device),
                                 "want": links_ref.links(strings, k, True)}
        self.repeated_end = capi.DeviceSpss.from_strings(self.g, cases.repeated_end(k), device)
        off, to, max_arm, cls, rows = cases.bubbles_case(kb)
        self.graph = {"off": upload(off, device), "to": upload(to, device), "bad_to": upload(cases.no_twin(kb), device),
                      "cls": upload(cls, device, np.int32), "rows": rows,
                      "max_arm": {"A": max_arm, "B": cases.BUBBLES_MAX_ARM_B}}
        self.bubbles = {w: bubbles_ref.bubbles(off, to, m, cls, rows) for w, m in self.graph["max_arm"].items()}
        torch.cuda.synchronize()


class Store:
    """Everything that is computed once per module."""

    def __init__(self, device):
        self.device, self.data, self.kss, self.extra = device, {}, {}, {}

    def get(self, geom, role, empty=False):
        key = (geom, role, empty)
        if key not in self.data:
            seed = {"victim": 1000, "intruder": 2000}[role] + geom[0] + geom[1]
            self.data[key] = Data(geom, seed, self.device, empty=empty)
        return self.data[key]

    def kss_inputs(self, geom):
        if geom not in self.kss:
            k, n, kb = geom
            g = capi.geom(k, n, kb)
            sets, strings = cases.kss_sets(k), cases.kss_strings(k)
            comps = [capi.DeviceSpss.from_strings(g, st, self.device) for st in strings]
            rng = np.random.default_rng(k)
            q = np.concatenate([rng.choice(s, size=200, replace=False) for s in sets] +
                               [rng.integers(0, 1 << (2 * k), size=200, dtype=np.uint64)]).astype(U)
            self.kss[geom] = {"sets": sets, "comps": comps, "ids": synth.sample_bucket_ids(n, seed=5), "q": q}
        return self.kss[geom]

    def index_data(self, geom):
        if ("index", geom) not in self.extra:
            self.extra[("index", geom)] = IndexData(geom, self.device)
        return self.extra[("index", geom)]

    def string_data(self, geom):
        if ("strings", geom) not in self.extra:
            self.extra[("strings", geom)] = StringData(geom, self.device)
        return self.extra[("strings", geom)]

    def large(self):
        """~2 * 10^6 k-mers: a pair of sets and strings with as many k-mers, at (23, 14, u32)."""
        if "large" not in self.extra:
            import torch

            k, n, kb = 23, 14, 4
            g = capi.geom(k, n, kb)
            a, b = synth.phylogeny_sets(k, 2, cases.LARGE_KMERS, seed=9, rate=0.02)
            a, b = np.asarray(a, dtype=U), np.asarray(b, dtype=U)
            bases = synth.random_genome(cases.LARGE_KMERS + 2000 * (k - 1), 0xBA5E)
            step = bases.size // 2000
            strings = [synth.string_of_bases(bases[i:i + step]) for i in range(0, step * 2000, step)]
            text = "".join(s + "\n" for s in strings)
            self.extra["large"] = {
                "g": g, "k": k, "a": a, "b": b, "strings": strings, "text": text,
                "dA": capi.DeviceSet.from_kmers(g, a, self.device), "dB": capi.DeviceSet.from_kmers(g, b, self.device),
                "sp": capi.DeviceSpss.from_strings(g, strings, self.device),
                "d_text": torch.from_numpy(np.frombuffer(text.encode(), dtype=np.uint8).copy()).to(self.device),
                "sets": [synth.to_bucketed(x, k, n, kb) for x in (np.intersect1d(a, b), np.setdiff1d(a, b), np.setdiff1d(b, a))],
                "dec": synth.to_bucketed(gf.kmers_of_strings(strings, k, canonical=True), k, n, kb),
                "packed": synth.pack_strings(strings, k)}
            self.extra["large"]["results"] = (np.intersect1d(a, b), np.setdiff1d(a, b), np.setdiff1d(b, a))
            torch.cuda.synchronize()
        return self.extra["large"]

    def large_pair(self, n_bits):
        """The large pair at N = n_bits: ctx->plan is sized by the bucket count first (at least one tile per bucket,
        and plan_reserve keeps a quarter spare), so only more buckets than a row has seen make it grow."""
        key = ("large_pair", n_bits)
        if key not in self.extra:
            import torch

            lg = self.large()
            g = capi.geom(lg["k"], n_bits, 4)
            self.extra[key] = {"dA": capi.DeviceSet.from_kmers(g, lg["a"], self.device),
                               "dB": capi.DeviceSet.from_kmers(g, lg["b"], self.device),
                               "sets": [synth.to_bucketed(x, lg["k"], n_bits, 4) for x in lg["results"]]}
            torch.cuda.synchronize()
        return self.extra[key]

    def palindromic(self):
        """An even-k canonical set that holds a k-mer equal to its own reverse complement (the encode refuses it)."""
        if "pal" not in self.extra:
            k, n = 16, 14
            x = gf.family("genome", k, 5000, seed=3)
            h = x[:1] >> U(k)
            pal = (h << U(k)) | synth.revcomp(h, k // 2)
            assert gf.self_rc(pal, k).all()
            g = capi.geom(k, n)
            self.extra["pal"] = capi.DeviceSet.from_kmers(g, np.union1d(x, pal), self.device)
        return self.extra["pal"]

    def overdeclared(self, geom):
        """A container view that declares 64 bases more than its strings hold; d_words is allocated (and zero) for
        the declared count, so whatever reads by n_bases stays inside the buffer."""
        key = ("over", geom)
        if key not in self.extra:
            import torch

            d = self.get(geom, "intruder")
            words, lens = synth.pack_strings(d.spss, d.k)
            declared = d.sp.n_bases + 64
            w = torch.zeros((declared + 31) // 32 + 1, dtype=torch.int64, device=self.device)
            w[: words.size] = torch.from_numpy(words.view(np.int64).copy()).to(self.device)
            self.extra[key] = capi.DeviceSpss(d.g, w, d.sp.lens, d.sp.n_strings, declared)
        return self.extra[key]


@pytest.fixture(scope="module")
def store(gpu):
    t0 = time.time()
    s = Store(gpu)
    yield s
    WALL["module"] = time.time() - t0


# ---- the two contexts of a row ------------------------------------------------------------------------------------
def use(ctx):
    """torch's allocations, fills and copies go to torch's current stream, the library's kernels to the context's:
    one context at a time, everything drained in between."""
    import torch

    torch.cuda.synchronize()
    torch.cuda.set_stream(ctx.stream)


def sentinel(nbytes, device):
    import torch

    return torch.full((int(nbytes) + TAIL,), SENTINEL, dtype=torch.uint8, device=device)


def all_sentinel(buf):
    import torch

    return bool((buf.view(torch.uint8) == SENTINEL).all().item())


# ---- victims -----------------------------------------------------------------------------------------------------
class Victim:
    """One plan / write pair on one Data: plan(), write(), check_exact(), check_untouched()."""

    CUTOFF = 2

    def __init__(self, kind, data, ctx, plain=False):
        self.kind, self.d, self.ctx, self.p, self.plain = kind, data, ctx, None, plain
        self.bufs, self.result, self.snap = [], None, None

    def spss_truth(self):
        d = self.d
        return {"encode": d.spss, "cover": d.spss, "from_text": d.spss, "fasta": d.frags}[self.kind]

    def plan(self):
        import torch

        d, ctx, dev = self.d, self.ctx, self.ctx.device
        kb = d.g.key_bytes
        if self.kind == "pair":
            self.outs = [capi.DeviceSet.empty_like_offsets(d.g, 0, dev) for _ in range(3)]
            totals = ctx.pair_plan(d.dA, d.dB, *self.outs)
            want = [np.intersect1d(d.a, d.b), np.setdiff1d(d.a, d.b), np.setdiff1d(d.b, d.a)]
            assert totals == [w.size for w in want]
            self.truth = want
            for o, t in zip(self.outs, totals):
                o.n_keys, o.keys = t, sentinel(max(t * kb, 16), dev)
            self.bufs = [o.keys for o in self.outs]
            self.snap = [o.offsets.clone() for o in self.outs]
        elif self.kind == "union":
            self.p = ctx.set_union_plan(d.dA, d.dB)
            self.truth = np.union1d(d.a, d.b)
            assert self.p.n_keys == self.truth.size
            self.bufs = [sentinel(max(self.p.n_keys * kb, 16), dev)]
            self.snap = [self.p.out.offsets.clone()]
        elif self.kind in ("decode", "count"):
            sp = d.sp if self.kind == "decode" else d.dF
            strings = d.spss if self.kind == "decode" else d.frags
            self.p = ctx.spss_decode_plan(sp, canonical=True)
            assert self.p.n_keys == sum(len(s) - d.k + 1 for s in strings)
            self.bufs = [sentinel(max(self.p.n_keys * kb, 16), dev)]
            self.snap = [self.p.out.offsets.clone()]
        else:
            if self.kind == "encode":
                self.p = ctx.spss_encode_plan(d.dA, mode=0, canonical=True)
            elif self.kind == "cover":
                self.p = ctx.spss_cover_plan(d.dU, canonical=True, fast=True)
            elif self.kind == "from_text":
                self.p = ctx.spss_from_text_plan(d.g, d.d_text)
            else:
                self.p = ctx.fasta_plan(d.g, d.d_fasta)
            want = self.spss_truth()
            assert (self.p.n_strings, self.p.n_bases) == (len(want), sum(len(s) for s in want))
            self.n_words = (self.p.n_bases + 31) // 32
            words = sentinel(max(self.n_words, 1) * 8, dev).view(torch.int64)
            lens = sentinel(max(self.p.n_strings, 1) * 4, dev).view(torch.int32)
            self.bufs = [words, lens]

    def write(self, ctx=None):
        ctx = ctx or self.ctx
        d = self.d
        if self.kind == "pair":
            ctx.pair_write(d.dA, d.dB, *self.outs)
        elif self.kind == "union":
            self.result = ctx.set_union_write(self.p, keys=self.bufs[0])
        elif self.kind == "decode":
            self.result = ctx.spss_decode_write(self.p, keys=self.bufs[0])
        elif self.kind == "count":
            self.result = ctx.kmer_count_write(self.p, self.CUTOFF, keys=self.bufs[0])
        else:
            fn = {"encode": ctx.spss_encode_write, "cover": ctx.spss_cover_write,
                  "from_text": ctx.spss_from_text_write, "fasta": ctx.fasta_write}[self.kind]
            self.result = fn(self.p, words=self.bufs[0], lens=self.bufs[1], plain=self.plain)

    def _check_set(self, offsets, keys_buf, n_keys, kmers):
        g = self.d.g
        want_off, want_keys = synth.to_bucketed(kmers, g.k, g.n_bucket_bits, g.key_bytes)
        assert n_keys == kmers.size
        assert np.array_equal(offsets.cpu().numpy(), want_off)
        raw = keys_buf.cpu().numpy()
        nbytes = kmers.size * g.key_bytes
        assert np.array_equal(raw[:nbytes].view(capi.KEY_DTYPE[g.key_bytes]), want_keys)
        # (the decode's and the counter's buffer holds one slot per k-mer occurrence: what lies between the kept
        # keys and its end is the write's to use; the sentinel tail starts behind the capacity)
        assert (raw[raw.size - TAIL:] == SENTINEL).all(), "the write went past its buffer"

    def check_exact(self):
        import torch

        d = self.d
        if self.kind == "pair":
            for o, want in zip(self.outs, self.truth):
                self._check_set(o.offsets, o.keys, o.n_keys, want)
        elif self.kind == "union":
            self._check_set(self.result.offsets, self.bufs[0], self.result.n_keys, self.truth)
        elif self.kind == "decode":
            self._check_set(self.result.offsets, self.bufs[0], self.result.n_keys, d.dec_truth)
        elif self.kind == "count":
            out, n_cut = self.result
            assert n_cut == int((d.cnt < self.CUTOFF).sum())
            self._check_set(out.offsets, self.bufs[0], out.n_keys, d.uniq[d.cnt >= self.CUTOFF])
        else:
            want = self.spss_truth()
            sp = self.result
            assert (sp.n_strings, sp.n_bases) == (len(want), sum(len(s) for s in want))
            assert sp.to_strings() == want
            words, lens = (b.view(torch.uint8).cpu().numpy() for b in self.bufs)
            assert (words[max(self.n_words, 1) * 8:] == SENTINEL).all(), "the write went past d_words"
            assert (lens[max(sp.n_strings, 1) * 4:] == SENTINEL).all(), "the write went past d_lens"

    def check_untouched(self):
        for b in self.bufs:
            assert all_sentinel(b), "a refused write touched an output buffer"
        if self.snap is not None:
            offs = [o.offsets for o in self.outs] if self.kind == "pair" else [self.p.out.offsets]
            for now, before in zip(offs, self.snap):
                assert bool((now == before).all().item()), "a refused write touched the plan's offsets"


def assert_refused(exc, write_symbol, plan_symbol):
    assert exc.code == capi.KSH_FAILED_PRECONDITION, str(exc)
    assert write_symbol in str(exc) and plan_symbol in str(exc), str(exc)


# ---- intruders ----------------------------------------------------------------------------------------------------
def dsu_truth(n, xs, ys):
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for x, y in zip(xs, ys):
        parent[find(int(x))] = find(int(y))
    return np.array([find(i) for i in range(n)])


def same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def svb_size(v):
    lens = np.where(v == 0, 0, np.where(v < 256, 1, np.where(v < 65536, 2, 4)))
    return (v.size + 3) // 4 + int(lens.sum())


# ---- the calls that take their request first ------------------------------------------------------------------------
# Five of them are issued twice by their callers: count(which) is the counting call of request A or B and returns what
# the caller holds between the two calls; fill(which, held) is the filling call into sentinel buffers and returns the
# check of what it wrote; refused(held) is the fill of request A handed what belongs to request B.
REQUEST = {"A": cases.REQUEST_A, "B": cases.REQUEST_B}


def key_part(buf, n_keys, g):
    """(the first n_keys keys of a sentinel buffer in the key type, whether every byte behind them is intact)"""
    raw = buf.cpu().numpy()
    cut = n_keys * g.key_bytes
    return raw[:cut].view(capi.KEY_DTYPE[g.key_bytes]), bool((raw[cut:] == SENTINEL).all())


def part(buf, n, dtype):
    """(the first n elements of a sentinel buffer, whether every byte behind them is intact)"""
    import torch

    raw = buf.view(torch.uint8).cpu().numpy()
    cut = n * np.dtype(dtype).itemsize
    return raw[:cut].view(dtype), bool((raw[cut:] == SENTINEL).all())


def typed(n, dtype, device):
    """A sentinel buffer of n elements (and TAIL bytes behind them) as a tensor of dtype."""
    import torch

    size = torch.empty(0, dtype=dtype).element_size()
    return sentinel(n * size, device)[: n * size + TAIL - TAIL % size].view(dtype)


def failed_precondition(fn):
    with pytest.raises(capi.KshError) as e:
        fn()
    stop_on_internal(e.value)
    assert e.value.code == capi.KSH_FAILED_PRECONDITION, str(e.value)
    return str(e.value)


class SelectCall:
    """ksh_kss_select_count, then ksh_kss_select_keys."""

    def __init__(self, idx, data):
        self.idx, self.d, self.dev = idx, data, idx.ctx.device

    def count(self, which):
        off, n, spec = self.idx.select_count(spectrum=True, **REQUEST[which])
        kmers, want_off, _ = self.d.h["select"][which]
        assert n == kmers.size and np.array_equal(off.cpu().numpy(), want_off)
        assert np.array_equal(spec, self.d.h["spectrum"][which])
        return off, n

    def fill(self, which, held):
        off, n = held
        keys = sentinel(n * self.d.g.key_bytes, self.dev)
        self.idx.select_write(off, n, keys, **REQUEST[which])

        def verify():
            got, intact = key_part(keys, n, self.d.g)
            assert np.array_equal(got, self.d.h["select"][which][2]) and intact, "select %s" % which
        return verify

    def refused(self, held_a, held_b):
        """A's fill with B's offsets, then with B's count: refused, nothing at or behind the capacity it was given
        (the buffer has room for every k-mer of the structure, so even a wrong kernel stays inside it)."""
        for off, n in ((held_b[0], held_a[1]), (held_a[0], held_b[1])):
            keys = sentinel(self.d.h["n_distinct"] * self.d.g.key_bytes, self.dev)
            assert "ksh_kss_select_keys" in failed_precondition(
                lambda: self.idx.select_write(off, n, keys, **REQUEST["A"]))
            assert key_part(keys, n, self.d.g)[1], "a refused ksh_kss_select_keys wrote behind its capacity"


class ClassIdsCall:
    """ksh_kss_select_count of the union of the request's columns, then ksh_kss_select_class_ids with the table of
    those columns."""

    def __init__(self, idx, data):
        self.idx, self.d, self.dev = idx, data, idx.ctx.device

    def count(self, which):
        off, n, _ = self.idx.select_count(cols=REQUEST[which]["cols"])
        _, kmers, want_off, _, _ = self.d.h["class_ids"][which]
        assert n == kmers.size and np.array_equal(off.cpu().numpy(), want_off)
        return off, n

    def fill(self, which, held):
        import torch

        off, n = held
        rows, _, _, want_keys, want_ids = self.d.h["class_ids"][which]
        keys, ids = sentinel(n * self.d.g.key_bytes, self.dev), typed(n, torch.int32, self.dev)
        assert self.idx.select_class_ids(off, n, rows, keys, ids, cols=REQUEST[which]["cols"]) is None

        def verify():
            got, intact = key_part(keys, n, self.d.g)
            assert np.array_equal(got, want_keys) and intact, "class ids %s: keys" % which
            got, intact = part(ids, n, np.int32)
            assert np.array_equal(got, want_ids) and intact, "class ids %s: ids" % which
        return verify

    def refused(self, held_a, held_b):
        import torch

        rows, cols = self.d.h["class_ids"]["A"][0], REQUEST["A"]["cols"]
        for off, n in ((held_b[0], held_a[1]), (held_a[0], held_b[1])):
            room = self.d.h["n_distinct"]
            keys, ids = sentinel(room * self.d.g.key_bytes, self.dev), typed(room, torch.int32, self.dev)
            assert "ksh_kss_select_class_ids" in failed_precondition(
                lambda: self.idx.select_class_ids(off, n, rows, keys, ids, cols=cols))
            assert key_part(keys, n, self.d.g)[1] and part(ids, n, np.int32)[1], \
                "a refused ksh_kss_select_class_ids wrote behind its capacity"


class ClassRunsCall:
    """ksh_seq_class_runs with capacity 0, then with the number of runs it returned."""

    def __init__(self, idx, data, route=1):
        self.idx, self.d, self.dev, self.route = idx, data, idx.ctx.device, route

    def raw(self, which, capacity, off, start, cls):
        table = self.d.h["runs"][which][0]
        rc, n_runs, missing = self.idx.class_runs_raw(self.d.dseqs, table, capacity, off, start, cls,
                                                      cols=REQUEST[which]["cols"], canonicalize=True, route=self.route)
        if rc != capi.KSH_OK:
            raise capi.KshError(rc, capi.lib().ksh_last_error().decode())
        return n_runs, missing

    def count(self, which):
        n_runs, missing = self.raw(which, 0, None, None, None)
        assert n_runs == int(self.d.h["runs"][which][1][-1]) and missing == 0
        return n_runs

    def buffers(self, capacity):
        import torch

        return (typed(self.d.dseqs.n_strings + 1, torch.int64, self.dev), typed(capacity, torch.int32, self.dev),
                typed(capacity, torch.int32, self.dev))

    def fill(self, which, capacity):
        off, start, cls = self.buffers(capacity)
        assert self.raw(which, capacity, off, start, cls) == (capacity, 0)

        def verify():
            _, want_off, want_start, want_cls, _ = self.d.h["runs"][which]
            for buf, want, dtype in ((off, want_off, np.int64), (start, want_start, np.int32), (cls, want_cls, np.int32)):
                got, intact = part(buf, want.size, dtype)
                assert np.array_equal(got, want) and intact, "class runs %s" % which
        return verify

    def refused(self, capacity_a, capacity_b):
        """A's fill with room for B's runs: refused with the true number, nothing at or behind the capacity."""
        off, start, cls = self.buffers(capacity_b)
        message = failed_precondition(lambda: self.raw("A", capacity_b, off, start, cls))
        assert "capacity" in message and str(capacity_a) in message, message
        assert part(start, capacity_b, np.int32)[1] and part(cls, capacity_b, np.int32)[1]
        assert part(off, self.d.dseqs.n_strings + 1, np.int64)[1]


class LinksCall:
    """ksh_spss_links with capacity 0, then with the number of links it returned."""

    def __init__(self, ctx, data):
        self.ctx, self.d, self.dev = ctx, data, ctx.device

    def raw(self, which, capacity, off, to, seqs=None):
        seqs = seqs or self.d.links[which]["seqs"]
        rc, n_links = self.ctx.spss_links_raw(seqs, True, capacity, off, to)
        if rc != capi.KSH_OK:
            raise capi.KshError(rc, capi.lib().ksh_last_error().decode())
        return n_links

    def count(self, which):
        n_links = self.raw(which, 0, None, None)
        assert n_links == self.d.links[which]["want"][1].size
        return n_links

    def buffers(self, which, capacity):
        import torch

        return (typed(2 * self.d.links[which]["seqs"].n_strings + 1, torch.int64, self.dev),
                typed(capacity, torch.int64, self.dev))

    def fill(self, which, capacity):
        off, to = self.buffers(which, capacity)
        assert self.raw(which, capacity, off, to) == capacity

        def verify():
            for buf, want in zip((off, to), self.d.links[which]["want"]):
                got, intact = part(buf, want.size, np.int64)
                assert np.array_equal(got, want) and intact, "links %s" % which
        return verify

    def refused(self, capacity_a, capacity_b):
        """A's fill with too small a capacity: refused with the true number, the targets untouched, the offsets
        (the header: written whenever given) whole."""
        off, to = self.buffers("A", capacity_b)
        message = failed_precondition(lambda: self.raw("A", capacity_b, off, to))
        assert "capacity = %d" % capacity_b in message and "n_links = %d" % capacity_a in message, message
        assert all_sentinel(to), "a refused ksh_spss_links touched d_link_to"
        want = self.d.links["A"]["want"][0]
        got, intact = part(off, want.size, np.int64)
        assert np.array_equal(got, want) and intact


class BubblesCall:
    """ksh_link_bubbles with both capacities 0, then with the two numbers it returned."""

    def __init__(self, ctx, data):
        self.ctx, self.d, self.dev = ctx, data, ctx.device

    def raw(self, which, nb, na, bufs, to=None):
        g = self.d.graph
        rc, got_nb, got_na = self.ctx.link_bubbles_raw(g["off"], g["to"] if to is None else to, g["max_arm"][which], nb,
                                                       na, *bufs, string_class=g["cls"], rows=g["rows"])
        if rc != capi.KSH_OK:
            raise capi.KshError(rc, capi.lib().ksh_last_error().decode())
        return got_nb, got_na

    def count(self, which):
        held = self.raw(which, 0, 0, (None, None, None, None))
        want = self.d.bubbles[which]
        assert held == (len(want[0]), len(want[2]))
        return held

    def buffers(self, nb, na):
        import torch

        return [typed(size, torch.int64, self.dev) for size in (2 * nb, 2 * nb + 1, na, 4 * nb)]

    def fill(self, which, held):
        nb, na = held
        bufs = self.buffers(nb, na)
        assert self.raw(which, nb, na, bufs) == held

        def verify():
            ends, arm_off, arm, arm_rows = self.d.bubbles[which]
            wants = (ends.reshape(-1), arm_off, arm, arm_rows.reshape(-1).view(np.int64))
            for buf, want in zip(bufs, wants):
                got, intact = part(buf, want.size, np.int64)
                assert np.array_equal(got, want) and intact, "bubbles %s" % which
        return verify

    def refused(self, held_a, held_b):
        """A's fill with B's capacities: refused with the true numbers, all four outputs untouched."""
        bufs = self.buffers(*held_b)
        message = failed_precondition(lambda: self.raw("A", held_b[0], held_b[1], bufs))
        assert "capacity = %d but n_bubbles = %d" % (held_b[0], held_a[0]) in message, message
        assert all(all_sentinel(b) for b in bufs), "a refused ksh_link_bubbles touched an output"


def raw_cut(ctx, seqs, off, start, n_runs, words, lens):
    """ksh_spss_cut itself -> (status, n_bases_out)."""
    import torch

    view, n = seqs.view(), C.c_int64(-7)
    with torch.cuda.stream(ctx.stream):
        rc = capi.lib().ksh_spss_cut(C.byref(view), ctx.h, C.byref(seqs.g), off.data_ptr(), start.data_ptr(), n_runs,
                                     words.data_ptr(), lens.data_ptr(), C.byref(n))
    if rc == capi.KSH_INTERNAL:
        capi.check(rc)
    return rc, n.value


def run_cut(ctx, data, bad=False):
    import torch

    c = data.cut
    strings, want_lens, n_out = c["want"]
    n_words, n_runs = (n_out + 31) // 32, len(strings)
    words, lens = typed(n_words, torch.int64, ctx.device), typed(n_runs, torch.int32, ctx.device)
    rc, n = raw_cut(ctx, c["seqs"], c["bad_off"] if bad else c["off"], c["start"], n_runs, words, lens)
    if bad:
        message = capi.lib().ksh_last_error().decode()
        assert rc == capi.KSH_INVALID_ARGUMENT and "string 3 has no run" in message, (rc, message)
        assert all_sentinel(words) and all_sentinel(lens), "a refused ksh_spss_cut touched an output"
        return lambda: None
    assert (rc, n) == (capi.KSH_OK, n_out), capi.lib().ksh_last_error().decode()

    def verify():
        got, intact = part(words, n_words, np.uint64)
        got = got.copy()
        if n_out % 32:  # (the bits behind the last base are unspecified)
            got[-1] &= ~U(0) << U(64 - 2 * (n_out % 32))
        assert np.array_equal(got, c["words"]) and intact, "cut: words"
        got, intact = part(lens, n_runs, np.uint32)
        assert np.array_equal(got, want_lens) and intact, "cut: lens"
    return verify


def indexes(state, geom):
    """(the index that borrows the build's sets, the index that owns decoded ones) the row keeps at this geometry."""
    return state[("borrowed", geom)], state[("owned", geom)]


def run_new_op(op, ctx, store, geom, state):
    """One of the ops over the ten calls that take their request first, and their failing variants."""
    if op in cases.INDEX_OPS + ["fail:select_keys"]:
        d = store.index_data(geom)
        h = d.h
        checks = []
        for at, idx in enumerate(indexes(state, geom)):
            assert idx.ctx is ctx
            route = 1 + at  # the search on the borrowed index, the join on the owned one
            if op == "seq_hits":
                got = idx.seq_hits(d.dseqs, canonicalize=True, route=route)
                checks.append(lambda got=got: np.array_equal(got[:, :cases.KSS_SETS], h["hits"]) or pytest.fail(op))
            elif op == "pair_counts":
                got = idx.pair_counts(cols=cases.COLS, with_distinct=True)
                checks.append(lambda got=got: (np.array_equal(got[0], h["pairs"]) and got[1] == h["n_distinct"])
                              or pytest.fail(op))
            elif op == "select":
                call = SelectCall(idx, d)
                checks.append(call.fill("A", call.count("A")))
            elif op == "classes":
                got = idx.color_classes(cases.COLS, capacity=1 << len(cases.COLS))
                checks.append(lambda got=got: (np.array_equal(got[0], h["rows"]) and np.array_equal(got[1], h["counts"]))
                              or pytest.fail(op))
            elif op == "class_ids":  # (the offsets are the reference's: the op is this one call)
                checks.append(ClassIdsCall(idx, d).fill("A", (d.ids_off["A"], h["class_ids"]["A"][1].size)))
            elif op == "class_runs":
                checks.append(ClassRunsCall(idx, d, route).fill("A", int(h["runs"]["A"][1][-1])))
            else:  # fail:select_keys: request A's keys at the offsets of request B
                n = h["select"]["A"][0].size
                keys = sentinel(h["n_distinct"] * d.g.key_bytes, ctx.device)
                failed_precondition(lambda: idx.select_write(d.select_off["B"], n, keys, **cases.REQUEST_A))
                assert key_part(keys, n, d.g)[1], "a refused ksh_kss_select_keys wrote behind its capacity"
        return lambda: [check() for check in checks]
    d = store.string_data(geom)
    if op == "cut":
        return run_cut(ctx, d)
    if op == "fail:cut":
        return run_cut(ctx, d, bad=True)
    if op == "links":
        return LinksCall(ctx, d).fill("A", d.links["A"]["want"][1].size)
    if op == "bubbles":
        want = d.bubbles["A"]
        return BubblesCall(ctx, d).fill("A", (len(want[0]), len(want[2])))
    if op == "fail:links_capacity":
        n_links = d.links["A"]["want"][1].size
        LinksCall(ctx, d).refused(n_links, n_links - 1)
        return lambda: None
    if op == "fail:links_end":
        call = LinksCall(ctx, d)
        off, to = call.buffers("A", 16)
        off = typed(2 * d.repeated_end.n_strings + 1, off.dtype, ctx.device)
        with pytest.raises(capi.KshError) as e:
            call.raw("A", 16, off, to, seqs=d.repeated_end)
        stop_on_internal(e.value)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT and "string 1 " in str(e.value), str(e.value)
        assert all_sentinel(off) and all_sentinel(to), "a refused ksh_spss_links touched an output"
        return lambda: None
    assert op == "fail:bubbles", op
    call = BubblesCall(ctx, d)
    want = d.bubbles["A"]
    bufs = call.buffers(len(want[0]), len(want[2]))
    with pytest.raises(capi.KshError) as e:
        call.raw("A", len(want[0]), len(want[2]), bufs, to=d.graph["bad_to"])
    stop_on_internal(e.value)
    assert e.value.code == capi.KSH_INVALID_ARGUMENT and "has no twin" in str(e.value), str(e.value)
    assert all(all_sentinel(b) for b in bufs), "a refused ksh_link_bubbles touched an output"
    return lambda: None


def run_intruder(col, ctx, store, geom, state):
    """Runs one intruder on ctx; returns a function that checks what it produced (called after the victim's write)."""
    op = col["op"]
    L = capi.lib()
    if op in cases.INDEX_OPS + cases.STRING_OPS + cases.NEW_FAILING:
        return run_new_op(op, ctx, store, geom, state)
    if op.startswith(("full:", "abandon:", "plain:")):
        how, kind = op.split(":")
        d = store.get(geom, "intruder")
        v = Victim(kind, d, ctx, plain=how == "plain")
        v.plan()
        if how == "abandon":
            return lambda: None
        if how == "plain" and col["where"] == "own" and state.get("victim_kind") == kind:
            # the plain write cannot tell its plan from the victim's unwritten one that it replaced: refused, and
            # the refusal ends the plan
            plan_sym, write_sym, _ = cases.KINDS[kind]
            refused(v.write, write_sym, plan_sym)
            v.check_untouched()
            return lambda: None
        v.write()
        want = {"unitigs": len(d.unitigs), "strings": len(d.spss), "bases": sum(len(s) for s in d.spss)}
        if how == "full" and kind == "encode":
            st = ctx.spss_encode_stats()
            assert {key: st[key] for key in want} == want, st
            routes = ctx.spss_encode_routes()
            assert routes and routes <= set(ctx.ROUTES), routes
        if how == "full" and kind == "cover":
            st = ctx.spss_cover_stats()
            assert {key: st[key] for key in want} == want, st
        return v.check_exact
    d = store.get(geom, "intruder")
    k, n = d.k, geom[1]
    if op == "hash":
        h = ctx.set_hash(d.dA)
        return lambda: h == int(np.bitwise_xor.reduce(d.a)) or pytest.fail("hash")
    if op == "contains":
        q = np.concatenate([d.a[::40], d.b[::40], d.a[:50] ^ U(5)])
        got = ctx.set_contains(d.dA, q)
        return lambda: np.array_equal(got, np.isin(q, d.a)) or pytest.fail("contains")
    if op == "kmers":
        got = ctx.set_kmers(d.dA)
        return lambda: np.array_equal(got, d.a) or pytest.fail("kmers")
    if op == "diff":
        got = ctx.set_diff(d.dA, d.dB)
        return lambda: got == np.setdiff1d(d.a, d.b).size + np.setdiff1d(d.b, d.a).size or pytest.fail("diff")
    if op == "weights":
        ids = synth.sample_bucket_ids(n, seed=3)
        got = ctx.pair_weights([d.dA, d.dB], ids, [(0, 1)])
        both = np.intersect1d(d.a, d.b)
        want = int(np.isin(both >> U(2 * k - n), np.asarray(ids, dtype=U)).sum())
        return lambda: (got.tolist() == [want]) or pytest.fail("weights %s != %d" % (got, want))
    if op in ("algebra", "batch"):
        if op == "algebra":
            trios = [(ctx.pair_algebra_onepass(d.dA, d.dB), d.a, d.b)]
        else:
            res = ctx.pair_algebra_batch([(d.dA, d.dB), (d.dB, d.dA)])
            trios = [(res[0], d.a, d.b), (res[1], d.b, d.a)]

        def verify():
            for (i, amb, bma), x, y in trios:
                assert np.array_equal(i.kmers(), np.intersect1d(x, y))
                assert np.array_equal(amb.kmers(), np.setdiff1d(x, y))
                assert np.array_equal(bma.kmers(), np.setdiff1d(y, x))
        return verify
    if op == "dsu":
        rng = np.random.default_rng(4)
        xs, ys = rng.integers(0, 300, size=200), rng.integers(0, 300, size=200)
        got = ctx.dsu_components(300, xs, ys)
        return lambda: same_partition(got, dsu_truth(300, xs, ys)) or pytest.fail("dsu")
    if op == "svb":
        v = (synth.mix64(np.arange(1001, dtype=U)) >> U(40)).astype(np.uint32)
        v[::5] = 0
        v[1::7] &= 0xFF
        enc = ctx.svb_encode(v)
        back, used = ctx.svb_decode(enc, v.size)
        return lambda: (enc.size == svb_size(v) == used and np.array_equal(back, v)) or pytest.fail("svb")
    if op == "size":
        got = ctx.spss_size(d.sp)
        return lambda: got == sum(len(s) - k + 1 for s in d.spss) or pytest.fail("size")
    if op == "to_text":
        t = ctx.spss_to_text(d.sp)
        return lambda: bytes(t.cpu().numpy()) == d.text.encode() or pytest.fail("to_text")
    if op == "copies":
        import torch

        src = np.arange(4096, dtype=np.uint8)
        d1 = torch.zeros(4096, dtype=torch.uint8, device=ctx.device)
        d2 = torch.zeros(4096, dtype=torch.uint8, device=ctx.device)
        back = np.zeros(4096, dtype=np.uint8)
        capi.check(L.ksh_ctx_memcpy_h2d(ctx.h, d1.data_ptr(), src.ctypes.data_as(C.c_void_p), 4096))
        capi.check(L.ksh_ctx_memcpy_d2d(ctx.h, d2.data_ptr(), d1.data_ptr(), 4096))
        capi.check(L.ksh_ctx_memcpy_d2h(ctx.h, back.ctypes.data_as(C.c_void_p), d2.data_ptr(), 4096))
        return lambda: np.array_equal(back, src) or pytest.fail("copies")
    if op == "ctx_misc":
        ctx.sync()
        ctx.enable_timing(True)
        ctx.timing_reset()
        ctx.timing_read(0), ctx.timing_units(3), ctx.timing_wall(0)
        ctx.enable_timing(False)
        st = ctx.mem_stats()
        return lambda: st["scratch"] >= 0 or pytest.fail("mem_stats")
    if op == "reserve":
        before = ctx.mem_stats()["scratch"]
        capi.check(L.ksh_ctx_reserve(ctx.h, before + (16 << 20)))  # more than the arena holds: it is reallocated
        assert ctx.mem_stats()["scratch"] > before
        return lambda: None
    if op == "lanes":
        ctx.set_lanes(2)
        return lambda: None
    if op == "release:encode":
        ctx.spss_encode_release()
        return lambda: None
    if op == "release:cover":
        ctx.spss_cover_release()
        return lambda: None
    if op.startswith("fail:"):
        what = op.split(":")[1]
        code = capi.KSH_INVALID_ARGUMENT
        with pytest.raises(capi.KshError) as e:
            if what == "decode":
                ctx.spss_decode_plan(store.overdeclared(geom))
            elif what == "cover":
                ctx.spss_cover_plan(store.overdeclared(geom))
            elif what == "from_text":
                import torch

                bad = d.d_text.clone()
                bad[bad.numel() // 2] = ord("X")
                ctx.spss_from_text_plan(d.g, bad)
            elif what == "fasta":
                code = capi.KSH_FAILED_PRECONDITION
                cut = d.fasta.index("\n", d.fasta.rindex(">")) + 1  # the last record's read cut off: its header stays
                ctx.fasta_plan(d.g, d.d_fasta[:cut])
            else:
                ctx.spss_encode_plan(store.palindromic(), mode=0, canonical=True)
        stop_on_internal(e.value)
        assert e.value.code == code, str(e.value)
        return lambda: None
    if op.startswith("kss_build:"):
        ks = store.kss_inputs(geom)
        ctx.set_lanes(1 if op.endswith("lanes1") else 0)
        dk = capi.DeviceKmerSetSet(ctx, ks["comps"], ks["ids"])
        state[("kss", geom)] = dk
        n_nodes = dk.size()
        st = dk.stats()
        assert st["nodes"] == n_nodes >= 4
        dk.node_size(0), dk.children(0), dk.meta(), dk.trace(), dk.initial_weights(), dk.node_holder(0)
        cs = (C.c_int64 * 8)()
        capi.check(L.ksh_kss_comm_stats(dk.h, cs))

        def verify():  # Get(i) of an input is the input
            assert np.array_equal(dk.get_kmers(0), ks["sets"][0])
            assert np.array_equal(dk.get_kmers(3), ks["sets"][3])
        return verify
    if op == "kss_get":
        ks, dk = store.kss_inputs(geom), state[("kss", geom)]
        got = dk.get_kmers(1)
        return lambda: np.array_equal(got, ks["sets"][1]) or pytest.fail("kss_get")
    if op in ("kss_index_query", "kss_index_create"):
        ks = store.kss_inputs(geom)
        q = ks["q"]
        if op == "kss_index_query":
            idx = state[("borrowed", geom)] = capi.KssIndex.from_kss(state[("kss", geom)])
            assert idx.info()["n_nodes"] == state[("kss", geom)].size()
        else:
            idx = state[("owned", geom)] = capi.KssIndex.from_nodes(ctx, ks["comps"], [[] for _ in ks["comps"]])
            assert idx.info()["n_nodes"] == len(ks["comps"])
        got = idx.query(q, canonicalize=True, route=1)
        assert idx.routes() & capi.QROUTE_SEARCH
        # (the index stays open for the columns behind this one; kss_index_close ends it)
        want = np.stack([np.isin(synth.canonical(q, k).astype(U), s) for s in ks["sets"]], axis=1)
        return lambda: np.array_equal(got[:, : len(ks["sets"])], want) or pytest.fail(op)
    if op == "kss_index_close":
        state.pop(("borrowed", geom)).close()
        state.pop(("owned", geom)).close()
        return lambda: None
    if op == "kss_destroy":
        state.pop(("kss", geom)).close()
        return lambda: None
    if op in ("large:arena", "large:plans"):
        lg = store.large()
        before = ctx.mem_stats()["scratch"]

        def grew(what):  # (each of the three must be reallocated while the victim's plan is pending)
            nonlocal before
            now = ctx.mem_stats()["scratch"]
            assert now > before, "the large %s did not make the context's scratch grow" % what
            before = now

        if op == "large:arena":
            capi.check(L.ksh_ctx_reserve(ctx.h, before + (16 << 20)))
            trio = ctx.pair_algebra_onepass(lg["dA"], lg["dB"])
            text = ctx.spss_to_text(lg["sp"])
            dec = back = big = None
        else:
            big = store.large_pair(16 if geom[1] <= 14 else geom[1] + 2)  # more buckets than the row has planned with
            trio = ctx.pair_algebra(big["dA"], big["dB"])
            grew("pair plan (ctx->plan)")
            dec = ctx.spss_decode(lg["sp"], canonical=True)
            grew("decode (the decode slot)")
            back = ctx.spss_from_text(lg["g"], lg["d_text"])
            grew("text plan (the text slot)")
            text = None
        if op == "large:arena":
            grew("reserve + one-call operations (the arena)")

        def same_set(got, want):
            off, keys = got.to_numpy()
            return got.n_keys == want[1].size and np.array_equal(off, want[0]) and np.array_equal(keys, want[1])

        def verify():
            for got, want in zip(trio, lg["sets"] if text is not None else big["sets"]):
                assert same_set(got, want)
            if text is not None:
                assert bytes(text.cpu().numpy()) == lg["text"].encode()
            if dec is not None:
                assert same_set(dec, lg["dec"])
                words, lens = lg["packed"]
                assert (back.n_strings, back.n_bases) == (lens.size, len(lg["text"]) - lens.size)
                assert np.array_equal(back.words[: words.size].cpu().numpy().view(np.uint64), words)
                assert np.array_equal(back.lens[: lens.size].cpu().numpy().view(np.uint32), lens)
        return verify
    raise AssertionError("no such intruder: " + op)


# ---- the table ---------------------------------------------------------------------------------------------------
def run_cell(victim_row, col, ctxs, store, states):
    kind, geom = victim_row["kind"], victim_row["geom"]
    plan_sym, write_sym, _ = cases.KINDS[kind]
    own = ctxs["own"]
    use(own)
    v = Victim(kind, store.get(geom, "victim", victim_row["empty"]), own, plain=victim_row["plain"])
    v.plan()
    where = ctxs[col["where"]]
    states[col["where"]]["victim_kind"] = kind
    use(where)
    igeom = geom if col["width"] == "same" else cases.other_geom(geom)
    verify = run_intruder(col, where, store, igeom, states[col["where"]])
    use(own)
    expected = cases.TABLE[(victim_row["id"], col["id"])]
    try:
        v.write()
        observed = cases.EXACT
    except capi.KshError as e:
        stop_on_internal(e)
        observed = cases.REFUSED
        assert_refused(e, write_sym, plan_sym)
    OUTCOMES[(victim_row["id"], col["id"])] = observed
    assert observed == expected, "expected %s, the write was %s" % (expected, observed)
    if observed == cases.EXACT:
        v.check_exact()
    else:
        v.check_untouched()
        v.plan()  # the context stays usable: a fresh plan + write gives the truth
        v.write()
        v.check_exact()
    use(where)
    verify()
    use(own)


@pytest.mark.parametrize("row", cases.VICTIMS, ids=[r["id"] for r in cases.VICTIMS])
def test_victim_row(store, row):
    guard()
    WALL.setdefault("ran", []).append(row["id"])
    t0 = time.time()
    ctxs = {"own": capi.Context(0), "second": capi.Context(0)}
    states = {"own": {}, "second": {}}
    failures = []
    try:
        for col in cases.INTRUDERS:
            if STOP["why"]:
                failures.append("%s: not run (stopped: %s)" % (col["id"], STOP["why"]))
                continue
            cell_t0 = time.time()
            try:
                run_cell(row, col, ctxs, store, states)
            except BaseException as e:  # noqa: B902 -- every cell is reported; an internal error stops the module
                stop_on_internal(e)
                failures.append("%s: %s: %s" % (col["id"], type(e).__name__, str(e)[:300]))
                if isinstance(e, KeyboardInterrupt):
                    raise
            spent = WALL.setdefault("ops", {}).setdefault(col["op"], [0.0, 0.0])
            spent[row["geom"][1] >= 20] += time.time() - cell_t0
    finally:
        if not STOP["why"]:
            import torch

            torch.cuda.synchronize()
            for st in states.values():  # the indexes before the structures they borrow from
                for kind in ("borrowed", "owned", "kss"):
                    for key in [key for key in st if isinstance(key, tuple) and key[0] == kind]:
                        st.pop(key).close()
            for c in ctxs.values():
                c.close()
    WALL["rows"] = WALL.get("rows", 0.0) + time.time() - t0
    assert not failures, "%d of %d cells failed:\n%s" % (len(failures), len(cases.INTRUDERS), "\n".join(failures))


# ---- the rules beside the table --------------------------------------------------------------------------------
@pytest.fixture()
def ctx(gpu):
    guard()
    c = capi.Context(0)
    use(c)
    yield c
    if not STOP["why"]:
        c.close()


def refused(fn, write_sym, plan_sym):
    with pytest.raises(capi.KshError) as e:
        fn()
    stop_on_internal(e.value)
    assert_refused(e.value, write_sym, plan_sym)


@pytest.mark.parametrize("geom", [(23, 14, 4), (23, 16, 4)], ids=["narrow", "wide"])
@stops_module
def test_failed_plan_does_not_leave_the_older_plan_valid(ctx, store, geom):
    """A plan that fails after it has overwritten its group's scratch: the older plan's write is refused, nothing is
    written, and a fresh plan + write gives the truth.  The same for every group that has a failing plan."""
    failing = {"decode": "fail:decode", "count": "fail:decode", "cover": "fail:cover", "encode": "fail:encode",
               "from_text": "fail:from_text", "fasta": "fail:fasta"}
    for kind, op in failing.items():
        v = Victim(kind, store.get(geom, "victim"), ctx)
        v.plan()
        col = next(c for c in cases.INTRUDERS if c["op"] == op and c["where"] == "own")
        run_intruder(col, ctx, store, geom, {})
        plan_sym, write_sym, _ = cases.KINDS[kind]
        refused(v.write, write_sym, plan_sym)
        v.check_untouched()
        v.plan()
        v.write()
        v.check_exact()
    # a failing plan with NO older plan: its own write is refused too (it never returns KSH_OK with nothing written)
    for kind, op in failing.items():
        fresh = capi.Context(0)
        use(fresh)
        col = next(c for c in cases.INTRUDERS if c["op"] == op and c["where"] == "own")
        run_intruder(col, fresh, store, geom, {})
        v = Victim(kind, store.get(geom, "victim"), ctx)
        use(ctx)
        v.plan()
        use(fresh)
        plan_sym, write_sym, _ = cases.KINDS[kind]
        refused(lambda: v.write(fresh), write_sym, plan_sym)
        v.check_untouched()
        fresh.close()
        use(ctx)


@stops_module
def test_mismatched_writes_are_refused(ctx, store):
    """Geometry (k, N, key bytes) or canonical flag other than the planned ones, a pair write on a union plan and a
    union write on a pair plan, a `_for` write with other sizes or another input: refused on the host, outputs
    untouched, the plan still good for the right write."""
    d = store.get((23, 14, 4), "victim")
    others = [capi.geom(22, 14, 4), capi.geom(23, 15, 4), capi.geom(23, 14, 8)]
    for kind in ("decode", "count"):
        plan_sym, write_sym, _ = cases.KINDS[kind]
        v = Victim(kind, d, ctx)
        v.plan()
        for g in others:
            if kind == "decode":
                refused(lambda: ctx.spss_decode_write(v.p, keys=v.bufs[0], g=g), write_sym, plan_sym)
            else:
                refused(lambda: ctx.kmer_count_write(v.p, 2, keys=v.bufs[0], g=g), write_sym, plan_sym)
        if kind == "decode":
            refused(lambda: ctx.spss_decode_write(v.p, keys=v.bufs[0], canonical=False), write_sym, plan_sym)
            refused(lambda: ctx.spss_decode_write(v.p, keys=v.bufs[0], sp=d.dF), write_sym, plan_sym)
        else:
            refused(lambda: ctx.kmer_count_write(v.p, 2, keys=v.bufs[0], canonical=False), write_sym, plan_sym)
        v.check_untouched()
        v.write()
        v.check_exact()
    # pair / union
    v = Victim("pair", d, ctx)
    v.plan()
    for g in others:
        refused(lambda: ctx.pair_write(d.dA, d.dB, *v.outs, g=g), "ksh_pair_write", "ksh_pair_plan")
    refused(lambda: ctx.pair_write(d.dB, d.dA, *v.outs), "ksh_pair_write", "ksh_pair_plan")
    u = Victim("union", d, ctx)
    u.p = capi.Pending(kind="union", a=d.dA, b=d.dB, out=capi.DeviceSet.empty_like_offsets(d.g, 0, ctx.device), n_keys=0)
    u.bufs = [sentinel(16, ctx.device)]
    refused(lambda: ctx.set_union_write(u.p, keys=u.bufs[0]), "ksh_set_union_write", "ksh_set_union_plan")
    assert all_sentinel(u.bufs[0])
    v.check_untouched()
    v.write()
    v.check_exact()
    u = Victim("union", d, ctx)
    u.plan()
    outs = [capi.DeviceSet.empty_like_offsets(d.g, 0, ctx.device) for _ in range(3)]
    for o in outs:
        o.keys = sentinel(16, ctx.device)
    refused(lambda: ctx.pair_write(d.dA, d.dB, *outs), "ksh_pair_write", "ksh_pair_plan")
    assert all(all_sentinel(o.keys) for o in outs)
    for g in others:
        refused(lambda: ctx.set_union_write(u.p, keys=u.bufs[0], g=g), "ksh_set_union_write", "ksh_set_union_plan")
    u.check_untouched()
    u.write()
    u.check_exact()
    # the `_for` writes: sizes or input other than the pending plan's
    e = store.get((23, 14, 4), "intruder")
    other_input = {"encode": ("set", e.dA), "cover": ("unitigs", e.dU), "from_text": ("text", e.d_text),
                   "fasta": ("text", e.d_fasta)}
    for kind in cases.NAMELESS:
        plan_sym, write_sym, _ = cases.KINDS[kind]
        v = Victim(kind, d, ctx)
        v.plan()
        write = {"encode": ctx.spss_encode_write, "cover": ctx.spss_cover_write,
                 "from_text": ctx.spss_from_text_write, "fasta": ctx.fasta_write}[kind]
        field, value = other_input[kind]
        for change in ({"n_bases": v.p.n_bases + 1}, {"n_strings": v.p.n_strings + 1}, {field: value}):
            fake = capi.Pending(**dict(v.p.__dict__, **change))
            refused(lambda: write(fake, words=v.bufs[0], lens=v.bufs[1]), write_sym, plan_sym)
        v.check_untouched()
        v.write()
        v.check_exact()


# (kind, plain form) -> what a second write on one plan gives
REPLAY = {("pair", False): cases.EXACT, ("union", False): cases.EXACT, ("decode", False): cases.REFUSED,
          ("count", False): cases.REFUSED}
for _kind in cases.NAMELESS:
    REPLAY[(_kind, False)] = cases.EXACT    # the `_for` write leaves its plan as it is
    REPLAY[(_kind, True)] = cases.REFUSED   # the plain write serves a plan once


@pytest.mark.parametrize("geom", cases.NARROW + cases.WIDE[:1], ids=lambda g: "k%d-N%d-u%d" % (g[0], g[1], 8 * g[2]))
@stops_module
def test_replay_and_release(ctx, store, geom):
    """A second (and third) write on one plan is exact or refused, the same way every time (the header's table:
    the decode's write consumes its plan, the others leave theirs); a write after *_release is refused."""
    d = store.get(geom, "victim")
    for (kind, plain), expected in REPLAY.items():
        plan_sym, write_sym, _ = cases.KINDS[kind]
        v = Victim(kind, d, ctx, plain=plain)
        v.plan()
        v.write()
        v.check_exact()
        for _ in range(2):
            if v.snap is not None:  # (the first write may have rewritten the offsets: duplicates dropped)
                v.snap = [o.offsets.clone() for o in v.outs] if kind == "pair" else [v.p.out.offsets.clone()]
            first = v.bufs
            v.bufs = [sentinel(b.numel() * b.element_size() - TAIL, ctx.device).view(b.dtype) for b in first]
            if kind == "pair":
                for o, b in zip(v.outs, v.bufs):
                    o.keys = b
            if expected == cases.EXACT:
                v.write()
                v.check_exact()
            else:
                refused(v.write, write_sym, plan_sym)
                v.check_untouched()
    for kind, release, plain in (("encode", ctx.spss_encode_release, False), ("cover", ctx.spss_cover_release, True),
                                 ("encode", ctx.spss_cover_release, True), ("cover", ctx.spss_encode_release, False)):
        plan_sym, write_sym, _ = cases.KINDS[kind]
        v = Victim(kind, d, ctx, plain=plain)
        v.plan()
        release()
        refused(v.write, write_sym, plan_sym)
        v.check_untouched()
        v.plan()
        v.write()
        v.check_exact()


@stops_module
def test_plan_on_one_context_write_on_another(ctx, store):
    """The plan lives in the context that made it: the write on another context is refused there, touches nothing,
    and the write on the planning context is still exact."""
    d = store.get((23, 14, 4), "victim")
    other = capi.Context(0)
    for kind, plain in [(kind, False) for kind in cases.KINDS] + [(kind, True) for kind in cases.NAMELESS]:
        plan_sym, write_sym, _ = cases.KINDS[kind]
        use(ctx)
        v = Victim(kind, d, ctx, plain=plain)
        v.plan()
        use(other)
        refused(lambda: v.write(other), write_sym, plan_sym)
        v.check_untouched()
        use(ctx)
        v.write()
        v.check_exact()
    use(other)
    other.close()
    use(ctx)


def column(op):
    return next(c for c in cases.INTRUDERS if c["op"] == op and c["where"] == "own" and c["width"] == "same")


@pytest.mark.parametrize("geom", cases.NARROW, ids=lambda g: "k%d-N%d-u%d" % (g[0], g[1], 8 * g[2]))
@stops_module
def test_two_call_requests_keep_no_state(ctx, store, geom):
    """Five of the calls that take their request first are issued twice by their callers: a counting call, then a
    filling call with what the count returned.  The caller holds everything between the two; the library holds
    nothing.  So: count request A, run an intruder, fill A -- exact against the reference, whatever the intruder was:
    the same call counting request B on the same index or context (other columns, another container, another
    max_arm), each op over the ten calls, one victim of each plan group as plan + write.  And a fill that is handed
    B's offsets or B's count is refused, with every sentinel byte at or behind the capacity it was given intact
    (all of them where the header says the outputs stay untouched)."""
    state = {}
    try:
        for op in ("kss_build:lanes1", "kss_index_query", "kss_index_create"):
            run_intruder(column(op), ctx, store, geom, state)()
        d, sd = store.index_data(geom), store.string_data(geom)
        borrowed, owned = indexes(state, geom)
        calls = [SelectCall(borrowed, d), SelectCall(owned, d), ClassIdsCall(borrowed, d), ClassIdsCall(owned, d),
                 ClassRunsCall(borrowed, d, 1), ClassRunsCall(owned, d, 2), LinksCall(ctx, sd), BubblesCall(ctx, sd)]
        others = [column(op) for op in cases.INDEX_OPS + cases.STRING_OPS] + \
                 [column("full:" + kinds[0]) for kinds in cases.GROUPS.values()]
        assert len(others) == 9 + 4
        for call in calls:
            intruders = [lambda: (call.count("B"), lambda: None)[1]] + \
                        [lambda col=col: run_intruder(col, ctx, store, geom, state) for col in others]
            for intrude in intruders:
                held = call.count("A")
                check_intruder = intrude()
                call.fill("A", held)()
                check_intruder()
            held_a, held_b = call.count("A"), call.count("B")
            call.refused(held_a, held_b)
            call.fill("A", held_a)()  # (and the call still serves)
            call.fill("B", held_b)()
    finally:
        if not STOP["why"]:
            import torch

            torch.cuda.synchronize()
            for kind in ("borrowed", "owned", "kss"):
                if (kind, geom) in state:
                    state.pop((kind, geom)).close()


def test_outcome_table():
    """The victim x intruder outcome table (run with -s): one line per victim kind and intruder op, `E` exact,
    `R` refused, in the order own context same width / other width / second context; behind them the seconds the op's
    cells took, so that an op that rebuilds something per cell shows."""
    guard()
    if not set(WALL.get("ran", ())) >= {v["id"] for v in cases.VICTIMS}:
        pytest.skip("the table needs every victim row in the same run: select the whole module")
    assert len(OUTCOMES) == len(cases.TABLE), "%d of %d cells ran" % (len(OUTCOMES), len(cases.TABLE))
    assert OUTCOMES == cases.TABLE
    kinds = list(cases.KINDS)
    ops = []
    for c in cases.INTRUDERS:
        if c["op"] not in ops:
            ops.append(c["op"])
    print("\n%-20s %s" % ("intruder \\ victim", " ".join("%-9s" % k for k in kinds)))
    for op in ops:
        cells = []
        for kind in kinds:
            marks = ""
            for c in [c for c in cases.INTRUDERS if c["op"] == op]:
                got = {OUTCOMES[(v["id"], c["id"])] for v in cases.VICTIMS if v["kind"] == kind}
                marks += "E" if got == {cases.EXACT} else "R" if got == {cases.REFUSED} else "?"
            cells.append("%-9s" % marks)
        narrow, wide = WALL.get("ops", {}).get(op, (0.0, 0.0))
        print("%-20s %s %6.2f s + %.2f s" % (op, " ".join(cells), narrow, wide))
    print("(seconds per op over all its cells: the rows below N = 20, and the rows at N = 20)")
    print("replay: " + ", ".join("%s%s %s" % (k, "(plain)" if plain else "", r) for (k, plain), r in REPLAY.items()))
    print("wall: rows %.1f s, module so far %.1f s" % (WALL.get("rows", 0.0), time.time() - T0))

"""Designed inputs of ksh_link_bubbles, shared by test_link_bubbles_reference_cpu.py (which turns every edge class
listed here into a predicate) and test_gpu_link_bubbles.py (which runs every case on the device, without and with
classes).  A graph case is drawn as links between oriented strings, closed under twins by
link_bubbles_reference.csr; `want` is the answer worked out by hand, (v, w, len(arm_0), len(arm_1)) per reported
bubble.  The two families at the end are built from strings: genomes with planted substitutions and partial samples,
their k-mers merged into coloured unitigs by `colored_unitigs` below over spss_links_reference.links."""
import random

import numpy as np

import link_bubbles_reference as ref
import spss_links_reference as links_ref


class G:
    """A graph under construction: strings by number, links between oriented strings (one orientation is drawn)."""

    def __init__(self, reserved=0):
        self.n, self.links = reserved, []

    def new(self, count=1, flip=0):
        out = [2 * (self.n + i) + flip for i in range(count)]
        self.n += count
        return out

    def chain(self, vs):
        self.links += list(zip(vs[:-1], vs[1:]))

    def bubble(self, v, w, len0, len1, flip=0):
        a0, a1 = self.new(len0, flip), self.new(len1, flip)
        self.chain([v] + a0 + [w])
        self.chain([v] + a1 + [w])
        return a0, a1


# five classes over 128 columns, both words in use; class 4 holds every column
ROWS = np.array([[0x0000000000000F0F, 0x8000000000000001], [0x00000000000000FF, 0x8000000000000000],
                 [0xFFFF00000000000F, 0x0000000000000001], [0x0000000000000001, 0xFFFFFFFFFFFFFFFF],
                 [0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]], dtype=np.uint64)


def classes_of(n_strings):
    """The classes the designed graphs are run with: a fixed pattern over ROWS."""
    return np.array([(7 * s + 3) % len(ROWS) for s in range(n_strings)], dtype=np.int32)


CASES = []


def case(name, g, max_arm, classes, want):
    off, to = ref.csr(g.n, g.links)
    CASES.append(dict(id=name, n=g.n, off=off, to=to, max_arm=max_arm, classes=classes, want=sorted(want)))


def _simple(name, len0, len1, max_arm, classes, found=True):
    g = G()
    v, w = g.new(2)
    g.bubble(v, w, len0, len1)
    case(name, g, max_arm, classes, [(v, w, len0, len1)] if found else [])


_simple("arms-1-1", 1, 1, 8, ["arms_1_1", "source_at_0"])
_simple("arms-1-2", 1, 2, 8, ["arms_1_2"])
_simple("arms-max-max", 3, 3, 3, ["arms_max_max"])
_simple("arm-too-long", 1, 4, 3, ["arm_max_plus_1_nothing"], found=False)
_simple("arm-long-enough", 1, 4, 4, ["arm_max_plus_1_found"])
_simple("max-arm-64", 64, 64, 64, ["max_arm_64", "arms_max_max"])
_simple("max-arm-64-short-of-65", 65, 1, 64, ["max_arm_64", "arm_max_plus_1_nothing"], found=False)


def _max_arm_1():
    g = G()
    v, w, v2, w2 = g.new(4)
    g.bubble(v, w, 1, 1)
    g.bubble(v2, w2, 1, 2)
    case("max-arm-1", g, 1, ["max_arm_1", "arms_1_1", "arm_max_plus_1_nothing"], [(v, w, 1, 1)])


def _hairpins():
    g = G()
    (v,), (a,) = g.new(), g.new()
    g.chain([v, a, v ^ 1])  # the twins give v -> a ^ 1 -> v ^ 1: the other arm
    case("hairpin", g, 8, ["hairpin"], [(v, v ^ 1, 1, 1)])
    g = G()
    (v,), (a, b) = g.new(flip=1), g.new(2)
    g.chain([v, a, b, v ^ 1])
    case("hairpin-two-strings", g, 2, ["hairpin", "arms_max_max"], [(v, v ^ 1, 2, 2)])


def _fans(degree):
    g = G()
    v, w = g.new(2)
    for _ in range(degree):
        g.chain([v] + g.new() + [w])
    case("outdeg-%d" % degree, g, 8, ["outdeg_%d" % degree], [])


def _different_sinks():
    g = G()
    v, w0, w1, u0, u1 = g.new(5)
    g.chain([v] + g.new() + [w0])
    g.chain([v] + g.new() + [w1])
    g.chain([u0, w0])
    g.chain([u1, w1])
    case("different-sinks", g, 8, ["different_sinks"], [])


def _sink_indeg_3():
    g = G()
    v, w, u = g.new(3)
    g.bubble(v, w, 1, 2)
    g.chain([u, w])
    case("sink-indeg-3", g, 8, ["sink_indeg_3"], [])


def _side(kind):
    g = G()
    v, w, z, v2, w2 = g.new(5)
    a0, a1 = g.bubble(v, w, 2, 1)
    g.chain([a0[1], z] if kind == "exit" else [z, a0[1]])
    g.bubble(v2, w2, 1, 1)  # (an intact bubble beside it)
    case("side-%s" % kind, g, 8, ["side_%s" % kind], [(v2, w2, 1, 1)])


def _tip():
    g = G()
    v, w, u = g.new(3)
    g.chain([v] + g.new(2))  # an arm that ends nowhere
    g.chain([v] + g.new() + [w])
    g.chain([u, w])
    case("tip-arm", g, 8, ["tip"], [])


def _rings():
    g = G()
    v, w, u = g.new(3)
    r = g.new(3)
    g.chain([v] + g.new() + [r[0]])  # an arm into a ring: the ring's entry has two links in, the walk ends there
    g.chain(r + [r[0]])
    g.chain([v] + g.new() + [w])
    g.chain([u, w])
    case("ring-behind-source", g, 4, ["ring", "different_sinks"], [])
    g = G()
    (v,) = g.new()
    g.chain([v] + g.new(3) + [v])  # the source on a ring of one-in one-out strings: the walk comes back to it
    g.chain([v] + g.new(2))
    case("ring-through-source", g, 64, ["ring", "tip"], [])


def _self_link():
    g = G()
    v, w = g.new(2)
    g.chain([v, v])
    g.chain([v] + g.new() + [w])
    case("self-link", g, 8, ["self_link"], [])


def _back_to_back():
    g = G()
    nodes = g.new(4)
    want = []
    for i, (l0, l1) in enumerate([(1, 1), (2, 1), (1, 3)]):
        g.bubble(nodes[i], nodes[i + 1], l0, l1, flip=i & 1)
        want.append((nodes[i], nodes[i + 1], l0, l1))
    case("back-to-back", g, 8, ["back_to_back"], want)


def _twin_placements():
    g = G()
    v, w = g.new(2)
    g.bubble(v, w, 1, 2)  # v < w ^ 1: reported as drawn
    w2, v2 = g.new(2)
    a0, a1 = g.bubble(v2, w2, 1, 2)  # v2 > w2 ^ 1: its twin is reported, arms reversed and flipped
    case("twin-placements", g, 8, ["twin_low", "twin_high"], [(v, w, 1, 2), (w2 ^ 1, v2 ^ 1, 1, 2)])


def _sink_at_end():
    g = G()
    (v,) = g.new()
    a = g.new(3)
    (w,) = g.new(flip=1)
    g.chain([v, a[0], w])
    g.chain([v, a[1], a[2], w])
    case("sink-at-2n-1", g, 8, ["sink_at_2n_1", "source_at_0", "arms_1_2"], [(v, w, 1, 2)])


EDGE_SOURCES = [255, 256, 257, 511, 512, 1023, 1024, 2047, 2048, 2049, 4095, 4096]


def _block_edges():
    g = G(reserved=2100)  # strings 0 .. 2099 exist; the sources are taken from them, the rest stay alone
    want = []
    for i, v in enumerate(EDGE_SOURCES):
        (w,) = g.new()
        g.bubble(v, w, 1 + i % 2, 1 + i % 3)
        want.append((v, w, 1 + i % 2, 1 + i % 3))
    case("block-edges", g, 8, ["sources_255_256_257", "scan_block_edges"], want)


def _many():
    rng = random.Random(5)
    g = G()
    node, want = g.new()[0], []
    for i in range(1500):
        (nxt,) = g.new(flip=rng.randrange(2))
        l0, l1 = rng.randrange(1, 3), rng.randrange(1, 3)
        g.bubble(node, nxt, l0, l1, flip=rng.randrange(2))
        want.append((node, nxt, l0, l1))
        node = nxt
    case("many-bubbles", g, 2, ["many", "back_to_back"], want)


def _degenerate():
    case("no-strings", G(), 8, ["no_strings"], [])
    case("one-string", G(reserved=1), 8, ["one_string", "no_links"], [])
    case("no-links", G(reserved=5), 8, ["no_links"], [])


_max_arm_1()
_hairpins()
_fans(3)
_fans(4)
_different_sinks()
_sink_indeg_3()
_side("exit")
_side("entry")
_tip()
_rings()
_self_link()
_back_to_back()
_twin_placements()
_sink_at_end()
_block_edges()
_many()
_degenerate()


# ---- the families built from strings -----------------------------------------------------------------------------

def colored_unitigs(samples, k):
    """The coloured unitigs of `samples` (strings over ACGT), by a small merger over the links of the k-mers:
    (strings, string_class, rows).  Every canonical k-mer is a string of its own with the samples that hold it as
    its row; links_ref.links gives the de Bruijn edges; v -> w is merged when it is v's only link out, w's only link
    in, both have the same row and they are different k-mers.  Classes are the distinct rows, ascending by (high
    word, low word) as ksh_kss_color_classes orders them."""
    member = {}
    for i, t in enumerate(samples):
        for p in range(len(t) - k + 1):
            key = links_ref.canon(t[p:p + k])
            member[key] = member.get(key, 0) | 1 << i
    return colored_unitigs_of(member, k)


def colored_unitigs_of(member, k):
    """colored_unitigs of k-mer sets: member[canonical k-mer] is the bit mask of the columns that hold it."""
    kmers = sorted(member)
    off, to = links_ref.links(kmers, k, True)
    outdeg, _ = ref.degrees(off)

    def step(v):
        """The vertex merged behind v, or None."""
        if outdeg[v] != 1:
            return None
        w = int(to[off[v]])
        if outdeg[w ^ 1] != 1 or member[kmers[w >> 1]] != member[kmers[v >> 1]] or w >> 1 == v >> 1:
            return None
        return w

    used, strings, bits = set(), [], []
    for s in range(len(kmers)):
        if s in used:
            continue
        used.add(s)
        path = [2 * s]
        for end in (0, 1):  # forwards, then forwards from the twin of the first: backwards
            v = path[-1]
            while True:
                v = step(v)
                if v is None or v >> 1 in used:
                    break
                used.add(v >> 1)
                path.append(v)
            if end == 0:
                path = [x ^ 1 for x in reversed(path)]
        strings.append(ref.spell(kmers, k, path))
        bits.append(member[kmers[s]])
    table = sorted(set(bits), key=lambda b: (b >> 64, b & (2 ** 64 - 1)))
    rows = np.array([[b & (2 ** 64 - 1), b >> 64] for b in table], dtype=np.uint64)
    return strings, np.array([table.index(b) for b in bits], dtype=np.int32), rows


def family(seed, k, length, n_genomes, n_sites, n_close, partial):
    """A seeded family: a random genome, n_sites substitution sites at least K from each other and from the ends
    plus n_close sites one to K - 1 behind some of them (two substitutions closer than K: no simple bubble), every
    genome taking the alternative base at a random half of the sites; and, for each (genome, site, shift) of
    `partial`, a sample that is that genome up to `shift` bases behind the site, so that it covers half of an arm.
    Returns a dict with the samples, the coloured unitigs, their links and what the tests ask of them."""
    rng = random.Random(seed)
    base = "".join(rng.choice("ACGT") for _ in range(length))
    sites = []
    while len(sites) < n_sites:
        p = rng.randrange(2 * k, length - 2 * k)
        if all(abs(p - q) >= 3 * k for q in sites):
            sites.append(p)
    sites.sort()
    close = [p + rng.randrange(1, k) for p in sites[:n_close]]
    alt = {p: rng.choice([b for b in "ACGT" if b != base[p]]) for p in sites + close}
    takes = [{p for p in sites + close if rng.randrange(2)} for _ in range(n_genomes)]
    takes[0], takes[1] = set(), set(sites + close)  # (every site has both alleles)
    genomes = ["".join(alt[p] if p in t else b for p, b in enumerate(base)) for t in takes]
    samples = genomes + [genomes[g][:sites[i] + shift + 1] for g, i, shift in partial]
    isolated = [p for p in sites if all(abs(p - q) >= k for q in sites + close if q != p)]
    strings, cls, rows = colored_unitigs(samples, k)
    off, to = links_ref.links(strings, k, True)
    return dict(id="family-%d" % seed, seed=seed, k=k, samples=samples, genomes=genomes, isolated=isolated,
                close=close, partial=[(n_genomes + j, sites[i]) for j, (_, i, _) in enumerate(partial)],
                strings=strings, string_class=cls, rows=rows, off=off, to=to, n=len(strings), max_arm=4)


# (seed, K, length, genomes, sites, close pairs, partial samples).  The seeds are those for which
# test_link_bubbles_reference_cpu.py holds with the reference alone: no (K - 1)-mer of the samples repeats.
FAMILY_ARGS = [(11, 15, 900, 4, 8, 2, [(0, 3, 3), (1, 4, 7)]),
               (12, 17, 1500, 6, 14, 3, [(2, 4, 2), (3, 5, 5), (0, 9, 9)])]
_FAMILIES = {}


def families():
    """The two families, built once."""
    if not _FAMILIES:
        for args in FAMILY_ARGS:
            f = family(*args)
            _FAMILIES[f["id"]] = f
    return list(_FAMILIES.values())

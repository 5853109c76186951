"""Planted truth for capi.place_bubbles and capi.vcf_lines (host only): the two substitution families of
tests/link_bubbles_cases.py placed on several references, a small indel family, and one reference per reason for
which a bubble stays unplaced.  The graph side comes from the host references: tests/link_bubbles_reference.py for
the bubbles, tests/seq_locate_reference.py for the located ends."""
import random

import link_bubbles_cases as bc
import link_bubbles_reference as bubbles_ref
import seq_locate_reference as locate_ref
import spss_links_reference as links_ref
from kmersets import capi

rc = locate_ref.rc


def trim(start, ref, alt):
    """The trimming of the definition: common trailing bases first, then common leading ones, each while both
    alleles are longer than one base.  start is 0-based; returns (POS, REF, ALT) with POS 1-based."""
    while len(ref) > 1 and len(alt) > 1 and ref[-1] == alt[-1]:
        ref, alt = ref[:-1], alt[:-1]
    while len(ref) > 1 and len(alt) > 1 and ref[0] == alt[0]:
        ref, alt, start = ref[1:], alt[1:], start + 1
    return start + 1, ref, alt


def records(fam, reference, max_arm, canonical=True):
    """place_bubbles of the family's graph on `reference` (a list of strings), everything from the host references."""
    k = fam["k"]
    ends, arm_off, arm, arm_rows = bubbles_ref.bubbles(fam["off"], fam["to"], max_arm, fam["string_class"], fam["rows"])
    where, count = locate_ref.locate(fam["strings"], reference, k, canonical)
    return capi.place_bubbles(fam["strings"], k, ends, arm_off, arm, where, count, reference, arm_rows,
                              len(fam["samples"]))


def placed(recs):
    return [r for r in recs if "unplaced" not in r]


def two_contigs(genome, k, sites):
    """The genome cut half way between two neighbouring sites in the middle, the contigs overlapping by K + 4 bases:
    a few k-mers of the overlap lie in both, none of them next to a site.  Returns (contigs, start of the second)."""
    i = len(sites) // 2
    cut = (sites[i - 1] + sites[i]) // 2
    return [genome[:cut + k + 4], genome[cut:]], cut


# ---- the indel family ------------------------------------------------------------------------------------------------
INDEL_K = 15
# (kind, length): insertions and deletions of 1 to K bases; "str" is an insertion of one more unit behind a short
# tandem repeat, where the trimmed alleles move to the left end of the repeat
INDEL_SPECS = [("ins", 1), ("del", 1), ("ins", 5), ("del", 7), ("str", 2), ("ins", INDEL_K), ("del", INDEL_K), ("ins", 3)]
INDEL_SEED = 4


def indel_family(seed=INDEL_SEED, k=INDEL_K, length=800):
    """A random genome with one indel per spec at sites 4 K apart; genome 0 is the base, genome 1 takes every indel,
    genome 2 every other one.  planted: [(start, ref, alt)] in base coordinates, untrimmed: the K - 1 bases before the
    event, the event, the K - 1 bases behind it."""
    rng = random.Random(seed)
    base = [rng.choice("ACGT") for _ in range(length)]
    sites = [3 * k + 4 * k * i + rng.randrange(k) for i in range(len(INDEL_SPECS))]
    events = []
    for p, (kind, n) in zip(sites, INDEL_SPECS):
        if kind == "str":
            base[p - 6:p] = "ACACAC"
            if base[p - 7] == "C":
                base[p - 7] = "G"
            if base[p] == "A":
                base[p] = "T"
            events.append((p, "", "AC"))
        elif kind == "ins":
            events.append((p, "", "".join(rng.choice("ACGT") for _ in range(n))))
        else:
            events.append((p, "".join(base[p:p + n]), ""))
    base = "".join(base)

    def genome(take):
        out, at = [], 0
        for i, (p, gone, new) in enumerate(events):
            out.append(base[at:p])
            at = p
            if take(i):
                out.append(new)
                at = p + len(gone)
        return "".join(out) + base[at:]

    genomes = [base, genome(lambda i: True), genome(lambda i: i % 2 == 0)]
    planted = [(p - (k - 1), base[p - (k - 1):p + len(gone) + k - 1],
                base[p - (k - 1):p] + new + base[p + len(gone):p + len(gone) + k - 1]) for p, gone, new in events]
    strings, cls, rows = bc.colored_unitigs(genomes, k)
    off, to = links_ref.links(strings, k, True)
    return dict(id="indels-%d" % seed, seed=seed, k=k, samples=genomes, genomes=genomes, events=events, planted=planted,
                takes=[[0] * len(events), [1] * len(events), [1 - i % 2 for i in range(len(events))]],
                strings=strings, string_class=cls, rows=rows, off=off, to=to, n=len(strings), max_arm=4)


_INDELS = {}


def indels():
    if not _INDELS:
        _INDELS["f"] = indel_family()
    return _INDELS["f"]


def repeated(samples, k):
    """The (K - 1)-mers that lie, up to reverse complement, at two places of one sample."""
    twice = set()
    for t in samples:
        here = set()
        for p in range(len(t) - k + 2):
            x = links_ref.canon(t[p:p + k - 1])
            if x in here:
                twice.add(x)
            here.add(x)
    return twice


# ---- one reference per reason ----------------------------------------------------------------------------------------
def unplaced_cases():
    """[(reason, reference, (v, w) of the bubble that stays unplaced for it)] on family 11 with genome 0: the bubble
    of the first isolated site."""
    fam = bc.families()[0]
    k, genome = fam["k"], fam["genomes"][0]
    p = fam["isolated"][1]
    rec = next(r for r in placed(records(fam, [genome], 4)) if r["pos"] == p + 1)
    # the anchors of that bubble on genome 0: the source's end k-mer ends right before the site, the sink's starts
    # right behind it (the unitigs break at the site and nowhere nearer)
    p_a, p_b = p - k, p + 1
    source, sink = genome[p_a:p_a + k], genome[p_b:p_b + k]
    rng = random.Random(3)
    junk = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    third = next(b for b in "ACGT" if b not in (rec["ref"], rec["alt"]))
    return [
        ("anchor", [genome, junk(9) + source + junk(6)], (rec["v"], rec["w"])),
        ("apart", [genome[:p_a + k], genome[p_a + 1:]], (rec["v"], rec["w"])),
        ("order", [genome[p_b:p_b + k + 20] + junk(5) + genome[p_a - 20:p_a + k]], (rec["v"], rec["w"])),
        ("off", [genome[:p] + third + genome[p + 1:]], (rec["v"], rec["w"])),
    ]

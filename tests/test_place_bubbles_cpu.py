"""capi.place_bubbles and capi.vcf_lines against planted truth, host only (tests/place_bubbles_cases.py): the
substitution families on genome 0, genome 1, the reverse complement of genome 0 and genome 0 in two overlapping
contigs, the genotypes against the planted alleles, the indel family, one reference per unplaced reason, and the VCF
text parsed back.

Worked out beforehand with the references alone (the counts below are those runs' results, not the code's under test:
place_bubbles is checked against the planted sites, the counts only pin how many of them are bubbles):
  family 11: 4 bubbles at max_arm 1, 6 at 2 and 4; family 12: 9, 12, 12, one of them the 17-base MNP at POS 109 of
  genome 0 from a close pair that only two haplotype combinations carry.  On the reverse complement a record
  (POS, REF, ALT) of genome 0 becomes (L - POS - len(REF) + 2, rc(REF), rc(ALT)); on two contigs it keeps its
  alleles and moves to the contig that holds it."""
import pytest

import link_bubbles_cases as bc
import place_bubbles_cases as pc
from kmersets import capi

FAMILIES = bc.families()
N_BUBBLES = {"family-11": {1: 4, 2: 6, 4: 6}, "family-12": {1: 9, 2: 12, 4: 12}}


def key(r):
    return (r["seq"], r["pos"], r["ref"], r["alt"])


@pytest.mark.parametrize("max_arm", [1, 2, 4])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f["id"] for f in FAMILIES])
def test_substitution_sites_on_a_genome(fam, which, max_arm):
    genome, other = fam["genomes"][which], fam["genomes"][1 - which]
    recs = pc.records(fam, [genome], max_arm)
    assert len(recs) == N_BUBBLES[fam["id"]][max_arm] and len(pc.placed(recs)) == len(recs)  # none is unplaced
    by_pos = {r["pos"]: r for r in recs}
    assert len(by_pos) == len(recs)
    found = [p for p in fam["isolated"] if p + 1 in by_pos]
    assert len(found) >= 4 and (max_arm < 2 or found == fam["isolated"])
    for p in found:
        r = by_pos[p + 1]
        assert (r["seq"], r["ref"], r["alt"]) == (0, genome[p], other[p]) and genome[p] != other[p]
    for r in recs:  # whatever else is placed spells the reference, and its ALT is what some genome has there
        at = r["pos"] - 1
        assert genome[at:at + len(r["ref"])] == r["ref"] and len(r["alt"]) == len(r["ref"])
        assert any(g[at:at + len(r["alt"])] == r["alt"] for g in fam["genomes"])
    if fam["id"] == "family-12":
        mnp = by_pos[109]
        assert len(mnp["ref"]) == len(mnp["alt"]) == 17 and mnp["ref"][0] != mnp["alt"][0]
        assert mnp["ref"][-1] != mnp["alt"][-1] and mnp["ref"][1:-1] == mnp["alt"][1:-1]
        assert 109 - 1 + 16 in fam["close"]  # its last base is the close partner of the site at its first


@pytest.mark.parametrize("fam", FAMILIES, ids=[f["id"] for f in FAMILIES])
def test_genotypes_are_the_planted_alleles(fam):
    genome = fam["genomes"][0]
    recs = pc.records(fam, [genome], 4)
    by_pos = {r["pos"]: r for r in recs}
    n_genomes = len(fam["genomes"])
    for p in fam["isolated"]:
        gt = by_pos[p + 1]["gt"]
        assert len(gt) == len(fam["samples"])
        assert gt[:n_genomes] == ["0" if g[p] == genome[p] else "1" for g in fam["genomes"]]
        assert gt[0] == "0" and gt[1] == "1"
    for sample, site in fam["partial"]:  # a sample that ends inside the arms holds neither arm whole
        assert by_pos[site + 1]["gt"][sample] == "."
        t = fam["samples"][sample]
        for p in fam["isolated"]:
            if p + fam["k"] < len(t) - fam["k"]:      # well inside the sample: its genome's allele
                assert by_pos[p + 1]["gt"][sample] == ("0" if t[p] == genome[p] else "1")
            elif p > len(t):                           # behind its end
                assert by_pos[p + 1]["gt"][sample] == "."
    # without carriers there are no genotypes
    k = fam["k"]
    import link_bubbles_reference as bubbles_ref
    import seq_locate_reference as locate_ref

    ends, arm_off, arm, _ = bubbles_ref.bubbles(fam["off"], fam["to"], 4)
    where, count = locate_ref.locate(fam["strings"], [genome], k, True)
    bare = capi.place_bubbles(fam["strings"], k, ends, arm_off, arm, where, count, [genome])
    assert [key(r) for r in bare] == [key(r) for r in recs] and all(r["gt"] is None for r in bare)


@pytest.mark.parametrize("max_arm", [1, 2, 4])
@pytest.mark.parametrize("fam", FAMILIES, ids=[f["id"] for f in FAMILIES])
def test_reverse_complement_reference(fam, max_arm):
    genome = fam["genomes"][0]
    forward = pc.records(fam, [genome], max_arm)
    back = pc.records(fam, [pc.rc(genome)], max_arm)
    assert len(pc.placed(back)) == len(back) == len(forward)
    want = sorted((0, len(genome) - r["pos"] - len(r["ref"]) + 2, pc.rc(r["ref"]), pc.rc(r["alt"])) for r in forward)
    assert sorted(key(r) for r in back) == want
    gt = {(r["v"], r["w"]): r["gt"] for r in forward}
    assert all(r["gt"] == gt[(r["v"], r["w"])] for r in back)  # the same bubbles, the same carriers


@pytest.mark.parametrize("fam", FAMILIES, ids=[f["id"] for f in FAMILIES])
def test_two_overlapping_contigs(fam):
    genome, k = fam["genomes"][0], fam["k"]
    contigs, start = pc.two_contigs(genome, k, fam["isolated"])
    assert contigs[0][start:] == contigs[1][:k + 4] and contigs[0][:start] + contigs[1] == genome
    whole = pc.records(fam, [genome], 4)
    recs = pc.records(fam, contigs, 4)
    assert len(pc.placed(recs)) == len(recs) == len(whole)
    want = sorted((0, r["pos"], r["ref"], r["alt"]) if r["pos"] - 1 < start else
                  (1, r["pos"] - start, r["ref"], r["alt"]) for r in whole)
    assert sorted(key(r) for r in recs) == want and {w[0] for w in want} == {0, 1}


def test_indel_family():
    fam = pc.indels()
    k, base = fam["k"], fam["genomes"][0]
    assert not pc.repeated(fam["samples"], k)  # the seed's property, as the substitution families'
    assert {n for kind, n in pc.INDEL_SPECS if kind != "str"} >= {1, k} and len(fam["planted"]) == len(pc.INDEL_SPECS)
    want = sorted((0,) + pc.trim(*planted) for planted in fam["planted"])
    recs = pc.records(fam, [base], 4)
    assert len(pc.placed(recs)) == len(recs)
    assert sorted(key(r) for r in recs) == want
    for (seq, pos, ref, alt), (p, gone, new) in zip(want, fam["events"]):
        assert ref[0] == alt[0] and min(len(ref), len(alt)) == 1           # the padding base stays
        assert (len(ref) - 1, len(alt) - 1) == (len(gone), len(new)) and base[pos - 1:pos - 1 + len(ref)] == ref
    # the insertion behind the tandem repeat is reported at the repeat's left end
    i = [kind for kind, _ in pc.INDEL_SPECS].index("str")
    p = fam["events"][i][0]
    assert base[p - 6:p] == "ACACAC" and want[i][1:] == (p - 7 + 1, base[p - 7], base[p - 7] + "AC")
    # genotypes: the planted takes
    by_pos = {r["pos"]: r["gt"] for r in recs}
    for j, w in enumerate(want):
        assert by_pos[w[1]] == [str(t[j]) for t in fam["takes"]]
    # placed on genome 1, which takes every indel, REF and ALT change places
    other = pc.records(fam, [fam["genomes"][1]], 4)
    assert len(pc.placed(other)) == len(recs)
    assert sorted((len(r["ref"]), len(r["alt"])) for r in other) == sorted((len(r["alt"]), len(r["ref"])) for r in recs)


def test_every_unplaced_reason():
    fam = FAMILIES[0]
    whole = pc.records(fam, [fam["genomes"][0]], 4)
    seen = set()
    for reason, reference, (v, w) in pc.unplaced_cases():
        recs = pc.records(fam, reference, 4)
        assert len(recs) == len(whole)
        mine = next(r for r in recs if (r["v"], r["w"]) == (v, w))
        assert mine.get("unplaced") == reason and set(mine) == {"v", "w", "unplaced"}, (reason, mine)
        if reason in ("anchor", "apart", "off"):  # the other bubbles are placed as ever
            assert sum("unplaced" in r for r in recs) == 1
        seen.add(reason)
        lines, counts = capi.vcf_lines(recs, ["c%d" % i for i in range(len(reference))], [len(t) for t in reference])
        assert counts[reason] >= 1 and sum(counts.values()) == len(recs)
        assert sum(not line.startswith("#") for line in lines) == counts["placed"]
    assert seen == set(capi.UNPLACED_REASONS)


def test_vcf_lines_parse_back(tmp_path):
    fam = FAMILIES[1]
    genome = fam["genomes"][0]
    contigs, _ = pc.two_contigs(genome, fam["k"], fam["isolated"])
    recs = pc.records(fam, contigs, 4)
    names = ["left", "right"]
    samples = ["s%d" % i for i in range(len(fam["samples"]))]
    lines, counts = capi.vcf_lines(recs, names, [len(c) for c in contigs], samples)
    assert counts == {"placed": len(recs), "anchor": 0, "apart": 0, "order": 0, "off": 0}
    assert lines[0] == "##fileformat=VCFv4.2"
    assert lines[1:3] == ["##contig=<ID=left,length=%d>" % len(contigs[0]), "##contig=<ID=right,length=%d>" % len(contigs[1])]
    assert sum(line.startswith("##INFO=<ID=BUB,") for line in lines) == 1
    assert sum(line.startswith("##FORMAT=<ID=GT,") for line in lines) == 1
    head = next(line for line in lines if line.startswith("#CHROM"))
    assert head.split("\t") == ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples
    body = [line.split("\t") for line in lines if not line.startswith("#")]
    assert lines.index(head) + 1 + len(body) == len(lines)
    back = []
    for f in body:
        assert f[2] == f[5] == f[6] == "." and f[8] == "GT" and f[7].startswith("BUB=")
        v, w = (int(x) for x in f[7][4:].split(","))
        back.append({"v": v, "w": w, "seq": names.index(f[0]), "pos": int(f[1]), "ref": f[3], "alt": f[4], "gt": f[9:]})
    assert back == sorted(recs, key=key)
    assert [key(r) for r in back] == sorted(key(r) for r in back)
    # the file, and a call without carriers or names
    path = tmp_path / "sites.vcf"
    assert capi.write_vcf(str(path), recs, names, [len(c) for c in contigs], samples) == counts
    assert path.read_text() == "".join(line + "\n" for line in lines)
    bare = [dict(r, gt=None) for r in recs]
    lines, _ = capi.vcf_lines(bare, names, [len(c) for c in contigs])
    assert not any("FORMAT" in line for line in lines) and all(len(line.split("\t")) == 8 for line in lines if line[0] != "#")
    default = capi.vcf_lines(recs, names, [len(c) for c in contigs])[0]
    assert next(line for line in default if line.startswith("#CHROM")).endswith("\tS0\t" + "\t".join(
        "S%d" % i for i in range(1, len(samples))))
    with pytest.raises(ValueError):
        capi.vcf_lines(recs, names, [len(c) for c in contigs], samples[:-1])

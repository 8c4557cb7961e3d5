"""The panels of tests/test_gpu_cli.py's device-decode cases: one wide enough to take the device decode of its sample columns by
itself, and a small one with an allele number beyond a record's ALT list.  Built with malva_amd.synth (the product's generator, no
GPU); tests/test_gt_text_cases_cpu.py checks from the bytes that they hold what the CLI cases need."""
from collections import namedtuple

import numpy as np

from gt_text_cases import PHASED0

# ---- `call` on a panel that takes the device path by itself (tests/test_gpu_cli.py) ----------------------------------------------
CALL_SAMPLES, CALL_RECORDS, CALL_RUN, CALL_CUT_BATCH = 1030, 2200, 300, 100
WIDE_ALTS = 130                          # a record of 131 alleles: its samples' allele numbers 127, 128 and 129 do not fit the 7-bit words
WIDE_GTS = {5: "127|0", 6: "0|128", 7: "129/129", 1029: "128|127"}
CallPanel = namedtuple("CallPanel", "prefix panel wide_lone wide_clustered")


def _wide_line(line, rng):
    """the record with WIDE_ALTS ALT alleles (its own first, then insertions behind the REF base) and WIDE_GTS in its sample columns"""
    f = line.split("\t")
    alts = [f[4]]
    while len(alts) < WIDE_ALTS:
        a = f[3] + "".join(rng.choice(list("ACGT"), size=4))
        if a not in alts:
            alts.append(a)
    f[4] = ",".join(alts)
    f[7] = "AF=" + ",".join(["0.001"] * WIDE_ALTS)
    for s, g in WIDE_GTS.items():
        f[9 + s] = g
    return "\t".join(f)


def call_panel(prefix, seed=41, wide=True):
    """CALL_RECORDS mostly lone SNPs of CALL_SAMPLES diploid samples, a few dozen clusters among them; runs of CALL_RUN records in which
    0/0 and 0|0 take turns as the commonest word (about 1 % of a record's samples carry something else); with `wide`, two records of
    WIDE_ALTS ALT alleles, one alone and one inside a cluster (the same two records stay SNPs without it) -> CallPanel (<prefix>.fa,
    <prefix>.vcf)"""
    from malva_amd import synth
    rng = np.random.default_rng(seed)
    panel = synth.clustered_snp_panel(CALL_RECORDS, seed, n_contigs=2, cluster_frac=0.04, n_samples=CALL_SAMPLES)
    n = panel.n
    phased_run = (np.arange(n) // CALL_RUN) % 2 == 1                     # the first run is unphased-heavy
    gt = np.where(phased_run[:, None], np.uint16(PHASED0), np.uint16(0)) * np.ones((n, CALL_SAMPLES), np.uint16)
    carriers = rng.random((n, CALL_SAMPLES)) < 0.01
    carriers[np.arange(n), rng.integers(0, CALL_SAMPLES, size=n)] = True     # every ALT is carried
    words = np.array([1, 1 << 7, 1 | 1 << 7, 1 | PHASED0, 1 << 7 | PHASED0, 1 | 1 << 7 | PHASED0, 0, PHASED0], np.uint16)
    picks = words[rng.integers(0, len(words), size=(n, CALL_SAMPLES))]
    picks[np.arange(n), np.argmax(carriers, axis=1)] = np.uint16(1 | PHASED0)
    panel.gt = np.where(carriers, picks, gt).astype(np.uint16)
    synth.write_vcf_fasta(panel, prefix)
    gap_before = np.full(n, 1 << 30, np.int64)
    same = panel.contig_id[1:] == panel.contig_id[:-1]
    gap_before[1:][same] = np.diff(panel.pos.astype(np.int64))[same]
    gap_after = np.append(gap_before[1:], 1 << 30)
    near = np.minimum(gap_before, gap_after)
    inside = np.arange(n) % CALL_RUN
    ok = (inside > 110) & (inside < 190) & (np.arange(n) > CALL_RUN)
    wide_lone = int(np.flatnonzero(ok & (near > 40))[0])
    wide_clustered = int(np.flatnonzero(ok & (near <= 17) & (np.arange(n) > wide_lone + 5))[0])
    lines = open(prefix + ".vcf").read().split("\n")
    first = next(i for i, l in enumerate(lines) if l and not l.startswith("#"))
    for v in (wide_lone, wide_clustered) if wide else ():
        lines[first + v] = _wide_line(lines[first + v], rng)
    with open(prefix + ".vcf", "w") as fh:
        fh.write("\n".join(lines))
    return CallPanel(prefix, panel, wide_lone, wide_clustered)


BEYOND_ALLELES = ("5", "128", "32768", "2147483648", "4294967296")       # against a record of 3 alleles
BEYOND_RECORDS, BEYOND_AT, BEYOND_SAMPLE = 40, 20, 7


def beyond_panel(prefix, seed=43):
    """BEYOND_RECORDS records of CALL_SAMPLES samples, record BEYOND_AT with two ALT alleles -> (lines of the VCF, index of that record's line)"""
    from malva_amd import synth
    panel = synth.clustered_snp_panel(BEYOND_RECORDS, seed, n_contigs=1, n_samples=CALL_SAMPLES)
    synth.write_vcf_fasta(panel, prefix)
    lines = open(prefix + ".vcf").read().split("\n")
    at = next(i for i, l in enumerate(lines) if l and not l.startswith("#")) + BEYOND_AT
    f = lines[at].split("\t")
    f[4] = f[4] + "," + f[3] + "GG"
    f[7] = "AF=0.2,0.1"
    f[9 + BEYOND_SAMPLE - 1] = "2|1"
    lines[at] = "\t".join(f)
    return lines, at


def write_beyond(prefix, lines, at, allele):
    """the panel with `allele`|0 in sample BEYOND_SAMPLE of the three-allele record (None: 2|0, inside its ALT list) -> that record's (SEQ, POS)"""
    f = lines[at].split("\t")
    f[9 + BEYOND_SAMPLE] = "%s|0" % (allele if allele is not None else "2")
    with open(prefix + ".vcf", "w") as fh:
        fh.write("\n".join(lines[:at] + ["\t".join(f)] + lines[at + 1:]))
    return f[0], int(f[1])

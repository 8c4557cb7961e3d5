"""`call --cohort --cohort-priors --prior-groups` end to end, on the two cohorts of tests/test_gpu_cohort_priors_cli.py with
MALVA_GENO_BATCH=400 (several batches): a cohort that runs as several groups -- coverage pass per group, estimate pass over all
of them, output pass per group -- writes byte for byte what the one-group run writes, in every output (-o, --merged in text and BCF
with --gp, --site-tags and -v, --pairs, --sample-stats, --priors-out; the BCF as its inflated stream), and leaves no scratch behind.  The coverages stay far below
65536 a record, where the identity holds.

A 70-sample manifest over the haploid cohort's six inputs is a cohort no single group holds: its groupings agree with each other,
samples that share an input share their columns, more than 64 samples inform a record, and the table's COHORT_AF written into the
panel gives the same columns in a plain run."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from test_bcf_out_cpu import bgzf_members
from test_gpu_cohort import BIN, _cli
from test_gpu_cohort_priors_cli import _call, _records, cohort  # noqa: F401 (cohort: the module's fixture, made again for this module)

pytestmark = pytest.mark.gpu

GROUPS = ["--cohort-priors", "--prior-groups"]


def _parts(root):
    return [os.path.join(d, n) for d, _, names in os.walk(str(root)) for n in names if n.endswith(".part")]


def _run(c, out, extra, table, **kw):
    """one run with --priors-out -> its files, the table among them"""
    files = _call(c, out, extra + ["--priors-out", str(table)], **kw)
    files["priors.tsv"] = open(str(table), "rb").read()
    assert not os.path.exists(str(table) + ".part")
    return files


def _same(a, b, what, bgzf=False):
    """every file byte for byte; bgzf: the merged file is a BCF in BGZF members, whose cuts follow the grouping with or without
    --cohort-priors (one group compresses batch by batch, the paste pass its own pieces) -- the inflated stream is the file"""
    assert sorted(a) == sorted(b) and len(a) >= 6, (what, sorted(a), sorted(b))
    for n in a:
        if bgzf and n == "merged":
            x, y = (b"".join(raw for _, raw in bgzf_members(f[n])) for f in (a, b))
            assert len(x) > 1000 and x == y, (what, n, "inflated")
        else:
            assert a[n] == b[n], (what, n)


_ONE = {}


def _one_group(c, fmt=None, iso=False):
    """the one-group --cohort-priors run of a cohort, made once and shared"""
    key = (c["kind"], fmt, iso)
    if key not in _ONE:
        tag = "g_one_%s%s" % (fmt or "txt", "_iso" if iso else "")
        _ONE[key] = _run(c, c["tmp"] / tag, ["--cohort-priors"], c["tmp"] / (tag + ".tsv"), merged_format=fmt,
                         env=dict(c["env"], MALVA_GENO_ISO_PATH="1") if iso else None)
    return _ONE[key]


def test_several_groups_write_what_one_group_writes(cohort):
    c, tmp = cohort, cohort["tmp"]
    for fmt in (None, "bcf"):
        tag = fmt or "txt"
        two = _run(c, tmp / ("g_two_" + tag), GROUPS + ["--cohort-group", "2"], tmp / ("g_two_%s.tsv" % tag), merged_format=fmt)
        _same(_one_group(c, fmt), two, "--cohort-group 2 " + tag, bgzf=bool(fmt))
    each = _run(c, tmp / "g_each", GROUPS + ["--cohort-group", "1"], tmp / "g_each.tsv")
    _same(_one_group(c), each, "--cohort-group 1")
    # --prior-groups with a cohort that runs as one group anyway: the run without it
    whole = _run(c, tmp / "g_whole", GROUPS, tmp / "g_whole.tsv")
    _same(_one_group(c), whole, "--prior-groups, one group")
    assert not _parts(tmp)


def test_record_ranges_the_host_enumerator_and_lone_records(cohort):
    c, tmp = cohort, cohort["tmp"]
    two = GROUPS + ["--cohort-group", "2"]
    # every batch cut into several record ranges (2 KiB hold some 85 slots of six planes, 170 of three)
    cut = _run(c, tmp / "g_cut", two, tmp / "g_cut.tsv", env=dict(c["env"], MALVA_GENO_PRIOR_RANGE_BYTES="2048"))
    _same(_one_group(c), cut, "record ranges")
    # every block enumerated on the host
    host = _run(c, tmp / "g_host", two, tmp / "g_host.tsv", env=dict(c["env"], MALVA_GENO_HOST_ENUM="1"))
    _same(_one_group(c), host, "host enumerator")
    if c["kind"] == "diploid":                                                        # the batches of lone records
        two_iso = _run(c, tmp / "g_two_iso", two, tmp / "g_two_iso.tsv", env=dict(c["env"], MALVA_GENO_ISO_PATH="1"))
        _same(_one_group(c, iso=True), two_iso, "--cohort-group 2, lone records")
    assert not _parts(tmp)


def test_the_timers_name_the_three_passes(cohort):
    c, tmp = cohort, cohort["tmp"]
    out = tmp / "g_timers"
    r = subprocess.run([BIN, "call"] + c["opts"] + ["--cohort", "--merged", str(out)] + GROUPS + ["--cohort-group", "2", c["fa"], c["vcf"], c["manifest"]],
                       capture_output=True, text=True, timeout=300, env=dict(c["env"], MALVA_GENO_TIMERS="1"))
    assert r.returncode == 0, r.stderr
    for name in ("cohort: coverage pass", "cohort: estimate pass", "cohort: output pass", "mg_estimate_priors, device ms per call"):
        assert name in r.stderr, name
    assert not _parts(tmp)


def test_refusals(cohort):
    """--prior-groups without --cohort-priors: refused with the options, nothing written, no device; without --prior-groups a
    --cohort-group below the cohort is refused as before"""
    c, tmp = cohort, cohort["tmp"]
    out = tmp / "g_refused"
    for extra, words in ((["--prior-groups"], ("--prior-groups goes with --cohort-priors",)),
                         (["--cohort-priors", "--cohort-group", "2"], ("--cohort-group 2", "--cohort-priors", "one group"))):
        r = subprocess.run([BIN, "call"] + c["opts"] + ["--cohort", "-o", str(out)] + extra + [c["fa"], c["vcf"], c["manifest"]], capture_output=True, text=True,
                           timeout=300, env=c["env"])
        assert r.returncode != 0 and all(w in r.stderr for w in words) and "HIP device" not in r.stderr and r.stdout == "", (extra, r.stderr[-400:])
        assert not os.path.exists(str(out))


def test_seventy_samples(cohort):
    c, tmp = cohort, cohort["tmp"]
    if c["kind"] != "haploid":
        return                                                                        # (the manifest cycles through the haploid cohort's inputs)
    inputs = [l.split("\t") for l in open(c["manifest"]).read().split("\n") if l]
    assert len(inputs) == 6
    manifest = str(tmp / "seventy.tsv")
    open(manifest, "w").write("".join("n%02d_%s\t%s\n" % (i, inputs[i % 6][0], inputs[i % 6][1]) for i in range(70)))
    c70 = dict(c, manifest=manifest)
    wide = _run(c70, tmp / "s_wide", GROUPS, tmp / "s_wide.tsv")                      # 64 + 6
    narrow = _run(c70, tmp / "s_narrow", GROUPS + ["--cohort-group", "16"], tmp / "s_narrow.tsv")
    _same(wide, narrow, "64 + 6 against groups of 16")
    assert not _parts(tmp)
    samples = sorted(n for n in wide if n.startswith("o/"))
    assert len(samples) == 70
    for i in range(6, 70):                                                            # samples that share an input share their columns
        a, b = _records(wide[samples[i]]), _records(wide[samples[i % 6]])
        assert len(a) == len(b) and all(x[8:] == y[8:] for x, y in zip(a, b)), samples[i]
    merged = _records(wide["merged"])
    assert all(len(r) == 9 + 70 for r in merged)
    for r in merged[::37]:
        assert all(r[9 + i] == r[9 + i % 6] for i in range(70))
    rows = [r.split("\t") for r in wide["priors.tsv"].decode().split("\n")[1:-1]]
    assert len(rows) == len(merged) and max(int(r[7]) for r in rows) > 64
    # substitution: the table's COHORT_AF as the panel's AF, the six inputs called plainly: the same sample columns
    vcf2 = str(tmp / "seventy.vcf")
    at_row = n_moved = 0
    with gzip.open(c["vcf"], "rt") as src, open(vcf2, "w") as dst:
        for line in src:
            f = line.rstrip("\n").split("\t")
            if not line.startswith("#") and at_row < len(rows) and f[:5] == rows[at_row][:5]:
                row = rows[at_row]
                at_row += 1
                info = f[7].split(";")
                at = [i for i, kv in enumerate(info) if kv.startswith("AF=")][0]
                if row[5] != ".":
                    n_moved += int(np.float32([float(x) for x in row[5].split(",")]).tolist() != np.float32([float(x) for x in row[6].split(",")]).tolist())
                    info[at] = "AF=" + row[6]
                    f[7] = ";".join(info)
                line = "\t".join(f) + "\n"
            dst.write(line)
    assert at_row == len(rows) and n_moved > 0
    _cli(["index"] + c["index_opts"] + [c["fa"], vcf2, c["third"]], env=c["env"])
    second = _call(c, tmp / "s_second", [], vcf=vcf2, tables=False)
    for i, (name, _) in enumerate(inputs):
        a, b = _records(wide[samples[i]]), _records(second["o/%s.vcf" % name])
        assert len(a) == len(b) == len(rows)
        for x, y in zip(a, b):
            assert x[:5] == y[:5] and x[8:] == y[8:], (name, x, y)

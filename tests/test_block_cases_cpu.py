"""tests/block_cases.py on any machine: every directed panel holds what its name claims (chains, members, reach, picks, bits and
bytes counted with the oracle's Python model, exactly), the restated dealing rules send every record of the cluster where the
case intends -- and nothing outside a cluster to the host -- and the C oracle (mo_cover_blocks, mo_index_blocks: the reference
of the GPU tests) equals the Python model on the clusters: at 17 chains a side, 33 members a side, records that step back in
the file and 15 unphased members, where tests/test_oracle_blocks_cpu.py's random panels never were."""
import numpy as np
import pytest

import block_cases as bc
from block_util import model_coverages
from oracle import capi as ocapi


def _central(case, s):
    b, i = case.flat()[case.central[s]]
    return case.blocks[b][0], i


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_holds_its_claim(name):
    case = bc.get(name)
    cl = case.claim
    assert case.k == cl.get("k", 35) and case.n_samples == cl.get("n_samples", case.n_samples)
    assert max(v.ref_pos for vb, _ in case.blocks for v in vb.variants) < 1 << 24
    for s in range(len(case.central)):
        vb, i = _central(case, s)
        sides = {-1: bc.walk(vb, i, -1), +1: bc.walk(vb, i, +1)}
        for step, (chains, far, _) in sides.items():
            assert chains == vb._chains(i, step), "the restated walk finds the model's chains"
        (L, far_l, back_l), (R, far_r, back_r) = sides[-1], sides[+1]
        combs = vb.combine(L, R, i)
        if "chains_left" in cl:
            assert (len(L), len(R)) == (cl["chains_left"], cl["chains_right"])
            assert max(map(len, L + R)) <= bc.FW_MAXM and max(far_l, far_r) <= bc.FW_REACH       # nothing but the count decides
        if "members_left" in cl:
            assert [len(c) for c in L] == [cl["members_left"]] * bool(cl["members_left"])
            assert [len(c) for c in R] == [cl["members_right"]] * bool(cl["members_right"])
            assert (back_l or back_r) == (max(cl["members_left"], cl["members_right"]) > (case.k + 1) // 2 - 1), "only the 32nd member steps back"
        if "reach_left" in cl:
            assert (far_l, far_r) == (cl["reach_left"], cl["reach_right"])
            assert [abs(c[0] - i) for c in L] == [cl["reach_left"]] * bool(cl["reach_left"]), "the only near record is the farthest one"
            assert [abs(c[0] - i) for c in R] == [cl["reach_right"]] * bool(cl["reach_right"])
            skipped = vb.variants[i - far_l + 1:i] + vb.variants[i + 1:i + far_r]
            assert any(not v.is_present for v in skipped) and any(v.is_present for v in skipped)
        if "unphased_members" in cl:
            assert [len(c) for c in combs] == [cl["unphased_members"]] and bc.unphased_along(vb, combs[0], False)
            assert len(vb.allele_combs(combs[0], i, False)) <= 4 + 2 * (case.n_samples - 1) if cl["unphased_members"] <= 13 else True
        if "code_bits" in cl:
            assert [bc.code_bits(vb, c) for c in combs] == [cl["code_bits"]]
        if "staging" in cl:
            assert [bc.staging_bytes(vb, c) for c in combs] == [cl["staging"]] and bc.FW_POOL // (64 // bc.lanes(case.n_samples)) == 256
        if "picks" in cl:
            assert [bc.n_picks(bc.coded(vb), c, i, case.haploid) for c in combs] == [cl["picks"]]
        if "far" in cl and cl["picks"] == 385:   # the pick beyond the share is a sample's of the second turn, and allele 3's only support
            assert cl["far"] >= 64 and case.n_samples > 64
            for j in combs[0]:
                assert [s_ for s_, g in enumerate(vb.variants[j].genotypes) if 3 in g] == [cl["far"]]
            without = bc.coded(vb)
            for v in without.variants:
                v.genotypes = v.genotypes[:64]
                v.phasing = v.phasing[:64]
            assert bc.n_picks(without, combs[0], i, False) == 384, "samples 0..63 fill the share exactly"
        if "wide_alleles" in cl:
            assert [[len(vb.variants[j].alts) + 1 for j in c] for c in combs] == [[2, cl["wide_alleles"]]]


@pytest.mark.parametrize("k", [35, 32])
def test_tier1_positions_are_the_boundaries(k):
    """the four A-positions panels of a k together put a SNP at k/2 - 1, k/2, k - 1, k, clen - k, clen - k + 1, the last position
    whose right flank fits and the one behind it -- on both sequences"""
    seen = {n: set() for n in bc.genome()}
    for v in range(4):
        case = bc.get("A-positions-k%d-%d" % (k, v))
        for r in case.central:
            b, i = case.flat()[r]
            seen[case.blocks[b][1]].add(case.blocks[b][0].variants[i].ref_pos)
            assert len(case.blocks[b][0].variants) == 1, "lone by spacing"
    for n, clen in ((n, len(s)) for n, s in bc.genome().items()):
        p_max = max(p for p in range(clen) if p + 1 + (k + 1) // 2 <= clen)
        assert seen[n] == {k // 2 - 1, k // 2, k - 1, k, clen - k, clen - k + 1, p_max, p_max + 1}


@pytest.mark.parametrize("name", list(bc.CASES))
def test_rules_send_every_record_where_the_case_intends(name):
    case = bc.get(name)
    for index in (False, True):
        d = bc.deal(case, index)
        n = len(d)
        assert n >= 2000
        per_site = getattr(case, "index_want_per_site" if index else "want_per_site", None) or getattr(case, "want_per_site", None)
        for s, r in enumerate(case.central):
            assert d[r]["tier"] == (per_site[s] if per_site else case.want), "site %d" % s
        in_cluster = {r for site in case.cluster for r in site}
        hosts = [r for r in range(n) if d[r]["tier"] == "host"]
        assert set(hosts) <= in_cluster
        if not per_site:
            assert [sum(d[r]["tier"] == "host" for r in site) for site in case.cluster] == [case.hosts] * len(case.cluster)
        if "listed" in case.claim:
            assert (sum(x["listed"] for x in d) > 0) == case.claim["listed"]
        combs, slides = sum(x["combs"] for x in d), sum(x["slides"] for x in d)
        round_ = min(n, 1 << dict(case.options).get("blocks_round_log2", 24))
        if name == "D-descriptors":
            assert combs > bc.FW_COMBS_PER_REC * n and all(x["combs"] <= 36 for x in d)
        elif name == "D-slides":
            assert slides > n // bc.SLIDE_DIV + bc.SLIDE_ADD
        else:   # the round's buffers have room: no record changes tier for want of it
            assert combs <= bc.FW_COMBS_PER_REC * round_ and slides <= round_ // bc.SLIDE_DIV + bc.SLIDE_ADD
            assert max(x["combs"] for x in d) <= 36
        if name == "D-rounds":
            assert sum(x["tier"] != "lone" for x in d) > 2 << 10


@pytest.mark.parametrize("name", list(bc.CASES))
def test_c_oracle_equals_the_python_model_on_the_clusters(name):
    case = bc.get(name)
    sites = min(case.model_sites, 16 if name.startswith("D-") else 8, len(case.cluster))
    if name.startswith("A-"):
        sites = len(case.cluster)
    blocks = case.cluster_blocks(sites)
    lone = [b for b in case.blocks if len(b[0].variants) == 1 and b not in blocks][:20]
    blocks = blocks + lone
    args = case.args(blocks)
    triples = [(vb, n, case.refs[n]) for vb, n in blocks]
    # index: same bf bits, same exact-map keys as add_kmers_to_bf over the model's signatures
    obf, omap = bc.oracle_index(case, args, bits=1 << 22)
    mbf, mmap = ocapi.BF(1 << 22), ocapi.KMAP()
    n_sigs = 0
    for vb, _, reference in triples:
        for per in vb.extract_kmers(reference, case.haploid).values():
            for a, sigs in per.items():
                for sig in sigs:
                    n_sigs += 1
                    for km in sig:
                        (mmap if a == 0 else mbf).add_key(km.encode())
    mbf.switch_mode()
    assert np.array_equal(obf.set_positions(), mbf.set_positions())
    assert sorted(k_ for k_, _ in omap.items()) == sorted(k_ for k_, _ in mmap.items())
    assert n_sigs > 20
    # call: same coverages
    want = model_coverages(triples, obf, omap, case.haploid)
    got = ocapi.cover_blocks(obf, omap, case.reference, **args, haploid=case.haploid, k=case.k)
    assert np.array_equal(got, want) and (want > 0).sum() > 20

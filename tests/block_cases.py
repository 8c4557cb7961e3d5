"""Directed panels that put the record loop (csrc/block_pipeline.h, csrc/variant_kernels.h) exactly on, one below and one
above every fixed capacity that decides which tier a record goes to, and a pure-Python restatement of the dealing rules that
says for every record of such a panel whether tier 1 ('lone'), tier 2, tier 3 or the host gets it.  No GPU and no HIP here:
tests/test_block_cases_cpu.py checks on any machine that every case holds what its name claims and that the C oracle equals
the Python model there, tests/test_gpu_block_edges.py hands the same arrays to the device.

A case is a panel of its own: the cluster under test at SITES sites of a random ACGT genome (so the same shape meets different
sequence), then FILL lone SNPs 100 nt apart.  The fillers matter: the host forms take all records of a call as one round, so
the descriptor buffer holds 8 descriptors per record of the PANEL, and a small panel of big clusters would send its records
to tier 3 for want of room, not for the capacity under test.  Everything is built from oracle.model Variant / VB objects (the
model then says what the chains, picks and coverages are) and turned into flat arrays with block_util.pack_blocks.
Positions stay far below 2^24 (the float arithmetic of are_near is pinned by other tests)."""
import functools
import itertools

import numpy as np

from oracle.model import VB, Variant

# ---- the capacities, restated as numbers (a test's copy: nothing here is read from the code under test) -----------------------
FW_MAXC = 6             # chains per side, tier 2                      block_pipeline.h:28
FW_MAXM = 10            # members per chain side, tier 2               block_pipeline.h:29
FW_REACH = 120          # records a tier-2 walk may move away          block_pipeline.h:30
FW_SET = 512            # slots of a wave's set (3/4 used)             block_pipeline.h:31
FW_MAXU = 12            # unphased chain length, tier 2                block_pipeline.h:32
FW_MAX_SAMPLES = 512    # wider panels: every general record to tier 3 block_pipeline.h:33
FW_COMBS_PER_REC = 8    # descriptors per record of a round            block_pipeline.h:34
FW_CODE_BITS = 55       # width of a pick's code, tier 2               block_pipeline.h:566
FW_SNP_MAX_HAPS = 16    # haplotypes fw_snp_kernel takes               block_pipeline.h:761
FW_POOL = 2048          # bytes of staging area per wave               block_pipeline.h:1064
FC_SET = 512            # slots of fw_chain_kernel's set               block_pipeline.h:1183
FC_CODE_BITS = 24       # width of a pick's code in fw_chain_kernel    block_pipeline.h:1186
FC_HEAD, FC_MEMBER = 32, 16  # bytes of a staged chain's head / member block_pipeline.h:1065-1079
BK_MAXC = 16            # chains per side, tier 3                      variant_kernels.h:429
BK_MAXL = 32            # members per chain side, tier 3               variant_kernels.h:430
BK_MAXU = 14            # unphased chain length, tier 3                variant_kernels.h:431
BK_CODE_BITS = 63       # width of a pick's code in tier 3's set       variant_kernels.h:432
BK_SET_CAP = 2048       # tier 3's set; half of it is the limit        variant_kernels.h:433
LONE_MAX_ALLELES = 64   # alleles of a tier-1 record                   block_pipeline.h:159
HOST_ALLELES = 127      # more alleles: the host                       block_pipeline.h:418, variant_kernels.h:721
SLIDE_DIV, SLIDE_ADD = 4, 4096  # sliding items of a round: n/4 + 4096 malva_hip.hip:2891

SITES = 4               # copies of the cluster under test
SITE0, SITE_STEP = 4000, 4000
FILL = 2000             # lone SNPs behind the clusters
FILL0, FILL_STEP = 60_000, 100
CONTIGS = (("1", FILL0 + FILL * FILL_STEP + 2000), ("2", 30_000))


@functools.lru_cache(maxsize=None)
def genome(seed=20):
    rng = np.random.default_rng(seed)
    return {name: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n)).decode() for name, n in CONTIGS}


def lanes(n_samples):
    """G: lanes a chain gets in tier 2's picks kernels = the panel's samples rounded up to a power of two, 2..64 (malva_hip.hip:2908)"""
    g = 2
    while g < 64 and g < n_samples:
        g *= 2
    return g


def fw_bits(n_alleles):
    """bits of a member's field in a pick's code (block_pipeline.h:75)"""
    return 1 if n_alleles <= 2 else (n_alleles - 1).bit_length()


class Case:
    """name, k, haploid, n_samples, refs {contig: sequence}, blocks [(VB, contig)], cluster [[flat record index]] per site in file
    order, central [flat index] per site, want [tier] per record of a cluster (the same at every site), claim {what the name
    says, as numbers}, options [(name, value)] set on the context"""

    def __init__(self, name, k, haploid, n_samples, refs):
        self.name, self.k, self.haploid, self.n_samples, self.refs = name, k, haploid, n_samples, refs
        self.blocks, self.cluster, self.central, self.want, self.claim, self.options = [], [], [], None, {}, []
        self.hosts = 0              # records of a cluster the rules hand to the host
        self._flat = None
        self.exact_tier3 = True     # the tier-3 count is predicted (classes A, B, C, E), or only known to be positive (D)
        self.model_sites = SITES    # sites the CPU test runs through the Python model

    @property
    def names(self):
        return list(self.refs)

    @property
    def base(self):
        out, off = {}, 0
        for n in self.names:
            out[n] = off
            off += len(self.refs[n])
        return out

    @property
    def reference(self):
        return "".join(self.refs[n] for n in self.names).encode()

    def args(self, blocks=None):
        from block_util import pack_blocks
        return pack_blocks(self.blocks if blocks is None else blocks, self.base, {n: len(s) for n, s in self.refs.items()})

    def flat(self):
        """[(block number, index in block)] per flat record"""
        if self._flat is None:
            self._flat = [(b, i) for b, (vb, _) in enumerate(self.blocks) for i in range(len(vb.variants))]
        return self._flat

    def cluster_blocks(self, sites=None):
        """the blocks that hold a record of a cluster (of the first `sites` sites), in order"""
        fl = self.flat()
        want = sorted({fl[r][0] for site in self.cluster[:sites] for r in site})
        return [self.blocks[b] for b in want]


class Builder:
    """records in FILE ORDER (contig by contig; a block may step back in position: the record loop takes what it is given)"""

    def __init__(self, name, k, n_samples=8, haploid=False, seed=1, refs=None):
        self.case = Case(name, k, haploid, n_samples, dict(refs or genome()))
        self.rng = np.random.default_rng(seed)
        self.recs = []          # (contig, Variant)
        self.sites = []         # [[Variant]]
        self.mid = []           # [Variant]
        self._fill_gt = None

    def gts(self, n_alleles, phased=True):
        """random genotypes over all alleles; the LAST sample carries the highest allele"""
        n = self.case.n_samples
        top = min(n_alleles, 128)            # (a genotype word holds allele numbers below 128)
        g = [(int(a), int(b)) for a, b in self.rng.integers(0, top, size=(n, 2))]
        g[-1] = (top - 1, g[-1][1])
        return g, [bool(phased)] * n

    def rec(self, contig, pos, ref_len=1, alts=None, gts=None, phasing=None, present=True, n_alts=1):
        ref = self.case.refs[contig]
        v = Variant(seq_name=contig, ref_pos=pos, ref_sub=ref[pos:pos + ref_len], ref_size=ref_len)
        if alts is None:
            alts = self.alts(v.ref_sub, n_alts)
        v.alts = list(alts)
        v.set_sizes()
        v.coverages = [0] * (len(v.alts) + 1)
        v.is_present = bool(present)
        if gts is None:
            gts, ph = self.gts(len(v.alts) + 1)
            phasing = ph if phasing is None else phasing
        v.genotypes, v.phasing = list(gts), list(phasing if phasing is not None else [True] * len(gts))
        assert len(v.genotypes) == len(v.phasing) == self.case.n_samples
        self.recs.append((contig, v))
        return v

    def alts(self, ref_sub, n):
        """n distinct ALT texts: one base for a record of one ALT (a SNP, or a deletion down to its first base's SNP-free
        form); for more, the three other bases first and then insertions of two to five bases"""
        if len(ref_sub) > 1 and n == 1:
            return [ref_sub[0]]                                        # a deletion, VCF style
        out = [b for b in "ACGT" if b != ref_sub[:1]][:n] if len(ref_sub) == 1 else [ref_sub[0]]
        for ln in range(2, 7):
            for t in itertools.product("ACGT", repeat=ln):
                if len(out) >= n:
                    return out
                a = "".join(t)
                if a != ref_sub:
                    out.append(a)
        raise ValueError("too many ALTs")

    def site(self, central, records):
        self.mid.append(central)
        self.sites.append(list(records))

    def fill(self, n=FILL):
        """n lone SNPs FILL_STEP apart behind the clusters: they share one genotype list (a panel of 513 samples has 1e6 of them)"""
        ns = self.case.n_samples
        g = [(s % 2, (s // 2) % 2) for s in range(ns)]
        g[-1] = (1, 1)
        ph = [True] * ns
        for i in range(n):
            self.rec("1", FILL0 + i * FILL_STEP, gts=g, phasing=ph)

    def finish(self, want=None, hosts=None, **claim):
        c = self.case
        order = {n: i for i, n in enumerate(c.names)}
        seen = [order[n] for n, _ in self.recs]
        assert seen == sorted(seen), "records contig by contig"
        vb, last = None, None
        for n, v in self.recs:
            if vb is None or n != last or not vb.is_near_to_last(v):
                vb = VB(c.k, 0.001)
                c.blocks.append((vb, n))
                last = n
            vb.add_variant(v)
        at = {id(v): r for r, v in enumerate(v for vb, _ in c.blocks for v in vb.variants)}
        c.cluster = [[at[id(v)] for v in site] for site in self.sites]
        c.central = [at[id(v)] for v in self.mid]
        c.want, c.claim = want, claim
        c.hosts = (1 if want == "host" else 0) if hosts is None else hosts
        return c


# ---- the dealing rules, restated ---------------------------------------------------------------------------------------------
def walk(vb, i, step):
    """get_combs_on_the_right (step +1) / _left (step -1) as both walks on the device run them (fw_walk, block_pipeline.h:335;
    bk_chains, variant_kernels.h:532) -> (chains as lists of record indices, the largest record distance the walk LOOKED at:
    absent records and records overlapping the central one are skipped but looked at; whether a record it looked at lies
    BEFORE its neighbour in the file that is nearer to the central record: the block steps back there)"""
    V = vb.variants
    mid = V[i]
    pair = (lambda x, y: (x, y)) if step > 0 else (lambda x, y: (y, x))
    ov = lambda a, b: VB.are_overlapping(*pair(a, b))
    chains, sums, far, halt, back = [], [], 0, False, False
    j = i + step
    while 0 <= j < len(V) and not halt:
        cur, far = V[j], abs(j - i)
        back = back or (cur.ref_pos < V[j - 1].ref_pos if step > 0 else cur.ref_pos > V[j + 1].ref_pos)
        jn, j = j, j + step
        if not cur.is_present or ov(mid, cur):
            continue
        gain = cur.ref_size - cur.min_size
        if not chains:
            if vb.are_near(*pair(mid, cur)):
                chains.append([jn])
                sums.append(gain)
            continue
        added = False
        for c in range(len(chains)):
            if not ov(V[chains[c][-1]], cur):
                added = True
                if vb.are_near(*pair(mid, cur), sums[c]):
                    chains[c].append(jn)
                    sums[c] += gain
        if not added:
            for c in range(len(chains)):
                nc, ns = list(chains[c]), sums[c]
                while nc and ov(V[nc[-1]], cur):
                    m = V[nc.pop()]
                    ns -= m.ref_size - m.min_size
                if vb.are_near(*pair(mid, cur), ns):
                    added = True
                    chains.append(nc + [jn])
                    sums.append(ns + gain)
            halt = not added
    return chains, far, back


def coded(vb):
    """the block with every allele's text replaced by its NUMBER: VB.allele_combs over it gives the distinct picks as the
    device counts them (codes of allele numbers, two ALTs of one text being two codes), not the distinct texts"""
    out = VB(vb.k, 0.001)
    for v in vb.variants:
        out.add_variant(Variant(ref_pos=v.ref_pos, ref_sub="0", alts=[str(a + 1) for a in range(len(v.alts))], ref_size=v.ref_size,
                                genotypes=v.genotypes, phasing=v.phasing, is_present=v.is_present))
    return out


def n_picks(cvb, comb, central, haploid):
    """distinct picks along a chain; the 2^m mixes of an unphased sample are only enumerated where they can matter"""
    return len(cvb.allele_combs(comb, central, haploid))


def unphased_along(vb, comb, haploid):
    """some sample is unphased at some member of a chain of two or more, diploid: its 2^m mixes are taken"""
    if haploid or len(comb) < 2:
        return False
    V = vb.variants
    return any(not all(V[j].phasing[s] for j in comb) for s in range(len(V[comb[0]].genotypes)))


def staging_bytes(vb, comb):
    """what fw_chain_kernel stages of a chain: head, a block per member, the offsets of all its alleles and one more per member"""
    return FC_HEAD + FC_MEMBER * len(comb) + 4 * sum(len(vb.variants[j].alts) + 2 for j in comb)


def code_bits(vb, comb):
    return sum(fw_bits(len(vb.variants[j].alts) + 1) for j in comb)


def carried(v, haploid):
    """raw allele numbers some panel haplotype carries"""
    return {a for g in v.genotypes for a in (g[:1] if haploid else g)}


def deal(case, index=False):
    """-> [dict(tier='lone'|'tier2'|'tier3'|'host', took3=tier 3 had the record in its list, combs=descriptors it takes in tier 2,
              listed=chains of it fw_chain_kernel hands to the list path, slides=sliding picks)] per record, in flat order"""
    k, hap, ns = case.k, case.haploid, case.n_samples
    G = lanes(ns)
    per_wave = 64 // G
    out = []
    for vb, name in case.blocks:
        V, clen, cvb = vb.variants, len(case.refs[name]), None
        ref = case.refs[name]
        for i, v in enumerate(V):
            lens = [v.ref_size] + [len(a) for a in v.alts]
            A, p = len(lens), v.ref_pos
            d = dict(tier="tier2", took3=False, combs=0, listed=0, slides=0)
            out.append(d)
            eligible = v.is_present and k <= p <= clen - k                                   # var_block.hpp:104
            lone = len(V) == 1 and A <= LONE_MAX_ALLELES and all(l < k for l in lens) and p >= k // 2 and p + v.ref_size + (k + 1) // 2 <= clen
            if lone:
                d["tier"] = "lone"
                if index and eligible:   # index time: a base outside ACGT in the window of a carried allele -> the host enumerates the record
                    for a in carried(v, hap):
                        al = len(v.get_allele(a))
                        mp, ms = k // 2 - al // 2, (k + 1) // 2 - (al - al // 2)
                        if set(ref[p - mp:p] + v.get_allele(a) + ref[p + v.ref_size:p + v.ref_size + ms]) - set("ACGT"):
                            d["tier"] = "host"
                continue
            if A > HOST_ALLELES:
                d["tier"] = "host"
                continue
            t3 = ns > FW_MAX_SAMPLES
            L = R = None
            if eligible:
                (L, far_l, back_l), (R, far_r, back_r) = walk(vb, i, -1), walk(vb, i, +1)
                combs = vb.combine(L, R, i)
                assert p - 200 >= 0 and p + 200 <= clen, "a general record's windows stay inside the sequence"
            if eligible and not t3:
                cvb = cvb or coded(vb)
                t3 = max(len(L), len(R)) > FW_MAXC or max((len(c) for c in L + R), default=0) > FW_MAXM or max(far_l, far_r) > FW_REACH
                t3 = t3 or back_l or back_r          # a walk that meets a step back in position gives the record up (block_pipeline.h:350)
                if not t3:
                    d["combs"] = len(combs)
                for comb in ([] if t3 else combs):
                    bits, m, unph = code_bits(vb, comb), len(comb), unphased_along(vb, comb, hap)
                    if bits > FW_CODE_BITS or (unph and m > FW_MAXU):
                        t3 = True
                        continue
                    bound = ns if hap else 2 * ns if not unph else None
                    share_alone = FW_SET * 3 // 4
                    share_here = FC_SET * 3 // 4 // per_wave
                    picks = bound if bound is not None and bound <= share_here else n_picks(cvb, comb, i, hap)
                    if picks > share_alone:
                        t3 = True
                    wide = any(fw_bits(len(V[j].alts) + 1) > 7 for j in comb)
                    if wide or bits > FC_CODE_BITS or staging_bytes(vb, comb) > FW_POOL // per_wave or picks > share_here:
                        d["listed"] += 1
                    if m == 1:
                        d["slides"] = sum(1 for a in carried(v, hap) if lens[a] >= k)
            if not t3:
                continue
            d["took3"], d["tier"] = True, "tier3"
            if not eligible:
                continue
            if any(b.ref_pos < a.ref_pos for a, b in zip(V, V[1:])):      # tier 3 leaves a block that steps back to the host (variant_kernels.h:741)
                d["tier"] = "host"
            elif max(len(L), len(R)) > BK_MAXC or max((len(c) for c in L + R), default=0) > BK_MAXL:
                d["tier"] = "host"
            elif any(len(comb) > BK_MAXU and unphased_along(vb, comb, hap) for comb in combs):
                d["tier"] = "host"
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------
CASES = {}


def case(name):
    def reg(fn):
        CASES[name] = fn
        return fn
    return reg


@functools.lru_cache(maxsize=None)
def get(name):
    c = CASES[name](name)
    assert c.name == name
    return c


def site_pos(s):
    return SITE0 + s * SITE_STEP


# class A: tier 1's classification ----------------------------------------------------------------------------------------------
def _edge_positions(k, clen):
    """(two sets of positions at a sequence's start whose records are not near one another, the four positions at its end)"""
    p_max = clen - 1 - (k + 1) // 2          # the largest p with p + rs + (k + 1) / 2 <= clen, rs = 1
    return ([k // 2 - 1, k - 1], [k // 2, k]), [clen - k, clen - k + 1, p_max, p_max + 1]


def _tier1_of(k, clen, p):
    """a lone-by-spacing SNP at p: tier 1 takes it iff both flanks lie inside the sequence; else it is listed and, not being
    eligible (var_block.hpp:104), nothing is done for it in tier 2"""
    return "lone" if p >= k // 2 and p + 1 + (k + 1) // 2 <= clen else "tier2"


def _positions_case(name, k, variant):
    b = Builder(name, k, seed=100 + variant)
    want = []
    for ci, contig in enumerate(b.case.names):
        clen = len(b.case.refs[contig])
        starts, ends = _edge_positions(k, clen)
        if contig == "1":
            ps = starts[variant % 2] + [ends[variant]]
        else:
            ps = starts[(variant + 1) % 2] + [ends[(variant + 2) % 4]]
        recs = []
        for p in ps[:2]:
            recs.append(b.rec(contig, p))
        if contig == "1":
            b.fill()
        recs.append(b.rec(contig, ps[2]))
        for v in recs:
            b.site(v, [v])
            want.append(_tier1_of(k, clen, v.ref_pos))
    c = b.finish(want=None, k=k)
    c.want_per_site = want
    return c


for _k in (35, 32):
    for _v in range(4):
        CASES["A-positions-k%d-%d" % (_k, _v)] = functools.partial(_positions_case, k=_k, variant=_v)


def _kinds_case(name, haploid=False, k=35):
    """one record of every kind tier 1 tells apart, each alone (300 nt apart), on both sequences"""
    refs = dict(genome())
    spots = {}
    for contig in refs:                       # bases outside ACGT: at the first and the last base of a SNP's window, and just outside it
        g = list(refs[contig])
        for i, off in enumerate((-(k // 2), (k + 1) // 2 - 1, -(k // 2) - 1, (k + 1) // 2)):
            p = 20_000 + 300 * i
            g[p + off] = "N"
            spots.setdefault(contig, []).append(p)
        refs[contig] = "".join(g)
    b = Builder(name, k, seed=7, haploid=haploid, refs=refs)
    ns = b.case.n_samples
    want, index_want = [], []
    for contig in b.case.names:
        ref = refs[contig]
        p = 2000

        def put(tier, index_tier=None, **kw):
            nonlocal p
            v = b.rec(contig, p, **kw)
            b.site(v, [v])
            want.append(tier)
            index_want.append(index_tier or tier)
            p += 300
            return v
        for ln in (k - 2, k - 1, k, k + 1):                  # REF of ln bases; ALT of ln bases: k and more is a sliding signature
            put("lone" if ln < k else "tier2", ref_len=ln)
            put("lone" if ln < k else "tier2", alts=[("C" if ref[p] != "C" else "G") + ref[p + 1:p + ln]])
        for A in (2, 4, 5, 64, 65, 127, 128):                # the last sample names the highest allele
            put("lone" if A <= 64 else "tier2" if A <= 127 else "host", n_alts=A - 1)
        other = "C" if ref[p] != "C" else "G"
        put("lone", alts=[other, other], gts=[(2, 0)] * ns, phasing=[True] * ns)       # two ALTs of one text: canon 1, 1
        put("lone", alts=[other, ref[p]], gts=[(2, 1)] * ns, phasing=[True] * ns)      # an ALT spelled like REF: canon 0
        put("lone", present=False)
        put("lone", gts=[(0, 1)] * ns, phasing=[False] + [True] * (ns - 1))            # an unphased sample
        put("lone", gts=[(1, 1)] * ns, phasing=[True] * ns)                            # sparse: every sample has an entry
        put("lone", gts=[(0, 0)] * ns, phasing=[True] * ns)                            # sparse: no sample has one
        for i, sp in enumerate(spots[contig]):               # index time: a base outside ACGT in the window -> the host
            p = sp
            put("lone", "host" if i < 2 else "lone", gts=[(0, 1)] * ns, phasing=[True] * ns)
        if contig == "1":
            b.fill()
    c = b.finish(want=None, k=k)
    c.want_per_site, c.index_want_per_site = want, index_want
    return c


CASES["A-kinds"] = _kinds_case
CASES["A-kinds-haploid"] = functools.partial(_kinds_case, haploid=True)


# class B: the walks' capacities ----------------------------------------------------------------------------------------------
# (offset from the central SNP, REF length) of SNPs and short deletions that give the central record exactly so many chains on
# one side, k = 35 (found by a random search over such records within 20 nt; the CPU test counts them with the model)
RIGHT = {5: [(13, 4), (14, 5), (15, 1), (17, 5), (18, 3)],
         6: [(13, 4), (14, 3), (15, 4), (17, 4), (18, 5)],
         7: [(12, 4), (14, 5), (15, 2), (18, 3), (18, 4)],
         15: [(11, 4), (11, 5), (12, 2), (15, 1), (15, 4), (17, 2), (18, 3)],
         16: [(7, 4), (10, 2), (10, 2), (10, 4), (10, 5)],
         17: [(9, 1), (11, 4), (13, 1), (16, 5), (19, 5), (20, 1), (20, 2), (20, 3)]}
LEFT = {5: [(10, 4), (12, 2), (17, 3), (19, 3), (19, 5)],
        6: [(13, 5), (13, 5), (17, 4), (18, 5), (19, 3)],
        7: [(10, 1), (10, 5), (10, 5), (17, 5), (19, 5)],
        15: [(8, 5), (9, 1), (9, 3), (15, 2), (15, 4), (17, 2), (18, 3)],
        16: [(10, 5), (11, 4), (11, 4), (13, 5), (13, 5)],
        17: [(5, 5), (9, 1), (9, 3), (9, 3), (17, 5), (19, 4), (20, 3)]}


def _tier_by_count(n, lo, hi):
    return "tier2" if n <= lo else "tier3" if n <= hi else "host"


def _chains_case(name, n_left, n_right):
    b = Builder(name, 35, seed=n_left * 100 + n_right)
    for s in range(SITES):
        c = site_pos(s)
        spec = [(c, 1, True)]
        spec += [(c + d, rs, False) for d, rs in RIGHT.get(n_right, [])]
        spec += [(c - d - rs + 1, rs, False) for d, rs in LEFT.get(n_left, [])]     # (a record reaching back to offset -d)
        spec.sort(key=lambda r: r[0])
        recs = [(b.rec("1", p, ref_len=rs), mid) for p, rs, mid in spec]
        b.site(next(v for v, mid in recs if mid), [v for v, _ in recs])
    b.fill()
    # (RIGHT[17] gives its first record 17 chains as well: two records a site go to the host there)
    return b.finish(want=_tier_by_count(max(n_left, n_right), FW_MAXC, BK_MAXC), hosts=2 if (n_left, n_right) == (0, 17) else None,
                    chains_left=n_left, chains_right=n_right)


for _n in (5, 6, 7, 15, 16, 17):
    CASES["B-chains-right-%d" % _n] = functools.partial(_chains_case, n_left=0, n_right=_n)
    CASES["B-chains-left-%d" % _n] = functools.partial(_chains_case, n_left=_n, n_right=0)
for _l, _r in ((6, 6), (7, 6), (6, 7), (16, 16), (17, 16)):
    CASES["B-chains-both-%d-%d" % (_l, _r)] = functools.partial(_chains_case, n_left=_l, n_right=_r)


def _members_case(name, n_left, n_right):
    """SNPs at consecutive positions beside the central one: a single chain per side.  A record joins while it lies within
    (k + 1) / 2 - 1 bases of the central one plus the chain's gain, and a record that adds g bases of gain takes g + 1 bases
    of room: in a sorted block a side holds at most (k + 1) / 2 - 1 members, 31 at k = 64 (the largest k of the packed
    paths), and BK_MAXL = 32 cannot be met.  The 32nd and 33rd are records that STEP BACK in the file -- a block is whatever
    the cut hands over, and the walks compare a record only with each chain's last member.  The reference takes the rest of
    the sequence for the negative gap between two such members (get_ref_subs, var_block.hpp:682-702); the device hands every
    eligible record of such a block to the host, which is what these cases pin."""
    k = 35 if max(n_left, n_right) <= 11 else 64
    room = (k + 1) // 2 - 1
    b = Builder(name, k, seed=n_left * 100 + n_right)
    for s in range(SITES):
        c = site_pos(s)
        offs = [-2 - i for i in range(max(0, n_left - room))]                   # stepped back: in the file BEFORE the sorted run
        offs += list(range(-min(n_left, room), min(n_right, room) + 1))
        offs += [room - 1 - i for i in range(max(0, n_right - room))]           # stepped back: behind the sorted run
        recs = [b.rec("1", c + d) for d in offs]
        b.site(recs[offs.index(0)], recs)
    b.fill()
    stepped = max(n_left, n_right) > room
    want = "host" if stepped else _tier_by_count(max(n_left, n_right), FW_MAXM, BK_MAXL)
    return b.finish(want=want, hosts=len(offs) if stepped else None, members_left=n_left, members_right=n_right, k=k)


for _n in (9, 10, 11, 31, 32, 33):
    CASES["B-members-right-%d" % _n] = functools.partial(_members_case, n_left=0, n_right=_n)
    CASES["B-members-left-%d" % _n] = functools.partial(_members_case, n_left=_n, n_right=0)
for _l, _r in ((9, 9), (10, 10), (11, 10), (31, 31), (32, 32), (32, 33)):
    CASES["B-members-both-%d-%d" % (_l, _r)] = functools.partial(_members_case, n_left=_l, n_right=_r)


def _reach_case(name, d_left, d_right):
    """the central record's only near record on a side is the d-th record away: between them lie records that overlap the central
    one (the walk skips them) and absent records (skipped too) -- looked at, and counted by FW_REACH, all the same"""
    k = 35
    b = Builder(name, k, seed=d_left * 1000 + d_right)
    ns = b.case.n_samples
    for s in range(SITES):
        c = site_pos(s)
        recs = []
        if d_left:      # the near SNP, absent records, two deletions that reach over the central position
            recs.append(b.rec("1", c - 10))
            recs += [b.rec("1", c - 8 + i * 3 // (d_left - 3), present=False) for i in range(d_left - 3)]
            recs += [b.rec("1", c - 5 + i, ref_len=8) for i in range(2)]
            mid = b.rec("1", c, ref_len=40 if d_right else 1)
        else:
            mid = b.rec("1", c, ref_len=40 if d_right else 1)
        recs.append(mid)
        if d_right:     # (the central record is then a deletion of 39 bases) SNPs inside it, absent records, the near SNP
            recs += [b.rec("1", c + 2 + 2 * i) for i in range(19)]
            recs += [b.rec("1", c + 40 + i * 3 // (d_right - 20), present=False) for i in range(d_right - 20)]
            recs.append(b.rec("1", c + 45))
        b.site(mid, recs)
    b.fill()
    return b.finish(want="tier2" if max(d_left, d_right) <= FW_REACH else "tier3", reach_left=d_left, reach_right=d_right)


for _d in (119, 120, 121):
    CASES["B-reach-right-%d" % _d] = functools.partial(_reach_case, d_left=0, d_right=_d)
    CASES["B-reach-left-%d" % _d] = functools.partial(_reach_case, d_left=_d, d_right=0)
for _l, _r in ((120, 120), (121, 120), (120, 121)):
    CASES["B-reach-both-%d-%d" % (_l, _r)] = functools.partial(_reach_case, d_left=_l, d_right=_r)


# class C: the picks' capacities -----------------------------------------------------------------------------------------------
def _run_of(b, c, n, n_alts=1, mid=None, gts=None):
    """n records at consecutive positions around c (every one near every other: each record's chain is the whole run);
    n_alts: one number or one per record; gts(j) -> (genotypes, phasing) of record j or None for random phased ones"""
    mid = (n - 1) // 2 if mid is None else mid
    recs = []
    for j in range(n):
        g = gts(j) if gts else None
        recs.append(b.rec("1", c - mid + j, n_alts=n_alts[j] if isinstance(n_alts, (list, tuple)) else n_alts,
                          gts=g[0] if g else None, phasing=g[1] if g else None))
    b.site(recs[mid], recs)
    return recs


def _unphased_case(name, m):
    """a run of m SNPs; sample 0 is unphased and heterozygous at two members only: 4 distinct mixes, 2^m to walk"""
    b = Builder(name, 35, seed=m)
    ns = b.case.n_samples

    def gts(j):
        g, ph = b.gts(2)
        g[0] = (0, 1) if j in (m // 2, m // 2 + 1) else (0, 0)
        return g, [False] + ph[1:]
    for s in range(SITES):
        _run_of(b, site_pos(s), m, gts=gts)
    b.fill()
    c = b.finish(want=_tier_by_count(m, FW_MAXU, BK_MAXU), hosts=m if m > BK_MAXU else 0, unphased_members=m)
    c.model_sites = 1 if m >= 14 else SITES          # (2^15 mixes per record of the run through the Python model: once)
    return c


for _m in (12, 13, 14, 15):
    CASES["C-unphased-%d" % _m] = functools.partial(_unphased_case, m=_m)


def _bits_case(name, alleles, n_samples, want, **claim):
    b = Builder(name, 35, n_samples=n_samples, seed=sum(alleles))
    for s in range(SITES):
        _run_of(b, site_pos(s), len(alleles), n_alts=[a - 1 for a in alleles])
    b.fill()
    return b.finish(want=want, **claim)


CASES["C-bits-55"] = functools.partial(_bits_case, alleles=[65, 100, 127, 65, 5, 100, 127, 65, 8], n_samples=8, want="tier2", code_bits=55)
CASES["C-bits-56"] = functools.partial(_bits_case, alleles=[65, 100, 127, 65, 5, 100, 127, 65, 9], n_samples=8, want="tier3", code_bits=56)
CASES["C-bits-24"] = functools.partial(_bits_case, alleles=[16] * 6, n_samples=40, want="tier2", code_bits=24, listed=False)
CASES["C-bits-25"] = functools.partial(_bits_case, alleles=[16] * 5 + [17], n_samples=40, want="tier2", code_bits=25, listed=True)
CASES["C-bits-63"] = functools.partial(_bits_case, alleles=[100] * 9, n_samples=8, want="tier3", code_bits=63)
CASES["C-bits-64"] = functools.partial(_bits_case, alleles=[100] * 8 + [16, 16], n_samples=8, want="tier3", code_bits=64)
CASES["C-staging-256"] = functools.partial(_bits_case, alleles=[9, 9, 9, 9], n_samples=8, want="tier2", staging=256, listed=False)
CASES["C-staging-260"] = functools.partial(_bits_case, alleles=[9, 9, 9, 10], n_samples=8, want="tier2", staging=260, listed=True)


def _picks_case(name, n_samples, m, het0, het1, extra, want, far=None, **claim):
    """a run of m SNPs of three alleles.  Sample 0 is unphased and 0/1 at the first het0 members: 2^het0 picks.  Sample 1 is
    unphased, 0/2 at the first het1 members and 2/2 at the next: 2^het1 picks, none of them one of sample 0's.  `extra`: sample 2
    is 1|1 at the last member -- one pick more.  Every other genotype is 0|0: the all-REF pick, one of sample 0's.
    `far`: the records have FOUR alleles and the one pick more is sample `far`'s instead, 3|3 at every member: the only haplotype
    that carries allele 3 anywhere.  With far >= 64 a lane meets that sample on its SECOND turn (G = 64 lanes stride over the
    samples), after samples 0 and 1 have filled the chain's share: a kernel that stops at `count >= share` where `count > share`
    is meant never looks at it, keeps the chain, and leaves allele 3 of every record without coverage."""
    b = Builder(name, 35, n_samples=n_samples, seed=m)

    def gts(j):
        g = [(0, 0)] * n_samples
        ph = [True] * n_samples
        ph[0] = False
        if j < het0:
            g[0] = (0, 1)
        if het1:
            ph[1] = False
            g[1] = (0, 2) if j < het1 else (2, 2) if j == het1 else (0, 0)
        if extra and far is not None:
            g[far] = (3, 3)
        elif extra and j == m - 1:
            g[2] = (1, 1)
        return g, ph
    for s in range(SITES):
        _run_of(b, site_pos(s), m, n_alts=2 if far is None else 3, gts=gts)
    b.fill()
    if far is not None:
        claim["far"] = far
    return b.finish(want=want, picks=(1 << het0) + ((1 << het1) if het1 else 0) + int(extra), **claim)


CASES["C-share-8-48"] = functools.partial(_picks_case, n_samples=8, m=6, het0=5, het1=4, extra=False, want="tier2", listed=False)
CASES["C-share-8-49"] = functools.partial(_picks_case, n_samples=8, m=6, het0=5, het1=4, extra=True, want="tier2", listed=True)
CASES["C-share-40-384"] = functools.partial(_picks_case, n_samples=40, m=9, het0=8, het1=7, extra=False, want="tier2", listed=False)
CASES["C-share-40-385"] = functools.partial(_picks_case, n_samples=40, m=9, het0=8, het1=7, extra=True, want="tier3", listed=True)
CASES["C-share-130-384"] = functools.partial(_picks_case, n_samples=130, m=9, het0=8, het1=7, extra=False, far=100, want="tier2", listed=False)
CASES["C-share-130-385"] = functools.partial(_picks_case, n_samples=130, m=9, het0=8, het1=7, extra=True, far=100, want="tier3", listed=True)
CASES["C-set-1024"] = functools.partial(_picks_case, n_samples=8, m=11, het0=10, het1=0, extra=False, want="tier3")
CASES["C-set-1025"] = functools.partial(_picks_case, n_samples=8, m=11, het0=10, het1=0, extra=True, want="tier3")


def _wide_case(name, A):
    """a SNP of two alleles whose only neighbour has A >= 128 alleles: the neighbour goes to the host, the SNP's chain holds it"""
    b = Builder(name, 35, seed=A)
    for s in range(SITES):
        c = site_pos(s)
        mid = b.rec("1", c)
        b.site(mid, [mid, b.rec("1", c + 3, n_alts=A - 1)])
    b.fill()
    return b.finish(want="tier2", hosts=1, wide_alleles=A)


for _a in (128, 129, 130):
    CASES["C-wide-%d" % _a] = functools.partial(_wide_case, A=_a)


# class D: a round's buffers and seams -----------------------------------------------------------------------------------------
def _descriptors_case(name):
    """no fillers; blocks of 20 positions 8 nt apart with two SNPs each.  The two records of a position overlap, so a walk forks
    there: two positions are in reach on each side, 4 chains a side, 16 descriptors per record against the 8 a round has room for.
    (Not the 36 chain pairs per record one could ask for: in a cluster that gives ONE record 6 x 6 pairs its neighbours have fewer,
    4.9 a record on average in B-chains-both-6-6, which fits the buffer.  16 for every record overflows it twice over, which is
    what the case is for; a single record's 36 are B-chains-both-6-6's.)"""
    b = Builder(name, 35, seed=3)
    for blk in range(60):
        c = 3000 + blk * 400
        recs = [b.rec("1", c + 8 * (j // 2), alts=["ACGT".replace(b.case.refs["1"][c + 8 * (j // 2)], "")[j % 2]]) for j in range(40)]
        b.site(recs[20], recs)
    c = b.finish(want="tier2")
    c.exact_tier3, c.model_sites = False, 16
    return c


def _slides_case(name):
    """no fillers; 3,000 lone records with two ALTs of k and k + 1 bases that every sample carries: 6,000 sliding picks against
    the n / 4 + 4096 = 4,846 a round has room for"""
    k = 35
    b = Builder(name, k, seed=4)
    ns = b.case.n_samples
    ref = b.case.refs["1"]
    for i in range(3000):
        p = 3000 + 80 * i
        v = b.rec("1", p, alts=[ref[p + 100:p + 100 + k], ref[p + 200:p + 201 + k]], gts=[(1, 2)] * ns, phasing=[True] * ns)
        b.site(v, [v])
    c = b.finish(want="tier2")
    c.exact_tier3, c.model_sites = False, 16
    return c


def _rounds_case(name):
    """3,000 general records (pairs of SNPs) and rounds of 2^10: two seams inside the general list"""
    b = Builder(name, 35, seed=5)
    for i in range(1500):
        p = 3000 + 150 * i
        v = b.rec("1", p)
        b.site(v, [v, b.rec("1", p + 7)])
    c = b.finish(want="tier2")
    c.options, c.model_sites = [("blocks_round_log2", 10)], 16
    return c


CASES["D-descriptors"] = _descriptors_case
CASES["D-slides"] = _slides_case
CASES["D-rounds"] = _rounds_case


# class E: the panel's width ---------------------------------------------------------------------------------------------------
def _width_case(name, n_samples, haploid=False):
    """one small mixed panel at every width at which the lane groups, fw_snp_kernel's 16 haplotypes or the 512-sample limit change"""
    k = 35
    b = Builder(name, k, n_samples=n_samples, haploid=haploid, seed=11)
    ref = b.case.refs["1"]
    for s in range(SITES):
        c = site_pos(s)
        for base, offs in ((0, (0, 6)), (200, (0, 5, 11)), (400, (0, 3, 9, 15))):      # chains of two, three and four SNPs
            recs = [b.rec("1", c + base + d) for d in offs]
            b.site(recs[0], recs)
        g, _ = b.gts(2)
        ph = [bool(x) for x in b.rng.integers(0, 2, size=n_samples)]                  # a chain with an indel, unphased samples
        recs = [b.rec("1", c + 600, ref_len=4), b.rec("1", c + 606, alts=[ref[c + 606] + "ACGTA"], gts=g, phasing=ph), b.rec("1", c + 612, n_alts=2)]
        b.site(recs[1], recs)
        v = b.rec("1", c + 800, alts=[ref[c + 900:c + 900 + k + 3]])                   # an allele of k bases and more, alone
        b.site(v, [v])
    b.fill()
    return b.finish(want="tier3" if n_samples > FW_MAX_SAMPLES else "tier2", n_samples=n_samples)


for _n in (1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 512, 513):
    CASES["E-width-%d" % _n] = functools.partial(_width_case, n_samples=_n)
for _n in (16, 17):
    CASES["E-width-haploid-%d" % _n] = functools.partial(_width_case, n_samples=_n, haploid=True)


# ---- an index for a case, from the oracle -------------------------------------------------------------------------------------
def oracle_index(case, args, bits=1 << 24):
    """the oracle's index of the panel (mo_index_blocks) with a counter of its own for every key, derived from the key (from its
    place in the filter for `bf`, whose keys are not kept): 1 + hash % 65521, so that a k-mer assembled one base off -- another
    key -- almost never finds an equal weight.  Keys with a letter outside ACGT keep 0, as a scan would leave them."""
    from oracle import capi as ocapi
    obf, omap = ocapi.BF(bits), ocapi.KMAP()
    ocapi.index_blocks(obf, omap, case.reference, **args, haploid=case.haploid, k=case.k)
    obf.switch_mode()
    cnts = obf.counts()
    cnts[:] = (1 + (obf.set_positions() * np.uint64(2654435761)) % np.uint64(65521)).astype(np.uint16)
    acgt = set(b"ACGT")
    for key, _ in list(omap.items()):
        if set(key) <= acgt:
            omap.increment(key, 1 + ocapi.xxh3_64(key) % 65521)
    return obf, omap

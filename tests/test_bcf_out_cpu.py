"""`--merged-format`: what of the BCF output can be checked without a GPU -- the exported symbols, the command line's refusals and
help text, and the yardstick itself: the BCF decoder of the tests (BCF -> VCF text, written here from the VCF/BCF specification
v4.3, section 6) reads back what tests/bcf_writer.py writes, before tests/test_gpu_bcf.py uses it on the product."""
import os
import struct
import subprocess
import zlib

import pytest

import bcf_writer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
WIDTH = {1: 1, 2: 2, 3: 4, 5: 4, 7: 1}
UNPACK = {1: "<b", 2: "<h", 3: "<i"}
MISSING = {1: -128, 2: -32768, 3: -(1 << 31)}
EOV = {1: -127, 2: -32767, 3: -(1 << 31) + 1}


# ---- the decoder of the tests ---------------------------------------------------------------------------------------------------

def bgzf_members(data):
    """-> [(member bytes, inflated bytes)]; every member carries the BC field with a true BSIZE, CRC32 and ISIZE"""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 10:at + 16] == b"\x06\x00BC\x02\x00", "not a BGZF member at %d" % at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        assert at + size <= len(data), "BSIZE runs past the file"
        member = data[at:at + size]
        d = zlib.decompressobj(-15)
        raw = d.decompress(member[18:-8]) + d.flush()
        assert d.eof and d.unused_data == b"", "BSIZE is not the member's size"
        crc, isize = struct.unpack("<II", member[-8:])
        assert crc == zlib.crc32(raw) and isize == len(raw)
        out.append((member, raw))
        at += size
    return out


def bcf_bytes(path):
    """the BCF stream of a file, BGZF-compressed or not"""
    data = open(path, "rb").read()
    return b"".join(raw for _, raw in bgzf_members(data)) if data[:2] == b"\x1f\x8b" else data


class _Cur:
    def __init__(self, b, at=0, end=None):
        self.b, self.at, self.end = b, at, len(b) if end is None else end

    def take(self, n):
        assert self.at + n <= self.end, "a record overruns its length"
        self.at += n
        return self.b[self.at - n:self.at]

    def int_of(self, t):
        return struct.unpack(UNPACK[t], self.take(WIDTH[t]))[0]

    def desc(self):
        d = self.take(1)[0]
        t, n = d & 15, d >> 4
        if n == 15:
            t2, one = self.desc()
            assert one == 1
            n = self.int_of(t2)
        return t, n

    def typed_int(self):
        t, n = self.desc()
        assert n == 1
        return self.int_of(t)

    def typed_str(self):
        t, n = self.desc()
        assert t == 7 or n == 0
        return self.take(n).decode()


def _float_text(key, bits):
    if bits == 0x7F800001:
        return "."
    return "%g" % struct.unpack("<f", struct.pack("<I", bits))[0]


def _vector(cur, t, n, key, float_text):
    if t == 7:
        s = cur.take(n).rstrip(b"\0").decode()
        return s or "."
    vals = []
    for _ in range(n):
        if t == 5:
            bits = struct.unpack("<I", cur.take(4))[0]
            if bits != 0x7F800002:
                vals.append(float_text(key, bits))
        else:
            v = cur.int_of(t)
            if v != EOV[t]:
                vals.append("." if v == MISSING[t] else str(v))
    return ",".join(vals) or "."


def _attr(line, key):
    return bcf_writer._attr(line, key) if "<" in line and ">" in line else None


def bcf_to_vcf(data, float_text=_float_text):
    """the VCF text a BCF stream encodes -> lines (header lines first).  float_text(key, bits): how a float prints (QUAL: key None)"""
    assert data[:5] == b"BCF\x02\x02"
    l_text = struct.unpack_from("<I", data, 5)[0]
    text = data[9:9 + l_text]
    assert text.endswith(b"\0") and b"\0" not in text[:-1]
    lines = text[:-1].decode().split("\n")
    assert lines[-1] == "" and lines[-2].startswith("#CHROM")
    lines = lines[:-1]
    dic, contigs = {0: "PASS"}, {}
    for l in lines:                                                               # section 6.2.1
        if l.startswith(("##INFO=", "##FORMAT=", "##FILTER=")):
            i, idx = _attr(l, "ID"), _attr(l, "IDX")
            if idx is None and (i == "PASS" or i in dic.values()):
                continue
            dic[int(idx) if idx is not None else max(dic) + 1] = i
        elif l.startswith("##contig="):
            idx = _attr(l, "IDX")
            contigs[int(idx) if idx is not None else (max(contigs) + 1 if contigs else 0)] = _attr(l, "ID")
    at = 9 + l_text
    while at < len(data):
        l_shared, l_indiv = struct.unpack_from("<II", data, at)
        at += 8
        c = _Cur(data, at, at + l_shared)
        chrom, pos0, rlen = struct.unpack("<iii", c.take(12))
        qual, nai, nfs = struct.unpack("<III", c.take(12))
        n_allele, n_info, n_fmt, n_sample = nai >> 16, nai & 0xFFFF, nfs >> 24, nfs & 0xFFFFFF
        vid = c.typed_str()
        alleles = [c.typed_str() for _ in range(n_allele)]
        assert rlen == len(alleles[0])
        cols = [contigs[chrom], str(pos0 + 1), vid or ".", alleles[0], ",".join(alleles[1:]) or ".", float_text(None, qual)]
        t, n = c.desc()
        cols.append(";".join(dic[c.int_of(t)] for _ in range(n)) or ".")
        infos = []
        for _ in range(n_info):
            key = dic[c.typed_int()]
            t, n = c.desc()
            infos.append(key if t == 0 or n == 0 else key + "=" + _vector(c, t, n, key, float_text))
        cols.append(";".join(infos) or ".")
        assert c.at == c.end, "the shared block is longer than its fields"
        at += l_shared
        if n_fmt and n_sample:
            c = _Cur(data, at, at + l_indiv)
            fields = []
            for _ in range(n_fmt):
                key = dic[c.typed_int()]
                t, n = c.desc()
                fields.append((key, t, n, c.at))
                c.take(n_sample * n * WIDTH[t])
            assert c.at == c.end, "the per-sample block is longer than its fields"
            cols.append(":".join(f[0] for f in fields))
            for s in range(n_sample):
                cell = []
                for key, t, n, start in fields:
                    v = _Cur(data, start + s * n * WIDTH[t], start + (s + 1) * n * WIDTH[t])
                    if key == "GT":
                        g = ""
                        for q in range(n):
                            x = v.int_of(t)
                            if x == EOV[t]:
                                break
                            g += ("|" if x & 1 else "/") * (q > 0) + ("." if x >> 1 == 0 else str((x >> 1) - 1))
                        cell.append(g or ".")
                    else:
                        cell.append(_vector(v, t, n, key, float_text))
                cols.append(":".join(cell))
        else:
            assert l_indiv == 0
        at += l_indiv
        lines.append("\t".join(cols))
    return lines


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------

def test_the_decoder_reads_back_the_test_writer(tmp_path):
    """a small multi-sample VCF with int8 / int16 / int32 fields, a vector longer than 14, floats, flags, strings, missing values,
    haploid and phased cells: VCF -> tests/bcf_writer.py -> the decoder gives the VCF back, with and without explicit IDX="""
    alts = ",".join("ACGT"[i % 4] * (2 + i // 4) for i in range(70))            # 71 alleles: GT code (70 + 1) << 1 = 142 needs int16
    header = ["##fileformat=VCFv4.3",
              '##FILTER=<ID=PASS,Description="All filters passed">',
              "##contig=<ID=chr2,length=1000>",
              "##contig=<ID=chr1,length=2000>",
              '##FILTER=<ID=q10,Description="Quality below 10">',
              '##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth">',
              '##INFO=<ID=AC,Number=A,Type=Integer,Description="Allele count, with a comma">',
              '##INFO=<ID=AF,Number=A,Type=Float,Description="Frequency">',
              '##INFO=<ID=DB,Number=0,Type=Flag,Description="A flag">',
              '##INFO=<ID=AA,Number=1,Type=String,Description="A string">',
              '##INFO=<ID=DP,Number=1,Type=Integer,Description="Declared twice: one entry">',
              '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">']
    chrom = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\ts3"
    records = ["chr2\t5\t.\tA\tC\t.\tPASS\tDP=127;AC=1;AF=0.5\tGT\t0/1\t1|1\t./.",                      # int8 everywhere
               "chr2\t9\trs1\tAC\tA,ACC\t30\tq10\tDP=128;AC=-121,3;AF=0.25,.;DB\tGT\t0/2\t2|0\t0",      # int16 values; a haploid cell among diploid ones
               "chr1\t70000\trs2;x\tG\tT\t12.5\tPASS;q10\tDP=32768;AC=-32761;AA=hello\tGT\t0|0\t.|1\t1/.",  # int32 values
               "chr1\t70001\t.\tG\t" + alts + "\t1e+06\t.\tAC=" + ",".join(str(i) for i in range(70)) + ";DP=.\tGT\t70/0\t0/69\t1/1",  # a vector of 70, GT as int16
               "chr1\t70002\t.\tT\t.\t0\tPASS\t.\tGT\t0\t0\t.",                                          # no ALT, haploid
               "chr1\t70003\t.\tT\tTTTTTTTTTTTTTTTTTTTT\t3\tPASS\tDP=2147483647;AC=-2147483640\tGT\t1/1\t0/0\t0/1"]  # a string longer than 14, int32's ends
    vcf = tmp_path / "y.vcf"
    vcf.write_text("\n".join(header + [chrom] + records) + "\n")
    for with_idx in (False, True):
        out = str(tmp_path / ("y%d.bcf" % with_idx))
        bcf_writer.vcf_to_bcf(str(vcf), out, with_idx=with_idx)
        data = open(out, "rb").read()
        members = bgzf_members(data)
        assert members[-1][0] == BGZF_EOF and all(len(m) <= 1 << 16 for m, _ in members)
        got = bcf_to_vcf(bcf_bytes(out))
        head = [l for l in got if l.startswith("#")]
        strip = lambda l: l if not with_idx else l.replace(",IDX=%s>" % _attr(l, "IDX"), ">")
        assert [strip(l) for l in head] == header + [chrom]
        assert got[len(head):] == records
    # the types the writer chose are the ones the case is about
    raw = bcf_bytes(str(tmp_path / "y0.bcf"))
    assert bytes([0x11, 127]) in raw and bytes([0x12]) + struct.pack("<h", 128) in raw and bytes([0x13]) + struct.pack("<i", 32768) in raw
    assert bytes([0xF1, 0x11, 70]) in raw                                          # desc(70, int8): the overflow form


# ---- the product, as far as it goes without a GPU ----------------------------------------------------------------------------------

def test_the_three_symbols_are_exported():
    from malva_amd import capi
    L = capi.lib()
    for name in ("mg_encode_calls_bcf", "mg_encode_calls_bcf_device", "mg_bcf_stats"):
        assert name in capi.EXPORTED and hasattr(L, name), name
    from malva_amd import Context
    for name in ("encode_calls_bcf", "encode_calls_bcf_device", "bcf_stats"):
        assert hasattr(Context, name), name


def _refused(args):
    r = subprocess.run([BIN, "call"] + args + ["ref.fa", "panel.vcf", "cohort.tsv"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr


def test_merged_format_on_the_command_line():
    assert "--merged-format goes with --merged" in _refused(["--cohort", "-o", "out", "--merged-format", "bcf"])
    assert "--merged-format goes with --merged" in _refused(["--merged-format", "ubcf"])
    for bad in ("sam", "BCF", ""):
        assert "--merged-format takes vcf, bcf or ubcf" in _refused(["--cohort", "--merged", "m", "--merged-format", bad])
    r = subprocess.run([BIN, "call", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--merged-format" in r.stdout and "ubcf" in r.stdout and "BGZF" in r.stdout
    assert "bcftools" in r.stdout and "UNPINNED" in r.stdout

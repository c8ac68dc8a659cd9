"""FASTA inputs for the `bwa-amd index` tests (tests/test_fasta_index.py, tests/test_gpu_fasta_index.py): the cases of kseq_read +
add1 (kseq.h:175-215, bntseq.c:232-278) that decide which bytes become bases, how ambiguity codes are replaced and where holes start."""
import gzip
import os

import numpy as np


def _acgt(rng, n, lower=False):
    s = np.frombuffer(b"acgt" if lower else b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    return s


def _lines(s: bytes, width=60, eol=b"\n"):
    return b"".join(s[i:i + width] + eol for i in range(0, len(s), width))


def small_cases():
    """name -> bytes: small files (the tiny-chunk sweeps run on these)"""
    rng = np.random.default_rng(2024)
    c = {}
    c1 = b"N" * 70 + _acgt(rng, 500) + b"N" * 130 + _acgt(rng, 400) + b"N" * 61
    c["multi_contig"] = (b">chr1\n" + _lines(c1) + b">chr2 second contig\n" + _lines(b"N" * 250) + b">chr3\n" + _lines(_acgt(rng, 777) + b"NNN")
                         + b">chr4\n" + _lines(b"A" * 3 + b"N" * 5 + b"C" * 2))
    c["ambiguity_codes"] = (b">mix\n" + _lines(_acgt(rng, 50) + b"NNnnNnRRYKMSWBDHVNrykmswbdhvn-*.--**..N" + _acgt(rng, 40, lower=True) + b"acgtNNNNacgt"
                                               + _acgt(rng, 30) + b"XxZz0123 \t" + _acgt(rng, 10)) + b">nN\n" + b"nNnN" * 20 + b"\n")
    c["crlf"] = (b">c1 comment\r\n" + _lines(_acgt(rng, 130) + b"NNN" + _acgt(rng, 70), eol=b"\r\n") + b">c2\r\n\r\nACGT\r\n"
                 + b">c3\r\n\r\r\nACGT\r\r\nGG\r\n" + b">c4\r\nAC\r\r\r\nN\r\nN\r\n")
    c["headers"] = (b">tab\tcomment with\ttabs\nACGTACGT\n>  two spaces\nCCCC\n>trail \r\nGGGG\n>cr\r\nTTTT\n>\nAAAA\n>sp_only \nACAC\n"
                    + b">long " + b"x" * 3000 + b" end\nGTGT\n>vt\x0bv\fw\nAC\n")
    c["structure"] = (b"some text before the first record\nACGT > here\n>first\n\n\nACGT\n\n>empty\n>e2\n\n>x\nAAAA\nCC\n\n\nGGNN\n>last\nACGTNN")
    c["lone_cr_first"] = b">a\n\r\nACGT\n\r\n>b\n\r\n\r\nAC\n>c\nAC\n\r"
    c["cr_eof"] = b">a\nACGT\r"
    c["gt_eof"] = b">a\nACGTN\n>"
    c["name_only_eof"] = b">a\nACGT\n>b"
    c["mid_gt"] = b"xx>chr0 c\nAC>GT\n>chr1\nA\n"
    return c


def big_cases():
    """name -> bytes: a 1 Mbp single-line contig, and > 2^20 ambiguous bases (the high entries of the lrand48 jump table)"""
    rng = np.random.default_rng(7)
    one = bytearray(_acgt(rng, 1_000_000))
    one[1000:1500] = b"N" * 500
    one[500_000:500_010] = b"RYKMSWBDHV"
    c = {"single_line_1m": b">one line\n" + bytes(one) + b"\n"}
    amb = b"N" * 700_000 + b"nNRn" * 100_000 + b"N" * 300_000
    c["many_ambiguous"] = b">lots\n" + _lines(_acgt(rng, 5000) + amb + _acgt(rng, 5000)) + b">tail\n" + _lines(_acgt(rng, 3000))
    return c


def write_all(d, cases):
    """write the cases as <d>/<name>.fa (plus a gzip copy of the first as <name>.fa.gz); returns [path]"""
    out = []
    for i, (name, data) in enumerate(cases.items()):
        p = os.path.join(d, name + ".fa")
        with open(p, "wb") as f:
            f.write(data)
        out.append(p)
        if i == 0:
            with gzip.open(p + ".gz", "wb") as f:
                f.write(data)
            out.append(p + ".gz")
    return out


# input the reference reads as FASTQ or leaves undefined: rejected with BWAGPU_EINVAL and no files
REJECTED = {
    "at_before_gt": b"junk @read\nACGT\n>a\nACGT\n",
    "plus_line": b">a\nACGT\n+\nIIII\n",
    "at_line": b">a\nACGT\n@b\nACGT\n",
    "nul_byte": b">a\nAC\x00GT\n",
    "high_byte": b">a\nAC\xc3\xa9GT\n",
    "no_record": b"ACGT\nACGT\n",
    "empty_file": b"",
    "gt_only": b">",
    "no_base": b">a\n>b\n\n",
}

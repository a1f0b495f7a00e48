#!/usr/bin/env python3
"""Fixtures for the FASTQ-format reference reader of `smaltgpu-map index` (smalt_amd/csrc/smg_fastq_ref.hpp), from the UNMODIFIED
reference.

The three random sequences of make_golden_fasta.py (500, 333 and 401 bases) as FASTQ records in several dresses, texts the reader
has to refuse among them: each text is about 1 to 3 kB (7 kB with the long '+' line).  Every text goes through the reference's `smalt index -k 11 -s 2`; the
manifest (manifest_fastq_ref.json) keeps its exit status, the md5 of the `.sma` / `.smi` files it wrote, the names and lengths of
the sequences read back from its `.sma`, and its message where it failed.  The texts are committed gzipped
(fastq_ref_<tag>.fa.gz).  Runs only where the reference is built (`make -C oracle ref`).  Fixtures are data only."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden_fasta import K, REF, S, md5, read_back, wrap  # noqa: E402


def texts():
    rng = np.random.default_rng(20260)
    a, b, c = (bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]) for n in (500, 333, 401))
    qrng = np.random.default_rng(20261)

    def qual(n, lo=35, hi=62):            # no '@' (64) and no '+' (43), '>' (62) unless a case puts them somewhere
        q = qrng.integers(lo, hi, n).astype(np.uint8)
        q[q == 43] = 44
        return q.tobytes()

    qa, qb, qc = qual(500), qual(333), qual(401)

    def rec(name, seq, q, plus=b"+"):
        return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + q + b"\n"

    four = rec(b"s1", a, qa) + rec(b"s2 second sequence", b, qb, b"+s2 second sequence") + rec(b"s3", c, qc)
    t = {}
    t["four_line"] = four
    # sequence and quality wrapped; quality lines that begin with '@', '+' and '>'
    qa2 = bytearray(qa)
    qa2[60], qa2[120], qa2[180] = ord("@"), ord("+"), ord(">")
    t["wrapped"] = (b"@s1\n" + wrap(a, 60) + b"+\n" + wrap(bytes(qa2), 60) + b"@s2 second sequence\n" + wrap(b, 70) + b"+\n" + wrap(qb, 50) +
                    b"@s3\n" + wrap(c, 50) + b"+s3\n" + wrap(qc, 80))
    t["qual_at_first"] = rec(b"s1", a, b"@" + qa[1:]) + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    t["plus_segment_between"] = rec(b"s1", a, qa) + b"+zz\n" + qual(10) + b"\n" + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    t["plus_segment_first"] = b"+junk\n" + qual(25) + b"\n" + four
    t["fasta_then_fastq"] = b">s1\n" + wrap(a, 60) + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    t["fasta_with_quality"] = b">s1\n" + wrap(a, 60) + b"+\n" + wrap(qa, 60) + b">s2 second sequence\n" + wrap(b, 70) + b">s3\n" + wrap(c, 50) + b"+\n" + qc + b"\n"
    t["qual_at_behind_plus"] = b"@s1\n" + wrap(a, 100) + b"+\n@" + qa[1:100] + b"\n" + wrap(qa[100:], 100) + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    t["crlf_blank_noeol"] = (rec(b"s1", a, qa) + b"\n" + rec(b"s2  two   spaces\t tab ", b, qb) + b"\n" + rec(b"s3", c, qc)).replace(b"\n", b"\r\n")[:-2]
    # refused: the quality does not have the length of the sequence
    t["qual_one_more"] = rec(b"s1", a, qa + b"I") + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    t["qual_extra_line"] = rec(b"s1", a, qa + b"\nII") + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    t["qual_short_at_end"] = rec(b"s1", a, qa) + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc[:-4])
    t["qual_short_first"] = rec(b"s1", a, qa[:-10]) + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    # further shapes
    t["header_after_header"] = b"@s1\n@s2\n" + a + b"\n+\n" + qual(3) + qa + b"\n" + rec(b"s3", c, qc)           # '@s2' and the bases are one sequence
    t["space_before_at"] = rec(b"s1", a, qa) + b" @x\n" + rec(b"s3", c, qc)                               # ' @x' is data of s1's quality: refused
    t["space_before_at_in_fasta"] = b">s1\n" + wrap(a, 60) + b" @x\n" + wrap(b, 70) + rec(b"s3", c, qc)  # data of s1
    t["lower_iupac"] = rec(b"s1", a[:150].lower() + a[150:], qa) + rec(b"s2", b[:90] + b"N" * 25 + b[115:], qb) + rec(b"s3", c[:40] + b"RYKMU" + c[45:300] + b"rykmu" + c[305:], qc)
    t["at_inside_fasta_data"] = b">s1\n" + wrap(a[:240], 60) + b"@s2 opened inside\n" + wrap(a[240:], 60) + b">s3\n" + wrap(c, 50)
    t["long_plus_header"] = rec(b"s1", a, qa, b"+" + b"".join(b"w%03d " % i for i in range(999)) + b"end") + rec(b"s2 second sequence", b, qb) + rec(b"s3", c, qc)
    assert len(t["long_plus_header"].split(b"\n")[2]) > 4990
    return t


if __name__ == "__main__":
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", "oracle"], check=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, text in texts().items():
            fa = os.path.join(tmp, tag + ".fa")
            with open(fa, "wb") as f:
                f.write(text)
            pre = os.path.join(tmp, tag)
            r = subprocess.run([os.path.join(REF, "smalt"), "index", "-k", str(K), "-s", str(S), pre, fa], capture_output=True)
            e = dict(tag=tag, file="fastq_ref_%s.fa.gz" % tag, k=K, s=S, ref_status=r.returncode)
            if r.returncode == 0:
                e["sma_md5"], e["smi_md5"] = md5(pre + ".sma"), md5(pre + ".smi")
                e["names"], e["lengths"] = read_back(pre)
            else:
                e["ref_message"] = [ln.split("ERROR:")[-1].strip() for ln in (r.stderr + r.stdout).decode("latin-1").split("\n") if "ERROR:" in ln][:1]
            with gzip.GzipFile(os.path.join(HERE, e["file"]), "wb", mtime=0) as g:
                g.write(text)
            manifest.append(e)
            print(e)
    json.dump(manifest, open(os.path.join(HERE, "manifest_fastq_ref.json"), "w"), indent=1)

#!/usr/bin/env python3
"""Fixtures for the FASTA reader of `smaltgpu-map index` (smalt_amd/csrc/smg_fasta.hpp), from the UNMODIFIED reference.

Three random sequences of 500, 333 and 401 bases in several dresses: each text is about 1 kB.  Every text goes through the
reference's `smalt index -k 11 -s 2`; the manifest (manifest_fasta.json) keeps its exit status, the md5 of the `.sma` / `.smi`
files it wrote and the names and lengths of the sequences read back from its `.sma` (or_index_read).  The texts are committed
gzipped (fasta_<tag>.fa.gz).  Runs only where the reference is built (`make -C oracle ref`).  Fixtures are data only."""
import ctypes as C
import gzip
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
K, S = 11, 2


def wrap(seq, width, eol=b"\n"):
    return b"".join(seq[o:o + width] + eol for o in range(0, len(seq), width))


def texts():
    rng = np.random.default_rng(20260)
    a, b, c = (bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)]) for n in (500, 333, 401))
    plain = b">s1\n" + wrap(a, 60) + b">s2 second sequence\n" + wrap(b, 70) + b">s3\n" + wrap(c, 50)
    t = {}
    t["plain"] = plain
    t["plaingz"] = plain                          # handed to the programs gzipped
    t["crlf"] = b">s1\r\n" + wrap(a, 60, b"\r\n") + b">s2  two   spaces\t tab \r\n" + wrap(b, 70, b"\r\n") + b">s3\r\n" + wrap(c, 50, b"\r\n")
    t["noeol"] = plain[:-1]
    t["blank"] = (b"\n\n>s1\n\n" + wrap(a, 60).replace(b"\n", b"\n\n", 3) + b"\n>s2 second sequence\n" + wrap(b, 70) + b"\n\n>s3\n" + wrap(c, 50) + b"\n\n")
    t["oneline"] = b">s1\n" + a + b"\n>s2 second sequence\n" + b + b"\n>s3\n" + c + b"\n"
    t["inner_space"] = (b">s1\n" + wrap(a, 60, b"  \n") + b">s2 second sequence\n" + b[:70] + b"\n " + b[70:140] + b" \t\n" + wrap(b[140:], 70) + b">s3\n" + wrap(c, 50))
    t["gt_in_header"] = plain.replace(b">s1\n", b">s1 a>b >c\n")
    t["space_before_prompt"] = b">s1\n" + wrap(a, 60) + b" >s2\n" + wrap(b, 70) + b">s3\n" + wrap(c, 50)
    t["header_after_header"] = b">s1\n>s2\n" + wrap(a, 60) + b">s3\n" + wrap(c, 50)
    t["digit"] = b">s1\n" + wrap(a[:100] + b"1" + a[100:], 60) + b">s2\n" + wrap(b, 70) + b">s3\n" + wrap(c, 50)
    t["dash"] = b">s1\n" + wrap(a, 60) + b">s2\n" + wrap(b[:200] + b"-*" + b[200:], 70) + b">s3\n" + wrap(c, 50)
    t["lower_iupac"] = (b">s1\n" + wrap(a[:150].lower() + a[150:], 60) + b">s2\n" + wrap(b[:90] + b"N" * 25 + b[115:], 70) +
                        b">s3\n" + wrap(c[:40] + b"RYKMU" + c[45:300] + b"rykmu" + c[305:], 50))
    t["empty_name"] = b">s1\n" + wrap(a, 60) + b">\n" + wrap(b, 70) + b">s3\n" + wrap(c, 50)
    t["longhead"] = b">s1\n" + wrap(a, 60) + b">s2 " + b"".join(b"w%03d " % i for i in range(999)) + b"end\n" + wrap(b, 70) + b">s3\n" + wrap(c, 50)
    assert len(t["longhead"].split(b"\n")[10]) > 4990
    t["nohead"] = wrap(a[:120], 60) + plain
    t["short_last"] = b">s1\n" + wrap(a, 60) + b">s2\n" + wrap(b, 70) + b">s3\nACGT\n"
    t["fastq"] = b"@r1\n" + a[:80] + b"\n+\n" + b"I" * 80 + b"\n@r2 x\n" + b[:64] + b"\n+r2\n" + b"5" * 64 + b"\n"
    return t


# what this project does with the text (the reference takes `fastq` too: that is the documented refusal)
EXPECT = {"nohead": "nohead", "short_last": "short", "fastq": "fastq"}


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def read_back(prefix):
    ix = ol.lib().or_index_read(prefix.encode())
    assert ix
    x = ix.contents
    addr = C.cast(C.byref(x, ol.OrIndex.names.offset), C.POINTER(C.c_void_p))[0]
    names = C.string_at(addr, x.namsiz).split(b"\0")[:x.nseq]
    lens = [int(x.sop[i + 1] - x.sop[i]) for i in range(x.nseq)]
    ol.lib().or_index_free(ix)
    return [n.decode("latin-1") for n in names], lens


if __name__ == "__main__":
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", "oracle"], check=True)
    manifest = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, text in texts().items():
            gz = tag.endswith("gz")
            fa = os.path.join(tmp, tag + (".fa.gz" if gz else ".fa"))
            with open(fa, "wb") as f:
                f.write(gzip.compress(text, mtime=0) if gz else text)
            pre = os.path.join(tmp, tag)
            r = subprocess.run([os.path.join(REF, "smalt"), "index", "-k", str(K), "-s", str(S), pre, fa], capture_output=True)
            e = dict(tag=tag, file="fasta_%s.fa.gz" % tag, gz=gz, k=K, s=S, ref_status=r.returncode, expect=EXPECT.get(tag, "ok"))
            if r.returncode == 0:
                e["sma_md5"], e["smi_md5"] = md5(pre + ".sma"), md5(pre + ".smi")
                e["names"], e["lengths"] = read_back(pre)
            else:
                e["ref_message"] = [ln.split("ERROR:")[-1].strip() for ln in (r.stderr + r.stdout).decode("latin-1").split("\n") if "ERROR:" in ln][:1]
            with gzip.GzipFile(os.path.join(HERE, e["file"]), "wb", mtime=0) as g:
                g.write(text)
            manifest.append(e)
            print(e)
    json.dump(manifest, open(os.path.join(HERE, "manifest_fasta.json"), "w"), indent=1)

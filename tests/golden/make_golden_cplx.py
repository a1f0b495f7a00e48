"""Fixtures of tests/test_cplx.py from the unmodified reference program (oracle/_ref/smalt, built by `make -C oracle ref`), for
the single reads of tests/cplx_data.py (the first read of every pair) on its reference, index k = 11, s = 3:
  cplx.fa.gz            the reference sequences,
  cplx.fq.gz            the reads,
  cplx.cigar.out.gz     what `smalt map -f cigar -d 3 -r -1` printed,
  cplx.cigar_w.out.gz   what `smalt map -w -f cigar -d 3 -r -1` printed.
Data only.  Usage: python tests/golden/make_golden_cplx.py"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cplx_data  # noqa: E402

SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")


def _gz(name, data):
    with open(os.path.join(HERE, name), "wb") as f:
        with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
            g.write(data)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        w = cplx_data.prepare(tmp, SMALT)
        _gz("cplx.fa.gz", open(w["fa"], "rb").read())
        _gz("cplx.fq.gz", open(w["fq1"], "rb").read())
        outs = {}
        for tag, opt in (("cigar", []), ("cigar_w", ["-w"])):
            out = os.path.join(tmp, tag + ".out")
            subprocess.run([SMALT, "map"] + opt + ["-f", "cigar", "-d", "3", "-r", "-1", "-o", out, w["pre"], w["fq1"]], check=True, capture_output=True)
            outs[tag] = open(out, "rb").read()
            _gz("cplx.%s.out.gz" % tag, outs[tag])
        a, b = outs["cigar"].split(b"\n"), outs["cigar_w"].split(b"\n")
        print(len(a), len(b), "lines;", sum(1 for x in b if x not in set(a)), "of the -w lines are not among the lines without -w")


if __name__ == "__main__":
    main()

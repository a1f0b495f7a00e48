"""Fixtures of tests/test_inshist.py from the unmodified reference program (oracle/_ref/smalt, built by `make -C oracle ref`):
for the 1800-pair input of tests/inshist_data.py (`all`) and for its first 100 pairs (`first`, a histogram with bins wider
than 1)
  inshist_<tag>.sample.txt   what `smalt sample -o` wrote from the line `# Sampled histogram` to the end of the file: the two
                             prints of the histogram made from the sample and the section `smalt map -g` reads,
  inshist_<tag>.stdout.txt   what `smalt map -g <that file>` wrote to standard output: the two prints, at 80 columns, of the
                             histogram it read back and smoothed again.
Usage: python tests/golden/make_golden_inshist.py"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import inshist_data  # noqa: E402

SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        pre, pairs = inshist_data.prepare(tmp, SMALT)
        for tag, sub in (("all", pairs), ("first", pairs[:100])):
            fqs = inshist_data.write_pairs(os.path.join(tmp, tag), sub)
            smp = os.path.join(tmp, tag + ".smp")
            subprocess.run([SMALT, "sample", "-o", smp, pre] + fqs, check=True, capture_output=True)
            text = open(smp, "rb").read()
            tail = text[text.index(b"# Sampled histogram\n"):]
            r = subprocess.run([SMALT, "map", "-g", smp, "-f", "cigar", "-r", "7", "-o", os.path.join(tmp, "map.out"), pre] + fqs, check=True, capture_output=True)
            for ext, data in (("sample", tail), ("stdout", r.stdout)):
                with open(os.path.join(HERE, "inshist_%s.%s.txt" % (tag, ext)), "wb") as f:
                    f.write(data)
            head = [ln for ln in tail.decode().split("\n") if ln.startswith("HISTO_")]
            print(tag, len(tail), len(r.stdout), " ".join(head[1:7]))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates the fixtures of the explicit alignment blocks (`smalt map -a`): what the reference program (oracle/_ref/smalt, the
reference compiled here by oracle/Makefile) prints behind the line of every mapped alignment -- the read and the reference side by
side in blocks of 60 columns with a row of markers between them (fprintAlignment, report.c:248-388).  Two kinds of fixture:

  * `-a` variants of committed inputs (single reads, one paired and one split-read fixture): `<tag>.<variant>.out.gz`, no new input;
  * `ali_shapes`, a small synthetic input written here with a fixed seed (`ali_shapes.fa.gz`, `ali_shapes.fq.gz`) whose reads pin
    down the corners of the block layout: alignments of exactly 60 and 120 columns (the reference prints one more block with empty
    rows behind them), a run of more than 62 matches (two codes of the alignment string), a gap in the 60th column of a line,
    transitions and transversions, N and an IUPAC letter in a read on both strands, an N in the reference, a lower-case read.

The generator ASSERTS that the reference's output shows every shape and records the counts per case in manifest_ali.json; the tests
assert the same counts on the committed text before they compare, so a fixture that lost a shape fails instead of passing on less.
The marker `!` (a non-standard letter) is counted too, but no input can produce it: the reference's codec files every letter other
than ACGT under "unknown" (make3BitMangledCodec, sequence.c:287-318 gives them the 3-bit code of N), which prints `?`.
Data only; needs the reference program (oracle/_ref, built from its sources by oracle/Makefile) and is not run by the tests.

    python tests/golden/make_golden_ali.py
"""
import gzip
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
from ali_data import shapes_of  # noqa: E402

SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
# (fixture, variant, options behind the fixture's own) -- single reads
SINGLE = [("g_k13s6_ties", "ali_cigar", ["-r", "3", "-f", "cigar", "-a"]),
          ("g_k13s6_ties", "ali_sam", ["-r", "3", "-f", "sam", "-a"]),
          ("g_k13s6_ties", "ali_ssaha_d0", ["-r", "3", "-d", "0", "-f", "ssaha", "-a"]),
          ("g_k11s2_d20", "ali_cigar", ["-r", "3", "-f", "cigar", "-a"]),                 # rich in insertions and deletions
          ("g_k11s4_cat", "ali_cigar", ["-r", "3", "-f", "cigar", "-a"])]                 # concatenated mode: alignments cut at sequence junctions
PAIRED = [("gp_k13s6_pe", "ali_sam", ["-r", "3", "-f", "sam", "-a"]), ("gp_k13s6_pe", "ali_cigar", ["-r", "3", "-f", "cigar", "-a"])]
SPLIT = [("gs_k11s3_q10", "ali_split_cigar", ["-p", "-r", "-1", "-f", "cigar", "-a"])]
SHAPES_TAG, SHAPES_K, SHAPES_S, SHAPES_OPTS = "ali_shapes", 11, 2, ["-r", "-1", "-f", "cigar", "-a"]

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(COMPLEMENT.get(c, c) for c in reversed(s))


def run_map(opts, prefix, reads):
    """`smalt map` in the directory of its input, all files named without it: the @PG line of a SAM header repeats the command line,
    the program too is called by a link from there.  The fixtures must come out the same byte for byte wherever they are made"""
    cwd = os.path.dirname(prefix)
    if not os.path.exists(os.path.join(cwd, "smalt")):
        os.symlink(SMALT, os.path.join(cwd, "smalt"))
    subprocess.run(["./smalt", "map"] + opts + ["-o", "o.txt", os.path.basename(prefix)] + [os.path.basename(r) for r in reads], check=True, capture_output=True, cwd=cwd)
    return open(os.path.join(cwd, "o.txt"), "rb").read()


def keep(tag, variant, txt):
    with gzip.GzipFile(os.path.join(HERE, "%s.%s.out.gz" % (tag, variant)), "wb", mtime=0) as g:
        g.write(txt)
    sh = shapes_of(txt)
    print(tag, variant, txt.count(b"\n"), "lines", sh)
    return sh


def make_shapes(tmp):
    """the synthetic input: two sequences (the second with one N) and reads cut from them -> (fasta path, fastq path)"""
    rnd = random.Random(20240611)
    seq = {"shapeA": [rnd.choice("ACGT") for _ in range(2400)], "shapeB": [rnd.choice("ACGT") for _ in range(1300)]}
    seq["shapeB"][640] = "N"
    seq = {k: "".join(v) for k, v in seq.items()}
    A, B = seq["shapeA"], seq["shapeB"]
    reads = []

    def both(name, s):
        reads.append((name + "_f", s))
        reads.append((name + "_r", revcomp(s)))

    def change(s, at, kind):
        to = {"transition": {"A": "G", "G": "A", "C": "T", "T": "C"}, "transversion": {"A": "C", "C": "A", "G": "T", "T": "G"}}[kind][s[at]]
        return s[:at] + to + s[at + 1:]

    def unambiguous(s, at):                 # a place where a single-base gap can stand in one column only
        while not (s[at - 1] != s[at] != s[at + 1]):
            at += 1
        return at

    both("exact60", A[100:160])                                         # 60 and 120 columns: a block with empty rows follows
    both("exact120", A[200:320])
    both("run150", A[350:500])                                          # more than 124 bases without a difference: two codes of 62 matches
    both("run_then_subst", change(A[520:670], 140, "transversion"))     # a run of more than 62 matches in front of a substitution
    p = unambiguous(A, 759)                                             # deletion: the base of the reference in column 60 has no partner
    both("del_col60", A[p - 59:p] + A[p + 1:p + 72])
    p = unambiguous(A, 959)                                             # insertion: the read's extra base is column 60
    extra = [c for c in "ACGT" if c != A[p - 1] and c != A[p]][0]
    both("ins_col60", A[p - 59:p] + extra + A[p:p + 70])
    p = unambiguous(A, 1130)
    both("del2_mid", A[1100:p] + A[p + 2:1230])                         # a longer gap inside a line
    both("subst_both", change(change(A[1250:1350], 30, "transition"), 70, "transversion"))
    both("subst_col60", change(A[1370:1500], 59, "transition"))         # a substitution in the last column of a line
    both("read_N", A[1520:1560] + "N" + A[1561:1620])                   # letters other than ACGT inside the aligned part
    both("read_R", A[1640:1680] + "R" + A[1681:1740])
    both("across_ref_N", B[590:700])                                    # the N of the second sequence
    both("ref_N_and_subst", change(B[600:720], 90, "transition"))
    both("exact60_B", B[900:960])
    reads.append(("lower_case", A[1760:1860].lower()))
    reads.append(("lower_case_r", revcomp(A[1880:1990]).lower()))
    reads.append(("exact61", A[2000:2061]))                             # one column into the second block
    reads.append(("exact59", A[2080:2139]))
    reads.append(("exact180_r", revcomp(A[2150:2330])))
    reads.append(("unmapped", "".join(rnd.choice("ACGT") for _ in range(80))))
    fa, fq = os.path.join(tmp, SHAPES_TAG + ".fa"), os.path.join(tmp, SHAPES_TAG + ".fq")
    with open(fa, "w") as f:
        for k, s in seq.items():
            f.write(">%s\n" % k)
            for o in range(0, len(s), 70):
                f.write(s[o:o + 70] + "\n")
    with open(fq, "w") as f:
        for nm, s in reads:
            f.write("@%s\n%s\n+\n%s\n" % (nm, s, "I" * len(s)))
    for path in (fa, fq):
        with open(path, "rb") as f, gzip.GzipFile(os.path.join(HERE, os.path.basename(path) + ".gz"), "wb", mtime=0) as g:
            g.write(f.read())
    return fa, fq, len(reads)


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    man = []
    with tempfile.TemporaryDirectory() as tmp:
        entries = {e["tag"]: e for e in gu.MANIFEST_ALL}
        unpacked = {}
        for tag, variant, vopts in SINGLE:
            if tag not in unpacked:
                unpacked[tag] = gu.unpack(entries[tag], tmp)
            fx = unpacked[tag]
            opts = entries[tag]["opts"].split() + vopts
            txt = run_map(opts, fx["prefix"], [fx["fq"]])
            man.append(dict(kind="single", tag=tag, variant=variant, opts=opts, lines=txt.count(b"\n"), shapes=keep(tag, variant, txt)))
        for kind, cases, manifest, exts in (("pair", PAIRED, "manifest_pairs.json", (".fa", "_1.fq", "_2.fq")), ("split", SPLIT, "manifest_split.json", (".fa", ".fq"))):
            known = {e["tag"]: e for e in json.load(open(os.path.join(HERE, manifest)))}
            for tag, variant, vopts in cases:
                e = known[tag]
                paths = []
                for ext in exts:
                    paths.append(os.path.join(tmp, tag + ext))
                    with gzip.open(os.path.join(HERE, tag + ext + ".gz"), "rb") as g, open(paths[-1], "wb") as f:
                        f.write(g.read())
                pre = os.path.join(tmp, tag)
                subprocess.run([SMALT, "index", "-k", str(e["k"]), "-s", str(e["s"]), pre, paths[0]], check=True, capture_output=True)
                opts = e["opts"].split() + vopts
                txt = run_map(opts, pre, paths[1:])
                man.append(dict(kind=kind, tag=tag, variant=variant, opts=opts, lines=txt.count(b"\n"), shapes=keep(tag, variant, txt)))
        fa, fq, nreads = make_shapes(tmp)
        pre = os.path.join(tmp, SHAPES_TAG)
        subprocess.run([SMALT, "index", "-k", str(SHAPES_K), "-s", str(SHAPES_S), pre, fa], check=True, capture_output=True)
        txt = run_map(SHAPES_OPTS, pre, [fq])
        sh = keep(SHAPES_TAG, "ali_cigar", txt)
        # every shape the input was made for must show in what the reference printed
        for key in ("empty_blocks", "gap", "transition", "transversion", "unknown", "descending", "gap_in_last_column"):
            assert sh[key] >= 1, "ali_shapes: the reference's output shows no %s" % key
        assert sh["empty_blocks"] >= 7 and sh["gap_in_last_column"] >= 4, sh
        man.append(dict(kind="shapes", tag=SHAPES_TAG, variant="ali_cigar", k=SHAPES_K, s=SHAPES_S, nreads=nreads, opts=SHAPES_OPTS, lines=txt.count(b"\n"), shapes=sh))
    for m in man:                               # every case prints blocks, the paired and the split case on both strands
        assert m["shapes"]["blocks"] >= 1 and m["shapes"]["descending"] >= 1, m
    json.dump(man, open(os.path.join(HERE, "manifest_ali.json"), "w"), indent=1)


if __name__ == "__main__":
    main()

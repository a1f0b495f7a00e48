"""The input of the complexity-weighting tests (tests/test_cplx.py, tests/test_gpu_cplx.py, tests/golden/make_golden_cplx.py),
from fixed seeds: three sequences of about 22 kb of random sequence with a low-complexity insert of 30-160 bases every
400-900 bases (homopolymer, 2- and 3-base repeats, AT-rich), 400 read pairs of 40-150 bases (the read reverse-complemented
in half of the pairs, the mate 250 bases downstream; 0-3 substitutions, a 1-3-base deletion or insertion in one read of
five each, an N in one of ten) and 8 long reads of 257-3000 bases (2 % substitutions, 1 % insertions, 1 % deletions; the
lengths are a ladder, because the reference program needs 6 s for a read of 3000 bases at -d -1 and 0.5 s for one of 1250).
`smalt map -w` lowers the score of an alignment by the composition of the reference letters it pairs, so the inserts are
what makes it change lines.  The index is k = 11, s = 3, so that reads of 40 bases seed.

Also here: the restatement of the reference's arithmetic the tests compare with (scoreMatrixCalcLambda, score.c:252-277, and
scaleALICPLX, alignment.c:268-305, in Python floats, which are the C doubles) and the parser of CIGAR-format lines."""
import math
import os

import numpy as np

NPAIRS, K, S = 400, 11, 3
LONG_LENGTHS = (257, 320, 450, 640, 900, 1250, 1700, 3000)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
LN0P25 = -1.386294          # alignment.c:71


def _revcomp(b):
    return b[::-1].translate(_COMP)


def make(seed=4108):
    """-> (list of (name, sequence), list of (read, mate), list of long reads), all bytes"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rnd(n):
        return acgt[rng.integers(0, 4, size=n)].tobytes()

    def low(n):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            return b"ACGT"[int(rng.integers(0, 4)):][:1] * n
        if kind in (1, 2):
            u = rnd(kind + 1)
            return (u * (n // len(u) + 1))[:n]
        return acgt[rng.choice(4, size=n, p=[0.45, 0.05, 0.05, 0.45])].tobytes()

    def mut(r):
        r = bytearray(r)
        for _ in range(int(rng.integers(0, 4))):
            r[int(rng.integers(0, len(r)))] = b"ACGT"[int(rng.integers(0, 4))]
        if rng.random() < 0.2:
            p = int(rng.integers(10, len(r) - 10))
            del r[p:p + int(rng.integers(1, 4))]
        if rng.random() < 0.2:
            p = int(rng.integers(10, len(r) - 10))
            r[p:p] = rnd(int(rng.integers(1, 4)))
        if rng.random() < 0.1:
            r[int(rng.integers(0, len(r)))] = ord("N")
        return bytes(r)

    chrs = []
    for _ in range(3):
        parts = []
        for _ in range(30):
            parts.append(rnd(int(rng.integers(400, 900))))
            parts.append(low(int(rng.integers(30, 161))))
        chrs.append(b"".join(parts))
    pairs = []
    for _ in range(NPAIRS):
        c = chrs[int(rng.integers(0, 3))]
        n = int(rng.integers(40, 151))
        p = int(rng.integers(0, len(c) - 500))
        a, b = mut(c[p:p + n]), _revcomp(mut(c[p + 250:p + 250 + n]))
        if rng.random() < 0.5:
            a = _revcomp(a)
        pairs.append((a, b))
    longs = []
    for n in LONG_LENGTHS:
        c = chrs[int(rng.integers(0, 3))]
        p = int(rng.integers(0, len(c) - n))
        out = bytearray()
        for ch in c[p:p + n + n // 50]:
            u = rng.random()
            if u < 0.01:
                continue                                       # deletion
            if u < 0.02:
                out += rnd(1)                                  # insertion ahead of the base
            out.append(b"ACGT"[int(rng.integers(0, 4))] if u >= 0.98 else ch)
        r = bytes(out[:n])
        longs.append(_revcomp(r) if rng.random() < 0.5 else r)
    return [("chr%d" % (i + 1), c) for i, c in enumerate(chrs)], pairs, longs


def balanced_read():
    """(name, read, reference sequence): 4000 bases with exactly 1000 each of A, C, G and T that match their reference exactly --
    the composition for which the reference's cut-off ln(1/4) makes the weighted score exceed the unweighted one"""
    rng = np.random.default_rng(99)
    r = np.frombuffer(b"ACGT" * 1000, dtype=np.uint8).copy()
    rng.shuffle(r)
    return b"bal", r.tobytes(), r.tobytes()


def write_fasta(path, seqs):
    with open(path, "wb") as f:
        for name, s in seqs:
            f.write(b">" + name.encode() + b"\n")
            for o in range(0, len(s), 70):
                f.write(s[o:o + 70] + b"\n")


def fastq_text(reads, stem=b"r", suffix=b""):
    return b"".join(b"@" + stem + b"%d" % i + suffix + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))


def write_fastq(path, reads, stem=b"r", suffix=b""):
    with open(path, "wb") as f:
        f.write(fastq_text(reads, stem, suffix))


def prepare(tmp, smalt):
    """reference, index (k 11, s 3) and the read files under `tmp` -> dict of paths and the data"""
    import subprocess
    seqs, pairs, longs = make()
    w = {"seqs": seqs, "pairs": pairs, "longs": longs, "fa": os.path.join(tmp, "ref.fa"), "pre": os.path.join(tmp, "idx")}
    write_fasta(w["fa"], seqs)
    subprocess.run([smalt, "index", "-k", str(K), "-s", str(S), w["pre"], w["fa"]], check=True, capture_output=True)
    w["fq1"], w["fq2"], w["fql"], w["fql_upto1700"] = (os.path.join(tmp, n) for n in ("r_1.fq", "r_2.fq", "long.fq", "long_upto1700.fq"))
    write_fastq(w["fq1"], [p[0] for p in pairs], b"p", b"/1")
    write_fastq(w["fq2"], [p[1] for p in pairs], b"p", b"/2")
    write_fastq(w["fql"], longs, b"L")
    write_fastq(w["fql_upto1700"], [r for r in longs if len(r) <= 1700], b"L")
    return w


# ---- the reference's arithmetic, restated ----
def calc_lambda(match, mismatch):
    """scoreMatrixCalcLambda (score.c:252-277)"""
    def getsum(lam):
        s = 0.0
        for i in range(4):
            for j in range(4):
                s += math.exp(lam * (match if i == j else mismatch))
        return s * 0.0625
    lower, lam = 0.0, 0.5
    while getsum(lam) < 1.0:
        lower = lam
        lam *= 2.0
    upper = lam
    while upper - lower > .00001:
        lam = (lower + upper) / 2.0
        if getsum(lam) >= 1.0:
            upper = lam
        else:
            lower = lam
    return lam


def scale(counts, orig, lam):
    """scaleALICPLX (alignment.c:268-305): counts in code order A, C, G, T, X, N -> weighted score, or None for ERRCODE_CPLXSCOR"""
    t_factor = t_sum = 0.0
    t_counts = 0
    for c in counts:
        if c:
            t_factor += c * math.log(float(c))
            t_sum += c * LN0P25
            t_counts += c
    t_factor -= t_counts * math.log(float(t_counts))
    t_sum -= t_factor
    adj = int(orig + t_sum / lam + .999)
    if adj > orig:
        return None
    return max(adj, 0)


# ---- CIGAR-format lines (cigar:S name qstart qend strand ref rstart rend + score ops...) ----
def cigar_fields(line):
    """-> (name, ref, rstart, rend, score, ops) or None for a header line or an unmapped read"""
    t = line.split()
    if len(t) < 11 or not t[0].startswith(b"cigar") or t[5] == b"*":
        return None
    return t[1], t[5], int(t[6]), int(t[7]), int(t[9]), t[10:]


def m_counts(fields, ref):
    """letter counts (A, C, G, T, X, N) of the forward-strand reference under the M stretches of a line"""
    _, name, rstart, rend, _, ops = fields
    seq = ref[name]
    p = rstart - 1
    cnt = dict.fromkeys(b"ACGTXN", 0)
    for i in range(0, len(ops), 2):
        o, n = ops[i], int(ops[i + 1])
        if o == b"M":
            for ch in seq[p:p + n]:
                cnt[ch] += 1
            p += n
        elif o == b"D":
            p += n
    assert p == rend, (fields, p)
    return [cnt[c] for c in b"ACGTXN"]

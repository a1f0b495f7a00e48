"""The paired-end input of the insert-size tests (tests/test_gpu_inshist.py, tests/golden/make_golden_inshist.py), from fixed
seeds: 1500 pairs from unique sequence with template lengths drawn from N(300, 25), and 300 pairs whose mate also fits 120
bases further downstream (its 100-base target is there twice), so that a pair has two oriented pairings inside the default
insert range (template lengths 300 and 420) and only a histogram of insert sizes tells them apart."""
import os

import numpy as np

RLEN, NUNIQUE, NDUP = 100, 1500, 300
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(b):
    return b[::-1].translate(_COMP)


def make(seed=7301):
    """-> (list of (name, sequence), list of (read, mate)) with reads as bytes; the pairs are shuffled"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rnd = lambda n: acgt[rng.integers(0, 4, size=n)].tobytes()
    chr1 = rnd(600_000)
    pairs = []
    for _ in range(NUNIQUE):
        ins = max(2 * RLEN - 40, int(round(rng.normal(300, 25))))
        p = int(rng.integers(0, len(chr1) - ins))
        pairs.append((chr1[p:p + RLEN], _revcomp(chr1[p + ins - RLEN:p + ins])))
    units = []
    for _ in range(NDUP):
        head, target = rnd(RLEN), rnd(RLEN)
        units.append(rnd(500) + head + rnd(100) + target + rnd(20) + target + rnd(80))
        pairs.append((head, _revcomp(target)))
    chr2 = b"".join(units) + rnd(500)
    # a substitution in one read of five, none in the first or last 20 bases
    out = []
    for a, b in pairs:
        a, b = bytearray(a), bytearray(b)
        for r in (a, b):
            if rng.random() < 0.2:
                at = int(rng.integers(20, RLEN - 20))
                r[at] = ord("A") if r[at] != ord("A") else ord("C")
        out.append((bytes(a), bytes(b)))
    order = rng.permutation(len(out))
    return [("chr1", chr1), ("chr2", chr2)], [out[int(i)] for i in order]


def write_fasta(path, seqs):
    with open(path, "wb") as f:
        for name, s in seqs:
            f.write(b">" + name.encode() + b"\n")
            for o in range(0, len(s), 70):
                f.write(s[o:o + 70] + b"\n")


def write_pairs(prefix, pairs, copies=1):
    """<prefix>_1.fq / <prefix>_2.fq with `copies` copies of the pairs behind one another, names numbered through"""
    paths = [prefix + "_1.fq", prefix + "_2.fq"]
    for w in (0, 1):
        with open(paths[w], "wb") as f:
            i = 0
            for _ in range(copies):
                for pr in pairs:
                    f.write(b"@p%d/%d\n" % (i, w + 1) + pr[w] + b"\n+\n" + b"I" * len(pr[w]) + b"\n")
                    i += 1
    return paths


def prepare(tmp, smalt):
    """reference, index (k 13, s 6) and the 1800-pair and 100-pair inputs under `tmp` -> (index prefix, pairs)"""
    import subprocess
    seqs, pairs = make()
    fa = os.path.join(tmp, "ref.fa")
    write_fasta(fa, seqs)
    pre = os.path.join(tmp, "idx")
    subprocess.run([smalt, "index", "-k", "13", "-s", "6", pre, fa], check=True, capture_output=True)
    return pre, pairs

"""Seeded inputs of the stand-alone tests of the seeding stage (test_seed_ref.py, test_seed_paths.py, test_gpu_seed.py): one small
reference with repeat families, a high-copy element, a run of N and low-complexity runs; reads whose lengths and contents decide
which branch of stage_seed runs (tests/seed_ref.py: classify); parameter sets; the stretches of split-read calls; the mixed batch
of the scratch tests; the two reads at the limit of the packed sort element.  Everything is a pure function of its arguments."""
import functools
import os

import numpy as np

import oracle_lib as ol
import seed_ref as sr
from smalt_amd import synth

# (k, s): steps on both sides of the limit of the per-frame rank lists (s <= 16), perfect (k <= 13 here) and hashed indexes
# (the reference is small: only k = 9, s = 1 gives a perfect index)
SWEEP = [(20, 1), (20, 13), (20, 16), (20, 17), (20, 19), (20, 20), (17, 17), (13, 1), (13, 6), (13, 13), (9, 6), (9, 1)]
MAXLEN = 600                       # longest read of the sweep: the mappers of the tests take reads up to here
CHRLEN, ELEMENT_COPIES = 60000, 150
ARRAY_UNIT, ARRAY_COPIES = 23, 7800      # a tandem array: every word of it has ARRAY_COPIES / s positions, so 16384 hits are about two seeds per sampling frame


@functools.lru_cache(maxsize=None)
def reference():
    """-> (sequences, element), ASCII, 299 kb in all: two sequences of 60 kb with repeat families (synth.make_reference),
    150 copies of a 120-base element, a run of N, runs of A, C and AC; a third of 7800 copies of a 23-base unit in tandem, a few
    of its bases changed.  With that many positions per word the seed budget (HASH_MAXNHITS) ends after about two seeds per
    sampling frame at every step s, so the cover loops decide the rank."""
    rng = np.random.default_rng(811)
    chroms = synth.make_reference(2, CHRLEN, seed=812, repeat_frac=0.2, n_fam=4, cons_len=300, divergence=0.05)
    elem = rng.integers(0, 4, size=120, dtype=np.uint8)
    for _ in range(ELEMENT_COPIES):
        c = chroms[int(rng.integers(0, 2))]
        at = int(rng.integers(0, c.size - elem.size))
        e = elem.copy()
        m = rng.random(e.size) < 0.01
        e[m] = (e[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
        c[at:at + e.size] = e
    seqs = [bytearray(synth.codes_to_ascii(c)) for c in chroms]
    seqs[1][5000:5300] = b"N" * 300
    seqs[1][20000:20200] = b"A" * 200
    seqs[1][30000:30100] = b"C" * 100
    seqs[1][40000:40200] = b"AC" * 100
    unit = rng.integers(0, 4, size=ARRAY_UNIT, dtype=np.uint8)
    arr = np.tile(unit, ARRAY_COPIES)
    m = rng.random(arr.size) < 0.002
    arr[m] = (arr[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
    seqs.append(synth.codes_to_ascii(arr))
    return [bytes(s) for s in seqs], synth.codes_to_ascii(elem)


def _mutate(rng, read: bytes, rate=0.01):
    a = np.frombuffer(read, dtype=np.uint8).copy()
    for i in np.flatnonzero(rng.random(a.size) < rate):
        a[i] = b"ACGT"[int(rng.integers(0, 4))]
    return a.tobytes()


def _rc(read: bytes):
    return read[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def lengths(k, s):
    ls = [k - 1, k, k + 1, k + s - 1, k + s] + list(range(63, 67)) + list(range(127, 131)) + [n + k - 1 for n in range(63, 67)] + \
         [n + k - 1 for n in range(127, 131)] + [255, 256, 257, 600]
    return sorted(set(ls))


@functools.lru_cache(maxsize=None)
def sweep_reads(k, s):
    """-> (reads, quals) as tuples of bytes; at most about 300 reads.  Qualities are 'I' except where a read is dressed with a
    low quality ('#', phred 2): those only count with min_basq > 2."""
    rng = np.random.default_rng(1000 * k + s)
    seqs, elem = reference()
    reads, quals = [], []

    def add(r, q=None):
        reads.append(bytes(r))
        quals.append(bytes(q) if q is not None else b"I" * len(r))

    def locus(n, sq=None):                 # (sequence 2 is the tandem array)
        sq = int(rng.integers(0, 2)) if sq is None else sq
        at = int(rng.integers(0, len(seqs[sq]) - n))
        return seqs[sq][at:at + n]

    def tandem(n):                  # copies of the high-copy element, one after the other, from a random phase
        ph = int(rng.integers(0, len(elem)))
        return (elem * (n // len(elem) + 2))[ph:ph + n]

    for n in lengths(k, s):
        add(_mutate(rng, locus(n)))
        add(_rc(_mutate(rng, locus(n))))
        add(_mutate(rng, tandem(n)))
        add(_rc(_mutate(rng, tandem(n), 0.03)))
        add(bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8)))                    # no hit, or a chance hit
        if n >= 127:                                                                       # half element, half unique: the budget decides
            add(tandem(n // 2) + locus(n - n // 2))
        if n >= k + s:                                                                     # from the tandem array: the budget ends early, the cover loops decide
            add(locus(n, 2)); add(_mutate(rng, locus(n, 2), 0.02)); add(_rc(_mutate(rng, locus(n, 2), 0.04)))
            add(locus(n // 3, 2) + locus(n - n // 3))
    for i in range(8):              # 256 bases whose last word lies on a sampled position of the reference: the top of the 256-bit cover mask
        at = 1000 + 7307 * i
        at += (-(at + 256 - k)) % s
        add(seqs[0][at:at + 256])
    for n in (100, 151):
        base = locus(n)
        add(b"N" + base[1:]); add(base[:-1] + b"N"); add(b"N" + base[1:-1] + b"N")
        add(base.lower()); add(base.replace(b"T", b"U")); add(base.lower().replace(b"t", b"u"))
        iu = bytearray(base)
        for i, c in zip(rng.choice(n, size=13, replace=False), b"RYKMSWBDHV.-*"):
            iu[int(i)] = c
        add(iu)
        for pos in (0, 1, k - 2, k - 1, k, n - k - 1, n - k, n - k + 1, n - 2, n - 1):       # low quality at and beside the ends of the first and the last word
            q = bytearray(b"I" * n)
            q[pos] = ord("#")
            add(base, q)
        add(seqs[1][5000 - n // 2:5000 - n // 2 + n])                                      # into the run of N
        add(seqs[1][5300 - n // 3:5300 - n // 3 + n])                                      # out of it
    for unit in (b"A", b"C", b"G", b"T", b"AC", b"AT", b"CG", b"ACG"):
        for n in (100, 256):
            add((unit * n)[:n])
    add(seqs[1][19950:20110]); add(seqs[1][39940:40100]); add(_rc(seqs[1][19950:20110]))
    for p in (1, 2, 3, 4, 5):          # a period-p repeat from base b on: the repeat filter looks back over the boundary of the first 64-lane chunk
        for b in (60, 61, 62, 63):
            while True:
                unit = bytes(rng.choice(list(b"ACGT"), size=p).astype(np.uint8))
                if all(unit != unit[:d] * (p // d) for d in range(1, p) if p % d == 0):
                    break
            add(locus(b) + (unit * 200)[:150 - b])
    return tuple(reads), tuple(quals)


# name -> (Par, the library's totals_only)
def param_sets():
    P = sr.Par
    return {"default": (P(), False), "x": (P(noshort=True), False), "H1": (P(ncut=1), False), "H50": (P(ncut=50), False), "q10": (P(min_basq=10), False),
            "x-q10": (P(min_basq=10, noshort=True), False), "x-H1": (P(ncut=1, noshort=True), False), "totals": (P(), True), "totals-H50": (P(ncut=50), True),
            "totals-q10": (P(min_basq=10), True)}


def stretches(reads, k):
    """(first, last) per read for a split read's second call (-x): in turn a stretch of k - 1 bases (falls back to the whole
    read), of k bases, one that runs beyond the read, one with first > last, one that ends at the last base, (0, 0)"""
    out = []
    for i, r in enumerate(reads):
        n, q0 = len(r), (7 * i) % max(1, len(r) - k)
        out.append([(q0, q0 + k - 2), (q0, q0 + k - 1), (q0, n + 5), (n // 2 + 9, n // 2), (max(0, n - k - 3 - i % 40), n - 1), (0, 0),
                    (q0, min(n - 1, q0 + 3 * k))][i % 7])
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch(k):
    """600-base reads between reads of k .. 40 bases and reads without a hit: what a persistent workgroup meets one after the other"""
    rng = np.random.default_rng(77 + k)
    seqs, elem = reference()
    reads = []
    for i in range(20):
        at = int(rng.integers(0, CHRLEN - 1000))
        reads.append(_mutate(rng, seqs[(i & 1) + (i % 5 == 0)][at:at + 600]) if i % 3 else (elem * 6)[i:i + 600])
        n = int(rng.integers(k, 41)) if k < 40 else k
        at = int(rng.integers(0, CHRLEN - 1000))
        reads.append(seqs[1 - (i & 1)][at:at + n])
        reads.append(bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(k, 200))).astype(np.uint8)))
        if i % 4 == 0:
            reads.append(b"N" * 30)
            reads.append(seqs[0][at:at + k - 1])
    return tuple(reads), tuple(b"I" * len(r) for r in reads)


PACKED_K, PACKED_S, PACKED_NCUT = 11, 1, 1 << 21


@functools.lru_cache(maxsize=None)
def packed_limit():
    """-> (sequences, reads): a run of A of 2^20 + k - 2 bases (its word has 2^20 - 1 positions: the largest hit count the packed
    sort element (nhits << 12 | i) holds) and a run of C of 2^20 + k - 1 bases (2^20 positions: one too many), unique sequence
    around them.  Read 0 runs from unique sequence into the A run (20 A) and on in unique sequence; read 1 the same at the C run."""
    rng = np.random.default_rng(4242)
    k = PACKED_K
    u = [bytes(rng.choice(list(b"ACGT"), size=2000).astype(np.uint8)) for _ in range(3)]
    u = [x.replace(b"AAAA", b"AGTA").replace(b"CCCC", b"CTGC") for x in u]
    a_run, c_run = b"A" * ((1 << 20) + k - 2), b"C" * ((1 << 20) + k - 1)
    seq = u[0][:-1] + b"G" + a_run + b"G" + u[1][1:-1] + b"T" + c_run + b"T" + u[2][1:]
    reads = [u[0][-40:-1] + b"G" + b"A" * 20 + u[1][300:340], u[1][-40:-1] + b"T" + b"C" * 20 + u[2][300:340]]
    return (seq,), tuple(reads)


def build_index(seqs, k, s, tmpdir, name):
    """oracle index written to files and read back (as the library loads it) -> (POINTER(OrIndex), prefix)"""
    oix = ol.build_index(list(seqs), ["s%d" % i for i in range(len(seqs))], k, s)
    prefix = os.path.join(str(tmpdir), name)
    assert ol.lib().or_index_write(oix, prefix.encode()) == 0
    ol.lib().or_index_free(oix)
    oix2 = ol.lib().or_index_read(prefix.encode())
    assert oix2
    return oix2, prefix


def write_fastq(path, reads, quals):
    with open(path, "wb") as f:
        for i, (r, q) in enumerate(zip(reads, quals)):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, q))

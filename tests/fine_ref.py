"""Plain restatement of the on-the-fly index of rmapPair's rescue round (kernel k_fine_index, smalt_amd/csrc/smg_kernels.hip;
setupFineHashTable, rmap.c:495-517): a perfect index with k = 5, s = 1 over the windows of ONE read's search intervals.  numpy
only, from the ASCII reference; it shares no code with the library or the oracle.  Also the seeded reference and the cases that
tests/test_fine_ref.py (against the oracle, no GPU) and tests/test_gpu_fine_index.py (the kernel) both run."""
import numpy as np

FINE_K, FINE_NKEYS = 5, 1 << 10
_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i                                   # lower case


def fine_index(seqs, sop, intervals):
    """seqs: ASCII bytes per sequence; sop[i]: offset of sequence i in the concatenated reference; intervals: (sx, lo, hi) of one
    read, 0-based and inclusive.  -> (idx [1025], pos [idx[1024]], cap): every 5-mer of every window that touches no letter
    outside ACGT, key = its 2-bit word, position = sop[sx] + lo + j; idx = exclusive prefix of the key counts, every key's
    positions ascending; cap = words of the windows whatever their letters (the size of the read's slice)."""
    keys, poss, cap = [], [], 0
    for sx, lo, hi in intervals:
        n = hi - lo + 1
        if n < FINE_K:
            continue
        nk = n - FINE_K + 1
        cap += nk
        c = _CODE[np.frombuffer(seqs[sx], dtype=np.uint8)[lo:hi + 1]].astype(np.int64)
        word = np.zeros(nk, dtype=np.int64)
        bad = np.zeros(nk, dtype=bool)
        for t in range(FINE_K):
            word = (word << 2) | (c[t:t + nk] & 3)
            bad |= c[t:t + nk] == 255
        keys.append(word[~bad])
        poss.append((int(sop[sx]) + lo + np.arange(nk, dtype=np.int64))[~bad])
    keys = np.concatenate(keys) if keys else np.zeros(0, dtype=np.int64)
    poss = np.concatenate(poss) if poss else np.zeros(0, dtype=np.int64)
    order = np.lexsort((poss, keys))
    idx = np.zeros(FINE_NKEYS + 1, dtype=np.uint32)
    idx[1:] = np.cumsum(np.bincount(keys, minlength=FINE_NKEYS))
    return idx, poss[order].astype(np.uint32), cap


# ---- the reference and the cases --------------------------------------------------------------------------------------------
SEQ_LENS = (60_001, 50_002, 30_002, 20_001)               # 160 kb; the offsets of sequences 1 .. 3 are no multiples of 4 (asserted by the tests)
POLYA = (0, 20_000, 3000)                                 # (sequence, start, length) of the poly-A stretch
DINUC = (1, 10_000, 3000)                                 # ... of the AC repeat
NRUN = (2, 5000, 40)                                      # ... of a run of N
IUPAC = ((2, 7000, b"R"), (2, 7003, b"y"), (2, 7010, b"K"), (2, 7011, b"M"), (2, 7030, b"n"), (2, 7050, b"X"))


def workload(seed=20261):
    """-> sequences as ASCII bytes: random ACGT (some stretches in lower case) with the stretches above written in."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SEQ_LENS:
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
        out.append(a)
    out[0][POLYA[1]:POLYA[1] + POLYA[2]] = ord("A")
    out[1][DINUC[1]:DINUC[1] + DINUC[2]] = np.tile(np.frombuffer(b"AC", dtype=np.uint8), DINUC[2] // 2)
    out[2][NRUN[1]:NRUN[1] + NRUN[2]] = ord("N")
    for sx, at, letter in IUPAC:
        out[sx][at] = letter[0]
    out[3][100:400] |= 32                                 # lower case: standard bases all the same
    out[3][0] = ord("N")                                  # the first ...
    out[3][-1] = ord("N")                                 # ... and the last base of the last sequence
    return [a.tobytes() for a in out]


def _iv(sx, lo, n):
    return (sx, lo, lo + n - 1)


def cases():
    """-> dict name -> (per read a list of (sx, lo, hi), grid).  Sum of window lengths per call below 300 k."""
    L = SEQ_LENS
    c = {}
    # interval lengths: no word (1-4), one and two words, and around the stride of 64 lanes; then a read with no interval
    c["lengths"] = ([[_iv(1, 2000 + 300 * i, n)] for i, n in enumerate((1, 2, 3, 4, 5, 6, 63 + 4, 64 + 4, 65 + 4, 128 + 4, 129 + 4))] + [[]], 0)
    # first and last base of every sequence (of the whole reference: sequences 0 and 3), windows of 5 .. 40 bases
    c["edges"] = ([[_iv(sx, 0, 40)] for sx in range(4)] + [[_iv(sx, L[sx] - 40, 40)] for sx in range(4)]
                  + [[_iv(0, 0, 5)], [_iv(3, L[3] - 5, 5)], [_iv(3, 0, 4), _iv(3, L[3] - 4, 4)]], 0)
    # every sequence, lo in every residue mod 16
    c["residues"] = ([[_iv(sx, 1000 + 64 * r + r, 37)] for sx in range(4) for r in range(16)], 0)
    # non-standard letters inside, at the start and at the end of a window
    s, a, n = NRUN
    c["letters"] = ([[_iv(s, a - 30, 100)], [_iv(s, a, 60)], [_iv(s, a - 60, 60 + n)], [_iv(s, a + 1, n - 2)], [_iv(s, a - 4, 8)],
                     [_iv(2, 6990, 80)], [_iv(2, 7000, 5)], [_iv(2, 7046, 5)], [_iv(2, 7050, 30)], [_iv(3, 0, 30)], [_iv(3, L[3] - 30, 30)],
                     [_iv(s, a - 30, 100), _iv(2, 6990, 80)]], 0)
    # abutting intervals (no word across the seam), one of them shorter than a word; the same interval twice
    c["abutting"] = ([[_iv(0, 1000, 100), _iv(0, 1100, 100)], [_iv(0, 3000, 64), _iv(0, 3064, 3), _iv(0, 3067, 70)], [_iv(3, 100, 150), _iv(3, 250, 150)]], 0)
    c["twice"] = ([[_iv(0, 5000, 200), _iv(0, 5000, 200)], [_iv(0, POLYA[1] + 100, 600), _iv(0, POLYA[1] + 100, 600)],
                   [_iv(1, 300, 7), _iv(1, 300, 7), _iv(1, 300, 7)]], 0)
    # 2048 intervals for one read: 40 bases every 45, over all sequences
    many = [_iv(sx, lo, 40) for sx in range(4) for lo in range(10, L[sx] - 40, 45)][:2048]
    assert len(many) == 2048
    c["many"] = ([many, many[:3]], 0)
    # one or two keys own everything: the insertion sort runs on a long list
    c["polya"] = ([[_iv(*POLYA)], [_iv(POLYA[0], POLYA[1] - 50, POLYA[2] + 100)]], 0)
    c["dinuc"] = ([[_iv(*DINUC)], [_iv(DINUC[0], DINUC[1] + 1, DINUC[2] - 1)]], 0)
    # 10 mixed reads on 3 workgroups: the counters in LDS are used again by the next read of a workgroup
    mixed = [[_iv(0, POLYA[1], 500)], [], [_iv(1, 100, 3)], many[:300], [_iv(2, NRUN[1] - 10, 60)], [_iv(0, 7, 133), _iv(3, 9, 69)],
             [_iv(1, DINUC[1], 400)], [_iv(2, 0, 5)], many[1000:1100], [_iv(3, L[3] - 68, 68)]]
    c["mixed_grid3"] = (mixed, 3)
    for name, (reads, _) in c.items():
        assert sum(hi - lo + 1 for r in reads for _, lo, hi in r) < 300_000, name
    return c

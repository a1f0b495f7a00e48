"""Plain restatement of what the reference's index construction does with the sampling grid (hashTableSetUp, hashidx.c:829-998):
which serials it indexes, which index type it picks, and -- for a sampling step larger than the word length -- when it refuses a
reference and what it writes as `maxpos`.  Test infrastructure only; tests/test_index_ref.py holds every function here against the
reference program itself."""
import struct

IDX_PERFECT, IDX_HASH32MIX = 0, 1
ACGT = frozenset(b"ACGTUacgtu")


def _cdiv(a, b):
    """C's integer division: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def carry(lens, k, s):
    """The walk of doWordsInSeq (hashidx.c:465-531) over the sequence lengths: the offset of the first sampled word of the next
    sequence and the serial counter, both as the reference computes them -- the offset in an `unsigned char`, with the range check of
    hashidx.c:494 in front of every sequence.  -> (index of the sequence the reference refuses | None, maxpos | None).
    For s <= k the offset is always below s and maxpos is ceil(tot / s) - 1; for s > k neither holds."""
    offs, ctr = 0, 0
    for i, n in enumerate(lens):
        if offs >= s:
            return i, None
        c = (k + offs) & 255
        if n >= c:                              # the first word ends after c bases, every further one s bases later
            r = n - c
            ctr += 1 + r // s
            c = s - r % s
        else:
            c -= n
        d = k - c
        offs = (d - s * _cdiv(d, s)) & 255      # C's remainder (the sign of d), stored in an unsigned char
        if offs:
            offs = (s - offs) & 255
        ctr += _cdiv(k - c + offs, s)
    ctr &= 0xFFFFFFFF
    return None, (ctr - 1 if ctr else 0)


def grid_maxpos(lens, s):
    tot = sum(lens)
    return (tot + s - 1) // s - 1 if tot else 0


def geometry(k, s, tot):
    """selectHashTyp (smalt.c:268-332) -> (typ, nbits_key, nbits_lo); a perfect index has nbits_key = 2k"""
    nbk = 2 * k
    ntup = tot // s
    if nbk > 63 or ntup > 0xFFFFFFFF:
        raise ValueError("no index type for k=%d s=%d" % (k, s))
    if (1 << nbk) <= 2 * ntup:
        return IDX_PERFECT, nbk, 0
    last_b = ntup & 1
    t = ntup
    for i in range(32):
        t >>= 1
        if t & 1:
            last_b = i
    nk = last_b + 1 if last_b & 1 else last_b
    np_ = 0
    if nbk > 32:
        np_ = nbk - 32
        if np_ > 10:
            raise ValueError("no index type for k=%d s=%d" % (k, s))
    if nk + np_ > 26:
        nk = 26 - np_
    if nk < np_ + 1:
        nk = np_ + 1
    if nk > 26:
        nk = 26
    return IDX_HASH32MIX, nk, np_


def path(k, s, tot):
    """which of the device builder's two paths a reference takes: "k32" (perfect index, 32-bit sort keys with a sentinel) or "hash"
    (hashed index, compaction and 64-bit sort keys).  A perfect index with k = 16 has no path: the builder refuses it."""
    typ, nbits_key, _ = geometry(k, s, tot)
    if typ == IDX_PERFECT:
        if nbits_key > 30:
            raise ValueError("perfect index with k=%d: refused by the builder" % k)
        return "k32"
    return "hash"


def grid_positions(seqs, k, s):
    """Serials of the global sampling grid that are indexed: serial t covers the bases [t*s, t*s + k) of the concatenated sequences;
    it counts if it lies inside one sequence and holds only A, C, G, T (U) in either case.  Ascending."""
    out = []
    base = 0
    for q in seqs:
        end = base + len(q)
        bad = [0] * (len(q) + 1)                 # bad[i]: letters that are not ACGT among q[:i]
        for i, ch in enumerate(q):
            bad[i + 1] = bad[i] + (0 if ch in ACGT else 1)
        t = (base + s - 1) // s
        while t * s + k <= end:
            a = t * s - base
            if bad[a + k] == bad[a]:
                out.append(t)
            t += 1
        base = end
    return out


def read_smi(fn):
    """header fields and the position words of a `.smi` file (hashidx.c:1214-1255)"""
    raw = open(fn, "rb").read()
    h = struct.unpack_from("<8I", raw, 12 * 4)
    d = dict(k=h[0], s=h[1], npos=h[2], maxpos=h[3], typ=h[4], nbits_key=h[5], nbits_lo=h[6], nwords=h[7])
    o = (12 + 8 + (1 << d["nbits_key"]) + 1) * 4
    d["pos"] = list(struct.unpack_from("<%dI" % d["npos"], raw, o))
    return d


TINY_SEED = 20                # tests/test_index_ref.py asserts that this sample holds enough of every class


def tiny_cases(seed=TINY_SEED, n=200):
    """n seeded tiny references: (k, s, [sequences]) with 3 <= k <= 20, 1 <= s <= 127; every second one has k < s <= k + 12; 1 - 7
    sequences of k .. k + 3s + 10 letters, mostly ACGT with some N, lower case and IUPAC letters."""
    import numpy as np
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT" * 12 + b"acgtNnRYu", dtype=np.uint8)
    out = []
    for j in range(n):
        k = int(rng.integers(3, 21))
        s = int(rng.integers(k + 1, k + 13)) if j % 2 == 0 else int(rng.integers(1, 128))
        seqs = [letters[rng.integers(0, len(letters), int(rng.integers(k, k + 3 * s + 11)))].tobytes()
                for _ in range(int(rng.integers(1, 8)))]
        out.append((k, s, seqs))
    return out


def classify(lens, k, s):
    """"refused", "over" (built, maxpos one above the grid's), "grid" (built with s > k, the grid's maxpos) or "plain" (s <= k)"""
    bad, maxpos = carry(lens, k, s)
    if bad is not None:
        return "refused"
    if s <= k:
        return "plain"
    return "over" if maxpos == grid_maxpos(lens, s) + 1 else "grid"

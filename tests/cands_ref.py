"""Plain restatement of how the candidate stage walks a strand's sorted run when S3 ran ahead of it (stage_cands_v2<false, true>
in smalt_amd/csrc/smg_cands.hpp): chunks of the LDS working set that end at a hit-region boundary, the unfinished region
carried into the next chunk, and the fall back to the HBM working set.  numpy only; it shares no code with the library.  The
walk CHOOSES and COUNTS inputs (which strands take which path); what the stage computes is always compared with the oracle.
Also the seeded tandem-repeat workload whose strands take the fall back.  `file:line` citations: SMALT 0.7.6, src/."""
import collections

import numpy as np

KEY_QBITS, KEY_DIAGBITS = 20, 33                         # key = seq(10) | diagonal(33) | read offset(20)
HALFBIT = 31                                             # hashhit.h:68
SEGMENTING_DIFFSHIFT = 3                                 # segment.c:426
ONE_CHUNK, CHUNKS, FALLBACK_NO_BREAK, FALLBACK_CARRY = "one-chunk", "chunks", "fallback-no-break", "fallback-carry"

Walk = collections.namedtuple("Walk", "path chunks carry largest_region")
Walk.__doc__ = """path: ONE_CHUNK, CHUNKS (several), FALLBACK_NO_BREAK (a chunk with keys behind it holds no region break) or
FALLBACK_CARRY (the carried tail leaves fewer than 64 free keys); chunks: chunks completed (before the fall back, if any);
carry: the largest tail carried from one chunk into the next; largest_region: keys of the strand's largest hit region -- a
region above W can never be streamed, so it bounds the fall backs from below whatever the chunks are."""


def region_breaks(keys, k, s, qlen):
    """Indices i >= 1 at which a hit region starts: the sequence group of keys[i - 1] and keys[i] differs, or (diagonal << 31 |
    read offset) grows by at least min(k * 3 // s, (qlen - k) // s + 1) << 31 (defineHitRegions, segment.c:426-444)."""
    keys = np.asarray(keys, dtype=np.uint64)
    if keys.size < 2:
        return np.zeros(0, dtype=np.int64)
    max_dshift = min((k * SEGMENTING_DIFFSHIFT // s) & 0xffff, (qlen - k) // s + 1)
    grp = (keys >> np.uint64(KEY_QBITS + KEY_DIAGBITS)).astype(np.int64)
    diag = ((keys >> np.uint64(KEY_QBITS)) & np.uint64((1 << KEY_DIAGBITS) - 1)).astype(np.int64)
    q = (keys & np.uint64((1 << KEY_QBITS) - 1)).astype(np.int64)
    # (diag_b << 31 | q_b) - (diag_a << 31 | q_a) >= max_dshift << 31 in exact integers: q < 2^20 fits below bit 31
    ddiag, dq = diag[1:] - diag[:-1], q[1:] - q[:-1]
    far = (ddiag > max_dshift) | ((ddiag == max_dshift) & (dq >= 0))
    return np.flatnonzero((grp[1:] != grp[:-1]) | far) + 1


def walk(keys, W, k, s, qlen):
    """keys: the strand's run in ascending order; W: keys of a chunk (the smaller of the LDS working set and the window)."""
    n = int(np.asarray(keys).size)
    assert W >= 128                                       # (below, the stage does not stream at all)
    brk = region_breaks(keys, k, s, qlen)
    edges = np.concatenate([[0], brk, [n]])
    largest = int(np.diff(edges).max()) if n else 0
    carry = done = chunks = maxcarry = 0
    while done < n:
        if carry + 64 > W:
            return Walk(FALLBACK_CARRY, chunks, maxcarry, largest)
        take = min(n - done, W - carry)
        lo = done - carry                                 # the chunk is keys[lo:done + take]
        done += take
        if done < n:                                      # more keys follow: the chunk ends at its last region break
            j = int(np.searchsorted(brk, done, side="left")) - 1          # the last break below `done` ...
            if j < 0 or brk[j] <= lo:                                     # ... that lies inside the chunk, not at its start
                return Walk(FALLBACK_NO_BREAK, chunks, maxcarry, largest)
            carry = done - int(brk[j])
            maxcarry = max(maxcarry, carry)
        else:
            carry = 0
        chunks += 1
    return Walk(ONE_CHUNK if chunks <= 1 else CHUNKS, chunks, maxcarry, largest)


def is_fallback(w):
    return w.path in (FALLBACK_NO_BREAK, FALLBACK_CARRY)


def walk_batch(got, W, k, s, read_lens):
    """Walk per strand of a batch (the dict of Mapper.hits_batch or of the host emulation's dump), None for a strand the stage
    before left alone (HITRUN_NONE)."""
    out = []
    for rs in range(2 * len(read_lens)):
        if int(got["run_mode"][rs]) != 1:                 # HITRUN_SORTED
            out.append(None)
            continue
        off, n = int(got["run_off"][rs]), int(got["run_n"][rs])
        out.append(walk(got["pool"][off:off + n], W, k, s, int(read_lens[rs >> 1])))
    return out


def summary(walks):
    """Counts that the cases assert their conditions on."""
    live = [w for w in walks if w is not None]
    fb = [w for w in live if is_fallback(w)]
    return dict(none=sum(1 for w in walks if w is None), one_chunk=sum(1 for w in live if w.path == ONE_CHUNK and w.chunks == 1),
                chunks=sum(1 for w in live if w.path == CHUNKS), fallbacks=len(fb), no_break_first=sum(1 for w in fb if w.path == FALLBACK_NO_BREAK and w.chunks == 0),
                after_chunk=sum(1 for w in fb if w.chunks >= 1), by_carry=sum(1 for w in fb if w.path == FALLBACK_CARRY),
                max_chunks=max([w.chunks for w in live] or [0]), max_carry=max([w.carry for w in live] or [0]))


# ---- the tandem workload ---------------------------------------------------------------------------------------------------
TANDEM_STRETCHES = (300, 600, 900, 1200, 2400, 6000)
TANDEM_UNITS = (12, 12, 7)                               # unit length per sequence
TANDEM_DIVERGENCE = (0.01, 0.01, 0.0)                    # substitutions in the stretches per sequence
TANDEM_SPACER = 20_000
ALPHABET = np.frombuffer(b"ACGT", dtype=np.uint8)


def _ascii(codes):
    return ALPHABET[codes].tobytes()


def _mutate(rng, codes, rate):
    mut = rng.random(codes.size) < rate
    return np.where(mut, (codes + rng.integers(1, 4, size=codes.size)) & 3, codes).astype(np.uint8)


def tandem_workload(read_len=100, min_stretch=0, seed=4711):
    """-> (sequences, reads) as ASCII bytes.  Three sequences of random 20 kbp spacers around tandem stretches of 300 .. 6000 bases
    (units of 12, 12 and 7 bases, one unit per stretch; the third sequence exact, the others with 1 % substitutions).  Per stretch of at least
    max(min_stretch, read_len) bases three reads of read_len bases cut from it with 0, 2 and 4 % substitutions, the third
    reverse-complemented; then 20 reads from anywhere.  Hit regions of such reads span the stretch: 300 to 16 000 keys."""
    rng = np.random.default_rng(seed)
    seqs, stretches = [], []
    for unit_len, div in zip(TANDEM_UNITS, TANDEM_DIVERGENCE):
        parts = [rng.integers(0, 4, size=TANDEM_SPACER, dtype=np.uint8)]
        for ln in TANDEM_STRETCHES:
            unit = rng.integers(0, 4, size=unit_len, dtype=np.uint8)      # a unit of its own per stretch: a read hits one stretch
            t = np.tile(unit, ln // unit_len + 1)[:ln]
            if div:
                t = _mutate(rng, t, div)
            stretches.append(t)
            parts += [t, rng.integers(0, 4, size=TANDEM_SPACER, dtype=np.uint8)]
        seqs.append(np.concatenate(parts))
    reads = []
    for t in stretches:
        if t.size < max(min_stretch, read_len):
            continue
        for j, rate in enumerate((0.0, 0.02, 0.04)):
            o = int(rng.integers(0, t.size - read_len + 1))
            r = _mutate(rng, t[o:o + read_len], rate) if rate else t[o:o + read_len].copy()
            reads.append((3 - r[::-1]).astype(np.uint8) if j == 2 else r)
    for _ in range(20):
        c = seqs[int(rng.integers(0, len(seqs)))]
        o = int(rng.integers(0, c.size - read_len + 1))
        reads.append(c[o:o + read_len].copy())
    return [_ascii(c) for c in seqs], [_ascii(r) for r in reads]

"""Plain restatement of what S3 on its own (kernel k_hits, stage_hits in smalt_amd/csrc/smg_cands.hpp) promises for one read
strand: which seeds contribute, the 64-bit key of every hit, the run in ascending order.  numpy and Python integers only; it
shares no code with the library.  Inputs are the strand's hit info and seed table (an INPUT here: the seeding stage is pinned
by the reference dumps), the index arrays on the host and the parameters.  `file:line` citations: SMALT 0.7.6, src/."""
import math

import numpy as np

HITRUN_NONE, HITRUN_SORTED, HITRUN_OVERFLOW = 0, 1, 2
FLG_SEQBYSEQ = 0x10
HQ_MULTIHIT = 2                                          # hashhit.h:57-65
MINHIT_PER_TUPLE = 16                                    # hashhit.c:43
HITLST_MINSIZ, HITLST_BLKSZ, HITLST_LOGQLEN_FACT = 8192, 16384, 32   # hashhit.c:45-48
KEY_QBITS, KEY_DIAGBITS = 20, 33                         # key = seq(10) | diagonal(33) | read offset(20)


class HostIndex:
    """The index arrays of an oracle index (ctypes POINTER(OrIndex)) as numpy copies."""

    def __init__(self, oix):
        o = oix.contents
        self.k, self.s, self.typ, self.nseq = int(o.k), int(o.s), int(o.typ), int(o.nseq)
        self.pos = np.ctypeslib.as_array(o.pos, shape=(max(1, o.npos),))[:o.npos].copy()
        if self.typ == 0:                                # perfect index: one list per key
            self.first = np.ctypeslib.as_array(o.idx, shape=(o.nkeys + 1,)).copy()
        else:                                            # hashed index: one list per word
            self.first = np.ctypeslib.as_array(o.posidx, shape=(o.nwords + 1,)).copy()
        sop = np.ctypeslib.as_array(o.sop, shape=(self.nseq + 1,)).copy()
        self.seqlo = (sop // np.uint64(self.s)).astype(np.int64)      # k-mer serial where sequence i starts

    def positions(self, posidx):
        return self.pos[int(self.first[posidx]):int(self.first[posidx + 1])]


def hitlist_caps(qlen):
    """(nhits_alloc, nhits_max) of the reference's hit list for a read of qlen bases on its own (initHitList, hashhit.c:1262-1288)"""
    target = int(qlen * math.log(qlen) * HITLST_LOGQLEN_FACT)
    target = min(target, 0x7fffffff)
    if target < HITLST_MINSIZ:
        target = HITLST_MINSIZ
    alloc = HITLST_BLKSZ
    if target > alloc:
        alloc = ((target + HITLST_BLKSZ - 1) // HITLST_BLKSZ) * HITLST_BLKSZ
    return alloc, target


def min_cover_of(par, qlen):
    frac = float(getattr(par, "min_cover_frac", 0.0))
    if frac > 0.0:
        return min(int(frac * qlen), qlen)
    return int(par.min_cover)


class Expect:
    """mode: HITRUN_NONE or HITRUN_SORTED; keys: the run (sorted uint64); multihit: read offsets whose qualifier becomes
    HQ_MULTIHIT (seq-by-seq mode); eligible: all conditions on the strand held (mode NONE then means seq-by-seq over its
    allocation); ncutseeds: seeds below the rank with hits that the cut-off, the halving loop or the ceiling left out; halved,
    stopped: the halving loop ran / the walk stopped at the ceiling nhits_max (concatenated mode); nlist: position lists gathered."""
    __slots__ = ("mode", "keys", "multihit", "eligible", "over_alloc", "ncutseeds", "halved", "stopped", "nlist", "lists")


def window_counts(e, W):
    """Keys per window when the strand's run (total > W) is gathered in windows of ascending (sequence, diagonal): every list
    offers its next t = (W - lists) * rest // remaining + 1 keys, the window's bound is the least list element just past such a
    quota, and every list gives those of its t keys that lie below the bound.  Used to CHOOSE inputs (a window whose last or
    first window has a given number of keys); the kernel's output is compared with the sorted run as ever."""
    lists = [np.sort(l >> np.uint64(KEY_QBITS)).astype(np.int64) for l in e.lists]      # within a list the read offset is constant
    total = sum(l.size for l in lists)
    assert total > W > len(lists)
    room, cur, remaining, counts = W - len(lists), [0] * len(lists), total, []
    while remaining:
        quota = [(room * (l.size - c)) // remaining + 1 for l, c in zip(lists, cur)]
        over = [int(l[c + t]) for l, c, t in zip(lists, cur, quota) if t < l.size - c]
        bound = min(over) if over else None
        cnt = [min(t, l.size - c) if bound is None else int(np.searchsorted(l[c:c + t], bound, side="left")) for l, c, t in zip(lists, cur, quota)]
        assert 0 < sum(cnt) <= W
        cur = [c + n for c, n in zip(cur, cnt)]
        remaining -= sum(cnt)
        counts.append(sum(cnt))
    return counts


def expect_strand(hx, par, strand, qlen, n_seeds, seed_rank, seeds, window, tab):
    """seeds: array [>= n_seeds][3] of (posidx, nhits, qoffs) in table order; window, tab: geometry the kernel ran with."""
    k, s = hx.k, hx.s
    e = Expect()
    e.mode, e.keys, e.multihit, e.over_alloc, e.ncutseeds, e.halved, e.stopped, e.nlist, e.lists = HITRUN_NONE, np.zeros(0, np.uint64), [], False, 0, False, False, 0, []
    ncut = max(int(par.ktuple_maxhit), 0)
    seqbyseq = (int(par.rmapflg) & FLG_SEQBYSEQ) != 0
    n_use = int(seed_rank) if seed_rank > 0 else int(n_seeds)
    applicable = min_cover_of(par, qlen) < k + s or seqbyseq
    e.eligible = k <= qlen < 256 and applicable and n_use < tab and window > tab + 128
    if not e.eligible:
        return e
    nhits_alloc, nhits_max = hitlist_caps(qlen)
    tab_ = [(int(seeds[i][0]), int(seeds[i][1]), int(seeds[i][2])) for i in range(n_use)]
    if seqbyseq:
        tot = sum(nh for _, nh, _ in tab_ if not (ncut > 0 and nh > ncut))
        if tot > nhits_alloc:                            # allocation-boundary protocol (hashhit.c:1497): the candidate stage's business
            e.over_alloc = True
            return e
        take = [t for t in tab_ if not (ncut > 0 and t[1] > ncut)]
        e.multihit = [q for _, nh, q in tab_ if ncut > 0 and nh > ncut]
    else:                                                # hashCollectHitsUsingCutoff (hashhit.c:1593-1689)
        m = ncut
        while True:
            total, stop = 0, None
            for i, (_, nh, _) in enumerate(tab_):
                if nh < 1 or (m > 0 and nh > m):
                    continue
                if total + nh > nhits_max:
                    stop = i
                    break
                total += nh
            m_final = m
            m //= 2
            if not (stop is not None and m > MINHIT_PER_TUPLE):
                break
            e.halved = True
        e.stopped = stop is not None
        used = stop if stop is not None else n_use
        take = [t for t in tab_[:used] if t[1] >= 1 and not (m_final > 0 and t[1] > m_final)]
    parts = []
    for posidx, _, qoffs in take:
        pos = hx.positions(posidx).astype(np.int64)
        if pos.size == 0:
            continue
        e.nlist += 1
        if strand:
            diag = pos + qoffs // s
        else:
            diag = (pos | (1 << 32)) - qoffs // s
        key = (diag << KEY_QBITS) | qoffs
        if seqbyseq:
            seq = np.searchsorted(hx.seqlo[:hx.nseq], pos, side="right") - 1      # the last seqlo[i] <= pos
            key = key | (seq.astype(np.int64) << (KEY_DIAGBITS + KEY_QBITS))
        parts.append(key.astype(np.uint64))
    e.lists = parts
    e.ncutseeds = sum(1 for t in tab_ if t[1] >= 1) - sum(1 for t in take if t[1] >= 1)
    e.keys = np.sort(np.concatenate(parts)) if parts else np.zeros(0, np.uint64)
    e.mode = HITRUN_SORTED
    return e


def expect_batch(hx, par, read_lens, got, window=None, tab=None):
    """Expect per strand (rs = 2 * read + strand) from the hit info and seed tables in `got` (Mapper.hits_batch or the dump of the
    host emulation)."""
    window = got["window"] if window is None else window
    tab = got["tab"] if tab is None else tab
    return [expect_strand(hx, par, rs & 1, int(read_lens[rs >> 1]), int(got["n_seeds"][rs]), int(got["seed_rank"][rs]), got["seeds"][rs], window, tab)
            for rs in range(2 * len(read_lens))]


def check_batch(exp, got, seqbyseq, qmask_seed, read_lens, overflow=False):
    """The uniform assertions: mode, run length and keys per strand, runs disjoint and inside the pool, the pool cursor, the
    read-offset qualifiers.  qmask_seed: the qualifier rows as the seeding stage left them (from a run of the same reads and
    parameters in which S3 did not take place); the whole row of every strand, offsets 0 .. read length, must equal that row
    with HQ_MULTIHIT at the offsets of the seeds above the cut-off (seq-by-seq mode, strands the stage sorted) and nowhere
    else (qmask_seed None: the qualifiers are not looked at).  overflow: strands may come out HITRUN_OVERFLOW instead of HITRUN_SORTED (a pool smaller than the batch's keys;
    which strands is a matter of the order of the reservations)."""
    cap, pool = got["pool_cap"], got["pool"]
    reserved, spans, novf = 0, [], 0
    for rs, e in enumerate(exp):
        mode, off, n = int(got["run_mode"][rs]), int(got["run_off"][rs]), int(got["run_n"][rs])
        nrow = 0 if qmask_seed is None else min(int(read_lens[rs >> 1]) + 1, got["qmask"].shape[1], qmask_seed.shape[1])
        row = got["qmask"][rs][:0].copy() if qmask_seed is None else qmask_seed[rs][:nrow].copy()
        if seqbyseq and e.mode == HITRUN_SORTED and nrow:         # (an overflowed strand has marked its seeds before it asks for room)
            row[e.multihit] = HQ_MULTIHIT
        assert np.array_equal(got["qmask"][rs][:nrow], row), (rs, np.flatnonzero(got["qmask"][rs][:nrow] != row)[:8])
        if overflow and mode == HITRUN_OVERFLOW:
            assert e.mode == HITRUN_SORTED and n == e.keys.size and off + n > cap, rs
            novf += 1
            reserved += n
            continue
        assert mode == e.mode, (rs, mode, e.mode)
        if mode == HITRUN_SORTED:
            assert n == e.keys.size, (rs, n, e.keys.size)
            if n:
                assert off + n <= cap and off + n <= pool.size, rs
                assert np.array_equal(pool[off:off + n], e.keys), rs
                spans.append((off, off + n))
                reserved += n
        else:
            assert n == 0 and off == 0, rs
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], (a, b)
    assert got["hit_count"] == reserved
    return novf

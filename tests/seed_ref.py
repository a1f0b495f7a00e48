"""Reference of the seeding stage (kernels k_encode and k_seed; stage_seed in smalt_amd/csrc/smg_stages.hpp) for one read strand:
the oracle's restatement of collectHitInfo / hashCollectHitInfoShort (oracle/or_seed.c, reached through the flat entry
or_seed_flat), and in numpy what follows from its output: the hit numbers (hashhit.c:1200-1219), the hits below the cut-off
(hashhit.c:1171), the lookup count.  `classify` says which branches of the stage a strand takes -- it replays the budget and
cover loops (hashhit.c:769-891) in plain Python, which is also a second opinion on seed_rank -- and `listed_ranges` replays the
recursion of the reference's quicksort (sort.c:233) as the wave sort walks it.  Shares no code with the library.
`file:line` citations: SMALT 0.7.6, src/."""
import ctypes as C

import numpy as np

import oracle_lib as ol

HQ_TERM, HQ_NORMHIT, HQ_MULTIHIT, HQ_REPEAT, HQ_NOHIT, HQ_NONSTDNT = range(6)         # hashhit.h:57-65
HI_REVERSE, HI_SORTED, HI_RANK = 1, 2, 4                                              # hashhit.c:84-92
HASH_MAXNHITS = 16 * 1024                                                             # rmap.c:50
NREPEATS, MINSEEDNUM, MAXCOVER_PERCENT, MINCOVER_KMER = 4, 3, 80, 2                    # hashhit.c:42, 53-56
SEED_IDXBITS, SEED_LISTCAP, SORT_SMALL = 12, 32, 32                                   # the stage's instance of the wave sort
GUARD = 0xA5

# sequence.c:287-322: letters in either case; A C G T-or-U are 0..3, everything else is 5
CODE = np.full(256, 5, dtype=np.uint8)
for _c in range(256):
    _u = _c & 0xDF
    if _u in b"ACGTU":
        CODE[_c] = b"ACGTU".index(_u) if _u != ord("U") else 3


def encode(read: bytes):
    return CODE[np.frombuffer(read, dtype=np.uint8)]


def revcomp(codes):
    """sequence.c:884-896: codes >= 4 are kept"""
    r = codes[::-1]
    return np.where(r >= 4, r, 3 - r).astype(np.uint8)


class Par:
    """ncut: ktuple_maxhit; noshort: FLG_NOSHRTINFO (-x)"""

    def __init__(self, ncut=10000, min_basq=0, noshort=False):
        self.ncut, self.min_basq, self.noshort = ncut, min_basq, noshort

    def gpu(self, gix):
        p = gix.default_params()
        p.ktuple_maxhit, p.min_basqval = self.ncut, self.min_basq
        if self.noshort:
            p.rmapflg |= ol.FLG_NOSHRTINFO | ol.FLG_SENSITIVE
        return p


def _flat():
    f = ol.lib().or_seed_flat
    f.restype = C.c_int
    f.argtypes = [C.POINTER(ol.OrIndex), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return f


def word_range(k, qlen, rng):
    """[t_lo, t_hi) of word starts and whether the stretch fell back to the whole read (collectHitInfo, hashhit.c:536-551)"""
    if rng is None:
        return 0, qlen - k + 1, False
    q0, q1 = int(rng[0]), min(int(rng[1]), qlen - 1)
    if q0 <= q1 and q1 - q0 + 1 >= k:
        return q0, q1 - k + 2, False
    return 0, qlen - k + 1, True


class Strand:
    """What the reference defines for one strand.  hdr: n_seeds, seed_rank, status, qlen, nhit_rank, nhit_tot, nhit_cut;
    seeds [n_seeds][3] (posidx, nhits, qoffs) in rank order, None where the stage writes none; qmask [qlen + 1] or None."""
    __slots__ = ("hdr", "seeds", "qmask", "lookups", "short", "st", "qlen", "k", "s", "par", "rng", "totals_only", "codes", "qual")


def ref_strand(oix, codes, qual, st, par, rng=None, totals_only=False):
    """codes: the read's codes in forward orientation (both strands, as collectHitInfo takes them); qual: bytes/array or None"""
    k, s = int(oix.contents.k), int(oix.contents.s)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    qlen = codes.size
    e = Strand()
    e.st, e.qlen, e.k, e.s, e.par, e.rng, e.totals_only, e.codes = st, qlen, k, s, par, rng, totals_only, codes
    e.qual = None if qual is None else np.ascontiguousarray(np.frombuffer(bytes(qual), dtype=np.uint8))
    e.short = qlen < k
    if e.short:                                           # ERRCODE_SHORTSEQ, swallowed by rmapSingle (rmap.c:1736)
        e.hdr, e.seeds, e.qmask, e.lookups = np.array([0, 0, HI_REVERSE if st else 0, qlen, 0, 0, 0], dtype=np.uint32), None, None, 0
        return e
    assert rng is None or par.noshort, "a stretch of the read only occurs with -x (mapSecondary, rmap.c:1483)"
    hdr, seeds, qmask = np.zeros(4, np.uint32), np.zeros((qlen + 1, 3), np.uint32), np.zeros(qlen + 1, np.uint8)
    plain = par.noshort or totals_only                    # collectHitInfo alone
    ncut = 0 if par.noshort else max(par.ncut, 0)         # initRMAPINFO passes no cut-off (rmap.c:1027-1044)
    q0, q1 = (0, 0) if rng is None else (int(rng[0]), int(rng[1]))
    rv = _flat()(oix, st, int(plain), ncut, HASH_MAXNHITS, par.min_basq, q0, q1, codes.ctypes.data, None if e.qual is None else e.qual.ctypes.data,
                 qlen, hdr.ctypes.data, seeds.ctypes.data, qmask.ctypes.data)
    assert rv == 0, rv
    n = int(hdr[0])
    nh = seeds[:n, 1].astype(np.uint64)
    hcut = max(par.ncut, 0)
    nhit_cut = int(nh[nh <= hcut].sum() if hcut else nh.sum()) & 0xFFFFFFFF      # hashCalcHitInfoNumberOfHits, hashhit.c:1171
    t_lo, t_hi, _ = word_range(k, qlen, rng)
    e.lookups = int(np.isin(qmask[t_lo:t_hi], (HQ_NORMHIT, HQ_MULTIHIT, HQ_NOHIT)).sum())
    e.qmask = qmask
    if totals_only:                                       # calcTotalNumberOfHits (rmap.c:1076): no ranking, no seed table
        e.hdr, e.seeds = np.array([n, 0, HI_REVERSE if st else 0, qlen, 0, 0, nhit_cut], dtype=np.uint32), None
        return e
    rank = int(hdr[1])
    ns = rank if rank > 0 else n                          # hashHitInfoCalcHitNumbers, hashhit.c:1200-1219
    e.hdr = np.array([n, rank, int(hdr[2]), qlen, int(nh[:ns].sum()) & 0xFFFFFFFF, int(nh.sum()) & 0xFFFFFFFF, nhit_cut], dtype=np.uint32)
    e.seeds = seeds[:n].copy()
    return e


def ref_batch(oix, reads, quals, par, ranges=None, totals_only=False):
    """reads: ASCII bytes; -> list of Strand, index 2 * read + strand"""
    out = []
    for i, r in enumerate(reads):
        c = encode(r)
        for st in (0, 1):
            out.append(ref_strand(oix, c, None if quals is None else quals[i], st, par, None if ranges is None else ranges[i], totals_only))
    return out


def expect_arrays(exp, stride, guard=GUARD):
    """The arrays Mapper.seed_batch returns for these strands: what the reference defines, the guard everywhere else
    (seeds[i >= n_seeds], qmask[t > qlen], everything of a strand shorter than a word except its header, the unused header word,
    the row behind the last strand)."""
    rows = len(exp) + 1
    g32 = guard * 0x01010101
    hi, seeds, qmask = np.full((rows, 8), g32, np.uint32), np.full((rows, stride, 3), g32, np.uint32), np.full((rows, stride), guard, np.uint8)
    for rs, e in enumerate(exp):
        hi[rs, :7] = e.hdr
        if e.seeds is not None:
            seeds[rs, :len(e.seeds)] = e.seeds
        if e.qmask is not None:
            n = min(e.qlen + 1, stride)
            qmask[rs, :n] = e.qmask[:n]
    return hi, seeds, qmask


def expect_codes(reads):
    fw = [encode(r) for r in reads]
    cat = lambda a: np.concatenate(a) if a else np.zeros(0, np.uint8)
    return cat(fw), cat([revcomp(c) for c in fw])


def check_against(got, exp, reads, what=""):
    """Exact equality of everything Mapper.seed_batch (or the one-lane host build) returned with the reference, guards included."""
    hi, seeds, qmask = expect_arrays(exp, got["stride"], got.get("guard", GUARD))
    codes, codes_rc = expect_codes(reads)
    assert np.array_equal(got["codes"], codes), (what, "codes")
    assert np.array_equal(got["codes_rc"], codes_rc), (what, "codes_rc")
    bad = np.flatnonzero((got["hi"] != hi).any(axis=1))
    assert bad.size == 0, (what, "header of strand %d: got %s, expected %s" % (bad[0], got["hi"][bad[0]], hi[bad[0]]))
    bad = np.flatnonzero((got["qmask"] != qmask).any(axis=1))
    assert bad.size == 0, (what, "qualifiers of strand %d differ at %s" % (bad[0], np.flatnonzero(got["qmask"][bad[0]] != qmask[bad[0]])[:8]))
    bad = np.flatnonzero((got["seeds"] != seeds).any(axis=(1, 2)))
    assert bad.size == 0, (what, "seeds of strand %d differ at %s" % (bad[0], np.flatnonzero((got["seeds"][bad[0]] != seeds[bad[0]]).any(axis=1))[:8]))
    assert got["lookups"] == sum(e.lookups for e in exp), (what, "lookups", got["lookups"], sum(e.lookups for e in exp))


# ---------------------------------------------------------------------------------------------------------------------------
# which branches a strand takes
# ---------------------------------------------------------------------------------------------------------------------------
def _words(codes, k):
    """forward k-mer of every start as an integer (equal words <=> equal k-mers on either strand)"""
    c = (codes & 3).astype(np.uint64)
    n = codes.size - k + 1
    w = np.zeros(n, np.uint64)
    for i in range(k):
        w = (w << np.uint64(2)) | c[i:i + n]
    return w


def classify(e):
    """dict of the branches of stage_seed this strand takes (names as in DESIGN.md section 4)"""
    k, s, qlen = e.k, e.s, e.qlen
    d = dict(short=e.short, totals_only=e.totals_only, form="none", reason="", listed=False, budget_cut=False, cover_swap=False, maxcover_low=False,
             maxcover_high=False, minseed=False, rk_eq_nbud=False, mask_top=False, rep_cross=False, nvalid=0, nlook=0, range_given=e.rng is not None,
             range_fallback=False, range_clamped=False, lowq_word_first=False, lowq_word_last=False, qcount=[0] * 6)
    if e.short:
        d["reason"] = "qlen < k"
        return d
    d["qcount"] = [int((e.qmask[:qlen + 1] == c).sum()) for c in range(6)]
    t_lo, t_hi, fb = word_range(k, qlen, e.rng)
    d["range_fallback"] = fb
    d["range_clamped"] = e.rng is not None and int(e.rng[1]) >= qlen
    bad = (e.codes & 4) != 0
    if e.qual is not None:
        lowq = e.qual < e.par.min_basq + 33
        d["lowq_word_first"] = bool(lowq[t_lo] or lowq[t_hi - 1])            # first base of the first / the last word
        d["lowq_word_last"] = bool(lowq[t_lo + k - 1] or lowq[t_hi + k - 2])  # last base of the first / the last word
        bad = bad | lowq
    nbad = np.concatenate([[0], np.cumsum(bad)])
    valid = [t for t in range(t_lo, t_hi) if nbad[t + k] == nbad[t]]
    assert all((e.qmask[t] == HQ_NONSTDNT) == (nbad[t + k] != nbad[t]) for t in range(t_lo, t_hi))
    d["nvalid"], d["nlook"] = len(valid), e.lookups
    w = _words(e.codes, k)
    for j, t in enumerate(valid):                                            # the repeat filter over a 64-lane chunk boundary
        hit = [dd for dd in range(1, NREPEATS + 1) if dd <= j and w[valid[j - dd]] == w[t]]
        assert (e.qmask[t] == HQ_REPEAT) == bool(hit), (t, hit)
        if hit and any((j - dd) // 64 != j // 64 for dd in hit):
            d["rep_cross"] = True
    n = int(e.hdr[0])
    if e.totals_only:
        d["reason"] = "totals only"
        return d
    nh, qo = e.seeds[:, 1].astype(np.int64), e.seeds[:, 2].astype(np.int64)
    if e.par.noshort:
        d["reason"] = "noshort"
        assert int(e.hdr[1]) == 0 and not (int(e.hdr[2]) & (HI_SORTED | HI_RANK))
        return d
    if n <= 1:
        d["form"], d["reason"] = "trivial", "n_seeds <= 1"
        return d
    maxkey = int(nh.max())
    why = [r for c, r in ((qlen > 256, "qlen > 256"), (n >= 1 << SEED_IDXBITS, "n_seeds >= 4096"), (maxkey >= 1 << (32 - SEED_IDXBITS), "maxkey >= 2^20")) if c]
    d["form"], d["reason"], d["maxkey"] = ("lane", ", ".join(why), maxkey) if why else ("wave", "", maxkey)
    d["listed"] = d["form"] == "wave" and s <= 16
    assert np.all(np.diff(nh) >= 0)
    # budget and cover (getHitInfoMaxRank, hashhit.c:769-891)
    mincover, maxcover = MINCOVER_KMER * k + s, qlen * MAXCOVER_PERCENT // 100
    if maxcover < k + s:
        maxcover, d["maxcover_low"] = k + s, True
    elif maxcover > qlen - s:
        maxcover, d["maxcover_high"] = qlen - s, True
    if mincover > maxcover:
        mincover, maxcover, d["cover_swap"] = 0, qlen, True
    over = np.flatnonzero(np.cumsum(nh) > HASH_MAXNHITS)
    nbud = int(over[0]) if over.size else n
    d["budget_cut"] = nbud < n
    nmax = nbud
    for f in range(s):
        cov, cover, last = np.zeros(qlen + k, bool), 0, -1
        for rk in np.flatnonzero(qo % s == f):
            if not (cover <= maxcover and (cover < mincover or rk <= nbud)):
                break
            if cover >= mincover and rk == nbud:
                d["rk_eq_nbud"] = True
            q = int(qo[rk])
            cover += int((~cov[q:q + k - 1]).sum())                          # k - 1 bases (hashhit.c:873)
            cov[q:q + k - 1] = True
            if d["form"] == "wave" and q + k == 256:                     # the last word of a 256-base read: the top of the 256-bit mask
                d["mask_top"] = True                                         # (k - 1 bases: bit 254; bit 255 itself is out of reach)
            last = int(rk)
        nmax = max(nmax, last)
    rank = nmax
    if nmax < MINSEEDNUM:
        rank, d["minseed"] = min(MINSEEDNUM, n), True
    assert rank == int(e.hdr[1]), ("replay of the budget and cover loops", rank, int(e.hdr[1]))
    return d


def absent_behind_occupied_key(oix, e):
    """looked-up words of a forward strand that the hashed index does not hold although the bucket of their key is occupied"""
    if e.short or e.st:
        return 0
    f = ol.lib().or_index_bucket_size
    f.restype, f.argtypes = C.c_uint32, [C.POINTER(ol.OrIndex), C.c_uint64]
    t_lo, t_hi, _ = word_range(e.k, e.qlen, e.rng)
    w = _words(e.codes, e.k)
    bad = (e.codes & 4) != 0 if e.qual is None else ((e.codes & 4) != 0) | (e.qual < e.par.min_basq + 33)
    nbad = np.concatenate([[0], np.cumsum(bad)])
    return sum(1 for t in range(t_lo, t_hi) if e.qmask[t] == HQ_NOHIT and nbad[t + e.k] == nbad[t] and f(oix, int(w[t])) > 0)


BRANCHES = ("short", "form_wave", "form_lane_qlen", "form_lane_maxkey", "form_trivial", "form_none", "unlisted", "listed", "budget_cut", "budget_cut_wave",
            "cover_swap", "maxcover_low", "maxcover_high", "minseed", "rk_eq_nbud", "mask_top", "rep_cross", "valid_over_64", "seeds_over_64", "lowq_word_first",
            "lowq_word_last", "range_fallback", "range_kept", "range_clamped", "totals_only", "q_normhit", "q_multihit", "q_repeat", "q_nohit", "q_nonstdnt")


def tally(exp):
    """strands per branch over a list of Strand"""
    t = dict.fromkeys(BRANCHES, 0)
    for e in exp:
        d = classify(e)
        on = dict(short=d["short"], form_wave=d["form"] == "wave", form_lane_qlen="qlen > 256" in d["reason"], form_lane_maxkey="maxkey" in d["reason"],
                  form_trivial=d["form"] == "trivial", form_none=d["reason"] == "noshort", unlisted=d["form"] == "wave" and not d["listed"], listed=d["listed"],
                  budget_cut=d["budget_cut"], budget_cut_wave=d["budget_cut"] and d["form"] == "wave", cover_swap=d["cover_swap"], maxcover_low=d["maxcover_low"],
                  maxcover_high=d["maxcover_high"], minseed=d["minseed"], rk_eq_nbud=d["rk_eq_nbud"], mask_top=d["mask_top"], rep_cross=d["rep_cross"],
                  valid_over_64=d["nvalid"] > 64, seeds_over_64=not d["short"] and int(e.hdr[0]) > 64, lowq_word_first=d["lowq_word_first"],
                  lowq_word_last=d["lowq_word_last"], range_fallback=d["range_fallback"], range_kept=d["range_given"] and not d["range_fallback"] and not d["short"],
                  range_clamped=d["range_clamped"] and not d["short"], totals_only=d["totals_only"] and not d["short"], q_normhit=d["qcount"][HQ_NORMHIT] > 0,
                  q_multihit=d["qcount"][HQ_MULTIHIT] > 0, q_repeat=d["qcount"][HQ_REPEAT] > 0, q_nohit=d["qcount"][HQ_NOHIT] > 0, q_nonstdnt=d["qcount"][HQ_NONSTDNT] > 0)
        for b in BRANCHES:
            t[b] += bool(on[b])
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# the recursion of the quicksort as the wave sort walks it
# ---------------------------------------------------------------------------------------------------------------------------
def _partition(a, lo, hi):
    """sort.c:252-284 on a[lo..hi] (hi - lo >= 7), in place; -> the final i, j"""
    def swp(x, y):
        a[x], a[y] = a[y], a[x]
    mid = (lo + hi) >> 1
    swp(mid, lo + 1)
    if a[lo] > a[hi]:
        swp(lo, hi)
    if a[lo + 1] > a[hi]:
        swp(lo + 1, hi)
    if a[lo] > a[lo + 1]:
        swp(lo, lo + 1)
    i, j, pk = lo + 1, hi, a[lo + 1]
    while True:
        i += 1
        while a[i] < pk:
            i += 1
        j -= 1
        while a[j] > pk:
            j -= 1
        if j < i:
            break
        swp(i, j)
    a[lo + 1], a[j] = a[j], pk
    return i, j


def listed_ranges(keys):
    """Ranges of at most 32 (and at least 2) elements that the recursion over `keys` reaches -- the wave sort (wave_sort_kv,
    smg_wsort.hpp) finishes those one per lane and partitions the longer ones.  With a list of SEED_LISTCAP = 32 ranges the
    seeding stage's instance flushes its list in the middle of the recursion once for every 32 of them.
    -> (ranges, flushes before the end)."""
    a = [int(x) for x in keys]
    stack, ranges = [(0, len(a) - 1)], 0
    while stack:
        lo, hi = stack.pop()
        while hi > lo:
            if hi - lo + 1 <= SORT_SMALL:
                ranges += 1
                break
            i, j = _partition(a, lo, hi)
            if hi - i + 1 >= j - lo:                      # the larger part waits
                stack.append((i, hi))
                hi = j - 1
            else:
                stack.append((lo, j - 1))
                lo = i
    return ranges, ranges // SEED_LISTCAP

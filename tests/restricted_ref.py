"""Plain restatement of how the candidate stage decides the fill of a restricted call of rmapPair (interval mode of
stage_cands_v2, smalt_amd/csrc/smg_cands.hpp; collectHitsFromInterVal, rmap.c:438-492, hashCollectHitsForSegment,
hashhit.c:1416-1546): which of its branches a read strand takes and what the allocation-boundary protocol does per interval.
Python and numpy only; inputs are the seed tables of the ORACLE's dump (SD lines), the index arrays on the host
(hits_ref.HostIndex) and the intervals.  It CHOOSES and COUNTS inputs; what the stage computes is always compared with the
oracle.  Also the seeded workload of the restricted cases.  `file:line` citations: SMALT 0.7.6, src/."""
import collections

import numpy as np

import cands_ref as cr
import hits_ref as hr

HI_SORTED = 2                                             # hit info in its short form: the table is in rank order
IV_MAX = 2048
ALL_IN, COUNTED_LDS, COUNTED_SORT, DIRECT = "all_in", "counted-lds", "counted-sort", "direct"

Strand = collections.namedtuple("Strand", "branch n_seeds niv tot sorted order_differs aborted halved m_final quirk nkeys nk_first nk_last")
Strand.__doc__ = """branch: ALL_IN (the sum of the hit counts at or below the ceiling fits the allocation), COUNTED_LDS / COUNTED_SORT
(the counts of every (seed, interval) pair are taken first, in LDS or behind the ranking arrays) or DIRECT (the protocol
searches the lists interval by interval); sorted: the seed table is in rank order, so the stage builds the rank-to-offset
order; order_differs: that order is not the identity; aborted / halved: intervals whose fill met the allocation boundary /
whose ceiling was halved at least once; m_final: the smallest final ceiling; quirk: the keys gathered differ from what testing
the ceiling on the seed itself (not on the rank-sorted key, hashhit.c:1478) would gather; nkeys: keys the strand gathers; nk_first, nk_last: those of the
first and of the last interval (ALL_IN strands only, else -1)."""


def parse_seed_tables(dump_text):
    """-> [(n_seeds, status, [(qoffs, nhits, posidx) in table order])] for the forward and the reverse strand of one dump block"""
    out, cur = [], None
    for ln in dump_text.split("\n"):
        if ln.startswith("HI "):
            f = ln.split()
            cur = (int(f[2].split("=")[1]), int(f[4].split("=")[1]), [])
            out.append(cur)
        elif ln.startswith("SD "):
            f = ln.split()
            cur[2].append((int(f[3]), int(f[4]), int(f[5])))
    assert len(out) in (0, 2) and all(len(t[2]) == t[0] for t in out)
    return out


def iv_serials(sop, s, iv):
    """k-mer serial range [plo, phi) of an interval (hashhit.c:1711-1717 with rmap.c:462-474)"""
    sx, lo, hi = iv
    return (int(sop[sx]) + lo) // s, (int(sop[sx]) + hi + 1) // s


def _protocol(key_nhits, tails, insides, ncut, alloc):
    """One interval.  key_nhits[n]: the count the ceiling is tested on at step n; tails / insides[n]: positions of the n-th seed
    visited at or behind the interval's first serial / inside it.  -> (taken steps, aborted, halvings, final ceiling)"""
    m, halvings, ever = ncut, 0, False
    while True:
        total, aborted, n_used = 0, False, len(tails)
        for n in range(len(tails)):
            if m > 0 and key_nhits[n] > m:
                continue
            if tails[n] == 0:
                continue
            if total + tails[n] > alloc:
                if m > 0:
                    aborted, n_used = True, n
                    break
                continue
            total += insides[n]
        m_final = m
        m //= 2
        ever |= aborted
        if not (aborted and m > hr.MINHIT_PER_TUPLE):
            break
        halvings += 1
    taken = [n for n in range(n_used) if not (m_final > 0 and key_nhits[n] > m_final)]
    return taken, ever, halvings, m_final


def strand(hx, sop, table, intervals, qlen, ncut, candcap, lds_bytes, long_inst=False):
    """table: (n_seeds, status, seeds) of parse_seed_tables; candcap, lds_bytes: geometry of the slot the stage runs on;
    long_inst: the instance for reads of 256 bases and more (it never keeps the counts in LDS)"""
    n_seeds, status, seeds = table
    niv = len(intervals)
    alloc, _ = hr.hitlist_caps(qlen)
    tot = sum(nh for _, nh, _ in seeds if not (ncut > 0 and nh > ncut))
    srt = bool(status & HI_SORTED)
    order = sorted(range(n_seeds), key=lambda i: seeds[i][0]) if srt else list(range(n_seeds))
    differs = order != list(range(n_seeds))
    lists = [hx.positions(seeds[i][2]) for i in order]
    ser = [iv_serials(sop, hx.s, iv) for iv in intervals]
    ins = [[int(np.searchsorted(p, phi, "left") - np.searchsorted(p, plo, "left")) for p in lists] for plo, phi in ser]
    if tot <= alloc:
        per = [sum(c for c, i in zip(row, order) if not (ncut > 0 and seeds[i][1] > ncut)) for row in ins]
        return Strand(ALL_IN, n_seeds, niv, tot, srt, differs, 0, 0, ncut, False, sum(per), per[0] if per else 0, per[-1] if per else 0)
    ncnt = n_seeds * niv
    if ncnt + 2 * niv <= candcap and ncnt + n_seeds <= candcap:
        branch = COUNTED_LDS if (not long_inst and lds_bytes and ncnt * 8 <= lds_bytes) else COUNTED_SORT
    else:
        branch = DIRECT
    naborted = nhalved = nk = 0
    mmin, quirk = ncut, False
    for g, (plo, phi) in enumerate(ser):
        tails = [int(p.size - np.searchsorted(p, plo, "left")) for p in lists]
        taken, ab, hv, mf = _protocol([seeds[n][1] for n in range(n_seeds)], tails, ins[g], ncut, alloc)
        straight, _, _, _ = _protocol([seeds[i][1] for i in order], tails, ins[g], ncut, alloc)
        naborted += ab
        nhalved += hv > 0
        mmin = min(mmin, mf)
        nk += sum(ins[g][n] for n in taken)
        quirk |= [n for n in taken if ins[g][n]] != [n for n in straight if ins[g][n]]
    return Strand(branch, n_seeds, niv, tot, srt, differs, naborted, nhalved, mmin, quirk, nk, -1, -1)


def summary(strands):
    c = collections.Counter(s.branch for s in strands)
    return dict(strands=len(strands), all_in=c[ALL_IN], counted_lds=c[COUNTED_LDS], counted_sort=c[COUNTED_SORT], direct=c[DIRECT],
                sorted=sum(s.sorted and s.branch != ALL_IN for s in strands), order_differs=sum(s.order_differs and s.branch != ALL_IN for s in strands),
                quirk=sum(s.quirk for s in strands), aborted=sum(s.aborted > 0 for s in strands), halved=sum(s.halved > 0 for s in strands),
                max_keys=max([s.nkeys for s in strands] or [0]), above_1024=sum(s.nkeys > 1024 for s in strands))


# ---- the workload -----------------------------------------------------------------------------------------------------------
K, S = 11, 3
BIG_UNIT, BIG_COPIES, BIG_AT = 12, 20_000, 5000           # sequence 3: a 12-base unit (a multiple of s) x 20 000: one word holds 20 000 positions
MIX_UNIT, MIX_COPIES, MIX_DIV = 7, 3000, 0.01             # sequence 4: a 7-base unit x 3000 with 1 % substitutions: words of 900 .. 1000 positions
STRETCH_AT = (20_000, 40_300, 60_900, 81_800, 103_000, 125_400)      # cands_ref.tandem_workload: start of the stretches in sequences 0 .. 2
STRETCH_LEN = cr.TANDEM_STRETCHES


def workload(seed=977):
    """-> sequences as ASCII bytes: the three of cands_ref.tandem_workload(), the big array between spacers of 5000 bases, and the
    mixed array between spacers of 5000 bases (the last sequence)."""
    seqs, _ = cr.tandem_workload()
    rng = np.random.default_rng(seed)
    sp = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    big = np.concatenate([sp(BIG_AT), np.tile(sp(BIG_UNIT), BIG_COPIES), sp(5000)])
    mix = np.tile(sp(MIX_UNIT), MIX_COPIES)
    mut = rng.random(mix.size) < MIX_DIV
    mix = np.where(mut, (mix + rng.integers(1, 4, size=mix.size)) & 3, mix).astype(np.uint8)
    return seqs + [cr._ascii(big), cr._ascii(np.concatenate([sp(5000), mix, sp(5000)]))]


def cut(seqs, sx, at, n=100, rc=False, subst=0, seed=1):
    """A read of n bases from sequence sx at `at`, with `subst` substitutions, reverse-complemented if rc"""
    a = np.frombuffer(seqs[sx][at:at + n], dtype=np.uint8).copy()
    assert a.size == n
    if subst:
        rng = np.random.default_rng(seed)
        for i in rng.choice(n, size=subst, replace=False):
            a[i] = ord("ACGT"[("ACGT".index(chr(a[i])) + 1 + int(rng.integers(0, 3))) & 3])
    r = a.tobytes()
    return r[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")) if rc else r


def _win(at, before=150, after=250):
    return max(0, at - before), at + after


def cases(seqs):
    """-> dict name -> dict(reads=[ASCII bytes], ivs=[per read a list of (sx, lo, hi)], ncut=ktuple_maxhit).  Main-index rounds."""
    L = [len(x) for x in seqs]
    last = len(seqs) - 1
    c = {}
    # ---- all_in: geometry of the intervals (reads from the unique spacers and from short stretches)
    rd, iv = [], []

    def add(read, ivs):
        rd.append(read)
        iv.append(ivs)
    a = 5000
    add(cut(seqs, 0, a), [(0,) + _win(a)])                                             # one interval
    add(cut(seqs, 0, a, subst=3), [(0, a - 150, a + 49), (0, a + 50, a + 250)])       # two, abutting inside the read
    add(cut(seqs, 1, a, rc=True), [(0,) + _win(a), (1,) + _win(a), (last, 100, 400)])  # different sequences, the last among them
    add(cut(seqs, last, 2000), [(1,) + _win(a), (last,) + _win(2000)])
    add(cut(seqs, 0, 0), [(0, 0, 299)])                                               # at both ends of a sequence
    add(cut(seqs, 1, 0, rc=True), [(1, 0, 120)])
    add(cut(seqs, 0, L[0] - 100), [(0, L[0] - 300, L[0] - 1)])
    add(cut(seqs, last, L[last] - 100), [(last, L[last] - 300, L[last] - 1)])
    add(cut(seqs, 2, a), [(2, a - 100, a - 95), (2,) + _win(a)])                      # an interval shorter than k
    add(cut(seqs, 2, a), [(2, a + 3, a + 8), (2, a + 40, a + 50)])                    # ... and nothing else that holds the read whole
    for sx in range(3):                                                               # intervals that hold no sampled serial (plo == phi)
        g = sum(L[:sx])
        lo = a + ((-(g + a)) % S)                                                     # sop[sx] + lo is a multiple of s
        add(cut(seqs, sx, a), [(sx, lo, lo + 1)])
        add(cut(seqs, sx, a), [(sx, lo, lo + 1), (sx, lo + 30, lo + 31), (sx, lo + 60, lo + 200)])
    for sx in range(3):                                                               # lo, hi and sop[sx] in every residue mod s
        for dl in range(S):
            for dh in range(S):
                add(cut(seqs, sx, 7000 + 13 * dl, rc=bool(dh & 1)), [(sx, 7000 - 60 + dl, 7000 + 200 + dh)])
    add(cut(seqs, 0, a), [(0, 9000, 9400), (1, 9000, 9400)])                           # no hit in any interval
    add(cut(seqs, 0, a), [])                                                          # no interval at all
    add(cut(seqs, 0, a, n=10), [(0,) + _win(a)])                                      # a read shorter than k
    for j in (1, 2, 3):                                                               # stretches of 600 .. 1200 bases: a few thousand hits
        at = STRETCH_AT[j]
        add(cut(seqs, 0, at + 50, subst=2), [(0, at, at + STRETCH_LEN[j] // 2), (0, at + STRETCH_LEN[j] // 2 + 1, at + STRETCH_LEN[j] + 100)])
    c["geometry"] = dict(reads=rd, ivs=iv, ncut=10000)
    # ---- interval numbers: reads of the 6000-base stretch of sequence 0; the first and the last interval are wide, the others
    # hold two bases each (one sampled serial in two of three)
    at = STRETCH_AT[5]
    rd, iv = [], []
    for niv in (1023, 1024, 1025, 2047, 2048, 2049):
        mid = [(0, at + 400 + 2 * i, at + 401 + 2 * i) for i in range(niv - 2)]
        iv.append([(0, at, at + 300)] + mid + [(0, at + 5000, at + 5400)])
        rd.append(cut(seqs, 0, at + 100 + niv % 7, subst=niv % 3, rc=bool(niv & 1)))
    rd.append(cut(seqs, 0, 5000))
    iv.append([(0,) + _win(5000)])
    c["numbers"] = dict(reads=rd, ivs=iv, ncut=10000)
    # ---- !all_in with counts: reads of the mixed array (90 seeds of 900 .. 1000 hits, a ceiling of 884 between them); even reads
    # with 3 intervals (the counts fit the LDS working set), odd reads with 200 (they do not).  Reads near the array's end have
    # short tails behind their intervals and fill; the others meet the allocation boundary and halve the ceiling.
    mix_at, mix_len = 5000, MIX_UNIT * MIX_COPIES
    rd, iv = [], []
    for j in range(44):
        at = mix_at + (mix_len - 400 - 140 * (j // 2) if j % 4 < 2 else 300 + 700 * (j // 2))
        rd.append(cut(seqs, last, at, rc=bool(j & 2), subst=j % 3, seed=j))
        if j % 2 == 0:
            iv.append([(last, at - 120, at - 1), (last, at, at + 59), (last, at + 60, at + 260)])
        else:
            iv.append([(last, at - 600 + 6 * i, at - 600 + 6 * i + 3 + i % 3) for i in range(200)])
    c["counted"] = dict(reads=rd, ivs=iv, ncut=884)
    # ---- !all_in direct: the same kind of reads with 300 intervals each; slots of 2048 candidates have no room for the counts.
    # The intervals near the array's end hold two bases each, so that a strand stays below 1024 keys (first-pass slots).
    rd, iv = [], []
    for j in range(12):
        at = mix_at + mix_len - 1500 - 37 * j
        rd.append(cut(seqs, last, at, rc=bool(j & 1), subst=j % 3, seed=100 + j))
        iv.append([(last, at - 900 + 7 * i, at - 900 + 7 * i + 1 + (i % 3 == 0)) for i in range(300)])
    c["direct"] = dict(reads=rd, ivs=iv, ncut=884)
    # ---- the protocol aborts and halves: a ceiling of 100 000 and the big array (words of 20 000 positions), reads inside it and
    # across its ends; reads of the mixed array under the same ceiling
    big_end = BIG_AT + BIG_UNIT * BIG_COPIES
    rd, iv = [], []
    for j, at in enumerate((BIG_AT + 1000, BIG_AT + 120_001, big_end - 2000, BIG_AT - 50, BIG_AT - 30, big_end - 60, big_end - 45, big_end - 100)):
        rd.append(cut(seqs, 3, at, rc=bool(j & 1), subst=j % 2, seed=200 + j))
        iv.append([(3, max(0, at - 200), at + 99), (3, at + 100, at + 300)])
    for j in range(4):
        at = mix_at + 2000 + 4000 * j
        rd.append(cut(seqs, last, at, rc=bool(j & 1), seed=300 + j))
        iv.append([(last, at - 100, at + 200)])
    # chimeric reads, bases of the array first and of the spacer before it behind them, in an interval that holds both: in rank
    # order the array's seeds come last, in offset order first, so after the halving the ceiling test on the rank-sorted key
    # (hashhit.c:1478) skips the spacer's seeds and visits the array's, whose tails abort the fill again
    for j in range(24):
        split, upos = 36 + 2 * (j % 12), 600 + 150 * j
        r = cut(seqs, 3, BIG_AT + 1200 + j, n=split) + cut(seqs, 3, upos, n=100 - split)
        rd.append(r[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")) if j & 1 else r)
        w = 48 if j % 3 == 0 else 256                     # 160 intervals: the counts do not fit LDS; 30: they do
        iv.append([(3, 300 + w * i, 300 + w * i + w - 1) for i in range(7680 // w)])
    c["halving"] = dict(reads=rd, ivs=iv, ncut=100000)
    # ---- many keys per strand (all_in): reads of the stretches of 2400 and 6000 bases, the interval is the stretch
    rd, iv = [], []
    for sx in range(3):
        for j in (4, 5):
            for t in range(4):
                at = STRETCH_AT[j] + 100 + 250 * t
                rd.append(cut(seqs, sx, at, rc=bool(t & 1), subst=t, seed=400 + t))
                iv.append([(sx, STRETCH_AT[j] - 50, STRETCH_AT[j] + STRETCH_LEN[j] // 2), (sx, STRETCH_AT[j] + STRETCH_LEN[j] // 2 + 1, STRETCH_AT[j] + STRETCH_LEN[j] + 50)])
    c["many_keys"] = dict(reads=rd, ivs=iv, ncut=10000)
    # ---- reads of 300 bases (the instance for long reads): all_in in the stretches of 12-base units, counted in the exact
    # stretch of 7-base units of sequence 2 (290 seeds of 285 hits against an allocation of 65 536)
    rd, iv = [], []
    for t in range(6):
        at = STRETCH_AT[5] + 200 + 700 * t
        for sx in (0, 2):
            rd.append(cut(seqs, sx, at, n=300, rc=bool(t & 1), subst=2 * t, seed=500 + t))
            iv.append([(sx, at - 300, at + 149), (sx, at + 150, at + 700)] if t % 2 else [(sx, STRETCH_AT[5] + 5000, STRETCH_AT[5] + 6100)])
    c["long"] = dict(reads=rd, ivs=iv, ncut=10000)
    return c


def fine_case(seqs):
    """The rescue round (k = 5, s = 1 over the intervals, hit info in its long form) in the repeats: 400 intervals of 250 bases in the
    big array (every 5-mer of the unit holds 8333 positions, below the ceiling of 10 000), 50 of 280 bases in the mixed array,
    and 20 of 250 bases near the end of the big array (few enough for the counts to fit LDS)."""
    last = len(seqs) - 1
    big_end = BIG_AT + BIG_UNIT * BIG_COPIES
    rd, iv = [], []
    wide = [(3, BIG_AT + 1000 + 500 * i, BIG_AT + 1000 + 500 * i + 249) for i in range(400)]
    for j in range(6):                                    # 20 bases of the array and 80 of the spacer before it: 16 seeds of 8333 hits, below 200 k keys
        upos = 700 + 600 * j
        r = cut(seqs, 3, upos, n=80) + cut(seqs, 3, wide[40 + 70 * j][1] + 20 + j, n=20)
        rd.append(r[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA")) if j & 1 else r)
        iv.append([(3, upos - 100, upos + 200)] + wide)
    mixed = [(last, 5000 + 300 * i, 5000 + 300 * i + 279) for i in range(50)]
    for j, i in enumerate((35, 48)):
        rd.append(cut(seqs, last, mixed[i][1] + 50, rc=bool(j), subst=1, seed=610 + j))
        iv.append(mixed)
    few = [(3, big_end - 6000 + 300 * i, big_end - 6000 + 300 * i + 249) for i in range(20)]
    for j, i in enumerate((10, 19, 0, 5)):
        rd.append(cut(seqs, 3, few[i][1] + 30, rc=bool(j), subst=2 * j, seed=620 + j))
        iv.append(few)
    return dict(reads=rd, ivs=iv, ncut=10000)


# ---- running a case through the oracle, and what every case must hold -------------------------------------------------------
SCALARS = ("swmax", "sw2nd", "nseg", "nseg_tot", "nhit", "nhit_tot")


def stage_lines(text):
    """The lines of a dump block that are compared: everything but the hit lists (HL: one list per interval in a restricted call,
    which the two sides group differently) and the results (RS, RX: compared as results); the error code of the READ line apart."""
    return [ln.rstrip().rsplit(" err=", 1)[0] if ln.startswith("READ") else ln.rstrip() for ln in text.split("\n") if ln and ln[:2] not in ("HL", "RS", "RX")]


def oracle_case(ol, oix, case, raw=False, fine=False):
    """-> per read (rv, results, scalars, dump text, seed tables, index the seeds refer to as a hits_ref.HostIndex)"""
    par = ol.default_params(oix)
    par.ncut = case["ncut"]
    if raw:
        par.flags |= ol.FLG_RAWRESULTS
    out = []
    m = None if fine else ol.Mapper(oix)
    hx = None if fine else hr.HostIndex(oix)
    for i, (r, ivs) in enumerate(zip(case["reads"], case["ivs"])):
        if fine:                                          # the rescue round: an index of its own per read, the long form of the hit info
            fx = ol.build_fine_index(oix, ivs)
            m, hx = ol.Mapper(fx), hr.HostIndex(fx)
            par.flags |= ol.FLG_NOSHRTINFO
        rv, res = m.map(r, b"I" * len(r), par, ivs)
        text = m.dump(i, "r%d" % i, True)
        out.append((rv, res, dict(zip(SCALARS, m.stats()[:6])), text, parse_seed_tables(text), hx))
        if fine:
            m.close()
            ol.lib().or_index_free_fine(fx)
    if not fine:
        m.close()
    return out


def strands_of(exp, case, sop, candcap, lds_bytes, long_inst=False):
    """-> per read the Strand of its forward and reverse strand ([] for a read without seeds, e.g. shorter than k)"""
    return [[strand(e[5], sop, tb, ivs, len(r), case["ncut"], candcap, lds_bytes, long_inst) for tb in e[4]]
            for e, r, ivs in zip(exp, case["reads"], case["ivs"])]


def check_case(name, per_read, case):
    """What the inputs of case `name` must reach, from the predicates alone; -> the summary (the tests print it)"""
    flat = [s for ss in per_read for s in ss]
    sm = summary(flat)
    if name == "geometry":
        assert sm["all_in"] == sm["strands"] >= 80
        assert any(not ss for ss in per_read)                                       # the read shorter than k
        assert sum(1 for ss in per_read if ss and all(s.nkeys == 0 for s in ss)) >= 5    # no hit in any interval (no sampled serial, far away, none)
    elif name == "numbers":
        assert [len(v) for v in case["ivs"]] == [1023, 1024, 1025, 2047, 2048, 2049, 1]
        assert sm["all_in"] == sm["strands"]
        for ss in per_read[:6]:
            assert any(s.nk_first > 0 and s.nk_last > 0 for s in ss)
    elif name == "counted":
        assert sm["counted_lds"] >= 20 and sm["counted_sort"] >= 20 and sm["direct"] == 0
        assert sum(1 for s in flat if s.branch == COUNTED_LDS and s.order_differs) >= 20 and sum(1 for s in flat if s.branch == COUNTED_SORT and s.order_differs) >= 20
    elif name == "direct":
        assert sm["direct"] >= 10 and sm["counted_lds"] == sm["counted_sort"] == 0
    elif name == "halving":
        assert sm["aborted"] >= 5 and sm["halved"] >= 5 and sm["quirk"] >= 10 and sm["counted_lds"] >= 20 and sm["counted_sort"] >= 5
    elif name == "many_keys":
        assert sm["above_1024"] >= 20
    elif name == "long":
        assert sum(1 for s in flat if s.branch == ALL_IN and s.nkeys > 0) >= 4 and sm["counted_sort"] >= 4 and sm["counted_lds"] == 0
    elif name == "fine":
        assert sm["sorted"] == 0 and sm["counted_sort"] + sm["counted_lds"] >= 6 and sm["max_keys"] < 200_000
        assert all(s.tot > hr.hitlist_caps(100)[0] for s in flat if s.branch != ALL_IN)
    return sm

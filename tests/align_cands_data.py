"""Seeded cases for O1 (k_replay) and the K3 driver (stage_align as k_align runs it) on injected candidates, shared by
test_gpu_align_cands.py and test_align_cands_paths.py, with the oracle wrapper (or_map_injected) and the comparison.

A family is a dict(name, reads, cands, cdf, best, below_max, min_swatscor, prev_max, raw, rescore, max_len): per read a list of
candidate dicts (rs, re, qs, qe, band_l, band_r, sqidx, reverse, cover, swscor[, err]) in rank order and the cover deficit per
strand.  All families but the wide ones live in ONE reference (world()) of three sequences, so one index and one mapper serve them.

Reads are planted: a piece read[a:b] is copied to the reference so that the whole read would start at `pos0`; the bases next to a
piece are set to differ from the read, so a piece scores its length.  Windows and bands are laid around pos0 as cand_offsets lays
them around a segment that covers the read (smg_logic.hpp; with 7 bases on either side the band is [-14, 0], the formula's result
for s = 6 and a cover of the whole read); `extra` lowers band_l as a segment's srange does.

Every family has a `check` that asserts, on the oracle's output alone, that the family reaches what it is for."""
import numpy as np

import oracle_lib as ol

K, S = 13, 6
MATCH, MISMATCH, GAP_INIT, GAP_EXT = 1, -2, -4, -3
ERR_CAP, ERR_ASSERT = -5, -6
COMP = bytes.maketrans(b"ACGT", b"TGCA")
CTL_FIELDS = ("max1", "max2", "n_scored", "bandwidth_min", "min_swatscor", "scorlen_min", "go")


def revcomp(b):
    return bytes(b)[::-1].translate(COMP)


def rand_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n).astype(np.uint8))


def other_base(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))]


def mapper_geometry(max_len):
    """qmax, wincap, dircap and the result capacities a mapper for reads of max_len bases runs its second K3 pass with
    (smaltgpu_mapper_create_ex), for the host program"""
    qmax = (max_len + 8 + 7) & ~7
    wincap = 4 * qmax + 1024
    return dict(qmax=qmax, wincap=wincap, dircap=(qmax + 64) * (wincap + 8), rescap=16000, dstrcap=16000 * (qmax // 4 + 48))


class World:
    """reference sequences under construction"""

    def __init__(self, rng, lens):
        self.rng = rng
        self.seqs = [bytearray(rand_bases(rng, n)) for n in lens]

    def plant(self, sx, pos0, read, a=0, b=None):
        """read[a:b] at pos0 + a of sequence sx, the bases next to it unlike the read's"""
        b = len(read) if b is None else b
        s = self.seqs[sx]
        assert 0 <= pos0 + a and pos0 + b <= len(s)
        s[pos0 + a:pos0 + b] = read[a:b]
        if a > 0 and pos0 + a - 1 >= 0:
            s[pos0 + a - 1] = other_base(read[a - 1])
        if b < len(read) and pos0 + b < len(s):
            s[pos0 + b] = other_base(read[b])


def cand(seqlen, sx, pos0, qlen, lflank=7, rflank=7, bhalf=7, extra=0, cover=None, reverse=False, swscor=0):
    """the candidate of a read whose first base lies at pos0: the window reaches lflank bases to the left and rflank to the right
    of the read (clipped at the ends of the sequence), the band holds the read's diagonal and bhalf diagonals on either side, and
    `extra` more below"""
    left = min(lflank, pos0)
    rs, re = pos0 - left, min(pos0 + qlen - 1 + rflank, seqlen - 1)
    return dict(rs=rs, re=re, qs=0, qe=qlen - 1, band_l=-left - bhalf - extra, band_r=-left + bhalf, sqidx=sx, reverse=reverse,
                cover=qlen if cover is None else cover, swscor=swscor)


def family(name, reads, cands, cdf=None, best=True, below_max=0, min_swatscor=K + S - 1, prev_max=None, raw=False, rescore=True, max_len=150, check=None):
    return dict(name=name, reads=reads, cands=cands, cdf=cdf or [(0, 0)] * len(reads), best=best, below_max=below_max, min_swatscor=min_swatscor,
                prev_max=prev_max, raw=raw, rescore=rescore, max_len=max_len, check=check)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def or_params(oix, fam, raw=None):
    p = ol.default_params(oix)
    raw = fam["raw"] if raw is None else raw
    p.flags = (ol.FLG_BEST if fam["best"] else 0) | (ol.FLG_RAWRESULTS if raw else 0)
    p.min_swatscor_below_max, p.min_swatscor = fam["below_max"], fam["min_swatscor"]
    p.match, p.mismatch, p.gap_init, p.gap_ext = MATCH, MISMATCH, GAP_INIT, GAP_EXT
    return p


def oracle_eval(oix, fam, raw=None, fill=True):
    """or_map_injected over every read of the family -> per read dict(rv, ctl, swmax, sw2nd, results with cand_first, scores).
    With rescore the candidates' swscor is filled in from the oracle (0 behind the cover cut, where nothing reads it)."""
    m = ol.Mapper(oix)
    par = or_params(oix, fam, raw)
    out = []
    try:
        for r, read in enumerate(fam["reads"]):
            pm = fam["prev_max"][r] if fam["prev_max"] else None
            rv, res, scored = m.map_injected(read, par, fam["cands"][r], fam["cdf"][r], rescore=fam["rescore"], prevmax=pm)
            st, th = m.stats(), m.thresholds()
            for x, cf in zip(res, m.cand_first):
                x["cand_first"] = cf
            if fam["rescore"] and fill:
                for i, c in enumerate(fam["cands"][r]):
                    c["swscor"] = scored[i]["swscor"] if i < len(scored) else 0
            ctl = dict(max1=st[6], max2=st[7], n_scored=len(scored), bandwidth_min=th[0], min_swatscor=th[1], scorlen_min=th[2], go=th[3])
            out.append(dict(rv=rv, ctl=ctl, swmax=st[0], sw2nd=st[1], results=res, scores=[s["swscor"] for s in scored]))
    finally:
        m.close()
    return out


def compare(fam, exp, got, expect_err=None):
    """got: per read dict(ctl, err, swmax, sw2nd, results with cand_first), from the device or from the host program.
    expect_err: {read: code} for the reads that must fail with that code and no result (their scalars of O1 still compare).
    -> number of alignments compared"""
    assert len(got) == len(exp) == len(fam["reads"]), fam["name"]
    nali = 0
    for r, (e, g) in enumerate(zip(exp, got)):
        tag = (fam["name"], r)
        for f in CTL_FIELDS:
            assert g["ctl"][f] == e["ctl"][f], (tag, f, g["ctl"], e["ctl"])
        if expect_err and r in expect_err:
            assert g["err"] == expect_err[r] and g["results"] == [], (tag, g["err"], len(g["results"]))
            continue
        assert g["err"] == 0, (tag, g["err"])
        assert (g["swmax"], g["sw2nd"]) == (e["swmax"], e["sw2nd"]), (tag, g["swmax"], g["sw2nd"], e["swmax"], e["sw2nd"])
        assert len(g["results"]) == len(e["results"]), (tag, len(g["results"]), len(e["results"]))
        for j, (a, b) in enumerate(zip(g["results"], e["results"])):
            for f in ("score", "q_start", "q_end", "s_start", "s_end", "sidx", "reverse", "cand_first", "diffstr"):
                assert a[f] == b[f], (tag, j, f, a[f], b[f])
        nali += len(e["results"])
    return nali


def device_run(mp, gix, fam, antidiag=False, allow_read_errors=False, min_sw_per_read=False):
    """the family through smaltgpu_align_cands_batch -> (per read dicts as compare takes them, reads deferred).
    min_sw_per_read: the family's min_swatscor goes in through the call context, read by read, over another value in the parameters"""
    from smalt_amd import api
    par = gix.default_params()
    par.rmapflg = api.FLG_BEST if fam["best"] else 0
    par.min_swatscor_below_max, par.min_swatscor = fam["below_max"], fam["min_swatscor"]
    par.match, par.mismatch, par.gap_init, par.gap_ext = MATCH, MISMATCH, GAP_INIT, GAP_EXT
    cands = fam.get("packed") or fam["cands"]
    if min_sw_per_read:
        par.min_swatscor = 1
    res, stats, cf, ctl, ndef = mp.align_cands_batch(fam["reads"], par, cands, fam["cdf"], prev_max=fam["prev_max"], raw_alignments=fam["raw"],
                                                     min_swatscor=[fam["min_swatscor"]] * len(fam["reads"]) if min_sw_per_read else None,
                                                     antidiag=antidiag, allow_read_errors=allow_read_errors)
    got = []
    for r in range(len(fam["reads"])):
        for x, f in zip(res[r], cf[r]):
            x["cand_first"] = f
        assert stats[r]["nhit"] == 0 and stats[r]["nhit_tot"] == 0 and stats[r]["nseg"] == len(fam["cands"][r])
        got.append(dict(ctl=ctl[r], err=stats[r]["err"], swmax=stats[r]["swmax"], sw2nd=stats[r]["sw2nd"], results=res[r]))
    return got, ndef


def write_host_batch(path, fam):
    g = mapper_geometry(fam["max_len"])
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (MATCH, MISMATCH, GAP_INIT, GAP_EXT, fam["min_swatscor"], fam["below_max"],
                                                                   2 if fam["best"] else 0, 1 if fam["raw"] else 0, len(fam["reads"]), g["qmax"], g["wincap"],
                                                                   g["dircap"], g["rescap"], g["dstrcap"]))
        for r, read in enumerate(fam["reads"]):
            pm = fam["prev_max"][r] if fam["prev_max"] else (0, 0)
            f.write("%d %d %d %d %d %d\n%s\n" % (len(read), len(fam["cands"][r]), fam["cdf"][r][0], fam["cdf"][r][1], pm[0], pm[1], read.decode() or "-"))
            for c in fam["cands"][r]:
                f.write("%d %d %d %d %d %d %d %d %d %d\n" % (c["rs"], c["re"], c["qs"], c["qe"], c["band_l"], c["band_r"], c["sqidx"],
                                                             (1 if c["reverse"] else 0) | (2 if c.get("err") else 0), c["cover"], c["swscor"]))


def parse_host_output(text):
    got = []
    for ln in text.split("\n"):
        f = ln.split()
        if not f:
            continue
        if f[0] == "CTL":
            got.append(dict(ctl=dict(zip(CTL_FIELDS, [int(v) for v in f[1:8]])), results=[]))
        elif f[0] == "ST":
            got[-1].update(err=int(f[1]), swmax=int(f[2]), sw2nd=int(f[3]), nres=int(f[4]))
            assert int(f[6]) == 0
        else:
            assert f[0] == "RS"
            got[-1]["results"].append(dict(score=int(f[1]), q_start=int(f[2]), q_end=int(f[3]), s_start=int(f[4]), s_end=int(f[5]), sidx=int(f[6]),
                                           reverse=int(f[7]), cand_first=bool(int(f[8])), diffstr=b"" if f[9] == "-" else bytes.fromhex(f[9])))
    for g in got:
        assert g["nres"] == len(g["results"])
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the reference of the short families: two sequences of background and the array of 600 copies of a 40-base unit
# ---------------------------------------------------------------------------------------------------------------------
UNIT_N, UNIT_LEN, UNIT_STEP = 600, 40, 60
SEQLENS = (12000, 9000, UNIT_N * UNIT_STEP + 200)
_WORLD = {}


def world():
    """-> dict(seqs, fams): the reference and the short-driver families (a) .. (n) by name, built once"""
    if _WORLD:
        return _WORLD
    rng = np.random.default_rng(20240611)
    w = World(rng, SEQLENS)
    L = SEQLENS
    fams = {}
    free = [200, 200]                    # next free position per background sequence: every read gets a region of its own

    def region(sx, n):
        p = free[sx]
        free[sx] += n
        assert free[sx] < L[sx] - 200
        return p

    def mutated(read, nsub, indel=0, at=None):
        """a copy with nsub substitutions (a tuple: at these places), and `indel` bases deleted (> 0) or inserted (< 0) at `at`"""
        b = bytearray(read)
        for p in (nsub if isinstance(nsub, tuple) else rng.choice(len(b), size=nsub, replace=False)):
            b[p] = other_base(b[p])
        at = len(b) // 2 if at is None else at
        if indel > 0:
            del b[at:at + indel]
        elif indel < 0:
            b[at:at] = rand_bases(rng, -indel)
        return bytes(b)

    # --- (a) rising threshold: candidate 0 splits into [80, 70]; two candidates tie at the second-best first-pass score 65 -----
    R = rand_bases(rng, 150)
    p0 = region(0, 500) + 100
    w.plant(0, p0, R, 0, 80)
    w.plant(0, p0 + 40, R, 80, 150)                      # the tail 40 bases further right: a gap there costs more than the tail is worth
    ca = [cand(L[0], 0, p0, 150, rflank=47, extra=40)]
    for sx in (1, 1):
        q = region(sx, 400) + 100
        w.plant(sx, q, R, 20, 85)
        ca.append(cand(L[sx], sx, q, 150, cover=120))
    for n in (30, 25):
        q = region(0, 400) + 100
        w.plant(0, q, R, 100, 100 + n)
        ca.append(cand(L[0], 0, q, 150, cover=120))

    def check_a(exp):
        e = exp[0]
        th = e["ctl"]["min_swatscor"]
        assert sum(s >= th for s in e["scores"][1:]) >= 2 and sum(s < th for s in e["scores"]) >= 2, e["scores"]
        assert e["sw2nd"] > th and len(e["results"]) == 2 and sum(x["cand_first"] for x in e["results"]) == 1, (e["sw2nd"], th, e["results"])
    fams["a"] = family("a-rising-threshold", [R], [ca], check=check_a)

    # --- (b) ballot chunks: 130 candidates of one cover, the two that reach the threshold at ranks 70 and 129 ---------------------
    R = rand_bases(rng, 150)
    cb = []
    for i in range(130):
        if i == 70 or i == 129:
            q = region(1, 400) + 100
            w.plant(1, q, R if i == 70 else mutated(R, 2))
            cb.append(cand(L[1], 1, q, 150, cover=100))
        else:
            cb.append(cand(L[0], 0, 300 + 61 * i, 150, cover=100))

    def check_b(exp):
        e = exp[0]
        th = e["ctl"]["min_swatscor"]
        assert e["ctl"]["n_scored"] == 130 and [i for i, s in enumerate(e["scores"]) if s >= th] == [70, 129], th
        assert len(e["results"]) == 2
    fams["b"] = family("b-ballot-chunks", [R], [cb], check=check_b)

    # --- (c) plain duplicate, (d) lost alignment, (e) the same with raw_alignments ------------------------------------------------
    Rc = rand_bases(rng, 150)
    q = region(0, 400) + 100
    w.plant(0, q, Rc)
    cc = [cand(L[0], 0, q, 150), cand(L[0], 0, q, 150)]
    Rd = rand_bases(rng, 150)
    q = region(1, 500) + 100
    w.plant(1, q, Rd, 0, 80)
    w.plant(1, q + 40, Rd, 80, 150)
    c1 = cand(L[1], 1, q, 150, rflank=47, extra=40)
    c1["re"] = q + 95                                      # the smaller window ends in front of the second piece
    cd = [c1, cand(L[1], 1, q, 150, rflank=47, extra=40)]

    def check_cd(exp, raw):
        assert len(exp[0]["results"]) == 1 and len(raw[0]["results"]) == 2
        assert len(raw[1]["results"]) == 3 and len(exp[1]["results"]) == len(raw[1]["results"]) - 2, (len(exp[1]["results"]), len(raw[1]["results"]))
        assert exp[1]["swmax"] == raw[1]["swmax"] and exp[1]["sw2nd"] == raw[1]["sw2nd"] and exp[1]["sw2nd"] > 0      # the lost alignment still counts
    fams["cd"] = family("cd-duplicates", [Rc, Rd], [cc, cd], best=False, below_max=-1, check=check_cd)
    fams["e"] = family("e-raw", [Rc, Rd], [cc, cd], best=False, below_max=-1, raw=True)

    # --- (f) prev_max below, between and above the call's own scores ------------------------------------------------------------
    R = rand_bases(rng, 150)
    q1, q2 = region(0, 400) + 100, region(1, 400) + 100
    w.plant(0, q1, R)
    w.plant(1, q2, mutated(R, 3))
    cf = [cand(L[0], 0, q1, 150), cand(L[1], 1, q2, 150, cover=140)]
    pms = [(10, 5), (146, 144), (200, 180), (150, 0)]

    def check_f(exp):
        lo, mid, hi = exp[0], exp[1], exp[2]
        assert len(lo["results"]) == 2 and len(mid["results"]) == 1 and len(hi["results"]) == 0, [len(e["results"]) for e in exp]
        assert lo["ctl"] == mid["ctl"] == hi["ctl"] and (hi["swmax"], hi["sw2nd"]) == (200, 180)
    fams["f"] = family("f-prev-max", [R] * 4, [[dict(c) for c in cf] for _ in pms], prev_max=pms, check=check_f)

    # --- (g) band widening: reads with an indel of 4, bands of 2 and 4 diagonals (widened) and of 30 (not) ------------------------
    rg, cg = [], []
    # the last read: 3 substitutions and 4 bases deleted, so bandwidth_min is 3 + 4 = 7 against a band of 4: widened by (7 - 4 + 1) / 2
    # = 2 on either side, which just reaches the diagonal behind the deletion, 4 below the read's (rounded down it would not)
    for i, (bh, indel) in enumerate(((1, 4), (2, -4), (15, 4), (15, -4), (1, 0), (2, 4))):
        R = rand_bases(rng, 140)
        q = region(i & 1, 400) + 100
        w.plant(i & 1, q, R)
        rd = mutated(R, (20, 40, 100) if i == 5 else 4, indel, at=60)
        rev = i in (1, 3)
        rg.append(revcomp(rd) if rev else rd)
        cg.append([cand(L[i & 1], i & 1, q, len(rd), lflank=max(7, bh), rflank=max(7, bh) + 8, bhalf=bh, reverse=rev)])

    def check_g(exp):
        nar = [e["ctl"]["bandwidth_min"] > c[0]["band_r"] - c[0]["band_l"] for e, c in zip(exp, cg)]
        assert nar == [True, True, False, False, True, True] and all(e["ctl"]["bandwidth_min"] > 0 for e in exp), [e["ctl"] for e in exp]
        bw, bmin = cg[5][0]["band_r"] - cg[5][0]["band_l"], exp[5]["ctl"]["bandwidth_min"]
        assert (bmin - bw) % 2 == 1 and 2 + (bmin - bw + 1) // 2 == 4 and exp[5]["results"][0]["score"] == exp[5]["ctl"]["max1"] == 136 - 9 - 13
    fams["g"] = family("g-band-widening", rg, cg, check=check_g)

    # --- (h) split recursion: three pieces 20 bases apart in the reference; node, left, right ------------------------------------
    rh, chh = [], []
    for rev in (False, True):
        R = rand_bases(rng, 150)
        sx = 1 if rev else 0
        q = region(sx, 500) + 100
        w.plant(sx, q, R, 0, 45)
        w.plant(sx, q + 20, R, 45, 105)
        w.plant(sx, q + 40, R, 105, 150)
        rh.append(revcomp(R) if rev else R)
        chh.append([cand(L[sx], sx, q, 150, rflank=47, extra=40, reverse=rev)])

    # a third read: the node is read[0:130]; the 20 rows behind it, to the end of the window, hold read[50:70]: a right remainder of
    # exactly minscorlen + 1 = 20 rows, the shortest that is still aligned (alignment.c:1389)
    R = bytearray(rand_bases(rng, 150))
    if R[130] == R[50]:
        R[130] = other_base(R[130])                         # the node must not run on into the piece behind it
    R = bytes(R)
    q = region(0, 500) + 100
    w.plant(0, q, R, 0, 130)
    w.seqs[0][q + 130:q + 150] = R[50:70]
    rh.append(R)
    c3 = cand(L[0], 0, q, 150, extra=80)
    c3["re"] = q + 149
    chh.append([c3])

    def check_h(exp):
        e = exp[-1]
        assert e["ctl"]["scorlen_min"] == 19 and [x["score"] for x in e["results"]][:2] == [130, 20] and len(e["results"]) == 2, e["results"]
        assert e["results"][0]["s_end"] == c3["re"] - 20 + 1          # (1-based) the node ends 20 rows in front of the window's last
        for e in exp[:-1]:
            x = e["results"]
            assert len(x) == 3 and x[1]["s_start"] < x[0]["s_start"] < x[2]["s_start"] and x[0]["score"] > x[1]["score"], x
            assert [y["cand_first"] for y in x] == [True, False, False]
    fams["h"] = family("h-split-recursion", rh, chh, best=False, below_max=-1, check=check_h)

    # --- (i) a band that band_init refuses: skipped, no result, no error ----------------------------------------------------------
    R = rand_bases(rng, 150)
    q = region(0, 400) + 100
    w.plant(0, q, R)
    miss = cand(L[0], 0, q, 150)
    miss["band_l"], miss["band_r"] = 153, 167

    def check_i(exp):
        import band_data as bd
        e = exp[0]
        assert e["ctl"]["bandwidth_min"] == 0 and e["scores"] == [150, 150] and e["ctl"]["min_swatscor"] == 150 and len(e["results"]) == 1
        assert bd.py_band(153, 167, 0, 149, 150, 0, miss["re"] - miss["rs"], miss["re"] - miss["rs"] + 1) is None
    fams["i"] = family("i-refused-band", [R], [[cand(L[0], 0, q, 150), miss]], check=check_i)

    # --- (j) windows that start on base 0 of sequence 1 and end on the last base of the last sequence ----------------------------
    R1, R2, R3 = rand_bases(rng, 150), rand_bases(rng, 150), rand_bases(rng, 120)
    w.plant(1, 0, R1)
    w.plant(0, 3, R2)                                       # three bases into sequence 0: the left flank is clipped
    w.plant(2, L[2] - 120, R3)
    cj = [[cand(L[1], 1, 0, 150)], [cand(L[0], 0, 3, 150)], [cand(L[2], 2, L[2] - 120, 120, reverse=True)]]

    def check_j(exp):
        assert cj[0][0]["rs"] == 0 and cj[1][0]["rs"] == 0 and cj[2][0]["re"] == L[2] - 1
        assert exp[0]["results"][0]["s_start"] == 1 and exp[2]["results"][0]["s_end"] == L[2] and exp[0]["results"][0]["score"] == 150
        assert all(len(e["results"]) >= 1 for e in exp)
    fams["j"] = family("j-window-ends", [R1, R2, revcomp(R3)], cj, check=check_j)

    # --- (k) placement: window and directions in LDS; directions in HBM; a window of 1500 bases in HBM ----------------------------
    rk, ck = [], []
    for i, (lf, rf, bh) in enumerate(((7, 7, 7), (30, 38, 30), (700, 650, 7), (31, 31, 31))):
        R = rand_bases(rng, 150)
        sx = i & 1
        q = region(sx, 1800 if lf > 100 else 400) + (800 if lf > 100 else 100)
        w.plant(sx, q, R)
        rd = mutated(R, 3, 3 if i != 2 else 0, at=70)
        rk.append(rd)
        ck.append([cand(L[sx], sx, q, len(rd), lflank=lf, rflank=rf, bhalf=bh)])

    def check_k(exp):
        g = mapper_geometry(150)
        lds_win = g["qmax"] + g["qmax"] // 2 + 96             # align_lds_wincap: longer windows stay in the HBM slot
        wl = [c[0]["re"] - c[0]["rs"] + 1 for c in ck]
        bw = [c[0]["band_r"] - c[0]["band_l"] + 1 for c in ck]
        assert wl[0] <= lds_win and bw[0] * (wl[0] + 1) + 8 < 4096                      # directions fit the 8 KB LDS block beside the hot arrays
        assert wl[1] <= lds_win and wl[3] <= lds_win and bw[1] * wl[1] > 8192 and bw[3] * wl[3] > 8192 and bw[3] <= 64      # ... and cannot
        assert wl[2] == 1500 and wl[2] > lds_win and wl[2] <= g["wincap"]
        assert all(len(e["results"]) >= 1 for e in exp)
    fams["k"] = family("k-placement", rk, ck, check=check_k)

    # --- (l) empty reads: shorter than k, and without candidates, around an ordinary read -----------------------------------------
    R = rand_bases(rng, 100)
    q = region(0, 300) + 100
    w.plant(0, q, R)

    def check_l(exp):
        assert [len(e["results"]) for e in exp] == [0, 1, 0, 1] and exp[0]["ctl"]["go"] == 0 and exp[2]["ctl"]["go"] == 0
    fams["l"] = family("l-empty-reads", [R[:K - 1], R, rand_bases(rng, 100), R], [[], [cand(L[0], 0, q, 100)], [], [cand(L[0], 0, q, 100)]], check=check_l)

    # --- (m) result-slot deferral: 600 copies of a 40-base unit, 600 one-copy candidates, every one an alignment ------------------
    U = rand_bases(rng, UNIT_LEN)
    for i in range(UNIT_N):
        w.plant(2, 10 + UNIT_STEP * i, U)
    cm = [cand(L[2], 2, 10 + UNIT_STEP * i, UNIT_LEN, cover=UNIT_LEN) for i in range(UNIT_N)]

    def check_m(exp):
        assert len(exp[0]["results"]) == UNIT_N and all(x["score"] == UNIT_LEN and x["cand_first"] for x in exp[0]["results"])
    fams["m"] = family("m-result-slots", [U], [cm], best=False, below_max=-1, check=check_m)

    # --- (n) error paths: a window above the mapper's capacity; a broken candidate above and one below the threshold -------------
    R = rand_bases(rng, 150)
    qa, qb = region(0, 2300) + 200, region(1, 400) + 100
    w.plant(0, qa, R)
    w.plant(1, qb, mutated(R, 2))
    good, second = cand(L[0], 0, qa, 150), cand(L[1], 1, qb, 150, cover=140)
    big = cand(L[0], 0, qa, 150, rflank=1600)
    low = cand(L[1], 1, qb + 200, 150, cover=140)                   # (a cover the cut does not reach: the candidate is scored)

    def broken(c):
        return dict(c, err=True)

    def check_n(exp):
        g = mapper_geometry(150)
        assert big["re"] - big["rs"] + 1 > g["wincap"]
        assert exp[1]["scores"][1] >= exp[1]["ctl"]["min_swatscor"] and exp[3]["scores"][1] >= exp[3]["ctl"]["min_swatscor"]
        assert exp[5]["scores"][2] < exp[5]["ctl"]["min_swatscor"] and len(exp[5]["results"]) == 2
        assert all(len(exp[r]["results"]) == 2 for r in (0, 2, 4, 6))
    nb = [[dict(good), dict(second)] for _ in range(4)]
    fams["n"] = family("n-error-paths", [R] * 7, [nb[0], [dict(good), big, dict(second)], nb[1], [dict(good), broken(second)], nb[2],
                                                   [dict(good), dict(second), broken(low)], nb[3]], check=check_n)
    fams["n"]["expect_err"] = {1: ERR_CAP, 3: ERR_ASSERT}

    _WORLD.update(seqs=[bytes(s) for s in w.seqs], fams=fams)
    return _WORLD


SHORT_ANTIDIAG = ("a", "b", "cd", "e", "f", "g", "h", "i", "j", "k")      # the sub-cases that run a second time in the anti-diagonal form
SHORT_OK = ("a", "b", "cd", "e", "f", "g", "h", "i", "j", "k", "l", "m")  # the oracle returns OR_OK for every read
SHORT_NONEMPTY = ("a", "b", "cd", "e", "g", "h")                           # ... and at least one result ((f): the pair above leaves none)


def build_index(seqs, tmp_dir, name="ac"):
    """-> (oracle index, prefix of the index files)"""
    oix = ol.build_index(seqs, ["s%d" % i for i in range(len(seqs))], K, S)
    pre = str(tmp_dir / name)
    assert ol.lib().or_index_write(oix, pre.encode()) == 0
    return oix, pre


def check_family(fam, exp, raw=None):
    """the family's own conditions on the oracle's output"""
    name = fam["name"].split("-")[0]
    if name in SHORT_OK or name.startswith("w"):
        assert all(e["rv"] == 0 for e in exp), (fam["name"], [e["rv"] for e in exp])
    if name in SHORT_NONEMPTY:
        assert all(len(e["results"]) >= 1 for e in exp), fam["name"]
    if fam["check"]:
        if name == "cd":
            fam["check"](exp, raw)
        else:
            fam["check"](exp)


# ---------------------------------------------------------------------------------------------------------------------
# the wide driver: reads of 300 to 600 bases, bands of about 40, 100 and 300 diagonals after widening
# ---------------------------------------------------------------------------------------------------------------------
_WIDE = {}
WIDE_FORMS = {40: "ROWS", 100: "WAVE2", 300: "STRIP8"}
# SMALTGPU_ALIGN_DIRCAP takes effect only where a mapper's direction-matrix slots exceed 4 MiB, (qmax + 64) * (4 qmax + 1032): from
# reads of about 900 bases on.  The deferred reads are therefore run on a mapper for reads up to 1000 bases (still k_align<true>).
WIDE_DIRCAP, WIDE_DEFER_MAXLEN = 4096, 1000


def wide_world():
    if _WIDE:
        return _WIDE
    import band_data as bd
    rng = np.random.default_rng(777)
    lens = (12000, 9000)
    w = World(rng, lens)
    reads, cands, widths = [], [], []
    pos = [400, 400]
    for i, (qlen, width, indel) in enumerate(((300, 40, 5), (450, 40, -6), (600, 40, 0), (350, 100, 12), (580, 100, -15), (512, 100, 9), (400, 300, 30),
                                              (560, 300, -40))):
        sx = i & 1
        R = rand_bases(rng, qlen)
        q = pos[sx]
        pos[sx] += qlen + 900
        w.plant(sx, q, R)
        b = bytearray(R)
        for p in rng.choice(qlen, size=qlen // 40, replace=False):
            b[p] = other_base(b[p])
        at = qlen // 2
        if indel > 0:
            del b[at:at + indel]
        elif indel < 0:
            b[at:at] = rand_bases(rng, -indel)
        rd = bytes(b)
        rev = i % 3 == 1
        reads.append(revcomp(rd) if rev else rd)
        bh = width // 2
        cands.append([cand(lens[sx], sx, q, len(rd), lflank=bh, rflank=bh + 45, bhalf=bh, reverse=rev)])
        widths.append(width)

    def check_w(exp):
        from smalt_amd import api
        seen = set()
        for e, c, wd, rd in zip(exp, cands, widths, reads):
            c = c[0]
            bl, br = c["band_l"], c["band_r"]
            if br - bl < e["ctl"]["bandwidth_min"]:
                d = (e["ctl"]["bandwidth_min"] - (br - bl) + 1) // 2
                bl, br = bl - d, br + d
            wl = c["re"] - c["rs"] + 1
            geo = api.band_geometry(bl, br, c["qs"], c["qe"], len(rd), 0, wl - 1, wl, GAP_INIT, GAP_EXT)
            assert geo is not None and len(e["results"]) >= 1
            if bd.FORM_NAMES[geo["form"]] == WIDE_FORMS[wd]:
                seen.add(wd)
        assert seen == set(WIDE_FORMS), seen
    fam = family("w-wide", reads, cands, max_len=600, check=check_w)
    # the read whose band is deferred: its direction matrix exceeds a first-pass slot of 4096 bytes
    def check_wd(exp):
        assert all(len(e["results"]) >= 1 for e in exp)
        for c in (cands[1][0], cands[4][0]):
            assert (c["band_r"] - c["band_l"] + 1) * (c["re"] - c["rs"] + 1) > WIDE_DIRCAP
    fdef = family("wd-deferred", reads[1:2] + reads[4:5], [[dict(c) for c in cands[1]], [dict(c) for c in cands[4]]], max_len=WIDE_DEFER_MAXLEN, check=check_wd)
    _WIDE.update(seqs=[bytes(s) for s in w.seqs], fam=fam, fdef=fdef)
    return _WIDE


# ---------------------------------------------------------------------------------------------------------------------
# O1 lists: scores given, windows of 20 bases of background (nothing need align)
# ---------------------------------------------------------------------------------------------------------------------
O1_COMBOS = [(best, bm, ms) for best in (True, False) for bm in (-1, 0, 5, 1000) for ms in (K + S - 1, 60)]


def py_replay_branches(qlen, cands, cdf, best):
    """which branches of the sequential control a list reaches (a model of the rule for COUNTING only; expected values come from the
    oracle): (cut fired, cover <= cdf at a new maximum)"""
    max_cover = min_cover = max1 = max2 = 0
    low = False
    for i, c in enumerate(cands):
        d = cdf[1 if c["reverse"] else 0]
        if best and c["cover"] + d < min_cover:
            return True, low
        if c["swscor"] > max2:
            if c["swscor"] > max1:
                max2, max1 = max1, c["swscor"]
                if c["cover"] + d > max_cover:
                    low = low or c["cover"] <= d
                    max_cover = c["cover"] - d if c["cover"] > d else 0
            else:
                max2 = c["swscor"]
            dcov = ((max1 - max2) // (MATCH - MISMATCH) + 1) * S
            if dcov + d + min_cover < max_cover:
                min_cover = max_cover - dcov
    return False, low


def o1_lists(seqlens, n=400, seed=4242):
    """-> (reads, cands, cdf): 400 reads of 40 to 150 bases with 1 to 200 candidates each, covers descending, strands mixed"""
    rng = np.random.default_rng(seed)
    reads, cands, cdfs = [], [], []
    for r in range(n):
        qlen = int(rng.integers(40, 151))
        nc = int(rng.integers(1, 4)) if r % 5 == 0 else int(rng.integers(1, 201))
        top = int(rng.integers(K, qlen + 1))
        if r % 2 == 0:                                       # covers clustered within a few strides of the top: the cut seldom fires
            cov = top - rng.integers(0, 2 * S + 1, size=nc)
        else:
            cov = rng.integers(K, top + 1, size=nc)
        cov = np.sort(np.clip(cov, 1, qlen))[::-1]
        sc = cov - rng.integers(0, 31, size=nc)
        arb = rng.random(nc) < 0.15
        sc[arb] = rng.integers(0, qlen + 1, size=int(arb.sum()))
        sc = np.clip(sc, 0, qlen)
        kind = r % 16
        if kind == 3:
            sc[:] = 0                                        # max1 < 1: go == 0
        elif kind == 7 and nc >= 2:
            sc[int(rng.integers(1, nc))] = sc.max()          # max1 == max2
            sc[0] = sc.max()
        elif kind == 11:
            sc[1:] = 0                                       # max2 == 0
            sc[0] = max(1, sc[0])
        cdf = (0, 0)
        if r % 3 == 1:
            cdf = (int(rng.integers(0, 31)), int(rng.integers(0, 31)))
        if r % 8 == 5:
            cdf = (int(rng.integers(100, 200)), int(rng.integers(100, 200)))      # cover <= cdf
        lst = []
        for i in range(nc):
            sx = int(rng.integers(0, 2))
            rs = int(rng.integers(0, seqlens[sx] - 40))
            lst.append(dict(rs=rs, re=rs + 19, qs=0, qe=qlen - 1, band_l=-7, band_r=7, sqidx=sx, reverse=bool(rng.integers(0, 2)), cover=int(cov[i]),
                            swscor=int(sc[i])))
        reads.append(rand_bases(rng, qlen))
        cands.append(lst)
        cdfs.append(cdf)
    return reads, cands, cdfs


def o1_family(seqlens, best, below_max, min_swatscor, lists=None):
    reads, cands, cdfs = lists or o1_lists(seqlens)
    return family("o1-%s-d%d-m%d" % ("best" if best else "all", below_max, min_swatscor), reads, cands, cdf=cdfs, best=best, below_max=below_max,
                  min_swatscor=min_swatscor, rescore=False)


def check_o1(fam, exp):
    """the conditions on the lists (best mode: the cut; any mode: the maxima)"""
    n = len(exp)
    cut = sum(e["ctl"]["n_scored"] < len(c) for e, c in zip(exp, fam["cands"]))
    if fam["best"]:
        assert cut >= n // 4 and n - cut >= n // 4, (cut, n)
    else:
        assert cut == 0
    br = [py_replay_branches(len(r), c, d, fam["best"]) for r, c, d in zip(fam["reads"], fam["cands"], fam["cdf"])]
    assert sum(b[0] for b in br) == cut
    counts = dict(max2_zero=sum(e["ctl"]["max2"] == 0 and e["ctl"]["max1"] > 0 for e in exp),
                  max_equal=sum(e["ctl"]["max1"] == e["ctl"]["max2"] > 0 for e in exp),
                  all_zero=sum(e["ctl"]["max1"] < 1 and e["ctl"]["go"] == 0 for e in exp),
                  cover_le_cdf=sum(b[1] for b in br))
    assert all(v >= 20 for v in counts.values()), counts
    counts.update(cut=cut, no_cut=n - cut, go=sum(e["ctl"]["go"] for e in exp))
    return counts


def hand_lists(seqlens):
    """three lists with literal expected values: best mode, +1/-2, s = 6, 150-base reads, no cover deficit.
    List 1: after (140, 150) the maximal cover is 140; (128, 147) makes max2 147, dcov = ((150 - 147) / 3 + 1) * 6 = 12 and min_cover
    128; (100, 120) lies below: the loop ends with 2 scored.  List 2: (128, 120) has a cover EQUAL to min_cover and is still scored,
    (90, 10) is not.  List 3: list 1 without the best flag: no cut."""
    rng = np.random.default_rng(99)

    def mk(pairs):
        qlen = 150
        out = []
        for cov, sc in pairs:
            rs = int(rng.integers(0, seqlens[0] - 40))
            out.append(dict(rs=rs, re=rs + 19, qs=0, qe=qlen - 1, band_l=-7, band_r=7, sqidx=0, reverse=False, cover=cov, swscor=sc))
        return out
    l1 = [(140, 150), (128, 147), (100, 120)]
    l2 = [(140, 150), (128, 147), (128, 120), (90, 10)]
    reads = [rand_bases(rng, 150) for _ in range(2)]
    fb = family("hand-best", reads, [mk(l1), mk(l2)], rescore=False)
    fa = family("hand-all", reads[:1], [mk(l1)], best=False, rescore=False)
    return [(fb, [dict(n_scored=2, max1=150, max2=147), dict(n_scored=3, max1=150, max2=147)]), (fa, [dict(n_scored=3, max1=150, max2=147)])]

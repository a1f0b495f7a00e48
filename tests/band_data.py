"""Seeded task generators, oracle wrappers and the recursion driver shared by the banded parity tests: K2b
(test_gpu_band_k2b.py), K3 form by form (test_gpu_band_k3.py) and the same without a GPU (test_band_nodes.py).

A task is a dict(q, w, band) of a read and a window as bytes of 3-bit codes (0-3, 5 = N) and band = (band_l, band_r, qs, qe):
the diagonals (read column - window row) the band holds and the first and last read column.  Windows are built as
test_gpu_sw_handover._window builds them (the read, or its head, with a few substitutions at a random place), so an alignment
exists on the diagonal -at, and the band is laid around that diagonal.  Reads with a period of 2 to 7 bases in a window of
the same period make several diagonals and rows tie for the maximum: the first cell in row-major order must win
(alignment.c:826-830)."""
import ctypes as C

import numpy as np

import oracle_lib as ol

PENS = [(1, -2, -4, -3), (2, -3, -5, -2), (3, -4, -8, -1), (2, -3, -2, -4), (15, -14, -20, -10)]
PEN_IDS = ["m%d_x%d_g%d_e%d" % (p[0], -p[1], -p[2], -p[3]) for p in PENS]
OR_OK, OR_ERR, OR_ERR_BAND, OR_ERR_SWATSCOR = 0, 1, 3, 4
NODE_ALIGNED, NODE_REFUSED, NODE_BELOW, ESCORE, EINTERNAL = 0, 1, 2, -8, -6
ROWS, ANTIDIAG, WAVE2, WAVE4, WAVE7, WAVE12, STRIP8, STRIP16, SCALAR = range(9)
FORM_NAMES = ["ROWS", "ANTIDIAG", "WAVE2", "WAVE4", "WAVE7", "WAVE12", "STRIP8", "STRIP16", "SCALAR"]
WAVE_SLOTS = {WAVE2: 2, WAVE4: 4, WAVE7: 7, WAVE12: 12}
ALILEN_MIN = 5


def score_matrix(match, mismatch):
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, match, mismatch)
    return M


# ---------------------------------------------------------------------------------------------------------------------
# sequences
# ---------------------------------------------------------------------------------------------------------------------
def rq(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def periodic(rng, n, period):
    motif = rq(rng, period)
    while period > 1 and len(set(motif.tolist())) < 2:
        motif = rq(rng, period)
    return np.resize(motif, n).astype(np.uint8)


def mutate(rng, core, sub=0.05, nindel=0):
    """substitutions, and nindel insertions or deletions of 1 to 3 bases"""
    core = core.copy()
    m = rng.random(len(core)) < sub
    core[m] = (core[m] + 1) & 3
    for _ in range(nindel):
        if len(core) < 12:
            break
        p = int(rng.integers(5, len(core) - 5))
        k = int(rng.integers(1, 4))
        core = np.concatenate([core[:p], core[p + k:]]) if rng.random() < 0.5 else np.concatenate([core[:p], rq(rng, k), core[p:]])
    return core.astype(np.uint8)


def task(rng, qlen, wlen, ndiag, kind="plain", sub=0.05, nindel=0, period=0, qs=None, qe=None, n_read=False, n_win=False, shift=None, qoff=0):
    """One (read, window, band) task.  kind: plain -- the read (its head if the window is shorter) with substitutions and indels;
    exact -- a copy without any; split -- three exact pieces of the read with two long stretches between them in which no
    base matches, so that the node's alignment leaves pieces for the remainders of the window (recursion of depth 2 and more);
    periodic -- read and window of one period; miss -- a band that does not meet the read (band_init refuses it);
    whole -- band_r < band_l: band_init turns to the whole matrix.  shift: where in the band the read's diagonal lies;
    qoff: the window holds the read from this base on (band_l inside the read: a band that is not clipped at the left)."""
    q = periodic(rng, qlen, period) if kind == "periodic" else rng.integers(0, 3, size=qlen, dtype=np.uint8) if kind == "split" else rq(rng, qlen)
    n = min(qlen - qoff, wlen)
    if kind == "periodic":
        at = int(rng.integers(0, wlen - n + 1))
        w = np.resize(np.roll(q[:period], at % period), wlen).astype(np.uint8)       # the read fits at at, at +- period, ...
        if sub:
            m = rng.random(wlen) < sub / 4
            w[m] = (w[m] + 1) & 3
    else:
        core = q[qoff:qoff + n].copy()
        if kind == "plain":
            core = mutate(rng, core, sub, nindel)[:wlen]
        elif kind == "split" and n >= 72:
            # pieces of P bases with stretches of L = 3 P bases of T between them, the read being without T: nothing matches
            # there on any diagonal, L mismatches cost more than a piece is worth (match x P), and so does a gap of L bases
            # there and one back (2 (gi + (L - 1) ge)) with every penalty set of PENS, so each piece aligns alone
            P = n // 9
            L = 3 * P
            for a in (P, 2 * P + L):
                core[a:a + L] = 3
        at = int(rng.integers(0, wlen - len(core) + 1))
        w = rq(rng, wlen)
        w[at:at + len(core)] = core
    if n_read:
        q[int(rng.integers(0, qlen))] = 5
    if n_win:
        w[int(rng.integers(0, wlen))] = 5
    off = int(rng.integers(0, ndiag)) if shift is None else shift
    bl = qoff - at - off
    br = bl + ndiag - 1
    if kind == "miss":
        bl, br = qlen + 3, qlen + 3 + ndiag - 1
    elif kind == "whole":
        bl, br = 5, 2
    return dict(q=q.tobytes(), w=w.tobytes(), band=(bl, br, 0 if qs is None else qs, qlen - 1 if qe is None else qe), kind=kind)


# ---------------------------------------------------------------------------------------------------------------------
# band geometry: a plain restatement of the reference's initALIBAND (alignment.c:310-396) and of the choice of form
# ---------------------------------------------------------------------------------------------------------------------
def py_band(bl, br, qs, qe, qlen, s_left, s_right, wlen):
    """dict of the band's fields, or None if the band is refused"""
    b = {}
    b["s_len"] = wlen if (s_right < 0 or s_right >= wlen) else s_right + 1
    b["q_len"] = qlen if (qe < 0 or qe >= qlen) else qe + 1
    b["s_totlen"], b["q_totlen"] = wlen, qlen
    b["s_left"] = b["s_left_orig"] = s_left if 0 < s_left < b["s_len"] else 0
    b["q_left"] = b["q_left_orig"] = qs if 0 < qs < b["q_len"] else 0
    b["l_edge_orig"] = b["l_edge"] = bl
    b["r_edge_orig"] = b["r_edge"] = br
    if br - bl + 1 <= 0:
        b["l_edge"], b["r_edge"] = b["q_left"], b["q_len"] - 1
    else:
        if bl + b["s_len"] > b["q_len"]:
            b["s_len"] = b["q_len"] - bl
        b["l_edge"] += b["s_left"]
        if b["l_edge"] >= b["q_len"] or br + b["s_len"] <= b["q_left"]:
            return None
        b["r_edge"] += b["s_left"]
        if b["r_edge"] < b["q_left"]:
            d = b["q_left"] - b["r_edge"]
            b["s_left"] += d
            b["l_edge"] += d
            b["r_edge"] = b["q_left"]
        b["r_edge"] = min(b["r_edge"], b["q_len"] - 1)
    b["band_width"] = b["r_edge"] - b["l_edge"] + 1
    return b if b["band_width"] >= 0 else None


def nslot(b):
    return (b["r_edge"] - b["l_edge"]) // 128 + 1 if b["band_width"] >= 1 else 0


def form_ok(form, b, gi, ge):
    """the precondition of a form of the K3 band pass on an accepted band (gi, ge: positive penalties)"""
    bw = b["band_width"]
    if form == ROWS:
        return 1 <= bw <= 64 and gi >= ge >= 0
    if form == ANTIDIAG:
        return 1 <= bw <= 64
    if form in WAVE_SLOTS:
        return bw >= 1 and nslot(b) <= WAVE_SLOTS[form]
    if form == STRIP8:
        return 256 <= bw < 2048
    if form == STRIP16:
        return bw >= 2048
    return form == SCALAR


def py_form(b, gi, ge):
    """the form the mapper's K3 kernel for long reads picks (stage_align): strips from 256 diagonals on if a strip holds a
    visited column, rows (or anti-diagonals if gi < ge) up to 64, else the narrowest wave form, else one lane"""
    bw = b["band_width"]
    if bw >= 256:
        cbits = 3 if bw < 2048 else 4
        nrows = b["s_len"] - b["s_left"]
        jmin = max(b["q_left"], b["l_edge"])
        jmax = min(b["r_edge"] + nrows, b["q_len"])
        if nrows > 0 and jmax > (jmin & ~((1 << cbits) - 1)):
            return STRIP8 if bw < 2048 else STRIP16
    if 1 <= bw <= 64:
        return ROWS if gi >= ge >= 0 else ANTIDIAG
    for f in (WAVE2, WAVE4, WAVE7, WAVE12):
        if 1 <= nslot(b) <= WAVE_SLOTS[f]:
            return f
    return SCALAR


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def or_band_fast(t, pen, M):
    """(return code, score) of the oracle's K2b over the whole window"""
    sc = C.c_int()
    bl, br, qs, qe = t["band"]
    rv = ol.lib().or_sw_band_fast(C.byref(sc), t["q"], len(t["q"]), t["w"], len(t["w"]), M, pen[2], pen[3], bl, br, qs, qe, 0, len(t["w"]) - 1)
    return rv, sc.value


def minscorlen_of(pen, minscore, minscorlen=ALILEN_MIN):
    return minscore // pen[0] if minscorlen * pen[0] < minscore else minscorlen       # aliSmiWatInBand, alignment.c:1548-1601


def or_band_full(t, pen, M, minscore):
    """(return code, [(score, qs, qe, rs, re, DiffStr)]) of one or_sw_band_full call on the root"""
    out, n = C.POINTER(ol.OrAli)(), C.c_int()
    bl, br, qs, qe = t["band"]
    rv = ol.lib().or_sw_band_full(C.byref(out), C.byref(n), t["q"], len(t["q"]), t["w"], len(t["w"]), M, pen[2], pen[3], pen[0],
                                  bl, br, qs, qe, 0, len(t["w"]) - 1, minscore, ALILEN_MIN)
    res = [(out[i].score, out[i].qs, out[i].qe, out[i].rs, out[i].re, bytes(out[i].diffstr[:out[i].dlen])) for i in range(n.value)]
    ol.lib().or_ali_free(out, n.value)
    return rv, res


def has_diagonal_tie(t, pen, M, score):
    """whether two diagonals of the band reach `score` without a gap: two cells then tie for a maximum of `score`"""
    bl, br, qs, qe = t["band"]
    hits = 0
    for d in range(bl, br + 1):
        rv, sc = or_band_fast(dict(t, band=(d, d, qs, qe)), pen, M)
        hits += rv == OR_OK and sc == score
        if hits >= 2:
            return True
    return False


# ---------------------------------------------------------------------------------------------------------------------
# the recursion of alignSmiWatBandRecursive (alignment.c:1300-1434; oracle/or_align.c band_recursive), driven from here: a
# stack of (s_left, s_right) per task, one call of the node evaluator per round for all pending nodes
# ---------------------------------------------------------------------------------------------------------------------
def run_recursion(tasks, pen, minscore, evaluate, max_rounds=40):
    """evaluate(list of (task, (s_left, s_right))) -> list of dict(status, score, max_i, max_j, qs, rs, diffstr).
    Returns per task (return code, [(score, qs, qe, rs, re, DiffStr)], depth) as or_band_full gives them: results in the
    order node, left, right, and nothing after the first node that fails."""
    msl = minscorlen_of(pen, minscore)
    assert msl >= ALILEN_MIN and minscore >= 1
    trees = [dict(iv=(0, len(t["w"]) - 1), depth=1) for t in tasks]
    pending = [(i, trees[i]) for i in range(len(tasks))]
    for _ in range(max_rounds):
        if not pending:
            break
        outs = evaluate([(tasks[i], nd["iv"]) for i, nd in pending])
        assert len(outs) == len(pending)
        nxt = []
        for (i, nd), o in zip(pending, outs):
            nd["out"] = o
            nd["left"] = nd["right"] = None
            if o["status"] != NODE_ALIGNED:
                continue
            s_left, s_right = nd["iv"]
            qs, rs, qe, re = o["qs"], o["rs"], o["max_j"], o["max_i"]
            if qs + msl > qe + 1:                          # too short: neither a result nor a recursion
                nd["short"] = True
                continue
            if s_left + msl < rs:
                nd["left"] = dict(iv=(s_left, rs - 1), depth=nd["depth"] + 1)
                nxt.append((i, nd["left"]))
            if s_right > re + msl:
                nd["right"] = dict(iv=(re + 1, s_right), depth=nd["depth"] + 1)
                nxt.append((i, nd["right"]))
        pending = nxt
    assert not pending, "recursion deeper than %d rounds" % max_rounds
    res = []
    for tr in trees:
        alis, rv, depth = [], OR_OK, 0
        stack = [tr]
        while stack:
            nd = stack.pop()
            o = nd["out"]
            if o["status"] == ESCORE:
                rv = OR_ERR_SWATSCOR
                break
            if o["status"] < 0:
                rv = OR_ERR
                break
            if o["status"] != NODE_ALIGNED or nd.get("short"):
                continue
            alis.append((o["score"], o["qs"], o["max_j"], o["rs"], o["max_i"], o["diffstr"]))
            depth = max(depth, nd["depth"])
            for ch in (nd["right"], nd["left"]):          # the left remainder first
                if ch is not None:
                    stack.append(ch)
        res.append((rv, alis, depth))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the case lists of the K3 forms: the smallest shapes that cross each boundary of a form's code
# ---------------------------------------------------------------------------------------------------------------------
NARROW = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64]      # diagonals: the 16-, 32- and 64-lane instances of the row form


def narrow_cases(rng):
    """ROWS and ANTIDIAG: every band width around the lane counts; 1, 63, 64, 65, 128 and 129 rows (the 64-row code register);
    exact runs of 63, 64, 65 and 200 matches (the traceback's 64-step rounds, DIFF_MAXMISMATCH); clipped at both read ends"""
    t = []
    for nd in NARROW:
        t.append(task(rng, 150, 190, nd, nindel=1 if nd >= 15 else 0))
        t.append(task(rng, 150, 190, nd, kind="split"))
        if nd >= 15:
            t.append(task(rng, 120, 160, nd, kind="periodic", period=2 + nd % 6))
    for rows in (1, 63, 64, 65, 128, 129):
        t.append(task(rng, 100, rows, 17))
        t.append(task(rng, 140, rows, 33, kind="periodic", period=3))
    for run in (63, 64, 65, 200):
        t.append(task(rng, run, run + 30, 9, kind="exact"))
        t.append(task(rng, run, run + 30, 64, kind="exact"))
    t.append(task(rng, 120, 170, 17, qs=9, qe=100))
    t.append(task(rng, 120, 170, 32, qs=1, qe=118, kind="split"))
    t.append(task(rng, 100, 140, 40, shift=39))                      # band_l far below minus the left flank: clipped at the left
    t.append(task(rng, 100, 140, 40, shift=0))
    t.append(task(rng, 90, 130, 20, n_read=True, n_win=True))
    t.append(task(rng, 90, 130, 20, kind="miss"))
    t.append(task(rng, 400, 460, 64, kind="split", nindel=2))
    for nd in (2, 17, 33, 64):                                       # band_l inside the read: the band's first column advances row by row
        t.append(task(rng, 200, 110, nd, qoff=61, nindel=1 if nd > 2 else 0))
    t.append(task(rng, 180, 90, 40, qoff=53, kind="periodic", period=5, shift=20))
    return t


def wave_cases(rng, N):
    """bands of 128 (N - 1) + 1 and 128 N diagonals (one band for WAVE2: 129 would be the same instance's lower edge)"""
    t = []
    widths = [128 * N] if N == 2 else [128 * (N - 1) + 1, 128 * N]
    for nd in widths:
        ql = nd + 260
        t.append(task(rng, ql, 300, nd, nindel=3, shift=nd // 2))
        t.append(task(rng, ql, 260, nd, kind="split", shift=nd // 2))
        t.append(task(rng, ql, 200, nd, kind="periodic", period=2 + N % 6, shift=nd // 2))
    t.append(task(rng, 128 * N + 200, 129, 128 * N, shift=128 * N - 20))       # clipped at the left
    t.append(task(rng, 128 * N + 500, 150, 128 * N, qoff=128 * N // 2 + 101, shift=128 * N // 2, nindel=2))      # band_l inside the read
    t.append(task(rng, 128 * N + 400, 100, 128 * (N - 1) + 1, qoff=64 * N + 77, shift=64 * (N - 1), kind="periodic", period=3))
    return t


def strip_cases(rng, form):
    t = []
    if form == STRIP8:                       # strips of 512 columns; 1, 2 and 3 strips; j0 on and off a multiple of 8
        for nd, ql, wl, sh in ((256, 500, 200, 128), (511, 900, 300, 250), (512, 1100, 300, 256), (513, 1100, 320, 255), (2047, 2300, 200, 1000),
                               (300, 420, 100, 150), (700, 1500, 700, 349)):
            t.append(task(rng, ql, wl, nd, nindel=3, shift=sh))
            t.append(task(rng, ql, wl, nd, kind="split", shift=sh + 1))
        for nd, ql, wl, sh in ((256, 400, 129, 100), (512, 700, 64, 300), (600, 1300, 65, 290), (1030, 1290, 63, 515)):
            t.append(task(rng, ql, wl, nd, kind="exact", shift=sh))
        t.append(task(rng, 1300, 300, 300, qoff=503, shift=150, nindel=2))                    # band_l inside the read, j0 off a multiple of 8
        t.append(task(rng, 1500, 200, 520, qoff=701, shift=260, kind="periodic", period=6))
        t.append(task(rng, 900, 400, 400, kind="split", shift=203))
        t.append(task(rng, 800, 300, 380, kind="periodic", period=5, shift=190))
        t.append(task(rng, 1200, 500, 600, kind="periodic", period=7, shift=301, qs=3, qe=1190))
    else:                                    # strips of 1024 columns on reads of about 2300 bases
        t.append(task(rng, 2300, 2500, 2048, nindel=6, shift=1024))
        t.append(task(rng, 2300, 2500, 2100, kind="split", shift=1050))
        t.append(task(rng, 2290, 300, 2100, kind="periodic", period=6, shift=1000))
        t.append(task(rng, 2301, 150, 2048, nindel=2, shift=1029, qs=5, qe=2295))
        t.append(task(rng, 4400, 200, 2060, qoff=2211, shift=1030, nindel=2))                 # band_l inside the read
    return t


def scalar_cases(rng):
    return [task(rng, 60, 90, 9, nindel=1), task(rng, 150, 200, 70, kind="split"), task(rng, 100, 130, 20, kind="periodic", period=4),
            task(rng, 60, 40, 5, kind="whole"), task(rng, 200, 129, 150, nindel=2, shift=140), task(rng, 80, 100, 10, kind="miss"), task(rng, 90, 64, 17),
            task(rng, 300, 340, 130, nindel=2, shift=60), task(rng, 120, 150, 1, kind="exact"), task(rng, 100, 150, 25, qs=4, qe=90),
            task(rng, 130, 170, 64, kind="periodic", period=7), task(rng, 70, 65, 33, n_read=True, n_win=True),
            task(rng, 200, 100, 21, qoff=71, nindel=1)]


def common_cases(rng):
    """a small set every form can run: compared form against form (wide forms take it with a band they accept)"""
    return [task(rng, 150, 200, 30, nindel=1), task(rng, 150, 200, 33, kind="split"), task(rng, 120, 170, 40, kind="periodic", period=3),
            task(rng, 100, 64, 17), task(rng, 64, 100, 12, kind="exact")]


def cases_of(form, seed):
    rng = np.random.default_rng(1000 + 17 * form + seed)
    if form in (ROWS, ANTIDIAG):
        return narrow_cases(rng)
    if form in WAVE_SLOTS:
        return wave_cases(rng, WAVE_SLOTS[form])
    if form in (STRIP8, STRIP16):
        return strip_cases(rng, form)
    return scalar_cases(rng)


K2B_QLENS = [20, 255, 256, 1023, 1024, 1025, 2100]


def k2b_cases(rng, ql):
    """K2b tasks of one read length: bands of 1 to 1100 diagonals (strips of 1024 columns: 1, 2 and 3 strips at the longer reads), a
    band wider than the read, band_r < band_l (whole matrix; the window no longer than the read: past it the one-lane pass, like the
    reference, looks beyond its row buffers), band_l far below minus the left flank (clipped at the left: the band's first column
    never advances) and inside the read, qs > 0 and qe < qlen - 1, a band that misses the read, windows of 1 to 129 rows, N."""
    t = []
    for nd in (1, 2, 17, 64, 65, 300, 1100):
        t.append(task(rng, ql, ql + int(rng.integers(0, 60)), nd, nindel=2 if nd >= 17 else 0))
    t.append(task(rng, ql, ql + 40, ql + 50, nindel=1))
    t.append(task(rng, ql, max(1, ql - 3), 9, kind="whole"))
    t.append(task(rng, ql, ql + 30, 40, shift=39, nindel=1))
    t.append(task(rng, ql, max(1, ql // 2), 30, qoff=ql // 3, shift=3))
    t.append(task(rng, ql, ql + 25, 21, qs=min(7, ql - 2), qe=ql - 4, nindel=1))
    t.append(task(rng, ql, ql + 11, 12, kind="miss"))
    for rows in (1, 63, 64, 65, 129):
        t.append(task(rng, ql, rows, 17, qoff=min(ql // 4, max(0, ql - rows))))
    t.append(task(rng, ql, ql + 17, 33, n_read=True, n_win=True, nindel=1))
    t.append(task(rng, ql, ql + 9, 18, kind="periodic", period=2 + ql % 6))
    return t


def minscore_of(pen):
    return 8 * pen[0]


def open_mapper(tmp_dir, qmax=2400):
    """an index over a random sequence and a mapper for reads up to qmax bases (the stand-alone entries use its stream and its
    strip buffers only); returns (index, mapper, close)"""
    from smalt_amd import api
    rng = np.random.default_rng(7)
    seqs = [bytes(rng.choice(list(b"ACGT"), size=4000).astype(np.uint8))]
    oix = ol.build_index(seqs, ["s"], 11, 3)
    pre = str(tmp_dir / "x")
    ol.lib().or_index_write(oix, pre.encode())
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, 16, qmax)

    def close():
        mp.close()
        gix.close()
        ol.lib().or_index_free(oix)
    return gix, mp, close


def params_of(gix, pen):
    par = gix.default_params()
    par.match, par.mismatch, par.gap_init, par.gap_ext = pen
    return par

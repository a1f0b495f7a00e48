"""The lane hand-over of the packed K2a sweep as one v_cndmask_b32 with a DPP source, and the window entries kept as code
pair x 8 behind one row pointer per lane, through smaltgpu_sw_full_batch against the oracle's textbook Gotoh.

The shapes are the smallest at which the two can go wrong:
 * read lengths C - 1, C, C + 1, 2 C and G C: a lane's first and last column on a group's edge, and the padding columns;
 * window lengths 1, G - 1, G and four consecutive ones, every launch with windows of one length only (a wave iteration sweeps
   as far as its longest window), so that the sweep's step count takes every remainder of the four-row body;
 * 1, 2 and 2 (64 / G) + 1 tasks: a lone task in the low half of a lane group, a full pair, and a full wave iteration
   followed by a partly filled one; with G = 4 and 8 a group's first lane is lane 0, 4, 8 or 12 of a 16-lane DPP row;
 * a read equal to its window and one that matches nowhere: the first lane's floors and the maxima at both ends;
 * windows of N in both tasks of a pair: the code pair 5 | 5 << 3, the largest entry the sweep reads (x 8 = 360).
With the default penalties every launch runs three times, by the hooks of tests/test_gpu_sw_pairframe.py: pair frame, row frame,
half-float form.  One more set each runs in the row frame, in the half-float form and in the integer form by itself; the
pair-frame test has no set for the integer form (all of its scores are half floats with a zero low byte), so this one takes
a mismatch of -9."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROW_HOOK, PAIR_HOOK = "SMALTGPU_SW16_ROWFRAME", "SMALTGPU_SW16_PAIRFRAME"
TILINGS = [(4, 16), (8, 13), (8, 19), (8, 20), (16, 16), (16, 32)]
PENS = [((1, -2, -4, -3), "pair"),       # the default penalties: pair frame, and the other forms by the hooks
        ((3, -6, -8, -4), "row"),        # match + 2 ge = 11: row frame
        ((5, -4, -8, -6), "half"),       # match + ge = 11: half-float form without a frame
        ((2, -9, -5, -2), "int")]        # mismatch -9: four significant bits, no half-float form: integer form


@pytest.fixture(scope="module")
def raw_mapper(oracle_built, tmp_path_factory):
    from smalt_amd import api
    rng = np.random.default_rng(7)
    seqs = [bytes(rng.choice(list(b"ACGT"), size=4000).astype(np.uint8))]
    oix = ol.build_index(seqs, ["s"], 11, 3)
    pre = str(tmp_path_factory.mktemp("handover") / "x")
    ol.lib().or_index_write(oix, pre.encode())
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, 16, 512)
    yield gix, mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


def _window(rng, q, wl):
    """wl bases that hold the read (or its head) with a few substitutions"""
    w = rng.integers(0, 4, size=wl, dtype=np.uint8)
    n = min(len(q), wl)
    at = int(rng.integers(0, wl - n + 1))
    core = q[:n].copy()
    m = rng.random(n) < 0.05
    core[m] = (core[m] + 1) & 3
    w[at:at + n] = core
    return w


def _launches(rng, G, tile_c, wcap):
    """lists of (read, window) tasks, one list per launch; wcap: the longest window that still runs in the form the case is
    about (the edge cases cut theirs there: the read then equals its window over the window's length)"""
    gc = G * tile_c
    rq = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    qlens = [tile_c - 1, tile_c, tile_c + 1, 2 * tile_c, gc]
    out = []
    k = 0
    for wl in (1, G - 1, G, 40, 41, 42, 43):
        for ntask in (1, 2, 2 * (64 // G) + 1):
            t = []
            for i in range(ntask):
                q = rq(qlens[(i + k) % len(qlens)])
                t.append((q, _window(rng, q, wl)))
            # the longest read is in every full launch, so the tiling is the one asked for; the short launches get it as well
            if ntask <= 2:
                q = rq(gc)
                t[0] = (q, _window(rng, q, wl))
            out.append(t)
            k += 1
    # edge scores: match x length and 0, alone in a group's low half, as a pair, and in a partly filled iteration
    exact = lambda n: (lambda q: (q, q[:wcap].copy()))(rq(n))
    nomatch = lambda n, wl: (np.zeros(n, dtype=np.uint8), np.full(min(wl, wcap), 1, dtype=np.uint8))
    out.append([exact(gc)])
    out.append([nomatch(gc, gc)])
    out.append([exact(gc), nomatch(gc, 41)])
    t = []
    for i in range(2 * (64 // G) + 1):
        n = qlens[i % len(qlens)]
        t.append(exact(n) if i % 2 == 0 else nomatch(n, n + 1))
    t[0] = exact(gc)
    out.append(t)
    # the highest entry: N in both tasks of a pair, whole windows and runs inside a window that matches otherwise
    q0, q1 = rq(gc), rq(gc - 1)
    out.append([(q0, np.full(42, 5, dtype=np.uint8)), (q1, np.full(42, 5, dtype=np.uint8))])
    w0, w1 = q0.copy(), q1[:gc - 1].copy()
    w0[10:17] = 5
    w1[8:21] = 5
    w1 = np.concatenate([w1, rq(1)])
    out.append([(q0, w0[:wcap]), (q1, w1[:wcap]), (rq(tile_c + 1), np.full(min(gc, wcap), 5, dtype=np.uint8))])
    return out


@pytest.mark.parametrize("tiling", TILINGS, ids=lambda v: "G%dxC%d" % v)
@pytest.mark.parametrize("pen", PENS, ids=lambda v: v[1])
def test_handover_scores(pen, tiling, raw_mapper, monkeypatch):
    from smalt_amd import api
    gix, mp = raw_mapper
    G, tile_c = tiling
    (match, mismatch, gi, ge), form = pen
    par = gix.default_params()
    par.match, par.mismatch, par.gap_init, par.gap_ext = match, mismatch, gi, ge
    # the form the set is here for, and the longest sweep (window rows + G - 1 steps) that it takes
    psteps = api.lib().smaltgpu_sw_pairframe_max_steps(match, mismatch, gi, ge, G * tile_c)
    rsteps = api.lib().smaltgpu_sw_rowframe_max_steps(match, mismatch, gi, ge, G * tile_c)
    if form == "pair":
        limit = psteps
        assert rsteps >= psteps
    elif form == "row":
        limit = rsteps
        assert psteps < 0
    else:
        limit = 1 << 20
        assert psteps < 0 and rsteps < 0
    wcap = min(G * tile_c + 1, limit - (G - 1))
    assert wcap >= 43
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, match, mismatch)
    rng = np.random.default_rng(17 * G + 1000 * tile_c + match)
    monkeypatch.delenv(ROW_HOOK, raising=False)
    monkeypatch.delenv(PAIR_HOOK, raising=False)
    for tasks in _launches(rng, G, tile_c, wcap):
        qs, ws = [q.tobytes() for q, _ in tasks], [w.tobytes() for _, w in tasks]
        assert max(len(q) for q in qs) == G * tile_c and max(len(w) for w in ws) <= wcap
        exp = [ol.lib().or_sw_full(q, len(q), w, len(w), M, gi, ge) for q, w in zip(qs, ws)]
        got = mp.sw_full_batch(qs, ws, par, packed16=True)
        assert got == exp, (len(qs), [len(q) for q in qs], len(ws[0]), got, exp)
        if form == "pair":
            monkeypatch.setenv(PAIR_HOOK, "0")
            rowf = mp.sw_full_batch(qs, ws, par, packed16=True)
            monkeypatch.delenv(PAIR_HOOK, raising=False)
            monkeypatch.setenv(ROW_HOOK, "0")
            plain = mp.sw_full_batch(qs, ws, par, packed16=True)
            monkeypatch.delenv(ROW_HOOK, raising=False)
            assert rowf == exp and plain == exp, (len(qs), len(ws[0]), rowf, plain, exp)

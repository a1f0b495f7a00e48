"""The pair-frame form of the packed K2a sweep (sw16p_core) against the oracle's textbook Gotoh maximum and
against the forms it replaces: every case runs three times -- by default (pair frame, then row frame, then the plain
forms), with SMALTGPU_SW16_PAIRFRAME=0 (row frame, then the plain forms) and with SMALTGPU_SW16_ROWFRAME=0 (sw16f_core /
sw16_core only) -- and the three score arrays must be identical and equal to the oracle's.

The stand-alone kernel picks the form per wave iteration (16 / 8 / 4 task pairs) by the iteration's longest sweep, against
smaltgpu_sw_pairframe_max_steps() and smaltgpu_sw_rowframe_max_steps().  Each case holds windows on both sides of both
limits, ordered by the form they take, so that one launch runs all three."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROW_HOOK, PAIR_HOOK = "SMALTGPU_SW16_ROWFRAME", "SMALTGPU_SW16_PAIRFRAME"
TILINGS = [(4, 16), (8, 13), (8, 19), (8, 20), (16, 16), (16, 32)]
WMAX = 1016          # longest window of the stand-alone kernel
PENS = [(1, -2, -4, -3), (2, -3, -5, -2), (5, -4, -6, -1), (1, -1, -2, -1),      # pair frame
        (3, -6, -8, -4),     # match + 2 ge = 11: four significant bits, row frame only
        (1, -2, -8, -7),     # match + 2 ge = 15: row frame only
        (5, -4, -8, -6),     # match + ge = 11: no frame at all
        (6, -4, -8, -6)]     # match + 2 ge = 18 = 9 x 2: row frame only, and only for the shorter tilings


def _embed(rng, q, wl, rate=0.05):
    """A window of wl bases that holds the query (or its head), mutated."""
    w = rng.integers(0, 4, size=wl, dtype=np.uint8)
    n = min(len(q), wl)
    at = int(rng.integers(0, wl - n + 1))
    core = q[:n].copy()
    m = rng.random(n) < rate
    core[m] = (core[m] + 1) & 3
    w[at:at + n] = core
    return w


def _tasks(rng, G, tile_c, pmax, lmax):
    """About a hundred (query, window) tasks for tiling (G, tile_c); pmax, lmax: longest window that still runs in the pair
    frame and in the row frame (None: no window does)."""
    gc = G * tile_c
    rq = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    # padding that starts on an odd column, an even column and on a lane's first column
    qlens = [1, 2, tile_c - 1, tile_c, tile_c + 1, gc - 1, gc]
    wlens = [1, 2, G - 1, G, 100, 101, 102, 103]             # with the neighbours in the batch: odd and even sweeps, every tail
    edge = [l for m in (pmax, lmax) if m is not None for l in (m, m + 1) if 1 <= l <= WMAX]
    t = []
    # two tasks of a pair with very different windows (the pairs are tasks 2k, 2k + 1)
    far = min(pmax if pmax else (lmax if lmax else 249), WMAX)
    for a, b in ((1, far), (249, 2)):
        q = rq(gc)
        t.append((q, _embed(rng, q, a)))
        q = rq(gc - 1)
        t.append((q, _embed(rng, q, b)))
    for wl in wlens:
        for ql in qlens:
            q = rq(ql)
            t.append((q, _embed(rng, q, wl) if rng.random() < 0.8 else rq(wl)))
    for wl in edge:
        for ql in (1, tile_c + 1, gc - 1, gc):
            q = rq(ql)
            t.append((q, _embed(rng, q, wl)))
        q = rq(gc)                                            # the read at the window's end: the largest value in the last frames
        w = rq(wl)
        n = min(gc, wl)
        w[wl - n:] = q[gc - n:]
        t.append((q, w))
    # windows of N only, and with runs of N
    for wl in (1, 57, 248):
        t.append((rq(gc), np.full(wl, 5, dtype=np.uint8)))
    for _ in range(4):
        q = rq(int(rng.integers(tile_c, gc + 1)))
        w = _embed(rng, q, int(rng.integers(len(q), len(q) + 90)))
        for _ in range(int(rng.integers(1, 4))):
            at, n = int(rng.integers(0, len(w))), int(rng.integers(1, 21))
            w[at:at + n] = 5
        t.append((q, w))
    # read identical to the window: match x length, the largest value
    for ql in (gc, tile_c, 2):
        q = rq(ql)
        t.append((q, q.copy()))
    # no match at all / one match
    t.append((np.zeros(gc, dtype=np.uint8), np.full(200, 1, dtype=np.uint8)))
    w = np.full(200, 1, dtype=np.uint8)
    w[77] = 0
    t.append((np.zeros(gc - 1, dtype=np.uint8), w))
    # a long gap on either side: F crosses class wraps and lane boundaries, E runs through many rotations of the floors
    for gap in (12, 30, 60, tile_c + 3):
        h = gc // 2
        a, b = rq(h), rq(gc - h)
        t.append((np.concatenate([a, b]), np.concatenate([rq(5), a, rq(gap), b, rq(5)])))
        if gc - gap >= 8:
            h2 = (gc - gap) // 2
            a, b = rq(h2), rq(gc - gap - h2)
            t.append((np.concatenate([a, rq(gap), b]), np.concatenate([rq(5), a, b, rq(5)])))
    # random fill
    while len(t) < 108:
        q = rq(int(rng.integers(1, gc + 1)))
        wl = int(rng.integers(1, 300))
        t.append((q, _embed(rng, q, wl, rate=float(rng.choice([0.0, 0.02, 0.1, 0.3]))) if rng.random() < 0.8 else rq(wl)))
    # by the form they take: the iterations in front run in the pair frame, then the row frame, then the plain forms

    def form(x):
        wl = len(x[1])
        return 0 if (pmax is not None and wl <= pmax) else 1 if (lmax is not None and wl <= lmax) else 2
    t = [x for k in (0, 1, 2) for x in t if form(x) == k]
    if len(t) % 2 == 0:                       # an odd count: the last pair has a dead half
        q = rq(gc)
        t.append((q, _embed(rng, q, 100)))
    return [q.tobytes() for q, _ in t], [w.tobytes() for _, w in t]


@pytest.fixture(scope="module")
def raw_mapper(oracle_built, tmp_path_factory):
    from smalt_amd import api
    rng = np.random.default_rng(99)
    seqs = [bytes(rng.choice(list(b"ACGT"), size=4000).astype(np.uint8))]
    oix = ol.build_index(seqs, ["s"], 11, 3)
    pre = str(tmp_path_factory.mktemp("pairframe") / "x")
    ol.lib().or_index_write(oix, pre.encode())
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, 16, 512)
    yield gix, mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


def _three_ways(monkeypatch, run):
    monkeypatch.delenv(ROW_HOOK, raising=False)
    monkeypatch.delenv(PAIR_HOOK, raising=False)
    new = run()
    monkeypatch.setenv(PAIR_HOOK, "0")
    rowf = run()
    monkeypatch.delenv(PAIR_HOOK, raising=False)
    monkeypatch.setenv(ROW_HOOK, "0")
    old = run()
    return new, rowf, old


@pytest.mark.parametrize("tiling", TILINGS, ids=lambda v: "G%dxC%d" % v)
@pytest.mark.parametrize("pen", PENS, ids=lambda v: "m%d_x%d_g%d_e%d" % (v[0], -v[1], -v[2], -v[3]))
def test_pairframe_scores(pen, tiling, raw_mapper, monkeypatch):
    from smalt_amd import api
    gix, mp = raw_mapper
    G, tile_c = tiling
    match, mismatch, gi, ge = pen
    par = gix.default_params()
    par.match, par.mismatch, par.gap_init, par.gap_ext = match, mismatch, gi, ge
    psteps = api.lib().smaltgpu_sw_pairframe_max_steps(match, mismatch, gi, ge, G * tile_c)
    rsteps = api.lib().smaltgpu_sw_rowframe_max_steps(match, mismatch, gi, ge, G * tile_c)
    pmax = psteps - (G - 1) if psteps >= G else None
    lmax = rsteps - (G - 1) if rsteps >= G else None
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, match, mismatch)
    rng = np.random.default_rng(11 * G + 1000 * tile_c + 31 * match - ge)
    qs, ws = _tasks(rng, G, tile_c, pmax, lmax)
    assert len(qs) % 2 == 1 and max(len(q) for q in qs) == G * tile_c
    for m in (pmax, lmax):
        if m is not None and m < WMAX:
            assert any(len(w) == m for w in ws) and any(len(w) == m + 1 for w in ws)
    new, rowf, old = _three_ways(monkeypatch, lambda: mp.sw_full_batch(qs, ws, par, packed16=True))
    exp = [ol.lib().or_sw_full(q, len(q), w, len(w), M, gi, ge) for q, w in zip(qs, ws)]
    for i, (q, w) in enumerate(zip(qs, ws)):
        assert new[i] == exp[i], (i, len(q), len(w), new[i], exp[i])
    assert new == rowf
    assert new == old


@pytest.mark.parametrize("tiling", TILINGS, ids=lambda v: "G%dxC%d" % v)
def test_every_number_of_rows_left_over(tiling, raw_mapper, monkeypatch):
    """The loop body is four rows and a single-row loop does the rest: launches whose windows all have one length, for four
    consecutive lengths, so that the sweep's step count takes every remainder (the batch above leaves that to chance, a
    wave iteration sweeps as far as its longest window), and one sweep shorter than a body."""
    gix, mp = raw_mapper
    G, tile_c = tiling
    par = gix.default_params()
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, par.match, par.mismatch)
    rng = np.random.default_rng(5 * G + tile_c)
    for wl in (1, 2, 3, 40, 41, 42, 43):
        qs, ws = [], []
        for ql in (G * tile_c, G * tile_c - 1, tile_c + 1, 2, G * tile_c):
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)
            qs.append(q.tobytes())
            ws.append(_embed(rng, q, wl).tobytes())
        new, rowf, old = _three_ways(monkeypatch, lambda: mp.sw_full_batch(qs, ws, par, packed16=True))
        exp = [ol.lib().or_sw_full(q, len(q), w, len(w), M, par.gap_init, par.gap_ext) for q, w in zip(qs, ws)]
        assert new == exp, (wl, new, exp)
        assert new == rowf and new == old


def test_pairframe_limits_as_documented():
    """The figures the cases above rely on."""
    from smalt_amd import api
    f = api.lib().smaltgpu_sw_pairframe_max_steps
    assert f(1, -2, -4, -3, 152) == 625                       # (2040 - 4 - 152) / 3 - 3
    assert f(1, -2, -4, -3, 512) == 505
    assert f(5, -4, -6, -1, 152) == 1271
    assert f(3, -6, -8, -4, 152) == -1 and f(1, -2, -8, -7, 152) == -1 and f(6, -4, -8, -6, 152) == -1    # low byte of f16(11), (15), (18)
    assert f(5, -4, -8, -6, 152) == -1                        # no row frame either


def _map_golden(fx, reads, entry):
    from smalt_amd import api
    from test_gpu_golden import params_from_opts
    ix = api.Index.load(fx["prefix"], 0)
    mp = api.Mapper(ix, len(reads), max(len(r[1]) for r in reads))
    try:
        mp.set_debug(2)
        res, stats = mp.map_batch([r[1] for r in reads], [r[2] for r in reads], params_from_opts(ix, entry["opts"]))
        dump = "".join(mp.dump_read(i, reads[i][0]) for i in range(len(reads)))
    finally:
        mp.close()
        ix.close()
    return res, stats, dump


def test_mapper_output_is_the_same_in_all_three_forms(oracle_built, tmp_path, monkeypatch):
    """The smallest golden fixture whose candidates go through k_sw_full16, through the mapper in the three settings:
    results, per-read scalars and the stage dumps are identical and equal to the fixture."""
    entry = [e for e in gu.MANIFEST if e["tag"] == "g_k13s6_hash"][0]
    fx = gu.unpack(entry, tmp_path)
    reads = gu.read_fastq(fx["fq"])
    new, rowf, old = _three_ways(monkeypatch, lambda: _map_golden(fx, reads, entry))
    assert sum(len(r) for r in new[0]) > 0
    for other in (rowf, old):
        assert new[0] == other[0]
        assert new[1] == other[1]
        assert new[2] == other[2]
    assert new[2] == fx["expected"]

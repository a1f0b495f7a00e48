"""The row-frame form of the packed K2a sweep (sw16r_core) against the oracle's textbook Gotoh maximum and
against the forms it replaces: every case runs a second time with SMALTGPU_SW16_ROWFRAME=0 (sw16f_core / sw16_core), and
the two score arrays must be identical.

The stand-alone kernel picks the form per wave iteration (16 / 8 / 4 task pairs): the row frame when the iteration's
longest sweep stays within smaltgpu_sw_rowframe_max_steps().  Each case holds windows on both sides of that limit, the
longer ones at the end of the batch, so both sides of the choice run in one launch."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import oracle_lib as ol

pytestmark = pytest.mark.gpu

HOOK = "SMALTGPU_SW16_ROWFRAME"
TILINGS = [(4, 16), (8, 13), (8, 19), (8, 20), (16, 16), (16, 32)]
WMAX = 1016          # longest window of the stand-alone kernel
PENS = [(1, -2, -4, -3), (2, -3, -5, -2), (5, -4, -6, -1), (1, -1, -2, -1), (3, -6, -8, -4),   # the half-float sets of test_gpu_sw.py
        (1, -2, -8, -7),     # values near 1940 at 255 rows: close to the bound
        (5, -4, -8, -6),     # match + ge = 11: four significant bits, no row frame at all
        (6, -4, -8, -6)]     # table fits, range does not: 6 x 152 columns leave 185 steps, 6 x 256 leave 81, 6 x 512 none


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


def _tasks(rng, G, tile_c, lmax):
    """About a hundred (query, window) tasks for tiling (G, tile_c); lmax: longest window that still runs in the row frame
    (None: no window does)."""
    gc = G * tile_c
    rq = lambda n: rng.integers(0, 4, size=n, dtype=np.uint8)
    qlens = [1, tile_c, gc - 1, gc]
    wlens = [1, G - 1, 247, 248, 249]
    edge = [] if lmax is None else [l for l in (lmax, lmax + 1) if 1 <= l <= WMAX]
    t = []
    # two tasks of a pair with very different windows (the pairs are tasks 2k, 2k + 1)
    far = min(lmax, WMAX) if lmax else 249
    for a, b in ((1, far), (249, 2)):
        q = rq(gc)
        t.append((q, _embed(rng, q, a)))
        q = rq(gc - 1)
        t.append((q, _embed(rng, q, b)))
    for wl in wlens + edge:
        for ql in qlens:
            q = rq(ql)
            t.append((q, _embed(rng, q, wl) if rng.random() < 0.8 else rq(wl)))
    # windows of N only, and with runs of N
    for wl in (1, 57, 248):
        t.append((rq(gc), np.full(wl, 5, dtype=np.uint8)))
    for _ in range(6):
        q = rq(int(rng.integers(tile_c, gc + 1)))
        w = _embed(rng, q, int(rng.integers(len(q), len(q) + 90)))
        for _ in range(int(rng.integers(1, 4))):
            at, n = int(rng.integers(0, len(w))), int(rng.integers(1, 21))
            w[at:at + n] = 5
        t.append((q, w))
    # read identical to the window: match x length, the largest value
    for ql in (gc, tile_c):
        q = rq(ql)
        t.append((q, q.copy()))
    # no match at all / one match
    t.append((np.zeros(gc, dtype=np.uint8), np.full(200, 1, dtype=np.uint8)))
    w = np.full(200, 1, dtype=np.uint8)
    w[77] = 0
    t.append((np.zeros(gc - 1, dtype=np.uint8), w))
    # a long gap on either side: E and F run for tens of cells
    for gap in (12, 30, 60):
        h = gc // 2
        a, b = rq(h), rq(gc - h)
        t.append((np.concatenate([a, b]), np.concatenate([rq(5), a, rq(gap), b, rq(5)])))
        if gc - gap >= 8:
            h2 = (gc - gap) // 2
            a, b = rq(h2), rq(gc - gap - h2)
            t.append((np.concatenate([a, rq(gap), b]), np.concatenate([rq(5), a, b, rq(5)])))
    # random fill
    while len(t) < 98:
        q = rq(int(rng.integers(1, gc + 1)))
        wl = int(rng.integers(1, 300))
        t.append((q, _embed(rng, q, wl, rate=float(rng.choice([0.0, 0.02, 0.1, 0.3]))) if rng.random() < 0.8 else rq(wl)))
    # windows beyond the limit go last, so that the iterations in front of them run in the row frame
    if lmax is not None:
        t = [x for x in t if len(x[1]) <= lmax] + [x for x in t if len(x[1]) > lmax]
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
    pre = str(tmp_path_factory.mktemp("rowframe") / "x")
    ol.lib().or_index_write(oix, pre.encode())
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, 16, 512)
    yield gix, mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


@pytest.mark.parametrize("tiling", TILINGS, ids=lambda v: "G%dxC%d" % v)
@pytest.mark.parametrize("pen", PENS, ids=lambda v: "m%d_x%d_g%d_e%d" % (v[0], -v[1], -v[2], -v[3]))
def test_rowframe_scores(pen, tiling, raw_mapper, monkeypatch):
    from smalt_amd import api
    gix, mp = raw_mapper
    G, tile_c = tiling
    match, mismatch, gi, ge = pen
    par = gix.default_params()
    par.match, par.mismatch, par.gap_init, par.gap_ext = match, mismatch, gi, ge
    steps = api.lib().smaltgpu_sw_rowframe_max_steps(match, mismatch, gi, ge, G * tile_c)
    lmax = steps - (G - 1) if steps >= G else None
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, match, mismatch)
    rng = np.random.default_rng(7 * G + 1000 * tile_c + 31 * match - ge)
    qs, ws = _tasks(rng, G, tile_c, lmax)
    assert len(qs) % 2 == 1 and max(len(q) for q in qs) == G * tile_c
    if lmax is not None and lmax < WMAX:
        assert any(len(w) == lmax for w in ws) and any(len(w) == lmax + 1 for w in ws)
    monkeypatch.delenv(HOOK, raising=False)
    got = mp.sw_full_batch(qs, ws, par, packed16=True)
    monkeypatch.setenv(HOOK, "0")
    old = mp.sw_full_batch(qs, ws, par, packed16=True)
    exp = [ol.lib().or_sw_full(q, len(q), w, len(w), M, gi, ge) for q, w in zip(qs, ws)]
    for i, (q, w) in enumerate(zip(qs, ws)):
        assert got[i] == exp[i], (i, len(q), len(w), got[i], exp[i])
    assert got == old


def test_rowframe_limits_as_documented():
    """The figures the cases above rely on."""
    from smalt_amd import api
    f = api.lib().smaltgpu_sw_rowframe_max_steps
    assert f(1, -2, -4, -3, 152) == 627                       # (2040 - 4 - 152) / 3 - 1
    assert f(1, -2, -8, -7, 152) == 267
    assert f(5, -4, -8, -6, 152) == -1                        # low byte of f16(11)
    assert f(6, -4, -8, -6, 152) == 185 and f(6, -4, -8, -6, 256) == 81 and f(6, -4, -8, -6, 512) == -1


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


def test_mapper_output_is_the_same_in_both_forms(oracle_built, tmp_path, monkeypatch):
    """The smallest golden fixture whose candidates go through k_sw_full16, through the mapper in both forms: results,
    per-read scalars and the stage dumps are identical (tests/test_gpu_golden.py pins the default to the reference)."""
    entry = [e for e in gu.MANIFEST if e["tag"] == "g_k13s6_hash"][0]
    fx = gu.unpack(entry, tmp_path)
    reads = gu.read_fastq(fx["fq"])
    monkeypatch.delenv(HOOK, raising=False)
    new = _map_golden(fx, reads, entry)
    monkeypatch.setenv(HOOK, "0")
    old = _map_golden(fx, reads, entry)
    assert sum(len(r) for r in new[0]) > 0
    assert new[0] == old[0]
    assert new[1] == old[1]
    assert new[2] == old[2]
    assert new[2] == fx["expected"]

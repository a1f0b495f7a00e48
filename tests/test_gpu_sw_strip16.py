"""The packed strip kernel (sw_strip16_core: two tasks per wave in 16-bit halves, strips of 64 lanes x 16 columns, the boundary
column handed from strip to strip through a ring that is read ahead 64 rows at a time and written back in blocks of 64 of its
128 rows) through smaltgpu_sw_full_batch(packed16 = 1) beyond the register tiling, every score against the oracle's textbook
Gotoh.  Production reaches this kernel only through whole reads of more than 512 bases, and its plain-maximum instance
(M3 = false: longest read x match + 512 >= 0x7C00) only with reads above 2083 bases at match = 15.

Shapes: the smallest that cross each boundary of the code -- reads of 1023 to 2049 bases (1, 2 and 3 strips, a strip's last
column, the first of the next) paired with a read of their own length and with a 40-base partner (the shorter task idles);
windows of 1 to 200 rows around the ring's 64 and 128 and the pairs (1, 129), (129, 1); an odd task count; short reads with
windows above 1016; N in a window; N in one read of a pair (-2, the partner exact); a window above the mapper's capacity (-1)."""
import numpy as np
import pytest

import band_data as bd
import oracle_lib as ol

pytestmark = pytest.mark.gpu

QMAX = 2400
WINCAP = 4 * ((QMAX + 8 + 7) & ~7) + 1024       # the mapper's window capacity: four times its read capacity (rounded up to 8) + 1024


@pytest.fixture(scope="module")
def raw_mapper(oracle_built, tmp_path_factory):
    gix, mp, close = bd.open_mapper(tmp_path_factory.mktemp("strip16"), QMAX)
    yield gix, mp
    close()


def _window(rng, q, wl):
    """wl bases that hold the read (or its head) with a few substitutions (test_gpu_sw_handover._window)"""
    w = rng.integers(0, 4, size=wl, dtype=np.uint8)
    n = min(len(q), wl)
    at = int(rng.integers(0, wl - n + 1))
    core = q[:n].copy()
    m = rng.random(n) < 0.05
    core[m] = (core[m] + 1) & 3
    w[at:at + n] = core
    return w


def _launches(rng):
    t = lambda ql, wl: (lambda q: (q, _window(rng, q, wl)))(bd.rq(rng, ql))
    out = []
    a = []
    for L in (1023, 1024, 1025, 2048, 2049):            # strips of 1024 columns
        a += [t(L, L + 30), t(L, L + 17), t(L, L + 5), t(40, 200)]
    out.append(a)
    b = []
    for wl in (1, 63, 64, 65, 127, 128, 129, 200):      # the ring: chunks of 64 rows read ahead, 128 rows written back
        b += [t(1025, wl), t(600, wl)]
    b += [t(1025, 1), t(1030, 129), t(1100, 129), t(1025, 1), t(1500, 65)]      # odd count: the last task has no partner
    out.append(b)
    c = [t(513, 1017), t(300, 1500), t(64, 3000), t(512, 1017), t(20, 1018)]    # short reads, windows beyond the register tiling
    for q, w in c[:3]:
        w[[5, len(w) // 2, len(w) - 1]] = 5                                      # N inside a window
    out.append(c)
    q = bd.periodic(rng, 1200, 5)
    out.append([(q, np.resize(q[:5], 1400).astype(np.uint8)), t(1100, 1300), t(700, 1), t(1, 700)])
    return out


def _expect(tasks, pen, M):
    return [ol.lib().or_sw_full(q.tobytes(), len(q), w.tobytes(), len(w), M, pen[2], pen[3]) for q, w in tasks]


@pytest.mark.parametrize("pen", [(1, -2, -4, -3), (2, -3, -5, -2)], ids=["m1_x2_g4_e3", "m2_x3_g5_e2"])
def test_packed_strip_scores_max3_form(pen, raw_mapper):
    gix, mp = raw_mapper
    par = bd.params_of(gix, pen)
    M = bd.score_matrix(pen[0], pen[1])
    rng = np.random.default_rng(160 + pen[0])
    for tasks in _launches(rng):
        assert max(len(q) for q, _ in tasks) * pen[0] + 512 < 0x7C00
        assert max(len(q) for q, _ in tasks) > 512 or max(len(w) for _, w in tasks) > 1016
        exp = _expect(tasks, pen, M)
        got = mp.sw_full_batch([q.tobytes() for q, _ in tasks], [w.tobytes() for _, w in tasks], par, packed16=True)
        assert got == exp, ([(len(q), len(w)) for q, w in tasks], got, exp)
        assert max(exp) > 0


def test_packed_strip_scores_plain_maximum_form(raw_mapper):
    """(15, -14, -20, -10) on reads of 2100 to 2300 bases: 15 x 2300 + 512 passes 0x7C00, so the instance without the packed
    maximum of three runs; the exact copy scores 15 x its length, above 0x7C00 itself"""
    gix, mp = raw_mapper
    pen = (15, -14, -20, -10)
    par = bd.params_of(gix, pen)
    M = bd.score_matrix(pen[0], pen[1])
    rng = np.random.default_rng(1615)
    qe = bd.rq(rng, 2300)
    tasks = [(qe, np.concatenate([bd.rq(rng, 31), qe, bd.rq(rng, 50)])), (lambda q: (q, _window(rng, q, 2400)))(bd.rq(rng, 2100)),
             (lambda q: (q, _window(rng, q, 2250)))(bd.rq(rng, 2200)), (lambda q: (q, _window(rng, q, 129)))(bd.rq(rng, 2299)),
             (lambda q: (q, _window(rng, q, 2300)))(bd.rq(rng, 2250))]
    assert max(len(q) for q, _ in tasks) * pen[0] + 512 >= 0x7C00
    exp = _expect(tasks, pen, M)
    assert exp[0] == 15 * 2300 and exp[0] > 0x7C00
    got = mp.sw_full_batch([q.tobytes() for q, _ in tasks], [w.tobytes() for _, w in tasks], par, packed16=True)
    assert got == exp, (got, exp)


def test_packed_strip_n_in_a_read_and_window_above_capacity(raw_mapper):
    """N in one read of a pair: that task reports -2 and its partner is exact; a window above the mapper's window capacity
    reports -1 and its partner is exact; one of exactly that length is scored"""
    gix, mp = raw_mapper
    pen = (1, -2, -4, -3)
    par = bd.params_of(gix, pen)
    M = bd.score_matrix(pen[0], pen[1])
    rng = np.random.default_rng(1616)
    t = lambda ql, wl: (lambda q: (q, _window(rng, q, wl)))(bd.rq(rng, ql))
    tasks = [t(1025, 1100), t(1025, 1100), t(700, 900), t(1300, 1400), t(600, WINCAP + 1), t(900, 1000), t(800, WINCAP)]
    tasks[0][0][1024] = 5
    tasks[3][0][0] = 5
    exp = _expect(tasks, pen, M)
    got = mp.sw_full_batch([q.tobytes() for q, _ in tasks], [w.tobytes() for _, w in tasks], par, packed16=True)
    assert got == [-2, exp[1], exp[2], -2, -1, exp[5], exp[6]], (got, exp)


def test_packed_strip_refuses_scores_beyond_16_bits(raw_mapper):
    """no fall-back to the 32-bit kernel: penalties outside the packed kernel's range, and match x longest read >= 60000"""
    from smalt_amd import api
    gix, mp = raw_mapper
    rng = np.random.default_rng(1617)
    for pen, ql in (((70, -14, -20, -10), 600), ((15, -14, -20, -10), 4000), ((1, -300, -4, -3), 600)):
        q = bd.rq(rng, ql)
        with pytest.raises(api.SmaltGpuError):
            mp.sw_full_batch([q.tobytes()], [q[:300].tobytes()], bd.params_of(gix, pen), packed16=True)
    q = bd.rq(rng, 3999)                                   # 15 x 3999 = 59985: still in range
    pen = (15, -14, -20, -10)
    got = mp.sw_full_batch([q.tobytes()], [q[100:400].tobytes()], bd.params_of(gix, pen), packed16=True)
    assert got == [15 * 300]

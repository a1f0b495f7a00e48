"""A numpy float16 model of the pair-frame sweep of the packed K2a kernel (sw16p_core) as the lanes run it:
G lanes of C columns, lane g one row behind lane g - 1, a value of row r in a lane's column cc kept as X + ge * (r + (cc & 1)),
the three tables (plain, + ge for column 0 of an odd C, + 2 ge for odd columns), the F chain with its add on every other
column, the hand-over of H and F, the first lane's boundary, the two running maxima and the start-up values.  Its best
scores are compared with the oracle's plain integer Gotoh, and every intermediate value must be an integer of magnitude
<= 2048 (exact in half floats) for sweeps up to the length that the library admits to the form."""
import numpy as np
import pytest

from test_sw_rowframe_model import Track, gotoh, random_tasks
from test_sw_rowframe_model import max_steps_py as rowframe_steps_py

F16 = np.float16
PAD = 9          # column beyond the read: the selector of the constant 0
ADMITTED = [(1, -2, -4, -3), (2, -3, -5, -2), (5, -4, -6, -1), (1, -1, -2, -1), (2, -2, -6, -2), (4, -4, -10, -4)]
ROW_FRAME_ONLY = [(3, -6, -8, -4), (1, -2, -8, -7), (6, -4, -8, -6)]      # 11, 15, 18 = 9 * 2: four significant bits
NEITHER = [(5, -4, -8, -6), (9, -7, -9, -3), (1, -2, -3, -4), (13, -2, -4, -3)]


def max_steps_py(match, mismatch, gap_init, gap_ext, ncols):
    """The rule of DESIGN 4.1 spelled out: the row frame's conditions, match + 2 ge and mismatch + 2 ge with at most three
    significant bits as well, and match * ncols + ge * (steps + 3) + gi <= 2040."""
    if rowframe_steps_py(match, mismatch, gap_init, gap_ext, ncols) < 0:
        return -1
    gi, ge = -gap_init, -gap_ext
    for v in (match + 2 * ge, mismatch + 2 * ge, 2 * ge):
        a = abs(v)
        while a and a % 2 == 0:
            a //= 2
        if a > 7:
            return -1
    if ge == 0:
        return 0x7fffffff
    n = -1
    while match * ncols + ge * (n + 4) + gi <= 2040:
        n += 1
    return n


def pairframe_sweep(qs, ws, pen, G, tile_c, track):
    """Best scores of the tasks (all in one sweep of max window + G - 1 steps, as the tasks of a wave)."""
    match, mismatch, gi, ge = pen[0], pen[1], -pen[2], -pen[3]
    T, ncol = len(qs), G * tile_c
    nstep = max(len(w) for w in ws) + G - 1
    Q = np.full((T, ncol), PAD, dtype=np.int64)
    W = np.full((T, nstep + G), 5, dtype=np.int64)              # rows beyond the window: N
    for t, (q, w) in enumerate(zip(qs, ws)):
        Q[t, :len(q)] = np.frombuffer(q, dtype=np.uint8)
        W[t, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    wlen = np.array([len(w) for w in ws])
    Q = Q.reshape(T, G, tile_c)
    pl = (tile_c - 1) & 1                                        # class of a lane's last column
    pge, pge2, nge, nge2, ngo = F16(ge), F16(2 * ge), F16(-ge), F16(-2 * ge), F16(-(gi - ge))
    lane = np.arange(G)
    n0 = np.broadcast_to((pge * (-lane).astype(F16)).astype(F16), (T, G)).copy()         # floors of the row a lane does next: -g
    n1 = track(n0 + pge)
    n2 = track(n1 + pge)
    ma, mb = track(n0 - pge), n0.copy()                          # maxima of class 0 and class 1 of the row before
    H = np.empty((T, G, tile_c), dtype=F16)
    E = np.empty((T, G, tile_c), dtype=F16)
    H[:, :, 0::2], H[:, :, 1::2] = ma[:, :, None], mb[:, :, None]
    E[:, :, 0::2], E[:, :, 1::2] = n0[:, :, None], n1[:, :, None]
    F = ma.copy()
    prev_hl = (mb if pl else ma).copy()
    shift = [0, 2 * ge]                                          # what the table of a column's class adds to the scores
    for step in range(nstep):
        r = step - lane                                                                  # row of every lane
        inside = (r[None, :] >= 0) & (r[None, :] < wlen[:, None])
        wc = np.where(inside, W[np.arange(T)[:, None], np.clip(r, 0, None)[None, :]], 5)
        f0, f1, f2 = n0, n1, n2
        c0, c1 = mb, track(ma + pge2)                            # class 0 takes over the register of class 1, and back
        hl = np.concatenate([(f1 if pl else f0)[:, :1], H[:, :-1, tile_c - 1]], axis=1)  # the left neighbour's, same row
        fin = np.concatenate([f0[:, :1], F[:, :-1]], axis=1)
        carry, prev_hl, F = prev_hl, hl, fin
        Hold = H.copy()
        for cc in range(tile_c):
            odd = cc & 1
            sh = (0 if pl else ge) if cc == 0 else shift[odd]
            qc = Q[:, :, cc]
            s = np.where(qc == PAD, 0, np.where(wc >= 4, sh, np.where(qc == wc, match + sh, mismatch + sh))).astype(F16)
            dg = carry if cc == 0 else Hold[:, :, cc - 1]
            t = track(dg + s)
            hh = np.maximum(np.maximum(t, E[:, :, cc]), F)
            tt = track(hh + ngo)
            E[:, :, cc] = track(np.maximum(np.maximum(E[:, :, cc], tt), f2 if odd else f1))
            F = np.maximum(F, tt)
            if cc == tile_c - 1:
                F = track(F + (nge2 if pl else nge))
            elif odd:
                F = track(F + nge2)
            if odd:
                c1 = np.maximum(c1, hh)
            else:
                c0 = np.maximum(c0, hh)
            H[:, :, cc] = hh
        ma, mb = c0, c1
        n0, n1, n2 = n1, n2, track(n2 + pge)
    out = track(np.maximum(track(ma - track(n0 - pge)), track(mb - n0)))
    return [int(v) for v in out.max(axis=1)]


@pytest.mark.parametrize("tiling", [(4, 16), (8, 19), (16, 16)], ids=lambda v: "G%dxC%d" % v)
@pytest.mark.parametrize("pen", ADMITTED, ids=lambda v: "m%d_x%d_g%d_e%d" % (v[0], -v[1], -v[2], -v[3]))
def test_model_matches_gotoh_on_random_tasks(pen, tiling, oracle_built):
    G, tile_c = tiling
    steps = max_steps_py(*pen, G * tile_c)
    assert steps >= G
    rng = np.random.default_rng(2000 * G + tile_c + 7 * pen[0] - pen[3])
    qs, ws = random_tasks(rng, 24, G * tile_c, min(120, steps - G + 1))
    track = Track()
    assert pairframe_sweep(qs, ws, pen, G, tile_c, track) == gotoh(qs, ws, pen)
    assert track.peak <= 2048


@pytest.mark.parametrize("pen,tiling", [((1, -2, -4, -3), (8, 19)), ((1, -2, -4, -3), (8, 20)), ((1, -2, -4, -3), (16, 32)),
                                        ((4, -4, -10, -4), (8, 19)), ((5, -4, -6, -1), (8, 20))],
                         ids=lambda v: "_".join(str(abs(x)) for x in v))
def test_values_stay_exact_at_the_limit(pen, tiling, oracle_built):
    """The longest sweep that the library admits, with the read matching the window's end in full (the largest score in the
    frame of the last rows), matching its start, with no match at all and with a window of N only."""
    from smalt_amd import api
    G, tile_c = tiling
    ncol = G * tile_c
    steps = api.lib().smaltgpu_sw_pairframe_max_steps(pen[0], pen[1], pen[2], pen[3], ncol)
    assert steps == max_steps_py(*pen, ncol) and steps >= G
    wl = steps - (G - 1)
    rng = np.random.default_rng(ncol + steps)
    q = rng.integers(0, 4, size=ncol, dtype=np.uint8)
    n = min(ncol, wl)
    tail = rng.integers(0, 4, size=wl, dtype=np.uint8)
    tail[wl - n:] = q[ncol - n:]
    head = rng.integers(0, 4, size=wl, dtype=np.uint8)
    head[:n] = q[:n]
    none = ((q[0] + 1 + np.zeros(wl, dtype=np.uint8)) & 3).astype(np.uint8)
    qs = [q.tobytes()] * 2 + [bytes([int(q[0])]) * ncol, q.tobytes()]
    ws = [tail.tobytes(), head.tobytes(), none.tobytes(), bytes([5]) * wl]
    track = Track()
    got = pairframe_sweep(qs, ws, pen, G, tile_c, track)
    assert got == gotoh(qs, ws, pen)
    assert got[0] >= pen[0] * n and got[2] == 0 and got[3] == 0
    assert track.peak <= 2048
    assert track.peak >= got[0] - pen[3] * (wl - 1)        # the full score, seen from the frame of the last row


@pytest.mark.parametrize("ncol", [64, 104, 152, 160, 256, 512])
def test_library_limit_is_the_documented_rule(ncol):
    from smalt_amd import api
    f, fr = api.lib().smaltgpu_sw_pairframe_max_steps, api.lib().smaltgpu_sw_rowframe_max_steps
    for pen in ADMITTED + ROW_FRAME_ONLY + NEITHER:
        steps = f(pen[0], pen[1], pen[2], pen[3], ncol)
        assert steps == max_steps_py(*pen, ncol), (pen, ncol)
        if steps >= 0:
            gi, ge = -pen[2], -pen[3]
            assert pen[0] * ncol + ge * (steps + 3) + gi <= 2040          # the last sweep inside ...
            assert pen[0] * ncol + ge * (steps + 4) + gi > 2040           # ... and the first beyond it is refused
            assert steps == fr(pen[0], pen[1], pen[2], pen[3], ncol) - 2  # two more ge of room than the row frame
    for pen in ROW_FRAME_ONLY:                                            # these fall through to the row frame
        assert f(*pen, 152) == -1 and fr(*pen, 152) >= 8
    for pen in NEITHER:
        assert f(*pen, 152) == -1 and fr(*pen, 152) == -1
    for pen in ADMITTED:
        assert f(*pen, 152) >= 8
    assert f(1, -2, -4, -3, 152) == 625

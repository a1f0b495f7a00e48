"""A numpy float16 model of the row-frame sweep of the packed K2a kernel (sw16r_core) as the lanes run it:
G lanes of C columns, lane g one row behind lane g - 1, the hand-over of H and F, the first lane's boundary and the
start-up values.  Its best scores are compared with the oracle's plain integer Gotoh, and every intermediate value must be
an integer of magnitude <= 2048 (exact in half floats) for sweeps up to the length that the library admits to the form."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

F16 = np.float16
PAD = 9          # column beyond the read: the selector of the constant 0
PENS = [(1, -2, -4, -3), (2, -3, -5, -2), (5, -4, -6, -1), (1, -1, -2, -1), (3, -6, -8, -4), (1, -2, -8, -7), (6, -4, -8, -6)]


def max_steps_py(match, mismatch, gap_init, gap_ext, ncols):
    """The rule of DESIGN 4.1 spelled out: the table entries (and match and mismatch themselves, for the half-float form
    that takes the longer sweeps) have at most three significant bits, and match * ncols + ge * (steps + 1) + gi <= 2040."""
    gi, ge = -gap_init, -gap_ext
    if match <= 0 or ge < 0 or gi < ge:
        return -1
    for v in (match + ge, mismatch + ge, ge, match, mismatch):
        a = abs(v)
        while a and a % 2 == 0:
            a //= 2
        if a > 7:
            return -1
    if match * ncols + gi > 2040:
        return -1
    n = -1
    while ge and match * ncols + ge * (n + 2) + gi <= 2040:
        n += 1
    return n if ge else 0x7fffffff


class Track:
    def __init__(self):
        self.peak = 0.0

    def __call__(self, x):
        assert x.dtype == F16
        x32 = x.astype(np.float32)
        assert np.all(x32 == np.rint(x32)), "not an integer"
        self.peak = max(self.peak, float(np.abs(x32).max()))
        return x


def rowframe_sweep(qs, ws, pen, G, tile_c, track):
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
    pge, nge, ngo = F16(ge), F16(-ge), F16(-(gi - ge))
    lane = np.arange(G)
    flo1 = np.broadcast_to((pge * (-lane).astype(F16)).astype(F16), (T, G)).copy()       # the row a lane does next: -g
    f0 = track(flo1 - pge)
    H = np.repeat(f0[:, :, None], tile_c, axis=2)
    E = np.repeat(flo1[:, :, None], tile_c, axis=2)
    best, F, prev_hl, flo = f0.copy(), f0.copy(), f0.copy(), f0.copy()
    for step in range(nstep):
        r = step - lane                                                                  # row of every lane
        inside = (r[None, :] >= 0) & (r[None, :] < wlen[:, None])
        wc = np.where(inside, W[np.arange(T)[:, None], np.clip(r, 0, None)[None, :]], 5)
        flo = flo1
        flo1 = track(flo + pge)
        best = track(best + pge)
        hl = np.concatenate([flo[:, :1], H[:, :-1, tile_c - 1]], axis=1)                 # the left neighbour's, same row
        fin = np.concatenate([flo[:, :1], F[:, :-1]], axis=1)
        carry, prev_hl, F = prev_hl, hl, fin
        Hold = H.copy()
        for cc in range(tile_c):
            qc = Q[:, :, cc]
            s = np.where(qc == PAD, 0, np.where(wc >= 4, ge, np.where(qc == wc, match + ge, mismatch + ge))).astype(F16)
            dg = carry if cc == 0 else Hold[:, :, cc - 1]
            t = track(dg + s)
            hh = np.maximum(np.maximum(t, E[:, :, cc]), F)
            tt = track(hh + ngo)
            E[:, :, cc] = track(np.maximum(np.maximum(E[:, :, cc], tt), flo1))
            F = track(np.maximum(F, tt) + nge)
            best = np.maximum(best, hh)
            H[:, :, cc] = hh
    out = track(best - flo)
    return [int(v) for v in out.max(axis=1)]


def gotoh(qs, ws, pen):
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, pen[0], pen[1])
    return [ol.lib().or_sw_full(q, len(q), w, len(w), M, pen[2], pen[3]) for q, w in zip(qs, ws)]


def random_tasks(rng, n, ncol, wmax):
    qs, ws = [], []
    for _ in range(n):
        ql = int(rng.integers(1, ncol + 1))
        q = rng.integers(0, 4, size=ql, dtype=np.uint8)
        wl = int(rng.integers(1, wmax + 1))
        w = rng.integers(0, 4, size=wl, dtype=np.uint8)
        if rng.random() < 0.8:
            n_ = min(ql, wl)
            at = int(rng.integers(0, wl - n_ + 1))
            core = q[:n_].copy()
            m = rng.random(n_) < rng.choice([0.0, 0.03, 0.15])
            core[m] = (core[m] + 1) & 3
            if n_ > 30 and rng.random() < 0.5:                                           # a gap of a few bases, or of tens
                p, d = int(rng.integers(5, n_ - 20)), int(rng.choice([1, 2, 3, 15]))
                core = np.concatenate([core[:p], core[p + d:], rng.integers(0, 4, size=d, dtype=np.uint8)])
            w[at:at + n_] = core
        if rng.random() < 0.3:
            at, k = int(rng.integers(0, wl)), int(rng.integers(1, 12))
            w[at:at + k] = 5                                                             # a run of N
        qs.append(q.tobytes())
        ws.append(w.tobytes())
    qs.append(rng.integers(0, 4, size=ncol, dtype=np.uint8).tobytes())                   # a window of N only
    ws.append(bytes([5]) * 40)
    return qs, ws


@pytest.mark.parametrize("tiling", [(4, 16), (8, 19), (16, 16)], ids=lambda v: "G%dxC%d" % v)
@pytest.mark.parametrize("pen", PENS, ids=lambda v: "m%d_x%d_g%d_e%d" % (v[0], -v[1], -v[2], -v[3]))
def test_model_matches_gotoh_on_random_tasks(pen, tiling, oracle_built):
    G, tile_c = tiling
    steps = max_steps_py(*pen, G * tile_c)
    assert steps >= G
    rng = np.random.default_rng(1000 * G + tile_c + 7 * pen[0] - pen[3])
    qs, ws = random_tasks(rng, 24, G * tile_c, min(120, steps - G + 1))
    track = Track()
    assert rowframe_sweep(qs, ws, pen, G, tile_c, track) == gotoh(qs, ws, pen)
    assert track.peak <= 2048


@pytest.mark.parametrize("pen,tiling", [((1, -2, -4, -3), (8, 19)), ((1, -2, -8, -7), (8, 19)), ((3, -6, -8, -4), (8, 20)),
                                        ((6, -4, -8, -6), (16, 16)), ((1, -2, -4, -3), (16, 32))],
                         ids=lambda v: "_".join(str(abs(x)) for x in v))
def test_values_stay_exact_at_the_limit(pen, tiling, oracle_built):
    """The longest sweep that the library admits, with the read matching the window's end in full (the largest score in the
    frame of the last rows), matching its start, and with no match at all."""
    from smalt_amd import api
    G, tile_c = tiling
    ncol = G * tile_c
    steps = api.lib().smaltgpu_sw_rowframe_max_steps(pen[0], pen[1], pen[2], pen[3], ncol)
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
    qs = [q.tobytes()] * 2 + [bytes([int(q[0])]) * ncol, q[:1].tobytes()]
    ws = [tail.tobytes(), head.tobytes(), none.tobytes(), bytes([5]) * wl]
    track = Track()
    got = rowframe_sweep(qs, ws, pen, G, tile_c, track)
    assert got == gotoh(qs, ws, pen)
    assert got[0] >= pen[0] * n and got[2] == 0 and got[3] == 0
    assert track.peak <= 2048
    assert track.peak >= got[0] - pen[3] * (wl - 1)        # the full score, seen from the frame of the last row


@pytest.mark.parametrize("ncol", [64, 104, 152, 160, 256, 512])
def test_library_limit_is_the_documented_rule(ncol):
    from smalt_amd import api
    f = api.lib().smaltgpu_sw_rowframe_max_steps
    for pen in PENS + [(5, -4, -8, -6), (9, -7, -9, -3), (1, -2, -3, -4), (13, -2, -4, -3)]:
        steps = f(pen[0], pen[1], pen[2], pen[3], ncol)
        assert steps == max_steps_py(*pen, ncol), (pen, ncol)
        if steps >= 0:
            gi, ge = -pen[2], -pen[3]
            assert pen[0] * ncol + ge * (steps + 1) + gi <= 2040          # the last sweep inside ...
            assert pen[0] * ncol + ge * (steps + 2) + gi > 2040           # ... and the first beyond it is refused
    assert f(5, -4, -8, -6, 152) == -1 and f(1, -2, -4, -3, 152) == 627

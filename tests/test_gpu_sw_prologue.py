"""What the packed K2a kernels build in front of the sweep: the selectors of the read's columns (read codes staged in
LDS once per read and strand, kept while a wave's next iteration is still in that read) and the window's code pairs (decoded ten at a time
from whole words of the packed reference).

Case 1 drives the stand-alone kernel at the edges of every tile geometry; cases 2-4 map small batches on references of a
few hundred kilobases and require what tests/test_gpu_fuzz.py requires: the raw result array and the per-read scalars of
the CPU oracle, for every read."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

FLG_BEST = 0x02
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
K, S = 13, 6

QLENS = [K, 63, 64, 65, 103, 104, 105, 149, 150, 151, 152, 153, 159, 160, 161, 255]
WLENS = [1, 9, 10, 11, 247, 248, 249, 1016]


def _revcomp(r):
    return r[::-1].translate(COMP)


def _mutate(rng, r, rate):
    out = bytearray(r)
    for j in range(len(out)):
        if rng.random() < rate:
            out[j] = b"ACGT"[int(rng.integers(0, 4))]
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# 1. tile edges, stand-alone kernel
# ---------------------------------------------------------------------------------------------------------------------
def _edge_tasks(rng, qlen):
    """Queries of `qlen` (the longest of the batch picks the tile geometry) and of shorter lengths, against windows of
    every length in WLENS that hold the query, a part of it, or nothing of it."""
    qs, ws = [], []
    for wl in WLENS:
        for ql in (qlen, max(1, qlen - 1), K, max(1, qlen // 2)):
            q = rng.integers(0, 4, size=ql, dtype=np.uint8)
            w = rng.integers(0, 4, size=wl, dtype=np.uint8)
            if rng.random() < 0.8:                      # the query (mutated) or its head somewhere in the window
                n = min(ql, wl)
                at = int(rng.integers(0, wl - n + 1))
                core = q[:n].copy()
                m = rng.random(n) < 0.05
                core[m] = (core[m] + 1) & 3
                w[at:at + n] = core
            if rng.random() < 0.15:
                w[int(rng.integers(0, wl))] = 5         # an N in the window
            qs.append(q.tobytes())
            ws.append(w.tobytes())
    return qs, ws


@pytest.fixture(scope="module")
def raw_mapper(oracle_built, tmp_path_factory):
    from smalt_amd import api
    rng = np.random.default_rng(4242)
    seqs = [bytes(rng.choice(list(b"ACGT"), size=4000).astype(np.uint8))]
    oix = ol.build_index(seqs, ["s"], 11, 3)
    pre = str(tmp_path_factory.mktemp("prologue") / "x")
    ol.lib().or_index_write(oix, pre.encode())
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, 16, 512)
    yield gix, mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


@pytest.mark.parametrize("pen", [(1, -2, -4, -3), (9, -7, -9, -3)], ids=["default-halffloat", "m9_x7_g9_e3-integer"])
def test_tile_edges_raw_kernel(pen, raw_mapper):
    """Read lengths at both sides of every geometry's limit and windows at both sides of a packed word, of the short
    instance's limit and at the longest window, in the half-float and in the integer form of the sweep."""
    gix, mp = raw_mapper
    match, mismatch, gi, ge = pen
    par = gix.default_params()
    if pen != (1, -2, -4, -3):
        par.match, par.mismatch, par.gap_init, par.gap_ext = match, mismatch, gi, ge
    assert (par.match, par.mismatch, par.gap_init, par.gap_ext) == pen
    M = (C.c_int8 * 64)()
    ol.lib().or_score_matrix(M, match, mismatch)
    rng = np.random.default_rng(1000 * match - gi)
    for qlen in QLENS:
        qs, ws = _edge_tasks(rng, qlen)
        got = mp.sw_full_batch(qs, ws, par, packed16=True)
        for i, (q, w) in enumerate(zip(qs, ws)):
            exp = ol.lib().or_sw_full(q, len(q), w, len(w), M, gi, ge)
            assert got[i] == exp, (qlen, i, len(q), len(w), got[i], exp)


# ---------------------------------------------------------------------------------------------------------------------
# 2-4. whole path on small references
# ---------------------------------------------------------------------------------------------------------------------
def _random_seqs(rng, nseq, seqlen):
    return [ACGT[rng.integers(0, 4, size=seqlen)].tobytes() for _ in range(nseq)]


def placement_case():
    """Reads from the first and the last 200 bases of the concatenated reference (the window starts at base 0 / ends in the
    last packed word), across the border of two sequences, and from 60 consecutive start positions at three places (their
    windows start at every residue of 10 bases per packed word), on both strands."""
    rng = np.random.default_rng(20250)
    seqs = _random_seqs(rng, 2, 120_000)
    reads = []
    last = seqs[-1]
    for i in range(50):
        ln = int(rng.integers(100, 151))
        reads.append(seqs[0][i:i + ln])                                        # starts 0 .. 49 of the first sequence
        reads.append(last[len(last) - i - ln:len(last) - i])                   # ends 0 .. 49 before the end of the last
    for i in range(20):
        ln = int(rng.integers(100, 151))
        reads.append(seqs[0][len(seqs[0]) - ln - i:len(seqs[0]) - i])          # end of the first sequence ...
        reads.append(seqs[1][i:i + ln])                                        # ... and start of the second
    for si, p0 in ((0, 30_001), (1, 47_113), (1, 90_007)):
        for i in range(60):
            ln = int(rng.integers(100, 151))
            reads.append(_mutate(rng, seqs[si][p0 + i:p0 + i + ln], 0.02))
    reads = [(_revcomp(r) if j % 2 else r) for j, r in enumerate(reads)]
    return seqs, reads, dict(below_max=-1, best=False)


def task_mix_case():
    """Short unique reads (one to three candidates each, both strands: the 16 tasks of a wave span many reads) around two
    reads from a repeat of 3000 copies, each of which owns about a thousand consecutive tasks (the depth limit caps a
    read's ranked candidates at 2048)."""
    rng = np.random.default_rng(1)
    nseq, seqlen, unit, ncopy = 3, 200_000, 80, 3000
    seqs = [rng.integers(0, 4, size=seqlen, dtype=np.uint8) for _ in range(nseq)]
    cons = rng.integers(0, 4, size=unit, dtype=np.uint8)
    per = ncopy // nseq
    step = (seqlen // 2) // per
    for si in range(nseq):
        for c in range(per):                                                   # the repeat fills the second half of every sequence
            p = seqlen // 2 + c * step
            cp = cons.copy()
            m = rng.random(unit) < 0.04
            cp[m] = (cp[m] + rng.integers(1, 4, size=int(m.sum()))) & 3
            seqs[si][p:p + unit] = cp
    asc = [ACGT[s].tobytes() for s in seqs]
    reads = []
    for i in range(240):
        si, p, ln = int(rng.integers(0, nseq)), int(rng.integers(0, seqlen // 2 - 200)), int(rng.integers(40, 70))
        r = _mutate(rng, asc[si][p:p + ln], 0.01)
        reads.append(_revcomp(r) if i % 2 else r)
    rep = ACGT[cons].tobytes()
    reads.insert(100, rep)
    reads.append(_revcomp(rep[:72]))
    return asc, reads, {}


def dead_neighbour_case():
    """Reads with an N (scored by the 32-bit kernel, dead in the packed one) next to clean reads; a repeat family gives
    most reads a few candidates, so that dead and live tasks share lane groups."""
    from smalt_amd import synth
    rng = np.random.default_rng(77)
    ch = synth.make_reference(2, 150_000, seed=77, repeat_frac=0.2, n_fam=3, cons_len=400, divergence=0.06)
    seqs = [synth.codes_to_ascii(c) for c in ch]
    reads = []
    for i in range(300):
        si, ln = int(rng.integers(0, 2)), int(rng.integers(90, 151))
        p = int(rng.integers(0, len(seqs[si]) - ln))
        r = bytearray(_mutate(rng, seqs[si][p:p + ln], 0.02))
        if i % 2:
            r[int(rng.integers(0, ln))] = ord("N")
        r = bytes(r)
        reads.append(_revcomp(r) if (i // 2) % 2 else r)
    return seqs, reads, {}


def oracle_expectation(seqs, reads, par, prefix):
    """Index files at `prefix`, and per read (raw results or (None, rv), scalars, ranked candidates) of the CPU oracle."""
    names = ["s%d" % i for i in range(len(seqs))]
    oix0 = ol.build_index(seqs, names, K, S)
    assert ol.lib().or_index_write(oix0, prefix.encode()) == 0
    ol.lib().or_index_free(oix0)
    oix = ol.lib().or_index_read(prefix.encode())
    op = ol.default_params(oix)
    if "below_max" in par:
        op.min_swatscor_below_max = par["below_max"]
    if par.get("best") is False:
        op.flags &= ~FLG_BEST
    om = ol.Mapper(oix)
    exp = []
    for r in reads:
        rv, res = om.map(r, b"I" * len(r), op)
        st = om.stats()
        n = C.c_int()
        ol.lib().or_map_cands(om.m, C.byref(n))
        exp.append(((None, rv) if rv else res, dict(swmax=st[0], sw2nd=st[1], nseg=st[2], nseg_tot=st[3], nhit=st[4], nhit_tot=st[5]), n.value))
    om.close()
    return exp


def _map_and_compare(seqs, reads, par, exp, prefix):
    from smalt_amd import api
    gix = api.Index.load(prefix, 0)
    gp = gix.default_params()
    if "below_max" in par:
        gp.min_swatscor_below_max = par["below_max"]
    if par.get("best") is False:
        gp.rmapflg &= ~FLG_BEST
    mp = api.Mapper(gix, len(reads), 150)           # 150 bases: the tile geometry of the headline workload for every case
    try:
        res, stats = mp.map_batch(reads, [b"I" * len(r) for r in reads], gp, allow_read_errors=True)
    finally:
        mp.close()
        gix.close()
    for i in range(len(reads)):
        if isinstance(exp[i][0], tuple):
            assert stats[i]["err"] != 0 and res[i] == [], i
            continue
        assert stats[i]["err"] == 0, i
        assert res[i] == exp[i][0], (i, len(reads[i]))
        for kk, v in exp[i][1].items():
            assert stats[i][kk] == v, (i, kk)


def _oracle_maps_enough(exp):
    assert sum(1 for e in exp if not isinstance(e[0], tuple) and e[0]) > 100


def test_window_placement(oracle_built, tmp_path):
    seqs, reads, par = placement_case()
    pre = str(tmp_path / "pl")
    exp = oracle_expectation(seqs, reads, par, pre)
    _oracle_maps_enough(exp)
    _map_and_compare(seqs, reads, par, exp, pre)


@pytest.mark.parametrize("grid", [None, 3], ids=["grid-default", "grid-3"])
def test_task_mix_within_a_wave(grid, oracle_built, tmp_path, monkeypatch):
    """With three workgroups a wave's successive iterations lie 48 tasks apart: inside a repeat read's thousand tasks it
    keeps the read it has staged, and it changes over where the short reads begin.  With the default grid every wave has
    one iteration."""
    seqs, reads, par = task_mix_case()
    pre = str(tmp_path / "mix")
    exp = oracle_expectation(seqs, reads, par, pre)
    _oracle_maps_enough(exp)
    ncand = [e[2] for e in exp]
    big = sorted(i for i, n in enumerate(ncand) if n >= 800)
    assert big == [100, len(reads) - 1], big                           # the two repeat reads own about a thousand tasks each ...
    small = [n for i, n in enumerate(ncand) if i not in big]
    assert max(small) <= 3 and sum(1 for n in small if n >= 1) > 200   # ... the others one to three
    if grid is not None:
        monkeypatch.setenv("SMALTGPU_SWFULL_GRID", str(grid))
    _map_and_compare(seqs, reads, par, exp, pre)


def test_dead_neighbours(oracle_built, tmp_path):
    seqs, reads, par = dead_neighbour_case()
    assert sum(1 for r in reads if b"N" in r) > 100 and sum(1 for r in reads if b"N" not in r) > 100
    pre = str(tmp_path / "dn")
    exp = oracle_expectation(seqs, reads, par, pre)
    _oracle_maps_enough(exp)
    _map_and_compare(seqs, reads, par, exp, pre)

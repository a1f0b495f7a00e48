"""K2b, the banded score pass (alignment.c:1029), in both forms the mapper has -- band_fast_wave (k_sw_band: one wave per task,
strips of 1024 read columns with the band as an activity mask) and band_fast_scalar (k_sw_scalar: one lane per task) -- through
smaltgpu_sw_band_batch against the oracle's or_sw_band_fast: every score, and status 1 exactly where the oracle refuses the band
(OR_ERR_BAND).  The tasks are those of band_data.k2b_cases (read lengths 20 to 2100: no strip, one, and the edges of two and
three; bands of 1 to 1100 diagonals, wider than the read, band_r < band_l, clipped at the left and not, qs > 0 and qe < qlen - 1,
a band that misses the read, windows of 1 to 129 rows, N in read and window), with the five penalty sets the biased 8-byte score
table of the wave form depends on.  The entry packs the windows back to back in the index's 3-bit layout, so they start at every
phase of a 10-base word."""
import numpy as np
import pytest

import band_data as bd

pytestmark = pytest.mark.gpu

_EXP = {}


@pytest.fixture(scope="module")
def raw_mapper(oracle_built, tmp_path_factory):
    gix, mp, close = bd.open_mapper(tmp_path_factory.mktemp("k2b"), 2400)
    yield gix, mp
    close()


def _cases(pen, ql):
    """tasks of one read length and the oracle's (return code, score) for them, computed once per penalty set"""
    if (pen, ql) not in _EXP:
        tasks = bd.k2b_cases(np.random.default_rng(500 + ql), ql)
        M = bd.score_matrix(pen[0], pen[1])
        _EXP[(pen, ql)] = (tasks, [bd.or_band_fast(t, pen, M) for t in tasks])
    return _EXP[(pen, ql)]


@pytest.mark.parametrize("form", [0, 1], ids=["wave", "lane"])
@pytest.mark.parametrize("pen", bd.PENS, ids=bd.PEN_IDS)
def test_k2b_scores_and_refused_bands(pen, form, raw_mapper):
    gix, mp = raw_mapper
    par = bd.params_of(gix, pen)
    phases = set()
    for ql in bd.K2B_QLENS:
        tasks, exp = _cases(pen, ql)
        got, status = mp.sw_band_batch([t["q"] for t in tasks], [t["w"] for t in tasks], par, [t["band"] for t in tasks], form)
        o = 0
        for i, t in enumerate(tasks):
            rv, sc = exp[i]
            assert rv in (bd.OR_OK, bd.OR_ERR_BAND)
            assert status[i] == (1 if rv == bd.OR_ERR_BAND else 0), (ql, i, t["kind"], t["band"], status[i], rv)
            assert got[i] == sc, (ql, i, t["kind"], t["band"], len(t["w"]), got[i], sc)
            phases.add(o % 10)
            o += len(t["w"])
        assert sum(status) >= 1 and max(got) > 0
    assert len(phases) == 10

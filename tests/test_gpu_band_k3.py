"""K3's band pass form by form: smaltgpu_band_align_nodes runs ONE node of the recursion (alignment.c:1300) in one named form of
the pass -- rows of up to 64 diagonals (16-, 32- and 64-lane instances; global pointers, or read and window staged in LDS with the
directions in LDS or in global memory), anti-diagonals, the wave forms with 2, 4, 7 and 12 columns per lane (row-major directions
and the anti-diagonal-major layout of a direction matrix in HBM), strips of 64 x 8 and 64 x 16 columns with 2-bit directions, one
lane -- with the traceback the mapper pairs with it.  The recursion is driven from here (band_data.run_recursion, as
band_recursive of oracle/or_align.c): a stack of (s_left, s_right) per task, one launch per round for all pending nodes, results in
the order node, left, right.  The full list per task (score, qs, qe, rs, re, DiffStr bytes) and the return code are held against
ONE or_sw_band_full call on the root, which also exercises band_init with s_left > 0.

A node of the recursion whose band has left the forced form's precondition (a remainder of the window in which the band, cut at
the read's end, is narrower than a strip form takes) is sent to the one-lane form by the driver, openly and counted; every root
must be inside it.  The case lists (band_data.cases_of) hold the shapes at which each form's code takes another path; that they
hold alignments, ties of the maximum and recursions is checked on the oracle in test_band_nodes.py."""
import pytest

import band_data as bd

pytestmark = pytest.mark.gpu

# (form, lds, tw)
VARIANTS = [(bd.ROWS, 0, 0), (bd.ROWS, 1, 0), (bd.ANTIDIAG, 0, 0), (bd.ANTIDIAG, 0, 1)] + \
           [(f, 0, tw) for f in (bd.WAVE2, bd.WAVE4, bd.WAVE7, bd.WAVE12) for tw in (0, 1)] + \
           [(bd.STRIP8, 0, 0), (bd.STRIP16, 0, 0), (bd.SCALAR, 0, 0)]
VIDS = [bd.FORM_NAMES[f] + ("-lds" if lds else "") + ("-tw" if tw else "") for f, lds, tw in VARIANTS]
_EXP = {}


@pytest.fixture(scope="module")
def raw_mapper(oracle_built, tmp_path_factory):
    gix, mp, close = bd.open_mapper(tmp_path_factory.mktemp("k3"), 2400)
    yield gix, mp
    close()


def _oracle(form, pen):
    if (form, pen) not in _EXP:
        M = bd.score_matrix(pen[0], pen[1])
        tasks = bd.cases_of(form, 0)
        _EXP[(form, pen)] = (tasks, [bd.or_band_full(t, pen, M, bd.minscore_of(pen)) for t in tasks])
    return _EXP[(form, pen)]


def _evaluator(mp, par, pen, minscore, form, lds, tw, counts):
    """nodes inside the form's precondition (and those band_init refuses: any form reports them) in one launch of the form, the
    others in one launch of the one-lane form"""
    gi, ge = -pen[2], -pen[3]

    def evaluate(nodes):
        sel = [[], []]
        for k, (t, iv) in enumerate(nodes):
            b = bd.py_band(*t["band"], len(t["q"]), iv[0], iv[1], len(t["w"]))
            inside = b is None or b["s_left"] >= b["s_len"] or bd.form_ok(form, b, gi, ge)
            sel[0 if inside else 1].append(k)
            root = iv == (0, len(t["w"]) - 1)
            counts["root_outside"] += root and not inside
            counts["inside"] += inside
            counts["outside"] += not inside
            if b is not None and form == bd.ROWS:
                counts["dir_lds" if b["band_width"] * (b["s_len"] - b["s_left"]) + b["band_width"] + 8 <= 16384 else "dir_global"] += 1
        out = [None] * len(nodes)
        for ks, f, l, w in ((sel[0], form, lds, tw), (sel[1], bd.SCALAR, 0, 0)):
            if ks:
                res = mp.band_align_nodes([nodes[k][0]["q"] for k in ks], [nodes[k][0]["w"] for k in ks], par, [nodes[k][0]["band"] for k in ks],
                                          [nodes[k][1] for k in ks], minscore, f, bool(l), bool(w))
                for k, r in zip(ks, res):
                    out[k] = r
        return out
    return evaluate


@pytest.mark.parametrize("pen", bd.PENS, ids=bd.PEN_IDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VIDS)
def test_k3_form_matches_oracle(variant, pen, raw_mapper):
    from smalt_amd import api
    form, lds, tw = variant
    gix, mp = raw_mapper
    par = bd.params_of(gix, pen)
    minscore = bd.minscore_of(pen)
    tasks, exp = _oracle(form, pen)
    if form == bd.ROWS and -pen[2] < -pen[3]:                 # the row form's gap scan needs gi >= ge: no fall-back, the call fails
        with pytest.raises(api.SmaltGpuError):
            mp.band_align_nodes([t["q"] for t in tasks], [t["w"] for t in tasks], par, [t["band"] for t in tasks],
                                [(0, len(t["w"]) - 1) for t in tasks], minscore, form, bool(lds), False)
        return
    counts = dict(root_outside=0, inside=0, outside=0, dir_lds=0, dir_global=0)
    got = bd.run_recursion(tasks, pen, minscore, _evaluator(mp, par, pen, minscore, form, lds, tw, counts))
    assert counts["root_outside"] == 0 and counts["inside"] > counts["outside"], counts
    if form == bd.ROWS:
        assert counts["dir_lds"] > 0 and counts["dir_global"] > 0, counts
    assert max(d for _, _, d in got) >= 2
    for i, ((rv, alis, _), (erv, ealis)) in enumerate(zip(got, exp)):
        assert rv == erv, (i, tasks[i]["kind"], tasks[i]["band"], rv, erv)
        assert alis == ealis, (i, tasks[i]["kind"], tasks[i]["band"], len(tasks[i]["q"]), len(tasks[i]["w"]), alis, ealis)


@pytest.mark.parametrize("lds", [0, 1], ids=["global", "lds"])
def test_k3_row_form_with_equal_gap_penalties(lds, raw_mapper):
    """gi == ge: the edge of the row form's precondition (its prefix-maximum scan of the horizontal gap score is exact for gi >= ge)"""
    gix, mp = raw_mapper
    pen = (1, -2, -3, -3)
    par = bd.params_of(gix, pen)
    minscore = bd.minscore_of(pen)
    M = bd.score_matrix(pen[0], pen[1])
    tasks = bd.cases_of(bd.ROWS, 0)
    exp = [bd.or_band_full(t, pen, M, minscore) for t in tasks]
    counts = dict(root_outside=0, inside=0, outside=0, dir_lds=0, dir_global=0)
    got = bd.run_recursion(tasks, pen, minscore, _evaluator(mp, par, pen, minscore, bd.ROWS, lds, 0, counts))
    assert counts["outside"] == 0
    assert [(rv, alis) for rv, alis, _ in got] == exp


@pytest.mark.parametrize("pen", [bd.PENS[0], bd.PENS[2]], ids=[bd.PEN_IDS[0], bd.PEN_IDS[2]])
def test_k3_forms_agree_with_each_other(pen, raw_mapper):
    """every form on the same small task set, form against form on (status, score, max_i, max_j, qs, rs, DiffStr): narrow bands in all
    forms but the strips, bands of 400 diagonals in STRIP8, the wave forms from 4 columns per lane on and one lane, bands of 2100
    diagonals in STRIP16 and one lane"""
    import numpy as np
    gix, mp = raw_mapper
    par = bd.params_of(gix, pen)
    minscore = bd.minscore_of(pen)
    rng = np.random.default_rng(4242)
    narrow = bd.common_cases(rng)
    mid = [bd.task(rng, 700, 150, 400, nindel=2, shift=200), bd.task(rng, 650, 129, 400, kind="periodic", period=4, shift=200),
           bd.task(rng, 900, 200, 400, kind="split", shift=199)]
    wide = [bd.task(rng, 2300, 100, 2100, nindel=2, shift=1050), bd.task(rng, 2290, 65, 2100, kind="periodic", period=6, shift=1000)]
    groups = [(narrow, [v for v in VARIANTS if v[0] not in (bd.STRIP8, bd.STRIP16)]),
              (mid, [v for v in VARIANTS if v[0] in (bd.STRIP8, bd.WAVE4, bd.WAVE7, bd.WAVE12, bd.SCALAR)]),
              (wide, [(bd.STRIP16, 0, 0), (bd.SCALAR, 0, 0)])]
    for tasks, variants in groups:
        ref = None
        for form, lds, tw in variants:
            res = mp.band_align_nodes([t["q"] for t in tasks], [t["w"] for t in tasks], par, [t["band"] for t in tasks],
                                      [(0, len(t["w"]) - 1) for t in tasks], minscore, form, bool(lds), bool(tw))
            if ref is None:
                ref = res
                assert any(r["status"] == bd.NODE_ALIGNED for r in res), res
            assert res == ref, (bd.FORM_NAMES[form], lds, tw, res, ref)

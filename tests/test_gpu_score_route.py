"""The first-pass score stage as a mapping call runs it: launch_sw_full, launch_sw_strip and launch_sw_scalar with the seven kernels
behind them, on the lists and flags the candidate stage leaves.  Ordinary mapping calls on the workloads of tests/score_route_data.py
(each holds its route by construction, tests/test_score_route_cases.py), then smaltgpu_score_pool: every record of the pool must carry
the window and band of the oracle's ranked candidate, and the flags and the score tests/score_route_ref.py predicts for the kernel
that has to score it; the counters work[2], work[3], work[7], work[17], work[18] must equal the predicted integers (k_sw_scalar's early
return rests on work[3]); a second call through the same mapper must leave the same; results and per-read stats must equal the
oracle's.  Everything is an integer and compared for equality."""
import numpy as np
import pytest

import score_route_data as srd
import score_route_ref as srr

pytestmark = pytest.mark.gpu

WORK = (2, 3, 7, 17, 18)
GEO_KEYS = ("rccap", "long_cap", "strip_cap", "tile_qmax", "wincap", "tile_g", "tile_c")


def _by_read(rec):
    """pool order -> read order; the records of a read are contiguous and in rank order, so a stable sort by read keeps the ranks"""
    return rec[np.argsort(rec["rid"], kind="stable")]


@pytest.mark.parametrize("name", srd.CASES)
def test_score_stage_routes_and_scores(name, oracle_built, monkeypatch):
    from smalt_amd import api
    cs, e = srd.case(name), srd.expect(name)
    # hooks of the mapper's creation that an earlier test module may have left in the process's environment
    for var in ("SMALTGPU_CANDS_PER_READ", "SMALTGPU_SWFULL_GRID", "SMALTGPU_STRIP_GRID"):
        monkeypatch.delenv(var, raising=False)
    for var, value in cs.env.items():
        monkeypatch.setenv(var, value)
    gix = api.Index.load(e.prefix, 0)
    mp = api.Mapper(gix, cs.mapper[0], cs.mapper[1], cands_per_read=cs.mapper[2])
    try:
        par = cs.params(gix.default_params())
        pls = []
        for bi, b in enumerate(e.batches):
            rb = b["reads"]
            quals = [b"I" * len(r) for r in rb]
            first = None
            for rep in range(2):
                res, stats = mp.map_batch(rb, quals, par)
                work = mp.timers()[1]
                rec, geo = mp.score_pool()
                rec = _by_read(rec)
                got_work = {i: int(work[i]) for i in WORK}
                if first is not None:                       # the second call leaves what the first left
                    assert np.array_equal(rec, first[0]), (name, bi, "records of the second call")
                    assert got_work == first[1], (name, bi, got_work, first[1])
                    assert (res, stats) == first[2]
                    continue
                first = (rec, got_work, (res, stats))
                # the geometry: the restatement the CPU tests use, and the grid hooks of the case
                want_geo = srr.geometry(*cs.mapper)
                assert {k: geo[k] for k in GEO_KEYS} == want_geo, (geo, want_geo)
                assert geo["full_grid"] == int(cs.env.get("SMALTGPU_SWFULL_GRID", 8192))
                if "SMALTGPU_STRIP_GRID" in cs.env:
                    assert geo["strip_grid"] == int(cs.env["SMALTGPU_STRIP_GRID"])
                assert geo["rc_count"] <= geo["rccap"] and len(rec) == geo["rc_count"]      # no overflow: no read was re-mapped
                # which copy of S7's listing rule ran: only the wave-parallel form of the candidate stage counts its candidates (work[5])
                assert (int(work[5]) == 0) == cs.seq_form, (name, int(work[5]))
                # the pool holds the oracle's ranked candidates: window, band, strand, sequence, cover
                want = b["cands"]
                assert len(rec) == len(want), (name, bi, len(rec), len(want))
                got = [dict(rid=int(r["rid"]), reverse=int(r["flags"] & srr.REVERSE), qs=int(r["qs"]), qe=int(r["qe"]), rs=int(r["rs"]), re=int(r["re"]),
                            band_l=int(r["band_l"]), band_r=int(r["band_r"]), sqidx=int(r["sqidx"]), cover=int(r["cover"])) for r in rec]
                for i, (g, c) in enumerate(zip(got, want)):
                    assert g == {k: c[k] for k in g}, (name, bi, i, g, c)
                # what the stage must have left, from the pool's own records
                pl = srr.plan(got, b["qlens"], b["has_n"], geo, e.par, srr.Scorer(e.oix, rb, e.par))
                print(name, "batch", bi, "work", got_work, "predicted", pl["work"])
                bad = [(i, pl["kernel"][i], int(rec["swscor"][i]), pl["score"][i], int(rec["flags"][i]), pl["flags"][i]) for i in range(len(rec))
                       if int(rec["swscor"][i]) != pl["score"][i] or int(rec["flags"][i]) != pl["flags"][i]]
                assert not bad, (name, bi, len(bad), bad[:8])
                for i in range(len(rec)):
                    assert stats[int(rec["rid"][i])]["err"] != 0 or int(rec["flags"][i]) & (srr.SCORED | srr.ERR), (name, bi, i)
                assert got_work == pl["work"], (name, bi, got_work, pl["work"])
                assert pl["long_overflow"] == (got_work[17] > geo["long_cap"]) and pl["strip_overflow"] == (got_work[18] > geo["strip_cap"])
                pls.append(pl)
                # results and per-read scalars
                for i in range(len(rb)):
                    assert stats[i]["err"] == 0, (name, bi, i, stats[i])
                    assert res[i] == b["res"][i], (name, bi, i)
                    for kk, v in b["stats"][i].items():
                        assert stats[i][kk] == v, (name, bi, i, kk)
        # the populations of the case, on the pool itself
        for what, holds in cs.need.items():
            assert holds(pls), (name, what)
    finally:
        mp.close()
        gix.close()

"""The workloads of tests/score_route_data.py reach the routes they are named after -- by the oracle's candidates alone, without a
GPU: a case that no longer reaches its branch fails here and does not pass quietly in tests/test_gpu_score_route.py.  Per case: the
populations on both sides of each border, the counts above the list capacities and the score >= 65535 (the case's `need`), over the
plan tests/score_route_ref.py makes of the oracle's ranked candidates (or_map_cands without FLG_BEST; the RC lines of the oracle's
dump are the same list); the banded rule of score_route_ref against the kernel the oracle's predicate picked (used_simd) and its
expected score against the oracle's own first-pass score, on every candidate."""
import pytest

import score_route_data as srd
import score_route_ref as srr


@pytest.mark.parametrize("name", srd.CASES)
def test_case_reaches_its_routes(name, oracle_built):
    cs, e = srd.case(name), srd.expect(name)
    assert sum(len(s) for s in cs.seqs) <= 1_000_000 and all(len(rb) <= 1000 for rb in cs.batches)
    assert cs.mapper[0] >= max(len(rb) for rb in cs.batches) and cs.mapper[1] >= max(len(r) for rb in cs.batches for r in rb)
    pls = srd.plans(name)
    for b, pl in zip(e.batches, pls):
        n = len(b["cands"])
        assert n > 0 and n <= srr.geometry(*cs.mapper)["rccap"]
        lines = [ln for per in b["rc_lines"] for ln in per]
        assert len(lines) == n
        for i, (c, ln) in enumerate(zip(b["cands"], lines)):
            # RC i flags qs qe rs re band_l band_r sqidx swscor (oracle/DUMPFORMAT.md)
            assert [int(x) for x in ln[2:]] == [c["reverse"] | 2, c["qs"], c["qe"], c["rs"], c["re"], c["band_l"], c["band_r"], c["sqidx"], c["swscor"]], (i, ln)
            assert pl["banded"][i] == (not c["used_simd"]), (i, c)
            assert pl["score"][i] == c["swscor"], (i, c, pl["kernel"][i])
            assert pl["kernel"][i] in srr.KERNELS and not pl["flags"][i] & srr.ERR
    for what, holds in cs.need.items():
        assert holds(pls), (name, what)
    if cs.seq_form:
        assert all(c["sqidx"] == -1 for b in e.batches for c in b["cands"])       # the call is not sequence by sequence
        assert e.par.min_cover >= cs.k + cs.s


def test_cases_cover_every_kernel_and_both_overflows(oracle_built):
    seen, over = set(), set()
    for name in srd.CASES:
        if name in srd.SAME_WORKLOAD:
            continue
        for pl in srd.plans(name):
            seen.update(pl["kernel"])
            over.update(k for k in ("long_overflow", "strip_overflow") if pl[k])
    assert seen == set(srr.KERNELS)
    assert over == {"long_overflow", "strip_overflow"}

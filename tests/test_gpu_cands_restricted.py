"""The interval mode of the candidate stage (the restricted rounds of rmapPair, DESIGN 5a rounds B and D) branch by branch on
the device: Mapper.map_batch_ctx with intervals against the CPU oracle, exactly.  Every case first asserts, from the predicates
of tests/restricted_ref.py alone (the oracle's seed tables, the index arrays on the host, the intervals and the geometry of the
mapper's slots), that its inputs reach the branch it is about, and prints the counts.  Then a debug batch: the stage lines of
every read against the oracle's, line by line (a debug batch has one pass over first-pass slots, so reads whose strands gather
more keys than such a slot holds are left to the plain batch); and a plain batch: results, the six scalars, err == 0.
tests/test_cands_restricted_paths.py runs the main-index cases through the one-lane host build."""
import functools

import numpy as np
import pytest

import oracle_lib as ol
import restricted_ref as rr

pytestmark = pytest.mark.gpu


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle_built, tmp_path_factory):
    from smalt_amd import api
    c = Ctx()
    c.seqs = rr.workload()
    c.cases = dict(rr.cases(c.seqs), fine=rr.fine_case(c.seqs))
    oix0 = ol.build_index(c.seqs, ["t%d" % i for i in range(len(c.seqs))], rr.K, rr.S)
    pre = str(tmp_path_factory.mktemp("restricted") / "ix")
    assert ol.lib().or_index_write(oix0, pre.encode()) == 0
    ol.lib().or_index_free(oix0)
    c.oix = ol.lib().or_index_read(pre.encode())
    c.sop = np.ctypeslib.as_array(c.oix.contents.sop, shape=(len(c.seqs) + 1,)).copy()
    c.gix = api.Index.load(pre, 0)
    c.oracle = functools.lru_cache(maxsize=None)(lambda name: rr.oracle_case(ol, c.oix, c.cases[name], raw=True, fine=(name == "fine")))
    yield c
    c.gix.close()


def _blocks_equal(got_text, want_text, i):
    a, b = rr.stage_lines(got_text), rr.stage_lines(want_text)
    for j, (x, y) in enumerate(zip(a, b)):
        assert x == y, "read %d, stage line %d" % (i, j)
    assert len(a) == len(b), i


def _run(ctx, name, max_len=100, check=None, debug_batch=True, refused=()):
    """Predicates, debug batch, plain batch.  refused: reads the stage must refuse with SMALTGPU_ECAP (more than 2048 intervals)"""
    from smalt_amd import api
    case = ctx.cases[name]
    reads, ivs = case["reads"], case["ivs"]
    quals = [b"I" * len(r) for r in reads]
    par = ctx.gix.default_params()
    par.ktuple_maxhit = case["ncut"]
    exp = ctx.oracle(name)
    assert all(e[0] == 0 for e in exp)
    mp = api.Mapper(ctx.gix, 2048 if max_len <= 100 else 512, max_len)      # (pools for that many average reads: these reads rank thousands of candidates)
    try:
        g = mp.cands_geometry()
        per = rr.strands_of(exp, case, ctx.sop, g["candcap"], g["lds_bytes"], long_inst=max_len > 247)
        sm = rr.summary([s for ss in per for s in ss])
        print(name, "hcap_strand", g["hcap_strand"], "candcap", g["candcap"], "lds_bytes", g["lds_bytes"], "pass 2:", g["hcap_strand2"], g["candcap2"], sm)
        first_pass = [all(s.nkeys <= g["hcap_strand"] for s in ss) for ss in per]       # reads a debug batch (one pass) can hold
        if check is None:
            rr.check_case(name, per, case)
        else:
            check(per, sm, g, first_pass)
        kw = dict(intervals=ivs, fine_index=(name == "fine"), raw_alignments=True, allow_read_errors=True)
        if debug_batch:
            mp.set_debug(1)
            res, stats, _ = mp.map_batch_ctx(reads, quals, par, **kw)
            ncmp = 0
            for i in range(len(reads)):
                if i in refused or not first_pass[i]:
                    assert stats[i]["err"] == api.ECAP, i
                    continue
                assert stats[i]["err"] == 0, (i, stats[i])
                _blocks_equal(mp.dump_read(i, "r%d" % i), exp[i][3], i)
                ncmp += 1
            print(name, "debug batch: reads compared", ncmp, "of", len(reads))
            assert ncmp >= 4
        mp.set_debug(0)
        res, stats, _ = mp.map_batch_ctx(reads, quals, par, **kw)
        for i in range(len(reads)):
            if i in refused:
                assert stats[i]["err"] == api.ECAP and not res[i], i
                continue
            assert stats[i]["err"] == 0, (i, stats[i])
            assert res[i] == exp[i][1], i
            for kk in rr.SCALARS:
                assert stats[i][kk] == exp[i][2][kk], (i, kk)
        return per, sm, g
    finally:
        mp.close()


def test_all_in_geometry_of_intervals(ctx):
    """Every strand fits the allocation (all_in).  One and two intervals, abutting, in different sequences (the last among them),
    at both ends of a sequence, shorter than k, holding no sampled serial (plo == phi), lo / hi / sop[sx] in every residue mod s;
    reads whose intervals hold no hit, a read with no interval and a read shorter than k."""
    _run(ctx, "geometry")


def test_interval_numbers_up_to_the_limit(ctx):
    """1023, 1024, 1025, 2047 and 2048 intervals with hits in the first and in the last (the interval number takes the sequence field
    of the sort key and, from 1024 on, the bit above it); the read with 2049 intervals comes back with SMALTGPU_ECAP and every
    other read of the batch equals the oracle."""
    _run(ctx, "numbers", refused=(5,))


def test_counted_decisions_in_lds_and_behind_the_ranking_arrays(ctx):
    """The sum of the hit counts exceeds the allocation; the hit info is sorted (main-index round), so the stage builds the
    rank-to-offset order: at least 20 strands with the counts in LDS and 20 with the counts behind the ranking arrays, in all of
    which the offset order differs from the rank order."""
    _run(ctx, "counted")


def test_protocol_aborts_and_halves(ctx):
    """ktuple_maxhit = 100000 and seeds of 20 000 positions behind the first serial of the interval: the fill meets the allocation
    boundary and halves the ceiling (at least 5 strands), after which the oracle's dump shows the seeds as MULTIHIT; among them
    at least 10 strands where testing the ceiling on the rank-sorted key (hashhit.c:1478) gathers other keys than testing it on
    the seed itself would."""
    _run(ctx, "halving")


def test_direct_decisions_when_the_counts_have_no_room(ctx, monkeypatch):
    """SMALTGPU_CANDS_HCAP=1024: first-pass slots of 2048 candidates, 300 intervals per read: seeds x intervals is above the
    capacity and the protocol searches the lists interval by interval (fill_decide_iv).  At least 5 of these strands belong to
    reads that stay in the first pass (at most 1024 keys per strand); the others are deferred and decided again on the second
    pass's slots."""
    monkeypatch.setenv("SMALTGPU_CANDS_HCAP", "1024")

    def check(per, sm, g, first_pass):
        assert g["hcap_strand"] == 1024 and g["candcap"] == 2048 and g["hcap_strand2"] > 1024
        rr.check_case("direct", per, ctx.cases["direct"])
        assert sum(1 for ss, ok in zip(per, first_pass) for s in ss if ok and s.branch == rr.DIRECT) >= 5
    _run(ctx, "direct", check=check)


def test_reads_deferred_to_the_second_pass(ctx, monkeypatch):
    """SMALTGPU_CANDS_HCAP=1024 and at least 20 strands that gather more than 1024 keys over their intervals: the slot overflows,
    the read is deferred (SMG_ERR_RETRY) and mapped on the second pass's slots; results equal the oracle's and err == 0.  (Plain
    batch only: a debug batch has no second pass.)"""
    monkeypatch.setenv("SMALTGPU_CANDS_HCAP", "1024")

    def check(per, sm, g, first_pass):
        assert g["hcap_strand"] == 1024 and g["hcap_strand2"] >= 32768
        assert sum(1 for ss in per for s in ss if s.nkeys > g["hcap_strand"]) >= 20
        assert max(s.nkeys for ss in per for s in ss) <= g["hcap_strand2"]
    _run(ctx, "many_keys", check=check, debug_batch=False)


def test_many_keys_in_one_pass(ctx):
    """The same reads on slots of the usual size: up to 25 000 keys per strand over two intervals, all_in."""
    _run(ctx, "many_keys")


def test_fine_round_in_a_repeat(ctx):
    """The rescue round over the on-the-fly k=5 index (kernel k_fine_index ahead of the seeding), hit info in its long form (no
    rank-to-offset order): 401 intervals in the big tandem array, 50 in the mixed one, 20 near the array's end; the sum of the
    hit counts exceeds the allocation, up to 170 000 keys per strand."""
    _run(ctx, "fine")


def test_long_read_instance(ctx):
    """A mapper for reads of up to 400 bases and reads of 300: the instance for long reads (k_cands<true>) in the all_in branch
    and in the counted branch (its counts always lie behind the ranking arrays)."""
    _run(ctx, "long", max_len=400)


def test_ceiling_of_zero_is_refused(ctx):
    """ktuple_maxhit <= 0 (no ceiling): the reference's fill then skips a seed whose tail passes the allocation boundary and goes on
    (hashhit.c:1497 with ncut == 0), which the stage's gather does not restate; the library refuses the parameter loudly."""
    from smalt_amd import api
    case = ctx.cases["geometry"]
    par = ctx.gix.default_params()
    par.ktuple_maxhit = 0
    mp = api.Mapper(ctx.gix, 4, 100)
    try:
        with pytest.raises(api.SmaltGpuError) as e:
            mp.map_batch_ctx(case["reads"][:2], None, par, intervals=case["ivs"][:2])
        assert "ktuple_maxhit" in str(e.value)
    finally:
        mp.close()

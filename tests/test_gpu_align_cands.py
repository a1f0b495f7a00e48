"""k_replay and the K3 driver (k_align<false> and k_align<true>, both passes) alone, on injected candidates with their first-pass
scores (smaltgpu_align_cands_batch), against the oracle run from the score pass on over the same candidates (or_map_injected).
Per read: the scalars k_replay leaves (n_scored, max1, max2, the three thresholds, go), the error code, the running score maxima
and the result list in order, field by field, with the first-of-candidate mark and every DiffStr byte.  Everything is integer:
the comparisons are exact.  The families and their conditions are those of align_cands_data.py (asserted on the oracle's output
before anything is compared; proven without a GPU in test_align_cands_paths.py)."""
import time

import pytest

import align_cands_data as ad
import oracle_lib as ol

pytestmark = pytest.mark.gpu
SHORT = ["a", "b", "cd", "e", "f", "g", "h", "i", "j", "k", "l", "m", "n"]


def _open(seqs, tmp, name, nreads, max_len):
    from smalt_amd import api
    oix, pre = ad.build_index(seqs, tmp, name)
    gix = api.Index.load(pre, 0)
    return oix, gix, api.Mapper(gix, nreads, max_len)


@pytest.fixture(scope="module")
def short_env(oracle_built, tmp_path_factory):
    """one index and one mapper for reads of up to 150 bases (k_align<false>) for the short driver and the O1 lists"""
    oix, gix, mp = _open(ad.world()["seqs"], tmp_path_factory.mktemp("acgpu"), "ac", 512, 150)
    yield oix, gix, mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


def report(fam, nali, ndef, t0, extra=""):
    print("ALIGN_CANDS %s: %d reads, %d candidates, %d alignments compared, %d reads deferred, %.2f s %s"
          % (fam["name"], len(fam["reads"]), sum(len(c) for c in fam["cands"]), nali, ndef, time.time() - t0, extra))


def oracle_of(oix, fam):
    exp = ad.oracle_eval(oix, fam)
    raw = ad.oracle_eval(oix, fam, raw=True, fill=False) if fam["name"].startswith("cd-") else None
    ad.check_family(fam, exp, raw)
    return exp


# (a) .. (k) run a second time with narrow bands in the anti-diagonal form
@pytest.mark.parametrize("name,antidiag", [(n, False) for n in SHORT] + [(n, True) for n in ad.SHORT_ANTIDIAG],
                         ids=SHORT + [n + "-antidiag" for n in ad.SHORT_ANTIDIAG])
def test_short_driver_matches_oracle(name, antidiag, short_env):
    oix, gix, mp = short_env
    t0 = time.time()
    fam = ad.world()["fams"][name]
    exp = oracle_of(oix, fam)
    got, ndef = ad.device_run(mp, gix, fam, antidiag=antidiag, allow_read_errors="expect_err" in fam)
    nali = ad.compare(fam, exp, got, fam.get("expect_err"))
    if name == "m":
        assert ndef == 1 and len(got[0]["results"]) == ad.UNIT_N       # more alignments than a first-pass result slot holds
    else:
        assert ndef == 0
    report(fam, nali, ndef, t0, "antidiag" if antidiag else "")


_LISTS = {}


@pytest.mark.parametrize("best,below_max,min_swatscor", ad.O1_COMBOS)
def test_replay_lists_match_oracle(best, below_max, min_swatscor, short_env):
    oix, gix, mp = short_env
    t0 = time.time()
    if not _LISTS:
        _LISTS["l"] = ad.o1_lists(ad.SEQLENS)
        from smalt_amd import api
        _LISTS["packed"] = api.Mapper.pack_cands(_LISTS["l"][1])
    fam = ad.o1_family(ad.SEQLENS, best, below_max, min_swatscor, lists=_LISTS["l"])
    fam["packed"] = _LISTS["packed"]
    exp = ad.oracle_eval(oix, fam)
    assert all(e["rv"] == 0 for e in exp)
    counts = ad.check_o1(fam, exp)
    got, ndef = ad.device_run(mp, gix, fam, min_sw_per_read=below_max == 5)      # (two of the combinations: the threshold per read, as rmapPair passes it)
    nali = ad.compare(fam, exp, got)
    assert ndef == 0
    report(fam, nali, ndef, t0, str(counts))


def test_hand_derived_lists(short_env):
    """three lists with literal expected values, so that the oracle is not the only judge (align_cands_data.hand_lists)"""
    oix, gix, mp = short_env
    for fam, lit in ad.hand_lists(ad.SEQLENS):
        exp = ad.oracle_eval(oix, fam)
        got, _ = ad.device_run(mp, gix, fam)
        for g, want in zip(got, lit):
            for f, v in want.items():
                assert g["ctl"][f] == v, (fam["name"], f, g["ctl"], v)
        ad.compare(fam, exp, got)


def test_entry_refuses_what_production_cannot_produce(short_env):
    """preconditions are answered with SMALTGPU_EARG, never repaired"""
    from smalt_amd import api
    oix, gix, mp = short_env
    fam = ad.world()["fams"]["i"]
    oracle_of(oix, fam)
    good = fam["cands"][0][0]
    par = gix.default_params()
    for bad in (dict(good, swscor=151), dict(good, swscor=-1), dict(good, sqidx=3), dict(good, re=ad.SEQLENS[good["sqidx"]]), dict(good, rs=good["re"] + 1)):
        with pytest.raises(api.SmaltGpuError) as e:
            mp.align_cands_batch(fam["reads"], par, [[bad]])
        assert e.value.code == -3
    got, _ = ad.device_run(mp, gix, fam)                     # the mapper still works
    assert len(got[0]["results"]) == 1


def test_wide_driver_matches_oracle(oracle_built, tmp_path):
    """k_align<true>: the row form, the two-column wave form and the strip form, each predicted by the host rule for one read at least"""
    t0 = time.time()
    W = ad.wide_world()
    oix, gix, mp = _open(W["seqs"], tmp_path, "wide", 16, 600)
    try:
        fam = W["fam"]
        exp = oracle_of(oix, fam)
        got, ndef = ad.device_run(mp, gix, fam)
        nali = ad.compare(fam, exp, got)
        assert ndef == 0
        report(fam, nali, ndef, t0)
    finally:
        mp.close()
        gix.close()
        ol.lib().or_index_free(oix)


def test_wide_driver_defers_bands_to_the_second_pass(oracle_built, tmp_path, monkeypatch):
    """first-pass direction-matrix slots of 4096 bytes: both reads wait for the second launch and come out the same"""
    t0 = time.time()
    monkeypatch.setenv("SMALTGPU_ALIGN_DIRCAP", str(ad.WIDE_DIRCAP))
    W = ad.wide_world()
    oix, gix, mp = _open(W["seqs"], tmp_path, "wide", 16, ad.WIDE_DEFER_MAXLEN)
    try:
        fam = W["fdef"]
        exp = oracle_of(oix, fam)
        got, ndef = ad.device_run(mp, gix, fam)
        nali = ad.compare(fam, exp, got)
        assert ndef >= 1
        report(fam, nali, ndef, t0)
    finally:
        mp.close()
        gix.close()
        ol.lib().or_index_free(oix)

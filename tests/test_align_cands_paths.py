"""O1 and the K3 driver on injected candidates without a GPU: stage_replay and stage_align from the product's headers, built for the
host with one lane (tests/hostemu/align_cands_check.cpp), over the families of align_cands_data.py against the oracle
(or_map_injected).  Each family's own conditions are asserted here on the oracle's output, so the GPU test, which uses the same
families, cannot pass on empty cases.  The program runs once more built with the address and undefined-behaviour sanitizers, as a
stand-alone binary with the runtimes linked in, and must print what the plain build prints."""
import os
import subprocess

import pytest

import align_cands_data as ad
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "align_cands_check.cpp")
SHORT = ["a", "b", "cd", "e", "f", "g", "h", "i", "j", "k", "l", "m", "n"]


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-o", exe, SRC] + flags, check=True)
    return exe


@pytest.fixture(scope="module")
def check_bin(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("aligncands"), "align_cands_check", ["-O2"])


@pytest.fixture(scope="module")
def check_bin_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("aligncands_san"), "align_cands_check_san",
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])


@pytest.fixture(scope="module")
def short_index(oracle_built, tmp_path_factory):
    oix, pre = ad.build_index(ad.world()["seqs"], tmp_path_factory.mktemp("acix"))
    yield oix, pre
    ol.lib().or_index_free(oix)


@pytest.fixture(scope="module")
def wide_index(oracle_built, tmp_path_factory):
    oix, pre = ad.build_index(ad.wide_world()["seqs"], tmp_path_factory.mktemp("acwide"), "wide")
    yield oix, pre
    ol.lib().or_index_free(oix)


def run_host(exe, pre, fam, tmp):
    path = str(tmp / (fam["name"] + ".txt"))
    ad.write_host_batch(path, fam)
    p = subprocess.run([exe, pre, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return p.stdout


def oracle_of(oix, fam):
    exp = ad.oracle_eval(oix, fam)
    raw = ad.oracle_eval(oix, fam, raw=True, fill=False) if fam["name"].startswith("cd-") else None
    ad.check_family(fam, exp, raw)
    return exp


@pytest.mark.parametrize("name", SHORT)
def test_short_driver_one_lane_matches_oracle(name, short_index, check_bin, tmp_path):
    oix, pre = short_index
    fam = ad.world()["fams"][name]
    exp = oracle_of(oix, fam)
    got = ad.parse_host_output(run_host(check_bin, pre, fam, tmp_path))
    ad.compare(fam, exp, got, fam.get("expect_err"))


@pytest.mark.parametrize("which", ["fam", "fdef"], ids=["forms", "deferred-reads"])
def test_wide_driver_one_lane_matches_oracle(which, wide_index, check_bin, tmp_path):
    oix, pre = wide_index
    fam = ad.wide_world()[which]
    exp = oracle_of(oix, fam)
    assert ad.compare(fam, exp, ad.parse_host_output(run_host(check_bin, pre, fam, tmp_path))) >= len(fam["reads"])


_LISTS = {}


def o1_lists():
    if not _LISTS:
        _LISTS["l"] = ad.o1_lists(ad.SEQLENS)
    return _LISTS["l"]


@pytest.mark.parametrize("best,below_max,min_swatscor", ad.O1_COMBOS)
def test_replay_lists_one_lane_match_oracle(best, below_max, min_swatscor, short_index, check_bin, tmp_path):
    oix, pre = short_index
    fam = ad.o1_family(ad.SEQLENS, best, below_max, min_swatscor, lists=o1_lists())
    exp = ad.oracle_eval(oix, fam)
    assert all(e["rv"] == 0 for e in exp)
    ad.check_o1(fam, exp)
    ad.compare(fam, exp, ad.parse_host_output(run_host(check_bin, pre, fam, tmp_path)))


def test_hand_derived_lists(short_index, check_bin, tmp_path):
    """the three lists whose expected values are literals: the oracle and the one-lane stage must both give them"""
    oix, pre = short_index
    for fam, lit in ad.hand_lists(ad.SEQLENS):
        exp = ad.oracle_eval(oix, fam)
        got = ad.parse_host_output(run_host(check_bin, pre, fam, tmp_path))
        for e, g, want in zip(exp, got, lit):
            for f, v in want.items():
                assert e["ctl"][f] == v and g["ctl"][f] == v, (fam["name"], f, e["ctl"], g["ctl"], v)
        ad.compare(fam, exp, got)


def test_one_lane_stages_under_sanitizers(short_index, wide_index, check_bin, check_bin_san, tmp_path):
    """every family once more through the program built with -fsanitize=address,undefined: it ends clean and prints the same"""
    oix, pre = short_index
    fams = [ad.world()["fams"][n] for n in SHORT]
    for fam in fams:
        if fam["rescore"]:
            ad.oracle_eval(oix, fam)                     # fills in the first-pass scores
    fams += [f for f, _ in ad.hand_lists(ad.SEQLENS)]
    fams += [ad.o1_family(ad.SEQLENS, True, 0, ad.K + ad.S - 1, lists=o1_lists()), ad.o1_family(ad.SEQLENS, False, -1, 60, lists=o1_lists())]
    for fam in fams:
        assert run_host(check_bin_san, pre, fam, tmp_path) == run_host(check_bin, pre, fam, tmp_path), fam["name"]
    woix, wpre = wide_index
    for which in ("fam", "fdef"):
        fam = ad.wide_world()[which]
        ad.oracle_eval(woix, fam)
        assert run_host(check_bin_san, wpre, fam, tmp_path) == run_host(check_bin, wpre, fam, tmp_path), fam["name"]

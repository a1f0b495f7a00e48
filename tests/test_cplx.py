"""Complexity-weighted alignment scores (smalt map -w) on the host: the scaling function of the device path
(smalt_amd/csrc/smg_cplx.hpp, the function k_align calls) and the host's lambda (smg_cplx.cpp), built into a stand-alone
program (tests/hostemu/cplx_check.cpp), against the reference program's own output.  tests/golden/cplx.* holds what
`smalt map -d 3 -r -1` printed for the reads of tests/cplx_data.py with and without -w (tests/golden/make_golden_cplx.py):
wherever -w left placement and CIGAR of a line alone, its score must be the unweighted score scaled by the letter counts of
the reference under the line's M stretches -- which pins the formula, the order of the letter codes, the order of the
floating-point operations and lambda, to the bit."""
import gzip
import os
import subprocess

import pytest

import cplx_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cplx") / "cplx_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "hostemu", "cplx_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), check=True, capture_output=True, text=True).stdout
        return out.split("\n")[:len(lines)]
    return run


def _gold(name):
    with gzip.open(os.path.join(GOLD, name), "rb") as g:
        return g.read()


def test_lambda_is_the_reference_bisection(check):
    pairs = [(1, -2), (2, -3), (1, -1)]
    got = [float.fromhex(x) for x in check(["L %d %d" % p for p in pairs])]
    for p, g in zip(pairs, got):
        assert g == cplx_data.calc_lambda(*p), (p, g.hex())
    assert got[0] == 1.3327102661132812


def test_scaling_turns_the_unweighted_score_into_the_reference_w_score(check):
    ref = {}
    name = None
    for ln in _gold("cplx.fa.gz").split(b"\n"):
        if ln.startswith(b">"):
            name = ln[1:].split()[0]
            ref[name] = []
        elif ln:
            ref[name].append(ln)
    ref = {k: b"".join(v) for k, v in ref.items()}
    # the -w lines by everything but the score and the mapping quality: read, reference, both ends, the operations
    weighted = {}
    for ln in _gold("cplx.cigar_w.out.gz").split(b"\n"):
        t = ln.split()
        f = cplx_data.cigar_fields(ln)
        if f:
            weighted[(tuple(t[1:9]), tuple(t[10:]))] = f[4]
    nreads = _gold("cplx.fq.gz").count(b"\n") // 4
    nlines = len(weighted)
    assert nreads == cplx_data.NPAIRS and nlines >= 300
    req, want = ["L 1 -2"], []
    for ln in _gold("cplx.cigar.out.gz").split(b"\n"):
        t = ln.split()
        f = cplx_data.cigar_fields(ln)
        if not f:
            continue
        key = (tuple(t[1:9]), tuple(t[10:]))
        if key not in weighted:
            continue
        cnt = cplx_data.m_counts(f, ref)
        req.append("S %d %s" % (f[4], " ".join(str(c) for c in cnt)))
        want.append((f[4], weighted[key], ln))
    got = check(req)[1:]
    lower = 0
    for (orig, w, ln), g in zip(want, got):
        assert g == "0 %d" % w, (ln, g, w)
        lower += w < orig
    print("reads %d, -w lines %d, checked %d, lower under -w %d" % (nreads, nlines, len(want), lower))
    # At least half of the fixture's lines are checked this way.  The lines counted are those of the -w output, one or two per
    # read: without -w the same run lists every placement of a read inside a repeat within 3 of its best score (over 1300 lines for
    # 400 reads), most of which -w prunes, so the two files do not pair up line by line; every checked line is a -w line.
    assert 2 * len(want) >= nlines and 2 * len(want) >= nreads
    assert 20 * lower >= len(want)               # at least 5 % of them score lower under -w


def test_balanced_composition_exceeds_the_unweighted_score(check):
    """exactly 1000 each of A, C, G and T: the reference's cut-off ln(1/4) leaves a positive rest, ERRCODE_CPLXSCOR"""
    out = check(["L 1 -2", "S 4000 1000 1000 1000 1000 0 0", "S 4000 999 1001 1000 1000 0 0"])
    assert out[1].split()[0] == "1"
    assert out[2] == "0 %d" % cplx_data.scale([999, 1001, 1000, 1000, 0, 0], 4000, cplx_data.calc_lambda(1, -2))
    assert cplx_data.scale([1000, 1000, 1000, 1000, 0, 0], 4000, cplx_data.calc_lambda(1, -2)) is None
    assert cplx_data.scale([999, 1001, 1000, 1000, 0, 0], 4000, cplx_data.calc_lambda(1, -2)) in (3999, 4000)

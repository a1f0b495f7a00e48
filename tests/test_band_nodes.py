"""The banded passes without a GPU: the one-lane forms of K2b and K3 from the product's headers (tests/hostemu/band_node_check.cpp)
on the tasks the GPU tests use (band_data.py), the K3 recursion driven from Python with that program as the node evaluator, and
everything held against the oracle.  Checked here on the oracle alone, per case list: at most 5 % of the tasks end in
OR_ERR_SWATSCOR (and those are compared, not skipped), at most 10 % yield no alignment, one task at least has two cells that tie
for the maximum, and one at least recurses to depth 2 or more -- so the GPU tests, which use the same lists, are about
alignments, ties and recursions and not about empty results.  The host rules (smaltgpu_band_geometry: the band's fields and the
form the mapper would pick) are held against a plain restatement, and the program runs once more under the address and
undefined-behaviour sanitizers (the runtimes linked into the program itself), stand-alone, on the generated cases."""
import os
import subprocess

import numpy as np
import pytest

import band_data as bd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "band_node_check.cpp")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-o", exe, SRC] + flags, check=True)
    return exe


@pytest.fixture(scope="module")
def node_bin(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("bandnode"), "band_node_check", ["-O2"])


@pytest.fixture(scope="module")
def node_bin_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("bandnode_san"), "band_node_check_san",
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])


def write_tasks(path, pen, minscore, items):
    """items: (mode, task, (s_left, s_right))"""
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %d\n" % (pen + (minscore, len(items))))
        for mode, t, iv in items:
            f.write("%d %d %d %d %d %d %d %d %d\n" % ((mode, len(t["q"]), len(t["w"])) + tuple(t["band"]) + tuple(iv)))
            f.write("".join(chr(48 + c) for c in t["q"]) + "\n" + "".join(chr(48 + c) for c in t["w"]) + "\n")


def run_program(exe, path):
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    return p.stdout.split("\n")[:-1]


def parse_nodes(lines):
    out = []
    for ln in lines:
        f = ln.split()
        assert f[0] == "NODE"
        out.append(dict(status=int(f[1]), score=int(f[2]), max_i=int(f[3]), max_j=int(f[4]), qs=int(f[5]), rs=int(f[6]),
                        diffstr=b"" if f[7] == "-" else bytes.fromhex(f[7])))
    return out


def host_evaluator(exe, tmp, pen, minscore):
    n = [0]

    def evaluate(nodes):
        path = str(tmp / ("nodes%d.txt" % n[0]))
        n[0] += 1
        write_tasks(path, pen, minscore, [(1, t, iv) for t, iv in nodes])
        return parse_nodes(run_program(exe, path))
    return evaluate


_ORACLE = {}


def oracle_results(form, pen):
    """or_sw_band_full on the root of every task of a case list, computed once per (form, penalties)"""
    key = (form, pen)
    if key not in _ORACLE:
        M = bd.score_matrix(pen[0], pen[1])
        tasks = bd.cases_of(form, 0)
        _ORACLE[key] = (tasks, [bd.or_band_full(t, pen, M, bd.minscore_of(pen)) for t in tasks])
    return _ORACLE[key]


@pytest.mark.parametrize("pen", bd.PENS, ids=bd.PEN_IDS)
@pytest.mark.parametrize("form", range(9), ids=bd.FORM_NAMES)
def test_case_lists_hold_alignments_ties_and_recursions(form, pen, oracle_built):
    """the conditions on the case lists, on the oracle alone"""
    tasks, exp = oracle_results(form, pen)
    M = bd.score_matrix(pen[0], pen[1])
    n = len(tasks)
    nerr = sum(rv == bd.OR_ERR_SWATSCOR for rv, _ in exp)
    nempty = sum(rv == bd.OR_OK and not alis for rv, alis in exp)
    assert all(rv in (bd.OR_OK, bd.OR_ERR_SWATSCOR) for rv, _ in exp)
    assert nerr <= 0.05 * n, (nerr, n)
    assert nempty <= 0.10 * n, (nempty, n)
    assert any(alis and bd.has_diagonal_tie(t, pen, M, alis[0][0]) for (rv, alis), t in zip(exp, tasks) if t["kind"] == "periodic"), "no tie"
    assert any(len(alis) >= 2 for _, alis in exp), "no recursion below the root"


@pytest.mark.parametrize("pen", bd.PENS, ids=bd.PEN_IDS)
@pytest.mark.parametrize("form", range(9), ids=bd.FORM_NAMES)
def test_recursion_over_one_lane_nodes_matches_oracle(form, pen, node_bin, oracle_built, tmp_path):
    """the Python recursion driver of the GPU test with the product's one-lane node as the evaluator: the full list per task
    (score, qs, qe, rs, re, DiffStr) and the return code against one or_sw_band_full call on the root"""
    tasks, exp = oracle_results(form, pen)
    minscore = bd.minscore_of(pen)
    got = bd.run_recursion(tasks, pen, minscore, host_evaluator(node_bin, tmp_path, pen, minscore))
    assert max(d for _, _, d in got) >= 2
    for i, ((rv, alis, _), (erv, ealis)) in enumerate(zip(got, exp)):
        assert rv == erv, (i, tasks[i]["kind"], tasks[i]["band"], rv, erv)
        assert alis == ealis, (i, tasks[i]["kind"], tasks[i]["band"], alis, ealis)


@pytest.mark.parametrize("pen", bd.PENS, ids=bd.PEN_IDS)
def test_k2b_one_lane_matches_oracle(pen, node_bin, oracle_built, tmp_path):
    M = bd.score_matrix(pen[0], pen[1])
    phases = set()
    for ql in bd.K2B_QLENS:
        tasks = bd.k2b_cases(np.random.default_rng(500 + ql), ql)
        path = str(tmp_path / ("k2b%d.txt" % ql))
        write_tasks(path, pen, 1, [(0, t, (0, len(t["w"]) - 1)) for t in tasks])
        lines = run_program(node_bin, path)
        assert len(lines) == len(tasks)
        nband = 0
        for i, (t, ln) in enumerate(zip(tasks, lines)):
            rv, sc = bd.or_band_fast(t, pen, M)
            assert rv in (bd.OR_OK, bd.OR_ERR_BAND)
            assert ln == "K2B %d %d" % (1 if rv == bd.OR_ERR_BAND else 0, sc), (ql, i, t["kind"], t["band"], ln, rv, sc)
            nband += rv == bd.OR_ERR_BAND
            phases.add(i % 10)
        assert 1 <= nband <= 2                 # the band that misses the read, and nothing else
    assert len(phases) == 10


def test_band_geometry_matches_restatement():
    """smaltgpu_band_geometry (band_init and the form the mapper picks) against py_band / py_form over random and edge bands"""
    from smalt_amd import api
    rng = np.random.default_rng(99)
    cases = []
    for _ in range(4000):
        qlen, wlen = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
        bl = int(rng.integers(-wlen - 50, qlen + 50))
        nd = int(rng.choice([0, 1, 2, 16, 17, 64, 65, 128, 129, 255, 256, 257, 512, 896, 897, 1536, 1537, 2047, 2048, 2100]))
        qs, qe = int(rng.integers(-2, qlen + 2)), int(rng.integers(-2, qlen + 2))
        s_left = int(rng.integers(-2, wlen + 2)) if rng.random() < 0.5 else 0
        s_right = int(rng.integers(-2, wlen + 2)) if rng.random() < 0.5 else wlen - 1
        gi, ge = (4, 3) if rng.random() < 0.7 else (2, 4)
        cases.append((bl, bl + nd - 1 - (3 if nd == 0 else 0), qs, qe, qlen, s_left, s_right, wlen, gi, ge))
    forms = set()
    for c in cases:
        exp = bd.py_band(*c[:8])
        got = api.band_geometry(*c[:8], -c[8], -c[9])
        if exp is None:
            assert got is None, c
            continue
        assert got is not None, c
        form = got.pop("form")
        assert got == exp, (c, got, exp)
        assert form == bd.py_form(exp, c[8], c[9]), (c, form)
        assert bd.form_ok(form, exp, c[8], c[9])
        forms.add(form)
    # with room for every direction layout a band of 256 diagonals and more always takes a strip form, so the wave forms of 4, 7 and
    # 12 columns per lane and the one-lane form are never the mapper's choice here (they are when the strips do not fit)
    assert forms == {bd.ROWS, bd.ANTIDIAG, bd.WAVE2, bd.STRIP8, bd.STRIP16}


def test_one_lane_forms_under_sanitizers(node_bin, node_bin_san, oracle_built, tmp_path):
    """the program with -fsanitize=address,undefined, stand-alone, on every case list (roots and the second round of the
    recursion) and on the K2b tasks: it ends clean and prints what the plain build prints"""
    pen = bd.PENS[0]
    minscore = bd.minscore_of(pen)
    for form in range(9):
        tasks, _ = oracle_results(form, pen)
        rounds = []

        def evaluate(nodes, rounds=rounds):
            path = str(tmp_path / ("san_f%d_r%d.txt" % (form, len(rounds))))
            write_tasks(path, pen, minscore, [(1, t, iv) for t, iv in nodes])
            plain = run_program(node_bin, path)
            if len(rounds) < 2:
                assert run_program(node_bin_san, path) == plain
            rounds.append(path)
            return parse_nodes(plain)
        bd.run_recursion(tasks, pen, minscore, evaluate)
        assert len(rounds) >= 2
    for ql in (20, 256, 1025):
        tasks = bd.k2b_cases(np.random.default_rng(500 + ql), ql)
        path = str(tmp_path / ("san_k2b%d.txt" % ql))
        write_tasks(path, bd.PENS[4], 1, [(0, t, (0, len(t["w"]) - 1)) for t in tasks])
        assert run_program(node_bin_san, path) == run_program(node_bin, path)

"""The sampling grid of the index construction when the step exceeds the word length (`-s` > `-k`), without a GPU.  The rule is stated
once in plain Python (tests/index_ref.py) and held here against the reference program (`smalt index` of oracle/_ref, where it was
built), against the oracle's builder (oracle/or_index.c) and against the product's own statement of the walk (index_carry of
smalt_amd/csrc/smg_indexbuild.h, through the stand-alone program tests/hostemu/index_carry_check.cpp, plain and under sanitizers).

200 seeded tiny references, half of them with k < s <= k + 12.  For s > k the reference either refuses the reference sequences
(hashidx.c:494: the offset carried from one sequence to the next reaches the step), or builds with the global grid's positions and
a `maxpos` that may be one above ceil(tot / s) - 1 (hashidx.c:524-528 after the last sequence)."""
import os
import subprocess

import pytest

import index_ref as ir
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
CASES = ir.tiny_cases()
CLASSES = [ir.classify([len(q) for q in seqs], k, s) for k, s, seqs in CASES]


def _names(seqs):
    return ["s%d" % i for i in range(len(seqs))]


def test_the_sample_holds_every_class():
    """at least 20 references the reference refuses, 20 it builds with maxpos one over the grid's, 20 it builds with s > k and the
    grid's maxpos; and the references with s <= k are neither refused nor off the grid"""
    n = {c: CLASSES.count(c) for c in ("refused", "over", "grid", "plain")}
    print(n)
    assert n["refused"] >= 20 and n["over"] >= 20 and n["grid"] >= 20, n
    assert sum(1 for (k, s, _) in CASES if k < s <= k + 12) >= 100
    for (k, s, seqs), c in zip(CASES, CLASSES):
        lens = [len(q) for q in seqs]
        assert 3 <= k <= 20 and 1 <= s <= 127 and 1 <= len(seqs) <= 7 and all(k <= n <= k + 3 * s + 10 for n in lens)
        if s <= k:
            assert c == "plain" and ir.carry(lens, k, s) == (None, ir.grid_maxpos(lens, s))


@pytest.fixture(scope="module")
def reference_runs(tmp_path_factory):
    """`smalt index` of the reference on every case -> (exit code, stderr, prefix)"""
    if not os.path.exists(REF_SMALT):
        pytest.skip("oracle/_ref/smalt is not built (the reference's sources are not on this machine)")
    d = tmp_path_factory.mktemp("refix")
    runs = []
    for j, (k, s, seqs) in enumerate(CASES):
        fa, pre = str(d / ("c%d.fa" % j)), str(d / ("c%d" % j))
        with open(fa, "wb") as f:
            for name, q in zip(_names(seqs), seqs):
                f.write(b">" + name.encode() + b"\n" + q + b"\n")
        r = subprocess.run([REF_SMALT, "index", "-k", str(k), "-s", str(s), pre, fa], capture_output=True)
        runs.append((r.returncode, r.stderr.decode(errors="replace"), pre))
    return runs


def test_rule_against_the_reference_program(reference_runs):
    """refusal, maxpos, npos, the index type and the sorted position words of every case"""
    for j, ((k, s, seqs), (rc, err, pre)) in enumerate(zip(CASES, reference_runs)):
        lens = [len(q) for q in seqs]
        bad, maxpos = ir.carry(lens, k, s)
        if bad is not None:
            assert rc == 1 and "arguments outside expected range" in err, (j, k, s, lens, rc, err)
            continue
        assert rc == 0, (j, k, s, lens, err)
        smi = ir.read_smi(pre + ".smi")
        want = ir.grid_positions(seqs, k, s)
        assert (smi["k"], smi["s"]) == (k, s)
        assert smi["maxpos"] == maxpos, (j, k, s, lens)
        assert smi["npos"] == len(want), (j, k, s, lens)
        assert sorted(smi["pos"]) == want, (j, k, s, lens)
        assert (smi["typ"], smi["nbits_key"], smi["nbits_lo"]) == ir.geometry(k, s, sum(lens)), (j, k, s, lens)


def _oracle_files(seqs, k, s, prefix):
    """the oracle's index files, or None where its builder refuses"""
    import ctypes as C
    n = len(seqs)
    names = [x.encode() for x in _names(seqs)]
    oix = ol.lib().or_index_build(n, (C.c_char_p * n)(*seqs), (C.c_uint32 * n)(*[len(q) for q in seqs]), (C.c_char_p * n)(*names), k, s)
    if not oix:
        return None
    try:
        assert ol.lib().or_index_write(oix, prefix.encode()) == 0
    finally:
        ol.lib().or_index_free(oix)
    return open(prefix + ".sma", "rb").read(), open(prefix + ".smi", "rb").read()


def test_oracle_builder_follows_the_rule(oracle_built, tmp_path):
    """or_index_build returns NULL exactly where the rule refuses; elsewhere its file carries the rule's maxpos and the grid's positions"""
    for j, (k, s, seqs) in enumerate(CASES):
        lens = [len(q) for q in seqs]
        bad, maxpos = ir.carry(lens, k, s)
        got = _oracle_files(seqs, k, s, str(tmp_path / "o"))
        if bad is not None:
            assert got is None, (j, k, s, lens)
            continue
        assert got is not None, (j, k, s, lens)
        smi = ir.read_smi(str(tmp_path / "o.smi"))
        assert smi["maxpos"] == maxpos and sorted(smi["pos"]) == ir.grid_positions(seqs, k, s), (j, k, s, lens)


def test_oracle_builder_against_the_reference_program(oracle_built, reference_runs, tmp_path):
    """where the reference builds, the oracle's files are the reference's byte for byte; where it refuses, the oracle returns NULL"""
    for j, ((k, s, seqs), (rc, err, pre)) in enumerate(zip(CASES, reference_runs)):
        got = _oracle_files(seqs, k, s, str(tmp_path / "o"))
        if rc != 0:
            assert got is None, (j, k, s)
            continue
        assert got is not None, (j, k, s)
        assert got[0] == open(pre + ".sma", "rb").read(), (j, k, s)
        assert got[1] == open(pre + ".smi", "rb").read(), (j, k, s)


# ---- the product's statement of the walk: index_carry of smg_indexbuild.h, on the host ----------------------------------------------
LONG = [(13, 20, [2**31 - 1, 13, 2**31 - 1]), (3, 127, [2**31 - 1] * 3), (20, 21, [20] * 7), (8, 13, [203]), (8, 13, [207]),
        (13, 6, [2**31 - 1, 2**31 - 1]), (20, 127, [2**31 - 1] * 100), (5, 9, [5, 5, 5]), (3, 4, [3] * 50)]


def _carry_lines():
    jobs = [(k, s, [len(q) for q in seqs]) for k, s, seqs in CASES] + LONG
    text = "".join("%d %d %d %s\n" % (k, s, len(lens), " ".join(map(str, lens))) for k, s, lens in jobs)
    want = []
    for k, s, lens in jobs:
        bad, maxpos = ir.carry(lens, k, s)
        want.append("refused %d" % bad if bad is not None else "built %d" % maxpos)
    return text, want


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "sanitized"])
def test_index_carry_of_the_library_on_the_host(sanitized, tmp_path):
    """tests/hostemu/index_carry_check.cpp includes smg_indexbuild.h and nothing else of the library; once built plainly and once with
    -fsanitize=address,undefined (the runtimes linked into the program itself).  The 200 cases plus sequences of 2^31 - 1 bases."""
    exe = str(tmp_path / "index_carry_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"] if sanitized else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "hostemu", "index_carry_check.cpp")], check=True)
    text, want = _carry_lines()
    r = subprocess.run([exe], input=text.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stderr == b""
    got = r.stdout.decode().split("\n")[:-1]
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, (n, g, w)


def test_geometry_and_path_at_the_shapes_the_gpu_tests_use():
    """index_ref.geometry is held against the reference's files above; here the values tests/test_gpu_index_shapes.py builds on: the
    switch between the perfect and the hashed type sits where 4^k <= 2 * (tot / s)"""
    assert ir.path(8, 3, 98304) == "k32" and ir.path(8, 3, 98303) == "hash"
    assert ir.geometry(8, 3, 98304) == (ir.IDX_PERFECT, 16, 0)
    assert ir.geometry(13, 6, 39) == (ir.IDX_HASH32MIX, 2, 0)
    assert ir.geometry(20, 127, 15600) == (ir.IDX_HASH32MIX, 9, 8)
    assert ir.path(11, 1, 2_200_000) == "k32" and ir.path(11, 2, 500) == "hash" and ir.path(4, 1, 5000) == "k32"
    with pytest.raises(ValueError):
        ir.path(16, 1, 1 << 31)                   # a perfect index with k = 16: the builder refuses it

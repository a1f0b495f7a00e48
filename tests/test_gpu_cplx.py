"""Complexity-weighted alignment scores (smalt map -w) end to end against the unmodified reference program (oracle/_ref/smalt,
built by build() and shipped with the tree): `smaltgpu-map -w` must print the lines `smalt map -w` prints -- single reads under
eight sets of options, pairs, long reads (k_align<true>, the strip traceback) -- stop at the read the reference stops at with
"complexity weighted score exceeds unweighted score", and the library flag SMALTGPU_FLG_CMPLXW must give the reference's
scores.  The input (tests/cplx_data.py) has a low-complexity insert every 400-900 bases, so -w changes a third of the lines."""
import os
import subprocess

import pytest

import cplx_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
needs_ref = pytest.mark.skipif(not os.path.exists(SMALT), reason="reference binary not built (make -C oracle ref)")
SENTENCE = b"complexity weighted score exceeds unweighted score"


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """index (k 11, s 3), the read files and the runs made so far (once for the module)"""
    tmp = str(tmp_path_factory.mktemp("cplx"))
    w = cplx_data.prepare(tmp, SMALT)
    w.update(tmp=tmp, runs={})
    return w


def _lines(path):
    return [ln for ln in open(path, "rb").read().split(b"\n") if not ln.startswith(b"@PG")]


def _map(w, who, opts, files, block="256"):
    """lines (without @PG) of one `map` run of the reference (who = 'ref') or of smaltgpu-map in blocks of `block` reads; runs are kept"""
    key = (who, block if who != "ref" else "") + tuple(opts) + tuple(files)
    if key not in w["runs"]:
        out = os.path.join(w["tmp"], "map_%d.out" % len(w["runs"]))
        cmd = [SMALT, "map"] + opts if who == "ref" else [PROG] + opts + ["-B", block]
        r = subprocess.run(cmd + ["-o", out, w["pre"]] + files, capture_output=True)
        assert r.returncode == 0, (cmd, r.stderr.decode()[-2000:])
        w["runs"][key] = _lines(out)
    return w["runs"][key]


def _same_as_reference(w, opts, files, block="256"):
    ref_w, ref_0 = _map(w, "ref", ["-w"] + opts, files), _map(w, "ref", opts, files)
    got_w, got_0 = _map(w, "prog", ["-w"] + opts, files, block), _map(w, "prog", opts, files, block)
    # not vacuous: -w changes lines, in the reference and here
    assert ref_w != ref_0 and got_w != got_0
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(ref_w, got_w)) if x != y]
    assert len(got_w) == len(ref_w) and not diff, (len(ref_w), len(got_w), len(diff), diff[:3])
    assert got_0 == ref_0
    return ref_w, ref_0


SINGLE = {
    "d3": ["-f", "cigar", "-d", "3", "-r", "-1"],
    "all": ["-f", "cigar", "-d", "-1", "-r", "-1"],
    "best": ["-f", "cigar", "-r", "-1"],
    "x_d3": ["-f", "cigar", "-x", "-d", "3", "-r", "-1"],
    "split_sam": ["-p", "-r", "5", "-f", "sam"],
    "scores": ["-f", "cigar", "-S", "match=2,subst=-3,gapopen=-6,gapext=-4", "-d", "4", "-r", "-1"],
    "sam_d3": ["-f", "sam", "-d", "3", "-r", "-1"],
}


@needs_ref
@pytest.mark.parametrize("case", sorted(SINGLE))
def test_single_reads_print_the_reference_programs_lines(world, case):
    ref_w, ref_0 = _same_as_reference(world, SINGLE[case], [world["fq1"]])
    if case == "best":
        # the reference's quirk at -d 0: the threshold is the unweighted best score, so a read whose weighted score falls
        # below it comes out unmapped
        unmapped = lambda lines: sum(1 for ln in lines if ln.startswith(b"cigar:") and ln.split()[5] == b"*")
        assert unmapped(ref_w) > unmapped(ref_0) + 20


@needs_ref
def test_single_reads_across_blocks(world):
    _same_as_reference(world, SINGLE["d3"], [world["fq1"]], block="100")


@needs_ref
@pytest.mark.parametrize("fmt", ["cigar", "sam"])
def test_pairs_print_the_reference_programs_lines(world, fmt):
    _same_as_reference(world, ["-f", fmt, "-i", "600", "-r", "7"], [world["fq1"], world["fq2"]])


@needs_ref
@pytest.mark.parametrize("d,which", [("8", "fql"), ("-1", "fql_upto1700")])
def test_long_reads_print_the_reference_programs_lines(world, d, which):
    """reads of 257-3000 bases: k_align<true> and the strip traceback.  At -d -1 the reference program itself needs 6 s for the
    read of 3000 bases, so that run takes the reads of up to 1700 bases"""
    _same_as_reference(world, ["-f", "cigar", "-d", d, "-r", "-1"], [world[which]], block="8")


@pytest.fixture(scope="module")
def balanced(world):
    """a reference that holds the balanced 4000 bases, its index (k 13, s 6), and the two reads: an ordinary one, then the balanced one"""
    import numpy as np
    w = world
    name, read, target = cplx_data.balanced_read()
    rng = np.random.default_rng(5)
    flank = lambda: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=700)].tobytes()
    fa, pre = os.path.join(w["tmp"], "bal.fa"), os.path.join(w["tmp"], "bal")
    cplx_data.write_fasta(fa, w["seqs"] + [("chrB", flank() + target + flank())])
    subprocess.run([SMALT, "index", "-k", "13", "-s", "6", pre, fa], check=True, capture_output=True)
    ordinary = w["seqs"][0][1][1000:1120]
    fq, fq_ord = os.path.join(w["tmp"], "bal.fq"), os.path.join(w["tmp"], "ord.fq")
    open(fq, "wb").write(b"@ord\n" + ordinary + b"\n+\n" + b"I" * len(ordinary) + b"\n@" + name + b"\n" + read + b"\n+\n" + b"I" * len(read) + b"\n")
    open(fq_ord, "wb").write(b"@ord\n" + ordinary + b"\n+\n" + b"I" * len(ordinary) + b"\n")
    return dict(pre=pre, fq=fq, fq_ord=fq_ord, reads=[ordinary, read], name=name)


@needs_ref
def test_both_programs_stop_at_the_balanced_read(world, balanced):
    b = balanced
    out = os.path.join(world["tmp"], "bal.out")
    for cmd in ([SMALT, "map"], [PROG, "-B", "16"]):
        r = subprocess.run(cmd + ["-w", "-f", "cigar", "-r", "-1", "-o", out, b["pre"], b["fq"]], capture_output=True)
        assert r.returncode != 0, cmd
        assert SENTENCE in r.stderr and b["name"] in r.stderr, (cmd, r.stderr.decode()[-1000:])
        # without -w the same input runs clean
        r = subprocess.run(cmd + ["-f", "cigar", "-r", "-1", "-o", out, b["pre"], b["fq"]], capture_output=True)
        assert r.returncode == 0, (cmd, r.stderr.decode()[-1000:])


@needs_ref
def test_library_marks_the_balanced_read_and_completes_the_other(world, balanced):
    from smalt_amd import api
    b = balanced
    out = os.path.join(world["tmp"], "ord.out")
    subprocess.run([SMALT, "map", "-w", "-f", "cigar", "-r", "-1", "-o", out, b["pre"], b["fq_ord"]], check=True, capture_output=True)
    want = cplx_data.cigar_fields(_lines(out)[0])
    gix = api.Index.load(b["pre"], 0)
    mp = api.Mapper(gix, 16, 4096)
    par = gix.default_params()
    par.rmapflg |= api.FLG_CMPLXW
    with pytest.raises(Exception):
        mp.map_batch(b["reads"], [b"I" * len(r) for r in b["reads"]], par)
    res, stats = mp.map_batch(b["reads"], [b"I" * len(r) for r in b["reads"]], par, allow_read_errors=True)
    assert stats[1]["err"] == api.ECPLX and not res[1]
    assert stats[0]["err"] == 0 and res[0] and max(r["score"] for r in res[0]) == want[4]
    par.rmapflg &= ~api.FLG_CMPLXW
    res, stats = mp.map_batch(b["reads"], [b"I" * len(r) for r in b["reads"]], par)
    assert stats[1]["err"] == 0 and max(r["score"] for r in res[1]) == 4000
    mp.close()
    gix.close()


@needs_ref
def test_library_flag(world):
    """flag off: what the CPU oracle gives, as smoke() compares; flag on: the best score of every read is the best score among the
    read's lines of `smalt map -w -d -1` (scores below the report's floor of 18 are not printed)"""
    import oracle_lib as ol
    from smalt_amd import api
    w = world
    reads = [p[0] for p in w["pairs"]]
    quals = [b"I" * len(r) for r in reads]
    gix = api.Index.load(w["pre"], 0)
    mp = api.Mapper(gix, 512, 160)
    par = gix.default_params()
    assert not par.rmapflg & api.FLG_CMPLXW
    res, _ = mp.map_batch(reads, quals, par)
    oix = ol.lib().or_index_read(w["pre"].encode())
    om = ol.Mapper(oix)
    opar = ol.default_params(oix)
    for i, r in enumerate(reads):
        rv, ores = om.map(r, quals[i], opar)
        assert rv == 0 and res[i] == ores, "read %d differs from the oracle" % i
    om.close()
    # -d -1: no best-only mode, every alignment above the threshold
    par.rmapflg = (par.rmapflg & ~api.FLG_BEST) | api.FLG_CMPLXW
    par.min_swatscor_below_max = -1
    res_w, stats = mp.map_batch(reads, quals, par)
    best = {}
    for ln in _map(w, "ref", ["-w"] + SINGLE["all"], [w["fq1"]]):
        f = cplx_data.cigar_fields(ln)
        if f:
            best[f[0]] = max(best.get(f[0], 0), f[4])
    assert len(best) > 300
    nlower = 0
    for i in range(len(reads)):
        got = max([r["score"] for r in res_w[i]], default=0)
        assert (got if got >= 18 else 0) == best.get(b"p%d/1" % i, 0), (i, got, best.get(b"p%d/1" % i))
        nlower += bool(res[i]) and got < max(r["score"] for r in res[i])
    assert nlower > 50
    mp.close()
    gix.close()

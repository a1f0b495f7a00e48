"""The candidate stage's paths behind the presorted stream (stage_cands_v2<false, true>: one chunk, several chunks, the fall back
to the HBM working set with its roll-back) in the one-lane host build (tests/hostemu), on the tandem workload of
tests/cands_ref.py: the stage dump against the oracle's, and the number of strands on the HBM working set against the plain
chunk walk of cands_ref over the pool that stage_hits left.  This pins the one-lane form and proves the walk on a machine without
a GPU; tests/test_gpu_cands.py holds the kernel against the same oracle and the same walk."""
import functools
import os
import re
import subprocess

import pytest

import cands_ref as cr
import oracle_lib as ol
from test_hits_ref import read_hits_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_HITS = 640                                            # CANDS_LDS_HITS: keys of the LDS working set


@pytest.fixture(scope="module")
def emu_bin():
    out = os.path.join(ROOT, "tests", "hostemu", "emu")
    tmp = "%s.%d.cands" % (out, os.getpid())        # other workers build the same file at the same time: never run a half-written one
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, os.path.join(ROOT, "tests", "hostemu", "emu_main.cpp")], check=True)
    os.replace(tmp, out)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_dump(k, s, xflag):
    """The oracle's stage dump with hit lists of the tandem workload, read after read."""
    seqs, reads = cr.tandem_workload()
    oix = ol.build_index(seqs, ["t%d" % i for i in range(len(seqs))], k, s)
    par = ol.default_params(oix)
    if xflag:
        par.flags |= ol.FLG_NOSHRTINFO | ol.FLG_SENSITIVE
    m = ol.Mapper(oix)
    out = []
    for i, r in enumerate(reads):
        rv, _ = m.map(r, b"I" * len(r), par)
        assert rv == 0
        out.append(m.dump(i, "r%d" % i, True))
    m.close()
    ol.lib().or_index_free(oix)
    return "".join(out)


@pytest.fixture(scope="module")
def tandem_files(oracle_built, tmp_path_factory):
    """(k, s) -> index prefix; the reads as a FASTQ file"""
    seqs, reads = cr.tandem_workload()
    assert len(seqs) == 3 and len(reads) == 54 + 20 and all(len(r) == 100 for r in reads)
    d = tmp_path_factory.mktemp("tandem")
    fq = str(d / "reads.fq")
    with open(fq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))
    pre = {}
    for k, s in ((13, 6), (11, 3)):
        oix = ol.build_index(seqs, ["t%d" % i for i in range(len(seqs))], k, s)
        pre[k, s] = str(d / ("ix%d_%d" % (k, s)))
        assert ol.lib().or_index_write(oix, pre[k, s].encode()) == 0
        ol.lib().or_index_free(oix)
    return pre, fq


def _same_text(got, want):
    a, b = got.split("\n"), want.split("\n")
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, "line %d" % (i + 1)
    assert len(a) == len(b)


@pytest.mark.parametrize("window", [0, 300], ids=["w640", "w300"])
@pytest.mark.parametrize("xflag", [False, True], ids=["plain", "x"])
@pytest.mark.parametrize("k,s", [(13, 6), (11, 3)], ids=["k13s6", "k11s3"])
def test_presorted_stream_paths_one_lane(k, s, xflag, window, emu_bin, tandem_files, tmp_path):
    """S3 ahead of the candidate stage (EMU_SPLIT=1), chunks of 640 (EMU_WINDOW unset) and 300 keys.  The dump equals the oracle's;
    the strands the stage took on the HBM working set are those the walk predicts to fall back plus those stage_hits left
    HITRUN_NONE (they are gathered and sorted there).  Conditions from the walk first: at least 20 fall backs with no region
    break in the first chunk, at least 20 strands in one chunk; at k=11 s=3 at least 5 fall backs after a completed chunk (the
    roll-back of the candidates of the chunks before)."""
    pre, fq = tandem_files
    _, reads = cr.tandem_workload()
    dump = str(tmp_path / "hits.bin")
    env = dict(os.environ, EMU_SPLIT="1", EMU_STATS="1", EMU_DUMP_HITS=dump)
    env.pop("EMU_WINDOW", None)
    if window:
        env["EMU_WINDOW"] = str(window)
    run = subprocess.run([emu_bin] + (["-x"] if xflag else []) + [pre[k, s], fq], check=True, capture_output=True, text=True, env=env)
    got = read_hits_dump(dump)
    W = min(LDS_HITS, window or LDS_HITS)
    walks = cr.walk_batch(got, W, k, s, [len(r) for r in reads])
    sm = cr.summary(walks)
    largest = max(int(got["run_n"][rs]) for rs, w in enumerate(walks) if w is not None and cr.is_fallback(w))
    print(k, s, xflag, W, sm, "largest fall-back run", largest)
    assert sm["no_break_first"] >= 20 and sm["one_chunk"] >= 20 and largest > 8192
    assert all(w.largest_region > W for w in walks if w is not None and cr.is_fallback(w) and w.path == cr.FALLBACK_NO_BREAK)
    if k == 11:
        assert sm["after_chunk"] >= 5
    assert "emu:" not in run.stderr, run.stderr
    m = re.search(r"HBM strands (\d+), strands sorted ahead (\d+)", run.stderr)
    assert m, run.stderr
    assert int(m.group(2)) == 2 * len(reads) - sm["none"]
    assert int(m.group(1)) == sm["fallbacks"] + sm["none"]
    _same_text(run.stdout, _oracle_dump(k, s, xflag))


@pytest.mark.parametrize("window", [0, 300], ids=["w640", "w300"])
@pytest.mark.parametrize("xflag", [False, True], ids=["plain", "x"])
@pytest.mark.parametrize("k,s", [(13, 6), (11, 3)], ids=["k13s6", "k11s3"])
def test_fused_form_one_lane(k, s, xflag, window, emu_bin, tandem_files):
    """The same runs with S3 inside the candidate stage (EMU_SPLIT=0: windows of ascending diagonal, and the HBM working set with
    its own sort for a region above the window): the dump equals the oracle's, and at least as many strands take the HBM
    working set as hold a region above the window."""
    pre, fq = tandem_files
    env = dict(os.environ, EMU_SPLIT="0", EMU_STATS="1")
    env.pop("EMU_WINDOW", None)
    if window:
        env["EMU_WINDOW"] = str(window)
    run = subprocess.run([emu_bin] + (["-x"] if xflag else []) + [pre[k, s], fq], check=True, capture_output=True, text=True, env=env)
    assert "emu:" not in run.stderr, run.stderr
    m = re.search(r"HBM strands (\d+)", run.stderr)
    assert m and int(m.group(1)) >= 20, run.stderr
    _same_text(run.stdout, _oracle_dump(k, s, xflag))

"""The raised window bound of stage_hits in the one-lane host build (tests/hostemu/hits_walk_check.cpp: the seeding stage and
stage_hits alone, with the window, the per-list tables, the fill target and the hit-list mode as arguments) on the inputs of
the GPU test (tests/hits_fill_cases.py): every strand equals the plain reference key by key, and the stage's count of windows and of raised bounds equals the restatement of the walk
(tests/hits_fill_ref.py) on every strand.  This proves the restatement and the cases on a machine without a GPU."""
import os
import subprocess
import types

import numpy as np
import pytest

import hits_fill_cases as fc
import hits_ref as hr
import oracle_lib as ol
from test_hits_ref import FLG_BEST, read_hits_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walk_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hitswalkbin") / "hits_walk_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", out, os.path.join(ROOT, "tests", "hostemu", "hits_walk_check.cpp")], check=True)
    return out


@pytest.fixture(scope="module")
def files(oracle_built, tmp_path_factory):
    """-> (index prefix, FASTQ of the inputs, read lengths, index arrays on the host)"""
    seqs, rb = fc.inputs()
    d = tmp_path_factory.mktemp("hitsfillemu")
    pre = str(d / "ix")
    oix0 = ol.build_index(seqs, ["c%d" % i for i in range(len(seqs))], fc.K, fc.S)
    assert ol.lib().or_index_write(oix0, pre.encode()) == 0
    ol.lib().or_index_free(oix0)
    oix = ol.lib().or_index_read(pre.encode())
    hx = hr.HostIndex(oix)
    ol.lib().or_index_free(oix)
    fq = str(d / "reads.fq")
    with open(fq, "w") as f:
        for i, r in enumerate(rb):
            f.write("@r%d\n%s\n+\n%s\n" % (i, r.decode(), "I" * len(r)))
    return pre, fq, [len(r) for r in rb], hx


@pytest.mark.parametrize("fill,window,concat", fc.CONFIGS, ids=fc.CONFIG_IDS)
def test_one_lane_raised_bound_equals_reference_and_restatement(files, walk_bin, tmp_path, fill, window, concat):
    pre, fq, lens, hx = files
    dump, wdump = str(tmp_path / "hits.bin"), str(tmp_path / "win.bin")
    subprocess.run([walk_bin, pre, fq, str(window), str(fc.TAB), str(fill), "1" if concat else "0", dump, wdump], check=True, capture_output=True)
    got = read_hits_dump(dump)
    win = np.fromfile(wdump, dtype=np.uint32)
    assert got["window"] == window and got["tab"] == fc.TAB and win.size == 2 * len(lens)
    par = types.SimpleNamespace(ktuple_maxhit=10000, min_cover=0, min_cover_frac=0.0, rmapflg=FLG_BEST | (0 if concat else hr.FLG_SEQBYSEQ))
    exp = hr.expect_batch(hx, par, lens, got)
    before, after = fc.check_windows(exp, window, hx, not concat, fill, win & 0xffff, win >> 16)
    print("fill %d W %d %s: windows of the strands of %d..%d keys %d -> %d" % (fill, window, "concat" if concat else "seqbyseq", fc.KEYS_MIN, fc.KEYS_MAX, before, after))
    assert sum(1 for rs, e in enumerate(exp) if e.eligible and not e.over_alloc and got["run_mode"][rs] == hr.HITRUN_NONE) == 0
    hr.check_batch(exp, got, not concat, got["qmask_seed"], lens)

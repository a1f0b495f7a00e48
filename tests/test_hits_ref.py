"""The plain reference of S3 (tests/hits_ref.py) against stage_hits compiled for the host with one lane (tests/hostemu,
EMU_SPLIT=1 EMU_DUMP_HITS=<file>), on committed fixtures: this proves the reference and the layout of the stand-alone entry on
a machine without a GPU, and pins the one-lane form.  The GPU tests (test_gpu_hits.py) hold the kernel against the same
reference."""
import os
import struct
import subprocess
import types

import numpy as np
import pytest

import golden_util as gu
import hits_ref as hr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLG_BEST, FLG_SEQBYSEQ, FLG_NOSHRTINFO, FLG_SENSITIVE = 0x02, 0x10, 0x20, 0x80


@pytest.fixture(scope="module")
def emu_bin():
    out = os.path.join(ROOT, "tests", "hostemu", "emu")
    tmp = "%s.%d.hits" % (out, os.getpid())         # other workers build the same file at the same time: never run a half-written one
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, os.path.join(ROOT, "tests", "hostemu", "emu_main.cpp")], check=True)
    os.replace(tmp, out)
    return out


def read_hits_dump(path):
    """The layout EMU_DUMP_HITS writes (tests/hostemu/emu_main.cpp) -> the dict Mapper.hits_batch returns."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"SMGHITS1"
    ns, stride, window, tab, hit_count, pool_cap = struct.unpack_from("<4I2Q", raw, 8)
    at = 8 + 16 + 16

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at).copy()
        at += a.nbytes
        return a
    n_seeds, seed_rank, status = take(np.uint32, ns), take(np.uint32, ns), take(np.uint32, ns)
    seeds = take(np.uint32, ns * stride * 3).reshape(ns, stride, 3)
    qmask = take(np.uint8, ns * stride).reshape(ns, stride)
    runs = take(np.dtype([("off", "<u8"), ("n", "<u4"), ("mode", "<u4")]), ns)
    pool = take(np.uint64, min(hit_count, pool_cap))
    qmask_seed = take(np.uint8, ns * stride).reshape(ns, stride)
    assert at == len(raw)
    return dict(qmask_seed=qmask_seed, n_seeds=n_seeds, seed_rank=seed_rank, status=status, seeds=seeds, qmask=qmask, run_off=runs["off"].copy(), run_n=runs["n"].copy(),
                run_mode=runs["mode"].copy(), hit_count=hit_count, pool_cap=pool_cap, pool=pool, window=window, tab=tab, stride=stride)


def _entry(pred):
    return next(e for e in gu.MANIFEST if pred(e))


TIES, XOPT = _entry(lambda e: e["tag"] == "g_k13s6_ties"), _entry(lambda e: "-x" in e["opts"].split())
# fixture, further options, keys per window, entries of the per-list tables (0: all 264), one hit list over all sequences,
# least number of strands: gathered in several windows, with seeds above the cut-off marked HQ_MULTIHIT (sequence by
# sequence), with seeds the cut-off leaves out (one list)
CASES = [(TIES, "", 400, 0, False, 1, 0, 0), (TIES, "", 256, 120, False, 20, 0, 0), (XOPT, "", 400, 0, False, 0, 0, 0), (XOPT, "", 256, 120, False, 0, 0, 0),
         (XOPT, "-H 1", 400, 0, False, 0, 20, 0), (XOPT, "-H 1", 256, 120, True, 0, 0, 20), (TIES, "-x -H 4", 256, 120, False, 0, 20, 0),
         (TIES, "-x -H 4", 400, 0, True, 0, 0, 20), (TIES, "", 256, 120, True, 20, 0, 0)]


@pytest.mark.parametrize("entry,more,window,tab,concat,min_windowed,min_multihit,min_cut", CASES,
                         ids=["%s%s-w%d%s" % (c[0]["tag"], c[1].replace(" ", ""), c[2], "-concat" if c[4] else "") for c in CASES])
def test_one_lane_stage_hits_equals_plain_reference(entry, more, window, tab, concat, min_windowed, min_multihit, min_cut, emu_bin, oracle_built, tmp_path):
    """window 400 with the full per-list tables (264 entries), window 256 with tables of 120 entries (a mapper of 100-base reads:
    with the full tables a window of 256 keys switches the stage off; strands with 120 seeds and more stay with the candidate
    stage).  The reads of g_k13s6_ties lie in repeats: strands of up to 480 keys, gathered in several windows.  With -x the
    seeding stage keeps the seeds above the cut-off (-H) in the table and the stage leaves them out itself: sequence by sequence
    it marks their read offsets HQ_MULTIHIT, with one hit list over all sequences (EMU_CONCAT=1) it goes through
    hashCollectHitsUsingCutoff's loop.  Every strand: mode, run length, keys, pool cursor, the whole row of qualifiers -- and no
    eligible strand left to the candidate stage."""
    fx = gu.unpack(entry, tmp_path)
    dump = str(tmp_path / "hits.bin")
    env = dict(os.environ, EMU_SPLIT="1", EMU_HITS_WINDOW=str(window), EMU_DUMP_HITS=dump, EMU_CONCAT="1" if concat else "0")
    if tab:
        env["EMU_HITS_TAB"] = str(tab)
    opts = entry["opts"].split() + more.split()
    subprocess.run([emu_bin] + opts + [fx["prefix"], fx["fq"]], check=True, capture_output=True, env=env)
    got = read_hits_dump(dump)
    assert got["window"] == window and got["tab"] == (tab or 264)
    oix = ol.lib().or_index_read(fx["prefix"].encode())
    hx = hr.HostIndex(oix)
    ol.lib().or_index_free(oix)
    xflag = "-x" in opts
    seqbyseq = hx.nseq < 512 and not concat
    par = types.SimpleNamespace(ktuple_maxhit=int(opts[opts.index("-H") + 1]) if "-H" in opts else 10000, min_cover=0, min_cover_frac=0.0,
                                rmapflg=(FLG_BEST if "-d" not in opts else 0) | (FLG_SEQBYSEQ if seqbyseq else 0) | ((FLG_NOSHRTINFO | FLG_SENSITIVE) if xflag else 0))
    lens = [len(s) for _, s, _ in gu.read_fastq(fx["fq"])]
    assert got["n_seeds"].size == 2 * len(lens)
    exp = hr.expect_batch(hx, par, lens, got)
    nsorted = sum(1 for e in exp if e.mode == hr.HITRUN_SORTED and e.keys.size)
    nwindowed = sum(1 for e in exp if e.mode == hr.HITRUN_SORTED and e.keys.size > window)
    nmulti = sum(1 for e in exp if e.mode == hr.HITRUN_SORTED and e.multihit)
    ncut = sum(1 for e in exp if e.mode == hr.HITRUN_SORTED and e.ncutseeds)
    print("strands %d, sorted with keys %d, of them in several windows %d, eligible %d, marking offsets %d, leaving seeds out %d, halved %d, at the ceiling %d"
          % (len(exp), nsorted, nwindowed, sum(e.eligible for e in exp), nmulti, ncut, sum(e.halved for e in exp), sum(e.stopped for e in exp)))
    assert nsorted >= 20 and nwindowed >= min_windowed
    assert nmulti >= min_multihit and (seqbyseq or nmulti == 0) and ncut >= min_cut
    assert sum(1 for rs, e in enumerate(exp) if e.eligible and not e.over_alloc and got["run_mode"][rs] == hr.HITRUN_NONE) == 0
    hr.check_batch(exp, got, seqbyseq, got["qmask_seed"], lens)

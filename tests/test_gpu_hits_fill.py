"""The raised window bound of k_hits (stage_hits, smalt_amd/csrc/smg_cands.hpp) through smaltgpu_hits_batch at windows of 256 and
300 keys: a window that its safe bound leaves under-filled gets a second bound and an exact second count.  Inputs and the events
each configuration must reach come from tests/hits_fill_cases.py (asserted from the restatement of the walk before anything is
compared); every strand is then held to tests/hits_ref.py key by key -- mode, run length, keys, disjoint runs, the pool cursor,
no eligible strand left to the candidate stage -- and the kernel's own count of windows and raised bounds
(smaltgpu_hits_windows) to the restatement's.  Second part: k_hits runs ahead of a mapping call only where the candidate stage
consumes its runs (strides up to 255 read offsets)."""
import os

import numpy as np
import pytest

import hits_fill_cases as fc
import hits_ref as hr
import oracle_lib as ol

pytestmark = pytest.mark.gpu


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle_built, tmp_path_factory):
    """Index of the workload's reference at k=13 s=6, its arrays on the host, and two mappers of 100-base reads (per-list tables
    of 120 entries): the fill target at 3/4 of a window's room, and at the whole room (the default)."""
    from smalt_amd import api
    c = Ctx()
    c.seqs, c.rb = fc.inputs()
    oix0 = ol.build_index(c.seqs, ["c%d" % i for i in range(len(c.seqs))], fc.K, fc.S)
    pre = str(tmp_path_factory.mktemp("hitsfill") / "ix")
    assert ol.lib().or_index_write(oix0, pre.encode()) == 0
    ol.lib().or_index_free(oix0)
    c.oix = ol.lib().or_index_read(pre.encode())
    c.hx = hr.HostIndex(c.oix)
    c.gix = api.Index.load(pre, 0)
    c.mp = {}
    for fill in sorted(set(f for f, _ in fc.REQUIRED)):
        c.mp[fill] = _mapper_with_fill(c.gix, fill)
    c.mp_off = api.Mapper(c.gix, 256, 150)                  # tables of 168 entries: a window of 256 keys switches S3 off
    c.exp = {}
    yield c
    for m in list(c.mp.values()) + [c.mp_off]:
        m.close()
    c.gix.close()


def _mapper_with_fill(gix, fill):
    """A mapper of 100-base reads whose k_hits takes the fill target from SMALTGPU_HITS_FILL (read when the mapper is made)"""
    from smalt_amd import api
    old = os.environ.get("SMALTGPU_HITS_FILL")
    os.environ["SMALTGPU_HITS_FILL"] = str(fill)
    try:
        return api.Mapper(gix, 256, 100)
    finally:
        if old is None:
            os.environ.pop("SMALTGPU_HITS_FILL", None)
        else:
            os.environ["SMALTGPU_HITS_FILL"] = old


def _par(c, concat):
    p = c.gix.default_params()
    assert p.rmapflg & hr.FLG_SEQBYSEQ
    if concat:
        p.rmapflg &= ~hr.FLG_SEQBYSEQ
    return p


@pytest.mark.parametrize("fill,window,concat", fc.CONFIGS, ids=fc.CONFIG_IDS)
def test_raised_bound_runs_equal_reference(ctx, fill, window, concat):
    par = _par(ctx, concat)
    quals = [b"I" * len(r) for r in ctx.rb]
    lens = [len(r) for r in ctx.rb]
    got = ctx.mp[fill].hits_batch(ctx.rb, quals, par, window=window)
    win = ctx.mp[fill].hits_windows(2 * len(ctx.rb))
    assert got["window"] == window and got["tab"] == fc.TAB and window > got["tab"] + 128
    if concat not in ctx.exp:                               # (the reference: once per hit-list mode, not changed afterwards)
        ctx.exp[concat] = hr.expect_batch(ctx.hx, par, lens, got, window=1024)
    exp = ctx.exp[concat]
    before, after = fc.check_windows(exp, window, ctx.hx, not concat, fill, win["windows"], win["raised"])
    multi = [rs for rs, e in enumerate(exp) if e.mode == hr.HITRUN_SORTED and e.keys.size > window]
    print("fill %d W %d %s: windows of the strands of %d..%d keys %d -> %d; all strands above one window: %d strands, %d windows, %.1f keys per window"
          % (fill, window, "concat" if concat else "seqbyseq", fc.KEYS_MIN, fc.KEYS_MAX, before, after, win["strands"], win["nwindows"], win["keys"] / max(1, win["nwindows"])))
    assert win["strands"] == len(multi) and win["nwindows"] == int(win["windows"].sum()) and win["keys"] == sum(exp[rs].keys.size for rs in multi)
    assert win["reserved"] == got["hit_count"]
    left = [rs for rs, e in enumerate(exp) if e.eligible and not e.over_alloc and int(got["run_mode"][rs]) == hr.HITRUN_NONE]
    assert left == [], "eligible strands the kernel left to the candidate stage: %r" % left[:10]
    off = ctx.mp_off.hits_batch(ctx.rb, quals, par, window=256)
    assert off["window"] <= off["tab"] + 128 and (off["run_mode"] == hr.HITRUN_NONE).all() and off["hit_count"] == 0
    assert ctx.mp_off.hits_windows(2 * len(ctx.rb))["nwindows"] == 0
    hr.check_batch(exp, got, not concat, off["qmask"], lens)


def test_no_raised_bound_with_the_target_at_zero(ctx):
    """SMALTGPU_HITS_FILL=0: the safe bounds alone -- the windows of hits_ref.window_counts, the same runs."""
    mp = _mapper_with_fill(ctx.gix, 0)
    try:
        par = _par(ctx, False)
        quals = [b"I" * len(r) for r in ctx.rb]
        got = mp.hits_batch(ctx.rb, quals, par, window=300)
        win = mp.hits_windows(2 * len(ctx.rb))
        exp = hr.expect_batch(ctx.hx, par, [len(r) for r in ctx.rb], got)
        assert (win["raised"] == 0).all()
        for rs, e in enumerate(exp):
            assert int(win["windows"][rs]) == (len(hr.window_counts(e, 300)) if e.mode == hr.HITRUN_SORTED and e.keys.size > 300 else 0), rs
        hr.check_batch(exp, got, True, None, [len(r) for r in ctx.rb])
    finally:
        mp.close()


@pytest.mark.parametrize("maxlen", [240, 241, 245, 248])
def test_hits_run_ahead_only_where_the_candidate_stage_consumes_them(ctx, maxlen):
    """max_read_len 241..248 gives a stride of 256 read offsets: the candidate kernel's general instance gathers the hits itself,
    so a mapping call launches no k_hits -- nothing is reserved in the pool (smaltgpu_hits_windows: the call's pool cursor and
    windows are 0), and the results equal the oracle's.  At 240 (stride 248) the runs are consumed: the cursor counts keys."""
    from smalt_amd import api
    n = min(maxlen, 245)
    src = ctx.seqs[1]
    rb = [src[5000:5000 + n], src[90000:90000 + n], ctx.rb[0] + ctx.rb[2] + ctx.rb[4][:n - 200], ctx.rb[1] + ctx.rb[3] + ctx.rb[5][:n - 200], src[200000:200000 + n]]
    assert all(len(r) == n for r in rb)
    par = ctx.gix.default_params()
    mp = api.Mapper(ctx.gix, 8, maxlen)
    try:
        res, _ = mp.map_batch(rb, [b"I" * n for _ in rb], par)
        win = mp.hits_windows(2 * len(rb))
        if maxlen <= 240:
            assert win["reserved"] > 1024 and win["nwindows"] > 0
        else:
            assert win["reserved"] == 0 and win["nwindows"] == 0 and win["strands"] == 0 and (win["windows"] == 0).all()
        om = ol.Mapper(ctx.oix)
        opar = ol.default_params(ctx.oix)
        nres = 0
        for i, r in enumerate(rb):
            rv, ores = om.map(r, b"I" * n, opar)
            assert rv == 0 and res[i] == ores, i
            nres += len(ores)
        om.close()
        assert nres >= len(rb)
    finally:
        mp.close()

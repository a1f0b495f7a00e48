"""The candidate stage k_cands (S4-S7) on inputs chosen for its working sets: the presorted stream in one chunk, in several chunks
and its fall back to the HBM working set (with the roll-back of the chunks before), the fused instance with its own sort over
global memory, the deferred second pass and the instance for long reads -- against the CPU oracle, exactly.  Every case first
asserts, from references alone (tests/hits_ref.py for the pool, tests/cands_ref.py for the walk over it), that the batch holds
the strands the case is about; then the stage dump of a debug batch equals the oracle's line by line, the results and per-read
scalars of a plain batch equal the oracle's (debug batches switch off the early prune and the second pass, so both are needed),
and the stage's own counters say that the paths were taken: work[22] counts the strands on the HBM working set, work[20] the
keys streamed from the pool."""
import functools

import pytest

import cands_ref as cr
import hits_ref as hr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

LDS_HITS = 640
STAGE_TAGS = ("HL ", "CA ", "ST ", "SI ", "RC ")
WK_STREAMED, WK_HBM_STRANDS = 20, 22                     # WK_PHASE0 + 12, + 14 (smg_stages.hpp; bench.py: hbm_fallback_strands)
SCALARS = ("swmax", "sw2nd", "nseg", "nseg_tot", "nhit", "nhit_tot")


def _stage_lines(text):
    return [ln for ln in text.split("\n") if ln[:3] in STAGE_TAGS]


class Ctx:
    pass


@pytest.fixture(scope="module", params=[(13, 6), (11, 3)], ids=["k13s6", "k11s3"])
def ctx(request, oracle_built, tmp_path_factory):
    """The tandem reference under one (k, s): the index written by the oracle and loaded by the library."""
    from smalt_amd import api
    c = Ctx()
    c.k, c.s = request.param
    c.seqs, c.reads = cr.tandem_workload()
    c.pre = _index(tmp_path_factory.mktemp("cands"), c.seqs, c.k, c.s)
    c.oix = ol.lib().or_index_read(c.pre.encode())
    c.hx = hr.HostIndex(c.oix)
    c.gix = api.Index.load(c.pre, 0)
    c.oracle = functools.lru_cache(maxsize=None)(lambda xflag: _oracle(c.oix, c.reads, xflag))
    yield c
    c.gix.close()


def _index(d, seqs, k, s):
    oix0 = ol.build_index(seqs, ["t%d" % i for i in range(len(seqs))], k, s)
    pre = str(d / ("ix%d_%d" % (k, s)))
    assert ol.lib().or_index_write(oix0, pre.encode()) == 0
    ol.lib().or_index_free(oix0)
    return pre


def _oracle(oix, reads, xflag):
    """-> per read (results, scalars, stage lines of the dump with hit lists)"""
    par = ol.default_params(oix)
    if xflag:
        par.flags |= ol.FLG_NOSHRTINFO | ol.FLG_SENSITIVE
    m = ol.Mapper(oix)
    out = []
    for i, r in enumerate(reads):
        rv, res = m.map(r, b"I" * len(r), par)
        assert rv == 0
        st = m.stats()
        out.append((res, dict(zip(SCALARS, st[:6])), _stage_lines(m.dump(i, "r%d" % i, True))))
    m.close()
    return out


def _params(gix, xflag):
    from smalt_amd import api
    p = gix.default_params()
    assert p.rmapflg & hr.FLG_SEQBYSEQ
    if xflag:
        p.rmapflg |= api.FLG_NOSHRTINFO | api.FLG_SENSITIVE
    return p


def _pool(mp, hx, par, reads):
    """S3 alone on the reads (the pool and the runs the candidate stage will stream), held against the plain reference."""
    lens = [len(r) for r in reads]
    got = mp.hits_batch(reads, [b"I" * n for n in lens], par)
    exp = hr.expect_batch(hx, par, lens, got)
    hr.check_batch(exp, got, True, None, lens)
    return got


def _map_and_compare(mp, reads, par, exp, debug):
    """One batch; debug: the stage lines of every read against the oracle's, else results and scalars.  -> the work counters"""
    quals = [b"I" * len(r) for r in reads]
    mp.set_debug(2 if debug else 0)
    res, stats = mp.map_batch(reads, quals, par)
    _, work = mp.timers()
    assert all(s["err"] == 0 for s in stats)
    for i in range(len(reads)):
        if debug:
            got = _stage_lines(mp.dump_read(i, "r%d" % i))
            for j, (x, y) in enumerate(zip(got, exp[i][2])):
                assert x == y, "read %d, stage line %d" % (i, j)
            assert len(got) == len(exp[i][2]), i
        else:
            assert res[i] == exp[i][0], i
            for kk in SCALARS:
                assert stats[i][kk] == exp[i][1][kk], (i, kk)
    return work


def _check_counters(work, got, nfallback, nnone):
    assert nfallback <= work[WK_HBM_STRANDS] <= nfallback + nnone, (work[WK_HBM_STRANDS], nfallback, nnone)
    assert work[WK_STREAMED] == int(got["run_n"][got["run_mode"] == hr.HITRUN_SORTED].sum())


def _set_env(monkeypatch, window, **more):
    monkeypatch.setenv("SMALTGPU_CANDS_LDS_HITS", str(LDS_HITS))
    if window:
        monkeypatch.setenv("SMALTGPU_CANDS_WINDOW", str(window))
    else:
        monkeypatch.delenv("SMALTGPU_CANDS_WINDOW", raising=False)
    for name, value in more.items():
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("window", [0, 300], ids=["w640", "w300"])
@pytest.mark.parametrize("xflag", [False, True], ids=["plain", "x"])
def test_tandem_reads_fall_back_to_the_hbm_working_set(ctx, xflag, window, monkeypatch):
    """Split instance, chunks of 640 and 300 keys.  From the walk: at least 20 strands fall back with no region break in their
    first chunk, at least 20 strands stream in one chunk, the largest run that falls back holds more than 8192 keys (one region
    on one lane of S5), and at k=11 s=3 at least 5 strands fall back after a completed chunk, whose candidates are rolled back.
    (Predicted by the walk for this workload: 36-57 fall backs, 9-14 of them after a completed chunk -- the carried tail of a
    region left fewer than 64 free keys --, 37-85 one-chunk strands, largest run 12 546 / 16 268 keys.)"""
    from smalt_amd import api
    _set_env(monkeypatch, window)
    W = min(LDS_HITS, window or LDS_HITS)
    par = _params(ctx.gix, xflag)
    mp = api.Mapper(ctx.gix, 2048, 100)                      # (pools for 2048 average reads: the tandem reads rank thousands of candidates)
    try:
        got = _pool(mp, ctx.hx, par, ctx.reads)
        walks = cr.walk_batch(got, W, ctx.k, ctx.s, [len(r) for r in ctx.reads])
        sm = cr.summary(walks)
        largest = max(int(got["run_n"][rs]) for rs, w in enumerate(walks) if w is not None and cr.is_fallback(w))
        print(ctx.k, ctx.s, xflag, W, sm, "largest run that falls back:", largest)
        assert sm["no_break_first"] >= 20 and sm["one_chunk"] >= 20 and largest > 8192
        if ctx.k == 11:
            assert sm["after_chunk"] >= 5
        exp = ctx.oracle(xflag)
        for debug in (True, False):
            work = _map_and_compare(mp, ctx.reads, par, exp, debug)
            print("debug" if debug else "plain", "work[20] =", work[WK_STREAMED], "work[22] =", work[WK_HBM_STRANDS])
            _check_counters(work, got, sm["fallbacks"], sm["none"])
    finally:
        mp.close()


@pytest.mark.parametrize("window", [0, 300], ids=["w640", "w300"])
def test_tandem_reads_fused_instance(ctx, window, monkeypatch):
    """SMALTGPU_HITS_SPLIT=0: S3 inside k_cands (windows of ascending diagonal); a strand with a region above the window is redone
    on the HBM working set, gathered there and sorted by the sort in chunks of 1024 keys -- on real runs of up to 16 thousand
    keys.  At least as many strands take the HBM working set as hold a region above the window (at least 20)."""
    from smalt_amd import api
    par = _params(ctx.gix, False)
    _set_env(monkeypatch, window)
    W = min(LDS_HITS, window or LDS_HITS)
    mp = api.Mapper(ctx.gix, 2048, 100)
    try:
        got = _pool(mp, ctx.hx, par, ctx.reads)
    finally:
        mp.close()
    walks = cr.walk_batch(got, W, ctx.k, ctx.s, [len(r) for r in ctx.reads])
    nabove = sum(1 for w in walks if w is not None and w.largest_region > W)
    assert nabove >= 20 and max(int(n) for n in got["run_n"]) > 8192
    _set_env(monkeypatch, window, SMALTGPU_HITS_SPLIT="0")
    mp = api.Mapper(ctx.gix, 2048, 100)
    try:
        with pytest.raises(api.SmaltGpuError):              # the mapper really keeps S3 inside k_cands
            mp.hits_batch(ctx.reads[:1], None, par)
        exp = ctx.oracle(False)
        for debug in (True, False):
            work = _map_and_compare(mp, ctx.reads, par, exp, debug)
            print("debug" if debug else "plain", "work[22] =", work[WK_HBM_STRANDS], "regions above the window:", nabove)
            assert work[WK_HBM_STRANDS] >= nabove
    finally:
        mp.close()


def test_tandem_reads_deferred_to_the_second_pass(ctx, monkeypatch):
    """SMALTGPU_CANDS_HCAP=1024: first-pass slots of 1024 hits per strand.  A strand that falls back with more keys overflows its
    slot, and the read is deferred to the second pass over the full-size slots: at least 20 such strands by the walk."""
    from smalt_amd import api
    _set_env(monkeypatch, 0, SMALTGPU_CANDS_HCAP="1024")
    par = _params(ctx.gix, False)
    mp = api.Mapper(ctx.gix, 2048, 100)
    try:
        got = _pool(mp, ctx.hx, par, ctx.reads)
        walks = cr.walk_batch(got, LDS_HITS, ctx.k, ctx.s, [len(r) for r in ctx.reads])
        ndeferred = sum(1 for rs, w in enumerate(walks) if w is not None and cr.is_fallback(w) and int(got["run_n"][rs]) > 1024)
        assert ndeferred >= 20
        _map_and_compare(mp, ctx.reads, par, ctx.oracle(False), False)
    finally:
        mp.close()


@pytest.fixture(scope="module")
def stream(ctx, tmp_path_factory):
    """At most 64 reads of the test_gpu_hits workload under ctx's (k, s), chosen by the walk over the pool of the whole workload:
    no strand of theirs falls back at chunks of 300 or of 128 keys, and as many as possible stream in several chunks at both.
    With them the index and the oracle's answers."""
    from smalt_amd import api
    from test_gpu_hits import workload
    seqs, rb = workload()
    c = Ctx()
    c.pre = _index(tmp_path_factory.mktemp("stream"), seqs, ctx.k, ctx.s)
    c.oix = ol.lib().or_index_read(c.pre.encode())
    c.hx = hr.HostIndex(c.oix)
    c.gix = api.Index.load(c.pre, 0)
    mp = api.Mapper(c.gix, 600, 100)                        # (a pool of 6144 keys per read: 600 reads' hold the 2.5 million keys at k=11 s=3)
    try:
        got = _pool(mp, c.hx, _params(c.gix, False), rb)
    finally:
        mp.close()
    lens = [len(r) for r in rb]
    w300, w128 = cr.walk_batch(got, 300, ctx.k, ctx.s, lens), cr.walk_batch(got, 128, ctx.k, ctx.s, lens)
    score = []
    for i in range(len(rb)):
        ws = [w300[2 * i], w300[2 * i + 1], w128[2 * i], w128[2 * i + 1]]
        if any(w is None or cr.is_fallback(w) for w in ws):
            continue
        n = min(sum(1 for w in ws[:2] if w.path == cr.CHUNKS), sum(1 for w in ws[2:] if w.path == cr.CHUNKS))
        if n:
            score.append((-n, i))
    c.reads = [rb[i] for i in sorted(i for _, i in sorted(score)[:64])]
    c.exp = _oracle(c.oix, c.reads, False)
    yield c
    c.gix.close()


@pytest.mark.parametrize("window", [300, 128], ids=["w300", "w128"])
def test_streaming_in_several_chunks_without_fallback(ctx, stream, window, monkeypatch):
    """The repeat family of the test_gpu_hits workload (300-base copies, regions of a few hundred keys): at least 50 strands stream
    in several chunks with the unfinished region carried over, none falls back and none was left to the candidate stage, so
    work[22] is 0."""
    from smalt_amd import api
    reads = stream.reads
    assert 0 < len(reads) <= 64
    _set_env(monkeypatch, window)
    mp = api.Mapper(stream.gix, 2048, 100)
    try:
        par = _params(stream.gix, False)
        got = _pool(mp, stream.hx, par, reads)
        sm = cr.summary(cr.walk_batch(got, window, ctx.k, ctx.s, [len(r) for r in reads]))
        print(ctx.k, ctx.s, window, len(reads), sm)
        assert sm["chunks"] >= 50 and sm["fallbacks"] == 0 and sm["none"] == 0 and sm["max_carry"] > 0
        for debug in (True, False):
            work = _map_and_compare(mp, reads, par, stream.exp, debug)
            assert work[WK_HBM_STRANDS] == 0
            _check_counters(work, got, 0, 0)
    finally:
        mp.close()


def test_long_reads_with_regions_of_several_segments(oracle_built, tmp_path):
    """The instance for reads of 256 bases and more: 400-base reads cut from the tandem stretches of 600 bases and more, k=11 s=3.
    Their regions hold several segments (substitutions, and the unit's period against the sampling step), so the coverage masks
    in memory are worked by the whole wave: at least 20 candidates of 3 and more segments by the oracle's CA lines."""
    from smalt_amd import api
    seqs, reads = cr.tandem_workload(read_len=400, min_stretch=600)
    assert len(reads) == 45 + 20 and all(len(r) == 400 for r in reads)
    pre = _index(tmp_path, seqs, 11, 3)
    oix = ol.lib().or_index_read(pre.encode())
    exp = _oracle(oix, reads, False)
    nseg = [int(ln.split()[11]) for e in exp for ln in e[2] if ln.startswith("CA ")]
    print("candidates", len(nseg), "of 3 and more segments", sum(1 for n in nseg if n >= 3), "most segments", max(nseg))
    assert sum(1 for n in nseg if n >= 3) >= 20
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, len(reads), 400)
    try:
        par = _params(gix, False)
        for debug in (True, False):
            _map_and_compare(mp, reads, par, exp, debug)
    finally:
        mp.close()
        gix.close()

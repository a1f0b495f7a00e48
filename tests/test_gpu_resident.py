"""The device-resident entry points, which bench.py times and no other test calls: smaltgpu_map_batch_device with
smaltgpu_fetch_results / _fetch_begin / _fetch_end (single reads, part A) and smaltgpu_map_batch_ctx_resident,
smaltgpu_hit_totals_resident and smaltgpu_map_pairs_resident (pairs, part B).

Part A is compared read by read with the CPU oracle (alignments and the six scalars swmax, sw2nd, nseg, nseg_tot, nhit,
nhit_tot) on the workloads of tests/resident_data.py; part B with the committed pair fixtures: the dumps of the reference's
rmapPair (manifest_pairs.json) and the output of the reference program (manifest_pair_reports.json).  Device buffers are torch
tensors.  No test breaks the rules smaltgpu_map_batch_device leaves to its caller (offsets from 0, reads within max_read_len,
total_bases = the last offset): the kernels would run out of bounds.  The tests without the gpu mark check on the oracle and on
the fixtures that the workloads have the properties the GPU tests rely on."""
import ctypes as C
import gzip
import json
import os
import threading

import numpy as np
import pytest

import golden_util as gu
import pair_replay as pr
import resident_data as rd

gpu = pytest.mark.gpu
PAIRS = {e["tag"]: e for e in json.load(open(os.path.join(gu.GOLD, "manifest_pairs.json")))}
REPORTS = json.load(open(os.path.join(gu.GOLD, "manifest_pair_reports.json")))
EARG, ECAP = -3, -5
SCALARS = ("swmax", "sw2nd", "nseg", "nseg_tot", "nhit", "nhit_tot")
# Work counters (smg_stages.hpp, WK_*) that are sums of per-read quantities and so do not depend on how the workgroups were
# scheduled: index lookups, k-mer hits, candidates made and kept, ranked candidates of reads with non-ACGT letters, of windows
# above the short kernel's, and beyond the register tiling.  (The others are clock ticks, or cells and tasks of kernels that
# pack tasks as they come.)
WORK_STABLE = {"lookups": 0, "hits": 1, "ncand": 5, "nkept": 6, "qn_tasks": 7, "long_tasks": 17, "strip_tasks": 18}


# ---------------------------------------------------------------- the workloads' conditions (CPU) ----------------------------------------------------------------

def test_single_read_workload_has_the_properties_the_gpu_tests_rely_on(oracle_built):
    w = rd.single()
    reads, quals, kinds, exp = w["reads"], w["quals"], w["kinds"], w["exp"]
    assert len(reads) == rd.NREADS == 600
    lens = [len(r) for r in reads]
    assert min(lens) >= 8 and max(lens) <= 250 + 13 and sum(1 for n in lens if n < rd.K) >= 5      # (insertions lengthen a read of 250 a little)
    assert sum(1 for n in lens if n > 200) >= 50
    assert 200 < sum(1 for _, rev in kinds if rev) < 400                                           # both strands
    assert sum(1 for m, _ in kinds if m == 5) == 75 and sum(1 for m, _ in kinds if m in (6, 7)) == 150      # unrelated reads, indels
    assert 60 <= sum(1 for r in reads if b"N" in r) <= 75                                          # one in eight, where the read is long enough
    nq = sum(len(q) for q in quals)
    assert 0.07 * nq < sum(1 for q in quals for c in q if c - 33 < 10) < 0.09 * nq
    for name, e in exp.items():
        assert all(x[0] == 0 for x in e), name                                                     # the reference maps every read without an error
        assert sum(1 for x in e if x[1]) >= 300, name
    assert sum(1 for x in exp["default"] if len(x[1]) > 1) >= 20                                   # reads with several alignments
    # the parameter sets tell: qualities change the seeding, the second set of the pipeline test changes the alignments
    assert sum(1 for a, b in zip(exp["default"], exp["basq10"]) if a[2]["nhit_tot"] != b[2]["nhit_tot"]) >= 100
    assert sum(1 for a, b in zip(exp["default"], exp["all40"]) if a[1] != b[1]) >= 50
    cuts = rd.sub_batches()
    assert [b - a for a, b in cuts] == [97, 260, 1, 200, 42] and cuts[-1][1] == len(reads)
    for j in range(1, len(cuts)):                                                                  # a leak between neighbours would show
        assert rd.batch_parset(j) != rd.batch_parset(j - 1)
    assert len(exp["default"][cuts[2][0]][1]) >= 1                                                 # the batch of one read maps


def test_overflow_workload_exceeds_the_pool(oracle_built):
    o = rd.overflow()
    n = len(o["reads"])
    nseg = [e[2]["nseg"] for e in o["exp"]]
    assert n == 300 and all(e[0] == 0 for e in o["exp"])
    assert sum(nseg) > rd.pool_capacity(n) >= 8 * n                  # ranked candidates of the batch vs the room of a mapper with cands_per_read = 8
    assert len(o["plain"]) >= 50 and sum(nseg[i] for i in o["plain"]) < rd.pool_capacity(n) // 2
    assert sum(1 for i in o["plain"] if o["exp"][i][1]) >= 50


def _fixture_calls(tag):
    with gzip.open(os.path.join(gu.GOLD, tag + ".refdump.txt.gz"), "rt") as g:
        pairs = pr.parse(g.read())
    calls = [(P, c) for P in pairs for c in P["calls"]]
    return pairs, _rounds(calls)


def _rounds(calls):
    return {"plain": [pc for pc in calls if pc[1]["niv"] < 0], "restricted": [pc for pc in calls if pc[1]["niv"] >= 0 and not pc[1]["fine"]],
            "fine": [pc for pc in calls if pc[1]["fine"]]}


def _copies_to_overflow(lst):
    """how often a round is sent in one batch so that its ranked candidates (the reference's nseg, RX) exceed the pool of a
    mapper with cands_per_read = 8 sized for that batch"""
    nseg = sum(c["rx"][3] for _, c in lst)
    for r in range(1, 40):
        if nseg * r > rd.pool_capacity(len(lst) * r):
            return r
    return None


def test_restricted_rounds_of_the_fixtures_overflow_only_in_copies():
    """Observed on the dumps: one copy of the restricted round of gp_k13s6_ties ranks 1542 candidates and of its fine round 1199
    (gp_k13s6_pe: 133 and 71), all below the pool's floor of 8000, so neither fixture overflows such a round at any
    cands_per_read.  Sent 6 and 7 times over in one batch they do, and some calls still rank fewer than 8."""
    _, rounds = _fixture_calls("gp_k13s6_ties")
    assert {k: sum(c["rx"][3] for _, c in v) for k, v in rounds.items()} == {"plain": 4813, "restricted": 1542, "fine": 1199}
    assert {k: _copies_to_overflow(v) for k, v in rounds.items()} == {"plain": 2, "restricted": 6, "fine": 7}
    for v in rounds.values():
        assert any(c["rx"][3] < rd.POOL_PER_READ for _, c in v)
        assert len(v) * _copies_to_overflow(v) <= 2048


# ---------------------------------------------------------------- helpers (GPU) ----------------------------------------------------------------

def _dev():
    import torch
    return torch.device("cuda", 0)


class DevBatch:
    """reads (and qualities) in device buffers `pad` bytes behind an allocation's start, offsets from 0"""

    def __init__(self, reads, quals=None, pad=0):
        import torch
        self.n = len(reads)
        self.total = sum(len(r) for r in reads)
        self.keep = []
        self.d_bases = self._up(b"".join(reads), pad)
        self.d_quals = self._up(b"".join(quals), pad) if quals is not None else 0
        self.h_off = np.zeros(self.n + 1, dtype=np.uint64)
        self.h_off[1:] = np.cumsum([len(r) for r in reads])
        off = torch.from_numpy(self.h_off.astype(np.int64)).to(_dev())
        self.keep.append(off)
        self.d_off = off.data_ptr()
        torch.cuda.synchronize()                       # the copies ran on torch's stream, the mapper has its own

    def _up(self, data, pad):
        import torch
        t = torch.zeros(pad + len(data) + 16, dtype=torch.uint8, device=_dev())
        assert t.data_ptr() % 16 == 0
        if data:
            t[pad:pad + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(_dev())
        self.keep.append(t)
        return t.data_ptr() + pad

    def launch(self, mp, par):
        mp.map_batch_device(self.d_bases, self.d_quals, self.d_off, self.n, self.total, par)


def _check_reads(res, stats, exp, ids, what=""):
    """reads `ids` of a workload, in this order, against the oracle"""
    assert len(res) == len(stats) == len(ids), (what, len(res), len(ids))
    for t, i in enumerate(ids):
        rv, eres, est = exp[i]
        assert rv == 0 and stats[t]["err"] == 0, (what, t, i, stats[t]["err"], stats[t]["errsite"])
        assert res[t] == eres, (what, t, i)
        for kk in SCALARS:
            assert stats[t][kk] == est[kk], (what, t, i, kk, stats[t][kk], est[kk])


@pytest.fixture(autouse=True)
def _own_pool_size(monkeypatch):
    """SMALTGPU_CANDS_PER_READ overrides the cands_per_read a mapper is created with, and an earlier test module may have left
    it in the process's environment (tests/test_gpu_fullsize.py sets 768): the overflow tests below need their pool of 8"""
    monkeypatch.delenv("SMALTGPU_CANDS_PER_READ", raising=False)


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    """index of the single-read workload on the device and two mappers for its 600 reads"""
    import oracle_lib as ol
    from smalt_amd import api
    w = rd.single()
    pre = str(tmp_path_factory.mktemp("resident") / "single")
    assert ol.lib().or_index_write(w["oix0"], pre.encode()) == 0
    gix = api.Index.load(pre, 0)
    maxlen = max(len(r) for r in w["reads"])
    mappers = [api.Mapper(gix, rd.NREADS, maxlen, slot_budget_gb=4) for _ in range(2)]
    yield dict(w=w, gix=gix, mappers=mappers, maxlen=maxlen, api=api)
    for m in mappers:
        m.close()
    gix.close()


# ---------------------------------------------------------------- A. single reads ----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("parset", ["default", "basq10"])
@pytest.mark.parametrize("pad", [0, 1, 3, 8, 15])
def test_device_batch_at_any_alignment_matches_the_oracle(world, pad, parset):
    """A.1: d_bases (and d_quals) at every class of misalignment; without qualities under the default parameters, with
    qualities under min_basqval = 10"""
    w, mp, api = world["w"], world["mappers"][0], world["api"]
    over, with_q = rd.PARSETS[parset]
    b = DevBatch(w["reads"], w["quals"] if with_q else None, pad)
    assert b.d_bases % 16 == pad and (not with_q or b.d_quals % 16 == pad)
    b.launch(mp, rd.gpu_params(world["gix"], over))
    rc, out = mp.fetch_results_rc()
    assert rc == 0, api.lib().smaltgpu_last_error()
    assert out.nreads == rd.NREADS
    res, stats = mp.unpack(out)
    _check_reads(res, stats, w["exp"][parset], range(rd.NREADS), "pad %d" % pad)


def _schedule(mp, gix, batches, jobs, got, check_intact=True):
    """bench.py's order of calls over the sub-batches `jobs` = [(sub-batch, parameter set)] on one mapper, as a generator that
    stops behind every library call: launch(0); then begin(), launch(j), end() for every further job; begin(), end().
    got[sub-batch] = (return code of fetch_end, results, stats, work counters read between begin and the next launch)"""
    prev = None
    for j, ps in jobs + [(None, None)]:
        if prev is not None:
            mp.fetch_begin()
            work = mp.timers()[1]
            yield
        if j is not None:
            batches[j].launch(mp, rd.gpu_params(gix, rd.PARSETS[ps][0]))
            yield
        if prev is not None:
            rc, out = mp.fetch_end_rc()
            first = mp.unpack(out)
            nreads = out.nreads
            yield
            if j is not None and check_intact:
                mp.synchronize()                       # batch j has run to its end: the results handed out must not have moved
                yield
                assert mp.unpack(out) == first and out.nreads == nreads, "the BatchOut of sub-batch %d changed while the next batch ran" % prev
            got[prev] = (rc, nreads) + first + (work,)
        prev = j


def _run_interleaved(gens):
    gens = list(gens)
    while gens:
        for g in list(gens):
            try:
                next(g)
            except StopIteration:
                gens.remove(g)


def _sub_batches(w):
    return [DevBatch(w["reads"][a:b]) for a, b in rd.sub_batches()]


def _check_schedule(w, got, jobs, what):
    cuts = rd.sub_batches()
    for j, ps in jobs:
        rc, nreads, res, stats, _ = got[j]
        assert rc == 0 and nreads == cuts[j][1] - cuts[j][0], (what, j, rc, nreads)
        _check_reads(res, stats, w["exp"][ps], range(*cuts[j]), "%s, sub-batch %d under %s" % (what, j, ps))


@gpu
def test_fetch_end_hands_out_batch_n_while_batch_n_plus_1_runs(world):
    """A.2 on one mapper: sub-batches of 97, 260, 1, 200 and 42 reads, parameters alternating; every fetch_end returns the batch
    before the one just launched, under that batch's own parameters; its BatchOut stays intact while the next batch runs; the
    work counters read behind fetch_begin are those of that batch run alone."""
    w, mp, gix = world["w"], world["mappers"][0], world["gix"]
    batches = _sub_batches(w)
    jobs = [(j, rd.batch_parset(j)) for j in range(len(batches))]
    got = {}
    _run_interleaved([_schedule(mp, gix, batches, jobs, got)])
    assert sorted(got) == list(range(len(batches)))
    _check_schedule(w, got, jobs, "one mapper")
    alone = {}
    for j, ps in jobs:
        batches[j].launch(mp, rd.gpu_params(gix, rd.PARSETS[ps][0]))
        rc, out = mp.fetch_results_rc()
        assert rc == 0
        alone[j] = mp.timers()[1]
    for j, _ in jobs:
        for name, ix in WORK_STABLE.items():
            assert got[j][4][ix] == alone[j][ix], (j, name, got[j][4][ix], alone[j][ix])
    for j in range(1, len(jobs)):                              # the comparison can tell neighbours apart
        assert alone[j][WORK_STABLE["lookups"]] != alone[j - 1][WORK_STABLE["lookups"]]
        assert alone[j][WORK_STABLE["lookups"]] > 0


@gpu
def test_two_mappers_on_one_index_take_the_sub_batches_in_turn(world):
    """A.2, the --streams 2 pattern: the same schedule over two mappers whose calls alternate; on each mapper the parameters
    alternate from one of its batches to the next"""
    w, gix = world["w"], world["gix"]
    batches = _sub_batches(w)
    got, jobs = {}, []
    gens = []
    for si, mp in enumerate(world["mappers"]):
        mine = [(j, "default" if t % 2 == 0 else "all40") for t, j in enumerate(range(si, len(batches), 2))]
        jobs += mine
        gens.append(_schedule(mp, gix, batches, mine, got))
    _run_interleaved(gens)
    assert sorted(got) == list(range(len(batches)))
    _check_schedule(w, got, jobs, "two mappers")


@gpu
def test_fetch_protocol_errors(world):
    """A.2: fetch_end without fetch_begin, a second fetch_end, a batch above max_batch_reads, total_bases above the capacity"""
    w, gix, api = world["w"], world["gix"], world["api"]
    par = gix.default_params()
    mp = api.Mapper(gix, 64, world["maxlen"], slot_budget_gb=2)
    try:
        rc, _ = mp.fetch_end_rc()
        assert rc == EARG and b"fetch_begin" in api.lib().smaltgpu_last_error()
        b = DevBatch(w["reads"][:64])
        b.launch(mp, par)
        mp.fetch_begin()
        rc, out = mp.fetch_end_rc()
        assert rc == 0 and out.nreads == 64
        _check_reads(*mp.unpack(out), w["exp"]["default"], range(64), "after a refused fetch_end")
        rc, _ = mp.fetch_end_rc()
        assert rc == EARG
        cap_reads, cap_len, cap_bases = C.c_uint32(), C.c_uint32(), C.c_uint64()
        assert api.lib().smaltgpu_mapper_capacity(mp.h, C.byref(cap_reads), C.byref(cap_len), C.byref(cap_bases)) == 0
        assert cap_reads.value == 64
        big = DevBatch(w["reads"][:65])
        with pytest.raises(api.SmaltGpuError) as e:
            big.launch(mp, par)
        assert e.value.code == EARG
        with pytest.raises(api.SmaltGpuError) as e:             # refused before anything is launched: the arguments alone decide
            mp.map_batch_device(b.d_bases, 0, b.d_off, b.n, cap_bases.value + 1, par)
        assert e.value.code == EARG
        b.launch(mp, par)                                       # the mapper is usable after the refusals
        rc, out = mp.fetch_results_rc()
        assert rc == 0
        _check_reads(*mp.unpack(out), w["exp"]["default"], range(64), "after the refusals")
    finally:
        mp.close()


@gpu
def test_fetch_end_on_three_host_threads(world):
    """A.3: 16 400 reads (the first 400 of the workload, 41 times over) so that fetch_end splits its copy over three threads
    (n / 8192 + 1 = 3); every copy of a read carries that read's results, res_off is monotone, no DiffStr range overlaps
    another; one thread gives the same."""
    w, gix, api = world["w"], world["gix"], world["api"]
    nrep, nuniq = 41, 400
    n = nrep * nuniq
    assert n // 8192 + 1 == 3
    b = DevBatch(w["reads"][:nuniq] * nrep)
    exp = w["exp"]["default"]
    mp = api.Mapper(gix, n, world["maxlen"], slot_budget_gb=4)
    try:
        runs = []
        for nt in (3, 1):
            mp.set_host_threads(nt)
            b.launch(mp, gix.default_params())
            mp.fetch_begin()
            rc, out = mp.fetch_end_rc()
            assert rc == 0 and out.nreads == n, (rc, api.lib().smaltgpu_last_error())
            off = np.array([out.res_off[i] for i in range(n + 1)], dtype=np.int64)
            assert off[0] == 0 and (np.diff(off) >= 0).all()
            assert [out.stat[i].nres for i in range(n)] == list(np.diff(off))
            spans = sorted((out.res[j].stroffs, out.res[j].strlen) for j in range(int(off[n])))
            assert all(s[1] >= 1 for s in spans)
            assert all(a[0] + a[1] <= c[0] for a, c in zip(spans, spans[1:])), "DiffStr ranges overlap"
            res, stats = mp.unpack(out)
            _check_reads(res, stats, exp, [i % nuniq for i in range(n)], "%d host threads" % nt)
            runs.append((res, stats))
        assert runs[0] == runs[1]
    finally:
        mp.close()


@gpu
def test_pool_overflow_on_the_device_path(oracle_built, tmp_path):
    """A.4: a mapper with 8 ranked candidates per read under a batch that ranks more: fetch_end returns SMALTGPU_ECAP with the
    batch filled; every read either carries that code and no results, or no code and the oracle's results; both kinds occur.
    The same batch through smaltgpu_map_batch on the same mapper matches the oracle for every read, and a device batch of the
    reads that rank few candidates comes back whole."""
    import oracle_lib as ol
    from smalt_amd import api
    o = rd.overflow()
    reads, exp = o["reads"], o["exp"]
    n = len(reads)
    pre = str(tmp_path / "ovf")
    assert ol.lib().or_index_write(o["oix0"], pre.encode()) == 0
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, n, 100, cands_per_read=rd.POOL_PER_READ, slot_budget_gb=4)
    try:
        par = gix.default_params()
        b = DevBatch(reads)
        b.launch(mp, par)
        mp.fetch_begin()
        rc, out = mp.fetch_end_rc()
        assert rc == ECAP and out.nreads == n, (rc, out.nreads)
        res, stats = mp.unpack(out)
        dropped = [i for i in range(n) if stats[i]["err"] == ECAP]
        whole = [i for i in range(n) if stats[i]["err"] == 0]
        print("reads that did not fit: %d of %d" % (len(dropped), n))
        assert len(dropped) + len(whole) == n and dropped and whole
        assert all(res[i] == [] for i in dropped)
        _check_reads([res[i] for i in whole], [stats[i] for i in whole], exp, whole, "reads that fitted")
        assert mp.remap_batches() == 0                           # the device path leaves the recovery to its caller
        res, stats = mp.map_batch(reads, None, par)
        _check_reads(res, stats, exp, range(n), "map_batch on the same mapper")
        assert mp.remap_batches() > 0
        plain = o["plain"]
        b2 = DevBatch([reads[i] for i in plain])
        b2.launch(mp, par)
        rc, out = mp.fetch_results_rc()
        assert rc == 0 and out.nreads == len(plain)
        _check_reads(*mp.unpack(out), exp, plain, "device batch after the overflow")
    finally:
        mp.close()
        gix.close()


# ---------------------------------------------------------------- B. pairs ----------------------------------------------------------------

class ResidentFile:
    """reads1 / reads2 of a pair fixture as the two resident batches, with their qualities, and the host copies"""

    def __init__(self, api, fx, with_quals=True):
        import torch
        self.keep = []
        self.n = len(fx["reads1"])
        self.bases, self.quals, self.h_off, self.d_bases, self.d_quals, self.d_off = [], [], [], [], [], []
        for rds in (fx["reads1"], fx["reads2"]):
            bs = np.frombuffer(b"".join(r[1] for r in rds), dtype=np.uint8).copy()
            qs = np.frombuffer(b"".join(r[2] for r in rds), dtype=np.uint8).copy()
            off = np.zeros(len(rds) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(r[1]) for r in rds])
            slack = np.zeros(512, dtype=np.uint8)                 # room behind the last read, as the mapper's own buffers have
            t = [torch.from_numpy(np.concatenate([bs, slack])).to(_dev()), torch.from_numpy(np.concatenate([qs, slack])).to(_dev()),
                 torch.from_numpy(off.astype(np.int64)).to(_dev())]
            self.keep += t
            self.bases.append(bs); self.quals.append(qs); self.h_off.append(off)
            self.d_bases.append(t[0].data_ptr()); self.d_quals.append(t[1].data_ptr() if with_quals else None); self.d_off.append(t[2].data_ptr())
        torch.cuda.synchronize()
        self.api = api

    def src(self, b0=0, n=None, quals=True):
        """the window of n pairs from pair b0 on: the whole d_bases, the offsets from entry b0 on"""
        s = self.api.ResidentReads()
        n = self.n - b0 if n is None else n
        for w in (0, 1):
            s.d_bases[w] = self.d_bases[w]
            s.d_quals[w] = self.d_quals[w] if quals else None
            s.d_read_off[w] = self.d_off[w] + 8 * b0
            s.read_off[w] = self.h_off[w].ctypes.data + 8 * b0
            s.nreads[w] = n
        return s


@pytest.fixture(scope="module")
def pairworld(oracle_built, tmp_path_factory):
    from smalt_amd import api
    tmp = tmp_path_factory.mktemp("respairs")
    cache = {}

    def get(tag):
        if tag not in cache:
            fx = pr.load_fixture(PAIRS[tag], tmp)
            gix = api.Index.load(fx["prefix"], 0)
            cache[tag] = dict(fx=fx, gix=gix, file=ResidentFile(api, fx), maxlen=max(len(r[1]) for r in fx["reads1"] + fx["reads2"]),
                              fq=[open(os.path.join(str(tmp), tag + e), "rb").read() for e in ("_1.fq", "_2.fq")])
        return cache[tag]
    yield get
    for v in cache.values():
        v["gix"].close()


def _round_params(api, gix, fx, key):
    par = gix.default_params()
    par.min_cover, par.min_swatscor_below_max, par.min_basqval = key[0], key[2], fx["min_basq"]
    par.rmapflg = key[1] & (api.FLG_BEST | api.FLG_SEQBYSEQ | api.FLG_NOSHRTINFO | api.FLG_SENSITIVE)
    return par


def _round_groups(lst):
    """the calls of a round by batch-wide parameters, each group in recorded call order"""
    keys = sorted({(c["mincov"], c["flags"], c["belowmax"]) for _, c in lst})
    return [(key, [(P, c) for P, c in lst if (c["mincov"], c["flags"], c["belowmax"]) == key]) for key in keys]


def _check_results_only(call, results, cand_first, stats):
    """pair_replay.check_call without the stage lines: the alignments behind append_rule (which reads the candidate-first
    flags) and the RX scalars"""
    got = pr.append_rule(results, cand_first, call["pl"])
    assert len(got) == len(call["rs"]), (len(got), len(call["rs"]))
    for a, b in zip(got, call["rs"]):
        assert a == b, (a, b)
    assert (len(got),) + tuple(stats[0:6]) == call["rx"], ((len(got),) + tuple(stats[0:6]), call["rx"])


def _resident_round(mp, src, what, sub, par, copies=1):
    sub = sub * copies
    return mp.map_batch_ctx_resident(src, [2 * P["no"] + c["mate"] for P, c in sub], par,
                                     intervals=None if what == "plain" else [c["ivs"] for _, c in sub],
                                     min_swatscor=[c["minscor"] for _, c in sub], prev_max=[c["prevmax"] for _, c in sub],
                                     fine_index=(what == "fine"), raw_alignments=True)


@gpu
@pytest.mark.parametrize("tag", ["gp_k13s6_ties", "gp_k13s2_d5"])
def test_recorded_calls_through_the_resident_round_calls(tag, pairworld):
    """B.5: every recorded mapSingleRead call of the fixture through smaltgpu_map_batch_ctx_resident, ids = 2 * pair + mate in
    recorded call order (a round mixes both batches).  smaltgpu_dump_read serves a resident round -- it reads the stages' state
    on the device and the read lengths that gather_round leaves in the mapper -- so every call passes pair_replay.check_call in
    full: stage lines at debug level 1, alignments behind append_rule, RX.  Then the hit totals of all 2 * npairs reads from
    the resident batches: equal to those from host memory, and the rare-mate order the reference took."""
    from smalt_amd import api
    pw = pairworld(tag)
    fx, gix, rf, entry = pw["fx"], pw["gix"], pw["file"], PAIRS[tag]
    assert rf.n == entry["npairs"]
    rounds = _rounds([(P, c) for P in fx["pairs"] for c in P["calls"]])
    assert len(rounds["fine"]) == entry["fine_calls"] and len(rounds["restricted"]) == entry["restricted_calls"]
    src = rf.src()
    ndone = 0
    for what, lst in rounds.items():
        for key, sub in _round_groups(lst):
            mates = [c["mate"] for _, c in sub]
            assert 0 in mates and 1 in mates                     # the round draws on both batches
            mp = api.Mapper(gix, len(sub), pw["maxlen"], slot_budget_gb=4)
            mp.set_debug(1)
            try:
                res, stats, cf = _resident_round(mp, src, what, sub, _round_params(api, gix, fx, key))
                for i, (P, c) in enumerate(sub):
                    st = stats[i]
                    assert st["err"] == 0
                    name = (fx["reads2"] if c["mate"] else fx["reads1"])[P["no"]][0]
                    lines = pr.stage_lines(mp.dump_read(i, name))
                    lines[0] = lines[0].replace("READ %d " % i, "READ %d " % P["no"], 1)
                    try:
                        pr.check_call(c, lines, res[i], cf[i], tuple(st[k] for k in SCALARS))
                    except AssertionError as e:
                        raise AssertionError("%s round, pair %d (mate %d, %d intervals): %s" % (what, P["no"], c["mate"], c["niv"], str(e)[:800]))
                    assert (st["max1"] >= 1) or not res[i]
                    ndone += 1
            finally:
                mp.close()
    assert ndone == entry["calls"]
    mp = api.Mapper(gix, 2 * rf.n, pw["maxlen"], slot_budget_gb=4)
    try:
        par = gix.default_params()
        par.min_basqval = fx["min_basq"]
        rds = [x for p in range(rf.n) for x in (fx["reads1"][p], fx["reads2"][p])]
        tot = mp.hit_totals_resident(src, list(range(2 * rf.n)), par)
        assert tot == mp.hit_totals([r[1] for r in rds], [r[2] for r in rds], par)
        assert sum(1 for t in tot if t) > rf.n
        perm = list(np.random.default_rng(7).permutation(2 * rf.n))              # any order of ids
        assert mp.hit_totals_resident(src, [int(x) for x in perm], par) == [tot[int(x)] for x in perm]
        k = gix.info().k
        for P in fx["pairs"]:
            j = P["no"]
            l1, l2 = len(rds[2 * j][1]), len(rds[2 * j + 1][1])
            if l1 < k or l2 < k or not P["calls"]:
                continue
            first = P["calls"][0]["mate"]
            assert first == (1 if tot[2 * j] > tot[2 * j + 1] else 0), (P["no"], tot[2 * j], tot[2 * j + 1], first)
    finally:
        mp.close()


@gpu
def test_resident_rounds_recover_from_a_pool_overflow(pairworld):
    """B.5 on a mapper with cands_per_read = 8.  One copy of a restricted or fine round of the fixtures cannot overflow the pool
    (test_restricted_rounds_of_the_fixtures_overflow_only_in_copies), so every round is sent 2, 6 and 7 times over in one
    batch.  The round must come back through the host copy of the gathered round -- remap_batches() rises, in the restricted
    and in the fine round too -- and every copy of every call must pass.  A debug batch is not recovered (the dump needs the
    state of the one batch), so the stage lines are left to the test above: alignments, candidate-first flags and RX here."""
    from smalt_amd import api
    tag = "gp_k13s6_ties"
    pw = pairworld(tag)
    fx, gix, rf = pw["fx"], pw["gix"], pw["file"]
    rounds = _rounds([(P, c) for P in fx["pairs"] for c in P["calls"]])
    src = rf.src()
    for what, lst in rounds.items():
        groups = _round_groups(lst)
        assert len(groups) == 1
        key, sub = groups[0]
        copies = _copies_to_overflow(sub)
        n = len(sub) * copies
        mp = api.Mapper(gix, n, pw["maxlen"], cands_per_read=rd.POOL_PER_READ, slot_budget_gb=4)
        try:
            assert mp.remap_batches() == 0
            res, stats, cf = _resident_round(mp, src, what, sub, _round_params(api, gix, fx, key), copies)
            print("%s round: %d calls x %d, recovered in %d batches" % (what, len(sub), copies, mp.remap_batches()))
            assert mp.remap_batches() > 0, what
            for i in range(n):
                P, c = sub[i % len(sub)]
                st = stats[i]
                assert st["err"] == 0, (what, i, st["err"])
                try:
                    _check_results_only(c, res[i], cf[i], tuple(st[k] for k in SCALARS))
                except AssertionError as e:
                    raise AssertionError("%s round, copy %d of pair %d (mate %d): %s" % (what, i // len(sub), P["no"], c["mate"], str(e)[:800]))
        finally:
            mp.close()


def _report_setup(api, gix, opts, k):
    """`smalt map` options -> (Params, PairOpts, ReportOpts, seed of the random draws or None), as smaltgpu-map sets them"""
    from test_pairs_replay import driver_args
    a = dict(x.split("=") for x in driver_args(opts, k))
    par = gix.default_params()
    o = dict(zip(opts[0::2], opts[1::2]))
    if "-m" in o:
        par.min_swatscor = int(o["-m"])
    par.min_swatscor_below_max = int(a["below"])
    if int(a["below"]):
        par.rmapflg &= ~api.FLG_BEST
    par.min_basqval = int(o.get("-q", 0))
    po = api.PairOpts(int(a["dmin"]), int(a["dmax"]), int(a["lib"]), 0, 2)
    ro = api.ReportOpts()
    ro.format, ro.modflags, ro.outflags = int(a["fmt"]), int(a["mod"]), int(a["out"])
    ro.min_swscor, ro.min_swscor_below_max, ro.min_identity = int(a["minsw"]), int(a["below"]), float(a["minid"])
    seed = int(a["seed"]) if ro.outflags & api.OUT_RANDSEL else None
    assert seed is None or seed > 0
    return par, po, ro, seed


class Reporter:
    """smaltgpu_report_emit_pairs over blocks of a fixture's read files"""

    def __init__(self, api, gix, fq, ro):
        self.api, self.L, self.fq = api, api.lib(), fq
        self.names_p, self.sop_p, self.nseq = C.POINTER(C.c_char_p)(), C.POINTER(C.c_uint64)(), C.c_int64()
        assert self.L.smaltgpu_index_seqnames(gix.h, C.byref(self.names_p), C.byref(self.sop_p), C.byref(self.nseq)) == 0
        self.rep = self.L.smaltgpu_report_create()
        txt, ln = C.c_void_p(), C.c_uint64()
        argv = (C.c_char_p * 1)(b"smalt")
        assert self.L.smaltgpu_report_header(self.rep, self.names_p, self.sop_p, self.nseq, C.byref(ro), b"smalt", b"0.7.6", 1, argv, C.byref(txt), C.byref(ln)) == 0
        self.recs = [t.split(b"\n") for t in fq]
        self.rs = [self.L.smaltgpu_reads_create() for _ in (0, 1)]

    def seed(self, seed):
        if seed is not None:
            C.CDLL(None).srand48(C.c_long(seed))

    def lines(self, handle, b0, n, ro, po):
        views, texts = [], []
        for w in (0, 1):
            text = b"\n".join(self.recs[w][4 * b0:4 * (b0 + n)]) + b"\n"
            v = self.api.ReadsView()
            assert self.L.smaltgpu_reads_parse(self.rs[w], text, len(text), 1, 0, 1, C.byref(v)) == 0 and v.nreads == n
            views.append(v); texts.append(text)
        txt, ln = C.c_void_p(), C.c_uint64()
        assert self.L.smaltgpu_report_emit_pairs(self.rep, handle, C.byref(views[0]), C.byref(views[1]), self.names_p, self.nseq, C.byref(ro), C.byref(po), 2,
                                                 C.byref(txt), C.byref(ln)) == 0, self.L.smaltgpu_last_error()
        return [x for x in C.string_at(txt.value, ln.value).split(b"\n") if x] if ln.value else []

    def close(self):
        self.L.smaltgpu_report_free(self.rep)
        for r in self.rs:
            self.L.smaltgpu_reads_free(r)


def _block_variants():
    """per fixture tag the SAM variant and the CIGAR variant whose -m changes the mapping itself"""
    out = []
    for tag in PAIRS:
        mine = {c["variant"]: c for c in REPORTS if c["tag"] == tag}
        assert mine["cigar_filt"]["remap"] and "-m" in mine["cigar_filt"]["opts"]
        out += [mine["sam"], mine["cigar_filt"]]
    return out


def test_block_variants_cover_every_fixture():
    v = _block_variants()
    assert len(v) == 2 * len(PAIRS) == 10
    assert all("-r" in c["opts"] and int(c["opts"][c["opts"].index("-r") + 1]) > 0 for c in v)      # random draws in every case
    assert sum(1 for t in PAIRS if PAIRS[t]["npairs"] % 32) >= 4                                    # a last block that is not full


def _expected_lines(case):
    with gzip.open(os.path.join(gu.GOLD, "%s.%s.out.gz" % (case["tag"], case["variant"])), "rb") as g:
        return [x for x in g.read().split(b"\n") if x and not x.startswith(b"@")]


@gpu
@pytest.mark.parametrize("case", _block_variants(), ids=["%s-%s" % (c["tag"], c["variant"]) for c in _block_variants()])
def test_resident_blocks_print_what_smalt_map_prints(case, pairworld):
    """B.6 with host copies of bases and qualities: the file as one block, and as blocks of 32 pairs that are windows into the
    resident file, mapped and emitted in file order (the random draws run through the file)"""
    from smalt_amd import api
    pw = pairworld(case["tag"])
    fx, gix, rf = pw["fx"], pw["gix"], pw["file"]
    par, po, ro, seed = _report_setup(api, gix, case["opts"], PAIRS[case["tag"]]["k"])
    want = _expected_lines(case)
    assert len(want) >= 2 * rf.n
    mp = api.Mapper(gix, 2 * rf.n, pw["maxlen"], slot_budget_gb=4)
    rp = Reporter(api, gix, pw["fq"], ro)
    h = None
    try:
        for step in (rf.n, 32):
            rp.seed(seed)
            got = []
            for b0 in range(0, rf.n, step):
                n = min(step, rf.n - b0)
                h, info, calls, _ = mp.map_pairs_resident(rf.src(b0, n), n, par, po, rf.bases[0], rf.quals[0], rf.bases[1], rf.quals[1], pairs_handle=h)
                assert len(info) == n and calls[0] >= 1
                got += rp.lines(h, b0, n, ro, po)
            assert len(got) == len(want), (step, len(got), len(want))
            for i, (x, y) in enumerate(zip(got, want)):
                assert x == y, (step, i, x, y)
    finally:
        if h:
            api.lib().smaltgpu_pairs_free(h)
        rp.close()
        mp.close()


def _bench_opts(api, gix):
    par = gix.default_params()
    po = api.PairOpts(0, 500, api.LIB_PE, 0, 2)
    ro = api.ReportOpts()
    ro.format, ro.min_swscor, ro.outflags = api.FMT_CIGAR, 18, api.OUT_BEST | api.OUT_SINGLE | api.OUT_RANDSEL
    return par, po, ro


@gpu
@pytest.mark.parametrize("tag", ["gp_k13s6_pe", "gp_k13s6_ties"])
def test_resident_block_as_the_benchmark_calls_it(tag, pairworld):
    """B.6 without host copies and without qualities on either side: pair info, calls per round and report lines equal those of
    smaltgpu_map_pairs on the same reads with quals = None"""
    from smalt_amd import api
    pw = pairworld(tag)
    gix, rf = pw["gix"], pw["file"]
    par, po, ro = _bench_opts(api, gix)
    mp = api.Mapper(gix, 2 * rf.n, pw["maxlen"], slot_budget_gb=4)
    rp = Reporter(api, gix, pw["fq"], ro)
    try:
        h1, info1, calls1, _ = mp.map_pairs_raw(rf.bases[0], rf.h_off[0], None, rf.bases[1], rf.h_off[1], None, par, po)
        info1 = info1.copy()
        rp.seed(3)
        lines1 = rp.lines(h1, 0, rf.n, ro, po)
        h2, info2, calls2, _ = mp.map_pairs_resident(rf.src(quals=False), rf.n, par, po)
        rp.seed(3)
        lines2 = rp.lines(h2, 0, rf.n, ro, po)
        assert calls1 == calls2 and calls1[0] >= rf.n // 2 and calls1[1] >= rf.n // 2
        assert np.array_equal(info1, info2)
        assert lines1 == lines2 and len(lines1) >= 2 * rf.n
        assert int((info2[:, 0] & 1).sum()) >= rf.n // 2           # pairs were found
        api.lib().smaltgpu_pairs_free(h1)
        api.lib().smaltgpu_pairs_free(h2)
    finally:
        rp.close()
        mp.close()


@gpu
def test_two_host_threads_with_a_mapper_each_on_one_index(pairworld):
    """B.6: two host threads, each with its own mapper and handle, take blocks of 32 pairs in turn as bench.py's one_step does;
    per block the pair info equals that of a serial run"""
    from smalt_amd import api
    pw = pairworld("gp_k13s6_pe")
    gix, rf = pw["gix"], pw["file"]
    par, po, _ = _bench_opts(api, gix)
    blocks = [(b0, min(32, rf.n - b0)) for b0 in range(0, rf.n, 32)]
    mappers = [api.Mapper(gix, 64, pw["maxlen"], slot_budget_gb=4) for _ in range(3)]
    try:
        serial = {}
        h = None
        for b0, n in blocks:
            h, info, calls, _ = mappers[2].map_pairs_resident(rf.src(b0, n, quals=False), n, par, po, pairs_handle=h)
            serial[b0] = (info.copy(), calls)
        api.lib().smaltgpu_pairs_free(h)
        state = {"next": 0, "err": []}
        got, who = {}, {}
        lock = threading.Lock()
        turn = threading.Barrier(2)

        def drive(si):
            h = None
            try:
                turn.wait(timeout=60)
                while True:
                    with lock:
                        b = state["next"]
                        state["next"] += 1
                    if b >= len(blocks) or state["err"]:
                        break
                    b0, n = blocks[b]
                    h, info, calls, _ = mappers[si].map_pairs_resident(rf.src(b0, n, quals=False), n, par, po, pairs_handle=h)
                    got[b0] = (info.copy(), calls)
                    who[b0] = si
            except Exception as e:                                 # noqa: BLE001 -- reported by the main thread
                state["err"].append(repr(e))
            finally:
                if h:
                    api.lib().smaltgpu_pairs_free(h)
        th = [threading.Thread(target=drive, args=(i,)) for i in (0, 1)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not state["err"], state["err"]
        assert sorted(got) == [b0 for b0, _ in blocks]
        for b0, _ in blocks:
            assert np.array_equal(got[b0][0], serial[b0][0]) and got[b0][1] == serial[b0][1], (b0, who[b0])
    finally:
        for m in mappers:
            m.close()


@gpu
def test_concatenated_mode_and_short_batches_on_the_resident_call(pairworld):
    """B.6: with SMALTGPU_FLG_SEQBYSEQ cleared the call needs the host bases and says so; with them it equals smaltgpu_map_pairs
    under the same flags; resident batches shorter than the block are refused"""
    from smalt_amd import api
    pw = pairworld("gp_k13s6_ties")
    gix, rf = pw["gix"], pw["file"]
    par, po, ro = _bench_opts(api, gix)
    assert par.rmapflg & api.FLG_SEQBYSEQ
    par.rmapflg &= ~api.FLG_SEQBYSEQ
    L = api.lib()
    mp = api.Mapper(gix, 2 * rf.n, pw["maxlen"], slot_budget_gb=4)
    rp = Reporter(api, gix, pw["fq"], ro)
    try:
        with pytest.raises(api.SmaltGpuError) as e:
            mp.map_pairs_resident(rf.src(), rf.n, par, po)
        assert e.value.code == EARG and "concatenated mode" in str(e.value)
        h1, info1, calls1, _ = mp.map_pairs_raw(rf.bases[0], rf.h_off[0], rf.quals[0], rf.bases[1], rf.h_off[1], rf.quals[1], par, po)
        info1 = info1.copy()
        rp.seed(3)
        lines1 = rp.lines(h1, 0, rf.n, ro, po)
        h2, info2, calls2, _ = mp.map_pairs_resident(rf.src(), rf.n, par, po, rf.bases[0], rf.quals[0], rf.bases[1], rf.quals[1])
        rp.seed(3)
        lines2 = rp.lines(h2, 0, rf.n, ro, po)
        assert calls1 == calls2 and np.array_equal(info1, info2) and lines1 == lines2 and len(lines1) >= 2 * rf.n
        L.smaltgpu_pairs_free(h1)
        L.smaltgpu_pairs_free(h2)
        par.rmapflg |= api.FLG_SEQBYSEQ
        for w in (0, 1):
            s = rf.src()
            s.nreads[w] = rf.n - 1
            with pytest.raises(api.SmaltGpuError) as e:
                mp.map_pairs_resident(s, rf.n, par, po)
            assert e.value.code == EARG and "do not hold the block" in str(e.value)
    finally:
        rp.close()
        mp.close()

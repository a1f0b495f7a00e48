"""bench.py --dump-outputs without a device: OutputDump takes the sampled reads of each BatchOut the timed path hands back
(ReadStat, alignments, DiffStr bytes) and writes them in read order, within the size budget."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _batches(nreads, sub, seed):
    """BatchOut structures as smaltgpu_fetch_end fills them, and per read the (score, s_start, DiffStr) it must come back with"""
    from smalt_amd import api
    rng = np.random.default_rng(seed)
    truth, outs, keep = {}, [], []
    for first in range(0, nreads, sub):
        n = min(sub, nreads - first)
        cnt = rng.integers(0, 4, n)
        off = (C.c_uint64 * (n + 1))(*np.concatenate([[0], np.cumsum(cnt)]).tolist())
        nres = int(cnt.sum())
        res = (api.Result * max(1, nres))()
        ds = bytearray()
        for j in range(nres):
            ln = int(rng.integers(1, 6))
            res[j].swatscor, res[j].s_start, res[j].stroffs, res[j].strlen = j + 10 * first, 3_000_000_000 + j, len(ds), ln
            ds += bytes(rng.integers(0, 256, ln).astype(np.uint8))
        dsb = (C.c_uint8 * max(1, len(ds)))(*ds)
        st = (api.ReadStat * n)()
        for i in range(n):
            st[i].swatscor_max, st[i].n_hits_tot = first + i, 4_000_000_000
            truth[first + i] = [(res[j].swatscor, res[j].s_start, bytes(ds[res[j].stroffs:res[j].stroffs + res[j].strlen])) for j in range(off[i], off[i + 1])]
        out = api.BatchOut()
        out.nreads, out.res_off, out.res, out.diffstr, out.stat = n, off, res, C.cast(dsb, C.POINTER(C.c_uint8)), st
        keep += [off, res, dsb, st]
        outs.append((out, first, n))
    return truth, outs, keep


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in os.listdir(path)}


def test_dump_holds_the_sampled_reads_in_read_order(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_READS", 50)
    truth, outs, _keep = _batches(300, 128, 1)
    d = bench.OutputDump(300)
    for out, first, n in outs:
        d.take(out, first, n)
    assert d.write(str(tmp_path)) == 50
    a = _load(str(tmp_path))
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    ri = a["read_index"].astype(int)
    assert len(ri) == 50 and (np.diff(ri) > 0).all()
    assert (a["read_stat"][:, 0] == ri).all() and (a["read_stat"][:, 5] == 4e9).all()
    r = b = 0
    for i, c in zip(ri, a["read_nres"].astype(int)):
        assert len(truth[i]) == c
        for sw, s_start, ds in truth[i]:
            assert a["results"][r, 0] == sw and a["results"][r, 3] == s_start and a["results"][r, 7] == len(ds)
            assert bytes(a["diffstr"][b:b + len(ds)].astype(np.uint8)) == ds
            r, b = r + 1, b + len(ds)
    assert r == len(a["results"]) and b == len(a["diffstr"])
    # the same seed picks the same reads
    assert (bench.OutputDump(300).pick == d.pick).all()


def test_dump_keeps_a_prefix_of_the_sample_within_the_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_READS", 50)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 4096 + 2000)
    _truth, outs, _keep = _batches(300, 128, 2)
    d = bench.OutputDump(300)
    for out, first, n in outs:
        d.take(out, first, n)
    kept = d.write(str(tmp_path))
    assert 0 < kept < 50
    a = _load(str(tmp_path))
    assert (a["read_index"] == d.pick[:kept]).all()
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))) <= 4096 + 2000 + 5 * 128

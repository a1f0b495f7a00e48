"""The seeding stage's instance of the wave sort, wave_sort_kv<SEED_IDXBITS, SEED_LISTCAP, SEED_LSTK> on elements packed
(key << 12) | i in LDS (Mapper.rank_sort_batch(instance=1)), against the oracle's restatement of the reference's unstable
quicksort (sort.c:233): keys and permutation equal.  test_gpu_ranksort.py holds the default instance of the candidate ranking
only; with a list of 32 short ranges this one flushes the list in the middle of the recursion on the committed adversaries
(tests/golden/seedsort_adversaries.json; test_seed_ref.py counts their ranges)."""
import json
import os

import numpy as np
import pytest

import golden_util as gu
import oracle_lib as ol
import seed_inputs as si
import seed_ref as sr

pytestmark = pytest.mark.gpu
EARG = -3                       # SMALTGPU_EARG


def _expect(a):
    k = np.ascontiguousarray(a, dtype=np.uint32).copy()
    v = np.arange(len(a), dtype=np.uint32)
    if len(a):
        ol.lib().or_sort2_u32(len(a), k.ctypes.data, v.ctypes.data)
    return k, v


def _shapes(a):
    """sorted, reversed, organ pipe, valley, constant"""
    a = np.sort(a)
    up, down = a[::2], a[1::2][::-1]
    return [a, a[::-1].copy(), np.concatenate([up, down]), np.concatenate([down, up]), np.full(a.size, a[a.size // 2], dtype=np.uint32)]


@pytest.fixture(scope="module")
def mapper(oracle_built, tmp_path_factory):
    from smalt_amd import api
    oix, prefix = si.build_index([b"ACGGTCATTGCAGTCAGGATCCATGACGTTAGCATCAGT" * 40], 11, 3, tmp_path_factory.mktemp("sortix"), "x")
    gix = api.Index.load(prefix, 0)
    mp = api.Mapper(gix, 16, 128)
    yield mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


def _check(mapper, arrs):
    got = mapper.rank_sort_batch(arrs, instance=1)
    for t, (a, (gk, gi)) in enumerate(zip(arrs, got)):
        ek, ei = _expect(a)
        assert np.array_equal(gk, ek), (t, len(a))
        assert np.array_equal(gi, ei), (t, len(a), int(a.max()) if len(a) else 0)


def test_seed_sort_sizes_and_key_ranges(mapper):
    rng = np.random.default_rng(12)
    arrs = []
    for n in list(range(0, 81)) + [127, 128, 129, 254, 255]:
        for kmax in (1, 2, 3, 8, 40, 1000, (1 << 20) - 1):
            arrs.append(rng.integers(0, kmax, size=n, endpoint=True, dtype=np.uint32))
    for n in (8, 33, 64, 255, 1000, 4095):
        for kmax in (5, 100, (1 << 20) - 1):
            arrs += _shapes(rng.integers(0, kmax, size=n, endpoint=True, dtype=np.uint32))
    _check(mapper, arrs)


def test_seed_sort_adversaries_flush_the_range_list(mapper):
    """more than 32 listed ranges: the one-lane finish runs on 32 of the 64 lanes in the middle of the recursion; exactly 32:
    the flush empties the list at the very end"""
    with open(os.path.join(gu.GOLD, "seedsort_adversaries.json")) as f:
        adv = [np.array(d["keys"], dtype=np.uint32) for d in json.load(f)["arrays"]]
    counts = [sr.listed_ranges(a)[0] for a in adv]
    assert sum(1 for c in counts if c > 32) >= 3 and 32 in counts
    # the same orders with ties: every key halved and quartered (equal keys change the partitions: these are further inputs,
    # not adversaries by construction), and with the largest key the packed element holds
    more = [a // 2 for a in adv] + [a // 4 for a in adv] + [a + ((1 << 20) - 1 - int(a.max())) for a in adv]
    _check(mapper, adv + more)


def test_seed_sort_hit_counts_of_the_sweep(mapper, tmp_path):
    """the arrays the stage sorts: hit counts of the seeds of every sweep strand in read order"""
    arrs = []
    for k, s in ((20, 1), (13, 1), (9, 6), (20, 17)):
        oix, _ = si.build_index(si.reference()[0], k, s, tmp_path, "ix%d_%d" % (k, s))
        try:
            reads, quals = si.sweep_reads(k, s)
            for e in sr.ref_batch(oix, reads, quals, sr.Par()):
                if e.seeds is not None and len(e.seeds) > 1 and int(e.seeds[:, 1].max()) < 1 << 20:
                    arrs.append(e.seeds[np.argsort(e.seeds[:, 2], kind="stable"), 1].astype(np.uint32))
        finally:
            ol.lib().or_index_free(oix)
    assert len(arrs) > 400 and max(a.size for a in arrs) > 500
    _check(mapper, arrs)


def test_seed_sort_refusals(mapper):
    from smalt_amd import api
    with pytest.raises(api.SmaltGpuError) as e:
        mapper.rank_sort_batch([np.zeros(4096, dtype=np.uint32)], instance=1)
    assert e.value.code == EARG
    with pytest.raises(api.SmaltGpuError) as e:
        mapper.rank_sort_batch([np.array([1, 1 << 20], dtype=np.uint32)], instance=1)
    assert e.value.code == EARG
    with pytest.raises(api.SmaltGpuError) as e:
        mapper.rank_sort_batch([np.array([1, 2], dtype=np.uint32)], instance=2)
    assert e.value.code == EARG
    _check(mapper, [np.arange(4095, dtype=np.uint32)[::-1].copy(), np.array([(1 << 20) - 1, 0, (1 << 20) - 1], dtype=np.uint32)])

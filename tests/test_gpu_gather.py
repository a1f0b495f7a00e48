"""k_gather_reads on its own (Mapper.gather_batch) against the numpy gather: the aligned 16-byte path, the byte path and the
tail, by the alignment of source and destination offsets; with and without qualities; the guard behind the last read."""
import numpy as np
import pytest

import oracle_lib as ol
import seed_inputs as si

pytestmark = pytest.mark.gpu
LENS = (0, 1, 15, 16, 17, 31, 32, 33, 64, 150, 151, 1000)
GUARD = 0xA5


@pytest.fixture(scope="module")
def mapper(oracle_built, tmp_path_factory):
    from smalt_amd import api
    oix, prefix = si.build_index([b"ACGGTCATTGCAGTCAGGATCCATGACGTTAGCATCAGT" * 40], 11, 3, tmp_path_factory.mktemp("gix"), "x")
    gix = api.Index.load(prefix, 0)
    mp = api.Mapper(gix, 128, 1000)
    yield mp
    mp.close()
    gix.close()
    ol.lib().or_index_free(oix)


def _batch(rng, lens):
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    tot = int(off[-1])
    return rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=tot), rng.integers(33, 75, size=tot, dtype=np.uint8), off


def _batches():
    rng = np.random.default_rng(2024)
    a = _batch(rng, rng.choice(LENS, size=40))
    b = _batch(rng, rng.choice(LENS, size=40))
    m16 = _batch(rng, rng.choice((0, 16, 32, 64, 992), size=40))           # every length a multiple of 16: every offset is one
    return a, b, m16


def _cases(a, b):
    """id lists by the alignment of (source offset, destination offset) of their reads"""
    def ids_where(batches, want_src, pad_to):
        # reads whose source offset is (not) a multiple of 16, the destination offset steered by the lengths in front
        out, d = [], 0 if pad_to else int(a[2][odd // 2 + 1] - a[2][odd // 2])
        for w, (_, _, off) in enumerate(batches):
            for i in range(len(off) - 1):
                n = int(off[i + 1] - off[i])
                if ((int(off[i]) & 15) == 0) == want_src and ((d & 15) == 0) == pad_to and n:
                    out.append(2 * i + w)
                    d += n
        return out
    every = [2 * i + w for w in (0, 1) for i in range(40)]
    odd = next(2 * i for i in range(40) if int(a[2][i + 1] - a[2][i]) & 15)      # a read that leaves the destination off a multiple of 16
    return {
        "first read of a list": [every[3]],
        "source aligned only": [odd] + ids_where((a, b), True, False),
        "destination aligned only": ids_where((a, b), False, True),
        "neither": [odd] + ids_where((a, b), False, False),
        "both where the lengths allow": ids_where((a, b), True, True),
        "the same read twice": [2 * 5 + 1, 2 * 5 + 1, 2 * 7, 2 * 7, 2 * 7],
        "all from one batch": [2 * i + 1 for i in range(40)],
        "alternating batches": [2 * (i // 2) + (i & 1) for i in range(80)],
        "in reverse": every[::-1],
        "none": [],
    }


def _paths(batches, ids):
    """which of the kernel's paths a list runs: (vector or bytes, with a tail or not, (source, destination) offset a multiple of 16)"""
    seen, d = set(), 0
    for i in ids:
        so, n = int(batches[i & 1][2][i >> 1]), int(batches[i & 1][2][(i >> 1) + 1] - batches[i & 1][2][i >> 1])
        if n:
            seen.add(("vector" if (so | d) & 15 == 0 and n >= 16 else "bytes", "tail" if n & 15 else "whole", (so & 15 == 0, d & 15 == 0)))
        d += n
    return seen


def _expect(batches, ids, with_quals):
    db = [batches[i & 1][0][int(batches[i & 1][2][i >> 1]):int(batches[i & 1][2][(i >> 1) + 1])] for i in ids]
    dq = [batches[i & 1][1][int(batches[i & 1][2][i >> 1]):int(batches[i & 1][2][(i >> 1) + 1])] for i in ids]
    cat = lambda x: np.concatenate(x + [np.full(16, GUARD, np.uint8)])
    off = np.zeros(len(ids) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in db])
    return cat(db), (cat(dq) if with_quals else np.full(int(off[-1]) + 16, GUARD, np.uint8)), off


@pytest.mark.parametrize("with_quals", [True, False], ids=["quals", "noquals"])
def test_gather_equals_numpy(mapper, with_quals):
    a, b, m16 = _batches()
    strip = lambda t: t if with_quals else (t[0], None, t[2])
    seen = set()
    for batches, cases in (((a, b), _cases(a, b)), ((m16, m16), {"all offsets multiples of 16": [2 * i + (i & 1) for i in range(40)]})):
        for name, ids in cases.items():
            assert len(ids) <= 128 and (ids or name == "none"), name
            db, dq, do = mapper.gather_batch([strip(batches[0]), strip(batches[1])], ids, guard=GUARD)
            eb, eq, eo = _expect(batches, ids, with_quals)
            assert np.array_equal(do, eo), name
            assert np.array_equal(db, eb), (name, np.flatnonzero(db != eb)[:8])
            assert np.array_equal(dq, eq), (name, np.flatnonzero(dq != eq)[:8])
            seen |= _paths(batches, ids)
    assert {x[0] for x in seen} == {"vector", "bytes"} and ("vector", "tail", (True, True)) in seen and ("vector", "whole", (True, True)) in seen
    assert {x[2] for x in seen} == {(True, True), (True, False), (False, True), (False, False)}

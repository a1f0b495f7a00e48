"""The plain reference of the on-the-fly k=5 index (tests/fine_ref.py) against the oracle's or_index_build_fine, for every read of
every case that tests/test_gpu_fine_index.py gives the kernel; and what the cases promise about themselves.  No GPU."""
import numpy as np
import pytest

import fine_ref as fr
import oracle_lib as ol


@pytest.fixture(scope="module")
def ref(oracle_built):
    seqs = fr.workload()
    oix = ol.build_index(seqs, ["f%d" % i for i in range(len(seqs))], 13, 6)
    sop = np.ctypeslib.as_array(oix.contents.sop, shape=(len(seqs) + 1,)).copy()
    yield seqs, oix, sop
    ol.lib().or_index_free(oix)


def test_reference_geometry(ref):
    seqs, _, sop = ref
    assert sum(len(s) for s in seqs) <= 300_000
    assert all(int(sop[i]) % 4 for i in range(1, len(seqs)))
    assert all(int(sop[i + 1] - sop[i]) >= len(seqs[i]) for i in range(len(seqs)))
    lo_res = {(int(sop[sx]) + lo) % 16 for reads, _ in [fr.cases()["residues"]] for r in reads for sx, lo, _ in r}
    assert lo_res == set(range(16))


@pytest.mark.parametrize("name", sorted(fr.cases()))
def test_reference_equals_the_oracle(ref, name):
    seqs, oix, sop = ref
    reads, _ = fr.cases()[name]
    for r, ivs in enumerate(reads):
        idx, pos, cap = fr.fine_index(seqs, sop, ivs)
        fx = ol.build_fine_index(oix, ivs)
        try:
            o = fx.contents
            assert o.k == 5 and o.s == 1 and o.nkeys == fr.FINE_NKEYS
            assert np.array_equal(np.ctypeslib.as_array(o.idx, shape=(fr.FINE_NKEYS + 1,)), idx), (name, r)
            assert o.npos == pos.size == idx[-1] <= cap, (name, r)
            if pos.size:
                assert np.array_equal(np.ctypeslib.as_array(o.pos, shape=(pos.size,)), pos), (name, r)
        finally:
            ol.lib().or_index_free_fine(fx)


def test_cases_hold_what_they_are_about(ref):
    seqs, _, sop = ref
    cs = fr.cases()
    built = {name: [fr.fine_index(seqs, sop, ivs) for ivs in reads] for name, (reads, _) in cs.items()}
    # lengths 1-4: no word, a slice of no position; 5 and 6: one and two
    assert [b[2] for b in built["lengths"]] == [0, 0, 0, 0, 1, 2, 63, 64, 65, 128, 129, 0]
    assert all(int(b[0][-1]) == b[2] for b in built["lengths"])
    # letters: words are left out, so the slice has a tail that nobody writes
    assert all(int(b[0][-1]) < b[2] for b in built["letters"])
    assert int(built["letters"][3][0][-1]) == 0 and built["letters"][3][2] > 0            # a window of N only
    # abutting: no position whose word would cross the seam
    (_, lo0, hi0), _ = cs["abutting"][0][0]
    assert not set(range(int(sop[0]) + hi0 - 3, int(sop[0]) + hi0 + 1)) & set(built["abutting"][0][1].tolist())
    # twice: every position twice
    assert np.array_equal(built["twice"][0][1][0::2], built["twice"][0][1][1::2])
    # many: 2048 intervals; polya and dinuc: one and two keys own the list
    assert len(cs["many"][0][0]) == 2048
    assert int(np.diff(built["polya"][0][0].astype(np.int64)).max()) == 3000 - 4
    assert sorted(np.diff(built["dinuc"][0][0].astype(np.int64)).tolist())[-2:] == [1498, 1498]
    assert cs["mixed_grid3"][1] == 3 and len(cs["mixed_grid3"][0]) == 10

"""The kernel k_fine_index on its own (smaltgpu_fine_index_batch): the per-read k=5 index of the rescue round against the plain
reference of tests/fine_ref.py (which tests/test_fine_ref.py holds against the oracle), array by array.  The position buffer and
the index rows go in filled with a guard pattern: the unused tail of every read's slice, the pad words of every index row and
the word behind the last slice must come back as they went in."""
import numpy as np
import pytest

import fine_ref as fr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

GUARD = 0xA5C3E187


@pytest.fixture(scope="module")
def ctx(oracle_built, tmp_path_factory):
    from smalt_amd import api
    seqs = fr.workload()
    oix = ol.build_index(seqs, ["f%d" % i for i in range(len(seqs))], 13, 6)
    pre = str(tmp_path_factory.mktemp("fine") / "ix")
    assert ol.lib().or_index_write(oix, pre.encode()) == 0
    sop = np.ctypeslib.as_array(oix.contents.sop, shape=(len(seqs) + 1,)).copy()
    ol.lib().or_index_free(oix)
    gix = api.Index.load(pre, 0)
    mp = api.Mapper(gix, 64, 100)
    yield seqs, sop, mp
    mp.close()
    gix.close()


@pytest.mark.parametrize("name", sorted(fr.cases()))
def test_fine_index_equals_the_reference(ctx, name):
    seqs, sop, mp = ctx
    reads, grid = fr.cases()[name]
    got = mp.fine_index_batch(reads, grid=grid, guard=GUARD)
    exp = [fr.fine_index(seqs, sop, ivs) for ivs in reads]
    off = np.concatenate([[0], np.cumsum([e[2] for e in exp])])
    assert np.array_equal(got["fine_off"], off)
    assert got["pos"].size == off[-1] + 1 and got["pos"][-1] == GUARD, "the word behind the last slice was written"
    for r, (idx, pos, cap) in enumerate(exp):
        row = got["idx"][r]
        assert np.array_equal(row[:fr.FINE_NKEYS + 1], idx), (name, r, np.flatnonzero(row[:fr.FINE_NKEYS + 1] != idx)[:8])
        assert np.all(row[fr.FINE_NKEYS + 1:] == GUARD), (name, r)
        sl = got["pos"][off[r]:off[r + 1]]
        n = int(idx[-1])
        assert np.array_equal(sl[:n], pos), (name, r, np.flatnonzero(sl[:n] != pos)[:8])
        assert np.all(sl[n:] == GUARD), (name, r, "pos[idx[1024] .. cap) was written")
    print(name, "reads", len(reads), "grid", grid or len(reads), "words", int(off[-1]), "indexed", sum(int(e[0][-1]) for e in exp))

"""k_encode and k_seed on their own (Mapper.seed_batch) against the reference of tests/seed_ref.py: codes, all seven header fields,
the whole seed table and the whole row of qualifiers of every strand, the guard everywhere the reference defines nothing, the
lookup counter -- exact equality.  Inputs: tests/seed_inputs.py; which branch of stage_seed each strand takes is counted without
a GPU in test_seed_ref.py, and the one-lane form is held against the same reference in test_seed_paths.py.  Here the wave form
runs: the shuffle prefix sums, the reduction of the seed budget, the per-frame rank lists (s <= 16) and the walk over all seeds
(s > 16), in LDS and in HBM slots, with one workgroup meeting every strand in turn."""
import numpy as np
import pytest

import oracle_lib as ol
import seed_inputs as si
import seed_ref as sr

pytestmark = pytest.mark.gpu
EARG = -3                       # SMALTGPU_EARG


class Rig:
    """index on the device and in the oracle, one mapper"""

    def __init__(self, seqs, k, s, tmp, max_reads=320, max_len=si.MAXLEN):
        from smalt_amd import api
        self.k, self.s = k, s
        self.oix, prefix = si.build_index(seqs, k, s, tmp, "ix")
        self.gix = api.Index.load(prefix, 0)
        self.mp = api.Mapper(self.gix, max_reads, max_len)

    def close(self):
        self.mp.close()
        self.gix.close()
        ol.lib().or_index_free(self.oix)


@pytest.fixture
def rig(request, oracle_built, tmp_path):
    k, s = request.param
    r = Rig(si.reference()[0], k, s, tmp_path)
    yield r
    r.close()


IDS = ["k%ds%d" % ks for ks in si.SWEEP]


@pytest.mark.parametrize("rig", si.SWEEP, ids=IDS, indirect=True)
def test_seed_sweep(rig):
    """every parameter set on the sweep reads; the default set again from HBM slots (the wave form on global memory) and with
    another guard byte; the stretches of split-read calls; the totals against Mapper.hit_totals"""
    reads, quals = si.sweep_reads(rig.k, rig.s)
    for name, (par, totals) in si.param_sets().items():
        exp = sr.ref_batch(rig.oix, reads, quals, par, totals_only=totals)
        got = rig.mp.seed_batch(reads, quals, par.gpu(rig.gix), totals_only=totals)
        assert got["in_lds"]
        sr.check_against(got, exp, reads, name)
        if name == "default":
            sr.check_against(rig.mp.seed_batch(reads, quals, par.gpu(rig.gix), scratch_home=1), exp, reads, "default, HBM slots")
            sr.check_against(rig.mp.seed_batch(reads, quals, par.gpu(rig.gix), guard=0x3C), exp, reads, "default, guard 0x3C")
            sr.check_against(rig.mp.seed_batch(reads, None, par.gpu(rig.gix)), sr.ref_batch(rig.oix, reads, None, par), reads, "default, no qualities")
        if totals:
            tot = rig.mp.hit_totals(reads, quals, par.gpu(rig.gix))
            assert tot == [(int(exp[2 * i].hdr[6]) + int(exp[2 * i + 1].hdr[6])) & 0xFFFFFFFF for i in range(len(reads))], name
    par = sr.Par(noshort=True)
    rng = si.stretches(reads, rig.k)
    exp = sr.ref_batch(rig.oix, reads, quals, par, ranges=rng)
    sr.check_against(rig.mp.seed_batch(reads, quals, par.gpu(rig.gix), seed_range=rng), exp, reads, "stretches")
    sr.check_against(rig.mp.seed_batch(reads, quals, par.gpu(rig.gix), seed_range=rng, scratch_home=1, grid=2), exp, reads, "stretches, HBM slots, 2 workgroups")


@pytest.mark.parametrize("rig", [(20, 17), (13, 6), (9, 1)], ids=["k20s17", "k13s6", "k9s1"], indirect=True)
def test_seed_scratch_reuse_and_homes(rig, tmp_path):
    """the mixed batch (600-base reads between short ones and reads without a hit) with 1, 3 and the launcher's number of
    workgroups, the scratch in LDS and in HBM slots, and on a mapper of 2000-base reads whose launcher takes HBM itself: all
    equal to the reference.  One workgroup meets all strands in turn: what a longer strand left in the scratch lies behind
    every shorter one."""
    from smalt_amd import api
    reads, quals = si.mixed_batch(rig.k)
    par = sr.Par()
    exp = sr.ref_batch(rig.oix, reads, quals, par)
    for home in (0, 1):
        for grid in (0, 1, 3):
            got = rig.mp.seed_batch(reads, quals, par.gpu(rig.gix), scratch_home=home, grid=grid)
            assert got["in_lds"] == (home == 0) and got["grid"] == (grid or 2 * len(reads))
            sr.check_against(got, exp, reads, "home %d grid %d" % (home, grid))
    big = api.Mapper(rig.gix, 128, 2000)
    try:
        for home, grid in ((0, 0), (0, 1), (1, 3)):
            got = big.seed_batch(reads, quals, par.gpu(rig.gix), scratch_home=home, grid=grid)
            assert not got["in_lds"] and got["stride"] >= 2008
            sr.check_against(got, exp, reads, "max_read_len 2000, home %d grid %d" % (home, grid))
    finally:
        big.close()


def test_seed_totals_equal_the_oracles_mapping_call(oracle_built, tmp_path):
    """calcTotalNumberOfHits of the oracle's own mapping call (or_map_hit_total) on a few reads, against the totals_only headers"""
    r = Rig(si.reference()[0], 13, 6, tmp_path)
    try:
        reads, quals = si.sweep_reads(13, 6)
        pick = [i for i in range(0, len(reads), 9) if len(reads[i]) <= 160][:24]
        reads, quals = [reads[i] for i in pick], [quals[i] for i in pick]
        for ncut in (10000, 50, 1):
            par = sr.Par(ncut=ncut)
            got = r.mp.seed_batch(reads, quals, par.gpu(r.gix), totals_only=True)
            om, opar = ol.Mapper(r.oix), ol.default_params(r.oix)
            opar.ncut = ncut
            for i, (rd, q) in enumerate(zip(reads, quals)):
                rv, _ = om.map(rd, q, opar)
                assert rv == 0
                assert om.hit_total(ncut) == (int(got["hi"][2 * i][6]) + int(got["hi"][2 * i + 1][6])) & 0xFFFFFFFF, (ncut, i)
            om.close()
    finally:
        r.close()


def test_seed_packed_element_limit(oracle_built, tmp_path):
    """maxkey 0xFFFFF runs the wave form, 2^20 the one-lane form (test_seed_ref.py asserts the forms); both equal the reference"""
    seqs, reads = si.packed_limit()
    r = Rig(seqs, si.PACKED_K, si.PACKED_S, tmp_path, max_reads=8, max_len=128)
    try:
        par = sr.Par(ncut=si.PACKED_NCUT)
        exp = sr.ref_batch(r.oix, reads, None, par)
        assert int(exp[0].seeds[:, 1].max()) == 0xFFFFF and int(exp[2].seeds[:, 1].max()) == 1 << 20
        for home, grid in ((0, 0), (0, 1), (1, 1)):
            sr.check_against(r.mp.seed_batch(reads, None, par.gpu(r.gix), scratch_home=home, grid=grid), exp, reads, "home %d grid %d" % (home, grid))
    finally:
        r.close()


def test_seed_batch_refusals(oracle_built, tmp_path):
    from smalt_amd import api
    r = Rig(si.reference()[0], 13, 6, tmp_path, max_reads=8, max_len=100)
    try:
        p = r.gix.default_params()
        reads = [b"ACGTTGCATGCATGGCATGCAAAC" * 3] * 2
        with pytest.raises(api.SmaltGpuError) as e:
            r.mp.seed_batch(reads, None, p, seed_range=[(0, 30), (0, 30)], totals_only=True)
        assert e.value.code == EARG
        with pytest.raises(api.SmaltGpuError) as e:
            r.mp.seed_batch(reads, None, p, scratch_home=1, grid=8193)
        assert e.value.code == EARG
        with pytest.raises(api.SmaltGpuError) as e:
            r.mp.seed_batch([b"A" * 101], None, p)
        assert e.value.code == EARG
        with pytest.raises(api.SmaltGpuError) as e:
            r.mp.seed_batch(reads * 4, None, p)               # no room for the guard row behind the last strand
        assert e.value.code == EARG
        got = r.mp.seed_batch(reads, None, p, grid=8193)      # in LDS any grid will do
        sr.check_against(got, sr.ref_batch(r.oix, reads, None, sr.Par()), reads, "after the refusals")
    finally:
        r.close()

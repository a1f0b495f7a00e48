"""S3 on its own (kernel k_hits, smaltgpu_hits_batch) and the 64-bit wave sorts (smaltgpu_sort_u64_batch) against plain
references: tests/hits_ref.py for the hit runs (exact integer equality, key by key), np.sort for the sorts (in LDS up to 1024 keys,
and the two sorts of the HBM working set in place on global memory up to 65 536 keys).  Every case first
asserts, from the reference alone, that the batch holds the strands the case is about -- and that no eligible strand was left
to the candidate stage (HITRUN_NONE), which end-to-end parity cannot see: k_cands would quietly gather that strand again."""
import functools

import numpy as np
import pytest

import hits_ref as hr
import oracle_lib as ol

pytestmark = pytest.mark.gpu

NCHR, CHRLEN, CONS = 3, 300_000, 300
REF_SEED = 81


@functools.lru_cache(maxsize=None)
def _reference():
    """3 sequences of 300 kbp, three tenths of them copies of one 300-base family (1 % divergence: 900 copies) -> the
    sequences and the family's consensus"""
    from smalt_amd import synth
    ch, fams = synth.make_reference(NCHR, CHRLEN, seed=REF_SEED, repeat_frac=0.3, n_fam=1, cons_len=CONS, divergence=0.01, return_families=True)
    assert fams.shape == (1, CONS)
    return ch, fams[0]


@functools.lru_cache(maxsize=None)
def workload():
    """The reference of _reference(); 400 reads of 100 bases: 200 from anywhere, 200 cut from the repeat family with 0 to 24 %
    substitutions, so that the strands' key counts spread from a few to 16 thousand (one window, several windows, the ceiling
    of the hit list)."""
    from smalt_amd import synth
    ch, cons = _reference()
    seqs = [synth.codes_to_ascii(c) for c in ch]
    reads, _ = synth.make_reads(ch, 200, 100, seed=REF_SEED + 1, sub_rate=0.01, indel_read_frac=0.05)
    rng = np.random.default_rng(REF_SEED + 2)
    for i in range(200):
        o = int(rng.integers(0, CONS - 100))
        r = cons[o:o + 100].copy()
        mut = rng.random(100) < 0.24 * ((i % 25) / 24.0) ** 1.5
        r = np.where(mut, (r + rng.integers(1, 4, size=100)) & 3, r).astype(np.uint8)
        reads.append(synth.revcomp_codes(r) if i % 2 else r)
    return seqs, [synth.codes_to_ascii(r) for r in reads]


class Ctx:
    pass


@pytest.fixture(scope="module", params=[(13, 6), (11, 3)], ids=["k13s6", "k11s3"])
def ctx(request, oracle_built, tmp_path_factory):
    """Index (written by the oracle, loaded by the library), its arrays on the host and a mapper of 100-base reads whose pool
    (6144 keys per read of its capacity) holds the 2.5 million keys of the batch at k=11 s=3; a second mapper in which S3
    can be switched off, for the qualifiers as the seeding stage leaves them."""
    from smalt_amd import api
    k, s = request.param
    seqs, rb = workload()
    c = Ctx()
    oix0 = ol.build_index(seqs, ["c%d" % i for i in range(NCHR)], k, s)
    c.pre = str(tmp_path_factory.mktemp("hits") / ("ix%d_%d" % (k, s)))
    assert ol.lib().or_index_write(oix0, c.pre.encode()) == 0
    ol.lib().or_index_free(oix0)
    c.oix = ol.lib().or_index_read(c.pre.encode())
    c.hx = hr.HostIndex(c.oix)
    c.k, c.s, c.seqs, c.rb = k, s, seqs, rb
    c.lens = [len(r) for r in rb]
    c.gix = api.Index.load(c.pre, 0)
    c.mp = api.Mapper(c.gix, 600, 100)
    c.mp_off = api.Mapper(c.gix, 600, 150)                  # per-list tables of 168 entries: a window of 256 keys switches S3 off
    yield c
    c.mp_off.close()
    c.mp.close()
    c.gix.close()


def _params(gix, name):
    p = gix.default_params()                         # 3 sequences: sequence by sequence (smalt.c:599)
    assert p.rmapflg & hr.FLG_SEQBYSEQ
    if name.startswith("concat"):
        p.rmapflg &= ~hr.FLG_SEQBYSEQ
    if name.endswith("ncut50"):
        p.ktuple_maxhit = 50
    if "-x-" in name:                                # smalt map -x: the seeding stage keeps the seeds above the cut-off in the table
        from smalt_amd import api
        p.rmapflg |= api.FLG_NOSHRTINFO | api.FLG_SENSITIVE
    return p


def _run(c, par, window=0, pool_keys=0, reads=None, mp=None):
    rb = c.rb if reads is None else reads
    got = (mp or c.mp).hits_batch(rb, [b"I" * len(r) for r in rb], par, window=window, pool_keys=pool_keys)
    exp = hr.expect_batch(c.hx, par, [len(r) for r in rb], got)
    return got, exp


def _check(c, par, exp, got, reads=None, mp_off=None, overflow=False):
    """hits_ref.check_batch with the qualifiers of the seeding stage: the same reads and parameters through a mapper and a
    window with which S3 does not take place (W <= tab + 128), so that k_hits returns before it marks anything."""
    rb = c.rb if reads is None else reads
    off = (mp_off or c.mp_off).hits_batch(rb, [b"I" * len(r) for r in rb], par, window=256)
    assert off["window"] <= off["tab"] + 128 and (off["run_mode"] == hr.HITRUN_NONE).all() and off["hit_count"] == 0
    assert np.array_equal(off["n_seeds"], got["n_seeds"]) and np.array_equal(off["seed_rank"], got["seed_rank"])
    return hr.check_batch(exp, got, (par.rmapflg & hr.FLG_SEQBYSEQ) != 0, off["qmask"], [len(r) for r in rb], overflow=overflow)


def _no_eligible_strand_left(exp, got):
    left = [rs for rs, e in enumerate(exp) if e.eligible and not e.over_alloc and int(got["run_mode"][rs]) == hr.HITRUN_NONE]
    assert left == [], "eligible strands the kernel left to the candidate stage: %r" % left[:10]


@pytest.mark.parametrize("window", [0, 256], ids=["w-default", "w256"])
@pytest.mark.parametrize("pname", ["seqbyseq", "seqbyseq-ncut50", "concat", "concat-ncut50", "seqbyseq-x-ncut50", "concat-x-ncut50"])
def test_hit_runs_equal_reference(ctx, pname, window):
    """Every strand of the batch: mode, run length, keys, disjoint runs, pool cursor, qualifiers.  At least 20 strands gather in
    one window; with the default cut-off at least 20 in several windows (up to 16 windows of 1024 keys), and at k=11 s=3 in one
    hit list over all sequences at least 20 strands pass the list's ceiling and go through the halving loop.  With the cut-off
    at 50 a plain call's seeding stage leaves the repeat's seeds out of the table itself (short runs only, nothing for the stage
    to cut: these two cases claim the one-window path alone); with -x it keeps them, and the stage leaves them out: sequence by
    sequence at least 20 strands mark read offsets HQ_MULTIHIT, in one list at least 20 strands have seeds above the cut-off."""
    par = _params(ctx.gix, pname)
    got, exp = _run(ctx, par, window)
    W = got["window"]
    assert W == (window or 1024) and got["tab"] == 120 and W > got["tab"] + 128
    tot = [e.keys.size for e in exp if e.mode == hr.HITRUN_SORTED]
    paths = dict(one_window=sum(1 for t in tot if 0 < t <= W), windows=sum(1 for t in tot if t > W), cut=sum(1 for e in exp if e.ncutseeds),
                 marking=sum(1 for e in exp if e.mode == hr.HITRUN_SORTED and e.multihit),
                 halved=sum(1 for e in exp if e.halved), ceiling=sum(1 for e in exp if e.stopped), over_alloc=sum(1 for e in exp if e.over_alloc),
                 empty=sum(1 for t in tot if t == 0), largest=max(tot), total=sum(tot))
    print(pname, W, paths)
    assert paths["one_window"] >= 20
    if not pname.endswith("ncut50"):
        assert paths["windows"] >= 20 and paths["largest"] > 8 * W
    if pname == "seqbyseq-x-ncut50":
        assert paths["marking"] >= 20 and paths["cut"] >= 20
    elif pname == "concat-x-ncut50":
        assert paths["cut"] >= 20 and paths["marking"] == 0
    elif pname.endswith("ncut50"):
        assert paths["cut"] == 0 and paths["marking"] == 0       # the seeding stage has left them out already
    if pname == "concat" and ctx.k == 11:
        assert paths["halved"] >= 20 and paths["cut"] >= 20
    _no_eligible_strand_left(exp, got)
    _check(ctx, par, exp, got)


def test_reference_counts_agree_with_oracle(ctx):
    """Guard on the reference itself: the oracle's per-read hit number (or_map_stats, calcTotalHitNumStats, rmap.c:1086) counts the
    hits of the seeds below the rank BEFORE the cut-off; for every read whose strands leave no seed out it equals the sum of
    the two expected run lengths."""
    par = ctx.gix.default_params()
    got, exp = _run(ctx, par)
    m = ol.Mapper(ctx.oix)
    opar = ol.default_params(ctx.oix)
    nchecked = 0
    for i in range(len(ctx.rb)):
        e0, e1 = exp[2 * i], exp[2 * i + 1]
        if e0.mode != hr.HITRUN_SORTED or e1.mode != hr.HITRUN_SORTED or e0.ncutseeds or e1.ncutseeds:
            continue
        rv, _ = m.map(ctx.rb[i], b"I" * len(ctx.rb[i]), opar)
        assert rv == 0
        assert e0.keys.size + e1.keys.size == m.stats()[4], i
        nchecked += 1
    m.close()
    assert nchecked >= 300


def test_window_boundary_between_the_two_paths(ctx):
    """Three strands of 256 < total <= 1023 keys, each alone in a batch, at windows of total (one window: total <= W), total - 1
    and total + 1 keys."""
    par = _params(ctx.gix, "concat")
    _, exp = _run(ctx, par)
    picks = [rs for rs, e in enumerate(exp) if e.mode == hr.HITRUN_SORTED and 257 < e.keys.size <= 1023][:3]
    assert len(picks) == 3
    for rs in picks:
        total = exp[rs].keys.size
        for w in (total, total - 1, total + 1):
            rb = [ctx.rb[rs >> 1]]
            got, e1 = _run(ctx, par, window=w, reads=rb)
            assert got["window"] == w and e1[rs & 1].keys.size == total
            assert (total <= w) == (w != total - 1)              # which of the two paths the strand takes
            _no_eligible_strand_left(e1, got)
            _check(ctx, par, e1, got, reads=rb)


# k -> (strand of the workload, keys per window) with which the strand's last window holds a single key (found with
# hits_ref.window_counts over the strands of up to 4000 keys and every window; asserted from the reference below)
ONE_KEY_LAST_WINDOW = {13: (683, 374), 11: (488, 607)}


@pytest.mark.parametrize("pname", ["seqbyseq", "concat"])
def test_last_window_of_a_single_key(ctx, pname):
    """The windows take what lies below their bound, so a last window of one key is an accident of the data: a strand and a
    window for which the reference's walk over the windows ends on one (three windows; the last sort is of a single key and the
    run's last key is written alone)."""
    par = _params(ctx.gix, pname)
    rs, w = ONE_KEY_LAST_WINDOW[ctx.k]
    rb = [ctx.rb[rs >> 1]]
    got, exp = _run(ctx, par, window=w, reads=rb)
    e = exp[rs & 1]
    assert got["window"] == w and e.mode == hr.HITRUN_SORTED and e.keys.size > w
    counts = hr.window_counts(e, w)
    assert len(counts) == 3 and counts[-1] == 1 and sum(counts) == e.keys.size
    _no_eligible_strand_left(exp, got)
    _check(ctx, par, exp, got, reads=rb)


def _probe_read(j):
    """Read j of a family of 100-base reads cut from the repeat with 6 to 22 % substitutions: their forward strands hold from a
    few dozen to a few thousand keys, densely enough that some land on a given count."""
    from smalt_amd import synth
    rng = np.random.default_rng(1000 + j)
    o = int(rng.integers(0, CONS - 100))
    r = _reference()[1][o:o + 100].copy()
    mut = rng.random(100) < 0.06 + 0.16 * rng.random()
    return synth.codes_to_ascii(np.where(mut, (r + rng.integers(1, 4, size=100)) & 3, r).astype(np.uint8))


# key count of the forward strand -> probe read (found by running the one-lane host build over probes 0..11999; k=13 s=6 has no
# strand of exactly 513 keys among them: there a window of the workload's strand 4 lands on the count)
SORT_SWITCH_PROBES = {13: {256: 347, 257: 4628, 512: 1270}, 11: {256: 549, 257: 3823, 512: 2853, 513: 973}}
WINDOW_OF_513 = {13: (4, 743)}                    # k -> (strand of the workload, keys per window)


def test_sort_instance_switches(ctx):
    """Strands of exactly 256 / 257 and 512 / 513 keys gathered in one window: the last run of the 4-keys-per-lane sort and the
    first of the 8-keys-per-lane one, likewise 8 and 16.  Where no strand has 513 keys, a strand in several windows with a
    window of 513 keys (the reference's walk over the windows says which).  The counts are asserted from the reference before
    the comparison."""
    par = ctx.gix.default_params()
    probes = SORT_SWITCH_PROBES[ctx.k]
    rb = [_probe_read(j) for j in probes.values()]
    got, exp = _run(ctx, par, reads=rb)
    assert [exp[2 * i].keys.size for i in range(len(rb))] == list(probes)
    assert got["window"] == 1024
    _no_eligible_strand_left(exp, got)
    _check(ctx, par, exp, got, reads=rb)
    if 513 not in probes:
        rs, w = WINDOW_OF_513[ctx.k]
        rb = [ctx.rb[rs >> 1]]
        got, exp = _run(ctx, par, window=w, reads=rb)
        assert got["window"] == w and exp[rs & 1].mode == hr.HITRUN_SORTED and 513 in hr.window_counts(exp[rs & 1], w)
        _no_eligible_strand_left(exp, got)
        _check(ctx, par, exp, got, reads=rb)


def test_short_and_longest_reads(ctx):
    """Reads of k - 1, k, 20 and the mapper's longest length.  A mapper takes S3 ahead of the candidate stage up to
    max_read_len = 248 (stride 256); 240 is the longest for which the split candidate kernel consumes the runs, at 248 the
    per-list tables have their full 264 entries."""
    from smalt_amd import api
    par = ctx.gix.default_params()
    for maxlen in (240, 248):
        src = ctx.seqs[1]
        rb = [src[5000:5000 + ctx.k - 1], src[6000:6000 + ctx.k], src[7000:7020], src[8000:8000 + maxlen], ctx.rb[200] + ctx.rb[202] + ctx.rb[204][:maxlen - 200]]
        mp = api.Mapper(ctx.gix, 8, maxlen)
        try:
            got, exp = _run(ctx, par, reads=rb, mp=mp)
            assert got["tab"] == min(264, ((maxlen + 15) & ~7) + 8)
            assert [e.eligible for e in exp] == [False, False] + [True] * 8
            assert exp[6].keys.size > 0 or exp[7].keys.size > 0
            assert max(exp[8].keys.size, exp[9].keys.size) > 1024
            _no_eligible_strand_left(exp, got)
            _check(ctx, par, exp, got, reads=rb, mp_off=mp)          # (tables of 264 entries: no S3 at a window of 256 keys)
        finally:
            mp.close()


def test_window_not_above_the_tables_switches_the_stage_off(ctx):
    """max_read_len = 150: per-list tables of 168 entries, so a window of 256 keys is not above tab + 128 -- every strand stays
    with the candidate stage and nothing is reserved or written."""
    from smalt_amd import api
    par = ctx.gix.default_params()
    mp = api.Mapper(ctx.gix, 600, 150)                       # (the pool of 600 reads holds the batch's keys)
    try:
        got, exp = _run(ctx, par, window=256, mp=mp)
        assert got["tab"] == 168 and got["window"] == 256
        assert not any(e.eligible for e in exp)
        assert (got["run_mode"] == hr.HITRUN_NONE).all() and (got["run_n"] == 0).all() and got["hit_count"] == 0 and got["pool"].size == 0
        got, exp = _run(ctx, par, window=300, mp=mp)             # the same mapper with a window above the tables
        assert sum(1 for e in exp if e.mode == hr.HITRUN_SORTED and e.keys.size > 300) >= 20
        _no_eligible_strand_left(exp, got)
        _check(ctx, par, exp, got)
    finally:
        mp.close()


@pytest.mark.parametrize("maxlen", [256, 255, 249])
def test_mapper_without_the_split_is_refused(ctx, maxlen):
    from smalt_amd import api
    mp = api.Mapper(ctx.gix, 8, maxlen)
    try:
        with pytest.raises(api.SmaltGpuError):
            mp.hits_batch([ctx.rb[0]], None, ctx.gix.default_params())
    finally:
        mp.close()


def test_batch_and_pool_above_the_capacity_are_refused(ctx):
    from smalt_amd import api
    par = ctx.gix.default_params()
    mp = api.Mapper(ctx.gix, 8, 100)
    try:
        with pytest.raises(api.SmaltGpuError):
            mp.hits_batch(ctx.rb[:9], None, par)
        with pytest.raises(api.SmaltGpuError):
            mp.hits_batch(ctx.rb[:2], None, par, pool_keys=(1 << 20) + 1)       # the pool's floor is what a mapper of 8 reads allocates
        got = mp.hits_batch(ctx.rb[:2], None, par, pool_keys=1 << 20)
        assert got["pool_cap"] == 1 << 20
    finally:
        mp.close()


def test_full_pool_marks_strands_overflowed(ctx):
    """A pool of half the batch's keys: strands that reserve beyond it come out HITRUN_OVERFLOW (off + n > cap) and write
    nothing, every other strand is exact and inside the pool, the cursor counts all reservations.  Which strands overflow
    depends on the order of the reservations."""
    par = ctx.gix.default_params()
    _, exp = _run(ctx, par)
    total = sum(e.keys.size for e in exp)
    assert total > 100_000
    got, exp = _run(ctx, par, pool_keys=total // 2)
    assert got["pool_cap"] == total // 2 and got["hit_count"] == total
    novf = _check(ctx, par, exp, got, overflow=True)
    assert novf >= 1
    got, exp = _run(ctx, par)                                  # the mapper's own capacity again on the next call
    _check(ctx, par, exp, got)


@pytest.fixture(scope="module")
def sort_mapper():
    """The sorts take a mapper for its device and stream only: any small index will do."""
    from smalt_amd import api, synth
    ch = synth.make_reference(1, 20_000, seed=5, repeat_frac=0.0)
    gix = api.Index.build([synth.codes_to_ascii(c) for c in ch], ["c0"], 13, 6, 0)
    mp = api.Mapper(gix, 8, 100)
    yield mp
    mp.close()
    gix.close()


SORT_LENGTHS = {0: [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256], 1: [257, 511, 512], 2: [513, 1023, 1024]}
SORT_MAX = {0: 256, 1: 512, 2: 1024, 3: 1024}


def _sort_arrays(n, rng):
    """The contents of the issue for one length: random, all equal, ascending, descending, high word only, low word only, with
    0 and ~0 (the register forms pad with ~0)."""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    rnd = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    asc = np.sort(rnd)
    hi = (rng.integers(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32)) | np.uint64(0x9E3779B9)
    lo = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) | (np.uint64(0x12345678) << np.uint64(32))
    ext = rnd.copy()
    ext[::3] = full
    ext[1::3] = 0
    few = rng.integers(0, 4, size=n, dtype=np.uint64) * np.uint64(0x0000000100000001)      # many equal keys
    return [rnd, np.full(n, 0xDEADBEEF12345678, dtype=np.uint64), asc, asc[::-1].copy(), hi, lo, ext, np.full(n, full, dtype=np.uint64),
            np.zeros(n, dtype=np.uint64), few]


@pytest.mark.parametrize("form", [0, 1, 2, 3], ids=["reg4", "reg8", "reg16", "lds"])
def test_wave_sorts_equal_numpy(sort_mapper, form):
    """Every length a form admits (0..3, around 64, 128 and 256; then 257..512; then 513..1024), ten contents each, one wave
    per array, all arrays of a form in one launch."""
    rng = np.random.default_rng(91 + form)
    lengths = [n for f in sorted(SORT_LENGTHS) for n in SORT_LENGTHS[f] if n <= SORT_MAX[form]]
    assert lengths[-1] == SORT_MAX[form]
    arrays = [a for n in lengths for a in _sort_arrays(n, rng)]
    out = sort_mapper.sort_u64_batch(arrays, form)
    assert len(out) == len(arrays)
    for t, (a, o) in enumerate(zip(arrays, out)):
        assert np.array_equal(o, np.sort(a)), (form, len(a), t % 10)


def test_sort_refuses_an_array_above_the_form(sort_mapper):
    from smalt_amd import api
    for form, n in ((0, 257), (1, 513), (2, 1025), (3, 1025), (4, 65537), (5, 65537), (6, 1), (-1, 1)):
        with pytest.raises(api.SmaltGpuError):
            sort_mapper.sort_u64_batch([np.zeros(n, dtype=np.uint64)], form)


# The sorts of the HBM working set, in place on global memory (forms 4 and 5: wave_sort_u64, wave_sort_u64_chunked).  Lengths
# around the wave, the 256-key threshold and every chunk count at which the chunked sort changes shape: n - 1 keys leave the last
# chunk partial (and, at 2^m + 1024 c - 1, the mirror step with partners beyond n), n + 1 adds a chunk of one key and at a power
# of two doubles the padded size; above 2048 keys the half-cleaners that span chunks (j >= 1024) run, at 3072 and 12288 the
# padded size is not the array's.
HBM_SORT_LENGTHS = ([0, 1, 2, 63, 64, 65, 255, 256, 257] + [n + d for n in (1024, 2048, 3072, 4096, 8192, 12288, 16384, 32768) for d in (-1, 0, 1)]
                    + [1500, 5000, 40000, 65535, 65536])
# form -> lengths: the network in memory pays a round trip per stage, so it takes the lengths up to 16385 and one full array
HBM_SORT_FORMS = {4: [n for n in HBM_SORT_LENGTHS if n <= 16385] + [65536], 5: HBM_SORT_LENGTHS}
HBM_SORT_PATTERNS = ["rnd63", "rnd64", "8values", "sorted", "reversed", "organpipe", "constant", "chunks-sorted"]


def _hbm_sort_array(pattern, n, rng):
    if pattern == "rnd63":
        return rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    if pattern == "rnd64":                                    # up to 2^64 - 2: the register forms pad with ~0
        return rng.integers(0, 0xFFFFFFFFFFFFFFFF, size=n, dtype=np.uint64)
    if pattern == "8values":
        return rng.integers(0, 1 << 63, size=8, dtype=np.uint64)[rng.integers(0, 8, size=n)]
    if pattern == "constant":
        return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    a = np.sort(rng.integers(0, 1 << 63, size=n, dtype=np.uint64))
    if pattern == "reversed":
        return a[::-1].copy()
    if pattern == "organpipe":
        return np.concatenate([a[::2], a[1::2][::-1]])
    if pattern == "chunks-sorted":                            # every chunk of 1024 keys in order on its own
        a = rng.permutation(a)
        return np.concatenate([np.sort(a[o:o + 1024]) for o in range(0, n, 1024)] or [a])
    assert pattern == "sorted"
    return a


@pytest.mark.parametrize("form", [4, 5], ids=["hbm", "chunked"])
def test_hbm_sorts_equal_numpy(sort_mapper, form):
    """Every length of the form's list in eight contents, one wave per array, all arrays in one launch; exact equality with
    np.sort, and the guard behind the last array (the wrapper's) comes back untouched."""
    from smalt_amd import api
    assert (api.SORT_HBM, api.SORT_CHUNKED) == (4, 5)
    rng = np.random.default_rng(95 + form)
    cases = [(p, n) for n in HBM_SORT_FORMS[form] for p in HBM_SORT_PATTERNS]
    arrays = [_hbm_sort_array(p, n, rng) for p, n in cases]
    assert all(a.size == n and a.dtype == np.uint64 for a, (_, n) in zip(arrays, cases))
    out = sort_mapper.sort_u64_batch(arrays, form)
    assert len(out) == len(arrays)
    for (p, n), a, o in zip(cases, arrays, out):
        assert np.array_equal(o, np.sort(a)), (form, p, n)


def test_hbm_sorts_on_runs_of_the_workload(ctx, sort_mapper):
    """Production-shaped input: what the candidate stage sorts is a concatenation of ascending position lists (one per seed).  The
    lists of the workload's strands (hits_ref, which takes them from the index), strand after strand, cut into arrays of every
    length of the forms' lists; both forms."""
    par = _params(ctx.gix, "seqbyseq")
    _, exp = _run(ctx, par)
    lists = [l for e in exp if e.mode == hr.HITRUN_SORTED for l in e.lists]
    assert all(l.size < 2 or bool((l[1:] > l[:-1]).all()) for l in lists)
    stream = np.concatenate(lists)
    assert stream.size > 100_000 and len(lists) > 1000
    for form, lengths in HBM_SORT_FORMS.items():
        arrays, at = [], 0
        for n in lengths:
            if at + n > stream.size:
                at = (at + n) % 997                       # start over, off the earlier cuts
            arrays.append(stream[at:at + n].copy())
            at += n
        assert [a.size for a in arrays] == lengths
        assert all(np.count_nonzero(a[1:] < a[:-1]) >= 4 for a in arrays if a.size > 4096)       # several lists each
        out = sort_mapper.sort_u64_batch(arrays, form)
        for a, o in zip(arrays, out):
            assert np.array_equal(o, np.sort(a)), (form, a.size)

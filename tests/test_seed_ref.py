"""The reference of the seeding stage (tests/seed_ref.py) and the inputs of its tests (tests/seed_inputs.py), without a GPU: the
code table, the flat view of the oracle's hit info against the committed dump of the reference program, how many strands of
the committed inputs take each branch of stage_seed (classify), and the count of listed ranges on the committed adversaries of
the seed sort."""
import json
import os
import re

import numpy as np

import golden_util as gu
import oracle_lib as ol
import seed_inputs as si
import seed_ref as sr


def test_code_table():
    """sequence.c:287-322: A C G T/U in either case are 0..3, every other byte is 5; the reverse complement keeps codes >= 4"""
    want = np.full(256, 5, dtype=np.uint8)
    for ch, c in ((b"Aa", 0), (b"Cc", 1), (b"Gg", 2), (b"TtUu", 3)):
        for x in ch:
            want[x] = c
    assert np.array_equal(sr.CODE, want)
    assert sr.encode(b"ACGTUacgtuNnRYKMSWBDHV.-*@ ").tolist() == [0, 1, 2, 3, 3, 0, 1, 2, 3, 3] + [5] * 17
    assert sr.revcomp(np.array([0, 1, 5, 2, 3, 3], dtype=np.uint8)).tolist() == [0, 0, 1, 5, 2, 3]
    assert int((sr.CODE != 5).sum()) == 10


def test_flat_view_equals_the_reference_programs_dump(oracle_built, tmp_path):
    """HI / QM / SD lines of the committed dump of g_k13s6_ties (the reference program's own output) against the flat view"""
    entry = next(e for e in gu.MANIFEST if e["tag"] == "g_k13s6_ties")
    assert entry["opts"] == ""
    fx = gu.unpack(entry, tmp_path)
    oix = ol.lib().or_index_read(fx["prefix"].encode())
    try:
        reads = gu.read_fastq(fx["fq"])
        exp = sr.ref_batch(oix, [s for _, s, _ in reads], [q for _, _, q in reads], sr.Par())
        lines, at, nsd = fx["expected"].splitlines(), -1, 0
        for ln in lines:
            m = re.match(r"READ (\d+) ", ln)
            if m:
                at = int(m.group(1))
                continue
            if ln[:3] not in ("HI ", "QM ", "SD "):
                continue
            e = exp[2 * at + (ln[3] == "R")]
            f = ln.split()
            if f[0] == "HI":
                assert [int(x.split("=")[1]) for x in f[2:5]] == [int(e.hdr[0]), int(e.hdr[1]), int(e.hdr[2])], ln
            elif f[0] == "QM":
                assert f[2] == "".join(chr(48 + c) for c in e.qmask[:e.qlen]), ln
            else:
                i = int(f[2])
                assert [int(f[3]), int(f[4]), int(f[5])] == [int(e.seeds[i][2]), int(e.seeds[i][1]), int(e.seeds[i][0])], ln
                nsd += 1
        assert at == len(reads) - 1 and nsd == sum(int(e.hdr[0]) for e in exp) and nsd > 1000
    finally:
        ol.lib().or_index_free(oix)


# least number of strands per branch over the committed inputs (tests/seed_inputs.py): 5 for every branch a sweep can reach
NEED = dict.fromkeys(sr.BRANCHES, 5)
NEED["form_lane_maxkey"] = 0        # built for one strand: test_packed_limit_reads_take_both_forms


def test_committed_inputs_reach_every_branch(oracle_built, tmp_path):
    """classify over the step sweep with five parameter sets, the stretches and the mixed batch: strands per branch, printed and held
    against NEED; both sides of `listed` (s <= 16) in the wave form; per hashed index words that the index does not hold behind an
    occupied key.  classify also replays the budget and cover loops and asserts seed_rank for every strand it sees."""
    seqs, _ = si.reference()
    tot, types = dict.fromkeys(sr.BRANCHES, 0), set()
    for k, s in si.SWEEP:
        oix, _ = si.build_index(seqs, k, s, tmp_path, "ix%d_%d" % (k, s))
        try:
            reads, quals = si.sweep_reads(k, s)
            assert len(reads) <= 310                      # "about 300"
            row, absent = dict.fromkeys(sr.BRANCHES, 0), 0
            sets = si.param_sets()
            for name in ("default", "q10", "H50", "x", "totals"):
                par, totals = sets[name]
                exp = sr.ref_batch(oix, reads, quals, par, totals_only=totals)
                if name == "default":
                    absent = sum(sr.absent_behind_occupied_key(oix, e) for e in exp)
                for b, v in sr.tally(exp).items():
                    row[b] += v
            for b, v in sr.tally(sr.ref_batch(oix, reads, quals, sr.Par(noshort=True), ranges=si.stretches(reads, k))).items():
                row[b] += v
            m, mq = si.mixed_batch(k)
            for b, v in sr.tally(sr.ref_batch(oix, m, mq, sr.Par())).items():
                row[b] += v
            typ = int(oix.contents.typ)
            types.add(typ)
            print("k %d s %d %s, %d reads: %s; absent words behind an occupied key %d"
                  % (k, s, "hashed" if typ else "perfect", len(reads), " ".join("%s %d" % (b, row[b]) for b in sr.BRANCHES), absent))
            assert (row["listed"] >= 5 and row["unlisted"] == 0) if s <= 16 else (row["unlisted"] >= 5 and row["listed"] == 0)
            assert row["form_lane_qlen"] >= 5 and row["form_trivial"] >= 5 and row["short"] >= 5 and row["rep_cross"] >= 5
            assert absent >= 5 or typ == 0
            for b in tot:
                tot[b] += row[b]
        finally:
            ol.lib().or_index_free(oix)
    print("all: " + " ".join("%s %d" % (b, tot[b]) for b in sr.BRANCHES))
    assert types == {0, 1}
    assert all(tot[b] >= NEED[b] for b in sr.BRANCHES), {b: tot[b] for b in sr.BRANCHES if tot[b] < NEED[b]}


def test_packed_limit_reads_take_both_forms(oracle_built, tmp_path):
    """2^20 - 1 positions of the A word fit the packed sort element (wave form, maxkey 0xFFFFF); 2^20 of the C word do not"""
    seqs, reads = si.packed_limit()
    assert len(seqs[0]) < 2200000
    oix, _ = si.build_index(seqs, si.PACKED_K, si.PACKED_S, tmp_path, "px")
    try:
        assert int(oix.contents.typ) == 0
        exp = sr.ref_batch(oix, reads, None, sr.Par(ncut=si.PACKED_NCUT))
        a, c = sr.classify(exp[0]), sr.classify(exp[2])
        assert a["form"] == "wave" and a["maxkey"] == 0xFFFFF and a["budget_cut"] and a["listed"]
        assert c["form"] == "lane" and c["reason"] == "maxkey >= 2^20" and c["maxkey"] == 1 << 20
        assert sr.classify(exp[1])["form"] == "trivial" and sr.classify(exp[3])["form"] == "trivial"      # (the reverse strands find nothing)
    finally:
        ol.lib().or_index_free(oix)


def adversaries():
    with open(os.path.join(gu.GOLD, "seedsort_adversaries.json")) as f:
        return [(d["ranges"], np.array(d["keys"], dtype=np.uint32)) for d in json.load(f)["arrays"]]


def test_listed_ranges_on_the_adversaries(oracle_built):
    """at least three committed arrays of at most 255 keys flush the list of 32 ranges in the middle of the recursion, one fills
    it exactly; the plain arrays stay far below; the Python replay and the oracle's count agree"""
    f = ol.lib().or_sort_listed_ranges
    f.argtypes = [ol.C.c_int, ol.C.c_void_p]
    adv = adversaries()
    counts = []
    for want, keys in adv:
        assert keys.size <= 255
        n, flushes = sr.listed_ranges(keys)
        assert n == want and flushes == want // 32
        buf = keys.copy()
        assert f(buf.size, buf.ctypes.data) == n
        counts.append(n)
    print("listed ranges of the adversaries:", counts)
    assert sum(1 for c in counts if c > 32) >= 3 and 32 in counts
    rng = np.random.default_rng(3)
    s = np.sort(rng.integers(0, 1000, size=255, dtype=np.uint32))
    for a in (s, s[::-1].copy(), np.concatenate([s[::2], s[::-2]]), np.full(255, 7, np.uint32), rng.integers(0, 1000, size=255, dtype=np.uint32),
              rng.integers(0, 3, size=255, dtype=np.uint32), rng.permutation(4000).astype(np.uint32)):
        n, _ = sr.listed_ranges(a)
        buf = a.copy()
        assert f(buf.size, buf.ctypes.data) == n
        assert a.size > 255 or n < 32          # none of these would flush: why the adversaries are needed

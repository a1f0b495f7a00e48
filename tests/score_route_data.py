"""Workloads that send ordinary mapping calls down every route of the first-pass score stage (tests/score_route_ref.py restates the
routing; tests/test_score_route_cases.py holds each case's conditions against the oracle's candidates on the CPU,
tests/test_gpu_score_route.py checks what the stage left in the pool).  A case is a small synthetic reference with repeat families,
reads cut from it, and a mapper shape; all calls run without FLG_BEST, so that the oracle scores every ranked candidate and its
candidate list is the ranked list of the pool.

The two copies of S7's listing rule.  Every instance of k_cands compiles both: one is the tail ("S7") of stage_cands_v2 in smg_cands.hpp (the
wave-parallel form), the other the tail of stage_cands in smg_stages.hpp (the sequential form).  Which one a read runs is decided per
read at run time by cands_v2_applicable (smg_cands.hpp): the wave-parallel form whenever the call is sequence by sequence
(FLG_SEQBYSEQ, the default below 512 sequences), restricted to intervals, or has min_cover < k + s; the sequential form otherwise.
Every case below runs the first copy; `w248_seq` and `long_mapper_short_reads_seq` repeat two workloads with FLG_SEQBYSEQ cleared and
min_cover = k + s, which is the second copy (their windows lie in the concatenated set, sqidx = -1).

A window above wincap (4 * qmax + 1024) does come out of a mapping call (`wincap`): a read made of pieces of k + 1 bases that leave
out just under 3 k bases of the reference between them keeps all its seeds in one hit region (defineHitRegions, segment.c:396-453:
steps of less than 3 k / s between the diagonals), so in one candidate, whose band spans the whole drift of about 2.7 read lengths
and whose window is the read plus twice the drift.  No wave kernel takes such a window; k_sw_scalar scores it.  The case raises
min_swatscor above what the pieces can score, so that the traceback pass, for which such a window is a per-read capacity error, leaves
the candidate alone as the oracle does."""
import functools
import os
import tempfile

import numpy as np

import oracle_lib as ol
import score_route_ref as srr

COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(r):
    return r[::-1].translate(COMP)


def _mutate(rng, src, sub=0.0, ins=0.0, dele=0.0):
    out = bytearray()
    for ch in src:
        u = rng.random()
        if u < sub:
            out.append(b"ACGT"[int(rng.integers(0, 4))])
        elif u < sub + ins:
            out.append(ch)
            out.append(b"ACGT"[int(rng.integers(0, 4))])
        elif u < sub + ins + dele:
            continue
        else:
            out.append(ch)
    return bytes(out)


def _cut(rng, seqs, n, lengths, sub=0.01, ins=0.0, dele=0.0, exact_every=0):
    """n reads of the given lengths in turn, from uniform places, every other one reverse-complemented; the edits apply to a source
    that is long enough for the read to keep its length; exact_every: every such read is an exact copy"""
    rb = []
    for i in range(n):
        ln = lengths[i % len(lengths)]
        s = seqs[int(rng.integers(0, len(seqs)))]
        p = int(rng.integers(0, len(s) - 2 * ln - 8))
        if exact_every and i % exact_every == 0:
            r = s[p:p + ln]
        else:
            r = _mutate(rng, s[p:p + 2 * ln], sub, ins, dele)[:ln]
        rb.append(_revcomp(r) if i % 2 else r)
    return rb


def _family_reads(rng, fam, n, lengths, sub=0.01):
    """reads cut from the consensus of a repeat family: one candidate per copy in the reference"""
    from smalt_amd import synth
    cons = synth.codes_to_ascii(fam)
    rb = []
    for i in range(n):
        ln = lengths[i % len(lengths)]
        p = int(rng.integers(0, len(cons) - ln + 1))
        r = _mutate(rng, cons[p:p + ln + 8], sub)[:ln]
        rb.append(_revcomp(r) if i % 2 else r)
    return rb


def _with_n(rng, rb, every):
    out = []
    for i, r in enumerate(rb):
        if i % every == 0:
            a = bytearray(r)
            a[int(rng.integers(0, len(a)))] = ord("N")
            r = bytes(a)
        out.append(r)
    return out


class Case:
    """seqs: the reference; batches: lists of reads that go through ONE mapper in turn; mapper: (max_batch_reads, max_read_len,
    cands_per_read); par: attribute overrides of the default parameters; seq_form: the sequential form of the candidate stage;
    env: environment of the mapper's creation; need: the conditions, name -> function of the plans of the batches"""

    def __init__(self, name, k, s, seqs, batches, mapper, need, par=None, seq_form=False, env=None):
        self.name, self.k, self.s, self.seqs, self.batches, self.mapper, self.need = name, k, s, seqs, batches, mapper, need
        self.par, self.seq_form, self.env = dict(par or {}), seq_form, dict(env or {})

    def params(self, p):
        """the case's parameters on a default set of the oracle or of the library (same field meanings, different names)"""
        flags = "rmapflg" if hasattr(p, "rmapflg") else "flags"
        setattr(p, flags, getattr(p, flags) & ~ol.FLG_BEST)
        if self.seq_form:
            setattr(p, flags, getattr(p, flags) & ~ol.FLG_SEQBYSEQ)
            p.min_cover = self.k + self.s
        for name, v in self.par.items():
            setattr(p, name, v)
        return p


def _ref(nchr, chrlen, seed, **kw):
    from smalt_amd import synth
    ch, fams = synth.make_reference(nchr, chrlen, seed=seed, return_families=True, **kw)
    return [synth.codes_to_ascii(c) for c in ch], fams


def _count(pl, pred):
    return sum(1 for i in range(len(pl["kernel"])) if pred(pl, i))


def _k(name):
    return lambda pl, i: pl["kernel"][i] == name


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _w248(seq_form=False, env=None, name="w248"):
    seqs, _ = _ref(2, 200_000, 101, repeat_frac=0.1, n_fam=3, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(102)
    rb = _cut(rng, seqs, 240, W248_LENGTHS, sub=0.01)
    need = {
        "20 un-banded records with w <= 248": lambda pls: _count(pls[0], lambda p, i: not p["banded"][i] and p["w"][i] <= 248) >= 20,
        "20 un-banded records with w >= 249": lambda pls: _count(pls[0], lambda p, i: not p["banded"][i] and p["w"][i] >= 249) >= 20,
        "a record with w of 248 or 249": lambda pls: _count(pls[0], lambda p, i: not p["banded"][i] and p["w"][i] in (248, 249)) >= 1,
        "both packed instances score": lambda pls: _count(pls[0], _k("full16_short")) >= 20 and _count(pls[0], _k("full16_long")) >= 20,
        "work[17] counts the long ones": lambda pls: pls[0]["work"][17] >= 20 and pls[0]["work"][18] == 0,
    }
    return Case(name, 13, 6, seqs, [rb], (len(rb), 256, 0), need, seq_form=seq_form, env=env)


W248_LENGTHS = (200, 205, 210, 214, 218, 222, 226, 230, 235, 240, 245)


def _w1016():
    seqs, _ = _ref(2, 300_000, 111, repeat_frac=0.1, n_fam=3, cons_len=400, divergence=0.05)
    rng = np.random.default_rng(112)
    rb = _cut(rng, seqs, 60, (500, 504, 508, 512), sub=0.03, ins=0.05, dele=0.04, exact_every=7)
    # ... and reads that leave out 30 bases of the reference at 5 to 12 places: steps of less than 3 k bases between the diagonals keep
    # the pieces in one hit region (defineHitRegions, segment.c:396-453) and so in one candidate, whose band and window span the
    # whole drift of 150 to 360 bases
    for i in range(48):
        ln, ndel = (500, 504, 508, 512)[i % 4], 5 + i % 8
        piece = ln // (ndel + 1) + 1
        s0 = seqs[i % 2]
        p = int(rng.integers(0, len(s0) - 3 * ln))
        r = b"".join(s0[p + j * (piece + 30):p + j * (piece + 30) + piece] for j in range(ndel + 1))[:ln]
        assert len(r) == ln
        rb.append(_revcomp(r) if i % 2 else r)
    need = {
        "5 un-banded records with 248 < w <= 1016": lambda pls: _count(pls[0], lambda p, i: not p["banded"][i] and 248 < p["w"][i] <= 1016) >= 5,
        "5 un-banded records with w >= 1017": lambda pls: _count(pls[0], lambda p, i: not p["banded"][i] and p["w"][i] >= 1017) >= 5,
        "the wide ones reach the strip kernels although q <= tile_qmax": lambda pls: _count(pls[0], lambda p, i: p["kernel"][i] == "strip16" and p["q"][i] <= 512) >= 5,
        "both lists are in use": lambda pls: pls[0]["work"][17] >= 5 and pls[0]["work"][18] >= 5,
    }
    return Case("w1016", 13, 6, seqs, [rb], (len(rb), 512, 0), need)


def _q_tile(max_len, lengths, name):
    seqs, _ = _ref(2, 150_000, 121, repeat_frac=0.1, n_fam=3, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(122 + max_len)
    rb = _cut(rng, seqs, 20 * len(lengths), lengths, sub=0.02, ins=0.002, dele=0.002)
    need = {
        "a read of every length": lambda pls: all(any(q == ln for q in pls[0]["q"]) for ln in lengths),
        "the register kernels take every un-banded task": lambda pls: _count(pls[0], lambda p, i: not p["banded"][i] and p["kernel"][i] not in ("full16_short", "full16_long")) == 0
        and _count(pls[0], _k("full16_short")) + _count(pls[0], _k("full16_long")) >= 20 * len(lengths),
        "work[18] == 0": lambda pls: pls[0]["work"][18] == 0,
    }
    return Case(name, 13, 6, seqs, [rb], (len(rb), max_len, 0), need)


def _qn():
    seqs, _ = _ref(2, 150_000, 131, repeat_frac=0.1, n_fam=3, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(132)
    rb = _cut(rng, seqs, 150, (100, 180, 230), sub=0.02)
    with_n = _with_n(rng, rb, 5)
    need = {
        "the first batch has reads with N, the second none": lambda pls: pls[0]["work"][7] >= 30 and pls[1]["work"][7] == 0,
        "the 32-bit kernel scores exactly the candidates of reads with N": lambda pls: _count(pls[0], _k("full32_qn")) >= 30 and _count(pls[1], _k("full32_qn")) == 0,
        "reads with N have windows on both sides of 248": lambda pls: _count(pls[0], lambda p, i: p["kernel"][i] == "full32_qn" and p["w"][i] <= 248) >= 5
        and _count(pls[0], lambda p, i: p["kernel"][i] == "full32_qn" and p["w"][i] > 248) >= 5,
    }
    return Case("qn", 13, 6, seqs, [with_n, rb], (len(rb), 256, 0), need)


def _banded_255():
    # S7 leaves a candidate to K2b when 48 x its band width is at most the read length (smg_logic.hpp:553); the band of an exact copy
    # is 2 s + 2 diagonals wide, so reads of 250 bases need an index with s = 1
    seqs, _ = _ref(2, 150_000, 141, repeat_frac=0.1, n_fam=3, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(142)
    rb = _cut(rng, seqs, 110, tuple(range(250, 261)), sub=0.02, exact_every=2)
    need = {
        "banded records with q <= 255": lambda pls: _count(pls[0], lambda p, i: p["banded"][i] and p["q"][i] <= 255) >= 10,
        "banded records with q >= 256": lambda pls: _count(pls[0], lambda p, i: p["banded"][i] and p["q"][i] >= 256) >= 10,
        "banded records with q of 255 and of 256": lambda pls: all(_count(pls[0], lambda p, i: p["banded"][i] and p["q"][i] == ql) >= 1 for ql in (255, 256)),
        "the wave form of K2b exactly on the long side": lambda pls: _count(pls[0], lambda p, i: p["banded"][i] and (p["kernel"][i] == "band_wave") != (p["q"][i] >= 256)) == 0,
    }
    return Case("banded_255", 11, 1, seqs, [rb], (len(rb), 300, 0), need)


def _short_reads():
    seqs, _ = _ref(2, 100_000, 151, repeat_frac=0.1, n_fam=3, cons_len=200, divergence=0.05)
    rng = np.random.default_rng(152)
    rb = _cut(rng, seqs, 180, tuple(range(28, 37)), sub=0.01)
    need = {
        "below MINLEN_QUERY_STRIPED every candidate takes the one-lane banded pass": lambda pls: _count(pls[0], lambda p, i: p["q"][i] < 32) >= 20
        and _count(pls[0], lambda p, i: p["q"][i] < 32 and p["kernel"][i] != "scalar_band") == 0,
        "at and above it the packed kernel scores": lambda pls: all(_count(pls[0], lambda p, i: p["q"][i] == ql and p["kernel"][i] == "full16_short") >= 1 for ql in range(32, 37)),
    }
    return Case("short_reads", 11, 3, seqs, [rb], (len(rb), 64, 0), need)


def _long_mapper_short_reads(seq_form=False, env=None, name="long_mapper_short_reads"):
    seqs, _ = _ref(2, 150_000, 161, repeat_frac=0.1, n_fam=3, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(162)
    rb = _cut(rng, seqs, 200, tuple(range(40, 121, 8)), sub=0.02) + _cut(rng, seqs, 6, (520, 560, 600), sub=0.02)
    order = rng.permutation(len(rb))
    rb = [rb[int(i)] for i in order]
    need = {
        "every un-banded task is a strip task": lambda pls: pls[0]["work"][17] == 0 and _count(pls[0], lambda p, i: not p["banded"][i] and p["kernel"][i] != "strip16") == 0,
        "short and long reads share the strip list": lambda pls: _count(pls[0], lambda p, i: p["kernel"][i] == "strip16" and p["q"][i] <= 120) >= 100
        and _count(pls[0], lambda p, i: p["kernel"][i] == "strip16" and p["q"][i] >= 520) >= 6,
    }
    return Case(name, 13, 6, seqs, [rb], (len(rb), 600, 0), need, seq_form=seq_form, env=env)


def _long_list_overflow():
    seqs, fams = _ref(1, 150_000, 171, repeat_frac=OVF_COPIES * 300 / 150_000, n_fam=1, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(172)
    rb = _family_reads(rng, fams[0], 700, (228, 230, 232), sub=0.01)
    geo = srr.geometry(1000, 256, 8)
    need = {
        "work[17] > long_cap": lambda pls: pls[0]["work"][17] > geo["long_cap"],
        "the pool does not overflow": lambda pls: len(pls[0]["kernel"]) <= geo["rccap"],
        "three or more candidates per read": lambda pls: len(pls[0]["kernel"]) >= 3 * 700,
        "the large instance scores them all": lambda pls: _count(pls[0], _k("full16_long")) == pls[0]["work"][17],
    }
    return Case("long_list_overflow", 13, 6, seqs, [rb], (1000, 256, 8), need)


OVF_COPIES = 6


def _strip_list_overflow():
    # s = 2: the exact copies of 300 bases get bands of 6 diagonals, 48 x 6 <= 300 (see _banded_255)
    seqs, fams = _ref(1, 150_000, 181, repeat_frac=OVF_COPIES * 300 / 150_000, n_fam=1, cons_len=300, divergence=0.05)
    rng = np.random.default_rng(182)
    rb = _family_reads(rng, fams[0], 700, (60, 80, 100), sub=0.01)
    for j, p in enumerate(int(x) for x in rng.integers(0, 149_000, size=12)):      # spread over the batch: listed early and late
        rb.insert(59 * j, seqs[0][p:p + 300])
    geo = srr.geometry(1000, 600, 8)
    need = {
        "work[18] > strip_cap": lambda pls: pls[0]["work"][18] > geo["strip_cap"],
        "the pool does not overflow": lambda pls: len(pls[0]["kernel"]) <= geo["rccap"],
        "k_sw_strip scores the un-banded tasks by its scan": lambda pls: _count(pls[0], _k("strip32")) > geo["strip_cap"] - 100 and _count(pls[0], _k("strip16")) == 0,
        "banded long tasks go to the one-lane kernel": lambda pls: _count(pls[0], lambda p, i: p["banded"][i] and p["q"][i] > 255 and p["kernel"][i] == "scalar_band") >= 5
        and _count(pls[0], _k("band_wave")) == 0,
        "work[3] misses exactly the banded ones": lambda pls: pls[0]["work"][3] == len(pls[0]["kernel"]) - sum(pls[0]["banded"]),
    }
    return Case("strip_list_overflow", 11, 2, seqs, [rb], (1000, 600, 8), need)


def _exceed():
    seqs, _ = _ref(1, 40_000, 191, repeat_frac=0.0)
    # an exact copy (narrow band: K2b from the start), a read that leaves out 100 bases of the reference in its middle (a band wider than
    # q / 48, so K2a scores it: 4500 x 15 less one gap of 100 is above 65535) and the same with substitutions (K2a, below 65535)
    rng = np.random.default_rng(192)
    gapped = seqs[0][20_000:22_250] + seqs[0][22_350:24_600]
    rb = [seqs[0][3000:7400], _revcomp(gapped), _mutate(rng, seqs[0][30_000:32_250] + seqs[0][32_350:34_600], 0.05)]
    need = {
        "a K2a score >= 65535": lambda pls: _count(pls[0], lambda p, i: (p["flags"][i] & (srr.SCORED | srr.BANDED | srr.BSCORED)) == (srr.SCORED | srr.BANDED | srr.BSCORED)
                                              and not p["banded"][i] and p["kernel"][i] == "strip32") >= 1,
        "a K2a score below 65535 from the same kernel": lambda pls: _count(pls[0], lambda p, i: p["kernel"][i] == "strip32" and not p["flags"][i] & srr.BANDED) >= 1,
        "a candidate that S7 left to K2b": lambda pls: _count(pls[0], _k("band_wave")) >= 1,
    }
    return Case("exceed", 20, 13, seqs, [rb], (len(rb), 4500, 0), need, par={"match": 15})


def _wincap():
    seqs, _ = _ref(1, 120_000, 201, repeat_frac=0.0)
    rng = np.random.default_rng(202)
    rb = _cut(rng, seqs, 24, (100, 300, 600), sub=0.02)
    for i, (piece, gap) in enumerate(((21, 58), (21, 57), (22, 56), (22, 52), (23, 50), (24, 46), (25, 42), (26, 40))):
        p = 4000 + 9000 * i
        r = b"".join(seqs[0][p + j * (piece + gap):p + j * (piece + gap) + piece] for j in range(600 // piece + 1))[:600]
        rb.insert(3 * i, _revcomp(r) if i % 2 else r)
    wincap = srr.geometry(len(rb), 600, 0)["wincap"]
    need = {
        "windows above wincap": lambda pls: _count(pls[0], lambda p, i: p["w"][i] > wincap) >= 2,
        "windows of the same kind at and below wincap": lambda pls: _count(pls[0], lambda p, i: wincap - 800 <= p["w"][i] <= wincap) >= 2,
        "the one-lane kernel scores exactly the windows above wincap": lambda pls: _count(pls[0], lambda p, i: (p["kernel"][i] == "scalar_k2a") != (p["w"][i] > wincap)) == 0,
        "work[3] misses exactly those": lambda pls: pls[0]["work"][3] == len(pls[0]["kernel"]) - _count(pls[0], _k("scalar_k2a")),
    }
    return Case("wincap", 20, 1, seqs, [rb], (len(rb), 600, 0), need, par={"min_swatscor": 100})


def _builders():
    b = {
        "w248": _w248, "w1016": _w1016,
        "q_tile_152": lambda: _q_tile(152, (150, 151, 152), "q_tile_152"),
        "q_tile_160": lambda: _q_tile(160, tuple(range(153, 161)), "q_tile_160"),
        "qn": _qn, "banded_255": _banded_255, "short_reads": _short_reads, "long_mapper_short_reads": _long_mapper_short_reads,
        "long_list_overflow": _long_list_overflow, "strip_list_overflow": _strip_list_overflow, "exceed": _exceed, "wincap": _wincap,
        "w248_seq": lambda: _w248(seq_form=True, name="w248_seq"),
        "long_mapper_short_reads_seq": lambda: _long_mapper_short_reads(seq_form=True, name="long_mapper_short_reads_seq"),
    }
    for g in (1, 3):
        b["grids_full%d" % g] = (lambda g=g: _w248(env={"SMALTGPU_SWFULL_GRID": str(g)}, name="grids_full%d" % g))
        b["grids_strip%d" % g] = (lambda g=g: _long_mapper_short_reads(env={"SMALTGPU_STRIP_GRID": str(g)}, name="grids_strip%d" % g))
    return b


CASES = tuple(_builders())
# cases that repeat the workload of another one (their oracle work is shared)
SAME_WORKLOAD = {"grids_full1": "w248", "grids_full3": "w248", "grids_strip1": "long_mapper_short_reads", "grids_strip3": "long_mapper_short_reads"}


@functools.lru_cache(maxsize=None)
def case(name):
    return _builders()[name]()


class Expect:
    """What the oracle says about a case: per batch the candidates of all reads in read order (with rid, used_simd and the oracle's
    own swscor), per-read results and stats; the oracle's index (oix) and the index files' prefix stay for the GPU test."""


@functools.lru_cache(maxsize=None)
def expect(name):
    name = SAME_WORKLOAD.get(name, name)
    cs = case(name)
    e = Expect()
    e.tmp = tempfile.TemporaryDirectory()
    e.prefix = os.path.join(e.tmp.name, name)
    oix0 = ol.build_index(cs.seqs, ["c%d" % i for i in range(len(cs.seqs))], cs.k, cs.s)
    assert ol.lib().or_index_write(oix0, e.prefix.encode()) == 0
    e.oix = ol.lib().or_index_read(e.prefix.encode())
    e.par = cs.params(ol.default_params(e.oix))
    e.batches = []
    m = ol.Mapper(e.oix)
    for rb in cs.batches:
        cands, per_read, res, stats, rc_lines = [], [], [], [], []
        for rid, r in enumerate(rb):
            rv, rr = m.map(r, b"I" * len(r), e.par)
            assert rv == 0, (name, rid, rv)
            st = m.stats()
            res.append(rr)
            stats.append(dict(swmax=st[0], sw2nd=st[1], nseg=st[2], nseg_tot=st[3], nhit=st[4], nhit_tot=st[5]))
            cl = m.cands()
            for c in cl:
                c["rid"] = rid
            per_read.append(cl)
            cands += cl
            rc_lines.append([ln.split() for ln in m.dump(rid, "r%d" % rid).splitlines() if ln.startswith("RC ")])
        e.batches.append(dict(reads=rb, cands=cands, per_read=per_read, res=res, stats=stats, rc_lines=rc_lines,
                              qlens=[len(r) for r in rb], has_n=[any(ch not in b"ACGTacgtUu" for ch in r) for r in rb]))
    m.close()
    return e


def plans(name, geo=None, with_scores=True):
    """score_route_ref.plan over the oracle's candidates of every batch of the case; geo: the mapper's geometry (default: restated)"""
    cs, e = case(name), expect(name)
    geo = geo or srr.geometry(*cs.mapper)
    out = []
    for b in e.batches:
        sc = srr.Scorer(e.oix, b["reads"], e.par) if with_scores else None
        out.append(srr.plan(b["cands"], b["qlens"], b["has_n"], geo, e.par, sc))
    return out

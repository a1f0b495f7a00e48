"""Workloads of tests/test_gpu_resident.py and what the CPU oracle makes of them, computed once per process and shared by the
GPU tests and by the checks of the workloads' conditions in the same file, which run without a GPU.

single():   two sequences of 60 kbp with one 300-base repeat family, k = 11, s = 3, and 600 reads drawn as
            test_gpu_fuzz._make draws them: lengths 8 to 250 (some below k), both strands, substitutions and indels, one read in
            eight with an N, unrelated reads, base qualities with 8 % below 10.
overflow(): 300 reads of 100 bases on a reference that is 30 % copies of one repeat, k = 11, s = 3: more ranked candidates than
            a mapper with cands_per_read = 8 has room for.
Expectations are per read (alignments, the six scalars), by parameter set."""
import functools
import os
import tempfile

import numpy as np

import oracle_lib as ol

FLG_BEST = 0x02
K, S = 11, 3
NREADS = 600
# the parameter sets of the single-read tests: name -> (overrides, with qualities)
PARSETS = {
    "default": (dict(), False),
    "basq10": (dict(min_basq=10), True),                              # qualities change the seeding
    "all40": (dict(min_swatscor=40, below_max=12, best=False), False),
}
SUB_BATCHES = (97, 260, 1, 200)          # then the rest: sizes that go up and down
POOL_PER_READ = 8                        # cands_per_read of the overflow tests
POOL_FLOOR = 8000                        # MAXIMUM_DEPTH (smg_common.h): the candidate pool never holds fewer, so that one read alone fits


def _reads(seqs, n, lo, hi, seed):
    """the draws of test_gpu_fuzz._make, with low base qualities for every read"""
    rng = np.random.default_rng(seed)
    reads, quals, kinds = [], [], []
    for i in range(n):
        c = int(rng.integers(0, len(seqs))); ln = int(rng.integers(lo, hi + 1))
        p = int(rng.integers(0, len(seqs[c]) - ln - 1))
        r = bytearray(seqs[c][p:p + ln])
        mode = i % 8
        out = bytearray()
        for ch_ in r:
            u = rng.random()
            if mode == 7 and u < 0.06:
                continue
            if mode == 6 and u < 0.05:
                out.append(ch_); out.append(b"ACGT"[int(rng.integers(0, 4))]); continue
            if u < (0.0 if mode == 0 else 0.02 + 0.01 * mode):
                out.append(b"ACGT"[int(rng.integers(0, 4))])
            else:
                out.append(ch_)
        if mode == 3 and len(out) > 12:
            out[int(rng.integers(0, len(out)))] = ord("N")
        if mode == 5:                                           # unrelated read
            out = bytearray(b"ACGT"[int(x)] for x in rng.integers(0, 4, len(out)))
        r = bytes(out) if out else b"A"
        rev = bool(rng.random() < 0.5)
        if rev:
            r = r[::-1].translate(bytes.maketrans(b"ACGTN", b"TGCAN"))
        q = bytearray(b"I" * len(r))
        for j in range(len(q)):
            if rng.random() < 0.08:
                q[j] = 33 + int(rng.integers(0, 10))            # phred 0..9: below min_basqval = 10
        reads.append(r); quals.append(bytes(q)); kinds.append((mode, rev))
    return reads, quals, kinds


def oracle_params(oix, over):
    p = ol.default_params(oix)
    for name, key in (("min_swatscor", "min_swatscor"), ("min_swatscor_below_max", "below_max"), ("min_basq", "min_basq")):
        if key in over:
            setattr(p, name, over[key])
    if over.get("best") is False:
        p.flags &= ~FLG_BEST
    return p


def gpu_params(gix, over):
    p = gix.default_params()
    for name, key in (("min_swatscor", "min_swatscor"), ("min_swatscor_below_max", "below_max"), ("min_basqval", "min_basq")):
        if key in over:
            setattr(p, name, over[key])
    if over.get("best") is False:
        p.rmapflg &= ~FLG_BEST
    return p


def _oracle_index(seqs, names):
    """the oracle's index as it reads it back from its files (what the GPU library loads too)"""
    oix0 = ol.build_index(seqs, names, K, S)
    with tempfile.TemporaryDirectory() as tmp:
        pre = os.path.join(tmp, "ix")
        assert ol.lib().or_index_write(oix0, pre.encode()) == 0
        oix = ol.lib().or_index_read(pre.encode())
    return oix0, oix


def _oracle_map(oix, reads, quals, par):
    """-> per read (return code of the oracle, alignments, the six scalars)"""
    m = ol.Mapper(oix)
    out = []
    for r, q in zip(reads, quals):
        rv, res = m.map(r, q, par)
        st = m.stats()
        out.append((rv, res, dict(swmax=st[0], sw2nd=st[1], nseg=st[2], nseg_tot=st[3], nhit=st[4], nhit_tot=st[5])))
    m.close()
    return out


@functools.lru_cache(maxsize=None)
def single():
    """-> dict(oix0 (write it with or_index_write), seqs, reads, quals, kinds [(mode, reverse)], exp {parameter set: per read
    (rv, alignments, scalars)})"""
    from smalt_amd import synth
    ch = synth.make_reference(2, 60_000, seed=5101, repeat_frac=0.2, n_fam=1, cons_len=300, divergence=0.06)
    seqs = [synth.codes_to_ascii(c) for c in ch]
    reads, quals, kinds = _reads(seqs, NREADS, 8, 250, 5102)
    oix0, oix = _oracle_index(seqs, ["s0", "s1"])
    exp = {}
    for name, (over, with_q) in PARSETS.items():
        exp[name] = _oracle_map(oix, reads, quals if with_q else [b"I" * len(r) for r in reads], oracle_params(oix, over))
    return dict(oix0=oix0, seqs=seqs, reads=reads, quals=quals, kinds=kinds, exp=exp)


def sub_batches(n=NREADS):
    """[(first read, one past the last)] of the pipeline test"""
    cuts, at = [], 0
    for c in SUB_BATCHES:
        cuts.append((at, at + c)); at += c
    cuts.append((at, n))
    return cuts


def batch_parset(j):
    """the parameters alternate from batch to batch"""
    return "default" if j % 2 == 0 else "all40"


@functools.lru_cache(maxsize=None)
def overflow():
    """-> dict(oix0, reads, exp (default parameters), plain: indices of the reads that rank fewer than POOL_PER_READ candidates)"""
    from smalt_amd import synth
    ch = synth.make_reference(2, 150_000, seed=41, repeat_frac=0.3, n_fam=1, cons_len=300, divergence=0.03)
    rd, _ = synth.make_reads(ch, 300, 100, seed=42, sub_rate=0.01, indel_read_frac=0.05)
    seqs = [synth.codes_to_ascii(c) for c in ch]
    reads = [synth.codes_to_ascii(r) for r in rd]
    oix0, oix = _oracle_index(seqs, ["c0", "c1"])
    exp = _oracle_map(oix, reads, [b"I" * len(r) for r in reads], ol.default_params(oix))
    plain = [i for i, e in enumerate(exp) if e[2]["nseg"] < POOL_PER_READ]
    return dict(oix0=oix0, reads=reads, exp=exp, plain=plain)


def pool_capacity(max_batch_reads, per=POOL_PER_READ):
    """ranked candidates the pool of a mapper created with cands_per_read = per holds (smaltgpu_mapper_create_ex)"""
    return max(max_batch_reads * per, POOL_FLOOR)

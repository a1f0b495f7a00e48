"""stage_seed compiled for the host with one lane (tests/hostemu/emu_main.cpp, EMU_SEED_DUMP) against the reference of
tests/seed_ref.py, on every input the GPU tests of the seeding stage use (tests/seed_inputs.py): the step sweep, the parameter
sets, the stretches of split-read calls, the mixed batch and the two reads at the limit of the packed sort element.  This proves
the reference, the inputs and the layout of the stand-alone entry on a machine without a GPU, and pins the one-lane form of the
ranking; the wave form, the shuffles and the flush of the sort's range list exist on the device only (test_gpu_seed.py,
test_gpu_seed_sort.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import seed_inputs as si
import seed_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_main.cpp")


@pytest.fixture(scope="module")
def emu_bin():
    out = os.path.join(ROOT, "tests", "hostemu", "emu")
    tmp = "%s.%d.seed" % (out, os.getpid())          # other workers build the same file at the same time: never run a half-written one
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", tmp, SRC], check=True)
    os.replace(tmp, out)
    return out


def read_seed_dump(path):
    """The layout EMU_SEED_DUMP writes -> the dict Mapper.seed_batch returns."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"SMGSEED1"
    rows, stride, nbases, lookups = struct.unpack_from("<2I2Q", raw, 8)
    at = 8 + 8 + 16

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at).copy()
        at += a.nbytes
        return a
    codes, codes_rc = take(np.uint8, nbases), take(np.uint8, nbases)
    hi = take(np.uint32, rows * 8).reshape(rows, 8)
    seeds = take(np.uint32, rows * stride * 3).reshape(rows, stride, 3)
    qmask = take(np.uint8, rows * stride).reshape(rows, stride)
    assert at == len(raw)
    return dict(codes=codes, codes_rc=codes_rc, hi=hi, seeds=seeds, qmask=qmask, lookups=lookups, stride=stride, guard=sr.GUARD)


def run_emu(exe, prefix, reads, quals, par, tmp_path, totals_only=False, ranges=None, tag="e"):
    fq, dump = str(tmp_path / (tag + ".fq")), str(tmp_path / (tag + ".bin"))
    si.write_fastq(fq, reads, quals)
    env = dict(os.environ, EMU_SEED_DUMP=dump)
    if totals_only:
        env["EMU_TOTALS"] = "1"
    if ranges is not None:
        rf = str(tmp_path / (tag + ".rng"))
        with open(rf, "w") as f:
            f.write("".join("%d %d\n" % (a, b) for a, b in ranges))
        env["EMU_SEED_RANGE"] = rf
    opts = ["-H", str(par.ncut), "-q", str(par.min_basq)] + (["-x"] if par.noshort else [])
    subprocess.run([exe] + opts + [prefix, fq], check=True, capture_output=True, env=env)
    return read_seed_dump(dump)


@pytest.mark.parametrize("k,s", si.SWEEP, ids=["k%ds%d" % ks for ks in si.SWEEP])
def test_one_lane_stage_seed_equals_reference(k, s, emu_bin, oracle_built, tmp_path):
    """every parameter set, the stretches of split-read calls (-x) and the mixed batch, one index per (k, s)"""
    seqs, _ = si.reference()
    oix, prefix = si.build_index(seqs, k, s, tmp_path, "ix")
    try:
        reads, quals = si.sweep_reads(k, s)
        for name, (par, totals) in si.param_sets().items():
            got = run_emu(emu_bin, prefix, reads, quals, par, tmp_path, totals_only=totals, tag=name)
            sr.check_against(got, sr.ref_batch(oix, reads, quals, par, totals_only=totals), reads, name)
        rng = si.stretches(reads, k)
        par = sr.Par(noshort=True)
        got = run_emu(emu_bin, prefix, reads, quals, par, tmp_path, ranges=rng, tag="stretch")
        sr.check_against(got, sr.ref_batch(oix, reads, quals, par, ranges=rng), reads, "stretches")
        mreads, mquals = si.mixed_batch(k)
        got = run_emu(emu_bin, prefix, mreads, mquals, sr.Par(), tmp_path, tag="mixed")
        sr.check_against(got, sr.ref_batch(oix, mreads, mquals, sr.Par()), mreads, "mixed batch")
    finally:
        ol.lib().or_index_free(oix)


def test_one_lane_stage_seed_at_the_packed_element_limit(emu_bin, oracle_built, tmp_path):
    seqs, reads = si.packed_limit()
    oix, prefix = si.build_index(seqs, si.PACKED_K, si.PACKED_S, tmp_path, "px")
    try:
        quals = [b"I" * len(r) for r in reads]
        par = sr.Par(ncut=si.PACKED_NCUT)
        exp = sr.ref_batch(oix, reads, quals, par)
        assert int(exp[0].seeds[:, 1].max()) == (1 << 20) - 1 and int(exp[2].seeds[:, 1].max()) == 1 << 20
        got = run_emu(emu_bin, prefix, reads, quals, par, tmp_path)
        sr.check_against(got, exp, reads, "packed limit")
    finally:
        ol.lib().or_index_free(oix)


def test_sanitized_one_lane_build(oracle_built, tmp_path):
    """the same stand-alone program under the address and undefined-behaviour sanitizers (the runtimes linked into the program),
    on the sweep reads of one hashed and one perfect index with the default parameters and the stretches"""
    exe = str(tmp_path / "emu_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC], check=True)
    seqs, _ = si.reference()
    for k, s in ((20, 17), (13, 6)):
        oix, prefix = si.build_index(seqs, k, s, tmp_path, "sx%d" % k)
        try:
            reads, quals = si.sweep_reads(k, s)
            got = run_emu(exe, prefix, reads, quals, sr.Par(), tmp_path, tag="san%d" % k)
            sr.check_against(got, sr.ref_batch(oix, reads, quals, sr.Par()), reads, "sanitized")
            rng = si.stretches(reads, k)
            got = run_emu(exe, prefix, reads, quals, sr.Par(noshort=True), tmp_path, ranges=rng, tag="sanx%d" % k)
            sr.check_against(got, sr.ref_batch(oix, reads, quals, sr.Par(noshort=True), ranges=rng), reads, "sanitized stretches")
        finally:
            ol.lib().or_index_free(oix)

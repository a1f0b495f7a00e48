"""`smaltgpu-map` with SMALTGPU_DEVICE_PARSE=1 (the reads parsed on the device, smalt_amd/csrc/smg_reads_dev.hip) writes the bytes
it writes without the variable: single reads as FASTQ and as FASTA wrapped at 60 columns, read pairs from two files, and batches
of 16 reads so that an input takes several chunks; the stage line names the route only where the variable is set."""
import json
import os
import subprocess

import pytest

import golden_util as gu
import pair_replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
SINGLE, PAIR = "g_k11s4_cat", "gp_k13s6_pe"


@pytest.fixture(scope="module")
def inputs(oracle_built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("reads_dev_tool")
    fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == SINGLE][0], tmp)
    fa = str(tmp / "reads60.fa")
    with open(fa, "wb") as f:
        for nm, sq, _ in gu.read_fastq(fx["fq"]):
            f.write(b">" + nm.encode() + b"\n" + b"".join(sq[o:o + 60] + b"\n" for o in range(0, len(sq), 60)))
    px = pair_replay.load_fixture([e for e in json.load(open(os.path.join(gu.GOLD, "manifest_pairs.json"))) if e["tag"] == PAIR][0], tmp)
    return dict(tmp=tmp, fastq=(fx["prefix"], [fx["fq"]]), fasta=(fx["prefix"], [fa]), pairs=(px["prefix"], [str(tmp / (PAIR + e)) for e in ("_1.fq", "_2.fq")]))


def both_routes(inputs, key, opts):
    prefix, reads = inputs[key]
    outs = []
    for route in (None, "1"):
        env = dict(os.environ, SMALTGPU_MAP_VERBOSE="1")
        env.pop("SMALTGPU_DEVICE_PARSE", None)
        if route:
            env["SMALTGPU_DEVICE_PARSE"] = route
        out = str(inputs["tmp"] / ("out%s" % (route or "0")))
        r = subprocess.run([PROG] + opts + ["-o", out, prefix] + reads, capture_output=True, env=env)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        stages = [ln for ln in r.stderr.decode().split("\n") if "stages [s]: parse" in ln]
        assert len(stages) == 1 and ("parse (on the device) " in stages[0]) == bool(route), stages
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1]
    return outs[0]


@pytest.mark.parametrize("key,opts", [("fastq", ["-d", "-1", "-r", "3", "-f", "sam:nohead"]), ("fasta", ["-d", "-1", "-r", "3", "-f", "sam:nohead"]),
                                      ("pairs", ["-i", "500", "-r", "3", "-f", "sam:nohead"]), ("fastq", ["-r", "3", "-f", "cigar", "-B", "16"]),
                                      ("fasta", ["-r", "3", "-f", "cigar", "-B", "16"]), ("pairs", ["-i", "500", "-r", "3", "-f", "cigar", "-B", "16"])],
                         ids=["fastq_sam", "fasta60_sam", "pairs_sam", "fastq_B16", "fasta60_B16", "pairs_B16"])
def test_same_bytes_on_both_routes(inputs, key, opts):
    out = both_routes(inputs, key, opts)
    assert out.count(b"\n") > 100


def test_sample_counts_and_maps_on_both_routes(inputs):
    prefix, reads = inputs["pairs"]
    outs = []
    for route in ("0", "1"):
        out = str(inputs["tmp"] / ("sample" + route))
        r = subprocess.run([PROG, "sample", "-u", "2", "-o", out, prefix] + reads, capture_output=True, env=dict(os.environ, SMALTGPU_DEVICE_PARSE=route))
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and len(outs[0]) > 1000

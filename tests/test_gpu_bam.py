"""`smaltgpu-map -f bam`, file to file on the device: the BAM file must decode (tests/bam_reader.py) to the SAM lines the same program
writes with `-f sam` for the same command line -- which tests/test_gpu_report.py holds against the reference program.  Single reads
with several alignments a read and random choices, the SAM modifiers, gzipped input, pairs; batch sizes, host threads and two images
of the index; output on standard output; the option combinations the program refuses."""
import gzip
import json
import os
import subprocess

import pytest

import bam_reader as br
import golden_util as gu
import pair_replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
SINGLE, SINGLE_OPTS = "g_k11s2_d20", ["-d", "20", "-r", "3"]            # the options of its committed report cases
PAIR, PAIR_OPTS = "gp_k13s6_pe", ["-i", "500", "-r", "3"]


@pytest.fixture(scope="module")
def inputs(oracle_built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam")
    fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == SINGLE][0], tmp)
    gz = str(tmp / "reads.fq.gz")
    with open(fx["fq"], "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    px = pair_replay.load_fixture([e for e in json.load(open(os.path.join(gu.GOLD, "manifest_pairs.json"))) if e["tag"] == PAIR][0], tmp)
    return {"tmp": tmp, SINGLE: (fx["prefix"], [fx["fq"]]), SINGLE + ".gz": (fx["prefix"], [gz]), PAIR: (px["prefix"], [str(tmp / (PAIR + e)) for e in ("_1.fq", "_2.fq")]),
            "names": {SINGLE: (fx["names"], fx["seqs"])}}


def run(inputs, key, opts, name="out"):
    prefix, reads = inputs[key]
    out = str(inputs["tmp"] / name)
    r = subprocess.run([PROG] + opts + ["-o", out, prefix] + reads, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return open(out, "rb").read(), r.stdout


def same_as_sam(bam, sam, with_text=True):
    text, refs, recs, sizes = br.read_bam(bam)
    want = br.sam_records(sam)
    assert len(recs) == len(want) > 100
    for i, (x, y) in enumerate(zip(recs, want)):
        assert x == y, (i, x, y)
    if with_text:
        assert br.sam_header(text) == br.sam_header(sam) != []
        assert [ln for ln in br.sam_header(text) if ln.startswith(b"@SQ")] == [b"@SQ\tSN:%s\tLN:%d" % (n.encode(), ln) for n, ln in refs]
        pg = [ln for ln in text.split(b"\n") if ln.startswith(b"@PG")]
        assert len(pg) == 1 and b"-f bam" in pg[0]
    else:
        assert text == b"" and not br.sam_header(sam)
    return recs, refs


@pytest.mark.parametrize("key,mods", [(SINGLE, ""), (SINGLE, ":x"), (SINGLE, ":clip"), (SINGLE, ":nohead,x"), (SINGLE + ".gz", "")], ids=["plain", "x", "clip", "nohead_x", "gzip"])
def test_single_reads_decode_to_the_programs_sam(inputs, key, mods):
    sam, _ = run(inputs, key, SINGLE_OPTS + ["-f", "sam" + mods], "s.sam")
    bam, _ = run(inputs, key, SINGLE_OPTS + ["-f", "bam" + mods], "s.bam")
    recs, refs = same_as_sam(bam, sam, with_text="nohead" not in mods)
    names, seqs = inputs["names"][SINGLE]
    assert refs == [(n.split()[0], len(s)) for n, s in zip(names, seqs)]
    if mods == ":x":
        assert any("X" in r[5] for r in recs if r[5])
    if mods == ":clip":
        assert any("H" in r[5] for r in recs if r[5]) and not any("S" in r[5] for r in recs if r[5])


def test_pairs_decode_to_the_programs_sam(inputs):
    sam, _ = run(inputs, PAIR, PAIR_OPTS + ["-f", "sam"], "p.sam")
    bam, _ = run(inputs, PAIR, PAIR_OPTS + ["-f", "bam"], "p.bam")
    recs, refs = same_as_sam(bam, sam)
    assert sum(1 for r in recs if r[1] & 0x2) > 50 and any(r[8] < 0 for r in recs) and any(r[8] > 0 for r in recs)      # proper pairs, template lengths of both signs


def test_records_do_not_depend_on_batches_threads_or_devices(inputs):
    opts = SINGLE_OPTS + ["-f", "bam"]
    files = [run(inputs, SINGLE, opts + extra, "b%d.bam" % i)[0] for i, extra in enumerate((["-B", "64", "-n", "3"], ["-B", "7", "-n", "1"], ["-B", "20", "-g", "0,0"]))]
    decoded = [br.read_bam(f)[:3] for f in files]

    def without_program_line(d):
        return (b"\n".join(ln for ln in d[0].split(b"\n") if not ln.startswith(b"@PG")),) + d[1:]
    assert without_program_line(decoded[0]) == without_program_line(decoded[1]) == without_program_line(decoded[2])
    # equal -B, other threads: the same file, byte for byte (without the header text, which holds the command line)
    for batch, threads in (("64", ("3", "1")), ("7", ("1", "3"))):
        a, b = (run(inputs, SINGLE, SINGLE_OPTS + ["-f", "bam:nohead", "-B", batch, "-n", n], "t.bam")[0] for n in threads)
        assert a == b and br.read_bam(a)[2] == decoded[0][2]


def test_bam_on_standard_output(inputs):
    prefix, reads = inputs[SINGLE]
    r = subprocess.run([PROG] + SINGLE_OPTS + ["-f", "bam", prefix] + reads, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    sam, _ = run(inputs, SINGLE, SINGLE_OPTS + ["-f", "sam"], "s.sam")
    same_as_sam(r.stdout, sam)


def test_refused_combinations_and_the_histogram_prints(inputs):
    from smalt_amd import api
    prefix, reads = inputs[PAIR]
    out = str(inputs["tmp"] / "never.bam")
    r = subprocess.run([PROG, "-a", "-f", "bam", "-o", out, prefix] + reads, capture_output=True)
    assert r.returncode == 1 and b"-a" in r.stderr and b"bam" in r.stderr and not r.stdout and not os.path.exists(out)
    hist = str(inputs["tmp"] / "lib.smp")
    h = api.InsertHistogram.from_sample([250 + (7 * i) % 100 for i in range(400)])
    open(hist, "wb").write(h.text(api.HIST_SECTION))
    h.close()
    r = subprocess.run([PROG, "-I", hist, "-f", "bam:x"] + PAIR_OPTS + [prefix] + reads, capture_output=True)
    assert r.returncode == 1 and b"-I" in r.stderr and b"-o" in r.stderr and not r.stdout
    # with -o: the BAM file is whole, the two prints of the histogram stay on standard output
    bam, stdout = run(inputs, PAIR, ["-I", hist, "-f", "bam"] + PAIR_OPTS, "h.bam")
    sam, stdout_sam = run(inputs, PAIR, ["-I", hist, "-f", "sam"] + PAIR_OPTS, "h.sam")
    assert stdout == stdout_sam and stdout.startswith(b"#") and stdout.count(b"\n") > 4
    same_as_sam(bam, sam)

"""`smaltgpu-map -F sam|bam`, file to file on the device: reads from a SAM or BAM file must print, byte for byte, what the same command
prints for the same reads in FASTQ files -- which tests/test_gpu_report.py and tests/test_gpu_pair_report.py hold against the reference
program.  Single reads, pairs with the mates next to each other and shuffled apart, the program's own BAM output fed back, a file of
pairs, single reads and orphans mixed (batch sizes, threads, two images of the index, split reads, BAM out), a corrupt file.  The input
files come from tests/bam_writer.py, the template order from the restatement of the collation rules in tests/test_alnin.py."""
import json
import os
import random
import re
import subprocess

import pytest

import bam_reader as br
import bam_writer as bw
import golden_util as gu
import pair_replay
from test_alnin import expected_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
SINGLE, SINGLE_OPTS = "g_k11s2_d20", ["-d", "20", "-r", "3"]            # the options of its committed report cases
PAIR, PAIR_OPTS = "gp_k13s6_pe", ["-i", "500", "-r", "3"]
MATE1, MATE2 = 0x1 | 0x4 | 0x8 | 0x40, 0x1 | 0x4 | 0x8 | 0x80


def fastq(reads):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, s, q) for n, s, q in reads)


@pytest.fixture(scope="module")
def inputs(oracle_built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("alnin")
    fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == SINGLE][0], tmp)
    px = pair_replay.load_fixture([e for e in json.load(open(os.path.join(gu.GOLD, "manifest_pairs.json"))) if e["tag"] == PAIR][0], tmp)
    singles = [(n.encode(), 0x4, s, q) for n, s, q in gu.read_fastq(fx["fq"])]
    pairs = []
    for (n1, s1, q1), (n2, s2, q2) in zip(px["reads1"], px["reads2"]):
        assert n1.endswith("/1") and n2 == n1[:-1] + "2"
        pairs += [(n1[:-2].encode(), MATE1, s1, q1), (n1[:-2].encode(), MATE2, s2, q2)]
    shuffled = list(pairs)
    random.Random(20).shuffle(shuffled)
    # pairs, every fifth template a single read instead, three orphans; the single reads once more as a FASTQ file under the names they get
    mixed, alone = [], []
    for i in range(0, len(pairs), 2):
        if (i // 2) % 5 == 0:
            mixed.append((b"s%d" % (i // 2), 0x4, pairs[i + (i // 10) % 2][2], pairs[i + (i // 10) % 2][3]))
            alone.append((mixed[-1][0], mixed[-1][2], mixed[-1][3]))
        else:
            mixed += pairs[i:i + 2]
    for k, at in enumerate((7, 100, len(mixed))):
        name, flag, s, q = pairs[10 * k + (k & 1)]                              # a mate of a pair that was replaced: its partner never comes
        mixed.insert(at, (b"o%d" % k, flag, s, q))
        alone.append((b"o%d/%d" % (k, 1 + (k & 1)), s, q))
    files = {}
    for key, recs in (("singles", singles), ("pairs", pairs), ("shuffled", shuffled), ("mixed", mixed)):
        files[key + ".bam"] = str(tmp / (key + ".bam"))
        open(files[key + ".bam"], "wb").write(bw.bam_bytes(recs, 5000))         # several members, records across their seams
        files[key + ".sam"] = str(tmp / (key + ".sam"))
        open(files[key + ".sam"], "wb").write(bw.sam_text(recs))
    files["alone.fq"] = str(tmp / "alone.fq")
    open(files["alone.fq"], "wb").write(fastq(alone))
    return {"tmp": tmp, "files": files, SINGLE: (fx["prefix"], [fx["fq"]]), PAIR: (px["prefix"], [str(tmp / (PAIR + e)) for e in ("_1.fq", "_2.fq")]),
            "records": {"shuffled": shuffled, "mixed": mixed}, "cache": {}}


def run(inputs, prefix, reads, opts, name="out"):
    """the bytes the program writes for these options and input files (a command line that ran before is not run again)"""
    key = (prefix, tuple(reads), tuple(opts))
    if key not in inputs["cache"]:
        out = str(inputs["tmp"] / name)
        r = subprocess.run([PROG] + opts + ["-o", out, prefix] + reads, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        inputs["cache"][key] = open(out, "rb").read()
    return inputs["cache"][key]


def template_of(line, fmt):
    """the name of the template a line belongs to"""
    name = line.split(b"\t")[0] if fmt.startswith("sam") else line.split(b" ")[1]
    return re.sub(rb"/[12]$", b"", name)


def by_template(text, fmt):
    out = {}
    for ln in text.splitlines(keepends=True):
        out.setdefault(template_of(ln, fmt), []).append(ln)
    return out


@pytest.mark.parametrize("how,fmt", [("-F bam", "cigar"), ("-F bam", "sam:nohead"), ("-F sam", "cigar"), ("-F sam", "sam:nohead"), ("magic", "cigar")])
def test_single_reads_print_what_the_fastq_file_prints(inputs, how, fmt):
    prefix, reads = inputs[SINGLE]
    want = run(inputs, prefix, reads, SINGLE_OPTS + ["-f", fmt])
    assert want.count(b"\n") >= 150
    if how == "magic":                                                           # no -F: a BAM file is found by its magic
        got = run(inputs, prefix, [inputs["files"]["singles.bam"]], SINGLE_OPTS + ["-f", fmt])
    else:
        got = run(inputs, prefix, [inputs["files"]["singles." + how[3:]]], ["-F", how[3:]] + SINGLE_OPTS + ["-f", fmt])
    assert got == want


@pytest.mark.parametrize("fmt", ["cigar", "sam:nohead"])
@pytest.mark.parametrize("infmt", ["bam", "sam"])
def test_pairs_print_what_the_two_fastq_files_print(inputs, infmt, fmt):
    prefix, reads = inputs[PAIR]
    want = run(inputs, prefix, reads, PAIR_OPTS + ["-f", fmt])
    assert want.count(b"\n") >= 280
    assert run(inputs, prefix, [inputs["files"]["pairs." + infmt]], ["-F", infmt] + PAIR_OPTS + ["-f", fmt]) == want


def shuffled_templates(inputs):
    templates = expected_templates(inputs["records"]["shuffled"])
    order = [t[0][0][:-2] for t in templates]
    assert len(order) == 140 == len(set(order)) and order != sorted(order, key=lambda n: int(n[1:])) and all(len(t) == 2 for t in templates)
    return templates, order


@pytest.mark.parametrize("fmt", ["cigar", "sam:nohead"])
def test_shuffled_pairs_print_the_pairs_in_template_order(inputs, fmt):
    """The mates lie apart: a pair takes the place of its later record.  Without draws (-r -1) the output is the two-file run's lines,
    reordered into the template order."""
    prefix, reads = inputs[PAIR]
    templates, order = shuffled_templates(inputs)
    norand = ["-i", "500", "-r", "-1", "-f", fmt]
    lines = by_template(run(inputs, prefix, reads, norand), fmt)
    assert run(inputs, prefix, [inputs["files"]["shuffled.bam"]], ["-F", "bam"] + norand) == b"".join(b"".join(lines[name]) for name in order)


@pytest.mark.parametrize("fmt", ["cigar", "sam:nohead"])
def test_shuffled_pairs_draw_in_template_order(inputs, fmt):
    """With -r 3 the choice among equally good pairings draws from drand48 in the order of the templates, so the lines of such a pair
    depend on the pairs in front of it (reordering the lines of the two-file run does not give them).  The yardstick is the two-file
    run over FASTQ files that hold the pairs in the template order: byte for byte."""
    prefix, reads = inputs[PAIR]
    templates, order = shuffled_templates(inputs)
    inorder = [str(inputs["tmp"] / ("inorder_%d.fq" % k)) for k in (1, 2)]
    for k, path in enumerate(inorder):
        open(path, "wb").write(fastq([t[k] for t in templates]))
    want = run(inputs, prefix, inorder, PAIR_OPTS + ["-f", fmt])
    assert want.count(b"\n") >= 280 and want != run(inputs, prefix, reads, PAIR_OPTS + ["-f", fmt])
    assert run(inputs, prefix, [inputs["files"]["shuffled.bam"]], ["-F", "bam"] + PAIR_OPTS + ["-f", fmt]) == want


@pytest.mark.parametrize("which", ["pairs", "singles"])
def test_round_trip_of_the_programs_own_bam_output(inputs, which):
    """reverse-strand records, soft clips and unmapped mates as the writer left them give the reads back"""
    prefix, reads = inputs[PAIR if which == "pairs" else SINGLE]
    opts = PAIR_OPTS if which == "pairs" else ["-r", "3"]
    bam = run(inputs, prefix, reads, opts + ["-f", "bam"])
    recs = br.read_bam(bam)[2]
    assert len(recs) == (280 if which == "pairs" else 150) and any(r[1] & 0x10 for r in recs) and any(r[5] and "S" in r[5] for r in recs)
    path = str(inputs["tmp"] / ("back_%s.bam" % which))
    open(path, "wb").write(bam)
    assert run(inputs, prefix, [path], ["-F", "bam"] + opts + ["-f", "sam:nohead"]) == run(inputs, prefix, reads, opts + ["-f", "sam:nohead"])


MIXED_OPTS = ["-i", "500", "-r", "-1", "-f", "cigar"]


def mixed_expectation(inputs, extra, fmt="cigar"):
    prefix, reads = inputs[PAIR]
    opts = extra + MIXED_OPTS[:-1] + [fmt]
    paired = by_template(run(inputs, prefix, reads, opts), fmt)
    single = by_template(run(inputs, prefix, [inputs["files"]["alone.fq"]], opts), fmt)
    templates = expected_templates(inputs["records"]["mixed"])
    kinds = [len(t) for t in templates]
    assert kinds.count(1) == 28 + 3 and kinds.count(2) == 112 and kinds[-1] == 1
    want = b""
    for t in templates:
        name = re.sub(rb"/[12]$", b"", t[0][0])
        want += b"".join(paired[name] if len(t) == 2 else single[name])
    return want


@pytest.mark.parametrize("extra", [["-B", "64", "-n", "3"], ["-B", "7", "-n", "1"], ["-B", "20", "-g", "0,0"]], ids=["B64n3", "B7n1", "B20g00"])
def test_mixed_file_prints_every_template_by_its_own_route(inputs, extra):
    prefix, _ = inputs[PAIR]
    want = mixed_expectation(inputs, [])
    assert want.count(b"\n") == 2 * 112 + 31                                     # one line per read
    for infmt in ("bam", "sam") if extra[1] == "64" else ("bam",):
        assert run(inputs, prefix, [inputs["files"]["mixed." + infmt]], ["-F", infmt] + extra + MIXED_OPTS) == want


def test_mixed_file_with_split_reads(inputs):
    prefix, _ = inputs[PAIR]
    assert run(inputs, prefix, [inputs["files"]["mixed.bam"]], ["-F", "bam", "-p", "-B", "50"] + MIXED_OPTS) == mixed_expectation(inputs, ["-p"])


def test_mixed_file_bam_in_bam_out(inputs):
    prefix, _ = inputs[PAIR]
    opts = ["-F", "bam", "-B", "33"] + MIXED_OPTS[:-1]
    sam = run(inputs, prefix, [inputs["files"]["mixed.bam"]], opts + ["sam"])
    bam = run(inputs, prefix, [inputs["files"]["mixed.bam"]], opts + ["bam"])
    recs, want = br.read_bam(bam)[2], br.sam_records(sam)
    assert len(recs) == len(want) == 2 * 112 + 31
    for i, (x, y) in enumerate(zip(recs, want)):
        assert x == y, (i, x, y)
    body = b"".join(ln for ln in sam.splitlines(keepends=True) if not ln.startswith(b"@"))
    assert body == mixed_expectation(inputs, [], "sam:nohead")


def test_corrupt_file_ends_the_program_with_the_offset(inputs):
    prefix, _ = inputs[PAIR]
    good = open(inputs["files"]["mixed.bam"], "rb").read()
    data, offs = bw.bgzf(b"".join(br.bgzf_members(good)), 5000)
    assert data == good and len(offs) > 4
    at = offs[2] + 40
    bad = str(inputs["tmp"] / "corrupt.bam")
    open(bad, "wb").write(good[:at] + bytes([good[at] ^ 0x5a]) + good[at + 1:])
    out = str(inputs["tmp"] / "corrupt.out")
    r = subprocess.run([PROG, "-F", "bam"] + MIXED_OPTS + ["-o", out, prefix, bad], capture_output=True)
    assert r.returncode == 1 and b"byte offset %d " % offs[2] in r.stderr and b"BAM" in r.stderr, r.stderr.decode()[-2000:]

"""`smaltgpu-map -a`: the program with the explicit alignment blocks must print what the reference program `smalt map -a` printed for
the same command line -- every case of tests/golden/manifest_ali.json (tests/golden/make_golden_ali.py): single reads in CIGAR, SAM
and SSAHA lines, concatenated mode, pairs, split reads and the synthetic input `ali_shapes` for the corners of the block layout.
The alignments are the device's here; tests/test_report_ali.py checks the same text on the CPU from recorded alignments."""
import gzip
import json
import os
import subprocess
import sys

import pytest

import ali_data
import golden_util as gu
import pair_replay
import split_replay

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
ALI = json.load(open(os.path.join(gu.GOLD, "manifest_ali.json")))


@pytest.fixture(scope="module")
def inputs(oracle_built, tmp_path_factory):
    """(index prefix, read files) per fixture of the manifest, unpacked once"""
    import oracle_lib as ol
    tmp = tmp_path_factory.mktemp("ali")
    known = {"single": {e["tag"]: e for e in gu.MANIFEST_ALL}, "split": {e["tag"]: e for e in split_replay.MANIFEST},
             "pair": {e["tag"]: e for e in json.load(open(os.path.join(gu.GOLD, "manifest_pairs.json")))}}
    out = {}
    for c in ALI:
        tag = c["tag"]
        if tag in out:
            continue
        if c["kind"] == "single":
            fx = gu.unpack(known["single"][tag], tmp)
            out[tag] = (fx["prefix"], [fx["fq"]])
        elif c["kind"] == "split":
            fx = split_replay.load_fixture(known["split"][tag], tmp)
            out[tag] = (fx["prefix"], [fx["fq"]])
        elif c["kind"] == "pair":
            fx = pair_replay.load_fixture(known["pair"][tag], tmp)
            out[tag] = (fx["prefix"], [os.path.join(str(tmp), tag + e) for e in ("_1.fq", "_2.fq")])
        else:
            paths = {}
            for ext in ("fa", "fq"):
                paths[ext] = str(tmp / ("%s.%s" % (tag, ext)))
                with gzip.open(os.path.join(gu.GOLD, "%s.%s.gz" % (tag, ext)), "rb") as g, open(paths[ext], "wb") as f:
                    f.write(g.read())
            names, seqs = gu.read_fasta(paths["fa"])
            ix = ol.build_index(seqs, names, c["k"], c["s"])
            assert ol.lib().or_index_write(ix, str(tmp / tag).encode()) == 0
            ol.lib().or_index_free(ix)
            out[tag] = (str(tmp / tag), [paths["fq"]])
    return out, tmp


def _lines(b):
    return [x for x in b.split(b"\n") if not x.startswith(b"@PG")]


def _run(opts, extra, inp, out):
    prefix, reads = inp
    r = subprocess.run([PROG] + opts + extra + ["-o", out, prefix] + reads, capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return open(out, "rb").read()


@pytest.mark.parametrize("case", ALI, ids=["%s-%s" % (c["tag"], c["variant"]) for c in ALI])
def test_program_prints_the_blocks_smalt_map_prints(case, inputs):
    fxs, tmp = inputs
    with gzip.open(os.path.join(gu.GOLD, "%s.%s.out.gz" % (case["tag"], case["variant"])), "rb") as g:
        exp = g.read()
    assert ali_data.shapes_of(exp) == case["shapes"] and case["shapes"]["blocks"] >= 1          # the committed text still holds what it was made for
    # small batches and several host threads: the blocks must come out in input order
    got = _run(case["opts"], ["-B", "64", "-n", "3"], fxs[case["tag"]], str(tmp / "out.txt"))
    gl, el = _lines(got), _lines(exp)
    for i, (x, y) in enumerate(zip(gl, el)):
        assert x == y, (i, x, y)
    assert len(gl) == len(el)


def test_text_does_not_depend_on_batches_threads_devices_or_O(inputs):
    """one case again in batches of 7 reads on one host thread, on two images of the index (-g 0,0), and with -O, which the reference
    needs for output in input order and this program accepts without effect"""
    fxs, tmp = inputs
    case = [c for c in ALI if c["tag"] == "g_k11s2_d20"][0]
    outs = [_run(case["opts"], extra, fxs[case["tag"]], str(tmp / "cmp.txt")) for extra in (["-B", "64", "-n", "3"], ["-B", "7", "-n", "1"], ["-B", "20", "-g", "0,0"], ["-O", "-B", "64"])]
    assert outs[0] == outs[1] == outs[2] == outs[3] and outs[0].count(b"\n") == case["lines"]
    # -O alone changes nothing either
    plain = [x for x in case["opts"] if x != "-a"]
    assert _run(plain, [], fxs[case["tag"]], str(tmp / "cmp.txt")) == _run(plain, ["-O"], fxs[case["tag"]], str(tmp / "cmp.txt"))


def test_sample_does_not_take_a(inputs):
    fxs, tmp = inputs
    prefix, reads = fxs[[c for c in ALI if c["kind"] == "pair"][0]["tag"]]
    r = subprocess.run([PROG, "sample", "-a", "-o", str(tmp / "s.txt"), prefix] + reads, capture_output=True)
    assert r.returncode == 2 and r.stderr.startswith(b"usage: smaltgpu-map")


@pytest.mark.skipif(not os.path.exists(SMALT), reason="reference binary not built (make -C oracle ref)")
@pytest.mark.parametrize("tool,ncases,n,seed", [("fuzz_single.py", 5, 500, 31), ("fuzz_pairs.py", 5, 500, 32)], ids=["single", "pairs"])
def test_random_configurations_with_blocks(tool, ncases, n, seed):
    """a short run of the fuzzers with FUZZ_ALI=1, accepted as tests/test_gpu_fuzz_programs.py accepts theirs"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), str(ncases), str(n), str(seed)], capture_output=True, text=True, env=dict(os.environ, FUZZ_ALI="1"))
    ok = sum(1 for ln in r.stdout.split("\n") if " ok:" in ln)
    assert r.returncode == 0 and ok >= ncases - 3, r.stdout[-3000:] + r.stderr[-1000:]     # (a case the reference itself rejects is not counted)
    assert all(" -a ->" in ln for ln in r.stdout.split("\n") if " ok:" in ln)

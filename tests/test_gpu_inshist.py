"""Insert-size histograms end to end against the unmodified reference program (oracle/_ref/smalt, built by build() and shipped
with the tree): `smaltgpu-map sample` must write the file `smalt sample` writes, and `smaltgpu-map -I <file>` the lines
`smalt map -g <file>` prints.  The input (tests/inshist_data.py) has 300 pairs with two oriented pairings inside the default
insert range, which only the histogram tells apart, so the histogram changes hundreds of lines; 12 copies of it (21600 pairs)
give sampling intervals above 1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import inshist_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALT = os.path.join(ROOT, "oracle", "_ref", "smalt")
PROG = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
needs_ref = pytest.mark.skipif(not os.path.exists(SMALT), reason="reference binary not built (make -C oracle ref)")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """index, the three inputs and what `smalt sample` writes for them (once for the module)"""
    tmp = str(tmp_path_factory.mktemp("inshist"))
    pre, pairs = inshist_data.prepare(tmp, SMALT)
    w = {"tmp": tmp, "pre": pre, "pairs": pairs, "fq": {}, "smp": {}, "runs": {}}
    w["fq"]["all"] = inshist_data.write_pairs(os.path.join(tmp, "all"), pairs)
    w["fq"]["first"] = inshist_data.write_pairs(os.path.join(tmp, "first"), pairs[:100])
    w["fq"]["x12"] = inshist_data.write_pairs(os.path.join(tmp, "x12"), pairs, copies=12)
    for tag in ("all", "first"):
        w["smp"][tag] = os.path.join(tmp, tag + ".ref.smp")
        subprocess.run([SMALT, "sample", "-o", w["smp"][tag], pre] + w["fq"][tag], check=True, capture_output=True)
    return w


def _lines(path):
    return [ln for ln in open(path, "rb").read().split(b"\n") if not ln.startswith(b"@PG")]


def _map(w, who, opts):
    """lines (without @PG) and standard output of one `map` run of the reference (who = 'ref') or of smaltgpu-map; runs are kept"""
    key = (who,) + tuple(opts)
    if key not in w["runs"]:
        out = os.path.join(w["tmp"], "map_%d.out" % len(w["runs"]))
        if who == "ref":
            cmd = [SMALT, "map"] + opts
        else:                                              # the histogram file is -I here, -g names the devices; blocks of 700 pairs
            cmd = [PROG] + ["-I" if o == "-g" else o for o in opts] + ["-B", "700"]
        r = subprocess.run(cmd + ["-o", out, w["pre"]] + w["fq"]["all"], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        w["runs"][key] = (_lines(out), r.stdout)
    return w["runs"][key]


@needs_ref
@pytest.mark.parametrize("tag,opts,batch", [("all", [], 500), ("first", [], 262144), ("x12", ["-u", "100"], 3000), ("x12", ["-u", "3"], 2500)])
def test_sample_writes_the_reference_programs_file(world, tag, opts, batch):
    """SAM lines of the sampled pairs, both prints and the section, byte for byte; sampling intervals 1, 1, 5 and 3; blocks
    smaller than the sample and stretches of input smaller than a block"""
    w = world
    ref = w["smp"].get(tag) or os.path.join(w["tmp"], "x12%s.ref.smp" % "".join(opts))
    if not os.path.exists(ref):
        subprocess.run([SMALT, "sample"] + opts + ["-o", ref, w["pre"]] + w["fq"][tag], check=True, capture_output=True)
    out = os.path.join(w["tmp"], "prog.smp")
    r = subprocess.run([PROG, "sample"] + opts + ["-n", "4", "-B", str(batch), "-o", out, w["pre"]] + w["fq"][tag], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    a, b = open(ref, "rb").read(), open(out, "rb").read()
    assert a.count(b"\n") > 150 and b"HISTO_END\n" in a
    if a != b:
        al, bl = a.split(b"\n"), b.split(b"\n")
        diff = [(i, x, y) for i, (x, y) in enumerate(zip(al, bl)) if x != y]
        assert False, (len(al), len(bl), len(diff), diff[:3])


@needs_ref
def test_sample_refuses_a_single_file(world):
    r = subprocess.run([PROG, "sample", world["pre"], world["fq"]["all"][0]], capture_output=True)
    assert r.returncode != 0 and b"two read files" in r.stderr


@needs_ref
@pytest.mark.parametrize("hist", ["all", "first"])
@pytest.mark.parametrize("rng", [[], ["-i", "350", "-j", "250"]], ids=["default_range", "i350_j250"])
@pytest.mark.parametrize("fmt", ["cigar", "sam"])
def test_map_with_a_histogram_prints_the_reference_programs_lines(world, fmt, rng, hist):
    w = world
    base = ["-f", fmt, "-r", "7"] + rng
    ref_with, ref_stdout = _map(w, "ref", base + ["-g", w["smp"][hist]])
    ref_without, _ = _map(w, "ref", base)
    got_with, got_stdout = _map(w, "prog", base + ["-g", w["smp"][hist]])
    got_without, _ = _map(w, "prog", base)
    # not vacuous: the histogram changes lines, in the reference and here
    assert len(ref_with) == len(ref_without) and sum(1 for x, y in zip(ref_with, ref_without) if x != y) >= 1
    assert len(got_with) == len(got_without) and sum(1 for x, y in zip(got_with, got_without) if x != y) >= 1
    assert len(got_with) == len(ref_with)
    diff = [(i, x, y) for i, (x, y) in enumerate(zip(ref_with, got_with)) if x != y]
    assert not diff, (len(diff), diff[:3])
    assert got_without == ref_without
    assert got_stdout == ref_stdout and got_stdout.startswith(b"#")          # the two prints of the histogram as read back


@needs_ref
def test_a_malformed_histogram_stops_the_program_before_mapping(world):
    w = world
    bad = os.path.join(w["tmp"], "bad.smp")
    open(bad, "wb").write(open(w["smp"]["all"], "rb").read().replace(b"HISTO_END\n", b""))
    out = os.path.join(w["tmp"], "bad.out")
    r = subprocess.run([PROG, "-I", bad, "-o", out, "/no/such/index"] + w["fq"]["all"], capture_output=True)
    assert r.returncode != 0 and b"HISTO_END" in r.stderr and not os.path.exists(out)


def _views(api, pairs):
    L = api.lib()
    views, keep = [], []
    for which in (0, 1):
        text = b"".join(b"@p%d/%d\n" % (i, which + 1) + pr[which] + b"\n+\n" + b"I" * len(pr[which]) + b"\n" for i, pr in enumerate(pairs))
        rs = L.smaltgpu_reads_create()
        v = api.ReadsView()
        assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, 2, C.byref(v)) == 0, L.smaltgpu_last_error()
        views.append(v)
        keep.append((rs, text))
    return views, keep


@needs_ref
def test_library_calls_give_the_programs_lines_and_the_sample(world):
    """smaltgpu_map_pairs, smaltgpu_report_set_inshist, smaltgpu_report_emit_pairs: the CIGAR lines of the program (= the
    reference's); and with the settings of `sample` the insert sizes of smaltgpu_report_pair_inserts make the section that
    `smalt sample` wrote"""
    from smalt_amd import api
    L = api.lib()
    w = world
    pairs = w["pairs"]
    n = len(pairs)
    gix = api.Index.load(w["pre"], 0)
    mp = api.Mapper(gix, 2048, 128)
    names_p, sop_p, nseq = C.POINTER(C.c_char_p)(), C.POINTER(C.c_uint64)(), C.c_int64()
    assert L.smaltgpu_index_seqnames(gix.h, C.byref(names_p), C.byref(sop_p), C.byref(nseq)) == 0
    b = [np.frombuffer(b"".join(pr[which] for pr in pairs), dtype=np.uint8).copy() for which in (0, 1)]
    q = [np.full(b[which].shape, ord("I"), dtype=np.uint8) for which in (0, 1)]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(inshist_data.RLEN)
    views, keep = _views(api, pairs)
    rep = L.smaltgpu_report_create()
    txt, ln = C.c_void_p(), C.c_uint64()

    # `smalt map -f cigar -r 7 -g <file>`
    hist = api.InsertHistogram.read(w["smp"]["all"])
    lo, hi, _, _ = hist.bounds()
    po = api.PairOpts(min(0, lo), max(500, hi), api.LIB_PE, 0, 2)
    par = gix.default_params()
    h, _, _, _ = mp.map_pairs_raw(b[0], off, q[0], b[1], off, q[1], par, po)
    ro = api.ReportOpts()
    ro.format, ro.min_swscor, ro.outflags = api.FMT_CIGAR, 18, api.OUT_BEST | api.OUT_SINGLE | api.OUT_RANDSEL
    lines = {}
    for attach in (True, False):
        assert L.smaltgpu_report_set_inshist(rep, hist.h if attach else None) == 0
        C.CDLL(None).srand48(C.c_long(7))
        assert L.smaltgpu_report_emit_pairs(rep, h, C.byref(views[0]), C.byref(views[1]), names_p, nseq, C.byref(ro), C.byref(po), 2, C.byref(txt), C.byref(ln)) == 0, L.smaltgpu_last_error()
        lines[attach] = C.string_at(txt.value, ln.value).split(b"\n") if ln.value else []
    want, _ = _map(w, "ref", ["-f", "cigar", "-r", "7", "-g", w["smp"]["all"]])
    assert lines[True] == want
    assert lines[False] != want                      # detached: the lines without a histogram (and the widened range)
    L.smaltgpu_pairs_free(h)
    hist.close()

    # `smalt sample`: exhaustive search, every pair through the unrestricted round, any orientation, no draws
    po = api.PairOpts(0, 500, api.LIB_ANY, 1, 2)
    par.rmapflg |= api.FLG_NOSHRTINFO | api.FLG_SENSITIVE
    h, _, _, _ = mp.map_pairs_raw(b[0], off, q[0], b[1], off, q[1], par, po)
    ro.format, ro.modflags, ro.outflags = api.FMT_SAM, api.REP_SOFTCLIP, api.OUT_BEST | api.OUT_SINGLE
    assert L.smaltgpu_report_emit_pairs(rep, h, C.byref(views[0]), C.byref(views[1]), names_p, nseq, C.byref(ro), C.byref(po), 2, C.byref(txt), C.byref(ln)) == 0, L.smaltgpu_last_error()
    sam = C.string_at(txt.value, ln.value)
    isz, known, np_ = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint8)(), C.c_uint32()
    assert L.smaltgpu_report_pair_inserts(rep, C.byref(isz), C.byref(known), C.byref(np_)) == 0 and np_.value == n
    sizes = [isz[i] for i in range(n) if known[i]]
    assert 0.5 * n < len(sizes) < n                  # the ambiguous pairs have no size
    made = api.InsertHistogram.from_sample(sizes)
    ref = open(w["smp"]["all"], "rb").read()
    assert sam == ref[:ref.index(b"# Sampled histogram\n")]
    assert made.text(api.HIST_SECTION) == ref[ref.index(b"# SMALT histogram of insert sizes\n"):]
    made.close()
    L.smaltgpu_pairs_free(h)
    L.smaltgpu_report_free(rep)
    for rs, _ in keep:
        L.smaltgpu_reads_free(rs)
    mp.close()
    gix.close()

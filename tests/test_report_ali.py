"""Explicit alignment blocks (`smalt map -a`, SMALTGPU_REP_ALIOUT) of libsmaltgpu against the reference program: the committed
`<tag>.<variant>.out.gz` files of tests/golden/manifest_ali.json are what `smalt map ... -a` (oracle/_ref/smalt) printed
(tests/golden/make_golden_ali.py) -- behind the line of every mapped alignment the read and the reference side by side in blocks of
60 columns with a row of markers between them (fprintAlignment, report.c:248-388).  Host code, no GPU needed:

  * single reads: the raw alignments of the `*.post.txt.gz` fixtures go through smaltgpu_postprocess and smaltgpu_report_emit as in
    tests/test_report.py, with the flag set and the oracle's packed reference handed to smaltgpu_report_set_reference;
  * `ali_shapes`: the synthetic input for the corners of the layout (alignments of exactly 60 and 120 columns and the empty block
    behind them, runs of more than 62 matches, a gap in the last column of a line, N and IUPAC letters on both strands, an N in the
    reference, a lower-case read), mapped here by the CPU oracle;
  * split reads and pairs: the alignment sets and mapping calls the reference recorded, replayed as tests/test_split_report.py and
    tests/test_pairs_replay.py do (tests/hostemu/pair_ali_check.cpp for the pairs).

Before a text is compared, the counts of those corners recorded in the manifest are looked for in the committed text itself."""
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

import ali_data
import golden_util as gu
import pair_replay as pr
import split_replay as sr
from test_pairs_replay import driver_args
from test_postprocess import _blocks
from test_report import raw_batch, report_opts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALI = json.load(open(os.path.join(gu.GOLD, "manifest_ali.json")))
EARG = -3                                                    # SMALTGPU_EARG
SINGLE = [c for c in ALI if c["kind"] == "single"]
CASE_ID = lambda c: "%s-%s" % (c["tag"], c["variant"])       # noqa: E731


def expected(case):
    """the committed text, after a look that it still holds every corner of the layout the manifest counted in it"""
    with gzip.open(os.path.join(gu.GOLD, "%s.%s.out.gz" % (case["tag"], case["variant"])), "rb") as g:
        exp = g.read()
    assert ali_data.shapes_of(exp) == case["shapes"] and exp.count(b"\n") == case["lines"]
    assert case["shapes"]["blocks"] >= 1 and case["shapes"]["descending"] >= 1
    return exp


def same_lines(got, exp):
    gl = [x for x in got.split(b"\n") if not x.startswith(b"@PG")]          # the program line names the program and its command line
    el = [x for x in exp.split(b"\n") if not x.startswith(b"@PG")]
    for i, (x, y) in enumerate(zip(gl, el)):
        assert x == y, (i, x, y)
    assert len(gl) == len(el)


def ali_opts(api, opts):
    """options of `smalt map` with -a -> (report options with the flag, seed)"""
    assert "-a" in opts
    ro, seed = report_opts(api, [x for x in opts if x not in ("-a", "-p")])
    ro.modflags |= api.REP_ALIOUT
    if "-p" in opts:
        ro.outflags |= api.OUT_SPLIT
    return ro, seed


class Emitter:
    """a report with its header made, for one set of reference sequences"""

    def __init__(self, api, names, seqs, ro):
        self.api, self.L, self.ro, self.n = api, api.lib(), ro, len(seqs)
        self.sop = (C.c_uint64 * (len(seqs) + 1))()
        for i, s_ in enumerate(seqs):
            self.sop[i + 1] = self.sop[i] + len(s_)
        self.names = (C.c_char_p * len(names))(*[x.encode() for x in names])
        self.rep = self.L.smaltgpu_report_create()
        self.head = b""

    def header(self):
        txt, ln = C.c_void_p(), C.c_uint64()
        assert self.L.smaltgpu_report_header(self.rep, self.names, self.sop, self.n, C.byref(self.ro), b"smalt", b"0.7.6", 1, (C.c_char_p * 1)(b"t"), C.byref(txt), C.byref(ln)) == 0
        self.head = C.string_at(txt, ln.value)

    def emit(self, pout, raw, view, nthreads, ro=None):
        txt, ln = C.c_void_p(), C.c_uint64()
        rv = self.L.smaltgpu_report_emit(self.rep, C.byref(pout), C.byref(raw) if raw is not None else None, C.byref(view), self.names, self.n, C.byref(ro or self.ro), nthreads,
                                         C.byref(txt), C.byref(ln))
        return rv, (C.string_at(txt, ln.value) if rv == 0 else None)

    def close(self):
        self.L.smaltgpu_report_free(self.rep)


def postprocessed(api, L, post, em, raw, view, packed):
    par = api.Params()
    par.match, par.mismatch, par.gap_init, par.gap_ext = 1, -2, -4, -3
    pout = api.PostOut()
    assert L.smaltgpu_postprocess(post, em.sop, em.n, C.byref(raw), view.bases, view.quals if view.has_qual else None, view.read_off, packed, C.byref(par), 2, C.byref(pout)) == 0
    return pout


@pytest.mark.parametrize("case", SINGLE, ids=[CASE_ID(c) for c in SINGLE])
def test_blocks_of_single_reads_match_reference_program(case, oracle_built, tmp_path):
    from smalt_amd import api
    import oracle_lib as ol
    L = api.lib()
    exp = expected(case)
    fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == case["tag"]][0], tmp_path)
    text = open(fx["fq"], "rb").read()
    ro, seed = ali_opts(api, case["opts"])
    rs, post, em = L.smaltgpu_reads_create(), L.smaltgpu_post_create(), Emitter(api, fx["names"], fx["seqs"], ro)
    oix = ol.lib().or_index_read(fx["prefix"].encode())
    try:
        view = api.ReadsView()
        assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, 3, C.byref(view)) == 0, L.smaltgpu_last_error()
        blocks = list(_blocks(case["tag"]))
        assert view.nreads == len(blocks)
        raw, keep = raw_batch(api, blocks, view)
        packed = C.cast(oix.contents.packed, C.c_void_p)
        pout = postprocessed(api, L, post, em, raw, view, packed)
        em.header()
        assert L.smaltgpu_report_set_reference(em.rep, packed) == 0
        texts = []
        for nthreads in (1, 3):
            if ro.outflags & api.OUT_RANDSEL:
                C.CDLL(None).srand48(C.c_long(seed))
            rv, body = em.emit(pout, raw, view, nthreads)
            assert rv == 0, L.smaltgpu_last_error()
            texts.append(body)
        assert texts[0] == texts[1]
        same_lines(em.head + texts[0], exp)
    finally:
        L.smaltgpu_reads_free(rs)
        L.smaltgpu_post_free(post)
        em.close()
        ol.lib().or_index_free(oix)


@pytest.fixture(scope="module")
def shapes(oracle_built, tmp_path_factory):
    """ali_shapes, its index built and its reads mapped by the CPU oracle: computed once for the tests below"""
    from smalt_amd import api
    import oracle_lib as ol
    case = [c for c in ALI if c["kind"] == "shapes"][0]
    tmp = tmp_path_factory.mktemp("shapes")
    paths = {}
    for ext in ("fa", "fq"):
        paths[ext] = str(tmp / ("%s.%s" % (case["tag"], ext)))
        with gzip.open(os.path.join(gu.GOLD, "%s.%s.gz" % (case["tag"], ext)), "rb") as g, open(paths[ext], "wb") as f:
            f.write(g.read())
    names, seqs = gu.read_fasta(paths["fa"])
    oix = ol.build_index(seqs, names, case["k"], case["s"])
    om, opar = ol.Mapper(oix), ol.default_params(oix)
    blocks = []
    for nm, sq, ql in gu.read_fastq(paths["fq"]):
        rv, res = om.map(sq, ql, opar)
        assert rv == 0
        st = om.stats()
        # in the form test_report.raw_batch reads: RW fields, RX = count + the six statistics, RC = the best first-pass score
        blocks.append(dict(name=nm, rs=[[None, None, "R" if r["reverse"] else "F", r["score"], r["q_start"], r["q_end"], r["s_start"], r["s_end"], r["sidx"], r["diffstr"].hex()] for r in res],
                           rx=[len(res)] + st[0:6], rc=[st[6]]))
    om.close()
    assert len(blocks) == case["nreads"]
    yield dict(case=case, api=api, names=names, seqs=seqs, text=open(paths["fq"], "rb").read(), blocks=blocks, packed=C.cast(oix.contents.packed, C.c_void_p))
    ol.lib().or_index_free(oix)


def emit_shapes(sh, modflags, set_reference=True, header=True, nthreads=(1, 3)):
    api = sh["api"]
    L = api.lib()
    ro, seed = ali_opts(api, sh["case"]["opts"])
    ro.modflags = modflags
    rs, post, em = L.smaltgpu_reads_create(), L.smaltgpu_post_create(), Emitter(api, sh["names"], sh["seqs"], ro)
    try:
        view = api.ReadsView()
        assert L.smaltgpu_reads_parse(rs, sh["text"], len(sh["text"]), 1, 0, 1, C.byref(view)) == 0 and view.nreads == len(sh["blocks"])
        raw, keep = raw_batch(api, sh["blocks"], view)
        pout = postprocessed(api, L, post, em, raw, view, sh["packed"])
        if header:
            em.header()
        if set_reference:
            assert L.smaltgpu_report_set_reference(em.rep, sh["packed"]) == 0
        out = []
        for n in nthreads:
            rv, body = em.emit(pout, raw, view, n)
            out.append((rv, body, L.smaltgpu_last_error() if rv else b""))
        return out
    finally:
        L.smaltgpu_reads_free(rs)
        L.smaltgpu_post_free(post)
        em.close()


def test_shapes_match_reference_program(shapes):
    """every corner of the layout, against what the reference printed for the synthetic input"""
    case, api = shapes["case"], shapes["api"]
    exp = expected(case)
    for key in ("empty_blocks", "gap", "transition", "transversion", "unknown", "descending", "gap_in_last_column"):
        assert case["shapes"][key] >= 1, key
    (rv1, one, _), (rv3, three, _) = emit_shapes(shapes, api.REP_ALIOUT)
    assert rv1 == 0 and rv3 == 0
    assert one == three                                      # the text does not depend on the number of threads
    same_lines(one, exp)


def test_blocks_need_the_reference_and_the_header(shapes):
    api = shapes["api"]
    for kw in (dict(set_reference=False), dict(header=False)):
        (rv, body, msg), = emit_shapes(shapes, api.REP_ALIOUT, nthreads=(1,), **kw)
        assert rv == EARG and body is None and b"smaltgpu_report_set_reference" in msg          # never lines without their blocks


def test_without_the_flag_nothing_changes(shapes, oracle_built, tmp_path):
    """flag clear: the lines alone, with or without a reference set -- for the synthetic input the reference's lines without its
    blocks, for a committed case its committed text byte for byte"""
    api = shapes["api"]
    (rv, plain, _), = emit_shapes(shapes, 0, nthreads=(1,))
    (rv2, plain2, _), = emit_shapes(shapes, 0, set_reference=False, nthreads=(1,))
    assert rv == 0 and rv2 == 0 and plain == plain2
    exp = expected(shapes["case"])
    assert plain == b"".join(ln + b"\n" for ln in exp.split(b"\n") if ln.startswith(b"cigar:"))
    # an existing case through the same calls as tests/test_report.py, a reference set on the report
    import oracle_lib as ol
    L = api.lib()
    case = [c for c in json.load(open(os.path.join(gu.GOLD, "manifest_report.json"))) if c["tag"] == "g_k11s2_d20" and c["variant"] == "cigar"][0]
    fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == case["tag"]][0], tmp_path)
    text = open(fx["fq"], "rb").read()
    ro, seed = report_opts(api, case["opts"])
    rs, post, em = L.smaltgpu_reads_create(), L.smaltgpu_post_create(), Emitter(api, fx["names"], fx["seqs"], ro)
    oix = ol.lib().or_index_read(fx["prefix"].encode())
    try:
        view = api.ReadsView()
        assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, 3, C.byref(view)) == 0
        raw, keep = raw_batch(api, list(_blocks(case["tag"])), view)
        packed = C.cast(oix.contents.packed, C.c_void_p)
        pout = postprocessed(api, L, post, em, raw, view, packed)
        em.header()
        assert L.smaltgpu_report_set_reference(em.rep, packed) == 0
        C.CDLL(None).srand48(C.c_long(seed))
        rv, body = em.emit(pout, raw, view, 3)
        assert rv == 0
        with gzip.open(os.path.join(gu.GOLD, "%s.%s.out.gz" % (case["tag"], case["variant"])), "rb") as g:
            assert em.head + body == g.read()
    finally:
        L.smaltgpu_reads_free(rs)
        L.smaltgpu_post_free(post)
        em.close()
        ol.lib().or_index_free(oix)


def test_blocks_of_split_reads_match_reference_program(oracle_built, tmp_path):
    """partial alignments (class P) get their blocks too: the alignment sets the reference left under RMAPFLG_SPLIT, as
    tests/test_split_report.py feeds them to smaltgpu_report_emit"""
    from smalt_amd import api
    import oracle_lib as ol
    L = api.lib()
    case = [c for c in ALI if c["kind"] == "split"][0]
    exp = expected(case)
    entry = [e for e in sr.MANIFEST if e["tag"] == case["tag"]][0]
    fx = sr.load_fixture(entry, tmp_path)
    text = open(fx["fq"], "rb").read()
    n = len(fx["reads"])
    by_no = {R["no"]: sr.post_state(R["post_final"]) for R in fx["dump"]}
    rows, sortr, segsrtr, segnor, dstr = [], [], [], [], bytearray()
    res_off, sort_off, seg_off = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))()
    qsegno, setstatus, needs = (C.c_int32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)()
    for i in range(n):
        res_off[i], sort_off[i], seg_off[i] = len(rows), len(sortr), len(segnor)
        st = by_no.get(i)
        if not st or not st["ps"]:
            continue
        for w in st["rows"]:
            rows.append((w, len(dstr)))
            dstr += w["diffstr"]
        sortr += st["so"]
        segsrtr += st["ss"] if st["ss"] is not None else [-1] * len(st["so"])
        segnor += st["sg"] or []
        qsegno[i], setstatus[i] = st["ps"][2], st["ps"][3]
    res_off[n], sort_off[n], seg_off[n] = len(rows), len(sortr), len(segnor)
    res = (api.PostResult * max(1, len(rows)))()
    for j, (w, at) in enumerate(rows):
        r = res[j]
        r.swatscor, r.q_start, r.q_end, r.s_start, r.s_end, r.sidx = w["score"], w["q_start"], w["q_end"], w["s_start"], w["s_end"], w["sidx"]
        r.status, r.mapscor, r.prob, r.rsltx, r.qsegx, r.swrank = w["status"], w["mapscor"], w["prob"], w["rsltx"], w["qsegx"], w["swrank"]
        r.stroffs, r.strlen = at, len(w["diffstr"])
    arrays = [(C.c_int32 * max(1, len(v)))(*v) for v in (sortr, segsrtr, segnor)]
    a_dstr = (C.c_uint8 * max(1, len(dstr))).from_buffer_copy(bytes(dstr) or b"\0")
    pout = api.PostOut(n, res_off, res, a_dstr, sort_off, arrays[0], arrays[1], seg_off, arrays[2], qsegno, setstatus, needs)
    ro, seed = ali_opts(api, case["opts"])
    rs, em = L.smaltgpu_reads_create(), Emitter(api, fx["names"], fx["seqs"], ro)
    oix = ol.lib().or_index_read(fx["prefix"].encode())
    try:
        view = api.ReadsView()
        assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, 2, C.byref(view)) == 0 and view.nreads == n
        em.header()
        assert L.smaltgpu_report_set_reference(em.rep, C.cast(oix.contents.packed, C.c_void_p)) == 0
        texts = []
        for nthreads in (1, 3):
            rv, body = em.emit(pout, None, view, nthreads)
            assert rv == 0, L.smaltgpu_last_error()
            texts.append(body)
        assert texts[0] == texts[1]
        same_lines(texts[0], exp)
        # blocks behind partial alignments are part of what was compared
        el = exp.split(b"\n")
        assert sum(1 for i, x in enumerate(el) if x.startswith(b"cigar:P") and el[i + 1].startswith(b"    QUERY: ")) >= 30
    finally:
        L.smaltgpu_reads_free(rs)
        em.close()
        ol.lib().or_index_free(oix)


@pytest.fixture(scope="module")
def pair_ali_check(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    exe = str(tmp_path_factory.mktemp("pac") / "pair_ali_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "hostemu", "pair_ali_check.cpp"),
                    "-L" + os.path.join(ROOT, "smalt_amd"), "-lsmaltgpu", "-Wl,-rpath," + os.path.join(ROOT, "smalt_amd"), "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


PAIRED = [c for c in ALI if c["kind"] == "pair"]


@pytest.mark.parametrize("case", PAIRED, ids=[CASE_ID(c) for c in PAIRED])
def test_blocks_of_pairs_match_reference_program(case, pair_ali_check, tmp_path):
    """both mates of a pair, paired entries first, then the left-over alignments: the mapping calls the reference recorded for the
    paired fixture replayed into the product's pair logic, as tests/test_pairs_replay.py does"""
    exp = expected(case)
    tag = case["tag"]
    k = [e for e in json.load(open(os.path.join(gu.GOLD, "manifest_pairs.json"))) if e["tag"] == tag][0]["k"]
    paths = {}
    for ext in (".fa", "_1.fq", "_2.fq", ".refdump.txt"):
        paths[ext] = str(tmp_path / (tag + ext))
        with gzip.open(os.path.join(gu.GOLD, tag + ext + ".gz"), "rb") as g, open(paths[ext], "wb") as f:
            f.write(g.read())
    assert len(pr.parse(open(paths[".refdump.txt"]).read())) == len(gu.read_fastq(paths["_1.fq"]))
    outs = []
    for threads in (1, 3):
        r = subprocess.run([pair_ali_check, paths[".refdump.txt"], paths["_1.fq"], paths["_2.fq"], paths[".fa"], "threads=%d" % threads, "ali=1"] + driver_args(case["opts"], k),
                           capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    same_lines(outs[0], b"".join(ln + b"\n" for ln in exp.split(b"\n")[:-1] if not ln.startswith(b"@")))
    # flag set, no reference: an error, not lines without blocks
    r = subprocess.run([pair_ali_check, paths[".refdump.txt"], paths["_1.fq"], paths["_2.fq"], paths[".fa"], "threads=1", "ali=1", "noref=1"] + driver_args(case["opts"], k), capture_output=True)
    assert r.returncode != 0 and b"smaltgpu_report_set_reference" in r.stderr and not r.stdout

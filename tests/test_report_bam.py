"""BAM output (`smalt map -f bam`, SMALTGPU_FMT_BAM) of libsmaltgpu.  Host code, no GPU needed.  The reference build has no BAM writer
(it lacks the library), so the yardstick is the reference's SAM output: a BAM record is the SAM line of the same alignment in binary,
and tests/bam_reader.py -- pure Python, nothing of smg_bam.hpp -- decodes the file into the tuples it makes of SAM lines.

  * single reads: the SAM variants of tests/golden/manifest_report.json through the calls of tests/test_report.py with FMT_BAM;
    header + emit + finish must decode to the committed output of the reference program, record for record;
  * pairs: the SAM variants of manifest_pair_reports.json through the replay of tests/test_pairs_replay.py (tests/hostemu/pair_check.cpp
    prints what smaltgpu_report_emit_pairs hands out);
  * framing, determinism over threads and calls, the shapes of records (a record across blocks, no qualities, letters outside the
    alphabet, odd length), the limits, the ABI;
  * tests/hostemu/bam_check.cpp: smg_bam.hpp alone under the address and undefined-behaviour sanitizers, byte for byte against the library."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess
import zlib

import pytest

import bam_reader as br
import golden_util as gu
from test_pairs_replay import PAIRS, driver_args
from test_postprocess import _blocks
from test_report import raw_batch, report_opts
from test_report_ali import Emitter, postprocessed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARG = -3                                                    # SMALTGPU_EARG
IS_SAM = lambda c: c["opts"][c["opts"].index("-f") + 1].startswith("sam")       # noqa: E731
SINGLE = [c for c in json.load(open(os.path.join(gu.GOLD, "manifest_report.json"))) if IS_SAM(c) and not c.get("remap")]
PAIRED = [c for c in json.load(open(os.path.join(gu.GOLD, "manifest_pair_reports.json"))) if IS_SAM(c) and not c.get("remap")]
CASE_ID = lambda c: "%s-%s" % (c["tag"], c["variant"])       # noqa: E731


def test_the_cases_are_the_sam_variants_of_the_manifests():
    assert len(SINGLE) == 21 and {c["variant"] for c in SINGLE} == {"sam", "samx", "samclip", "sam_d0", "wrapped_sam", "fasta_sam"}
    assert len(PAIRED) == 19


def committed(case):
    with gzip.open(os.path.join(gu.GOLD, "%s.%s.out.gz" % (case["tag"], case["variant"])), "rb") as g:
        return g.read()


def bam_opts(api, opts):
    ro, seed = report_opts(api, opts)
    assert ro.format == api.FMT_SAM
    ro.format = api.FMT_BAM
    return ro, seed


def finish(L, em, ro=None):
    txt, ln = C.c_void_p(), C.c_uint64()
    assert L.smaltgpu_report_finish(em.rep, C.byref(ro or em.ro), C.byref(txt), C.byref(ln)) == 0
    return C.string_at(txt, ln.value)


def check_header(case_text, text, refs, names, seqs, with_text):
    """header text = the reference's header lines but the program line; the binary list = the sequences of the index"""
    assert refs == [(n.split()[0], len(s)) for n, s in zip(names, seqs)]
    if with_text:
        assert br.sam_header(text) == br.sam_header(case_text) != []
        assert [ln for ln in br.sam_header(text) if ln.startswith(b"@SQ")] == [b"@SQ\tSN:%s\tLN:%d" % (n.encode(), ln) for n, ln in refs]
        assert text.endswith(b"\n") and b"\0" not in text
    else:
        assert text == b""


class SingleRun:
    """the route of tests/test_report.py for one committed case: reads parsed, alignments post-processed, ready to emit any range of reads"""

    def __init__(self, case, tmp_path):
        from smalt_amd import api
        import oracle_lib as ol
        self.api, self.L, self.ol, self.case = api, api.lib(), ol, case
        L = self.L
        self.fx = fx = gu.unpack([e for e in gu.MANIFEST_ALL if e["tag"] == case["tag"]][0], tmp_path)
        style = case.get("input")
        self.text = open(gu.reshape_reads(fx["fq"], style, str(tmp_path / "reshaped.txt")) if style else fx["fq"], "rb").read()
        self.blocks = list(_blocks(case["tag"]))
        self.ro, self.seed = bam_opts(api, case["opts"])
        self.rs, self.post = L.smaltgpu_reads_create(), L.smaltgpu_post_create()
        self.oix = ol.lib().or_index_read(fx["prefix"].encode())
        self.packed = C.cast(self.oix.contents.packed, C.c_void_p)

    def close(self):
        self.L.smaltgpu_reads_free(self.rs)
        self.L.smaltgpu_post_free(self.post)
        self.ol.lib().or_index_free(self.oix)

    def bam(self, nthreads=3, pieces=1, ro=None):
        """header + emit (the reads in `pieces` calls) + finish"""
        api, L = self.api, self.L
        ro = ro or self.ro
        em = Emitter(api, self.fx["names"], self.fx["seqs"], ro)
        try:
            em.header()
            out = em.head
            if ro.outflags & api.OUT_RANDSEL:
                C.CDLL(None).srand48(C.c_long(self.seed))
            n, at = len(self.blocks), 0
            for k in range(pieces):
                lo, hi = n * k // pieces, n * (k + 1) // pieces
                view = api.ReadsView()
                chunk = self.text[at:]
                assert L.smaltgpu_reads_parse(self.rs, chunk, len(chunk), 1, hi - lo, 3, C.byref(view)) == 0, L.smaltgpu_last_error()
                assert view.nreads == hi - lo
                at += view.consumed
                raw, keep = raw_batch(api, self.blocks[lo:hi], view)
                pout = postprocessed(api, L, self.post, em, raw, view, self.packed)
                rv, body = em.emit(pout, raw, view, nthreads)
                assert rv == 0, L.smaltgpu_last_error()
                assert body[-28:] != br.EOF_BLOCK
                out += body
            return out + finish(L, em)
        finally:
            em.close()


@pytest.mark.parametrize("case", SINGLE, ids=[CASE_ID(c) for c in SINGLE])
def test_single_reads_decode_to_the_reference_programs_sam(case, oracle_built, tmp_path):
    run = SingleRun(case, tmp_path)
    try:
        exp = committed(case)
        data = run.bam()
        text, refs, recs, sizes = br.read_bam(data)
        want = br.sam_records(exp)
        assert len(recs) == len(want) >= len(run.blocks)
        for i, (x, y) in enumerate(zip(recs, want)):
            assert x == y, (i, x, y)
        assert all(t == [("NM", "i", t[0][2]), ("AS", "i", t[1][2])] for t in (r[11] for r in recs))
        with_text = bool(run.ro.modflags & run.api.REP_HEADER)
        assert with_text == bool(br.sam_header(exp))
        check_header(exp, text, refs, run.fx["names"], run.fx["seqs"], with_text)
        # the other setting of the header flag: the text comes or goes, the binary list stays
        other = run.api.ReportOpts.from_buffer_copy(run.ro)
        other.modflags ^= run.api.REP_HEADER
        em = Emitter(run.api, run.fx["names"], run.fx["seqs"], other)
        try:
            em.header()
            text2, refs2, at = br.decode_header(b"".join(br.bgzf_members(em.head)))
            assert refs2 == refs and bool(text2) != with_text
            if not with_text:
                assert [ln for ln in br.sam_header(text2) if ln.startswith(b"@SQ")] == [b"@SQ\tSN:%s\tLN:%d" % (n.encode(), ln) for n, ln in refs]
        finally:
            em.close()
    finally:
        run.close()


@pytest.fixture(scope="module")
def pair_check(tmp_path_factory):
    """the replay driver of tests/test_pairs_replay.py: it prints whatever smaltgpu_report_emit_pairs hands out"""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "smalt_amd", "csrc")], check=True)
    exe = str(tmp_path_factory.mktemp("pcb") / "pair_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "hostemu", "pair_check.cpp"),
                    "-L" + os.path.join(ROOT, "smalt_amd"), "-lsmaltgpu", "-Wl,-rpath," + os.path.join(ROOT, "smalt_amd"), "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return exe


@pytest.mark.parametrize("case", PAIRED, ids=[CASE_ID(c) for c in PAIRED])
def test_pairs_decode_to_the_reference_programs_sam(case, pair_check, tmp_path):
    from smalt_amd import api
    tag = case["tag"]
    exp = committed(case)
    paths = {}
    for ext in (".fa", "_1.fq", "_2.fq", ".refdump.txt"):
        paths[ext] = str(tmp_path / (tag + ext))
        with gzip.open(os.path.join(gu.GOLD, tag + ext + ".gz"), "rb") as g, open(paths[ext], "wb") as f:
            f.write(g.read())
    names, seqs = gu.read_fasta(paths[".fa"])
    seqinfo = str(tmp_path / "seqinfo.txt")
    with open(seqinfo, "w") as o:
        for n, s in zip(names, seqs):
            o.write("%s %d\n" % (n.split()[0], len(s)))
    refs = [(n.split()[0], len(s)) for n, s in zip(names, seqs)]
    args = ["fmt=%d" % api.FMT_BAM if a == "fmt=%d" % api.FMT_SAM else a for a in driver_args(case["opts"], PAIRS[tag]["k"])]
    assert "fmt=%d" % api.FMT_BAM in args
    want = br.sam_records(exp)
    outs = []
    for threads in (1, 3):
        r = subprocess.run([pair_check, paths[".refdump.txt"], paths["_1.fq"], paths["_2.fq"], seqinfo, "threads=%d" % threads] + args, capture_output=True)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs.append(r.stdout)
        recs = br.decode_records(b"".join(br.bgzf_members(r.stdout)), refs)
        assert len(recs) == len(want) > 0
        for i, (x, y) in enumerate(zip(recs, want)):
            assert x == y, (i, x, y)
    assert outs[0] == outs[1]
    # the header of the same report options
    ro, seed = bam_opts(api, ["-f", case["opts"][case["opts"].index("-f") + 1]])
    em = Emitter(api, names, seqs, ro)
    try:
        em.header()
        text, refs_got, at = br.decode_header(b"".join(br.bgzf_members(em.head)))
        check_header(exp, text, refs_got, names, seqs, bool(ro.modflags & api.REP_HEADER))
        assert bool(ro.modflags & api.REP_HEADER) == bool(br.sam_header(exp))
    finally:
        em.close()


@pytest.fixture(scope="module")
def big(oracle_built, tmp_path_factory):
    """g_k13s6_hash / sam (250 reads, random choices with -r 3): the records fill more than one block"""
    case = [c for c in SINGLE if c["tag"] == "g_k13s6_hash" and c["variant"] == "sam"][0]
    run = SingleRun(case, tmp_path_factory.mktemp("big"))
    yield run
    run.close()


def test_framing(big):
    data = big.bam()
    assert data[-28:].hex() == "1f8b08040000000000ff0600424302001b0003000000000000000000"
    payloads = br.bgzf_members(data)                          # walks the members to the last byte: nothing follows the end-of-file block
    assert payloads[-1] == b"" and all(p for p in payloads[:-1])
    # header, every emit and finish end their blocks: the header's members hold the header alone
    em = Emitter(big.api, big.fx["names"], big.fx["seqs"], big.ro)
    try:
        em.header()
        head = b"".join(br.bgzf_members(em.head))
        assert br.decode_header(head)[2] == len(head) and data.startswith(em.head)
    finally:
        em.close()
    sizes = [len(p) for p in payloads]
    assert len(sizes) >= 4 and sizes[1] == br.PAYLOAD_MAX      # header | full block(s) of records, cut inside a record | rest | end


def test_bytes_do_not_depend_on_threads_nor_records_on_calls(big):
    one = big.bam(nthreads=1)
    assert big.bam(nthreads=3) == one and big.bam(nthreads=7) == one
    whole = br.read_bam(one)
    for pieces in (2, 5):
        split = br.read_bam(big.bam(nthreads=3, pieces=pieces))
        assert split[:3] == whole[:3]
        assert len(split[3]) == pieces + 2 and sum(split[3]) == sum(whole[3])      # header | a block per call, each ended by its call | end


# ---- shapes: synthetic blocks of unplaced reads (no alignments needed) ----------------------------------------------------------
def emit_unplaced(text, fmt, nthreads=3, modflags=None, names=("chr1",), lengths=(1000,)):
    """reads of `text` with empty alignment sets -> (rv of emit, header bytes, emit bytes, finish bytes, message)"""
    from smalt_amd import api
    L = api.lib()
    ro = api.ReportOpts()
    ro.format, ro.min_swscor = fmt, 18
    ro.modflags = api.REP_HEADER | api.REP_SOFTCLIP if modflags is None else modflags
    ro.outflags = api.OUT_BEST | api.OUT_SINGLE
    rs = L.smaltgpu_reads_create()
    em = Emitter(api, list(names), ["A" * n for n in lengths], ro)
    try:
        view = api.ReadsView()
        assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, 2, C.byref(view)) == 0, L.smaltgpu_last_error()
        n = view.nreads
        zeros = (C.c_uint64 * (n + 1))()
        i32 = (C.c_int32 * max(1, n))()
        pout = api.PostOut(n, zeros, (api.PostResult * 1)(), (C.c_uint8 * 1)(), zeros, i32, i32, zeros, i32, (C.c_int32 * max(1, n))(), (C.c_uint32 * max(1, n))(),
                           (C.c_int32 * max(1, n))())
        txt, ln = C.c_void_p(), C.c_uint64()
        hrv = L.smaltgpu_report_header(em.rep, em.names, em.sop, em.n, C.byref(ro), b"t", b"0", 1, (C.c_char_p * 1)(b"t"), C.byref(txt), C.byref(ln))
        head = C.string_at(txt, ln.value) if hrv == 0 else None
        rv, body = em.emit(pout, None, view, nthreads)
        msg = L.smaltgpu_last_error() if rv else b""
        return rv, head, body, finish(L, em), msg, hrv
    finally:
        L.smaltgpu_reads_free(rs)
        em.close()


def fastq(reads):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, s, q) for n, s, q in reads)


LONG_SEQ = (b"ACGTTGCAAGCTTAGGCATCGATCCGATTAGCAT" * 2100)[:70000]
LONG_QUAL = bytes(33 + (i * 7 + i // 11) % 41 for i in range(70000))
SHAPES = [(b"before", b"ACGTACGTAC", b"IIIIIHHHHH"), (b"long", LONG_SEQ, LONG_QUAL), (b"odd", b"ACGTA", b"!#5I~"), (b"letters", b"ARXUNacgt", b"IIIIIIIII"),
          (b"after", b"TTTT", b"ABCD")]


def test_shapes_long_record_letters_and_odd_length():
    from smalt_amd import api
    rv, head, body, end, msg, _ = emit_unplaced(fastq(SHAPES), api.FMT_BAM)
    assert rv == 0, msg
    text, refs, recs, sizes = br.read_bam(head + body + end)
    assert [r[0] for r in recs] == ["before", "long", "odd", "letters", "after"]
    assert all(r[1] == 4 and r[2] is None and r[3] == 0 and r[5] is None and r[6] is None and r[7] == 0 and r[11] == [("NM", "i", 0), ("AS", "i", 0)] for r in recs)
    # the long record spans blocks: the members of the emit call are full ones and a rest, and no record starts at their seams
    body_sizes = [len(p) for p in br.bgzf_members(body)]
    assert body_sizes[0] == br.PAYLOAD_MAX and len(body_sizes) >= 2 and sum(body_sizes) > 105000
    assert recs[1][9] == LONG_SEQ.decode() and recs[1][10] == LONG_QUAL.decode()
    assert recs[2][9] == "ACGTA" and recs[2][10] == "!#5I~"                      # odd length (the reader checks the unused half byte)
    assert recs[3][9] == "ARNTNACGT"                                             # R stays, X is outside the alphabet, U reads as T (the parser's codec)
    assert recs[4][9] == "TTTT" and recs[4][10] == "ABCD"
    # the same reads as SAM: the lines the records are defined by
    rv, head_s, body_s, end_s, msg, _ = emit_unplaced(fastq(SHAPES), api.FMT_SAM)
    assert rv == 0 and end_s == b"" and recs == br.sam_records(body_s)
    # threads
    for n in (1, 7):
        assert emit_unplaced(fastq(SHAPES), api.FMT_BAM, nthreads=n)[2] == body


def test_shapes_fasta_reads_have_no_qualities():
    from smalt_amd import api
    rv, head, body, end, msg, _ = emit_unplaced(b">f1 x\nACGTN\n>f2\nAC\nGT\n", api.FMT_BAM)
    assert rv == 0, msg
    stream = b"".join(br.bgzf_members(body))
    recs = br.decode_records(stream, [("chr1", 1000)])
    assert [(r[0], r[9], r[10]) for r in recs] == [("f1", "ACGTN", None), ("f2", "ACGT", None)]
    assert b"f1\0\x12\x48\xf0" + b"\xff" * 5 + b"NMi" in stream and b"f2\0\x12\x48" + b"\xff" * 4 + b"NMi" in stream      # l_seq bytes of 0xFF each
    # hard clipping prints '*' for an unplaced read: no sequence at all
    rv, head, body, end, msg, _ = emit_unplaced(fastq(SHAPES[:1]), api.FMT_BAM, modflags=0)
    recs = br.decode_records(b"".join(br.bgzf_members(body)), [("chr1", 1000)])
    assert rv == 0 and recs[0][9] is None and recs[0][10] is None
    text, refs, at = br.decode_header(b"".join(br.bgzf_members(head)))
    assert text == b"" and refs == [("chr1", 1000)]


def test_limits():
    from smalt_amd import api
    ok = b"n" * 254
    rv, head, body, end, msg, _ = emit_unplaced(fastq([(ok, b"ACGT", b"IIII")]), api.FMT_BAM)
    assert rv == 0 and br.decode_records(b"".join(br.bgzf_members(body)), [("chr1", 1000)])[0][0] == ok.decode()
    long_name = b"read_with_a_long_name_" + b"x" * 233
    assert len(long_name) == 255
    rv, head, body, end, msg, _ = emit_unplaced(fastq([(b"fine", b"ACGT", b"IIII"), (long_name + b" second word", b"ACGT", b"IIII")]), api.FMT_BAM)
    assert rv == EARG and body is None and long_name in msg and b"second" not in msg
    assert emit_unplaced(fastq([(long_name, b"ACGT", b"IIII")]), api.FMT_SAM)[0] == 0          # a limit of the BAM record only
    # alignment blocks have no place in a BAM file: header and emit refuse
    rv, head, body, end, msg, hrv = emit_unplaced(fastq(SHAPES[:1]), api.FMT_BAM, modflags=api.REP_ALIOUT | api.REP_HEADER)
    assert rv == EARG and hrv == EARG and body is None and b"ALIOUT" in msg


def test_abi():
    from smalt_amd import api
    L = api.lib()
    assert api.FMT_BAM == 3
    header = open(os.path.join(ROOT, "include", "smaltgpu.h")).read()
    assert re.search(r"SMALTGPU_FMT_BAM = 3\b", header)
    assert re.search(r"^int smaltgpu_report_finish\(smaltgpu_report \*rp, const smaltgpu_report_opts \*op, const char \*\*text, uint64_t \*len\);", header, re.M)
    assert hasattr(C.CDLL(os.path.join(ROOT, "smalt_amd", "libsmaltgpu.so")), "smaltgpu_report_finish")
    rep = L.smaltgpu_report_create()
    try:
        for fmt, want in ((api.FMT_SAM, b""), (api.FMT_CIGAR, b""), (api.FMT_SSAHA, b""), (api.FMT_BAM, br.EOF_BLOCK)):
            ro = api.ReportOpts()
            ro.format = fmt
            txt, ln = C.c_void_p(), C.c_uint64(99)
            assert L.smaltgpu_report_finish(rep, C.byref(ro), C.byref(txt), C.byref(ln)) == 0
            assert ln.value == len(want) and C.string_at(txt, ln.value) == want
        assert L.smaltgpu_report_finish(rep, None, C.byref(txt), C.byref(ln)) == EARG
    finally:
        L.smaltgpu_report_free(rep)


def test_compression_level_switch(monkeypatch):
    """SMALTGPU_BAM_LEVEL is read when the report is created: level 0 stores, the records stay the same"""
    from smalt_amd import api
    out = {}
    for level in ("0", "9", "x", None):
        if level is None:
            monkeypatch.delenv("SMALTGPU_BAM_LEVEL", raising=False)
        else:
            monkeypatch.setenv("SMALTGPU_BAM_LEVEL", level)
        rv, head, body, end, msg, _ = emit_unplaced(fastq(SHAPES), api.FMT_BAM)
        assert rv == 0
        out[level] = body
    assert out["x"] == out[None]                              # not a level: zlib's default
    plain = [b"".join(br.bgzf_members(out[k])) for k in ("0", "9", None)]
    assert plain[0] == plain[1] == plain[2]
    assert len(out["0"]) > len(plain[0]) > len(out[None]) >= len(out["9"])      # stored blocks are larger than their payload


# ---- smg_bam.hpp alone, under sanitizers ------------------------------------------------------------------------------------------
def test_encoder_alone_under_sanitizers_gives_the_librarys_bytes(big, tmp_path):
    """tests/hostemu/bam_check.cpp includes smg_bam.hpp and nothing else of the library; built with -fsanitize=address,undefined (the
    runtimes linked into the program itself) it turns SAM lines into a BAM stream on its own and runs the corner shapes.  Its bytes must be the library's for the same records."""
    from smalt_amd import api
    exe = str(tmp_path / "bam_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(ROOT, "tests", "hostemu", "bam_check.cpp"), "-lz"], check=True)
    # (a) the synthetic shapes: the SAM lines of the library, the BAM bytes of the library
    rv, _, sam, _, _, _ = emit_unplaced(fastq(SHAPES), api.FMT_SAM)
    rv2, _, bam, end, _, _ = emit_unplaced(fastq(SHAPES), api.FMT_BAM)
    assert rv == 0 and rv2 == 0
    # (b) a committed case with placed reads: names looked up in the sequence list
    names = [n.split()[0] for n in big.fx["names"]]
    sam_ro = big.api.ReportOpts.from_buffer_copy(big.ro)
    sam_ro.format = api.FMT_SAM
    whole = big.bam(nthreads=3)
    head_len = len(Emitter_header(big))
    sam_big = b"\n".join(ln for ln in sam_text(big, sam_ro).split(b"\n") if not ln.startswith(b"@"))
    for tag, lines, want, refs in (("shapes", sam, bam + end, []), ("placed", sam_big, whole[head_len:], names)):
        src, dst = str(tmp_path / (tag + ".sam")), str(tmp_path / (tag + ".bgzf"))
        open(src, "wb").write(lines)
        r = subprocess.run([exe, src, dst, "5"] + refs, capture_output=True)
        assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
        got = open(dst, "rb").read()
        assert got == want
        m = re.search(rb"stream: (\d+) bytes, crc32 ([0-9a-f]{8})", r.stdout)
        assert m and int(m.group(1)) == len(got) and int(m.group(2), 16) == zlib.crc32(got)
        assert b"corner cases ok" in r.stdout


def Emitter_header(run):
    em = Emitter(run.api, run.fx["names"], run.fx["seqs"], run.ro)
    try:
        em.header()
        return em.head
    finally:
        em.close()


def sam_text(run, sam_ro):
    """the SAM lines of a committed case from the library (what the records are defined by)"""
    api, L = run.api, run.L
    em = Emitter(api, run.fx["names"], run.fx["seqs"], sam_ro)
    try:
        em.header()
        C.CDLL(None).srand48(C.c_long(run.seed))
        view = api.ReadsView()
        assert L.smaltgpu_reads_parse(run.rs, run.text, len(run.text), 1, 0, 3, C.byref(view)) == 0
        raw, keep = raw_batch(api, run.blocks, view)
        pout = postprocessed(api, L, run.post, em, raw, view, run.packed)
        rv, body = em.emit(pout, raw, view, 2)
        assert rv == 0
        return body
    finally:
        em.close()


def test_program_refuses_what_a_bam_file_cannot_hold(tmp_path):
    """the option checks of smaltgpu-map come before any device call: -a with -f bam, -I with BAM on standard output; usage and the
    message for an unknown format name bam"""
    from smalt_amd import api
    prog = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
    out = str(tmp_path / "never.bam")
    r = subprocess.run([prog, "-a", "-f", "bam", "-o", out, "/no/such/index", "/no/such/reads.fq"], capture_output=True)
    assert r.returncode == 1 and b"-a" in r.stderr and b"bam" in r.stderr and not r.stdout and not os.path.exists(out)
    hist = str(tmp_path / "lib.smp")
    h = api.InsertHistogram.from_sample([250 + (7 * i) % 100 for i in range(400)])
    open(hist, "wb").write(h.text(api.HIST_SECTION))
    h.close()
    r = subprocess.run([prog, "-I", hist, "-f", "bam:nohead", "/no/such/index", "/no/such/r1.fq", "/no/such/r2.fq"], capture_output=True)
    assert r.returncode == 1 and b"-I" in r.stderr and b"-o" in r.stderr and not r.stdout
    r = subprocess.run([prog, "-f", "gff", "/no/such/index", "/no/such/reads.fq"], capture_output=True)
    assert r.returncode == 1 and b"(cigar, sam, samsoft, ssaha, bam)" in r.stderr
    r = subprocess.run([prog], capture_output=True)
    assert r.returncode == 2 and b"| bam" in r.stderr

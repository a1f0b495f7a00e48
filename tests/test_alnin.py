"""Reads from SAM and BAM files (`smalt map -F sam|bam`, smaltgpu_alnreads_* of libsmaltgpu; smalt_amd/csrc/smg_alnin.hpp).  Host code,
no GPU needed.  The reference build has no SAM/BAM reader (it lacks the library), so the yardsticks are
  * smaltgpu_reads_parse: the reads of two committed FASTQ fixtures, written as SAM and as BAM by tests/bam_writer.py (pure Python,
    nothing of the library), must come out of feed / take with the same bases, qualities, offsets and names -- for several numbers of
    threads, windows of the input, sizes of the BGZF members and run lengths;
  * `expected_templates` below, a restatement of the collation rules in a few lines of Python, on a hand-made list of records;
  * every error the reader knows, with the offset or record number it must name;
  * tests/hostemu/alnin_check.cpp: smg_alnin.hpp alone under the address and undefined-behaviour sanitizers (the runtimes linked into
    the program), on the files of the groups above, the corrupt ones, and every prefix of a small BAM file."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess
import zlib

import pytest

import bam_writer as bw
import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARG, EFILE = -3, -2                                        # SMALTGPU_EARG, SMALTGPU_EFILE
UNMAPPED = 0x4
SINGLE, PAIR = "g_k11s2_d20", "gp_k13s6_pe"


def golden_text(name):
    with gzip.open(os.path.join(gu.GOLD, name + ".gz"), "rb") as g:
        return g.read()


def view_arrays(v):
    """a smaltgpu_reads_view -> (nreads, has_qual, bases, quals or None, read_off, names, name_off)"""
    n = v.nreads
    off, noff = list(v.read_off[:n + 1]), list(v.name_off[:n + 1])
    return (n, v.has_qual, C.string_at(v.bases, off[n]), C.string_at(v.quals, off[n]) if v.has_qual else None, off, C.string_at(v.names, noff[n]), noff)


def reads_of(arr):
    """-> [(name, bases, quals or None)]"""
    n, hq, bases, quals, off, names, noff = arr
    return [(names[noff[i]:noff[i + 1] - 1], bases[off[i]:off[i + 1]], quals[off[i]:off[i + 1]] if hq else None) for i in range(n)]


def parsed(text):
    """the yardstick: the arrays smaltgpu_reads_parse makes of a FASTQ text"""
    from smalt_amd import api
    L = api.lib()
    rs, view = L.smaltgpu_reads_create(), api.ReadsView()
    try:
        assert L.smaltgpu_reads_parse(rs, text, len(text), 1, 0, 2, C.byref(view)) == 0, L.smaltgpu_last_error()
        return view_arrays(view)
    finally:
        L.smaltgpu_reads_free(rs)


def read_runs(fmt, data, nthreads=1, window=None, max_templates=0, reader=None):
    """feed `data` in windows of `window` bytes (None: whole; a window grows by its size until the reader uses some of it) and take after
    every feed -> [(kind, arrays of the reads, arrays of the mates or None)]"""
    from smalt_amd import api
    rd = reader or api.AlnReads(fmt)
    runs, pos, step = [], 0, window or max(1, len(data))
    cur = step
    try:
        while True:
            last = pos + cur >= len(data)
            used = rd.feed(data[pos:pos + cur], last, nthreads)
            assert used <= cur and (not last or pos + used == len(data))
            pos += used
            while True:
                kind, v, m = rd.take(max_templates)
                if not kind:
                    assert v.nreads == 0 and m.nreads == 0
                    break
                assert v.nreads > 0 and m.nreads == (v.nreads if kind == 2 else 0) and (not max_templates or v.nreads <= max_templates)
                runs.append((kind, view_arrays(v), view_arrays(m) if kind == 2 else None))
            if last:
                return runs
            cur = step if used else cur + step
    finally:
        if reader is None:
            rd.close()


def records_of_fastq(arr, flag):
    return [(name, flag, bases, quals) for name, bases, quals in reads_of(arr)]


@pytest.fixture(scope="module")
def fixtures():
    """the two committed fixtures as the FASTQ parser sees them, and as records: the single reads unplaced, the pairs with mate 1 and
    mate 2 next to each other under one name"""
    one = parsed(golden_text(SINGLE + ".fq"))
    m1, m2 = parsed(golden_text(PAIR + "_1.fq")), parsed(golden_text(PAIR + "_2.fq"))
    assert one[0] == 150 and m1[0] == m2[0] == 140
    singles = records_of_fastq(one, UNMAPPED)
    pairs = []
    for (n1, b1, q1), (n2, b2, q2) in zip(reads_of(m1), reads_of(m2)):
        assert n1.endswith(b"/1") and n2 == n1[:-1] + b"2"
        pairs += [(n1[:-2], 0x1 | 0x4 | 0x8 | 0x40, b1, q1), (n1[:-2], 0x1 | 0x4 | 0x8 | 0x80, b2, q2)]
    return {"one": one, "m1": m1, "m2": m2, "singles": singles, "pairs": pairs}


def encoded(fmt, records, payload=0xff00, level=6, eof=True):
    from smalt_amd import api
    return bw.sam_text(records) if fmt == api.IN_SAM else bw.bam_bytes(records, payload, level, eof)


def joined(runs, side):
    return [r for run in runs for r in reads_of(run[side])]


# (threads, window, BGZF payload, max_templates, deflate level, end-of-file block)
SHAPES = [(1, None, 0xff00, 0, 6, True), (3, None, 300, 0, 6, True), (7, None, 1, 0, 1, True), (3, 1, 300, 0, 6, False), (1, 37, 300, 7, 0, True), (7, 65536, 0xff00, 1, 0, False),
          (3, 37, 1, 7, 6, True), (1, 65536, 300, 1, 9, True)]


@pytest.mark.parametrize("shape", SHAPES, ids=["t%d-w%s-p%d-m%d" % s[:4] for s in SHAPES])
@pytest.mark.parametrize("fmt", ["sam", "bam"])
def test_same_views_as_the_fastq_parser(fixtures, fmt, shape):
    from smalt_amd import api
    nthreads, window, payload, max_templates, level, eof = shape
    f = api.IN_SAM if fmt == "sam" else api.IN_BAM
    # single reads: one run of singles
    runs = read_runs(f, encoded(f, fixtures["singles"], payload, level, eof), nthreads, window, max_templates)
    assert all(k == 1 and m is None for k, v, m in runs)
    if not max_templates and not window:
        assert len(runs) == 1 and runs[0][1] == fixtures["one"][:7]              # bases, qualities, offsets and names, array for array
    if max_templates and not window:
        assert [r[1][0] for r in runs[:-1]] == [max_templates] * (len(runs) - 1)
    assert joined(runs, 1) == reads_of(fixtures["one"])
    assert all(r[1][1] == 1 for r in runs)
    # pairs: one run of pairs, mate 1 the read and mate 2 the mate
    runs = read_runs(f, encoded(f, fixtures["pairs"], payload, level, eof), nthreads, window, max_templates)
    assert all(k == 2 for k, v, m in runs)
    if not max_templates and not window:
        assert len(runs) == 1 and runs[0][1] == fixtures["m1"] and runs[0][2] == fixtures["m2"]
    assert joined(runs, 1) == reads_of(fixtures["m1"]) and joined(runs, 2) == reads_of(fixtures["m2"])


# ---- reverse strand and letters --------------------------------------------------------------------------------------------------
COMPLEMENT = dict(zip(b"ACGTUMRWSYKVHDBNacgtumrwsykvhdbn", b"TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn"))


def canonical(seq):
    """the letters as smaltgpu_reads_parse stores them: upper case, U -> T, anything that is no letter N"""
    out = bytearray()
    for c in seq.upper():
        c = ord("T") if c == ord("U") else c
        out.append(c if ord("A") <= c <= ord("Z") else ord("N"))
    return bytes(out)


def as_sequenced(rec):
    """a record -> (name, bases, quals) of the read it stands for, without the mate suffix"""
    name, flag, seq, qual = rec
    seq = seq or b""
    if flag & 0x10:
        seq = bytes(COMPLEMENT.get(c, c) for c in reversed(seq))
        qual = qual[::-1] if qual is not None else None
    return (name, canonical(seq), qual if seq else b"")


def ramp(n, start=0):
    return bytes(33 + (start + 3 * i) % 60 for i in range(n))


def strand_records():
    """all 16 BAM letters on both strands, odd and even lengths, one base, a name of 254 bytes, a read without qualities (the last)"""
    every = b"=ACMGRSVTWYHKDBN"
    return [(b"fwd16", 0x4, every, ramp(16)), (b"rev16", 0x4 | 0x10, every, ramp(16, 5)), (b"rev17", 0x10, every + b"A", ramp(17, 1)), (b"fwd17", 0, b"T" + every, ramp(17, 2)),
            (b"one", 0x4, b"G", b"I"), (b"one_rev", 0x14, b"R", b"#"), (b"n" * 254, 0x14, b"ACCGT", ramp(5)), (b"noqual_rev", 0x10, b"AACGN", None)]


SAM_LETTERS = [(b"low", 0x4, b"acgtuNrykm", ramp(10)), (b"low_rev", 0x14, b"acgtuNrykmX.-", ramp(13))]      # lower case, U, letters outside the BAM alphabet, non-letters


def test_reverse_strand_letters_lengths_and_names():
    from smalt_amd import api
    assert COMPLEMENT[ord("R")] == ord("Y") and COMPLEMENT[ord("K")] == ord("M") and COMPLEMENT[ord("B")] == ord("V") and COMPLEMENT[ord("D")] == ord("H")
    recs = strand_records()
    assert len(recs[6][0]) == 254
    want = [as_sequenced(r) for r in recs]
    assert want[0][1] == b"NACMGRSVTWYHKDBN" and want[1][1] == b"NVHMDRWABSYCKGTN" and want[1][2] == ramp(16, 5)[::-1] and want[5][1] == b"Y"
    for fmt in (api.IN_SAM, api.IN_BAM):
        for payload in (0xff00, 5):
            runs = read_runs(fmt, encoded(fmt, recs[:7], payload), 2)
            assert len(runs) == 1 and runs[0][0] == 1 and runs[0][1][1] == 1
            assert reads_of(runs[0][1]) == want[:7]
        runs = read_runs(fmt, encoded(fmt, recs), 2)                             # one read without qualities: the run has none
        assert len(runs) == 1 and runs[0][1][1] == 0 and runs[0][1][3] is None
        assert reads_of(runs[0][1]) == [(n, b, None) for n, b, q in want]
    # SAM alone: lower case, U, letters outside the BAM alphabet and non-letters
    recs = SAM_LETTERS
    runs = read_runs(api.IN_SAM, bw.sam_text(recs, header=False))
    assert reads_of(runs[0][1]) == [(b"low", b"ACGTTNRYKM", ramp(10)), (b"low_rev", b"NNXKMRYNAACGT", ramp(13)[::-1])]
    assert [as_sequenced(r) for r in recs] == reads_of(runs[0][1])


def test_a_record_without_sequence_is_a_read_of_no_bases():
    """as the FASTQ parser treats an empty sequence line: a read of length 0 that says nothing about qualities"""
    from smalt_amd import api
    ref = parsed(b"@a\nACGT\n+\nIIII\n@empty\n\n+\n\n@b\nGG\n+\n##\n")
    assert ref[0] == 3 and ref[1] == 1 and ref[4] == [0, 4, 4, 6]
    recs = [(b"a", 0x4, b"ACGT", b"IIII"), (b"empty", 0x4, None, None), (b"b", 0x4, b"GG", b"##")]
    for fmt in (api.IN_SAM, api.IN_BAM):
        runs = read_runs(fmt, encoded(fmt, recs))
        assert len(runs) == 1 and runs[0][1] == ref


# ---- collation -------------------------------------------------------------------------------------------------------------------
def expected_templates(records):
    """the rules, restated: -> [(read,)] or [(read, mate)] in output order, reads as (name, bases, quals or None)"""
    out, waiting = [], {}
    for serial, rec in enumerate(records):
        name, flag = rec[0], rec[1]
        if flag & 0x900:
            continue
        read = as_sequenced(rec)
        if not flag & 0x1 or bool(flag & 0x40) == bool(flag & 0x80):
            out.append((read,))
            continue
        mate = 1 if flag & 0x40 else 2
        read = (name + b"/%d" % mate,) + read[1:]
        if name in waiting and waiting[name][0] != mate:
            other = waiting.pop(name)[1]
            out.append((read, other) if mate == 1 else (other, read))
        else:
            if name in waiting:
                out.append((waiting[name][1],))
            waiting[name] = (mate, read, serial)
    return out + [(w[1],) for w in sorted(waiting.values(), key=lambda w: w[2])]


def expected_runs(templates, max_templates=0):
    """maximal stretches of one kind, cut at max_templates -> [(kind, has_qual, reads, mates)]; qualities None throughout a run without"""
    runs = []
    for t in templates:
        if not runs or runs[-1][0] != len(t) or (max_templates and len(runs[-1][2]) == max_templates):
            runs.append([len(t), 1, [], []])
        runs[-1][2].append(t[0])
        if len(t) == 2:
            runs[-1][3].append(t[1])
    for run in runs:
        if any(r[2] is None for r in run[2] + run[3]):
            run[1], run[2], run[3] = 0, [(n, b, None) for n, b, q in run[2]], [(n, b, None) for n, b, q in run[3]]
    return [tuple(r) for r in runs]


def seq_of(i, n=24):
    return bytes(b"ACGT"[(i * 7 + j * (i + 3) + j // 3) % 4] for j in range(n + i % 5))


def rec(name, flag, i, qual=True):
    s = seq_of(i)
    return (name, flag, s, ramp(len(s), i) if qual else None)


M1, M2, REV, SEC, SUP = 0x1 | 0x40, 0x1 | 0x80, 0x10, 0x100, 0x800
COLLATION = [
    rec(b"adj", M1, 0), rec(b"adj", M2, 1),                                     # mates next to each other
    rec(b"apart", M1, 2), rec(b"solo1", 0, 3), rec(b"swap", M2 | REV, 4),       # mates apart, a single between them, mate 2 in front of mate 1
    rec(b"apart", M1 | SEC, 5), rec(b"apart", M2 | SUP, 6),                     # secondary and supplementary records in between: dropped
    rec(b"solo2", 0x4, 7), rec(b"apart", M2, 8), rec(b"swap", M1, 9),
    rec(b"both", 0x1 | 0x40 | 0x80, 10), rec(b"neither", 0x1, 11), rec(b"both", 0x1 | 0x40 | 0x80, 12),      # 0x1 with both / neither: single reads, plain names
    rec(b"twice", M1, 13), rec(b"p2", M1, 14), rec(b"twice", M1 | REV, 15), rec(b"p2", M2, 16), rec(b"twice", M2, 17),      # a name that waits twice
    rec(b"nq", M1, 18, qual=False), rec(b"nq", M2, 19), rec(b"p3", M2, 20), rec(b"p3", M1 | REV, 21),        # a pair without qualities in a run of pairs
    rec(b"s3", 0, 22), rec(b"s4", REV, 23, qual=False), rec(b"s5", 0, 24),     # ... and a single without, in a run of singles
    rec(b"orph_a", M2, 25), rec(b"p4", M1, 26), rec(b"late", M1, 27), rec(b"p4", M2, 28), rec(b"orph_b", M1 | REV, 29),
    rec(b"p5", M1, 30), rec(b"p5", M2, 31), rec(b"p6", M2, 32), rec(b"p6", M1, 33),
    rec(b"s6", 0, 34), rec(b"orph_a", M2, 35), rec(b"s7", SEC, 36), rec(b"late", M2, 37), rec(b"orph_c", M2, 38), rec(b"s8", 0, 39),
]


def as_runs(runs):
    return [(k, v[1], reads_of(v), reads_of(m) if m else []) for k, v, m in runs]


def test_collation_rules():
    from smalt_amd import api
    assert len(COLLATION) == 40
    templates = expected_templates(COLLATION)
    names = [tuple(r[0] for r in t) for t in templates]
    assert names[:4] == [(b"adj/1", b"adj/2"), (b"solo1",), (b"solo2",), (b"apart/1", b"apart/2")] and (b"swap/1", b"swap/2") in names
    assert (b"both",) in names and (b"neither",) in names and names.count((b"twice/1",)) == 1 and (b"twice/1", b"twice/2") in names
    assert names[-4:] == [(b"s8",), (b"orph_b/1",), (b"orph_a/2",), (b"orph_c/2",)] and names.count((b"orph_a/2",)) == 2
    want = expected_runs(templates)
    assert [w[1] for w in want].count(0) == 2 and {w[0] for w in want if not w[1]} == {1, 2} and len(want) >= 10
    for fmt in (api.IN_SAM, api.IN_BAM):
        for payload, nthreads in ((0xff00, 1), (17, 3)):
            data = encoded(fmt, COLLATION, payload)
            assert as_runs(read_runs(fmt, data, nthreads)) == want
            for m in (1, 2, 3):
                assert as_runs(read_runs(fmt, data, nthreads, None, m)) == expected_runs(templates, m)
    # a pair completed in a later feed call: the reader is fed record by record, and emptied after every one
    for fmt in (api.IN_SAM, api.IN_BAM):
        rd = api.AlnReads(fmt)
        try:
            got, seen = [], 0
            pieces = [bw.sam_line(r) for r in COLLATION] if fmt == api.IN_SAM else [bw.bgzf(bw.bam_header(), eof=False)[0]] + [bw.bgzf_member(bw.bam_record(r)) for r in COLLATION]
            for i, piece in enumerate(pieces):
                assert rd.feed(piece, i == len(pieces) - 1, 2) == len(piece)
                while True:
                    kind, v, m = rd.take(0)
                    if not kind:
                        break
                    got += [(r,) for r in reads_of(view_arrays(v))] if kind == 1 else list(zip(reads_of(view_arrays(v)), reads_of(view_arrays(m))))
                if i == len(pieces) // 2:
                    seen = len(got)
            flat = [tuple((n, b, q) for n, b, q in t) for t in templates]
            strip = lambda ts: [tuple((n, b) for n, b, q in t) for t in ts]      # noqa: E731  (runs of one template: qualities per run differ from the whole file's)
            assert strip(got) == strip(flat) and 0 < seen < len(got)
        finally:
            rd.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def small_records():
    return [rec(b"e%d" % i, 0x4 if i % 3 else 0, i) for i in range(30)]


def error_cases():
    """-> [(label, format name, data, 'offset' or 'record', the number the message must name)]"""
    recs = small_records()
    stream = bw.bam_stream(recs)
    good, offs = bw.bgzf(stream, 300)
    assert len(offs) > 8
    cases = []

    def patched(at, new):
        return good[:at] + new + good[at + len(new):]
    third = offs[2]
    bsize = struct.unpack_from("<H", good, third + 16)[0]
    cases.append(("bad_magic", "bam", patched(third, b"\x1e"), "offset", third))
    cases.append(("no_extra_field", "bam", patched(third + 3, b"\0"), "offset", third))
    cases.append(("no_bc_field", "bam", patched(third + 12, b"XY"), "offset", third))
    cases.append(("bsize_tiny", "bam", patched(third + 16, struct.pack("<H", 20)), "offset", third))
    cases.append(("bsize_short", "bam", patched(third + 16, struct.pack("<H", bsize - 1)), "offset", third))
    cases.append(("bsize_past_end", "bam", patched(offs[-1] + 16, struct.pack("<H", 200)), "offset", offs[-1]))
    cases.append(("crc", "bam", patched(offs[3] - 8, bytes([good[offs[3] - 8] ^ 0x40])), "offset", third))
    cases.append(("isize", "bam", patched(offs[3] - 4, struct.pack("<I", 301)), "offset", third))
    cases.append(("isize_huge", "bam", patched(offs[3] - 4, struct.pack("<I", 70000)), "offset", third))
    cases.append(("deflate_data", "bam", patched(third + 25, bytes([good[third + 25] ^ 0xff])), "offset", third))
    cases.append(("truncated_member", "bam", good[:offs[5] + 40], "offset", offs[5]))
    cases.append(("truncated_header_of_member", "bam", good[:offs[5] + 7], "offset", offs[5]))
    head, body = bw.bam_header(), [bw.bam_record(r) for r in recs]

    def with_record(k, bad):
        return bw.bgzf(head + b"".join(body[:k]) + bad + b"".join(body[k + 1:]), 300)[0]
    cases.append(("block_size_past_the_data", "bam", with_record(29, bw.bam_record(recs[29], block_size=5000)), "record", 30))
    cases.append(("block_size_small", "bam", with_record(4, bw.bam_record(recs[4], block_size=20)), "record", 5))
    cases.append(("l_read_name_0", "bam", with_record(6, bw.bam_record(recs[6], l_read_name=0)), "record", 7))
    cases.append(("name_without_nul", "bam", with_record(7, bw.bam_record(recs[7], l_read_name=2)), "record", 8))
    cases.append(("fields_past_block_size", "bam", with_record(8, bw.bam_record(recs[8], l_read_name=250)), "record", 9))
    cases.append(("truncated_last_record", "bam", bw.bgzf(stream[:-9], 300)[0], "record", 30))
    cases.append(("truncated_block_size", "bam", bw.bgzf(stream + b"\x10\0", 300)[0], "record", 31))
    lines = [bw.sam_line(r) for r in recs]

    def with_line(k, bad):
        return bw.HEADER_TEXT + b"".join(lines[:k]) + bad + b"".join(lines[k + 1:])
    f = lines[10].split(b"\t")
    cases.append(("flag_not_a_number", "sam", with_line(10, b"\t".join([f[0], b"0x4"] + f[2:])), "record", 11))
    cases.append(("flag_empty", "sam", with_line(10, b"\t".join([f[0], b""] + f[2:])), "record", 11))
    cases.append(("flag_too_large", "sam", with_line(10, b"\t".join([f[0], b"65536"] + f[2:])), "record", 11))
    cases.append(("seq_and_qual_differ", "sam", with_line(12, b"\t".join(lines[12].split(b"\t")[:10] + [b"IIII\n"])), "record", 13))
    cases.append(("ten_fields", "sam", with_line(29, b"\t".join(lines[29].split(b"\t")[:10])), "record", 30))
    cases.append(("header_line_behind_a_record", "sam", with_line(3, b"@CO\tlate\n"), "record", 4))
    return cases


ERRORS = error_cases()


@pytest.mark.parametrize("case", ERRORS, ids=[c[0] for c in ERRORS])
def test_errors_name_the_place_and_leave_a_reader_that_can_be_freed(case):
    from smalt_amd import api
    label, fmt, data, what, number = case
    for nthreads, window in ((1, None), (3, 64)):
        rd = api.AlnReads(api.IN_SAM if fmt == "sam" else api.IN_BAM)
        try:
            with pytest.raises(api.SmaltGpuError) as e:
                read_runs(None, data, nthreads, window, reader=rd)
            assert e.value.code == EFILE
            msg = str(e.value)
            m = re.search(r"byte offset (\d+)" if what == "offset" else r"record (\d+)", msg)
            assert m and int(m.group(1)) == number, msg
            with pytest.raises(api.SmaltGpuError) as again:                      # a failed reader repeats its error
                rd.take(0)
            assert again.value.code == EFILE
            with pytest.raises(api.SmaltGpuError):
                rd.feed(b"", True)
        finally:
            rd.close()


def test_arguments():
    from smalt_amd import api
    L = api.lib()
    with pytest.raises(api.SmaltGpuError) as e:
        api.AlnReads(3)
    assert e.value.code == EARG
    used, kind, v = C.c_uint64(), C.c_int(), api.ReadsView()
    assert L.smaltgpu_alnreads_feed(None, b"", 0, 1, 1, C.byref(used)) == EARG
    L.smaltgpu_alnreads_free(None)
    rd = api.AlnReads(api.IN_BAM)
    try:
        assert L.smaltgpu_alnreads_feed(rd.h, None, 5, 0, 1, C.byref(used)) == EARG and L.smaltgpu_alnreads_feed(rd.h, b"", 0, 0, 1, None) == EARG
        assert L.smaltgpu_alnreads_take(rd.h, 0, None, C.byref(v), C.byref(v)) == EARG and L.smaltgpu_alnreads_take(rd.h, 0, C.byref(kind), None, C.byref(v)) == EARG
        assert rd.feed(b"", False) == 0 and rd.take()[0] == 0
        good = bw.bam_bytes(small_records(), 300)
        assert rd.feed(good[:10], False) == 0                                    # not one whole member: nothing used
        assert rd.feed(good, True, 0) == len(good)                               # nthreads below 1 counts as 1
        assert rd.take()[1].nreads == 30
        assert all(0 <= t < 5 for t in rd.times()) and rd.times()[0] > 0
        with pytest.raises(api.SmaltGpuError) as e:                              # bytes behind the end
            rd.feed(good, True)
        assert e.value.code == EARG
    finally:
        rd.close()
    # an empty file is no BAM file; an empty SAM file has no reads
    with pytest.raises(api.SmaltGpuError):
        read_runs(api.IN_BAM, b"")
    assert read_runs(api.IN_SAM, b"") == [] and read_runs(api.IN_SAM, bw.HEADER_TEXT) == []
    # a last line without its newline, CR LF, empty lines
    recs = small_records()[:3]
    text = bw.sam_text(recs).replace(b"\n", b"\r\n") + b"\r\n\n"
    assert joined(read_runs(api.IN_SAM, text, 2, 5), 1) == joined(read_runs(api.IN_SAM, text[:-5], 1, 7), 1) == joined(read_runs(api.IN_SAM, bw.sam_text(recs)), 1) == [as_sequenced(r) for r in recs]


# ---- ABI and program -------------------------------------------------------------------------------------------------------------
def test_abi():
    from smalt_amd import api
    header = open(os.path.join(ROOT, "include", "smaltgpu.h")).read()
    so = C.CDLL(os.path.join(ROOT, "smalt_amd", "libsmaltgpu.so"))
    declared = sorted(set(re.findall(r"\b(smaltgpu_alnreads_[a-z_]+)\s*\(", header)))
    assert declared == ["smaltgpu_alnreads_create", "smaltgpu_alnreads_feed", "smaltgpu_alnreads_free", "smaltgpu_alnreads_take", "smaltgpu_alnreads_times"]
    assert all(hasattr(so, name) for name in declared)
    assert re.search(r"^int smaltgpu_alnreads_feed\(smaltgpu_alnreads \*r, const char \*bytes, uint64_t len, int is_last, int nthreads, uint64_t \*consumed\);", header, re.M)
    assert re.search(r"^int smaltgpu_alnreads_take\(smaltgpu_alnreads \*r, uint32_t max_templates, int \*kind, smaltgpu_reads_view \*reads, smaltgpu_reads_view \*mates\);", header, re.M)
    m = re.search(r"SMALTGPU_IN_SAM = (\d+), SMALTGPU_IN_BAM = (\d+)", header)
    assert m and (api.IN_SAM, api.IN_BAM) == (int(m.group(1)), int(m.group(2))) == (1, 2)


def test_program_refuses_bad_input_options_before_any_device_call(tmp_path, monkeypatch):
    prog = os.path.join(ROOT, "smalt_amd", "smaltgpu-map")
    out = str(tmp_path / "never.out")
    r = subprocess.run([prog, "-F", "cram", "-o", out, "/no/such/index", "/no/such/reads.cram"], capture_output=True)
    assert r.returncode == 1 and b"-F" in r.stderr and b"cram" in r.stderr and not r.stdout and not os.path.exists(out)
    for fmt in ("bam", "sam"):
        r = subprocess.run([prog, "-F", fmt, "-o", out, "/no/such/index", "/no/such/a." + fmt, "/no/such/b." + fmt], capture_output=True)
        assert r.returncode == 1 and b"one input file" in r.stderr and not r.stdout and not os.path.exists(out)
    monkeypatch.setenv("SMALTGPU_SERIAL_ORDER", "1")
    r = subprocess.run([prog, "-F", "bam", "-o", out, "/no/such/index", "/no/such/a.bam"], capture_output=True)
    assert r.returncode == 1 and b"SMALTGPU_SERIAL_ORDER" in r.stderr and not os.path.exists(out)
    monkeypatch.delenv("SMALTGPU_SERIAL_ORDER")
    r = subprocess.run([prog], capture_output=True)
    assert r.returncode == 2 and r.stderr.startswith(b"usage: smaltgpu-map [options] <index prefix>") and b"| bam" in r.stderr
    assert b"-F <fmt>" in r.stderr and b"-T <dir>" in r.stderr and b"without effect" in r.stderr
    r = subprocess.run([prog, "sample", "-F", "bam", "/no/such/index", "/no/such/a.bam", "/no/such/b.bam"], capture_output=True)
    assert r.returncode == 2                                                     # `sample` keeps its option list


# ---- smg_alnin.hpp alone, under sanitizers -----------------------------------------------------------------------------------------
def checksum(runs):
    """template by template: kind, whether its run has qualities, names, bases, qualities -- what tests/hostemu/alnin_check.cpp prints"""
    crc, n = 0, 0
    for kind, v, m in runs:
        sides = [reads_of(v)] + ([reads_of(m)] if kind == 2 else [])
        for i in range(v[0]):
            crc = zlib.crc32(struct.pack("<II", kind, v[1]), crc)
            for side in sides:
                name, bases, quals = side[i]
                crc = zlib.crc32(name + b"\0" + bases + (quals if quals is not None else b""), crc)
            n += 1
    return n, crc


def test_decoder_alone_under_sanitizers(fixtures, tmp_path):
    """tests/hostemu/alnin_check.cpp includes smg_alnin.hpp and nothing else of the library.  Built with -fsanitize=address,undefined (the
    runtimes linked into the program itself) it decodes the files of the groups above and prints a checksum of what it got, which must
    be the library's; it runs every error file and every prefix of a small BAM file: errors or clean results, never a sanitizer report."""
    from smalt_amd import api
    exe = str(tmp_path / "alnin_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe,
                    os.path.join(ROOT, "tests", "hostemu", "alnin_check.cpp"), "-lz"], check=True)
    jobs, want = [], []

    def job(tag, fmt, data, nthreads, window, max_templates):
        path = str(tmp_path / ("%03d_%s.%s" % (len(jobs), tag, fmt)))
        open(path, "wb").write(data)
        jobs.append("%s %s %d %d %d" % (fmt, path, nthreads, window, max_templates))
        f = api.IN_SAM if fmt == "sam" else api.IN_BAM
        try:
            want.append("ok %d %08x" % checksum(read_runs(f, data, nthreads, window or None, max_templates)))
        except api.SmaltGpuError as e:
            want.append("error %s" % str(e).split(": ", 1)[-1])
    for fmt in ("sam", "bam"):
        f = api.IN_SAM if fmt == "sam" else api.IN_BAM
        for nthreads, window, payload, max_templates, level, eof in ((1, 0, 0xff00, 0, 6, True), (3, 37, 300, 7, 0, False), (7, 0, 1, 1, 6, True)):
            job("singles", fmt, encoded(f, fixtures["singles"], payload, level, eof), nthreads, window, max_templates)
            job("pairs", fmt, encoded(f, fixtures["pairs"], payload, level, eof), nthreads, window, max_templates)
        job("strands", fmt, encoded(f, strand_records()[:7], 5), 2, 0, 0)
        job("strands_noqual", fmt, encoded(f, strand_records(), 300), 1, 11, 3)
        job("collation", fmt, encoded(f, COLLATION, 17), 3, 0, 0)
        job("collation_cut", fmt, encoded(f, COLLATION, 300), 2, 50, 2)
    job("sam_letters", "sam", bw.sam_text(SAM_LETTERS, header=False), 1, 0, 0)
    for label, fmt, data, what, number in ERRORS:
        job(label, fmt, data, 3, 0, 0)
        job(label + "_w", fmt, data, 1, 64, 0)
    manifest = str(tmp_path / "jobs.txt")
    open(manifest, "w").write("\n".join(jobs) + "\n")
    small = str(tmp_path / "small.bam")
    data = bw.bam_bytes(COLLATION[:20], 150, 0)
    assert 1500 < len(data) < 3500
    open(small, "wb").write(data)
    r = subprocess.run([exe, manifest, small], capture_output=True)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
    lines = r.stdout.decode().splitlines()
    got = [ln.split(" ", 1)[1] for ln in lines if ln.startswith("job ")]
    assert len(got) == len(jobs) and sum(1 for w in want if w.startswith("error")) == 2 * len(ERRORS)
    for g, w, j in zip(got, want, jobs):
        assert g == w, (j, g, w)
    m = re.search(r"prefixes: (\d+) cut, (\d+) clean, (\d+) errors", r.stdout.decode())
    assert m and int(m.group(1)) == len(data) == int(m.group(2)) + int(m.group(3)) and int(m.group(2)) >= 1 and int(m.group(3)) > len(data) // 2

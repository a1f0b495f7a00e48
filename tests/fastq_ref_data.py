"""Shared by the tests of the FASTQ-format reference reader (CPU: test_fastq_ref_model.py, GPU: test_gpu_fastq_ref.py): the
committed texts with what the reference made of them (tests/golden/make_golden_fastq_ref.py), a plain Python walk over the records
by the reference's rules (smalt_amd/csrc/smg_fastq_ref.hpp states them), and texts made for the tests: chosen bytes on chosen
offsets of 64-byte blocks, a random reference re-dressed as wrapped FASTQ."""
import gzip
import json
import os

import numpy as np

import fasta_data as fd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_fastq_ref.json")))
ACCEPTED = [e for e in MANIFEST if e["ref_status"] == 0]
REFUSED = [e for e in MANIFEST if e["ref_status"] != 0]
WRONG = "wrong FASTQ/FASTA format"
WS = fd.WS
PROMPTS = b">@+"


def text_of(entry):
    with gzip.open(os.path.join(GOLD, entry["file"]), "rb") as g:
        return g.read()


def _clean_name(line):
    nm, was_space = bytearray(), True
    for b in line:
        sp = bytes([b]) in WS
        if was_space and sp:
            continue
        was_space = sp
        nm.append(b)
    if was_space and nm:
        nm.pop()
    return bytes(nm).decode("latin-1")


def _read_data(text, i, minlen):
    """readSeqFast from offset i (directly behind a header line): -> (bytes counted, offset of the prompt that ended them or len)"""
    out, was_newline, n = bytearray(), False, len(text)
    while i < n:
        c = text[i:i + 1]
        if c in WS:
            was_newline = c == b"\n"
        else:
            if was_newline and len(out) >= minlen and c in PROMPTS:
                return bytes(out), i
            was_newline = False
            out += c
        i += 1
    return bytes(out), n


def parse_model_fq(text):
    """The reference's reader (seqFastqRead sequence.c:1960-1990) over a whole text, record by record.
    -> (names, sequences); ValueError("wrong FASTQ/FASTA format ...") for a text it refuses."""
    names, seqs = [], []
    n, i = len(text), 0
    while i < n and text[i:i + 1] in WS:
        i += 1
    if i < n and text[i:i + 1] not in PROMPTS:
        raise ValueError(WRONG + ": no prompt")
    while i < n:
        prompt = text[i:i + 1]
        e = text.find(b"\n", i + 1)
        line, d0 = (text[i + 1:], n) if e < 0 else (text[i + 1:e], e + 1)
        data, q = _read_data(text, d0, 0)
        i = q
        if prompt == b"+":
            continue
        names.append(_clean_name(line))
        seqs.append(data)
        if q < n and text[q:q + 1] == b"+":
            e = text.find(b"\n", q + 1)
            qual, i = _read_data(text, n if e < 0 else e + 1, len(data))
            if len(qual) != len(data):
                raise ValueError("%s: record '%s' has %d quality characters for %d bases" % (WRONG, names[-1], len(qual), len(data)))
    return names, seqs


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


QUAL = bytes(range(33, 127))


def placed_texts(block=64):
    """{tag: text}: FASTQ texts of three records in which a chosen byte of the SECOND record is the LAST (tag ..._last) or the FIRST
    (..._first) byte of a block of `block` bytes.  The bytes: the one with which the quality section reaches n, the '\\n' in front
    of the '+' prompt, the '+' itself, the '\\n' of the quality header line, a quality line's leading '@'.  Plus a one-line
    quality longer than five blocks, one longer than 128 blocks, 300 quality lines that begin with '@', and a text whose last byte
    is the one that reaches n."""
    rng = np.random.default_rng(4711)
    t = {}

    def record(name, seq, qual_lines, plus=b"+"):
        return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + b"\n".join(qual_lines) + b"\n"

    first = record(b"first one", _rand(rng, 61), [_rand(rng, 61, QUAL[1:30])])
    tail = record(b"tail", _rand(rng, 70), [_rand(rng, 70, QUAL[40:60])]) + b">fa\n" + _rand(rng, 33) + b"\n"

    def place(tag, build, where):
        """build(pad) -> (text of the second record, offset in it of the byte of interest); pad: bases added to its sequence"""
        for pad in range(0, 4 * block):
            rec2, off = build(pad)
            at = len(first) + off
            if (at + 1) % block == 0 and where == "last" or at % block == 0 and where == "first":
                t["%s_%s" % (tag, where)] = first + rec2 + tail
                return
        raise AssertionError(tag)

    def hdr(pad):                         # with n = 40 + pad // 2 the offsets behind it take every value
        return b"@second " + b"x" * (1 + pad % 2) + b"\n", 40 + pad // 2

    def build_reach(pad):                 # the byte with which the quality reaches n: the last one of a two-line quality
        h, n = hdr(pad)
        q = _rand(np.random.default_rng(pad), n, QUAL[1:30])
        r = h + _rand(np.random.default_rng(pad + 1), n) + b"\n+\n" + q[:17] + b"\n" + q[17:] + b"\n"
        return r, len(r) - 2

    def build_nl_before_plus(pad):
        h, n = hdr(pad)
        head = h + _rand(np.random.default_rng(pad), n)
        return head + b"\n+\n" + _rand(np.random.default_rng(pad + 1), n, QUAL[1:30]) + b"\n", len(head)

    def build_plus(pad):
        r, off = build_nl_before_plus(pad)
        return r, off + 1

    def build_qual_header_nl(pad):
        h, n = hdr(pad)
        head = h + _rand(np.random.default_rng(pad), n) + b"\n+second x"
        return head + b"\n" + _rand(np.random.default_rng(pad + 1), n, QUAL[1:30]) + b"\n", len(head)

    def build_qual_at(pad):               # a quality line that begins with '@', behind a first quality line
        h, n = hdr(pad)
        q = _rand(np.random.default_rng(pad), n, QUAL[1:30])
        head = h + _rand(np.random.default_rng(pad + 1), n) + b"\n+\n" + q[:13] + b"\n"
        return head + b"@" + q[14:] + b"\n", len(head)

    for where in ("last", "first"):
        place("reach_n", build_reach, where)
        place("nl_before_plus", build_nl_before_plus, where)
        place("plus", build_plus, where)
        place("qual_header_nl", build_qual_header_nl, where)
        place("qual_line_at", build_qual_at, where)
    n = 5 * block + 37
    t["long_quality_line"] = first + record(b"second", _rand(rng, n), [b"@" + _rand(rng, n - 1, QUAL)]) + tail
    # searches that cut their range more than once: a quality of more than 128 blocks, more than 128 lines that begin with a prompt
    n = 130 * block + 5
    t["quality_of_many_blocks"] = first + record(b"second", _rand(rng, n), [_rand(rng, n, QUAL)]) + tail
    t["many_prompt_lines"] = first + record(b"second", _rand(rng, 900), [b"@" + _rand(rng, 2, QUAL[40:60]) for _ in range(300)]) + tail
    last = record(b"last", _rand(rng, 50), [_rand(rng, 50, QUAL[1:30])])
    t["reach_n_ends_text"] = first + tail + last[:-1]
    return t


def wrapped_fastq(seed, total=200_000):
    """fasta_data.dressed_reference(seed) re-dressed as FASTQ: sequence and quality wrapped at random widths, random quality
    characters with '@', '+' and '>' at line starts, CRLF on some lines, a blank line here and there.
    -> (text, names, sequences)"""
    _, names, seqs = fd.dressed_reference(seed, total)
    rng = np.random.default_rng(seed + 1000)
    out = bytearray()
    for nm, sq in zip(names, seqs):
        n = len(sq)
        eol = b"\r\n" if rng.random() < 0.3 else b"\n"
        out += b"@" + nm.encode("latin-1") + eol
        width = int(rng.integers(20, 200))
        for o in range(0, n, width):
            out += sq[o:o + width] + eol
        out += b"+" + (nm.encode("latin-1") if rng.random() < 0.5 else b"") + eol
        q = bytearray(_rand(rng, n, QUAL))
        width = int(rng.integers(20, 200))
        for o in range(0, n, width):
            if rng.random() < 0.3:
                q[o] = PROMPTS[int(rng.integers(0, 3))]
            out += bytes(q[o:o + width]) + eol
            if rng.random() < 0.02:
                out += b"\n"
    text = bytes(out)
    got = parse_model_fq(text)
    assert got == (names, seqs)
    return text, names, seqs

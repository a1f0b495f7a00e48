"""Shared by the FASTA-reader tests (CPU: test_fasta_parse.py, GPU: test_gpu_fasta_index.py): the committed texts with what the
reference made of them (tests/golden/make_golden_fasta.py), a plain Python statement of the reader's automaton, and texts made
for the tests: block boundaries placed by construction, random references in random dresses."""
import gzip
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest_fasta.json")))
ACCEPTED = [e for e in MANIFEST if e["expect"] == "ok"]
REFUSED = [e for e in MANIFEST if e["expect"] != "ok"]
# the cause a refusal has to name
CAUSE = {"nohead": "does not begin with a '>' prompt", "short": "shorter than the word length", "fastq": "FASTQ-format reference files are not supported"}
WS = b" \t\n\v\f\r"


def text_of(entry):
    with gzip.open(os.path.join(GOLD, entry["file"]), "rb") as g:
        return g.read()


def parse_model(text):
    """The reference's reader (readHeader sequence.c:1056-1146, readSeqFast :1229-1304) over a whole text, one byte at a time.
    -> (names, sequences); ValueError for a text without a prompt at its start."""
    names, seqs = [], []
    state, i, n = "P", 0, len(text)
    while i < n:
        c = text[i:i + 1]
        if state == "P":
            if c not in WS:
                if c not in b">@+":
                    raise ValueError("wrong format")
                state = "H"
                hdr = bytearray()
        elif state == "H":
            if c == b"\n":
                state = "S0"
            else:
                hdr += c
            if state == "S0" or i + 1 == n:
                nm, was_space = bytearray(), True
                for b in bytes(hdr):
                    sp = bytes([b]) in WS
                    if was_space and sp:
                        continue
                    was_space = sp
                    nm.append(b)
                if was_space and nm:
                    nm.pop()
                names.append(bytes(nm).decode("latin-1"))
                seqs.append(bytearray())
        else:
            if c == b"\n":
                state = "S1"
            elif c in WS:
                state = "S0"
            elif state == "S1" and c in b">@+":
                state = "H"
                hdr = bytearray()
            else:
                seqs[-1] += c
                state = "S0"
        i += 1
    return names, [bytes(s) for s in seqs]


def _rand_bases(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)])


def boundary_texts(block=64):
    """Texts in which a chosen byte is the LAST byte of a block of `block` bytes: {tag: text}.  Every text also has sequences long
    enough for a word length of 11 and a third record behind the place of interest."""
    rng = np.random.default_rng(99)
    tail = b">tail\n" + _rand_bases(rng, 70) + b"\n" + _rand_bases(rng, 33) + b"\n"

    def upto(prefix, last):
        """prefix + one line of bases + last, so that the final byte of `last` stands at offset k * block - 1"""
        need = (-(len(prefix) + len(last) + 1)) % block + 1          # bases incl. none of the line ends: at least 1
        if need < 20:
            need += block
        t = prefix + _rand_bases(rng, need) + last
        assert len(t) % block == 0
        return t

    head = b">first one\n" + _rand_bases(rng, 61) + b"\n"
    t = {}
    t["newline_then_prompt"] = upto(head, b"\n") + b">second\n" + _rand_bases(rng, 90) + b"\n" + tail
    t["cr_of_crlf"] = upto(head, b"\r") + b"\n>second\r\n" + _rand_bases(rng, 90) + b"\r\n" + tail
    t["prompt_itself"] = upto(head, b"\n>") + b"second\n" + _rand_bases(rng, 90) + b"\n" + tail
    t["header_last_byte"] = upto(head, b"\n>second x") + b"\n" + _rand_bases(rng, 90) + b"\n" + tail
    t["header_newline"] = upto(head, b"\n>second x\n") + _rand_bases(rng, 90) + b"\n" + tail
    t["newline_then_blank_prompt"] = upto(head, b"\n") + b" >nothead\n" + _rand_bases(rng, 90) + b"\n" + tail
    t["header_then_header"] = upto(head, b"\n>second\n") + b">bases\n" + _rand_bases(rng, 90) + b"\n" + tail
    t["long_header"] = head + b">second " + b"word  " * (3 * block // 6 + 9) + b"\n" + _rand_bases(rng, 90) + b"\n" + tail
    t["long_line"] = head + b">second\n" + _rand_bases(rng, 5 * block + 37) + b"\n" + tail
    t["leading_space"] = b" \n" * (block + 5) + head + tail               # more than a block of white space ahead of the first prompt
    return t


def dressed_reference(seed, total=200_000):
    """A random reference (runs of N, IUPAC letters, lower case, as tests/test_gpu_indexbuild._messy_reference) written as FASTA
    with random line widths, CRLF on some lines, blank lines and descriptions.  -> (text, names, sequences)"""
    rng = np.random.default_rng(seed)
    seqs, out = [], bytearray()
    left = total
    while left > 0:
        n = int(rng.integers(400, 40_000))
        left -= n
        a = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
        for _ in range(int(rng.integers(0, 4))):
            p = int(rng.integers(0, n - 50))
            a[p:p + int(rng.integers(1, 300))] = ord("N")
        for _ in range(10):
            a[int(rng.integers(0, n))] = ord("RYKMSWU"[int(rng.integers(0, 7))])
        a[rng.random(n) < 0.2] |= 0x20
        sq = a.tobytes()
        nm = "seq%d" % len(seqs) + (" description  of %d\twith a tab" % len(seqs) if rng.random() < 0.4 else "")
        seqs.append(sq)
        crlf = rng.random() < 0.3
        out += b">" + nm.encode() + (b"\r\n" if crlf else b"\n")
        width = int(rng.integers(1, 200)) if rng.random() < 0.8 else n
        for o in range(0, n, width):
            out += sq[o:o + width] + (b"\r\n" if crlf and rng.random() < 0.7 else b"\n")
            if rng.random() < 0.02:
                out += b"\n"
    names, model_seqs = parse_model(bytes(out))         # the names as the reader cleans them
    assert model_seqs == seqs
    return bytes(out), names, seqs

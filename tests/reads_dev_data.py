"""Read files for the device parser (smalt_amd/csrc/smg_reads_dev.hpp), built in Python as small byte strings and shared by the CPU
tests (tests/test_reads_dev_model.py) and the GPU tests (tests/test_gpu_reads_dev.py).

The authority is smaltgpu_reads_parse (host code, called through ctypes: no GPU): host_line() prints its result in the form
tests/hostemu/reads_dev_check.cpp prints its own, view_line() does the same for any view.  Every case of CORPUS names the rule it
is there for as a predicate over the host parser's result; check_case() asserts it."""
import ctypes as C
import random
import struct

from smalt_amd import api

FA_TILE = 4096           # smg_fasta.hpp
GRAN = 64                # FQ_GRAN
REC_PER_TILE = FA_TILE // 2
BLOCK = 8192             # the bytes per block the placed cases are built around (a multiple of FA_TILE; the tests set it)
E_NOPROMPT = "not in FASTA/FASTQ format (a header line was expected)"
E_QLEN = "sequence and quality string differ in length (read '%s')"
EFILE = -2


def _hex(b):
    return b.hex() if b else "-"


def view_line(v):
    """a filled ReadsView in the form of reads_dev_check"""
    n = v.nreads
    off = [v.read_off[i] for i in range(n + 1)]
    nb = off[n]
    bases = C.string_at(v.bases, nb) if nb else b""
    quals = C.string_at(v.quals, nb) if (v.has_qual and nb) else b""
    names = C.string_at(v.names, v.name_off[n]) if n else b""
    return "OK %d %d %d %s %s %s %s" % (n, v.has_qual, v.consumed, _hex(bases), _hex(quals) if v.has_qual else "-", ",".join(map(str, off)), _hex(names))


_host = []


def host_line(text, is_last=True, max_reads=0, nthreads=1, general=True):
    """smaltgpu_reads_parse on the text -> (line, consumed).

    general: the text is handed over behind one '\\n' and `consumed` is counted back.  A text whose first byte is '@' is otherwise
    tried on the host parser's four-line path (strict_record) first, which leaves a last record of fewer than four lines where it
    is -- with is_last too -- while general_parse, the rules the device parser restates, takes what the reference's reader takes.
    Leading white space changes nothing else: general_parse skips it in front of the first prompt."""
    L = api.lib()
    if not _host:
        _host.append(L.smaltgpu_reads_create())
    v = api.ReadsView()
    buf = b"\n" + text if general else text
    rv = L.smaltgpu_reads_parse(_host[0], buf, len(buf), 1 if is_last else 0, max_reads, nthreads, C.byref(v))
    if rv:
        assert rv == EFILE, rv
        return "ERR " + L.smaltgpu_last_error().decode("latin-1"), 0
    if general and v.consumed:
        v.consumed -= 1
    return view_line(v), v.consumed


def parse_line(line):
    """-> dict(nreads, has_qual, consumed, reads, quals, names) or dict(error)"""
    if line.startswith("ERR "):
        return dict(error=line[4:])
    f = line.split(" ")
    assert f[0] == "OK" and len(f) == 8, line
    off = [int(x) for x in f[6].split(",")]
    un = lambda s: b"" if s == "-" else bytes.fromhex(s)
    bases, quals, names = un(f[4]), un(f[5]), un(f[7])
    n = int(f[1])
    return dict(nreads=n, has_qual=int(f[2]), consumed=int(f[3]), reads=[bases[off[i]:off[i + 1]] for i in range(n)],
                quals=[quals[off[i]:off[i + 1]] for i in range(n)] if int(f[2]) else None, names=names.split(b"\0")[:-1] if n else [], error=None)


def case_record(text, mode=0, is_last=True, max_reads=0):
    """one case of the case file of reads_dev_check"""
    return struct.pack("<IBBI", len(text), mode, 1 if is_last else 0, max_reads) + text


def wrap(s, w):
    return b"".join(s[i:i + w] + b"\n" for i in range(0, len(s), w)) if s else b"\n"


def fastq(recs, w=0, nl=b"\n"):
    out = []
    for name, seq, qual in recs:
        body = b"@" + name + b"\n" + (wrap(seq, w) if w else seq + b"\n") + b"+\n" + (wrap(qual, w) if w else qual + b"\n")
        out.append(body.replace(b"\n", nl))
    return b"".join(out)


def fasta(recs, w=0):
    return b"".join(b">" + name + b"\n" + (wrap(seq, w) if w else seq + b"\n") for name, seq in recs)


def _seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _qual(rng, n, first=None):
    q = bytearray(rng.choice(b"#+5?I@>") for _ in range(n))
    if first is not None and n:
        q[0] = first
    return bytes(q)


def _recs(seed, n, lo, hi):
    rng = random.Random(seed)
    return [(b"r%d" % i, _seq(rng, ln), _qual(rng, ln)) for i, ln in ((i, rng.randint(lo, hi)) for i in range(n))]


def placed(seed, where, what):
    """a FASTQ text in which byte `what` of record 2 lies at offset `where`: 'prompt' (the record's '@'), 'hdr_nl' (the '\\n' of its
    header), 'reach' (the last quality character: the byte that reaches n) or 'end' (the '\\n' behind the quality line)"""
    rng = random.Random(seed)
    small = where < 200                                    # in front of the first granule boundary there is room for less
    head = fastq([(b"a", _seq(rng, 3), _qual(rng, 3, ord("@")))] if small else [(b"a", _seq(rng, 30), _qual(rng, 30, ord("@"))), (b"b", _seq(rng, 41), _qual(rng, 41))])
    n = 10 if small else 50
    rel = {"prompt": 0, "hdr_nl": 3, "reach": 4 + n + 1 + 2 + n - 1, "end": 4 + n + 1 + 2 + n}[what]
    pad = where - rel - len(head) - 4                      # a FASTA record ">p\n" + pad bases + "\n" in front
    assert pad >= 0
    text = head + b">p\n" + _seq(rng, pad) + b"\n" + fastq([(b"cc", _seq(rng, n), _qual(rng, n)), (b"d", _seq(rng, 9), _qual(rng, 9, ord("+")))])
    key = {"prompt": b"@", "hdr_nl": b"\n", "end": b"\n"}.get(what)
    assert key is None or text[where:where + 1] == key, (what, where)
    return text


# ---- the corpus: tag -> (text, is_last, predicate over parse_line(host result), the rule) --------------------------------------
def _names(*want):
    return lambda r: r["error"] is None and r["names"] == list(want)


def _build():
    rng = random.Random(20240611)
    c = {}
    four = _recs(1, 12, 20, 90)
    c["four_line"] = (fastq(four), True, lambda r: r["nreads"] == 12 and r["has_qual"] == 1 and r["reads"] == [s for _, s, _ in four] and r["quals"] == [q for _, _, q in four],
                      "plain four-line FASTQ")
    long_ = [(b"w%d" % i, _seq(rng, ln), _qual(rng, ln)) for i, ln in enumerate((1, 6, 7, 8, 59, 60, 61, 150, 333))]
    for w in (7, 60):
        c["wrapped_%d" % w] = (fastq(long_, w), True, lambda r: r["reads"] == [s for _, s, _ in long_] and r["quals"] == [q for _, _, q in long_] and r["has_qual"] == 1,
                               "sequence and quality lines wrapped at %d columns" % w)
    fa = [(b"f%d x y" % i, _seq(rng, ln)) for i, ln in enumerate((5, 60, 61, 200))]
    c["fasta_wrapped"] = (fasta(fa, 60), True, lambda r: r["has_qual"] == 0 and r["quals"] is None and r["reads"] == [s for _, s in fa], "FASTA, wrapped at 60 columns")
    c["fasta_one_line"] = (fasta(fa), True, lambda r: r["has_qual"] == 0 and r["reads"] == [s for _, s in fa] and r["names"] == [b"f%d" % i for i in range(4)], "FASTA on one line")
    c["mixed"] = (fastq(four[:3]) + fasta(fa[:1]) + fastq(four[3:5]), True, lambda r: r["nreads"] == 6 and r["has_qual"] == 0 and r["quals"] is None,
                  "one FASTA record among FASTQ records: no qualities for the block")
    c["crlf"] = (fastq(four[:4], nl=b"\r\n"), True, lambda r: r["reads"] == [s for _, s, _ in four[:4]] and r["names"] == [b"r0", b"r1", b"r2", b"r3"], "CRLF line ends")
    c["blank_lines"] = (b"\n\n@a\n\nAC\n\nGT\n+\n\nII\nII\n\n\n@b\nA\n \n+\nI\n\n", True, lambda r: r["reads"] == [b"ACGT", b"A"] and r["quals"] == [b"IIII", b"I"],
                        "blank lines between and inside records")
    c["no_final_newline"] = (b"@a\nACGT\n+\nIIII\n@b\nAC\n+\nII", True, lambda r: r["reads"] == [b"ACGT", b"AC"] and r["consumed"] == 25, "no newline at the end")
    c["no_final_newline_fasta"] = (b">a\nACGT\n>b\nAC", True, lambda r: r["reads"] == [b"ACGT", b"AC"] and r["has_qual"] == 0, "FASTA without a newline at the end")
    letters = b"acgtnRYKMSWBDHVUu019-*.[_`{\x80"
    c["letters"] = (b"@l\n" + letters + b"\n+\n" + b"I" * len(letters) + b"\n", True,
                    lambda r: r["reads"] == [b"ACGTNRYKMSWBDHVTTNNNNNN[_NNN"], "lower case, IUPAC letters, U, digits and '-' as bases")
    c["header_no_name"] = (b"@\nAC\n+\nII\n@ \t x y\nG\n+\nI\n> \nT\n", True, lambda r: r["names"] == [b"", b"x", b""] and r["has_qual"] == 0, "headers without a name")
    c["header_words"] = (b"@name one two\tthree\nAC\n+name again\nII\n", True, _names(b"name"), "a header of several words")
    c["empty_read"] = (b"@e\n\n+\n\n@f\nAC\n+\nII\n>g\n\n>h\nA\n", True, lambda r: r["reads"] == [b"", b"AC", b"", b"A"] and r["names"] == [b"e", b"f", b"g", b"h"], "reads of no bases")
    c["qual_prompt_lines"] = (b"@a\nACGTAC\nGTACGT\n+\n@IIIII\n+IIIII\n@b\nACGTAC\n+\n>IIII\nI\n@c\nA\n+\n@\n", True,
                              lambda r: r["quals"] == [b"@IIIII+IIIII", b">IIIII", b"@"] and r["names"] == [b"a", b"b", b"c"],
                              "quality lines that begin with '@', '+' or '>' before the section has reached n")
    every = [(b"q%d" % i, _seq(rng, 3 * 9), b"".join(b"@" + _qual(rng, 8) for _ in range(3))) for i in range(40)]
    c["every_qual_line_at"] = (fastq(every, 9), True, lambda r: r["nreads"] == 40 and r["quals"] == [q for _, _, q in every], "every quality line begins with '@': most candidates are no records")
    c["stray_plus"] = (b"+stray\nIIII\n+more\nKK\n@a\nAC\n+\nII\n+between\nJJJJ\nJJ\n@b\nG\n+\nI\n+last\nKK\n", True, lambda r: r["names"] == [b"a", b"b"] and r["reads"] == [b"AC", b"G"] and r["quals"] == [b"II", b"I"] and r["consumed"] == 67,
                       "stray '+' segments in front of the first record, between records and at the end")
    c["only_plus"] = (b"+x\nII\n+y\nJJ\n", True, lambda r: r["error"] is None and r["nreads"] == 0 and r["consumed"] == 12, "nothing but '+' segments: no reads, no error")
    c["blank_only"] = (b" \n\t\r\n\n", True, lambda r: r["error"] is None and r["nreads"] == 0 and r["consumed"] == 6, "white space only")
    c["header_ends_text"] = (b"@a\nAC\n+\nII\n@last", True, lambda r: r["names"] == [b"a", b"last"] and r["reads"] == [b"AC", b""] and r["has_qual"] == 0, "a header line that ends the text")
    c["plus_ends_text"] = (b"@a\nAC\n+", True, lambda r: r["error"] == E_QLEN % "a", "a quality header that ends the text")
    c["space_before_first"] = (b" \n  @a\nAC\n+\nII\n", True, _names(b"a"), "white space in front of the first prompt, which is not behind a newline")
    c["err_noprompt"] = (b"\n  ACGT\n@a\nAC\n+\nII\n", True, lambda r: r["error"] == E_NOPROMPT, "first non-blank byte not a prompt")
    c["err_qual_short"] = (b"@a\nACGT\n+\nIIII\n@bb x\nACGT\n+\nIII\n@c\nA\n+\nI\n", True, lambda r: r["error"] == E_QLEN % "bb", "a quality section one character short: it takes the next record in")
    c["err_qual_long"] = (b"@a\nACGT\n+\nIIIII\n@c\nA\n+\nI\n", True, lambda r: r["error"] == E_QLEN % "a", "a quality section one character long")
    c["err_qual_short_at_end"] = (b"@a\nACGT\n+\nIIII\n@z\nACGT\n+\nIII\n", True, lambda r: r["error"] == E_QLEN % "z", "a quality section short at the end of the text")
    c["short_at_end_not_last"] = (b"@a\nACGT\n+\nIIII\n@z\nACGT\n+\nIII\n", False, lambda r: r["error"] is None and r["names"] == [b"a"] and r["consumed"] == 15,
                                  "the same text as a chunk: the record is left for the next call")
    c["fasta_not_last"] = (b">a\nAC\n>b\nGT\n", False, lambda r: r["names"] == [b"a"] and r["consumed"] == 6, "a FASTA record that no prompt follows is left for the next call")
    # placement against the layout constants
    for where in (GRAN, FA_TILE, BLOCK):
        for d in (-1, 0, 1):
            for what in ("prompt", "hdr_nl", "reach", "end"):
                t = placed(where + d, where + d, what)
                c["placed_%s_%d%+d" % (what, where, d)] = (t, True, lambda r: r["nreads"] in (4, 5) and r["names"][-2:] == [b"cc", b"d"] and len(r["reads"][-2]) in (10, 50) and len(r["reads"][-1]) == 9 and r["has_qual"] == 0,
                                                          "%s of a record at byte %d%+d" % (what, where, d))
    tiny = [(b"", _seq(rng, 1 + i % 2), _qual(rng, 1 + i % 2, ord("@") if i % 5 == 0 else None)) for i in range(2 * REC_PER_TILE // 3)]
    tt = b"".join(b"@\n" + s + b"\n+\n" + q + b"\n" for _, s, q in tiny)
    c["tiny_reads"] = (tt, True, lambda r: r["nreads"] == len(tiny) and r["reads"] == [s for _, s, _ in tiny] and r["quals"] == [q for _, _, q in tiny],
                       "reads of 1-2 bases: more records than FQ_REC_PER_TILE / 3 begin in a tile, with two candidates each")
    return c


CORPUS = _build()


def check_case(tag):
    text, is_last, pred, rule = CORPUS[tag]
    line, _ = host_line(text, is_last)
    try:
        ok = pred(parse_line(line))
    except (KeyError, TypeError, IndexError):          # an error where reads were expected, or the other way round
        ok = False
    assert ok, (tag, rule, line[:300])


def deep_text(n=70_000):
    """n two-base reads: the path through the candidates is 2 n long, the doubling needs more than 16 levels"""
    return b"".join(b"@%x\nAC\n+\n@I\n" % i for i in range(n))


ALPHABET = [b"@", b"+", b">", b"\n", b"\r", b" ", b"A", b"c", b"N", b"I"]


def random_texts(n=2000, seed=7, maxlen=200):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ln = rng.randint(0, maxlen) if i % 4 else rng.randint(0, 24)
        w = [3 if i % 3 == 0 else 1, 3, 1, 6 if i % 2 else 3, 1, 1, 5, 3, 2, 5]          # more newlines: more records
        out.append(b"".join(rng.choices(ALPHABET, weights=w, k=ln)))
    return out


def chunk_calls(parse, text, chunk):
    """The chunk protocol: windows of `chunk` bytes from where the last call stopped, a window that yields nothing grows by `chunk`.
    parse(buffer, is_last) -> (line, consumed); -> the lines of all calls"""
    pos, win, lines = 0, chunk, []
    while True:
        end = min(pos + win, len(text))
        last = end == len(text)
        line, used = parse(text[pos:end], last)
        lines.append(line)
        if last or line.startswith("ERR"):
            return lines
        if used == 0:
            win += chunk
        else:
            pos += used
            win = chunk

"""A SAM and BAM writer for the tests, in pure Python (struct, zlib) and independent of smalt_amd/csrc/smg_alnin.hpp and smg_bam.hpp:
it turns a list of records (name, flag, sequence, qualities) into SAM text or into a BAM file whose BGZF members hold a chosen number
of payload bytes -- so that records span members --, deflated at a chosen level (0: stored), with or without the end-of-file block.

Record: (name: bytes, flag: int, seq: bytes or None for '*', qual: phred+33 bytes or None for none).  Only these four fields matter to
the reader under test; the others are filled in so that they have to be stepped over: a record without flag 0x4 is placed on the first
reference sequence at position 100 with a CIGAR of one M operation (and a soft clip when the read is longer than 3 bases), a record
with 0x4 is unplaced and has no CIGAR."""
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
ALPHABET = "=ACMGRSVTWYHKDBN"
REFS = (("chr1", 100000), ("chr2", 5000))
HEADER_TEXT = b"@HD\tVN:1.4\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), ln) for n, ln in REFS) + b"@CO\ta comment\twith tabs in it, eleven, of, them\t5\t6\t7\t8\t9\t10\t11\t12\n"


def cigar_of(flag, seq):
    """[(length, op)] of a record: none for unplaced reads and reads without sequence"""
    if flag & 0x4 or not seq:
        return []
    return [(2, "S"), (len(seq) - 2, "M")] if len(seq) > 3 else [(len(seq), "M")]


def sam_line(rec):
    name, flag, seq, qual = rec
    ops = cigar_of(flag, seq)
    placed = not flag & 0x4
    fields = [name, b"%d" % flag, REFS[0][0].encode() if placed else b"*", b"100" if placed else b"0", b"37" if placed else b"0",
              "".join("%d%s" % o for o in ops).encode() or b"*", b"*", b"0", b"0", seq if seq else b"*", qual if qual is not None and seq else b"*"]
    if placed:
        fields += [b"NM:i:0", b"AS:i:%d" % len(seq or b"")]
    return b"\t".join(fields) + b"\n"


def sam_text(records, header=True):
    return (HEADER_TEXT if header else b"") + b"".join(sam_line(r) for r in records)


def bam_record(rec, l_read_name=None, block_size=None):
    """one record, block_size included; l_read_name / block_size: values to write instead of the true ones (for the error cases)"""
    name, flag, seq, qual = rec
    seq = seq or b""
    ops = cigar_of(flag, seq)
    placed = not flag & 0x4
    codes = [ALPHABET.index(chr(c).upper()) if chr(c).upper() in ALPHABET else 15 for c in seq]
    if len(codes) & 1:
        codes.append(0)
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(codes), 2))
    quals = bytes(q - 33 for q in qual) if qual is not None else b"\xff" * len(seq)
    assert len(quals) == len(seq)
    tags = b"NMC\0" + b"ASC" + bytes([min(255, len(seq))]) if placed else b""
    body = struct.pack("<iiBBHHHiiii", 0 if placed else -1, 99 if placed else -1, len(name) + 1 if l_read_name is None else l_read_name, 37 if placed else 0,
                       4681 if placed else 4680, len(ops), flag, len(seq), -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", n << 4 | "MIDNSHP=X".index(op)) for n, op in ops) + packed + quals + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def bam_header(text=HEADER_TEXT, refs=REFS):
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, ln in refs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return out


def bgzf_member(payload, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    data = c.compress(payload) + c.flush()
    total = 18 + len(data) + 8
    assert total <= 65536
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + data + struct.pack("<II", zlib.crc32(payload), len(payload))


def bgzf(stream, payload=0xff00, level=6, eof=True):
    """the stream cut into members of `payload` bytes each (the last one shorter) -> (bytes, [offset of each member])"""
    out, offs = bytearray(), []
    for at in range(0, len(stream), payload):
        offs.append(len(out))
        out += bgzf_member(stream[at:at + payload], level)
    if eof:
        offs.append(len(out))
        out += EOF_BLOCK
    return bytes(out), offs


def bam_stream(records, text=HEADER_TEXT, refs=REFS):
    return bam_header(text, refs) + b"".join(bam_record(r) for r in records)


def bam_bytes(records, payload=0xff00, level=6, eof=True):
    return bgzf(bam_stream(records), payload, level, eof)[0]

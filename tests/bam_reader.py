"""A BAM reader for the tests, in pure Python (gzip, struct, zlib) and independent of smalt_amd/csrc/smg_bam.hpp: it walks the BGZF
members of a file, checks the bytes every member must have, inflates them with the standard library (so CRC32 and ISIZE are
checked by code that is not ours) and decodes header and records into the tuples that `canonical_sam_line` makes of a SAM line.

Record tuple: (qname, flag, rname, pos1, mapq, cigar, rnext, pnext1, tlen, seq, qual, [(tag, type, value)]) -- text fields as
str, positions 1-based as SAM prints them, rname / rnext None for '*', seq None for '*', qual None where the SAM line has '*'."""
import gzip
import struct
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
PAYLOAD_MAX = 0xff00
ALPHABET = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


def bgzf_members(data):
    """-> the payloads of the BGZF members of `data`, every member checked"""
    out, at = [], 0
    while at < len(data):
        head = data[at:at + 18]
        assert len(head) == 18, "truncated member header at %d" % at
        assert head[:4] == b"\x1f\x8b\x08\x04", "gzip magic, deflate, FEXTRA at %d" % at
        assert head[4:8] == b"\0\0\0\0" and head[8] == 0 and head[9] == 0xff, "MTIME 0, XFL 0, OS unknown at %d" % at
        assert head[10:12] == b"\x06\x00" and head[12:14] == b"BC" and head[14:16] == b"\x02\x00", "the BC subfield at %d" % at
        bsize = struct.unpack("<H", head[16:18])[0]
        member = data[at:at + bsize + 1]
        assert len(member) == bsize + 1, "BSIZE runs past the end of the data at %d" % at
        d = zlib.decompressobj(-15)
        payload = d.decompress(member[18:-8])
        assert d.eof and not d.unused_data, "the deflate stream does not fill the member at %d" % at
        crc, isize = struct.unpack("<II", member[-8:])
        assert isize == len(payload) and crc == zlib.crc32(payload), "CRC32 / ISIZE at %d" % at
        assert gzip.decompress(member) == payload            # the standard library's own check of CRC32 and ISIZE
        assert len(payload) <= PAYLOAD_MAX
        out.append(payload)
        at += bsize + 1
    return out


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def decode_records(stream, refs, at=0):
    """the records in stream[at:] -> list of tuples; refs: [(name, length)]"""
    recs = []
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        assert size >= 32 and at + 4 + size <= len(stream), "block_size at %d" % at
        ref_id, pos, l_name, mapq, bin_, n_ops, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", stream, at + 4)
        p = at + 36
        name = stream[p:p + l_name]
        assert l_name >= 2 and name[-1] == 0 and 0 not in name[:-1]
        p += l_name
        ops = struct.unpack_from("<%dI" % n_ops, stream, p)
        p += 4 * n_ops
        cigar = "".join("%d%s" % (v >> 4, CIGAR_OPS[v & 15]) for v in ops) or None
        packed = stream[p:p + (l_seq + 1) // 2]
        p += (l_seq + 1) // 2
        seq = "".join(ALPHABET[b >> 4] + ALPHABET[b & 15] for b in packed)
        if l_seq & 1:
            assert packed[-1] & 15 == 0, "the unused half byte behind an odd-length sequence"
            seq = seq[:-1]
        q = stream[p:p + l_seq]
        p += l_seq
        if l_seq and all(b == 0xff for b in q):
            qual = None
        else:
            qual = "".join(chr(b + 33) for b in q) if l_seq else None
        tags = []
        end = at + 4 + size
        while p < end:
            tag, typ = stream[p:p + 2].decode(), chr(stream[p + 2])
            assert typ == "i", "only int32 fields are written"
            tags.append((tag, typ, struct.unpack_from("<i", stream, p + 3)[0]))
            p += 7
        assert p == end
        assert -1 <= ref_id < len(refs) and -1 <= next_id < len(refs)
        # bin: recomputed from pos and the reference bases the CIGAR consumes
        span = sum(v >> 4 for v in ops if CIGAR_OPS[v & 15] in "MDN=X")
        if pos < 0:
            want_bin = 4680
        else:
            want_bin = reg2bin(pos, pos + (span if span > 0 and not flag & 4 else 1))
        assert bin_ == want_bin, (name, bin_, want_bin)
        recs.append((name[:-1].decode(), flag, refs[ref_id][0] if ref_id >= 0 else None, pos + 1, mapq, cigar, refs[next_id][0] if next_id >= 0 else None,
                     next_pos + 1, tlen, seq if l_seq else None, qual, tags))
        at += 4 + size
    return recs


def decode_header(stream):
    """-> (header text, [(name, length)], offset of the first record)"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        name = stream[at + 4:at + 4 + l_name]
        assert name[-1] == 0
        refs.append((name[:-1].decode(), struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
        at += 8 + l_name
    return text, refs, at


def read_bam(data, need_eof=True):
    """a whole BAM file -> (header text, [(name, length)], records, payload sizes of its members)"""
    if need_eof:
        assert data[-28:] == EOF_BLOCK, "the file does not end with the end-of-file block"
    payloads = bgzf_members(data)
    if need_eof:
        assert payloads[-1] == b""
    stream = b"".join(payloads)
    text, refs, at = decode_header(stream)
    return text, refs, decode_records(stream, refs, at), [len(p) for p in payloads]


def canonical_sam_line(line):
    """a SAM line (str or bytes, no newline) -> the tuple decode_records gives for its record"""
    if isinstance(line, bytes):
        line = line.decode()
    f = line.split("\t")
    rname = None if f[2] == "*" else f[2]
    rnext = None if f[6] == "*" else rname if f[6] == "=" else f[6]
    seq = None if f[9] == "*" else "".join(c if c in ALPHABET else "N" for c in f[9])
    qual = None if f[10] == "*" or seq is None else f[10]
    tags = []
    for t in f[11:]:
        tag, typ, val = t.split(":", 2)
        tags.append((tag, typ, int(val) if typ == "i" else val))
    return (f[0], int(f[1]), rname, int(f[3]), int(f[4]), None if f[5] == "*" else f[5], rnext, int(f[7]), int(f[8]), seq, qual, tags)


def sam_records(text):
    """the alignment lines of a SAM text (bytes) -> tuples; header lines are left out"""
    return [canonical_sam_line(ln) for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]


def sam_header(text, keep_pg=False):
    return [ln for ln in text.split(b"\n") if ln.startswith(b"@") and (keep_pg or not ln.startswith(b"@PG"))]

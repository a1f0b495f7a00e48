// smg_bam.hpp -- BAM output (smalt map -f bam) without a BAM library: the record and header layout of the SAM/BAM
// specification, and BGZF, which is a series of gzip members with a 6-byte extra field (zlib does the deflate).
//
// A BAM record is DEFINED here by the SAM line the report prints for the same alignment: record_of_sam_line() turns that line
// into the binary record, so which alignments are reported, their flags, mate fields, clipping, CIGAR, NM and AS are the SAM
// path's and are stated nowhere else.  The two numbers a line does not hold -- the indices of RNAME and RNEXT in the header's
// sequence list -- come from the caller, who knows them where it prints the names.
//
// Pure host C++ over zlib: no HIP header and nothing of the library, so that a stand-alone program can include this file
// (tests/hostemu/bam_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <thread>
#include <vector>

namespace smgbam {

enum { PAYLOAD_MAX = 0xff00,          // uncompressed bytes of one BGZF block (what htslib cuts at; < 64 KiB so that a stored block fits BSIZE)
       QNAME_MAX = 254,               // l_read_name is one byte and counts the NUL
       CIGAR_OPS_MAX = 65535,         // n_cigar_op is 16 bits wide (the CG tag for longer ones is not built)
       BIN_UNPLACED = 4680 };         // reg2bin(-1, 0)
enum { OK = 0, MALFORMED = 1, NAME_TOO_LONG = 2, TOO_MANY_OPS = 3 };

// the 28 bytes that end a BAM file: an empty BGZF block
static const unsigned char END_OF_FILE[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 'B', 'C', 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

inline void put16(std::string &o, uint32_t v) { o.push_back((char)(v & 0xff)); o.push_back((char)((v >> 8) & 0xff)); }
inline void put32(std::string &o, uint32_t v) { put16(o, v & 0xffffu); put16(o, v >> 16); }
inline void set32(std::string &o, size_t at, uint32_t v) { for (int k = 0; k < 4; k++) o[at + (size_t)k] = (char)((v >> (8 * k)) & 0xff); }

// bin of the half-open interval [beg, end) (SAM specification, section 5.3)
inline uint32_t reg2bin(int64_t beg, int64_t end) {
  --end;
  if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
  if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
  if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
  if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
  if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
  return 0;
}

// 4-bit code of a sequence letter: its place in "=ACMGRSVTWYHKDBN", any other letter reads as N
inline uint8_t base_code(unsigned char c) {
  static const char ALPHABET[] = "=ACMGRSVTWYHKDBN";
  const char *p = c ? (const char *)memchr(ALPHABET, c, 16) : nullptr;
  return p ? (uint8_t)(p - ALPHABET) : (uint8_t)15;
}

// a decimal number that fills [p, e) -> false when it does not
inline bool number(const char *p, const char *e, int64_t *v) {
  bool neg = false;
  if (p < e && (*p == '-' || *p == '+')) neg = *p++ == '-';
  if (p >= e || e - p > 18) return false;
  int64_t x = 0;
  for (; p < e; p++) { if (*p < '0' || *p > '9') return false; x = x * 10 + (*p - '0'); }
  *v = neg ? -x : x;
  return true;
}

// One SAM line (with or without its newline) -> one BAM record appended to o, block_size included.  ref_id / next_ref_id: the places
// of RNAME / RNEXT in the header's sequence list; they are used where the line names a sequence, '*' gives -1 and an RNEXT of '='
// the record's own ref_id.  Optional fields: integers (TAG:i:<n>) only, stored as int32 in the order of the line.
// -> OK, or MALFORMED / NAME_TOO_LONG / TOO_MANY_OPS with o as it was
inline int record_of_sam_line(std::string &o, const char *line, size_t len, int32_t ref_id, int32_t next_ref_id) {
  const char *end = line + len;
  if (end > line && end[-1] == '\n') end--;
  const char *f[12];                                         // starts of the 11 mandatory fields, f[11]: behind the last of them
  int nf = 0;
  f[nf++] = line;
  for (const char *p = line; p < end && nf < 12; p++) if (*p == '\t') f[nf++] = p + 1;
  if (nf < 11) return MALFORMED;
  const char *tags = nf == 12 ? f[11] : nullptr;
  if (nf == 11) f[11] = end + 1;
  auto field_end = [&](int k) { return f[k + 1] - 1; };
  auto is_star = [&](int k) { return field_end(k) - f[k] == 1 && *f[k] == '*'; };
  int64_t flag, pos, mapq, pnext, tlen;
  if (!number(f[1], field_end(1), &flag) || !number(f[3], field_end(3), &pos) || !number(f[4], field_end(4), &mapq) || !number(f[7], field_end(7), &pnext) ||
      !number(f[8], field_end(8), &tlen))
    return MALFORMED;
  const size_t l_name = (size_t)(field_end(0) - f[0]);
  if (l_name < 1) return MALFORMED;
  if (l_name > QNAME_MAX) return NAME_TOO_LONG;
  const size_t at = o.size();
  auto give_up = [&](int why) { o.resize(at); return why; };
  const int32_t rid = is_star(2) ? -1 : ref_id;
  const int32_t nid = is_star(6) ? -1 : (field_end(6) - f[6] == 1 && *f[6] == '=') ? rid : next_ref_id;
  const bool no_seq = is_star(9);
  const uint32_t l_seq = no_seq ? 0u : (uint32_t)(field_end(9) - f[9]);
  o.append(36, '\0');                                        // block_size and the fixed part, filled in below
  o.append(f[0], l_name);
  o.push_back('\0');
  // CIGAR
  uint32_t n_ops = 0;
  int64_t ref_span = 0;
  if (!is_star(5)) {
    static const char OPS[] = "MIDNSHP=X";
    for (const char *p = f[5]; p < field_end(5);) {
      const char *d = p;
      while (p < field_end(5) && *p >= '0' && *p <= '9') p++;
      int64_t n;
      const char *op = p < field_end(5) ? (const char *)memchr(OPS, *p, 9) : nullptr;
      if (!op || !number(d, p, &n) || n >= (1 << 28)) return give_up(MALFORMED);
      p++;
      if (n_ops == CIGAR_OPS_MAX) return give_up(TOO_MANY_OPS);
      n_ops++;
      put32(o, (uint32_t)n << 4 | (uint32_t)(op - OPS));
      if (*op == 'M' || *op == 'D' || *op == 'N' || *op == '=' || *op == 'X') ref_span += n;
    }
  }
  // SEQ: two letters a byte, the first in the high half
  for (uint32_t k = 0; k < l_seq; k += 2) {
    const uint8_t hi = base_code((unsigned char)f[9][k]), lo = k + 1 < l_seq ? base_code((unsigned char)f[9][k + 1]) : (uint8_t)0;
    o.push_back((char)(hi << 4 | lo));
  }
  // QUAL: Phred values; absent ('*') with a sequence present: 0xFF throughout
  if (is_star(10)) o.append(l_seq, (char)0xff);
  else {
    if ((size_t)(field_end(10) - f[10]) != l_seq) return give_up(MALFORMED);
    for (uint32_t k = 0; k < l_seq; k++) o.push_back((char)((unsigned char)f[10][k] - 33));
  }
  for (const char *p = tags; p && p < end;) {
    const char *e = (const char *)memchr(p, '\t', (size_t)(end - p));
    if (!e) e = end;
    int64_t v;
    if (e - p < 6 || p[2] != ':' || p[3] != 'i' || p[4] != ':' || !number(p + 5, e, &v) || v < INT32_MIN || v > INT32_MAX) return give_up(MALFORMED);
    o.push_back(p[0]); o.push_back(p[1]); o.push_back('i');
    put32(o, (uint32_t)(int32_t)v);
    p = e + 1;
  }
  const int64_t pos0 = pos - 1, pnext0 = pnext - 1;
  const bool placed = pos0 >= 0;
  const uint32_t bin = placed ? reg2bin(pos0, pos0 + (((flag & 0x4) || ref_span < 1) ? 1 : ref_span)) : (uint32_t)BIN_UNPLACED;
  set32(o, at, (uint32_t)(o.size() - at - 4));
  set32(o, at + 4, (uint32_t)rid);
  set32(o, at + 8, (uint32_t)(int32_t)pos0);
  set32(o, at + 12, bin << 16 | ((uint32_t)mapq & 0xffu) << 8 | (uint32_t)(l_name + 1));
  set32(o, at + 16, ((uint32_t)flag & 0xffffu) << 16 | n_ops);
  set32(o, at + 20, l_seq);
  set32(o, at + 24, (uint32_t)nid);
  set32(o, at + 28, (uint32_t)(int32_t)pnext0);
  set32(o, at + 32, (uint32_t)(int32_t)tlen);
  return OK;
}

// the uncompressed header: magic, the SAM header text (may be empty), the sequence list
inline void header(std::string &o, const char *text, size_t text_len, const std::vector<std::string> &names, const uint32_t *lengths) {
  o.append("BAM\1", 4);
  put32(o, (uint32_t)text_len);
  o.append(text, text_len);
  put32(o, (uint32_t)names.size());
  for (size_t s = 0; s < names.size(); s++) {
    put32(o, (uint32_t)names[s].size() + 1);
    o.append(names[s]);
    o.push_back('\0');
    put32(o, lengths[s]);
  }
}

// compression level from the text of an environment switch: 0..9, anything else zlib's default
inline int level_of(const char *s) {
  if (!s || s[0] < '0' || s[0] > '9' || s[1]) return Z_DEFAULT_COMPRESSION;
  return s[0] - '0';
}

// [data, data + n) as BGZF blocks appended to out.  The stream is cut every PAYLOAD_MAX bytes, whatever it holds, and the blocks are
// deflated independently of each other: the bytes that come out depend on neither the number of threads nor who took which block.
// n == 0: nothing.  -> false when zlib fails
inline bool bgzf(std::string &out, const char *data, size_t n, int level, int nthreads) {
  const size_t nblocks = (n + PAYLOAD_MAX - 1) / PAYLOAD_MAX;
  if (!nblocks) return true;
  if (nthreads < 1) nthreads = 1;
  if ((size_t)nthreads > nblocks) nthreads = (int)nblocks;
  std::vector<std::string> part((size_t)nthreads);
  std::vector<char> failed((size_t)nthreads, 0);
  auto work = [&](int t) {
    std::string &o = part[(size_t)t];
    const size_t lo = nblocks * (size_t)t / (size_t)nthreads, hi = nblocks * (size_t)(t + 1) / (size_t)nthreads;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { failed[(size_t)t] = 1; return; }
    const size_t room = (size_t)deflateBound(&zs, PAYLOAD_MAX);
    o.reserve((hi - lo) * 20000);
    for (size_t b = lo; b < hi && !failed[(size_t)t]; b++) {
      const char *src = data + b * PAYLOAD_MAX;
      const size_t m = n - b * PAYLOAD_MAX < (size_t)PAYLOAD_MAX ? n - b * PAYLOAD_MAX : (size_t)PAYLOAD_MAX;
      static const unsigned char HEAD[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 'B', 'C', 0x02, 0};
      const size_t at = o.size();
      o.append((const char *)HEAD, 16);
      o.append(2 + room, '\0');
      zs.next_in = (Bytef *)src; zs.avail_in = (uInt)m;
      zs.next_out = (Bytef *)&o[at + 18]; zs.avail_out = (uInt)room;
      const int rv = deflate(&zs, Z_FINISH);
      const size_t clen = room - zs.avail_out, total = 18 + clen + 8;
      if (rv != Z_STREAM_END || total > 65536) { failed[(size_t)t] = 1; break; }
      o.resize(at + 18 + clen);
      o[at + 16] = (char)((total - 1) & 0xff); o[at + 17] = (char)((total - 1) >> 8);
      put32(o, (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)src, (uInt)m));
      put32(o, (uint32_t)m);
      deflateReset(&zs);
    }
    deflateEnd(&zs);
  };
  if (nthreads == 1) work(0);
  else { std::vector<std::thread> th; for (int t = 0; t < nthreads; t++) th.emplace_back(work, t); for (std::thread &x : th) x.join(); }
  size_t tot = out.size();
  for (int t = 0; t < nthreads; t++) { if (failed[(size_t)t]) return false; tot += part[(size_t)t].size(); }
  out.reserve(tot);
  for (const std::string &s : part) out += s;
  return true;
}

}  // namespace smgbam

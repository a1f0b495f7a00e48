// smg_alnin.hpp -- reads from SAM and BAM files (smalt map -F sam|bam) without a BAM library.  The reference reads such files through
// the bambamc library (infmt.c, smalt.c:584, :804-826, :1129-1184), which its build here lacks; the record layout and BGZF are those of
// the SAM/BAM specification, zlib does the inflate.  The reference tree does not hold the order in which bambamc's collator hands
// templates out, so the rules below are this project's own.
//
// Records
//   BAM   a series of BGZF members (gzip members with a 'BC' extra field that holds their size).  The members of a feed call are
//         inflated on `nthreads` threads; the inflated stream is decoded on the calling thread.  A record may span members and feed
//         calls.  The magic, the header text and the sequence list are skipped.  The 28-byte end-of-file block is an empty member like
//         any other: a file without it is taken as it is.
//   SAM   lines; those that begin with '@' in front of the first record are skipped, wholly empty lines are skipped, fields are
//         tab-separated and a line with fewer than 11 of them is an error.  One thread (nthreads is not used).
//   Only QNAME, FLAG, SEQ and QUAL are used.
// Which records count
//   Records with flag 0x100 (secondary) or 0x800 (supplementary) are dropped.  Every other record is one read, mapped or not.
// The read as it was sequenced
//   With flag 0x10 the sequence is reverse-complemented (IUPAC letters too: R<->Y, K<->M, B<->V, D<->H; S, W, N stay) and the
//   qualities are reversed.  BAM letters come from "=ACMGRSVTWYHKDBN".  After that the letters follow smaltgpu_reads_parse: upper
//   case, U -> T, non-letters N ('=' becomes N).  Qualities are phred+33 characters.  BAM qualities that begin with 0xFF, or a SAM
//   QUAL of '*', mean that the read has none: BOTH views of a run that holds such a read have has_qual = 0, like a FASTQ block with a
//   FASTA record.  A record without sequence ('*', l_seq 0) is a read of no bases, as the FASTQ parser makes of an empty sequence
//   line; it says nothing about qualities.  Hard-clipped bases are gone: the read is what SEQ holds.
// Names
//   QNAME; with flag 0x1 and exactly one of 0x40 / 0x80 set, "/1" or "/2" is appended (the SAM writer takes it off again,
//   report.c:452-455; CIGAR and SSAHA lines keep it, as for FASTQ reads named x/1, x/2).  Flag 0x1 with both or neither of
//   0x40 / 0x80 is a single read with its plain name.
// Collation, over the whole input
//   A mate (0x1 with exactly one of 0x40 / 0x80) waits in a table keyed by QNAME until the other mate arrives.  The pair takes the
//   place of its later record and always has mate 1 as the read and mate 2 as the mate.  A record whose name AND mate number
//   already wait releases the waiting one as a single read at that point, and waits itself.  What still waits at the end of the
//   input follows as single reads in input order, "/1" or "/2" kept.  The table lives in memory: no temporary files.
// Runs
//   take() hands out maximal stretches of consecutive templates of one kind (single reads, or pairs), cut at max_templates.
//   Nothing is reordered across kinds: runs processed in order print in template order.
// Errors
//   BAD_FILE with a message that names the byte offset in the file (BGZF) or the record number, counted from 1 over all records
//   (SAM: all record lines) of the input.  After an error the reader only repeats it; it can be freed.
//
// Pure host C++ over zlib: no HIP header and nothing of the library, so that a stand-alone program can include this file
// (tests/hostemu/alnin_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace smgaln {

enum { FMT_SAM = 1, FMT_BAM = 2 };
enum { OK = 0, BAD_ARG = 1, BAD_FILE = 2 };
enum { MEMBER_MAX = 65536 };          // a BGZF member and its payload are at most 64 KiB each (BSIZE and the writers' limit)

// the letters of a read as smaltgpu_reads_parse stores them (make3BitMangledCodec, sequence.c:287-318), straight and complemented
struct Letters {
  uint8_t fwd[256], rev[256];
  static uint8_t canon(unsigned c) {
    if (c >= 'a' && c <= 'z') c -= 32;
    if (c == 'U') c = 'T';
    return (c >= 'A' && c < 'A' + 31) ? (uint8_t)c : (uint8_t)'N';
  }
  Letters() {
    static const char FROM[] = "ACGTUMRWSYKVHDBN", TO[] = "TGCAAKYWSRMBDHVN";
    for (unsigned c = 0; c < 256; c++) {
      unsigned d = c;
      const unsigned up = (c >= 'a' && c <= 'z') ? c - 32 : c;
      const char *p = up ? (const char *)memchr(FROM, (int)up, 16) : nullptr;
      if (p) d = (unsigned char)TO[p - FROM];
      fwd[c] = canon(c);
      rev[c] = canon(d);
    }
  }
};
inline const Letters &letters() { static const Letters t; return t; }

struct Read {                          // blob: the name (suffix included), the bases, the qualities (if any)
  std::string blob;
  uint32_t name_len = 0, len = 0;
  bool has_qual = true;
};
struct Template { int kind = 0; Read r, m; };        // kind 1: r alone; 2: r = mate 1, m = mate 2

struct Side {                          // one view of a run, in the layout of smaltgpu_reads_parse
  std::vector<uint8_t> bases, quals;
  std::vector<uint64_t> off, name_off;
  std::vector<char> names;
  void clear() { bases.clear(); quals.clear(); names.clear(); off.assign(1, 0); name_off.assign(1, 0); }
  void add(const Read &x) {
    const char *b = x.blob.data();
    names.insert(names.end(), b, b + x.name_len); names.push_back('\0');
    bases.insert(bases.end(), b + x.name_len, b + x.name_len + x.len);
    if (x.has_qual && x.len) quals.insert(quals.end(), b + x.name_len + x.len, b + x.name_len + 2 * (size_t)x.len);
    else quals.resize(bases.size(), (uint8_t)'!');                       // a place holder: the run has no qualities then (or the read no bases)
    off.push_back(bases.size()); name_off.push_back(names.size());
  }
};

inline uint32_t le16(const unsigned char *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const unsigned char *p) { return le16(p) | le16(p + 2) << 16; }

struct Reader {
  int format = 0;
  int err_code = OK;                   // != OK: the reader has failed, err says why
  std::string err;
  uint64_t file_off = 0;               // bytes of the file that earlier feed calls consumed
  uint64_t nrec = 0;                   // records seen so far, dropped ones included
  bool ended = false;                  // a feed call with is_last has been through
  bool sam_body = false;               // SAM: the first record has been seen ('@' lines are records from here on)
  // BAM: the inflated stream that is not decoded yet, and where in the file's layout it stands
  std::string stream;
  size_t spos = 0;
  int stage = 0;                       // 0 magic + l_text, 1 text, 2 n_ref, 3 l_name, 4 name + l_ref, 5 records
  uint64_t skip = 0;
  uint32_t nref_left = 0;
  std::deque<Template> ready;          // templates in output order
  struct Waiting { Read rd; int mate; uint64_t serial; };
  std::unordered_map<std::string, Waiting> table;
  Side side[2];
  bool run_has_qual = true;
  double sec_inflate = 0, sec_decode = 0, sec_take = 0;      // wall time: BGZF members walked and inflated | records decoded and collated | runs copied out
  static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

  int fail(int code, const std::string &why) { err_code = code; err = why; return code; }
  int fail_at(const char *what, uint64_t off) {
    char m[200];
    snprintf(m, sizeof(m), "BAM input: %s at byte offset %llu of the file", what, (unsigned long long)off);
    return fail(BAD_FILE, m);
  }
  int fail_rec(const char *what) {
    char m[200];
    snprintf(m, sizeof(m), "%s input: %s in record %llu", format == FMT_BAM ? "BAM" : "SAM", what, (unsigned long long)nrec);
    return fail(BAD_FILE, m);
  }

  // ---- one record: name [0, name_len), flag, `len` letters through letter(i), qualities (phred+33) through qual(i) unless !has_qual
  template <class LetterAt, class QualAt>
  void record(const char *name, size_t name_len, uint32_t flag, uint32_t len, bool has_qual, LetterAt letter, QualAt qual) {
    if (flag & (0x100u | 0x800u)) return;
    const int mate = (flag & 0x1u) && (((flag & 0x40u) != 0) != ((flag & 0x80u) != 0)) ? ((flag & 0x40u) ? 1 : 2) : 0;
    Read rd;
    rd.name_len = (uint32_t)name_len + (mate ? 2u : 0u);
    rd.len = len;
    rd.has_qual = has_qual || !len;
    const bool q = has_qual && len;
    rd.blob.resize((size_t)rd.name_len + (size_t)len * (q ? 2 : 1));
    char *o = &rd.blob[0];
    memcpy(o, name, name_len);
    if (mate) { o[name_len] = '/'; o[name_len + 1] = (char)('0' + mate); }
    uint8_t *b = (uint8_t *)o + rd.name_len, *qq = b + len;
    const Letters &L = letters();
    if (flag & 0x10u) {
      for (uint32_t i = 0; i < len; i++) b[i] = L.rev[letter(len - 1 - i)];
      if (q) for (uint32_t i = 0; i < len; i++) qq[i] = qual(len - 1 - i);
    } else {
      for (uint32_t i = 0; i < len; i++) b[i] = L.fwd[letter(i)];
      if (q) for (uint32_t i = 0; i < len; i++) qq[i] = qual(i);
    }
    if (!mate) { ready.emplace_back(); ready.back().kind = 1; ready.back().r = std::move(rd); return; }
    std::string key(name, name_len);
    auto it = table.find(key);
    if (it == table.end()) { table.emplace(std::move(key), Waiting{std::move(rd), mate, nrec}); return; }
    Waiting &w = it->second;
    ready.emplace_back();
    Template &t = ready.back();
    if (w.mate == mate) {                                    // the same mate again: the waiting one goes out alone, the new one waits
      t.kind = 1; t.r = std::move(w.rd);
      w.rd = std::move(rd); w.serial = nrec;
    } else {
      t.kind = 2;
      t.r = std::move(mate == 1 ? rd : w.rd);
      t.m = std::move(mate == 1 ? w.rd : rd);
      table.erase(it);
    }
  }

  void release_waiting() {                                   // the end of the input: orphans in input order
    std::vector<Waiting *> left;
    left.reserve(table.size());
    for (auto &kv : table) left.push_back(&kv.second);
    std::sort(left.begin(), left.end(), [](const Waiting *a, const Waiting *b) { return a->serial < b->serial; });
    for (Waiting *w : left) { ready.emplace_back(); ready.back().kind = 1; ready.back().r = std::move(w->rd); }
    table.clear();
  }

  // ---- SAM --------------------------------------------------------------------------------------------------------------
  int sam_line(const char *p, const char *e) {
    if (e > p && e[-1] == '\r') e--;
    if (p == e) return OK;
    if (!sam_body && *p == '@') return OK;
    sam_body = true;
    nrec++;
    const char *f[12];
    int nf = 0;
    f[nf++] = p;
    for (const char *c = p; c < e && nf < 12; c++) if (*c == '\t') f[nf++] = c + 1;
    if (nf < 11) return fail_rec("a line with fewer than 11 fields");
    if (nf == 11) f[11] = e + 1;
    auto flen = [&](int k) { return (size_t)(f[k + 1] - 1 - f[k]); };
    if (!flen(0)) return fail_rec("an empty QNAME");
    uint32_t flag = 0;
    if (!flen(1) || flen(1) > 5) return fail_rec("a FLAG that is not a number");
    for (size_t i = 0; i < flen(1); i++) {
      if (f[1][i] < '0' || f[1][i] > '9') return fail_rec("a FLAG that is not a number");
      flag = flag * 10 + (uint32_t)(f[1][i] - '0');
    }
    if (flag > 0xffffu) return fail_rec("a FLAG that is not a number");
    const bool no_seq = flen(9) == 1 && *f[9] == '*', no_qual = flen(10) == 1 && *f[10] == '*';
    const size_t len = no_seq ? 0 : flen(9);
    if (!no_qual && flen(10) != len) return fail_rec("SEQ and QUAL of different lengths");
    if (len > 0x7fffffffu) return fail_rec("a sequence too long");
    const unsigned char *s = (const unsigned char *)f[9], *q = (const unsigned char *)f[10];
    record(f[0], flen(0), flag, (uint32_t)len, !no_qual, [s](uint32_t i) { return s[i]; }, [q](uint32_t i) { return q[i]; });
    return OK;
  }

  int feed_sam(const char *bytes, uint64_t len, bool is_last, uint64_t *consumed) {
    uint64_t p = 0;
    const double t0 = now();
    while (p < len) {
      const char *nl = (const char *)memchr(bytes + p, '\n', (size_t)(len - p));
      if (!nl && !is_last) break;
      const uint64_t e = nl ? (uint64_t)(nl - bytes) : len;
      if (sam_line(bytes + p, bytes + e)) return err_code;
      p = nl ? e + 1 : len;
    }
    sec_decode += now() - t0;
    *consumed = p;
    return OK;
  }

  // ---- BAM --------------------------------------------------------------------------------------------------------------
  struct Member { uint64_t at; uint32_t data_off, data_len, isize, crc; size_t out_at; int bad; };

  // the members that lie whole in [bytes, bytes + len) -> mem, *used = where the first one that does not begins
  int walk(const unsigned char *bytes, uint64_t len, bool is_last, std::vector<Member> &mem, uint64_t *used, size_t *total) {
    uint64_t p = 0;
    size_t out = 0;
    while (p < len) {
      const uint64_t left = len - p;
      if (left < 18) { if (is_last) return fail_at("a truncated BGZF header", file_off + p); break; }
      const unsigned char *h = bytes + p;
      if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return fail_at("a bad BGZF header (not a gzip member with an extra field)", file_off + p);
      const uint32_t xlen = le16(h + 10);
      if (left < 12 + (uint64_t)xlen) { if (is_last) return fail_at("a truncated BGZF header", file_off + p); break; }
      int64_t bsize = -1;
      for (uint32_t x = 0; x + 4 <= xlen;) {                 // the subfields of the extra field: SI1 SI2 SLEN data
        const unsigned char *sf = h + 12 + x;
        const uint32_t slen = le16(sf + 2);
        if (x + 4 + (uint64_t)slen > xlen) break;
        if (sf[0] == 'B' && sf[1] == 'C' && slen == 2) { bsize = (int64_t)le16(sf + 4); break; }
        x += 4 + slen;
      }
      if (bsize < 0) return fail_at("a bad BGZF header (no BC field)", file_off + p);
      const uint64_t total_len = (uint64_t)bsize + 1;
      if (total_len < 12 + (uint64_t)xlen + 8) return fail_at("a wrong BSIZE (smaller than header and trailer)", file_off + p);
      if (left < total_len) { if (is_last) return fail_at("a wrong BSIZE or a truncated file (the BGZF member runs past the end)", file_off + p); break; }
      Member m;
      m.at = p; m.data_off = 12 + xlen; m.data_len = (uint32_t)(total_len - 12 - xlen - 8);
      m.crc = le32(h + total_len - 8); m.isize = le32(h + total_len - 4); m.out_at = out; m.bad = 0;
      if (m.isize > MEMBER_MAX) return fail_at("an ISIZE above 64 KiB", file_off + p);
      out += m.isize;
      mem.push_back(m);
      p += total_len;
    }
    *used = p; *total = out;
    return OK;
  }

  int feed_bam(const char *bytes_, uint64_t len, bool is_last, int nthreads, uint64_t *consumed) {
    const unsigned char *bytes = (const unsigned char *)bytes_;
    const double t0 = now();
    std::vector<Member> mem;
    uint64_t used = 0;
    size_t total = 0;
    if (walk(bytes, len, is_last, mem, &used, &total)) return err_code;
    if (spos && (spos == stream.size() || spos > (1u << 20))) { stream.erase(0, spos); spos = 0; }
    const size_t base = stream.size();
    stream.resize(base + total);
    const size_t n = mem.size();
    if (nthreads < 1) nthreads = 1;
    if ((size_t)nthreads > n / 4 + 1) nthreads = (int)(n / 4 + 1);
    char *dst = total ? &stream[base] : nullptr;
    auto work = [&](int t) {
      const size_t lo = n * (size_t)t / (size_t)nthreads, hi = n * (size_t)(t + 1) / (size_t)nthreads;
      std::vector<unsigned char> tmp(MEMBER_MAX);
      z_stream zs;
      memset(&zs, 0, sizeof(zs));
      if (inflateInit2(&zs, -15) != Z_OK) { for (size_t i = lo; i < hi; i++) mem[i].bad = 1; return; }
      for (size_t i = lo; i < hi; i++) {
        Member &m = mem[i];
        zs.next_in = (Bytef *)(bytes + m.at + m.data_off); zs.avail_in = m.data_len;
        zs.next_out = tmp.data(); zs.avail_out = MEMBER_MAX;
        const int rv = inflate(&zs, Z_FINISH);
        const size_t got = MEMBER_MAX - zs.avail_out;
        if (rv != Z_STREAM_END || zs.avail_in) m.bad = 1;                                   // not a deflate stream that fills the member
        else if (got != m.isize) m.bad = 2;
        else if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), tmp.data(), (uInt)got) != m.crc) m.bad = 3;
        else if (got) memcpy(dst + m.out_at, tmp.data(), got);
        if (m.bad) break;                                                                  // (what lies behind is not decoded anyway)
        inflateReset(&zs);
      }
      inflateEnd(&zs);
    };
    if (nthreads == 1) work(0);
    else { std::vector<std::thread> th; for (int t = 0; t < nthreads; t++) th.emplace_back(work, t); for (std::thread &x : th) x.join(); }
    for (const Member &m : mem)
      if (m.bad) {
        stream.resize(base);
        return fail_at(m.bad == 1 ? "a BGZF member that does not inflate (corrupt data or a wrong BSIZE)" : m.bad == 2 ? "an ISIZE mismatch" : "a CRC mismatch", file_off + m.at);
      }
    const double t1 = now();
    sec_inflate += t1 - t0;
    const int rv = decode(is_last);
    sec_decode += now() - t1;
    if (rv) return rv;
    *consumed = used;
    return OK;
  }

  // decode what the stream holds; is_last: nothing follows
  int decode(bool is_last) {
    for (;;) {
      const size_t avail = stream.size() - spos;
      const unsigned char *p = (const unsigned char *)stream.data() + spos;
      if (stage == 1 || stage == 4) {                        // bytes to pass over
        const size_t n = skip < avail ? (size_t)skip : avail;
        spos += n; skip -= n;
        if (skip) break;
        stage = stage == 1 ? 2 : 3;
      } else if (stage == 0) {
        if (avail < 8) break;
        if (memcmp(p, "BAM\1", 4)) return fail(BAD_FILE, "BAM input: not a BAM file (the inflated stream does not begin with the magic), byte offset 0 of the file");
        skip = le32(p + 4); spos += 8; stage = 1;
      } else if (stage == 2) {
        if (avail < 4) break;
        nref_left = le32(p); spos += 4; stage = 3;
      } else if (stage == 3) {
        if (!nref_left) { stage = 5; continue; }
        if (avail < 4) break;
        skip = (uint64_t)le32(p) + 4; spos += 4; nref_left--; stage = 4;
      } else {
        if (avail < 4) break;
        const uint64_t block_size = le32(p);
        if (block_size < 32) { nrec++; return fail_rec("a block_size below the fixed part of a record"); }
        if (avail - 4 < block_size) {
          if (is_last) { nrec++; return fail_rec("a block_size that runs past the data (truncated last record)"); }
          break;
        }
        nrec++;
        const unsigned char *r = p + 4;
        const uint32_t l_name = r[8], n_cigar = le16(r + 12), flag = le16(r + 14), l_seq = le32(r + 16);
        if (!l_name) return fail_rec("l_read_name 0");
        const uint64_t need = 32 + (uint64_t)l_name + 4 * (uint64_t)n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
        if (need > block_size) return fail_rec("fields that run past block_size");
        const char *name = (const char *)r + 32;
        if (name[l_name - 1]) return fail_rec("a name without its NUL");
        const size_t name_len = strnlen(name, l_name - 1);
        if (!name_len) return fail_rec("an empty read name");
        const unsigned char *seq = r + 32 + l_name + 4 * (size_t)n_cigar, *qual = seq + ((size_t)l_seq + 1) / 2;
        static const char ALPHABET[] = "=ACMGRSVTWYHKDBN";
        record(name, name_len, flag, l_seq, !(l_seq && qual[0] == 0xff),
               [seq](uint32_t i) { return (unsigned char)ALPHABET[(seq[i >> 1] >> ((~i & 1u) << 2)) & 0xfu]; },
               [qual](uint32_t i) { return (uint8_t)(qual[i] > 93 ? 126 : qual[i] + 33); });
        spos += 4 + (size_t)block_size;
      }
    }
    if (is_last && stage == 5 && spos < stream.size()) { nrec++; return fail_rec("a truncated last record"); }
    if (is_last && stage != 5) return fail(BAD_FILE, "BAM input: the file ends inside its header (magic, text or sequence list), byte offset " + std::to_string(file_off) + " of the file or behind");
    return OK;
  }

  // ---- the two calls ------------------------------------------------------------------------------------------------------
  int feed(const char *bytes, uint64_t len, bool is_last, int nthreads, uint64_t *consumed) {
    *consumed = 0;
    if (err_code) return err_code;
    if (ended) return len ? fail(BAD_ARG, "feed: bytes behind a call with is_last") : OK;
    const int rv = format == FMT_BAM ? feed_bam(bytes, len, is_last, nthreads, consumed) : feed_sam(bytes, len, is_last, consumed);
    if (rv) { *consumed = 0; return rv; }
    file_off += *consumed;
    if (is_last) { ended = true; release_waiting(); }
    return OK;
  }

  // the next run -> kind (0: none ready) and its number of templates; side[0] (and side[1] for pairs) hold it until the next call
  uint32_t take(uint32_t max_templates, int *kind) {
    side[0].clear(); side[1].clear();
    run_has_qual = true;
    *kind = 0;
    if (err_code || ready.empty()) return 0;
    const double t0 = now();
    const int k = ready.front().kind;
    uint32_t n = 0;
    while (!ready.empty() && ready.front().kind == k && (!max_templates || n < max_templates)) {
      const Template &t = ready.front();
      side[0].add(t.r);
      if (!t.r.has_qual) run_has_qual = false;
      if (k == 2) { side[1].add(t.m); if (!t.m.has_qual) run_has_qual = false; }
      ready.pop_front();
      n++;
    }
    *kind = k;
    sec_take += now() - t0;
    return n;
  }
};

}  // namespace smgaln

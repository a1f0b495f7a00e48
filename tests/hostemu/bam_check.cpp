// tests/hostemu/bam_check.cpp -- TEST DRIVER (no device, no library): smalt_amd/csrc/smg_bam.hpp on its own, meant to be built with
// -fsanitize=address,undefined and run directly (tests/test_report_bam.py).
//
//   bam_check <lines.sam> <out.bgzf> <threads> [<sequence name> ...]
//
// Every alignment line of <lines.sam> becomes a BAM record (RNAME / RNEXT looked up in the names given, in their order), the records
// are cut into BGZF blocks on <threads> threads, the end-of-file block follows, and the bytes go to <out.bgzf>: they must be the ones
// the library hands out for the same records.  The same stream is made once more on one thread and compared.  Then the corner shapes
// run on made-up lines: a record across three blocks, an empty SEQ, absent qualities, odd length, letters outside the alphabet,
// '=' as RNEXT, the limits of the name and of the CIGAR, broken lines.  Prints the length and CRC32 of the stream.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>

#include "../../smalt_amd/csrc/smg_bam.hpp"

static int failures = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bam_check: line %d: %s\n", __LINE__, #x); failures++; } } while (0)

static int32_t id_of(const std::vector<std::string> &names, const char *b, const char *e) {
  for (size_t k = 0; k < names.size(); k++) if (names[k].size() == (size_t)(e - b) && !memcmp(names[k].data(), b, names[k].size())) return (int32_t)k;
  return -1;
}

static uint32_t get32(const std::string &s, size_t at) { uint32_t v = 0; for (int k = 3; k >= 0; k--) v = v << 8 | (unsigned char)s[at + (size_t)k]; return v; }

// inflate the members of a BGZF stream again (zlib's gzip reader checks CRC32 and ISIZE of each)
static bool inflate_all(const std::string &z, std::string &plain) {
  plain.clear();
  for (size_t at = 0; at < z.size();) {
    if (z.size() - at < 28) return false;
    const size_t total = ((unsigned char)z[at + 16] | (size_t)(unsigned char)z[at + 17] << 8) + 1;
    if (at + total > z.size()) return false;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, 15 + 16) != Z_OK) return false;
    std::string out((size_t)smgbam::PAYLOAD_MAX + 1, '\0');
    zs.next_in = (Bytef *)(z.data() + at); zs.avail_in = (uInt)total;
    zs.next_out = (Bytef *)&out[0]; zs.avail_out = (uInt)out.size();
    const int rv = inflate(&zs, Z_FINISH);
    const size_t n = out.size() - zs.avail_out;
    inflateEnd(&zs);
    if (rv != Z_STREAM_END || zs.avail_in || n > (size_t)smgbam::PAYLOAD_MAX) return false;
    plain.append(out, 0, n);
    at += total;
  }
  return true;
}

static void corner_cases(int nthreads) {
  using namespace smgbam;
  std::string rec, z, back;
  // a record across three blocks between two small ones
  std::string seq(150001, 'A'), qual(150001, 'I');
  for (size_t k = 0; k < seq.size(); k++) { seq[k] = "ACGTRXN"[k % 7]; qual[k] = (char)(33 + k % 60); }
  const std::string small = "r1\t0\tchr\t101\t60\t3S4=1X2I5M2D6M1H\t=\t301\t210\tACGTACGTACGTACGTACGTA\tIIIIIIIIIIIIIIIIIIIII\tNM:i:5\tAS:i:-12\n";
  const std::string big = "r2\t4\t*\t0\t0\t*\t*\t0\t0\t" + seq + "\t" + qual + "\tNM:i:0\tAS:i:0";
  CHECK(record_of_sam_line(rec, small.data(), small.size(), 7, 9) == OK);
  const size_t first = rec.size();
  CHECK(get32(rec, 0) == first - 4 && (int32_t)get32(rec, 4) == 7 && get32(rec, 8) == 100 && (int32_t)get32(rec, 24) == 7 && get32(rec, 28) == 300 && get32(rec, 32) == 210);
  CHECK((get32(rec, 12) & 0xff) == 3 && ((get32(rec, 12) >> 8) & 0xff) == 60 && (get32(rec, 12) >> 16) == reg2bin(100, 100 + 4 + 1 + 5 + 2 + 6));
  CHECK((get32(rec, 16) & 0xffff) == 8 && (get32(rec, 16) >> 16) == 0 && get32(rec, 20) == 21);
  CHECK(get32(rec, 36 + 3) == (3u << 4 | 4u) && get32(rec, 36 + 3 + 4) == (4u << 4 | 7u) && get32(rec, 36 + 3 + 28) == (1u << 4 | 5u));
  CHECK((unsigned char)rec[36 + 3 + 32] == 0x12 && (unsigned char)rec[36 + 3 + 32 + 10] == 0x10);          // "AC" ...; odd length: the last half byte is 0
  CHECK((unsigned char)rec[36 + 3 + 32 + 11] == 'I' - 33);
  CHECK(!memcmp(rec.data() + first - 14, "NMi\5\0\0\0ASi\xf4\xff\xff\xff", 14));
  CHECK(record_of_sam_line(rec, big.data(), big.size(), 3, 3) == OK);
  CHECK((int32_t)get32(rec, first + 4) == -1 && (int32_t)get32(rec, first + 8) == -1 && (int32_t)get32(rec, first + 24) == -1 && (int32_t)get32(rec, first + 28) == -1);
  CHECK((get32(rec, first + 12) >> 16) == (uint32_t)BIN_UNPLACED && get32(rec, first + 20) == 150001);
  CHECK((unsigned char)rec[first + 36 + 3 + 2] == 0x5f);                                                       // "RX": R stays, X reads as N
  CHECK(record_of_sam_line(rec, small.data(), small.size(), 0, 0) == OK);
  CHECK(bgzf(z, rec.data(), rec.size(), Z_DEFAULT_COMPRESSION, nthreads) && inflate_all(z, back) && back == rec);
  CHECK(rec.size() > 3 * (size_t)PAYLOAD_MAX);
  std::string z1;
  CHECK(bgzf(z1, rec.data(), rec.size(), Z_DEFAULT_COMPRESSION, 1) && z1 == z);
  for (int level = 0; level <= 9; level += 3) { std::string zl; CHECK(bgzf(zl, rec.data(), rec.size(), level, nthreads) && inflate_all(zl, back) && back == rec); }
  // exactly one payload, one byte more, nothing
  std::string exact((size_t)PAYLOAD_MAX, 'x'), zz;
  CHECK(bgzf(zz, exact.data(), exact.size(), 6, nthreads) && zz.size() == ((unsigned char)zz[16] | (size_t)(unsigned char)zz[17] << 8) + 1);
  exact.push_back('y'); zz.clear();
  CHECK(bgzf(zz, exact.data(), exact.size(), 6, nthreads) && inflate_all(zz, back) && back == exact && zz.size() > ((unsigned char)zz[16] | (size_t)(unsigned char)zz[17] << 8) + 1);
  zz.clear();
  CHECK(bgzf(zz, exact.data(), 0, 6, nthreads) && zz.empty());
  // bytes that do not deflate: a stored block still fits BSIZE
  std::string noise((size_t)PAYLOAD_MAX, '\0');
  uint32_t x = 12345;
  for (char &c : noise) { x = x * 1664525u + 1013904223u; c = (char)(x >> 24); }
  for (int level : {0, 1, 9}) { zz.clear(); CHECK(bgzf(zz, noise.data(), noise.size(), level, 1) && zz.size() <= 65536 && inflate_all(zz, back) && back == noise); }
  // no SEQ; SEQ without qualities
  rec.clear();
  const std::string noseq = "r3\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\tNM:i:0\tAS:i:0\n", noqual = "r4\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*\tNM:i:0\tAS:i:0\n";
  CHECK(record_of_sam_line(rec, noseq.data(), noseq.size(), -1, -1) == OK && get32(rec, 20) == 0 && rec.size() == 36 + 3 + 14);
  const size_t second = rec.size();
  CHECK(record_of_sam_line(rec, noqual.data(), noqual.size(), -1, -1) == OK && get32(rec, second + 20) == 3 && !memcmp(rec.data() + second + 36 + 3 + 2, "\xff\xff\xff", 3));
  // limits and broken lines leave the output as it was
  const size_t before = rec.size();
  const std::string name254(254, 'n'), name255(255, 'n'), tail = "\t4\t*\t0\t0\t*\t*\t0\t0\tAC\tII\tNM:i:0\tAS:i:0\n";
  CHECK(record_of_sam_line(rec, (name255 + tail).data(), name255.size() + tail.size(), -1, -1) == NAME_TOO_LONG && rec.size() == before);
  CHECK(record_of_sam_line(rec, (name254 + tail).data(), name254.size() + tail.size(), -1, -1) == OK && (get32(rec, before + 12) & 0xff) == 255);
  std::string ops;
  for (int k = 0; k < 32768; k++) ops += "1M1I";
  const size_t again = rec.size();
  std::string many = "r5\t0\tchr\t1\t0\t" + ops + "\t*\t0\t0\t*\t*";
  CHECK(record_of_sam_line(rec, many.data(), many.size(), 0, -1) == TOO_MANY_OPS && rec.size() == again);
  ops.resize(ops.size() - 2);
  many = "r5\t0\tchr\t1\t0\t" + ops + "\t*\t0\t0\t*\t*";
  CHECK(record_of_sam_line(rec, many.data(), many.size(), 0, -1) == OK && (get32(rec, again + 16) & 0xffff) == 65535);
  const size_t end = rec.size();
  for (const char *bad : {"", "r\t0\t*\t0", "r\tx\t*\t0\t0\t*\t*\t0\t0\t*\t*", "r\t0\t*\t0\t0\t5Q\t*\t0\t0\t*\t*", "r\t0\t*\t0\t0\t5\t*\t0\t0\t*\t*", "r\t0\t*\t0\t0\t*\t*\t0\t0\tACG\tII",
                          "r\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\tNM:Z:x", "r\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*\tNM:i:", "\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*"})
    CHECK(record_of_sam_line(rec, bad, strlen(bad), -1, -1) == MALFORMED && rec.size() == end);
  // header
  std::string h;
  const uint32_t lens[2] = {1000, 4000000000u};
  header(h, "@HD\n", 4, {"a", "chr2"}, lens);
  CHECK(h.size() == 4 + 4 + 4 + 4 + (4 + 2 + 4) + (4 + 5 + 4) && !memcmp(h.data(), "BAM\1\4\0\0\0@HD\n\2\0\0\0\2\0\0\0a\0", 22) && get32(h, h.size() - 4) == 4000000000u);
  CHECK(level_of(nullptr) == Z_DEFAULT_COMPRESSION && level_of("0") == 0 && level_of("9") == 9 && level_of("10") == Z_DEFAULT_COMPRESSION && level_of("") == Z_DEFAULT_COMPRESSION);
  CHECK(reg2bin(-1, 0) == (uint32_t)BIN_UNPLACED && reg2bin(0, 1) == 4681 && reg2bin(16383, 16385) == 585 && reg2bin(0, 1 << 29) == 0);
  CHECK(sizeof(END_OF_FILE) == 28);
}

int main(int argc, char **argv) {
  if (argc < 4) { fprintf(stderr, "usage: bam_check <lines.sam> <out.bgzf> <threads> [<sequence name> ...]\n"); return 2; }
  const int nthreads = atoi(argv[3]);
  std::vector<std::string> names;
  for (int a = 4; a < argc; a++) names.push_back(argv[a]);
  std::string text;
  { std::ifstream f(argv[1], std::ios::binary); std::stringstream ss; ss << f.rdbuf(); text = ss.str(); }
  std::string records;
  size_t nrec = 0;
  for (size_t at = 0; at < text.size();) {
    size_t e = text.find('\n', at);
    if (e == std::string::npos) e = text.size();
    if (e > at && text[at] != '@') {
      const char *f[8];
      int nf = 0;
      f[nf++] = text.data() + at;
      for (size_t k = at; k < e && nf < 8; k++) if (text[k] == '\t') f[nf++] = text.data() + k + 1;
      if (nf < 8) { fprintf(stderr, "bam_check: short line at byte %zu\n", at); return 1; }
      const int rv = smgbam::record_of_sam_line(records, text.data() + at, e - at, id_of(names, f[2], f[3] - 1), id_of(names, f[6], f[7] - 1));
      if (rv != smgbam::OK) { fprintf(stderr, "bam_check: line at byte %zu: error %d\n", at, rv); return 1; }
      nrec++;
    }
    at = e + 1;
  }
  const int level = smgbam::level_of(getenv("SMALTGPU_BAM_LEVEL"));
  std::string stream, single, back;
  if (!smgbam::bgzf(stream, records.data(), records.size(), level, nthreads) || !smgbam::bgzf(single, records.data(), records.size(), level, 1)) { fprintf(stderr, "bam_check: deflate failed\n"); return 1; }
  CHECK(stream == single);
  CHECK(inflate_all(stream, back) && back == records);
  stream.append((const char *)smgbam::END_OF_FILE, sizeof(smgbam::END_OF_FILE));
  { std::ofstream o(argv[2], std::ios::binary); o.write(stream.data(), (std::streamsize)stream.size()); if (!o) { fprintf(stderr, "bam_check: cannot write %s\n", argv[2]); return 1; } }
  printf("records: %zu\nstream: %zu bytes, crc32 %08lx\n", nrec, stream.size(), (unsigned long)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)stream.data(), (uInt)stream.size()));
  corner_cases(nthreads);
  if (failures) return 1;
  printf("corner cases ok\n");
  return 0;
}

// reads_dev_check.cpp -- the read parser of smalt_amd/csrc/smg_reads_dev.hpp run the way the kernels of smg_reads_dev.hip run it,
// on the host and in one lane: block counts, granule prefixes and the candidate list (as tests/hostemu/fastq_ref_check.cpp), the
// speculative step for every node, the jump tables level by level, the marking from the highest level down, the numbering in tiles
// of RD_NODE_TILE nodes with the scan over the tiles between its two passes, and the output pass per block and lane of 16 bytes.
//   reads_dev_check <case file> <bytes per block, 0 = the default>
// The case file holds any number of cases: u32 length of the text, u8 mode, u8 is_last, u32 max_reads (little endian), the text.
//   mode 0   one parse of the text;
//   mode 1   for every cut 0 < c < length: text[0, c) with is_last = 0, then text[consumed, length) with is_last = 1.
// Per parse one line: "OK <nreads> <has_qual> <consumed> <bases> <quals> <read_off> <names>" (hex, '-' for nothing; offsets with
// commas) or "ERR <message>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../smalt_amd/csrc/smg_reads_dev.hpp"

using namespace smg;

static void hex(std::string &o, const uint8_t *p, size_t n) {
  static const char d[] = "0123456789abcdef";
  if (!n) { o.push_back('-'); return; }
  for (size_t i = 0; i < n; i++) { o.push_back(d[p[i] >> 4]); o.push_back(d[p[i] & 15]); }
}

// -> consumed; line: what the parse printed
static uint64_t parse(const uint8_t *tx, uint64_t len, bool is_last, uint32_t max_reads, uint64_t block, std::string &line) {
  line.clear();
  if (!len) { line = "OK 0 0 0 - - 0 -"; return 0; }
  const uint64_t nblk = (len + block - 1) / block, ngran = (len + FQ_GRAN - 1) / FQ_GRAN;
  // k_fq_count, k_fq_scan, k_fq_cands
  std::vector<uint32_t> gran(ngran, 0xdeadbeefu);
  std::vector<uint64_t> blk_nb(nblk + 1, 0), blk_cd(nblk + 1, 0);
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    uint32_t run_nb = 0, run_cd = 0;
    for (uint64_t o = b0; o < b1; o += FA_LANE_BYTES) {
      const uint32_t n = b1 - o < FA_LANE_BYTES ? (uint32_t)(b1 - o) : FA_LANE_BYTES, v = fq_lane_counts(tx + o, n, o ? tx[o - 1] : 0);
      if (o % FQ_GRAN == 0) gran[o / FQ_GRAN] = run_nb;
      run_nb += v & 0xFFFFu; run_cd += v >> 16;
    }
    blk_nb[b] = run_nb; blk_cd[b] = run_cd;
  }
  uint64_t ra = 0, rb = 0;
  for (uint64_t b = 0; b < nblk; b++) { const uint64_t xa = blk_nb[b], xb = blk_cd[b]; blk_nb[b] = ra; blk_cd[b] = rb; ra += xa; rb += xb; }
  blk_nb[nblk] = ra; blk_cd[nblk] = rb;
  const uint64_t ncand = rb;
  std::vector<uint64_t> cand(ncand + 1, ~0ull);
  for (uint64_t b = 0; b < nblk; b++) {
    uint64_t at = blk_cd[b];
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    for (uint64_t x = b0; x < b1; x++) if (fq_candidate(x ? tx[x - 1] : 0, tx[x])) { if (at >= ncand) { line = "ERR the two passes disagree"; return 0; } cand[at++] = x; }
  }
  FqText t;
  t.text = tx; t.len = len; t.block_bytes = (uint32_t)block; t.pad = 0; t.blk_nb = blk_nb.data(); t.gran_nb = gran.data(); t.cand = cand.data(); t.ncand = ncand; t.nblk = nblk;
  // k_rd_step: every node
  const uint64_t nn = ncand + 1;
  std::vector<RdStep> step(nn);
  for (uint64_t v = 0; v < nn; v++) {
    step[v] = rd_step(t, v);
    if (step[v].link <= v || step[v].link > nn) { line = "ERR a link does not point forward"; return 0; }
  }
  // k_rd_jump0 / k_rd_double: the tables, the sink points at itself
  const uint32_t L = rd_levels(nn);
  std::vector<std::vector<uint32_t>> J(L ? L : 1, std::vector<uint32_t>(nn + 1));
  for (uint64_t v = 0; v < nn; v++) J[0][v] = step[v].link;
  J[0][nn] = (uint32_t)nn;
  for (uint32_t r = 1; r < L; r++) for (uint64_t v = 0; v <= nn; v++) J[r][v] = J[r - 1][J[r - 1][v]];
  // k_rd_mark: from the highest level down
  std::vector<uint8_t> mark(nn + 1, 0);
  mark[0] = 1;
  for (uint32_t r = L; r-- > 0;) for (uint64_t v = 0; v < nn; v++) if (mark[v]) mark[J[r][v]] = 1;
  {                                                     // the marks are the path, no more and no less
    std::vector<uint8_t> path(nn + 1, 0);
    for (uint64_t v = 0; v < nn; v = step[v].link) path[v] = 1;
    for (uint64_t v = 0; v < nn; v++) if (path[v] != mark[v]) { line = "ERR the marks are not the path"; return 0; }
  }
  // k_rd_sums: per tile the records and their bases, and the first node the batch stops at
  const uint64_t ntile = (nn + RD_NODE_TILE - 1) / RD_NODE_TILE;
  std::vector<uint64_t> part_c(ntile + 1, 0), part_b(ntile + 1, 0);
  RdSum sum;
  memset(&sum, 0, sizeof(sum));
  sum.stop_node = RD_NONE;
  for (uint64_t v = 0; v < nn; v++) {
    if (!mark[v]) continue;
    if (rd_is_record(step[v].kf)) { part_c[v / RD_NODE_TILE]++; part_b[v / RD_NODE_TILE] += step[v].n; }
    if (rd_stops(step[v].kf, is_last) && v < sum.stop_node) sum.stop_node = (uint32_t)v;
  }
  // k_fq_scan over the tiles
  ra = rb = 0;
  for (uint64_t i = 0; i < ntile; i++) { const uint64_t xa = part_c[i], xb = part_b[i]; part_c[i] = ra; part_b[i] = rb; ra += xa; rb += xb; }
  part_c[ntile] = ra; part_b[ntile] = rb;
  // k_rd_number
  std::vector<RdRec> rec(nn);
  std::vector<uint64_t> read_off(nn + 1, ~0ull);
  read_off[0] = 0;
  for (uint64_t tile = 0; tile < ntile; tile++) {
    uint64_t idx = part_c[tile], off = part_b[tile];
    for (uint64_t v = tile * RD_NODE_TILE; v < nn && v < (tile + 1) * RD_NODE_TILE; v++) {
      const bool r = mark[v] && rd_is_record(step[v].kf);
      if (v == sum.stop_node) { sum.stop_kf = step[v].kf; sum.stop_idx = idx; sum.stop_hdr_off = step[v].hdr_off; }
      if (rd_taken(step[v].kf, mark[v] != 0, v, idx, sum.stop_node, max_reads)) {
        rec[idx] = rd_record(step[v], off); read_off[idx + 1] = off + step[v].n;
        if (idx + 1 > sum.nreads) sum.nreads = (uint32_t)(idx + 1);
        if (rd_kind(step[v].kf) == RD_FASTA) sum.any_fasta = 1;
      }
      if (r) { idx++; off += step[v].n; }
    }
  }
  if (sum.stop_node != RD_NONE && rd_stop_is_error(sum.stop_kf, is_last) && (!max_reads || sum.stop_idx < max_reads)) {
    line = "ERR " + rd_error_text(sum.stop_kf, (const char *)tx, len, sum.stop_hdr_off);
    return 0;
  }
  const uint64_t nreads = sum.nreads, total = read_off[nreads];
  const bool has_qual = nreads && !sum.any_fasta;
  // k_rd_emit: per block and lane
  std::vector<uint8_t> bases(total + 1, 0xA5), quals(total + 1, 0xA5);
  for (uint64_t b = 0; b < nblk && nreads; b++) {
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    uint64_t nb = blk_nb[b];
    for (uint64_t o = b0; o < b1; o += FA_LANE_BYTES) {
      const uint32_t n = b1 - o < FA_LANE_BYTES ? (uint32_t)(b1 - o) : FA_LANE_BYTES;
      if (o % FQ_GRAN == 0 && nb != blk_nb[b] + gran[o / FQ_GRAN]) { line = "ERR the granule prefixes disagree"; return 0; }
      rd_emit_lane(tx + o, n, o, nb, rec.data(), nreads, bases.data(), has_qual ? quals.data() : nullptr, total);
      nb += fq_lane_counts(tx + o, n, 0) & 0xFFFFu;
    }
  }
  if (bases[total] != 0xA5 || quals[total] != 0xA5) { line = "ERR the output pass wrote behind the arrays"; return 0; }
  const uint64_t consumed = rd_consumed(len, is_last, max_reads, nreads, nreads ? rec[nreads - 1].q1 : 0);
  std::string names;
  for (uint64_t i = 0; i < nreads; i++) { names += rd_name((const char *)tx, len, rec[i].hdr_off); names.push_back('\0'); }
  char buf[96];
  snprintf(buf, sizeof(buf), "OK %llu %d %llu ", (unsigned long long)nreads, has_qual ? 1 : 0, (unsigned long long)consumed);
  line = buf;
  hex(line, bases.data(), (size_t)total); line.push_back(' ');
  if (has_qual) hex(line, quals.data(), (size_t)total); else line.push_back('-');
  line.push_back(' ');
  for (uint64_t i = 0; i <= nreads; i++) { snprintf(buf, sizeof(buf), i ? ",%llu" : "%llu", (unsigned long long)read_off[i]); line += buf; }
  line.push_back(' ');
  hex(line, (const uint8_t *)names.data(), names.size());
  return consumed;
}

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: reads_dev_check <case file> <bytes per block>\n"); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  const uint64_t block = atoll(argv[2]) > 0 ? fa_block_bytes(argv[2]) : RD_BLOCK_DEFAULT;
  std::string line;
  uint8_t head[10];
  while (fread(head, 1, 10, fp) == 10) {
    uint32_t len, max_reads;
    memcpy(&len, head, 4); memcpy(&max_reads, head + 6, 4);
    const int mode = head[4];
    const bool is_last = head[5] != 0;
    std::vector<uint8_t> text((size_t)len + 1);       // the copies below are exact: the sanitizer sees every byte behind a chunk
    if (len && fread(text.data(), 1, len, fp) != len) { fprintf(stderr, "short case file\n"); return 2; }
    if (mode == 0) {
      std::vector<uint8_t> t(text.begin(), text.begin() + len);
      parse(t.data(), len, is_last, max_reads, block, line);
      puts(line.c_str());
    } else {
      for (uint32_t c = 1; c < len; c++) {
        std::vector<uint8_t> a(text.begin(), text.begin() + c);
        const uint64_t used = parse(a.data(), c, false, max_reads, block, line);
        puts(line.c_str());
        std::vector<uint8_t> b(text.begin() + used, text.begin() + len);
        parse(b.data(), len - used, true, max_reads, block, line);
        puts(line.c_str());
      }
    }
  }
  fclose(fp);
  return 0;
}

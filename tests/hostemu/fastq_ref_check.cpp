// fastq_ref_check.cpp -- the reader of smalt_amd/csrc/smg_fastq_ref.hpp run the way the kernels of smg_fastq_ref.hip run it, on
// the host and in one lane: per block of text and per lane of 16 bytes the counts of non-blank bytes and of candidates with the
// prefixes per granule of 64 bytes, the scan of the block counts, the list of candidates, the walk over the records (fq_walk, the
// function the kernel runs) and the output pass over blocks of text with the record table.
//   fastq_ref_check <file> <bytes per block, 0 = the default>
// prints "OK <nseq>" and per sequence "<name in hex or -> <bases or ->", or "REFUSED <cause>" (exit status 1).
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../smalt_amd/csrc/smg_fastq_ref.hpp"

using namespace smg;

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: fastq_ref_check <file> <bytes per block>\n"); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string text;
  char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) text.append(buf, n);
  fclose(fp);
  const uint64_t len = text.size();
  if (!len) { printf("REFUSED %s\n", fa_refusal(0, FA_P, 0, 0)); return 1; }
  const uint8_t *tx = (const uint8_t *)text.data();
  const uint64_t block = fa_block_bytes(atoll(argv[2]) > 0 ? argv[2] : nullptr), nblk = (len + block - 1) / block, ngran = (len + FQ_GRAN - 1) / FQ_GRAN;

  // k_fq_count: lanes of 16 bytes; a granule is four of them
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
  // k_fq_scan
  uint64_t ra = 0, rb = 0;
  for (uint64_t b = 0; b < nblk; b++) { const uint64_t xa = blk_nb[b], xb = blk_cd[b]; blk_nb[b] = ra; blk_cd[b] = rb; ra += xa; rb += xb; }
  blk_nb[nblk] = ra; blk_cd[nblk] = rb;
  // k_fq_cands
  const uint64_t ncand = rb, cap = ncand + 1;
  std::vector<uint64_t> cand(cap, ~0ull);
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    uint64_t at = blk_cd[b];
    for (uint64_t x = b0; x < b1; x++)
      if (fq_candidate(x ? tx[x - 1] : 0, tx[x])) { if (at >= ncand) { printf("REFUSED the two passes disagree (candidates)\n"); return 3; } cand[at++] = x; }
    if (at != blk_cd[b + 1]) { printf("REFUSED the two passes disagree (block %llu)\n", (unsigned long long)b); return 3; }
  }
  // k_fq_walk
  FqText t;
  t.text = tx; t.len = len; t.block_bytes = (uint32_t)block; t.pad = 0; t.blk_nb = blk_nb.data(); t.gran_nb = gran.data(); t.cand = cand.data(); t.ncand = ncand; t.nblk = nblk;
  std::vector<FqRecord> rec(cap);
  FqWalk w;
  fq_walk(t, rec.data(), cap, &w);
  const std::string why = fq_refusal(w, text.data(), len);
  if (!why.empty()) { printf("REFUSED %s\n", why.c_str()); return 1; }
  // k_fq_emit: per block, with the lanes' own searches of the record table
  std::string bases((size_t)w.nbases, '\0');
  std::vector<char> written((size_t)w.nbases, 0);
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    uint64_t u_tile = fq_rec_upper(rec.data(), 0, w.nrec, b0);
    uint64_t base = fq_block_base(rec.data(), w.nrec, w.nbases, u_tile, b0, blk_nb[b]);
    for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
      const uint64_t u_hi = w.nrec - u_tile < FQ_REC_PER_TILE ? w.nrec : u_tile + FQ_REC_PER_TILE;
      for (uint64_t o = t0; o < b1 && o < t0 + FA_TILE; o += FA_LANE_BYTES) {
        uint64_t u = fq_rec_upper(rec.data(), u_tile, u_hi, o);
        if (u != fq_rec_upper(rec.data(), 0, w.nrec, o)) { printf("REFUSED the window of records of a tile is too small\n"); return 3; }
        for (uint64_t x = o; x < b1 && x < o + FA_LANE_BYTES; x++) {
          while (u < w.nrec && rec[u].d0 <= x) u++;
          if (u > 0 && x < rec[u - 1].d1 && !fa_isspace(tx[x])) {
            if (base >= w.nbases || written[(size_t)base]) { printf("REFUSED the output pass disagrees with the walk (bases)\n"); return 3; }
            written[(size_t)base] = 1; bases[(size_t)base++] = text[x];
          }
        }
      }
      u_tile = fq_rec_upper(rec.data(), u_tile, u_hi, t0 + FA_TILE - 1);
    }
  }
  for (const char x : written) if (!x) { printf("REFUSED the output pass disagrees with the walk (holes)\n"); return 3; }
  printf("OK %llu\n", (unsigned long long)w.nrec);
  for (uint64_t i = 0; i < w.nrec; i++) {
    const std::string nm = fa_clean_name(text.data() + rec[i].hdr_off + 1, (size_t)(len - rec[i].hdr_off - 1));
    const uint64_t e = i + 1 < w.nrec ? rec[i + 1].base_off : w.nbases;
    if (nm.empty()) printf("-");
    for (const char c : nm) printf("%02x", (unsigned)(uint8_t)c);
    printf(" %s\n", e > rec[i].base_off ? bases.substr((size_t)rec[i].base_off, (size_t)(e - rec[i].base_off)).c_str() : "-");
  }
  return 0;
}

// fasta_check.cpp -- the FASTA automaton of smalt_amd/csrc/smg_fasta.hpp run the way the kernels of smg_fasta.hip run it, on the
// host and in one lane: per block of text the lanes' 16-byte stretches for the four entry states, the scan of their maps, the block
// summary (pass A); the composition of the summaries in block order; the output pass with the true entry states (pass B).
//   fasta_check <file> <bytes per block, 0 = the whole text in one block>
// prints "OK <nseq>" and per sequence "<name in hex or -> <bases or ->", or "REFUSED <cause>" (exit status 1).
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../smalt_amd/csrc/smg_fasta.hpp"

using namespace smg;

namespace {

const uint32_t NLANE = FA_TILE / FA_LANE_BYTES;

// the lanes of the tile [t0, end): what every lane finds for the four entry states, and the exclusive scan of the maps
void tile_lanes(const std::string &text, uint64_t t0, uint64_t end, std::vector<FaLane> &lane, std::vector<uint32_t> &excl, uint32_t *tile_map) {
  lane.assign(NLANE, FaLane());
  excl.assign(NLANE, FA_MAP_ID);
  uint32_t run = FA_MAP_ID;
  for (uint32_t t = 0; t < NLANE; t++) {
    fa_lane_init(lane[t]);
    const uint64_t o = t0 + (uint64_t)t * FA_LANE_BYTES;
    for (uint32_t i = 0; i < FA_LANE_BYTES && o + i < end; i++) fa_lane_byte(lane[t], (uint8_t)text[o + i]);
    excl[t] = run;
    run = fa_map_compose(run, lane[t].map);
  }
  *tile_map = run;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) { fprintf(stderr, "usage: fasta_check <file> <bytes per block>\n"); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string text;
  char buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), fp)) > 0;) text.append(buf, n);
  fclose(fp);
  const uint64_t len = text.size();
  if (!len) { printf("REFUSED %s\n", fa_refusal(0, FA_P, 0, 0)); return 1; }
  const uint64_t block = atoll(argv[2]) > 0 ? fa_block_bytes(argv[2]) : (len + 63) / 64 * 64;
  const uint64_t nblk = (len + block - 1) / block;
  std::vector<FaLane> lane;
  std::vector<uint32_t> excl;

  // pass A
  std::vector<FaSummary> sum(nblk);
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    FaSummary s = {FA_MAP_ID, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
      uint32_t tile_map;
      tile_lanes(text, t0, b1, lane, excl, &tile_map);
      for (uint32_t e = 0; e < FA_NENTRY; e++)
        for (uint32_t t = 0; t < NLANE; t++) {
          const uint32_t le = fa_map_at(excl[t], fa_map_at(s.map, e));
          s.nb[e] += fa_lane_count(lane[t].nb, le); s.nh[e] += fa_lane_count(lane[t].nh, le);
        }
      s.map = fa_map_compose(s.map, tile_map);
    }
    sum[b] = s;
  }
  // compose
  std::vector<FaEntry> at(nblk + 1);
  FaEntry a = {0, 0, FA_P, 0};
  for (uint64_t b = 0; b < nblk; b++) { at[b] = a; fa_entry_advance(a, sum[b]); }
  at[nblk] = a;
  if (const char *why = fa_refusal(len, a.state, a.hdr_off, 0)) { printf("REFUSED %s\n", why); return 1; }
  // pass B
  std::string bases((size_t)a.base_off, '\0');
  std::vector<FaHeader> hdr((size_t)a.hdr_off);
  uint64_t nfastq = 0;
  for (uint64_t b = 0; b < nblk; b++) {
    const uint64_t b0 = b * block, b1 = len - b0 < block ? len : b0 + block;
    uint32_t state = at[b].state;
    uint64_t base = at[b].base_off, hd = at[b].hdr_off;
    for (uint64_t t0 = b0; t0 < b1 && state < FA_NENTRY; t0 += FA_TILE) {
      uint32_t tile_map;
      tile_lanes(text, t0, b1, lane, excl, &tile_map);
      for (uint32_t t = 0; t < NLANE; t++) {
        uint32_t st = fa_map_at(excl[t], state);
        const uint64_t o = t0 + (uint64_t)t * FA_LANE_BYTES;
        const uint32_t nb = fa_lane_count(lane[t].nb, st), nh = fa_lane_count(lane[t].nh, st);
        uint64_t pb = base, ph = hd;
        for (uint32_t i = 0; i < FA_LANE_BYTES && o + i < b1; i++) {
          const uint32_t r = fa_step(st, fa_row((uint8_t)text[o + i]));
          if (r & FA_EMIT) { if (pb >= bases.size()) { printf("REFUSED the two passes disagree (bases)\n"); return 3; } bases[(size_t)pb++] = text[o + i]; }
          if (r & FA_HDR) {
            if (ph >= hdr.size()) { printf("REFUSED the two passes disagree (headers)\n"); return 3; }
            hdr[(size_t)ph].text_off = o + i; hdr[(size_t)ph].base_off = pb; ph++;
            if (r & FA_FQ) nfastq++;
          }
          st = r & 7u;
        }
        if (pb != base + nb || ph != hd + nh) { printf("REFUSED the two passes disagree (lane counts)\n"); return 3; }
        base = pb; hd = ph;
      }
      state = fa_map_at(tile_map, state);
    }
    if (base != at[b + 1].base_off || hd != at[b + 1].hdr_off || state != at[b + 1].state) { printf("REFUSED the two passes disagree (block %llu)\n", (unsigned long long)b); return 3; }
  }
  if (const char *why = fa_refusal(len, a.state, a.hdr_off, nfastq)) { printf("REFUSED %s\n", why); return 1; }
  printf("OK %zu\n", hdr.size());
  for (size_t i = 0; i < hdr.size(); i++) {
    const std::string nm = fa_clean_name(text.data() + hdr[i].text_off + 1, (size_t)(len - hdr[i].text_off - 1));
    const uint64_t e = i + 1 < hdr.size() ? hdr[i + 1].base_off : a.base_off;
    if (nm.empty()) printf("-");
    for (const char c : nm) printf("%02x", (unsigned)(uint8_t)c);
    printf(" %s\n", e > hdr[i].base_off ? bases.substr((size_t)hdr[i].base_off, (size_t)(e - hdr[i].base_off)).c_str() : "-");
  }
  return 0;
}

// tests/hostemu/hits_walk_check.cpp -- TEST-ONLY host build (one lane, SMG_NLANES = 1) of the seeding stage and of S3 on its
// own (stage_seed, stage_hits of smalt_amd/csrc), nothing behind them: what stage_hits left in the pool and how many windows it
// took per strand.  tests/test_hits_fill_emu.py holds both to the plain references.  Not part of libsmaltgpu.so.
// usage: hits_walk_check <index_prefix> <reads.fq> <window> <tab> <fill> <concat 0|1> <hits.bin> <windows.bin>
//   hits.bin: the layout of emu_main.cpp's EMU_DUMP_HITS ("SMGHITS1", read by tests/test_hits_ref.read_hits_dump)
//   windows.bin: u32 per strand, bits 0..15 the windows the strand was gathered in, 16..31 those whose bound was raised
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../smalt_amd/csrc/smg_cands.hpp"
#include "../../smalt_amd/csrc/smg_indexfile.hpp"

using namespace smg;

static uint8_t code_of(unsigned char c) {       // sequence.c:287-322
  switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 5;
  }
}

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  const uint32_t hitsW = (uint32_t)atoi(argv[3]), fill = (uint32_t)atoi(argv[5]);
  uint32_t hitsTab = (uint32_t)atoi(argv[4]);
  if (hitsTab < 8 || hitsTab > (uint32_t)CANDS_TAB) hitsTab = CANDS_TAB;
  HostIndex hix;
  std::string err;
  if (!read_index_files(argv[1], hix, err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
  std::vector<uint32_t> seqlo((size_t)hix.nseq + 1);
  for (int64_t i = 0; i <= hix.nseq; i++) seqlo[(size_t)i] = (uint32_t)(hix.sop[(size_t)i] / (uint64_t)hix.s);
  DevIndex ix;
  ix.k = hix.k; ix.s = hix.s; ix.typ = hix.typ; ix.nbits_key = hix.nbits_key; ix.nbits_lo = hix.nbits_lo;
  ix.nkeys = hix.nkeys; ix.npos = hix.npos; ix.nwords = hix.nwords;
  ix.idx = hix.idx.data(); ix.pos = hix.pos.data(); ix.wordidx = hix.wordidx.data(); ix.posidx = hix.posidx.data();
  ix.packed = hix.packed.data(); ix.sop = hix.sop.data(); ix.seqlo = seqlo.data(); ix.nseq = (int32_t)hix.nseq; ix.totlen = hix.totlen;

  MapPar p; p.cov_frac = 0.0;                   // smalt map's defaults, as emu_main.cpp sets them
  p.ncut = 10000; p.min_cover = 0; p.min_swatscor = ix.k + ix.s - 1; p.below_max = 0;
  p.min_basq = 0; p.target_depth = 512; p.max_depth = 2048;
  p.flags = FLG_BEST | (ix.nseq < 512 && atoi(argv[6]) == 0 ? FLG_SEQBYSEQ : 0);
  p.match = 1; p.mismatch = -2; p.gap_init = -4; p.gap_ext = -3;

  std::vector<uint8_t> codes, codes_rc, qual;
  std::vector<uint64_t> off(1, 0);
  FILE *fp = fopen(argv[2], "r");
  if (!fp) return 1;
  char *l1 = nullptr, *l2 = nullptr, *l3 = nullptr, *l4 = nullptr;
  size_t c1 = 0, c2 = 0, c3 = 0, c4 = 0;
  uint32_t qmaxlen = 0;
  while (getline(&l1, &c1, fp) > 0 && getline(&l2, &c2, fp) > 0 && getline(&l3, &c3, fp) > 0 && getline(&l4, &c4, fp) > 0) {
    const uint32_t len = (uint32_t)strcspn(l2, "\r\n");
    for (uint32_t i = 0; i < len; i++) { codes.push_back(code_of((unsigned char)l2[i])); qual.push_back((uint8_t)l4[i]); }
    for (uint32_t i = 0; i < len; i++) { const uint8_t cc = codes[off.back() + len - 1 - i]; codes_rc.push_back((uint8_t)((cc & 4) ? cc : 3 - cc)); }
    off.push_back(off.back() + len);
    if (len > qmaxlen) qmaxlen = len;
  }
  fclose(fp);
  free(l1); free(l2); free(l3); free(l4);
  const uint32_t n = (uint32_t)off.size() - 1, qmax = qmaxlen + 8;

  std::vector<HitInfoHdr> hi(2 * (size_t)n + 1);
  std::vector<SeedRec> seeds((2 * (size_t)n + 1) * qmax);
  std::vector<uint8_t> qmask((2 * (size_t)n + 1) * qmax, 0), qmask_seed;
  std::vector<uint64_t> hitpool((size_t)n * 2 * 4096 + (1u << 20));
  std::vector<HitRun> hitrun((size_t)2 * n + 1);
  std::vector<uint32_t> hitwin((size_t)2 * n + 1, 0);
  unsigned long long hit_count = 0, workctr[WK_NWORK] = {0};
  int32_t err_flag = 0;
  Batch b;
  memset((void *)&b, 0, sizeof(b));
  b.nreads = n; b.qmax = qmax; b.codes = codes.data(); b.codes_rc = codes_rc.data(); b.qual = qual.data(); b.read_off = off.data();
  b.hi = hi.data(); b.seeds = seeds.data(); b.qmask = qmask.data(); b.err_flag = &err_flag; b.work = workctr;
  b.hitpool = hitpool.data(); b.hitpool_cap = hitpool.size(); b.hitrun = hitrun.data(); b.hit_count = &hit_count; b.hitwin = hitwin.data();

  std::vector<uint8_t> sscr(seed_scratch_bytes(qmax, ix.s));
  for (uint32_t r = 0; r < n; r++) {
    SeedScratch sx = seed_scratch_carve(sscr.data(), qmax, ix.s);
    stage_seed(b, ix, p, r, 0, sx);
    stage_seed(b, ix, p, r, 1, sx);
  }
  qmask_seed = qmask;                           // the qualifiers as the seeding stage left them
  std::vector<uint8_t> hitlds(hits_lds_bytes(hitsW, CANDS_TAB) + 64);
  HitsScratch hx;
  hx.lds = hitlds.data(); hx.lds_bytes = hitlds.size(); hx.W = hitsW; hx.tab = hitsTab; hx.fill = fill;
  unsigned long long hph[4] = {0, 0, 0, 0};
  for (uint32_t rs = 0; rs < 2 * n; rs++) stage_hits(b, ix, p, rs >> 1, rs & 1u, hx, hph);

  FILE *hf = fopen(argv[7], "wb");
  if (!hf) { fprintf(stderr, "cannot write %s\n", argv[7]); return 1; }
  const uint32_t head[4] = {2 * n, qmax, hitsW, hitsTab};
  const uint64_t cnt[2] = {hit_count, (uint64_t)hitpool.size()};
  fwrite("SMGHITS1", 1, 8, hf); fwrite(head, 4, 4, hf); fwrite(cnt, 8, 2, hf);
  for (int f = 0; f < 3; f++) for (uint32_t rs = 0; rs < 2 * n; rs++) { const uint32_t v = f == 0 ? hi[rs].n_seeds : (f == 1 ? hi[rs].seed_rank : hi[rs].status); fwrite(&v, 4, 1, hf); }
  fwrite(seeds.data(), sizeof(SeedRec), (size_t)2 * n * qmax, hf);
  fwrite(qmask.data(), 1, (size_t)2 * n * qmax, hf);
  fwrite(hitrun.data(), sizeof(HitRun), (size_t)2 * n, hf);
  fwrite(hitpool.data(), 8, (size_t)(hit_count < hitpool.size() ? hit_count : hitpool.size()), hf);
  fwrite(qmask_seed.data(), 1, (size_t)2 * n * qmax, hf);
  if (fclose(hf)) return 1;
  FILE *wf = fopen(argv[8], "wb");
  if (!wf) { fprintf(stderr, "cannot write %s\n", argv[8]); return 1; }
  fwrite(hitwin.data(), 4, (size_t)2 * n, wf);
  return fclose(wf) ? 1 : 0;
}

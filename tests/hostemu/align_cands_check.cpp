// O1 and the K3 driver from the product's headers on injected candidates, without a GPU: stage_replay and stage_align built for the
// host with one lane, over the batch a test writes (tests/align_cands_data.py) and an index read through smg_indexfile.hpp.  What
// smaltgpu_align_cands_batch uploads is laid out here in host memory: reads encoded in both orientations, one CandHdr per read,
// the candidates in one pool with RCF_SCORED set.  The scratch slot of every read has exactly the size the product gives a slot of
// these capacities, and the pools are sized exactly, so that a sanitizer build sees an access outside.
//   align_cands_check INDEX_PREFIX FILE
// FILE: "match mismatch gap_init gap_ext min_swatscor below_max flags raw nreads qmax wincap dircap rescap dstrcap", then per read
// "qlen ncand cdf_forward cdf_reverse prev_max prev_2nd" and the bases ("-" for an empty read), then per candidate
// "rs re qs qe band_l band_r sqidx flags cover swscor" (flags: 1 reverse, 2 broken).
// Prints per read "CTL max1 max2 n_scored bandwidth_min min_swatscor scorlen_min go", "ST err swmax sw2nd nres nseg nhit" and per
// result "RS score q_start q_end s_start s_end sidx reverse cand_first DiffStr-in-hex".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
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
  if (argc != 3) { fprintf(stderr, "usage: align_cands_check INDEX_PREFIX FILE\n"); return 2; }
  HostIndex hix;
  std::string err;
  if (!read_index_files(argv[1], hix, err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
  std::vector<uint32_t> seqlo((size_t)hix.nseq + 1);
  for (int64_t i = 0; i <= hix.nseq; i++) seqlo[(size_t)i] = (uint32_t)(hix.sop[(size_t)i] / (uint64_t)hix.s);
  DevIndex ix;
  ix.k = hix.k; ix.s = hix.s; ix.typ = hix.typ; ix.nbits_key = hix.nbits_key; ix.nbits_lo = hix.nbits_lo;
  ix.nkeys = hix.nkeys; ix.npos = hix.npos; ix.nwords = hix.nwords;
  ix.idx = hix.idx.data(); ix.pos = hix.pos.data(); ix.wordidx = hix.wordidx.data(); ix.posidx = hix.posidx.data();
  ix.packed = hix.packed.data(); ix.sop = hix.sop.data(); ix.seqlo = seqlo.data(); ix.nseq = (int32_t)hix.nseq; ix.totlen = hix.totlen;

  FILE *f = fopen(argv[2], "r");
  if (!f) { perror(argv[2]); return 2; }
  MapPar p;
  memset((void *)&p, 0, sizeof(p));
  unsigned flags, raw, n, qmax, wincap, rescap, dstrcap;
  unsigned long long dircap;
  if (fscanf(f, "%d %d %d %d %d %d %u %u %u %u %u %llu %u %u", &p.match, &p.mismatch, &p.gap_init, &p.gap_ext, &p.min_swatscor, &p.below_max,
             &flags, &raw, &n, &qmax, &wincap, &dircap, &rescap, &dstrcap) != 14) return 2;
  p.flags = flags; p.ncut = 10000; p.target_depth = 512; p.max_depth = 2048;

  std::vector<uint8_t> codes, codes_rc;
  std::vector<uint64_t> off(1, 0);
  std::vector<CandHdr> ch(n ? n : 1);
  std::vector<RCand> rcpool;
  std::vector<int32_t> prevmax(2 * (size_t)n + 2, 0);
  memset((void *)ch.data(), 0, ch.size() * sizeof(CandHdr));
  for (unsigned r = 0; r < n; r++) {
    unsigned qlen, nc, cdf0, cdf1;
    if (fscanf(f, "%u %u %u %u %d %d", &qlen, &nc, &cdf0, &cdf1, &prevmax[2 * r], &prevmax[2 * r + 1]) != 6 || qlen + 8 > qmax) return 2;
    std::vector<char> bb((size_t)qlen + 3);
    char fmt[32];
    snprintf(fmt, sizeof fmt, "%%%us", qlen + 1);
    if (fscanf(f, fmt, bb.data()) != 1 || strlen(bb.data()) != (qlen ? qlen : 1)) return 2;
    for (unsigned i = 0; i < qlen; i++) codes.push_back(code_of((unsigned char)bb[i]));
    for (unsigned i = 0; i < qlen; i++) { const uint8_t cc = codes[off.back() + qlen - 1 - i]; codes_rc.push_back((uint8_t)((cc & 4) ? cc : 3 - cc)); }
    off.push_back(off.back() + qlen);
    CandHdr &h = ch[r];
    h.ncand = h.n_sort = h.n_mincover = h.n_reserved = nc;
    h.rc_off = (uint32_t)rcpool.size();
    h.cover_deficit[0] = cdf0; h.cover_deficit[1] = cdf1;
    for (unsigned i = 0; i < nc; i++) {
      RCand c;
      memset((void *)&c, 0, sizeof(c));
      unsigned long long rs, re;
      unsigned cf;
      if (fscanf(f, "%llu %llu %u %u %d %d %d %u %u %d", &rs, &re, &c.qs, &c.qe, &c.band_l, &c.band_r, &c.sqidx, &cf, &c.cover, &c.swscor) != 10) return 2;
      if (c.sqidx < 0 || c.sqidx >= ix.nseq || rs > re || re >= hix.sop[(size_t)c.sqidx + 1] - hix.sop[(size_t)c.sqidx]) { fprintf(stderr, "candidate outside its sequence\n"); return 2; }
      c.rs = rs; c.re = re; c.rid = r;
      c.flags = ((cf & 1) ? (uint32_t)RCF_REVERSE : 0u) | ((cf & 2) ? (uint32_t)RCF_ERR : 0u) | (uint32_t)RCF_SCORED;
      rcpool.push_back(c);
    }
  }
  fclose(f);
  if (codes.empty()) { codes.push_back(0); codes_rc.push_back(0); }
  if (rcpool.empty()) rcpool.resize(1);

  std::vector<HitInfoHdr> hi(2 * (size_t)n + 1);
  memset((void *)hi.data(), 0, hi.size() * sizeof(HitInfoHdr));
  std::vector<ReadCtl> ctl(n ? n : 1);
  std::vector<ReadStat> stat(n ? n : 1);
  std::vector<Result> respool((size_t)n * 8 + 4096);                       // the pools of a mapper for n reads
  std::vector<uint8_t> dstrpool(respool.size() * (size_t)(qmax / 4 + 48));
  uint32_t rc_count = (uint32_t)rcpool.size();
  unsigned long long res_count = 0, dstr_count = 0, workctr[WK_NWORK] = {0};
  int32_t err_flag = 0;
  Batch b;
  memset((void *)&b, 0, sizeof(b));
  b.nreads = n; b.qmax = qmax; b.codes = codes.data(); b.codes_rc = codes_rc.data(); b.read_off = off.data();
  b.hi = hi.data(); b.ch = ch.data(); b.rcpool = rcpool.data(); b.rccap = (uint32_t)rcpool.size(); b.rc_count = &rc_count;
  b.ctl = ctl.data(); b.stat = stat.data(); b.respool = respool.data(); b.rescap = respool.size(); b.res_count = &res_count;
  b.dstrpool = dstrpool.data(); b.dstrcap = dstrpool.size(); b.dstr_count = &dstr_count; b.err_flag = &err_flag; b.work = workctr;
  b.prevmax = prevmax.data(); b.raw_results = raw;

  for (unsigned r = 0; r < n; r++) {
    stage_replay(b, ix, p, r);
    std::vector<uint8_t> slot(align_scratch_bytes(qmax, wincap, dircap, rescap, dstrcap));
    AlignScratch ax = align_scratch_carve(slot.data(), qmax, wincap, dircap, rescap, dstrcap);
    stage_align(b, ix, p, r, ax);
    align_tally_flush(b, ax);
  }
  for (unsigned r = 0; r < n; r++) {
    const ReadCtl &c = ctl[r];
    const ReadStat &st = stat[r];
    printf("CTL %d %d %d %d %d %d %d\n", c.max1, c.max2, c.n_scored, c.bandwidth_min, c.min_swatscor, c.scorlen_min, c.go);
    printf("ST %d %d %d %u %d %u\n", st.err, st.swmax, st.sw2nd, st.nres, st.nseg, st.nhit + st.nhit_tot);
    for (uint32_t j = 0; j < st.nres; j++) {
      const Result &a = respool[st.res_off + j];
      std::string hex;
      for (uint32_t t = 0; t < a.strlen; t++) { char h2[4]; snprintf(h2, sizeof h2, "%02x", dstrpool[st.dstr_off + a.stroffs + t]); hex += h2; }
      printf("RS %d %u %u %llu %llu %d %u %u %s\n", a.swatscor, a.q_start, a.q_end, (unsigned long long)a.s_start, (unsigned long long)a.s_end, a.sidx,
             a.reverse, a.pad, hex.empty() ? "-" : hex.c_str());
    }
  }
  return 0;
}

// smg_fasta.hip -- the text of a FASTA reference parsed in HBM: bases, sequence offsets and header positions for
// build_index_device (smg_indexbuild.hip).  The automaton is the one of smg_fasta.hpp; a block of text does not know the state
// it is entered in, so the parse is three launches on the stream of the index construction:
//   pass A   k_fa_summary: one workgroup per block of text; per entry state the exit state, the bases and the headers of the block;
//   compose  k_fa_compose: one workgroup walks the summaries in block order: entry state, first base and first header of every block;
//   pass B   k_fa_emit: one workgroup per block again, now with its entry state: bases compacted into d_bases, one record per header.
// Inside a block a workgroup takes FA_TILE bytes at a time, 16 per lane (one 128-bit load, a wave reads 1 KiB in a row; the tile
// steps are those of smg_text.hpp).  A lane runs its 16 bytes for the four possible entry states at once (FaLane); an exclusive
// scan of the lanes' state maps under composition -- wave shuffles, then the four wave totals through LDS -- gives every lane its
// true entry state, a sum over the counts that belong to that state its place in the output.  No workgroup waits for another one.
#include <stdint.h>
#include <stdio.h>
#include <chrono>
#include <hip/hip_runtime.h>
#include "smg_text.hpp"

namespace smg {

// exclusive scan of the lanes' maps over the workgroup (256 threads) under composition; *total: all of them.  wmap: 4 words of LDS
__device__ inline uint32_t fa_block_scan_map(uint32_t m, uint32_t *wmap, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(m, d);
    if (lane >= d) m = fa_map_compose(o, m);
  }
  uint32_t excl = __shfl_up(m, 1);
  if (lane == 0) excl = FA_MAP_ID;
  __syncthreads();                       // the last use of wmap is over
  if (lane == 63) wmap[wave] = m;
  __syncthreads();
  uint32_t pre = FA_MAP_ID, all = FA_MAP_ID;
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) { if (w == wave) pre = all; all = fa_map_compose(all, wmap[w]); }
  *total = all;
  return fa_map_compose(pre, excl);
}

// the sums of four values over the workgroup, together: wave shuffles, then the wave totals through LDS.  wsum4: 16 words of LDS
__device__ inline void fa_block_sum4(const uint32_t (&v)[FA_NENTRY], uint32_t *wsum4, uint32_t (&total)[FA_NENTRY]) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t s[FA_NENTRY];
#pragma unroll
  for (uint32_t e = 0; e < FA_NENTRY; e++) { s[e] = v[e]; for (int d = 32; d > 0; d >>= 1) s[e] += __shfl_xor(s[e], d); }
  __syncthreads();                       // the last use of wsum4 is over
  if (lane == 0) for (uint32_t e = 0; e < FA_NENTRY; e++) wsum4[wave * FA_NENTRY + e] = s[e];
  __syncthreads();
#pragma unroll
  for (uint32_t e = 0; e < FA_NENTRY; e++) total[e] = wsum4[e] + wsum4[FA_NENTRY + e] + wsum4[2 * FA_NENTRY + e] + wsum4[3 * FA_NENTRY + e];
}

// pass A
__global__ void __launch_bounds__(256) k_fa_summary(const uint8_t *text, uint64_t len, uint32_t block_bytes, FaSummary *sum) {
  __shared__ uint32_t wmap[4], wsum4[4 * FA_NENTRY];
  const auto [b0, b1] = tx_block_range(len, block_bytes);
  uint32_t map = FA_MAP_ID, nb[FA_NENTRY] = {0, 0, 0, 0}, nh[FA_NENTRY] = {0, 0, 0, 0};       // of the tiles so far; the same in every thread
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES];
    uint64_t o;
    const uint32_t n = tx_lane_load(text, t0, b1, &o, c);
    FaLane l;
    fa_lane_init(l);
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) if (i < n) fa_lane_byte(l, c[i]);
    uint32_t tile_map;
    const uint32_t excl = fa_block_scan_map(l.map, wmap, &tile_map);
    uint32_t v[FA_NENTRY], tot[FA_NENTRY];                                     // a tile holds at most 4096 bases and 2048 headers: 16 bits each
    for (uint32_t e = 0; e < FA_NENTRY; e++) {
      const uint32_t le = fa_map_at(excl, fa_map_at(map, e));                  // the lane's entry state if the block is entered in e
      v[e] = fa_lane_count(l.nb, le) | fa_lane_count(l.nh, le) << 16;
    }
    fa_block_sum4(v, wsum4, tot);
    for (uint32_t e = 0; e < FA_NENTRY; e++) { nb[e] += tot[e] & 0xFFFFu; nh[e] += tot[e] >> 16; }
    map = fa_map_compose(map, tile_map);
  }
  if (threadIdx.x == 0) {
    FaSummary s;
    s.map = map;
    for (uint32_t e = 0; e < FA_NENTRY; e++) { s.nb[e] = nb[e]; s.nh[e] = nh[e]; }
    sum[blockIdx.x] = s;
  }
}

// compose: one workgroup.  Every thread folds a stretch of the summaries for the four entry states, thread 0 chains the 256
// stretches, every thread walks its stretch again from its true entry.  at[nblk] and *end: where the text ends.
__global__ void __launch_bounds__(256) k_fa_compose(const FaSummary *sum, uint64_t nblk, FaEntry *at, FaEntry *end) {
  __shared__ FaEntry fold[256][FA_NENTRY];
  __shared__ FaEntry start[256];
  const uint64_t per = (nblk + 255) / 256, i0 = (uint64_t)threadIdx.x * per < nblk ? (uint64_t)threadIdx.x * per : nblk, i1 = i0 + per < nblk ? i0 + per : nblk;
  for (uint32_t e = 0; e < FA_NENTRY; e++) {
    FaEntry a;
    a.base_off = 0; a.hdr_off = 0; a.state = e; a.pad = 0;
    for (uint64_t i = i0; i < i1; i++) fa_entry_advance(a, sum[i]);
    fold[threadIdx.x][e] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    FaEntry a;
    a.base_off = 0; a.hdr_off = 0; a.state = FA_P; a.pad = 0;
    for (uint32_t t = 0; t < 256; t++) {
      start[t] = a;
      if (a.state < FA_NENTRY) { const FaEntry f = fold[t][a.state]; a.base_off += f.base_off; a.hdr_off += f.hdr_off; a.state = f.state; }
    }
    *end = a;
  }
  __syncthreads();
  FaEntry a = start[threadIdx.x];
  for (uint64_t i = i0; i < i1; i++) { at[i] = a; fa_entry_advance(a, sum[i]); }
}

// pass B
__global__ void __launch_bounds__(256) k_fa_emit(const uint8_t *text, uint64_t len, uint32_t block_bytes, const FaEntry *at, uint8_t *bases, uint64_t nbases,
                                                 FaHeader *hdr, uint64_t nhdr, unsigned long long *nfastq) {
  __shared__ uint32_t wmap[4], wsum[4];
  __shared__ uint8_t stage[FA_TILE];                                           // the bases of a tile, compacted, before they go out in a row
  const auto [b0, b1] = tx_block_range(len, block_bytes);
  const FaEntry a = at[blockIdx.x];
  uint32_t state = a.state, fq = 0;
  uint64_t base = a.base_off, hd = a.hdr_off;
  if (state >= FA_NENTRY) return;                                              // the text is refused
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES];
    uint64_t o;
    const uint32_t n = tx_lane_load(text, t0, b1, &o, c);
    FaLane l;
    fa_lane_init(l);
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) if (i < n) fa_lane_byte(l, c[i]);
    uint32_t tile_map, tot;
    const uint32_t excl = fa_block_scan_map(l.map, wmap, &tile_map);
    uint32_t st = fa_map_at(excl, state);
    const uint32_t pre = tx_block_scan_sum(fa_lane_count(l.nb, st) | fa_lane_count(l.nh, st) << 16, wsum, &tot);
    uint32_t pb = pre & 0xFFFFu, ph = pre >> 16;
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) {
      if (i < n) {
        const uint32_t t = fa_step(st, fa_row(c[i]));
        if ((t & FA_EMIT) && pb < FA_TILE) stage[pb++] = c[i];
        if (t & FA_HDR) {
          if (hd + ph < nhdr) { FaHeader h; h.text_off = o + i; h.base_off = base + pb; hdr[hd + ph] = h; }
          ph++;
          if (t & FA_FQ) fq++;
        }
        st = t & 7u;
      }
    }
    const uint32_t tb = tot & 0xFFFFu;
    tx_stage_flush(stage, tb, bases, base, nbases);
    base += tb; hd += tot >> 16;
    state = fa_map_at(tile_map, state);
    if (state >= FA_NENTRY) break;                                             // uniform
  }
  for (int d = 32; d > 0; d >>= 1) fq += __shfl_xor(fq, d);
  if ((threadIdx.x & 63) == 0 && fq) atomicAdd(nfastq, (unsigned long long)fq);
}

int fasta_parse_device(const char *text, uint64_t text_len, uint32_t block_bytes, FastaParsed *out, char *err, size_t errlen) {
  if (!text_len) { snprintf(err, errlen, "%s", fa_refusal(0, FA_P, 0, 0)); return -1; }
  if (block_bytes < FA_BLOCK_MIN || (block_bytes & 63u)) { snprintf(err, errlen, "bad block size %u", block_bytes); return -1; }
  TextBlocks g;
  if (!text_blocks(text_len, block_bytes, &g)) { snprintf(err, errlen, "text of %llu bytes in blocks of %u: too many blocks", (unsigned long long)text_len, g.block_bytes); return -1; }
  const uint64_t nblk = g.nblk;
  DevMem<uint8_t> d_text, d_bases; DevMem<FaSummary> d_sum; DevMem<FaEntry> d_at; DevMem<FaHeader> d_hdr; DevMem<unsigned long long> d_fq;
  DevEvent ev[5];
  for (DevEvent &e : ev) SMG_HIP(e.create());
  SMG_HIP(d_text.alloc(g.padded));
  {
    const auto t0 = std::chrono::steady_clock::now();
    SMG_HIP(hipMemcpy(d_text.get(), text, text_len, hipMemcpyHostToDevice));
    out->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  SMG_HIP(d_sum.alloc(nblk));
  SMG_HIP(d_at.alloc(nblk + 1));
  SMG_HIP(d_fq.alloc(1));
  FaEntry h_end = {};
  SMG_HIP(hipMemsetAsync(d_fq.get(), 0, 8, 0));
  SMG_HIP(hipEventRecord(ev[0], 0));
  hipLaunchKernelGGL(k_fa_summary, dim3((unsigned)nblk), dim3(256), 0, 0, d_text.get(), text_len, g.block_bytes, d_sum.get());
  SMG_HIP(hipGetLastError());
  SMG_HIP(hipEventRecord(ev[1], 0));
  hipLaunchKernelGGL(k_fa_compose, dim3(1), dim3(256), 0, 0, d_sum.get(), nblk, d_at.get(), d_at + nblk);
  SMG_HIP(hipGetLastError());
  SMG_HIP(hipEventRecord(ev[2], 0));
  SMG_HIP(hipMemcpy(&h_end, d_at + nblk, sizeof(h_end), hipMemcpyDeviceToHost));
  const char *why = fa_refusal(text_len, h_end.state, h_end.hdr_off, 0);
  if (why) { snprintf(err, errlen, "%s", why); return -1; }
  SMG_HIP(d_bases.alloc(h_end.base_off ? h_end.base_off : 1));
  SMG_HIP(d_hdr.alloc(h_end.hdr_off));
  SMG_HIP(hipEventRecord(ev[3], 0));
  hipLaunchKernelGGL(k_fa_emit, dim3((unsigned)nblk), dim3(256), 0, 0, d_text.get(), text_len, g.block_bytes, d_at.get(), d_bases.get(), h_end.base_off,
                     d_hdr.get(), h_end.hdr_off, d_fq.get());
  SMG_HIP(hipGetLastError());
  SMG_HIP(hipEventRecord(ev[4], 0));
  SMG_HIP(hipEventSynchronize(ev[4]));
  SMG_HIP(hipEventElapsedTime(&out->pass_a_ms, ev[0], ev[1]));
  SMG_HIP(hipEventElapsedTime(&out->compose_ms, ev[1], ev[2]));
  SMG_HIP(hipEventElapsedTime(&out->pass_b_ms, ev[3], ev[4]));
  unsigned long long h_fq = 0;
  SMG_HIP(hipMemcpy(&h_fq, d_fq.get(), 8, hipMemcpyDeviceToHost));
  if ((why = fa_refusal(text_len, h_end.state, h_end.hdr_off, h_fq))) {
    snprintf(err, errlen, "%s", why);
    if (h_fq && out->keep_fastq_text) out->d_text = std::move(d_text);         // for smg_fastq_ref.hip: the text stays in HBM
    return -1;
  }
  std::vector<FaHeader> hdr((size_t)h_end.hdr_off);
  SMG_HIP(hipMemcpy(hdr.data(), d_hdr.get(), hdr.size() * sizeof(FaHeader), hipMemcpyDeviceToHost));
  out->seq_off.clear(); out->hdr_text_off.clear();
  for (const FaHeader &h : hdr) {
    if (h.text_off >= text_len || h.base_off > h_end.base_off || (!out->seq_off.empty() && h.base_off < out->seq_off.back())) { snprintf(err, errlen, "the two passes over the text disagree"); return -1; }
    out->seq_off.push_back(h.base_off); out->hdr_text_off.push_back(h.text_off);
  }
  out->seq_off.push_back(h_end.base_off);
  out->d_bases = std::move(d_bases); out->nbases = h_end.base_off;
  return 0;
}

}  // namespace smg

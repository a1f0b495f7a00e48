// smg_fastq_ref.hip -- a reference file with FASTQ records parsed in HBM (the rules: smg_fastq_ref.hpp).  Five launches on the
// stream of the index construction, none of which waits for another workgroup:
//   k_fq_count   one workgroup per block of text: its non-blank bytes and its candidates (prompts directly behind a '\n'), and per
//                granule of 64 bytes the non-blank bytes of the block in front of it;
//   k_fq_scan    one workgroup: the block counts become exclusive prefixes;
//   k_fq_cands   one workgroup per block again: the offsets of the candidates, one ascending list;
//   k_fq_walk    one wave goes through the records in order (fq_walk) and writes the record table, or the record it refuses;
//   k_fq_emit    one workgroup per block: the non-blank bytes inside the records' data ranges, compacted through LDS into d_bases.
// A workgroup takes FA_TILE bytes at a time, 16 per lane, as the FASTA kernels do, with the same tile steps (smg_text.hpp).
#include <stdint.h>
#include <stdio.h>
#include <chrono>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "smg_fastq_ref.hpp"
#include "smg_text.hpp"

namespace smg {

// blk_nb[b], blk_cd[b]: the counts of block b (a tile holds at most 4096 non-blank bytes and 2048 candidates: 16 bits each)
__global__ void __launch_bounds__(256) k_fq_count(const uint8_t *text, uint64_t len, uint32_t block_bytes, uint32_t *gran_nb, uint64_t *blk_nb, uint64_t *blk_cd) {
  __shared__ uint32_t wsum[4];
  const auto [b0, b1] = tx_block_range(len, block_bytes);
  uint32_t run_nb = 0, run_cd = 0;                                             // of the tiles so far; the same in every thread
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES], prev;
    uint64_t o;
    const uint32_t n = tx_lane_load<true>(text, t0, b1, &o, c, &prev);
    uint32_t tot;
    const uint32_t pre = tx_block_scan_sum(fq_lane_counts(c, n, prev), wsum, &tot);
    if (n && (threadIdx.x & 3u) == 0) gran_nb[o / FQ_GRAN] = run_nb + (pre & 0xFFFFu);
    run_nb += tot & 0xFFFFu; run_cd += tot >> 16;
  }
  if (threadIdx.x == 0) { blk_nb[blockIdx.x] = run_nb; blk_cd[blockIdx.x] = run_cd; }
}

// in place: a[i] becomes the sum of a[0, i), a[n] the sum of all; the same for b.  Every thread sums a stretch, thread 0 chains the
// 256 stretches, every thread walks its stretch again.
__global__ void __launch_bounds__(256) k_fq_scan(uint64_t *a, uint64_t *b, uint64_t n) {
  __shared__ uint64_t part[256][2];
  const uint64_t per = (n + 255) / 256, i0 = (uint64_t)threadIdx.x * per < n ? (uint64_t)threadIdx.x * per : n, i1 = i0 + per < n ? i0 + per : n;
  uint64_t sa = 0, sb = 0;
  for (uint64_t i = i0; i < i1; i++) { sa += a[i]; sb += b[i]; }
  part[threadIdx.x][0] = sa; part[threadIdx.x][1] = sb;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t ra = 0, rb = 0;
    for (uint32_t t = 0; t < 256; t++) { const uint64_t xa = part[t][0], xb = part[t][1]; part[t][0] = ra; part[t][1] = rb; ra += xa; rb += xb; }
    a[n] = ra; b[n] = rb;
  }
  __syncthreads();
  sa = part[threadIdx.x][0]; sb = part[threadIdx.x][1];
  for (uint64_t i = i0; i < i1; i++) { const uint64_t xa = a[i], xb = b[i]; a[i] = sa; b[i] = sb; sa += xa; sb += xb; }
}

__global__ void __launch_bounds__(256) k_fq_cands(const uint8_t *text, uint64_t len, uint32_t block_bytes, const uint64_t *blk_cd, uint64_t *cand, uint64_t ncand) {
  __shared__ uint32_t wsum[4];
  const auto [b0, b1] = tx_block_range(len, block_bytes);
  uint64_t at = blk_cd[blockIdx.x];
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES], prev;
    uint64_t o;
    const uint32_t n = tx_lane_load<true>(text, t0, b1, &o, c, &prev);
    uint32_t tot;
    uint32_t k = tx_block_scan_sum(fq_lane_counts(c, n, prev) >> 16, wsum, &tot);
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) {
      if (i < n) {
        if (fq_candidate(prev, c[i])) { if (at + k < ncand) cand[at + k] = o + i; k++; }
        prev = c[i];
      }
    }
    at += tot;
  }
}

// the three launches in front of a walk, for fastq_ref_parse_device and for the readers of other files (smg_reads_dev.hip)
hipError_t fq_launch_counts(hipStream_t st, const uint8_t *text, uint64_t len, uint32_t block_bytes, uint64_t nblk, uint32_t *gran_nb, uint64_t *blk_nb, uint64_t *blk_cd) {
  hipLaunchKernelGGL(k_fq_count, dim3((unsigned)nblk), dim3(256), 0, st, text, len, block_bytes, gran_nb, blk_nb, blk_cd);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : fq_launch_scan(st, blk_nb, blk_cd, nblk);
}
hipError_t fq_launch_scan(hipStream_t st, uint64_t *a, uint64_t *b, uint64_t n) {
  hipLaunchKernelGGL(k_fq_scan, dim3(1), dim3(256), 0, st, a, b, n);
  return hipGetLastError();
}
hipError_t fq_launch_cands(hipStream_t st, const uint8_t *text, uint64_t len, uint32_t block_bytes, uint64_t nblk, const uint64_t *blk_cd, uint64_t *cand, uint64_t ncand) {
  hipLaunchKernelGGL(k_fq_cands, dim3((unsigned)nblk), dim3(256), 0, st, text, len, block_bytes, blk_cd, cand, ncand);
  return hipGetLastError();
}

__global__ void __launch_bounds__(64) k_fq_walk(FqText t, FqRecord *rec, uint64_t cap, FqWalk *out) {
  FqWalk w;
  fq_walk(t, rec, cap, &w);
  if (threadIdx.x == 0) *out = w;
}

__global__ void __launch_bounds__(256) k_fq_emit(const uint8_t *text, uint64_t len, uint32_t block_bytes, const uint64_t *blk_nb, const FqRecord *rec, uint64_t nrec,
                                                 uint8_t *bases, uint64_t nbases) {
  __shared__ uint32_t wsum[4];
  __shared__ uint8_t stage[FA_TILE];                                           // the bases of a tile, compacted, before they go out in a row
  const auto [b0, b1] = tx_block_range(len, block_bytes);
  uint64_t u_tile = fq_rec_upper(rec, 0, nrec, b0);                            // the same in every thread
  uint64_t base = fq_block_base(rec, nrec, nbases, u_tile, b0, blk_nb[blockIdx.x]);
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES];
    uint64_t o;
    const uint32_t n = tx_lane_load(text, t0, b1, &o, c);
    const uint64_t u_hi = nrec - u_tile < FQ_REC_PER_TILE ? nrec : u_tile + FQ_REC_PER_TILE;
    uint64_t u = n ? fq_rec_upper(rec, u_tile, u_hi, o) : u_tile;
    uint64_t cur_d1 = u > 0 ? rec[u - 1].d1 : 0, next_d0 = u < nrec ? rec[u].d0 : ~0ull;
    uint32_t take = 0, cnt = 0;                                                // bit i: byte i is a base
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) {
      if (i < n) {
        const uint64_t x = o + i;
        while (next_d0 <= x) { cur_d1 = rec[u].d1; u++; next_d0 = u < nrec ? rec[u].d0 : ~0ull; }
        if (x < cur_d1 && !fa_isspace(c[i])) { take |= 1u << i; cnt++; }
      }
    }
    uint32_t tot;
    uint32_t pb = tx_block_scan_sum(cnt, wsum, &tot);
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) if (((take >> i) & 1u) && pb < FA_TILE) stage[pb++] = c[i];
    tx_stage_flush(stage, tot, bases, base, nbases);
    base += tot;
    u_tile = fq_rec_upper(rec, u_tile, u_hi, t0 + FA_TILE - 1);
  }
}

int fastq_ref_parse_device(const char *text, uint64_t text_len, uint32_t block_bytes, FastaParsed *out, char *err, size_t errlen) {
  DevMem<uint8_t> d_text = std::move(out->d_text);                                       // freed on every return
  if (!text_len) { snprintf(err, errlen, "%s", fa_refusal(0, FA_P, 0, 0)); return -1; }
  if (block_bytes < FA_BLOCK_MIN || (block_bytes & 63u)) { snprintf(err, errlen, "bad block size %u", block_bytes); return -1; }
  TextBlocks g;
  if (!text_blocks(text_len, block_bytes, &g)) { snprintf(err, errlen, "text of %llu bytes in blocks of %u: too many blocks", (unsigned long long)text_len, g.block_bytes); return -1; }
  const uint64_t nblk = g.nblk;
  DevMem<uint8_t> d_bases; DevMem<uint32_t> d_gran; DevMem<uint64_t> d_blk_nb, d_blk_cd, d_cand; DevMem<FqRecord> d_rec; DevMem<FqWalk> d_walk;
  DevEvent ev[7];
  for (DevEvent &e : ev) SMG_HIP(e.create());
  if (!d_text) {
    SMG_HIP(d_text.alloc(g.padded));
    const auto t0 = std::chrono::steady_clock::now();
    SMG_HIP(hipMemcpy(d_text.get(), text, text_len, hipMemcpyHostToDevice));
    out->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  SMG_HIP(d_gran.alloc(g.padded / FQ_GRAN));
  SMG_HIP(d_blk_nb.alloc(nblk + 1));
  SMG_HIP(d_blk_cd.alloc(nblk + 1));
  SMG_HIP(d_walk.alloc(1));
  SMG_HIP(hipEventRecord(ev[0], 0));
  SMG_HIP(fq_launch_counts(0, d_text.get(), text_len, g.block_bytes, nblk, d_gran.get(), d_blk_nb.get(), d_blk_cd.get()));
  SMG_HIP(hipEventRecord(ev[1], 0));
  uint64_t h_tot[2] = {0, 0};
  SMG_HIP(hipMemcpy(&h_tot[0], d_blk_nb + nblk, 8, hipMemcpyDeviceToHost));
  SMG_HIP(hipMemcpy(&h_tot[1], d_blk_cd + nblk, 8, hipMemcpyDeviceToHost));
  if (h_tot[0] > text_len || h_tot[1] > text_len) { snprintf(err, errlen, "the counts of the text exceed its length"); return -1; }
  const uint64_t ncand = h_tot[1], cap = ncand + 1;
  SMG_HIP(d_cand.alloc(cap));
  SMG_HIP(d_rec.alloc(cap));
  SMG_HIP(hipEventRecord(ev[2], 0));
  SMG_HIP(fq_launch_cands(0, d_text.get(), text_len, g.block_bytes, nblk, d_blk_cd.get(), d_cand.get(), ncand));
  SMG_HIP(hipEventRecord(ev[3], 0));
  FqText t;
  t.text = d_text.get(); t.len = text_len; t.block_bytes = g.block_bytes; t.pad = 0; t.blk_nb = d_blk_nb.get(); t.gran_nb = d_gran.get();
  t.cand = d_cand.get(); t.ncand = ncand; t.nblk = nblk;
  hipLaunchKernelGGL(k_fq_walk, dim3(1), dim3(64), 0, 0, t, d_rec.get(), cap, d_walk.get());
  SMG_HIP(hipGetLastError());
  SMG_HIP(hipEventRecord(ev[4], 0));
  FqWalk h_walk = {};
  SMG_HIP(hipMemcpy(&h_walk, d_walk.get(), sizeof(h_walk), hipMemcpyDeviceToHost));
  const std::string why = fq_refusal(h_walk, text, text_len);
  if (!why.empty()) { snprintf(err, errlen, "%s", why.c_str()); return -1; }
  if (h_walk.nrec > cap || h_walk.nbases > h_tot[0]) { snprintf(err, errlen, "the walk over the records disagrees with the counts of the text"); return -1; }
  SMG_HIP(d_bases.alloc(h_walk.nbases ? h_walk.nbases : 1));
  SMG_HIP(hipEventRecord(ev[5], 0));
  hipLaunchKernelGGL(k_fq_emit, dim3((unsigned)nblk), dim3(256), 0, 0, d_text.get(), text_len, g.block_bytes, d_blk_nb.get(), d_rec.get(), h_walk.nrec,
                     d_bases.get(), h_walk.nbases);
  SMG_HIP(hipGetLastError());
  SMG_HIP(hipEventRecord(ev[6], 0));
  SMG_HIP(hipEventSynchronize(ev[6]));
  float ms_counts = 0, ms_cands = 0;
  SMG_HIP(hipEventElapsedTime(&ms_counts, ev[0], ev[1]));
  SMG_HIP(hipEventElapsedTime(&ms_cands, ev[2], ev[3]));
  out->pass_a_ms = ms_counts + ms_cands;
  SMG_HIP(hipEventElapsedTime(&out->compose_ms, ev[3], ev[4]));
  SMG_HIP(hipEventElapsedTime(&out->pass_b_ms, ev[5], ev[6]));
  std::vector<FqRecord> rec((size_t)h_walk.nrec);
  SMG_HIP(hipMemcpy(rec.data(), d_rec.get(), rec.size() * sizeof(FqRecord), hipMemcpyDeviceToHost));
  out->seq_off.clear(); out->hdr_text_off.clear();
  for (const FqRecord &r : rec) {
    if (r.hdr_off >= text_len || r.base_off > h_walk.nbases || (!out->seq_off.empty() && r.base_off < out->seq_off.back())) { snprintf(err, errlen, "the record table is out of order"); return -1; }
    out->seq_off.push_back(r.base_off); out->hdr_text_off.push_back(r.hdr_off);
  }
  out->seq_off.push_back(h_walk.nbases);
  out->d_bases = std::move(d_bases); out->nbases = h_walk.nbases;
  return 0;
}

}  // namespace smg


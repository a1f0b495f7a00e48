// smg_fastq_ref.hip -- a reference file with FASTQ records parsed in HBM (the rules: smg_fastq_ref.hpp).  Five launches on the
// stream of the index construction, none of which waits for another workgroup:
//   k_fq_count   one workgroup per block of text: its non-blank bytes and its candidates (prompts directly behind a '\n'), and per
//                granule of 64 bytes the non-blank bytes of the block in front of it;
//   k_fq_scan    one workgroup: the block counts become exclusive prefixes;
//   k_fq_cands   one workgroup per block again: the offsets of the candidates, one ascending list;
//   k_fq_walk    one wave goes through the records in order (fq_walk) and writes the record table, or the record it refuses;
//   k_fq_emit    one workgroup per block: the non-blank bytes inside the records' data ranges, compacted through LDS into d_bases.
// A workgroup takes FA_TILE bytes at a time, 16 per lane, as the FASTA kernels do (smg_fasta.hip).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "smg_fastq_ref.hpp"

namespace smg {

#define FQ_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(err, errlen, "%s: %s", #x, hipGetErrorString(e_)); goto fail; } } while (0)

// blk_nb[b], blk_cd[b]: the counts of block b (a tile holds at most 4096 non-blank bytes and 2048 candidates: 16 bits each)
__global__ void __launch_bounds__(256) k_fq_count(const uint8_t *text, uint64_t len, uint32_t block_bytes, uint32_t *gran_nb, uint64_t *blk_nb, uint64_t *blk_cd) {
  __shared__ uint32_t wsum[4];
  const uint64_t b0 = (uint64_t)blockIdx.x * block_bytes, b1 = len - b0 < block_bytes ? len : b0 + block_bytes;
  uint32_t run_nb = 0, run_cd = 0;                                             // of the tiles so far; the same in every thread
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES], prev;
    uint64_t o;
    const uint32_t n = fq_lane_load(text, t0, b1, &o, c, &prev);
    uint32_t tot;
    const uint32_t pre = fq_block_scan_sum(fq_lane_counts(c, n, prev), wsum, &tot);
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
  const uint64_t b0 = (uint64_t)blockIdx.x * block_bytes, b1 = len - b0 < block_bytes ? len : b0 + block_bytes;
  uint64_t at = blk_cd[blockIdx.x];
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES], prev;
    uint64_t o;
    const uint32_t n = fq_lane_load(text, t0, b1, &o, c, &prev);
    uint32_t tot;
    uint32_t k = fq_block_scan_sum(fq_lane_counts(c, n, prev) >> 16, wsum, &tot);
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

// the three launches in front of a walk, for the readers of other files (smg_reads_dev.hip): what fastq_ref_parse_device launches itself
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
  const uint64_t b0 = (uint64_t)blockIdx.x * block_bytes, b1 = len - b0 < block_bytes ? len : b0 + block_bytes;
  uint64_t u_tile = fq_rec_upper(rec, 0, nrec, b0);                            // the same in every thread
  uint64_t base = fq_block_base(rec, nrec, nbases, u_tile, b0, blk_nb[blockIdx.x]);
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES], prev;
    uint64_t o;
    const uint32_t n = fq_lane_load(text, t0, b1, &o, c, &prev);
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
    uint32_t pb = fq_block_scan_sum(cnt, wsum, &tot);
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) if (((take >> i) & 1u) && pb < FA_TILE) stage[pb++] = c[i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < tot; i += 256) if (base + i < nbases) bases[base + i] = stage[i];
    __syncthreads();
    base += tot;
    u_tile = fq_rec_upper(rec, u_tile, u_hi, t0 + FA_TILE - 1);
  }
}

int fastq_ref_parse_device(const char *text, uint64_t text_len, uint32_t block_bytes, uint8_t *d_text, FastaParsed *out, char *err, size_t errlen) {
  uint8_t *d_bases = nullptr;
  uint32_t *d_gran = nullptr;
  uint64_t *d_blk_nb = nullptr, *d_blk_cd = nullptr, *d_cand = nullptr, h_tot[2] = {0, 0};
  FqRecord *d_rec = nullptr;
  FqWalk *d_walk = nullptr, h_walk;
  hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<FqRecord> rec;
  std::string why;
  memset(&h_walk, 0, sizeof(h_walk));
  if (!text_len) { snprintf(err, errlen, "%s", fa_refusal(0, FA_P, 0, 0)); (void)hipFree(d_text); return -1; }
  if (block_bytes < FA_BLOCK_MIN || (block_bytes & 63u)) { snprintf(err, errlen, "bad block size %u", block_bytes); (void)hipFree(d_text); return -1; }
  while ((text_len + block_bytes - 1) / block_bytes > (1ull << 20) && block_bytes < FA_BLOCK_MAX) block_bytes *= 2;      // as fasta_parse_device
  {
  const uint64_t nblk = (text_len + block_bytes - 1) / block_bytes, padded = (text_len + FA_TILE - 1) / FA_TILE * FA_TILE;
  FqText t;
  if (nblk > 0x7fffffffull) { snprintf(err, errlen, "text of %llu bytes in blocks of %u: too many blocks", (unsigned long long)text_len, block_bytes); (void)hipFree(d_text); return -1; }
  for (hipEvent_t &e : ev) FQ_HIP(hipEventCreate(&e));
  if (!d_text) {
    FQ_HIP(hipMalloc((void **)&d_text, padded));
    const auto t0 = std::chrono::steady_clock::now();
    FQ_HIP(hipMemcpy(d_text, text, text_len, hipMemcpyHostToDevice));
    out->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  FQ_HIP(hipMalloc((void **)&d_gran, padded / FQ_GRAN * sizeof(uint32_t)));
  FQ_HIP(hipMalloc((void **)&d_blk_nb, (nblk + 1) * sizeof(uint64_t)));
  FQ_HIP(hipMalloc((void **)&d_blk_cd, (nblk + 1) * sizeof(uint64_t)));
  FQ_HIP(hipMalloc((void **)&d_walk, sizeof(FqWalk)));
  FQ_HIP(hipEventRecord(ev[0], 0));
  hipLaunchKernelGGL(k_fq_count, dim3((unsigned)nblk), dim3(256), 0, 0, d_text, text_len, block_bytes, d_gran, d_blk_nb, d_blk_cd);
  FQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_fq_scan, dim3(1), dim3(256), 0, 0, d_blk_nb, d_blk_cd, nblk);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipEventRecord(ev[1], 0));
  FQ_HIP(hipMemcpy(&h_tot[0], d_blk_nb + nblk, 8, hipMemcpyDeviceToHost));
  FQ_HIP(hipMemcpy(&h_tot[1], d_blk_cd + nblk, 8, hipMemcpyDeviceToHost));
  if (h_tot[0] > text_len || h_tot[1] > text_len) { snprintf(err, errlen, "the counts of the text exceed its length"); goto fail; }
  {
  const uint64_t ncand = h_tot[1], cap = ncand + 1;
  FQ_HIP(hipMalloc((void **)&d_cand, cap * sizeof(uint64_t)));
  FQ_HIP(hipMalloc((void **)&d_rec, cap * sizeof(FqRecord)));
  FQ_HIP(hipEventRecord(ev[2], 0));
  hipLaunchKernelGGL(k_fq_cands, dim3((unsigned)nblk), dim3(256), 0, 0, d_text, text_len, block_bytes, d_blk_cd, d_cand, ncand);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipEventRecord(ev[3], 0));
  t.text = d_text; t.len = text_len; t.block_bytes = block_bytes; t.pad = 0; t.blk_nb = d_blk_nb; t.gran_nb = d_gran; t.cand = d_cand; t.ncand = ncand; t.nblk = nblk;
  hipLaunchKernelGGL(k_fq_walk, dim3(1), dim3(64), 0, 0, t, d_rec, cap, d_walk);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipEventRecord(ev[4], 0));
  FQ_HIP(hipMemcpy(&h_walk, d_walk, sizeof(h_walk), hipMemcpyDeviceToHost));
  why = fq_refusal(h_walk, text, text_len);
  if (!why.empty()) { snprintf(err, errlen, "%s", why.c_str()); goto fail; }
  if (h_walk.nrec > cap || h_walk.nbases > h_tot[0]) { snprintf(err, errlen, "the walk over the records disagrees with the counts of the text"); goto fail; }
  FQ_HIP(hipMalloc((void **)&d_bases, h_walk.nbases ? h_walk.nbases : 1));
  FQ_HIP(hipEventRecord(ev[5], 0));
  hipLaunchKernelGGL(k_fq_emit, dim3((unsigned)nblk), dim3(256), 0, 0, d_text, text_len, block_bytes, d_blk_nb, d_rec, h_walk.nrec, d_bases, h_walk.nbases);
  FQ_HIP(hipGetLastError());
  FQ_HIP(hipEventRecord(ev[6], 0));
  FQ_HIP(hipEventSynchronize(ev[6]));
  {
    float a = 0, b = 0;
    FQ_HIP(hipEventElapsedTime(&a, ev[0], ev[1]));
    FQ_HIP(hipEventElapsedTime(&b, ev[2], ev[3]));
    out->pass_a_ms = a + b;
    FQ_HIP(hipEventElapsedTime(&out->compose_ms, ev[3], ev[4]));
    FQ_HIP(hipEventElapsedTime(&out->pass_b_ms, ev[5], ev[6]));
  }
  rec.resize((size_t)h_walk.nrec);
  FQ_HIP(hipMemcpy(rec.data(), d_rec, rec.size() * sizeof(FqRecord), hipMemcpyDeviceToHost));
  out->seq_off.clear(); out->hdr_text_off.clear();
  for (const FqRecord &r : rec) {
    if (r.hdr_off >= text_len || r.base_off > h_walk.nbases || (!out->seq_off.empty() && r.base_off < out->seq_off.back())) { snprintf(err, errlen, "the record table is out of order"); goto fail; }
    out->seq_off.push_back(r.base_off); out->hdr_text_off.push_back(r.hdr_off);
  }
  out->seq_off.push_back(h_walk.nbases);
  out->d_bases = d_bases; out->nbases = h_walk.nbases;
  }
  }
  (void)hipFree(d_text); (void)hipFree(d_gran); (void)hipFree(d_blk_nb); (void)hipFree(d_blk_cd); (void)hipFree(d_cand); (void)hipFree(d_rec); (void)hipFree(d_walk);
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  return 0;
fail:
  (void)hipFree(d_text); (void)hipFree(d_gran); (void)hipFree(d_blk_nb); (void)hipFree(d_blk_cd); (void)hipFree(d_cand); (void)hipFree(d_rec); (void)hipFree(d_walk); (void)hipFree(d_bases);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return -1;
}

}  // namespace smg

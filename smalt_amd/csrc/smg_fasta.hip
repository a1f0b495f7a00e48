// smg_fasta.hip -- the text of a FASTA reference parsed in HBM: bases, sequence offsets and header positions for
// build_index_device (smg_indexbuild.hip).  The automaton is the one of smg_fasta.hpp; a block of text does not know the state
// it is entered in, so the parse is three launches on the stream of the index construction:
//   pass A   k_fa_summary: one workgroup per block of text; per entry state the exit state, the bases and the headers of the block;
//   compose  k_fa_compose: one workgroup walks the summaries in block order: entry state, first base and first header of every block;
//   pass B   k_fa_emit: one workgroup per block again, now with its entry state: bases compacted into d_bases, one record per header.
// Inside a block a workgroup takes FA_TILE bytes at a time, 16 per lane (one 128-bit load, a wave reads 1 KiB in a row).  A lane
// runs its 16 bytes for the four possible entry states at once (FaLane); an exclusive scan of the lanes' state maps under
// composition -- wave shuffles, then the four wave totals through LDS -- gives every lane its true entry state, a sum over the
// counts that belong to that state its place in the output.  No workgroup waits for another one.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <hip/hip_runtime.h>
#include "smg_fasta.hpp"

namespace smg {

#define FA_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(err, errlen, "%s: %s", #x, hipGetErrorString(e_)); goto fail; } } while (0)

// the lane's bytes of the tile that starts at t0: text[o, o + n), n <= 16.  The text buffer is padded to a multiple of FA_TILE
// behind `len`, and o is a multiple of 16, so the load stays inside the allocation; bytes behind `end` are not looked at.
__device__ inline uint32_t fa_lane_load(const uint8_t *text, uint64_t t0, uint64_t end, uint64_t *o_out, uint8_t (&c)[FA_LANE_BYTES]) {
  const uint64_t o = t0 + (uint64_t)threadIdx.x * FA_LANE_BYTES;
  *o_out = o;
  if (o >= end) return 0;
  const uint4 v = *reinterpret_cast<const uint4 *>(text + o);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t i = 0; i < FA_LANE_BYTES; i++) c[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  return end - o < FA_LANE_BYTES ? (uint32_t)(end - o) : FA_LANE_BYTES;
}

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

// exclusive sum of v over the workgroup; *total: the sum.  wsum: 4 words of LDS
__device__ inline uint32_t fa_block_scan_sum(uint32_t v, uint32_t *wsum, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t s = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(s, d); if (lane >= d) s += o; }
  __syncthreads();
  if (lane == 63) wsum[wave] = s;
  __syncthreads();
  uint32_t pre = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) { if (w == wave) pre = all; all += wsum[w]; }
  *total = all;
  return pre + s - v;
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
  const uint64_t b0 = (uint64_t)blockIdx.x * block_bytes, b1 = len - b0 < block_bytes ? len : b0 + block_bytes;
  uint32_t map = FA_MAP_ID, nb[FA_NENTRY] = {0, 0, 0, 0}, nh[FA_NENTRY] = {0, 0, 0, 0};       // of the tiles so far; the same in every thread
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES];
    uint64_t o;
    const uint32_t n = fa_lane_load(text, t0, b1, &o, c);
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
  const uint64_t b0 = (uint64_t)blockIdx.x * block_bytes, b1 = len - b0 < block_bytes ? len : b0 + block_bytes;
  const FaEntry a = at[blockIdx.x];
  uint32_t state = a.state, fq = 0;
  uint64_t base = a.base_off, hd = a.hdr_off;
  if (state >= FA_NENTRY) return;                                              // the text is refused
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES];
    uint64_t o;
    const uint32_t n = fa_lane_load(text, t0, b1, &o, c);
    FaLane l;
    fa_lane_init(l);
#pragma unroll
    for (uint32_t i = 0; i < FA_LANE_BYTES; i++) if (i < n) fa_lane_byte(l, c[i]);
    uint32_t tile_map, tot;
    const uint32_t excl = fa_block_scan_map(l.map, wmap, &tile_map);
    uint32_t st = fa_map_at(excl, state);
    const uint32_t pre = fa_block_scan_sum(fa_lane_count(l.nb, st) | fa_lane_count(l.nh, st) << 16, wsum, &tot);
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
    __syncthreads();
    const uint32_t tb = tot & 0xFFFFu;
    for (uint32_t i = threadIdx.x; i < tb; i += 256) if (base + i < nbases) bases[base + i] = stage[i];
    __syncthreads();
    base += tb; hd += tot >> 16;
    state = fa_map_at(tile_map, state);
    if (state >= FA_NENTRY) break;                                             // uniform
  }
  for (int d = 32; d > 0; d >>= 1) fq += __shfl_xor(fq, d);
  if ((threadIdx.x & 63) == 0 && fq) atomicAdd(nfastq, (unsigned long long)fq);
}

int fasta_parse_device(const char *text, uint64_t text_len, uint32_t block_bytes, FastaParsed *out, char *err, size_t errlen) {
  uint8_t *d_text = nullptr, *d_bases = nullptr;
  FaSummary *d_sum = nullptr;
  FaEntry *d_at = nullptr, h_end;
  FaHeader *d_hdr = nullptr;
  unsigned long long *d_fq = nullptr, h_fq = 0;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<FaHeader> hdr;
  const char *why = nullptr;
  memset(&h_end, 0, sizeof(h_end));
  if (!text_len) { snprintf(err, errlen, "%s", fa_refusal(0, FA_P, 0, 0)); return -1; }
  if (block_bytes < FA_BLOCK_MIN || (block_bytes & 63u)) { snprintf(err, errlen, "bad block size %u", block_bytes); return -1; }
  // the compose step is one workgroup: block sizes far below the default are for small texts (tests); a large text gets at most 2^20 blocks
  while ((text_len + block_bytes - 1) / block_bytes > (1ull << 20) && block_bytes < FA_BLOCK_MAX) block_bytes *= 2;
  {
  const uint64_t nblk = (text_len + block_bytes - 1) / block_bytes, padded = (text_len + FA_TILE - 1) / FA_TILE * FA_TILE;
  if (nblk > 0x7fffffffull) { snprintf(err, errlen, "text of %llu bytes in blocks of %u: too many blocks", (unsigned long long)text_len, block_bytes); return -1; }
  for (hipEvent_t &e : ev) FA_HIP(hipEventCreate(&e));
  FA_HIP(hipMalloc((void **)&d_text, padded));
  {
    const auto t0 = std::chrono::steady_clock::now();
    FA_HIP(hipMemcpy(d_text, text, text_len, hipMemcpyHostToDevice));
    out->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  FA_HIP(hipMalloc((void **)&d_sum, nblk * sizeof(FaSummary)));
  FA_HIP(hipMalloc((void **)&d_at, (nblk + 1) * sizeof(FaEntry)));
  FA_HIP(hipMalloc((void **)&d_fq, 8));
  FA_HIP(hipMemsetAsync(d_fq, 0, 8, 0));
  FA_HIP(hipEventRecord(ev[0], 0));
  hipLaunchKernelGGL(k_fa_summary, dim3((unsigned)nblk), dim3(256), 0, 0, d_text, text_len, block_bytes, d_sum);
  FA_HIP(hipGetLastError());
  FA_HIP(hipEventRecord(ev[1], 0));
  hipLaunchKernelGGL(k_fa_compose, dim3(1), dim3(256), 0, 0, d_sum, nblk, d_at, d_at + nblk);
  FA_HIP(hipGetLastError());
  FA_HIP(hipEventRecord(ev[2], 0));
  FA_HIP(hipMemcpy(&h_end, d_at + nblk, sizeof(h_end), hipMemcpyDeviceToHost));
  if ((why = fa_refusal(text_len, h_end.state, h_end.hdr_off, 0))) { snprintf(err, errlen, "%s", why); goto fail; }
  FA_HIP(hipMalloc((void **)&d_bases, h_end.base_off ? h_end.base_off : 1));
  FA_HIP(hipMalloc((void **)&d_hdr, h_end.hdr_off * sizeof(FaHeader)));
  FA_HIP(hipEventRecord(ev[3], 0));
  hipLaunchKernelGGL(k_fa_emit, dim3((unsigned)nblk), dim3(256), 0, 0, d_text, text_len, block_bytes, d_at, d_bases, h_end.base_off, d_hdr, h_end.hdr_off, d_fq);
  FA_HIP(hipGetLastError());
  FA_HIP(hipEventRecord(ev[4], 0));
  FA_HIP(hipEventSynchronize(ev[4]));
  FA_HIP(hipEventElapsedTime(&out->pass_a_ms, ev[0], ev[1]));
  FA_HIP(hipEventElapsedTime(&out->compose_ms, ev[1], ev[2]));
  FA_HIP(hipEventElapsedTime(&out->pass_b_ms, ev[3], ev[4]));
  FA_HIP(hipMemcpy(&h_fq, d_fq, 8, hipMemcpyDeviceToHost));
  if ((why = fa_refusal(text_len, h_end.state, h_end.hdr_off, h_fq))) {
    snprintf(err, errlen, "%s", why);
    if (h_fq && out->keep_fastq_text) { out->d_text = d_text; d_text = nullptr; }        // for smg_fastq_ref.hip: the text stays in HBM
    goto fail;
  }
  hdr.resize((size_t)h_end.hdr_off);
  FA_HIP(hipMemcpy(hdr.data(), d_hdr, hdr.size() * sizeof(FaHeader), hipMemcpyDeviceToHost));
  out->seq_off.clear(); out->hdr_text_off.clear();
  for (const FaHeader &h : hdr) {
    if (h.text_off >= text_len || h.base_off > h_end.base_off || (!out->seq_off.empty() && h.base_off < out->seq_off.back())) { snprintf(err, errlen, "the two passes over the text disagree"); goto fail; }
    out->seq_off.push_back(h.base_off); out->hdr_text_off.push_back(h.text_off);
  }
  out->seq_off.push_back(h_end.base_off);
  out->d_bases = d_bases; out->nbases = h_end.base_off;
  }
  (void)hipFree(d_text); (void)hipFree(d_sum); (void)hipFree(d_at); (void)hipFree(d_hdr); (void)hipFree(d_fq);
  for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  return 0;
fail:
  (void)hipFree(d_text); (void)hipFree(d_sum); (void)hipFree(d_at); (void)hipFree(d_hdr); (void)hipFree(d_fq); (void)hipFree(d_bases);
  for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  return -1;
}

}  // namespace smg

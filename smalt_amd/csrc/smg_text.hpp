// smg_text.hpp -- what the readers of text in HBM share (smg_fasta.hip, smg_fastq_ref.hip, smg_reads_dev.hip): how a text is cut
// into blocks, and the steps of a workgroup of 256 threads that takes its block FA_TILE bytes at a time, 16 per lane.  The wave
// primitives of smg_exec.h are for workgroups of one wave; these are for four.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "smg_fasta.hpp"

namespace smg {

// One workgroup per block of block_bytes: block sizes far below the default are for small texts (tests), a large text gets at most
// 2^20 blocks (the steps that chain the blocks are one workgroup).  padded: the bytes of the text's buffer, a multiple of FA_TILE.
struct TextBlocks { uint32_t block_bytes; uint64_t nblk, padded; };
// false: the text cannot be cut into fewer than 2^31 blocks
inline bool text_blocks(uint64_t len, uint32_t block_bytes, TextBlocks *g) {
  while ((len + block_bytes - 1) / block_bytes > (1ull << 20) && block_bytes < FA_BLOCK_MAX) block_bytes *= 2;
  g->block_bytes = block_bytes;
  g->nblk = (len + block_bytes - 1) / block_bytes;
  g->padded = (len + FA_TILE - 1) / FA_TILE * FA_TILE;
  return g->nblk <= 0x7fffffffull;
}

#if defined(__HIPCC__)
// the bytes [b0, b1) of the text that belong to this workgroup's block
struct TxRange { uint64_t b0, b1; };
__device__ inline TxRange tx_block_range(uint64_t len, uint32_t block_bytes) {
  const uint64_t b0 = (uint64_t)blockIdx.x * block_bytes;
  return TxRange{b0, len - b0 < block_bytes ? len : b0 + block_bytes};
}

// the lane's bytes of the tile that starts at t0: text[o, o + n), n <= 16, and with PREV the byte in front of them (0: none).  The
// text buffer is padded to a multiple of FA_TILE behind `len`, and o is a multiple of 16, so the load stays inside the allocation;
// bytes behind `end` are not looked at.
template <bool PREV = false>
__device__ inline uint32_t tx_lane_load(const uint8_t *text, uint64_t t0, uint64_t end, uint64_t *o_out, uint8_t (&c)[FA_LANE_BYTES], uint8_t *prev = nullptr) {
  const uint64_t o = t0 + (uint64_t)threadIdx.x * FA_LANE_BYTES;
  *o_out = o;
  if (PREV) *prev = 0;
  if (o >= end) return 0;
  const uint4 v = *reinterpret_cast<const uint4 *>(text + o);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t i = 0; i < FA_LANE_BYTES; i++) c[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  if (PREV && o > 0) *prev = text[o - 1];
  return end - o < FA_LANE_BYTES ? (uint32_t)(end - o) : FA_LANE_BYTES;
}

// two 64-bit sums that are scanned together
struct TxPair { uint64_t a, b; };
__device__ inline TxPair operator+(TxPair x, TxPair y) { return TxPair{x.a + y.a, x.b + y.b}; }
__device__ inline TxPair operator-(TxPair x, TxPair y) { return TxPair{x.a - y.a, x.b - y.b}; }
__device__ inline uint32_t tx_shfl_up(uint32_t v, uint32_t d) { return __shfl_up(v, d); }
__device__ inline TxPair tx_shfl_up(TxPair v, uint32_t d) {
  return TxPair{(uint64_t)__shfl_up((unsigned long long)v.a, d), (uint64_t)__shfl_up((unsigned long long)v.b, d)};
}

// exclusive sum of v over the workgroup (256 threads); *total: the sum.  T: uint32_t (also two 16-bit counts in one word) or
// TxPair.  Wave shuffles, then the four wave totals through wsum: 4 values of LDS
template <class T>
__device__ inline T tx_block_scan_sum(T v, T *wsum, T *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T s = v;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) { const T o = tx_shfl_up(s, d); if (lane >= d) s = s + o; }
  __syncthreads();                       // the last use of wsum is over
  if (lane == 63) wsum[wave] = s;
  __syncthreads();
  T pre = T(), all = T();
#pragma unroll
  for (uint32_t w = 0; w < 4; w++) { if (w == wave) pre = all; all = all + wsum[w]; }
  *total = all;
  return pre + s - v;
}

// the n bases a tile has compacted into `stage` go out in a row to bases[base, base + n); nothing is written at or behind nbases.
// Behind the first barrier the stage is whole, behind the second it is free for the next tile.
__device__ inline void tx_stage_flush(const uint8_t *stage, uint32_t n, uint8_t *bases, uint64_t base, uint64_t nbases) {
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += 256) if (base + i < nbases) bases[base + i] = stage[i];
  __syncthreads();
}
#endif

}  // namespace smg

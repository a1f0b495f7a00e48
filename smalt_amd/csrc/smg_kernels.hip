// smg_kernels.hip -- gfx950 kernels of libsmaltgpu: thin wave-per-read wrappers around the
// stage functions of smg_stages.hpp, and the wide Smith-Waterman score pass (K2a).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "smg_kernels.h"
#include "smg_stages.hpp"

namespace smg {

// ---------------------------------------------------------------------------------------
// read encoding: ASCII -> 3-bit codes (sequence.c:287-322) + reverse complement
// (sequence.c:884-896: non-standard codes are kept).  One wave per read.
// ---------------------------------------------------------------------------------------
__device__ inline uint8_t code_of(uint8_t c) {
  c &= 0xDF;   // upper case for letters
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'U') ? 3 : 5;
}

__global__ void __launch_bounds__(64) k_encode(const uint8_t *bases, const uint64_t *off, uint32_t n, uint8_t *codes, uint8_t *codes_rc) {
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint64_t o = off[r];
    const uint32_t len = (uint32_t)(off[r + 1] - o);
    for (uint32_t i = threadIdx.x; i < len; i += 64) {
      uint8_t c = code_of(bases[o + i]);
      codes[o + i] = c;
      codes_rc[o + len - 1 - i] = (c & 4) ? c : (uint8_t)(3 - c);
    }
  }
}

// The reads of one round of a block of pairs, taken from the two batches that are resident in HBM (reads and mates): read i of
// the round is read ids[i] >> 1 of batch ids[i] & 1.  One workgroup per read, bytes copied 16 at a time where both sides
// allow it (HBM to HBM, coalesced on both ends).
__global__ void __launch_bounds__(64) k_gather_reads(uint8_t *dst_bases, uint8_t *dst_quals, const uint64_t *dst_off, uint32_t n, const uint32_t *ids,
                                                     const uint8_t *b0, const uint8_t *b1, const uint8_t *q0, const uint8_t *q1, const uint64_t *o0, const uint64_t *o1) {
  for (uint32_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint32_t id = ids[r], w = id & 1u, i = id >> 1;
    const uint64_t so = w ? o1[i] : o0[i], d = dst_off[r];
    const uint32_t len = (uint32_t)(dst_off[r + 1] - d);
    const uint8_t *sb = (w ? b1 : b0) + so, *sq = dst_quals ? (w ? q1 : q0) + so : nullptr;
    if ((((uintptr_t)sb | (uintptr_t)(dst_bases + d)) & 15u) == 0 && (!sq || (((uintptr_t)sq | (uintptr_t)(dst_quals + d)) & 15u) == 0)) {
      const uint32_t nv = len >> 4;
      for (uint32_t v = threadIdx.x; v < nv; v += 64) {
        ((uint4 *)(dst_bases + d))[v] = ((const uint4 *)sb)[v];
        if (sq) ((uint4 *)(dst_quals + d))[v] = ((const uint4 *)sq)[v];
      }
      for (uint32_t t = (nv << 4) + threadIdx.x; t < len; t += 64) { dst_bases[d + t] = sb[t]; if (sq) dst_quals[d + t] = sq[t]; }
    } else
      for (uint32_t t = threadIdx.x; t < len; t += 64) { dst_bases[d + t] = sb[t]; if (sq) dst_quals[d + t] = sq[t]; }
  }
}

// ---------------------------------------------------------------------------------------
// S1 + S2: one wave per (read, strand); scratch in LDS when it fits, else in HBM slots
// ---------------------------------------------------------------------------------------
// Stage code reaches its LDS arrays through generic pointers (the same source serves HBM slots).  A flat
// access whose register address lies below the LDS aperture faults even if the instruction offset
// brings it back inside (e.g. a[i + 1] with i == -1 compiled as base a + 4*i, offset 4), so no array
// starts at LDS offset 0.
enum : uint32_t { LDS_GUARD = 64 };

// Persistent workgroups take the next item from a batch-wide cursor: per-read cost is heavy-tailed (repeat-rich
// reads), a static stride leaves most of the chip idle behind the slowest workgroup.
__device__ inline uint32_t next_item(uint32_t *cursor, uint32_t *lds_slot) {
  __syncthreads();
  if (threadIdx.x == 0) *lds_slot = atomicAdd(cursor, 1u);
  __syncthreads();
  return *lds_slot;
}

__global__ void __launch_bounds__(64) k_seed(Batch b, DevIndex ix, MapPar p, uint8_t *gscratch, size_t gbytes, int use_lds) {
  extern __shared__ __align__(16) uint8_t lds[];
  uint8_t *base = use_lds ? lds + LDS_GUARD : gscratch + gbytes * blockIdx.x;
  SeedScratch x = seed_scratch_carve(base, b.qmax, b.fine_idx ? (int)FINE_S : ix.s);
  unsigned long long nlook = 0;
  __shared__ uint32_t qslot;
  for (uint32_t rs = next_item(b.next_item + 0, &qslot); rs < 2 * b.nreads; rs = next_item(b.next_item + 0, &qslot)) {
    nlook += stage_seed(b, read_index(b, ix, rs >> 1), p, rs >> 1, rs & 1, x);
    __syncthreads();
  }
  if (threadIdx.x == 0 && nlook) atomicAdd(b.work + WK_LOOKUPS, nlook);
}

// The on-the-fly index of rmapPair's rescue round (rmap.c:495-517 setupFineHashTable -> hashTableSetUp with an interval set,
// hashidx.c:549-575): perfect type, k = 5, s = 1, over the windows of ONE read's intervals.  One wave per read: key
// histogram in LDS, exclusive scan = idx, positions scattered behind per-key cursors, then every key's (short) list put
// in ascending order -- the reference fills the lists in ascending order because its intervals are sorted and disjoint.
__global__ void __launch_bounds__(64) k_fine_index(Batch b, DevIndex ix) {
  __shared__ uint32_t cnt[FINE_NKEYS + 1];
  for (uint32_t r = blockIdx.x; r < b.nreads; r += gridDim.x) {
    uint32_t *idx = b.fine_idx + (size_t)r * FINE_IDX_STRIDE;
    uint32_t *pos = b.fine_pos + b.fine_off[r];
    const uint32_t cap = b.fine_off[r + 1] - b.fine_off[r];
    const uint32_t niv = b.iv_off[r + 1] - b.iv_off[r];
    const IvRec *iv = b.iv + b.iv_off[r];
    for (uint32_t i = threadIdx.x; i <= (uint32_t)FINE_NKEYS; i += 64) cnt[i] = 0;
    __syncthreads();
    for (int pass = 0; pass < 2; pass++) {
      for (uint32_t v = 0; v < niv; v++) {
        const uint32_t sl = iv[v].hi - iv[v].lo + 1;
        if (sl < (uint32_t)FINE_K) continue;                        // hashidx.c:561-563
        const uint64_t g0 = ix.sop[iv[v].sx] + iv[v].lo;
        const uint32_t nk = sl - FINE_K + 1;
        for (uint32_t j = threadIdx.x; j < nk; j += 64) {
          uint32_t w = 0;
          bool ok = true;
          for (int t = 0; t < FINE_K; t++) { const uint32_t c = ref_code(ix.packed, g0 + j + (uint32_t)t); if (c & 4u) ok = false; w = (w << 2) | (c & 3u); }
          if (!ok) continue;                                         // words with non-standard bases are not indexed (hashidx.c:497-503)
          if (pass == 0) atomicAdd(&cnt[w], 1u);
          else { const uint32_t at = atomicAdd(&cnt[w], 1u); if (at < cap) pos[at] = (uint32_t)(g0 + j); }     // serial = base offset (s = 1)
        }
      }
      __syncthreads();
      if (pass == 0) {
        if (threadIdx.x == 0) { uint32_t c = 0; for (uint32_t i = 0; i < (uint32_t)FINE_NKEYS; i++) { const uint32_t t = cnt[i]; cnt[i] = c; c += t; } cnt[FINE_NKEYS] = c; }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i <= (uint32_t)FINE_NKEYS; i += 64) idx[i] = cnt[i];
        __syncthreads();
      }
    }
    for (uint32_t key = threadIdx.x; key < (uint32_t)FINE_NKEYS; key += 64) {      // ascending serials per key
      const uint32_t a = idx[key], e = idx[key + 1] < cap ? idx[key + 1] : cap;
      for (uint32_t i = a + 1; i < e; i++) { const uint32_t v = pos[i]; uint32_t j = i; while (j > a && pos[j - 1] > v) { pos[j] = pos[j - 1]; j--; } pos[j] = v; }
    }
    __syncthreads();
  }
}

int launch_fine_index(hipStream_t s, const Batch &b, const DevIndex &ix, uint32_t grid) {
  if (!b.nreads) return 0;
  hipLaunchKernelGGL(k_fine_index, dim3(fine_index_grid(b.nreads, grid)), dim3(64), 0, s, b, ix);
  return (int)hipGetLastError();
}

// S3 ahead of the candidate stage: one wave per read strand (stage_hits, smg_cands.hpp); 4 waves per SIMD by registers,
// the LDS block (window keys + list tables) sized by the launcher for as many
template <int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_hits(Batch b, DevIndex ix, MapPar p, uint32_t W, uint32_t tab, uint32_t lds_bytes, uint32_t fill) {
  extern __shared__ __align__(16) uint8_t lds[];
  unsigned long long ph[4] = {0, 0, 0, 0};
  __shared__ uint32_t qslot;
  if (ix.nseq > 0 && ix.nseq < 512) {               // first k-mer serial of every sequence: looked up per hit
    uint32_t *sl = (uint32_t *)(lds + LDS_GUARD + lds_bytes);
    for (int i = (int)threadIdx.x; i <= ix.nseq; i += 64) sl[i] = ix.seqlo[i];
    ix.seqlo = sl;
    __syncthreads();
  }
  HitsScratch x;
  x.lds = lds + LDS_GUARD; x.lds_bytes = lds_bytes; x.W = W; x.tab = tab; x.fill = fill < 1024u ? fill : 1024u;
  const uint32_t nitem = 2 * b.nreads;
  for (uint32_t it = next_item(b.hits_cursor, &qslot); it < nitem; it = next_item(b.hits_cursor, &qslot)) {
    stage_hits(b, ix, p, it >> 1, it & 1u, x, ph);
    __syncthreads();
  }
  if (threadIdx.x == 0) for (int i = 0; i < 3; i++) if (ph[i]) atomicAdd(b.work + WK_PHASE0 + i, ph[i]);
}

// S3 - S7: one wave per read.  Reads the wave-parallel form covers (smg_cands.hpp) keep their
// per-strand working set in LDS; everything else takes the sequential restatement on the HBM slot.
// LONGK: the mapper takes reads of 256 bases and more; every read then goes through the general instance of the
// wave-parallel form (mappers for short reads keep the lean one: fewer registers, more resident waves).
template <bool LONGK, bool SPLIT = false, int WAVES = 2>
__global__ void __launch_bounds__(64, WAVES) k_cands(Batch b, DevIndex ix, MapPar p, uint8_t *gscratch, CandGeom g, uint32_t lds_bytes) {
  extern __shared__ __align__(16) uint8_t lds[];
  unsigned long long nhit = 0;
  unsigned long long ph[16] = {0};
  __shared__ uint32_t qslot;
  // the first k-mer serial of every sequence goes to LDS (behind the working set): each hit looks its sequence up
  // there (a binary search = five reads) instead of in global memory
  if (lds_bytes && ix.nseq > 0 && ix.nseq < 512) {
    uint32_t *sl = (uint32_t *)(lds + LDS_GUARD + lds_bytes);
    for (int i = (int)threadIdx.x; i <= ix.nseq; i += 64) sl[i] = ix.seqlo[i];
    ix.seqlo = sl;
    __syncthreads();
  }
  uint32_t *cursor = b.next_item + NEXT_ITEM_STRIDE * (g.pass == 2 ? 4 : 1);
  // second pass: only the reads the first pass deferred (usually none: the launch ends at once)
  const uint32_t nitem = g.pass == 2 ? *b.cands_retry_n : b.nreads;
  for (uint32_t it = next_item(cursor, &qslot); it < nitem; it = next_item(cursor, &qslot)) {
    const uint32_t r = g.pass == 2 ? b.cands_retry[it] : it;
    uint8_t *base = gscratch + g.slot_bytes * (g.debug ? r : blockIdx.x);
    const DevIndex rix = read_index(b, ix, r);
    if (cands_v2_applicable(p, rix.k, rix.s, read_len(b, r), b.iv_off != nullptr)) {
      CandsV2Scratch x = cands_v2_carve(lds + LDS_GUARD, lds_bytes, base, b.qmax, rix.s, g.hcap_strand, g.ngrp, g.candcap, g.debug != 0);
      x.window = g.window; x.lds_hits = g.lds_hits; x.tab = g.tab; x.pass = g.pass;
      nhit += stage_cands_v2<LONGK, SPLIT>(b, rix, p, r, x, ph);
    } else if (b.iv_off) {                                           // interval-restricted calls exist in the wave-parallel form only
      if (threadIdx.x == 0) { CandHdr &ch = b.ch[r]; ch.ncand = ch.n_sort = ch.n_mincover = ch.n_reserved = 0; ch.rc_off = 0; ch.err = SMG_ERR_ASSERT; ch.err_site = __LINE__; ch.max_cover = ch.max2nd_cover = 0; }
    } else if (g.pass == 1) {                                        // the sequential form waits for the full-size slots
      if (threadIdx.x == 0) { CandHdr &ch = b.ch[r]; ch.ncand = ch.n_sort = ch.n_mincover = ch.n_reserved = 0; ch.rc_off = 0; ch.err = SMG_ERR_RETRY; ch.err_site = __LINE__; }
    } else {
      CandScratch x = cand_scratch_carve(base, b.qmax, ix.s, g.hcap, g.ngrp, g.segcap, g.candcap);
      nhit += stage_cands(b, ix, p, r, x);
    }
    __syncthreads();
    if (g.pass == 1 && threadIdx.x == 0 && b.ch[r].err == SMG_ERR_RETRY) b.cands_retry[atomicAdd(b.cands_retry_n, 1u)] = r;
  }
  if (threadIdx.x == 0) {
    if (nhit) atomicAdd(b.work + WK_HITS, nhit);
    for (int i = 0; i < 9; i++) if (ph[i]) atomicAdd(b.work + WK_PHASE0 + i, ph[i]);
    if (ph[9]) { atomicAdd(b.work + WK_NCAND, ph[9]); atomicAdd(b.work + WK_NKEPT, ph[10]); }
    for (int i = 11; i < 16; i++) if (ph[i]) atomicAdd(b.work + WK_PHASE0 + i, ph[i]);
  }
}

// O1: one thread per read
__global__ void __launch_bounds__(256) k_replay(Batch b, DevIndex ix, MapPar p) {
  uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long scored = 0;
  if (r < b.nreads) {
    stage_replay(b, read_index(b, ix, r), p, r);
    scored = (unsigned long long)b.ctl[r].n_scored;                               // candidates the reference would have scored
  }
  for (int o = 32; o > 0; o >>= 1) scored += __shfl_xor(scored, o);               // one atomic per wave, not per read
  if ((threadIdx.x & 63) == 0 && scored) atomicAdd(b.work + WK_CELLS_BAND, scored);
}

// K3: one wave per read; hot arrays in LDS, results and oversized direction matrices in the HBM slot
// CPLX: complexity-weighted scores (MapPar::flags & FLG_CMPLXW): a compile-time switch, so that the instances without it stay the code
// they were; cp is the table of logarithms and lambda (CplxPar) for the weighted instances and an empty argument otherwise
template <bool WIDE, bool CPLX = false>
__global__ void __launch_bounds__(64) k_align(Batch b, DevIndex ix, MapPar p, uint8_t *gscratch, size_t gbytes, uint32_t wincap,
                                              uint64_t dircap, uint32_t rescap, uint32_t dstrcap, uint32_t lds_bytes, int pass, typename cplx_arg<CPLX>::type cp) {
  extern __shared__ __align__(16) uint8_t lds[];
  uint8_t *base = gscratch + gbytes * blockIdx.x;
  AlignScratch x = align_scratch_carve_lds(lds_bytes ? lds + LDS_GUARD : nullptr, lds_bytes, base, b.qmax, wincap, dircap, rescap, dstrcap);
  x.rows_form = !(pass & 0x100);          // bit 8 of the launch's pass word: anti-diagonal form for narrow bands (test hook)
  pass &= 0xff;
  x.pass = pass;
  __shared__ int2 strip_ring[WIDE ? 256 : 1];
  x.ring = WIDE ? (void *)strip_ring : nullptr;
  __shared__ uint32_t qslot;
  uint32_t *cursor = b.next_item + NEXT_ITEM_STRIDE * (pass == 2 ? 3 : 2);
  if (pass == 2) {                        // only the reads the first pass deferred (usually none: the launch ends at once)
    const uint32_t n = *b.align_retry_n;
    for (uint32_t i = next_item(cursor, &qslot); i < n; i = next_item(cursor, &qslot)) {
      stage_align<WIDE, CPLX>(b, ix, p, b.align_retry[i], x, cp);
      __syncthreads();
    }
    align_tally_flush(b, x);
    return;
  }
  for (uint32_t r = next_item(cursor, &qslot); r < b.nreads; r = next_item(cursor, &qslot)) {
    stage_align<WIDE, CPLX>(b, ix, p, r, x, cp);
    __syncthreads();
  }
  align_tally_flush(b, x);
}

// ---------------------------------------------------------------------------------------
// K2a: un-banded Smith-Waterman score pass (swsimd.c:868 -- textbook Gotoh maximum).
//
// A task = one ranked candidate (read x reference window).  G adjacent lanes own one task;
// lane g keeps C consecutive query columns (H, E and a byte selector per column) in
// registers and sweeps the window row by row, one row behind lane g-1 (anti-diagonal skew
// ACROSS lanes only).  Per row a lane receives H[row][first-1] and the running F from its
// left neighbour with DPP row_shr:1 -- no LDS traffic in the recurrence.  Substitution
// scores come from one v_perm_b32 per cell on an 8-byte row of the biased score matrix.
// Window bases are decoded once per task into LDS.  Rows beyond a task's window and columns
// beyond the read are fed 'N' (score 0), which can never raise the maximum, so lanes need no
// predication.  int32 arithmetic equals the reference's 8-bit pass, and its 16-bit re-run on
// saturation, for any score < 65535.
//
// The stand-alone entries of the parity tests (smaltgpu_sw_*_raw -> k_sw_full_raw, k_sw_full16_raw) run the sweep
// bodies of the production kernels (SW32_CORE; sw16_tabs, sw16_nstep, sw16_sweep): a kernel and its entry differ only
// in where a task comes from, how its window and selectors get into LDS and registers, and where its score goes.
// ---------------------------------------------------------------------------------------
// the score matrix is kept biased so that every entry fits an unsigned byte: bias >= -min(M)
__host__ __device__ inline int sw_bias(const MapPar &p) {
  return p.mismatch < p.mismatch - p.match ? -p.mismatch : -(p.mismatch - p.match);
}
// a task's window starts here in the concatenated reference, and this is its read on the task's strand
__device__ inline uint64_t sw_task_gbase(const DevIndex &ix, const RCand &c) { return (c.sqidx < 0 ? 0ull : ix.sop[c.sqidx]) + c.rs; }
__device__ inline const uint8_t *sw_task_query(const Batch &b, const RCand &c) {
  return ((c.flags & RCF_REVERSE) ? b.codes_rc : b.codes) + b.read_off[c.rid];
}
// window code of a byte of the stand-alone entries, as ref_code decodes the packed reference: 7 -> A, 4 and 6 -> N
__device__ inline uint32_t sw_code_of_byte(uint32_t v) {
  const uint32_t cd = v & 7u;
  return cd == 7 ? 0 : (cd == 6 || cd == 4) ? 5 : cd;
}
// write-back of a scored K2a task (rc: its record, flags: as read from it) and its share of the two work counters
__device__ inline void sw_store_score(RCand *rc, uint32_t flags, int best, uint32_t qlen, uint32_t wlen, unsigned long long &cells,
                                      unsigned long long &ntasks_done) {
  rc->swscor = best;
  rc->flags = flags | RCF_SCORED | (best >= 65535 ? RCF_BANDED : 0u);   // ERRCODE_SWATEXCEED -> K2b
  cells += (unsigned long long)qlen * wlen;
  ntasks_done += best < 65535 ? 1 : 0;      /* a score that left 16 bits waits for K2b */
}

__device__ inline void sw_tab8(uint2 *tab, const MapPar &p, int bias) {
  if (threadIdx.x < 8) {                     // biased score matrix rows (score.c:138-173; rows 4,6 = N, 7 = A)
    const int lane = (int)threadIdx.x;
    const int rb = lane == 7 ? 0 : ((lane == 6 || lane == 4) ? 5 : lane);
    uint32_t w[2] = {0, 0};
    for (int qc = 0; qc < 8; qc++) {
      const int v = (rb == 5 || qc >= 4) ? 0 : ((rb == qc) ? p.match : p.mismatch);
      w[qc >> 2] |= (uint32_t)((v + bias) & 0xff) << (8 * (qc & 3));
    }
    tab[lane] = make_uint2(w[0], w[1]);
  }
}

// value of the lane to the left inside a 16-lane row
__device__ inline uint32_t shr1_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /* row_shr:1 */, 0xf, 0xf, true); }

// The sweep of one task by its G lanes, declaring `best` = the task's score in all lanes of the group: wrow = the window's
// codes in LDS (wlen of them, written by these lanes just before), sel = the lane's C selectors, tab = the table of sw_tab8;
// G and C are the tiling of the kernel around it.  Every lane of the workgroup runs it (the barrier, the wave-wide number
// of steps).  A macro and not a function on purpose: a function, also a force-inlined one, is simplified on its own before
// it is inlined, and the loop of k_sw_full<8,20> and <16,32> then comes out one instruction longer than from this text in
// the kernel (the running maximum's chain of v_max3 ends in a two-operand v_max; profiles/k2a_shared_body_static.txt).
#define SW32_CORE(best, wrow, wlen, sel, g, tab, bias, gi, ge)                                           \
  int best = 0;                                                                                          \
  {                                                                                                      \
    int H[C], E[C];                                                                                      \
    _Pragma("unroll") for (int cc = 0; cc < C; cc++) { H[cc] = 0; E[cc] = 0; }                           \
    int F = 0, prev_hl = 0;                                                                              \
    int nstep = (int)(wlen) + G - 1;                        /* wave-uniform number of steps */           \
    for (int o = 32; o > 0; o >>= 1) nstep = max(nstep, __shfl_xor(nstep, o));                           \
    __syncthreads();                                                                                     \
    for (int step = 0; step < nstep; step++) {                                                           \
      const int row = step - (g);                                                                        \
      const uint32_t rb = (row >= 0 && row < (int)(wlen)) ? (wrow)[row] : 5u;                            \
      const uint2 tr = (tab)[rb];                                                                        \
      int hl = (int)shr1_u32((uint32_t)H[C - 1]);                                                        \
      int fin = (int)shr1_u32((uint32_t)F);                                                              \
      if ((g) == 0) { hl = 0; fin = 0; }                                                                 \
      int diag = prev_hl;                                                                                \
      prev_hl = hl;                                                                                      \
      F = fin;                                                                                           \
      _Pragma("unroll") for (int cc = 0; cc < C; cc++) {                                                 \
        const int w = (int)__builtin_amdgcn_perm(tr.y, tr.x, (sel)[cc]);                                 \
        const int h = diag + w - (bias);                                                                 \
        const int hh = max(max(h, E[cc]), F);               /* v_max3_i32; E, F >= 0 keep H >= 0 */      \
        best = max(best, hh);                                                                            \
        diag = H[cc];                                                                                    \
        H[cc] = hh;                                                                                      \
        const int tt = hh - (gi);                                                                        \
        E[cc] = max(max(E[cc] - (ge), tt), 0);                                                           \
        F = max(max(F - (ge), tt), 0);                                                                   \
      }                                                                                                  \
    }                                                                                                    \
    for (int o = G / 2; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));                           \
  }

template <int G, int C>
__global__ void __launch_bounds__(64) k_sw_full(Batch b, DevIndex ix, MapPar p, uint32_t ntask_cap, int after16) {
  // after16: the packed 16-bit kernel ran first; what is left are the candidates of reads with non-ACGT codes
  if (after16 && b.work[WK_QN_TASKS] == 0) return;
  constexpr int NG = 64 / G;                 // tasks in flight per wave
  constexpr int WMAX = SW_FULL_WMAX;         // longest window handled here
  __shared__ uint8_t win[NG][WMAX + 8];
  __shared__ uint2 tab[8];
  const int lane = threadIdx.x, g = lane % G, grp = lane / G;
  const uint32_t ntask = min(*b.rc_count, ntask_cap);
  const int bias = sw_bias(p);
  const int gi = -p.gap_init, ge = -p.gap_ext;
  sw_tab8(tab, p, bias);
  __syncthreads();
  const uint32_t ngroups = gridDim.x * NG;
  unsigned long long cells = 0, ntasks_done = 0;
  for (uint32_t t0 = blockIdx.x * NG; t0 < ntask; t0 += ngroups) {
    const uint32_t t = t0 + grp;
    RCand c;
    bool live = false;
    uint32_t qlen = 0, wlen = 0;
    uint64_t gbase = 0;
    if (t < ntask) {
      c = b.rcpool[t];
      qlen = read_len(b, c.rid);
      wlen = (uint32_t)(c.re - c.rs + 1);
      live = !(c.flags & (RCF_BANDED | RCF_ERR | RCF_SCORED)) && wlen <= (uint32_t)WMAX && qlen <= (uint32_t)(G * C);
      gbase = sw_task_gbase(ix, c);
    }
    if (!live) { qlen = 0; wlen = 0; }
    // window -> LDS (sequence.c:1499 decode folded into the fetch)
    for (uint32_t i = g; i < wlen; i += G) win[grp][i] = (uint8_t)ref_code(ix.packed, gbase + i);
    // query columns of this lane: selector byte = code (0..3 standard, 5 = N -> score 0 column)
    uint32_t sel[C];
    {
      const uint8_t *q = live ? sw_task_query(b, c) : b.codes;      // a group without a task has no record to decode
#pragma unroll
      for (int cc = 0; cc < C; cc++) {
        uint32_t j = (uint32_t)(g * C + cc);
        uint32_t qc = j < qlen ? q[j] : 5u;
        sel[cc] = 0x0c0c0c00u | qc;
      }
    }
    SW32_CORE(best, win[grp], wlen, sel, g, tab, bias, gi, ge)
    if (live && g == 0) sw_store_score(b.rcpool + t, c.flags, best, qlen, wlen, cells, ntasks_done);
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) { cells += __shfl_xor(cells, o); ntasks_done += __shfl_xor(ntasks_done, o); }
  if (lane == 0 && cells) { atomicAdd(b.work + WK_CELLS_FULL, cells); atomicAdd(b.work + WK_TASKS_FULL, ntasks_done); }
}

// stand-alone K2a over explicit (query, window) code arrays -- parity tests of the kernel
template <int G, int C>
__global__ void __launch_bounds__(64) k_sw_full_raw(const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                                                     const uint32_t *r_off, uint32_t ntask, MapPar p, int32_t *scores) {
  constexpr int NG = 64 / G;
  constexpr int WMAX = SW_FULL_WMAX;
  __shared__ uint8_t win[NG][WMAX + 8];
  __shared__ uint2 tab[8];
  const int lane = threadIdx.x, g = lane % G, grp = lane / G;
  const int bias = sw_bias(p);
  const int gi = -p.gap_init, ge = -p.gap_ext;
  sw_tab8(tab, p, bias);
  __syncthreads();
  const uint32_t ngroups = gridDim.x * NG;
  for (uint32_t t0 = blockIdx.x * NG; t0 < ntask; t0 += ngroups) {
    const uint32_t t = t0 + grp;
    uint32_t qlen = 0, wlen = 0;
    const uint8_t *q = qcodes, *r = rcodes;
    bool live = false;
    if (t < ntask) {
      qlen = q_off[t + 1] - q_off[t]; wlen = r_off[t + 1] - r_off[t];
      q += q_off[t]; r += r_off[t];
      live = wlen <= (uint32_t)WMAX && qlen <= (uint32_t)(G * C);
    }
    if (!live) { qlen = 0; wlen = 0; }
    for (uint32_t i = g; i < wlen; i += G) win[grp][i] = (uint8_t)sw_code_of_byte(r[i]);
    uint32_t sel[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      uint32_t j = (uint32_t)(g * C + cc);
      uint32_t qc = (j < qlen) ? (q[j] & 7u) : 5u;
      sel[cc] = 0x0c0c0c00u | qc;
    }
    SW32_CORE(best, win[grp], wlen, sel, g, tab, bias, gi, ge)
    if (t < ntask && g == 0) scores[t] = live ? best : -1;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// K2a, two tasks per lane group in packed 16-bit halves (v_pk_*_u16).
//
// Same tiling as k_sw_full; every register holds the cell of task A in its low half and the cell of
// task B (the next ranked candidate) in its high half.  All quantities are kept non-negative and
// subtractions saturate at 0, which is the recurrence of the 32-bit kernel with its max(.., 0)
// folded into the subtract: H = max(sat(Hdiag + (w + bias) - bias), E, F), E = max(sat(E - ge),
// sat(H - gi)).  One v_perm_b32 yields both substitution scores from an 8-byte source holding the
// ACGT row of either task (selector bytes {qA, 0x0c, 4 + qB, 0x0c}).  That leaves no byte for a
// query 'N' (score 0), so reads with non-ACGT codes stay with the 32-bit kernel (RCF_QN); columns
// beyond the read take the constant 0 (score -bias <= 0) and rows beyond the window an all-'N' row,
// neither of which can raise a maximum.  Requires match * 512 + bias < 65535 (checked by the launcher).
// ---------------------------------------------------------------------------------------
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ inline us2 as_us2(uint32_t v) { return __builtin_bit_cast(us2, v); }
__device__ inline uint32_t as_u32(us2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ inline us2 pk_max(us2 a, us2 b) { return __builtin_elementwise_max(a, b); }
__device__ inline us2 pk_subs(us2 a, us2 b) { return __builtin_elementwise_sub_sat(a, b); }
// sum of two packed pairs whose halves cannot overflow (score + biased substitution score < 65536, checked by the
// launcher): one full-rate 32-bit add instead of a packed add at half the issue rate
__device__ inline us2 pk_add_nc(us2 a, us2 b) { return as_us2(as_u32(a) + as_u32(b)); }
// Packed maximum of three: gfx950's v_pk_maximum3_f16 on the u16 bit patterns.  Non-negative half floats order like
// their bit patterns (denormals are kept in the default mode), and the values here stay far below 0x7C00 (infinity):
// scores of reads up to 512 bases with match <= 15 plus the bias.  Checked bit for bit against the integer maximum
// on 10^6 random triples including the denormal range.
typedef _Float16 hf2 __attribute__((ext_vector_type(2)));
__device__ inline us2 pk_max3(us2 a, us2 b, us2 c) {
  const hf2 r = __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(hf2, a), __builtin_bit_cast(hf2, b)), __builtin_bit_cast(hf2, c));
  return __builtin_bit_cast(us2, r);
}
// The two lane hand-overs of a sweep row, each with its select in the same instruction: h = first lane of its group ?
// hfirst : hv of the lane to the left, f likewise from its own value one lane to the left.  v_cndmask_b32 is VOP2 and
// takes a DPP source here: dst = VCC ? src1 : dpp(src0).  The compiler does not form it from update_dpp and a select (it
// keeps a v_mov_b32_dpp and a v_cndmask_b32), hence the assembly.  What it rests on:
//  * every lane is on: a DPP read of a lane that a branch has switched off yields 0, so this is never under a divergent
//    branch (the sweeps run under wave-uniform, scalar branches only);
//  * bound_ctrl: lane 0 of a DPP row of 16 has no source lane and takes 0 instead of skipping its write; it is the first
//    lane of a group for G = 4, 8, 16, so VCC picks src1 there anyway;
//  * a VALU write of a register needs two wait states before a DPP read of it, and the hazard pass does not look into
//    inline assembly: the s_mov and the s_nop are those two for hv, whatever came before the block, and f has three;
//  * VCC is set from the mask inside the block and listed as clobbered, so nothing can come between setting and use.
template <int G>
__device__ inline void shr1_first2_u32(uint32_t &h, uint32_t &f, uint32_t hv, uint32_t hfirst, uint32_t ffirst) {
  static_assert(G == 4 || G == 8 || G == 16, "a group starts on lane 0 of every DPP row");
  constexpr unsigned long long first = G == 4 ? 0x1111111111111111ull : G == 8 ? 0x0101010101010101ull : 0x0001000100010001ull;
  asm volatile("s_mov_b64 vcc, %5\n\t"
               "s_nop 0\n\t"
               "v_cndmask_b32_dpp %0, %2, %3, vcc row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
               "v_cndmask_b32_dpp %1, %1, %4, vcc row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1"
               : "=&v"(h), "+v"(f) : "v"(hv), "v"(hfirst), "v"(ffirst), "s"(first) : "vcc");
}
// entry of a score table by byte offset (the window arrays hold code pair x 8): the LDS read takes the entry register
// and the table's address as its immediate offset
__device__ inline uint2 sw16_tab(const uint2 *tab, uint32_t e8) { return *(const uint2 *)((const char *)tab + e8); }

enum : int { SW16_BLK = 5 };
struct Sw16Par { uint32_t mm4, dlt, n4; us2 bias, gi, ge; int fp; uint32_t hi_match, hi_mismatch; us2 ngi, nge;
                 int rf_steps; uint32_t hi_rmatch, hi_rmismatch, hi_rn; us2 pge, ngo;         // row-frame form (sw16r_core)
                 int pf_steps; uint32_t hi_pmatch, hi_pmismatch, hi_pn; us2 nge2; };          // pair-frame form (sw16p_core)
// half-float bit pattern of a small integer (|n| <= 2048: exact)
__device__ inline uint32_t f16_bits_of_int(int n) {
  if (n == 0) return 0;
  const uint32_t sign = n < 0 ? 0x8000u : 0u, a = (uint32_t)(n < 0 ? -n : n);
  const int e = 31 - __clz((int)a);
  return sign | ((uint32_t)(e + 15) << 10) | ((e <= 10 ? a << (10 - e) : a >> (e - 10)) & 0x3ffu);
}
// Row-frame form of the half-float sweep (sw16r_core): the longest sweep (steps = window rows + G - 1) that it may run
// for these penalties and ncols tile columns, -1 if none.  The shifted scores match + ge, mismatch + ge and ge must be
// half floats with a zero low byte (v_perm fetches high bytes), and every value must stay an exact integer: the largest
// is a full-length match seen from the frame of the row after the last, match * ncols + ge * (steps + 1), with gi of room
// for the sums in between; the smallest, -ge * G - gi in front of the window, is covered by steps >= G - 1.
__host__ __device__ inline int sw16_rowframe_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols) {
  const int gi = -gap_init, ge = -gap_ext;
  if (match <= 0 || ge < 0 || gi < ge || gi > 2040 || mismatch < -1024 || match + ge > 2040) return -1;
  const int sc[5] = {match + ge, mismatch + ge, ge, match, mismatch};      // the last two: its fallback is sw16f_core, same selectors
  for (int k = 0; k < 5; k++) {                 // zero low byte: at most three significant bits
    int a = sc[k] < 0 ? -sc[k] : sc[k];
    while (a && !(a & 1)) a >>= 1;
    if (a > 7) return -1;
  }
  const int room = 2040 - gi - match * ncols;
  if (room < 0) return -1;
  if (ge == 0) return 0x7fffffff;
  return room / ge - 1;
}
// Pair-frame form (sw16p_core): the same question.  Its tables are the row frame's, the plain one and one of scores + 2 ge:
// match + 2 ge, mismatch + 2 ge and 2 ge must have a zero low byte as half floats on top of what the row frame asks.  Its
// values lie up to two ge further from the true scores (the second floor ge * (r + 2), the class-1 maximum in the frame of
// row r + 1), so the range is the row frame's with two more ge of room: match * ncols + ge * (steps + 3) + gi <= 2040.
// That covers the most negative value too, -ge * (G + 1) - gi in front of the window, as steps >= G.
__host__ __device__ inline int sw16_pairframe_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols) {
  const int rf = sw16_rowframe_steps(match, mismatch, gap_init, gap_ext, ncols);
  if (rf < 0) return -1;
  const int ge = -gap_ext;
  const int sc[2] = {match + 2 * ge, mismatch + 2 * ge};          // 2 ge: as ge
  for (int k = 0; k < 2; k++) {
    int a = sc[k] < 0 ? -sc[k] : sc[k];
    while (a && !(a & 1)) a >>= 1;
    if (a > 7) return -1;
  }
  if (ge == 0) return rf;
  return rf >= 2 ? rf - 2 : -1;
}
// ncols: columns of the register tile (longest read of this instance)
__device__ inline Sw16Par sw16_par(const MapPar &p, int ncols = 512) {
  Sw16Par s;
  // Half-float form (sw16f_core): scores as half floats -- integers up to 2048 are exact -- so that the substitution
  // score is signed (no bias to take off again) and gfx950's packed maximum3 floors the gap scores at 0 in the same
  // instruction.  One v_perm fetches the HIGH bytes of both tasks' scores: match and mismatch must be half floats with a
  // zero low byte (integers with at most three significant bits: 1, -2, 3, -4, 5, -6, ...).
  const uint32_t fm = f16_bits_of_int(p.match), fx = f16_bits_of_int(p.mismatch);
  s.fp = (fm & 0xffu) == 0 && (fx & 0xffu) == 0 && p.match > 0 && p.match * ncols <= 2040 && -p.gap_init >= 0 && -p.gap_init <= 2040 &&
         -p.gap_ext >= 0 && -p.gap_ext <= 2040 && p.mismatch >= -1024;
  s.hi_match = fm >> 8; s.hi_mismatch = fx >> 8;
  { const uint32_t a = f16_bits_of_int(p.gap_init), e = f16_bits_of_int(p.gap_ext);      // gap_init, gap_ext are negative: added
    s.ngi = us2{(unsigned short)a, (unsigned short)a}; s.nge = us2{(unsigned short)e, (unsigned short)e}; }
  s.rf_steps = s.fp ? sw16_rowframe_steps(p.match, p.mismatch, p.gap_init, p.gap_ext, ncols) : -1;
  s.hi_rmatch = f16_bits_of_int(p.match - p.gap_ext) >> 8; s.hi_rmismatch = f16_bits_of_int(p.mismatch - p.gap_ext) >> 8;
  s.hi_rn = f16_bits_of_int(-p.gap_ext) >> 8;
  { const uint32_t e = f16_bits_of_int(-p.gap_ext), o = f16_bits_of_int(p.gap_init - p.gap_ext);       // + ge, - (gi - ge)
    s.pge = us2{(unsigned short)e, (unsigned short)e}; s.ngo = us2{(unsigned short)o, (unsigned short)o}; }
  s.pf_steps = s.fp ? sw16_pairframe_steps(p.match, p.mismatch, p.gap_init, p.gap_ext, ncols) : -1;
  s.hi_pmatch = f16_bits_of_int(p.match - 2 * p.gap_ext) >> 8; s.hi_pmismatch = f16_bits_of_int(p.mismatch - 2 * p.gap_ext) >> 8;
  s.hi_pn = f16_bits_of_int(-2 * p.gap_ext) >> 8;
  { const uint32_t e = f16_bits_of_int(2 * p.gap_ext); s.nge2 = us2{(unsigned short)e, (unsigned short)e}; }      // - 2 ge
  const int bias = sw_bias(p);
  s.mm4 = (uint32_t)((p.mismatch + bias) & 0xff) * 0x01010101u;      // a row of mismatches ...
  s.dlt = (uint32_t)(p.match - p.mismatch);                          // ... plus this at the byte of the matching base
  s.n4 = (uint32_t)(bias & 0xff) * 0x01010101u;                      // reference 'N': score 0 against everything
  s.bias = us2{(unsigned short)bias, (unsigned short)bias};
  s.gi = us2{(unsigned short)(-p.gap_init), (unsigned short)(-p.gap_init)};
  s.ge = us2{(unsigned short)(-p.gap_ext), (unsigned short)(-p.gap_ext)};
  return s;
}

// wrow: per-row code pairs (code of task A | code of task B << 3) of this lane group, each times 8 -- the byte offset of
// the pair's entry in the score tables, at most 63 x 8 = 504; entry r + G - 1 = row r; the entries before row 0 and from
// the last row up to nstep + G - 1 hold the N pair, so the sweep reads without bounds checks.
// rowtab2[pair]: the biased ACGT score rows of both codes (one 8-byte LDS read per row, sw16_tab).
template <int G, int C>
__device__ inline uint32_t sw16_core(const uint16_t *wrow, int nstep, const uint32_t (&sel)[C], int g, const Sw16Par &sp, const uint2 *rowtab2) {
  us2 H[C], E[C];
#pragma unroll
  for (int cc = 0; cc < C; cc++) { H[cc] = us2{0, 0}; E[cc] = us2{0, 0}; }
  us2 best = us2{0, 0}, F = us2{0, 0}, prev_hl = us2{0, 0};
  const uint32_t gmask = g == 0 ? 0u : 0xffffffffu;       // the first lane of a group has no left neighbour
  const uint16_t *wp = wrow + (G - 1) - g;                // the lane's row pointer, one bump per row
  for (int step = 0; step < nstep; step++, wp++) {
    const uint2 rr = sw16_tab(rowtab2, *wp);
    const uint32_t rowA = rr.x, rowB = rr.y;                              // ACGT scores (+ bias) against this reference base
    const uint32_t hl = shr1_u32(as_u32(H[C - 1])) & gmask;
    const uint32_t fin = shr1_u32(as_u32(F)) & gmask;
    us2 carry = prev_hl;                       // H[row-1] of the column left of the block
    prev_hl = as_us2(hl);
    F = as_us2(fin);
    // Blocks of SW16_BLK columns: first everything that does not depend on the running F (independent across the
    // columns, so the packed-op forwarding hazards are filled with useful work), then the F chain.
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += SW16_BLK) {
      us2 t3[SW16_BLK];
      const us2 last_old = H[(c0 + SW16_BLK - 1 < C) ? c0 + SW16_BLK - 1 : C - 1];
#pragma unroll
      for (int u = 0; u < SW16_BLK; u++) {
        const int cc = c0 + u;
        if (cc < C) {
          const us2 w = as_us2(__builtin_amdgcn_perm(rowB, rowA, sel[cc]));
          const us2 dg = u == 0 ? carry : H[cc - 1];
          t3[u] = pk_subs(pk_add_nc(dg, w), sp.bias);
        }
      }
#pragma unroll
      for (int u = 0; u < SW16_BLK; u++) {
        const int cc = c0 + u;
        if (cc < C) {
          const us2 hh = pk_max3(t3[u], E[cc], F);
          H[cc] = hh;
          const us2 tt = pk_subs(hh, sp.gi);
          E[cc] = pk_max(pk_subs(E[cc], sp.ge), tt);
          F = pk_max(pk_subs(F, sp.ge), tt);
        }
      }
#pragma unroll
      for (int u = 0; u < SW16_BLK; u += 2) {            // the running maximum takes the block's cells two at a time
        const int cc = c0 + u;
        if (cc + 1 < C && u + 1 < SW16_BLK) best = pk_max3(best, H[cc], H[cc + 1]);
        else if (cc < C) best = pk_max(best, H[cc]);
      }
      carry = last_old;
    }
  }
  uint32_t bb = as_u32(best);
  for (int o = G / 2; o > 0; o >>= 1) bb = as_u32(pk_max(as_us2(bb), as_us2((uint32_t)__shfl_xor((int)bb, o))));
  return bb;
}

// The same sweep in half floats (Sw16Par::fp).  Per cell pair: perm (high bytes of both signed scores), add, max3 (value,
// E, F -- both kept >= 0, which floors the value too), add (gap open), 2 x (add, max3 with 0) and 0.6 for the running
// maximum: 8.6 instructions.  Every value is an integer of magnitude <= 2048, so the arithmetic is exact.
__device__ inline hf2 hf_max3(hf2 a, hf2 b, hf2 c) { return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c); }
template <int G, int C>
__device__ inline uint32_t sw16f_core(const uint16_t *wrow, int nstep, const uint32_t (&sel)[C], int g, const Sw16Par &sp, const uint2 *rowtab2) {
  hf2 H[C], E[C];
  const hf2 zero = hf2{(_Float16)0, (_Float16)0};
#pragma unroll
  for (int cc = 0; cc < C; cc++) { H[cc] = zero; E[cc] = zero; }
  hf2 best = zero, F = zero, prev_hl = zero;
  const hf2 ngi = __builtin_bit_cast(hf2, sp.ngi), nge = __builtin_bit_cast(hf2, sp.nge);
  const uint32_t gmask = g == 0 ? 0u : 0xffffffffu;
  const uint16_t *wp = wrow + (G - 1) - g;
  for (int step = 0; step < nstep; step++, wp++) {
    const uint2 rr = sw16_tab(rowtab2, *wp);
    const uint32_t hl = shr1_u32(__builtin_bit_cast(uint32_t, H[C - 1])) & gmask;
    const uint32_t fin = shr1_u32(__builtin_bit_cast(uint32_t, F)) & gmask;
    hf2 carry = prev_hl;
    prev_hl = __builtin_bit_cast(hf2, hl);
    F = __builtin_bit_cast(hf2, fin);
#pragma unroll
    for (int c0 = 0; c0 < C; c0 += SW16_BLK) {
      hf2 t3[SW16_BLK];
      const hf2 last_old = H[(c0 + SW16_BLK - 1 < C) ? c0 + SW16_BLK - 1 : C - 1];
#pragma unroll
      for (int u = 0; u < SW16_BLK; u++) {
        const int cc = c0 + u;
        if (cc < C) {
          const hf2 w = __builtin_bit_cast(hf2, __builtin_amdgcn_perm(rr.y, rr.x, sel[cc]));
          const hf2 dg = u == 0 ? carry : H[cc - 1];
          t3[u] = dg + w;
        }
      }
#pragma unroll
      for (int u = 0; u < SW16_BLK; u++) {
        const int cc = c0 + u;
        if (cc < C) {
          const hf2 hh = hf_max3(t3[u], E[cc], F);
          H[cc] = hh;
          const hf2 tt = hh + ngi;
          E[cc] = hf_max3(E[cc] + nge, tt, zero);
          F = hf_max3(F + nge, tt, zero);
        }
      }
#pragma unroll
      for (int u = 0; u < SW16_BLK; u += 2) {
        const int cc = c0 + u;
        if (cc + 1 < C && u + 1 < SW16_BLK) best = hf_max3(best, H[cc], H[cc + 1]);
        else if (cc < C) best = __builtin_elementwise_maximum(best, H[cc]);
      }
      carry = last_old;
    }
  }
  for (int o = G / 2; o > 0; o >>= 1)
    best = __builtin_elementwise_maximum(best, __builtin_bit_cast(hf2, (uint32_t)__shfl_xor((int)__builtin_bit_cast(uint32_t, best), o)));
  return (uint32_t)(int)(float)best.x | ((uint32_t)(int)(float)best.y << 16);
}

// The half-float sweep in a row frame: every value of window row r is kept as X + ge * r, so that E, which moves down a
// column, decays by changing rows and needs no add.  With go = gi - ge, flo_r = ge * r (what a true 0 looks like in row
// r) and T = H - go:  H(r, j) = max3(H(r-1, j-1) + (s + ge), E, F);  E(r+1, j) = max3(E(r, j), T, flo_(r+1));
// F(j+1) = max(F(j), T(j)) - ge.  F shares T with E and loses its floor at 0: the floored and the unfloored chain differ
// only where both are <= 0, and E >= 0 floors H, so H is what it was; F stays >= flo_r - gi.  The + ge of the diagonal is
// in the score table (sw16_rowtab2r).  Per cell pair: perm, add, max3, add, max3, max, add and 0.6 for the running
// maximum: 7.6 instructions, one add fewer than sw16f_core.  The running maximum follows the frame (+ ge per row) and
// comes back to true scores per lane after the loop, because the lanes of a group end on different rows.  Lane g takes
// H and F of its left neighbour in the same row, hence the same frame; the first lane of a group takes flo_r.  A lane
// starts on row -g with everything at the true 0 of the row it was last seen from.  sw16_rowframe_steps() says when all
// of this stays within the exact integers.
template <int G, int C>
__device__ inline uint32_t sw16r_core(const uint16_t *wrow, int nstep, const uint32_t (&sel)[C], int g, const Sw16Par &sp, const uint2 *rowtab2r) {
  hf2 H[C], E[C];
  const hf2 pge = __builtin_bit_cast(hf2, sp.pge), nge = __builtin_bit_cast(hf2, sp.nge), ngo = __builtin_bit_cast(hf2, sp.ngo);
  const _Float16 r0 = (_Float16)(-(g + 1));
  hf2 flo1 = pge * hf2{r0, r0} + pge;          // flo of the row the lane does next: ge * -g
  {
    const hf2 f0 = flo1 - pge;
#pragma unroll
    for (int cc = 0; cc < C; cc++) { H[cc] = f0; E[cc] = flo1; }
  }
  hf2 best = flo1 - pge, F = best, prev_hl = best, flo = best;
  const uint16_t *wp = wrow + (G - 1) - g;
  for (int step = 0; step < nstep; step++, wp++) {
    const uint2 rr = sw16_tab(rowtab2r, *wp);
    flo = flo1;
    flo1 = flo + pge;
    const uint32_t flob = __builtin_bit_cast(uint32_t, flo);
    // the hand-over runs in every lane; the first lane of a group has no left neighbour: it takes flo (shr1_first2_u32)
    uint32_t hl, fin = __builtin_bit_cast(uint32_t, F);
    shr1_first2_u32<G>(hl, fin, __builtin_bit_cast(uint32_t, H[C - 1]), flob, flob);
    hf2 carry = prev_hl;
    prev_hl = __builtin_bit_cast(hf2, hl);
    F = __builtin_bit_cast(hf2, fin);
    // The F chain is four dependent packed operations per cell, and a packed operation that reads the result of the one
    // before it waits a cycle.  What does not depend on the chain (perm and add of the column two ahead, E, the running
    // maximum, the row's frame constants) goes between its links, and the order is pinned.
#define SW16R_SB() __builtin_amdgcn_sched_barrier(0)
    hf2 t3[C + 2];
    t3[0] = carry + __builtin_bit_cast(hf2, __builtin_amdgcn_perm(rr.y, rr.x, sel[0]));
    if (C > 1) t3[1] = H[0] + __builtin_bit_cast(hf2, __builtin_amdgcn_perm(rr.y, rr.x, sel[1]));
    SW16R_SB();
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      const hf2 hh = hf_max3(t3[cc], E[cc], F);
      SW16R_SB();
      hf2 w = hh;
      if (cc + 2 < C) w = __builtin_bit_cast(hf2, __builtin_amdgcn_perm(rr.y, rr.x, sel[cc + 2 < C ? cc + 2 : 0]));
      SW16R_SB();
      const hf2 tt = hh + ngo;
      SW16R_SB();
      if (cc + 2 < C) t3[cc + 2] = H[cc + 1 < C ? cc + 1 : 0] + w;
      SW16R_SB();
      const hf2 fm = __builtin_elementwise_maximum(F, tt);
      SW16R_SB();
      E[cc] = hf_max3(E[cc], tt, flo1);
      H[cc] = hh;
      SW16R_SB();
      F = fm + nge;
      SW16R_SB();
      if (cc & 1) best = hf_max3(best, H[cc - 1], H[cc]);
      else if (cc == 0) best = best + pge;
      else if (cc == C - 1) best = __builtin_elementwise_maximum(best, H[cc]);
      SW16R_SB();
    }
#undef SW16R_SB
  }
  best = best - flo;                            // true scores, per lane: flo is the frame of the lane's last row
  for (int o = G / 2; o > 0; o >>= 1)
    best = __builtin_elementwise_maximum(best, __builtin_bit_cast(hf2, (uint32_t)__shfl_xor((int)__builtin_bit_cast(uint32_t, best), o)));
  return (uint32_t)(int)(float)best.x | ((uint32_t)(int)(float)best.y << 16);
}

// The half-float sweep in a column-pair frame: a lane's column cc has class p = cc & 1, and a value of window row r in a
// column of class p is kept as X + ge * (r + p).  E is as in the row frame, with the floor ge * (r + 1 + p).  F decays by
// ge per column and the frame rises by ge from an even to an odd column, so there F(cc + 1) = max(F, T) with no add; from
// an odd column to the next even one it is max(F, T) - 2 ge, and behind the lane's last column (to column 0 of the right
// neighbour, same row) - ge * (1 + class of the last column).  The diagonal into an odd column changes frame by 2 ge (table
// sw16_rowtab2p), into an even column cc >= 2 by nothing (the plain table), into column 0 by ge * (1 - class of the left
// neighbour's last column): the row-frame table for odd C, the plain one for even C.  Columns beyond the read keep the
// selector of the constant 0: a true 0, - ge or - 2 ge, never positive.  The running maximum is one register per class;
// going to the next row the class-1 register holds the class-0 maximum as it is and the class-0 register, + 2 ge, the
// class-1 maximum.  The floors ge * r, ge * (r + 1), ge * (r + 2) of a row share two values with the next row's, so one
// add per row makes the new one; with four floor registers, four rows bring every register back to its role, and the
// loop body is four rows with the roles written out (no register moves, and none for the diagonal of column 0 either).
// Per cell pair: perm, add, max3, add, max3, max, half an add and 0.5 for the running maximum: 7 instructions.
// sw16_pairframe_steps() says when every value stays within the exact integers.
template <int G, int C>
__device__ inline uint32_t sw16p_core(const uint16_t *wrow, int nstep, const uint32_t (&sel)[C], int g, const Sw16Par &sp,
                                      const uint2 *rowtab2, const uint2 *rowtab2r, const uint2 *rowtab2p) {
  constexpr int PL = (C - 1) & 1;                // class of the lane's last column
  hf2 H[C], E[C];
  const hf2 pge = __builtin_bit_cast(hf2, sp.pge), nge = __builtin_bit_cast(hf2, sp.nge), ngo = __builtin_bit_cast(hf2, sp.ngo);
  const hf2 nge2 = __builtin_bit_cast(hf2, sp.nge2), pge2 = pge + pge;
  const _Float16 r0 = (_Float16)(-g);
  hf2 n0 = pge * hf2{r0, r0}, n1 = n0 + pge, n2 = n1 + pge, n3 = n2;  // floors of the row the lane does next (row -g at first)
  // the row before the first: everything at the true 0 of the frame it is next read in
  hf2 ma = n0 - pge, mb = n0;                    // maxima of class 0 and class 1 of the row done last
  {
#pragma unroll
    for (int cc = 0; cc < C; cc++) { H[cc] = (cc & 1) ? mb : ma; E[cc] = (cc & 1) ? n1 : n0; }
  }
  hf2 F = ma, pa = PL ? mb : ma, pb = pa;        // pa / pb: H of the left neighbour's last column, one row back, in turn
  const uint16_t *wp = wrow + (G - 1) - g;       // the lane's row pointer: entry r + G - 1 is row r, and the lane starts on row -g
#define SW16P_SB() __builtin_amdgcn_sched_barrier(0)
  // one row with floors f0, f1, f2; c0: the register that takes the class-0 maximum (it held class 1 of the row before),
  // c1: the one that takes class 1 (it held class 0); carry: diagonal of column 0, hl: where the next row's goes
  // k: the row's entry behind the lane's row pointer wp, which the loops bump (the body once for its four rows)
  auto row = [&](int k, const hf2 f0, const hf2 f1, const hf2 f2, hf2 &c0, hf2 &c1, const hf2 carry, hf2 &hl) __attribute__((always_inline)) {
    const uint32_t e = wp[k];
    const uint2 rq = sw16_tab(rowtab2, e), rp = sw16_tab(rowtab2p, e);
    const uint2 rz = PL ? rq : sw16_tab(rowtab2r, e);
    // the hand-over runs in every lane; the first lane of a group has no left neighbour: it takes the floors (shr1_first2_u32)
    uint32_t hlb, fb = __builtin_bit_cast(uint32_t, F);
    shr1_first2_u32<G>(hlb, fb, __builtin_bit_cast(uint32_t, H[C - 1]), __builtin_bit_cast(uint32_t, PL ? f1 : f0), __builtin_bit_cast(uint32_t, f0));
    hl = __builtin_bit_cast(hf2, hlb);
    F = __builtin_bit_cast(hf2, fb);
    // As in sw16r_core: what does not depend on the F chain goes between its links (three on an even column, four on an
    // odd one), and the order is pinned.
    hf2 t3[C + 2];
    t3[0] = carry + __builtin_bit_cast(hf2, __builtin_amdgcn_perm(rz.y, rz.x, sel[0]));
    if (C > 1) t3[1] = H[0] + __builtin_bit_cast(hf2, __builtin_amdgcn_perm(rp.y, rp.x, sel[1]));
    SW16P_SB();
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      const bool odd = cc & 1;
      const hf2 hh = hf_max3(t3[cc], E[cc], F);
      SW16P_SB();
      hf2 w = hh;
      if (cc + 2 < C) w = __builtin_bit_cast(hf2, odd ? __builtin_amdgcn_perm(rp.y, rp.x, sel[cc + 2 < C ? cc + 2 : 0])
                                                      : __builtin_amdgcn_perm(rq.y, rq.x, sel[cc + 2 < C ? cc + 2 : 0]));
      SW16P_SB();
      const hf2 tt = hh + ngo;
      SW16P_SB();
      if (cc + 2 < C) t3[cc + 2] = H[cc + 1 < C ? cc + 1 : 0] + w;
      SW16P_SB();
      const hf2 fm = __builtin_elementwise_maximum(F, tt);
      SW16P_SB();
      E[cc] = hf_max3(E[cc], tt, odd ? f2 : f1);
      H[cc] = hh;
      SW16P_SB();
      if (cc == C - 1) F = fm + (PL ? nge2 : nge);
      else if (odd) F = fm + nge2;
      else F = fm;
      SW16P_SB();
      if (cc == 0) c1 = c1 + pge2;
      hf2 &cm = odd ? c1 : c0;
      if ((cc >> 1) & 1) cm = hf_max3(cm, H[cc - 2 >= 0 ? cc - 2 : 0], H[cc]);
      else if (cc + 2 >= C) cm = __builtin_elementwise_maximum(cm, H[cc]);
      SW16P_SB();
    }
  };
  int step = 0;
  // The four-row body takes some fifteen registers more than a single row (the compiler renames across the rows).  The
  // 32-column tiling would go from three waves per SIMD to two with it, so it runs the single rows only.
  if (C <= 20) for (; step + 3 < nstep; step += 4, wp += 4) {
    row(0, n0, n1, n2, mb, ma, pa, pb);
    n3 = n2 + pge;
    row(1, n1, n2, n3, ma, mb, pb, pa);
    n0 = n3 + pge;
    row(2, n2, n3, n0, mb, ma, pa, pb);
    n1 = n0 + pge;
    row(3, n3, n0, n1, ma, mb, pb, pa);
    n2 = n1 + pge;
  }
  for (; step < nstep; step++, wp++) {           // the up to three rows left, the roles kept by moves
    row(0, n0, n1, n2, mb, ma, pa, pb);
    { const hf2 t = ma; ma = mb; mb = t; }
    pa = pb;
    n0 = n1; n1 = n2; n2 = n2 + pge;
  }
#undef SW16P_SB
  // true scores, per lane: ma is in the frame of the lane's last row (n0 - ge), mb in that of the row after it
  hf2 best = __builtin_elementwise_maximum(ma - (n0 - pge), mb - n0);
  for (int o = G / 2; o > 0; o >>= 1)
    best = __builtin_elementwise_maximum(best, __builtin_bit_cast(hf2, (uint32_t)__shfl_xor((int)__builtin_bit_cast(uint32_t, best), o)));
  return (uint32_t)(int)(float)best.x | ((uint32_t)(int)(float)best.y << 16);
}

// rowtab[code]: the four biased ACGT scores against reference code 0..7 (4, 5, 6: 'N' -> score 0; 7 decodes as A upstream)
__device__ inline void sw16_rowtab(uint32_t *rowtab, const Sw16Par &sp) {
  if (threadIdx.x < 8) rowtab[threadIdx.x] = threadIdx.x < 4 ? sp.mm4 + (sp.dlt << (8 * threadIdx.x)) : sp.n4;
}
// the same for a pair of codes: entry a | b << 3
__device__ inline void sw16_rowtab2(uint2 *rowtab2, const Sw16Par &sp) {
  const uint32_t a = threadIdx.x & 7u, bq = threadIdx.x >> 3;
  if (sp.fp) {                                  // high bytes of the half-float scores against A, C, G, T; N rows: 0
    const uint32_t x4 = sp.hi_mismatch * 0x01010101u;
    rowtab2[threadIdx.x] = make_uint2(a < 4 ? (x4 & ~(0xffu << (8 * a))) | (sp.hi_match << (8 * a)) : 0u,
                                      bq < 4 ? (x4 & ~(0xffu << (8 * bq))) | (sp.hi_match << (8 * bq)) : 0u);
    return;
  }
  rowtab2[threadIdx.x] = make_uint2(a < 4 ? sp.mm4 + (sp.dlt << (8 * a)) : sp.n4, bq < 4 ? sp.mm4 + (sp.dlt << (8 * bq)) : sp.n4);
}
// the table of the row-frame form: every score + ge; N rows hold ge (a true 0).  Columns beyond the read keep the selector
// of the constant 0, now a true score of -ge: such a column influences only columns to its right, and its H never exceeds
// an H of a real column, so it still cannot raise the maximum.
__device__ inline void sw16_rowtab2r(uint2 *rowtab2r, const Sw16Par &sp) {
  const uint32_t a = threadIdx.x & 7u, bq = threadIdx.x >> 3;
  const uint32_t x4 = sp.hi_rmismatch * 0x01010101u, n4 = sp.hi_rn * 0x01010101u;
  rowtab2r[threadIdx.x] = make_uint2(a < 4 ? (x4 & ~(0xffu << (8 * a))) | (sp.hi_rmatch << (8 * a)) : n4,
                                     bq < 4 ? (x4 & ~(0xffu << (8 * bq))) | (sp.hi_rmatch << (8 * bq)) : n4);
}
// the third table, of the pair-frame form's odd columns: every score + 2 ge; N rows hold 2 ge (a true 0)
__device__ inline void sw16_rowtab2p(uint2 *rowtab2p, const Sw16Par &sp) {
  const uint32_t a = threadIdx.x & 7u, bq = threadIdx.x >> 3;
  const uint32_t x4 = sp.hi_pmismatch * 0x01010101u, n4 = sp.hi_pn * 0x01010101u;
  rowtab2p[threadIdx.x] = make_uint2(a < 4 ? (x4 & ~(0xffu << (8 * a))) | (sp.hi_pmatch << (8 * a)) : n4,
                                     bq < 4 ? (x4 & ~(0xffu << (8 * bq))) | (sp.hi_pmatch << (8 * bq)) : n4);
}
enum : uint32_t { SW16_NPAIR = 5u | (5u << 3) };

// ---------------------------------------------------------------------------------------
// What the packed sweep is handed -- the selectors of the read's columns and the code pairs of the window's rows -- is
// put together from whole words:
//  * the codes of a read go through LDS once per read (both strands, one coalesced load by the whole wave, padded with
//    the selector of the constant 0 beyond the read); a lane takes its C columns as dwords and one v_perm per column
//    makes the selector.  Consecutive ranked candidates belong to one read, so the tasks of a wave iteration nearly
//    always share it (and a wave whose next iteration is still in that read keeps it);
//  * a lane decodes ten window entries at a time from two adjacent words of the packed reference (ten bases each), all
//    ten codes at once in their 3-bit fields.
// ---------------------------------------------------------------------------------------
template <int G, int C>
struct Sw16Geo {
  enum : int { CP = (C + 3) & ~3,      // bytes that the C columns of a lane take in the staged read: whole dwords
               NW = CP / 4, QST = G * CP };
};
typedef uint32_t __attribute__((may_alias)) u32_alias;
enum : uint32_t { SW16_PAD4 = 0x0c0c0c0cu, SW16_N10 = 0x2DB6DB6Du /* ten codes 5 */ };
// entries of a group's window array: rows -(G-1) .. WMAX+G-2, in whole runs of ten
constexpr int sw16_went(int G, int WMAX) { return (WMAX + 2 * G - 2 + 9) / 10 * 10; }

// Selector bytes of one read, both strands, to qst[2][G * CP]: column j = gg * C + cc at byte gg * CP + cc; the code
// below the read's length, 0x0c (the constant 0 of v_perm) from there on.  RAW: codes as the test entry passes them
// (3 bits, one array for both); returns whether the read has a code beyond ACGT.
template <int G, int C, bool RAW>
__device__ inline bool sw16_stage(uint8_t *qst, const uint8_t *fw, const uint8_t *rc, uint32_t qlen) {
  constexpr uint32_t CP = Sw16Geo<G, C>::CP, QST = Sw16Geo<G, C>::QST;
  bool bad = false;
  for (uint32_t t = threadIdx.x; t < QST; t += 64) {
    const uint32_t gg = t / CP, cc = t % CP, j = gg * (uint32_t)C + cc;
    uint32_t a = 0x0cu, r = 0x0cu;
    if (cc < (uint32_t)C && j < qlen) {
      a = fw[j];
      if (RAW) { bad = bad || (a & 7u) >= 4u; a &= 3u; r = a; }
      else r = rc[j];
    }
    qst[t] = (uint8_t)a; qst[QST + t] = (uint8_t)r;
  }
  return RAW && __any(bad);
}
// the C selector bytes of lane g from the staged read
template <int G, int C, int NW>
__device__ inline void sw16_fetch(uint32_t (&x)[NW], const uint8_t *qst, int g, bool rev) {
  const u32_alias *src = (const u32_alias *)(qst + (rev ? (int)Sw16Geo<G, C>::QST : 0) + g * (int)Sw16Geo<G, C>::CP);
#pragma unroll
  for (int w = 0; w < NW; w++) x[w] = src[w];
}
// sel[cc]: selector bytes {qA, 4 + qB} of column cc next to two bytes 0x0c (half floats: the score byte is the high byte)
template <int G, int C, int NW>
__device__ inline void sw16_sel(uint32_t (&sel)[C], const uint32_t (&xa)[NW], const uint32_t (&xb)[NW], int fp) {
  uint32_t xh[NW];
#pragma unroll
  for (int w = 0; w < NW; w++) xh[w] = xb[w] + 0x04040404u - ((xb[w] & 0x08080808u) >> 1);     // + 4 on the codes, 0x0c stays
  if (fp) {
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      const uint32_t t = (uint32_t)(cc & 3);
      sel[cc] = __builtin_amdgcn_perm(xh[cc >> 2], xa[cc >> 2], 0x000c000cu | (t << 8) | ((4u + t) << 24)) | 0x000c000cu;
    }
  } else {
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      const uint32_t t = (uint32_t)(cc & 3);
      sel[cc] = __builtin_amdgcn_perm(xh[cc >> 2], xa[cc >> 2], 0x0c000c00u | t | ((4u + t) << 16)) | 0x0c000c00u;
    }
  }
}

// Entry 0 of a task's window array (row -(G-1)) is base s of word wbase of ix.packed; wbase may lie before word 0.
template <int G>
__device__ inline void sw16_win_origin(uint64_t gbase, bool small, int64_t &wbase, uint32_t &s) {
  uint64_t w0; uint32_t r0;
  if (small) { const uint32_t p32 = (uint32_t)gbase, w = p32 / 10u; w0 = w; r0 = p32 - w * 10u; }     // wave-uniform choice: a multiply-high
  else { w0 = gbase / 10; r0 = (uint32_t)(gbase - w0 * 10); }
  const uint32_t a = r0 + 20u - (uint32_t)(G - 1), qq = a / 10u;
  s = a - qq * 10u;
  wbase = (int64_t)w0 - 2 + (int64_t)qq;
}
// ten packed codes at once: 7 -> A (0), 4, 5, 6 -> N (5)
__device__ inline uint32_t sw16_map10(uint32_t w) {
  const uint32_t b2 = w & 0x24924924u;                       // bit 2 of every code
  const uint32_t is7 = b2 & (w << 1) & (w << 2);
  const uint32_t isn = b2 ^ is7;
  const uint32_t full = b2 | (b2 >> 1) | (b2 >> 2);
  return (w & ~full) | isn | (isn >> 2);
}
// codes of entries 10 m .. 10 m + 9 of one task (entry d in bits 3 (9 - d)); rows outside the window are N
// (words wbase + m and the next one, both kept inside the packed array: mlo, mhi are the task's bounds of m for that)
template <int G>
__device__ inline uint32_t sw16_codes10(const uint32_t *packed, int64_t wbase, uint32_t s, uint32_t m, uint32_t mlo, uint32_t mhi, uint32_t wlen) {
  const uint32_t ka = min(max(m, mlo), mhi), kb = min(max(m + 1u, mlo), mhi);
  const uint32_t *pw = packed + wbase;
  const uint32_t hi = pw[ka] & 0x3fffffffu, lo = pw[kb] & 0x3fffffffu;
  const uint64_t cat = ((uint64_t)hi << 30) | lo;
  const uint32_t raw = (uint32_t)(cat >> (3u * (10u - s))) & 0x3fffffffu;
  const int i0 = (int)(10u * m) - (G - 1);                   // row of entry 10 m
  int dlo = -i0, dhi = (int)wlen - i0;
  dlo = dlo < 0 ? 0 : (dlo > 10 ? 10 : dlo);
  dhi = dhi < 0 ? 0 : (dhi > 10 ? 10 : dhi);
  const uint32_t valid = ((1u << (3 * (10 - dlo))) - 1u) & ~((1u << (3 * (10 - dhi))) - 1u);
  return (sw16_map10(raw) & valid) | (SW16_N10 & ~valid);
}
// the window array of a lane group: entry e = row e - (G-1) as (code of task A | code of task B << 3) x 8, N pairs around the windows
template <int G>
__device__ inline void sw16_window(uint16_t *wrow, int g, uint32_t nent, const uint32_t *packed, int64_t lastw, const int64_t (&wbase)[2],
                                   const uint32_t (&ws)[2], const uint32_t (&wlen)[2]) {
  u32_alias *dst = (u32_alias *)wrow;
  const uint32_t nchunk = (nent + 9u) / 10u;
  uint32_t mlo[2], mhi[2];
#pragma unroll
  for (int u = 0; u < 2; u++) {                               // wbase >= -2 and wbase <= lastw
    const int64_t room = lastw - wbase[u];
    mlo[u] = wbase[u] < 0 ? (uint32_t)(-wbase[u]) : 0u;
    mhi[u] = room > 0x7fffffff ? 0x7fffffffu : (uint32_t)room;
  }
  for (uint32_t m = (uint32_t)g; m < nchunk; m += G) {
    const uint32_t ma = sw16_codes10<G>(packed, wbase[0], ws[0], m, mlo[0], mhi[0], wlen[0]);
    const uint32_t mb = sw16_codes10<G>(packed, wbase[1], ws[1], m, mlo[1], mhi[1], wlen[1]);
#pragma unroll
    for (int pr = 0; pr < 5; pr++) {
      const int s0 = 3 * (9 - 2 * pr), s1 = s0 - 3;
      const uint32_t e0 = ((ma >> s0) & 7u) | (((mb >> s0) & 7u) << 3), e1 = ((ma >> s1) & 7u) | (((mb >> s1) & 7u) << 3);
      dst[5 * m + (uint32_t)pr] = (e0 | (e1 << 16)) << 3;                   // pair x 8 in either half (< 512: no carry across)
    }
  }
}

// The score tables of the forms a launch may run (frames bit 0: row frame, bit 1: pair frame) and the longest sweep of
// either frame, -1 where the form is off or does not hold these penalties.
__device__ inline void sw16_tabs(uint2 *rowtab2, uint2 *rowtab2r, uint2 *rowtab2p, const Sw16Par &sp, int frames, int &rf_steps, int &pf_steps) {
  sw16_rowtab2(rowtab2, sp);
  rf_steps = (frames & 1) ? sp.rf_steps : -1;      // sweeps up to this many steps run in the row frame
  pf_steps = (frames & 2) ? sp.pf_steps : -1;      // and up to this many in the pair frame, which goes first
  if (rf_steps >= 0) sw16_rowtab2r(rowtab2r, sp);
  if (pf_steps >= 0) sw16_rowtab2p(rowtab2p, sp);
}
// steps of the wave's sweep: the longest window among its tasks (wmax: the longer one of this group), the groups' skew
template <int G>
__device__ inline int sw16_nstep(uint32_t wmax) {
  int nstep = (int)wmax + G - 1;
  for (int o = 32; o > 0; o >>= 1) nstep = max(nstep, __shfl_xor(nstep, o));
  return __builtin_amdgcn_readfirstlane(nstep);                          // wave-uniform: a scalar loop bound for the sweep
}
// The choice of form, by the sweep's length; nstep is wave-uniform (sw16_nstep): scalar branches.
template <int G, int C>
__device__ inline uint32_t sw16_sweep(const uint16_t *wrow, int nstep, const uint32_t (&sel)[C], int g, const Sw16Par &sp, int rf_steps, int pf_steps,
                                      const uint2 *rowtab2, const uint2 *rowtab2r, const uint2 *rowtab2p) {
  return nstep <= pf_steps ? sw16p_core<G, C>(wrow, nstep, sel, g, sp, rowtab2, rowtab2r, rowtab2p)
         : nstep <= rf_steps ? sw16r_core<G, C>(wrow, nstep, sel, g, sp, rowtab2r)
         : sp.fp ? sw16f_core<G, C>(wrow, nstep, sel, g, sp, rowtab2) : sw16_core<G, C>(wrow, nstep, sel, g, sp, rowtab2);
}

template <int G, int C, int WMAX>
__global__ void __launch_bounds__(64) k_sw_full16(Batch b, DevIndex ix, MapPar p, uint32_t ntask_cap, int frames) {
  // the small-LDS instance (WMAX = SW_SHORT_WMAX) runs first; the large one only sees what is left
  // (through the list S7 made of them; if the list overflowed, by scanning all candidates)
  const unsigned long long nlong = WMAX > SW_SHORT_WMAX ? b.work[WK_LONG_TASKS] : 0;
  if (WMAX > SW_SHORT_WMAX && nlong == 0) return;
  const uint32_t *list = (WMAX > SW_SHORT_WMAX && b.long_list && nlong <= b.long_cap) ? b.long_list : nullptr;
  constexpr int NG = 64 / G, NW = Sw16Geo<G, C>::NW;
  __shared__ __attribute__((aligned(16))) uint16_t win[NG][sw16_went(G, WMAX)];
  // each on a multiple of its 512 bytes: the paired read of two tables (ds_read2st64) counts its offsets in units of 512
  __shared__ __attribute__((aligned(512))) uint2 rowtab2[64], rowtab2r[64], rowtab2p[64];
  __shared__ __attribute__((aligned(16))) uint8_t qst[2 * Sw16Geo<G, C>::QST];
  const int lane = threadIdx.x, g = lane % G, grp = lane / G;
  const uint32_t ntask = list ? (uint32_t)nlong : min(*b.rc_count, ntask_cap), npair = (ntask + 1) / 2;
  const Sw16Par sp = sw16_par(p, G * C);
  int rf_steps, pf_steps;
  sw16_tabs(rowtab2, rowtab2r, rowtab2p, sp, frames, rf_steps, pf_steps);
  const uint32_t niter = (npair + NG - 1) / NG;                             // iterations of NG task pairs, dealt to the waves in turn
  const bool small = ix.totlen <= 0xffffffffull;
  const int64_t lastw = (int64_t)(ix.totlen / 10);
  uint32_t staged = 0xffffffffu;                                           // read whose codes are in qst
  unsigned long long cells = 0, ntasks_done = 0;
  for (uint32_t it = blockIdx.x; it < niter; it += gridDim.x) {
    const uint32_t tp = it * NG + grp;
    // lanes 0 and 1 of a group read the records of its two tasks and hand the others what they need
    uint32_t tix = 0, flags = 0, rid = 0, meta = 0, wlo = 0, whi = 0;
    {
      const uint32_t tl = 2 * tp + (uint32_t)g;
      if (g < 2 && tp < npair && tl < ntask) {
        tix = list ? list[tl] : tl;
        const RCand *rc = b.rcpool + tix;
        flags = rc->flags;
        const uint32_t r = rc->rid;
        const uint64_t rs = rc->rs;
        const uint32_t ql = read_len(b, r), wl = (uint32_t)(rc->re - rs + 1);
        if (!(flags & (RCF_BANDED | RCF_ERR | RCF_QN | RCF_SCORED)) && wl <= (uint32_t)WMAX && ql <= (uint32_t)(G * C)) {
          int64_t wb; uint32_t s;
          sw16_win_origin<G>(sw_task_gbase(ix, *rc), small, wb, s);
          rid = r; wlo = (uint32_t)(uint64_t)wb; whi = (uint32_t)((uint64_t)wb >> 32);
          meta = ql | (wl << 10) | (s << 20) | ((flags & RCF_REVERSE) ? 1u << 24 : 0u) | (1u << 25);
        }
      }
    }
    uint32_t qlen[2], wlen[2], ws[2], key[2];
    int64_t wbase[2];
    bool live[2], rev[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int src = (lane & ~(G - 1)) + u;
      const uint32_t mt = (uint32_t)__shfl((int)meta, src);
      key[u] = (uint32_t)__shfl((int)rid, src);
      wbase[u] = (int64_t)(((uint64_t)(uint32_t)__shfl((int)whi, src) << 32) | (uint32_t)__shfl((int)wlo, src));
      qlen[u] = mt & 0x3ffu; wlen[u] = (mt >> 10) & 0x3ffu; ws[u] = (mt >> 20) & 0xfu; rev[u] = (mt >> 24) & 1u; live[u] = (mt >> 25) & 1u;
    }
    const int nstep = sw16_nstep<G>(wlen[0] > wlen[1] ? wlen[0] : wlen[1]);
    sw16_window<G>(win[grp], g, (uint32_t)(nstep + G - 1), ix.packed, lastw, wbase, ws, wlen);
    // selectors: one pass per distinct read among the wave's tasks (nearly always one, and often the read staged already)
    uint32_t xa[NW], xb[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) { xa[w] = SW16_PAD4; xb[w] = SW16_PAD4; }
    bool pend0 = live[0], pend1 = live[1];
    for (;;) {
      const unsigned long long pm = __ballot(pend0 || pend1);
      if (!pm) break;
      const uint32_t R = (uint32_t)__builtin_amdgcn_readlane((int)(pend0 ? key[0] : key[1]), __ffsll(pm) - 1);
      if (R != staged) {
        __syncthreads();
        const uint64_t o = b.read_off[R];
        sw16_stage<G, C, false>(qst, b.codes + o, b.codes_rc + o, (uint32_t)(b.read_off[R + 1] - o));
        staged = R;
        __syncthreads();
      }
      if (pend0 && key[0] == R) { sw16_fetch<G, C>(xa, qst, g, rev[0]); pend0 = false; }
      if (pend1 && key[1] == R) { sw16_fetch<G, C>(xb, qst, g, rev[1]); pend1 = false; }
    }
    uint32_t sel[C];
    sw16_sel<G, C>(sel, xa, xb, sp.fp);
    __syncthreads();
    const uint32_t bb = sw16_sweep<G, C>(win[grp], nstep, sel, g, sp, rf_steps, pf_steps, rowtab2, rowtab2r, rowtab2p);
    if ((meta >> 25) & 1u) {                                               // lanes 0 and 1 with a task of their own that was scored
      const int best = (int)((bb >> (16 * g)) & 0xffffu);                   // as sw_store_score
      b.rcpool[tix].swscor = best;
      b.rcpool[tix].flags = flags | RCF_SCORED | (best >= 65535 ? RCF_BANDED : 0u);   // ERRCODE_SWATEXCEED -> K2b
      cells += (unsigned long long)(meta & 0x3ffu) * ((meta >> 10) & 0x3ffu);
      ntasks_done += best < 65535 ? 1 : 0;      /* a score that left 16 bits waits for K2b */
    }
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) { cells += __shfl_xor(cells, o); ntasks_done += __shfl_xor(ntasks_done, o); }
  if (lane == 0 && cells) { atomicAdd(b.work + WK_CELLS_FULL, cells); atomicAdd(b.work + WK_TASKS_FULL, ntasks_done); }
}

// stand-alone form over explicit code arrays (tasks with non-ACGT query codes report -2: not handled here); every task
// brings a query of its own, so the selectors take one staging pass per task
template <int G, int C>
__global__ void __launch_bounds__(64) k_sw_full16_raw(const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                                                       const uint32_t *r_off, uint32_t ntask, MapPar p, int32_t *scores, int frames) {
  constexpr int NG = 64 / G, NW = Sw16Geo<G, C>::NW;
  constexpr int WMAX = SW_FULL_WMAX;
  __shared__ uint16_t win[NG][WMAX + 2 * G];
  // each on a multiple of its 512 bytes: the paired read of two tables (ds_read2st64) counts its offsets in units of 512
  __shared__ __attribute__((aligned(512))) uint2 rowtab2[64], rowtab2r[64], rowtab2p[64];
  __shared__ __attribute__((aligned(16))) uint8_t qst[2 * Sw16Geo<G, C>::QST];
  const int lane = threadIdx.x, g = lane % G, grp = lane / G;
  const uint32_t npair = (ntask + 1) / 2;
  const Sw16Par sp = sw16_par(p, G * C);
  int rf_steps, pf_steps;
  sw16_tabs(rowtab2, rowtab2r, rowtab2p, sp, frames, rf_steps, pf_steps);
  const uint32_t ngroups = gridDim.x * NG;
  for (uint32_t t0 = blockIdx.x * NG; t0 < npair; t0 += ngroups) {
    const uint32_t tp = t0 + grp;
    bool live[2] = {false, false};
    uint32_t qlen[2] = {0, 0}, wlen[2] = {0, 0}, key[2] = {0, 0};
    const uint8_t *r[2] = {rcodes, rcodes};
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint32_t t = 2 * tp + (uint32_t)u;
      if (tp < npair && t < ntask) {
        qlen[u] = q_off[t + 1] - q_off[t]; wlen[u] = r_off[t + 1] - r_off[t];
        r[u] += r_off[t]; key[u] = t;
        live[u] = wlen[u] <= (uint32_t)WMAX && qlen[u] <= (uint32_t)(G * C);
      }
      if (!live[u]) { qlen[u] = 0; wlen[u] = 0; }
    }
    const int nstep = sw16_nstep<G>(wlen[0] > wlen[1] ? wlen[0] : wlen[1]);
    for (uint32_t e = g; e < (uint32_t)(nstep + G - 1); e += G) {
      const uint32_t i = e - (uint32_t)(G - 1);
      uint32_t cd[2];
#pragma unroll
      for (int u = 0; u < 2; u++) cd[u] = i < wlen[u] ? sw_code_of_byte(r[u][i]) : 5u;
      win[grp][e] = (uint16_t)((cd[0] | (cd[1] << 3)) << 3);                // pair x 8, as sw16_window writes it
    }
    uint32_t xa[NW], xb[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) { xa[w] = SW16_PAD4; xb[w] = SW16_PAD4; }
    bool qn[2] = {false, false};
    bool pend0 = live[0], pend1 = live[1];
    for (;;) {
      const unsigned long long pm = __ballot(pend0 || pend1);
      if (!pm) break;
      const uint32_t R = (uint32_t)__builtin_amdgcn_readlane((int)(pend0 ? key[0] : key[1]), __ffsll(pm) - 1);
      __syncthreads();
      const uint32_t o = q_off[R];
      const bool bad = sw16_stage<G, C, true>(qst, qcodes + o, qcodes + o, q_off[R + 1] - o);
      __syncthreads();
      if (pend0 && key[0] == R) { sw16_fetch<G, C>(xa, qst, g, false); qn[0] = bad; pend0 = false; }
      if (pend1 && key[1] == R) { sw16_fetch<G, C>(xb, qst, g, false); qn[1] = bad; pend1 = false; }
    }
    uint32_t sel[C];
    sw16_sel<G, C>(sel, xa, xb, sp.fp);
    __syncthreads();
    const uint32_t bb = sw16_sweep<G, C>(win[grp], nstep, sel, g, sp, rf_steps, pf_steps, rowtab2, rowtab2r, rowtab2p);
    if (g == 0) {
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const uint32_t t = 2 * tp + (uint32_t)u;
        if (tp < npair && t < ntask) scores[t] = !live[u] ? -1 : (qn[u] ? -2 : (int)((bb >> (16 * u)) & 0xffffu));
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------
// K2a for reads or windows beyond the register tiling (long reads): one wave per task.  The read is cut
// into strips of 64 x SW_STRIP_C columns (lane g owns SW_STRIP_C consecutive columns of the strip) and the
// window is swept once per strip, lane g one row behind lane g-1 (DPP wave_shr:1 hands over H of the last
// column and the running F).  H and F of a strip's last column go, row by row, through an LDS ring into a
// boundary buffer in HBM that feeds lane 0 of the next strip (read back 64 rows at a time, ahead of use).
// 32-bit lanes, full 8-byte score rows: any code (N) and any score below 2^31.
// ---------------------------------------------------------------------------------------
enum : int { SW_STRIP_C = 16 };

// win: window codes (HBM, wlen bytes), bnd: 2 x wcap (H, F) pairs of this workgroup
__device__ inline int sw_strip_core(const uint8_t *q, uint32_t qlen, const uint8_t *win, uint32_t wlen, int2 *bnd, uint32_t wcap,
                                    const uint2 *tab, int2 *ring /* LDS [256] */, int bias, int gi, int ge) {
  constexpr int C = SW_STRIP_C;
  const int g = (int)threadIdx.x;
  int2 *ring_in = ring, *ring_out = ring + 128;
  int best = 0;
  const uint32_t nstrip = (qlen + 64 * C - 1) / (64 * C);
  const int nstep = (int)wlen + 63;
  for (uint32_t sidx = 0; sidx < nstrip; sidx++) {
    const int2 *bprev = bnd + (size_t)((sidx + 1) & 1) * wcap;
    int2 *bnext = bnd + (size_t)(sidx & 1) * wcap;
    uint32_t sel[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      const uint32_t j = sidx * 64 * C + (uint32_t)(g * C + cc);
      sel[cc] = 0x0c0c0c00u | (j < qlen ? (uint32_t)(q[j] & 7) : 5u);
    }
    int H[C], E[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) { H[cc] = 0; E[cc] = 0; }
    int F = 0, prev_hl = 0;
    __syncthreads();
    if (sidx > 0) {                                  // first 64 boundary rows of the previous strip
      const int r0 = g;
      ring_in[g] = r0 < (int)wlen ? bprev[r0] : make_int2(0, 0);
    }
    __syncthreads();
    for (int step = 0; step < nstep; step++) {
      const int row = step - g;
      if (sidx > 0 && (step & 63) == 0) {            // read ahead: boundary rows step+64 .. step+127
        const int r1 = step + 64 + g;
        ring_in[((step >> 6) + 1) % 2 * 64 + g] = r1 < (int)wlen ? bprev[r1] : make_int2(0, 0);
      }
      const uint32_t rb = (row >= 0 && row < (int)wlen) ? win[row] : 5u;
      const uint2 tr = tab[rb];
      int hl = wave_shr1(H[C - 1]);
      int fin = wave_shr1(F);
      if (g == 0) {
        if (sidx > 0) { const int2 v = ring_in[(step >> 6) % 2 * 64 + (step & 63)]; hl = step < (int)wlen ? v.x : 0; fin = step < (int)wlen ? v.y : 0; }
        else { hl = 0; fin = 0; }
      }
      int diag = prev_hl;
      prev_hl = hl;
      F = fin;
#pragma unroll
      for (int cc = 0; cc < C; cc++) {
        const int w = (int)__builtin_amdgcn_perm(tr.y, tr.x, sel[cc]);
        const int h = diag + w - bias;
        const int hh = max(max(h, E[cc]), F);
        best = max(best, hh);
        diag = H[cc];
        H[cc] = hh;
        const int tt = hh - gi;
        E[cc] = max(max(E[cc] - ge, tt), 0);
        F = max(max(F - ge, tt), 0);
      }
      if (sidx + 1 < nstrip) {                       // hand the last column to the next strip
        if (g == 63 && row >= 0 && row < (int)wlen) ring_out[row & 127] = make_int2(H[C - 1], F);
        const int rdone = step - 63;                 // row lane 63 has just finished
        if (rdone >= 0 && ((rdone & 63) == 63 || rdone == (int)wlen - 1)) {
          __syncthreads();
          const int base = rdone & ~63, r2 = base + g;
          if (r2 <= rdone && r2 < (int)wlen) bnext[r2] = ring_out[r2 & 127];
        }
      }
      if (sidx > 0 && (step & 63) == 63) __syncthreads();   // the read-ahead chunk is in place before lane 0 turns to it
    }
    __threadfence();
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  return best;
}

// The same in packed 16-bit halves: two tasks per wave (as k_sw_full16; reads without non-ACGT codes, scores < 65535).
// win2: per-row code pairs (low byte task A, high byte task B); bnd: 2 x wcap packed (H pair, F pair).
// M3: every value stays below 0x7C00, so the packed maximum of three (pk_max3) applies
template <bool M3>
__device__ inline uint32_t sw_strip16_core(const uint8_t *qa, uint32_t qlen_a, const uint8_t *qb, uint32_t qlen_b, const uint16_t *win2, uint32_t wmax,
                                           uint2 *bnd, uint32_t wcap, const uint32_t *rowtab, uint2 *ring /* LDS [256] */, const Sw16Par &sp) {
  constexpr int C = SW_STRIP_C;
  const int g = (int)threadIdx.x;
  uint2 *ring_in = ring, *ring_out = ring + 128;
  us2 best = us2{0, 0};
  const uint32_t qmaxlen = qlen_a > qlen_b ? qlen_a : qlen_b;
  const uint32_t nstrip = (qmaxlen + 64 * C - 1) / (64 * C);
  const int nstep = (int)wmax + 63;
  for (uint32_t sidx = 0; sidx < nstrip; sidx++) {
    const uint2 *bprev = bnd + (size_t)((sidx + 1) & 1) * wcap;
    uint2 *bnext = bnd + (size_t)(sidx & 1) * wcap;
    uint32_t sel[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) {
      const uint32_t j = sidx * 64 * C + (uint32_t)(g * C + cc);
      const uint32_t sa = j < qlen_a ? (uint32_t)(qa[j] & 3) : 0x0cu, sb = j < qlen_b ? 4u + (uint32_t)(qb[j] & 3) : 0x0cu;
      sel[cc] = 0x0c000c00u | sa | (sb << 16);
    }
    us2 H[C], E[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) { H[cc] = us2{0, 0}; E[cc] = us2{0, 0}; }
    us2 F = us2{0, 0}, prev_hl = us2{0, 0};
    __syncthreads();
    if (sidx > 0) ring_in[g] = g < (int)wmax ? bprev[g] : make_uint2(0, 0);
    __syncthreads();
    for (int step = 0; step < nstep; step++) {
      const int row = step - g;
      if (sidx > 0 && (step & 63) == 0) {
        const int r1 = step + 64 + g;
        ring_in[((step >> 6) + 1) % 2 * 64 + g] = r1 < (int)wmax ? bprev[r1] : make_uint2(0, 0);
      }
      const uint32_t rp = (row >= 0 && row < (int)wmax) ? win2[row] : 0x0505u;
      const uint32_t rowA = rowtab[rp & 0xffu], rowB = rowtab[rp >> 8];
      uint32_t hl = (uint32_t)wave_shr1((int)as_u32(H[C - 1]));
      uint32_t fin = (uint32_t)wave_shr1((int)as_u32(F));
      if (g == 0) {
        if (sidx > 0) { const uint2 v = ring_in[(step >> 6) % 2 * 64 + (step & 63)]; hl = step < (int)wmax ? v.x : 0u; fin = step < (int)wmax ? v.y : 0u; }
        else { hl = 0; fin = 0; }
      }
      us2 carry = prev_hl;
      prev_hl = as_us2(hl);
      F = as_us2(fin);
#pragma unroll
      for (int c0 = 0; c0 < C; c0 += 4) {
        us2 t3[4];
        const us2 last_old = H[c0 + 3];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const us2 w = as_us2(__builtin_amdgcn_perm(rowB, rowA, sel[c0 + u]));
          const us2 dg = u == 0 ? carry : H[c0 + u - 1];
          t3[u] = pk_subs(pk_add_nc(dg, w), sp.bias);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const us2 hh = M3 ? pk_max3(t3[u], E[c0 + u], F) : pk_max(pk_max(t3[u], E[c0 + u]), F);
          if (!M3) best = pk_max(best, hh);
          H[c0 + u] = hh;
          const us2 tt = pk_subs(hh, sp.gi);
          E[c0 + u] = pk_max(pk_subs(E[c0 + u], sp.ge), tt);
          F = pk_max(pk_subs(F, sp.ge), tt);
        }
        if (M3) { best = pk_max3(best, H[c0], H[c0 + 1]); best = pk_max3(best, H[c0 + 2], H[c0 + 3]); }
        carry = last_old;
      }
      if (sidx + 1 < nstrip) {
        if (g == 63 && row >= 0 && row < (int)wmax) ring_out[row & 127] = make_uint2(as_u32(H[C - 1]), as_u32(F));
        const int rdone = step - 63;
        if (rdone >= 0 && ((rdone & 63) == 63 || rdone == (int)wmax - 1)) {
          __syncthreads();
          const int r2 = (rdone & ~63) + g;
          if (r2 <= rdone && r2 < (int)wmax) bnext[r2] = ring_out[r2 & 127];
        }
      }
      if (sidx > 0 && (step & 63) == 63) __syncthreads();
    }
    __threadfence();
  }
  uint32_t bb = as_u32(best);
  for (int o = 32; o > 0; o >>= 1) bb = as_u32(pk_max(as_us2(bb), as_us2((uint32_t)__shfl_xor((int)bb, o))));
  return bb;
}

// packed strip kernel over the strip list: two consecutive list entries per wave; reads with non-ACGT codes are left
// to k_sw_strip (32-bit lanes), which runs afterwards on whatever is still unscored
template <bool M3>
__global__ void __launch_bounds__(64) k_sw_strip16(Batch b, DevIndex ix, MapPar p, uint2 *bnd_all, uint16_t *win_all, uint32_t wcap) {
  const unsigned long long nlist = b.work[WK_STRIP_TASKS];
  if (nlist == 0 || !b.strip_list || nlist > b.strip_cap) return;
  __shared__ uint32_t rowtab[8];
  __shared__ uint2 ring[256];
  const Sw16Par sp = sw16_par(p);
  sw16_rowtab(rowtab, sp);
  __syncthreads();
  const uint32_t npair = ((uint32_t)nlist + 1) / 2;
  uint2 *bnd = bnd_all + (size_t)blockIdx.x * 2 * wcap;
  uint16_t *win = win_all + (size_t)blockIdx.x * wcap;
  unsigned long long cells = 0, ntasks_done = 0;
  __shared__ uint32_t qslot;
  // pairs from a cursor, not by a static stride: windows of 8 kbp reads differ in length, and the launch has more workgroups
  // than are resident at a time
  for (uint32_t tp = next_item(b.strip_cursor, &qslot); tp < npair; tp = next_item(b.strip_cursor, &qslot)) {
    RCand c[2];
    bool live[2] = {false, false};
    uint32_t qlen[2] = {0, 0}, wlen[2] = {0, 0}, tix[2] = {0, 0};
    uint64_t gbase[2] = {0, 0};
    const uint8_t *q[2] = {b.codes, b.codes};
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint32_t tl = 2 * tp + (uint32_t)u;
      if (tl < (uint32_t)nlist) {
        tix[u] = b.strip_list[tl];
        c[u] = b.rcpool[tix[u]];
        qlen[u] = read_len(b, c[u].rid);
        wlen[u] = (uint32_t)(c[u].re - c[u].rs + 1);
        live[u] = !(c[u].flags & (RCF_BANDED | RCF_ERR | RCF_QN | RCF_SCORED)) && wlen[u] <= wcap;
        gbase[u] = sw_task_gbase(ix, c[u]);
        q[u] = sw_task_query(b, c[u]);
      }
      if (!live[u]) { qlen[u] = 0; wlen[u] = 0; }
    }
    const uint32_t wmax = wlen[0] > wlen[1] ? wlen[0] : wlen[1];
    if (wmax == 0) continue;                                   // wave-uniform
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wmax; i += 64) {
      const uint32_t a = i < wlen[0] ? ref_code(ix.packed, gbase[0] + i) : 5u, bb = i < wlen[1] ? ref_code(ix.packed, gbase[1] + i) : 5u;
      win[i] = (uint16_t)(a | (bb << 8));
    }
    __threadfence();
    __syncthreads();
    const uint32_t bb = sw_strip16_core<M3>(q[0], qlen[0], q[1], qlen[1], win, wmax, bnd, wcap, rowtab, ring, sp);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int u = 0; u < 2; u++) {
        if (live[u]) {
          const int best = (int)((bb >> (16 * u)) & 0xffffu);               // as sw_store_score
          b.rcpool[tix[u]].swscor = best;
          b.rcpool[tix[u]].flags = c[u].flags | RCF_SCORED | (best >= 65535 ? RCF_BANDED : 0u);   // ERRCODE_SWATEXCEED -> K2b
          cells += (unsigned long long)qlen[u] * wlen[u];
          ntasks_done += best < 65535 ? 1 : 0;      /* a score that left 16 bits waits for K2b */
        }
      }
    }
  }
  if (threadIdx.x == 0 && cells) { atomicAdd(b.work + WK_CELLS_FULL, cells); atomicAdd(b.work + WK_TASKS_FULL, ntasks_done); }
}

// tasks: the strip list S7 made (ranked candidates whose read or window exceeds the register tiling)
__global__ void __launch_bounds__(64) k_sw_strip(Batch b, DevIndex ix, MapPar p, int2 *bnd_all, uint8_t *win_all, uint32_t wcap) {
  const unsigned long long nlist = b.work[WK_STRIP_TASKS];
  if (nlist == 0) return;
  __shared__ uint2 tab[8];
  __shared__ int2 ring[256];
  const int bias = sw_bias(p);
  sw_tab8(tab, p, bias);
  __syncthreads();
  const bool listed = b.strip_list && nlist <= b.strip_cap;
  const uint32_t ntask = listed ? (uint32_t)nlist : min(*b.rc_count, b.rccap);
  int2 *bnd = bnd_all + (size_t)blockIdx.x * 2 * wcap;
  uint8_t *win = win_all + (size_t)blockIdx.x * wcap;
  unsigned long long cells = 0, ntasks_done = 0;
  for (uint32_t tl = blockIdx.x; tl < ntask; tl += gridDim.x) {
    const uint32_t t = listed ? b.strip_list[tl] : tl;
    const RCand c = b.rcpool[t];
    const uint32_t qlen = read_len(b, c.rid), wlen = (uint32_t)(c.re - c.rs + 1);
    if ((c.flags & (RCF_BANDED | RCF_ERR | RCF_SCORED)) || wlen > wcap) continue;     // wave-uniform
    const uint64_t gbase = sw_task_gbase(ix, c);
    const uint8_t *q = sw_task_query(b, c);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wlen; i += 64) win[i] = (uint8_t)ref_code(ix.packed, gbase + i);
    __threadfence();
    __syncthreads();
    const int best = sw_strip_core(q, qlen, win, wlen, bnd, wcap, tab, ring, bias, -p.gap_init, -p.gap_ext);
    if (threadIdx.x == 0) sw_store_score(b.rcpool + t, c.flags, best, qlen, wlen, cells, ntasks_done);
  }
  if (threadIdx.x == 0 && cells) { atomicAdd(b.work + WK_CELLS_FULL, cells); atomicAdd(b.work + WK_TASKS_FULL, ntasks_done); }
}

// stand-alone form over explicit code arrays (parity tests)
__global__ void __launch_bounds__(64) k_sw_strip_raw(const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes, const uint32_t *r_off,
                                                     uint32_t ntask, MapPar p, int32_t *scores, int2 *bnd_all, uint8_t *win_all, uint32_t wcap) {
  __shared__ uint2 tab[8];
  __shared__ int2 ring[256];
  const int bias = sw_bias(p);
  sw_tab8(tab, p, bias);
  __syncthreads();
  int2 *bnd = bnd_all + (size_t)blockIdx.x * 2 * wcap;
  uint8_t *win = win_all + (size_t)blockIdx.x * wcap;
  for (uint32_t t = blockIdx.x; t < ntask; t += gridDim.x) {
    const uint32_t qlen = q_off[t + 1] - q_off[t], wlen = r_off[t + 1] - r_off[t];
    if (wlen > wcap) { if (threadIdx.x == 0) scores[t] = -1; continue; }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wlen; i += 64) win[i] = (uint8_t)sw_code_of_byte(rcodes[r_off[t] + i]);
    __threadfence();
    __syncthreads();
    const int best = sw_strip_core(qcodes + q_off[t], qlen, win, wlen, bnd, wcap, tab, ring, bias, -p.gap_init, -p.gap_ext);
    if (threadIdx.x == 0) scores[t] = best;
  }
}

// stand-alone form of the packed strip kernel: tasks 2t, 2t+1 share a wave as the list entries of k_sw_strip16 do; a read
// with non-ACGT codes reports -2 (production leaves it to k_sw_strip), a window above wcap -1, and the partner runs on
template <bool M3>
__global__ void __launch_bounds__(64) k_sw_strip16_raw(const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes, const uint32_t *r_off,
                                                       uint32_t ntask, MapPar p, int32_t *scores, uint2 *bnd_all, uint16_t *win_all, uint32_t wcap) {
  __shared__ uint32_t rowtab[8];
  __shared__ uint2 ring[256];
  const Sw16Par sp = sw16_par(p);
  sw16_rowtab(rowtab, sp);
  __syncthreads();
  const uint32_t npair = (ntask + 1) / 2;
  uint2 *bnd = bnd_all + (size_t)blockIdx.x * 2 * wcap;
  uint16_t *win = win_all + (size_t)blockIdx.x * wcap;
  for (uint32_t tp = blockIdx.x; tp < npair; tp += gridDim.x) {
    bool live[2] = {false, false}, qn[2] = {false, false};
    uint32_t qlen[2] = {0, 0}, wlen[2] = {0, 0};
    const uint8_t *q[2] = {qcodes, qcodes}, *r[2] = {rcodes, rcodes};
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const uint32_t t = 2 * tp + (uint32_t)u;
      if (t < ntask) {
        qlen[u] = q_off[t + 1] - q_off[t]; wlen[u] = r_off[t + 1] - r_off[t];
        q[u] += q_off[t]; r[u] += r_off[t];
        bool bad = false;
        for (uint32_t j = threadIdx.x; j < qlen[u]; j += 64) bad |= (q[u][j] & 4) != 0;
        qn[u] = __any(bad);
        live[u] = wlen[u] <= wcap && !qn[u];
      }
      if (!live[u]) { qlen[u] = 0; wlen[u] = 0; }
    }
    const uint32_t wmax = wlen[0] > wlen[1] ? wlen[0] : wlen[1];
    uint32_t bb = 0;
    if (wmax) {                                                  // wave-uniform
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < wmax; i += 64) {
        uint32_t cd[2];
#pragma unroll
        for (int u = 0; u < 2; u++) cd[u] = i < wlen[u] ? sw_code_of_byte(r[u][i]) : 5u;
        win[i] = (uint16_t)(cd[0] | (cd[1] << 8));
      }
      __threadfence();
      __syncthreads();
      bb = sw_strip16_core<M3>(q[0], qlen[0], q[1], qlen[1], win, wmax, bnd, wcap, rowtab, ring, sp);
    }
    if (threadIdx.x == 0) {
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const uint32_t t = 2 * tp + (uint32_t)u;
        if (t < ntask) scores[t] = live[u] ? (int)((bb >> (16 * u)) & 0xffffu) : (qn[u] ? -2 : -1);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// K2b (alignSmiWatBandFast, alignment.c:1029-1233) for long reads: one wave per task, the strip scheme of
// sw_strip_core with the restricted cell update and the band as an activity mask.  Row r of the band visits the
// columns [js(r), jl(r)): js(r) = q_left for ever when the band starts clipped at the read's left end (the
// reference never advances it then), l_edge + r otherwise; jl(r) = min(r_edge + 1 + r, q_len).  Cells outside keep
// H and E (the reference's row buffers persist) and hand F = 0 to the right; every value a visited cell reads
// from an unvisited neighbour is then what the reference reads (0 for a cell never visited, else the stale
// buffer value, which only cells on the same diagonal -- visited or never visited together -- can reach).
// A strip sweeps only the rows in which it has visited cells.
// ---------------------------------------------------------------------------------------
__device__ inline int band_fast_wave(const Band &bp, const uint8_t *q, const uint8_t *win /* row i of the window */, int2 *bnd, uint32_t wcap,
                                     const uint2 *tab, int2 *ring /* LDS [256] */, int bias, int gi, int ge) {
  constexpr int C = SW_STRIP_C;
  const int g = (int)threadIdx.x;
  const bool clipped = bp.q_left > bp.l_edge;
  const int j0 = clipped ? bp.q_left : bp.l_edge;
  const int nrows = bp.s_len - bp.s_left;
  if (nrows <= 0) return 0;
  const int jmax = min(bp.r_edge + nrows, bp.q_len);          // jl(nrows - 1)
  if (jmax <= j0 || (uint32_t)nrows > wcap) return 0;
  const int nstrip = (jmax - j0 + 64 * C - 1) / (64 * C);
  int2 *ring_in = ring, *ring_out = ring + 128;
  int best = 0, plo = 0, phi = 0;                             // [plo, phi): rows the previous strip swept
  for (int sidx = 0; sidx < nstrip; sidx++) {
    const int c_lo = j0 + sidx * 64 * C, c_hi = c_lo + 64 * C;
    const int r_lo = max(c_lo - bp.r_edge, 0);
    const int r_hi = clipped ? nrows : min(nrows, c_hi - bp.l_edge);
    const int nr = r_hi - r_lo;
    const int2 *bprev = bnd + (size_t)((sidx + 1) & 1) * wcap;
    int2 *bnext = bnd + (size_t)(sidx & 1) * wcap;
    const int jb = c_lo + g * C;
    uint32_t sel[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) sel[cc] = 0x0c0c0c00u | (jb + cc < bp.q_len ? (uint32_t)(q[jb + cc] & 7) : 5u);
    int H[C], E[C];
#pragma unroll
    for (int cc = 0; cc < C; cc++) { H[cc] = 0; E[cc] = 0; }
    int F = 0, prev_hl = 0;
#define SMG_BGET(r) ((sidx > 0 && (r) >= plo && (r) < phi) ? bprev[(r)] : make_int2(0, 0))
    __syncthreads();
    if (sidx > 0) {
      ring_in[g] = SMG_BGET(r_lo + g);
      if (g == 0) prev_hl = SMG_BGET(r_lo - 1).x;
    }
    __syncthreads();
    const int nstep = nr + 63;
    for (int step = 0; step < nstep; step++) {
      const int rel = step - g, row = r_lo + rel;
      if (sidx > 0 && (step & 63) == 0) ring_in[((step >> 6) + 1) % 2 * 64 + g] = SMG_BGET(r_lo + step + 64 + g);
      const bool rowok = rel >= 0 && rel < nr;
      const uint32_t rb = rowok ? win[bp.s_left + row] : 5u;
      const uint2 tr = tab[rb];
      int hl = wave_shr1(H[C - 1]);
      int fin = wave_shr1(F);
      if (g == 0) {
        if (sidx > 0) { const int2 v = ring_in[(step >> 6) % 2 * 64 + (step & 63)]; hl = v.x; fin = v.y; }
        else { hl = 0; fin = 0; }
      }
      int diag = prev_hl;
      prev_hl = hl;
      F = fin;
      if (rowok) {
        const int jsr = clipped ? bp.q_left : bp.l_edge + row;
        const int jlr = min(bp.r_edge + 1 + row, bp.q_len);
#pragma unroll
        for (int cc = 0; cc < C; cc++) {
          const int hold = H[cc];
          const int j = jb + cc;
          if (j >= jsr && j < jlr) {
            const int hin = diag + (int)__builtin_amdgcn_perm(tr.y, tr.x, sel[cc]) - bias;
            bool cand;
            (void)cell_update(H[cc], E[cc], F, hin, gi, ge, cand);
            if (cand && hin > best) best = hin;
          } else F = 0;
          diag = hold;
        }
      } else F = 0;
      if (sidx + 1 < nstrip) {                       // hand the last column to the next strip
        if (g == 63 && rowok) ring_out[rel & 127] = make_int2(H[C - 1], F);
        const int rdone = step - 63;                 // row lane 63 has just finished
        if (rdone >= 0 && ((rdone & 63) == 63 || rdone == nr - 1)) {
          __syncthreads();
          const int base = rdone & ~63, r2 = base + g;
          if (r2 <= rdone && r2 < nr) bnext[r_lo + r2] = ring_out[r2 & 127];
        }
      }
      if (sidx > 0 && (step & 63) == 63) __syncthreads();   // the read-ahead chunk is in place before lane 0 turns to it
    }
#undef SMG_BGET
    plo = r_lo; phi = r_hi;
    __threadfence();
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  return best;
}

// banded tasks of long reads (S7 lists them with the strip tasks) and K2a tasks whose score left 16 bits
__global__ void __launch_bounds__(64) k_sw_band(Batch b, DevIndex ix, MapPar p, int2 *bnd_all, uint8_t *win_all, uint32_t wcap) {
  const unsigned long long nlist = b.work[WK_STRIP_TASKS];
  if (nlist == 0 || !b.strip_list || nlist > b.strip_cap) return;       // k_sw_scalar takes whatever is left
  __shared__ uint2 tab[8];
  __shared__ int2 ring[256];
  const int bias = sw_bias(p);
  sw_tab8(tab, p, bias);
  __syncthreads();
  int2 *bnd = bnd_all + (size_t)blockIdx.x * 2 * wcap;
  uint8_t *win = win_all + (size_t)blockIdx.x * wcap;
  unsigned long long nband = 0;
  for (uint32_t tl = blockIdx.x; tl < (uint32_t)nlist; tl += gridDim.x) {
    const uint32_t t = b.strip_list[tl];
    const RCand c = b.rcpool[t];
    const uint32_t qlen = read_len(b, c.rid), wlen = (uint32_t)(c.re - c.rs + 1);
    if (!(c.flags & RCF_BANDED) || (c.flags & (RCF_ERR | RCF_BSCORED)) || wlen > wcap) continue;     // wave-uniform
    Band bd;
    if (band_init(bd, c.band_l, c.band_r, (int)c.qs, (int)c.qe, (int)qlen, 0, (int)wlen - 1, (int)wlen)) {
      if (threadIdx.x == 0) b.rcpool[t].flags = c.flags | RCF_ERR;
      continue;
    }
    const uint64_t gbase = sw_task_gbase(ix, c);
    const uint8_t *q = sw_task_query(b, c);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wlen; i += 64) win[i] = (uint8_t)ref_code(ix.packed, gbase + i);
    __threadfence();
    __syncthreads();
    const int best = band_fast_wave(bd, q, win, bnd, wcap, tab, ring, bias, -p.gap_init, -p.gap_ext);
    if (threadIdx.x == 0) {
      b.rcpool[t].swscor = best;
      b.rcpool[t].flags = c.flags | RCF_SCORED | RCF_BSCORED;
      nband++;
    }
  }
  if (threadIdx.x == 0 && nband) atomicAdd(b.work + WK_TASKS_FULL, nband);
}

// K2a for tasks the register-tiled kernel does not cover (long reads / long windows) and
// K2b (banded score-only pass, alignment.c:1029) -- one lane per task, rows in HBM scratch.
__global__ void __launch_bounds__(64) k_sw_scalar(Batch b, DevIndex ix, MapPar p, int *rows, uint32_t rowlen, int full_gc) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nthr = gridDim.x * blockDim.x;
  const uint32_t ntask = min(*b.rc_count, b.rccap);      // the cursor runs past the pool when it overflows (reads keep SMG_ERR_CAP)
  if (b.work[WK_TASKS_FULL] >= (unsigned long long)ntask) return;      // every ranked candidate has its score already (the usual case)
  int *Hp = rows + (size_t)tid * 2 * rowlen, *Ep = Hp + rowlen;
  int8_t M[64];
  score_matrix(M, p.match, p.mismatch);
  for (uint32_t t = tid; t < ntask; t += nthr) {
    RCand c = b.rcpool[t];
    if (c.flags & (RCF_ERR | RCF_SCORED)) { if (!(c.flags & RCF_BANDED) || (c.flags & (RCF_ERR | RCF_BSCORED))) continue; }
    const uint32_t qlen = read_len(b, c.rid), wlen = (uint32_t)(c.re - c.rs + 1);
    const uint8_t *q = sw_task_query(b, c);
    const uint64_t gbase = sw_task_gbase(ix, c);
    bool banded = (c.flags & RCF_BANDED) != 0;
    if (!banded) {
      if (wlen <= (uint32_t)SW_FULL_WMAX && qlen <= (uint32_t)full_gc) continue;   // k_sw_full did / will do it
      c.swscor = sw_full_scalar(q, qlen, ix.packed, gbase, wlen, M, -p.gap_init, -p.gap_ext, Hp, Ep);
      if (c.swscor >= 65535) banded = true;
    }
    if (banded) {
      Band bd;
      if (band_init(bd, c.band_l, c.band_r, (int)c.qs, (int)c.qe, (int)qlen, 0, (int)wlen - 1, (int)wlen)) { b.rcpool[t].flags = c.flags | RCF_ERR; continue; }
      c.swscor = band_fast_scalar(bd, q, ix.packed, gbase, M, -p.gap_init, -p.gap_ext, Hp, Ep);
    }
    b.rcpool[t].swscor = c.swscor;
    b.rcpool[t].flags = c.flags | RCF_SCORED;
  }
}

// stand-alone K2b over explicit reads and a packed array of windows (parity tests): band[t] = {band_l, band_r, qs, qe};
// a band that band_init refuses keeps score 0 (the host reports it in the status).  One wave per task, as k_sw_band ...
__global__ void __launch_bounds__(64) k_sw_band_raw(const uint8_t *qcodes, const uint32_t *q_off, const uint32_t *packed, const uint32_t *r_off,
                                                    uint32_t ntask, MapPar p, const int4 *band, int32_t *scores, int2 *bnd_all, uint8_t *win_all,
                                                    uint32_t wcap) {
  __shared__ uint2 tab[8];
  __shared__ int2 ring[256];
  const int bias = sw_bias(p);
  sw_tab8(tab, p, bias);
  __syncthreads();
  int2 *bnd = bnd_all + (size_t)blockIdx.x * 2 * wcap;
  uint8_t *win = win_all + (size_t)blockIdx.x * wcap;
  for (uint32_t t = blockIdx.x; t < ntask; t += gridDim.x) {
    const uint32_t qlen = q_off[t + 1] - q_off[t], wlen = r_off[t + 1] - r_off[t];
    const int4 bd4 = band[t];
    Band bd;
    if (wlen > wcap || band_init(bd, bd4.x, bd4.y, bd4.z, bd4.w, (int)qlen, 0, (int)wlen - 1, (int)wlen)) {     // wave-uniform
      if (threadIdx.x == 0) scores[t] = 0;
      continue;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < wlen; i += 64) win[i] = (uint8_t)ref_code(packed, (uint64_t)r_off[t] + i);
    __threadfence();
    __syncthreads();
    const int best = band_fast_wave(bd, qcodes + q_off[t], win, bnd, wcap, tab, ring, bias, -p.gap_init, -p.gap_ext);
    if (threadIdx.x == 0) scores[t] = best;
  }
}

// ... and one lane per task, as the banded tasks of k_sw_scalar; rows: 2 x rowlen ints per lane
__global__ void __launch_bounds__(64) k_sw_band_scalar_raw(const uint8_t *qcodes, const uint32_t *q_off, const uint32_t *packed, const uint32_t *r_off,
                                                           uint32_t ntask, MapPar p, const int4 *band, int32_t *scores, int *rows, uint32_t rowlen) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntask) return;
  int *Hp = rows + (size_t)t * 2 * rowlen, *Ep = Hp + rowlen;
  int8_t M[64];
  score_matrix(M, p.match, p.mismatch);
  const uint32_t qlen = q_off[t + 1] - q_off[t], wlen = r_off[t + 1] - r_off[t];
  const int4 bd4 = band[t];
  Band bd;
  int best = 0;
  if (!band_init(bd, bd4.x, bd4.y, bd4.z, bd4.w, (int)qlen, 0, (int)wlen - 1, (int)wlen))
    best = band_fast_scalar(bd, qcodes + q_off[t], packed, (uint64_t)r_off[t], M, -p.gap_init, -p.gap_ext, Hp, Ep);
  scores[t] = best;
}

// ---------------------------------------------------------------------------------------
// host-side launchers (declared in smg_kernels.h)
// ---------------------------------------------------------------------------------------
#define SMG_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

int launch_encode(hipStream_t s, const uint8_t *bases, const uint64_t *off, uint32_t n, uint8_t *codes, uint8_t *codes_rc) {
  if (!n) return 0;
  uint32_t grid = n < 16384u ? n : 16384u;
  hipLaunchKernelGGL(k_encode, dim3(grid), dim3(64), 0, s, bases, off, n, codes, codes_rc);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_gather_reads(hipStream_t s, uint8_t *dst_bases, uint8_t *dst_quals, const uint64_t *dst_off, uint32_t n, const uint32_t *ids,
                        const uint8_t *const src_bases[2], const uint8_t *const src_quals[2], const uint64_t *const src_off[2]) {
  if (!n) return 0;
  const uint32_t grid = n < 32768u ? n : 32768u;
  hipLaunchKernelGGL(k_gather_reads, dim3(grid), dim3(64), 0, s, dst_bases, dst_quals, dst_off, n, ids, src_bases[0], src_bases[1],
                     dst_quals ? src_quals[0] : nullptr, dst_quals ? src_quals[1] : nullptr, src_off[0], src_off[1]);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_seed(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint8_t *scratch, size_t sbytes, uint32_t nslots, int force_hbm,
                uint32_t grid_fixed) {
  if (!b.nreads) return 0;
  const int use_lds = sbytes <= 48 * 1024 && !force_hbm;
  uint32_t items = 2 * b.nreads;
  uint32_t grid = use_lds ? (items < 32768u ? items : 32768u) : (items < nslots ? items : nslots);
  if (grid_fixed) {                                      // test entry (smaltgpu_seed_batch): a workgroup of an HBM launch owns slot blockIdx.x
    if (!use_lds && (grid_fixed > nslots || !scratch)) return (int)hipErrorInvalidValue;
    grid = grid_fixed;
  }
  if (!use_lds && !scratch) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_seed, dim3(grid), dim3(64), use_lds ? sbytes + LDS_GUARD : 0, s, b, ix, p, scratch, sbytes, use_lds);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_hits(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint32_t W, uint32_t tab, uint32_t nwg, uint32_t fill) {
  if (!b.nreads || !b.hitrun) return 0;
  const uint32_t lds_bytes = (uint32_t)((hits_lds_bytes(W, tab) + 15) & ~(size_t)15);
  const size_t seq_bytes = (ix.nseq > 0 && ix.nseq < 512) ? (((size_t)ix.nseq + 1) * 4 + 15) & ~(size_t)15 : 0;
  uint32_t grid = 2 * b.nreads < nwg ? 2 * b.nreads : nwg;
  static const int waves = getenv("SMALTGPU_HITS_WAVES") ? atoi(getenv("SMALTGPU_HITS_WAVES")) : 3;      // tuning hook (3 waves per SIMD: 148 registers, no spills; 2 and 4 measured the same)
  if (waves == 3) hipLaunchKernelGGL(k_hits<3>, dim3(grid), dim3(64), lds_bytes + LDS_GUARD + seq_bytes, s, b, ix, p, W, tab, lds_bytes, fill);
  else if (waves == 2) hipLaunchKernelGGL(k_hits<2>, dim3(grid), dim3(64), lds_bytes + LDS_GUARD + seq_bytes, s, b, ix, p, W, tab, lds_bytes, fill);
  else hipLaunchKernelGGL(k_hits<4>, dim3(grid), dim3(64), lds_bytes + LDS_GUARD + seq_bytes, s, b, ix, p, W, tab, lds_bytes, fill);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_cands(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint8_t *scratch, uint32_t nslots, const CandGeom &g) {
  if (!b.nreads) return 0;
  uint32_t grid = b.nreads < nslots ? b.nreads : nslots;
  const uint32_t lds_bytes = cands_lds_bytes(g);
  const size_t seq_bytes = (ix.nseq > 0 && ix.nseq < 512) ? (((size_t)ix.nseq + 1) * 4 + 15) & ~(size_t)15 : 0;     // LDS copy of seqlo
  if (!hits_consumed(b.qmax)) hipLaunchKernelGGL(k_cands<true>, dim3(grid), dim3(64), lds_bytes + LDS_GUARD + seq_bytes, s, b, ix, p, scratch, g, lds_bytes);
  else if (b.hitrun) {                                   // (begin_call sets it by hits_consumed(qmax) alone)
    // S3 ran ahead (k_hits): no per-list tables in this kernel's LDS block, and (tuning hook) three waves per SIMD
    static const int waves3 = getenv("SMALTGPU_CANDS_WAVES") && atoi(getenv("SMALTGPU_CANDS_WAVES")) == 3;
    const uint32_t lb = (uint32_t)((strand_work_bytes<uint16_t>(g.lds_hits) + 15) & ~(size_t)15);
    if (waves3) hipLaunchKernelGGL((k_cands<false, true, 3>), dim3(grid), dim3(64), lb + LDS_GUARD + seq_bytes, s, b, ix, p, scratch, g, lb);
    else hipLaunchKernelGGL((k_cands<false, true, 2>), dim3(grid), dim3(64), lb + LDS_GUARD + seq_bytes, s, b, ix, p, scratch, g, lb);
  }
  else hipLaunchKernelGGL(k_cands<false>, dim3(grid), dim3(64), lds_bytes + LDS_GUARD + seq_bytes, s, b, ix, p, scratch, g, lds_bytes);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_replay(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p) {
  if (!b.nreads) return 0;
  hipLaunchKernelGGL(k_replay, dim3((b.nreads + 255) / 256), dim3(256), 0, s, b, ix, p);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_align(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint8_t *scratch, size_t sbytes, uint32_t nslots,
                 uint32_t wincap, uint64_t dircap, uint32_t rescap, uint32_t dstrcap, int pass, const CplxPar *cplx) {
  if (!b.nreads) return 0;
  uint32_t grid = b.nreads < nslots ? b.nreads : nslots;
  size_t small = align_lds_small_bytes(b.qmax, wincap);
  static const uint32_t lds_kb = getenv("SMALTGPU_ALIGN_LDS_KB") ? (uint32_t)atoi(getenv("SMALTGPU_ALIGN_LDS_KB")) : 8u;   // tuning hook; 8 KB = 20 workgroups per CU
  uint32_t kb = lds_kb;
  if (b.qmax > 256 && small + 4096 > (size_t)kb * 1024 && small + 8192 <= 64 * 1024) kb = (uint32_t)((small + 8192 + 1023) / 1024);   // long reads: read, window and traceback string stay in LDS
  uint32_t lds_bytes = small + 4096 <= (size_t)kb * 1024 ? kb * 1024 - LDS_GUARD : 0;      // rows + window + direction bytes
  static const int antidiag = getenv("SMALTGPU_ALIGN_ANTIDIAG") ? 0x100 : 0;      // test hook: narrow bands in the anti-diagonal form (band_track_wave)
  pass |= antidiag;
  const size_t dyn = lds_bytes ? lds_bytes + LDS_GUARD : 0;
  if (p.flags & FLG_CMPLXW) {
    if (!cplx || !cplx->logtab || !(cplx->lambda > 0.0)) return (int)hipErrorInvalidValue;      // the weighting needs its table and lambda: no launch without them
    if (b.qmax > 256) hipLaunchKernelGGL((k_align<true, true>), dim3(grid), dim3(64), dyn, s, b, ix, p, scratch, sbytes, wincap, dircap, rescap, dstrcap, lds_bytes, pass, *cplx);
    else hipLaunchKernelGGL((k_align<false, true>), dim3(grid), dim3(64), dyn, s, b, ix, p, scratch, sbytes, wincap, dircap, rescap, dstrcap, lds_bytes, pass, *cplx);
  } else if (b.qmax > 256) hipLaunchKernelGGL((k_align<true, false>), dim3(grid), dim3(64), dyn, s, b, ix, p, scratch, sbytes, wincap, dircap, rescap, dstrcap, lds_bytes, pass, NoCplx());
  else hipLaunchKernelGGL((k_align<false, false>), dim3(grid), dim3(64), dyn, s, b, ix, p, scratch, sbytes, wincap, dircap, rescap, dstrcap, lds_bytes, pass, NoCplx());
  SMG_LAUNCH_CHECK();
  return 0;
}

// The tilings of the register-tiled K2a kernels: reads of up to qmax bases (qmax <= G * C) take G lanes of C columns.
// A new tiling is a line here and a case in sw_tiling_dispatch.
struct SwTiling { uint32_t qmax; int G, C; };
static const SwTiling sw_tilings[] = {{64, 4, 16}, {104, 8, 13}, {152, 8, 19}, {160, 8, 20}, {256, 16, 16}, {512, 16, 32}};

int sw_full_geometry(uint32_t qmax_len, int *G, int *C) {
  for (const SwTiling &t : sw_tilings)
    if (qmax_len <= t.qmax) { *G = t.G; *C = t.C; return 0; }
  *G = 0; *C = 0;
  return -1;
}

// f(SwTile<G, C>()): the tiling as compile-time constants; false for a tiling that has no instances
template <int TG, int TC> struct SwTile { enum : int { G = TG, C = TC }; };
template <typename F>
static bool sw_tiling_dispatch(int G, int C, F &&f) {
#define SW_TILING(g, c) case (g) * 64 + (c): f(SwTile<g, c>()); return true
  switch (G * 64 + C) {
    SW_TILING(4, 16);
    SW_TILING(8, 13);
    SW_TILING(8, 19);
    SW_TILING(8, 20);
    SW_TILING(16, 16);
    SW_TILING(16, 32);
  }
#undef SW_TILING
  return false;
}

// the packed kernel's 16-bit lanes hold any score of a read of up to 512 bases
static bool sw16_ok(const MapPar &p) {
  const int bias = sw_bias(p);
  return p.match > 0 && p.match * 512 + bias + 256 < 0x7C00 /* pk_max3 */ && bias >= 0 && p.match + bias < 256 && p.mismatch + bias >= 0 &&
         -p.gap_init >= 0 && -p.gap_init < 30000 && -p.gap_ext >= 0 && -p.gap_ext < 30000;
}

// the packed strip kernel's max3 form: every value of the longest read stays below the half-float infinity pattern
static bool sw_strip16_max3(uint32_t qmax_len, int match) { return (uint64_t)qmax_len * (uint64_t)match + 512 < 0x7C00ull; }

// test hooks: SMALTGPU_SW16_ROWFRAME=0 keeps the packed sweep in its forms without any frame (sw16f_core, sw16_core),
// SMALTGPU_SW16_PAIRFRAME=0 gives the row frame wherever it applies, so that the forms can be compared on the same tasks;
// read at every launch, which lets one process run all three.  Bit 0: row frame, bit 1: pair frame.
static int sw16_frames_on() {
  const char *e = getenv("SMALTGPU_SW16_ROWFRAME");
  if (e && e[0] == '0') return 0;
  e = getenv("SMALTGPU_SW16_PAIRFRAME");
  return (e && e[0] == '0') ? 1 : 3;
}
int sw16_rowframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols) {
  return sw16_rowframe_steps(match, mismatch, gap_init, gap_ext, ncols);
}
int sw16_pairframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols) {
  return sw16_pairframe_steps(match, mismatch, gap_init, gap_ext, ncols);
}

int launch_sw_full(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint32_t qmax_len, uint32_t ntask_cap, uint32_t grid) {
  int G, C;
  if (sw_full_geometry(qmax_len, &G, &C)) return 0;    // nothing for the register-tiled kernel: k_sw_scalar takes all
  const int use16 = sw16_ok(p);
  const bool known = sw_tiling_dispatch(G, C, [&](auto tile) {
    constexpr int TG = decltype(tile)::G, TC = decltype(tile)::C;
    if (use16) {
      const int rf = sw16_frames_on();
      hipLaunchKernelGGL((k_sw_full16<TG, TC, SW_SHORT_WMAX>), dim3(grid), dim3(64), 0, s, b, ix, p, ntask_cap, rf);
      hipLaunchKernelGGL((k_sw_full16<TG, TC, SW_FULL_WMAX>), dim3(grid), dim3(64), 0, s, b, ix, p, ntask_cap, rf);
    }
    hipLaunchKernelGGL((k_sw_full<TG, TC>), dim3(grid), dim3(64), 0, s, b, ix, p, ntask_cap, use16);
  });
  if (!known) return (int)hipErrorInvalidValue;
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_sw_strip(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid) {
  if (!b.nreads || !grid) return 0;
  if (sw16_ok(p) && (uint64_t)b.qmax * (uint64_t)p.match < 60000ull)          // 16-bit halves hold every score of these reads
  {
    if (sw_strip16_max3(b.qmax, p.match))
      hipLaunchKernelGGL(k_sw_strip16<true>, dim3(grid), dim3(64), 0, s, b, ix, p, (uint2 *)bnd, (uint16_t *)win, wcap);
    else hipLaunchKernelGGL(k_sw_strip16<false>, dim3(grid), dim3(64), 0, s, b, ix, p, (uint2 *)bnd, (uint16_t *)win, wcap);
  }
  hipLaunchKernelGGL(k_sw_strip, dim3(grid), dim3(64), 0, s, b, ix, p, (int2 *)bnd, win, wcap);
  hipLaunchKernelGGL(k_sw_band, dim3(grid), dim3(64), 0, s, b, ix, p, (int2 *)bnd, win, wcap);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_sw_strip_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint8_t *r, const uint32_t *ro, uint32_t n, const MapPar &p,
                        int32_t *sc, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_sw_strip_raw, dim3(n < grid ? n : grid), dim3(64), 0, s, q, qo, r, ro, n, p, sc, (int2 *)bnd, win, wcap);
  SMG_LAUNCH_CHECK();
  return 0;
}

// -2: the penalties or the longest read's score do not fit 16-bit halves (the rule of launch_sw_strip, no fall-back here)
int launch_sw_strip16_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint8_t *r, const uint32_t *ro, uint32_t n, const MapPar &p,
                          int32_t *sc, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid, uint32_t qmax_len) {
  if (!n) return 0;
  if (!sw16_ok(p) || (uint64_t)qmax_len * (uint64_t)p.match >= 60000ull) return -2;
  const uint32_t npair = (n + 1) / 2;
  const dim3 g(npair < grid ? npair : grid);
  if (sw_strip16_max3(qmax_len, p.match))
    hipLaunchKernelGGL(k_sw_strip16_raw<true>, g, dim3(64), 0, s, q, qo, r, ro, n, p, sc, (uint2 *)bnd, (uint16_t *)win, wcap);
  else hipLaunchKernelGGL(k_sw_strip16_raw<false>, g, dim3(64), 0, s, q, qo, r, ro, n, p, sc, (uint2 *)bnd, (uint16_t *)win, wcap);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_sw_band_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint32_t *packed, const uint32_t *ro, uint32_t n,
                       const MapPar &p, const int32_t *band, int32_t *sc, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_sw_band_raw, dim3(n < grid ? n : grid), dim3(64), 0, s, q, qo, packed, ro, n, p, (const int4 *)band, sc, (int2 *)bnd, win, wcap);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_sw_band_scalar_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint32_t *packed, const uint32_t *ro, uint32_t n,
                              const MapPar &p, const int32_t *band, int32_t *sc, int *rows, uint32_t rowlen) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_sw_band_scalar_raw, dim3((n + 63) / 64), dim3(64), 0, s, q, qo, packed, ro, n, p, (const int4 *)band, sc, rows, rowlen);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_sw_scalar(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, int *rows, uint32_t rowlen, uint32_t nthreads,
                     uint32_t qmax_len) {
  int G, C;
  int full_gc = sw_full_geometry(qmax_len, &G, &C) ? 0 : G * C;
  hipLaunchKernelGGL(k_sw_scalar, dim3(nthreads / 64), dim3(64), 0, s, b, ix, p, rows, rowlen, full_gc);
  SMG_LAUNCH_CHECK();
  return 0;
}

// test entry of the candidate ranking sort (smg_wsort.hpp): one wave per array of keys
__global__ void __launch_bounds__(64) k_rank_sort_raw(const uint32_t *keys, const uint32_t *off, uint32_t narr, int nneed, int in_lds,
                                                      uint32_t *kv, uint32_t *out_key, uint32_t *out_idx) {
  __shared__ uint32_t sh[16 + WSORT_WORDS + 8192];
  uint32_t *wk = sh + 16, *arr = wk + WSORT_WORDS;
  for (uint32_t t = blockIdx.x; t < narr; t += gridDim.x) {
    const uint32_t o = off[t], n = off[t + 1] - o;
    uint32_t *a = (in_lds && n <= 8192) ? arr : kv + o;
    for (uint32_t i = threadIdx.x; i < n; i += 64) a[i] = (keys[o + i] << WSORT_IDXBITS) | i;
    __syncthreads();
    wave_sort_kv(a, (int)n, nneed < 0 ? (int)n : nneed, wk);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 64) { out_key[o + i] = a[i] >> WSORT_IDXBITS; out_idx[o + i] = a[i] & ((1u << WSORT_IDXBITS) - 1u); }
    __syncthreads();
  }
}

int launch_rank_sort_raw(hipStream_t s, const uint32_t *keys, const uint32_t *off, uint32_t narr, int nneed, int in_lds, uint32_t *kv,
                         uint32_t *out_key, uint32_t *out_idx) {
  if (!narr) return 0;
  hipLaunchKernelGGL(k_rank_sort_raw, dim3(narr < 4096 ? narr : 4096), dim3(64), 0, s, keys, off, narr, nneed, in_lds, kv, out_key, out_idx);
  SMG_LAUNCH_CHECK();
  return 0;
}

// test entry of the 64-bit key sorts (smg_exec.h): one wave per array, the array in LDS behind an LDS-typed pointer as in
// k_hits and k_cands (the host checks that every array fits the form: n <= 64 * E, n <= 1024)
__global__ void __launch_bounds__(64) k_sort_u64_raw(const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out) {
  __shared__ __align__(16) uint64_t sh[1024];
  typedef typename ptr_of<uint64_t, true>::type P64;
  P64 a = (P64)sh;
  for (uint32_t t = blockIdx.x; t < narr; t += gridDim.x) {
    const uint32_t o = off[t];
    uint32_t n = off[t + 1] - o;
    if (n > 1024u) n = 1024u;
    for (uint32_t i = threadIdx.x; i < n; i += 64) a[i] = keys[o + i];
    __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)      // (the register forms exist in the device pass only)
    if (form == 0) wave_sort_u64_reg<4>(a, n);
    else if (form == 1) wave_sort_u64_reg<8>(a, n);
    else if (form == 2) wave_sort_u64_reg<16>(a, n);
    else wave_sort_u64(a, n);
#endif
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 64) out[o + i] = a[i];
    __syncthreads();
  }
}

int launch_sort_u64_raw(hipStream_t s, const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out) {
  if (!narr) return 0;
  hipLaunchKernelGGL(k_sort_u64_raw, dim3(narr < 4096 ? narr : 4096), dim3(64), 0, s, keys, off, narr, form, out);
  SMG_LAUNCH_CHECK();
  return 0;
}

int launch_sw_full_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint8_t *r, const uint32_t *ro, uint32_t n,
                       const MapPar &p, int32_t *sc, uint32_t qmax_len, int packed16) {
  int G, C;
  if (!n) return 0;
  if (sw_full_geometry(qmax_len, &G, &C)) return -1;
  if (packed16 && !sw16_ok(p)) return -2;
  uint32_t grid = (n + (64 / G) - 1) / (64 / G);
  if (grid > 8192) grid = 8192;
  const bool known = sw_tiling_dispatch(G, C, [&](auto tile) {
    constexpr int TG = decltype(tile)::G, TC = decltype(tile)::C;
    if (packed16) hipLaunchKernelGGL((k_sw_full16_raw<TG, TC>), dim3(grid), dim3(64), 0, s, q, qo, r, ro, n, p, sc, sw16_frames_on());
    else hipLaunchKernelGGL((k_sw_full_raw<TG, TC>), dim3(grid), dim3(64), 0, s, q, qo, r, ro, n, p, sc);
  });
  if (!known) return (int)hipErrorInvalidValue;
  SMG_LAUNCH_CHECK();
  return 0;
}

}  // namespace smg

// smg_indexbuild.hip -- the k-mer index and the packed reference built in HBM.
//
// What the reference does on one host thread (hashTableSetUp, hashidx.c:829-998: count words, allocate, fill the
// position lists sequence by sequence; seqSetCompress, sequence.c:1360-1424) is here a stream compaction, one stable
// radix sort and two prefix sums over the sampled k-mers:
//   * k-mer serial t covers the bases [t*s, t*s + k) of the concatenated reference; it is indexed iff it lies inside
//     one sequence and holds no non-ACGT base (doWordsInSeq, hashidx.c:465-531: the sampling grid is global, serial
//     numbers run on across sequence boundaries; with s > k the reference refuses some sets of sequence lengths and counts
//     maxpos its own way -- index_carry of smg_indexbuild.h, run on the host in front of the kernels);
//   * PERFECT: key = the 2k-bit word; pos lists = serials sorted by (key, serial); idx = prefix sums of key counts;
//   * HASH32MIX (hashidx.c:155-172): key = hash32mix(word >> nbits_lo) % 2^(nbits_key - nbits_lo) << nbits_lo | low
//     bits; serials sorted by (key, word_hi, serial); one (wordidx, posidx) entry per distinct (key, word_hi); idx =
//     prefix sums of the number of distinct words per key.
// Serials are generated in ascending order and rocPRIM's radix sort is stable, so sorting by the key alone leaves the
// serials of equal keys ascending.  All of it is HBM-bound integer work: no LDS tiling to speak of, rocPRIM's device
// scan / sort do the passes.
#include <cstring>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include "smg_common.h"
#include "smg_indexbuild.h"

namespace smg {

// sequence.c:287-322: upper-case; U -> T; A C G T -> 0..3; everything else -> 5
__device__ inline uint8_t ref_code_of_ascii(uint8_t c) {
  c &= 0xDF;                                   // upper case (letters)
  return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : (c == 'T' || c == 'U') ? 3 : 5;
}

// letters [g0, g0 + span) of the reference as codes into LDS; beyond the end: `fill` (and 7 right at the end if term).
// Four letters per load when the source is word-aligned (g0 is a multiple of 4 for every caller).
__device__ inline void ib_stage_codes(uint8_t *cd, const uint8_t *ascii, uint64_t g0, uint32_t span, uint64_t tot, bool term, uint8_t fill) {
  if ((((uintptr_t)ascii + g0) & 3) == 0) {
    for (uint32_t i = threadIdx.x * 4; i < span; i += 256 * 4) {
      const uint64_t o = g0 + i;
      uint32_t w = 0;
      if (o + 4 <= tot) w = *(const uint32_t *)(ascii + o);
      else for (int u = 0; u < 4; u++) if (o + u < tot) w |= (uint32_t)ascii[o + u] << (8 * u);
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (i + u < span) cd[i + u] = o + u < tot ? ref_code_of_ascii((uint8_t)(w >> (8 * u))) : ((term && o + u == tot) ? 7 : fill);
    }
  } else {
    for (uint32_t i = threadIdx.x; i < span; i += 256) { const uint64_t o = g0 + i; cd[i] = o < tot ? ref_code_of_ascii(ascii[o]) : ((term && o == tot) ? 7 : fill); }
  }
}

// compressSeq (sequence.c:1360-1424): 10 codes per word, first base in the highest bits, terminator 7 after the last base.
// A block stages the 2560 letters of its 256 words through LDS (coalesced reads), then each thread packs one word.
__global__ void __launch_bounds__(256) k_ib_pack(const uint8_t *ascii, uint64_t tot, uint64_t nwords, uint32_t *packed) {
  __shared__ uint8_t cd[2560];
  for (uint64_t w0 = (uint64_t)blockIdx.x * 256; w0 < nwords; w0 += (uint64_t)gridDim.x * 256) {
    __syncthreads();
    ib_stage_codes(cd, ascii, w0 * 10, 2560, tot, true, 0);
    __syncthreads();
    const uint64_t w = w0 + threadIdx.x;
    if (w < nwords) {
      uint32_t v = 0;
      for (int i = 0; i < 10; i++) v |= (uint32_t)cd[threadIdx.x * 10 + i] << (3 * (9 - i));
      packed[w] = v;
    }
  }
}

__device__ inline uint32_t ib_hash32mix(uint32_t a) {        // hashidx.c:163-172
  a = (a + 0x7ed55d16) + (a << 12);
  a = (a ^ 0xc761c23c) ^ (a >> 19);
  a = (a + 0x165667b1) + (a << 5);
  a = (a + 0xd3a2646c) ^ (a << 9);
  a = (a + 0xfd7046c5) + (a << 3);
  a = (a ^ 0xb55a4f09) ^ (a >> 16);
  return a;
}

// one thread per k-mer serial.  K32 (PERFECT with 2k <= 30): 32-bit sort key, the sentinel 2^2k for serials that are not
// indexed (they sort behind every key), value = serial; the number of indexed serials goes to *nvalid.  Otherwise (HASH32MIX; a
// PERFECT index with 2k > 30 would be k = 16, which build_index_device refuses): validity flag and 64-bit sort key
// ((key << 32) | word_hi) for the compaction path.
template <bool K32>
__global__ void __launch_bounds__(256) k_ib_kmers(const uint8_t *ascii, const uint64_t *sop, int nseq, uint64_t ntup, int k, int s,
                                                  int nbits_key, int nbits_lo, uint32_t *flag, uint64_t *key64, uint32_t *key32, uint32_t *pos32,
                                                  unsigned long long *nvalid) {
  unsigned long long mine = 0;
  // the letters of the block's 256 serials go through LDS as codes (coalesced reads; a base is in k / s words)
  extern __shared__ uint8_t cd[];                      // 256 * s + k codes
  const uint32_t span = 256u * (uint32_t)s + (uint32_t)k;
  for (uint64_t t0 = (uint64_t)blockIdx.x * 256; t0 < ntup; t0 += (uint64_t)gridDim.x * 256) {
    const uint64_t g0 = t0 * (uint64_t)s, tot = sop[nseq];
    __syncthreads();
    ib_stage_codes(cd, ascii, g0, span, tot, false, 5);
    __syncthreads();
    const uint64_t t = t0 + threadIdx.x;
    if (t >= ntup) continue;
    const uint64_t g = t * (uint64_t)s;
    int lo = 0, hi = nseq;                       // sequence of base g: last i with sop[i] <= g
    {                                            // block-uniform search for the block's first base; nearly always the answer
      int ulo = 0, uhi = nseq;
      while (uhi - ulo > 1) { const int mid = (ulo + uhi) >> 1; if (sop[mid] <= g0) ulo = mid; else uhi = mid; }
      if (g < sop[ulo + 1]) { lo = ulo; hi = ulo + 1; } else lo = ulo;
    }
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (sop[mid] <= g) lo = mid; else hi = mid; }
    bool ok = g + (uint64_t)k <= sop[lo + 1];
    uint64_t word = 0;
    if (ok) {
      const uint8_t *c0 = cd + threadIdx.x * (uint32_t)s;
      for (int j = 0; j < k; j++) { const uint32_t c = c0[j]; if (c & 4) ok = false; word = (word << 2) | (c & 3); }
    }
    if (K32) {
      key32[t] = ok ? (uint32_t)word : (1u << (2 * k));
      pos32[t] = (uint32_t)t;
      mine += ok ? 1ull : 0ull;
    } else {
      uint64_t kv = 0;
      if (ok) {
        const uint64_t mask_lo = (1ull << nbits_lo) - 1ull;
        const uint32_t whi = (uint32_t)(word >> nbits_lo);
        const uint32_t keymod = 1u << (nbits_key - nbits_lo);
        const uint32_t key = ((ib_hash32mix(whi) % keymod) << nbits_lo) + (uint32_t)(word & mask_lo);
        kv = ((uint64_t)key << 32) | whi;
      }
      flag[t] = ok ? 1u : 0u;
      key64[t] = kv;
    }
  }
  if (K32) {
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(nvalid, mine);
  }
}

__global__ void __launch_bounds__(256) k_ib_scatter(const uint32_t *flag, const uint32_t *slot, const uint64_t *key64, uint64_t ntup, uint64_t *okey, uint32_t *opos) {
  for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < ntup; t += (uint64_t)gridDim.x * 256)
    if (flag[t]) { okey[slot[t]] = key64[t]; opos[slot[t]] = (uint32_t)t; }
}

// idx[key + 1] = number of sorted elements with a key <= key: written where a run of equal keys ends (no atomics;
// keys without elements keep 0 and are filled by the running maximum afterwards -- the sequence is non-decreasing)
__global__ void __launch_bounds__(256) k_ib_runend32(const uint32_t *skey, uint64_t n, uint32_t *idx) {
  for (uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x; a < n; a += (uint64_t)gridDim.x * 256)
    if (a + 1 == n || skey[a] != skey[a + 1]) idx[(uint64_t)skey[a] + 1] = (uint32_t)(a + 1);
}

// HASH32MIX: heads of runs of equal (key, word_hi)
__global__ void __launch_bounds__(256) k_ib_heads(const uint64_t *skey, uint64_t n, uint32_t *head) {
  for (uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x; a < n; a += (uint64_t)gridDim.x * 256) head[a] = (a == 0 || skey[a] != skey[a - 1]) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_ib_words(const uint64_t *skey, const uint32_t *head, const uint32_t *slot, uint64_t n, uint32_t *wordidx, uint32_t *posidx, uint32_t *idx) {
  for (uint64_t a = (uint64_t)blockIdx.x * 256 + threadIdx.x; a < n; a += (uint64_t)gridDim.x * 256) {
    if (head[a]) { wordidx[slot[a]] = (uint32_t)skey[a]; posidx[slot[a]] = (uint32_t)a; }
    const uint32_t key = (uint32_t)(skey[a] >> 32);
    if (a + 1 == n || key != (uint32_t)(skey[a + 1] >> 32)) idx[(uint64_t)key + 1] = slot[a] + head[a];   // distinct words with a key <= key
  }
}

static inline unsigned ib_grid(uint64_t n, unsigned cap) { uint64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g)); }

// SMALTGPU_INDEX_GRID=<1..65536> caps the workgroups of every launch of the construction.  It exists for the tests only: with
// the default of 65536 a kernel's grid-stride loop runs a second time only past 16.7 M serials or words, with a cap of 1 or 3
// it does so on a reference of a few kB.  Anything else is ignored.
static unsigned ib_grid_cap(const char *v) {
  if (!v || !*v) return 65536;
  char *end = nullptr;
  const long x = strtol(v, &end, 10);
  return (*end || x < 1 || x > 65536) ? 65536u : (unsigned)x;
}

// selectHashTyp (smalt.c:268-332)
int index_geometry(int k, int s, uint64_t totlen, int *typ, int *nbits_key, int *nbits_lo) {
  const int nbk = 2 * k;
  *typ = IDX_PERFECT; *nbits_key = nbk; *nbits_lo = 0;
  if (nbk > 63 || s < 1) return -1;
  const uint64_t ntup = totlen / (uint64_t)s, nkey = 1ull << nbk;
  if (ntup > 0xFFFFFFFFull) return -1;
  if (nkey > 2 * ntup) {
    int last_b = (ntup & 1) ? 1 : 0, nk, np = 0;
    uint32_t t = (uint32_t)ntup;
    for (int i = 0; i < 32; i++) { t >>= 1; if (t & 1) last_b = i; }
    nk = (last_b & 1) ? last_b + 1 : last_b;
    if (nbk > 32) { np = nbk - 32; if (np > 10) return -1; }
    if (nk + np > 26) nk = 26 - np;
    if (nk < np + 1) nk = np + 1;
    if (nk > 26) nk = 26;
    *typ = IDX_HASH32MIX; *nbits_key = nk; *nbits_lo = np;
  }
  return 0;
}

int build_index_device(const uint8_t *d_ascii, uint64_t tot, const uint64_t *h_sop, int nseq, int k, int s, BuiltIndex *out, char *err, size_t errlen) {
  BuiltIndex b;
  if (index_geometry(k, s, tot, &b.typ, &b.nbits_key, &b.nbits_lo) || b.nbits_key > 31 || nseq < 1 || s > 200) { snprintf(err, errlen, "unsupported index geometry (k=%d s=%d)", k, s); return -1; }
  for (int i = 0; i < nseq; i++) if (h_sop[i + 1] - h_sop[i] < (uint64_t)k) { snprintf(err, errlen, "sequence %d is shorter than the word length (hashidx.c:499)", i); return -1; }
  const int64_t bad = index_carry(h_sop, nseq, k, s, &b.maxpos);         // the reference's walk over the lengths: refusal and maxpos (hashidx.c:992)
  if (bad >= 0) {
    snprintf(err, errlen, "the reference refuses sampling step %d with word length %d for sequence %lld: the one in front of it ends too far before the next sampled word (hashidx.c:494)",
             s, k, (long long)bad);
    return -1;
  }
  const unsigned cap = ib_grid_cap(getenv("SMALTGPU_INDEX_GRID"));      // read once per build
  b.nkeys = 1u << b.nbits_key;
  const uint64_t ntup = (tot + (uint64_t)s - 1) / (uint64_t)s;           // serials 0 .. ntup-1 start inside the reference
  const uint64_t nwords = tot / 10 + 1;
  const bool k32 = b.typ == IDX_PERFECT && 2 * k <= 30;                  // 32-bit keys with a sentinel behind the largest word
  // scratch: it goes with this scope on every return, and so do the arrays of b until they are moved out
  DevMem<uint64_t> sop, key64, okey, skey; DevMem<uint32_t> flag, slot, opos, head, key32, skey32; DevMem<unsigned long long> nvalid; DevMem<char> tmp;
  DevEvent e0, e1;
  size_t need = 0;                                                     // bytes of temporary storage a rocPRIM call asks for
  uint64_t n = 0;                                                      // indexed serials
  // a rocPRIM call: once for the bytes of temporary storage it needs, once for the work
#define IB_TMP(call_null, call_real) { SMG_HIP(call_null); if (need > tmp.bytes()) SMG_HIP(tmp.alloc(need)); SMG_HIP(call_real); }
  SMG_HIP(e0.create()); SMG_HIP(e1.create());
  SMG_HIP(sop.alloc((size_t)nseq + 1));
  SMG_HIP(hipMemcpy(sop, h_sop, ((size_t)nseq + 1) * 8, hipMemcpyHostToDevice));
  SMG_HIP(b.packed.alloc(nwords));
  SMG_HIP(b.idx.alloc((size_t)b.nkeys + 2));
  SMG_HIP(nvalid.alloc(1));
  if (k32) {
    SMG_HIP(key32.alloc(ntup + 1)); SMG_HIP(skey32.alloc(ntup + 1));
    SMG_HIP(opos.alloc(ntup + 1)); SMG_HIP(b.pos.alloc(ntup + 1));
  } else {
    SMG_HIP(flag.alloc(ntup + 1)); SMG_HIP(slot.alloc(ntup + 1));
    SMG_HIP(key64.alloc(ntup + 1));
  }
  SMG_HIP(hipEventRecord(e0, 0));
  SMG_HIP(hipMemsetAsync(nvalid, 0, 8, 0));
  SMG_HIP(hipMemsetAsync(b.idx, 0, ((size_t)b.nkeys + 2) * 4, 0));
  hipLaunchKernelGGL(k_ib_pack, dim3(ib_grid(nwords, cap)), dim3(256), 0, 0, d_ascii, tot, nwords, b.packed.get());
  if (k32) {
    hipLaunchKernelGGL(k_ib_kmers<true>, dim3(ib_grid(ntup, cap)), dim3(256), (size_t)(256 * s + k + 16), 0, d_ascii, sop.get(), nseq, ntup, k, s, b.nbits_key, b.nbits_lo,
                       (uint32_t *)nullptr, (uint64_t *)nullptr, key32.get(), opos.get(), nvalid.get());
    SMG_HIP(hipGetLastError());
    // stable sort by key: serials of equal keys stay ascending, serials that are not indexed end up behind
    IB_TMP(rocprim::radix_sort_pairs(nullptr, need, key32.get(), skey32.get(), opos.get(), b.pos.get(), (size_t)ntup, 0u, (unsigned)(2 * k + 1), 0),
           rocprim::radix_sort_pairs(tmp.get(), need, key32.get(), skey32.get(), opos.get(), b.pos.get(), (size_t)ntup, 0u, (unsigned)(2 * k + 1), 0));
    unsigned long long h_nvalid = 0;
    SMG_HIP(hipMemcpy(&h_nvalid, nvalid, 8, hipMemcpyDeviceToHost));
    n = h_nvalid;
    b.npos = (uint32_t)n;
    hipLaunchKernelGGL(k_ib_runend32, dim3(ib_grid(n, cap)), dim3(256), 0, 0, skey32.get(), n, b.idx.get());
    SMG_HIP(hipGetLastError());
  } else {
    uint32_t last_slot = 0, last_flag = 0, lh = 0, ls = 0;
    hipLaunchKernelGGL(k_ib_kmers<false>, dim3(ib_grid(ntup, cap)), dim3(256), (size_t)(256 * s + k + 16), 0, d_ascii, sop.get(), nseq, ntup, k, s, b.nbits_key, b.nbits_lo,
                       flag.get(), key64.get(), (uint32_t *)nullptr, (uint32_t *)nullptr, nvalid.get());
    SMG_HIP(hipGetLastError());
    // ordered compaction of the indexed serials
    IB_TMP(rocprim::exclusive_scan(nullptr, need, flag.get(), slot.get(), 0u, (size_t)ntup, rocprim::plus<uint32_t>(), 0),
           rocprim::exclusive_scan(tmp.get(), need, flag.get(), slot.get(), 0u, (size_t)ntup, rocprim::plus<uint32_t>(), 0));
    if (ntup) {
      SMG_HIP(hipMemcpy(&last_slot, slot + (ntup - 1), 4, hipMemcpyDeviceToHost));
      SMG_HIP(hipMemcpy(&last_flag, flag + (ntup - 1), 4, hipMemcpyDeviceToHost));
    }
    n = (uint64_t)last_slot + last_flag;
    b.npos = (uint32_t)n;
    SMG_HIP(okey.alloc(n + 1)); SMG_HIP(skey.alloc(n + 2));
    SMG_HIP(opos.alloc(n + 1)); SMG_HIP(b.pos.alloc(n + 1));
    hipLaunchKernelGGL(k_ib_scatter, dim3(ib_grid(ntup, cap)), dim3(256), 0, 0, flag.get(), slot.get(), key64.get(), ntup, okey.get(), opos.get());
    SMG_HIP(hipGetLastError());
    const unsigned end_bit = (unsigned)(32 + b.nbits_key);
    IB_TMP(rocprim::radix_sort_pairs(nullptr, need, okey.get(), skey.get(), opos.get(), b.pos.get(), (size_t)n, 0u, end_bit, 0),
           rocprim::radix_sort_pairs(tmp.get(), need, okey.get(), skey.get(), opos.get(), b.pos.get(), (size_t)n, 0u, end_bit, 0));
    SMG_HIP(head.alloc(n + 1));
    hipLaunchKernelGGL(k_ib_heads, dim3(ib_grid(n, cap)), dim3(256), 0, 0, skey.get(), n, head.get());
    SMG_HIP(hipGetLastError());
    IB_TMP(rocprim::exclusive_scan(nullptr, need, head.get(), slot.get(), 0u, (size_t)n, rocprim::plus<uint32_t>(), 0),
           rocprim::exclusive_scan(tmp.get(), need, head.get(), slot.get(), 0u, (size_t)n, rocprim::plus<uint32_t>(), 0));
    if (n) {
      SMG_HIP(hipMemcpy(&ls, slot + (n - 1), 4, hipMemcpyDeviceToHost));
      SMG_HIP(hipMemcpy(&lh, head + (n - 1), 4, hipMemcpyDeviceToHost));
    }
    b.nwords = ls + lh;
    SMG_HIP(b.wordidx.alloc((size_t)b.nwords + 2)); SMG_HIP(b.posidx.alloc((size_t)b.nwords + 2));
    SMG_HIP(hipMemsetAsync(b.wordidx, 0, ((size_t)b.nwords + 2) * 4, 0)); SMG_HIP(hipMemsetAsync(b.posidx, 0, ((size_t)b.nwords + 2) * 4, 0));
    hipLaunchKernelGGL(k_ib_words, dim3(ib_grid(n, cap)), dim3(256), 0, 0, skey.get(), head.get(), slot.get(), n, b.wordidx.get(), b.posidx.get(), b.idx.get());
    SMG_HIP(hipGetLastError());
    SMG_HIP(hipMemcpyAsync(b.posidx + b.nwords, &b.npos, 4, hipMemcpyHostToDevice, 0));       // posidx[nwords] = npos
  }
  // run ends -> prefix sums: keys without elements take the count of their predecessor (running maximum)
  IB_TMP(rocprim::inclusive_scan(nullptr, need, b.idx.get(), b.idx.get(), (size_t)b.nkeys + 1, rocprim::maximum<uint32_t>(), 0),
         rocprim::inclusive_scan(tmp.get(), need, b.idx.get(), b.idx.get(), (size_t)b.nkeys + 1, rocprim::maximum<uint32_t>(), 0));
  SMG_HIP(hipEventRecord(e1, 0));
  SMG_HIP(hipEventSynchronize(e1));
  SMG_HIP(hipEventElapsedTime(&b.build_ms, e0, e1));
#undef IB_TMP
  *out = std::move(b);
  return 0;
}

}  // namespace smg

// smg_exec.h -- the execution model the per-read stage functions are written against.
//
// A read (or read-strand) is owned by ONE 64-lane wavefront (a 64-thread workgroup).  Stage
// code is written once with the macros below:
//   SMG_PAR_CHUNKS(base, n)  wave-uniform loop over chunks of SMG_NLANES items; inside, the
//                            item of this lane is  base + SMG_LANE  (may be >= n)
//   SMG_LANE0                the sequential sections (one lane; the reference's order matters)
//   SMG_SYNC()               workgroup barrier + memory visibility between the two
// On the device SMG_NLANES = 64.  The same source also compiles for the host with
// SMG_NLANES = 1 (tests/hostemu): that build exists to unit-test this logic on a machine
// without a GPU and is never part of libsmaltgpu.so.
//
// Below the macros: the wave primitives (compaction, sums, minima and maxima, ballot, the add scan and the running maximum),
// each one function with its device and host form inside, so that stage code holds no #if; then the sort of 64-bit keys
// (one network over memory, one over registers, the forms built from them and wave_sort_keys, which picks a form).
#pragma once
#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define SMG_LANE ((uint32_t)threadIdx.x)
#define SMG_NLANES 64u
#define SMG_SYNC() __syncthreads()
#else
#define SMG_LANE 0u
#define SMG_NLANES 1u
#define SMG_SYNC() do {} while (0)
#endif

// Pointers that are known to address the workgroup's LDS block carry the LDS address space on the device, so that
// the compiler emits ds_* instructions (32-bit addresses) instead of flat ones; plain pointers on the host build.
#if defined(__HIP_DEVICE_COMPILE__)
#define SMG_LDSQ __attribute__((address_space(3)))
#else
#define SMG_LDSQ
#endif
namespace smg {
template <class T, bool IN_LDS> struct ptr_of { typedef T *type; };
template <class T> struct ptr_of<T, true> { typedef SMG_LDSQ T *type; };
}

#define SMG_PAR_CHUNKS(base, n) for (uint32_t base = 0; base < (uint32_t)(n); base += SMG_NLANES)
#define SMG_LANE0 if (SMG_LANE == 0)

namespace smg {

// phase clock for the diagnostic counters (shader clock on the device, nothing on the host)
SMG_HD inline unsigned long long phase_clock() {
#if defined(__HIP_DEVICE_COMPILE__)
  return (unsigned long long)__builtin_readcyclecounter();
#else
  return 0;
#endif
}

// Ordered stream compaction: lanes with flag get consecutive slots in lane order.
// `counter` is wave-uniform.
SMG_HD inline uint32_t compact_slot(bool flag, uint32_t &counter) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned long long m = __ballot(flag);
  uint32_t slot = counter + (uint32_t)__popcll(m & ((1ull << SMG_LANE) - 1ull));
  counter += (uint32_t)__popcll(m);
  return slot;
#else
  uint32_t slot = counter;
  if (flag) counter++;
  return slot;
#endif
}

SMG_HD inline uint32_t wave_sum_u32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
#else
  return v;
#endif
}

SMG_HD inline uint32_t wave_max_u32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int o = 32; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o); if (u > v) v = u; }
#endif
  return v;
}

SMG_HD inline uint32_t wave_min_u32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int o = 32; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o); if (u < v) v = u; }
#endif
  return v;
}

SMG_HD inline uint64_t wave_min_u64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
    const uint64_t u = ((uint64_t)hi << 32) | lo;
    if (u < v) v = u;
  }
#endif
  return v;
}

SMG_HD inline bool wave_any(bool f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(f) != 0ull;
#else
  return f;
#endif
}

// one bit per lane (the host build's one lane is bit 0)
SMG_HD inline unsigned long long wave_ballot(bool f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(f);
#else
  return f ? 1ull : 0ull;
#endif
}

// Add scan over the lanes, continued from the wave-uniform running `total` (the sum of everything before lane 0): returns the
// lane's exclusive prefix, total included, and advances the total by the wave's sum.  The inclusive prefix is the result + v.
SMG_HD inline uint32_t wave_scan_add_u32(uint32_t v, uint32_t &total) {
  uint32_t incl = v;
#if defined(__HIP_DEVICE_COMPILE__)
  for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)incl, o); if ((int)SMG_LANE >= o) incl += u; }
#endif
  const uint32_t excl = total + incl - v;
#if defined(__HIP_DEVICE_COMPILE__)
  total += (uint32_t)__shfl((int)incl, 63);
#else
  total += incl;
#endif
  return excl;
}

// inclusive running maximum over the lanes, continued from `carry` (the maximum of everything before lane 0); returns the
// lane's value, *carry_out = the wave's maximum (wave-uniform)
SMG_HD inline uint32_t wave_scan_max_u32(uint32_t v, uint32_t carry, uint32_t *carry_out) {
#if defined(__HIP_DEVICE_COMPILE__)
  int x = (int)v;                                  // values are small non-negative numbers: 0 is the identity
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x111 /* row_shr:1 */, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x112 /* row_shr:2 */, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x114 /* row_shr:4 */, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x118 /* row_shr:8 */, 0xf, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x142 /* row_bcast:15 */, 0xa, 0xf, false));
  x = max(x, __builtin_amdgcn_update_dpp(0, x, 0x143 /* row_bcast:31 */, 0xc, 0xf, false));
  x = max(x, (int)carry);
  *carry_out = (uint32_t)__builtin_amdgcn_readlane(x, 63);
  return (uint32_t)x;
#else
  const uint32_t r = v > carry ? v : carry;
  *carry_out = r;
  return r;
#endif
}

SMG_HD inline uint32_t bcast_lane0(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
  return v;
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// Ascending sort of 64-bit keys by the whole wave: ONE bitonic network in its normalised form (every comparator puts the
// smaller key at the lower index: the first step of a merge pairs i with its mirror image in the block of k, the others pair
// i with i + j), written once over memory (sort_mirror_mem, sort_halfclean_mem) and once over registers (sort_network_reg).
// Keys beyond n are virtual +inf: a comparator that touches one never swaps, so no padding is stored and only comparators
// below n are visited.  The forms put the two together:
//   wave_sort_u64          every step in memory (LDS or HBM, by the pointer type)
//   wave_sort_u64_reg<E>   up to 64 * E keys, the whole network in registers
//   wave_sort_u64_chunked  runs in HBM: chunks of 1024 keys in registers, the steps that span chunks in memory
//   wave_sort_keys         which of them a stage takes for n keys
// Neither memory step ends with a barrier: the callers differ in what they need there.

// One step over memory.  Each lane loads the operands of up to four comparators before it stores any: the step is bound by the
// memory's latency, and four independent round trips overlap.
template <class P>
SMG_HD inline void sort_mirror_mem(P a, uint32_t n, uint32_t k) {          // first step of the merge into blocks of k
  const uint32_t h = k >> 1;
  const uint32_t tmax = (n / k) * h + ((n % k) < h ? (n % k) : h);
  for (uint32_t t0 = 0; t0 < tmax; t0 += 4 * SMG_NLANES) {
    uint32_t ii[4], pp[4];
    uint64_t x[4], y[4];
    bool on[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t t = t0 + (uint32_t)u * SMG_NLANES + SMG_LANE;
      const uint32_t blk = t / h, off = t % h;
      ii[u] = blk * k + off; pp[u] = blk * k + (k - 1 - off);
      on[u] = t < tmax && pp[u] < n;
      if (on[u]) { x[u] = a[ii[u]]; y[u] = a[pp[u]]; }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) if (on[u] && x[u] > y[u]) { a[ii[u]] = y[u]; a[pp[u]] = x[u]; }
  }
}
template <class P>
SMG_HD inline void sort_halfclean_mem(P a, uint32_t n, uint32_t j) {       // half-cleaner: i with i + j
  const uint32_t tmax = (n / (2 * j)) * j + ((n % (2 * j)) < j ? (n % (2 * j)) : j);
  for (uint32_t t0 = 0; t0 < tmax; t0 += 4 * SMG_NLANES) {
    uint32_t ii[4];
    uint64_t x[4], y[4];
    bool on[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint32_t t = t0 + (uint32_t)u * SMG_NLANES + SMG_LANE;
      ii[u] = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      on[u] = t < tmax && (ii[u] | j) < n;
      if (on[u]) { x[u] = a[ii[u]]; y[u] = a[ii[u] | j]; }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) if (on[u] && x[u] > y[u]) { a[ii[u]] = y[u]; a[ii[u] | j] = x[u]; }
  }
}

// In place, n keys, every step in memory.
template <class P>
SMG_HD inline void wave_sort_u64(P a, uint32_t n) {
  if (n < 2) return;
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t np = 1;
  while (np < n) np <<= 1;
  for (uint32_t k = 2; k <= np; k <<= 1) {
    sort_mirror_mem(a, n, k);
    SMG_SYNC();
    for (uint32_t j = k >> 2; j > 0; j >>= 1) { sort_halfclean_mem(a, n, j); SMG_SYNC(); }
  }
#else
  // host build: any correct sort gives the same array (keys are plain integers)
  std::sort((uint64_t *)a, (uint64_t *)a + n);
#endif
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline uint64_t shfl_xor_u64(uint64_t v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
  return ((uint64_t)hi << 32) | lo;
}
// One side of a comparator whose two keys sit in two lanes: v is the lane's own key, o the partner's; the lower lane keeps the
// smaller key, the upper lane the larger one.  One 64-bit compare, turned round on the upper side: take = (o < v) != upper.
// That differs from "o < v below, o > v above" only where o == v, and there taking o or keeping v leaves the same bits in the
// register, so it is the same network; the ~0 padding beyond n is just another equal key (a real key ~0 beside it included).
// Written with two compares and a choice between them, the compiler turns both conditions into 0/1 values, selects one, masks
// and compares again: nine vector instructions per exchange.  This form is one v_cmp_lt_u64, one s_xor_b64 with the step's lane
// mask (scalar unit) and the two selects of the key's halves (profiles/hits_sort_exchange_static.txt).
__device__ inline uint64_t keep_side_u64(uint64_t v, uint64_t o, bool upper) { return ((o < v) != upper) ? o : v; }
// compare-exchange between two registers of one lane
__device__ inline void order_u64(uint64_t &lo, uint64_t &hi) { const uint64_t x = lo, y = hi; const bool sw = x > y; lo = sw ? y : x; hi = sw ? x : y; }

// The whole network over 64 * E keys in registers.  Lane l holds the logical elements E * l .. E * l + E - 1 (which unsorted
// key starts where is free, so the callers' loads are coalesced); comparators whose span stays below E are compare-exchanges
// between a lane's own registers, the others pair register r of a lane with register r (mirror step: E - 1 - r) of the lane
// at distance span / E and keep the smaller or the larger key by side.  34 of the 55 steps of a 1024-key sort touch neither
// memory nor another lane.
template <int E>
__device__ inline void sort_network_reg(uint64_t (&v)[E], uint32_t lane) {
#pragma unroll
  for (int k = 2; k <= 64 * E; k <<= 1) {
    if (k <= E) {                                      // mirror step inside the lane
#pragma unroll
      for (int r = 0; r < E; r++) { const int q = r ^ (k - 1); if (r < q) order_u64(v[r], v[q]); }
    } else {                                           // mirror step across lanes
      const int m = k / E - 1;
      const bool upper = (lane & (uint32_t)(k / (2 * E))) != 0;
      uint64_t pv[E];
#pragma unroll
      for (int r = 0; r < E; r++) pv[r] = shfl_xor_u64(v[E - 1 - r], m);
#pragma unroll
      for (int r = 0; r < E; r++) { v[r] = keep_side_u64(v[r], pv[r], upper); }
    }
#pragma unroll
    for (int j = k / 4; j >= 1; j >>= 1) {
      if (j < E) {
#pragma unroll
        for (int r = 0; r < E; r++) { if (!(r & j)) order_u64(v[r], v[r | j]); }
      } else {
        const int m = j / E;
        const bool upper = (lane & (uint32_t)m) != 0;
#pragma unroll
        for (int r = 0; r < E; r++) { v[r] = keep_side_u64(v[r], shfl_xor_u64(v[r], m), upper); }
      }
    }
  }
}

// In place, at most 64 * E keys (in LDS, or a short run in HBM): coalesced load, the network, store in order.
// Not inlined, which is what the compiler chose for every caller anyway: said here, it no longer depends on how the call is
// wrapped (behind wave_sort_keys the short HBM form went inline into k_cands and the tightest instance spilled more).
template <int E, class P>
__device__ __noinline__ void wave_sort_u64_reg(P a, uint32_t n) {
  if (n < 2) return;
  const uint32_t lane = threadIdx.x;
  uint64_t v[E];
#pragma unroll
  for (int r = 0; r < E; r++) { const uint32_t idx = (uint32_t)r * 64u + lane; v[r] = idx < n ? a[idx] : ~0ull; }
  sort_network_reg<E>(v, lane);
  __syncthreads();
#pragma unroll
  for (int r = 0; r < E; r++) { const uint32_t i = (uint32_t)E * lane + (uint32_t)r; if (i < n) a[i] = v[r]; }
  __syncthreads();
}

// Runs of more than 1024 keys in HBM (the exhaustive search: every seed of a strand in a repeat): wave_sort_u64 over global
// memory pays a round trip per stage -- 105 of them for 16 384 keys.  Here every chunk of 1024 keys is sorted in registers, and of
// the later merges only the comparators that span chunks run in memory (the mirror step and the half-cleaners with j >= 1024);
// the rest of each merge, j = 512 .. 1, stays inside a chunk and runs in registers again: about ten passes over the memory
// and five register passes per chunk for 16 384 keys.  Same network, same +inf convention for the keys beyond n.
// MERGE = false: the chunk's keys in any order -> sorted (the full network; loads in the order that coalesces, lane l ends up
// with the logical elements 16 l .. 16 l + 15).  MERGE = true: only the half-cleaners j = 512 .. 1 of a larger merge; here register
// r of lane l holds element 64 r + l, so that loads and stores coalesce: j >= 64 pairs registers of one lane, j < 64 lanes.
template <bool MERGE, class P>
__device__ inline void sort_chunk_1024(P a, uint32_t base, uint32_t n) {
  constexpr int E = 16;
  const uint32_t lane = threadIdx.x;
  uint64_t v[E];
#pragma unroll
  for (int r = 0; r < E; r++) { const uint32_t idx = base + (uint32_t)r * 64u + lane; v[r] = idx < n ? a[idx] : ~0ull; }
  if (MERGE) {
#pragma unroll
    for (int j = 512; j >= 64; j >>= 1) {
#pragma unroll
      for (int r = 0; r < E; r++) { if (!(r & (j / 64))) order_u64(v[r], v[r | (j / 64)]); }
    }
#pragma unroll
    for (int j = 32; j >= 1; j >>= 1) {
      const bool upper = (lane & (uint32_t)j) != 0;
#pragma unroll
      for (int r = 0; r < E; r++) { v[r] = keep_side_u64(v[r], shfl_xor_u64(v[r], j), upper); }
    }
#pragma unroll
    for (int r = 0; r < E; r++) { const uint32_t idx = base + (uint32_t)r * 64u + lane; if (idx < n) a[idx] = v[r]; }
    return;
  }
  sort_network_reg<E>(v, lane);
#pragma unroll
  for (int r = 0; r < E; r++) { const uint32_t idx = base + (uint32_t)E * lane + (uint32_t)r; if (idx < n) a[idx] = v[r]; }
}

// (not inlined: one function, fitted to all its callers -- see smg_sortraw.hip)
template <class P>
__device__ __noinline__ void wave_sort_u64_chunked(P a, uint32_t n) {
  constexpr uint32_t C = 1024;
  for (uint32_t base = 0; base < n; base += C) sort_chunk_1024<false>(a, base, n);
  __threadfence_block();
  __syncthreads();
  uint32_t np = C;
  while (np < n) np <<= 1;
  for (uint32_t k = 2 * C; k <= np; k <<= 1) {
    sort_mirror_mem(a, n, k);
    __threadfence_block();
    __syncthreads();
    for (uint32_t j = k >> 2; j >= C; j >>= 1) {                // half-cleaners that span chunks
      sort_halfclean_mem(a, n, j);
      __threadfence_block();
      __syncthreads();
    }
    for (uint32_t base = 0; base < n; base += C) sort_chunk_1024<true>(a, base, n);      // j = 512 .. 1 inside the chunks
    __threadfence_block();
    __syncthreads();
  }
}
#endif

// The form a stage takes for n unsorted keys.  Up to 256 keys go to registers wherever they lie (the few hits of a restricted
// call in the HBM working set: ten round trips to HBM with the network in memory); beyond that the LDS arrays take the wider
// register forms up to 1024 keys and the network in LDS above, and only the HBM working set (HBM = true: longer runs of the
// exhaustive search) takes the chunked sort.  P keeps the array's address space, so LDS arrays are sorted with ds_* code.
template <bool HBM, class P>
SMG_HD inline void wave_sort_keys(P a, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (n <= 1024 && (!HBM || n <= 256)) {
    if (n <= 256) wave_sort_u64_reg<4>(a, n);
    else if (n <= 512) wave_sort_u64_reg<8>(a, n);
    else wave_sort_u64_reg<16>(a, n);
  } else if (HBM) wave_sort_u64_chunked(a, n);
  else wave_sort_u64(a, n);
#else
  wave_sort_u64(a, n);
#endif
}

}  // namespace smg

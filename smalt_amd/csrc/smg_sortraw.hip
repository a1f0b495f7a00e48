// smg_sortraw.hip -- stand-alone entry of the 64-bit key sorts of the HBM working set (parity tests): wave_sort_u64 and
// wave_sort_u64_chunked (smg_exec.h) in place on global memory, behind the pointer type StrandWork<uint32_t>::dat has in k_cands.
// A translation unit of its own on purpose.  wave_sort_u64_chunked is not inlined; a kernel beside k_cands in smg_kernels.hip
// that calls it shares the one function with k_cands, and the function is then compiled for all its callers together (register
// budget, what is known of its arguments): the VGPR, spill and scratch figures of four k_cands instances moved when the forms
// were tried inside k_sort_u64_raw.  Here the sorts are the same source under the same compiler and nothing in smg_kernels.hip
// changes.
#include <hip/hip_runtime.h>
#include "smg_kernels.h"
#include "smg_exec.h"
#include "smg_stages.hpp"

namespace smg {

// one wave per array: array t is copied to out[off[t] .. off[t + 1]) and sorted there; nothing past off[t + 1] is touched.
// Three waves per SIMD as in the tightest k_cands instance: the register budget under which k_cands' copy of the function is compiled.
__global__ void __launch_bounds__(64, 3) k_sort_u64_hbm_raw(const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out) {
  for (uint32_t t = blockIdx.x; t < narr; t += gridDim.x) {
    const uint32_t o = off[t], n = off[t + 1] - o;
    typename ptr_of<uint64_t, false>::type a = out + o;
    for (uint32_t i = threadIdx.x; i < n; i += 64) a[i] = keys[o + i];
    __threadfence_block();
    __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)
    if (form == 4) wave_sort_u64(a, n);
    else wave_sort_u64_chunked(a, n);
#endif
    __syncthreads();
  }
}

int launch_sort_u64_hbm_raw(hipStream_t s, const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out) {
  if (!narr) return 0;
  if (form != 4 && form != 5) return -1;
  hipLaunchKernelGGL(k_sort_u64_hbm_raw, dim3(narr < 4096 ? narr : 4096), dim3(64), 0, s, keys, off, narr, form, out);
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? (int)e : 0;
}

// The seed ranking's instance of the wave sort (stage_seed, wave form): elements packed (key << SEED_IDXBITS) | i in LDS, the
// work words sized as the stage's (SEED_WSORT_WORDS).  With SEED_LISTCAP = 32 short ranges the list of short ranges is flushed in
// the middle of the recursion; the default instance of the candidate ranking (k_rank_sort_raw) never gets there on such arrays.
// The host has checked n < 2^SEED_IDXBITS and keys < 2^(32 - SEED_IDXBITS).
__global__ void __launch_bounds__(64) k_seed_sort_raw(const uint32_t *keys, const uint32_t *off, uint32_t narr, uint32_t *out_key, uint32_t *out_idx) {
  __shared__ uint32_t sh[16 + SEED_WSORT_WORDS + (1 << SEED_IDXBITS)];
  uint32_t *wk = sh + 16, *a = wk + SEED_WSORT_WORDS;
  for (uint32_t t = blockIdx.x; t < narr; t += gridDim.x) {
    const uint32_t o = off[t];
    uint32_t n = off[t + 1] - o;
    if (n > (1u << SEED_IDXBITS) - 1u) n = (1u << SEED_IDXBITS) - 1u;
    for (uint32_t i = threadIdx.x; i < n; i += 64) a[i] = (keys[o + i] << SEED_IDXBITS) | i;
    __syncthreads();
    wave_sort_kv<SEED_IDXBITS, SEED_LISTCAP, SEED_LSTK>(a, (int)n, (int)n, wk);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += 64) { out_key[o + i] = a[i] >> SEED_IDXBITS; out_idx[o + i] = a[i] & ((1u << SEED_IDXBITS) - 1u); }
    __syncthreads();
  }
}

int launch_seed_sort_raw(hipStream_t s, const uint32_t *keys, const uint32_t *off, uint32_t narr, uint32_t *out_key, uint32_t *out_idx) {
  if (!narr) return 0;
  hipLaunchKernelGGL(k_seed_sort_raw, dim3(narr < 4096 ? narr : 4096), dim3(64), 0, s, keys, off, narr, out_key, out_idx);
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? (int)e : 0;
}

}  // namespace smg

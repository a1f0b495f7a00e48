// smg_kernels.h -- host-callable launchers of the gfx950 kernels (smg_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include "smg_cands.hpp"
#include "smg_bandnode.h"

namespace smg {

enum : int { SW_FULL_WMAX = 1016,   // longest reference window of the register-tiled K2a kernels
             SW_SHORT_WMAX = 248 };  // windows up to here take the small-LDS instance of the packed kernel (more resident waves)

int launch_encode(hipStream_t s, const uint8_t *bases, const uint64_t *off, uint32_t n, uint8_t *codes, uint8_t *codes_rc);
int launch_gather_reads(hipStream_t s, uint8_t *dst_bases, uint8_t *dst_quals, const uint64_t *dst_off, uint32_t n, const uint32_t *ids,
                        const uint8_t *const src_bases[2], const uint8_t *const src_quals[2], const uint64_t *const src_off[2]);
// needs b.iv_off/iv, b.fine_idx/fine_pos/fine_off; grid: workgroups (test hook), 0 = one per read up to 65535
int launch_fine_index(hipStream_t s, const Batch &b, const DevIndex &ix, uint32_t grid = 0);
inline uint32_t fine_index_grid(uint32_t nreads, uint32_t grid) { const uint32_t g = grid && grid < 65535u ? grid : 65535u; return nreads < g ? nreads : g; }
// force_hbm: scratch in the HBM slots even where it would fit LDS; grid_fixed: that many workgroups, 0 = the launcher's own choice
// (test hooks of smaltgpu_seed_batch; an HBM launch of more workgroups than slots is refused)
int launch_seed(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint8_t *scratch, size_t sbytes, uint32_t nslots, int force_hbm = 0,
                uint32_t grid_fixed = 0);
struct CandGeom {              // scratch geometry of the candidate stage (both code paths share one HBM slot)
  uint32_t hcap;               // hits of both strands, power of two (sequential path)
  uint32_t hcap_strand;        // hits of one strand (wave-parallel path)
  uint32_t ngrp, segcap, candcap;
  size_t slot_bytes;
  int debug;                   // keep per-read slots + the grouped hit words for smaltgpu_dump_read
  uint32_t window;             // test hook: hits per LDS window of the candidate stage (0 = default)
  uint32_t lds_hits, tab;      // LDS block of the candidate stage: hits of the working set, per-list table entries
  int pass;                    // 0: only pass; 1: first of two (a read that overflows its slot is deferred); 2: second pass over full-size slots
};
inline size_t cand_slot_bytes(const CandGeom &g, uint32_t qmax, int s) {
  size_t a = cand_scratch_bytes(qmax, s, g.hcap, g.ngrp, g.segcap, g.candcap);
  size_t b = cands_v2_hbm_bytes(qmax, s, g.hcap_strand, g.ngrp, g.candcap, true);
  return a > b ? a : b;
}
// LDS working set of the candidate stage when S3 runs inside it (k_cands<false>, k_cands<true>): hits and per-list tables
inline uint32_t cands_lds_bytes(const CandGeom &g) { return (uint32_t)(((strand_work_bytes<uint16_t>(g.lds_hits) + 15) & ~(size_t)15) + (size_t)5 * g.tab * 4); }
int launch_hits(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint32_t W, uint32_t tab, uint32_t nwg, uint32_t fill);
int launch_cands(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint8_t *scratch, uint32_t nslots, const CandGeom &g);
int launch_replay(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p);
// cplx: table of logarithms and lambda; needed (and read) only when p.flags has FLG_CMPLXW
int launch_align(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint8_t *scratch, size_t sbytes, uint32_t nslots,
                 uint32_t wincap, uint64_t dircap, uint32_t rescap, uint32_t dstrcap, int pass, const CplxPar *cplx = nullptr);
int sw_full_geometry(uint32_t qmax_len, int *G, int *C);
int launch_sw_full(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, uint32_t qmax_len, uint32_t ntask_cap, uint32_t grid);
int launch_sw_strip(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid);
int launch_sw_strip_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint8_t *r, const uint32_t *ro, uint32_t n, const MapPar &p,
                        int32_t *sc, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid);
// stand-alone packed strip kernel (pairs of tasks); -2: penalties or the longest read's score beyond its 16-bit halves
int launch_sw_strip16_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint8_t *r, const uint32_t *ro, uint32_t n, const MapPar &p,
                          int32_t *sc, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid, uint32_t qmax_len);
// stand-alone K2b: band = n x {band_l, band_r, qs, qe}, windows in the index's packed layout at the base offsets ro;
// band_fast_wave (one wave per task) and band_fast_scalar (one lane per task, rows: n x 2 x rowlen ints)
int launch_sw_band_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint32_t *packed, const uint32_t *ro, uint32_t n,
                       const MapPar &p, const int32_t *band, int32_t *sc, void *bnd, uint8_t *win, uint32_t wcap, uint32_t grid);
int launch_sw_band_scalar_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint32_t *packed, const uint32_t *ro, uint32_t n,
                              const MapPar &p, const int32_t *band, int32_t *sc, int *rows, uint32_t rowlen);
// stand-alone K3 nodes, one wave per task in the form a.form (smg_bandnode.hip); the caller has checked the form's precondition
int launch_band_nodes(hipStream_t s, const BandNodeArgs &a, const MapPar &p);
int launch_sw_scalar(hipStream_t s, const Batch &b, const DevIndex &ix, const MapPar &p, int *rows, uint32_t rowlen, uint32_t nthreads,
                     uint32_t qmax_len);
int launch_sw_full_raw(hipStream_t s, const uint8_t *q, const uint32_t *qo, const uint8_t *r, const uint32_t *ro, uint32_t n,
                       const MapPar &p, int32_t *sc, uint32_t qmax_len, int packed16);
// longest sweep (window rows + G - 1) that the packed K2a kernel runs in its row-frame form for these penalties and this
// many tile columns (G * C); -1: none
int sw16_rowframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols);
// the same for its pair-frame form, which goes first
int sw16_pairframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols);
int launch_rank_sort_raw(hipStream_t s, const uint32_t *keys, const uint32_t *off, uint32_t narr, int nneed, int in_lds, uint32_t *kv,
                         uint32_t *out_key, uint32_t *out_idx);
// test entry of the 64-bit key sorts: form 0/1/2 = wave_sort_u64_reg<4|8|16>, 3 = wave_sort_u64; every array at most 1024 keys (in LDS)
int launch_sort_u64_raw(hipStream_t s, const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out);
// ... and of the sorts of the HBM working set, in place on global memory (in `out`), any length: form 4 = wave_sort_u64,
// 5 = wave_sort_u64_chunked (smg_sortraw.hip: a translation unit of its own, see there)
int launch_sort_u64_hbm_raw(hipStream_t s, const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out);
// test entry of the seed ranking's instance of the wave sort, wave_sort_kv<SEED_IDXBITS, SEED_LISTCAP, SEED_LSTK> in LDS as in
// stage_seed: arrays of fewer than 4096 keys below 2^20 (smg_sortraw.hip)
int launch_seed_sort_raw(hipStream_t s, const uint32_t *keys, const uint32_t *off, uint32_t narr, uint32_t *out_key, uint32_t *out_idx);

}  // namespace smg

// smg_bandnode.h -- one node of the K3 recursion in one named form of the band pass (smaltgpu_band_align_nodes, parity
// tests): the forms, the host rules that go with them, and the arguments of its launcher (smg_kernels.h).  Host rules only: builds with a plain C++ compiler.
#pragma once
#include "smg_stages.hpp"

namespace smg {

enum : int { BF_ROWS = 0, BF_ANTIDIAG = 1, BF_WAVE2 = 2, BF_WAVE4 = 3, BF_WAVE7 = 4, BF_WAVE12 = 5, BF_STRIP8 = 6, BF_STRIP16 = 7,
             BF_SCALAR = 8, BF_NFORMS = 9 };      // = SMALTGPU_BAND_*
enum : int { NODE_ALIGNED = 0, NODE_REFUSED = 1, NODE_BELOW = 2 };
enum : uint32_t { NODE_LDS_CODES = 4096,          // lds = 1: longest read and window staged in LDS
                  NODE_LDS_DIR = 16384 };         // ... and the largest direction matrix kept there

struct BandNodeOut { int32_t status, score, max_i, max_j, qs, rs, dlen; uint32_t stroffs; };      // = smaltgpu_band_node

SMG_HD inline int band_nslot(const Band &b) { return b.band_width >= 1 ? (b.r_edge - b.l_edge) / 128 + 1 : 0; }   // live columns per lane of the wave forms

// bytes per anti-diagonal step of the wave forms' HBM layout: a power of two >= band_width / 2 + 2 (stage_align)
SMG_HD inline int band_tw(const Band &b) {
  int w = 64;
  while (w < b.band_width / 2 + 2) w <<= 1;
  return w;
}

// whether `form` may run this (accepted) band; gi, ge: the positive gap penalties
SMG_HD inline bool band_form_ok(int form, const Band &b, int gi, int ge) {
  const int bw = b.band_width;
  switch (form) {
    case BF_ROWS: return bw >= 1 && bw <= 64 && gi >= ge && ge >= 0;
    case BF_ANTIDIAG: return bw >= 1 && bw <= 64;
    case BF_WAVE2: return bw >= 1 && band_nslot(b) <= 2;
    case BF_WAVE4: return bw >= 1 && band_nslot(b) <= 4;
    case BF_WAVE7: return bw >= 1 && band_nslot(b) <= 7;
    case BF_WAVE12: return bw >= 1 && band_nslot(b) <= 12;
    case BF_STRIP8: return bw >= 256 && bw < 2048;
    case BF_STRIP16: return bw >= 2048;
    case BF_SCALAR: return true;
  }
  return false;
}

// the form k_align<true> picks (rows form on, direction matrix in HBM with room for every layout, hand-over rows that fit)
SMG_HD inline int band_form_production(const Band &b, int gi, int ge) {
  const int bw = b.band_width;
  if (bw >= 256 && strip_geom(b, bw < 2048 ? 3 : 4).nstrip > 0) return bw < 2048 ? BF_STRIP8 : BF_STRIP16;
  if (bw >= 1 && bw <= 64) return (gi >= ge && ge >= 0) ? BF_ROWS : BF_ANTIDIAG;
  const int ns = band_nslot(b);
  if (ns >= 1 && ns <= 2) return BF_WAVE2;
  if (ns >= 1 && ns <= 4) return BF_WAVE4;
  if (ns >= 1 && ns <= 7) return BF_WAVE7;
  if (ns >= 1 && ns <= 12) return BF_WAVE12;
  return BF_SCALAR;
}

// bytes of direction storage the form writes for this band (tw: anti-diagonal-major layout of the wave forms)
SMG_HD inline uint64_t band_dir_bytes(int form, const Band &b, bool tw) {
  const int nrows = b.s_len - b.s_left;
  if (form == BF_STRIP8 || form == BF_STRIP16) { const StripGeom sg = strip_geom(b, form == BF_STRIP8 ? 3 : 4); return strip_words(sg, sg.nstrip) * 4 + 16; }
  if (tw && form >= BF_ANTIDIAG && form <= BF_WAVE12) {
    const int jmin = b.q_left > b.l_edge ? b.q_left : b.l_edge;
    int jlast = b.r_edge + nrows - 1; if (jlast > b.q_len - 1) jlast = b.q_len - 1;
    const int64_t tmax = (int64_t)(nrows - 1) + (jlast - jmin);
    return tmax >= 0 ? (uint64_t)(tmax + 1) * (uint64_t)band_tw(b) + 8 : 8;
  }
  return (uint64_t)b.band_width * (uint64_t)nrows + (uint64_t)b.band_width + 8;      // the reference's size (alignment.c:459)
}

struct BandNodeArgs {
  const uint8_t *q; const uint32_t *q_off;       // read codes
  const uint8_t *win; const uint32_t *r_off;     // decoded window codes (0-3, 5)
  uint32_t ntask;
  const int32_t *band, *iv;                      // {band_l, band_r, qs, qe}, {s_left, s_right} per task
  int minscore, form, lds, tw;
  uint8_t *dir; const uint64_t *dir_off;         // direction storage per task (16-byte aligned offsets)
  void *bnd; uint32_t bndcap;                    // strip forms: 2 x bndcap (H, F) pairs per task
  int *rows; uint32_t rowlen;                    // scalar form: 2 x rowlen ints per task
  uint8_t *dtmp, *dstr; const uint32_t *dstr_off;   // reversed and forward DiffStr per task
  BandNodeOut *out;
};

}  // namespace smg

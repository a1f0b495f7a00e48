// smg_bandnode.hip -- stand-alone entry of the K3 band pass (parity tests): one wave runs one node of the recursion
// (alignment.c:1300) in ONE named form -- band set-up, band pass, the traceback stage_align pairs with that form, forward
// DiffStr.  Thin wrappers over the cores of smg_stages.hpp; no recurrence is restated here.
#include <hip/hip_runtime.h>
#include "smg_kernels.h"
#include "smg_stages.hpp"

namespace smg {

// LDS: read and window staged in LDS with LDS-typed pointers (row form only), the directions there as well if they fit
template <int FORM, bool LDS>
__global__ void __launch_bounds__(64) k_band_node_raw(BandNodeArgs a, MapPar p) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr bool STRIP = FORM == BF_STRIP8 || FORM == BF_STRIP16;
  __shared__ int2 ring[STRIP ? 256 : 1];
  __shared__ int st[4];
  __shared__ __align__(16) uint8_t lq[LDS ? NODE_LDS_CODES : 1], lw[LDS ? NODE_LDS_CODES : 1], ldir[LDS ? NODE_LDS_DIR : 1];
  const uint32_t t = blockIdx.x;
  if (t >= a.ntask) return;
  const uint32_t qlen = a.q_off[t + 1] - a.q_off[t], wlen = a.r_off[t + 1] - a.r_off[t];
  const uint8_t *q = a.q + a.q_off[t], *win = a.win + a.r_off[t];
  uint8_t *dirm = a.dir + a.dir_off[t];
  uint8_t *dtmp = a.dtmp + a.dstr_off[t], *dstr = a.dstr + a.dstr_off[t];
  const uint32_t dtmpcap = qlen + wlen + 16;
  const int gi = -p.gap_init, ge = -p.gap_ext;
  int8_t M[64];
  score_matrix(M, p.match, p.mismatch);
  BandNodeOut o;
  o.status = NODE_ALIGNED; o.score = o.max_i = o.max_j = o.qs = o.rs = o.dlen = 0; o.stroffs = a.dstr_off[t];
  Band band;
  if (band_init(band, a.band[4 * t], a.band[4 * t + 1], a.band[4 * t + 2], a.band[4 * t + 3], (int)qlen, a.iv[2 * t], a.iv[2 * t + 1], (int)wlen)) o.status = NODE_REFUSED;
  else if (band.s_left >= band.s_len || band.band_width < 0) o.status = SMG_ERR_ASSERT;
  else if (!band_form_ok(FORM, band, gi, ge)) o.status = SMG_ERR_ASSERT;          // (the host has checked this already)
  if (o.status) { if (threadIdx.x == 0) a.out[t] = o; return; }                   // wave-uniform
  if (LDS) {
    for (uint32_t i = threadIdx.x; i < qlen; i += 64) lq[i] = q[i];
    for (uint32_t i = threadIdx.x; i < wlen; i += 64) lw[i] = win[i];
    q = lq; win = lw;
    if (band_dir_bytes(FORM, band, false) <= (uint64_t)NODE_LDS_DIR) dirm = ldir;
    __syncthreads();
  }
  int max_i = 0, max_j = 0, max_scor = 0, tW = 0;
  StripGeom sg = strip_geom(band, FORM == BF_STRIP16 ? 4 : 3);
  typedef SMG_LDSQ const uint8_t *PL;
  typedef SMG_LDSQ uint8_t *PLD;
  if constexpr (FORM == BF_ROWS) {
    if (LDS && dirm == ldir) max_scor = band_track_rows<PL, PLD>(band, (PL)q, (PL)win, p.match, p.mismatch, gi, ge, (PLD)dirm, &max_i, &max_j);
    else if (LDS) max_scor = band_track_rows<PL, uint8_t *>(band, (PL)q, (PL)win, p.match, p.mismatch, gi, ge, dirm, &max_i, &max_j);
    else max_scor = band_track_rows<const uint8_t *, uint8_t *>(band, q, win, p.match, p.mismatch, gi, ge, dirm, &max_i, &max_j);
  } else if constexpr (FORM == BF_ANTIDIAG) {
    tW = a.tw ? band_tw(band) : 0;
    max_scor = band_track_wave<const uint8_t *>(band, q, win, p.match, p.mismatch, gi, ge, dirm, &max_i, &max_j, tW);
  } else if constexpr (FORM >= BF_WAVE2 && FORM <= BF_WAVE12) {
    constexpr int NS = FORM == BF_WAVE2 ? 2 : FORM == BF_WAVE4 ? 4 : FORM == BF_WAVE7 ? 7 : 12;
    tW = a.tw ? band_tw(band) : 0;
    max_scor = band_track_wave_n<NS, const uint8_t *>(band, q, win, p.match, p.mismatch, gi, ge, dirm, &max_i, &max_j, tW);
  } else if constexpr (STRIP) {
    tW = -1;
    max_scor = band_track_strip<const uint8_t *, FORM == BF_STRIP8 ? 8 : 16>(band, sg, q, win, p.match, p.mismatch, gi, ge, (uint32_t *)dirm,
                                                                           (int2 *)a.bnd + (size_t)t * 2 * a.bndcap, a.bndcap, ring, &max_i, &max_j);
  } else {
    if (threadIdx.x == 0) {
      int *Hp = a.rows + (size_t)t * 2 * a.rowlen;
      st[0] = band_track_scalar(band, q, win, M, gi, ge, Hp, Hp + a.rowlen, dirm, &max_i, &max_j); st[1] = max_i; st[2] = max_j;
    }
    __syncthreads();
    max_scor = st[0]; max_i = st[1]; max_j = st[2];
  }
  __threadfence();
  __syncthreads();
  o.score = max_scor; o.max_i = max_i; o.max_j = max_j;
  if (max_scor < a.minscore) o.status = NODE_BELOW;
  else {
    int dn, qs = 0, rs = 0;
    if constexpr (FORM == BF_ROWS) dn = traceback_uniform<false>(dtmp, dtmpcap, &qs, &rs, band, dirm, max_i, max_j, max_scor, q, win, (int)M[0], (int)M[1], gi, ge);
    else {
      if (threadIdx.x == 0) { st[0] = traceback_scalar<false>(dtmp, dtmpcap, &qs, &rs, band, dirm, max_i, max_j, max_scor, q, win, M, gi, ge, tW, &sg); st[1] = qs; st[2] = rs; }
      __syncthreads();
      dn = st[0]; qs = st[1]; rs = st[2];
    }
    if (dn < 0) o.status = dn == -2 ? SMG_ERR_CAP : (dn == -3 ? SMG_ERR_SCORE : SMG_ERR_ASSERT);
    else {
      o.qs = qs; o.rs = rs;
      if (threadIdx.x == 0) {
        o.dlen = diffstr_reverse(dstr, dtmp, dn);
        if (o.dlen < 0) { o.status = SMG_ERR_ASSERT; o.dlen = 0; }
      }
    }
  }
  if (threadIdx.x == 0) a.out[t] = o;
#endif
}

template <int FORM, bool LDS>
static void launch_node_t(hipStream_t s, const BandNodeArgs &a, const MapPar &p) {
  hipLaunchKernelGGL((k_band_node_raw<FORM, LDS>), dim3(a.ntask), dim3(64), 0, s, a, p);
}

int launch_band_nodes(hipStream_t s, const BandNodeArgs &a, const MapPar &p) {
  if (!a.ntask) return 0;
  switch (a.form) {
    case BF_ROWS: if (a.lds) launch_node_t<BF_ROWS, true>(s, a, p); else launch_node_t<BF_ROWS, false>(s, a, p); break;
    case BF_ANTIDIAG: launch_node_t<BF_ANTIDIAG, false>(s, a, p); break;
    case BF_WAVE2: launch_node_t<BF_WAVE2, false>(s, a, p); break;
    case BF_WAVE4: launch_node_t<BF_WAVE4, false>(s, a, p); break;
    case BF_WAVE7: launch_node_t<BF_WAVE7, false>(s, a, p); break;
    case BF_WAVE12: launch_node_t<BF_WAVE12, false>(s, a, p); break;
    case BF_STRIP8: launch_node_t<BF_STRIP8, false>(s, a, p); break;
    case BF_STRIP16: launch_node_t<BF_STRIP16, false>(s, a, p); break;
    case BF_SCALAR: launch_node_t<BF_SCALAR, false>(s, a, p); break;
    default: return -1;
  }
  hipError_t e = hipGetLastError();
  return e != hipSuccess ? (int)e : 0;
}

}  // namespace smg

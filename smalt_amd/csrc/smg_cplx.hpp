// smg_cplx.hpp -- complexity-weighted alignment scores (smalt map -w, RMAPFLG_CMPLXW): what makeMetaFromTrack does with
// the letter counts of a traceback (scaleALICPLX, alignment.c:268-305), bit for bit.
//
// The reference counts the reference letter under every diagonal step of the traceback (alignment.c:706-707, codes
// 0..5 of the alphabet "ACGTXN") and replaces the score of the alignment by
//     (int)(score + (sum_c n_c ln(1/4) - (sum_c n_c ln n_c - n ln n)) / lambda + .999)
// in doubles, on gcc / x86-64 without fused multiply-adds.  Three rules keep the device on the same bits:
//   * no device logarithm: ln n comes from a table the host's libm filled (cplx_fill_logtab), n = 0 .. longest read;
//   * no contraction: hipcc would fuse a * b + c, so the function switches contraction off and keeps the order of
//     the reference's operations;
//   * lambda is computed on the host (cplx_lambda in smg_cplx.cpp, built with -ffp-contract=off).
// Table and lambda reach the device as one argument (CplxPar) of the weighted kernel instances only: the structures every
// kernel takes (Batch, MapPar) keep their layout, so no other kernel's argument offsets or register allocation move.
// `file:line` citations refer to the reference tree (SMALT 0.7.6, src/).
#pragma once
#include <stdint.h>
#include "smg_common.h"

namespace smg {

enum : int { CPLX_NCODES = 6 };                 // alphabet size of the codec ("ACGTXN", sequence.c:101): countp[0..5]
enum : int { CPLX_OK = 0, CPLX_EXCEEDS = 1,     // ERRCODE_CPLXSCOR: "complexity weighted score exceeds unweighted score"
             CPLX_RANGE = 2 };                  // more counted steps than the table holds (cannot happen: steps <= read length)

struct CplxPar { const double *logtab; uint32_t nlog, pad; double lambda; };     // logtab[i] = log((double)i), i < nlog (per mapper); lambda per call
struct NoCplx {};
template <bool CPLX> struct cplx_arg { typedef NoCplx type; };
template <> struct cplx_arg<true> { typedef CplxPar type; };

// scoreMatrixCalcLambda (score.c:252-277) for a match / mismatch pair; host only (smg_cplx.cpp)
double cplx_lambda(int match, int mismatch);
// tab[i] = log((double)i) for i < n (tab[0] is never read)
void cplx_fill_logtab(double *tab, uint32_t n);

// scaleALICPLX (alignment.c:268-305).  cnt: diagonal steps per reference letter code; logtab[i] = log((double)i), i < nlog.
SMG_HD inline int cplx_scale(int *adj_score, int orig_score, const int (&cnt)[CPLX_NCODES], const double *logtab, uint32_t nlog, double lambda) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double LN0P25 = -1.386294;              // alignment.c:71 (truncated on purpose: it is the reference's constant)
  double t_factor = 0.0, t_sum = 0.0;
  int t_counts = 0;
  for (int i = 0; i < CPLX_NCODES; i++) {
    const int count = cnt[i];
    if (count) {
      if ((uint32_t)count >= nlog) return CPLX_RANGE;
      t_factor += count * logtab[count];
      t_sum += count * LN0P25;
      t_counts += count;
    }
  }
  // (no diagonal step: the reference computes 0 * log(0), a NaN that its x86 conversion turns into INT_MIN and :301 into 0;
  //  an alignment with a positive score has at least one)
  if (t_counts <= 0) { *adj_score = 0; return CPLX_OK; }
  if ((uint32_t)t_counts >= nlog) return CPLX_RANGE;
  t_factor -= t_counts * logtab[t_counts];
  t_sum -= t_factor;
  const int adj = (int)(orig_score + t_sum / lambda + .999);
  *adj_score = adj;
  if (adj > orig_score) return CPLX_EXCEEDS;
  if (adj < 0) *adj_score = 0;
  return CPLX_OK;
}

}  // namespace smg

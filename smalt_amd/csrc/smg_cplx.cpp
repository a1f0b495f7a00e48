// smg_cplx.cpp -- host side of the complexity weighting (smalt map -w): lambda of the score matrix and the table of
// logarithms the device reads.  Built with -ffp-contract=off like the other host files: the reference is gcc -O2 on
// x86-64, which never fuses a multiply into an add.  `file:line` citations refer to the reference tree (SMALT 0.7.6, src/).
#include <math.h>
#include "smg_cplx.hpp"

namespace smg {

// scoreMatrixCalcLambda (score.c:252-277): doubling, then bisection to 1e-5, on sum_{4x4} exp(lambda * score[i][j]) / 16 >= 1.
// The value returned is the last one tried, not the upper bound.
double cplx_lambda(int match, int mismatch) {
  double lambda, sum, lambda_lower, lambda_upper;
  auto getsum = [&]() {
    sum = 0;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) sum += exp(lambda * (i == j ? match : mismatch));
    sum *= 0.0625;
  };
  lambda_lower = 0.0;
  lambda = 0.5;
  for (;;) {
    getsum();
    if (sum >= 1.0) break;
    lambda_lower = lambda;
    lambda *= 2.0;
  }
  lambda_upper = lambda;
  while (lambda_upper - lambda_lower > .00001) {
    lambda = (lambda_lower + lambda_upper) / 2.0;
    getsum();
    if (sum >= 1.0) lambda_upper = lambda;
    else lambda_lower = lambda;
  }
  return lambda;
}

void cplx_fill_logtab(double *tab, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) tab[i] = i ? log((double)i) : 0.0;
}

}  // namespace smg

// cplx_check.cpp -- the complexity weighting of smalt map -w (smalt_amd/csrc/smg_cplx.hpp, smg_cplx.cpp) on the host, for
// tests/test_cplx.py.  Standard input, one request per line:
//   L <match> <mismatch>                 -> lambda as a hexadecimal float (every bit of the double)
//   S <orig> <nA> <nC> <nG> <nT> <nX> <nN>  -> <code> <weighted score>   (code: CPLX_OK 0, CPLX_EXCEEDS 1, CPLX_RANGE 2; lambda of the last L line)
// build: g++ -O2 -std=c++17 -ffp-contract=off -o cplx_check cplx_check.cpp   (add -fsanitize=address,undefined for a checked run)
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../smalt_amd/csrc/smg_cplx.cpp"

int main() {
  const uint32_t nlog = 1u << 16;
  std::vector<double> logtab(nlog);
  smg::cplx_fill_logtab(logtab.data(), nlog);
  double lambda = smg::cplx_lambda(1, -2);
  char line[256];
  while (fgets(line, sizeof(line), stdin)) {
    int a[7];
    if (line[0] == 'L' && sscanf(line + 1, "%d %d", &a[0], &a[1]) == 2) {
      lambda = smg::cplx_lambda(a[0], a[1]);
      printf("%a\n", lambda);
    } else if (line[0] == 'S' && sscanf(line + 1, "%d %d %d %d %d %d %d", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6]) == 7) {
      const int cnt[smg::CPLX_NCODES] = {a[1], a[2], a[3], a[4], a[5], a[6]};
      int adj = 0;
      const int rc = smg::cplx_scale(&adj, a[0], cnt, logtab.data(), nlog, lambda);
      printf("%d %d\n", rc, adj);
    } else {
      fprintf(stderr, "cplx_check: bad request: %s", line);
      return 2;
    }
  }
  return 0;
}

// tests/hostemu/index_carry_check.cpp -- TEST DRIVER: smg::index_carry (smalt_amd/csrc/smg_indexbuild.h) on the host, for
// tests/test_index_ref.py.  Standard input, one reference per line: <k> <s> <nseq> <len> ... ; output lines: `refused <sequence>`
// where the reference's `smalt index` refuses the sampling step for that sequence, else `built <maxpos>`.
#include <stdio.h>
#include <vector>
#include "../../smalt_amd/csrc/smg_indexbuild.h"

int main() {
  int k, s;
  long nseq;
  while (scanf("%d %d %ld", &k, &s, &nseq) == 3) {
    if (k < 3 || k > 20 || s < 1 || s > 127 || nseq < 1) { fprintf(stderr, "bad line: k=%d s=%d nseq=%ld\n", k, s, nseq); return 2; }
    std::vector<uint64_t> sop(1, 0);
    for (long i = 0; i < nseq; i++) {
      unsigned long long len;
      if (scanf("%llu", &len) != 1) { fprintf(stderr, "short line\n"); return 2; }
      sop.push_back(sop.back() + len);
    }
    uint32_t maxpos = 0;
    const int64_t bad = smg::index_carry(sop.data(), (int64_t)nseq, k, s, &maxpos);
    if (bad >= 0) printf("refused %lld\n", (long long)bad);
    else printf("built %u\n", maxpos);
  }
  return 0;
}

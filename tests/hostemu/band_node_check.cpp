// The one-lane forms of K2b and K3 from the product's headers on explicit tasks, without a GPU: band_init, band_fast_scalar
// (window read through ref_code from a packed array that starts at a word phase of its own per task), and one node of the K3
// recursion -- band_track_scalar, traceback_scalar, diffstr_reverse -- as smaltgpu_band_align_nodes runs it in its SCALAR form.
// Every buffer has exactly the size the product gives it, so that a sanitizer build sees an access outside.
//   band_node_check FILE
// FILE: "match mismatch gap_init gap_ext minscore ntask", then per task "mode qlen wlen band_l band_r qs qe s_left s_right",
// the read and the window as strings of code digits.  mode 0: K2b, prints "K2B status score"; mode 1: K3 node, prints
// "NODE status score max_i max_j qs rs DiffStr-in-hex" (status as smaltgpu_band_node).
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "../../smalt_amd/csrc/smg_bandnode.h"
using namespace smg;

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: band_node_check FILE\n"); return 2; }
  FILE *f = fopen(argv[1], "r");
  if (!f) { perror(argv[1]); return 2; }
  int match, mismatch, gap_init, gap_ext, minscore, ntask;
  if (fscanf(f, "%d %d %d %d %d %d", &match, &mismatch, &gap_init, &gap_ext, &minscore, &ntask) != 6) return 2;
  const int gi = -gap_init, ge = -gap_ext;
  int8_t M[64];
  score_matrix(M, match, mismatch);
  for (int t = 0; t < ntask; t++) {
    int mode, qlen, wlen, bl, br, qs, qe, s_left, s_right;
    if (fscanf(f, "%d %d %d %d %d %d %d %d %d", &mode, &qlen, &wlen, &bl, &br, &qs, &qe, &s_left, &s_right) != 9 || qlen < 1 || wlen < 1) return 2;
    std::vector<char> qb((size_t)qlen + 2), wb((size_t)wlen + 2);
    char fmt[32];
    snprintf(fmt, sizeof fmt, "%%%ds", qlen + 1);
    if (fscanf(f, fmt, qb.data()) != 1 || (int)strlen(qb.data()) != qlen) return 2;
    snprintf(fmt, sizeof fmt, "%%%ds", wlen + 1);
    if (fscanf(f, fmt, wb.data()) != 1 || (int)strlen(wb.data()) != wlen) return 2;
    std::vector<uint8_t> q((size_t)qlen), w((size_t)wlen);
    for (int i = 0; i < qlen; i++) q[i] = (uint8_t)((qb[i] - '0') & 7);
    for (int i = 0; i < wlen; i++) w[i] = (uint8_t)((wb[i] - '0') & 7);
    std::vector<int> Hp((size_t)qlen + 2, 0), Ep((size_t)qlen + 2, 0);
    Band band;
    if (mode == 0) {
      const uint64_t phase = (uint64_t)(t % 10);
      std::vector<uint32_t> packed((size_t)((phase + (uint64_t)wlen + 9) / 10), 0u);
      for (int i = 0; i < wlen; i++) { const uint64_t o = phase + (uint64_t)i; packed[o / 10] |= (uint32_t)w[i] << (3 * (9 - (uint32_t)(o % 10))); }
      if (band_init(band, bl, br, qs, qe, qlen, 0, wlen - 1, wlen)) { printf("K2B 1 0\n"); continue; }
      printf("K2B 0 %d\n", band_fast_scalar(band, q.data(), packed.data(), phase, M, gi, ge, Hp.data(), Ep.data()));
      continue;
    }
    int status = NODE_ALIGNED, score = 0, max_i = 0, max_j = 0, tqs = 0, trs = 0;
    std::string hex;
    if (band_init(band, bl, br, qs, qe, qlen, s_left, s_right, wlen)) status = NODE_REFUSED;
    else if (band.s_left >= band.s_len || band.band_width < 0) status = SMG_ERR_ASSERT;
    else {
      std::vector<uint8_t> dir((size_t)band_dir_bytes(BF_SCALAR, band, false), 0);
      score = band_track_scalar(band, q.data(), w.data(), M, gi, ge, Hp.data(), Ep.data(), dir.data(), &max_i, &max_j);
      if (score < minscore) status = NODE_BELOW;
      else {
        std::vector<uint8_t> dtmp((size_t)qlen + wlen + 16), dstr((size_t)qlen + wlen + 16);
        const int dn = traceback_scalar<false>(dtmp.data(), (uint32_t)dtmp.size(), &tqs, &trs, band, dir.data(), max_i, max_j, score, q.data(), w.data(), M, gi, ge);
        if (dn < 0) status = dn == -2 ? SMG_ERR_CAP : (dn == -3 ? SMG_ERR_SCORE : SMG_ERR_ASSERT);
        else {
          const int fl = diffstr_reverse(dstr.data(), dtmp.data(), dn);
          if (fl < 0) status = SMG_ERR_ASSERT;
          for (int i = 0; i < fl; i++) { char b[4]; snprintf(b, sizeof b, "%02x", dstr[i]); hex += b; }
        }
      }
    }
    printf("NODE %d %d %d %d %d %d %s\n", status, score, max_i, max_j, tqs, trs, hex.empty() ? "-" : hex.c_str());
  }
  fclose(f);
  return 0;
}

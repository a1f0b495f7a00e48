// smg_indexbuild.h -- device-side construction of the index image (smg_indexbuild.hip)
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include "smg_devmem.hpp"
#endif

namespace smg {

// selectHashTyp (smalt.c:268-332): 0 or -1 (unsupported)
int index_geometry(int k, int s, uint64_t totlen, int *typ, int *nbits_key, int *nbits_lo);

// The walk of doWordsInSeq (hashidx.c:465-531) over the sequence lengths alone: the countdown to the end of the next sampled word
// and the offset of the first word of the next sequence, both held by the reference in an `unsigned char`, and the serial counter.
// With s <= k the offset stays below s and the counter ends at ceil(tot / s): the global grid.  With s > k a sequence can end more
// than k bases in front of the next grid point; then the offset carried over is s or more and the reference refuses the next
// sequence (hashidx.c:494), and behind the last sequence the counter can end one above the grid's (hashidx.c:524-528).
// -> -1 and *maxpos as hashidx.c:992 writes it, or the index of the sequence the reference refuses.  Host code, O(nseq).
inline int64_t index_carry(const uint64_t *sop, int64_t nseq, int k, int s, uint32_t *maxpos) {
  unsigned char offs = 0;
  uint32_t ctr = 0;
  for (int64_t i = 0; i < nseq; i++) {
    if (offs >= s) return i;
    const uint64_t len = sop[i + 1] - sop[i];
    unsigned char c = (unsigned char)(k + offs);          // bases to the end of the next sampled word
    if (len >= c) {                                       // that word ends after c bases, every further one s bases later
      const uint64_t r = len - c;
      ctr += (uint32_t)(1 + r / (uint64_t)s);
      c = (unsigned char)(s - (int)(r % (uint64_t)s));
    } else c = (unsigned char)(c - len);
    offs = (unsigned char)((k - c) % s);                  // C's remainder: negative where the countdown is above k
    if (offs) offs = (unsigned char)(s - offs);
    ctr += (uint32_t)((k - c + offs) / s);
  }
  *maxpos = ctr ? ctr - 1 : 0;
  return -1;
}

#if defined(__HIPCC__)
struct BuiltIndex {                 // the device arrays go with it, or are released to whoever keeps the index
  int typ = 0, nbits_key = 0, nbits_lo = 0;
  uint32_t nkeys = 0, npos = 0, nwords = 0, maxpos = 0;
  DevMem<uint32_t> idx, pos, wordidx, posidx, packed;
  float build_ms = 0;               // device time of the whole construction (HIP events)
};

// d_ascii: the concatenated reference sequences in HBM (tot bytes, letters as in FASTA); h_sop: nseq + 1 offsets (host)
int build_index_device(const uint8_t *d_ascii, uint64_t tot, const uint64_t *h_sop, int nseq, int k, int s, BuiltIndex *out, char *err, size_t errlen);
#endif

}  // namespace smg

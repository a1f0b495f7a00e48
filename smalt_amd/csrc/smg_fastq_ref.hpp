// smg_fastq_ref.hpp -- a reference file with FASTQ records ('@' and '+' prompts) read as the reference program reads it, stated
// once for the kernels of smg_fastq_ref.hip and for a host build (tests/hostemu/fastq_ref_check.cpp).
//
// The lexing is the one of smg_fasta.hpp: white space is isspace() of the C locale, a prompt is a '>', '@' or '+' directly behind
// a '\n', and behind leading white space the text begins with a prompt.  The records (seqFastqRead sequence.c:1960-1990 over
// readHeader :1056-1146, readSeqFast :1229-1304 and readQual :1743-1772):
//   1  a prompt opens a header line that runs to the next '\n'; '>' and '@' are the same thing;
//   2  data follows: every byte that is not white space counts, up to the next eligible prompt or the end of the text.  A prompt on
//      the line directly behind the header line is not eligible (it is data).  n: the count;
//   3  behind a '+' prompt the segment is dropped (no sequence, no name);
//   4  otherwise it is a sequence of n bases.  If the prompt that ended it is '+', a quality section follows: its header line is
//      thrown away, then bytes are counted as in 2, but a prompt ends the section only once the count has reached n -- lines
//      that begin with a prompt before that are quality data.  m: the count at the end; m != n is "wrong FASTQ/FASTA format";
//   5  a sequence that no '+' follows is a FASTA record.
// Where a quality section ends depends on n, so the text is no regular language and the block summaries of smg_fasta.hpp do not
// compose.  Two facts about the text do not depend on the parse and make a walk over the records cheap:
//   candidates   the offsets of all '>', '@', '+' directly behind a '\n', one ascending list.  In data every candidate is eligible
//                but one directly behind the header line's '\n', so "the prompt that ends this data" is the first candidate
//                behind a known offset;
//   non-blank prefix counts   per block of text (64 bits) and, inside a block, per granule of 64 bytes (32 bits): n and m are
//                differences of such prefixes, and the byte with which a quality section reaches n is a search over them.
// The walk (fq_walk) runs in ONE wave: every step that looks at 64 things at once goes through fq_mask64 -- a ballot over the lanes
// on the device, a loop on the host -- and everything else is the same in all lanes.  Every loop advances its offset strictly or
// shrinks its range strictly.
#pragma once
#include <stdio.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include "smg_fasta.hpp"

namespace smg {

enum : uint32_t { FQ_GRAN = 64 /* bytes per granule of the non-blank prefix counts */, FQ_REC_PER_TILE = FA_TILE / 2 /* more records than begin in a tile */ };
enum : uint32_t { FQ_OK = 0, FQ_ERR_NOPROMPT = 1 /* the text does not begin with a prompt */, FQ_ERR_QUAL = 2 /* m != n */, FQ_ERR_TABLE = 3 /* more records than prompts */ };

SMG_HD inline bool fq_prompt(uint8_t c) { return c == '>' || c == '@' || c == '+'; }
SMG_HD inline bool fq_candidate(uint8_t prev, uint8_t c) { return prev == '\n' && fq_prompt(c); }

// a sequence: its header's prompt, the text range of its data [d0, d1), the bases in front of it and the non-blank bytes in front of d0
struct FqRecord { uint64_t hdr_off, d0, d1, base_off, nb0; };
// what the walk found.  err_*: the record whose quality section holds err_m characters for err_n bases
struct FqWalk { uint64_t nrec, nbases, nprompt, err_hdr_off, err_prompt_no, err_n, err_m; uint32_t err, pad; };
// the text with what the passes in front of the walk made of it.  blk_nb: nblk + 1 exclusive prefixes; gran_nb: non-blank bytes of
// the granule's block in front of the granule
struct FqText {
  const uint8_t *text; uint64_t len; uint32_t block_bytes, pad;
  const uint64_t *blk_nb; const uint32_t *gran_nb; const uint64_t *cand; uint64_t ncand, nblk;
};

SMG_HD inline bool fq_lane0() {
#if defined(__HIP_DEVICE_COMPILE__)
  return (threadIdx.x & 63u) == 0;
#else
  return true;
#endif
}
// bit i of the result: pred(i), i < 64
template <class F> SMG_HD inline uint64_t fq_mask64(F pred) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ballot(pred(threadIdx.x & 63u));
#else
  uint64_t m = 0;
  for (uint32_t i = 0; i < 64; i++) if (pred(i)) m |= 1ull << i;
  return m;
#endif
}
SMG_HD inline uint32_t fq_ctz(uint64_t m) { return (uint32_t)__builtin_ctzll(m); }
SMG_HD inline uint32_t fq_popc(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// what a lane finds in its n bytes (prev: the byte in front of them, 0 at the start of the text): non-blank bytes | candidates << 16
SMG_HD inline uint32_t fq_lane_counts(const uint8_t *c, uint32_t n, uint8_t prev) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < n; i++) { r += (fa_isspace(c[i]) ? 0u : 1u) + (fq_candidate(prev, c[i]) ? 1u << 16 : 0u); prev = c[i]; }
  return r;
}

// the first offset >= from whose byte is a '\n' (nl) / is not white space (!nl); len: none
SMG_HD inline uint64_t fq_find_byte(const FqText &t, uint64_t from, bool nl) {
  for (uint64_t o = from; o < t.len; o += 64) {
    const uint64_t m = fq_mask64([&](uint32_t i) { return o + i < t.len && (nl ? t.text[o + i] == '\n' : !fa_isspace(t.text[o + i])); });
    if (m) return o + fq_ctz(m);
  }
  return t.len;
}
// the non-blank bytes of text[0, x)
SMG_HD inline uint64_t fq_nb(const FqText &t, uint64_t x) {
  if (x >= t.len) return t.blk_nb[t.nblk];
  const uint64_t g0 = x & ~(uint64_t)(FQ_GRAN - 1);
  const uint64_t m = fq_mask64([&](uint32_t i) { return g0 + i < x && !fa_isspace(t.text[g0 + i]); });
  return t.blk_nb[x / t.block_bytes] + t.gran_nb[x / FQ_GRAN] + fq_popc(m);
}
// The first index i of [lo, hi) with f(i) >= x; hi: none.  f ascends.  64 values per step: the 64 behind lo first (the walk asks
// for places close by), then the range is cut into 64 parts, and again, until 64 values are left: every round shrinks it.
template <class F> SMG_HD inline uint64_t fq_first_ge(F f, uint64_t lo, uint64_t hi, uint64_t x) {
  const uint64_t none = hi;
  uint64_t m = fq_mask64([&](uint32_t i) { return lo + i >= hi || f(lo + i) >= x; });
  if (m) { const uint64_t r = lo + fq_ctz(m); return r < hi ? r : none; }
  lo += 64;
  while (hi - lo > 64) {
    const uint64_t step = (hi - lo + 63) / 64;                        // lane i looks at the last value of part i
    m = fq_mask64([&](uint32_t i) { const uint64_t p = lo + (uint64_t)(i + 1) * step - 1; return p >= hi || f(p) >= x; });
    if (!m) return none;
    lo += (uint64_t)fq_ctz(m) * step;
    if (hi - lo > step) hi = lo + step;
  }
  m = fq_mask64([&](uint32_t i) { return lo + i >= hi || f(lo + i) >= x; });
  if (!m) return none;
  const uint64_t r = lo + fq_ctz(m);
  return r < hi ? r : none;
}
// the smallest r with fq_nb(r) == want.  fq_nb(from) < want <= all non-blank bytes of the text
SMG_HD inline uint64_t fq_nb_reach(const FqText &t, uint64_t from, uint64_t want) {
  const uint64_t b_from = from / t.block_bytes;
  // the last block with blk_nb[b] < want
  const uint64_t b = fq_first_ge([&](uint64_t i) { return t.blk_nb[i]; }, b_from + 1, t.nblk + 1, want) - 1;
  if (b >= t.nblk) return t.len;
  const uint64_t per = t.block_bytes / FQ_GRAN, ngran = (t.len + FQ_GRAN - 1) / FQ_GRAN, g_end = (b + 1) * per < ngran ? (b + 1) * per : ngran;
  const uint64_t in_block = want - t.blk_nb[b], g_from = b == b_from ? from / FQ_GRAN : b * per;
  // the last granule of the block with gran_nb[g] < in_block
  const uint64_t g = fq_first_ge([&](uint64_t i) { return (uint64_t)t.gran_nb[i]; }, g_from + 1, g_end, in_block) - 1;
  if (g >= g_end) return t.len;
  const uint64_t g0 = g * FQ_GRAN, k = in_block - t.gran_nb[g];      // the k-th non-blank byte of the granule, 1 <= k <= 64
  uint64_t m = fq_mask64([&](uint32_t i) { return g0 + i < t.len && !fa_isspace(t.text[g0 + i]); });
  if (k < 1 || k > fq_popc(m)) return t.len;
  for (uint64_t j = 1; j < k; j++) m &= m - 1;
  return g0 + fq_ctz(m) + 1;
}
// the first candidate at or behind x; len: none.  ci: a cursor into the list that only moves up
SMG_HD inline uint64_t fq_cand_from(const FqText &t, uint64_t &ci, uint64_t x) {
  ci = fq_first_ge([&](uint64_t i) { return t.cand[i]; }, ci, t.ncand, x);
  return ci < t.ncand ? t.cand[ci] : t.len;
}

// The records in order.  rec: room for cap records.  Per record a scan for the header's '\n', the first candidate behind it, two
// prefix counts; with a quality section the same again and the search for the byte that reaches n.
SMG_HD inline void fq_walk(const FqText &t, FqRecord *rec, uint64_t cap, FqWalk *out) {
  FqWalk w;
  w.nrec = w.nbases = w.nprompt = w.err_hdr_off = w.err_prompt_no = w.err_n = w.err_m = 0; w.err = FQ_OK; w.pad = 0;
  const uint64_t all = t.blk_nb[t.nblk];
  uint64_t ci = 0, p = fq_find_byte(t, 0, false);
  if (p < t.len && !fq_prompt(t.text[p])) { w.err = FQ_ERR_NOPROMPT; w.err_hdr_off = p; p = t.len; }
  while (p < t.len) {                                       // p: a prompt; every round moves it up
    const uint8_t c = t.text[p];
    const uint64_t e = fq_find_byte(t, p + 1, true), d0 = e < t.len ? e + 1 : t.len;
    const uint64_t q = d0 + 1 < t.len ? fq_cand_from(t, ci, d0 + 1) : t.len;
    w.nprompt++;
    if (c == '+') { p = q; continue; }                      // rule 3
    const uint64_t nb0 = fq_nb(t, d0), n = fq_nb(t, q) - nb0;
    if (w.nrec >= cap) { w.err = FQ_ERR_TABLE; break; }
    if (fq_lane0()) { FqRecord r; r.hdr_off = p; r.d0 = d0; r.d1 = q; r.base_off = w.nbases; r.nb0 = nb0; rec[w.nrec] = r; }
    const uint64_t hdr_off = p, prompt_no = w.nprompt;
    w.nrec++; w.nbases += n;
    p = q;
    if (q < t.len && t.text[q] == '+') {                    // rule 4
      const uint64_t e1 = fq_find_byte(t, q + 1, true), q0 = e1 < t.len ? e1 + 1 : t.len, nb1 = fq_nb(t, q0);
      w.nprompt++;
      uint64_t x = t.len;
      if (all - nb1 >= n) {
        const uint64_t r = n ? fq_nb_reach(t, q0, nb1 + n) : q0, lo = r > q0 + 1 ? r : q0 + 1;
        if (lo < t.len) x = fq_cand_from(t, ci, lo);
      }
      const uint64_t m = fq_nb(t, x) - nb1;
      if (m != n) { w.err = FQ_ERR_QUAL; w.err_hdr_off = hdr_off; w.err_prompt_no = prompt_no; w.err_n = n; w.err_m = m; break; }
      p = x;
    }
  }
  *out = w;
}

// the records of [lo, hi) whose data begins at or in front of x, plus lo
SMG_HD inline uint64_t fq_rec_upper(const FqRecord *rec, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (rec[mid].d0 <= x) lo = mid + 1; else hi = mid; }
  return lo;
}
// where the bases of the block that begins at b0 go: u = fq_rec_upper(rec, 0, nrec, b0), nb_b0: the non-blank bytes in front of b0
SMG_HD inline uint64_t fq_block_base(const FqRecord *rec, uint64_t nrec, uint64_t nbases, uint64_t u, uint64_t b0, uint64_t nb_b0) {
  if (u > 0 && b0 < rec[u - 1].d1) return rec[u - 1].base_off + (nb_b0 - rec[u - 1].nb0);
  return u < nrec ? rec[u].base_off : nbases;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// why a walk cannot be used (empty: it can)
inline std::string fq_refusal(const FqWalk &w, const char *text, uint64_t text_len) {
  char buf[512];
  if (w.err == FQ_ERR_NOPROMPT) return fa_refusal(text_len, FA_E, 0, 0);
  if (w.err == FQ_ERR_QUAL) {
    std::string nm = w.err_hdr_off < text_len ? fa_clean_name(text + w.err_hdr_off + 1, (size_t)(text_len - w.err_hdr_off - 1)) : std::string();
    if (nm.size() > 120) nm = nm.substr(0, 117) + "...";
    snprintf(buf, sizeof(buf), "wrong FASTQ/FASTA format: the quality section of record '%s' (prompt %llu of the text, at byte %llu) holds %llu characters for %llu bases",
             nm.c_str(), (unsigned long long)w.err_prompt_no, (unsigned long long)w.err_hdr_off, (unsigned long long)w.err_m, (unsigned long long)w.err_n);
    return buf;
  }
  if (w.err) return "the walk over the records found more records than prompts";
  if (w.nrec == 0) return fa_refusal(text_len, FA_S0, 0, 0);
  return std::string();
}

#if defined(__HIPCC__)
// The parse on the device (smg_fastq_ref.hip), with the results of fasta_parse_device.  The text in HBM is out->d_text where
// fasta_parse_device has left it there (it is taken from there and gone when the call returns), otherwise it is copied there.
// pass_a_ms: candidates and prefix counts (three launches), compose_ms: the walk, pass_b_ms: the output pass.
int fastq_ref_parse_device(const char *text, uint64_t text_len, uint32_t block_bytes, FastaParsed *out, char *err, size_t errlen);

// launchers of k_fq_count + k_fq_scan, of k_fq_scan alone (a and b: n + 1 entries) and of k_fq_cands (smg_fastq_ref.hip)
hipError_t fq_launch_counts(hipStream_t st, const uint8_t *text, uint64_t len, uint32_t block_bytes, uint64_t nblk, uint32_t *gran_nb, uint64_t *blk_nb, uint64_t *blk_cd);
hipError_t fq_launch_scan(hipStream_t st, uint64_t *a, uint64_t *b, uint64_t n);
hipError_t fq_launch_cands(hipStream_t st, const uint8_t *text, uint64_t len, uint32_t block_bytes, uint64_t nblk, const uint64_t *blk_cd, uint64_t *cand, uint64_t ncand);
#endif

}  // namespace smg

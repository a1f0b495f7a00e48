// smg_reads_dev.hpp -- a file of READS (FASTQ / FASTA text, a whole file or a chunk of it) parsed for all its records at once, stated
// once for the kernels of smg_reads_dev.hip and for a host build (tests/hostemu/reads_dev_check.cpp).
//
// The authority is smaltgpu_reads_parse (smg_report.cpp: general_parse, which restates seqFastqRead, sequence.c:1960-1990); the
// lexing, the candidates and the non-blank prefix counts are the ones of smg_fastq_ref.hpp.  Where a quality section ends depends on
// the number of bases in front of it, so which candidates are prompts of records is only known along the chain of records.  Instead
// of walking that chain (fq_walk: one wave, one record after the other) the text is taken in four steps:
//   step      every NODE -- node 0: the first non-blank byte of the text, node i > 0: candidate i - 1 -- is read as if a record
//             began there (rd_step): one step of the walk.  It yields the node where the next record would begin (the LINK; the
//             node behind the last one is the sink: the end of the text), what the node is (a dropped '+' segment, a FASTA record,
//             a FASTQ record, or a first byte that is no prompt), its ranges of data and quality bytes, its number of bases and the
//             flags "quality length differs" and "ran into the end of the text";
//   mark      the records of the text are the nodes on the path from node 0 along the links.  Links point forward only, so with
//             J_0 = link and J_r = J_(r-1) o J_(r-1) (pointer doubling, L = ceil(log2(nodes)) tables) the path is marked from
//             node 0 downwards from the highest level: a marked node marks J_r of itself in round r, and behind round r every
//             path position that is a multiple of 2^r is marked.  Only nodes of the path are ever marked;
//   number    prefix sums over the marked nodes that are records give every record its index and the offset of its bases.  The
//             first marked node (they come in text order) that general_parse would stop at -- an error, or with is_last = 0 a
//             record that ran into the end of the text -- cuts the batch, and so does max_reads;
//   emit      per block of text the non-blank bytes inside the data and quality ranges of the records taken go to their places
//             (rd_emit_lane): the place of a byte is the record's offset plus a difference of non-blank prefix counts.
// What differs from fq_walk (a reference file): a text that ends in a '+' segment or in a header line is no error, a quality
// section of another length only is one if the record is reached and complete (chunks), and no record at all is no error.
// Every loop advances its offset strictly or shrinks its range strictly.
#pragma once
#include "smg_fastq_ref.hpp"

namespace smg {

enum : uint32_t { RD_DROP = 0 /* a '+' segment, or nothing but white space */, RD_FASTA = 1, RD_FASTQ = 2, RD_NOPROMPT = 3 /* node 0 only */ };
enum : uint32_t { RD_F_QLEN = 4 /* m != n */, RD_F_END = 8 /* no prompt ends the record: it ran into the end of the text */ };
enum : uint32_t { RD_NODE_TILE = 256 /* nodes a workgroup numbers in one step */, RD_BLOCK_DEFAULT = 32u << 10, RD_GROUPS_DEFAULT = 2048, RD_NONE = 0xFFFFFFFFu };

// one step of the walk from a node.  kf: kind | flags; the ranges are empty where the node has none (q0 = q1 = d1 without qualities)
struct RdStep { uint64_t hdr_off, d0, d1, q0, q1, n, nb0 /* non-blank bytes in front of d0 */, nbq /* in front of q0 */; uint32_t link, kf; };
// a record taken, in text order
struct RdRec { uint64_t hdr_off, d0, d1, q0, q1, base_off, nb0, nbq; };
// what the numbering found.  stop_*: the first marked node the batch cannot go beyond (RD_NONE: none); stop_idx: the records in front
struct RdSum { uint32_t stop_node, stop_kf, nreads, any_fasta; uint64_t stop_idx, stop_hdr_off; };

SMG_HD inline uint32_t rd_kind(uint32_t kf) { return kf & 3u; }
SMG_HD inline bool rd_is_record(uint32_t kf) { return rd_kind(kf) == RD_FASTA || rd_kind(kf) == RD_FASTQ; }
// does general_parse stop at this node once it reaches it (before it takes it)?
SMG_HD inline bool rd_stops(uint32_t kf, bool is_last) {
  if (rd_kind(kf) == RD_NOPROMPT) return true;
  if (!rd_is_record(kf)) return false;
  return ((kf & RD_F_END) && !is_last) || (kf & RD_F_QLEN);
}
// ... and is it an error then (otherwise: the record is left for the next call)
SMG_HD inline bool rd_stop_is_error(uint32_t kf, bool is_last) { return rd_kind(kf) == RD_NOPROMPT || !((kf & RD_F_END) && !is_last); }

// canon_base of smg_report.cpp: upper case, U -> T, N for what is not within 31 of 'A'
SMG_HD inline uint8_t rd_canon(uint8_t c) {
  if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
  if (c == 'U') c = 'T';
  return (c >= 'A' && c < 'A' + 31) ? c : (uint8_t)'N';
}

// node -> offset of its first byte, and the cursor into the candidate list behind it
SMG_HD inline RdStep rd_step(const FqText &t, uint64_t node) {
  RdStep s;
  const uint64_t sink = t.ncand + 1, all = t.blk_nb[t.nblk];
  uint64_t ci = node;                                                  // candidate node - 1 is this one: the search begins behind it
  const uint64_t p = node ? t.cand[node - 1] : fq_find_byte(t, 0, false);
  s.hdr_off = p; s.d0 = s.d1 = s.q0 = s.q1 = t.len; s.n = 0; s.nb0 = s.nbq = all; s.link = (uint32_t)sink; s.kf = RD_DROP | RD_F_END;
  if (p >= t.len) return s;                                            // nothing but white space
  const uint8_t c = t.text[p];
  if (!fq_prompt(c)) { s.kf = RD_NOPROMPT; return s; }
  const uint64_t e = fq_find_byte(t, p + 1, true), d0 = e < t.len ? e + 1 : t.len;
  const uint64_t q = d0 + 1 < t.len ? fq_cand_from(t, ci, d0 + 1) : t.len;
  const uint32_t link_q = q < t.len ? (uint32_t)(ci + 1) : (uint32_t)sink;
  s.d0 = d0; s.d1 = s.q0 = s.q1 = q; s.link = link_q;
  if (c == '+') { s.d1 = s.q0 = s.q1 = d0; s.kf = RD_DROP | (q < t.len ? 0u : RD_F_END); return s; }
  s.nb0 = fq_nb(t, d0); s.n = fq_nb(t, q) - s.nb0;
  if (q < t.len && t.text[q] == '+') {
    const uint64_t e1 = fq_find_byte(t, q + 1, true), q0 = e1 < t.len ? e1 + 1 : t.len, nb1 = fq_nb(t, q0);
    uint64_t x = t.len;
    uint32_t link_x = (uint32_t)sink;
    if (all - nb1 >= s.n) {
      const uint64_t r = s.n ? fq_nb_reach(t, q0, nb1 + s.n) : q0, lo = r > q0 + 1 ? r : q0 + 1;
      if (lo < t.len) { x = fq_cand_from(t, ci, lo); if (x < t.len) link_x = (uint32_t)(ci + 1); }
    }
    const uint64_t m = fq_nb(t, x) - nb1;
    s.q0 = q0; s.q1 = x; s.nbq = nb1; s.link = link_x;
    s.kf = RD_FASTQ | (m != s.n ? RD_F_QLEN : 0u) | (x < t.len ? 0u : RD_F_END);
    return s;
  }
  s.kf = RD_FASTA | (q < t.len ? 0u : RD_F_END);
  return s;
}

// the number of jump tables: the smallest L with 2^L >= nodes
SMG_HD inline uint32_t rd_levels(uint64_t nodes) { uint32_t l = 0; while (l < 63 && (1ull << l) < nodes) l++; return l; }

// is the node a record the batch takes?  idx: the marked records in front of it
SMG_HD inline bool rd_taken(uint32_t kf, bool marked, uint64_t node, uint64_t idx, uint32_t stop_node, uint32_t max_reads) {
  return marked && rd_is_record(kf) && node < stop_node && (!max_reads || idx < max_reads);
}
SMG_HD inline RdRec rd_record(const RdStep &s, uint64_t base_off) {
  RdRec r;
  r.hdr_off = s.hdr_off; r.d0 = s.d0; r.d1 = s.d1; r.q0 = s.q0; r.q1 = s.q1; r.base_off = base_off; r.nb0 = s.nb0; r.nbq = s.nbq;
  return r;
}

// the records of [lo, hi) whose data begins at or in front of x, plus lo
SMG_HD inline uint64_t rd_rec_upper(const RdRec *rec, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (rec[mid].d0 <= x) lo = mid + 1; else hi = mid; }
  return lo;
}
// A lane's bytes text[o, o + n) (c: a copy), nb: the non-blank bytes of the text in front of o.  Bases and quality characters of
// the records taken go to their places; nothing is written at or behind `total`.  quals: nullptr without qualities.
SMG_HD inline void rd_emit_lane(const uint8_t *c, uint32_t n, uint64_t o, uint64_t nb, const RdRec *rec, uint64_t nrec, uint8_t *bases, uint8_t *quals,
                                uint64_t total) {
  if (!n || !nrec) return;
  uint64_t u = rd_rec_upper(rec, 0, nrec, o);
  RdRec cur;
  cur.hdr_off = cur.d0 = cur.d1 = cur.q0 = cur.q1 = cur.base_off = cur.nb0 = cur.nbq = 0;
  if (u > 0) cur = rec[u - 1];
  uint64_t next_d0 = u < nrec ? rec[u].d0 : ~0ull;
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t x = o + i;
    while (next_d0 <= x) { cur = rec[u]; u++; next_d0 = u < nrec ? rec[u].d0 : ~0ull; }      // u only moves up
    if (fa_isspace(c[i])) continue;
    if (x >= cur.d0 && x < cur.d1) { const uint64_t at = cur.base_off + (nb - cur.nb0); if (at < total) bases[at] = rd_canon(c[i]); }
    else if (quals && x >= cur.q0 && x < cur.q1) { const uint64_t at = cur.base_off + (nb - cur.nbq); if (at < total) quals[at] = c[i]; }
    nb++;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// the first word of the header line whose prompt is at p (readHeader: white space behind the prompt is skipped up to the '\n')
inline std::string rd_name(const char *text, uint64_t len, uint64_t p) {
  uint64_t i = p + 1;
  while (i < len && text[i] != '\n' && fa_isspace((uint8_t)text[i])) i++;
  const uint64_t a = i;
  while (i < len && !fa_isspace((uint8_t)text[i])) i++;
  return std::string(text + a, (size_t)(i - a));
}
// the message of general_parse for the node the batch stopped at with an error
inline std::string rd_error_text(uint32_t kf, const char *text, uint64_t len, uint64_t hdr_off) {
  if (rd_kind(kf) == RD_NOPROMPT) return "not in FASTA/FASTQ format (a header line was expected)";
  return "sequence and quality string differ in length (read '" + rd_name(text, len, hdr_off) + "')";
}
// view->consumed of smaltgpu_reads_parse.  rec_end: the offset behind the last record taken
inline uint64_t rd_consumed(uint64_t len, bool is_last, uint32_t max_reads, uint64_t nreads, uint64_t rec_end) {
  if (!is_last) return nreads ? rec_end : 0;
  return (max_reads && nreads == max_reads) ? rec_end : len;
}

}  // namespace smg

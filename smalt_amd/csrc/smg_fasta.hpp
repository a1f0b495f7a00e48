// smg_fasta.hpp -- the automaton that turns the text of a FASTA reference into bases, sequence offsets and names, stated once
// for the kernels of smg_fasta.hip and for a host build (tests/hostemu/fasta_check.cpp).
//
// The reference reads a reference file record by record: readHeader (sequence.c:1056-1146) takes a header line, readSeqFast
// (sequence.c:1229-1304) takes text up to a prompt that stands directly behind a newline.  As one automaton over the bytes:
//   P   waiting for the first prompt: white space is skipped, '>' (or '@', '+') opens a header, anything else is
//       the reference's "wrong FASTQ/FASTA format";
//   H   in a header line: everything up to the next '\n'; behind it the state is S0 (readSeqFast starts with
//       was_newline = FALSE: a header line directly behind a header line is sequence data);
//   S0  in sequence data, not directly behind a '\n': white space is dropped ('\n' -> S1), every other byte is a base;
//   S1  in sequence data, directly behind a '\n': a prompt opens the next header, other white space -> S0 (so "\n >x" is
//       sequence data), any other byte is a base (-> S0);
//   E   the text did not begin with a prompt (absorbing).
// A finite-state transducer: a stretch of text maps every entry state to an exit state, a number of bases and a number of headers,
// and such maps compose.  That is what lets blocks of text be processed without knowing where they stand (smg_fasta.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "smg_common.h"
#if defined(__HIPCC__)
#include "smg_devmem.hpp"
#endif

namespace smg {

enum : uint32_t { FA_P = 0, FA_H = 1, FA_S0 = 2, FA_S1 = 3, FA_E = 4, FA_NSTATE = 5, FA_NENTRY = 4 /* a stretch is never entered in E with work left */ };
enum : uint32_t { FA_EMIT = 8 /* the byte is a base */, FA_HDR = 16 /* the byte is a prompt that opens a header */, FA_FQ = 32 /* ... a FASTQ prompt ('@', '+') */ };
enum : uint32_t { FA_LANE_BYTES = 16 /* bytes a lane takes in one step (one 128-bit load) */, FA_TILE = 256 * FA_LANE_BYTES /* bytes a workgroup takes in one step */,
                  FA_BLOCK_MIN = 64, FA_BLOCK_DEFAULT = 256u << 10, FA_BLOCK_MAX = 1u << 30 };

// a row of the transition table: 6 bits per state (next state | FA_EMIT | FA_HDR | FA_FQ), state s at bit 6 * s
#define SMG_FA_ROW(p, h, s0, s1) ((uint32_t)(p) | (uint32_t)(h) << 6 | (uint32_t)(s0) << 12 | (uint32_t)(s1) << 18 | (uint32_t)FA_E << 24)
enum : uint32_t {
  FA_ROW_NL = SMG_FA_ROW(FA_P, FA_S0, FA_S1, FA_S1),                                                        // '\n'
  FA_ROW_WS = SMG_FA_ROW(FA_P, FA_H, FA_S0, FA_S0),                                                         // other white space (isspace)
  FA_ROW_GT = SMG_FA_ROW(FA_H | FA_HDR, FA_H, FA_S0 | FA_EMIT, FA_H | FA_HDR),                              // '>'
  FA_ROW_FQ = SMG_FA_ROW(FA_H | FA_HDR | FA_FQ, FA_H, FA_S0 | FA_EMIT, FA_H | FA_HDR | FA_FQ),              // '@', '+'
  FA_ROW_BASE = SMG_FA_ROW(FA_E, FA_H, FA_S0 | FA_EMIT, FA_S0 | FA_EMIT)                                    // everything else
};

SMG_HD inline bool fa_isspace(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }       // isspace() of the C locale
SMG_HD inline uint32_t fa_row(uint8_t c) {
  return c == '\n' ? FA_ROW_NL : fa_isspace(c) ? FA_ROW_WS : c == '>' ? FA_ROW_GT : (c == '@' || c == '+') ? FA_ROW_FQ : FA_ROW_BASE;
}
// one byte in one state: next state | flags
SMG_HD inline uint32_t fa_step(uint32_t state, uint32_t row) { return (row >> (6 * state)) & 63u; }

// A map over the states: 3 bits per entry state, entry e at bit 3 * e; E maps to E.
enum : uint32_t { FA_MAP_ID = FA_P | FA_H << 3 | FA_S0 << 6 | FA_S1 << 9 | FA_E << 12 };
SMG_HD inline uint32_t fa_map_at(uint32_t map, uint32_t e) { return (map >> (3 * e)) & 7u; }
// first f, then g
SMG_HD inline uint32_t fa_map_compose(uint32_t f, uint32_t g) {
  uint32_t r = FA_E << 12;
  for (uint32_t e = 0; e < FA_NENTRY; e++) r |= fa_map_at(g, fa_map_at(f, e)) << (3 * e);
  return r;
}

// What a lane knows about its (at most FA_LANE_BYTES) bytes before it knows its entry state: for each of the four entry states the
// exit state (map), the number of bases (nb, 8 bits per entry state) and of headers opened (nh, likewise).
struct FaLane { uint32_t map, nb, nh; };
SMG_HD inline void fa_lane_init(FaLane &l) { l.map = FA_MAP_ID; l.nb = 0; l.nh = 0; }
SMG_HD inline void fa_lane_byte(FaLane &l, uint8_t c) {
  const uint32_t row = fa_row(c);
  uint32_t m = FA_E << 12;
  for (uint32_t e = 0; e < FA_NENTRY; e++) {
    const uint32_t t = fa_step(fa_map_at(l.map, e), row);
    m |= (t & 7u) << (3 * e);
    l.nb += ((t >> 3) & 1u) << (8 * e);
    l.nh += ((t >> 4) & 1u) << (8 * e);
  }
  l.map = m;
}
SMG_HD inline uint32_t fa_lane_count(uint32_t packed, uint32_t e) { return e < FA_NENTRY ? (packed >> (8 * e)) & 255u : 0u; }

// The summary of a block of text (pass A): per entry state the exit state and the counts.
struct FaSummary { uint32_t map, nb[FA_NENTRY], nh[FA_NENTRY]; };
// Where a block stands once the summaries in front of it are composed: its entry state, the bases and the headers before it.
struct FaEntry { uint64_t base_off, hdr_off; uint32_t state, pad; };
// the running composition (compose step): `at` becomes the entry of the block behind `s`
SMG_HD inline void fa_entry_advance(FaEntry &at, const FaSummary &s) {
  if (at.state < FA_NENTRY) { at.base_off += s.nb[at.state]; at.hdr_off += s.nh[at.state]; }
  at.state = fa_map_at(s.map, at.state);
}
// a header found by pass B: where its prompt stands in the text, and how many bases precede it (the sequence's offset)
struct FaHeader { uint64_t text_off, base_off; };

// ---- host side: names, verdicts (plain C++) --------------------------------------------------------------------------------
// The name of a sequence (readHeader, sequence.c:1094-1133): the header line behind the prompt without leading white space, every
// run of white space cut down to its first character, one trailing white-space character dropped.  `p` points behind the prompt.
inline std::string fa_clean_name(const char *p, size_t n) {
  std::string nm;
  bool was_space = true;
  for (size_t i = 0; i < n && p[i] != '\n'; i++) {
    const bool sp = fa_isspace((uint8_t)p[i]);
    if (was_space && sp) continue;
    was_space = sp;
    nm.push_back(p[i]);
  }
  if (was_space && !nm.empty()) nm.pop_back();
  return nm;
}
// why a parse cannot be used (nullptr: it can).  final_state: the state behind the last byte
inline const char *fa_refusal(uint64_t text_len, uint32_t final_state, uint64_t nheaders, uint64_t nfastq) {
  if (text_len == 0) return "the reference file is empty";
  if (final_state == FA_E) return "wrong FASTQ/FASTA format: the text does not begin with a '>' prompt";
  if (nfastq) return "FASTQ-format reference files are not supported ('@' or '+' prompt at the beginning of a line): convert the reference to FASTA";
  if (nheaders == 0) return "the reference file holds no sequence (white space only)";
  return nullptr;
}
inline uint32_t fa_block_bytes(const char *env) {       // SMALTGPU_FASTA_BLOCK: bytes of text per workgroup, a multiple of 64
  uint64_t v = FA_BLOCK_DEFAULT;
  if (env && *env) { const long long x = atoll(env); if (x > 0) v = (uint64_t)x; }
  v = (v + 63) / 64 * 64;
  return (uint32_t)(v < FA_BLOCK_MIN ? FA_BLOCK_MIN : v > FA_BLOCK_MAX ? FA_BLOCK_MAX : v);
}

#if defined(__HIPCC__)
// The parse on the device (smg_fasta.hip).  text: host memory.  d_bases receives the bases and goes with the FastaParsed;
// seq_off gets nseq + 1 entries; hdr_text_off the offset of each header's prompt in the text.  block_bytes: fa_block_bytes().
struct FastaParsed {
  DevMem<uint8_t> d_bases;
  uint64_t nbases = 0;
  std::vector<uint64_t> seq_off, hdr_text_off;
  float upload_ms = 0, pass_a_ms = 0, compose_ms = 0, pass_b_ms = 0;
  // in: a text refused for its '@' / '+' prompts is left in HBM (d_text, padded to a multiple of FA_TILE) for the reader of
  // smg_fastq_ref.hpp, which takes it from here
  bool keep_fastq_text = false;
  DevMem<uint8_t> d_text;
};
int fasta_parse_device(const char *text, uint64_t text_len, uint32_t block_bytes, FastaParsed *out, char *err, size_t errlen);
#endif

}  // namespace smg

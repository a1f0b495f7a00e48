// smg_alnin.cpp -- the C ABI of the SAM / BAM reader (smalt map -F sam|bam): smg_alnin.hpp holds the rules and the work, this file
// the entry points of include/smaltgpu.h.  Host code only.
#include <new>

#include "../../include/smaltgpu.h"
#include "smg_alnin.hpp"

extern "C" int smaltgpu_set_error(int code, const char *msg);   // smaltgpu.cpp: the per-thread message of smaltgpu_last_error()

struct smaltgpu_alnreads {
  smgaln::Reader rd;
};

namespace {

int report(const smgaln::Reader &rd) { return smaltgpu_set_error(rd.err_code == smgaln::BAD_ARG ? SMALTGPU_EARG : SMALTGPU_EFILE, rd.err.c_str()); }

void fill(smaltgpu_reads_view *v, smgaln::Side &s, uint32_t n, bool has_qual) {
  if (s.bases.empty()) s.bases.push_back(0);
  v->nreads = n;
  v->has_qual = has_qual && n ? 1u : 0u;
  v->bases = s.bases.data();
  v->quals = v->has_qual ? s.quals.data() : nullptr;
  v->read_off = s.off.data();
  v->names = s.names.data();
  v->name_off = s.name_off.data();
  v->consumed = 0;
}

}  // namespace

extern "C" smaltgpu_alnreads *smaltgpu_alnreads_create(int format) {
  if (format != SMALTGPU_IN_SAM && format != SMALTGPU_IN_BAM) { smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_alnreads_create: the format is SMALTGPU_IN_SAM or SMALTGPU_IN_BAM"); return nullptr; }
  smaltgpu_alnreads *r = new (std::nothrow) smaltgpu_alnreads();
  if (!r) { smaltgpu_set_error(SMALTGPU_ENOMEM, "smaltgpu_alnreads_create: out of memory"); return nullptr; }
  r->rd.format = format == SMALTGPU_IN_SAM ? smgaln::FMT_SAM : smgaln::FMT_BAM;
  return r;
}

extern "C" void smaltgpu_alnreads_free(smaltgpu_alnreads *r) { delete r; }

extern "C" int smaltgpu_alnreads_feed(smaltgpu_alnreads *r, const char *bytes, uint64_t len, int is_last, int nthreads, uint64_t *consumed) {
  if (!r || !consumed || (!bytes && len)) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_alnreads_feed: null argument");
  if (r->rd.feed(bytes, len, is_last != 0, nthreads, consumed)) return report(r->rd);
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_alnreads_take(smaltgpu_alnreads *r, uint32_t max_templates, int *kind, smaltgpu_reads_view *reads, smaltgpu_reads_view *mates) {
  if (!r || !kind || !reads || !mates) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_alnreads_take: null argument");
  if (r->rd.err_code) return report(r->rd);
  const uint32_t n = r->rd.take(max_templates, kind);
  if (r->rd.side[1].names.empty()) r->rd.side[1].names.push_back(0);
  if (r->rd.side[0].names.empty()) r->rd.side[0].names.push_back(0);
  fill(reads, r->rd.side[0], n, r->rd.run_has_qual);
  fill(mates, r->rd.side[1], *kind == 2 ? n : 0, r->rd.run_has_qual);
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_alnreads_times(const smaltgpu_alnreads *r, double *inflate_s, double *decode_s, double *take_s) {
  if (!r) return smaltgpu_set_error(SMALTGPU_EARG, "smaltgpu_alnreads_times: null argument");
  if (inflate_s) *inflate_s = r->rd.sec_inflate;
  if (decode_s) *decode_s = r->rd.sec_decode;
  if (take_s) *take_s = r->rd.sec_take;
  return SMALTGPU_OK;
}

// smg_mapper.hpp -- what the two host translation units of the C ABI share: smaltgpu.cpp (index, mapper, pipeline, fetch, remap)
// and smg_entries.cpp (the stand-alone entries of single kernels and stages, for tests).  Private to the library: the helpers
// declared here keep hidden visibility, the exported symbols are those of include/smaltgpu.h alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/smaltgpu.h"
#include "smg_kernels.h"

extern "C" int smaltgpu_set_error(int code, const char *msg);      // keeps the text for smaltgpu_last_error (smaltgpu.cpp)
#pragma GCC visibility push(hidden)
using namespace smg;

static int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return smaltgpu_set_error(code, buf);
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(SMALTGPU_ENODEV, "%s: %s", #x, hipGetErrorString(e_)); } while (0)
#define TRY(x) do { const int rv_ = (x); if (rv_) return rv_; } while (0)      // x: a call that has reported its failure through fail

// Device memory with an owner.  The mapper's per-round context buffers grow on demand (ensure); the buffers of a test entry are
// sized exactly, live for one call (alloc, fill, get) and go with the scope, on every return.  n counts elements.
template <class T> struct DevBuf {
  T *p = nullptr; size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int ensure(size_t n) {                                             // at least n, with headroom
    if (n <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t bytes = n * sizeof(T) + n * sizeof(T) / 2 + 256;
    if (hipMalloc((void **)&p, bytes) != hipSuccess) return fail(SMALTGPU_ENOMEM, "device memory");
    cap = bytes / sizeof(T);
    return 0;
  }
  int alloc(size_t n, const T *host = nullptr, size_t ncopy = 0) {    // exactly n (at least one), the first ncopy from the host
    if (hipMalloc((void **)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) return fail(SMALTGPU_ENOMEM, "device memory");
    cap = n ? n : 1;
    if (ncopy) HIPCHK(hipMemcpy(p, host, ncopy * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }
  int fill(int byte) { HIPCHK(hipMemset(p, byte, cap * sizeof(T))); return 0; }      // the whole allocation
  int get(T *host, size_t n) const { if (n) HIPCHK(hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost)); return 0; }
};

struct smaltgpu_index {
  DevIndex d;
  int device = 0;
  bool owns = true;
  std::vector<uint64_t> sop;       // host copy
  void *bufs[8] = {nullptr};
  int nbufs = 0;
  std::vector<std::string> names;  // set by smaltgpu_index_build (what smaltgpu_index_save writes)
  uint32_t maxpos = 0;
  bool built = false;
  std::vector<const char *> name_ptrs;  // smaltgpu_index_seqnames
  std::vector<uint32_t> packed_host;   // host copy of the packed reference, fetched on first request (smaltgpu_index_packed_host)
  std::mutex packed_mu;
};

enum { T_ENCODE = 0, T_SEED, T_HITS, T_CANDS, T_SW_FULL, T_SW_SCALAR, T_REPLAY, T_ALIGN, T_NUM };

struct smaltgpu_mapper {
  const smaltgpu_index *ix = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t max_reads = 0, max_len = 0, qmax = 0;
  uint64_t max_bases = 0;
  // device buffers: every allocation of smaltgpu_mapper_create_ex is recorded in `owned`, which smaltgpu_mapper_free walks
  std::vector<void *> owned;
  uint8_t *d_bases = nullptr, *d_quals = nullptr, *d_codes = nullptr, *d_codes_rc = nullptr;
  uint64_t *d_off = nullptr;
  uint32_t *d_ids = nullptr;                  // read ids of a round gathered from resident batches (smaltgpu_map_batch_ctx_resident)
  uint32_t hits_W = 0, hits_wg = 0;          // k_hits: keys per window, workgroups (0: S3 stays inside k_cands)
  bool hits_ran = false;                     // the last call launched k_hits (smaltgpu_hits_windows)
  uint32_t hits_fill = 0;                    // k_hits: fill target of a window (HitsScratch::fill)
  uint32_t *b_hitwin = nullptr;               // windows per strand (Batch::hitwin), allocated with the run table
  HitRun *b_hitrun = nullptr;                 // the run table; Batch::hitrun is set per call (begin_call): null where k_hits does not run
  Batch b;
  // Counters of a batch, one 128-byte line each: atomics on one line are served one after the other (2 ns each), and the pool cursors,
  // the work-queue cursors of the persistent kernels and the retry counts used to share the first line.
  enum : size_t { CT_LINE = 128, CT_RC = 0, CT_RES = 1 * CT_LINE, CT_DSTR = 2 * CT_LINE, CT_ERR = 3 * CT_LINE, CT_NEXT = 4 * CT_LINE /* 5 lines */,
                  CT_ALIGN_RETRY = 9 * CT_LINE, CT_CANDS_RETRY = 10 * CT_LINE, CT_HITS = 11 * CT_LINE, CT_HITS_CURSOR = 12 * CT_LINE, CT_STRIP_CURSOR = 13 * CT_LINE,
                  CT_WORK = 14 * CT_LINE /* 32 x 8 bytes */, CT_BYTES = 16 * CT_LINE };
  uint8_t *d_counters = nullptr;
  double *d_logtab = nullptr; uint32_t logtab_n = 0;     // log(n), n <= max_len, for the complexity-weighted scores (SMALTGPU_FLG_CMPLXW; smg_cplx.hpp)
  uint8_t *seed_scr = nullptr; size_t seed_bytes = 0; uint32_t seed_slots = 0;
  uint8_t *cand_scr = nullptr; size_t cand_bytes = 0; uint32_t cand_slots = 0;
  CandGeom cg2; uint8_t *cand_scr2 = nullptr; size_t cand_bytes2 = 0; uint32_t cand_slots2 = 0;   // second pass of the candidate stage: full-size slots
  CandGeom cg;
  uint8_t *cand_scr_dbg = nullptr; uint32_t cand_dbg_reads = 0;      // debug batches: grown by run_pipeline, not in `owned`
  int *sw_rows = nullptr; uint32_t sw_rowlen = 0, sw_threads = 0;
  void *strip_bnd = nullptr; uint8_t *strip_win = nullptr; uint32_t strip_grid = 0;   // k_sw_strip: boundary columns + decoded window per workgroup
  uint32_t full_grid = 8192;                          // workgroups (one wave each) of the register-tiled K2a kernels
  uint8_t *align_scr = nullptr; size_t align_bytes = 0; uint32_t align_slots = 0;
  uint8_t *align_scr2 = nullptr; size_t align_bytes2 = 0; uint32_t align_slots2 = 0; uint64_t dircap2 = 0;   // second K3 pass: few slots with full-size direction matrices
  uint32_t wincap = 0, rescap_slot = 0, dstrcap_slot = 0; uint64_t dircap = 0;
  uint32_t rescap_slot2 = 0, dstrcap_slot2 = 0;       // result slots of the second K3 pass (reads with more alignments than a first-pass slot holds)
  // host mirrors
  // results come back through pinned host memory: the copies are asynchronous, so the next batch can be launched
  // behind them (smaltgpu_fetch_begin / _end)
  template <class T> struct Pinned {
    T *p = nullptr; size_t cap = 0;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    int ensure(size_t n) {
      if (n <= cap) return 0;
      size_t c = cap ? cap : 1024;
      while (c < n) c += c / 2 + 1;
      T *q = nullptr;
      if (hipHostMalloc((void **)&q, c * sizeof(T), hipHostMallocDefault) != hipSuccess) return -1;
      if (p) (void)hipHostFree(p);
      p = q; cap = c;
      return 0;
    }
    T *data() { return p; }
    T &operator[](size_t i) { return p[i]; }
  };
  Pinned<ReadStat> h_stat;
  Pinned<Result> h_res;
  Pinned<uint8_t> h_dstr;
  hipEvent_t ev_fetch = nullptr;
  uint32_t fetch_n = 0; uint64_t fetch_nres = 0; bool fetch_open = false, pool_overflow = false;
  // smaltgpu_map_batch after a pool overflow: results of the whole batch assembled from several device batches
  std::vector<smaltgpu_result> fin_res; std::vector<uint8_t> fin_dstr; std::vector<smaltgpu_readstat> fin_stat; std::vector<uint64_t> fin_off;
  std::vector<uint64_t> h_res_off;
  std::vector<smaltgpu_result> o_res;
  std::vector<smaltgpu_readstat> o_stat;
  std::vector<uint64_t> h_off;              // read offsets of the last batch (host copy)
  uint32_t last_n = 0;
  MapPar last_par;
  bool have_host_off = false;
  int debug = 0;
  // per-read context of rmapPair's rounds (smaltgpu_map_batch_ctx): device copies, grown on demand
  DevBuf<uint32_t> cx_ivoff, cx_fineidx, cx_finepos, cx_fineoff, cx_alloclen, cx_seedrange;
  DevBuf<IvRec> cx_iv;
  DevBuf<int32_t> cx_minsw, cx_prevmax;
  int host_threads = 1;                      // smaltgpu_mapper_set_host_threads
  bool history = false;                      // serial-order mode (smaltgpu_mapper_set_history)
  uint32_t hist_longest = 0;                 // longest read of length >= k of the run so far
  std::vector<uint32_t> h_alloclen;
  std::vector<uint32_t> h_ivoff, h_fineoff, h_finepos, h_fineidx;      // (the last two: host copies for smaltgpu_fine_index_batch, test entry)
  std::vector<HitInfoHdr> h_hi;
  bool last_fine = false;
  uint64_t remap_batches = 0;               // device batches smaltgpu_map_batch ran to recover from pool overflows (diagnostic)
  // host copies of what k_hits left behind (smaltgpu_hits_batch, test entry)
  struct HitsHost { std::vector<HitInfoHdr> hi; std::vector<uint32_t> n_seeds, seed_rank, status; std::vector<SeedRec> seeds; std::vector<uint8_t> qmask;
                    std::vector<HitRun> runs; std::vector<uint64_t> pool; } hh;
  std::vector<ReadCtl> h_ctl;               // what k_replay left behind (smaltgpu_align_cands_batch, test entry)
  std::vector<RCand> h_pool;                // the candidate pool behind the score stage (smaltgpu_score_pool, test entry)
  hipEvent_t ev[T_NUM + 1] = {nullptr};
  double ms[T_NUM] = {0};
  unsigned long long work[WK_NWORK] = {0};
};

// the per-read context of one of rmapPair's rounds on the device (upload_ctx), or all null: a plain call
struct CtxDev { const uint32_t *iv_off; const IvRec *iv; const int32_t *min_sw, *prevmax; uint32_t *fine_idx, *fine_pos; const uint32_t *fine_off, *alloc_len, *seed_range; uint32_t raw; };

// One optional per-read array of a context (`per` values for each of n reads) into its device buffer, on the mapper's stream.
template <class T>
static int upload_per_read(smaltgpu_mapper *m, DevBuf<T> &buf, const T *host, uint32_t n, uint32_t per, const T **dev) {
  TRY(buf.ensure((size_t)(n ? n : 1) * per));
  if (n) HIPCHK(hipMemcpyAsync(buf.p, host, (size_t)n * per * sizeof(T), hipMemcpyHostToDevice, m->stream));
  *dev = buf.p;
  return 0;
}

// The steps of a call that the pipeline and the entries of smg_entries.cpp share (smaltgpu.cpp).
MapPar to_par(const smaltgpu_params *p);
int check_par(const smaltgpu_mapper *m, const smaltgpu_params *p);
// reads in host memory to d_bases / d_quals / d_off and h_off: offsets rebased to 0, every read checked against max_read_len
int stage_reads(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads);
// the round's reads gathered on the device from two resident batches
int gather_round(smaltgpu_mapper *m, const smaltgpu_resident_reads *src, const uint32_t *ids, uint32_t nreads, bool *with_quals);
// the context of a round to the device; fills cd
int upload_ctx(smaltgpu_mapper *m, const smaltgpu_callctx *ctx, uint32_t n, CtxDev *cd);
// the per-call fields of m->b and of the mapper for n staged reads, counters zeroed on the stream; *p: the call's parameters
int begin_call(smaltgpu_mapper *m, const uint8_t *d_quals, const uint64_t *d_off, uint32_t n, const smaltgpu_params *par, const CtxDev *cx,
               bool totals_only, MapPar *p);
#pragma GCC visibility pop

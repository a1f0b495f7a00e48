// smg_reads_dev.hip -- a chunk of a read file (FASTQ / FASTA text) parsed in HBM into the batch layout of smaltgpu_map_batch_device
// (the rules and the four steps: smg_reads_dev.hpp).  The launches of one parse, all on the handle's stream, none of which waits
// for another workgroup:
//   k_fq_count, k_fq_scan, k_fq_cands   candidates and non-blank prefix counts, the kernels of smg_fastq_ref.hip;
//   k_rd_step     one wave per node: rd_step, and the node's entry of the first jump table;
//   k_rd_double   one launch per further jump table: J_r = J_(r-1) o J_(r-1);
//   k_rd_mark     one launch per table, from the highest down: a marked node marks J_r of itself;
//   k_rd_sums     per tile of RD_NODE_TILE nodes the marked records and their bases, and the first node the batch stops at;
//   k_fq_scan     the tile sums become exclusive prefixes;
//   k_rd_number   every record taken gets its index and the offset of its bases: the record table, read_off, the header offsets;
//   k_rd_emit     one workgroup per block of text: bases and quality characters go to their places.
// With L = rd_levels(ncand + 1) that is 2 L + 7 launches (L - 1 doublings, L markings; 8 for a text without candidates).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/smaltgpu.h"
#include "smg_devmem.hpp"
#include "smg_reads_dev.hpp"
#include "smg_text.hpp"

extern "C" int smaltgpu_set_error(int code, const char *msg);   // smaltgpu.cpp

namespace smg {

// one wave per node; the waves of the grid stride over the nodes
__global__ void __launch_bounds__(256) k_rd_step(FqText t, uint64_t nn, RdStep *step, uint32_t *jump0) {
  const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (uint64_t)gridDim.x * 4;
  for (uint64_t v = wave; v < nn; v += nwave) {
    RdStep s = rd_step(t, v);
    if (s.link <= v || s.link > nn) s.link = (uint32_t)nn;                       // links point forward, whatever the text is
    if (fq_lane0()) { step[v] = s; jump0[v] = s.link; }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) jump0[nn] = (uint32_t)nn;             // the sink
}

// tables of nn + 1 entries
__global__ void __launch_bounds__(256) k_rd_double(const uint32_t *prev, uint32_t *next, uint64_t n1) {
  for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < n1; v += (uint64_t)gridDim.x * 256) {
    const uint32_t a = prev[v];
    next[v] = a < n1 ? prev[a] : (uint32_t)(n1 - 1);
  }
}

// mark: nn + 1 bytes, the sink's is never read.  Only nodes of the path are ever marked, so a node marked in this round by another
// thread may or may not pass its mark on in the same round: either is right.
__global__ void __launch_bounds__(256) k_rd_mark(const uint32_t *jump, uint8_t *mark, uint64_t nn) {
  for (uint64_t v = (uint64_t)blockIdx.x * 256 + threadIdx.x; v < nn; v += (uint64_t)gridDim.x * 256) {
    if (mark[v]) { const uint32_t a = jump[v]; if (a < nn) mark[a] = 1; }
  }
}

__global__ void __launch_bounds__(256) k_rd_sums(const RdStep *step, const uint8_t *mark, uint64_t nn, uint64_t ntile, int is_last, uint64_t *part_c, uint64_t *part_b,
                                                 RdSum *sum) {
  __shared__ TxPair wsum[4];
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t v = tile * RD_NODE_TILE + threadIdx.x;
    TxPair x = {0, 0}, tot;                                                    // records, bases
    if (v < nn && mark[v]) {
      const uint32_t kf = step[v].kf;
      if (rd_is_record(kf)) { x.a = 1; x.b = step[v].n; }
      if (rd_stops(kf, is_last != 0)) atomicMin(&sum->stop_node, (uint32_t)v);
    }
    tx_block_scan_sum(x, wsum, &tot);
    if (threadIdx.x == 0) { part_c[tile] = tot.a; part_b[tile] = tot.b; }
  }
}

// rec, read_off, hdr_off: room for nn records (read_off: nn + 1); read_off[0] is set by the caller
__global__ void __launch_bounds__(256) k_rd_number(const RdStep *step, const uint8_t *mark, uint64_t nn, uint64_t ntile, uint32_t max_reads, const uint64_t *part_c,
                                                   const uint64_t *part_b, RdSum *sum, RdRec *rec, uint64_t *read_off, uint64_t *hdr_off) {
  __shared__ TxPair wsum[4];
  const uint32_t stop_node = sum->stop_node;                                   // k_rd_sums is over
  for (uint64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const uint64_t v = tile * RD_NODE_TILE + threadIdx.x;
    const bool marked = v < nn && mark[v];
    RdStep s;
    s.kf = RD_DROP; s.n = 0;
    if (marked) s = step[v];
    const bool r = marked && rd_is_record(s.kf);
    TxPair tot;
    const TxPair pre = tx_block_scan_sum(TxPair{r ? 1u : 0u, r ? s.n : 0}, wsum, &tot);       // the tile's records and bases in front of the node
    const uint64_t idx = part_c[tile] + pre.a, off = part_b[tile] + pre.b;
    if (marked && v == stop_node) { sum->stop_kf = s.kf; sum->stop_idx = idx; sum->stop_hdr_off = s.hdr_off; }
    if (rd_taken(s.kf, marked, v, idx, stop_node, max_reads) && idx < nn) {
      rec[idx] = rd_record(s, off); read_off[idx + 1] = off + s.n; hdr_off[idx] = s.hdr_off;
      atomicMax(&sum->nreads, (uint32_t)(idx + 1));
      if (rd_kind(s.kf) == RD_FASTA) atomicOr(&sum->any_fasta, 1u);
    }
  }
}

__global__ void __launch_bounds__(256) k_rd_emit(const uint8_t *text, uint64_t len, uint32_t block_bytes, const uint64_t *blk_nb, const RdRec *rec, uint64_t nrec,
                                                 uint8_t *bases, uint8_t *quals, uint64_t total) {
  __shared__ uint32_t wsum[4];
  const auto [b0, b1] = tx_block_range(len, block_bytes);
  uint64_t run_nb = blk_nb[blockIdx.x];                                        // the non-blank bytes in front of the tile; the same in every thread
  for (uint64_t t0 = b0; t0 < b1; t0 += FA_TILE) {
    uint8_t c[FA_LANE_BYTES];
    uint64_t o;
    const uint32_t n = tx_lane_load(text, t0, b1, &o, c);
    uint32_t tot;
    const uint32_t pre = tx_block_scan_sum(fq_lane_counts(c, n, 0) & 0xFFFFu, wsum, &tot);
    rd_emit_lane(c, n, o, run_nb + pre, rec, nrec, bases, quals, total);
    run_nb += tot;
  }
}

}  // namespace smg

using namespace smg;

// ---- the handle ------------------------------------------------------------------------------------------------------------
struct smaltgpu_reads_dev {
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t block_bytes = RD_BLOCK_DEFAULT, max_groups = RD_GROUPS_DEFAULT, guard = 0;
  // scratch, sized from len and ncand; every allocation only grows (DevMem::need) and goes with the handle
  DevMem<uint8_t> text, mark; DevMem<uint32_t> gran, jump; DevMem<uint64_t> blk_nb, blk_cd, cand, part_c, part_b, hdr;
  DevMem<RdStep> step; DevMem<RdRec> rec; DevMem<RdSum> sum;
  // the device view
  DevMem<uint8_t> bases, quals; DevMem<uint64_t> read_off;
  size_t exact[3] = {0, 0, 0};           // bytes of the three arrays of the last parse (the guard lies behind them)
  // the host view
  std::vector<uint8_t> h_bases, h_quals;
  std::vector<uint64_t> h_off, h_name_off, h_hdr;
  std::vector<char> h_names;
  uint32_t launches = 0;
};

#define RD_HIP(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) { char b_[256]; hip_error_text(b_, sizeof(b_), #x, e_); \
                       return smaltgpu_set_error(e_ == hipErrorOutOfMemory ? SMALTGPU_ENOMEM : SMALTGPU_ENODEV, b_); } } while (0)

extern "C" smaltgpu_reads_dev *smaltgpu_reads_dev_create(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { smaltgpu_set_error(SMALTGPU_ENODEV, "no such HIP device"); return nullptr; }
  if (hipSetDevice(device) != hipSuccess) { smaltgpu_set_error(SMALTGPU_ENODEV, "hipSetDevice failed"); return nullptr; }
  smaltgpu_reads_dev *h = new smaltgpu_reads_dev();
  h->device = device;
  // the greatest priority the device has: a parse is some forty short launches, and behind the mapping kernels of the same device
  // (smaltgpu-map parses the next block while the last ones are mapped) each of them would wait for a turn
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
  if (hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, greatest) != hipSuccess) { delete h; smaltgpu_set_error(SMALTGPU_ENODEV, "hipStreamCreate failed"); return nullptr; }
  return h;
}

extern "C" void smaltgpu_reads_dev_free(smaltgpu_reads_dev *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  delete h;
}

extern "C" int smaltgpu_reads_dev_configure(smaltgpu_reads_dev *h, uint32_t block_bytes, uint32_t max_groups, uint32_t guard_bytes) {
  if (!h) return smaltgpu_set_error(SMALTGPU_EARG, "null argument");
  if (block_bytes && (block_bytes < FA_BLOCK_MIN || (block_bytes & 63u) || block_bytes > FA_BLOCK_MAX)) return smaltgpu_set_error(SMALTGPU_EARG, "bad block size");
  h->block_bytes = block_bytes ? block_bytes : RD_BLOCK_DEFAULT;
  h->max_groups = max_groups ? max_groups : RD_GROUPS_DEFAULT;
  h->guard = guard_bytes;
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_reads_dev_readback(smaltgpu_reads_dev *h, int which, void *dst, uint64_t cap, uint64_t *nbytes, uint32_t *launches) {
  if (!h || which < 0 || which > 2 || !dst || !nbytes) return smaltgpu_set_error(SMALTGPU_EARG, "bad argument");
  const void *src[3] = {h->bases.get(), h->quals.get(), h->read_off.get()};
  const size_t held[3] = {h->bases.bytes(), h->quals.bytes(), h->read_off.bytes()};
  const uint64_t n = h->exact[which] + h->guard;
  if (launches) *launches = h->launches;
  *nbytes = h->exact[which];
  if (!src[which] || n > held[which] || n > cap) return smaltgpu_set_error(SMALTGPU_EARG, "nothing to read back, or no room for it");
  RD_HIP(hipSetDevice(h->device));
  RD_HIP(hipStreamSynchronize(h->stream));
  RD_HIP(hipMemcpy(dst, src[which], n, hipMemcpyDeviceToHost));
  return SMALTGPU_OK;
}

static int rd_fill_views(smaltgpu_reads_dev *h, uint64_t len, int is_last, uint32_t max_reads, uint64_t nreads, uint64_t total, bool has_qual, uint64_t rec_end,
                         const char *text, smaltgpu_reads_view *hv, smaltgpu_reads_device_view *dv) {
  if (dv) {
    dv->d_bases = h->bases.get(); dv->d_quals = has_qual ? h->quals.get() : nullptr; dv->d_read_off = h->read_off.get();
    dv->nreads = (uint32_t)nreads; dv->has_qual = has_qual ? 1u : 0u; dv->total_bases = total;
    dv->consumed = rd_consumed(len, is_last != 0, max_reads, nreads, rec_end);
  }
  if (hv) {
    h->h_names.clear(); h->h_name_off.assign(1, 0);
    for (uint64_t i = 0; i < nreads; i++) {
      const std::string nm = rd_name(text, len, h->h_hdr[i]);
      h->h_names.insert(h->h_names.end(), nm.begin(), nm.end()); h->h_names.push_back('\0');
      h->h_name_off.push_back(h->h_names.size());
    }
    if (h->h_names.empty()) h->h_names.push_back(0);
    hv->nreads = (uint32_t)nreads; hv->has_qual = has_qual ? 1u : 0u;
    hv->bases = h->h_bases.data(); hv->quals = has_qual ? h->h_quals.data() : nullptr;
    hv->read_off = h->h_off.data(); hv->names = h->h_names.data(); hv->name_off = h->h_name_off.data();
    hv->consumed = rd_consumed(len, is_last != 0, max_reads, nreads, rec_end);
  }
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_reads_parse_device(smaltgpu_reads_dev *h, const char *text, uint64_t len, int is_last, uint32_t max_reads, smaltgpu_reads_view *hv,
                                           smaltgpu_reads_device_view *dv) {
  if (!h || (!text && len) || (!hv && !dv)) return smaltgpu_set_error(SMALTGPU_EARG, "null argument");
  if (hv) memset(hv, 0, sizeof(*hv));
  if (dv) memset(dv, 0, sizeof(*dv));
  RD_HIP(hipSetDevice(h->device));
  hipStream_t st = h->stream;
  TextBlocks g;
  if (!text_blocks(len, h->block_bytes, &g)) return smaltgpu_set_error(SMALTGPU_EARG, "the text is too long for one call");
  const uint32_t block = g.block_bytes;
  const uint64_t nblk = g.nblk, padded = g.padded;
  h->launches = 0;
  h->h_bases.assign(1, 0); h->h_quals.clear(); h->h_off.assign(1, 0); h->h_hdr.clear();
  h->exact[0] = h->exact[1] = 0; h->exact[2] = sizeof(uint64_t);
  const uint64_t zero = 0;
  if (!len) {                            // as the host parser: no reads, nothing consumed
    RD_HIP(h->bases.need(1 + h->guard)); RD_HIP(h->quals.need(1 + h->guard)); RD_HIP(h->read_off.need(1 + (h->guard + 7) / 8));
    if (h->guard) { RD_HIP(hipMemsetAsync(h->bases.get(), 0xA5, h->guard, st)); RD_HIP(hipMemsetAsync(h->quals.get(), 0xA5, h->guard, st)); RD_HIP(hipMemsetAsync(h->read_off.get(), 0xA5, 8 + h->guard, st)); }
    RD_HIP(hipMemcpyAsync(h->read_off.get(), &zero, sizeof(zero), hipMemcpyHostToDevice, st));
    RD_HIP(hipStreamSynchronize(st));
    return rd_fill_views(h, 0, is_last, max_reads, 0, 0, false, 0, text, hv, dv);
  }
  // candidates and prefix counts
  RD_HIP(h->text.need(padded));
  RD_HIP(h->gran.need(padded / FQ_GRAN));
  RD_HIP(h->blk_nb.need(nblk + 1));
  RD_HIP(h->blk_cd.need(nblk + 1));
  RD_HIP(h->sum.need(1));
  RD_HIP(hipMemcpyAsync(h->text.get(), text, len, hipMemcpyHostToDevice, st));
  RD_HIP(fq_launch_counts(st, h->text.get(), len, block, nblk, h->gran.get(), h->blk_nb.get(), h->blk_cd.get()));
  h->launches += 2;
  uint64_t tot[2] = {0, 0};
  RD_HIP(hipMemcpyAsync(&tot[0], h->blk_nb + nblk, 8, hipMemcpyDeviceToHost, st));
  RD_HIP(hipMemcpyAsync(&tot[1], h->blk_cd + nblk, 8, hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  if (tot[0] > len || tot[1] > len) return smaltgpu_set_error(SMALTGPU_EINTERNAL, "the counts of the text exceed its length");
  const uint64_t ncand = tot[1], nn = ncand + 1, ntile = (nn + RD_NODE_TILE - 1) / RD_NODE_TILE;
  if (nn >= 0x7fffffffull) return smaltgpu_set_error(SMALTGPU_EARG, "the text holds too many prompts for one call");
  const uint32_t L = rd_levels(nn), ntab = L ? L : 1;
  RD_HIP(h->cand.need(ncand + 1));
  RD_HIP(h->step.need(nn));
  RD_HIP(h->jump.need((size_t)ntab * (nn + 1)));
  RD_HIP(h->mark.need(nn + 1));
  RD_HIP(h->part_c.need(ntile + 1));
  RD_HIP(h->part_b.need(ntile + 1));
  RD_HIP(h->rec.need(nn));
  RD_HIP(h->hdr.need(nn));
  // the device view: no more bases than non-blank bytes, no more reads than nodes
  const size_t off_bytes = (size_t)(nn + 1) * sizeof(uint64_t);
  RD_HIP(h->bases.need((size_t)tot[0] + 1 + h->guard)); RD_HIP(h->quals.need((size_t)tot[0] + 1 + h->guard)); RD_HIP(h->read_off.need(nn + 1 + (h->guard + 7) / 8));
  if (h->guard) {                        // tests: the pattern lies everywhere, so whatever is written behind an array shows
    RD_HIP(hipMemsetAsync(h->bases.get(), 0xA5, (size_t)tot[0] + 1 + h->guard, st)); RD_HIP(hipMemsetAsync(h->quals.get(), 0xA5, (size_t)tot[0] + 1 + h->guard, st));
    RD_HIP(hipMemsetAsync(h->read_off.get(), 0xA5, off_bytes + h->guard, st));
  }
  if (ncand) { RD_HIP(fq_launch_cands(st, h->text.get(), len, block, nblk, h->blk_cd.get(), h->cand.get(), ncand)); h->launches++; }
  FqText t;
  t.text = h->text.get(); t.len = len; t.block_bytes = block; t.pad = 0; t.blk_nb = h->blk_nb.get(); t.gran_nb = h->gran.get();
  t.cand = h->cand.get(); t.ncand = ncand; t.nblk = nblk;
  const uint64_t G = h->max_groups;
  const unsigned g_wave = (unsigned)((nn + 3) / 4 < G ? (nn + 3) / 4 : G), g_node = (unsigned)((nn + 1 + 255) / 256 < G ? (nn + 1 + 255) / 256 : G),
                 g_tile = (unsigned)(ntile < G ? ntile : G);
  uint32_t *jump = h->jump.get();
  uint8_t *mark = h->mark.get();
  RdSum *sum = h->sum.get();
  RdSum s0;
  memset(&s0, 0, sizeof(s0));
  s0.stop_node = RD_NONE;
  const uint8_t one = 1;
  RD_HIP(hipMemsetAsync(mark, 0, nn + 1, st));
  RD_HIP(hipMemcpyAsync(mark, &one, 1, hipMemcpyHostToDevice, st));
  RD_HIP(hipMemcpyAsync(sum, &s0, sizeof(s0), hipMemcpyHostToDevice, st));
  RD_HIP(hipMemcpyAsync(h->read_off.get(), &zero, sizeof(zero), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_rd_step, dim3(g_wave), dim3(256), 0, st, t, nn, h->step.get(), jump);
  RD_HIP(hipGetLastError()); h->launches++;
  for (uint32_t r = 1; r < L; r++) {
    hipLaunchKernelGGL(k_rd_double, dim3(g_node), dim3(256), 0, st, jump + (size_t)(r - 1) * (nn + 1), jump + (size_t)r * (nn + 1), nn + 1);
    RD_HIP(hipGetLastError()); h->launches++;
  }
  for (uint32_t r = L; r-- > 0;) {
    hipLaunchKernelGGL(k_rd_mark, dim3(g_node), dim3(256), 0, st, jump + (size_t)r * (nn + 1), mark, nn);
    RD_HIP(hipGetLastError()); h->launches++;
  }
  hipLaunchKernelGGL(k_rd_sums, dim3(g_tile), dim3(256), 0, st, h->step.get(), mark, nn, ntile, is_last, h->part_c.get(), h->part_b.get(), sum);
  RD_HIP(hipGetLastError()); h->launches++;
  RD_HIP(fq_launch_scan(st, h->part_c.get(), h->part_b.get(), ntile));
  h->launches++;
  hipLaunchKernelGGL(k_rd_number, dim3(g_tile), dim3(256), 0, st, h->step.get(), mark, nn, ntile, max_reads, h->part_c.get(),
                     h->part_b.get(), sum, h->rec.get(), h->read_off.get(), h->hdr.get());
  RD_HIP(hipGetLastError()); h->launches++;
  RdSum hs;
  RD_HIP(hipMemcpyAsync(&hs, sum, sizeof(hs), hipMemcpyDeviceToHost, st));
  RD_HIP(hipStreamSynchronize(st));
  if (hs.stop_node != RD_NONE && rd_stop_is_error(hs.stop_kf, is_last != 0) && (!max_reads || hs.stop_idx < max_reads))
    return smaltgpu_set_error(SMALTGPU_EFILE, rd_error_text(hs.stop_kf, text, len, hs.stop_hdr_off).c_str());
  const uint64_t nreads = hs.nreads;
  if (nreads > nn) return smaltgpu_set_error(SMALTGPU_EINTERNAL, "more reads than prompts");
  const bool has_qual = nreads && !hs.any_fasta;
  uint64_t total = 0, rec_end = 0;
  if (nreads) {
    RdRec last;
    RD_HIP(hipMemcpyAsync(&total, h->read_off + nreads, 8, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(&last, h->rec + (nreads - 1), sizeof(last), hipMemcpyDeviceToHost, st));
    RD_HIP(hipStreamSynchronize(st));
    if (total > tot[0] || last.q1 > len) return smaltgpu_set_error(SMALTGPU_EINTERNAL, "the numbering disagrees with the counts of the text");
    rec_end = last.q1;
    hipLaunchKernelGGL(k_rd_emit, dim3((unsigned)nblk), dim3(256), 0, st, h->text.get(), len, block, h->blk_nb.get(), h->rec.get(),
                       nreads, h->bases.get(), has_qual ? h->quals.get() : nullptr, total);
    RD_HIP(hipGetLastError()); h->launches++;
  }
  h->exact[0] = (size_t)total; h->exact[1] = has_qual ? (size_t)total : 0; h->exact[2] = (size_t)(nreads + 1) * sizeof(uint64_t);
  if (hv) {                              // the compacted arrays, and the header offsets for the names
    h->h_bases.resize(total ? total : 1); h->h_off.resize(nreads + 1); h->h_hdr.resize(nreads);
    if (has_qual) h->h_quals.resize(total ? total : 1);
    if (total) RD_HIP(hipMemcpyAsync(h->h_bases.data(), h->bases.get(), total, hipMemcpyDeviceToHost, st));
    if (total && has_qual) RD_HIP(hipMemcpyAsync(h->h_quals.data(), h->quals.get(), total, hipMemcpyDeviceToHost, st));
    RD_HIP(hipMemcpyAsync(h->h_off.data(), h->read_off.get(), (nreads + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (nreads) RD_HIP(hipMemcpyAsync(h->h_hdr.data(), h->hdr.get(), nreads * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  RD_HIP(hipStreamSynchronize(st));
  if (hv) for (uint64_t i = 0; i < nreads; i++) if (h->h_hdr[i] >= len) return smaltgpu_set_error(SMALTGPU_EINTERNAL, "a header offset lies behind the text");
  return rd_fill_views(h, len, is_last, max_reads, nreads, total, has_qual, rec_end, text, hv, dv);
}

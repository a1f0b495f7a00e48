// smg_entries.cpp -- the entries of libsmaltgpu.so that run one kernel or one stage alone, for the tests (include/smaltgpu.h, "test
// entries").  Those that run a part of the pipeline stage their reads and begin the call with the functions the pipeline itself
// uses (smg_mapper.hpp); device memory of a call is held in DevBuf, so that every return frees it and every copy is checked.
#include "smg_mapper.hpp"
#include "smg_dump.hpp"

static int sync_kernel(smaltgpu_mapper *m) {
  if (hipStreamSynchronize(m->stream) != hipSuccess) return fail(SMALTGPU_ENODEV, "kernel failed");
  return 0;
}

template <class T>
static int fetch(std::vector<T> &v, const T *dev, size_t n) {
  v.resize(n ? n : 1);
  if (n) HIPCHK(hipMemcpy(v.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" long smaltgpu_dump_read(smaltgpu_mapper *m, uint32_t i, const char *name, char *buf, size_t bufsiz) {
  if (!m) return fail(SMALTGPU_EARG, "null mapper");
  if (!m->debug || !m->cand_scr_dbg) return fail(SMALTGPU_EARG, "smaltgpu_set_debug(m, 1) must precede the batch");
  if (i >= m->last_n || !m->have_host_off) return fail(SMALTGPU_EARG, "read index out of range");
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  const Batch &b = m->b;
  const DevIndex &d = m->ix->d;
  DumpView v;
  std::vector<HitInfoHdr> hi; std::vector<SeedRec> seeds; std::vector<uint8_t> qmask;
  std::vector<CandHdr> ch; std::vector<ReadCtl> ctl; std::vector<ReadStat> st;
  std::vector<uint8_t> slot;
  if (fetch(hi, b.hi + 2 * (size_t)i, 2) || fetch(seeds, b.seeds + 2 * (size_t)i * m->qmax, 2 * (size_t)m->qmax) ||
      fetch(qmask, b.qmask + 2 * (size_t)i * m->qmax, 2 * (size_t)m->qmax) || fetch(ch, b.ch + i, 1) || fetch(ctl, b.ctl + i, 1) ||
      fetch(st, b.stat + i, 1) || fetch(slot, m->cand_scr_dbg + m->cand_bytes * i, m->cand_bytes)) return SMALTGPU_ENODEV;
  const uint32_t ngrp = (m->last_par.flags & FLG_SEQBYSEQ) ? (uint32_t)d.nseq : 1u;
  const int dk = m->last_fine ? (int)FINE_K : d.k, dsx = m->last_fine ? (int)FINE_S : d.s;
  const bool v2 = cands_v2_applicable(m->last_par, dk, dsx, (uint32_t)(m->h_off[i + 1] - m->h_off[i]), b.iv_off != nullptr);
  CandScratch cx = cand_scratch_carve(slot.data(), m->qmax, dsx, m->cg.hcap, ngrp, m->cg.segcap, m->cg.candcap);
  CandsV2Scratch c2 = cands_v2_carve(nullptr, 0, slot.data(), m->qmax, dsx, m->cg.hcap_strand, ngrp, m->cg.candcap, true);
  std::vector<RCand> rc; std::vector<Result> res; std::vector<uint8_t> dstr;
  if (fetch(rc, b.rcpool + ch[0].rc_off, ch[0].n_sort) || fetch(res, b.respool + st[0].res_off, st[0].nres)) return SMALTGPU_ENODEV;
  size_t nd = 0;
  for (uint32_t j = 0; j < st[0].nres; j++) { size_t e = (size_t)res[j].stroffs + res[j].strlen; if (e > nd) nd = e; }
  if (fetch(dstr, b.dstrpool + st[0].dstr_off, nd)) return SMALTGPU_ENODEV;
  v.qlen = (uint32_t)(m->h_off[i + 1] - m->h_off[i]); v.qmax = m->qmax; v.k = dk;
  for (int s2 = 0; s2 < 2; s2++) { v.hi[s2] = hi[s2]; v.seeds[s2] = seeds.data() + (size_t)s2 * m->qmax; v.qmask[s2] = qmask.data() + (size_t)s2 * m->qmax; }
  v.ch = ch[0]; v.rc = rc.data(); v.ctl = ctl[0]; v.st = st[0]; v.res = res.data(); v.dstr = dstr.data(); v.ngrp = ngrp;
  std::vector<SegCand> crec;
  if (v2) { cands_v2_records(crec, c2, ch[0].ncand <= m->cg.candcap ? ch[0].ncand : 0, m->qmax > 255); v.cand = crec.data(); v.sort_idx = c2.sort_idx; v.sort_keys = c2.sort_keys; v.hitwords = c2.dbg_words; v.grp_first = c2.dbg_first; v.grp_cnt = c2.dbg_cnt; }
  else { v.cand = cx.cand; v.sort_idx = cx.sort_idx; v.sort_keys = cx.sort_keys; v.hitwords = cx.keys; v.grp_first = cx.grp_first; v.grp_cnt = cx.grp_cnt; }
  std::string o;
  dump_read(o, v, i, name, m->debug >= 2);
  if (buf && bufsiz) { size_t c = o.size() < bufsiz - 1 ? o.size() : bufsiz - 1; memcpy(buf, o.data(), c); buf[c] = 0; }
  return (long)o.size();
}

extern "C" int smaltgpu_sw_full_batch(smaltgpu_mapper *m, const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                                       const uint32_t *r_off, uint32_t ntask, const smaltgpu_params *par, int32_t *scores, int packed16) {
  if (!m || !qcodes || !q_off || !rcodes || !r_off || !par || !scores) return fail(SMALTGPU_EARG, "null argument");
  HIPCHK(hipSetDevice(m->device));
  uint32_t qmaxlen = 0, rmaxlen = 0;
  for (uint32_t t = 0; t < ntask; t++) {
    const uint32_t ql = q_off[t + 1] - q_off[t], wl = r_off[t + 1] - r_off[t];
    if (ql > qmaxlen) qmaxlen = ql;
    if (wl > rmaxlen) rmaxlen = wl;
  }
  DevBuf<uint8_t> dq, dr; DevBuf<uint32_t> dqo, dro; DevBuf<int32_t> dsc;
  TRY(dq.alloc(q_off[ntask] + 16, qcodes, q_off[ntask])); TRY(dr.alloc(r_off[ntask] + 16, rcodes, r_off[ntask]));
  TRY(dqo.alloc((size_t)ntask + 1, q_off, (size_t)ntask + 1)); TRY(dro.alloc((size_t)ntask + 1, r_off, (size_t)ntask + 1)); TRY(dsc.alloc(ntask));
  int lr;
  if (!packed16 && (qmaxlen > 512 || rmaxlen > (uint32_t)SW_FULL_WMAX))     // beyond the register tiling: the strip kernel (windows up to the mapper's capacity)
    lr = launch_sw_strip_raw(m->stream, dq.p, dqo.p, dr.p, dro.p, ntask, to_par(par), dsc.p, m->strip_bnd, m->strip_win, m->wincap, m->strip_grid);
  else if (packed16 && (qmaxlen > 512 || rmaxlen > (uint32_t)SW_FULL_WMAX))                         // ... and its packed form, two tasks per wave
    lr = launch_sw_strip16_raw(m->stream, dq.p, dqo.p, dr.p, dro.p, ntask, to_par(par), dsc.p, m->strip_bnd, m->strip_win, m->wincap, m->strip_grid, qmaxlen);
  else lr = launch_sw_full_raw(m->stream, dq.p, dqo.p, dr.p, dro.p, ntask, to_par(par), dsc.p, qmaxlen, packed16);
  if (lr) return fail(SMALTGPU_EARG, lr == -2 ? "scores do not fit the packed 16-bit kernel" : "query longer than the register-tiled kernel supports");
  TRY(sync_kernel(m));
  return dsc.get(scores, ntask);
}

extern "C" int smaltgpu_sw_band_batch(smaltgpu_mapper *m, const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                                       const uint32_t *r_off, uint32_t ntask, const smaltgpu_params *par, const int32_t *band, int form,
                                       int32_t *scores, int32_t *status) {
  if (!m || !qcodes || !q_off || !rcodes || !r_off || !par || !band || !scores || !status) return fail(SMALTGPU_EARG, "null argument");
  if (form != 0 && form != 1) return fail(SMALTGPU_EARG, "unknown form");
  uint32_t qmaxlen = 0, rmaxlen = 0;
  for (uint32_t t = 0; t < ntask; t++) {
    const uint32_t ql = q_off[t + 1] - q_off[t], wl = r_off[t + 1] - r_off[t];
    if (q_off[t + 1] <= q_off[t] || r_off[t + 1] <= r_off[t]) return fail(SMALTGPU_EARG, "empty read or window");
    if (form == 0 && wl > m->wincap) return fail(SMALTGPU_EARG, "window above the mapper's capacity");
    if (ql > qmaxlen) qmaxlen = ql;
    if (wl > rmaxlen) rmaxlen = wl;
    Band bd;
    status[t] = band_init(bd, band[4 * t], band[4 * t + 1], band[4 * t + 2], band[4 * t + 3], (int)ql, 0, (int)wl - 1, (int)wl) ? 1 : 0;
  }
  // the windows back to back in the index's layout: 10 codes per word, the first in bits 29..27
  const size_t nbase = r_off[ntask];
  std::vector<uint32_t> packed(nbase / 10 + 2, 0u);
  for (size_t o = 0; o < nbase; o++) packed[o / 10] |= (uint32_t)(rcodes[o] & 7u) << (3 * (9 - (uint32_t)(o % 10)));
  HIPCHK(hipSetDevice(m->device));
  const uint32_t rowlen = qmaxlen + rmaxlen + 2;      // band_fast_scalar looks one row past a band that has left the read
  const size_t nrows = form == 1 ? (size_t)((ntask + 63) / 64) * 64 * 2 * rowlen : 1;
  DevBuf<uint8_t> dq; DevBuf<uint32_t> dp, dqo, dro; DevBuf<int32_t> dsc, dbd; DevBuf<int> drows;
  TRY(dq.alloc(q_off[ntask] + 16, qcodes, q_off[ntask])); TRY(dp.alloc(packed.size(), packed.data(), packed.size()));
  TRY(dqo.alloc((size_t)ntask + 1, q_off, (size_t)ntask + 1)); TRY(dro.alloc((size_t)ntask + 1, r_off, (size_t)ntask + 1));
  TRY(dsc.alloc((size_t)ntask + 1)); TRY(dbd.alloc(4 * (size_t)ntask + 4, band, 4 * (size_t)ntask));
  TRY(drows.alloc(nrows)); TRY(drows.fill(0));
  const int lr = form == 0 ? launch_sw_band_raw(m->stream, dq.p, dqo.p, dp.p, dro.p, ntask, to_par(par), dbd.p, dsc.p, m->strip_bnd, m->strip_win, m->wincap, m->strip_grid)
                           : launch_sw_band_scalar_raw(m->stream, dq.p, dqo.p, dp.p, dro.p, ntask, to_par(par), dbd.p, dsc.p, drows.p, rowlen);
  if (lr) return fail(SMALTGPU_ENODEV, "kernel launch failed");
  TRY(sync_kernel(m));
  return dsc.get(scores, ntask);
}

static_assert(sizeof(smaltgpu_band_node) == sizeof(BandNodeOut), "smaltgpu_band_node is BandNodeOut");
static_assert((int)SMALTGPU_BAND_NFORMS == (int)BF_NFORMS && (int)SMALTGPU_BAND_SCALAR == (int)BF_SCALAR && (int)SMALTGPU_BAND_STRIP8 == (int)BF_STRIP8, "form numbers");

extern "C" int smaltgpu_band_geometry(int band_l, int band_r, int qs, int qe, int qlen, int s_left, int s_right, int wlen, int gap_init,
                                       int gap_ext, int32_t *geo) {
  if (!geo || qlen < 1 || wlen < 1) return fail(SMALTGPU_EARG, "bad argument");
  Band b;
  if (band_init(b, band_l, band_r, qs, qe, qlen, s_left, s_right, wlen)) return 1;
  const int32_t v[14] = {b.band_width, b.l_edge_orig, b.r_edge_orig, b.l_edge, b.r_edge, b.s_left_orig, b.s_left, b.s_len, b.s_totlen,
                         b.q_left_orig, b.q_left, b.q_len, b.q_totlen, band_form_production(b, -gap_init, -gap_ext)};
  memcpy(geo, v, sizeof(v));
  return 0;
}

extern "C" int smaltgpu_band_align_nodes(smaltgpu_mapper *m, const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                                          const uint32_t *r_off, uint32_t ntask, const smaltgpu_params *par, const int32_t *band, const int32_t *iv,
                                          int minscore, int form, int lds, int tw, smaltgpu_band_node *out, uint8_t *dstr) {
  if (!m || !qcodes || !q_off || !rcodes || !r_off || !par || !band || !iv || !out || !dstr) return fail(SMALTGPU_EARG, "null argument");
  if (form < 0 || form >= (int)BF_NFORMS || (lds && form != (int)BF_ROWS)) return fail(SMALTGPU_EARG, "unknown form");
  const MapPar p = to_par(par);
  const int gi = -p.gap_init, ge = -p.gap_ext;
  if (form == (int)BF_ROWS && !(gi >= ge && ge >= 0)) return fail(SMALTGPU_EARG, "the row form needs gap_init >= gap_ext >= 0");
  // per task: the form's precondition on the band the kernel will set up, and the room its directions take
  std::vector<uint64_t> dir_off((size_t)ntask + 1, 0);
  std::vector<uint32_t> dstr_off((size_t)ntask + 1, 0);
  uint32_t qmaxlen = 0, rmaxlen = 0;
  for (uint32_t t = 0; t < ntask; t++) {
    if (q_off[t + 1] <= q_off[t] || r_off[t + 1] <= r_off[t]) return fail(SMALTGPU_EARG, "empty read or window");
    const uint32_t ql = q_off[t + 1] - q_off[t], wl = r_off[t + 1] - r_off[t];
    if (ql > (1u << 20) || wl > (1u << 20)) return fail(SMALTGPU_EARG, "task too long");
    if (lds && (ql > NODE_LDS_CODES || wl > NODE_LDS_CODES)) return fail(SMALTGPU_EARG, "read or window too long for the LDS stage");
    if (ql > qmaxlen) qmaxlen = ql;
    if (wl > rmaxlen) rmaxlen = wl;
    Band b;
    uint64_t need = 16;
    if (!band_init(b, band[4 * t], band[4 * t + 1], band[4 * t + 2], band[4 * t + 3], (int)ql, iv[2 * t], iv[2 * t + 1], (int)wl) &&
        b.s_left < b.s_len && b.band_width >= 0) {
      if (!band_form_ok(form, b, gi, ge)) return fail(SMALTGPU_EARG, "a task's band is outside the form's precondition");
      need = band_dir_bytes(form, b, tw != 0) + 2 * (uint64_t)wl + 256;
    }
    dir_off[t + 1] = dir_off[t] + ((need + 15) & ~(uint64_t)15);
    dstr_off[t + 1] = dstr_off[t] + ql + wl + 16;
  }
  if (dir_off[ntask] > (4ull << 30)) return fail(SMALTGPU_EARG, "direction matrices above 4 GiB");
  std::vector<uint8_t> wdec(r_off[ntask] + 1);                       // window codes as the mapper decodes them (ref_code)
  for (size_t o = 0; o < r_off[ntask]; o++) { const uint8_t c = rcodes[o] & 7; wdec[o] = c == 7 ? 0 : ((c == 6 || c == 4) ? 5 : c); }
  HIPCHK(hipSetDevice(m->device));
  const bool strip = form == (int)BF_STRIP8 || form == (int)BF_STRIP16;
  const uint32_t rowlen = qmaxlen + rmaxlen + 2;
  const size_t nbnd = strip ? (size_t)ntask * 2 * rmaxlen : 1, nrows = form == (int)BF_SCALAR ? (size_t)ntask * 2 * rowlen : 1, n1 = (size_t)ntask + 1;
  DevBuf<uint8_t> dq, dw, ddir, dtmp, dds; DevBuf<uint32_t> dqo, dro, ddso; DevBuf<uint64_t> ddo; DevBuf<int32_t> dbd, div;
  DevBuf<int2> dbnd; DevBuf<int> drows; DevBuf<BandNodeOut> dout;
  TRY(dq.alloc(q_off[ntask] + 16, qcodes, q_off[ntask])); TRY(dw.alloc(r_off[ntask] + 16, wdec.data(), r_off[ntask]));
  TRY(ddir.alloc(dir_off[ntask] + 16)); TRY(ddir.fill(0)); TRY(dtmp.alloc((size_t)dstr_off[ntask] + 16));
  TRY(dds.alloc((size_t)dstr_off[ntask] + 16)); TRY(dds.fill(0));
  TRY(dqo.alloc(n1, q_off, n1)); TRY(dro.alloc(n1, r_off, n1)); TRY(ddso.alloc(n1, dstr_off.data(), n1)); TRY(ddo.alloc(n1, dir_off.data(), n1));
  TRY(dbd.alloc(4 * (size_t)ntask + 4, band, 4 * (size_t)ntask)); TRY(div.alloc(2 * (size_t)ntask + 2, iv, 2 * (size_t)ntask));
  TRY(dbnd.alloc(nbnd)); TRY(dbnd.fill(0)); TRY(drows.alloc(nrows)); TRY(drows.fill(0)); TRY(dout.alloc(n1));
  BandNodeArgs a;
  a.q = dq.p; a.q_off = dqo.p; a.win = dw.p; a.r_off = dro.p; a.ntask = ntask; a.band = dbd.p; a.iv = div.p;
  a.minscore = minscore; a.form = form; a.lds = lds; a.tw = tw;
  a.dir = ddir.p; a.dir_off = ddo.p; a.bnd = dbnd.p; a.bndcap = rmaxlen; a.rows = drows.p; a.rowlen = rowlen;
  a.dtmp = dtmp.p; a.dstr = dds.p; a.dstr_off = ddso.p; a.out = dout.p;
  if (launch_band_nodes(m->stream, a, p)) return fail(SMALTGPU_ENODEV, "kernel launch failed");
  TRY(sync_kernel(m));
  TRY(dout.get((BandNodeOut *)out, ntask));
  return dds.get(dstr, dstr_off[ntask]);
}

extern "C" int smaltgpu_sw_rowframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols) {
  return sw16_rowframe_max_steps(match, mismatch, gap_init, gap_ext, ncols);
}

extern "C" int smaltgpu_sw_pairframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols) {
  return sw16_pairframe_max_steps(match, mismatch, gap_init, gap_ext, ncols);
}

extern "C" int smaltgpu_rank_sort_batch(smaltgpu_mapper *m, const uint32_t *keys, const uint32_t *off, uint32_t narr, int nneed, int in_lds,
                                         int instance, uint32_t *out_keys, uint32_t *out_idx) {
  if (!m || !keys || !off || !out_keys || !out_idx) return fail(SMALTGPU_EARG, "null argument");
  if (instance != 0 && instance != 1) return fail(SMALTGPU_EARG, "unknown instance %d", instance);
  HIPCHK(hipSetDevice(m->device));
  const size_t tot = off[narr];
  const uint32_t nlim = instance ? (1u << SEED_IDXBITS) - 1u : (1u << 22), klim = instance ? 1u << (32 - SEED_IDXBITS) : 1024u;
  for (uint32_t t = 0; t < narr; t++) if (off[t + 1] < off[t] || off[t + 1] - off[t] > nlim) return fail(SMALTGPU_EARG, "bad array offsets");
  for (size_t i = 0; i < tot; i++) if (keys[i] >= klim) return fail(SMALTGPU_EARG, "key out of range");
  DevBuf<uint32_t> dk, doff, dkv, dok, doi;
  TRY(dk.alloc(tot + 1, keys, tot)); TRY(doff.alloc((size_t)narr + 1, off, (size_t)narr + 1));
  TRY(dkv.alloc(tot + 1)); TRY(dok.alloc(tot + 1)); TRY(doi.alloc(tot + 1));
  if (instance) launch_seed_sort_raw(m->stream, dk.p, doff.p, narr, dok.p, doi.p);
  else launch_rank_sort_raw(m->stream, dk.p, doff.p, narr, nneed, in_lds, dkv.p, dok.p, doi.p);
  TRY(sync_kernel(m));
  TRY(dok.get(out_keys, tot));
  return doi.get(out_idx, tot);
}

// S3 on its own: the launches of run_pipeline up to and including k_hits, on the mapper's buffers, and host copies of what they left
extern "C" int smaltgpu_hits_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                                   const smaltgpu_params *par, uint32_t window, uint64_t pool_keys, smaltgpu_hits_out *out) {
  static_assert(sizeof(SeedRec) == sizeof(smaltgpu_hit_seed) && sizeof(HitRun) == sizeof(smaltgpu_hit_run), "hit record layout");
  static_assert((uint32_t)HITRUN_NONE == (uint32_t)SMALTGPU_HITRUN_NONE && (uint32_t)HITRUN_SORTED == (uint32_t)SMALTGPU_HITRUN_SORTED &&
                (uint32_t)HITRUN_OVERFLOW == (uint32_t)SMALTGPU_HITRUN_OVERFLOW, "hit run modes");
  if (!m || !bases || !read_off || !par || !out) return fail(SMALTGPU_EARG, "null argument");
  if (!m->hits_W || !m->b_hitrun) return fail(SMALTGPU_EARG, "this mapper keeps S3 inside the candidate stage (max_read_len > 248 or SMALTGPU_HITS_SPLIT=0)");
  if (nreads > m->max_reads || read_off[nreads] - read_off[0] > m->max_bases) return fail(SMALTGPU_EARG, "batch exceeds the mapper's capacity");
  if (pool_keys > m->b.hitpool_cap) return fail(SMALTGPU_EARG, "pool_keys exceeds the pool's allocation (%llu keys)", (unsigned long long)m->b.hitpool_cap);
  TRY(check_par(m, par));
  uint32_t W = window ? window : m->hits_W;
  if (W < 256) W = 256;
  if (W > 1024) W = 1024;
  const uint64_t cap = pool_keys ? pool_keys : m->b.hitpool_cap;
  TRY(stage_reads(m, bases, quals, read_off, nreads));
  // the batch as run_pipeline begins a plain call (hitrun set: k_hits follows), but with no fetch behind it: an open one is dropped
  const Batch &b = m->b;
  const DevIndex &d = m->ix->d;
  hipStream_t s = m->stream;
  MapPar p;
  TRY(begin_call(m, quals ? m->d_quals : nullptr, m->d_off, nreads, par, nullptr, false, &p));
  m->fetch_open = false;
  Batch hb = b;
  m->hits_ran = true;
  hb.hitrun = m->b_hitrun; hb.hitwin = m->b_hitwin;       // (a mapping call of a mapper with a stride of 256 leaves k_hits out: begin_call)
  hb.hitpool_cap = cap;                                   // this call only: the kernels take a copy of the batch
  int rv = launch_encode(s, m->d_bases, m->d_off, nreads, m->d_codes, m->d_codes_rc);
  if (!rv) rv = launch_seed(s, hb, d, p, m->seed_scr, m->seed_bytes, m->seed_slots);
  if (!rv) rv = launch_hits(s, hb, d, p, W, m->cg.tab, m->hits_wg, m->hits_fill);
  if (rv) return fail(SMALTGPU_ENODEV, "kernel launch failed: %s", hipGetErrorString((hipError_t)rv));
  HIPCHK(hipStreamSynchronize(s));
  smaltgpu_mapper::HitsHost &h = m->hh;
  const size_t ns = 2 * (size_t)nreads, stride = m->qmax;
  h.hi.resize(ns ? ns : 1); h.n_seeds.assign(ns ? ns : 1, 0); h.seed_rank.assign(ns ? ns : 1, 0); h.status.assign(ns ? ns : 1, 0);
  h.seeds.resize(ns * stride + 1); h.qmask.resize(ns * stride + 1); h.runs.resize(ns ? ns : 1);
  unsigned long long count = 0;
  if (ns) {
    HIPCHK(hipMemcpy(h.hi.data(), b.hi, ns * sizeof(HitInfoHdr), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.seeds.data(), b.seeds, ns * stride * sizeof(SeedRec), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.qmask.data(), b.qmask, ns * stride, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h.runs.data(), m->b_hitrun, ns * sizeof(HitRun), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&count, b.hit_count, sizeof(count), hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < ns; i++) { h.n_seeds[i] = h.hi[i].n_seeds; h.seed_rank[i] = h.hi[i].seed_rank; h.status[i] = h.hi[i].status; }
  const uint64_t npool = count < cap ? count : cap;
  h.pool.resize(npool ? npool : 1);
  if (npool) HIPCHK(hipMemcpy(h.pool.data(), b.hitpool, npool * sizeof(uint64_t), hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(*out));
  out->nstrands = (uint32_t)ns; out->stride = (uint32_t)stride; out->window = W; out->tab = m->cg.tab;
  out->n_seeds = h.n_seeds.data(); out->seed_rank = h.seed_rank.data(); out->status = h.status.data();
  out->seeds = (const smaltgpu_hit_seed *)h.seeds.data(); out->qmask = h.qmask.data(); out->runs = (const smaltgpu_hit_run *)h.runs.data();
  out->hit_count = count; out->pool_cap = cap; out->pool = h.pool.data();
  return SMALTGPU_OK;
}

// How k_hits gathered the strands of the mapper's last call (a mapping call or smaltgpu_hits_batch), from the table the kernel leaves
extern "C" int smaltgpu_hits_windows(smaltgpu_mapper *m, uint32_t nstrands, uint32_t *windows, uint64_t totals[4]) {
  if (!m || !totals) return fail(SMALTGPU_EARG, "null argument");
  if (nstrands > 2 * (uint64_t)m->last_n) return fail(SMALTGPU_EARG, "the last call held %u strands", 2 * m->last_n);
  totals[0] = totals[1] = totals[2] = totals[3] = 0;
  if (windows) memset(windows, 0, (size_t)nstrands * sizeof(uint32_t));
  if (!m->hits_ran || !nstrands) return SMALTGPU_OK;
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  std::vector<uint32_t> win(nstrands);
  std::vector<HitRun> runs(nstrands);
  unsigned long long count = 0;
  HIPCHK(hipMemcpy(win.data(), m->b_hitwin, (size_t)nstrands * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(runs.data(), m->b_hitrun, (size_t)nstrands * sizeof(HitRun), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&count, m->b.hit_count, sizeof(count), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < nstrands; i++)
    if ((win[i] & 0xffffu) && runs[i].mode == HITRUN_SORTED) { totals[0]++; totals[1] += win[i] & 0xffffu; totals[2] += runs[i].n; }
  totals[3] = count;
  if (windows) memcpy(windows, win.data(), (size_t)nstrands * sizeof(uint32_t));
  return SMALTGPU_OK;
}

// k_fine_index on its own: the context of a fine round goes up as for a mapping call (upload_ctx), the position buffer and the
// index rows are filled with a guard pattern, launch_fine_index runs on the mapper's buffers, and everything comes back
extern "C" int smaltgpu_fine_index_batch(smaltgpu_mapper *m, uint32_t nreads, const uint64_t *iv_off, const smaltgpu_interval *iv, uint32_t grid,
                                         uint32_t guard, smaltgpu_fine_out *out) {
  if (!m || !iv_off || !out) return fail(SMALTGPU_EARG, "null argument");
  if (nreads > m->max_reads) return fail(SMALTGPU_EARG, "batch exceeds the mapper's capacity");
  HIPCHK(hipSetDevice(m->device));
  smaltgpu_callctx ctx;
  memset(&ctx, 0, sizeof(ctx));
  ctx.iv_off = iv_off; ctx.iv = iv; ctx.fine_index = 1;
  CtxDev cd;
  TRY(upload_ctx(m, &ctx, nreads, &cd));
  hipStream_t s = m->stream;
  const size_t npos = (size_t)m->h_fineoff[nreads] + 1, nidx = (size_t)nreads * FINE_IDX_STRIDE;      // (one word behind the last slice)
  std::vector<uint32_t> &hp = m->h_finepos, &hi = m->h_fineidx;
  hp.assign(npos, guard); hi.assign(nidx ? nidx : 1, guard);
  HIPCHK(hipMemcpyAsync(cd.fine_pos, hp.data(), npos * 4, hipMemcpyHostToDevice, s));
  if (nidx) HIPCHK(hipMemcpyAsync(cd.fine_idx, hi.data(), nidx * 4, hipMemcpyHostToDevice, s));
  Batch fb = m->b;                                        // no call begins on the mapper's batch: the kernel reads these fields of a copy
  fb.nreads = nreads; fb.iv_off = cd.iv_off; fb.iv = cd.iv; fb.fine_idx = cd.fine_idx; fb.fine_pos = cd.fine_pos; fb.fine_off = cd.fine_off;
  const int rv = launch_fine_index(s, fb, m->ix->d, grid);
  if (rv) return fail(SMALTGPU_ENODEV, "kernel launch failed: %s", hipGetErrorString((hipError_t)rv));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemcpy(hp.data(), cd.fine_pos, npos * 4, hipMemcpyDeviceToHost));
  if (nidx) HIPCHK(hipMemcpy(hi.data(), cd.fine_idx, nidx * 4, hipMemcpyDeviceToHost));
  out->nreads = nreads; out->idx_stride = FINE_IDX_STRIDE; out->nkeys = FINE_NKEYS; out->npos = (uint64_t)npos;
  out->fine_off = m->h_fineoff.data(); out->idx = hi.data(); out->pos = hp.data();
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_cands_geometry(smaltgpu_mapper *m, uint32_t out[8]) {
  if (!m || !out) return fail(SMALTGPU_EARG, "null argument");
  const bool two = m->cand_scr2 != nullptr;
  out[0] = m->cg.hcap_strand; out[1] = m->cg.candcap; out[2] = cands_lds_bytes(m->cg);
  out[3] = two ? m->cg2.hcap_strand : 0u; out[4] = two ? m->cg2.candcap : 0u; out[5] = two ? cands_lds_bytes(m->cg2) : 0u;
  out[6] = m->qmax; out[7] = (uint32_t)IV_MAX;
  return SMALTGPU_OK;
}

// The candidate pool as the score stage of the last mapping call left it, and the geometry its task routing follows (read-only)
static_assert(sizeof(smaltgpu_pool_rec) == sizeof(RCand) && offsetof(smaltgpu_pool_rec, flags) == offsetof(RCand, flags) &&
              offsetof(smaltgpu_pool_rec, swscor) == offsetof(RCand, swscor) && offsetof(smaltgpu_pool_rec, rid) == offsetof(RCand, rid),
              "smaltgpu_pool_rec is the layout of RCand");
static_assert(SMALTGPU_RCF_REVERSE == RCF_REVERSE && SMALTGPU_RCF_SCORED == RCF_SCORED && SMALTGPU_RCF_BANDED == RCF_BANDED &&
              SMALTGPU_RCF_ERR == RCF_ERR && SMALTGPU_RCF_QN == RCF_QN && SMALTGPU_RCF_BSCORED == RCF_BSCORED, "SMALTGPU_RCF_* mirror RCF_*");
extern "C" int smaltgpu_score_pool(smaltgpu_mapper *m, smaltgpu_score_pool_out *out) {
  if (!m || !out) return fail(SMALTGPU_EARG, "null argument");
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipStreamSynchronize(m->stream));
  const Batch &b = m->b;
  uint32_t count = 0;
  HIPCHK(hipMemcpy(&count, b.rc_count, sizeof(count), hipMemcpyDeviceToHost));
  const uint32_t n = count < b.rccap ? count : b.rccap;
  if (fetch(m->h_pool, b.rcpool, n)) return SMALTGPU_ENODEV;
  int G = 0, C = 0;
  (void)sw_full_geometry(m->max_len, &G, &C);
  memset(out, 0, sizeof(*out));
  out->rec = (const smaltgpu_pool_rec *)m->h_pool.data(); out->nrec = n; out->rc_count = count;
  out->rccap = b.rccap; out->long_cap = b.long_cap; out->strip_cap = b.strip_cap; out->tile_qmax = b.tile_qmax; out->wincap = m->wincap;
  out->tile_g = (uint32_t)G; out->tile_c = (uint32_t)C; out->full_grid = m->full_grid; out->strip_grid = m->strip_grid;
  return SMALTGPU_OK;
}

extern "C" int smaltgpu_sort_u64_batch(smaltgpu_mapper *m, const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out) {
  if (!m || !keys || !off || !out) return fail(SMALTGPU_EARG, "null argument");
  if (form < 0 || form > 5) return fail(SMALTGPU_EARG, "unknown form %d", form);
  const uint32_t nmax = form == 0 ? 256u : (form == 1 ? 512u : (form <= 3 ? 1024u : 65536u));
  for (uint32_t t = 0; t < narr; t++) if (off[t + 1] < off[t] || off[t + 1] - off[t] > nmax) return fail(SMALTGPU_EARG, "array %u does not fit form %d (at most %u keys)", t, form, nmax);
  HIPCHK(hipSetDevice(m->device));
  const size_t tot = narr ? off[narr] : 0;
  DevBuf<uint64_t> dk, dout; DevBuf<uint32_t> doff;
  TRY(dk.alloc(tot + 1, keys, tot)); TRY(dout.alloc(tot + 1)); TRY(doff.alloc((size_t)narr + 1, off, (size_t)narr + 1));
  if (form >= 4 ? launch_sort_u64_hbm_raw(m->stream, dk.p, doff.p, narr, form, dout.p) : launch_sort_u64_raw(m->stream, dk.p, doff.p, narr, form, dout.p))
    return fail(SMALTGPU_ENODEV, "kernel launch failed");
  TRY(sync_kernel(m));
  return dout.get(out, tot);
}

// S1 + S2 on their own: launch_encode and launch_seed on the mapper's buffers and nothing behind them.  The rows of the batch in
// hi, seeds and qmask and one row behind the last strand are filled with `guard` first, so that a test sees every byte the kernel wrote.
extern "C" int smaltgpu_seed_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                                   const smaltgpu_params *par, const uint32_t *seed_range, int totals_only, int scratch_home, uint32_t grid,
                                   uint8_t guard, smaltgpu_seed_out *out) {
  static_assert(sizeof(HitInfoHdr) == 8 * sizeof(uint32_t) && sizeof(SeedRec) == 3 * sizeof(uint32_t), "seed record layout");
  if (!m || !bases || !read_off || !par || !out || !out->codes || !out->codes_rc || !out->hi || !out->seeds || !out->qmask) return fail(SMALTGPU_EARG, "null argument");
  if (seed_range && totals_only) return fail(SMALTGPU_EARG, "seed_range and totals_only exclude each other (rmap.c:1076 counts the hits of whole reads)");
  if (scratch_home != 0 && scratch_home != 1) return fail(SMALTGPU_EARG, "scratch_home is 0 or 1");
  if (nreads >= m->max_reads || read_off[nreads] - read_off[0] > m->max_bases) return fail(SMALTGPU_EARG, "batch exceeds the mapper's capacity (one guard row is kept behind the last strand)");
  TRY(check_par(m, par));
  const bool hbm = scratch_home == 1 || m->seed_bytes > 48 * 1024;
  if (hbm && grid > m->seed_slots) return fail(SMALTGPU_EARG, "grid %u exceeds the %u scratch slots", grid, m->seed_slots);
  const uint64_t total = read_off[nreads] - read_off[0];
  TRY(stage_reads(m, bases, quals, read_off, nreads));
  CtxDev cd = {};                                         // of a round's context the entry takes the seed range alone
  if (seed_range) TRY(upload_per_read(m, m->cx_seedrange, seed_range, nreads, 2, &cd.seed_range));
  Batch &b = m->b;
  const DevIndex &d = m->ix->d;
  hipStream_t s = m->stream;
  MapPar p;
  TRY(begin_call(m, quals ? m->d_quals : nullptr, m->d_off, nreads, par, &cd, totals_only != 0, &p));
  b.hitrun = nullptr;                                     // no k_hits behind the seeding here, whatever the mapper
  m->fetch_open = false;                                  // no fetch follows: an open one is dropped
  const size_t rows = 2 * (size_t)nreads + 1, stride = m->qmax;
  HIPCHK(hipMemsetAsync(b.hi, guard, rows * sizeof(HitInfoHdr), s));
  HIPCHK(hipMemsetAsync(b.seeds, guard, rows * stride * sizeof(SeedRec), s));
  HIPCHK(hipMemsetAsync(b.qmask, guard, rows * stride, s));
  // scratch: the mapper's own, or HBM slots for this call only where the mapper's fits LDS
  uint8_t *scr = m->seed_scr;
  DevBuf<uint8_t> own;
  const uint32_t items = 2 * nreads;
  const uint32_t g = grid ? grid : (hbm ? (items < m->seed_slots ? items : m->seed_slots) : (items < 32768u ? items : 32768u));
  if (scratch_home == 1 && !scr && g) {
    TRY(own.alloc(m->seed_bytes * (size_t)g));
    scr = own.p;
  }
  int rv = launch_encode(s, m->d_bases, m->d_off, nreads, m->d_codes, m->d_codes_rc);
  if (!rv) rv = launch_seed(s, b, d, p, scr, m->seed_bytes, own.p ? g : m->seed_slots, scratch_home == 1, grid);
  b.seed_range = nullptr; b.totals_only = 0;
  const hipError_t he = hipStreamSynchronize(s);          // before any return: `own` goes with the scope
  if (rv) return fail(SMALTGPU_ENODEV, "kernel launch failed: %s", hipGetErrorString((hipError_t)rv));
  HIPCHK(he);
  unsigned long long work[WK_NWORK];
  if (total) { HIPCHK(hipMemcpy(out->codes, m->d_codes, total, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(out->codes_rc, m->d_codes_rc, total, hipMemcpyDeviceToHost)); }
  HIPCHK(hipMemcpy(out->hi, b.hi, rows * sizeof(HitInfoHdr), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->seeds, b.seeds, rows * stride * sizeof(SeedRec), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out->qmask, b.qmask, rows * stride, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(work, b.work, sizeof(work), hipMemcpyDeviceToHost));
  out->nrows = (uint32_t)rows; out->stride = (uint32_t)stride; out->in_lds = hbm ? 0u : 1u; out->grid = nreads ? g : 0u; out->lookups = work[WK_LOOKUPS];
  return SMALTGPU_OK;
}

// k_gather_reads on its own: the two host batches become the two resident batches, the mapper's read buffers are filled with
// `guard`, launch_gather_reads runs with `ids`, and the gathered bytes come back with the `tail` bytes behind the last read
extern "C" int smaltgpu_gather_batch(smaltgpu_mapper *m, const uint8_t *const bases[2], const uint8_t *const quals[2], const uint64_t *const read_off[2],
                                     const uint32_t nreads[2], const uint32_t *ids, uint32_t nids, uint8_t guard, uint32_t tail,
                                     uint8_t *dst_bases, uint8_t *dst_quals, uint64_t *dst_off) {
  if (!m || !bases || !read_off || !nreads || !ids || !dst_bases || !dst_off || !bases[0] || !bases[1] || !read_off[0] || !read_off[1]) return fail(SMALTGPU_EARG, "null argument");
  if (quals && (!quals[0] != !quals[1])) return fail(SMALTGPU_EARG, "qualities: both batches or neither");
  const bool wq_in = quals && quals[0];
  if (wq_in && !dst_quals) return fail(SMALTGPU_EARG, "null argument");
  if (nids > m->max_reads || tail > 16) return fail(SMALTGPU_EARG, "batch exceeds the mapper's capacity");
  for (int w = 0; w < 2; w++) if (read_off[w][0] != 0) return fail(SMALTGPU_EARG, "offsets start at 0");
  HIPCHK(hipSetDevice(m->device));
  DevBuf<uint8_t> db[2], dq[2];
  DevBuf<uint64_t> dof[2];
  smaltgpu_resident_reads src;
  memset(&src, 0, sizeof(src));
  for (int w = 0; w < 2; w++) {
    const size_t tot = read_off[w][nreads[w]];
    TRY(db[w].alloc(tot + 16, bases[w], tot)); TRY(dof[w].alloc((size_t)nreads[w] + 1, read_off[w], (size_t)nreads[w] + 1));
    if (wq_in) TRY(dq[w].alloc(tot + 16, quals[w], tot));
    src.d_bases[w] = db[w].p; src.d_quals[w] = dq[w].p; src.d_read_off[w] = dof[w].p; src.read_off[w] = read_off[w]; src.nreads[w] = nreads[w];
  }
  bool wq = false;
  if (hipMemsetAsync(m->d_bases, guard, m->max_bases + 16, m->stream) != hipSuccess || hipMemsetAsync(m->d_quals, guard, m->max_bases + 16, m->stream) != hipSuccess)
    return fail(SMALTGPU_ENODEV, "memset failed");
  TRY(gather_round(m, &src, ids, nids, &wq));
  TRY(sync_kernel(m));
  const size_t tot = m->h_off[nids];
  HIPCHK(hipMemcpy(dst_bases, m->d_bases, tot + tail, hipMemcpyDeviceToHost));
  if (dst_quals) HIPCHK(hipMemcpy(dst_quals, m->d_quals, tot + tail, hipMemcpyDeviceToHost));      // (without qualities: the guard, untouched)
  memcpy(dst_off, m->h_off.data(), ((size_t)nids + 1) * sizeof(uint64_t));
  return SMALTGPU_OK;
}

// O1 and the K3 driver on their own: reads staged and encoded as in a mapping call, the caller's candidates and first-pass scores
// in place of what k_cands and the score kernels leave in the batch, then the tail of run_pipeline (launch_replay, both passes of
// launch_align on the mapper's scratch, slots and capacities) and the ordinary fetch.  No rule of the stages is restated here: the
// entry checks what production guarantees about a candidate and fills in the book-keeping fields.
extern "C" int smaltgpu_align_cands_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                                          const smaltgpu_params *par, const smaltgpu_callctx *ctx, const uint64_t *cand_off, const smaltgpu_cand *cands,
                                          const uint32_t *cover_deficit, uint32_t flags, smaltgpu_align_cands_out *out) {
  static_assert(sizeof(smaltgpu_readctl) == sizeof(ReadCtl), "read control layout");
  static_assert((uint32_t)SMALTGPU_CAND_REVERSE == (uint32_t)RCF_REVERSE, "strand flag");
  if (!m || !bases || !read_off || !par || !cand_off || !cover_deficit || !out) return fail(SMALTGPU_EARG, "null argument");
  if (nreads > m->max_reads || read_off[nreads] - read_off[0] > m->max_bases) return fail(SMALTGPU_EARG, "batch exceeds the mapper's capacity");
  if (flags & ~(uint32_t)SMALTGPU_ALIGN_CANDS_ANTIDIAG) return fail(SMALTGPU_EARG, "unknown flags");
  if (ctx && (ctx->iv_off || ctx->fine_index || ctx->seed_range)) return fail(SMALTGPU_EARG, "intervals, the on-the-fly index and seed ranges belong to the stages in front of this entry");
  TRY(check_par(m, par));
  if (par->rmapflg & SMALTGPU_FLG_CMPLXW) return fail(SMALTGPU_EARG, "complexity-weighted scores are not part of this entry");
  const DevIndex &d = m->ix->d;
  const std::vector<uint64_t> &sop = m->ix->sop;
  for (uint32_t r = 0; r < nreads; r++) if (cand_off[r + 1] < cand_off[r] || read_off[r + 1] < read_off[r]) return fail(SMALTGPU_EARG, "offsets of read %u descend", r);
  const uint64_t c0 = cand_off[0], tot = cand_off[nreads] - c0;
  if (tot > m->b.rccap) return fail(SMALTGPU_EARG, "%llu candidates exceed the pool of %u", (unsigned long long)tot, m->b.rccap);
  if (tot && !cands) return fail(SMALTGPU_EARG, "null argument");
  std::vector<CandHdr> ch(nreads ? nreads : 1);
  std::vector<RCand> rc(tot ? tot : 1);
  memset((void *)ch.data(), 0, ch.size() * sizeof(CandHdr));
  memset((void *)rc.data(), 0, rc.size() * sizeof(RCand));
  for (uint32_t r = 0; r < nreads; r++) {
    const uint64_t qlen = read_off[r + 1] - read_off[r];
    const uint32_t nc = (uint32_t)(cand_off[r + 1] - cand_off[r]);
    CandHdr &h = ch[r];
    h.ncand = h.n_sort = h.n_mincover = h.n_reserved = nc;
    h.rc_off = (uint32_t)(cand_off[r] - c0);
    h.cover_deficit[0] = cover_deficit[2 * r]; h.cover_deficit[1] = cover_deficit[2 * r + 1];
    for (uint32_t i = 0; i < nc; i++) {
      const smaltgpu_cand &c = cands[cand_off[r] + i];
      if (c.flags & ~(uint32_t)(SMALTGPU_CAND_REVERSE | SMALTGPU_CAND_ERR)) return fail(SMALTGPU_EARG, "candidate %u of read %u: unknown flags", i, r);
      if (c.sqidx < -1 || c.sqidx >= d.nseq) return fail(SMALTGPU_EARG, "candidate %u of read %u: no sequence %d", i, r, c.sqidx);
      const uint64_t slen = c.sqidx < 0 ? sop[(size_t)d.nseq] : sop[(size_t)c.sqidx + 1] - sop[(size_t)c.sqidx];
      if (c.rs > c.re || c.re >= slen) return fail(SMALTGPU_EARG, "candidate %u of read %u: window outside its sequence", i, r);
      if (c.swscor < 0 || (uint64_t)c.swscor > qlen * (uint64_t)par->match) return fail(SMALTGPU_EARG, "candidate %u of read %u: score %d outside 0 .. read length x match", i, r, c.swscor);
      RCand &o = rc[h.rc_off + i];
      o.rs = c.rs; o.re = c.re; o.qs = c.qs; o.qe = c.qe; o.band_l = c.band_l; o.band_r = c.band_r; o.sqidx = c.sqidx;
      o.flags = (c.flags & SMALTGPU_CAND_REVERSE ? (uint32_t)RCF_REVERSE : 0u) | (c.flags & SMALTGPU_CAND_ERR ? (uint32_t)RCF_ERR : 0u) | (uint32_t)RCF_SCORED;
      o.cover = c.cover; o.swscor = c.swscor; o.rid = r;
    }
  }
  TRY(stage_reads(m, bases, quals, read_off, nreads));
  CtxDev cd;
  if (ctx) {
    smaltgpu_callctx own = *ctx;
    own.hitlist_len = nullptr;                             // sizes the hit lists of the seeding stage: nothing here reads it
    TRY(upload_ctx(m, &own, nreads, &cd));
  }
  const Batch &b = m->b;
  hipStream_t s = m->stream;
  MapPar p;
  TRY(begin_call(m, quals ? m->d_quals : nullptr, m->d_off, nreads, par, ctx ? &cd : nullptr, false, &p));
  const uint32_t tot32 = (uint32_t)tot;
  for (int i = 0; i <= T_REPLAY; i++) HIPCHK(hipEventRecord(m->ev[i], s));
  int rv = launch_encode(s, m->d_bases, m->d_off, nreads, m->d_codes, m->d_codes_rc);
  hipError_t he = hipSuccess;
  if (nreads) {
    he = hipMemsetAsync(b.hi, 0, 2 * (size_t)nreads * sizeof(HitInfoHdr), s);           // no seeding ran: nhit / nhit_tot come back 0
    if (he == hipSuccess) he = hipMemcpyAsync(b.ch, ch.data(), (size_t)nreads * sizeof(CandHdr), hipMemcpyHostToDevice, s);
    if (he == hipSuccess && tot) he = hipMemcpyAsync(b.rcpool, rc.data(), (size_t)tot * sizeof(RCand), hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipMemcpyAsync(b.rc_count, &tot32, sizeof(tot32), hipMemcpyHostToDevice, s);
  }
  if (he == hipSuccess && !rv) rv = launch_replay(s, b, d, p);
  if (he == hipSuccess) he = hipEventRecord(m->ev[T_ALIGN], s);
  const int passflg = (int)(flags & SMALTGPU_ALIGN_CANDS_ANTIDIAG);
  if (he == hipSuccess && !rv) rv = launch_align(s, b, d, p, m->align_scr, m->align_bytes, m->align_slots, m->wincap, m->dircap, m->rescap_slot, m->dstrcap_slot, 1 | passflg);
  if (he == hipSuccess && !rv) rv = launch_align(s, b, d, p, m->align_scr2, m->align_bytes2, m->align_slots2, m->wincap, m->dircap2, m->rescap_slot2, m->dstrcap_slot2, 2 | passflg);
  if (he == hipSuccess) he = hipEventRecord(m->ev[T_NUM], s);
  const hipError_t hs = hipStreamSynchronize(s);           // before any return: the uploads read ch, rc and tot32
  HIPCHK(he);
  if (rv) return fail(SMALTGPU_ENODEV, "kernel launch failed: %s", hipGetErrorString((hipError_t)rv));
  HIPCHK(hs);
  uint32_t nretry = 0;
  TRY(fetch(m->h_ctl, b.ctl, nreads));
  HIPCHK(hipMemcpy(&nretry, b.align_retry_n, sizeof(nretry), hipMemcpyDeviceToHost));
  memset(out, 0, sizeof(*out));
  out->ctl = (const smaltgpu_readctl *)m->h_ctl.data(); out->n_deferred = nretry;
  return smaltgpu_fetch_results(m, &out->batch);
}

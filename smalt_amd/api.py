"""ctypes binding of libsmaltgpu.so (C ABI in include/smaltgpu.h) and the host-side mirror of the
reference's per-read mapping interface (rmap.h:83-145): `Index` stands for the (HashTable,
SeqSet) pair that `rmapCreate` receives, `Mapper` for the `RMap`, `Mapper.map_batch` for a
block of `rmapSingle` calls followed by `rmapGetData`.

There is no CPU fallback: if the HIP library is missing or no device is present every call
raises `SmaltGpuError`.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(HERE, "libsmaltgpu.so")

FLG_CMPLXW, FLG_BEST, FLG_SEQBYSEQ, FLG_NOSHRTINFO, FLG_SENSITIVE = 0x01, 0x02, 0x10, 0x20, 0x80
# codes of stat[].errcode (and of the mapping calls: the first one among the batch's reads)
ECAP, EINTERNAL, ESCORE, ECPLX = -5, -6, -8, -9


class SmaltGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("smaltgpu error %d: %s" % (code, msg))
        self.code = code


class IndexDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("s", C.c_int32), ("typ", C.c_int32), ("nbits_key", C.c_int32), ("nbits_lo", C.c_int32),
                ("npos", C.c_uint32), ("nwords", C.c_uint32), ("idx", C.c_void_p), ("pos", C.c_void_p),
                ("wordidx", C.c_void_p), ("posidx", C.c_void_p), ("nseq", C.c_int64), ("sop", C.c_void_p),
                ("packed", C.c_void_p), ("on_device", C.c_int32)]


class FastaView(C.Structure):          # smaltgpu_fasta_view
    _fields_ = [("nseq", C.c_int64), ("names", C.POINTER(C.c_char_p)), ("seq_off", C.POINTER(C.c_uint64)), ("bases", C.POINTER(C.c_uint8)),
                ("upload_ms", C.c_float), ("parse_ms", C.c_float), ("step_ms", C.c_float * 3)]


class Params(C.Structure):
    _fields_ = [("ktuple_maxhit", C.c_int32), ("min_cover", C.c_uint32), ("min_swatscor", C.c_int32),
                ("min_swatscor_below_max", C.c_int32), ("min_basqval", C.c_int32), ("target_depth", C.c_int32),
                ("max_depth", C.c_int32), ("rmapflg", C.c_uint32), ("match", C.c_int32), ("mismatch", C.c_int32),
                ("gap_init", C.c_int32), ("gap_ext", C.c_int32), ("min_cover_frac", C.c_double)]


class Result(C.Structure):
    _fields_ = [("swatscor", C.c_int32), ("q_start", C.c_uint32), ("q_end", C.c_uint32), ("s_start", C.c_uint64),
                ("s_end", C.c_uint64), ("sidx", C.c_int32), ("reverse", C.c_uint32), ("stroffs", C.c_uint32),
                ("strlen", C.c_uint32)]


class ReadStat(C.Structure):
    _fields_ = [("swatscor_max", C.c_int32), ("swatscor_2ndmax", C.c_int32), ("n_ali_done", C.c_int32),
                ("n_ali_tot", C.c_int32), ("n_hits_used", C.c_uint32), ("n_hits_tot", C.c_uint32),
                ("errcode", C.c_int32), ("nres", C.c_uint32), ("max1scor", C.c_int32), ("errsite", C.c_int32)]


class Interval(C.Structure):
    _fields_ = [("sidx", C.c_int32), ("lo", C.c_uint32), ("hi", C.c_uint32)]


class CallCtx(C.Structure):
    _fields_ = [("iv_off", C.POINTER(C.c_uint64)), ("iv", C.POINTER(Interval)), ("min_swatscor", C.POINTER(C.c_int32)),
                ("prev_max", C.POINTER(C.c_int32)), ("fine_index", C.c_int32), ("raw_alignments", C.c_int32), ("hitlist_len", C.POINTER(C.c_uint32)), ("seed_range", C.POINTER(C.c_uint32))]


class PostResult(C.Structure):
    _fields_ = [("swatscor", C.c_int32), ("q_start", C.c_uint32), ("q_end", C.c_uint32), ("s_start", C.c_uint64), ("s_end", C.c_uint64),
                ("sidx", C.c_int32), ("status", C.c_uint32), ("mapscor", C.c_int32), ("prob", C.c_double), ("rsltx", C.c_int16),
                ("qsegx", C.c_int16), ("swrank", C.c_int16), ("pad", C.c_int16), ("stroffs", C.c_uint32), ("strlen", C.c_uint32)]


class PostOut(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("res_off", C.POINTER(C.c_uint64)), ("res", C.POINTER(PostResult)), ("diffstr", C.POINTER(C.c_uint8)),
                ("sort_off", C.POINTER(C.c_uint64)), ("sortr", C.POINTER(C.c_int32)), ("segsrtr", C.POINTER(C.c_int32)),
                ("seg_off", C.POINTER(C.c_uint64)), ("segnor", C.POINTER(C.c_int32)), ("qsegno", C.POINTER(C.c_int32)),
                ("setstatus", C.POINTER(C.c_uint32)), ("needs_reference", C.POINTER(C.c_int32))]


class ReadsView(C.Structure):          # smaltgpu_reads_view
    _fields_ = [("nreads", C.c_uint32), ("has_qual", C.c_uint32), ("bases", C.POINTER(C.c_uint8)), ("quals", C.POINTER(C.c_uint8)),
                ("read_off", C.POINTER(C.c_uint64)), ("names", C.POINTER(C.c_char)), ("name_off", C.POINTER(C.c_uint64)), ("consumed", C.c_uint64)]


class ReadsDeviceView(C.Structure):    # smaltgpu_reads_device_view
    _fields_ = [("d_bases", C.c_void_p), ("d_quals", C.c_void_p), ("d_read_off", C.c_void_p), ("nreads", C.c_uint32), ("has_qual", C.c_uint32),
                ("total_bases", C.c_uint64), ("consumed", C.c_uint64)]


IN_SAM, IN_BAM = 1, 2                  # smaltgpu_alnreads_create (smalt map -F sam | bam)


class ReportOpts(C.Structure):         # smaltgpu_report_opts
    _fields_ = [("format", C.c_int32), ("modflags", C.c_uint32), ("outflags", C.c_uint32), ("min_swscor", C.c_int32),
                ("min_swscor_below_max", C.c_int32), ("min_identity", C.c_double)]


FMT_CIGAR, FMT_SAM, FMT_SSAHA, FMT_BAM = 0, 1, 2, 3
REP_ALIOUT, REP_SOFTCLIP, REP_HEADER, REP_XMISMATCH = 0x01, 0x02, 0x04, 0x08
OUT_BEST, OUT_SINGLE, OUT_SPLIT, OUT_RANDSEL = 0x01, 0x02, 0x04, 0x08


class PairOpts(C.Structure):           # smaltgpu_pair_opts
    _fields_ = [("insert_min", C.c_int32), ("insert_max", C.c_int32), ("library", C.c_int32), ("every_pair", C.c_int32), ("nthreads", C.c_int32)]


class PairInfo(C.Structure):           # smaltgpu_pair_info
    _fields_ = [("pairflg", C.c_uint8), ("rounds", C.c_uint8), ("nali", C.c_uint16 * 2)]


LIB_PE, LIB_MP, LIB_PP, LIB_ANY = 1, 2, 3, 4


class ResidentReads(C.Structure):      # smaltgpu_resident_reads
    _fields_ = [("d_bases", C.c_void_p * 2), ("d_quals", C.c_void_p * 2), ("d_read_off", C.c_void_p * 2), ("read_off", C.c_void_p * 2), ("nreads", C.c_uint32 * 2)]


class MapperOpts(C.Structure):
    _fields_ = [("cands_per_read", C.c_uint32), ("slot_budget_gb", C.c_uint32)]


class BatchOut(C.Structure):
    _fields_ = [("nreads", C.c_uint32), ("res_off", C.POINTER(C.c_uint64)), ("res", C.POINTER(Result)),
                ("diffstr", C.POINTER(C.c_uint8)), ("stat", C.POINTER(ReadStat))]


class BandNode(C.Structure):           # smaltgpu_band_node
    _fields_ = [("status", C.c_int32), ("score", C.c_int32), ("max_i", C.c_int32), ("max_j", C.c_int32), ("qs", C.c_int32),
                ("rs", C.c_int32), ("dlen", C.c_int32), ("stroffs", C.c_uint32)]


class HitsOut(C.Structure):            # smaltgpu_hits_out
    _fields_ = [("nstrands", C.c_uint32), ("stride", C.c_uint32), ("window", C.c_uint32), ("tab", C.c_uint32),
                ("n_seeds", C.POINTER(C.c_uint32)), ("seed_rank", C.POINTER(C.c_uint32)), ("status", C.POINTER(C.c_uint32)),
                ("seeds", C.c_void_p), ("qmask", C.c_void_p), ("runs", C.c_void_p),
                ("hit_count", C.c_uint64), ("pool_cap", C.c_uint64), ("pool", C.c_void_p)]


class FineOut(C.Structure):            # smaltgpu_fine_out
    _fields_ = [("nreads", C.c_uint32), ("idx_stride", C.c_uint32), ("nkeys", C.c_uint32), ("npos", C.c_uint64),
                ("fine_off", C.c_void_p), ("idx", C.c_void_p), ("pos", C.c_void_p)]


class SeedOut(C.Structure):            # smaltgpu_seed_out
    _fields_ = [("codes", C.c_void_p), ("codes_rc", C.c_void_p), ("hi", C.c_void_p), ("seeds", C.c_void_p), ("qmask", C.c_void_p),
                ("nrows", C.c_uint32), ("stride", C.c_uint32), ("in_lds", C.c_uint32), ("grid", C.c_uint32), ("lookups", C.c_uint64)]


class Cand(C.Structure):               # smaltgpu_cand
    _fields_ = [("rs", C.c_uint64), ("re", C.c_uint64), ("qs", C.c_uint32), ("qe", C.c_uint32), ("band_l", C.c_int32), ("band_r", C.c_int32),
                ("sqidx", C.c_int32), ("flags", C.c_uint32), ("cover", C.c_uint32), ("swscor", C.c_int32)]


class ReadCtl(C.Structure):            # smaltgpu_readctl
    _fields_ = [("max1", C.c_int32), ("max2", C.c_int32), ("n_scored", C.c_int32), ("bandwidth_min", C.c_int32), ("min_swatscor", C.c_int32),
                ("scorlen_min", C.c_int32), ("go", C.c_int32), ("pad", C.c_int32)]


class AlignCandsOut(C.Structure):      # smaltgpu_align_cands_out
    _fields_ = [("batch", BatchOut), ("ctl", C.POINTER(ReadCtl)), ("n_deferred", C.c_uint32)]


class PoolRec(C.Structure):            # smaltgpu_pool_rec
    _fields_ = [("rs", C.c_uint64), ("re", C.c_uint64), ("qs", C.c_uint32), ("qe", C.c_uint32), ("band_l", C.c_int32), ("band_r", C.c_int32),
                ("sqidx", C.c_int32), ("flags", C.c_uint32), ("cover", C.c_uint32), ("swscor", C.c_int32), ("rid", C.c_uint32), ("pad", C.c_uint32)]


class ScorePoolOut(C.Structure):       # smaltgpu_score_pool_out
    _fields_ = [("rec", C.POINTER(PoolRec)), ("nrec", C.c_uint32), ("rc_count", C.c_uint32), ("rccap", C.c_uint32), ("long_cap", C.c_uint32),
                ("strip_cap", C.c_uint32), ("tile_qmax", C.c_uint32), ("wincap", C.c_uint32), ("tile_g", C.c_uint32), ("tile_c", C.c_uint32),
                ("full_grid", C.c_uint32), ("strip_grid", C.c_uint32)]


RCF_REVERSE, RCF_SCORED, RCF_BANDED, RCF_ERR, RCF_QN, RCF_BSCORED = 1, 2, 4, 8, 16, 32      # SMALTGPU_RCF_*
CAND_REVERSE, CAND_ERR = 1, 2                                  # SMALTGPU_CAND_*
ALIGN_CANDS_ANTIDIAG = 0x100                                   # SMALTGPU_ALIGN_CANDS_ANTIDIAG
HITRUN_NONE, HITRUN_SORTED, HITRUN_OVERFLOW = 0, 1, 2         # SMALTGPU_HITRUN_*
SORT_REG4, SORT_REG8, SORT_REG16, SORT_LDS, SORT_HBM, SORT_CHUNKED = 0, 1, 2, 3, 4, 5        # forms of smaltgpu_sort_u64_batch

# SMALTGPU_BAND_*: the forms of the K3 band pass (smaltgpu_band_align_nodes)
BAND_ROWS, BAND_ANTIDIAG, BAND_WAVE2, BAND_WAVE4, BAND_WAVE7, BAND_WAVE12, BAND_STRIP8, BAND_STRIP16, BAND_SCALAR = range(9)
NODE_ALIGNED, NODE_REFUSED, NODE_BELOW = 0, 1, 2
ESCORE, EINTERNAL = -8, -6
BAND_GEO_FIELDS = ("band_width", "l_edge_orig", "r_edge_orig", "l_edge", "r_edge", "s_left_orig", "s_left", "s_len", "s_totlen",
                   "q_left_orig", "q_left", "q_len", "q_totlen", "form")


def band_geometry(band_l, band_r, qs, qe, qlen, s_left, s_right, wlen, gap_init, gap_ext):
    """Host only: the band of a K3 node as the kernels set it up and the form the mapper picks for it; None if refused."""
    geo = (C.c_int32 * 14)()
    rv = lib().smaltgpu_band_geometry(band_l, band_r, qs, qe, qlen, s_left, s_right, wlen, gap_init, gap_ext, geo)
    if rv < 0:
        _check(rv)
    return None if rv else dict(zip(BAND_GEO_FIELDS, list(geo)))


def _offsets(seqs):
    off = (C.c_uint32 * (len(seqs) + 1))()
    a = 0
    for i, s in enumerate(seqs):
        off[i] = a
        a += len(s)
    off[len(seqs)] = a
    return off


_lib = None


def lib():
    """Load libsmaltgpu.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise SmaltGpuError(-1, "libsmaltgpu.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        try:                       # torch bundles its own HIP runtime: load it first so that one runtime serves both
            import torch  # noqa: F401
        except Exception:          # torch is plumbing for bench/tests, not a dependency of the library
            pass
        L = C.CDLL(LIBPATH)
        L.smaltgpu_last_error.restype = C.c_char_p
        L.smaltgpu_timer_name.restype = C.c_char_p
        L.smaltgpu_index_load.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_int]
        L.smaltgpu_index_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(IndexDesc), C.c_int]
        L.smaltgpu_index_free.argtypes = [C.c_void_p]
        L.smaltgpu_index_build.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p), C.c_int64,
                                           C.c_int32, C.c_int32, C.POINTER(C.c_float)]
        L.smaltgpu_index_build_device.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_char_p), C.c_int64,
                                                  C.c_int32, C.c_int32, C.POINTER(C.c_float)]
        L.smaltgpu_index_save.argtypes = [C.c_void_p, C.c_char_p]
        L.smaltgpu_index_build_text.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(C.c_float),
                                                C.POINTER(C.c_float)]
        L.smaltgpu_fasta_parse.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_char_p, C.c_uint64, C.POINTER(FastaView)]
        L.smaltgpu_index_build_text_ex.argtypes = L.smaltgpu_index_build_text.argtypes + [C.c_uint32]
        L.smaltgpu_fasta_parse_ex.argtypes = L.smaltgpu_fasta_parse.argtypes + [C.c_uint32]
        L.smaltgpu_fasta_free.argtypes = [C.c_void_p]
        L.smaltgpu_index_info.argtypes = [C.c_void_p, C.POINTER(IndexDesc)]
        L.smaltgpu_params_default.argtypes = [C.POINTER(Params), C.c_void_p]
        L.smaltgpu_mapper_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint32]
        L.smaltgpu_mapper_create_ex.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(MapperOpts)]
        L.smaltgpu_index_clone.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
        L.smaltgpu_mapper_free.argtypes = [C.c_void_p]
        L.smaltgpu_map_batch.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32,
                                         C.POINTER(Params), C.POINTER(BatchOut)]
        L.smaltgpu_map_batch_ctx.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32,
                                             C.POINTER(Params), C.POINTER(CallCtx), C.POINTER(BatchOut)]
        L.smaltgpu_hit_totals.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(Params), C.POINTER(C.c_uint32)]
        L.smaltgpu_post_create.restype = C.c_void_p
        L.smaltgpu_post_free.argtypes = [C.c_void_p]
        L.smaltgpu_postprocess.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64, C.POINTER(BatchOut), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                           C.c_void_p, C.POINTER(Params), C.c_int, C.POINTER(PostOut)]
        L.smaltgpu_reads_create.restype = C.c_void_p
        L.smaltgpu_reads_free.argtypes = [C.c_void_p]
        L.smaltgpu_reads_parse.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_uint32, C.c_int, C.POINTER(ReadsView)]
        L.smaltgpu_reads_dev_create.restype = C.c_void_p
        L.smaltgpu_reads_dev_create.argtypes = [C.c_int]
        L.smaltgpu_reads_dev_free.argtypes = [C.c_void_p]
        L.smaltgpu_reads_parse_device.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(ReadsView), C.POINTER(ReadsDeviceView)]
        L.smaltgpu_reads_dev_configure.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        L.smaltgpu_reads_dev_readback.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.smaltgpu_map_split.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(Params), C.c_void_p, C.c_int,
                                         C.POINTER(PostOut), C.POINTER(C.c_uint32)]
        L.smaltgpu_report_create.restype = C.c_void_p
        L.smaltgpu_report_free.argtypes = [C.c_void_p]
        L.smaltgpu_report_header.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.c_int64, C.POINTER(ReportOpts), C.c_char_p, C.c_char_p,
                                             C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.smaltgpu_report_emit.argtypes = [C.c_void_p, C.POINTER(PostOut), C.POINTER(BatchOut), C.POINTER(ReadsView), C.POINTER(C.c_char_p), C.c_int64,
                                           C.POINTER(ReportOpts), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.smaltgpu_pairs_create.restype = C.c_void_p
        L.smaltgpu_pairs_free.argtypes = [C.c_void_p]
        L.smaltgpu_map_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(Params),
                                         C.POINTER(PairOpts), C.c_void_p]
        L.smaltgpu_pairs_timers.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.smaltgpu_map_pairs_resident.argtypes = [C.c_void_p, C.POINTER(ResidentReads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(Params),
                                                  C.POINTER(PairOpts), C.c_void_p]
        L.smaltgpu_pairs_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.POINTER(PairInfo)), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.smaltgpu_report_emit_pairs.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(ReadsView), C.POINTER(ReadsView), C.POINTER(C.c_char_p), C.c_int64,
                                                 C.POINTER(ReportOpts), C.POINTER(PairOpts), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.smaltgpu_index_seqnames.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_char_p)), C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int64)]
        L.smaltgpu_map_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                                C.POINTER(Params)]
        L.smaltgpu_map_batch_ctx_resident.argtypes = [C.c_void_p, C.POINTER(ResidentReads), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Params),
                                                      C.POINTER(CallCtx), C.POINTER(BatchOut)]
        L.smaltgpu_hit_totals_resident.argtypes = [C.c_void_p, C.POINTER(ResidentReads), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Params), C.POINTER(C.c_uint32)]
        L.smaltgpu_mapper_set_host_threads.argtypes = [C.c_void_p, C.c_int]
        L.smaltgpu_mapper_remap_batches.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.smaltgpu_fetch_begin.argtypes = [C.c_void_p]
        L.smaltgpu_fetch_end.argtypes = [C.c_void_p, C.POINTER(BatchOut)]
        L.smaltgpu_fetch_results.argtypes = [C.c_void_p, C.POINTER(BatchOut)]
        L.smaltgpu_synchronize.argtypes = [C.c_void_p]
        L.smaltgpu_timers.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.smaltgpu_set_debug.argtypes = [C.c_void_p, C.c_int]
        L.smaltgpu_dump_read.restype = C.c_long
        L.smaltgpu_dump_read.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_size_t]
        L.smaltgpu_sw_full_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p,
                                             C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(Params), C.POINTER(C.c_int32), C.c_int]
        L.smaltgpu_sw_band_batch.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32,
                                             C.POINTER(Params), C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.smaltgpu_band_align_nodes.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_char_p, C.POINTER(C.c_uint32), C.c_uint32,
                                                C.POINTER(Params), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(BandNode), C.c_char_p]
        L.smaltgpu_band_geometry.argtypes = [C.c_int] * 10 + [C.POINTER(C.c_int32)]
        L.smaltgpu_sw_rowframe_max_steps.argtypes = [C.c_int] * 5
        L.smaltgpu_sw_pairframe_max_steps.argtypes = [C.c_int] * 5
        L.smaltgpu_rank_sort_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.smaltgpu_seed_batch.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(Params), C.c_void_p, C.c_int, C.c_int,
                                          C.c_uint32, C.c_uint8, C.POINTER(SeedOut)]
        L.smaltgpu_gather_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_void_p,
                                            C.c_uint32, C.c_uint8, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.smaltgpu_hits_batch.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(Params), C.c_uint32, C.c_uint64,
                                          C.POINTER(HitsOut)]
        L.smaltgpu_hits_windows.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64)]
        L.smaltgpu_align_cands_batch.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(Params), C.POINTER(CallCtx),
                                                 C.POINTER(C.c_uint64), C.POINTER(Cand), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(AlignCandsOut)]
        L.smaltgpu_fine_index_batch.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(Interval), C.c_uint32, C.c_uint32, C.POINTER(FineOut)]
        L.smaltgpu_cands_geometry.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.smaltgpu_score_pool.argtypes = [C.c_void_p, C.POINTER(ScorePoolOut)]
        L.smaltgpu_sort_u64_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
        L.smaltgpu_sample_interval.argtypes = [C.c_uint64, C.c_int]
        L.smaltgpu_inshist_from_sample.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_uint64]
        L.smaltgpu_inshist_read.argtypes = [C.POINTER(C.c_void_p), C.c_char_p]
        L.smaltgpu_inshist_free.argtypes = [C.c_void_p]
        L.smaltgpu_inshist_text.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.smaltgpu_inshist_bounds.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        L.smaltgpu_inshist_count.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.smaltgpu_report_set_inshist.argtypes = [C.c_void_p, C.c_void_p]
        L.smaltgpu_index_packed_host.restype = C.c_void_p
        L.smaltgpu_index_packed_host.argtypes = [C.c_void_p]
        L.smaltgpu_report_set_reference.argtypes = [C.c_void_p, C.c_void_p]      # the packed host copy (smaltgpu_index_packed_host) for REP_ALIOUT
        L.smaltgpu_report_pair_inserts.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32)]
        L.smaltgpu_report_finish.argtypes = [C.c_void_p, C.POINTER(ReportOpts), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]      # FMT_BAM: the end-of-file block
        L.smaltgpu_alnreads_create.restype = C.c_void_p                                                                             # reads from SAM / BAM files
        L.smaltgpu_alnreads_create.argtypes = [C.c_int]
        L.smaltgpu_alnreads_free.argtypes = [C.c_void_p]
        L.smaltgpu_alnreads_feed.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
        L.smaltgpu_alnreads_take.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int), C.POINTER(ReadsView), C.POINTER(ReadsView)]
        L.smaltgpu_alnreads_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _lib = L
    return _lib


def _check(rv):
    if rv != 0:
        raise SmaltGpuError(rv, lib().smaltgpu_last_error().decode())


def device_count() -> int:
    return lib().smaltgpu_device_count()


HIST_SAMPLED, HIST_SMOOTHED, HIST_SECTION = 0, 1, 2


def sample_interval(npairs: int, every: int = 100) -> int:
    """Every how many pairs `smalt sample -u every` maps one (insSetSamplingInterval, insert.c:192-205)."""
    return lib().smaltgpu_sample_interval(npairs, every)


def _fasta_text(path_or_bytes) -> bytes:
    """the text of a FASTA file: bytes as they are, a path read whole (through gzip when the file is compressed)"""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, "rb") as f:
        raw = f.read()
    if raw[:2] == b"\x1f\x8b":
        import gzip
        raw = gzip.decompress(raw)
    return raw


TEXT_FASTQ = 1                         # SMALTGPU_TEXT_FASTQ


def parse_fasta(path_or_bytes, device: int = 0, fastq: bool = False):
    """The reference sequences of a FASTA text as `smalt index` reads them, parsed on the device (smaltgpu_fasta_parse):
    -> (names, sequences, times) with times = dict(upload_ms, parse_ms, step_ms).  Names are the whole header lines.
    fastq: a text with '@' or '+' prompts is read as FASTQ records, qualities discarded (smaltgpu_fasta_parse_ex)."""
    text = _fasta_text(path_or_bytes)
    h, v = C.c_void_p(), FastaView()
    if fastq:
        _check(lib().smaltgpu_fasta_parse_ex(C.byref(h), device, text, len(text), C.byref(v), TEXT_FASTQ))
    else:
        _check(lib().smaltgpu_fasta_parse(C.byref(h), device, text, len(text), C.byref(v)))
    try:
        names = [v.names[i].decode("latin-1") for i in range(v.nseq)]
        base = C.addressof(v.bases.contents) if v.nseq else 0
        seqs = [C.string_at(base + v.seq_off[i], v.seq_off[i + 1] - v.seq_off[i]) for i in range(v.nseq)]
        times = dict(upload_ms=float(v.upload_ms), parse_ms=float(v.parse_ms), step_ms=[float(x) for x in v.step_ms])
    finally:
        lib().smaltgpu_fasta_free(h)
    return names, seqs, times


class InsertHistogram:
    """Histogram of the insert sizes of a read-pair library (smaltgpu_inshist): what `smalt sample` writes and
    `smalt map -g` reads.  Host code; needs no device."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def from_sample(cls, sizes: Sequence[int]) -> "InsertHistogram":
        arr = (C.c_int32 * max(1, len(sizes)))(*sizes)
        h = C.c_void_p()
        _check(lib().smaltgpu_inshist_from_sample(C.byref(h), arr, len(sizes)))
        return cls(h)

    @classmethod
    def read(cls, path: str) -> "InsertHistogram":
        h = C.c_void_p()
        _check(lib().smaltgpu_inshist_read(C.byref(h), os.fsencode(path)))
        return cls(h)

    def text(self, what: int = HIST_SECTION, width: int = 80) -> bytes:
        """HIST_SAMPLED / HIST_SMOOTHED: the bar print with lines of at most `width` bars; HIST_SECTION: the file section."""
        t, n = C.c_void_p(), C.c_uint64()
        _check(lib().smaltgpu_inshist_text(self.h, what, width, C.byref(t), C.byref(n)))
        return C.string_at(t.value, n.value) if n.value else b""

    def bounds(self):
        """-> (smallest insert size, largest insert size, number of bins, number of sizes counted)"""
        lo, hi, nb, tot = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        _check(lib().smaltgpu_inshist_bounds(self.h, C.byref(lo), C.byref(hi), C.byref(nb), C.byref(tot)))
        return lo.value, hi.value, nb.value, tot.value

    def count(self, insert_size: int, smoothed: bool = True):
        """-> (count of the bin of insert_size, cumulative count up to and including that bin)"""
        c, cc = C.c_int32(), C.c_int32()
        _check(lib().smaltgpu_inshist_count(self.h, insert_size, 1 if smoothed else 0, C.byref(c), C.byref(cc)))
        return c.value, cc.value

    def close(self):
        if self.h:
            lib().smaltgpu_inshist_free(self.h)
            self.h = None


class ReadsDevice:
    """FASTQ / FASTA text parsed on the device into a resident batch (smaltgpu_reads_parse_device): every rule is the one of the
    host parser (smaltgpu_reads_parse), whatever the shape of the records."""

    def __init__(self, device: int = 0):
        self.h = C.c_void_p(lib().smaltgpu_reads_dev_create(device))
        if not self.h:
            raise SmaltGpuError(-1, lib().smaltgpu_last_error().decode())
        self.raw = None

    def configure(self, block_bytes: int = 0, max_groups: int = 0, guard_bytes: int = 0):
        """tests and measurements: bytes of text per workgroup, a cap on the workgroups over the prompts, a guard behind the device arrays"""
        _check(lib().smaltgpu_reads_dev_configure(self.h, block_bytes, max_groups, guard_bytes))
        self.guard = guard_bytes

    def parse_raw(self, data: bytes, is_last: bool = True, max_reads: int = 0, host: bool = True):
        """-> (ReadsView or None, ReadsDeviceView); the arrays belong to the handle and hold until the next parse"""
        hv, dv = ReadsView(), ReadsDeviceView()
        _check(lib().smaltgpu_reads_parse_device(self.h, data, len(data), 1 if is_last else 0, max_reads, C.byref(hv) if host else None, C.byref(dv)))
        self.raw = (hv if host else None, dv)
        return self.raw

    def parse(self, data: bytes, is_last: bool = True, max_reads: int = 0):
        """-> (host, dev).  host: dict(names, reads, quals (None without qualities), read_off, has_qual, consumed) as the host parser
        returns them.  dev: a ResidentReads whose side 0 is the batch in HBM (d_bases, d_quals, d_read_off, the offsets in host
        memory, nreads), with .total_bases beside it: what map_batch_device and map_batch_ctx_resident take.  dev holds until the
        next parse on this object."""
        hv, dv = self.parse_raw(data, is_last, max_reads)
        n = hv.nreads
        off = [hv.read_off[i] for i in range(n + 1)]
        bases = C.string_at(hv.bases, off[n]) if off[n] else b""
        quals = C.string_at(hv.quals, off[n]) if (hv.has_qual and off[n]) else b""
        names = C.string_at(hv.names, hv.name_off[n]).split(b"\0")[:-1] if n else []
        host = dict(names=names, reads=[bases[off[i]:off[i + 1]] for i in range(n)], quals=[quals[off[i]:off[i + 1]] for i in range(n)] if hv.has_qual else None,
                    read_off=off, has_qual=bool(hv.has_qual), consumed=int(hv.consumed))
        dev = ResidentReads()
        self._host_off = (C.c_uint64 * (n + 1))(*off)
        dev.d_bases[0], dev.d_quals[0], dev.d_read_off[0] = dv.d_bases, dv.d_quals, dv.d_read_off
        dev.read_off[0] = C.cast(self._host_off, C.c_void_p).value
        dev.nreads[0] = n
        dev.total_bases = int(dv.total_bases)
        return host, dev

    def readback(self, which: int):
        """array `which` (0 bases, 1 qualities, 2 offsets) of the last parse as it lies in HBM -> (its bytes, the guard behind them, launches)"""
        _, dv = self.raw
        cap = (int(dv.total_bases) if which < 2 else (dv.nreads + 1) * 8) + getattr(self, "guard", 0) + 16
        buf, n, launches = C.create_string_buffer(cap), C.c_uint64(), C.c_uint32()
        _check(lib().smaltgpu_reads_dev_readback(self.h, which, buf, cap, C.byref(n), C.byref(launches)))
        return buf.raw[:n.value], buf.raw[n.value:n.value + getattr(self, "guard", 0)], launches.value

    def close(self):
        if self.h:
            lib().smaltgpu_reads_dev_free(self.h)
            self.h = None


class AlnReads:
    """Reads from a SAM or BAM file (smaltgpu_alnreads; `smalt map -F sam|bam`): single reads and pairs, collated over the whole
    input.  feed() takes the next bytes of the file, take() hands out runs of templates of one kind.  Host code; needs no device."""

    def __init__(self, fmt: int):
        self.h = lib().smaltgpu_alnreads_create(fmt)
        if not self.h:
            raise SmaltGpuError(-3, lib().smaltgpu_last_error().decode())
        self.reads, self.mates = ReadsView(), ReadsView()

    def feed(self, data: bytes, is_last: bool, nthreads: int = 1) -> int:
        """-> how many of the bytes were used (whole SAM lines, whole BGZF blocks): the next call starts from there"""
        used = C.c_uint64()
        _check(lib().smaltgpu_alnreads_feed(self.h, data, len(data), 1 if is_last else 0, nthreads, C.byref(used)))
        return used.value

    def take(self, max_templates: int = 0):
        """-> (kind, reads, mates): kind 0 none ready, 1 single reads, 2 pairs; the two ReadsView hold until the next take"""
        kind = C.c_int()
        _check(lib().smaltgpu_alnreads_take(self.h, max_templates, C.byref(kind), C.byref(self.reads), C.byref(self.mates)))
        return kind.value, self.reads, self.mates

    def times(self):
        """-> seconds spent so far: (BGZF blocks inflated, records decoded and collated, runs copied out)"""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(lib().smaltgpu_alnreads_times(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        if self.h:
            lib().smaltgpu_alnreads_free(self.h)
            self.h = None


class Index:
    """Index image resident in HBM (replaces hashTableRead + seqSetReadBinFil)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def load(cls, prefix: str, device: int = 0) -> "Index":
        h = C.c_void_p()
        _check(lib().smaltgpu_index_load(C.byref(h), prefix.encode(), device))
        return cls(h)

    @classmethod
    def from_desc(cls, desc: IndexDesc, device: int = 0) -> "Index":
        h = C.c_void_p()
        _check(lib().smaltgpu_index_create(C.byref(h), C.byref(desc), device))
        return cls(h)

    @classmethod
    def build(cls, seqs: Sequence[bytes], names: Sequence[str], k: int, s: int, device: int = 0) -> "Index":
        """Build the index image on the device from reference sequences (replaces `smalt index`: hashTableSetUp
        hashidx.c:829-998 + seqSetCompress sequence.c:1360-1424).  `build_ms` holds the device time."""
        cat = b"".join(seqs)
        off = (C.c_uint64 * (len(seqs) + 1))()
        o = 0
        for i, q in enumerate(seqs):
            off[i] = o
            o += len(q)
        off[len(seqs)] = o
        nm = (C.c_char_p * len(seqs))(*[n.encode() for n in names])
        h = C.c_void_p()
        ms = C.c_float(0.0)
        _check(lib().smaltgpu_index_build(C.byref(h), device, cat, off, nm, C.c_int64(len(seqs)), k, s, C.byref(ms)))
        ix = cls(h)
        ix.build_ms = float(ms.value)
        return ix

    @classmethod
    def from_fasta(cls, path_or_bytes, k: int = 13, s: int = 6, device: int = 0, fastq: bool = False) -> "Index":
        """Build the index image from the text of a FASTA file (`smalt index`): a path (plain or gzipped) or the text itself.
        The text is parsed on the device by the reference's rules (smaltgpu_index_build_text); `parse_ms` and `build_ms` hold
        the device times of the parse and of the construction.  fastq: a text with '@' or '+' prompts is read as FASTQ
        records, as `smalt index` does (smaltgpu_index_build_text_ex with SMALTGPU_TEXT_FASTQ); without it such a text is refused."""
        text = _fasta_text(path_or_bytes)
        h = C.c_void_p()
        pms, bms = C.c_float(0.0), C.c_float(0.0)
        if fastq:
            _check(lib().smaltgpu_index_build_text_ex(C.byref(h), device, text, len(text), k, s, C.byref(pms), C.byref(bms), TEXT_FASTQ))
        else:
            _check(lib().smaltgpu_index_build_text(C.byref(h), device, text, len(text), k, s, C.byref(pms), C.byref(bms)))
        ix = cls(h)
        ix.parse_ms, ix.build_ms = float(pms.value), float(bms.value)
        return ix

    @classmethod
    def build_device(cls, d_bases_ptr: int, seq_off: Sequence[int], names: Sequence[str], k: int, s: int, device: int = 0) -> "Index":
        """Same from bases already in HBM (`d_bases_ptr`: device address of the concatenated sequences)."""
        n = len(names)
        off = (C.c_uint64 * (n + 1))(*[int(x) for x in seq_off])
        nm = (C.c_char_p * n)(*[x.encode() for x in names])
        h = C.c_void_p()
        ms = C.c_float(0.0)
        _check(lib().smaltgpu_index_build_device(C.byref(h), device, C.c_void_p(d_bases_ptr), off, nm, C.c_int64(n), k, s, C.byref(ms)))
        ix = cls(h)
        ix.build_ms = float(ms.value)
        return ix

    def clone(self, device: int) -> "Index":
        """A second image on `device`, copied device to device (xGMI) from this one."""
        h = C.c_void_p()
        _check(lib().smaltgpu_index_clone(C.byref(h), self.h, device))
        return Index(h)

    def save(self, prefix: str) -> None:
        """Write <prefix>.sma / <prefix>.smi, byte-compatible with the reference's index files."""
        _check(lib().smaltgpu_index_save(self.h, prefix.encode()))

    def info(self) -> IndexDesc:
        d = IndexDesc()
        _check(lib().smaltgpu_index_info(self.h, C.byref(d)))
        return d

    def default_params(self) -> Params:
        p = Params()
        lib().smaltgpu_params_default(C.byref(p), self.h)
        return p

    def close(self):
        if self.h:
            lib().smaltgpu_index_free(self.h)
            self.h = None


class Mapper:
    """Work buffers + stream for one host thread (the analogue of an RMap, rmap.h:83)."""

    def __init__(self, index: Index, max_batch_reads: int, max_read_len: int, cands_per_read: int = 0, slot_budget_gb: int = 0):
        self.index = index
        self.h = C.c_void_p()
        opts = MapperOpts(cands_per_read, slot_budget_gb)
        _check(lib().smaltgpu_mapper_create_ex(C.byref(self.h), index.h, max_batch_reads, max_read_len, C.byref(opts)))

    def close(self):
        if self.h:
            lib().smaltgpu_mapper_free(self.h)
            self.h = None

    def set_history(self, on: bool = True):
        """Serial-order mode (smaltgpu_mapper_set_history): consecutive map_batch calls form one serial run of `smalt map -n 0`
        as far as the hit-list capacity goes; calling it again starts a new run."""
        _check(lib().smaltgpu_mapper_set_history(self.h, 1 if on else 0))

    def set_debug(self, level: int):
        _check(lib().smaltgpu_set_debug(self.h, level))

    @staticmethod
    def _pack(reads: Sequence[bytes], quals: Optional[Sequence[bytes]]):
        n = len(reads)
        off = (C.c_uint64 * (n + 1))()
        t = 0
        for i, r in enumerate(reads):
            off[i] = t
            t += len(r)
        off[n] = t
        return b"".join(reads), (b"".join(quals) if quals is not None else None), off

    def map_split(self, reads: Sequence[bytes], quals: Optional[Sequence[bytes]], params: Params, post, nthreads: int = 2):
        """smaltgpu_map_split: both calls of every read (smalt map -p) and the post-call passes.  post: a handle of
        lib().smaltgpu_post_create() that owns the arrays -> (PostOut, number of reads that got a second call)"""
        bases, q, off = self._pack(reads, quals)
        out = PostOut()
        nsec = C.c_uint32()
        _check(lib().smaltgpu_map_split(self.h, post, bases, q, off, len(reads), C.byref(params), self.index.h, nthreads, C.byref(out), C.byref(nsec)))
        return out, nsec.value

    def map_batch(self, reads: Sequence[bytes], quals: Optional[Sequence[bytes]], params: Params, allow_read_errors: bool = False):
        """-> (list per read of result dicts in the reference's raw order, list of stat dicts).
        allow_read_errors: do not raise when single reads failed (device-side limit or the reference's own per-read
        errors ERRCODE_SWATSCOR and, with FLG_CMPLXW, ERRCODE_CPLXSCOR); their stat carries `err` and they have no results."""
        bases, q, off = self._pack(reads, quals)
        out = BatchOut()
        rv = lib().smaltgpu_map_batch(self.h, bases, q, off, len(reads), C.byref(params), C.byref(out))
        if rv != 0 and not (allow_read_errors and rv in (ECAP, EINTERNAL, ESCORE, ECPLX) and out.nreads == len(reads)):
            _check(rv)
        return self._unpack(out)

    @staticmethod
    def _ctx(n, intervals, min_swatscor, prev_max, fine_index, raw_alignments, seed_range):
        """the smaltgpu_callctx of a round over n reads -> (CallCtx, the arrays it points to: keep them until the call returns)"""
        ctx = CallCtx()
        keep = []
        if intervals is not None:
            ivo = (C.c_uint64 * (n + 1))()
            flat = [iv for lst in intervals for iv in lst]
            t = 0
            for i, lst in enumerate(intervals):
                ivo[i] = t
                t += len(lst)
            ivo[n] = t
            arr = (Interval * max(1, len(flat)))(*[Interval(a, b, c) for a, b, c in flat])
            ctx.iv_off, ctx.iv = ivo, arr
            keep += [ivo, arr]
        if min_swatscor is not None:
            ms = (C.c_int32 * max(1, n))(*min_swatscor)
            ctx.min_swatscor = ms
            keep.append(ms)
        if prev_max is not None:
            pm = (C.c_int32 * max(1, 2 * n))(*[x for pr_ in prev_max for x in pr_])
            ctx.prev_max = pm
            keep.append(pm)
        if seed_range is not None:
            sr = (C.c_uint32 * max(1, 2 * n))(*[x for pr_ in seed_range for x in pr_])
            ctx.seed_range = sr
            keep.append(sr)
        ctx.fine_index = 1 if fine_index else 0
        ctx.raw_alignments = 1 if raw_alignments else 0
        return ctx, keep

    def map_batch_ctx(self, reads: Sequence[bytes], quals: Optional[Sequence[bytes]], params: Params, intervals=None, min_swatscor=None,
                      prev_max=None, fine_index: bool = False, raw_alignments: bool = False, seed_range=None, allow_read_errors: bool = False):
        """One round of rmapPair over a batch (smaltgpu_map_batch_ctx): intervals = per read a list of (sidx, lo, hi) or None
        for no restriction at all; min_swatscor = per-read thresholds; prev_max = per read (max, 2ndmax) of the ResultSet
        the call appends to; fine_index = seed against the on-the-fly k=5 index of the intervals; seed_range = per read the
        (first, last) base its k-mer words come from (the second call of a split read); allow_read_errors as in map_batch.
        -> (results, stats, cand_first flags per result)"""
        bases, q, off = self._pack(reads, quals)
        n = len(reads)
        ctx, keep = self._ctx(n, intervals, min_swatscor, prev_max, fine_index, raw_alignments, seed_range)
        out = BatchOut()
        rv = lib().smaltgpu_map_batch_ctx(self.h, bases, q, off, n, C.byref(params), C.byref(ctx), C.byref(out))
        if rv != 0 and not (allow_read_errors and rv in (ECAP, EINTERNAL, ESCORE, ECPLX) and out.nreads == n):
            _check(rv)
        res, stats = self._unpack(out)
        cf = [[bool(out.res[j].reverse & 2) for j in range(out.res_off[i], out.res_off[i + 1])] for i in range(n)]
        return res, stats, cf

    def hit_totals(self, reads: Sequence[bytes], quals: Optional[Sequence[bytes]], params: Params) -> List[int]:
        """calcTotalNumberOfHits (rmap.c:1076) per read: what rmapPair compares to pick the mate it maps first."""
        bases, q, off = self._pack(reads, quals)
        out = (C.c_uint32 * max(1, len(reads)))()
        _check(lib().smaltgpu_hit_totals(self.h, bases, q, off, len(reads), C.byref(params), out))
        return list(out)[:len(reads)]

    def map_batch_ctx_resident(self, src: ResidentReads, ids: Sequence[int], params: Params, intervals=None, min_swatscor=None, prev_max=None,
                               fine_index: bool = False, raw_alignments: bool = False, seed_range=None, allow_read_errors: bool = False):
        """map_batch_ctx over reads of two batches resident in HBM (smaltgpu_map_batch_ctx_resident): read i of the round is read
        ids[i] >> 1 of batch ids[i] & 1 of `src`; the context arguments are indexed like ids.
        -> (results, stats, cand_first flags per result)"""
        n = len(ids)
        ctx, keep = self._ctx(n, intervals, min_swatscor, prev_max, fine_index, raw_alignments, seed_range)
        arr = (C.c_uint32 * max(1, n))(*ids)
        out = BatchOut()
        rv = lib().smaltgpu_map_batch_ctx_resident(self.h, C.byref(src), arr, n, C.byref(params), C.byref(ctx), C.byref(out))
        if rv != 0 and not (allow_read_errors and rv in (ECAP, EINTERNAL, ESCORE, ECPLX) and out.nreads == n):
            _check(rv)
        res, stats = self._unpack(out)
        cf = [[bool(out.res[j].reverse & 2) for j in range(out.res_off[i], out.res_off[i + 1])] for i in range(n)]
        return res, stats, cf

    def hit_totals_resident(self, src: ResidentReads, ids: Sequence[int], params: Params) -> List[int]:
        """hit_totals of the reads `ids` of two batches resident in HBM (smaltgpu_hit_totals_resident)."""
        n = len(ids)
        arr = (C.c_uint32 * max(1, n))(*ids)
        out = (C.c_uint32 * max(1, n))()
        _check(lib().smaltgpu_hit_totals_resident(self.h, C.byref(src), arr, n, C.byref(params), out))
        return list(out)[:n]

    def map_pairs_resident(self, src: ResidentReads, npairs: int, params: Params, popts: PairOpts, bases1=None, quals1=None, bases2=None, quals2=None,
                           pairs_handle=None):
        """smaltgpu_map_pairs_resident: rmapPair for the first npairs pairs of the resident batches `src`; bases / quals are the
        optional host copies (numpy uint8, indexed by src.read_off).  -> as map_pairs_raw"""
        L = lib()
        h = pairs_handle or C.c_void_p(L.smaltgpu_pairs_create())
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        _check(L.smaltgpu_map_pairs_resident(self.h, C.byref(src), ptr(bases1), ptr(quals1), ptr(bases2), ptr(quals2), npairs, C.byref(params), C.byref(popts), h))
        return (h,) + self._pairs_info(h)

    @staticmethod
    def _pairs_info(h):
        import numpy as np
        npairs = C.c_uint32()
        info = C.POINTER(PairInfo)()
        calls = (C.c_uint64 * 4)()
        ms = (C.c_double * 4)()
        _check(lib().smaltgpu_pairs_info(h, C.byref(npairs), C.byref(info), calls, ms))
        arr = np.ctypeslib.as_array(C.cast(info, C.POINTER(C.c_uint8)), shape=(max(1, npairs.value), 6))[:npairs.value]
        return arr, list(calls), list(ms)

    def set_host_threads(self, nthreads: int):
        """host threads for the mapper's own host work: the copy of a batch's results into read order in fetch_end"""
        _check(lib().smaltgpu_mapper_set_host_threads(self.h, nthreads))

    def remap_batches(self) -> int:
        """diagnostic: device batches run so far to map reads again that did not fit a work pool"""
        n = C.c_uint64()
        _check(lib().smaltgpu_mapper_remap_batches(self.h, C.byref(n)))
        return n.value

    def map_pairs_raw(self, bases1, off1, quals1, bases2, off2, quals2, params: Params, popts: PairOpts, pairs_handle=None):
        """smaltgpu_map_pairs on contiguous host arrays (numpy uint8 bases / uint64 offsets per mate file): rmapPair for a block.
        -> (handle of the mapped block, numpy view of smaltgpu_pair_info, calls per round, host ms per round); the handle goes to
        smaltgpu_report_emit_pairs and is freed with lib().smaltgpu_pairs_free (or handed back in as pairs_handle)."""
        import numpy as np
        L = lib()
        h = pairs_handle or C.c_void_p(L.smaltgpu_pairs_create())
        n = len(off1) - 1
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        _check(L.smaltgpu_map_pairs(self.h, ptr(bases1), ptr(quals1), ptr(off1), ptr(bases2), ptr(quals2), ptr(off2), n, C.byref(params), C.byref(popts), h))
        npairs = C.c_uint32()
        info = C.POINTER(PairInfo)()
        calls = (C.c_uint64 * 4)()
        ms = (C.c_double * 4)()
        _check(L.smaltgpu_pairs_info(h, C.byref(npairs), C.byref(info), calls, ms))
        arr = np.ctypeslib.as_array(C.cast(info, C.POINTER(C.c_uint8)), shape=(max(1, npairs.value), 6))[:npairs.value]
        return h, arr, list(calls), list(ms)

    def map_batch_raw(self, bases, off, quals, params: Params) -> BatchOut:
        """smaltgpu_map_batch on contiguous host arrays (numpy uint8 bases / uint64 offsets); the returned
        views stay valid until the next call on this mapper."""
        out = BatchOut()
        _check(lib().smaltgpu_map_batch(self.h, C.cast(bases.ctypes.data, C.c_char_p), None if quals is None else C.cast(quals.ctypes.data, C.c_char_p),
                                        C.cast(off.ctypes.data, C.POINTER(C.c_uint64)), len(off) - 1, C.byref(params), C.byref(out)))
        return out

    @staticmethod
    def _unpack(out: BatchOut):
        res, stats = [], []
        for i in range(out.nreads):
            rr = []
            for j in range(out.res_off[i], out.res_off[i + 1]):
                r = out.res[j]
                rr.append(dict(reverse=int(r.reverse & 1), score=r.swatscor, q_start=r.q_start, q_end=r.q_end, s_start=r.s_start,
                               s_end=r.s_end, sidx=r.sidx, diffstr=bytes(out.diffstr[r.stroffs:r.stroffs + r.strlen])))
            res.append(rr)
            s = out.stat[i]
            stats.append(dict(swmax=s.swatscor_max, sw2nd=s.swatscor_2ndmax, nseg=s.n_ali_done, nseg_tot=s.n_ali_tot,
                              nhit=s.n_hits_used, nhit_tot=s.n_hits_tot, err=s.errcode, max1=s.max1scor, errsite=s.errsite))
        return res, stats

    def map_batch_device(self, d_bases: int, d_quals: int, d_off: int, nreads: int, total_bases: int, params: Params):
        _check(lib().smaltgpu_map_batch_device(self.h, d_bases, d_quals, d_off, nreads, total_bases, C.byref(params)))

    def synchronize(self):
        _check(lib().smaltgpu_synchronize(self.h))

    def fetch_results(self):
        out = BatchOut()
        _check(lib().smaltgpu_fetch_results(self.h, C.byref(out)))
        return out

    def fetch_begin(self):
        """Wait for the enqueued batch and start copying its results; the next map_batch_device may follow at once."""
        _check(lib().smaltgpu_fetch_begin(self.h))

    def fetch_end(self):
        out = BatchOut()
        _check(lib().smaltgpu_fetch_end(self.h, C.byref(out)))
        return out

    def fetch_end_rc(self):
        """fetch_end -> (return code, BatchOut) without raising: a read error (ECAP, EINTERNAL, ESCORE, ECPLX) comes with the batch
        filled and the code of every read in stat[].errcode; any other code with whatever the call left in the BatchOut"""
        out = BatchOut()
        return lib().smaltgpu_fetch_end(self.h, C.byref(out)), out

    def fetch_results_rc(self):
        """fetch_results -> (return code, BatchOut) without raising, as fetch_end_rc"""
        out = BatchOut()
        return lib().smaltgpu_fetch_results(self.h, C.byref(out)), out

    unpack = _unpack                        # (results, stats) of a BatchOut, as map_batch returns them

    def timers(self):
        ms = (C.c_double * 32)()
        wk = (C.c_uint64 * 32)()
        n = lib().smaltgpu_timers(self.h, ms, wk, 32)
        names = [lib().smaltgpu_timer_name(i).decode() for i in range(n)]
        return dict(zip(names, list(ms)[:n])), list(wk)

    def dump_read(self, i: int, name: str) -> str:
        n = lib().smaltgpu_dump_read(self.h, i, name.encode(), None, 0)
        if n < 0:
            _check(int(n))
        buf = C.create_string_buffer(n + 1)
        lib().smaltgpu_dump_read(self.h, i, name.encode(), buf, n + 1)
        return buf.value.decode()

    def sw_full_batch(self, queries: Sequence[bytes], windows: Sequence[bytes], params: Params, packed16: bool = False) -> List[int]:
        """Stand-alone K2a over explicit 3-bit code arrays (bytes of codes 0..7); packed16 selects the
        two-tasks-per-lane-group 16-bit kernel (-2 for queries with non-ACGT codes)."""
        n = len(queries)
        qo = (C.c_uint32 * (n + 1))()
        ro = (C.c_uint32 * (n + 1))()
        a = b = 0
        for i in range(n):
            qo[i], ro[i] = a, b
            a += len(queries[i])
            b += len(windows[i])
        qo[n], ro[n] = a, b
        sc = (C.c_int32 * n)()
        _check(lib().smaltgpu_sw_full_batch(self.h, b"".join(queries), qo, b"".join(windows), ro, n, C.byref(params), sc, int(packed16)))
        return list(sc)

    def sw_band_batch(self, queries: Sequence[bytes], windows: Sequence[bytes], params: Params, bands, form: int = 0):
        """Stand-alone K2b; bands: (band_l, band_r, qs, qe) per task; form 0: wave kernel, 1: one lane per task.
        Returns (scores, status) with status 1 where the band is refused."""
        n = len(queries)
        bd = (C.c_int32 * (4 * n + 4))(*[int(v) for b in bands for v in b])
        sc, st = (C.c_int32 * (n + 1))(), (C.c_int32 * (n + 1))()
        _check(lib().smaltgpu_sw_band_batch(self.h, b"".join(queries), _offsets(queries), b"".join(windows), _offsets(windows), n,
                                            C.byref(params), bd, form, sc, st))
        return list(sc)[:n], list(st)[:n]

    def band_align_nodes(self, queries: Sequence[bytes], windows: Sequence[bytes], params: Params, bands, ivs, minscore: int, form: int,
                         lds: bool = False, tw: bool = False):
        """Stand-alone K3 nodes in one form of the band pass; bands: (band_l, band_r, qs, qe), ivs: (s_left, s_right) per task.
        Returns per task a dict(status, score, max_i, max_j, qs, rs, diffstr)."""
        n = len(queries)
        bd = (C.c_int32 * (4 * n + 4))(*[int(v) for b in bands for v in b])
        iv = (C.c_int32 * (2 * n + 2))(*[int(v) for b in ivs for v in b])
        out = (BandNode * (n + 1))()
        ds = C.create_string_buffer(sum(len(q) + len(w) + 16 for q, w in zip(queries, windows)) + 16)
        _check(lib().smaltgpu_band_align_nodes(self.h, b"".join(queries), _offsets(queries), b"".join(windows), _offsets(windows), n,
                                               C.byref(params), bd, iv, minscore, form, int(lds), int(tw), out, ds))
        raw = ds.raw
        return [dict(status=o.status, score=o.score, max_i=o.max_i, max_j=o.max_j, qs=o.qs, rs=o.rs,
                     diffstr=raw[o.stroffs:o.stroffs + o.dlen]) for o in out[:n]]

    def seed_batch(self, reads: Sequence[bytes], quals: Optional[Sequence[bytes]], params: Params, seed_range=None, totals_only: bool = False,
                   scratch_home: int = 0, grid: int = 0, guard: int = 0xA5):
        """Stand-alone S1 + S2 (smaltgpu_seed_batch): k_encode and k_seed over the reads, nothing else.  seed_range: (first, last)
        per read.  scratch_home 1 forces the stage's scratch into HBM slots, grid is the number of workgroups (0: the launcher's
        choice).  -> dict of numpy arrays: codes, codes_rc [bases]; off [n + 1]; hi [2n + 1][8] (n_seeds, seed_rank, status, qlen,
        nhit_rank, nhit_tot, nhit_cut, unused), seeds [2n + 1][stride][3], qmask [2n + 1][stride] -- the last row is the guard row
        behind the batch, everything was filled with the byte `guard` before the launch --; lookups, in_lds, grid, stride, guard."""
        import numpy as np
        n = len(reads)
        bases, q, off = self._pack(reads, quals)
        stride = self.cands_geometry()["qmax"]
        rows, tot = 2 * n + 1, len(bases)
        codes, codes_rc = np.zeros(tot + 1, np.uint8), np.zeros(tot + 1, np.uint8)
        hi, seeds, qmask = np.zeros((rows, 8), np.uint32), np.zeros((rows, stride, 3), np.uint32), np.zeros((rows, stride), np.uint8)
        sr = None
        if seed_range is not None:
            sr = np.ascontiguousarray(np.asarray(seed_range, dtype=np.uint32).reshape(n, 2))
        out = SeedOut(codes.ctypes.data, codes_rc.ctypes.data, hi.ctypes.data, seeds.ctypes.data, qmask.ctypes.data)
        _check(lib().smaltgpu_seed_batch(self.h, bases, q, off, n, C.byref(params), None if sr is None else sr.ctypes.data, int(totals_only), scratch_home,
                                         grid, guard, C.byref(out)))
        assert out.nrows == rows and out.stride == stride
        return dict(codes=codes[:tot], codes_rc=codes_rc[:tot], off=np.array(list(off), dtype=np.int64), hi=hi, seeds=seeds, qmask=qmask,
                    lookups=int(out.lookups), in_lds=bool(out.in_lds), grid=int(out.grid), stride=stride, guard=guard)

    def gather_batch(self, batches, ids, guard: int = 0xA5, tail: int = 16):
        """Stand-alone k_gather_reads (smaltgpu_gather_batch).  batches: two (bases uint8 array, quals uint8 array or None, offsets
        uint64 array from 0); ids: read ids[i] >> 1 of batch ids[i] & 1.  -> (dst_bases, dst_quals, dst_off): the gathered bytes
        with `tail` bytes behind the last read, which were filled with the byte `guard` before the launch (dst_quals: all guard
        when the batches have no qualities)."""
        import numpy as np
        (b0, q0, o0), (b1, q1, o1) = batches
        o = [np.ascontiguousarray(o0, dtype=np.uint64), np.ascontiguousarray(o1, dtype=np.uint64)]
        b = [np.ascontiguousarray(np.concatenate([x, np.zeros(1, np.uint8)]), dtype=np.uint8) for x in (b0, b1)]
        qs = None if q0 is None else [np.ascontiguousarray(np.concatenate([x, np.zeros(1, np.uint8)]), dtype=np.uint8) for x in (q0, q1)]
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        lens = [int(o[i & 1][(i >> 1) + 1] - o[i & 1][i >> 1]) for i in ids.tolist()]
        tot = sum(lens)
        db, dq, do = np.zeros(tot + tail, np.uint8), np.zeros(tot + tail, np.uint8), np.zeros(len(ids) + 1, np.uint64)
        vp = lambda arrs: (C.c_void_p * 2)(*[a.ctypes.data for a in arrs])
        nr = (C.c_uint32 * 2)(len(o[0]) - 1, len(o[1]) - 1)
        idp = ids.ctypes.data if ids.size else np.zeros(1, np.uint32).ctypes.data
        _check(lib().smaltgpu_gather_batch(self.h, vp(b), None if qs is None else vp(qs), vp(o), nr, idp, len(ids), guard, tail,
                                           db.ctypes.data, dq.ctypes.data, do.ctypes.data))
        return db, dq, do

    def rank_sort_batch(self, arrays, nneed: int = -1, in_lds: bool = True, instance: int = 0):
        """Stand-alone candidate ranking sort: list of uint32 numpy arrays -> list of (keys, permutation).  instance 1: the sort
        as the seeding stage instantiates it (12 index bits, lists of 32 short ranges, in LDS; keys below 2^20, fewer than 4096)."""
        import numpy as np
        off = np.zeros(len(arrays) + 1, dtype=np.uint32)
        off[1:] = np.cumsum([len(a) for a in arrays])
        keys = np.ascontiguousarray(np.concatenate(arrays) if arrays else np.zeros(0), dtype=np.uint32)
        ok = np.zeros(max(1, keys.size), dtype=np.uint32)
        oi = np.zeros(max(1, keys.size), dtype=np.uint32)
        _check(lib().smaltgpu_rank_sort_batch(self.h, keys.ctypes.data, off.ctypes.data, len(arrays), nneed, int(in_lds), instance,
                                              ok.ctypes.data, oi.ctypes.data))
        return [(ok[off[t]:off[t + 1]], oi[off[t]:off[t + 1]]) for t in range(len(arrays))]

    def hits_batch(self, reads: Sequence[bytes], quals: Optional[Sequence[bytes]], params: Params, window: int = 0, pool_keys: int = 0):
        """Stand-alone S3 (smaltgpu_hits_batch): encode, seed and k_hits over the reads, nothing else.  -> dict of numpy copies,
        per strand rs = 2 * read + strand: n_seeds, seed_rank, status, seeds[rs] (posidx, nhits, qoffs), qmask[rs], run_off,
        run_n, run_mode; and hit_count, pool_cap, pool, window, tab."""
        import numpy as np
        bases, q, off = self._pack(reads, quals)
        out = HitsOut()
        _check(lib().smaltgpu_hits_batch(self.h, bases, q, off, len(reads), C.byref(params), window, pool_keys, C.byref(out)))
        ns, stride = out.nstrands, out.stride

        def arr(ptr, dtype, count):
            if not count:
                return np.zeros(0, dtype=dtype)
            nbytes = count * np.dtype(dtype).itemsize
            return np.frombuffer(C.string_at(ptr, nbytes), dtype=dtype).copy()
        seeds = arr(out.seeds, np.uint32, ns * stride * 3).reshape(ns, stride, 3)
        runs = arr(out.runs, np.dtype([("off", np.uint64), ("n", np.uint32), ("mode", np.uint32)]), ns)
        return dict(n_seeds=arr(C.cast(out.n_seeds, C.c_void_p), np.uint32, ns), seed_rank=arr(C.cast(out.seed_rank, C.c_void_p), np.uint32, ns),
                    status=arr(C.cast(out.status, C.c_void_p), np.uint32, ns), seeds=seeds, qmask=arr(out.qmask, np.uint8, ns * stride).reshape(ns, stride),
                    run_off=runs["off"].copy(), run_n=runs["n"].copy(), run_mode=runs["mode"].copy(), hit_count=int(out.hit_count),
                    pool_cap=int(out.pool_cap), pool=arr(out.pool, np.uint64, min(int(out.hit_count), int(out.pool_cap))),
                    window=int(out.window), tab=int(out.tab), stride=int(stride))

    def hits_windows(self, nstrands: int):
        """How k_hits gathered the strands of the last call (smaltgpu_hits_windows) -> dict: windows[nstrands] (0: one gather or
        none), raised[nstrands] (those of them whose bound was raised above the safe one), and the totals strands (gathered in
        several windows), nwindows, keys (of those strands) and reserved (the pool cursor; 0 where the call ran no k_hits)."""
        import numpy as np
        win = np.zeros(max(1, nstrands), dtype=np.uint32)
        tot = (C.c_uint64 * 4)()
        _check(lib().smaltgpu_hits_windows(self.h, nstrands, win.ctypes.data_as(C.c_void_p), tot))
        win = win[:nstrands]
        return dict(windows=(win & 0xffff).astype(np.int64), raised=(win >> 16).astype(np.int64), strands=int(tot[0]), nwindows=int(tot[1]), keys=int(tot[2]),
                    reserved=int(tot[3]))

    @staticmethod
    def pack_cands(cands):
        """per-read lists of candidate dicts -> (offsets, smaltgpu_cand array) as align_cands_batch passes them on; a caller that
        repeats a large batch converts it once and hands the pair in"""
        n = len(cands)
        co = (C.c_uint64 * (n + 1))()
        flat = [c for lst in cands for c in lst]
        t = 0
        for i, lst in enumerate(cands):
            co[i] = t
            t += len(lst)
        co[n] = t
        arr = (Cand * max(1, len(flat)))()
        for a, c in zip(arr, flat):
            a.rs, a.re, a.qs, a.qe, a.band_l, a.band_r, a.sqidx = c["rs"], c["re"], c["qs"], c["qe"], c["band_l"], c["band_r"], c["sqidx"]
            a.flags = (CAND_REVERSE if c["reverse"] else 0) | (CAND_ERR if c.get("err") else 0)
            a.cover, a.swscor = c["cover"], c["swscor"]
        return co, arr

    def align_cands_batch(self, reads: Sequence[bytes], params: Params, cands, cover_deficit=None, prev_max=None, min_swatscor=None,
                          raw_alignments: bool = False, antidiag: bool = False, allow_read_errors: bool = False):
        """Stand-alone O1 + K3 driver (smaltgpu_align_cands_batch): k_replay and both passes of k_align over the caller's ranked
        candidates and first-pass scores.  cands: per read a list of dicts of rs, re, qs, qe, band_l, band_r, sqidx, reverse, cover,
        swscor and optionally err, or what pack_cands made of them; cover_deficit: per read (forward, reverse), default (0, 0).
        -> (results, stats, cand_first flags per result, ctl dicts per read, number of reads deferred to the second pass)"""
        bases, _, off = self._pack(reads, None)
        n = len(reads)
        co, arr = cands if isinstance(cands, tuple) else self.pack_cands(cands)
        cdf = (C.c_uint32 * max(1, 2 * n))(*([x for pr_ in cover_deficit for x in pr_] if cover_deficit is not None else [0] * (2 * n)))
        ctx = CallCtx()
        keep = []
        if prev_max is not None:
            pm = (C.c_int32 * max(1, 2 * n))(*[x for pr_ in prev_max for x in pr_])
            ctx.prev_max = pm
            keep.append(pm)
        if min_swatscor is not None:
            ms = (C.c_int32 * max(1, n))(*min_swatscor)
            ctx.min_swatscor = ms
            keep.append(ms)
        ctx.raw_alignments = 1 if raw_alignments else 0
        out = AlignCandsOut()
        rv = lib().smaltgpu_align_cands_batch(self.h, bases, None, off, n, C.byref(params), C.byref(ctx), co, arr, cdf,
                                              ALIGN_CANDS_ANTIDIAG if antidiag else 0, C.byref(out))
        if rv != 0 and not (allow_read_errors and rv in (ECAP, EINTERNAL, ESCORE) and out.batch.nreads == n):
            _check(rv)
        res, stats = self._unpack(out.batch)
        cf = [[bool(out.batch.res[j].reverse & 2) for j in range(out.batch.res_off[i], out.batch.res_off[i + 1])] for i in range(n)]
        ctl = [dict(max1=c.max1, max2=c.max2, n_scored=c.n_scored, bandwidth_min=c.bandwidth_min, min_swatscor=c.min_swatscor,
                    scorlen_min=c.scorlen_min, go=c.go) for c in out.ctl[:n]]
        return res, stats, cf, ctl, int(out.n_deferred)

    def fine_index_batch(self, intervals, grid: int = 0, guard: int = 0xA5C3E187):
        """Stand-alone k_fine_index (smaltgpu_fine_index_batch): intervals = per read a list of (sidx, lo, hi).  The position buffer
        and the index rows are filled with `guard` before the kernel runs on `grid` workgroups (0 = one per read).
        -> dict of numpy copies: fine_off [n + 1], idx [n][idx_stride], pos [fine_off[n] + 1] (one word behind the last slice),
        nkeys."""
        import numpy as np
        n = len(intervals)
        ivo = (C.c_uint64 * (n + 1))()
        flat = [iv for lst in intervals for iv in lst]
        t = 0
        for i, lst in enumerate(intervals):
            ivo[i] = t
            t += len(lst)
        ivo[n] = t
        arr = (Interval * max(1, len(flat)))(*[Interval(a, b, c) for a, b, c in flat])
        out = FineOut()
        _check(lib().smaltgpu_fine_index_batch(self.h, n, ivo, arr, grid, guard, C.byref(out)))

        def take(ptr, count):
            return np.frombuffer(C.string_at(ptr, count * 4), dtype=np.uint32).copy() if count else np.zeros(0, dtype=np.uint32)
        return dict(fine_off=take(out.fine_off, n + 1), idx=take(out.idx, n * out.idx_stride).reshape(n, out.idx_stride),
                    pos=take(out.pos, int(out.npos)), nkeys=int(out.nkeys), guard=guard)

    def cands_geometry(self):
        """Scratch geometry of the candidate stage (smaltgpu_cands_geometry) -> dict; the pass-2 entries are 0 for a mapper with one pass."""
        g = (C.c_uint32 * 8)()
        _check(lib().smaltgpu_cands_geometry(self.h, g))
        return dict(hcap_strand=g[0], candcap=g[1], lds_bytes=g[2], hcap_strand2=g[3], candcap2=g[4], lds_bytes2=g[5], qmax=g[6], iv_max=g[7])

    def score_pool(self):
        """The candidate pool as the first-pass score stage of the last mapping call left it (smaltgpu_score_pool) -> (records,
        geometry): a numpy structured array of the first min(rc_count, rccap) records in pool order (fields rs, re, qs, qe, band_l,
        band_r, sqidx, flags, cover, swscor, rid; flags are RCF_*) and a dict of rc_count, rccap, long_cap, strip_cap, tile_qmax,
        wincap, tile_g, tile_c, full_grid, strip_grid."""
        import numpy as np
        out = ScorePoolOut()
        _check(lib().smaltgpu_score_pool(self.h, C.byref(out)))
        dt = np.dtype([("rs", np.uint64), ("re", np.uint64), ("qs", np.uint32), ("qe", np.uint32), ("band_l", np.int32), ("band_r", np.int32),
                       ("sqidx", np.int32), ("flags", np.uint32), ("cover", np.uint32), ("swscor", np.int32), ("rid", np.uint32), ("pad", np.uint32)])
        assert dt.itemsize == C.sizeof(PoolRec)
        n = int(out.nrec)
        rec = np.frombuffer(C.string_at(out.rec, n * dt.itemsize), dtype=dt).copy() if n else np.zeros(0, dtype=dt)
        geo = {k: int(getattr(out, k)) for k in ("rc_count", "rccap", "long_cap", "strip_cap", "tile_qmax", "wincap", "tile_g", "tile_c",
                                                 "full_grid", "strip_grid")}
        return rec, geo

    def sort_u64_batch(self, arrays, form: int):
        """Stand-alone 64-bit key sorts (smaltgpu_sort_u64_batch): list of uint64 numpy arrays -> list of sorted arrays.
        form: SORT_REG4 / SORT_REG8 / SORT_REG16 (register network, at most 256 / 512 / 1024 keys), SORT_LDS (the network in
        LDS, at most 1024 keys), SORT_HBM / SORT_CHUNKED (the network over global memory / the sort in chunks of 1024 keys, in
        place on global memory, at most 65536 keys).  A guard array of equal keys goes in behind the last array (no sort moves
        equal keys) and must come back as it went in: a store past the end of an array shows there."""
        import numpy as np
        guard = np.full(64, 0xA5C3A5C3A5C3A5C3, dtype=np.uint64)
        arrays = [np.ascontiguousarray(a, dtype=np.uint64) for a in arrays]
        off = np.zeros(len(arrays) + 2, dtype=np.uint32)
        off[1:] = np.cumsum([len(a) for a in arrays] + [guard.size])
        keys = np.concatenate(arrays + [guard])
        out = np.zeros(keys.size, dtype=np.uint64)
        _check(lib().smaltgpu_sort_u64_batch(self.h, keys.ctypes.data, off.ctypes.data, len(arrays) + 1, form, out.ctypes.data))
        if not np.array_equal(out[off[-2]:], guard):
            raise SmaltGpuError(EINTERNAL, "smaltgpu_sort_u64_batch: the guard behind the last array was written")
        return [out[off[t]:off[t + 1]] for t in range(len(arrays))]

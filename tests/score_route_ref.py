"""The task routing of the first-pass score stage (launch_sw_full, launch_sw_strip, launch_sw_scalar in run_pipeline and the seven
kernels behind them, smalt_amd/csrc/smg_kernels.hip) in plain Python: for the ranked candidates of one batch, which kernel must score
each of them, the flags and the score the stage leaves in its pool record, and the five work counters the stage adds up.  The scores
come from the oracle library (or_sw_full, or_sw_band_fast) on the read strand's codes and the window cut from the oracle's own
reference (or_index_fetch).  Shares no code with the library; what it restates is cited by file and line.

A candidate is a dict of rid, reverse, qs, qe, rs, re, band_l, band_r, sqidx (and optionally err: S7 marked it as broken).  The
geometry is what smaltgpu_score_pool returns, or `geometry()` below where there is no mapper."""
import ctypes as C

import numpy as np

import oracle_lib as ol

REVERSE, SCORED, BANDED, ERR, QN, BSCORED = 1, 2, 4, 8, 16, 32          # RCF_* (smg_common.h:26-28)
MINLEN_QUERY_STRIPED, BWSCAL_QLEN = 32, 48                              # rmap.c:83-86
SW_FULL_WMAX, SW_SHORT_WMAX = 1016, 248                                 # smg_kernels.h:9-10
BAND_WAVE_QMIN = 255                                                    # S7: banded candidates of reads longer than this are listed
EXCEED = 65535                                                          # ERRCODE_SWATEXCEED (rmap.c:730)
MAXIMUM_DEPTH = 8000                                                    # segment.c:119-141
TILINGS = ((64, 4, 16), (104, 8, 13), (152, 8, 19), (160, 8, 20), (256, 16, 16), (512, 16, 32))   # sw_tilings (smg_kernels.hip)
KERNELS = ("full16_short", "full16_long", "full32_qn", "strip16", "strip32", "band_wave", "scalar_k2a", "scalar_band")
WAVE_K2A = ("full16_short", "full16_long", "full32_qn", "strip16", "strip32")

# sequence.c:287-322: A C G T-or-U in either case are 0..3, everything else is 5; the reverse complement keeps codes >= 4
_CODE = np.full(256, 5, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _CODE[_c | 0x20] = _i
_CODE[ord("U")] = _CODE[ord("u")] = 3


def strand_codes(read: bytes):
    f = _CODE[np.frombuffer(read, dtype=np.uint8)]
    r = f[::-1]
    return f.tobytes(), np.where(r >= 4, r, 3 - r).astype(np.uint8).tobytes()


def geometry(max_batch_reads, max_read_len, cands_per_read=0):
    """smaltgpu_mapper_create_ex (smaltgpu.cpp:370, 389-403, 545) without the environment's overrides"""
    per = min(max(cands_per_read or 640, 8), 2048)
    cap = max_batch_reads * per
    if max_batch_reads <= 4096 and not cands_per_read:
        cap = max_batch_reads * 2048
    cap = min(max(cap, MAXIMUM_DEPTH), 0xFFFFFFF0)
    g = c = 0
    for qm, tg, tc in TILINGS:
        if max_read_len <= qm:
            g, c = tg, tc
            break
    qmax = (max_read_len + 8 + 7) & ~7
    return dict(rccap=cap, long_cap=cap // 8 + 1024, strip_cap=cap // 8 + 1024, tile_qmax=g * c, wincap=4 * qmax + 1024, tile_g=g, tile_c=c)


def is_banded(c, qlen):
    """S7 leaves the candidate to K2b: the `simd` rule of cand_offsets (smg_logic.hpp:553, rmap.c:715-718) fails"""
    bw = (c["band_r"] - c["band_l"]) & 0xFFFFFFFF
    simd = qlen >= MINLEN_QUERY_STRIPED and ((bw * BWSCAL_QLEN) & 0xFFFFFFFF) > qlen and c["qs"] == 0 and c["qe"] >= qlen - 1
    return not simd


def sw16_ok(par):
    """the packed kernels' 16-bit lanes hold the penalties (sw16_ok, smg_kernels.hip)"""
    bias = -par.mismatch if par.mismatch < par.mismatch - par.match else -(par.mismatch - par.match)
    return (par.match > 0 and par.match * 512 + bias + 256 < 0x7C00 and bias >= 0 and par.match + bias < 256 and par.mismatch + bias >= 0 and
            0 <= -par.gap_init < 30000 and 0 <= -par.gap_ext < 30000)


class Scorer:
    """or_sw_full / or_sw_band_fast over the oracle's index for the reads of one batch"""

    def __init__(self, oix, reads, par):
        L = ol.lib()
        L.or_index_fetch.restype = None
        L.or_index_fetch.argtypes = [C.POINTER(ol.OrIndex), C.c_uint64, C.c_uint32, C.c_char_p]
        self.oix, self.par = oix, par
        self.codes = [strand_codes(r) for r in reads]
        self.M = (C.c_int8 * 64)()
        L.or_score_matrix(self.M, par.match, par.mismatch)

    def window(self, c):
        o = self.oix.contents
        base = 0 if c["sqidx"] < 0 else int(o.sop[c["sqidx"]])
        n = int(c["re"]) - int(c["rs"]) + 1
        buf = C.create_string_buffer(n + 1)
        ol.lib().or_index_fetch(self.oix, base + int(c["rs"]), n, buf)
        return buf.raw[:n]

    def full(self, c):
        q = self.codes[c["rid"]][1 if c["reverse"] else 0]
        w = self.window(c)
        return int(ol.lib().or_sw_full(q, len(q), w, len(w), self.M, self.par.gap_init, self.par.gap_ext))

    def band(self, c):
        """-> score, or None where the band is refused (OR_ERR_BAND: band_init)"""
        q = self.codes[c["rid"]][1 if c["reverse"] else 0]
        w = self.window(c)
        sc = C.c_int(0)
        rv = ol.lib().or_sw_band_fast(C.byref(sc), q, len(q), w, len(w), self.M, self.par.gap_init, self.par.gap_ext, int(c["band_l"]), int(c["band_r"]),
                                      int(c["qs"]), int(c["qe"]), 0, len(w) - 1)
        assert rv in (0, 3), rv
        return None if rv else int(sc.value)


def plan(cands, qlens, has_n, geo, par, scorer=None):
    """cands: the ranked candidates of ALL reads of the batch (any order); qlens, has_n: per read.  -> dict: per candidate
    banded (S7's verdict), kernel (None: nobody scores an ERR candidate), flags and score (None without a scorer) as the stage
    leaves them; work: {2, 3, 7, 17, 18}; long_overflow, strip_overflow."""
    tile_qmax, wincap = geo["tile_qmax"], geo["wincap"]
    qmax = (wincap - 1024) // 4
    use16 = sw16_ok(par)
    strip16_on = use16 and qmax * par.match < 60000                     # launch_sw_strip
    n = len(cands)
    q = [qlens[c["rid"]] for c in cands]
    w = [int(c["re"]) - int(c["rs"]) + 1 for c in cands]
    err0 = [bool(c.get("err")) for c in cands]
    banded = [(not err0[i]) and is_banded(cands[i], q[i]) for i in range(n)]
    in_tile = [q[i] <= tile_qmax and w[i] <= SW_FULL_WMAX for i in range(n)]
    # S7's lists (the tails of stage_cands_v2 in smg_cands.hpp and of stage_cands in smg_stages.hpp)
    strip_listed = [(not err0[i]) and ((not banded[i] and not in_tile[i]) or (banded[i] and q[i] > BAND_WAVE_QMIN)) for i in range(n)]
    long_listed = [(not err0[i]) and not banded[i] and in_tile[i] and w[i] > SW_SHORT_WMAX for i in range(n)]
    work = {2: 0, 3: 0, 7: sum(1 for c in cands if has_n[c["rid"]]), 17: sum(long_listed), 18: sum(strip_listed)}
    over_long, over_strip = work[17] > geo["long_cap"], work[18] > geo["strip_cap"]
    kernel, flags, score = [None] * n, [0] * n, [None] * n
    for i, c in enumerate(cands):
        qn = bool(has_n[c["rid"]])
        f = (REVERSE if c["reverse"] else 0) | (QN if qn else 0)
        if err0[i]:
            flags[i] = f | ERR
            continue
        by_band_wave = strip_listed[i] and not over_strip and w[i] <= wincap      # k_sw_band reads the list, and only a list that was filled
        if not banded[i]:
            if in_tile[i]:
                # the scan of the large instance after an overflow of its list takes the same tasks as the list
                kernel[i] = "full32_qn" if (qn or not use16) else ("full16_short" if w[i] <= SW_SHORT_WMAX else "full16_long")
            elif w[i] > wincap:
                kernel[i] = "scalar_k2a"
            elif over_strip:
                kernel[i] = "strip32"                                              # k_sw_strip scans the pool, k_sw_strip16 returns
            else:
                kernel[i] = "strip16" if (strip16_on and not qn) else "strip32"
            f |= SCORED
            sc = scorer.full(c) if scorer else None
            if kernel[i] in WAVE_K2A:
                work[2] += q[i] * w[i]
                if sc is not None and sc < EXCEED:
                    work[3] += 1
            if sc is not None and sc >= EXCEED:                                    # the banded pass scores it again
                f |= BANDED
                bsc = scorer.band(c)
                if bsc is None:
                    f |= ERR                                                       # band refused: the K2a score stays in the record
                else:
                    sc = bsc
                    if by_band_wave and kernel[i] != "scalar_k2a":
                        f |= BSCORED
                        work[3] += 1
            flags[i], score[i] = f, sc
        else:
            kernel[i] = "band_wave" if by_band_wave else "scalar_band"
            sc = scorer.band(c) if scorer else 0
            if sc is None:
                flags[i] = f | BANDED | ERR
                score[i] = 0
                continue
            f |= BANDED | SCORED
            if kernel[i] == "band_wave":
                f |= BSCORED
                work[3] += 1
            flags[i], score[i] = f, (sc if scorer else None)
    return dict(banded=banded, kernel=kernel, flags=flags, score=score, work=work, q=q, w=w, long_overflow=over_long, strip_overflow=over_strip)

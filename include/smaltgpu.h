/* include/smaltgpu.h -- C ABI of libsmaltgpu.so: SMALT's seed-and-extend hot path on MI355X.
 *
 * Every entry point below is what the reference's per-read mapping API would bind for this
 * path (plain pointers and sizes only; no torch / HIP types).  `file:line` citations refer to
 * the reference tree (SMALT 0.7.6, src/).  INTEGRATION.md shows the rmap.c-side shim.
 *
 * All functions return 0 on success or a negative SMALTGPU_E* code; smaltgpu_last_error()
 * gives a message.  There is NO CPU fallback: without a HIP device every call fails.
 */
#ifndef SMALTGPU_H
#define SMALTGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  SMALTGPU_OK = 0,
  SMALTGPU_ENODEV = -1,     /* no HIP device / HIP runtime error */
  SMALTGPU_EFILE = -2,      /* cannot read .smi/.sma (ERRCODE_NOFILE / FILEFORM analogue) */
  SMALTGPU_EARG = -3,       /* bad argument (ERRCODE_ARGRANGE analogue) */
  SMALTGPU_ENOMEM = -4,     /* host or device allocation failed (ERRCODE_NOMEM) */
  SMALTGPU_ECAP = -5,       /* a work pool overflowed: smaltgpu_map_batch recovers by itself (reads re-mapped in smaller batches);
                             * from smaltgpu_fetch_* / in stat[].errcode it marks the reads to map again */
  SMALTGPU_EINTERNAL = -6,  /* device-side assertion (ERRCODE_ASSERT analogue) */
  SMALTGPU_ESCORE = -8,     /* in stat[].errcode: the traceback of one of the read's alignments does not add up to the score of its pass.
                             * The reference stops at such a read with ERRCODE_SWATSCOR (alignment.c:767, "Inconsistency when calculating
                             * Smith-Waterman scores"): it happens with alignment scores (-S) whose gap extension is much cheaper than
                             * the opening, because the banded passes do not re-open a gap from a gap cell (alignment.c:1126-1193) */
  SMALTGPU_ECPLX = -9       /* in stat[].errcode, with SMALTGPU_FLG_CMPLXW only: the complexity-weighted score of one of the read's alignments
                             * came out above the unweighted one.  The reference stops at such a read with ERRCODE_CPLXSCOR (alignment.c:290-299,
                             * "complexity weighted score exceeds unweighted score"): its constant for ln(1/4) is cut off at six digits, so an
                             * alignment over an exactly balanced composition (say 1000 each of A, C, G, T) gains a fraction of a point.
                             * A per-read code: every other read of the batch is complete */
};
/* return values of the mapping calls that mean "the batch is complete, some reads carry a code of their own in stat[].errcode" */
#define SMALTGPU_IS_READ_ERROR(rv) ((rv) == SMALTGPU_ECAP || (rv) == SMALTGPU_EINTERNAL || (rv) == SMALTGPU_ESCORE || (rv) == SMALTGPU_ECPLX)

/* RMAP_FLAGS subset honoured on this path (same values as rmap.h:53-65). */
enum {
  SMALTGPU_FLG_CMPLXW = 0x01,    /* complexity-weighted alignment scores (smalt map -w, RMAPFLG_CMPLXW): honoured by every mapping call, the rounds of
                                  * smaltgpu_map_pairs and both calls of smaltgpu_map_split included.  The score of every alignment of the traceback
                                  * pass is scaled by the composition of the reference letters it pairs (scaleALICPLX, alignment.c:268-305) before it
                                  * is compared with the threshold; swatscor, the score maxima and everything behind them see the weighted score.
                                  * The first-pass scores (max1scor) stay unweighted, as in the reference.  Bit-identical to the reference:
                                  * logarithms from a host-made table, lambda from the host, no fused multiply-adds */
  SMALTGPU_FLG_BEST = 0x02,
  SMALTGPU_FLG_SPLIT = 0x08,     /* split reads: honoured by smaltgpu_map_pairs (second calls of both mates ahead of the pairing, rmap.c:2073-2097);
                                  * the mapping calls themselves ignore it -- for single reads the two calls are smaltgpu_map_split */
  SMALTGPU_FLG_SEQBYSEQ = 0x10,
  SMALTGPU_FLG_NOSHRTINFO = 0x20,
  SMALTGPU_FLG_SENSITIVE = 0x80
};

typedef struct smaltgpu_index smaltgpu_index;    /* immutable index image resident in HBM */
typedef struct smaltgpu_mapper smaltgpu_mapper;  /* work buffers + stream; one per host thread */

/* Host-side description of an index: replaces struct _HashTable (hashidx.c:105-146) and the
 * SeqSet fields the path reads (sequence.c:148-171).  Pointers may be host or device memory
 * (see `on_device`). */
typedef struct smaltgpu_index_desc {
  int32_t k, s;              /* word length, sampling stride (hashidx.c:108-109) */
  int32_t typ;               /* 0 perfect, 1 hash32mix (hashidx.h:47-50) */
  int32_t nbits_key, nbits_lo;
  uint32_t npos, nwords;
  const uint32_t *idx;       /* 2^nbits_key + 1 */
  const uint32_t *pos;       /* npos */
  const uint32_t *wordidx;   /* nwords + 1 (hash32mix only) */
  const uint32_t *posidx;    /* nwords + 1 (hash32mix only) */
  int64_t nseq;
  const uint64_t *sop;       /* nseq + 1 cumulative base offsets; ALWAYS host memory */
  const uint32_t *packed;    /* totlen/10 + 1 words, 3 bits/base (sequence.c:1360) */
  int32_t on_device;         /* non-zero: idx/pos/wordidx/posidx/packed are device pointers (adopted, not copied) */
} smaltgpu_index_desc;

/* Scalar arguments of rmapSingle (rmap.h:127-145) + the score penalties (score.c:41-47). */
typedef struct smaltgpu_params {
  int32_t ktuple_maxhit;             /* -H, default 10000 */
  uint32_t min_cover;                /* covermin_tuple (smalt.c:1113-1126) */
  int32_t min_swatscor;              /* -m, default k+s-1 (smalt.c:608-615) */
  int32_t min_swatscor_below_max;    /* -d, default 0 */
  int32_t min_basqval;               /* -q, default 0 */
  int32_t target_depth, max_depth;   /* 512, 2048 (smalt.c:60-61) */
  uint32_t rmapflg;                  /* SMALTGPU_FLG_* */
  int32_t match, mismatch, gap_init, gap_ext;  /* +1 -2 -4 -3 */
  double min_cover_frac;             /* -c below 1.01: > 0 overrides min_cover with (uint32_t)(frac * read length) per read (smalt.c:1113-1122) */
} smaltgpu_params;

/* One alignment as left by resultSetAddFromAli (results.c:1852) before sorting/MAPQ. */
typedef struct smaltgpu_result {
  int32_t swatscor;
  uint32_t q_start, q_end;     /* 1-based, on the original read */
  uint64_t s_start, s_end;     /* 1-based, in sequence sidx (concatenated offset if sidx < 0) */
  int32_t sidx;
  uint32_t reverse;            /* bit 0: reverse-complement strand; bit 1 (SMALTGPU_RES_CANDFIRST): first alignment of its
                                * candidate, i.e. of one resultSetAddFromAli call (what a binding needs to append a call's
                                * alignments to a ResultSet that is not empty, results.c:1906-1935) */
  uint32_t stroffs, strlen;    /* DiffStr bytes in `diffstr`, strlen counts the terminating 0 */
} smaltgpu_result;
enum { SMALTGPU_RES_REVERSE = 1, SMALTGPU_RES_CANDFIRST = 2 };

/* Per-read scalars the host post-processing needs (resultSetAlignmentStats rmap.c:1338,
 * resultSetGetMaxSwat results.c:2163). */
typedef struct smaltgpu_readstat {
  int32_t swatscor_max, swatscor_2ndmax;
  int32_t n_ali_done, n_ali_tot;      /* nseg, nseg_tot */
  uint32_t n_hits_used, n_hits_tot;
  int32_t errcode;                    /* 0 or SMALTGPU_E* for this read */
  uint32_t nres;
  int32_t max1scor;                   /* best score of the score pass (rmap.c:1355); < 1: mapSingleRead returned before the
                                       * traceback pass and did NOT re-sort the ResultSet (rmap.c:1376) */
  int32_t errsite;                    /* diagnostic: source line (library build) of the device-side limit or assertion behind errcode; 0 if none */
} smaltgpu_readstat;

typedef struct smaltgpu_batch_out {
  uint32_t nreads;
  const uint64_t *res_off;            /* nreads + 1 offsets into `res` */
  const smaltgpu_result *res;
  const uint8_t *diffstr;
  const smaltgpu_readstat *stat;      /* nreads */
} smaltgpu_batch_out;

/* ---- index (replaces hashTableRead hashidx.c:1257 + seqSetReadBinFil sequence.c:2521) ---- */
int smaltgpu_index_load(smaltgpu_index **out, const char *prefix, int device);
int smaltgpu_index_create(smaltgpu_index **out, const smaltgpu_index_desc *desc, int device);
/* A copy of the image on another device of the node, device to device (hipMemcpyPeer: xGMI), instead of a second load from
 * disk: the reference's worker threads share one read-only HashTable/SeqSet (threads.c:793-985, rmap.h:83); with one image
 * per GPU the others are filled from the first.  (One process per GPU: broadcast the arrays of smaltgpu_index_info with
 * RCCL and adopt them with smaltgpu_index_create, as bench.py does.) */
int smaltgpu_index_clone(smaltgpu_index **out, const smaltgpu_index *src, int device);
void smaltgpu_index_free(smaltgpu_index *ix);
int smaltgpu_index_info(const smaltgpu_index *ix, smaltgpu_index_desc *desc_out); /* device pointers */
/* host copy of the packed reference (desc.packed), made on first request; for smaltgpu_postprocess.  NULL on failure */
const uint32_t *smaltgpu_index_packed_host(const smaltgpu_index *ix);
void smaltgpu_params_default(smaltgpu_params *p, const smaltgpu_index *ix);

/* ---- index construction (replaces `smalt index`: selectHashTyp smalt.c:268-332, hashTableSetUp
 * hashidx.c:829-998, seqSetCompress sequence.c:1360-1424, and the writers hashTableWrite hashidx.c:1214-1255 +
 * seqSetWriteBinFil sequence.c:2448-2519).  `bases`: the reference sequences concatenated, letters as in FASTA (anything
 * but ACGTU in either case counts as N); `seq_off`: nseq + 1 offsets into it (host memory); `names`: nseq strings.
 * _build takes host memory, _build_device bases already in HBM.  The image is built entirely on the device and is
 * ready for smaltgpu_mapper_create; smaltgpu_index_save writes <prefix>.sma / <prefix>.smi byte-compatible with the
 * reference's files.  build_ms (may be NULL) receives the device time of the construction.  SMALTGPU_EARG for what the
 * reference refuses: a sequence shorter than k, and with s > k a set of sequence lengths for which `smalt index` exits with
 * "arguments outside expected range" (hashidx.c:494; the message names the sequence). ---- */
int smaltgpu_index_build(smaltgpu_index **out, int device, const uint8_t *bases, const uint64_t *seq_off, const char *const *names,
                         int64_t nseq, int32_t k, int32_t s, float *build_ms);
int smaltgpu_index_build_device(smaltgpu_index **out, int device, const uint8_t *d_bases, const uint64_t *seq_off, const char *const *names,
                                int64_t nseq, int32_t k, int32_t s, float *build_ms);
int smaltgpu_index_save(const smaltgpu_index *ix, const char *prefix);

/* ---- index construction from the text of a FASTA file (`smalt index <prefix> <reference.fa>`: seqSetAddFromFastqFile
 * sequence.c:2391-2434 over seqFastqRead :1960-1990, readHeader :1056-1146 and readSeqFast :1229-1304, then buildHashIndex
 * smalt.c:338-412).  `text[0..text_len)`: the whole file in host memory (inflated if it was compressed).  The text is copied to
 * the device and parsed there (smg_fasta.hip); bases, offsets and names go to smaltgpu_index_build_device.  The rules are the
 * reference's: a prompt counts only as the first byte of a line and not on the line behind a header line, every other byte of the
 * sequence lines that is not white space is a base, the name of a sequence is its whole header line with each run of white space
 * cut down to its first character.  SMALTGPU_EARG with a message that names the cause: an empty text, a text that does not
 * begin with a prompt, a FASTQ-format reference ('@' or '+' prompts: taken by the _ex calls with SMALTGPU_TEXT_FASTQ, below), and
 * what smaltgpu_index_build_device refuses (a sequence shorter than the word length, ...).  parse_ms / build_ms (may be NULL):
 * device time of the parse and of the construction.  SMALTGPU_FASTA_BLOCK in the environment (read once per call; a test hook):
 * bytes of text per workgroup, at least 64 (default 256 KiB); small values are for small texts: the block size is doubled
 * until the text has at most 2^20 blocks. ---- */
int smaltgpu_index_build_text(smaltgpu_index **out, int device, const char *text, uint64_t text_len, int32_t k, int32_t s, float *parse_ms,
                              float *build_ms);
/* The same with flags.  0: the call above.  SMALTGPU_TEXT_FASTQ: a text with '@' or '+' prompts is read as the reference program
 * reads it (seqFastqRead sequence.c:1960-1990, readQual :1743-1772; the rules are stated in smg_fastq_ref.hpp): '@' opens a record
 * like '>'; a '+' prompt behind a sequence opens its quality section, which ends at the first prompt once it holds as many
 * characters as the sequence has bases -- lines that begin with '@', '+' or '>' before that are quality data; a segment behind
 * any other '+' prompt is dropped; a sequence that no '+' follows is a FASTA record, and a file may mix both kinds.  Qualities
 * are discarded.  A quality section of another length than its sequence is SMALTGPU_EARG "wrong FASTQ/FASTA format" with the
 * record's name, the number of its prompt in the text and its byte offset.  A text without such prompts takes the route and the
 * time of the call above.  A text whose first prompt is '@' or '+' is walked record by record on the device (smg_fastq_ref.hip);
 * one that begins with '>' and has such prompts further down is found out by the first route's output pass and walked then,
 * and parse_ms is the time of the walk's route alone.  SMALTGPU_FASTA_BLOCK holds for both routes. */
#define SMALTGPU_TEXT_FASTQ 1u
int smaltgpu_index_build_text_ex(smaltgpu_index **out, int device, const char *text, uint64_t text_len, int32_t k, int32_t s, float *parse_ms,
                                 float *build_ms, uint32_t flags);
/* The parse alone, back in host memory.  The view's arrays belong to `fa` and hold until smaltgpu_fasta_free. */
typedef struct smaltgpu_fasta smaltgpu_fasta;
typedef struct smaltgpu_fasta_view {
  int64_t nseq;
  const char *const *names;            /* nseq strings */
  const uint64_t *seq_off;             /* nseq + 1 offsets into bases */
  const uint8_t *bases;                /* the sequences concatenated, letters as in the file */
  float upload_ms;                     /* host time of the copy of the text to the device */
  float parse_ms;                      /* device time of the three steps together ... */
  float step_ms[3];                    /* ... and of each: block summaries, their composition, the output pass (a text with FASTQ
                                          records: candidates and prefix counts, the walk over the records, the output pass) */
} smaltgpu_fasta_view;
int smaltgpu_fasta_parse(smaltgpu_fasta **out, int device, const char *text, uint64_t text_len, smaltgpu_fasta_view *view);
int smaltgpu_fasta_parse_ex(smaltgpu_fasta **out, int device, const char *text, uint64_t text_len, smaltgpu_fasta_view *view, uint32_t flags);
void smaltgpu_fasta_free(smaltgpu_fasta *fa);

/* ---- mapper (replaces rmapCreate rmap.c:1511 / rmapDelete :1597) ---- */
int smaltgpu_mapper_create(smaltgpu_mapper **out, const smaltgpu_index *ix, uint32_t max_batch_reads,
                           uint32_t max_read_len);
/* Same with sizing options (0 = default): the RMap's buffers grow on demand (array.c), the mapper's pools are sized once.
 * cands_per_read: ranked candidates per read of the batch-wide pool (default 640 for large batches; the depth cut of
 * segment.c:1745-1775 leaves ~270 on a human-size reference, at most 2048).  slot_budget_gb: HBM for the scratch slots of
 * the persistent kernels (default 64) -- lower it when several mappers share a device.  A batch that overflows a pool is
 * not an error: smaltgpu_map_batch re-maps the reads that did not fit in smaller batches. */
typedef struct smaltgpu_mapper_opts {
  uint32_t cands_per_read;
  uint32_t slot_budget_gb;
} smaltgpu_mapper_opts;
int smaltgpu_mapper_create_ex(smaltgpu_mapper **out, const smaltgpu_index *ix, uint32_t max_batch_reads,
                              uint32_t max_read_len, const smaltgpu_mapper_opts *opts);
void smaltgpu_mapper_free(smaltgpu_mapper *m);
/* host threads a mapper may use for its own host work (the copy of a batch's results into read order in smaltgpu_fetch_end);
 * default 1 -- the reference's worker owns one thread (threads.c).  smaltgpu_map_pairs sets it from pair_opts.nthreads. */
int smaltgpu_mapper_set_host_threads(smaltgpu_mapper *m, int nthreads);
/* diagnostic, read only: device batches the mapper has run so far to map reads again that did not fit a work pool (the recovery of
 * smaltgpu_map_batch, smaltgpu_map_batch_ctx and smaltgpu_map_batch_ctx_resident from SMALTGPU_ECAP); 0 = no call ever overflowed */
int smaltgpu_mapper_remap_batches(const smaltgpu_mapper *m, uint64_t *nbatches);

/* Map a block of reads (the unit processArgBlock smalt.c:1221 hands to a worker).  `bases`:
 * concatenated ASCII reads, `quals`: concatenated phred+33 or NULL, `read_off`: nreads+1
 * offsets.  Replaces nreads calls of rmapSingle (rmap.c:1648) + rmapGetData (:1634).  The
 * returned arrays are owned by the mapper and valid until its next call. */
int smaltgpu_map_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals,
                       const uint64_t *read_off, uint32_t nreads, const smaltgpu_params *par,
                       smaltgpu_batch_out *out);

/* ---- paired reads: the mapSingleRead calls inside rmapPair (rmap.c:1744-2112) ----
 * rmapPair maps the mate with fewer k-mer hits first, then the other mate with its seeding restricted to the intervals the
 * first one implies (setupInterValFromResultSet rmap.c:354, collectHitsFromInterVal :438), and -- depending on the mapping
 * qualities and proper pairs found (results.c / resultpairs.c, host side) -- the second mate again without restriction and
 * the first mate again restricted, seeded against an on-the-fly k=5 s=1 index over the interval windows (setupFineHashTable
 * :495).  A binding runs a block of pairs through these rounds as batches: every round is one smaltgpu_map_batch_ctx call
 * over the reads that take part in it, with the per-read context of the round. */
typedef struct smaltgpu_interval { int32_t sidx; uint32_t lo, hi; } smaltgpu_interval;   /* interval.c:44-49: 0-based, inclusive, in sequence sidx */
typedef struct smaltgpu_callctx {
  const uint64_t *iv_off;        /* nreads + 1 offsets into iv, or NULL: no read is restricted.  An empty list is a valid
                                  * restriction (no seeds).  Intervals as interValPrune leaves them: sorted, disjoint */
  const smaltgpu_interval *iv;
  const int32_t *min_swatscor;   /* per read, overrides par->min_swatscor (rmap.c:2031), or NULL */
  const int32_t *prev_max;       /* per read (swatscor_max, swatscor_2ndmax) of the ResultSet the call appends to, or NULL (blank
                                  * sets): the traceback pass raises its threshold to the set's second-best score
                                  * (rmap.c:881-885); stat[].swatscor_max / _2ndmax return the pair after the call */
  int32_t fine_index;            /* != 0: seed against the on-the-fly index of each read's intervals (needs iv_off);
                                  * hit info is collected in the long form (initRMAPINFO, rmap.c:2024) */
  int32_t raw_alignments;        /* != 0: return every alignment of the call, candidate by candidate (SMALTGPU_RES_CANDFIRST marks the first
                                  * of each), without resultSetAddFromAli's duplicate handling (results.c:1906-1935: an alignment that
                                  * repeats the one before it is taken off again, and the alignment after it is lost).  For calls that
                                  * append to a non-empty ResultSet: the first comparison is with the set's last alignment, which only
                                  * the caller has (smgpost::Table::take_call; resultSetAppendRaw in integration/results_inject.c) */
  const uint32_t *hitlist_len;   /* per read, or NULL: length of the longest read that the reference's hit list has held up to and
                                  * including this call.  The list's capacity only grows (initHitList, hashhit.c:1280-1282) and decides
                                  * where the allocation-boundary protocol sets in (hashhit.c:1497), so a serial `smalt map` over reads
                                  * of different lengths depends on their order; NULL = every read as if it were the first
                                  * (smaltgpu_mapper_set_history keeps this array for the caller) */
  const uint32_t *seed_range;    /* per read (first, last) base, 0-based and inclusive, or NULL: k-mer words are taken from that stretch of
                                  * the read only -- the second call of a split read (mapSecondary, rmap.c:1435-1505 -> collectHitInfo with
                                  * a range, hashhit.c:536-551); a stretch shorter than a word means the whole read, as there.  The
                                  * alignment passes still see the whole read */
} smaltgpu_callctx;
int smaltgpu_map_batch_ctx(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                           const smaltgpu_params *par, const smaltgpu_callctx *ctx, smaltgpu_batch_out *out);
/* Serial-order mode of a mapper (off by default): smaltgpu_map_batch / smaltgpu_map_batch_ctx calls without ctx->hitlist_len take the
 * reads of consecutive calls as ONE serial run of `smalt map -n 0` -- the hit-list capacity of a read is that of the longest read
 * of length >= k seen so far, carried from call to call (rmap.c:1123 creates the list once per thread; reads shorter than k return
 * before they reach it, rmap.c:1274).  on = 0 switches the mode off, any call with on != 0 starts a new run. */
int smaltgpu_mapper_set_history(smaltgpu_mapper *m, int on);
/* calcTotalNumberOfHits (rmap.c:1076) of every read: k-mer hits over both strands counting only words with at most
 * par->ktuple_maxhit hits -- what rmapPair compares to decide which mate is mapped first (rmap.c:1866-1870). */
int smaltgpu_hit_totals(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                        const smaltgpu_params *par, uint32_t *nhits);

/* The same two calls for rounds whose reads come from two batches that are already resident in HBM (reads and mates of a block of
 * pairs): read i of the round is read ids[i] >> 1 of batch ids[i] & 1; the mapper gathers the round on the device.  Only the
 * offsets are needed on the host (read lengths). */
typedef struct smaltgpu_resident_reads {
  const uint8_t *d_bases[2], *d_quals[2];     /* device; d_quals: both or neither */
  const uint64_t *d_read_off[2];              /* device: nreads[w] + 1 offsets */
  const uint64_t *read_off[2];                /* the same offsets in host memory */
  uint32_t nreads[2];
} smaltgpu_resident_reads;
int smaltgpu_map_batch_ctx_resident(smaltgpu_mapper *m, const smaltgpu_resident_reads *src, const uint32_t *ids, uint32_t nreads,
                                    const smaltgpu_params *par, const smaltgpu_callctx *ctx, smaltgpu_batch_out *out);
int smaltgpu_hit_totals_resident(smaltgpu_mapper *m, const smaltgpu_resident_reads *src, const uint32_t *ids, uint32_t nreads,
                                 const smaltgpu_params *par, uint32_t *nhits);

/* ---- paired reads, whole: rmapPair (rmap.h:175-194, rmap.c:1744-2112) for a BLOCK of pairs -------------------
 * smaltgpu_map_pairs runs the block through the rounds above -- hit totals, first mate, second mate restricted, second mate
 * again, first mate again over the on-the-fly index; each round one batch of smaltgpu_map_batch_ctx -- and takes the decisions
 * between them itself: the post-call pass of every call (smaltgpu_postprocess's rules), the proper-pair probe
 * (resultSetFindProperPairs, resultpairs.c:1162), the search intervals (setupInterValFromResultSet, rmap.c:354).  What comes
 * back is a `smaltgpu_pairs`: per pair the two alignment sets as rmapPair leaves them in rmp->rsrp / rmp->rsmp and the pair
 * flags (*pairflgp).  smaltgpu_report_emit_pairs does the rest of the reference's flow for a pair: resultSetFindPairs
 * (resultpairs.c:1116), the output filters, resultSetAddPairToReport (:1222) and the CIGAR / SAM lines of both mates
 * (report.c:1758).  `par` as for single reads (rmapPair maps best-only: min_swatscor_below_max is taken as 0); reads and mates
 * in the batch layout of smaltgpu_map_batch, pair i = (read i of the first, read i of the second batch). */
enum { SMALTGPU_LIB_PE = 1, SMALTGPU_LIB_MP = 2, SMALTGPU_LIB_PP = 3, SMALTGPU_LIB_ANY = 4 };   /* -l pe | mp | pp (RSLTPAIRLIB_*, resultpairs.h:68-82) */
typedef struct smaltgpu_pair_opts {
  int32_t insert_min, insert_max;      /* -j, -i: d_min, d_max of rmapPair */
  int32_t library;                     /* SMALTGPU_LIB_* */
  int32_t every_pair;                  /* != 0: the unrestricted round for every pair (-x: RMAPFLG_ALLPAIR, smalt.c:533) */
  int32_t nthreads;                    /* host threads for the work between the rounds */
} smaltgpu_pair_opts;
typedef struct smaltgpu_pair_info {
  uint8_t pairflg;                     /* RSLTPAIRFLG_* (resultpairs.h:52-66): PAIRED 0x01, RAREMATE 0x02, RESTRICT_1st 0x04, RESTRICT_2nd 0x08 */
  uint8_t rounds;                      /* bit r: the pair took part in round r (0 first mate, 1 second mate restricted, 2 second mate again, 3 first mate again) */
  uint16_t nali[2];                    /* alignments that survived the post-call pass, read and mate */
} smaltgpu_pair_info;
typedef struct smaltgpu_pairs smaltgpu_pairs;
smaltgpu_pairs *smaltgpu_pairs_create(void);
void smaltgpu_pairs_free(smaltgpu_pairs *p);
int smaltgpu_map_pairs(smaltgpu_mapper *m, const uint8_t *bases1, const uint8_t *quals1, const uint64_t *read_off1, const uint8_t *bases2,
                       const uint8_t *quals2, const uint64_t *read_off2, uint32_t npairs, const smaltgpu_params *par, const smaltgpu_pair_opts *po,
                       smaltgpu_pairs *out);
/* Same with the reads and mates of the block resident in HBM (bench.py: the timed region starts with the inputs on the device).
 * `src` as above; host copies of the bases / qualities are optional: `bases1/2` are needed when alignments can cross reference
 * sequences (concatenated mode: the pieces are scored again on the host), `quals1/2` for the base-quality rule among equally
 * good alignments (results.c:1247-1285; without them reads count as FASTA input there). */
int smaltgpu_map_pairs_resident(smaltgpu_mapper *m, const smaltgpu_resident_reads *src, const uint8_t *bases1, const uint8_t *quals1, const uint8_t *bases2,
                                const uint8_t *quals2, uint32_t npairs, const smaltgpu_params *par, const smaltgpu_pair_opts *po, smaltgpu_pairs *out);
/* what a block looked like: per pair the flags and counts above; calls[4] (may be NULL) = mapping calls per round; round_ms[4]
 * (may be NULL) = host wall time of each round's batch incl. its copies */
int smaltgpu_pairs_info(const smaltgpu_pairs *p, uint32_t *npairs, const smaltgpu_pair_info **info, uint64_t *calls, double *round_ms);
/* device time per kernel (ms[5][16]: rounds 0-3 and the hit totals, kernels in the order of smaltgpu_timer_name) and the mapper's
 * work counters (work[5][32]) summed over the block's batches; either may be NULL.  For bench.py's roofline object. */
int smaltgpu_pairs_timers(const smaltgpu_pairs *p, double *kernel_ms, uint64_t *work);
/* host wall time [ms] of the work between the rounds of the block: passes behind round A (with the search intervals), behind B, the
 * proper-pair probe, behind C, the plan of round D, behind D, the hit-totals batches, and the whole call; returns the number of entries (8) */
int smaltgpu_pairs_host_times(const smaltgpu_pairs *p, double *ms, int n);
/* the index a mapper was created on, and the batch it was sized for (smaltgpu_map_pairs takes blocks of up to max_batch_reads pairs) */
const smaltgpu_index *smaltgpu_mapper_index(const smaltgpu_mapper *m);
int smaltgpu_mapper_capacity(const smaltgpu_mapper *m, uint32_t *max_batch_reads, uint32_t *max_read_len, uint64_t *max_bases);

/* Same with the inputs already resident in HBM (device pointers); results stay on the device
 * until smaltgpu_fetch_results().  Used by bench.py so that the timed region starts with the
 * reads in HBM.  The offsets live on the device, so the library cannot check them and the caller
 * guarantees what the kernels rely on: d_read_off[0] is 0 (d_bases / d_quals point at the first
 * read of the batch and may have any alignment), the offsets do not decrease, no read is longer
 * than the mapper's max_read_len, and total_bases equals d_read_off[nreads].  A batch that
 * overflows a work pool is NOT mapped again here: the reads that did not fit keep SMALTGPU_ECAP
 * in stat[].errcode, without results, and the fetch call returns that code with `out` filled. */
int smaltgpu_map_batch_device(smaltgpu_mapper *m, const uint8_t *d_bases, const uint8_t *d_quals,
                              const uint64_t *d_read_off, uint32_t nreads, uint64_t total_bases,
                              const smaltgpu_params *par);
int smaltgpu_fetch_results(smaltgpu_mapper *m, smaltgpu_batch_out *out);
/* The same in two steps, so that the device does not wait for the host between batches: _begin waits for the batch and
 * enqueues the copies of its results; the next smaltgpu_map_batch_device may follow at once; _end hands the results out
 * (valid until the next _begin on this mapper). */
int smaltgpu_fetch_begin(smaltgpu_mapper *m);
int smaltgpu_fetch_end(smaltgpu_mapper *m, smaltgpu_batch_out *out);
int smaltgpu_synchronize(smaltgpu_mapper *m);

/* ---- result post-processing: what resultSetSortAndAssignSequence (results.c:2022) does to the raw
 * alignments of every read of a batch -- assignSequenceIndex (:1695: concatenated mode, sequence and offsets),
 * sortAndPrune (:759: contained alignments out, output order, score ranks), labelComplementarySegments (:707) and
 * calcPhredScaledMappingQuality (:1143, with propagateMapQualAsProb :1343).  Host code on worker threads: the mapping
 * quality is double arithmetic through libm and the orders are libc qsort's on the reference's comparators, so
 * bit-identical results need the same libm / libc the reference runs on.  `raw` is a batch as smaltgpu_map_batch returns it
 * (alignments of ONE mapSingleRead call per read), `quals` / `read_off` the reads' phred+33 qualities (NULL: FASTA input),
 * `sop` the nseq + 1 cumulative sequence offsets (smaltgpu_index_info).  Concatenated mode: an alignment that spans several
 * reference sequences is cut at the junctions and its fragments re-scored (splitMultiSpan, results.c:1472: the fragments are
 * appended to the read's results, out->diffstr then holds their strings too) when `bases` (the reads, ASCII, by read_off),
 * `packed_host` (a host copy of the packed reference, sequence.c:1360) and `par` (penalties) are given; with any of them
 * NULL such a read is flagged needs_reference and left alone. ---- */
typedef struct smaltgpu_post_result {  /* struct _RESULT (results.c:121-160) after the post-processing */
  int32_t swatscor;
  uint32_t q_start, q_end;
  uint64_t s_start, s_end;             /* relative to sequence sidx once it is assigned */
  int32_t sidx;
  uint32_t status;                     /* RSLTFLAG_* (results.h:67-78): SELECT 0x01, REVERSE 0x04, NOSEQID 0x08, SINGLE 0x100 */
  int32_t mapscor;                     /* PHRED-scaled mapping quality */
  double prob;
  int16_t rsltx, qsegx, swrank, pad;
  uint32_t stroffs, strlen;
} smaltgpu_post_result;
typedef struct smaltgpu_post_out {
  uint32_t nreads;
  const uint64_t *res_off;             /* nreads + 1 offsets into res: the result array of read i in its original order */
  const smaltgpu_post_result *res;
  const uint8_t *diffstr;              /* raw->diffstr, or a copy of it with the strings of split fragments behind */
  const uint64_t *sort_off;            /* nreads + 1 offsets into sortr / segsrtr */
  const int32_t *sortr;                /* ResultSet.sortr: indices into the read's results, by decreasing score (results.c:478) */
  const int32_t *segsrtr;              /* ResultSet.segsrtr: by read segment, then score */
  const uint64_t *seg_off;             /* nreads + 1 offsets into segnor */
  const int32_t *segnor;               /* ResultSet.segnor: qsegno + 1 bounds of the segments in segsrtr */
  const int32_t *qsegno;               /* per read */
  const uint32_t *setstatus;           /* per read: RSLTSETFLG_* (results.c:93-100) */
  const int32_t *needs_reference;      /* per read: 1 = left to the caller (alignment across a sequence junction) */
} smaltgpu_post_out;
typedef struct smaltgpu_post smaltgpu_post;     /* owns the arrays of a smaltgpu_post_out */
smaltgpu_post *smaltgpu_post_create(void);
void smaltgpu_post_free(smaltgpu_post *p);
int smaltgpu_postprocess(smaltgpu_post *p, const uint64_t *sop, int64_t nseq, const smaltgpu_batch_out *raw, const uint8_t *bases,
                         const uint8_t *quals, const uint64_t *read_off, const uint32_t *packed_host, const smaltgpu_params *par, int nthreads,
                         smaltgpu_post_out *out);

/* ---- read ingest and report emit (host code, no device; smg_report.cpp) ------------------------------------
 * The reference reads FASTQ / FASTA through one reader thread (seqFastqRead, sequence.c:1960; readHeader :1056, readSeqFast
 * :1229) and prints through the main thread (reportWrite, report.c:1758).  Here a text buffer (a whole file or a chunk of it)
 * becomes the batch layout of smaltgpu_map_batch in one call, and the post-processed results of a batch become the text
 * `smalt map` prints for these reads (single reads; CIGAR and SAM formats), both with worker threads.
 *
 * smaltgpu_reads_parse: `text[0..len)`; is_last = 0: a record that may continue behind the buffer is left (view->consumed
 * says how far the text was used: call again from there with more text); max_reads = 0: no limit.  Plain four-line FASTQ is
 * split over `nthreads`; anything else (FASTA, wrapped lines, blank lines) takes the reference's rules on one thread.
 * The view's arrays belong to `rs` and hold until the next call: bases as the reference's codec prints them (upper case,
 * U -> T, non-letters N; smaltgpu_map_batch takes them as they are), quality characters as in the file (NULL without any:
 * a block with a FASTA record has none), names = the first word of each header, NUL-terminated, by name_off. */
typedef struct smaltgpu_reads smaltgpu_reads;
typedef struct smaltgpu_reads_view {
  uint32_t nreads, has_qual;
  const uint8_t *bases, *quals;
  const uint64_t *read_off;            /* nreads + 1 */
  const char *names;
  const uint64_t *name_off;            /* nreads + 1 */
  uint64_t consumed;                   /* bytes of text the reads came from */
} smaltgpu_reads_view;
smaltgpu_reads *smaltgpu_reads_create(void);
void smaltgpu_reads_free(smaltgpu_reads *rs);
int smaltgpu_reads_parse(smaltgpu_reads *rs, const char *text, uint64_t len, int is_last, uint32_t max_reads, int nthreads,
                         smaltgpu_reads_view *view);

/* ---- the same parse on the device (smg_reads_dev.hpp / smg_reads_dev.hip) -------------------------------------------------------
 * smaltgpu_reads_parse_device copies `text[0..len)` to the device, finds the records of ALL candidate prompts at once (one
 * speculative step of the reference's reader per prompt, the chain of records by pointer doubling, prefix sums, one output pass)
 * and leaves the batch in HBM in the layout smaltgpu_map_batch_device and one side of smaltgpu_resident_reads take: d_read_off[0]
 * is 0, d_quals is NULL without qualities.  Every rule is the one of smaltgpu_reads_parse for any shape of text (FASTA, wrapped
 * lines, blank lines, stray '+' segments): the same reads, names, has_qual and consumed for the same is_last / max_reads, the same
 * SMALTGPU_EFILE messages.  host_view (may be NULL: a caller who only maps and counts needs no host copy) is filled as
 * smaltgpu_reads_parse fills it, by one copy of the compacted arrays and the names cut on the host; dev_view may be NULL too, not
 * both.  The arrays of both views belong to the handle and hold until the next parse on it.  A handle serves one thread at a
 * time; its work runs on a stream of its own and is complete when the call returns. */
typedef struct smaltgpu_reads_dev smaltgpu_reads_dev;
typedef struct smaltgpu_reads_device_view {
  const uint8_t *d_bases, *d_quals;    /* device: total_bases bytes each; d_quals NULL without qualities */
  const uint64_t *d_read_off;          /* device: nreads + 1 */
  uint32_t nreads, has_qual;
  uint64_t total_bases;
  uint64_t consumed;                   /* as smaltgpu_reads_view.consumed */
} smaltgpu_reads_device_view;
smaltgpu_reads_dev *smaltgpu_reads_dev_create(int device);       /* NULL: no such device (smaltgpu_last_error) */
void smaltgpu_reads_dev_free(smaltgpu_reads_dev *rd);
int smaltgpu_reads_parse_device(smaltgpu_reads_dev *rd, const char *text, uint64_t len, int is_last, uint32_t max_reads,
                                smaltgpu_reads_view *host_view, smaltgpu_reads_device_view *dev_view);
/* For tests and measurements.  _configure: bytes of text per workgroup of the passes over the text (0: the default; a multiple of
 * 64), a cap on the workgroups of the passes over the prompts (0: the default), and a number of bytes behind each array of the
 * device view that the next parses fill with 0xA5 before they write.  _readback: array `which` (0 bases, 1 qualities, 2 offsets)
 * of the last parse with the bytes behind it copied to dst (room for cap bytes); *nbytes: the array's own size; *launches (may be
 * NULL): the kernel launches of the last parse. */
int smaltgpu_reads_dev_configure(smaltgpu_reads_dev *rd, uint32_t block_bytes, uint32_t max_groups, uint32_t guard_bytes);
int smaltgpu_reads_dev_readback(smaltgpu_reads_dev *rd, int which, void *dst, uint64_t cap, uint64_t *nbytes, uint32_t *launches);

/* ---- reads from SAM and BAM files (smalt map -F sam|bam; host code, smg_alnin.hpp / smg_alnin.cpp) ------------------------------
 * The reference reads such files through the bambamc library when it is linked with it (infmt.c; smalt.c:584 opens the file,
 * :804-826 loads reads and mates of a template into the buffers, :1129-1184 sends a pair to rmapPair and anything else to
 * rmapSingle, template by template); its build here lacks the library, and so does this one: the records and their BGZF blocks are
 * read here, over zlib.  Single reads and pairs may be mixed in one file.  The rules are this project's (the order of bambamc's
 * collator is not in the reference tree); smg_alnin.hpp states them in full:
 *   - only QNAME, FLAG, SEQ and QUAL are used; records with flag 0x100 or 0x800 are dropped, every other record is one read;
 *   - flag 0x10: the read is turned back into the strand it was sequenced in (IUPAC-aware complement, qualities reversed); letters
 *     then as smaltgpu_reads_parse stores them; BAM qualities of 0xFF / SAM '*': the read has none, and BOTH views of a run that
 *     holds such a read have has_qual = 0; a record without sequence is a read of no bases;
 *   - flag 0x1 with exactly one of 0x40 / 0x80: a mate, named QNAME/1 or QNAME/2; it waits in a table (in memory) keyed by QNAME
 *     until the other mate arrives from anywhere in the input; the pair takes the place of its later record, mate 1 is the read
 *     and mate 2 the mate.  A record whose name and mate number already wait releases the waiting one as a single read at that
 *     point.  What waits at the end follows as single reads in input order.  Everything else is a single read named QNAME.
 * smaltgpu_alnreads_feed: `bytes[0..len)` are the next bytes of the file from where the last call stopped; *consumed says how far
 * they were used (whole SAM lines, whole BGZF blocks): call again from there, with more bytes when nothing was consumed;
 * is_last != 0: nothing follows `bytes` (a last line without newline is taken, a truncated block or record is an error, waiting
 * mates are released).  BGZF blocks are inflated on `nthreads` threads.
 * smaltgpu_alnreads_take: the next run of templates of ONE kind, at most max_templates (0: no limit): *kind 0 = none ready (feed
 * more, or the end), 1 = single reads (`reads` only), 2 = pairs (read i of `reads` with read i of `mates`).  Runs are maximal
 * stretches of consecutive templates of one kind and come in template order.  The views are filled as smaltgpu_reads_parse
 * fills them (consumed = 0) and hold until the next take on this reader.
 * Errors: SMALTGPU_EARG (null pointers, an unknown format, bytes behind is_last) or SMALTGPU_EFILE with a message that names the
 * byte offset of the BGZF block in the file or the number of the record (from 1): a bad BGZF header, a wrong BSIZE, CRC or ISIZE
 * mismatch, a block_size that runs past the data, l_read_name 0, a name without its NUL, a truncated last record, a SAM line of
 * fewer than 11 fields, a SAM FLAG that is not a number, SEQ and QUAL of different lengths.  A reader that has failed repeats its
 * error; it can be freed. */
enum { SMALTGPU_IN_SAM = 1, SMALTGPU_IN_BAM = 2 };
typedef struct smaltgpu_alnreads smaltgpu_alnreads;
smaltgpu_alnreads *smaltgpu_alnreads_create(int format);     /* NULL: unknown format, or no memory */
void smaltgpu_alnreads_free(smaltgpu_alnreads *r);
int smaltgpu_alnreads_feed(smaltgpu_alnreads *r, const char *bytes, uint64_t len, int is_last, int nthreads, uint64_t *consumed);
int smaltgpu_alnreads_take(smaltgpu_alnreads *r, uint32_t max_templates, int *kind, smaltgpu_reads_view *reads, smaltgpu_reads_view *mates);
/* wall time [s] the reader has spent so far: BGZF blocks walked and inflated (the threaded part) | records decoded and collated
 * (one thread; SAM: all of feed) | runs copied into the views; any pointer may be NULL */
int smaltgpu_alnreads_times(const smaltgpu_alnreads *r, double *inflate_s, double *decode_s, double *take_s);

/* ---- split reads (smalt map -p): rmapSingle with RMAPFLG_SPLIT (rmap.c:1716-1728 -> mapSecondary, rmap.c:1435-1505) for a batch ----
 * Every read is mapped; where the best alignment of the read's first segment leaves a stretch of at least a word and a step
 * uncovered, the read is mapped once more with k-mer words from that stretch only (smaltgpu_callctx.seed_range), into the same
 * alignment set, and the set is put in order again.  The result has the layout of smaltgpu_postprocess (which this call replaces
 * for split reads) and goes to smaltgpu_report_emit with SMALTGPU_OUT_SPLIT.  par->rmapflg as smalt.c:508 sets it for -p:
 * NOSHRTINFO | SENSITIVE on top of the usual flags.  n_second_calls (may be NULL): how many reads got the second call. */
int smaltgpu_map_split(smaltgpu_mapper *m, smaltgpu_post *post, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                       const smaltgpu_params *par, const smaltgpu_index *ix, int nthreads, smaltgpu_post_out *out, uint32_t *n_second_calls);

/* Report: which alignments of a read are printed (resultSetFilterResults, results.c:2592; resultSetAddToReport, results.c:2282;
 * reportAddMap's duplicate test, report.c:545) and the lines themselves (fprintREPALIcigar report.c:711, fprintREPALIsam
 * report.c:762, writeDiffStrCIGAR diffstr.c:298, SAM header report.c:1266). */
enum { SMALTGPU_FMT_CIGAR = 0, SMALTGPU_FMT_SAM = 1, SMALTGPU_FMT_SSAHA = 2, SMALTGPU_FMT_BAM = 3 };   /* -f cigar | sam | ssaha | bam (REPORTFMT_*, report.h:46-52;
                                                                                          * fprintREPALIssaha report.c:579).  -f gff ends the reference program
                                                                                          * with a memory fault on its first read (report.c:1389-1401 drops the
                                                                                          * block list it has just made).  -f bam: the reference writes it through
                                                                                          * the bambamc library (report.c:916-1081), which its build here lacks;
                                                                                          * this library writes the records and their BGZF blocks itself, over
                                                                                          * zlib (smg_bam.hpp).  BAM takes the modflags of SAM except ALIOUT */
enum { SMALTGPU_REP_ALIOUT = 0x01, SMALTGPU_REP_SOFTCLIP = 0x02, SMALTGPU_REP_HEADER = 0x04, SMALTGPU_REP_XMISMATCH = 0x08 };   /* REPORTMODIF_* (report.h:54-59);
                                                                                          * ALIOUT (smalt map -a): the line of every mapped alignment, of any
                                                                                          * format, is followed by the alignment itself in blocks of three rows
                                                                                          * -- read, markers, reference -- 60 columns wide; needs
                                                                                          * smaltgpu_report_set_reference */
enum { SMALTGPU_OUT_BEST = 0x01, SMALTGPU_OUT_SINGLE = 0x02, SMALTGPU_OUT_SPLIT = 0x04, SMALTGPU_OUT_RANDSEL = 0x08 };   /* RESULTFLG_* (results.h:55-63); SPLIT: the best
                                                                                          * alignments of the other read segments follow as partial ones (results.c:2250-2278, :2337) */
typedef struct smaltgpu_report_opts {
  int32_t format;
  uint32_t modflags, outflags;
  int32_t min_swscor;                  /* resultSetFilterData (smalt.c:490): the -m value, 18 without one -- NOT the mapping threshold k+s-1 */
  int32_t min_swscor_below_max;        /* -d */
  double min_identity;                 /* -y: fraction of the read length if <= 1, else bases */
} smaltgpu_report_opts;
typedef struct smaltgpu_report smaltgpu_report;      /* owns the text it hands out */
smaltgpu_report *smaltgpu_report_create(void);
void smaltgpu_report_free(smaltgpu_report *rp);
/* text in front of the first read (the SAM header; empty for the other formats); the report keeps the sequence lengths, which
 * SSAHA lines print: call it once before the emit functions.  seqnames / sop / nseq: smaltgpu_index_seqnames */
int smaltgpu_report_header(smaltgpu_report *rp, const char *const *seqnames, const uint64_t *sop, int64_t nseq, const smaltgpu_report_opts *op,
                           const char *prognam, const char *version, int argc, const char *const *argv, const char **text, uint64_t *len);
/* the lines of a batch: post = smaltgpu_postprocess of `raw` (raw may be NULL: it only supplies the per-read error codes),
 * reads = the parsed block the batch was mapped from.  A random choice among equal best alignments (SMALTGPU_OUT_RANDSEL,
 * -r <seed>) draws from drand48() in read order: seed it with srand48 as RANSEED does (randef.h:19). */
int smaltgpu_report_emit(smaltgpu_report *rp, const smaltgpu_post_out *post, const smaltgpu_batch_out *raw, const smaltgpu_reads_view *reads,
                         const char *const *seqnames, int64_t nseq, const smaltgpu_report_opts *op, int nthreads, const char **text, uint64_t *len);
/* the lines of a block of pairs: both mates of pair 0, both mates of pair 1, ... (reportWrite, report.c:1758).  `reads` / `mates` =
 * the parsed blocks the pairs were mapped from.  Random choices (SMALTGPU_OUT_RANDSEL) draw from drand48() in pair order. */
int smaltgpu_report_emit_pairs(smaltgpu_report *rp, const smaltgpu_pairs *pairs, const smaltgpu_reads_view *reads, const smaltgpu_reads_view *mates,
                               const char *const *seqnames, int64_t nseq, const smaltgpu_report_opts *op, const smaltgpu_pair_opts *po, int nthreads,
                               const char **text, uint64_t *len);
/* SMALTGPU_FMT_BAM: the three calls above hand out whole BGZF blocks instead of text -- smaltgpu_report_header the magic, the SAM header
 * text (empty without SMALTGPU_REP_HEADER) and the list of sequences (always), the emit functions one record per line the SAM format
 * would have printed for the same modflags, in the same order: refID / next_refID are the places of RNAME / RNEXT in the sequence
 * list (-1 for '*'), pos / next_pos the printed values - 1, the optional fields NM and AS as int32.  The records of a call are cut into
 * payloads of 0xff00 bytes wherever that falls (a record may span blocks), the payloads are deflated on `nthreads` threads and every
 * call ends its last block, so the bytes depend neither on the number of threads nor on an earlier call.  The deflate level is
 * zlib's default, or SMALTGPU_BAM_LEVEL (0..9) as the environment has it when the report is created.  A read name longer than 254
 * bytes or an alignment of more than 65535 CIGAR operations fails the emit call with SMALTGPU_EARG (the message names the read);
 * SMALTGPU_REP_ALIOUT fails all three calls with SMALTGPU_EARG.
 * smaltgpu_report_finish: what ends the output -- for SMALTGPU_FMT_BAM the 28-byte empty block that marks the end of a BAM file, for
 * the text formats nothing (len 0).  Header, emit outputs and this, written one behind the other, are a complete BAM file. */
int smaltgpu_report_finish(smaltgpu_report *rp, const smaltgpu_report_opts *op, const char **text, uint64_t *len);
/* ---- insert-size histograms: `smalt sample` and `smalt map -g <file>` (insert.c; host code, smg_inshist.cpp) -------------------
 * `smalt sample` maps every n-th pair of a library, takes the template length of each pair whose two best alignments have a
 * mapping quality of at least 20 (resultSetInferInsertSize, results.c:2460; smalt.c:1180-1182, :850-854) and writes the histogram
 * of these lengths behind the SAM lines (outputHisto, smalt.c:1288-1310).  `smalt map -g` reads that file back, widens the insert
 * range to the histogram's (smalt.c:417-426, :570) and weighs oriented, in-range pairings by the cumulative smoothed count of
 * their template length when a pair has several pairings (assignProbabilityToPairs, resultpairs.c:782-806). */
typedef struct smaltgpu_inshist smaltgpu_inshist;
/* every how many pairs one is sampled: npairs / 4098, at least 1, `every` (-u) where that is smaller and above 0
 * (insSetSamplingInterval, insert.c:192-205).  Pair i is mapped when i % interval == 0 (loadIOBuffArg, smalt.c:795-835) */
int smaltgpu_sample_interval(uint64_t npairs, int every);
/* histogram of a sample of n insert sizes, smoothed (insMakeHistoFromSample insert.c:330-387, insSmoothHisto :472-514, smoothGauss
 * :253-303, calcKernelBandWidth :136-146).  SMALTGPU_EARG when the sample gives none (fewer than 2 sizes inside the binned range) */
int smaltgpu_inshist_from_sample(smaltgpu_inshist **out, const int32_t *sample, uint64_t n);
/* the HISTO_START ... HISTO_END section of a file, smoothed after reading; what stands ahead of the section is skipped
 * (insReadHisto, insert.c:632-705).  SMALTGPU_EFILE: no such file, HISTO_END missing, the counts do not add up to HISTO_TOTNUM,
 * a bin out of sequence, more bins than HISTO_BINNUM */
int smaltgpu_inshist_read(smaltgpu_inshist **out, const char *path);
void smaltgpu_inshist_free(smaltgpu_inshist *h);
/* text of a histogram, owned by it and valid until the next call: the bar print of the sampled or of the smoothed counts with
 * lines of at most `width` bars (insPrintHisto, insert.c:574-601), or the file section of the sampled counts with its title line
 * (insWriteHisto, insert.c:603-630; width is ignored) */
enum { SMALTGPU_HIST_SAMPLED = 0, SMALTGPU_HIST_SMOOTHED = 1, SMALTGPU_HIST_SECTION = 2 };
int smaltgpu_inshist_text(smaltgpu_inshist *h, int what, int width, const char **text, uint64_t *len);
/* smallest and largest insert size of the bins, their number and the number of sizes counted (insGetHistoData, insert.c:558-565);
 * any pointer may be NULL */
int smaltgpu_inshist_bounds(const smaltgpu_inshist *h, int32_t *lo, int32_t *hi, int32_t *nbins, uint64_t *total);
/* count of the bin of an insert size and the sum of the counts up to and including that bin, of the smoothed (smoothed != 0) or the
 * sampled counts; both 0 outside the bins (insGetHistoCount insert.c:531-542, insGetHistoCountCumulative :544-556); either may be NULL */
int smaltgpu_inshist_count(const smaltgpu_inshist *h, int32_t insert_size, int smoothed, int32_t *count, int32_t *cumulative);
/* later smaltgpu_report_emit_pairs calls on this report choose among pairings with the histogram (the ihistp argument of
 * resultSetAddPairToReport, smalt.c:1172-1176); h = NULL detaches it.  The report does not own the histogram.  The caller widens
 * insert_min / insert_max of the smaltgpu_pair_opts it hands to smaltgpu_map_pairs AND smaltgpu_report_emit_pairs to the
 * histogram's bounds (updateInsertBoundariesFromSample, smalt.c:417-426) */
int smaltgpu_report_set_inshist(smaltgpu_report *rp, const smaltgpu_inshist *h);
/* the host copy of the packed reference (smaltgpu_index_packed_host) for the alignment blocks of SMALTGPU_REP_ALIOUT (fprintAlignment,
 * report.c:248-388, called from writeReportForRead, report.c:1521-1526): the reference row of a block is read from it at the sequence
 * offsets smaltgpu_report_header was given.  Borrowed: it must outlive the report; NULL detaches it.  The emit functions return
 * SMALTGPU_EARG when the flag is set and no reference, or no header call, came first -- they never print lines without their blocks.
 * A block is "    QUERY: <first> <letters> <last>", a row of markers under the letters (blank: match, i: transition, v: transversion,
 * ?: a letter other than ACGT takes part, -: gap) and "REFERENCE: <first> <letters> <last>", then two empty lines.  Coordinates are
 * 1-based, the reference's within its sequence; the read of a reverse alignment is shown as its reverse complement with descending
 * coordinates.  A line breaks after 60 columns, gaps included; an alignment of exactly 60, 120, ... columns ends with one more block of
 * empty rows, as in the reference program. */
int smaltgpu_report_set_reference(smaltgpu_report *rp, const uint32_t *packed_host);
/* per pair of the last smaltgpu_report_emit_pairs call on this report: the insert size `smalt sample` would add to its sample and
 * whether there is one (resultSetInferInsertSize, results.c:2460-2483, called behind the report of the pair: smalt.c:1180-1182).
 * The arrays belong to the report and hold until its next emit call */
int smaltgpu_report_pair_inserts(const smaltgpu_report *rp, const int32_t **insert_size, const uint8_t **known, uint32_t *npairs);

/* names and offsets of the reference sequences of an index (for the two calls above); the arrays belong to the index */
int smaltgpu_index_seqnames(const smaltgpu_index *ix, const char *const **names, const uint64_t **sop, int64_t *nseq);

/* Per-kernel device time (ms, HIP events on the mapper's stream) and work counters of the last
 * batch: names in smaltgpu_timer_name().  For bench.py's roofline object. */
int smaltgpu_timers(const smaltgpu_mapper *m, double *ms, uint64_t *work, int n);
const char *smaltgpu_timer_name(int i);

/* Diagnostic: print the per-stage state of read `i` of the last batch in the line format of
 * oracle/DUMPFORMAT.md into buf (returns bytes needed).  Requires smaltgpu_set_debug(m, 1)
 * before the batch so that intermediate buffers are retained. */
int smaltgpu_set_debug(smaltgpu_mapper *m, int level);
long smaltgpu_dump_read(smaltgpu_mapper *m, uint32_t i, const char *name, char *buf, size_t bufsiz);

/* Stand-alone kernel entry points used by the parity tests (host pointers in, host out). */
/* K2a (swsimd.c:868, un-banded score pass) over explicit 3-bit code arrays.  packed16 = 1: the kernel that scores two
 * tasks per lane group in 16-bit halves (a task whose query holds non-ACGT codes reports -2: the mapper routes those
 * to the 32-bit kernel); packed16 = 0: the 32-bit kernel.  A batch with a read above 512 bases or a window above 1016
 * goes to the strip kernels: packed16 = 0 to the 32-bit one, packed16 = 1 to the packed one (tasks 2t and 2t+1 share a
 * wave; its max3 form where the longest read's best score + 512 stays below 0x7C00, else its plain form;
 * SMALTGPU_EARG if the penalties or match x longest read >= 60000 rule the 16-bit halves out).  Score -1: window above
 * the register tiling or, in the strip kernels, above the mapper's window capacity. */
int smaltgpu_sw_full_batch(smaltgpu_mapper *m, const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                           const uint32_t *r_off, uint32_t ntask, const smaltgpu_params *par, int32_t *scores, int packed16);

/* K2b (alignment.c:1029, banded score pass) over explicit 3-bit code arrays: band[4t..4t+3] = {band_l, band_r, qs, qe} of
 * task t, the band set up over the whole window as the mapper does.  form 0: the wave kernel's pass (one wave per task),
 * form 1: the one-lane pass.  The windows are packed back to back in the index's layout (10 bases per word), so they start
 * at every phase of a word.  status[t] = 1 where the band is refused (the mapper drops such a candidate), else 0. */
int smaltgpu_sw_band_batch(smaltgpu_mapper *m, const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                           const uint32_t *r_off, uint32_t ntask, const smaltgpu_params *par, const int32_t *band, int form,
                           int32_t *scores, int32_t *status);

/* K3, one node of the recursion (alignment.c:1300): band set-up over the window rows [s_left, s_right], the band pass in ONE
 * named form, the traceback the mapper pairs with that form, and the forward DiffStr.  A task outside the form's
 * precondition fails the whole call with SMALTGPU_EARG; there is no fall-back to another form. */
enum {
  SMALTGPU_BAND_ROWS = 0,      /* 1..64 diagonals, gap_init >= gap_ext >= 0 in absolute value; lds = 1: read and window (and the
                                  directions, if they fit) staged in LDS */
  SMALTGPU_BAND_ANTIDIAG = 1,  /* 1..64 diagonals */
  SMALTGPU_BAND_WAVE2 = 2, SMALTGPU_BAND_WAVE4 = 3, SMALTGPU_BAND_WAVE7 = 4, SMALTGPU_BAND_WAVE12 = 5,  /* (r_edge - l_edge) / 128 + 1 <= N */
  SMALTGPU_BAND_STRIP8 = 6,    /* 256 <= diagonals < 2048 */
  SMALTGPU_BAND_STRIP16 = 7,   /* diagonals >= 2048 */
  SMALTGPU_BAND_SCALAR = 8,    /* any band, one lane */
  SMALTGPU_BAND_NFORMS = 9
};
enum { SMALTGPU_NODE_ALIGNED = 0, SMALTGPU_NODE_REFUSED = 1 /* band refused: no node */, SMALTGPU_NODE_BELOW = 2 /* maximum below minscore */ };
typedef struct smaltgpu_band_node {
  int32_t status;              /* SMALTGPU_NODE_* or SMALTGPU_ESCORE / SMALTGPU_EINTERNAL / SMALTGPU_ECAP */
  int32_t score, max_i, max_j; /* maximum of the pass and its first cell in row-major order (window row, read column) */
  int32_t qs, rs;              /* where the traceback ends */
  int32_t dlen;                /* forward DiffStr with its terminator: dstr[stroffs .. stroffs + dlen) */
  uint32_t stroffs;
} smaltgpu_band_node;
/* band as above; iv[2t..2t+1] = {s_left, s_right}; tw = 1: directions of the anti-diagonal and wave forms in the
 * anti-diagonal-major layout the mapper uses for a direction matrix in HBM, tw = 0: row-major (other forms ignore it);
 * dstr: room for the sum over the tasks of (read length + window length + 16) bytes. */
int smaltgpu_band_align_nodes(smaltgpu_mapper *m, const uint8_t *qcodes, const uint32_t *q_off, const uint8_t *rcodes,
                              const uint32_t *r_off, uint32_t ntask, const smaltgpu_params *par, const int32_t *band, const int32_t *iv,
                              int minscore, int form, int lds, int tw, smaltgpu_band_node *out, uint8_t *dstr);
/* Host only: the band of such a node as the kernels see it.  geo[0..12] = band_width, l_edge_orig, r_edge_orig, l_edge, r_edge,
 * s_left_orig, s_left, s_len, s_totlen, q_left_orig, q_left, q_len, q_totlen; geo[13] = the form the mapper's K3 kernel for
 * long reads picks for it (SMALTGPU_BAND_*; an HBM direction matrix with room for any layout assumed).  Returns 0, or 1 if
 * the band is refused (geo is then undefined). */
int smaltgpu_band_geometry(int band_l, int band_r, int qs, int qe, int qlen, int s_left, int s_right, int wlen, int gap_init,
                           int gap_ext, int32_t *geo);

/* Which sweeps the packed K2a kernel runs in its row-frame form: the largest number of sweep steps (window
 * rows + G - 1) for these penalties (gap scores negative, as in smaltgpu_params) and a tiling of ncols = G * C read
 * columns; -1 if the penalties rule the form out.  No device needed. */
int smaltgpu_sw_rowframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols);
/* The same for the pair-frame form, which the kernel tries first: every sweep of at most this many steps runs in it. */
int smaltgpu_sw_pairframe_max_steps(int match, int mismatch, int gap_init, int gap_ext, int ncols);

/* The candidate ranking sort of segAliCandsStats (segment.c:1733 -> sort.c:233): `narr` arrays of keys (< 1024), array t
 * in keys[off[t]..off[t+1]); returns the keys and the permutation (index into the array) in the reference's tie order
 * for ranks < nneed (all ranks if nneed < 0; ranks at or beyond nneed may be left unsorted).  in_lds: sort in LDS.
 * instance 0: the sort as the candidate stage runs it.  instance 1: as the seeding stage runs it on the hit counts of a strand's
 * seeds (hashhit.c:1040 -> sort.c:233) -- elements packed with 12 index bits, in LDS, all ranks (nneed and in_lds are not
 * looked at): arrays of fewer than 4096 keys below 2^20, SMALTGPU_EARG otherwise. */
int smaltgpu_rank_sort_batch(smaltgpu_mapper *m, const uint32_t *keys, const uint32_t *off, uint32_t narr, int nneed, int in_lds,
                             int instance, uint32_t *out_keys, uint32_t *out_idx);

/* S1 + S2 on their own (kernels k_encode and k_seed): the reads are uploaded and the two launches of a mapping call run on the
 * mapper's own buffers, nothing behind them.  Before the launch the rows of the batch in the hit-info headers, the seed tables
 * and the qualifier rows, and ONE row behind the last strand, are filled with the byte `guard`; all nrows = 2 * nreads + 1 rows
 * come back, so what the kernel left alone still holds the guard.  The caller provides the arrays of smaltgpu_seed_out; their stride
 * is out[6] of smaltgpu_cands_geometry.
 * seed_range: [2 * nreads] (first, last) base as in smaltgpu_callctx, or NULL.  totals_only: the batch stops behind the
 * lookups as in smaltgpu_hit_totals.  scratch_home 0: the stage's scratch where the mapper keeps it (LDS up to 48 KiB, HBM
 * slots above); 1: HBM slots, allocated for this call where the mapper has none.  grid: workgroups, 0 = the launcher's choice.
 * SMALTGPU_EARG: seed_range together with totals_only; a grid above the slot count when the scratch is in HBM; a read longer
 * than the mapper's max_read_len; nreads >= the mapper's capacity (the guard row). */
typedef struct smaltgpu_seed_out {
  uint8_t *codes, *codes_rc;         /* [total bases] 3-bit codes, forward and reverse complement */
  uint32_t *hi;                      /* [nrows][8]: n_seeds, seed_rank, status, qlen, nhit_rank, nhit_tot, nhit_cut, (unused) */
  uint32_t *seeds;                   /* [nrows][stride][3]: posidx, nhits, qoffs in rank order */
  uint8_t *qmask;                    /* [nrows][stride] */
  uint32_t nrows, stride;
  uint32_t in_lds, grid;             /* where the scratch was and how many workgroups ran */
  uint64_t lookups;                  /* index lookups of the batch (work counter) */
} smaltgpu_seed_out;
int smaltgpu_seed_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                        const smaltgpu_params *par, const uint32_t *seed_range, int totals_only, int scratch_home, uint32_t grid,
                        uint8_t guard, smaltgpu_seed_out *out);

/* k_gather_reads on its own: two host batches (offsets from 0; qualities for both or neither) go up as the two resident batches
 * of a block of pairs, the mapper's read buffers are filled with the byte `guard`, the kernel gathers reads `ids` (read
 * ids[i] >> 1 of batch ids[i] & 1) and the result comes back: dst_off [nids + 1], dst_bases and dst_quals [dst_off[nids] + tail]
 * (tail <= 16 bytes behind the last read, which must still hold the guard; without qualities dst_quals, if given, is all guard). */
int smaltgpu_gather_batch(smaltgpu_mapper *m, const uint8_t *const bases[2], const uint8_t *const quals[2], const uint64_t *const read_off[2],
                          const uint32_t nreads[2], const uint32_t *ids, uint32_t nids, uint8_t guard, uint32_t tail,
                          uint8_t *dst_bases, uint8_t *dst_quals, uint64_t *dst_off);

/* S3 on its own (kernel k_hits): the reads are uploaded and the launches of a mapping call run up to and including k_hits
 * (encode, seed, hits -- the mapper's own launchers, geometry and buffers, no other kernel); what the kernel left behind comes
 * back in host copies owned by the mapper, valid until its next call.  Indexed by rs = 2 * read + strand; `stride` entries
 * per strand in seeds and qmask. */
enum { SMALTGPU_HITRUN_NONE = 0,     /* the candidate stage gathers and sorts this strand itself */
       SMALTGPU_HITRUN_SORTED = 1,   /* pool[off .. off + n) holds the strand's keys in ascending order */
       SMALTGPU_HITRUN_OVERFLOW = 2  /* the pool was full: a mapping call re-maps the read in a smaller batch */ };
typedef struct smaltgpu_hit_seed { uint32_t posidx, nhits, qoffs; } smaltgpu_hit_seed;
typedef struct smaltgpu_hit_run { uint64_t off; uint32_t n, mode; } smaltgpu_hit_run;
typedef struct smaltgpu_hits_out {
  uint32_t nstrands, stride;         /* 2 * nreads; entries per strand of seeds and qmask */
  uint32_t window, tab;              /* keys per window and entries of the per-list tables the kernel ran with */
  const uint32_t *n_seeds, *seed_rank, *status;   /* [nstrands] hit info of the seeding stage */
  const smaltgpu_hit_seed *seeds;    /* [nstrands][stride] */
  const uint8_t *qmask;              /* [nstrands][stride] hit qualifier per read offset, after k_hits */
  const smaltgpu_hit_run *runs;      /* [nstrands] */
  uint64_t hit_count;                /* keys reserved in the pool by all strands (may exceed pool_cap) */
  uint64_t pool_cap;                 /* capacity the kernel ran with */
  const uint64_t *pool;              /* the first min(hit_count, pool_cap) keys of the pool */
} smaltgpu_hits_out;
/* window: keys per window for this call (clamped to 256..1024 as at mapper creation), 0 = the mapper's; pool_keys: capacity of
 * the pool for this call, 0 = the mapper's (SMALTGPU_EARG above the allocation).  SMALTGPU_EARG for a mapper that keeps S3
 * inside the candidate stage (max_read_len > 248, that is a stride of more than 256 read offsets, or SMALTGPU_HITS_SPLIT=0) and
 * for a batch above the mapper's capacity. */
int smaltgpu_hits_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                        const smaltgpu_params *par, uint32_t window, uint64_t pool_keys, smaltgpu_hits_out *out);
/* How k_hits gathered the strands of the mapper's last call (a mapping call or smaltgpu_hits_batch).  windows (null, or
 * [nstrands], nstrands <= 2 * reads of that call): per strand, bits 0..15 the windows it was gathered in (0: one gather, no keys,
 * or a strand the kernel left alone), bits 16..31 those of them whose bound was raised above the safe one.  totals[0]: sorted
 * strands gathered in several windows, [1]: their windows, [2]: their keys, [3]: keys reserved in the pool by the call.  All
 * zero where the call did not run the kernel (restricted calls, mappers whose candidate stage keeps S3: max_read_len > 240). */
int smaltgpu_hits_windows(smaltgpu_mapper *m, uint32_t nstrands, uint32_t *windows, uint64_t totals[4]);

/* The on-the-fly index of the rescue round on its own (kernel k_fine_index): the intervals of nreads reads go up as in a call of
 * smaltgpu_map_batch_ctx with fine_index set, the mapper's position buffer (with one word behind the last read's slice) and
 * index rows are filled with `guard`, the kernel runs on `grid` workgroups (0 = one per read, as in a mapping call) and the
 * buffers come back in host copies owned by the mapper, valid until its next call of this function.  Read r owns
 * idx[r * idx_stride .. + nkeys] (first position of every key's list, idx[nkeys] = words indexed) and
 * pos[fine_off[r] .. fine_off[r + 1]): the slice is sized for every word of the windows, so its tail behind idx[nkeys] is
 * unused where words hold non-standard bases. */
typedef struct smaltgpu_fine_out {
  uint32_t nreads, idx_stride, nkeys;
  uint64_t npos;                     /* words of pos: fine_off[nreads] + 1 */
  const uint32_t *fine_off;          /* [nreads + 1] */
  const uint32_t *idx;               /* [nreads][idx_stride] */
  const uint32_t *pos;               /* [npos] */
} smaltgpu_fine_out;
int smaltgpu_fine_index_batch(smaltgpu_mapper *m, uint32_t nreads, const uint64_t *iv_off, const smaltgpu_interval *iv, uint32_t grid,
                              uint32_t guard, smaltgpu_fine_out *out);
/* Scratch geometry of the candidate stage (read-only, for tests that predict its branches): first-pass hits per strand,
 * candidate capacity and bytes of the LDS working set when S3 runs inside the stage; the same three of the second pass (0: the
 * mapper has one pass); the stride of read offsets; the most intervals a read of a restricted call may have. */
int smaltgpu_cands_geometry(smaltgpu_mapper *m, uint32_t out[8]);

/* The 64-bit key sorts of the candidate stage, one wave per array (array t in keys[off[t]..off[t+1])): the array is copied to
 * LDS, sorted and copied out.  form 0, 1, 2: the register network over 4, 8, 16 keys per lane (arrays of at most 256, 512,
 * 1024 keys); form 3: the network in LDS (at most 1024 keys).  form 4, 5: the sorts of the HBM working set, the network over
 * global memory and the sort in chunks of 1024 keys (registers inside a chunk, memory across chunks); the array is copied to its
 * place in out and sorted there, at most 65536 keys.  SMALTGPU_EARG for a longer array. */
int smaltgpu_sort_u64_batch(smaltgpu_mapper *m, const uint64_t *keys, const uint32_t *off, uint32_t narr, int form, uint64_t *out);

/* O1 and the K3 driver on their own (kernels k_replay and k_align): the reads are uploaded and encoded, the caller's ranked
 * candidates WITH their first-pass scores take the place of what the candidate stage and the score kernels leave in the batch,
 * and the tail of a mapping call runs on the mapper's own scratch, slots and capacities: k_replay, then both passes of k_align.
 * The production score kernels are not part of it (their task routing follows lists the candidate stage builds; smaltgpu_score_pool
 * below shows what they left after a mapping call), nor are the
 * complexity-weighted scores (SMALTGPU_EARG with SMALTGPU_FLG_CMPLXW).  Read r owns cands[cand_off[r] .. cand_off[r + 1]) in rank
 * order and cover_deficit[2 r + strand].  Of ctx (may be NULL) prev_max, min_swatscor and raw_alignments are honoured;
 * SMALTGPU_EARG if iv_off, fine_index or seed_range is set.  flags: SMALTGPU_ALIGN_CANDS_ANTIDIAG or 0.
 * Nothing is repaired: SMALTGPU_EARG unless the offsets ascend, the candidates fit the mapper's candidate pool, and every
 * candidate has -1 <= sqidx < nseq (-1: the window lies in the concatenated set), rs <= re inside that sequence and
 * 0 <= swscor <= read length x match (a larger score is the reference's error and cannot come from the score kernels).
 * The results come back as from a mapping call (out->batch; the return value is the first per-read error, as there), with the
 * hit numbers of the stats 0; out->ctl[r] is what k_replay left for read r; out->n_deferred counts the reads the first pass
 * of k_align handed to the second.  The arrays belong to the mapper and hold until its next call. */
enum { SMALTGPU_CAND_REVERSE = 1, SMALTGPU_CAND_ERR = 2 /* the candidate stage marked the candidate as broken (RCF_ERR) */ };
enum { SMALTGPU_ALIGN_CANDS_ANTIDIAG = 0x100 /* narrow bands in the anti-diagonal form, as under SMALTGPU_ALIGN_ANTIDIAG */ };
typedef struct smaltgpu_cand {
  uint64_t rs, re;                   /* window in sequence sqidx, 0-based inclusive */
  uint32_t qs, qe;
  int32_t band_l, band_r;
  int32_t sqidx;
  uint32_t flags;                    /* SMALTGPU_CAND_* */
  uint32_t cover;
  int32_t swscor;                    /* first-pass score */
} smaltgpu_cand;
typedef struct smaltgpu_readctl {    /* scalars of mapSingleRead (rmap.c:1373-1400) as k_replay leaves them */
  int32_t max1, max2, n_scored;
  int32_t bandwidth_min, min_swatscor, scorlen_min;
  int32_t go;                        /* 1: the traceback pass runs */
  int32_t pad;
} smaltgpu_readctl;
typedef struct smaltgpu_align_cands_out {
  smaltgpu_batch_out batch;
  const smaltgpu_readctl *ctl;       /* [nreads] */
  uint32_t n_deferred;
} smaltgpu_align_cands_out;
int smaltgpu_align_cands_batch(smaltgpu_mapper *m, const uint8_t *bases, const uint8_t *quals, const uint64_t *read_off, uint32_t nreads,
                               const smaltgpu_params *par, const smaltgpu_callctx *ctx, const uint64_t *cand_off, const smaltgpu_cand *cands,
                               const uint32_t *cover_deficit, uint32_t flags, smaltgpu_align_cands_out *out);

/* What the first-pass score stage (the launchers of K2a and K2b in a mapping call) left in the candidate pool of the mapper's
 * last mapping call, debug or not: the stream is waited for and the first min(rc_count, rccap) records come back in pool order
 * -- the records of a read are contiguous and in rank order, the reads in the order their waves reserved room -- in a host copy
 * the mapper owns until its next call.  Nothing is launched and nothing on the device changes.  With them the geometry the task
 * routing of the stage depends on (tests/score_route_ref.py restates the routing).  After a call that re-mapped reads of an
 * overflowing batch the pool is that of the last of the smaller batches. */
enum { SMALTGPU_RCF_REVERSE = 1, SMALTGPU_RCF_SCORED = 2, SMALTGPU_RCF_BANDED = 4 /* K2b scores it: by S7's rule, or after a K2a score >= 65535 */,
       SMALTGPU_RCF_ERR = 8, SMALTGPU_RCF_QN = 16 /* the read holds a non-ACGT code */, SMALTGPU_RCF_BSCORED = 32 /* swscor is the wave kernel's K2b score */ };
typedef struct smaltgpu_pool_rec {
  uint64_t rs, re;                   /* window in sequence sqidx (sqidx < 0: in the concatenated set), 0-based inclusive */
  uint32_t qs, qe;
  int32_t band_l, band_r;
  int32_t sqidx;
  uint32_t flags;                    /* SMALTGPU_RCF_*, as the stage left them */
  uint32_t cover;
  int32_t swscor;
  uint32_t rid;                      /* read of the batch */
  uint32_t pad;
} smaltgpu_pool_rec;
typedef struct smaltgpu_score_pool_out {
  const smaltgpu_pool_rec *rec;      /* [nrec] */
  uint32_t nrec;                     /* min(rc_count, rccap) */
  uint32_t rc_count;                 /* records the batch asked for (above rccap: the pool overflowed) */
  uint32_t rccap, long_cap, strip_cap;   /* capacities of the pool, of the list of windows above 248 bases and of the strip list */
  uint32_t tile_qmax;                /* longest read of the register-tiled kernels: tile_g * tile_c, 0 where the mapper has no tiling */
  uint32_t wincap;                   /* longest window of the strip kernels and of the wave form of K2b */
  uint32_t tile_g, tile_c;
  uint32_t full_grid, strip_grid;    /* workgroups of the register-tiled and of the strip kernels */
} smaltgpu_score_pool_out;
int smaltgpu_score_pool(smaltgpu_mapper *m, smaltgpu_score_pool_out *out);

const char *smaltgpu_last_error(void);
int smaltgpu_device_count(void);

#ifdef __cplusplus
}
#endif
#endif

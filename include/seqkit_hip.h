/*
 * seqkit_hip.h — C-ABI of the MI355X (gfx950) implementation of seqkit's per-read hot path.
 *
 * The reference (annalam/seqkit v0.8.0, Rust) has no FFI/plugin interface: every command is a
 * `while read_line` loop with the arithmetic inlined.  This header is the seam a
 * host (the reference's Rust `fasta`/`sam` binaries, or this repo's C++ ones) binds to replace the
 * inlined per-read arithmetic.  Each entry point cites the reference lines it replaces; paths are
 * relative to the reference tree.  INTEGRATION.md shows the Rust `extern "C"` block.
 *
 * Conventions
 *  - plain pointers and sizes only; every function returns SK_OK (0) or a negative SK_ERR_* code and
 *    never throws or aborts; sk_last_error() gives the message for the last failure on that ctx.
 *  - one sk_ctx per GPU; a ctx is used by one host thread at a time; a ctx owns one HIP stream.
 *  - read batches are fixed-stride SoA: row r of a byte matrix lives at base + r*stride, only its first
 *    len[r] bytes are data (len == NULL: every row holds exactly `stride` bytes).  Bytes past len[r]
 *    are ignored on input; on output (masked sequence) they are unspecified.
 *  - functions without suffix take HOST pointers and are synchronous (they stage through device
 *    workspace owned by the ctx).  `_dev` functions take DEVICE pointers, enqueue on the ctx stream
 *    and return immediately; sk_sync() waits.  Device byte matrices must be 16-byte aligned, and readable up
 *    to the next 4-byte boundary behind their last row (the kernels read whole dwords: when n * stride is not a
 *    multiple of 4, up to 3 bytes past the matrix are fetched and ignored — any allocation of a whole number of
 *    dwords, every hipMalloc, provides them).  Device OUTPUT columns of a demultiplex call are written with wide
 *    stores: assign must be 16-byte aligned, lowest_diff 4-byte, first_idx / last_idx 8-byte (any hipMalloc'ed base
 *    is; a column sliced at an odd row is refused with SK_ERR_INVALID).
 *  - there is no CPU fallback: without a usable GPU sk_create() fails and nothing else can be called.
 */
#ifndef SEQKIT_HIP_H
#define SEQKIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_OK            0
#define SK_ERR_INVALID  (-1)   /* bad argument (NULL, negative size, misaligned device pointer, ...) */
#define SK_ERR_HIP      (-2)   /* HIP runtime failure; sk_last_error() has hipGetErrorString          */
#define SK_ERR_NO_DEVICE (-3)  /* no gfx950-capable device at that index                              */
#define SK_ERR_STATE    (-4)   /* call order (e.g. demux before sk_set_barcodes)                      */
#define SK_ERR_NOMEM    (-5)
#define SK_ERR_COMM     (-6)   /* RCCL: library not loadable, or a collective failed                   */

/* assignment codes written by the demultiplex entry points (src/fasta_demultiplex.rs:168-194) */
#define SK_ASSIGN_NONE      (-1)   /* lowest_diff > max_diff                                   */
#define SK_ASSIGN_AMBIGUOUS (-2)   /* lowest_diff <= max_diff but best != equally_fine sample  */

#define SK_MAX_BARCODE_LEN 255
#define SK_MAX_SAMPLES     32767

typedef struct sk_ctx sk_ctx;

/* ---- lifetime ------------------------------------------------------------------------------ */
int  sk_version(void);                                   /* 0x00MMmmpp */
int  sk_device_count(void);                              /* number of visible HIP devices (>= 0) */
int  sk_create(int device_id, sk_ctx **out);
void sk_destroy(sk_ctx *ctx);
const char *sk_last_error(const sk_ctx *ctx);            /* ctx may be NULL: last sk_create failure */
int  sk_sync(sk_ctx *ctx);                               /* wait for everything enqueued on the ctx stream */
void *sk_stream(sk_ctx *ctx);                            /* the ctx's hipStream_t, for interop */
int  sk_planned_cus(sk_ctx *ctx);                        /* the CU count the ctx plans its launches with: the device's own,
                                                          * unless SK_PLAN_CUS (tests only; read once, at creation) names a smaller one */

/* ---- device / pinned memory for hosts that do not link HIP themselves ------------------------ */
int sk_malloc_device(sk_ctx *ctx, size_t bytes, void **out);
int sk_free_device(sk_ctx *ctx, void *p);
/* the two pinned calls may come from any thread while another runs a pass on the ctx: they write nothing to it (a failure is
 * the return code only; sk_last_error is unchanged) and bind the ctx's device to the calling thread */
int sk_malloc_pinned(sk_ctx *ctx, size_t bytes, void **out);
int sk_free_pinned(sk_ctx *ctx, void *p);
int sk_copy_h2d(sk_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* async on ctx stream */
int sk_copy_d2h(sk_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);   /* async on ctx stream */

/* ---- sample sheet -> barcode table -------------------------------------------------------------
 * Replaces the per-read walk over `samples[s].barcode` (src/fasta_demultiplex.rs:157-158, Sample
 * :23-28, sheet rules :58-104 stay on the host).  table = S rows of L bytes, sheet order.  Candidate
 * bytes 'N' and 'U' are wildcards (src/fasta_demultiplex.rs:273).  max_diff is the reference's
 * MAX_BARCODE_DIFFERENCE = 1 (:168).  Resets the counters.                                        */
int sk_set_barcodes(sk_ctx *ctx, const uint8_t *table, int S, int L, int max_diff);

/* ---- D1+D2+D3: barcode_diff + best-match loop + decision ----------------------------------------
 * src/fasta_demultiplex.rs:269-277, :154-166, :168-194.  bc = n observed barcodes of exactly L bytes,
 * row stride bc_stride >= L.  Outputs (each nullable except assign): assign[r] = sample index, or
 * SK_ASSIGN_NONE / SK_ASSIGN_AMBIGUOUS; lowest_diff[r] (saturates at 255; 255 when S == 0);
 * first_idx[r] = best_sample, last_idx[r] = equally_fine_sample.  Adds to the ctx counters.         */
int sk_demux_assign(sk_ctx *ctx, const uint8_t *bc, int bc_stride, int64_t n,
                    int32_t *assign, uint8_t *lowest_diff, int16_t *first_idx, int16_t *last_idx);
int sk_demux_assign_dev(sk_ctx *ctx, const uint8_t *bc, int bc_stride, int64_t n,
                        int32_t *assign, uint8_t *lowest_diff, int16_t *first_idx, int16_t *last_idx,
                        uint64_t *counts /* device u64[S+3], NULL = ctx counters */);

/* Which rows the detail columns (lowest_diff / first_idx / last_idx) are defined for.  The reference looks at them in one
 * place only, the ambiguity warning (src/fasta_demultiplex.rs:184-188), i.e. for reads with lowest_diff <= max_diff; the
 * branch of a read that matched nothing (:190-194) never does.
 *   SK_DETAIL_FULL    (default) every row, as the loop :154-166 leaves them.
 *   SK_DETAIL_MATCHED rows with assign != SK_ASSIGN_NONE; the detail of SK_ASSIGN_NONE rows is unspecified (255 / -1 /
 *                     -1 when the lookup table answers).  A demultiplex-alone call with max_diff <= 1 is then ONE table
 *                     lookup per read — the sheet's rows and their one-substitution neighbours, decided on the host with
 *                     the same loop — instead of S x L compares, for sheets of <= 1021 samples, <= 20 columns, <= 7
 *                     letters (8 to 15 letters — a sheet typed partly in lower case — when its rows, or the two halves
 *                     beside a separator, are at most 8 columns; a row with `N` / `U` where other rows hold a letter is entered once per class of that
 *                     column: a few such columns per row, up to 220 000 keys in all); a dual-index sheet whose table would not fit a
 *                     workgroup's LDS is looked up half by half when that is exact (its half-barcodes at least 3
 *                     apart); other sheets run the matchers and fill every row.  The decision-only form (all three
 *                     pointers NULL) takes the table under either mode, and so does the barcode phase of a fused call
 *                     whose sheet is beyond the tile pass's own matcher (128 samples).
 * Applies to sk_demux_assign(_dev) and sk_fused_pass(_dev) of this ctx from the next call on.                        */
#define SK_DETAIL_FULL    0
#define SK_DETAIL_MATCHED 1
int sk_set_detail_mode(sk_ctx *ctx, int mode);
/* What serves the calls described above for the current sheet (the table is built here if no call has asked for it yet;
 * src/fasta_demultiplex.rs:154-194 is what it answers either way): *kind = SK_TABLE_NONE (the S x L matchers), SK_TABLE_FULL_KEY
 * or SK_TABLE_FACTORED, or-ed with SK_TABLE_WIDE_CLASSES for a sheet of 8 to 15 letters; *keys = its entries, *bytes = its size
 * on the device.  Any of the three pointers may be NULL.  A host logs it; the tests assert which path they exercise.       */
#define SK_TABLE_NONE         0
#define SK_TABLE_FULL_KEY     1
#define SK_TABLE_FACTORED     2
#define SK_TABLE_WIDE_CLASSES 4
int sk_barcode_table_info(sk_ctx *ctx, int *kind, int64_t *keys, int64_t *bytes);

/* ---- T1: 3' running-sum quality trim --------------------------------------------------------------
 * src/fasta_trim_by_quality.rs:28-42.  qual rows are the quality line after trim_end(); writes
 * lowest_k[r] in [0, len[r]] (0 means the reference emits "N\n+\n!\n", :44-45).
 * _dev: qual must be 16-byte aligned (SK_ERR_INVALID otherwise, nothing is launched) and readable to the next
 * dword behind its last byte; len and lowest_k are u16 columns at their natural alignment; exactly 2 n bytes of
 * lowest_k are written.                                                                               */
int sk_trim_by_quality(sk_ctx *ctx, const uint8_t *qual, const uint16_t *len, int stride, int64_t n,
                       uint8_t min_baseq, uint16_t *lowest_k);
int sk_trim_by_quality_dev(sk_ctx *ctx, const uint8_t *qual, const uint16_t *len, int stride, int64_t n,
                           uint8_t min_baseq, uint16_t *lowest_k);

/* ---- M1: mask bases whose Phred+33 quality is below min_baseq ------------------------------------
 * src/fasta_mask_by_quality.rs:40-43 (byte form, i.e. ASCII lines; the host keeps non-ASCII lines).
 * out_seq may equal seq (in place).
 * _dev: seq, qual and out_seq must each be 16-byte aligned (SK_ERR_INVALID otherwise, nothing is launched); seq and
 * qual must be readable to the next dword behind their last byte; exactly n * stride bytes of out_seq are
 * written, whatever n * stride is a multiple of.                                                     */
int sk_mask_by_quality(sk_ctx *ctx, uint8_t *seq /* in/out */, const uint8_t *qual, const uint16_t *len,
                       int stride, int64_t n, uint8_t min_baseq);
int sk_mask_by_quality_dev(sk_ctx *ctx, const uint8_t *seq, const uint8_t *qual, int stride, int64_t n,
                           uint8_t min_baseq, uint8_t *out_seq);

/* ---- fused per-read pass: demultiplex (+ add barcode) + trim by quality + mask by quality ---------
 * One pass over a batch of n clusters with 1 or 2 mates.  `add barcode` (src/fasta_add_barcode.rs:
 * 19-44) is realised by handing the index read's bases over as the bc column instead of round-tripping
 * them through the header text; header handling (D4/D5) stays on the host.  Any of the three parts can
 * be switched off by leaving its outputs NULL:
 *   demultiplex : bc != NULL           -> assign (+ optional lowest_diff/first_idx/last_idx, counters)
 *   trim        : mate.lowest_k != NULL
 *   mask        : mate.out_seq  != NULL (may alias mate.seq)
 * The same struct serves the host and the _dev entry point.
 * _dev (sk_fused_pass_dev and every batch of sk_fused_pass_many_dev): qual of a mate with work, and seq and out_seq
 * of a mate that is masked, must be 16-byte aligned; bc and assign 16-byte, lowest_diff 4-byte, first_idx / last_idx
 * 8-byte aligned; len, lowest_k and counts at their natural alignment (2, 2 and 8 bytes).  A pointer short of its
 * rule: SK_ERR_INVALID, and nothing is launched — for the many-batch call no batch is.  seq, qual and bc must be
 * readable to the next dword behind their last byte (any allocation of a whole number of dwords provides that).
 * Outputs are written to exactly their size: n * stride bytes of out_seq (a row's bytes past len[r] unspecified),
 * 2 n of lowest_k, 4 n of assign, n of lowest_diff, 2 n of first_idx / last_idx, 8 (S + 3) of counts.          */
typedef struct {
	const uint8_t  *seq;        /* n x stride  (needed only for mask)           */
	const uint8_t  *qual;       /* n x stride                                   */
	const uint16_t *len;        /* n, or NULL = all rows are `stride` long      */
	uint8_t        *out_seq;    /* n x stride masked bases, or NULL             */
	uint16_t       *lowest_k;   /* n, or NULL                                   */
} sk_mate;

typedef struct {
	int64_t  n;                 /* clusters in the batch                        */
	int      n_mates;           /* 1 (single end) or 2 (paired end)             */
	int      stride;            /* row stride of seq/qual/out_seq, both mates   */
	uint8_t  min_baseq;         /* threshold for trim and mask                  */
	sk_mate  mate[2];
	const uint8_t *bc;          /* n x bc_stride observed barcodes, or NULL     */
	int      bc_stride;
	int32_t *assign;            /* n                                            */
	uint8_t *lowest_diff;       /* n or NULL                                    */
	int16_t *first_idx;         /* n or NULL                                    */
	int16_t *last_idx;          /* n or NULL                                    */
	uint64_t *counts;           /* _dev only: device u64[S+3] or NULL = ctx's   */
} sk_fused_args;

int sk_fused_pass(sk_ctx *ctx, const sk_fused_args *args);
int sk_fused_pass_dev(sk_ctx *ctx, const sk_fused_args *args);
/* Many independent batches in one call: what n_batches calls of sk_fused_pass_dev compute (same outputs; counters are sums, so
 * their order does not matter) — checked once, the sheet's table uploaded once.  Batches that are barcode assignment alone
 * and whose sheet is served by a table in LDS (sk_barcode_table_info) run as ONE launch whose waves walk the steps of all
 * batches (at most 256 batches a launch; the table staged once, ramp and tail paid once); every other shape is the
 * batches' launches back to back on the ctx stream — on the ctx's two streams in turn when no batch has a barcode phase (trim /
 * mask alone): sk_sync() waits for both — (src/fasta_demultiplex.rs:154-194, src/fasta_trim_by_quality.rs:28-42
 * work per read: reads are independent, so are batches).  Asynchronous like the _dev calls; sk_sync() waits.  The two
 * conveniences below build the argument blocks. */
int sk_fused_pass_many_dev(sk_ctx *ctx, const sk_fused_args *batches, int n_batches);
typedef struct sk_demux_batch {     /* device pointers, aligned as sk_fused_args' _dev rules say, batch by batch */
	const uint8_t *bc;          /* n x bc_stride; 16-byte aligned, readable to the next dword behind its last byte */
	int64_t n;
	int32_t *assign;            /* n; 16-byte aligned */
	uint8_t *lowest_diff;       /* n or NULL; 4-byte aligned */
	int16_t *first_idx, *last_idx;      /* n or NULL; 8-byte aligned */
} sk_demux_batch;
int sk_demux_assign_many_dev(sk_ctx *ctx, const sk_demux_batch *batches, int n_batches, int bc_stride);
typedef struct sk_trim_batch {      /* device pointers */
	const uint8_t *qual;        /* n x stride; 16-byte aligned, readable to the next dword behind its last byte */
	const uint16_t *len;        /* n or NULL */
	int64_t n;
	uint16_t *lowest_k;         /* n: exactly 2 n bytes are written */
} sk_trim_batch;
int sk_trim_by_quality_many_dev(sk_ctx *ctx, const sk_trim_batch *batches, int n_batches, int stride, uint8_t min_baseq);

/* ---- placement tuning for resident batches ---------------------------------------------------------------------------
 * WHERE the pages of a device buffer lie moves the fused pass by up to 12 % on one and the same GPU: measured on MI355X,
 * the same kernel on the same bytes takes 9.35 ms with one set of allocations and 10.6 ms with another, each reproducible
 * to 0.1 % for the life of the buffers, bimodal, and decided by how the buffers of the streams that are active together
 * relate to each other — not by their addresses' alignment, padding or order (tools/soa_placement_search.py,
 * tools/arena_sweep.py).  A host whose batch buffers live long (a resident shard that is processed many
 * times, a ring of staging buffers) can therefore choose once: it allocates k candidate device buffers for each big
 * matrix of the pass, fills the input candidates with the same bytes, and this call times the pass while it swaps one
 * matrix at a time for its other candidates (coordinate descent, `sweeps` rounds, 1 + 2 launches per probe) and leaves
 * the fastest combination in `args`.  The losers are the caller's to free.  Counters are not touched (the probes count
 * into a scratch vector).  ms_before / ms_after: the pass on the first candidates and on the chosen ones.            */
#define SK_MAX_CANDIDATES 8
typedef struct {
	int k;                                              /* candidates per matrix, 1..SK_MAX_CANDIDATES            */
	const uint8_t *seq[2][SK_MAX_CANDIDATES];           /* per mate; entries of an unused mate / matrix are NULL  */
	const uint8_t *qual[2][SK_MAX_CANDIDATES];
	uint8_t *out_seq[2][SK_MAX_CANDIDATES];
} sk_fused_candidates;
int sk_fused_tune_placement_dev(sk_ctx *ctx, sk_fused_args *args, const sk_fused_candidates *cands, int sweeps,
                                float *ms_before, float *ms_after, int *n_probes);

/* ---- the fused pass over a TILE-BLOCKED batch -----------------------------------------------------------------
 * Same arithmetic and the same reference lines as sk_fused_pass; only where the bytes sit differs.  A batch is cut
 * into tiles of 64 consecutive clusters.  Everything tile t READS is one contiguous block of `in_block` bytes at
 * in + t*in_block, everything it WRITES one block of `out_block` bytes at out + t*out_block; inside a block every
 * array of the 64 clusters is one segment: row (r mod 64) of mate m's qualities at  in_qual[m] + (r mod 64)*stride,
 * its bases at in_seq[m] + ..., the observed barcode at in_bc + (r mod 64)*bc_stride, the optional u16 length at
 * in_len[m] + 2*(r mod 64); outputs likewise (out_seq[m], u16 out_lowest_k[m], i32 out_assign, and with
 * SK_BLK_DETAIL u8 out_lowest_diff, i16 out_first_idx, i16 out_last_idx).  Offsets of absent segments are -1.
 * Both buffers hold WHOLE blocks also for the last, partial tile ((n+63)/64 blocks; the padding rows are read and
 * their outputs are unspecified).  Why: a device wave streams one read range and one write range per tile, and a
 * host moves a batch with ONE copy per direction.  sk_blocked_layout_init fills the struct from the shape; the
 * packer (host) owns the layout, so no existing file format is touched.  Served shapes: stride <= 960; with
 * barcodes, sheets of <= 128 samples over <= 7 distinct non-wildcard bytes, L <= 31, bc_stride <= 32 — everything
 * else takes sk_fused_pass(_dev) (SK_ERR_INVALID here).                                                          */
#define SK_BLK_MASK   1     /* out_seq segments (mask by quality)                 */
#define SK_BLK_TRIM   2     /* out_lowest_k segments (trim by quality)            */
#define SK_BLK_LEN    4     /* in_len segments (ragged rows); else every row is `stride` long */
#define SK_BLK_DETAIL 8     /* lowest_diff / first_idx / last_idx beside assign   */
typedef struct {
	int32_t n_mates, stride, bc_stride, flags;   /* bc_stride 0 = no barcodes (no demultiplex)                  */
	int32_t in_block, out_block;                 /* bytes per tile of 64 clusters (multiples of 128)            */
	int32_t in_qual[2], in_seq[2], in_len[2], in_bc;
	int32_t out_seq[2], out_lowest_k[2], out_assign, out_lowest_diff, out_first_idx, out_last_idx;
} sk_blocked_layout;
int sk_blocked_layout_init(sk_blocked_layout *lay, int n_mates, int stride, int bc_stride, int flags);
/* in/out: device buffers of ((n+63)/64) * in_block / out_block bytes, 16-byte aligned; counts as in sk_fused_args */
int sk_fused_pass_blocked_dev(sk_ctx *ctx, const sk_blocked_layout *lay, const uint8_t *in, uint8_t *out, int64_t n,
                              uint8_t min_baseq, uint64_t *counts);

/* ---- counters: sample.total_reads[S], total_reads, identified_reads (+ ambiguous) -----------------
 * src/fasta_demultiplex.rs:108-109,169,177-178.  Layout u64[S+3]: per-sample counts, then [S] total,
 * [S+1] identified, [S+2] ambiguous.  These are the only cross-shard state of the path; a multi-GPU
 * host sums them with one all-reduce (sk_counts_device_ptr gives the device buffer to reduce).       */
int sk_counts_reset(sk_ctx *ctx);
int sk_counts_get(sk_ctx *ctx, uint64_t *counts /* host, S+3 */);
/* The ctx's device u64[S+3].  It holds what was enqueued on the ctx BEFORE this call (once the ctx stream has got there):
 * ask again after later demultiplex calls, do not keep the pointer across them.                              */
void *sk_counts_device_ptr(sk_ctx *ctx);

/* ---- (e) multi-GPU: the count reduce over RCCL / xGMI ---------------------------------------------------------
 * Reads shard trivially (every cluster is independent); the additive counters above — and the BAM counters and
 * histogram — are the only state that crosses shards (src/fasta_demultiplex.rs:108-109,169,177-178 are plain `+= 1`
 * on one thread in the reference).  RCCL (librccl.so.1, loaded on first use) sums them; there is no other collective.
 *  - one process driving several GPUs (the C++ hosts): sk_counts_allreduce(ctxs, n) sums the u64[S+3] counters of
 *    all n ctxs in place, so that every ctx ends with the totals.  Ctxs that share a device are summed on that device
 *    first; distinct devices then take part in one ncclAllReduce(ncclSum, ncclUint64) on their ctx streams (a
 *    communicator per device set is created with ncclCommInitAll on first use).  Synchronous when n > 1.
 *  - one process per GPU (bench.py, torchrun): rank 0 calls sk_comm_get_unique_id, the host hands the 128 bytes to
 *    every rank (any side channel), every rank calls sk_comm_init_rank; afterwards sk_counts_allreduce(&ctx, 1) and
 *    sk_allreduce_u64_dev sum across the ranks, enqueued on the ctx stream (asynchronous; sk_sync waits).          */
#define SK_COMM_ID_BYTES 128
/* rank-local, talks to nobody: SK_OK when this ctx could join a communicator (librccl loadable, device bindable).
 * sk_comm_init_rank blocks until every rank has called it, so hosts exchange these answers first and only then join. */
int sk_comm_ready(sk_ctx *ctx);
int sk_comm_get_unique_id(uint8_t id[SK_COMM_ID_BYTES]);
int sk_comm_init_rank(sk_ctx *ctx, const uint8_t id[SK_COMM_ID_BYTES], int rank, int n_ranks);
int sk_comm_destroy(sk_ctx *ctx);
int sk_counts_allreduce(sk_ctx **ctxs, int n_ctx);
/* in-place sum of a device u64 vector over the ranks of sk_comm_init_rank (BAM counters + histogram, or counters
 * a host keeps in its own device buffer); a ctx without a communicator is its own world: nothing to do.           */
int sk_allreduce_u64_dev(sk_ctx *ctx, uint64_t *buf, size_t count);

/* ---- S1 + H1: BAM flag counters and |TLEN| histogram -----------------------------------------------
 * src/sam_statistics.rs:63-69 (counters[0]=total, [1]=aligned, [2]=duplicate) and
 * src/sam_fragment_lengths.rs:29-43 (hist[0..max_frag], *hist_total = records histogrammed).  Inputs
 * are the BAM fixed-core fields as SoA columns (flag@14, refID@0, next_refID@20, tlen@28 of the 32-byte
 * core).  Results are ADDED to the caller's arrays.  The --reads=N early stop (:42) is order dependent
 * and stays on the host.  counters or hist may be NULL to skip that half.  The --on-target fragments
 * (S2, :72-106) do not depend on record order: sk_on_target_add counts them, and these counters too. */
int sk_bam_flag_tlen(sk_ctx *ctx, const uint16_t *flag, const int32_t *tid, const int32_t *mtid,
                     const int32_t *tlen, int64_t n, int32_t max_frag,
                     uint64_t counters[3], uint64_t *hist, uint64_t *hist_total);
/* out = device u64[3 + 1 + (max_frag+1)]: counters, hist_total, hist; ADDED to. */
int sk_bam_flag_tlen_dev(sk_ctx *ctx, const uint16_t *flag, const int32_t *tid, const int32_t *mtid,
                         const int32_t *tlen, int64_t n, int32_t max_frag, uint64_t *out);

/* ---- B1 on the device: BGZF inflate and the BAM record walk ------------------------------------
 * src/common.rs:121-157: the reference reads a BAM through htslib, which inflates every BGZF block (SAMv1 §4.1: a gzip
 * member of at most 64 KiB, self-contained), checks its CRC-32 and walks the records (block_size + 32-byte core + ...).
 * Here the compressed file crosses PCIe and the device does all three.
 *
 * sk_bgzf_inflate_dev: blocks[i] says where block i's raw DEFLATE payload lies in comp (in_off, in_len: what is between
 * the gzip header and the 8-byte trailer), how many bytes it inflates to (out_len = the trailer's ISIZE), where they go
 * in out (out_off) and the trailer's CRC32.  comp must be readable up to the next 4-byte boundary behind the last
 * payload; out 16-byte aligned.  status[i] (device u32): 0 = block i was inflated (and, with check_crc, its CRC
 * matched); 1..8 = the decoder gave the block up (an irregular code, a distance before the block, sizes that do not
 * match: what zlib would call a data error, and a few legal rarities) — nothing is decided here: the caller inflates
 * such a block with zlib, whose verdict stands; bit 8 (0x100) = CRC mismatch.  A block with in_len == 0 is given up
 * too (8), whatever its out_len: no input is no DEFLATE stream.  All pointers are device pointers.
 *
 * sk_bam_walk_dev: stream = the inflated blocks back to back (out above, stream_len bytes, readable 8 bytes beyond),
 * block_end[c] = where block c ends in it (device u64[n], ascending), first_record = where the first record begins
 * (behind the BAM header), n_ref = the header's number of references (or -1: not used by the guesses).  Every block is
 * walked from a guessed entry — its first byte; for the blocks where that is no record's first byte, the first offset at
 * which three records in a row look like records — and the guesses are verified against the predecessors' exits until
 * nothing changes (at most max_rounds rounds).  *verified = 1: entry[c] (device u64[n]) is
 * where the first record that begins in block c begins, for every c — the chain from first_record, proven block by
 * block — and it ends exactly at stream_len; *n_records = records in the stream.  *verified = 0: the stream is not a
 * well-formed sequence of records (or did not settle): the caller's record-at-a-time path reports it as the reference
 * would.  exit_scratch (device u64[n]) and nrec_scratch (device u32[n + 1]) are work space.
 *
 * sk_bam_walk_reduce_dev: S1 + H1 (sk_bam_flag_tlen's predicates) over the records of a verified chain, read straight
 * from the inflated bytes.  out = device u64[3 + 1 + (max_frag + 1)] as sk_bam_flag_tlen_dev, ADDED to.
 *
 * sk_bam_file_reduce: the three above over a whole BAM file: reads it (pread into pinned buffers), ships the compressed
 * bytes, inflates, walks, reduces; blocks the device gave up are inflated with zlib on the host.  counters / hist as
 * sk_bam_flag_tlen (ADDED to; either may be NULL).  *handled = 0 (and nothing added): the file is not one this path
 * serves — not a regular file, not BGZF, cut short, a record chain that does not verify, a block zlib rejects too —
 * and the caller falls back to its record-at-a-time reader, which produces the reference's output and messages.
 * The device and page-locked buffers of a call (the compressed file; for the inflated stream a reserved address range of six
 * times the file's size into which memory is mapped as far as the file inflates) stay with the ctx for the next call;
 * sk_destroy frees them.
 * info (may be NULL): [0] compressed bytes, [1] inflated bytes, [2] BGZF blocks, [3] records, [4] blocks inflated by
 * zlib on the host, [5] walk rounds, [6] ms reading + copying, [7] ms of device work behind the last copy.          */
typedef struct sk_bgzf_block {
	uint64_t in_off;               /* of the DEFLATE payload in comp */
	uint32_t in_len, out_len;
	uint64_t out_off;
	uint32_t crc32, reserved;
} sk_bgzf_block;
int sk_bgzf_inflate_dev(sk_ctx *ctx, const uint8_t *comp, const sk_bgzf_block *blocks, int64_t n_blocks, uint8_t *out,
                        uint32_t *status, int check_crc);
int sk_bam_walk_dev(sk_ctx *ctx, const uint8_t *stream, uint64_t stream_len, const uint64_t *block_end, int64_t n,
                    uint64_t first_record, int32_t n_ref, uint64_t *entry, uint64_t *exit_scratch, uint32_t *nrec_scratch,
                    int max_rounds, int *verified, uint64_t *n_records, int *rounds);
int sk_bam_walk_reduce_dev(sk_ctx *ctx, const uint8_t *stream, uint64_t stream_len, const uint64_t *block_end,
                           const uint64_t *entry, int64_t n, int32_t max_frag, int want_counters, int want_hist, uint64_t *out);
int sk_bam_file_reduce(sk_ctx *ctx, const char *path, int32_t max_frag, uint64_t counters[3], uint64_t *hist,
                       uint64_t *hist_total, int *handled, double info[8]);

/* ---- B1 for the record commands: a BAM file as device SoA columns --------------------------------------------------------
 * sk_bam_file_columns: what sk_bam_file_reduce does up to and including the verified walk (same files served, same knobs
 * SK_BAMFILE_*, same *handled = 0 cases, info[] as there), then the fields `want` names of EVERY record, in file order, into SoA
 * columns on the device: flag, mapq, refID, next_refID, pos, next_pos, tlen of the 32-byte core, and END = cigar end_pos as the
 * reference's reader computes it for src/sam_count.rs:78-94 — pos plus the lengths of the ops M D N = X (codes 0 2 3 7 8) in 64
 * bits, truncated to int32; pos itself when the record's variable part is shorter than its read name and CIGAR.  The columns stay
 * with the ctx, 16-byte aligned (the _dev entries take them as they are), and hold until the next sk_bam_file_* call on the ctx
 * or sk_destroy; a column not asked for is NULL.  header (HOST, also the ctx's) holds the BAM header from "BAM\1" to the end of the
 * reference list (SAMv1 §4.2): the reference names, as src/sam_fragments.rs:22 and src/sam_count.rs:37 take them.  *handled = 0:
 * every case sk_bam_file_reduce leaves to its caller, and also when the device has no room for the columns; cols is then zeroed. */
#define SK_COL_FLAG 1u                 /* uint16 */
#define SK_COL_MAPQ 2u                 /* uint8 */
#define SK_COL_TID  4u                 /* int32 refID */
#define SK_COL_MTID 8u                 /* int32 next_refID */
#define SK_COL_POS  16u                /* int32 */
#define SK_COL_MPOS 32u                /* int32 next_pos */
#define SK_COL_TLEN 64u                /* int32 */
#define SK_COL_END  128u               /* int32 cigar end_pos */
#define SK_COL_ALL  255u
typedef struct sk_bam_columns {
	int64_t n;                         /* records in the file */
	uint16_t *flag;                    /* DEVICE columns of n entries, NULL if not asked for */
	uint8_t *mapq;
	int32_t *tid, *mtid, *pos, *mpos, *tlen, *end_pos;
	const uint8_t *header;             /* HOST: "BAM\1" .. the end of the reference list */
	uint64_t header_len;
	int32_t n_ref;
} sk_bam_columns;
int sk_bam_file_columns(sk_ctx *ctx, const char *path, uint32_t want, sk_bam_columns *cols, int *handled, double info[8]);

/* ---- B1 for `sam to [interleaved] raw|fasta|fastq` (src/sam_to_fastq.rs:61-149) ------------------------
 * sk_bam_file_reads: what sk_bam_file_reduce does up to and including the verified walk (same files, knobs SK_BAMFILE_*, *handled = 0
 * cases, info[] as there), then a device sizing pass over every record.  Records kept: neither 0x100 nor 0x800 (:102), and either
 * not paired (flag & 0x1 == 0; only with want_unpaired) or paired and flagged 0x40 or 0x80 (:114-130).  The text of a kept record is
 * what write_read (:138-149) writes for it — format 0 raw "SEQ\n", 1 fasta ">name\nSEQ\n", 2 fastq "@name\nSEQ\n+\nQUAL\n" — with SEQ
 * = sequence(read, min_baseq) (:31-59) and QUAL = 33 + q in u8 arithmetic, in stored order.  *n_kept, *text_bytes: the kept records
 * and their text.  *handled = 0 also, decided before any text is written, when a primary record's qname has a byte >= 0x80, when in
 * fastq mode a primary record has a quality q with 33 + q >= 0x80, when a primary record has l_seq > 65532, when a record's
 * variable part is shorter than its read name, CIGAR, bases and qualities, and when the device or host memory the call needs cannot
 * be had.  A bad format: SK_ERR_INVALID.  window_bytes (0: 64 MiB) bounds the text + name bytes of one window (a single record may
 * go beyond it).
 * sk_bam_file_reads_next: the next window of kept records, in file order; w->n == 0 at the end.  The window's HOST arrays (the
 * ctx's, page-locked) hold until the next call on the ctx; the device writes and copies the following window while the caller
 * works on this one.  Calling it after another sk_bam_file_* call, or without sk_bam_file_reads: SK_ERR_INVALID.               */
typedef struct sk_bam_reads_window {
	int64_t first, n;              /* kept records first .. first + n - 1 (numbered in file order); n == 0: the end */
	const uint8_t *text;           /* HOST, page-locked: the n records' write_read() texts back to back */
	const uint64_t *text_off;      /* HOST: n + 1 offsets into text */
	const uint8_t *kind;           /* HOST: 0 not paired (flag & 0x1 == 0), 1 first in template, 2 last in template */
	const uint64_t *key;           /* HOST: 64-bit hash of the qname, computed on the device */
	const uint8_t *names;          /* HOST: the qnames (no NUL) back to back ... */
	const uint32_t *name_off;      /* ... n + 1 offsets */
} sk_bam_reads_window;
int sk_bam_file_reads(sk_ctx *ctx, const char *path, int format /* 0 raw, 1 fasta, 2 fastq */, uint8_t min_baseq,
                      int want_unpaired, uint64_t window_bytes /* 0 = default */, int64_t *n_kept, uint64_t *text_bytes,
                      int *handled, double info[8]);
int sk_bam_file_reads_next(sk_ctx *ctx, sk_bam_reads_window *w);

/* ---- `sam to`, the mates paired on the device and the texts in output order (src/sam_to_fastq.rs:100-137) -----------------------
 * sk_bam_file_pairs: what sk_bam_file_reads does up to the kept records (same files, same records kept with want_unpaired =
 * !interleaved, same texts, same *handled = 0 cases), then the loop of :113-137 over them on the device.  Per name, in file order, a
 * first mate (0x40; kind 1) whose name has a pending last mate completes a pair, else it becomes the pending first mate of its name,
 * REPLACING one that is pending (the record replaced is written nowhere); a last mate (0x80 alone; kind 2) mirrors that.  Stream 1 and
 * stream 2 hold the first and the last mate of every pair, the pairs in the order of the records that completed them.  The single
 * stream holds the unpaired records in file order, then the first mates still pending at the end, then the last mates still pending,
 * each in the order their names became pending (the reference's order there is arbitrary).  interleaved != 0: one stream, stream 1,
 * with the two mates of pair p adjacent, the first mate first; unpaired records are not kept and pending ones are written nowhere.
 * counts[8]: pairs, unpaired records kept, first mates pending at the end, last mates pending at the end, paired records replaced
 * while pending, and the text bytes of stream 1, stream 2 and the single stream.  *handled = 0 also, before any text is written, when two different names have one 64-bit key (info[5] = -94; environment
 * SK_PAIR_KEY_BITS = 1..64 cuts the key, for tests), when 2^32 records or more are kept, and when the working memory cannot be had:
 * per kept record 33 B of columns, 12 B of permutation and offsets and 38 B of scratch (the scratch in the compressed file's device
 * buffer where it fits; SK_PAIRS_OWN_MEMORY: never there), and the scratch of the sort and the scans.
 * sk_bam_file_pairs_next: the next window; w->n == 0 at the end.  A window is a range of one stream's records: the windows of stream
 * 1 come first, then stream 2's, then the single stream's, and each stream's windows' bytes back to back are that output.  window_bytes
 * (0: 64 MiB) bounds a window's text (a single record may go beyond it).  The HOST text (the ctx's, page-locked) holds until the next
 * call on the ctx; the device writes and copies the following window while the caller writes this one.  Calling it after another
 * sk_bam_file_* call, or without sk_bam_file_pairs: SK_ERR_INVALID.                                                             */
typedef struct sk_bam_pairs_window {
	int32_t stream;                /* 0 stream 1 (interleaved: both mates), 1 stream 2, 2 the single stream */
	int64_t first, n;              /* the stream's records first .. first + n - 1; n == 0: the end */
	const uint8_t *text;           /* HOST, page-locked: their texts back to back */
	uint64_t bytes;
} sk_bam_pairs_window;
int sk_bam_file_pairs(sk_ctx *ctx, const char *path, int format /* 0 raw, 1 fasta, 2 fastq */, uint8_t min_baseq, int interleaved,
                      uint64_t window_bytes /* 0 = default */, uint64_t counts[8], int *handled, double info[8]);
int sk_bam_file_pairs_next(sk_ctx *ctx, sk_bam_pairs_window *w);

/* ---- `sam to` into three .gz files: the paired texts deflated and framed on the device ------------------------------------------
 * sk_bam_file_pairs_gz: exactly sk_bam_file_pairs with interleaved = 0 — the same records kept, the same three streams in the same
 * order, the same counts[8], the same *handled = 0 cases and info[5] codes (-94 under SK_PAIR_KEY_BITS among them), all taken before
 * any window exists — but a window leaves as complete BGZF members, compressed where its text lies, as sk_bam_file_rewrite's do.  One
 * more *handled = 0 case: the window area (a window's text, 31 B, and with level 1 a deflate slot and its tokens, per block; two packed
 * buffers on the device and two page-locked ones) cannot be had (info[5] = -21).  level as for sk_bam_file_rewrite: 0 stores every
 * member, 1 deflates on the device and stores a member that does not shrink.  A bad format or level: SK_ERR_INVALID.  There is no
 * interleaved form.
 * sk_bam_file_pairs_gz_next: the next window; w->n == 0 at the end.  A window is a rank range of one stream, stream 1's windows first,
 * then stream 2's, then the single stream's; window_bytes (0: 64 MiB) bounds its text (a single record may go beyond it).  The text is
 * cut into blocks of at most SK_DEFLATE_MAX_IN bytes wherever the byte count falls: a record may span members.  The windows of one
 * stream, concatenated, inflate to exactly the bytes sk_bam_file_pairs hands out for that stream.  A stream without records has no
 * window, and no window carries the BGZF EOF block: closing a file is the caller's job.  The HOST bytes (the ctx's, page-locked) hold
 * until the next call on the ctx; the device works on the following window meanwhile.  Calling it after another sk_bam_file_* call, or
 * without sk_bam_file_pairs_gz: SK_ERR_INVALID; so is sk_bam_file_pairs_next after sk_bam_file_pairs_gz.                          */
typedef struct sk_bam_pairs_gz_window {
	int32_t stream;            /* 0 first mates, 1 last mates, 2 the single stream */
	int64_t first, n;          /* the stream's records first .. first + n - 1; n == 0: the end */
	const uint8_t *bgzf;       /* HOST, page-locked: complete BGZF members back to back */
	uint64_t bytes, raw_bytes; /* compressed bytes; the text bytes they inflate to */
} sk_bam_pairs_gz_window;
int sk_bam_file_pairs_gz(sk_ctx *ctx, const char *path, int format, uint8_t min_baseq, int level /* 0 stored, 1 deflate */,
                         uint64_t window_bytes, uint64_t counts[8], int *handled, double info[8]);
int sk_bam_file_pairs_gz_next(sk_ctx *ctx, sk_bam_pairs_gz_window *w);

/* ---- BAM out for `sam trim qnames`, `sam tags from qname`, `sam qname from tags` (src/sam_trim_qnames.rs:20-30,
 * src/sam_tags_from_qname.rs:33-52, src/sam_qname_from_tags.rs:32-41) ------------------------------------------------------
 * sk_bam_file_rewrite: what sk_bam_file_reduce does up to and including the verified walk (same files, knobs SK_BAMFILE_*, *handled = 0
 * cases, info[] as there), then a device pass that rewrites every record and BGZF-compresses the result where it lies.  "qname" is the
 * read name without its final NUL.  op SK_REWRITE_TRIM_QNAMES: a name with a space at index t becomes qname[..t], or qname[..t - 2]
 * when "/1" or "/2" precedes the space.  SK_REWRITE_TAGS_FROM_QNAME: the name is split on every ' ', the first part stays the name,
 * each further part "UMI:v" appends RX:Z:v and "XY:v" appends XY:Z:v at the end of the aux data.  SK_REWRITE_QNAME_FROM_TAGS: when
 * the first RX field has type Z or H, the name becomes qname + " RX:" + its value (the field stays).  A changed record gets
 * l_read_name = its name + 1 and block_size to match, every other byte as it was; the other records pass byte for byte.  The header:
 * the text up to its first NUL with trailing '\n's stripped and one '\n' appended when not empty, the reference list as read (htslib's
 * Header::from_template would rebuild that list from the @SQ lines; this keeps the binary list).
 * *handled = 0 also, decided before any window exists, when a record would end the reference's loop (trim: a space at index 0 or 1;
 * tags from qname: a part that is neither "UMI:.." nor "XY:.."; qname from tags: a new name of more than 254 bytes, or aux data that
 * do not parse to the record's end), when a record's variable part is shorter than its fields, and when the device or page-locked
 * memory the call needs cannot be had.  A bad op or level: SK_ERR_INVALID.  level 0: every member is a stored block; 1: deflated on
 * the device (a block that does not shrink is stored).  window_bytes (0: 64 MiB) bounds the rewritten bytes of one window (a single
 * record may go beyond it).  *n_records: the records; *raw_bytes: the whole output BAM, inflated.
 * sk_bam_file_rewrite_next: the next window, in file order: first the header's members (n == 0, bytes > 0), then the records', the
 * last window ending with the 28-byte BGZF EOF block; n == 0 && bytes == 0 at the end.  Concatenated, the windows' bytes are the
 * output file.  The HOST bytes (the ctx's, page-locked) hold until the next call on the ctx; the device rewrites and compresses the
 * following window while the caller writes this one.  Calling it after another sk_bam_file_* call, or without
 * sk_bam_file_rewrite (or sk_bam_file_minimize, sk_bam_file_markdup, sk_bam_file_subsample, sk_bam_file_recalc_tlen, sk_bam_file_merge or sk_bam_file_concatenate, below, whose windows it hands out too; the last of them decides by its flags whether there is a header window and an EOF block):
 * SK_ERR_INVALID.                                                                                                                 */
#define SK_REWRITE_TRIM_QNAMES     1
#define SK_REWRITE_QNAME_FROM_TAGS 2
#define SK_REWRITE_TAGS_FROM_QNAME 3
typedef struct sk_bam_out_window {
	int64_t first, n;          /* records first .. first + n - 1; n == 0 && bytes == 0: the end */
	const uint8_t *bgzf;       /* HOST, page-locked: complete BGZF members back to back */
	uint64_t bytes, raw_bytes; /* compressed bytes; the BAM bytes they inflate to */
} sk_bam_out_window;
int sk_bam_file_rewrite(sk_ctx *ctx, const char *path, int op, int level /* 0 stored, 1 deflate */, uint64_t window_bytes /* 0 = default */,
                        int64_t *n_records, uint64_t *raw_bytes, int *handled, double info[8]);
int sk_bam_file_rewrite_next(sk_ctx *ctx, sk_bam_out_window *w);

/* ---- BAM out for `sam minimize` (src/sam_minimize.rs:46-82) -----------------------------------------------------------------
 * sk_bam_file_minimize: sk_bam_file_rewrite's front half, window pipeline and header, with the record rewrite of `sam minimize`.
 * flags: SK_MINIMIZE_READ_IDS | SK_MINIMIZE_BASE_QUALITIES | SK_MINIMIZE_TAGS.  READ_IDS: a read's key is its qname up to the first
 * '/' (a '/' at index 0: the empty key); in file order the 1st, 3rd, 5th .. record of a key takes the next unused number, starting
 * at 1, and the 2nd, 4th .. takes the number of the record of that key just before it (the reference's map, whose entry is removed
 * when the mate arrives); the new name is that number in decimal.  READ_IDS alone: the name, l_read_name and block_size change and
 * every other byte stays, aux data included (set_qname).  With TAGS (Record::set): the record ends behind its qualities — no aux data
 * — and for an odd l_seq the unused low nibble of the last base byte is 0; bin, mapq, flag and the mate fields stay, and without
 * READ_IDS so does the name.  With BASE_QUALITIES the qualities are l_seq copies of baseq_fill.  *handled = 0 (info[5] = -(30 +
 * bits)) leaves the file to the caller's reader: bit 8 an invalid record, 32 a CIGAR operation code above 8 (the reference panics
 * there), 64 two different keys with one 64-bit hash (verified byte for byte, never guessed); info[5] = -21: 2^32 records or more, or
 * the working memory (about 24 B per record for the ids, 16 for the offsets) cannot be had.  flags == 0, unknown bits, BASE_QUALITIES
 * without TAGS, or a bad level: SK_ERR_INVALID.  level, window_bytes, *n_records, *raw_bytes: as sk_bam_file_rewrite.  The windows come
 * from sk_bam_file_rewrite_next under its rules.  SK_MINIMIZE_KEY_BITS=k (1 .. 64, read per call) keeps only the low k bits of the
 * hash: a knob for tests of the collision check, of no other use.                                                               */
#define SK_MINIMIZE_READ_IDS       1
#define SK_MINIMIZE_BASE_QUALITIES 2
#define SK_MINIMIZE_TAGS           4
int sk_bam_file_minimize(sk_ctx *ctx, const char *path, int flags, uint8_t baseq_fill, int level /* 0 stored, 1 deflate */,
                         uint64_t window_bytes /* 0 = default */, int64_t *n_records, uint64_t *raw_bytes, int *handled, double info[8]);

/* ---- BAM out for `sam mark duplicates` (src/sam_mark_duplicates.rs:46-167) ---------------------------------------------------
 * sk_bam_file_markdup: sk_bam_file_rewrite's front half, window pipeline and header; every record passes byte for byte except bit
 * 0x400 of its flag.  A mapped read's signature: start_pos = pos, or for a reverse read (0x10) cigar end_pos as SK_COL_END; strand;
 * the UMI = the value of its first RX field when that has type Z or H and ignore_umi == 0, else empty; fraglen = min(|tlen|, 65535)
 * when the UMI is empty, else 0.  A group is the mapped reads of one run of equal refID in file order with one start_pos and strand.
 * Per group, in file order, the first read not yet in a cluster is a seed, and every later such read joins it whose fraglen equals
 * the seed's or either is 0, and whose UMI has the seed's length with at most one position where the bytes differ and neither is
 * 'N', or either is empty (compatible with the SEED: not transitive).  Every read of a cluster gets 0x400 except the one with the
 * largest l_seq, the earliest on a tie, which loses it.  Unmapped reads (0x4) keep their flag.  That is what the reference's FIFO
 * loop writes for a file it accepts as sorted whose mapped reads have 0 <= pos and end_pos <= INT32_MAX.  *n_duplicates: the
 * output records that carry 0x400.  *handled = 0 (info[5] = -(30 + bits)) leaves the file to the caller's reader, nothing written:
 * bit 1 a record with 0x100 or 0x800, 2 a record whose refID equals its predecessor's and whose (uint32) pos is below its
 * predecessor's, 4 a mapped read with pos < 0 or a reverse one with end_pos > INT32_MAX, 8 a record whose variable part is shorter
 * than its fields, 16 aux data that do not parse up to the first RX field or the record's end, 32 a CIGAR operation code above 8 on
 * a mapped reverse read (the reference panics there), 64 2^31 - 1 or more refID runs; info[5] = -21: 2^32 records or more, or the
 * working memory cannot be had: 18 B per record, and 44 B per record more with the sort's scratch where those do not fit into the
 * device buffer of the compressed file, which is idle by then and serves as scratch (SK_MARKDUP_OWN_MEMORY set: never there; for
 * tests).  A bad level: SK_ERR_INVALID.  level, window_bytes, *n_records, *raw_bytes: as sk_bam_file_rewrite.  The windows come from
 * sk_bam_file_rewrite_next under its rules.                                                                                      */
int sk_bam_file_markdup(sk_ctx *ctx, const char *path, int ignore_umi, int level /* 0 stored, 1 deflate */, uint64_t window_bytes /* 0 = default */,
                        int64_t *n_records, int64_t *n_duplicates, uint64_t *raw_bytes, int *handled, double info[8]);

/* ---- BAM out for `sam subsample` (src/sam_subsample.rs:30-62) ----------------------------------------------------------------
 * sk_subsample_keep: the fate of draw number `draw` (1, 2, 3 ..) under `seed`, host code that needs no device: with all arithmetic mod
 * 2^64, z = seed + draw * 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >>
 * 31 (splitmix64's draw-th output from state seed); m = z >> 40; 1 (keep) iff m <= floor(fraction * 2^24), else 0.  In integers that is
 * rand 0.5's random::<f32>() <= fraction with random::<f32>() = (u32 >> 8) * 2^-24.  A fraction outside [0, 1] or NaN: SK_ERR_INVALID.
 * sk_bam_file_subsample: sk_bam_file_rewrite's front half, window pipeline and header; a record is written byte for byte or not at all.
 * A record with 0x800 is passed over: not counted, not written.  Every other record is counted, and its key is its qname; in file order
 * the 1st, 3rd, 5th .. counted record of a key makes the next draw, starting at 1, and the 2nd, 4th .. takes the decision of the counted
 * record of that key just before it (the reference's map, whose entry is removed when the mate arrives).  *n_records: the records
 * written; *n_total: the records counted; *raw_bytes: the whole output BAM, inflated.  The windows come from sk_bam_file_rewrite_next
 * under its rules, first and n numbering the records WRITTEN; a file none of whose records is written yields, as a file without
 * records does there, one window: the header's members and the EOF block.  *handled = 0 (info[5] = -(30 + bits)) leaves the file to the caller's reader, nothing
 * written: bit 1 a counted record without 0x1 (the reference ends there), 8 a record whose variable part is shorter than its fields, 64
 * two different keys with one hash (verified byte for byte, never guessed); info[5] = -21: 2^32 records or more, or the working memory
 * (16 B per record for the offsets; 32 B per record and the sort's scratch for the passes where those do not fit into the device buffer
 * of the compressed file, which is idle by then) cannot be had.  A fraction outside [0, 1] or NaN, or a bad
 * level: SK_ERR_INVALID.  level, window_bytes: as sk_bam_file_rewrite.  SK_SUBSAMPLE_KEY_BITS=k (1 .. 64, read per call) keeps only the
 * low k bits of the hash (at most 63: the bit above them marks a record with 0x800): a knob for tests of the collision check, of no
 * other use.                                                                                                                      */
int sk_subsample_keep(uint64_t seed, uint64_t draw, float fraction);
int sk_bam_file_subsample(sk_ctx *ctx, const char *path, float fraction, uint64_t seed, int level /* 0 stored, 1 deflate */,
                          uint64_t window_bytes /* 0 = default */, int64_t *n_records, int64_t *n_total, uint64_t *raw_bytes, int *handled,
                          double info[8]);

/* ---- BAM out for `sam recalculate tlen` (src/sam_recalculate_tlen.rs:42-111) ----------------------------------------------------
 * sk_bam_file_recalc_tlen: sk_bam_file_rewrite's front half, window pipeline and header; a record is written byte for byte except its
 * TLEN (the 4 bytes at record offset 32), or not at all.  A record is a candidate iff it is paired (0x1), mapped and its mate mapped
 * (neither 0x4 nor 0x8), refID == next refID, |pos - next pos| <= max_len (in 64 bits) and bits 0x10 and 0x20 differ; every other
 * record is written with TLEN 0.  The candidates' key is the qname; in file order the 1st, 3rd, 5th .. candidate of a key waits, and
 * the 2nd, 4th .. is the mate of the one just before it (the reference's map, whose entry is removed when the mate arrives).  For a
 * pair, earlier record a and later b, all in 64 bits: start(x) = pos, or for a reverse read (0x10) the CIGAR's end_pos as SK_COL_END
 * less 1; t = |start(b) - start(a)| + 1, negated when pos(b) > pos(a), and 0 when start(b) < start(a) and b is reverse or start(b) >
 * start(a) and b is not; b gets the low 32 bits of t, a those of -t.  A candidate still waiting at the end is discarded: not written.
 * *n_records: the records written; *n_discarded: those discarded; *raw_bytes: the whole output BAM, inflated.  The windows come from
 * sk_bam_file_rewrite_next under its rules, first and n numbering the records WRITTEN; a file none of whose records is written yields,
 * as a file without records does there, one window: the header's members and the EOF block.
 * sk_bam_file_recalc_tlen_discarded: the names of discarded records first .. first + n - 1, in file order, into n slots of 256 bytes,
 * each the qname and NULs up to the slot's end.  Valid from sk_bam_file_recalc_tlen's return (*handled = 1) until the next
 * sk_bam_file_* call on the ctx other than sk_bam_file_rewrite_next, after the last window too; a range outside [0, *n_discarded], or
 * no such call to ask: SK_ERR_INVALID.
 * *handled = 0 (info[5] = -(30 + bits)) leaves the file to the caller's reader, nothing written: bit 1 a paired, mapped record with a
 * mapped mate and 0x100 or 0x800 (the reference ends there), 2 a pair whose records have equal 0x40 bits (the reference's assert), 8 a
 * record whose variable part is shorter than its fields, 16 a qname byte >= 0x80 on any record (the reference panics on a name that is
 * not UTF-8: the caller's reader decides exactly) or a NUL inside a qname (a slot could not say where it ends), 32 a CIGAR operation code above 8 on a reverse candidate (the reference panics
 * there if the record ends up in a pair: the caller's reader decides exactly), 64 two different keys with one hash (verified byte for
 * byte, never guessed; records linked under such a hash may add 2 or 32); info[5] = -21: 2^32 records or more, or the working memory
 * cannot be had: 16 B per record for the offsets, 8 B
 * per record and 1 MiB at most for the TLENs, the discard list and its name slots, and 32 B per record and the sort's scratch for the
 * passes where those do not fit into the device buffer of the compressed file, which is idle by then (SK_TLEN_OWN_MEMORY set: never
 * there; for tests).  max_len <= 0 or a bad level: SK_ERR_INVALID.  level, window_bytes: as sk_bam_file_rewrite.  SK_TLEN_KEY_BITS=k
 * (1 .. 63, read per call) keeps only the low k bits of the hash: a knob for tests of the collision check, of no other use.       */
int sk_bam_file_recalc_tlen(sk_ctx *ctx, const char *path, int64_t max_len, int level /* 0 stored, 1 deflate */,
                            uint64_t window_bytes /* 0 = default */, int64_t *n_records, int64_t *n_discarded, uint64_t *raw_bytes,
                            int *handled, double info[8]);
int sk_bam_file_recalc_tlen_discarded(sk_ctx *ctx, int64_t first, int64_t n, uint8_t *names /* HOST: n slots of 256 bytes */);

/* ---- BAM out for `sam merge` (src/sam_merge.rs:58-103) -----------------------------------------------------------------------
 * sk_bam_file_merge: sk_bam_file_rewrite's front half for each of n_paths files (2 .. 99), its window pipeline and header (input 1's).
 * A record's key is (uint32) refID, then pos as a signed 32-bit value: refID -1 sorts last, pos -1 before 0.  The output is what this
 * loop writes: among the inputs' current first records take the smallest key, among equal keys the lowest input; write it; advance that
 * input.  For inputs each sorted by the key that is the stable merge, and the reference's output byte for byte whenever no two records of
 * different inputs share a key (there its heap decides, here the command line's order).  suffix != 0: '.' and the decimal 1-based input
 * number are appended to every record's name, l_read_name and block_size grow by those 2 or 3 bytes, every other byte as it was;
 * suffix == 0: every record byte for byte.  The inputs' streams stay on the device together until the last window is written: input 1's
 * with ctx, each further one's with a helper context that ctx keeps and sk_destroy frees.  *n_records: the records of all inputs;
 * *raw_bytes: the whole output BAM, inflated.  The windows come from sk_bam_file_rewrite_next under its rules.  *handled = 0 leaves the
 * files to the caller's reader, nothing written: info[5] = -(30 + bits) with bit 1 a suffixed name of more than 254 bytes (the reference
 * panics there), 2 an input with a key below its predecessor's, 4 an input whose reference names differ from input 1's (lengths are not
 * compared), 8 a record whose variable part is shorter than its fields; info[5] = -21: more than 99 inputs, 2^32 records or more, or the
 * working memory cannot be had (17 B per record for the offsets and input numbers; 29 B per record and the sort's scratch for the passes
 * where those do not fit into the device buffer of input 1's compressed file, which is idle by then); any other negative info[5]: the
 * check at which the front half left one of the files.  n_paths < 2, a NULL path or a bad level: SK_ERR_INVALID.  level, window_bytes:
 * as sk_bam_file_rewrite.                                                                                                         */
int sk_bam_file_merge(sk_ctx *ctx, const char *const *paths, int n_paths, int suffix, int level /* 0 stored, 1 deflate */,
                      uint64_t window_bytes /* 0 = default */, int64_t *n_records, uint64_t *raw_bytes, int *handled, double info[8]);

/* ---- BAM out for `sam concatenate` (src/sam_concatenate.rs:35-49) ------------------------------------------------------------
 * sk_bam_file_concatenate: ONE input of the command — sk_bam_file_rewrite's front half and window pipeline over the file at path, every
 * record in file order with '.' and the decimal digits of number (1 .. 4294967295: 2 .. 11 bytes) appended to its name, l_read_name and
 * block_size grown by those bytes, every other byte as it was (refID and next refID too: nothing is remapped).  The caller chains the
 * inputs, one call each with number = 1, 2, ..; the ctx holds one input's streams at a time.  flags: with SK_CONCAT_HEADER the windows
 * begin with this file's output header (sk_bam_file_rewrite's rule) in members of its own, without it no header window is issued; with
 * SK_CONCAT_EOF the last window ends with the 28-byte BGZF EOF block, without it none does.  An input without records and with
 * flags == 0 has no window at all (the first sk_bam_file_rewrite_next returns the end); with SK_CONCAT_EOF alone it has one window of
 * n == 0, bytes == 28.  *n_records: the file's records; *raw_bytes: what this call's members inflate to (the header when asked for, and
 * the records).  The windows come from sk_bam_file_rewrite_next under its rules.  *handled = 0 leaves the file to the caller's reader,
 * nothing written: info[5] = -(30 + bits) with bit 1 a suffixed name of more than 254 bytes (the reference panics there), 8 a record
 * whose variable part is shorter than its fields; info[5] = -21: the working memory cannot be had (16 B per record for the offsets and
 * the scan's scratch where that does not fit into the device buffer of the compressed file, idle by then); any other negative info[5]:
 * the check at which the front half left the file.  number == 0, flags outside 0 .. 3 or a bad level: SK_ERR_INVALID.  level,
 * window_bytes: as sk_bam_file_rewrite.                                                                                            */
#define SK_CONCAT_HEADER 1   /* the windows begin with this file's output header in members of its own */
#define SK_CONCAT_EOF    2   /* the last window ends with the 28-byte BGZF EOF block */
int sk_bam_file_concatenate(sk_ctx *ctx, const char *path, uint32_t number, int flags, int level /* 0 stored, 1 deflate */,
                            uint64_t window_bytes /* 0 = default */, int64_t *n_records, uint64_t *raw_bytes, int *handled, double info[8]);

/* ---- BAM out for `sam discard tail artifacts` (src/sam_discard_tail_artifacts.rs:129-226, :243-348; src/genome_reader.rs) ---------
 * sk_bam_file_discard_tails: sk_bam_file_subsample's front half, window pipeline and header, the header's text followed by the co_bytes
 * bytes at co_line (whole lines; l_text says so); a record is written byte for byte or not at all.  The genome is the FASTA file at
 * fasta_path as its index describes it: n_refs entries (names[i], refs[i]), one per line of the caller's .fai, matched to the BAM
 * header's reference names here (of two entries with one name the later counts).  Base p of a chromosome is the file's byte file_offset
 * + p / line_bases * line_width + p % line_bases.  The library reads the file itself, only the spans of the chromosomes that mapped
 * records name, into device memory that it frees before it returns.  An unmapped record (0x4) is written, whatever its refID.  A
 * mapped record is walked from both ends as count_mismatches does: left from base 0 with ref_offset = pos over its operations in
 * order, right from base l_seq - 1 with ref_offset = pos + (the D lengths less the I lengths of the whole CIGAR) over them in reverse;
 * an operation reached when tail_length bases have been examined ends the walk; M = X examine their bases one by one (read base A C G T
 * for codes 1 2 4 8, else N; the chromosome's byte at ref_offset + base index, ASCII-upper-cased; a mismatch unless they are equal or
 * either is N), I counts one mismatch and moves the base index by its length and ref_offset against it, D counts one and moves
 * ref_offset.  The record is failed, and not written, iff either count >= min_mismatches (the caller's check_threshold(tail_length,
 * ratio); UINT32_MAX fails none).  *n_records: the records written; *n_total: all records; *n_failed, *n_passed: the mapped records
 * failed and passed; *n_loads: the chromosome loads of the reference's loop after its first — the mapped records whose refID differs
 * from the mapped record's before them, from 0 for the first; *raw_bytes: the whole output BAM, inflated.  The windows come from
 * sk_bam_file_rewrite_next under its rules, first and n numbering the records WRITTEN.
 * sk_bam_file_discard_tails_loads: the refIDs of loads first .. first + n - 1, in file order.  Valid from
 * sk_bam_file_discard_tails's return (*handled = 1) until the next sk_bam_file_* call on the ctx other than sk_bam_file_rewrite_next,
 * after the last window too; a range outside [0, *n_loads], or no such call to ask: SK_ERR_INVALID.
 * *handled = 0 (info[5] = -(30 + bits)) leaves the file to the caller's reader, nothing written: bit 1 a mapped record with an
 * operation outside M I D = X anywhere in its CIGAR (the reference panics where a walk reaches one: the caller's reader decides
 * exactly), 2 an examined base whose read index lies outside [0, l_seq) or whose reference index lies outside the chromosome, 4 a
 * header without references, a reference 0 or a mapped record's refID without a chromosome (outside the header, no entry of its name,
 * or a span that ends beyond the file), 8 a record whose variable part is shorter than its fields, 16 a value the reference holds in an
 * i32 outside that range (pos + the CIGAR's shift, a base index or ref_offset behind an I or D); info[5] = -21: 2^31 records or more
 * (the reference's counters are i32), or memory cannot be had: the chromosomes' spans, 16 B per record for the offsets, 4 B per record
 * for the loads, and 32 B per record, 36 B per reference and the scans' scratch for the passes where those do not fit into the device
 * buffer of the compressed file, which is idle by then (SK_TAILS_OWN_MEMORY set: never there; for tests).  tail_length == 0, a NULL
 * fasta_path or name, an entry with line_bases == 0 or line_width < line_bases, or a bad level: SK_ERR_INVALID.  level, window_bytes:
 * as sk_bam_file_rewrite.                                                                                                          */
typedef struct sk_genome_ref {     /* one line of a .fai behind its name */
	uint64_t file_offset, length;  /* the first base's byte in the FASTA file; the chromosome's bases */
	uint64_t line_bases, line_width;
} sk_genome_ref;
int sk_bam_file_discard_tails(sk_ctx *ctx, const char *path, const char *fasta_path, const char *const *names, const sk_genome_ref *refs,
                              int32_t n_refs, uint32_t tail_length, uint32_t min_mismatches, const uint8_t *co_line, uint32_t co_bytes,
                              int level /* 0 stored, 1 deflate */, uint64_t window_bytes /* 0 = default */, int64_t *n_records, int64_t *n_total,
                              int64_t *n_failed, int64_t *n_passed, int64_t *n_loads, uint64_t *raw_bytes, int *handled, double info[8]);
int sk_bam_file_discard_tails_loads(sk_ctx *ctx, int64_t first, int64_t n, int32_t *tids /* HOST */);

/* ---- `sam coverage histogram` (src/sam_coverage_histogram.rs; this build's reading of `samtools depth -a`) --------
 * sk_bam_file_coverage: what sk_bam_file_reduce does up to and including the verified walk (same files, knobs SK_BAMFILE_*, *handled = 0
 * cases, info[] as there), then the depth histogram of the target positions, from sorted CIGAR events on the device.  A record is
 * counted iff 0 <= refID < n_ref and flag & 0x704 == 0 (0x800 is counted; mapq and the qualities play no part; overlapping mates
 * each count).  From pos, its CIGAR's M = X ops (codes 0 7 8) cover [p, p + len) and advance, D N (2 3) advance, every other code
 * does neither, in 64 bits; what falls outside [0, l_ref) is dropped (l_ref read unsigned).  The order of the records plays no part.
 * Target positions: mode 0, every position of every reference with a counted record (targets ignored).  Mode 1, the union of the
 * `targets`, whether or not a record lies there.  Mode 2, the union of the `targets` on the references that have a counted record
 * whose span [pos, end) overlaps one of them; end = pos plus the lengths of the ops M D N = X, pos + 1 without one.  targets: n_targets
 * host triples (refID, beg, end), 0-based half-open, in any order, overlapping allowed; a refID outside the header or beg >= end is
 * ignored, beg < 0 reads as 0, and the interval is cut to [0, l_ref) as a target (not for mode 2's overlap test).
 * hist[k], k in 0 .. SK_COVERAGE_BINS - 1 = the target positions of depth k (set, not added to); *n_dropped = those deeper, which no
 * bin counts; *n_positions = the target positions = sum(hist) + *n_dropped; *n_counted = the counted records.  *handled = 0
 * (info[5] = -(30 + 8)): a record whose variable part is shorter than its fields; info[5] = -21: 2^32 events or more (two per run of
 * covering ops and per target interval), or the working memory (24 B per event and the sort's scratch, in the device buffer of the
 * compressed file where they fit: it is idle by then) cannot be had.  A bad mode, n_targets < 0 or hist == NULL: SK_ERR_INVALID.       */
#define SK_COVERAGE_BINS 10001
int sk_bam_file_coverage(sk_ctx *ctx, const char *path, int mode /* 0 everywhere, 1 region, 2 BED */, const int64_t *targets, int64_t n_targets,
                         uint64_t hist[SK_COVERAGE_BINS], uint64_t *n_positions, uint64_t *n_dropped, int64_t *n_counted, int *handled,
                         double info[8]);

/* ---- F2 on the device: the gzip writers' DEFLATE ------------------------------------------------
 * src/common.rs:49-81: every output file of the reference is a pipe into a gzip / pigz child; what a test can hold it to is
 * the decompressed stream.  sk_bgzf_deflate compresses n independent blocks of at most SK_DEFLATE_MAX_IN bytes (in +
 * blocks[i].in_off, in_len bytes; host pointers) into n complete BGZF members (SAMv1 §4.1: gzip members with the BC
 * subfield, CRC32 and ISIZE) written back to back into out: member i is out[out_off[i] .. out_off[i + 1]).  The device
 * finds the matches (a hash of four bytes, greedy), builds a Huffman code per block and writes the bits; a block that does
 * not shrink is framed as a stored block.  out_cap >= n * SK_DEFLATE_MAX_MEMBER always suffices.  in must be readable to the
 * next 4-byte boundary behind its last byte.
 * sk_bgzf_deflate_dev is the device half alone: slots[i * slot_stride ..] receives block i's DEFLATE payload (slot_stride
 * >= SK_DEFLATE_SLOT, a multiple of 4), result[2 i] its byte count, crc[i] the CRC-32 of the block's input; tokens is
 * scratch of n * SK_DEFLATE_MAX_IN dwords.  All pointers device pointers.                                             */
#define SK_DEFLATE_MAX_IN     0xff00
#define SK_DEFLATE_MAX_MEMBER 65536
#define SK_DEFLATE_SLOT       81920
typedef struct sk_deflate_block {
	uint64_t in_off;
	uint32_t in_len, reserved;
} sk_deflate_block;
int sk_bgzf_deflate(sk_ctx *ctx, const uint8_t *in, size_t in_bytes, const sk_deflate_block *blocks, int64_t n_blocks,
                    uint8_t *out, size_t out_cap, uint64_t *out_off);
int sk_bgzf_deflate_dev(sk_ctx *ctx, const uint8_t *in, const sk_deflate_block *blocks, int64_t n_blocks, uint8_t *slots,
                        uint32_t slot_stride, uint32_t *tokens, uint32_t *result, uint32_t *crc);

/* ---- f2: `sam fragments` record filter ---------------------------------------------------------------------
 * src/sam_fragments.rs:27-38: keep the forward mate of a converging, mapped, primary, non-duplicate, QC-passing pair on
 * one reference whose |tlen| lies in [min_size, max_size].  keep_bits: (n+7)/8 bytes, bit j of byte k <=> record 8k+j;
 * *kept is ADDED to.  The BED line of a kept record (:41): sk_bam_fragments_bed_dev.  Columns must be 16-byte
 * aligned for the _dev form.                                                                                */
int sk_bam_fragments(sk_ctx *ctx, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                     int64_t n, int64_t min_size, int64_t max_size, uint8_t *keep_bits, uint64_t *kept);
int sk_bam_fragments_dev(sk_ctx *ctx, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                         int64_t n, int64_t min_size, int64_t max_size, uint8_t *keep_bits, uint64_t *kept);
/* The BED lines of the kept records (src/sam_fragments.rs:41: chr_names[tid] \t pos \t pos + |tlen| \n, the numbers signed
 * 64-bit decimal), written on the device in record order.  keep_bits as sk_bam_fragments_dev writes them; tid, pos, tlen device
 * columns of n records (16-byte aligned).  names: the n_ref reference names back to back (HOST), name r = names[name_off[r] ..
 * name_off[r + 1]) copied verbatim.  Synchronous: *text points at *text_len bytes of page-locked HOST memory that stays with the
 * ctx until the next call.  *bad = index of the first kept record whose tid is not in [0, n_ref) — where the reference panics —
 * and *text then holds the lines before it; -1 when there is none.                                                         */
int sk_bam_fragments_bed_dev(sk_ctx *ctx, const uint8_t *keep_bits, const int32_t *tid, const int32_t *pos, const int32_t *tlen,
                             int64_t n, const uint8_t *names, const uint64_t *name_off, int32_t n_ref, const char **text,
                             uint64_t *text_len, int64_t *bad);

/* ---- f2 (second half): `sam count` ---------------------------------------------------------------------------
 * src/sam_count.rs:44-127.  sk_count_set_regions loads the BED regions grouped by BAM reference: regions of
 * reference c are entries chr_off[c] .. chr_off[c+1]-1 of rstart/rend (0-based half-open, any order inside a
 * group; they are sorted by start here, as :63 does) and ridx gives each entry's index in the caller's list of
 * n_regions regions (n_entries <= n_regions: regions on chromosomes the BAM does not have are simply not entered);
 * the n_regions counters (u32, like the reference's) are cleared.  sk_count_add runs, for every record, the filter
 * chain (:46-50, :78-94), the fragment interval in the reference's u32 arithmetic (:75,97-107) and adds 1 to every
 * region of the record's reference that the interval overlaps (:122-126).  Columns: flag, mapq, refID, next_refID,
 * pos, next_pos, tlen of the BAM core and, for single_end only, cigar end_pos (NULL otherwise).  What depends on
 * record order — the "not coordinate sorted" error (:70-72) and chr_names[tid] (:55) — is sk_count_order_check_dev's.  The counts
 * do not depend on the order of the records; the speed does: the region search of a record starts from its
 * predecessor's answer, which is two probes in a coordinate-sorted batch and more than a plain search otherwise.      */
int sk_count_set_regions(sk_ctx *ctx, int n_chr, const int32_t *chr_off, const uint32_t *rstart, const uint32_t *rend,
                         const int32_t *ridx /* NULL = 0,1,2,... */, int64_t n_entries, int64_t n_regions);
int sk_count_add(sk_ctx *ctx, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mtid,
                 const int32_t *pos, const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n,
                 uint8_t min_mapq, uint32_t max_frag_len, int single_end, int center);
int sk_count_add_dev(sk_ctx *ctx, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *mtid,
                     const int32_t *pos, const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n,
                     uint8_t min_mapq, uint32_t max_frag_len, int single_end, int center);
int sk_count_get(sk_ctx *ctx, uint32_t *region_frags /* n_regions */);
/* The order checks of src/sam_count.rs:52-73 over device columns of n records, in file order: among the records the filter of
 * :46-49 passes (none of 0x4 0x400 0x100 0x800, mapq >= min_mapq), starting from prev_chr = -1, prev_pos = 0, a record whose tid
 * differs from prev_chr and is not in [0, n_ref) panics (:55), a record on the same tid with pos < prev_pos ends the command ("not
 * coordinate sorted", :70-72); every passing record sets prev_chr and prev_pos.  Synchronous: *first_stop = index of the first
 * record where that loop stops, -1 if it runs through; *code = 101 (the tid) or 255 (the order), 0 for -1.  Columns 16-byte
 * aligned.                                                                                                                      */
int sk_count_order_check_dev(sk_ctx *ctx, const uint16_t *flag, const uint8_t *mapq, const int32_t *tid, const int32_t *pos, int64_t n,
                             uint8_t min_mapq, int32_t n_ref, int64_t *first_stop, int *code);

/* ---- S2: `sam statistics --on-target=BED` ------------------------------------------------------------------------
 * src/sam_statistics.rs:63-106.  sk_on_target_set_regions loads the target regions grouped by BAM reference: regions of
 * reference c are entries chr_off[c] .. chr_off[c+1]-1 of rstart/rend, 1-based inclusive in 64 bits as :44-47 keep them
 * (start = BED column 2 + 1, end = BED column 3; end < start is taken as it is), in any order inside a group: they are
 * sorted by start here (:51-53) and the running maximum of their ends is put beside them.  n_entries == 0 and references
 * without a region are valid.  The six counters are cleared.  sk_on_target_add runs, for every record, S1 (:64-69, the
 * predicates of sk_bam_flag_tlen) and S2: for a record that is neither secondary, supplementary nor unmapped — paired
 * (0x1): dropped when the mate is unmapped (0x8), tid != next_refID, pos > next_pos, pos == next_pos without 0x40, or
 * |tlen| > max_frag_len (:76-84), else start = pos + 1, end = start + |tlen| (:86-87); unpaired: start = pos + 1, end =
 * cigar end_pos + 1 (:90-91); all in 64 bits.  Every such record is a fragment (:94), and an on-target one when a region
 * of its reference has start <= r.end && end >= r.start.  The reference's walk over the sorted regions (:97-106) stops at
 * the first hit and at the first region that starts behind `end`; with k = the regions with r.start <= end that is
 * k > 0 && max(r.end of regions 0 .. k-1) >= start: one binary search, whatever the order of the records.  A fragment
 * whose tid is not in [0, n_chr) — where the reference panics (:97) — is counted in out[5] and not looked up.
 * Columns: flag, refID, next_refID, pos, next_pos, tlen of the BAM core and cigar end_pos (SK_COL_END); host columns of
 * any alignment for sk_on_target_add, device columns of any alignment (16-byte aligned ones are read with wide loads)
 * for the _dev form, which is asynchronous on the ctx stream.  Calls accumulate.  sk_on_target_get (synchronous):
 * out = total_reads, aligned_reads, duplicate_reads, total_fragments, on_target_fragments, bad_tid_fragments.          */
int sk_on_target_set_regions(sk_ctx *ctx, int n_chr, const int32_t *chr_off, const int64_t *rstart, const int64_t *rend,
                             int64_t n_entries);
int sk_on_target_add(sk_ctx *ctx, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *pos,
                     const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n, int64_t max_frag_len);
int sk_on_target_add_dev(sk_ctx *ctx, const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *pos,
                         const int32_t *mpos, const int32_t *tlen, const int32_t *end_pos, int64_t n, int64_t max_frag_len);
int sk_on_target_get(sk_ctx *ctx, uint64_t out[6]);

/* ---- `fasta gc content` ------------------------------------------------------------------------------------------
 * src/fasta_gc_content.rs:41-46.  sk_gc_set_genome copies the concatenated sequences to the device once (it stays
 * there until the next call or sk_destroy); sk_gc_count then returns, for region i = bytes [start[i], start[i]+len[i])
 * of that buffer, gc[i] = bytes that are C, G, c or g and total[i] = bytes that are neither N nor n.  Region bounds are
 * the caller's to check (the reference's `chr_seq.get(start..stop)`, :41).                                          */
int sk_gc_set_genome(sk_ctx *ctx, const uint8_t *genome, int64_t genome_len);
int sk_gc_count(sk_ctx *ctx, const int64_t *start, const int64_t *len, int64_t n_regions, uint64_t *gc, uint64_t *total);

/* ---- f4: `sam to fastq` sequence() ---------------------------------------------------------------------------
 * src/sam_to_fastq.rs:31-59: the bases of BAM records as ASCII — codes 1,2,4,8 -> A,C,G,T, anything else N; records
 * with flag & 0x10 come out reverse-complemented; a base whose quality is below min_baseq (the reference passes 10,
 * :103) is N.  SoA layout: row r of seq4 at seq4 + r*seq4_stride holds the record's packed bases exactly as BAM stores
 * them (two per byte, even positions in the high nibble); rows of qual (raw phred bytes) and out at + r*stride.
 * stride and seq4_stride must be multiples of 4 with 2*seq4_stride >= stride; len NULL = every row holds `stride`
 * bases; flag is the BAM flag column.  Bytes of out past a row's length are unspecified.  Pairing mates by qname
 * and the text around the bases (:96-149) stay on the host.                                                     */
int sk_bam_sequence(sk_ctx *ctx, const uint8_t *seq4, int seq4_stride, const uint8_t *qual, int stride,
                    const uint16_t *len, const uint16_t *flag, int64_t n, uint8_t min_baseq, uint8_t *out);
int sk_bam_sequence_dev(sk_ctx *ctx, const uint8_t *seq4, int seq4_stride, const uint8_t *qual, int stride,
                        const uint16_t *len, const uint16_t *flag, int64_t n, uint8_t min_baseq, uint8_t *out);

/* ---- f3: barcode census -----------------------------------------------------------------------------------
 * The HashMap<String, u64> of src/fasta_demultiplex.rs:190-194 (dry run: barcodes that matched no sample) and of
 * src/fasta_statistics.rs:23-27 (every BC: field), kept as a hash table in HBM that lives in the ctx.
 * bc is the SoA barcode matrix of sk_demux_assign: row r at bc + r*bc_stride, the barcode in its first L bytes,
 * ended early by a NUL.  L <= 31, bc_stride <= 64, alphabet ACGTNacgtn+ (what the reference's regexes admit); a row holding any
 * other byte is not counted and is reported in stats[2] (the host keeps such rows in its own map).  When assign is
 * not NULL only rows with assign[r] == SK_ASSIGN_NONE are counted (:190).  row_base + r is remembered as the first
 * occurrence of a barcode, so that results can be listed in first-seen order whatever the launch order was.    */
typedef struct sk_census_entry {
	char barcode[32];              /* NUL-terminated */
	uint64_t count;
	int64_t first_row;
} sk_census_entry;
int sk_census_reset(sk_ctx *ctx);                                 /* empty census (creates it on first use) */
int sk_census_add(sk_ctx *ctx, const uint8_t *bc, int bc_stride, int L, int64_t n, const int32_t *assign, int64_t row_base);
int sk_census_add_dev(sk_ctx *ctx, const uint8_t *bc, int bc_stride, int L, int64_t n, const int32_t *assign, int64_t row_base);
/* stats[0] distinct barcodes, [1] rows counted, [2] rows rejected, [3] table slots */
int sk_census_stats(sk_ctx *ctx, uint64_t stats[4]);
/* hist[b] = number of distinct barcodes whose count c has floor(log2(c)) == b: lets a caller pick min_count */
int sk_census_count_hist(sk_ctx *ctx, uint64_t hist[64]);
/* barcodes with count >= min_count in first-seen order; at most cap are written, *total = how many qualify */
int sk_census_entries(sk_ctx *ctx, uint64_t min_count, sk_census_entry *out, uint64_t cap, uint64_t *total);

/* ---- timing on the ctx stream (hipEvents), so a host without HIP can time device work -------------- */
int sk_timer_start(sk_ctx *ctx);
int sk_timer_stop(sk_ctx *ctx, float *ms);               /* records, synchronises, returns elapsed ms */

#ifdef __cplusplus
}
#endif
#endif

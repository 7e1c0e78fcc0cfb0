// sk_internal.h — shared between the C-ABI layer (sk_capi_*.cpp, sk_capi_comm.hip) and the gfx950 kernels (sk_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sk_lut.h"
#include "sk_tileplan.h"

namespace sk {

// (kWave, kTileRows, kLdsPad, kMaxTileStride, kMaxLdsHist, kSlots and LdsPlan: sk_tileplan.h, with the launch rules that use them)
constexpr int kMaxOneHotLen = 32;     // barcode length served by the one-hot popcount matcher (W <= 8 dwords)
constexpr int kKeyBits = 11;          // trim scan packs (U << 11 | j); rows up to 2047 bytes
constexpr int kAssignNone = -1;       // SK_ASSIGN_NONE
constexpr int kAssignAmbiguous = -2;  // SK_ASSIGN_AMBIGUOUS

// Quality threshold as packed-byte constants (see sk_kernels.hip: lowq_flags).
struct QualConsts {
	uint32_t cl2;      // splat of (256 - t2) & 0x7f
	uint32_t c72;      // 0x80808080 when (256 - t2) >= 128 else 0
	int mode;          // 0: min_baseq == 0 (never masks); 1: g1 & ~g2; 2: g1; 3: g1 | ~g2
	int min_baseq;
};
QualConsts make_qual_consts(int min_baseq);

struct MateDev {
	const uint8_t *seq;
	const uint8_t *qual;
	const uint16_t *len;
	uint8_t *out_seq;
	uint16_t *lowest_k;
};

struct BarcodeDev {
	const uint8_t *raw;        // S x L sheet bytes
	const uint32_t *onehot;    // S x W candidate codes (one-hot class bit, 0x80 wildcard), or nullptr
	const uint8_t *lut;        // L x 256 observed byte -> (class bit | 0x80), or nullptr
	// bit-sliced matcher tables (one blob, copied to LDS by every workgroup), or nullptr:
	//   [0,256)            byte -> class id 0..6 (a byte the sheet uses) or 7 (any other byte)
	//   [256, 256+4G)      valid-candidate mask, G = ceil(S/32) dwords (padded to 16 bytes)
	//   [mm_off, ...)      MM[k][class][g]: bit s%32 of dword g=s/32 set <=> candidate s counts a mismatch at
	//                      position k when the observed byte has that class
	const uint8_t *bs;
	int bs_bytes, bs_mm_off, G;
	int S, L, W, max_diff;
	// neighbourhood table (sk_lut.h; sk_kernels.hip: demux_lut_kernel); nbr.tab == nullptr: the sheet has none
	LutDev nbr;
	// spread counters (sk_kernels.hip: flush_counts_spread), or nullptr: kCountReplicas rows of count_rep_pitch u64, all zero
	// between launches
	unsigned long long *count_rep;
	int count_rep_pitch;
};
constexpr int kCountReplicas = 16;
constexpr int kMaxBitSlicedLen = 31;     // 5 counter planes
constexpr int kMaxBitSlicedBytes = 24 * 1024;

// One batch of a many-batch lookup launch (TileArgs::many).  The launch numbers the steps (256 rows each) of all batches in a row:
// batch b's are [q_begin_b, q_end).  Its pointers are BIASED by its first step — bc - q_begin * 256 * bc_stride, assign - q_begin *
// 256 and so on — so that the kernel's address of launch step gq, row r lands on the batch's own step gq - q_begin; its rows end at
// launch row row_end = q_begin * 256 + n (the launch's rows stay below 2^31).
struct ManyBatch {
	const uint8_t *bc;
	int32_t *assign;
	uint8_t *lowest_diff;
	int16_t *first_idx, *last_idx;
	uint32_t row_end;
	int32_t q_end;
};

struct TileArgs {
	int64_t n;
	int n_mates;
	int stride;
	QualConsts qc;
	MateDev mate[2];
	const uint8_t *bc;
	int bc_stride;
	BarcodeDev table;
	int32_t *assign;
	uint8_t *lowest_diff;
	int16_t *first_idx;
	int16_t *last_idx;
	int detail_matched;             // SK_DETAIL_MATCHED: the detail columns of SK_ASSIGN_NONE rows are unspecified
	unsigned long long *counts;     // device u64[S+3]
	unsigned long long *counts_wide;    // or nullptr: copies of the ctx's counters that the lookup kernel adds to instead of `counts`; the ctx folds
	                                    // them before anything reads.  counts_wide_rows == 0: kCountReplicas copies with one 128-byte line per
	                                    // counter (counter i of copy r at [(r * (S+3) + i) << kCountWideShift]: a few counters that hundreds of
	                                    // workgroups add to at once); > 0 (sheets of more than kCountDenseFrom counters): that many dense rows of
	                                    // S + 3, a workgroup adds to row blockIdx.x % rows — a thousand counters at a line each are a thousand
	                                    // uncoalesced atomics per workgroup, 17 us at the end of a 10 M-pair call of a 1 000-sample sheet
	int counts_wide_rows;
	const ManyBatch *many;          // or nullptr.  Device array of n_many batches: the lookup kernels then walk the steps of all of them in one launch
	int n_many, many_quads;         // (n = the rows of all batches, for the launch's shape; bc / assign / detail pointers above are not used)
};
constexpr int kCountWideShift = 4;
constexpr int kCountDenseFrom = 160;     // S + 3 above this: dense rows
constexpr int kCountDenseRows = 512;
hipError_t launch_counts_fold_wide(unsigned long long *wide, int nc, int dense_rows, unsigned long long *counts, hipStream_t st);

// Tile-blocked batch (include/seqkit_hip.h: sk_blocked_layout): tile t of 64 clusters reads the ONE byte range
// in + t*in_block .. +in_block and writes out + t*out_block .. +out_block; the offsets say where each segment of the
// tile sits inside its block (-1 = absent).  Both buffers hold whole blocks, also for the last, partial tile.
struct BlockedArgs {
	const uint8_t *in;
	uint8_t *out;
	int64_t n;
	int n_mates, stride, bc_stride;
	int in_block, out_block;
	int in_qual[2], in_seq[2], in_len[2], in_bc;
	int out_seq[2], out_lowest_k[2], out_assign, out_lowest_diff, out_first_idx, out_last_idx;
	QualConsts qc;
	BarcodeDev table;
	unsigned long long *counts;     // device u64[S+3]
};
hipError_t launch_tile_blocked(const BlockedArgs &a, int n_cu, hipStream_t st);
// true when the blocked kernel serves this shape (rows fit an LDS tile and the packed scan key; with barcodes: the
// bit-sliced matcher with <= 4 groups and a tile of barcodes in two 1 KiB chunks)
bool blocked_shape_ok(const BlockedArgs &a);

// launchers (all asynchronous on `st`); return hipError_t of the launch
// What launch_tile_pass decides — does the barcode phase ride in the tile pass, does the sheet's table serve a launch of its own, which
// kernel, what shape — is stated in sk_tileplan.h as functions of these two, so that the C-ABI layer asks the same rules what a call
// needs (tileplan::wants_neighbour_table, demux_plan().many_ok, demux_by_table) instead of repeating them:
//   tile_knobs(): the SK_* tuning variables, read from the environment (per call, or once per process: see there).  An entry point
//                 reads them once, so what it asks the plan and what the launcher then decides rest on the same values;
//   tile_shape(): the call as the plain facts the rules read.
// A many-batch TileArgs whose plan has no one-launch form (tileplan::DemuxPlan::many_ok) is refused with hipErrorInvalidValue.
tileplan::Knobs tile_knobs();
tileplan::Shape tile_shape(const TileArgs &a, int n_cu);
hipError_t launch_tile_pass(const TileArgs &a, const tileplan::Knobs &k, int n_cu, hipStream_t st);
hipError_t launch_mask_flat(const uint8_t *seq, const uint8_t *qual, uint8_t *out, int64_t bytes,
                            const QualConsts &qc, int n_cu, hipStream_t st);
hipError_t launch_bam_flag_tlen(const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen,
                                int64_t n, int32_t max_frag, unsigned long long *out, int want_counters, int want_hist,
                                int n_cu, hipStream_t st);

hipError_t launch_bam_fragments(const uint16_t *flag, const int32_t *tid, const int32_t *mtid, const int32_t *tlen, int64_t n,
                                int64_t min_size, int64_t max_size, uint8_t *keep_bits, unsigned long long *kept, int n_cu, hipStream_t st);

// `sam count`: record columns + the region tables of sk_count_set_regions
struct CountArgs {
	const uint16_t *flag;
	const uint8_t *mapq;
	const int32_t *tid, *mtid, *pos, *mpos, *tlen, *end_pos;
	int64_t n;
	uint32_t min_mapq, max_frag_len;
	int single_end, center;
	int n_chr;
	const int32_t *chr_off;        // n_chr + 1 offsets into the sorted region arrays
	const uint32_t *rstart, *rend, *rpmax;
	const int32_t *ridx;           // sorted position -> region index of the caller
	uint32_t *counts;
};
hipError_t launch_bam_count(const CountArgs &a, int n_cu, hipStream_t st);

// `sam statistics --on-target` (sk_bamtarget.hip): record columns + the region tables of sk_on_target_set_regions
struct TargetArgs {
	const uint16_t *flag;
	const int32_t *tid, *mtid, *pos, *mpos, *tlen, *end_pos;
	int64_t n;
	int64_t max_frag_len;
	int n_chr;
	const int32_t *chr_off;        // n_chr + 1 offsets into the sorted region arrays
	const int64_t *rstart, *rpmax; // 1-based inclusive starts, ascending per chromosome; the running maximum of the ends
	unsigned long long *out;       // u64[6]: total, aligned, duplicate reads; total, on-target fragments; fragments with a tid outside [0, n_chr)
};
hipError_t launch_bam_target(const TargetArgs &a, int n_cu, hipStream_t st);

hipError_t launch_gc_count(const uint8_t *genome, const int64_t *seg_start, const int32_t *seg_len, const int32_t *seg_region, int64_t nseg,
                           unsigned long long *out, int n_cu, hipStream_t st);

hipError_t launch_bam_sequence(const uint8_t *seq4, int seq4_stride, const uint8_t *qual, int stride, const uint16_t *len, const uint16_t *flag,
                               int64_t n, int min_baseq, uint8_t *out, int n_cu, hipStream_t st);

// ---- BGZF inflate and the BAM record walk on the device (sk_inflate.hip) ----
// blocks: device array of sk_bgzf_block; status: device u32 per block (0 = inflated; 1..8 the decoder gave up; | 0x100 CRC mismatch)
hipError_t launch_bgzf_inflate(const uint8_t *comp, const void *blocks, int64_t n_blocks, uint8_t *out, uint32_t *status, int check_crc, int n_cu, hipStream_t st);
hipError_t launch_bam_walk(const uint8_t *stream, uint64_t stream_len, const uint64_t *bend, uint64_t *entry, uint64_t *exitp, uint32_t *nrec, int64_t n,
                           uint64_t first, uint32_t *changed, int fix_round /* 0 first walk, 1 fix, 2 guess */, int32_t n_ref, hipStream_t st);
hipError_t launch_bam_walk_reduce(const uint8_t *stream, uint64_t stream_len, const uint64_t *bend, const uint64_t *entry, int64_t n, int32_t max_frag,
                                  int want_counters, int want_hist, unsigned long long *out, hipStream_t st);
hipError_t launch_bam_gather(const uint8_t *stream, uint64_t stream_len, const uint64_t *bend, const uint64_t *entry, const uint64_t *rec_base, int64_t n,
                             uint16_t *flag, uint8_t *mapq, int32_t *tid, int32_t *mtid, int32_t *pos, int32_t *mpos, int32_t *tlen, int32_t *end_pos,
                             hipStream_t st);
// sam to raw|fasta|fastq over a verified stream (sk_bamtext.hip): the sizing pass + the scans of its per-block sums, the kept records'
// columns, and one window's text
hipError_t launch_bam_reads_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int fmt, int want_unpaired,
                                 uint64_t *bk, uint64_t *bt, uint64_t *bn, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_reads_index(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int fmt, int want_unpaired,
                                  const uint64_t *bk, const uint64_t *bt, const uint64_t *bn, uint64_t *krec, uint64_t *ktoff, uint64_t *knoff,
                                  uint64_t *kkey, uint8_t *kkind, hipStream_t st);
hipError_t launch_bam_reads_text(const uint8_t *stream, const uint64_t *krec, const uint64_t *ktoff, const uint64_t *knoff, int64_t first, int64_t n,
                                 uint64_t t0, uint64_t n0, int fmt, uint8_t min_baseq, uint8_t *text, uint64_t *toff, uint8_t *names, uint32_t *noff,
                                 int n_cu, hipStream_t st);

// ---- BGZF deflate on the device (sk_deflate.hip) ----
// blocks: device array of sk_deflate_block; out: n_blocks slots of out_stride bytes (a block's payload from the slot's first byte on);
// tokens: device u32[n_blocks * deflate_tokens_per_block()] scratch; result: device u32[2 n] (payload bytes, tokens); crc: device u32[n]
hipError_t launch_bgzf_deflate(const uint8_t *in, const void *blocks, int64_t n_blocks, uint8_t *out, uint32_t out_stride, uint32_t *tokens, uint32_t *result,
                               uint32_t *crc, int n_cu, hipStream_t st);
size_t deflate_tokens_per_block();
hipError_t launch_bgzf_crc(const uint8_t *in, const void *blocks, int64_t n_blocks, uint32_t *crc, int n_cu, hipStream_t st);

hipError_t launch_scan_u64(uint64_t *v, int64_t n, hipStream_t st);     // sk_bamtext.hip: v[0 .. n) -> exclusive offsets, v[n] the sum
// the window plan of sk_bam_file_reads and of sk_bam_file_rewrite, _minimize and _markdup (sk_bamtext.hip): window w holds the records whose key off0[j] + off1[j]
// (off1 == nullptr: off0[j]) lies in [w W, (w + 1) W); ws[w] = its first record, w0[w] / w1[w] = that record's off0 / off1 (w1 only with
// off1).  The entries past the last record's window hold (n, total0, total1).  nw entries in all.
hipError_t launch_bam_windows(const uint64_t *off0, const uint64_t *off1, int64_t n, uint64_t W, uint64_t total0, uint64_t total1, uint64_t *ws,
                              uint64_t *w0, uint64_t *w1, int64_t nw, hipStream_t st);
// ---- BAM out: the per-record rewrite of sk_bam_file_rewrite and the BGZF member packing (sk_bamwrite.hip) ----
// One window of a BAM-writing call, as every window writer takes it: records first .. first + n - 1 of the written ones (krec: their
// stream offsets, kout: their output offsets) into out, whose first byte is output offset o0
struct WriteWindow {
	const uint8_t *stream;
	const uint64_t *krec, *kout;
	int64_t first, n;
	uint64_t o0;
	uint8_t *out;
};
// size: per block the rewritten bytes of the records that begin in it (then exclusive offsets, bo[nb] the total) and the OR of the
// records' decline bits; index: every record's stream offset and output offset (rb: the blocks' first record indices); write: the
// window's records into w.out
hipError_t launch_bam_rw_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int op, uint64_t *bo, uint32_t *decline,
                              hipStream_t st);
hipError_t launch_bam_rw_index(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, int op, const uint64_t *bo,
                               const uint64_t *rb, uint64_t *krec, uint64_t *kout, hipStream_t st);
hipError_t launch_bam_rw_write(const WriteWindow &w, int op, int n_cu, hipStream_t st);
// ---- sam minimize: the read ids and the per-record rewrite of sk_bam_file_minimize (sk_bamminimize.hip) ----
// The key rule of the id passes.  whole_name == 0: a record's key is its name up to the first '/' (minimize); else the whole name.
// skip_flags: a record with one of these flag bits takes no part — it neither opens nor closes an occurrence of its name, and its id is
// 0; key_bits is then at most 63, the key of such a record is bit key_bits alone, and bam_sort_pairs sorts key_bits + 1 bits.
struct IdRule { int whole_name; uint32_t skip_flags; };
inline uint64_t id_skip_bit(IdRule rule, int key_bits) { return rule.skip_flags ? (uint64_t)1 << key_bits : 0; }
// keys: every record's stream offset, the hash of its key (its low key_bits bits) and its index; decline bit 8: an
// invalid record.  bam_sort_pairs: (u64 key, u32 index) by the key's low key_bits bits, stable, between the two buffers of each kind (*sorted: the one that holds the result);
// temp == nullptr: only *temp_bytes.  ids: from the sorted pairs the records' ids (agg: u32[n / 1024 + 1] scratch; src, cnt: u32[n]
// scratch); decline bit 64: two different keys with one hash.  size / index / write: as launch_bam_rw_*; flags SK_MINIMIZE_*; ids ==
// nullptr without SK_MINIMIZE_READ_IDS; decline bit 32: a CIGAR operation code above 8.
hipError_t launch_bam_min_keys(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int key_bits,
                               IdRule rule, uint64_t *krec, uint64_t *key, uint32_t *idx, uint32_t *decline, hipStream_t st);
hipError_t bam_sort_pairs(void *temp, size_t *temp_bytes, uint64_t *key[2], uint32_t *idx[2], uint64_t n, int key_bits, int *sorted, hipStream_t st);
hipError_t launch_bam_min_ids(const uint8_t *stream, const uint64_t *krec, const uint64_t *key, const uint32_t *idx, uint64_t n, int key_bits,
                              IdRule rule, uint32_t *agg, uint32_t *src, uint32_t *cnt, uint32_t *ids, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_min_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int flags,
                               const uint32_t *ids, uint64_t *bo, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_min_index(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int flags,
                                const uint32_t *ids, const uint64_t *bo, uint64_t *krec, uint64_t *kout, hipStream_t st);
hipError_t launch_bam_min_write(const WriteWindow &w, const uint32_t *ids, int flags, uint8_t fill, int n_cu, hipStream_t st);
// ---- sam mark duplicates: the record passes of sk_bam_file_markdup (sk_bammarkdup.hip) ----
// The per-record columns, in file order: stream and output offsets, (tid << 32 | (u32) pos), start_pos, fraglen | strand << 16 |
// mapped << 17 (bit 31 is the cluster pass's), l_seq, the UMI's offset in the record and its length, and the flag to write.
struct MdCols {
	uint64_t *krec, *kout, *tidpos;
	uint32_t *start, *fl, *lseq, *uoff, *ulen;
	uint16_t *nflag;
};
// sig: the columns and the decline bits 1, 4, 8, 16, 32 of include/seqkit_hip.h (first: the stream offset of the first record).  order:
// runflag[k] = 1 where record k's tid differs from its predecessor's; decline bit 2.  run_scan: run = the inclusive sum of runflag (temp
// == nullptr: only *temp_bytes).  keys: (key, index) for bam_sort_pairs, key = (run - 1) << 33 | start_pos << 1 | strand, all ones for an
// unmapped read.  cluster: over the sorted pairs, every mapped read's flag into cols.nflag, then *count = the records with 0x400.
// write: as launch_bam_rw_write, bytes 18-19 of every record from nflag.
hipError_t launch_bam_md_sig(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int ignore_umi,
                             uint64_t first, const MdCols &cols, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_md_order(const uint64_t *tidpos, uint64_t n, uint32_t *runflag, uint32_t *decline, hipStream_t st);
hipError_t bam_md_run_scan(void *temp, size_t *temp_bytes, const uint32_t *runflag, uint32_t *run, uint64_t n, hipStream_t st);
hipError_t launch_bam_md_keys(const uint32_t *run, const MdCols &cols, uint64_t n, uint64_t *key, uint32_t *idx, hipStream_t st);
hipError_t launch_bam_md_cluster(const uint8_t *stream, const MdCols &cols, const uint64_t *key, const uint32_t *idx, uint64_t n, uint64_t *count,
                                 int n_cu, hipStream_t st);
hipError_t launch_bam_md_write(const WriteWindow &w, const uint16_t *nflag, int n_cu, hipStream_t st);
// ---- sam subsample: the keep pass, the compaction and the window copy of sk_bam_file_subsample (sk_bamsubsample.hip) ----
// Rule 3 of the command, the one statement of it (sk_subsample_keep, the keep pass): draw d of seed s is splitmix64's d-th output from
// state s, its top 24 bits m; keep iff m <= T.
__host__ __device__ inline bool subsample_keeps(uint64_t seed, uint64_t draw, uint32_t T)
{
	uint64_t z = seed + draw * 0x9E3779B97F4A7C15ull;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	return (uint32_t)(z >> 40) <= T;
}
inline uint32_t subsample_threshold(float fraction) { return (uint32_t)((double)fraction * 16777216.0); }   // floor(fraction 2^24), 0 <= fraction <= 1
// keep: per record (krec: its stream offset, ids: its fragment number from the id passes under IdRule{1, 0x800}) len[k] = the record's
// bytes when it is kept, 0 when it is dropped or has 0x800; counts[0 .. 2] += the counted records, the kept ones, the kept ones' bytes;
// decline bit 1: a counted record without 0x1.  scans (temp == nullptr: only *temp_bytes): pos[k] = the kept records before k, off[k] =
// their bytes.  compact: the kept records' stream and output offsets, in order.  copy_write: as launch_bam_rw_write, every record byte for
// byte (sam merge without --suffix writes its windows with it too).
hipError_t launch_bam_sub_keep(const uint8_t *stream, const uint64_t *krec, const uint32_t *ids, uint64_t n, uint64_t seed, uint32_t T, uint32_t *len,
                               uint64_t *counts, uint32_t *decline, int n_cu, hipStream_t st);
hipError_t bam_sub_scans(void *temp, size_t *temp_bytes, const uint32_t *len, uint32_t *pos, uint64_t *off, uint64_t n, hipStream_t st);
hipError_t launch_bam_sub_compact(const uint64_t *krec, const uint32_t *len, const uint32_t *pos, const uint64_t *off, uint64_t n, uint64_t *kept_rec,
                                  uint64_t *kept_out, hipStream_t st);
hipError_t launch_bam_copy_write(const WriteWindow &w, int n_cu, hipStream_t st);
// ---- sam recalculate tlen: the record passes of sk_bam_file_recalc_tlen (sk_bamtlen.hip) ----
// The rule its key columns are written under, for bam_sort_pairs and launch_bam_min_ids: the whole name is the key, and there are records
// that take no part, so key_bits is at most 63 (which ones the key kernel here decides by the record's class; the two read of
// skip_flags only that it is not 0).
constexpr IdRule kTlenIdRule{1, ~0u};
// keys: as launch_bam_min_keys, a candidate's key the hash of its name and every other record's the skip bit; decline bits 1 (a record
// the reference stops at), 8 (an invalid record), 16 (a name byte >= 0x80).  resolve: from src (launch_bam_min_ids) tlen[k] for every
// record that is written and len[k] = its bytes, 0 for a candidate without a mate; decline bits 2 (mates with equal 0x40 bits) and 32 (a
// CIGAR operation code above 8 on a reverse candidate).  gather (pos: bam_sub_scans over len): the written records' TLENs in written
// order and the discarded records' stream offsets in file order.  write: as launch_bam_copy_write, bytes 32-35 of every record from
// tlen.  names: discarded records first .. first + n - 1 into n slots of 256 bytes, each the name and NULs behind it.
hipError_t launch_bam_tlen_keys(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, int64_t max_len,
                                int key_bits, uint64_t *krec, uint64_t *key, uint32_t *idx, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_tlen_resolve(const uint8_t *stream, const uint64_t *krec, const uint32_t *src, uint64_t n, int32_t *tlen, uint32_t *len,
                                   uint32_t *decline, int n_cu, hipStream_t st);
hipError_t launch_bam_tlen_gather(const uint64_t *krec, const uint32_t *len, const uint32_t *pos, const int32_t *tlen, uint64_t n, int32_t *tlen_out,
                                  uint64_t *disc, int n_cu, hipStream_t st);
hipError_t launch_bam_tlen_write(const WriteWindow &w, const int32_t *tlen, int n_cu, hipStream_t st);
hipError_t launch_bam_tlen_names(const uint8_t *stream, const uint64_t *disc, int64_t first, int64_t n, uint8_t *out, int n_cu, hipStream_t st);
// ---- sam merge: the record passes of sk_bam_file_merge (sk_bammerge.hip) ----
// The per-record columns in input order (input 1's records first, then input 2's ..): the record's address as an offset from input 1's
// stream mod 2^64, its key (u32 refID) << 32 | (u32 pos ^ 0x80000000), its index, its output bytes and its input number (1-based).
struct MergeCols {
	uint64_t *addr, *key;
	uint32_t *idx, *len;
	uint8_t *in;
};
// keys: one input's blocks (rb: their first records' GLOBAL indices; delta: this stream's address less input 1's; suffix_len: 0 without
// --suffix, else the bytes of ".N") into the columns; decline bits 8 (an invalid record) and 1 (a suffixed name above 254 bytes).
// order: decline bit 2 where a key is below its predecessor's in the same input.  gather: output place p takes record idx[p]'s address,
// length (into kout) and input number; scan (temp == nullptr: only *temp_bytes): kout[0 .. n) -> exclusive offsets, kout[n] the sum.  write: as launch_bam_copy_write, ".N" behind every record's name; without a
// suffix launch_bam_copy_write itself writes the windows.
hipError_t launch_bam_merge_keys(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, uint64_t delta,
                                 uint32_t input, uint32_t suffix_len, const MergeCols &cols, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_merge_order(const MergeCols &cols, uint64_t n, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_merge_gather(const uint32_t *idx, const MergeCols &cols, uint64_t n, uint64_t *krec, uint64_t *kout, uint8_t *kin, hipStream_t st);
hipError_t bam_merge_scan(void *temp, size_t *temp_bytes, uint64_t *kout, uint64_t n, hipStream_t st);
hipError_t launch_bam_merge_write(const WriteWindow &w, const uint8_t *kin, int n_cu, hipStream_t st);
// ---- sam concatenate: the record passes of sk_bam_file_concatenate (sk_bamconcat.hip) ----
// size: every record's stream offset (krec) and output bytes block_size + 4 + suffix_len (kout; bam_merge_scan then makes offsets of
// them), rb: the blocks' first records; decline bits 8 (an invalid record) and 1 (a suffixed name above 254 bytes).  write: as
// launch_bam_copy_write, '.' and the decimal digits of number — suffix_len bytes, 2 .. 11 — behind every record's name.
hipError_t launch_bam_concat_size(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const uint64_t *rb, uint32_t suffix_len,
                                  uint64_t *krec, uint64_t *kout, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_concat_write(const WriteWindow &w, uint32_t number, uint32_t suffix_len, int n_cu, hipStream_t st);
// ---- sam discard tail artifacts: the record passes of sk_bam_file_discard_tails (sk_bamtails.hip) ----
// A BAM refID's chromosome on the device: where its span of the FASTA file begins in the genome buffer, its bases, and the .fai's line
// shape; line_bases == 0: the refID has none (no line of that name, or a span that ends beyond the file).
struct TailRef { uint64_t base, length, line_bases, line_width; };
constexpr int32_t kTailUnmapped = INT32_MIN;     // tidc of an unmapped record (as a refID it is outside every header, and declined)
// used: used[t] = 1 for the refIDs 0 .. n_refs - 1 that mapped records name (krec: the records' stream offsets).  keep: len[k] = record
// k's bytes where it is written, else 0; tidc[k] = its refID or kTailUnmapped; counts[0 .. 4] += the records, the failed, the passed
// and the written ones, the written bytes; decline bits 1 (an operation outside M I D = X on a mapped record), 2 (an examined base
// outside the read or the chromosome), 4 (a mapped record's refID without a chromosome), 16 (a value outside the i32 range).  loads
// (temp == nullptr: only *temp_bytes; last: n entries of scratch): the refIDs of the chromosome loads after the first, in file order,
// and *n_loads (device) their number.
hipError_t launch_bam_tail_used(const uint8_t *stream, const uint64_t *krec, uint64_t n, int32_t n_refs, uint32_t *used, int n_cu, hipStream_t st);
hipError_t launch_bam_tail_keep(const uint8_t *stream, const uint64_t *krec, uint64_t n, const uint8_t *genome, const TailRef *refs, int32_t n_refs,
                                uint32_t tail_length, uint32_t min_mismatches, uint32_t *len, int32_t *tidc, uint64_t *counts, uint32_t *decline, int n_cu,
                                hipStream_t st);
hipError_t bam_tail_loads(void *temp, size_t *temp_bytes, const int32_t *tidc, int32_t *last, int32_t *loads, uint64_t *n_loads, uint64_t n, hipStream_t st);
// ---- sam to: the mate pairing of sk_bam_file_pairs and its windows' text (sk_bampair.hip) ----
// Over the K kept records of launch_bam_reads_index (file order; kind 0 unpaired, 1 first, 2 last mate).  A record's fate: where its text
// goes; aux: for a record of a pair the kept index of the record that COMPLETED the pair, for a leftover its order record.  Its class: what
// it counts as in the scan of the ranks (one class at most).
constexpr int kPairBlock = 256;                  // the workgroup of every pairing kernel: one sorted position or kept record per lane
constexpr uint8_t kPairSingle = 0, kPairStream1 = 1, kPairStream2 = 2, kPairLeft1 = 3, kPairLeft2 = 4, kPairNowhere = 5;
constexpr uint8_t kPairClsNone = 0, kPairClsSingle = 1, kPairClsCompleter = 2, kPairClsOrder1 = 3, kPairClsOrder2 = 4;
struct PairRanks { uint32_t single, pair, order1, order2; };
// scan_bytes: the scratch every scan below takes over n elements.  scan_paired: ipos[k] = the paired records among 0 .. k.  compact: the
// paired records' (key cut to key_bits, index) at ipos - 1, every record's initial fate, aux and class.  [bam_sort_pairs.]  heads: lz[p] = p
// where sorted position p begins a run of one key or follows a record of its own kind, else 0; decline bit 64: two names under one key.
// scan_max (in place): lz[p] = the last such position.  holds, scan_max: hs[p] = where the stretch of held records around p begins.
// fates: fate, aux, class.  scan_ranks: per class the records among 0 .. k.  place: stream s's n[s] records into perm / slen from entry
// base[s] + s on (slen: n[s] + 1 entries, the last one 0); interleaved: stream 0 holds both mates of pair p at 2 p, 2 p + 1, streams 1 and 2
// nothing.  scan_offsets (in place): the text lengths to stream offsets.  text: ranks first .. first + n - 1 of one stream into text.
hipError_t bam_pair_scan_bytes(uint64_t n, size_t *temp_bytes, hipStream_t st);
hipError_t bam_pair_scan_paired(void *temp, size_t temp_bytes, const uint8_t *kkind, uint32_t *ipos, uint64_t n, hipStream_t st);
hipError_t bam_pair_scan_max(void *temp, size_t temp_bytes, uint32_t *v, uint64_t n, hipStream_t st);
hipError_t bam_pair_scan_ranks(void *temp, size_t temp_bytes, const uint8_t *cls, PairRanks *ranks, uint64_t n, hipStream_t st);
hipError_t bam_pair_scan_offsets(void *temp, size_t temp_bytes, uint64_t *lens, uint64_t n, hipStream_t st);
hipError_t launch_bam_pair_compact(const uint8_t *kkind, const uint64_t *kkey, const uint32_t *ipos, uint64_t K, int key_bits, uint64_t *key, uint32_t *idx,
                                   uint8_t *fate, uint32_t *aux, uint8_t *cls, hipStream_t st);
hipError_t launch_bam_pair_heads(const uint8_t *stream, const uint64_t *krec, const uint8_t *kkind, const uint64_t *key, const uint32_t *idx, uint64_t P,
                                 uint32_t *lz, uint32_t *decline, hipStream_t st);
hipError_t launch_bam_pair_holds(const uint64_t *key, const uint32_t *lz, uint64_t P, uint32_t *hs, hipStream_t st);
hipError_t launch_bam_pair_fates(const uint64_t *key, const uint32_t *idx, const uint8_t *kkind, const uint32_t *lz, const uint32_t *hs, uint64_t P,
                                 uint8_t *fate, uint32_t *aux, uint8_t *cls, hipStream_t st);
hipError_t launch_bam_pair_place(const uint8_t *fate, const uint32_t *aux, const PairRanks *ranks, const uint64_t *ktoff, uint64_t K, uint64_t T,
                                 const uint64_t n[3], const uint64_t base[3], uint32_t n_single, uint32_t n_left1, int interleaved, uint32_t *perm,
                                 uint64_t *slen, hipStream_t st);
hipError_t launch_bam_pair_text(const uint8_t *stream, const uint64_t *krec, const uint32_t *perm, const uint64_t *soff, int64_t first, int64_t n, int fmt,
                                uint8_t min_baseq, uint8_t *text, int n_cu, hipStream_t st);
// ---- sam coverage histogram: the record passes of sk_bam_file_coverage (sk_bamcoverage.hip) ----
// What the two record passes take (all device memory).  base[r] = the global coordinate of reference r's position 0, base[n_ref] the
// total.  ioff == nullptr: no intervals; else reference r's merged, sorted, disjoint intervals are [ibeg[k], iend[k]) for k in
// [ioff[r], ioff[r + 1]).  has / hit: a bit per reference (zeroed by the caller), counted and decline: one word each (zeroed).
constexpr uint32_t kCovDepthUp = 0u, kCovDepthDown = 1u, kCovInsideUp = 2u, kCovInsideDown = 3u;    // an event's kind: what it adds to which running sum
struct CovArgs {
	int32_t n_ref;
	const uint64_t *base;
	const uint32_t *ioff;
	const int64_t *ibeg, *iend;
	uint64_t *bruns;              // [nb + 1]: per block the runs of its records, then (launch_scan_u64) exclusive offsets
	uint32_t *has, *hit;
	unsigned long long *counted;
	uint32_t *decline;            // bit 8: an invalid record
};
// mark: bruns (scanned), has, hit, counted, decline.  emit: run q's two events into key / kind[2 q], [2 q + 1].  scan (temp == nullptr:
// only *temp_bytes): sums[i] = depth + inside * 2^32 behind sorted event i.  hist: hist[SK_COVERAGE_BINS] and totals[0 .. 1] = the
// positions inside the targets and those deeper than the last bin (both zeroed here).
hipError_t launch_bam_cov_mark(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const CovArgs &a, hipStream_t st);
hipError_t launch_bam_cov_emit(const uint8_t *stream, const uint64_t *bend, const uint64_t *entry, int64_t nb, const CovArgs &a, uint64_t *key,
                               uint32_t *kind, hipStream_t st);
hipError_t bam_cov_scan(void *temp, size_t *temp_bytes, const uint32_t *kind, int64_t *sums, uint64_t n, hipStream_t st);
hipError_t launch_bam_cov_hist(const uint64_t *key, const int64_t *sums, uint64_t n, uint64_t *hist, uint64_t *totals, int n_cu, hipStream_t st);
// BGZF members of raw[0 .. raw_len): the cut into blocks of at most 0xff00 bytes (blocks: device sk_deflate_block[n]), and, after the
// deflate (or at level 0 the CRC alone), the members back to back into out: msz[n + 1] scratch, msz[n] = their total bytes afterwards
hipError_t launch_bgzf_cut(uint64_t raw_len, void *blocks, int64_t n, hipStream_t st);
hipError_t launch_bgzf_pack(const uint8_t *raw, const void *blocks, int64_t n, const uint8_t *slots, uint32_t slot_stride, const uint32_t *result,
                            const uint32_t *crc, int stored_only, uint64_t *msz, uint8_t *out, int n_cu, hipStream_t st);

// ---- barcode census (sk_census.hip) ----
struct Census;
struct CensusEntry {            // == sk_census_entry of include/seqkit_hip.h
	char barcode[32];           // NUL-terminated
	uint64_t count;
	int64_t first_row;
};
hipError_t census_create(Census **out, hipStream_t st);
void census_destroy(Census *cs);
hipError_t census_reset(Census *cs, int n_cu, hipStream_t st);
hipError_t census_add(Census *cs, const uint8_t *bc, int bc_stride, int L, int64_t n, const int32_t *assign, int64_t row_base,
                      int n_cu, hipStream_t st);
hipError_t census_stats(Census *cs, uint64_t out[4], hipStream_t st);
uint64_t census_slots(const Census *cs);
hipError_t census_count_hist(Census *cs, uint64_t hist[64], int n_cu, hipStream_t st);
hipError_t census_entries(Census *cs, uint64_t min_count, CensusEntry *out, uint64_t cap, uint64_t *total, int n_cu, hipStream_t st);
constexpr int kMaxCensusLen = 31;

}  // namespace sk

// ---- what the file calls (sk_bamfile*.cpp) need of a ctx (sk_ctx.h holds the struct, for the units of the C-ABI layer alone; sk_capi_ctx.cpp defines these) ----
struct sk_ctx;
namespace sk {
// The buffers that stay with a ctx from call to call (ctx_keep).  The file calls' front half (sk_bamfile.cpp: bam_file_front) keeps the
// compressed file, the inflated stream, the reader ring, the block table and its device copy and the blocks' status.  The reads and
// rewrite calls share their three slots: only one file call's state is live on a ctx (the next file call ends the one before).
enum KeepSlot {
	kKeepComp = 0, kKeepOut = 1, kKeepPin = 2, kKeepTable = 3, kKeepBlocks = 4, kKeepStatus = 5,   // the front half
	kKeepCols = 6,                                      // sk_bam_file_columns: the columns, which sk_bam_fragments_bed_dev reads after it
	kKeepTextPin = 7, kKeepText = 8,                    // sk_bam_fragments_bed_dev: the BED text (sk_bamtext.hip)
	kKeepFileCols = 9, kKeepFileWin = 10, kKeepFilePin = 11,    // sk_bamfile_reads.cpp, sk_bamfile_out.cpp: per-record columns, windows
	// The record passes' working memory (sk_passmem.h: each call lists its regions in a Layout, and a Placement says where they lie).
	// Here lies what a call's windows read later — minimize's read ids, markdup's flag column, merge's input numbers — and behind it the
	// passes' scratch of markdup, subsample, merge and coverage where the compressed file's idle buffer is too small for it.
	kKeepPassWork = 12,
	kKeepDeflatePin = 13,                               // sk_bgzf_deflate: the pinned landing area of the compressed slots (a host may deflate while a file call's state is live)
	kKeepSlots = 14
};
hipStream_t ctx_stream(sk_ctx *c);
hipStream_t ctx_stream2(sk_ctx *c);
int ctx_n_cu(sk_ctx *c);
void *ctx_keep(sk_ctx *c, KeepSlot slot, size_t bytes, bool pinned, int *rc);      // a buffer that stays with the ctx from call to call (freed by sk_destroy)
size_t ctx_kept_bytes(sk_ctx *c, KeepSlot slot);
void *ctx_ext(sk_ctx *c);                                       // an object kept with the ctx (freed by sk_destroy through free_fn)
void ctx_set_ext(sk_ctx *c, void *p, void (*free_fn)(void *));
int ctx_bind(sk_ctx *c);                                        // hipSetDevice; SK_OK or an error code with the message set
int ctx_fail(sk_ctx *c, int code, const char *fmt, ...);       // sets sk_last_error, returns code
}  // namespace sk

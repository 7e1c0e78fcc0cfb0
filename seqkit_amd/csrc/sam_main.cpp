// sam — the `sam` binary of the reference, with the per-record work done by the MI355X library behind include/seqkit_hip.h
// (dispatch: src/sam_main.rs:50-53).  This file is the dispatch; the commands, and the file of this host that serves each:
//
//   sam statistics [--on-target=BED] <bam_file>                                 sam_columns.cpp   src/sam_statistics.rs
//   sam fragment lengths [--max-frag-size=F] [--reads=N] <bam_file>             sam_columns.cpp   src/sam_fragment_lengths.rs
//   sam fragments [--min-size=N] [--max-size=N] <bam_file>                      sam_columns.cpp   src/sam_fragments.rs
//   sam count [--min-mapq=N] [--max-frag-len=N] [--single-end] [--center] <bam_file> <regions.bed>
//                                                                               sam_columns.cpp   src/sam_count.rs
//   sam to raw|fasta|fastq <bam_file> <out_prefix>                              sam_reads.cpp     src/sam_to_fastq.rs
//   sam to interleaved raw|fasta|fastq <bam_file>                               sam_reads.cpp     src/sam_to_fastq.rs
//   sam trim qnames <bam_file>                                                  sam_bamout.cpp    src/sam_trim_qnames.rs
//   sam tags from qname [--uncompressed] <bam_file>                             sam_bamout.cpp    src/sam_tags_from_qname.rs
//   sam qname from tags [--uncompressed] <bam_file>                             sam_bamout.cpp    src/sam_qname_from_tags.rs
//   sam minimize [--uncompressed] [--read-ids] [--base-qualities] [--tags] [--baseq-fill=N] <bam_file>
//                                                                               sam_bamout.cpp    src/sam_minimize.rs
//   sam mark duplicates [--uncompressed] [--ignore-umi] <bam_file>              sam_bamout.cpp    src/sam_mark_duplicates.rs
//   sam subsample [--seed=N] <bam_file> <fraction>                              sam_bamout.cpp    src/sam_subsample.rs
//   sam recalculate tlen [--uncompressed] [--max-len=N] <bam_file>              sam_bamout.cpp    src/sam_recalculate_tlen.rs
//   sam merge [--suffix] [--uncompressed] <bam_files>...                        sam_bamout.cpp    src/sam_merge.rs
//   sam concatenate [--uncompressed] <bam_files>...                             sam_bamout.cpp    src/sam_concatenate.rs
//   sam discard tail artifacts [--tail-length=N] [--threshold=F] [--mismatches=N] [--debug] <ref_genome.fa> <bam_file> | --test
//                                                                               sam_tails.cpp     src/sam_discard_tail_artifacts.rs
//   sam coverage histogram [--region=REGION] [--regions=BED] <bam_file>         sam_coverage.cpp  src/sam_coverage_histogram.rs
//
// (`sam concatenate` and `sam discard tail artifacts` are source files of the reference that its src/sam_main.rs does not declare, as
// `sam recalculate tlen` is: the top-level usage below stays the reference's, which lists none of them.)
//
// The reference reads BAM through rust-htslib; this host reads and writes the container itself (sam_bamio.cpp, declared with everything
// else the files share in sam_host.h).  Every command offers a regular file to the device whole first and keeps a record-by-record
// reader for what the device does not take: stdin, SEQKIT_HOST_INFLATE=1, and each file it declines before anything has been written.
#include <malloc.h>
#include <unistd.h>

#include "sam_host.h"

static const char *USAGE_TOP =
	"\nUsage:\n"
	"  sam merge <bam_files>...\n  sam consensus <bam_file>\n  sam count <bam_file> <regions.bed>\n  sam coverage histogram <bam_file>\n"
	"  sam fragments <bam_file>\n  sam fragment lengths <bam_file>\n  sam mark duplicates <bam_file>\n  sam minimize <bam_file>\n"
	"  sam statistics <bam_file>\n  sam subsample <bam_file> <fraction>  \n  sam tags from qname <bam_file>\n  sam qname from tags <bam_file>\n"
	"  sam trim qnames <bam_file>  \n\nExtract reads from BAM files:  \n  sam to fasta <bam_file> <out_prefix>\n  sam to fastq <bam_file> <out_prefix>  \n"
	"  sam to interleaved fasta <bam_file>\n  sam to interleaved fastq <bam_file>\n  sam to interleaved raw <bam_file>\n  sam to raw <bam_file> <out_prefix>\n";

int main(int argc, char **argv)
{
	// blocks, per-sample strings and gzip jobs are hundreds of KiB each: above glibc's default mmap threshold every one of them was a
	// mapping of its own, faulted in page by page and given back when freed (2.3 s of system time in a demultiplex of 8 M reads).  From
	// the arenas they are recycled.  (SEQKIT_MALLOC_DEFAULT=1: glibc's defaults, for A/B)
	if (!getenv("SEQKIT_MALLOC_DEFAULT")) {
		mallopt(M_MMAP_THRESHOLD, 32 << 20);
		mallopt(M_TRIM_THRESHOLD, 1 << 30);
		mallopt(M_TOP_PAD, 64 << 20);
	}
	int rc = 0;
	auto is = [&](int i, const char *w) { return argc > i && strcmp(argv[i], w) == 0; };
	if (argc >= 2 && is(1, "count")) rc = count_cmd(argc, argv);
	else if (argc >= 2 && is(1, "fragments")) rc = fragments_cmd(argc, argv);
	else if (argc >= 2 && is(1, "statistics")) rc = statistics_cmd(argc, argv);
	else if (argc >= 3 && is(1, "fragment") && is(2, "lengths")) rc = fragment_lengths_cmd(argc, argv);
	else if (argc >= 3 && is(1, "to") && (is(2, "raw") || is(2, "fasta") || is(2, "fastq"))) rc = to_reads_cmd(argc, argv);
	else if (argc >= 4 && is(1, "to") && is(2, "interleaved") && (is(3, "raw") || is(3, "fasta") || is(3, "fastq"))) rc = to_reads_cmd(argc, argv);
	else if (argc >= 4 && is(1, "tags") && is(2, "from") && is(3, "qname")) rc = tags_from_qname_cmd(argc, argv);
	else if (argc >= 4 && is(1, "qname") && is(2, "from") && is(3, "tags")) rc = qname_from_tags_cmd(argc, argv);
	else if (argc >= 3 && is(1, "trim") && is(2, "qnames")) rc = trim_qnames_cmd(argc, argv);
	else if (argc >= 2 && is(1, "minimize")) rc = minimize_cmd(argc, argv);
	else if (argc >= 3 && is(1, "mark") && is(2, "duplicates")) rc = mark_duplicates_cmd(argc, argv);
	else if (argc >= 2 && is(1, "subsample")) rc = subsample_cmd(argc, argv);
	else if (argc >= 3 && is(1, "recalculate") && is(2, "tlen")) rc = recalculate_tlen_cmd(argc, argv);
	else if (argc >= 2 && is(1, "merge")) rc = merge_cmd(argc, argv);
	else if (argc >= 2 && is(1, "concatenate")) rc = concatenate_cmd(argc, argv);
	else if (argc >= 4 && is(1, "discard") && is(2, "tail") && is(3, "artifacts")) rc = discard_tail_artifacts_cmd(argc, argv);
	else if (argc >= 3 && is(1, "coverage") && is(2, "histogram")) rc = coverage_histogram_cmd(argc, argv);
	else fprintf(stderr, "%s\n", USAGE_TOP);
	host::out().flush();
	// everything is written and closed: what is left is taking the process apart (static destructors, the HIP runtime's exit handlers,
	// gigabytes of heap) — 0.16 s of a demultiplex of 8 M reads.  That is left to the kernel, as on the error path (host::error);
	// SEQKIT_SLOW_EXIT=1 (and SEQKIT_PROF, whose last lines are printed by destructors) returns from main instead.
	if (!getenv("SEQKIT_SLOW_EXIT") && !getenv("SEQKIT_PROF")) { host::flush_for_exit(); fflush(stdout); fflush(stderr); _exit(rc); }
	return rc;
}

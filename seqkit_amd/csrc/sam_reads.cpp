// sam_reads.cpp — `sam to [interleaved] raw|fasta|fastq`.  A regular file goes to the device whole: it writes every record's text, window
// by window, and pairs the mates or leaves the pairing to this host (sam_pairing.h); what the device does not take is read record by
// record here, the bases through sequence() on the device.
#include <unordered_map>

#include "sam_host.h"
#include "sam_pairing.h"

// ---- sam to raw|fasta|fastq -----------------------------------------------------------------
static const char *USAGE_TO =
	"\nUsage:\n"
	"  sam to raw <bam_file> <out_prefix>\n"
	"  sam to fasta <bam_file> <out_prefix>\n"
	"  sam to fastq <bam_file> <out_prefix>\n"
	"  sam to interleaved raw <bam_file>\n"
	"  sam to interleaved fasta <bam_file>\n"
	"  sam to interleaved fastq <bam_file>\n"
	"\n"
	"These commands convert BAM files into FASTQ, FASTA, or raw sequence-per-line\n"
	"format. Both name-sorted and position-sorted BAM files are supported,\n"
	"but memory usage can reach several GB for position-sorted BAM files.\n"
	"\n"
	"Output is written into files whose name is derived based on output prefix\n"
	"and format. For example, with output format FASTQ and prefix \"sample\",\n"
	"paired end reads are written into files sample_1.fq.gz and sample_2.fq.gz,\n"
	"and orphan reads are written into sample.fq.gz.\n";

enum class OutFmt { RAW, FASTA, FASTQ };

// one of the three destinations of write_reads (:92-93): a gzip file, stdout, or io::sink()
struct ReadSink {
	std::unique_ptr<host::GzWriter> gz;
	bool to_stdout = false;
	void write(const char *p, size_t n)
	{
		if (gz) gz->write(p, n);
		else if (to_stdout) host::out().write(p, n);
	}
	void write(const std::string &s) { write(s.data(), s.size()); }
};

static bool char_boundary(const std::string &s, size_t i) { return i == s.size() || (i < s.size() && ((uint8_t)s[i] & 0xC0) != 0x80); }

static void write_read(ReadSink &out, OutFmt format, const std::string &qname, const std::string &seq)       // :138-149
{
	if (format == OutFmt::FASTQ) {
		const size_t seq_len = (seq.size() - 1) / 2;                                                          // :141
		if (!char_boundary(seq, seq_len) || !char_boundary(seq, seq_len + 1)) panic("byte index is not a char boundary");
		out.write("@", 1); out.write(qname); out.write("\n", 1);
		out.write(seq.data(), seq_len); out.write("\n+\n", 3);
		out.write(seq.data() + seq_len + 1, seq.size() - seq_len - 1); out.write("\n", 1);
	} else if (format == OutFmt::FASTA) {
		out.write(">", 1); out.write(qname); out.write("\n", 1); out.write(seq); out.write("\n", 1);
	} else {
		out.write(seq); out.write("\n", 1);
	}
}

// HashMap<Box<str>, Box<str>> (:98-99) whose leftovers are listed in insertion order (the reference's order is arbitrary)
struct PendingReads {
	struct Val { std::string seq; uint64_t order; };
	std::unordered_map<std::string, Val> map;
	uint64_t next = 0;
	void insert(const std::string &qname, std::string &&seq)
	{
		auto it = map.find(qname);
		if (it != map.end()) it->second.seq = std::move(seq);           // HashMap::insert replaces the value
		else map.emplace(qname, Val{std::move(seq), next++});
	}
	std::vector<const std::pair<const std::string, Val> *> in_order() const
	{
		std::vector<const std::pair<const std::string, Val> *> v;
		v.reserve(map.size());
		for (const auto &kv : map) v.push_back(&kv);
		std::sort(v.begin(), v.end(), [](auto a, auto b) { return a->second.order < b->second.order; });
		return v;
	}
};

static ReadSink g_sinks[3];
static void close_sinks() { for (auto &s : g_sinks) if (s.gz) s.gz->close(); }

// Where the mates of `sam to` are paired when the device serves the file: SEQKIT_HOST_PAIRING=1 on the host, SEQKIT_DEVICE_PAIRING=1 on
// the device, else kDevicePairingDefault (what was measured, and the rule the default follows: on 20 M records the
// device pairing beat the parent commit's binary by more than that binary's own spread in every run, to /dev/null and to files).
static const bool kDevicePairingDefault = true;
static bool device_pairing_wanted()
{
	if (getenv("SEQKIT_HOST_PAIRING")) return false;
	if (getenv("SEQKIT_DEVICE_PAIRING")) return true;
	return kDevicePairingDefault;
}

// sam to over the FILE.  The device inflates, walks and sizes it, pairs the mates (:113-137) and writes the texts in the order they
// leave (sk_bam_file_pairs): this host writes each window to its sink.  Where the outputs are the three files the device also deflates
// and frames them (sk_bam_file_pairs_gz), and each window's members go to their file as they are.  SEQKIT_HOST_PAIRING=1, and every file that call declines (two
// names under one key: info[5] = -94; no room for its working memory: -21), take the path before it: the device writes every kept record's text in file
// order (sk_bam_file_reads) and the pairing runs here over the windows (sam_pairing.h: pair_on_host).  -1: nothing has been written, and
// the caller's reader serves the file (one the file path does not take, a device without room, or a record the reference would panic or
// stop at).  Otherwise the number of records in the file.  noinline pins the pairing loop's code: as g++ -O2 inlined it
// into to_reads_cmd in this file, the loop measured 3.9 s of CPU for 20 M records fed from host memory; out of line, 2.6 s.
__attribute__((noinline)) static int64_t to_reads_from_file(const std::string &path, OutFmt format, bool interleaved, ReadSink &out_1, ReadSink &out_2, ReadSink &out_single)
{
	sk_ctx *c = host::gpu();
	int handled = 0;
	double info[8];
	const int fmt = format == OutFmt::RAW ? 0 : format == OutFmt::FASTA ? 1 : 2;
	ReadSink *sinks[3] = {&out_1, &out_2, &out_single};
	auto write = [&](int stream, const char *p, size_t n) { sinks[stream]->write(p, n); };
	if (device_pairing_wanted()) {
		uint64_t counts[8];
		// the three files: the device deflates and frames the texts too, and the writers take finished members (SEQKIT_GPU_DEFLATE=0: the
		// texts come back as they are and go through the writers' pool)
		const char *gd = getenv("SEQKIT_GPU_DEFLATE");
		if (!interleaved && !(gd && atoi(gd) == 0)) {
			if (sk_bam_file_pairs_gz(c, path.c_str(), fmt, 10 /* :103 */, 1, file_window_bytes(), counts, &handled, info) == SK_OK && handled) {
				if (bamfile_trace()) fprintf(stderr, "sam to pairing: device\nsam to deflate: device\n");
				pairing::write_member_windows([&](sk_bam_pairs_gz_window *w) { check(sk_bam_file_pairs_gz_next(c, w), "sk_bam_file_pairs_gz_next"); },
				                              [&](int stream, const uint8_t *p, size_t n) { sinks[stream]->gz->write_members(p, n); });
				return (int64_t)info[3];
			}
		} else if (sk_bam_file_pairs(c, path.c_str(), fmt, 10 /* :103 */, interleaved ? 1 : 0, file_window_bytes(), counts, &handled, info) == SK_OK && handled) {
			if (bamfile_trace()) fprintf(stderr, "sam to pairing: device\n");
			pairing::write_pair_windows([&](sk_bam_pairs_window *w) { check(sk_bam_file_pairs_next(c, w), "sk_bam_file_pairs_next"); }, write);
			return (int64_t)info[3];
		}
		if (info[5] != -94.0 && info[5] != -21.0) return -1;            // (declined as sk_bam_file_reads would: not inflated a second time)
	}
	int64_t n_kept = 0;
	uint64_t text_bytes = 0;
	if (sk_bam_file_reads(c, path.c_str(), fmt, 10 /* :103 */, interleaved ? 0 : 1, file_window_bytes(), &n_kept, &text_bytes, &handled, info) != SK_OK || !handled) return -1;
	if (bamfile_trace()) fprintf(stderr, "sam to pairing: host\n");
	pairing::pair_on_host([&](sk_bam_reads_window *w) { check(sk_bam_file_reads_next(c, w), "sk_bam_file_reads_next"); }, write);
	return (int64_t)info[3];
}

int to_reads_cmd(int argc, char **argv)
{
	const bool interleaved = argc >= 4 && strcmp(argv[2], "interleaved") == 0;
	const char *fmtw = argv[interleaved ? 3 : 2];
	std::vector<host::Opt> opts;
	std::vector<std::string> pos;
	if (!host::parse_args(argc, argv, interleaved ? 4 : 3, opts, pos, 2) || pos.size() != (interleaved ? 1u : 2u)) error("Invalid arguments.\n%s", USAGE_TO);
	const OutFmt format = !strcmp(fmtw, "raw") ? OutFmt::RAW : !strcmp(fmtw, "fasta") ? OutFmt::FASTA : OutFmt::FASTQ;      // :68-71
	ReadSink &out_1 = g_sinks[0], &out_2 = g_sinks[1], &out_single = g_sinks[2];
	if (interleaved) { out_1.to_stdout = true; out_2.to_stdout = true; }                                    // :74-78
	else {                                                                                                   // :79-86
		const char *ext = format == OutFmt::RAW ? "seq" : format == OutFmt::FASTA ? "fa" : "fq";
		out_1.gz.reset(new host::GzWriter(pos[1] + "_1." + ext + ".gz"));
		out_2.gz.reset(new host::GzWriter(pos[1] + "_2." + ext + ".gz"));
		out_single.gz.reset(new host::GzWriter(pos[1] + "." + ext + ".gz"));
		host::at_exit_flush(close_sinks);
	}
	host::gpu_warmup();
	if (device_path("sam to", pos[0], [&] { return to_reads_from_file(pos[0], format, interleaved, out_1, out_2, out_single); }) >= 0) {
		close_sinks();
		return 0;
	}
	BamStream bam(pos[0]);                                                                                   // :96
	PendingReads reads_1, reads_2;

	// a batch of primary records: their bases go through sequence() on the device (:31-59), the rest is text
	struct Rec { std::string qname; uint16_t flag; uint32_t l_seq; size_t off4, offq; };
	std::vector<Rec> recs;
	std::vector<uint8_t> body, raw4, rawq, m4, mq, mout;
	std::vector<uint16_t> lens, flags;
	const size_t kBatchBytes = 48u << 20;
	BamCore c;
	BamStream::Var v;
	bool more = true;
	std::string read_seq;
	while (more) {
		recs.clear(); raw4.clear(); rawq.clear();
		uint32_t max_len = 0;
		while ((more = bam.next_full(c, v, body))) {                                                         // :101
			if ((c.flag & 0x100) || (c.flag & 0x800)) continue;                                              // :102
			if (v.l_seq > 65532) error("Read longer than 65532 bases: not supported by this build.");
			Rec r;
			r.qname.assign(reinterpret_cast<const char *>(body.data()), v.l_read_name - 1);                  // rust-htslib qname(): without the final NUL
			r.flag = c.flag;
			r.l_seq = v.l_seq;
			const uint8_t *seq4 = body.data() + v.l_read_name + 4 * (size_t)v.n_cigar, *qual = seq4 + (v.l_seq + 1) / 2;
			r.off4 = raw4.size(); r.offq = rawq.size();
			raw4.insert(raw4.end(), seq4, seq4 + (v.l_seq + 1) / 2);
			rawq.insert(rawq.end(), qual, qual + v.l_seq);
			recs.push_back(std::move(r));
			max_len = std::max(max_len, v.l_seq);
			if ((recs.size() + 1) * (size_t)(((max_len + 7) & ~7u) + 4) * 3 > kBatchBytes) break;
		}
		const size_t n = recs.size();
		if (n == 0) continue;
		// row pitch: a multiple of 8, so that sequence() runs as its eight-bytes-per-thread kernel whatever the read length
		// (reads within 4 bases of the C-ABI's 65 532 keep the multiple of 4)
		const size_t stride8 = std::max<size_t>(8, (max_len + 7) & ~(size_t)7);
		const size_t stride = stride8 <= 65532 ? stride8 : std::max<size_t>(4, (max_len + 3) & ~(size_t)3), stride4 = std::max<size_t>(4, (stride / 2 + 3) & ~(size_t)3);
		m4.assign(n * stride4, 0); mq.assign(n * stride, 0); mout.resize(n * stride);
		lens.resize(n); flags.resize(n);
		for (size_t i = 0; i < n; i++) {
			memcpy(m4.data() + i * stride4, raw4.data() + recs[i].off4, (recs[i].l_seq + 1) / 2);
			memcpy(mq.data() + i * stride, rawq.data() + recs[i].offq, recs[i].l_seq);
			lens[i] = (uint16_t)recs[i].l_seq;
			flags[i] = recs[i].flag;
		}
		check(sk_bam_sequence(host::gpu(), m4.data(), (int)stride4, mq.data(), (int)stride, lens.data(), flags.data(), (int64_t)n, 10 /* :105 */, mout.data()),
		      "sk_bam_sequence");
		for (size_t i = 0; i < n; i++) {
			const Rec &r = recs[i];
			if (!host::utf8_valid(reinterpret_cast<const uint8_t *>(r.qname.data()), r.qname.size())) {     // :104 str::from_utf8(..).unwrap()
				close_sinks();
				panic("called `Result::unwrap()` on an `Err` value: Utf8Error");
			}
			read_seq.assign(reinterpret_cast<const char *>(mout.data() + i * stride), r.l_seq);
			if (format == OutFmt::FASTQ) {                                                                   // :107-112
				read_seq.push_back('|');
				const uint8_t *q = rawq.data() + r.offq;
				// qualities below 95 (all real ones) are one ASCII byte each: add 33 to the whole row at once; a row with a
				// larger value takes the byte-by-byte form of char::from(u8)
				const size_t at = read_seq.size();
				read_seq.resize(at + r.l_seq);
				uint8_t high = 0;
				for (uint32_t k = 0; k < r.l_seq; k++) {
					const uint8_t ch = (uint8_t)(33 + q[k]);                                                 // u8 arithmetic wraps (release build)
					read_seq[at + k] = (char)ch;
					high |= ch;
				}
				if (high & 0x80) {
					read_seq.resize(at);
					for (uint32_t k = 0; k < r.l_seq; k++) {
						const uint8_t ch = (uint8_t)(33 + q[k]);
						if (ch < 0x80) read_seq.push_back((char)ch);
						else { read_seq.push_back((char)(0xC0 | (ch >> 6))); read_seq.push_back((char)(0x80 | (ch & 0x3F))); }   // char::from(u8) as UTF-8
					}
				}
			}
			if (!(r.flag & 0x1)) {                                                                           // :114-115
				write_read(out_single, format, r.qname, read_seq);
			} else if (r.flag & 0x40) {                                                                      // :116-122
				auto it = reads_2.map.find(r.qname);
				if (it != reads_2.map.end()) {
					write_read(out_1, format, r.qname, read_seq);
					write_read(out_2, format, r.qname, it->second.seq);
					reads_2.map.erase(it);
				} else reads_1.insert(r.qname, std::string(read_seq));
			} else if (r.flag & 0x80) {                                                                      // :123-130
				auto it = reads_1.map.find(r.qname);
				if (it != reads_1.map.end()) {
					write_read(out_1, format, r.qname, it->second.seq);
					write_read(out_2, format, r.qname, read_seq);
					reads_1.map.erase(it);
				} else reads_2.insert(r.qname, std::string(read_seq));
			}
		}
	}
	bam.raise_deferred();
	for (const PendingReads *m : {&reads_1, &reads_2})                                                       // :133-137
		for (const auto *kv : m->in_order()) write_read(out_single, format, kv->first, kv->second.seq);
	close_sinks();
	return 0;
}

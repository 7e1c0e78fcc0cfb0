// pairing_test.cpp — sam_pairing.h without a device: the host pairing over windows of file-order texts (pair_on_host, the path behind
// SEQKIT_HOST_PAIRING=1 and the fallback when sk_bam_file_pairs declines) against the loop of src/sam_to_fastq.rs:113-137 written with
// std::map, and the window loop of the device-paired path (write_pair_windows) over windows cut from that loop's outputs.  Built with
// -fsanitize=address,undefined by tests/test_pairing_cpu.py; the window arrays are heap blocks of exactly their size.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "sam_pairing.h"

struct Rec { uint8_t kind; std::string name, text; };

static uint64_t rnd_state = 88172645463325252ull;
static uint64_t rnd() { rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17; return rnd_state; }

// the reference's loop: map name -> (text, insertion order); leftovers in insertion order
static void reference(const std::vector<Rec> &recs, std::string out[3])
{
	struct Val { std::string text; uint64_t order; };
	std::map<std::string, Val> m1, m2;
	uint64_t n1 = 0, n2 = 0;
	for (const Rec &r : recs) {
		if (r.kind == 0) { out[2] += r.text; continue; }
		auto &mates = r.kind == 1 ? m2 : m1;
		auto &mine = r.kind == 1 ? m1 : m2;
		uint64_t &next = r.kind == 1 ? n1 : n2;
		auto it = mates.find(r.name);
		if (it != mates.end()) {
			out[0] += r.kind == 1 ? r.text : it->second.text;
			out[1] += r.kind == 1 ? it->second.text : r.text;
			mates.erase(it);
		} else {
			auto f = mine.find(r.name);
			if (f != mine.end()) f->second.text = r.text;
			else mine.emplace(r.name, Val{r.text, next++});
		}
	}
	for (auto *m : {&m1, &m2}) {
		std::map<uint64_t, const Val *> by_order;
		for (const auto &kv : *m) by_order[kv.second.order] = &kv.second;
		for (const auto &kv : by_order) out[2] += kv.second->text;
	}
}

// the records as windows of sk_bam_file_reads: `per` records each, every array a heap block of exactly its size
struct ReadsFeed {
	const std::vector<Rec> &recs;
	size_t per, at = 0;
	uint64_t (*key_of)(const std::string &);
	std::unique_ptr<uint8_t[]> text, names, kind;
	std::unique_ptr<uint64_t[]> toff, key;
	std::unique_ptr<uint32_t[]> noff;
	void operator()(sk_bam_reads_window *w)
	{
		memset(w, 0, sizeof *w);
		const size_t n = std::min(per, recs.size() - at);
		if (n == 0) return;
		size_t tb = 0, nb = 0;
		for (size_t j = 0; j < n; j++) { tb += recs[at + j].text.size(); nb += recs[at + j].name.size(); }
		text.reset(new uint8_t[tb ? tb : 1]); names.reset(new uint8_t[nb ? nb : 1]); kind.reset(new uint8_t[n]);
		toff.reset(new uint64_t[n + 1]); key.reset(new uint64_t[n]); noff.reset(new uint32_t[n + 1]);
		tb = nb = 0;
		for (size_t j = 0; j < n; j++) {
			const Rec &r = recs[at + j];
			toff[j] = tb; noff[j] = (uint32_t)nb; kind[j] = r.kind; key[j] = key_of(r.name);
			memcpy(text.get() + tb, r.text.data(), r.text.size()); tb += r.text.size();
			memcpy(names.get() + nb, r.name.data(), r.name.size()); nb += r.name.size();
		}
		toff[n] = tb; noff[n] = (uint32_t)nb;
		w->first = (int64_t)at; w->n = (int64_t)n;
		w->text = text.get(); w->text_off = toff.get(); w->kind = kind.get(); w->key = key.get(); w->names = names.get(); w->name_off = noff.get();
		at += n;
	}
};

// the three outputs as windows of sk_bam_file_pairs: `per` bytes each (a window of the real call ends at a record; the loop does not care)
struct PairsFeed {
	const std::string *out;
	size_t per;
	int stream = 0;
	size_t at = 0;
	std::unique_ptr<uint8_t[]> text;
	void operator()(sk_bam_pairs_window *w)
	{
		memset(w, 0, sizeof *w);
		while (stream < 3 && at == out[stream].size()) { stream++; at = 0; }
		if (stream == 3) return;
		const size_t n = std::min(per, out[stream].size() - at);
		text.reset(new uint8_t[n]);
		memcpy(text.get(), out[stream].data() + at, n);
		w->stream = stream; w->first = (int64_t)at; w->n = 1; w->text = text.get(); w->bytes = n;
		at += n;
	}
};

static uint64_t good_key(const std::string &s) { uint64_t h = 1469598103934665603ull; for (char ch : s) h = (h ^ (uint8_t)ch) * 1099511628211ull; return h; }
static uint64_t poor_key(const std::string &s) { return s.size() % 3; }      // names collide under it all the time: compared byte for byte

static int failures = 0;
static void run(const std::vector<Rec> &recs, size_t per, uint64_t (*key_of)(const std::string &), const char *what)
{
	std::string exp[3], got[3], again[3];
	reference(recs, exp);
	ReadsFeed feed{recs, per, 0, key_of, {}, {}, {}, {}, {}, {}};
	pairing::pair_on_host([&](sk_bam_reads_window *w) { feed(w); }, [&](int s, const char *p, size_t n) { got[s].append(p, n); });
	PairsFeed pf{exp, per * 7 + 1, 0, 0, {}};
	pairing::write_pair_windows([&](sk_bam_pairs_window *w) { pf(w); }, [&](int s, const char *p, size_t n) { again[s].append(p, n); });
	for (int s = 0; s < 3; s++)
		if (got[s] != exp[s] || again[s] != exp[s]) { fprintf(stderr, "%s, %zu per window: stream %d differs\n", what, per, s); failures++; }
}

int main()
{
	std::vector<Rec> recs;
	for (int i = 0; i < 30000; i++) {                                     // names that come 1 to 6 times, kinds at random, mates near and far
		const uint64_t r = rnd();
		const int id = (int)(r % 9000);
		Rec x;
		x.kind = (uint8_t)((r >> 20) % 8 == 0 ? 0 : 1 + ((r >> 24) & 1));
		x.name = (id % 5 == 0 ? "n" : "name:") + std::to_string(id % 50 == 0 ? id / 50 : id);
		x.text = "@" + x.name + "/" + std::to_string(i) + std::string((size_t)((r >> 32) % 40), 'A' + (char)(i % 26)) + "\n";
		recs.push_back(x);
	}
	for (size_t per : {(size_t)1, (size_t)7, (size_t)1000, recs.size()}) run(recs, per, good_key, "mixed names");
	run(recs, 64, poor_key, "colliding keys");
	std::vector<Rec> one;                                                 // one name on every record
	for (int i = 0; i < 4096; i++) one.push_back(Rec{(uint8_t)(1 + (i / 3) % 2), "same", std::to_string(i) + "\n"});
	run(one, 100, good_key, "one name");
	run({}, 5, good_key, "no records");
	run({Rec{0, "", "\n"}, Rec{1, "", "x\n"}, Rec{2, "", ""}}, 2, good_key, "empty name and text");
	if (failures) return 1;
	printf("ok: %zu records\n", recs.size());
	return 0;
}

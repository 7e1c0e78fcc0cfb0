// sk_capi_comm.hip — the C-ABI of include/seqkit_hip.h, the count reduce across GPUs: the RCCL loader, the communicators of
// sk_comm_*, sk_allreduce_u64_dev and sk_counts_allreduce.
#include <dlfcn.h>
#include <unistd.h>

#include <mutex>

#include "sk_ctx.h"

// ---- (e) the count reduce over RCCL ---------------------------------------------------------------------------
// librccl is 570 MB: the command-line hosts must not pay for loading it unless they drive several GPUs, so it is
// dlopen'ed on first use (the same SONAME torch loads, so a process that has torch in it shares its copy).
namespace {
struct Rccl {
	void *h = nullptr;
	decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
	decltype(&ncclCommInitRank) CommInitRank = nullptr;
	decltype(&ncclCommInitAll) CommInitAll = nullptr;
	decltype(&ncclCommDestroy) CommDestroy = nullptr;
	decltype(&ncclAllReduce) AllReduce = nullptr;
	decltype(&ncclGroupStart) GroupStart = nullptr;
	decltype(&ncclGroupEnd) GroupEnd = nullptr;
	decltype(&ncclGetErrorString) GetErrorString = nullptr;
	std::string err;
};

Rccl *rccl()
{
	static Rccl r;
	static std::once_flag once;
	std::call_once(once, [] {
		const char *names[] = {getenv("SK_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
		for (const char *nm : names) {
			if (!nm || !*nm) continue;
			r.h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
			if (r.h) break;
			r.err = dlerror();
		}
		if (!r.h) return;
		bool ok = true;
		auto sym = [&](const char *nm) { void *p = dlsym(r.h, nm); if (!p) { ok = false; r.err = std::string("missing symbol ") + nm; } return p; };
		r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
		r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
		r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
		r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
		r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
		r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
		r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
		r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
		if (!ok) { dlclose(r.h); r.h = nullptr; }
	});
	return &r;
}

// communicators of one process over a set of devices (ncclCommInitAll), made once per device list
struct LocalComms { std::vector<int> devs; std::vector<ncclComm_t> comms; };
std::mutex g_local_m;
std::vector<LocalComms> g_local;

__global__ void counts_add_kernel(unsigned long long *dst, const unsigned long long *src, int n)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) dst[i] += src[i];
}
}  // namespace

// RCCL announces itself on stdout when a communicator comes up (version banner).  stdout belongs to the host's results
// (the reference's commands print there), so while a communicator is being made fd 1 points at stderr, and what stdio
// buffered during that time is flushed there before fd 1 is put back.
// fd 1 is process-wide state: one redirection at a time (two callers could otherwise put each other's descriptor back),
// and only the calls that make a communicator take it — a host thread that prints a result at that very moment would see
// it on stderr, which is why the command-line hosts make their communicators before their workers start.
// The lock is held only around the descriptor swaps, never across the RCCL call: two ranks of ONE process joining from two
// threads both block in the bootstrap until the other has arrived — the first redirection stays in place (a count) until the
// last of them is back.
static std::mutex g_stdout_m;
static int g_stdout_depth = 0, g_stdout_saved = -1;
struct StdoutToStderr {
	StdoutToStderr()
	{
		std::lock_guard<std::mutex> lk(g_stdout_m);
		if (g_stdout_depth++ == 0) { fflush(stdout); g_stdout_saved = dup(1); if (g_stdout_saved >= 0) (void)dup2(2, 1); }
	}
	~StdoutToStderr()
	{
		std::lock_guard<std::mutex> lk(g_stdout_m);
		if (--g_stdout_depth == 0) { fflush(stdout); if (g_stdout_saved >= 0) { (void)dup2(g_stdout_saved, 1); close(g_stdout_saved); g_stdout_saved = -1; } }
	}
};

#define SK_NCCL(c, call)                                                                                  \
	do {                                                                                                  \
		ncclResult_t r_ = (call);                                                                         \
		if (r_ != ncclSuccess) return fail((c), SK_ERR_COMM, "%s: %s", #call, rccl()->GetErrorString(r_)); \
	} while (0)

static int rccl_ready(sk_ctx *c)
{
	Rccl *r = rccl();
	if (!r->h) return fail(c, SK_ERR_COMM, "librccl.so.1 cannot be loaded (%s): the count reduce across GPUs needs RCCL", r->err.c_str());
	return SK_OK;
}

extern "C" {

// A rank-local check that needs no other rank: can this ctx take part in an RCCL communicator at all (library loadable,
// device bindable)?  Hosts gather the answers of all ranks BEFORE any of them enters the blocking bootstrap.
int sk_comm_ready(sk_ctx *c)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = rccl_ready(c)) return r;
	return bind(c);
}

int sk_comm_get_unique_id(uint8_t id[SK_COMM_ID_BYTES])
{
	static_assert(SK_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
	if (!id) return SK_ERR_INVALID;
	if (int r = rccl_ready(nullptr)) return r;
	ncclUniqueId u;
	StdoutToStderr quiet;
	SK_NCCL(nullptr, rccl()->GetUniqueId(&u));
	memcpy(id, u.internal, SK_COMM_ID_BYTES);
	return SK_OK;
}

int sk_comm_init_rank(sk_ctx *c, const uint8_t id[SK_COMM_ID_BYTES], int rank, int n_ranks)
{
	if (!c || !id) return SK_ERR_INVALID;
	if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(c, SK_ERR_INVALID, "rank %d of %d", rank, n_ranks);
	if (c->comm) return fail(c, SK_ERR_STATE, "this ctx already has a communicator");
	if (int r = rccl_ready(c)) return r;
	if (int r = bind(c)) return r;
	ncclUniqueId u;
	memcpy(u.internal, id, SK_COMM_ID_BYTES);
	StdoutToStderr quiet;
	SK_NCCL(c, rccl()->CommInitRank(&c->comm, n_ranks, u, rank));
	c->comm_ranks = n_ranks;
	return SK_OK;
}

int sk_comm_destroy(sk_ctx *c)
{
	if (!c) return SK_ERR_INVALID;
	if (!c->comm) return SK_OK;
	(void)hipSetDevice(c->device);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	ncclResult_t r = rccl()->CommDestroy(c->comm);
	c->comm = nullptr; c->comm_ranks = 0;
	return r == ncclSuccess ? SK_OK : fail(c, SK_ERR_COMM, "ncclCommDestroy: %s", rccl()->GetErrorString(r));
}

int sk_allreduce_u64_dev(sk_ctx *c, uint64_t *buf, size_t count)
{
	if (!c || (count && !buf)) return SK_ERR_INVALID;
	if (!c->comm || c->comm_ranks <= 1 || count == 0) return SK_OK;          // a world of one
	if (int r = bind(c)) return r;
	SK_NCCL(c, rccl()->AllReduce(buf, buf, count, ncclUint64, ncclSum, c->comm, c->stream));
	return SK_OK;
}

int sk_counts_allreduce(sk_ctx **ctxs, int n_ctx)
{
	if (!ctxs || n_ctx < 1) return SK_ERR_INVALID;
	for (int i = 0; i < n_ctx; i++) if (!ctxs[i]) return SK_ERR_INVALID;
	sk_ctx *c0 = ctxs[0];
	for (int i = 0; i < n_ctx; i++) {
		if (!ctxs[i]->bar.have_table) return fail(c0, SK_ERR_STATE, "ctx %d: sk_set_barcodes has not been called", i);
		if (ctxs[i]->bar.S != c0->bar.S) return fail(c0, SK_ERR_INVALID, "ctx %d has %d samples, ctx 0 has %d", i, ctxs[i]->bar.S, c0->bar.S);
	}
	const int nc = c0->bar.S + 3;
	for (int i = 0; i < n_ctx; i++) {
		if (int r = bind(ctxs[i])) return r;
		if (int r = sk::fold_counts(ctxs[i])) return r;
	}
	if (n_ctx == 1) return sk_allreduce_u64_dev(c0, (uint64_t *)c0->bar.d_counts.get(), (size_t)nc);     // across ranks (or nothing to do)
	for (int i = 0; i < n_ctx; i++)
		if (ctxs[i]->comm) return fail(c0, SK_ERR_STATE, "ctx %d belongs to a one-process-per-GPU communicator: reduce it alone", i);

	// 1. everything enqueued so far must have happened before another stream reads the counters
	for (int i = 0; i < n_ctx; i++) { SK_HIP(c0, hipSetDevice(ctxs[i]->device)); SK_HIP(c0, hipStreamSynchronize(ctxs[i]->stream)); }
	// 2. ctxs that share a device: summed on that device into the first of them (its "leader")
	std::vector<int> leader_of(n_ctx), leaders;
	for (int i = 0; i < n_ctx; i++) {
		int l = -1;
		for (int k : leaders) if (ctxs[k]->device == ctxs[i]->device) { l = k; break; }
		if (l < 0) { leaders.push_back(i); l = i; }
		leader_of[i] = l;
	}
	for (int i = 0; i < n_ctx; i++) {
		const int l = leader_of[i];
		if (l == i) continue;
		SK_HIP(c0, hipSetDevice(ctxs[l]->device));
		counts_add_kernel<<<(nc + 255) / 256, 256, 0, ctxs[l]->stream>>>(ctxs[l]->bar.d_counts.get(), ctxs[i]->bar.d_counts.get(), nc);
		SK_HIP(c0, hipGetLastError());
	}
	// 3. distinct devices: one RCCL all-reduce (sum, u64) on the leaders' streams
	if (leaders.size() > 1) {
		if (int r = rccl_ready(c0)) return r;
		std::vector<int> devs;
		for (int k : leaders) devs.push_back(ctxs[k]->device);
		std::vector<ncclComm_t> comms;
		// the communicators of a device set are shared by every caller that reduces over it: the lock is held from their
		// lookup to the end of the grouped call, so two threads never interleave their operations on one ncclComm
		std::lock_guard<std::mutex> lk(g_local_m);
		{
			for (const LocalComms &lc : g_local) if (lc.devs == devs) { comms = lc.comms; break; }
			if (comms.empty()) {
				comms.resize(devs.size());
				StdoutToStderr quiet;
				SK_NCCL(c0, rccl()->CommInitAll(comms.data(), (int)devs.size(), devs.data()));
				g_local.push_back({devs, comms});
			}
		}
		SK_NCCL(c0, rccl()->GroupStart());
		for (size_t k = 0; k < leaders.size(); k++) {
			sk_ctx *l = ctxs[leaders[k]];
			(void)hipSetDevice(l->device);                         // each rank's call with its own device current
			ncclResult_t r = rccl()->AllReduce(l->bar.d_counts.get(), l->bar.d_counts.get(), (size_t)nc, ncclUint64, ncclSum, comms[k], l->stream);
			if (r != ncclSuccess) { (void)rccl()->GroupEnd(); return fail(c0, SK_ERR_COMM, "ncclAllReduce: %s", rccl()->GetErrorString(r)); }
		}
		SK_NCCL(c0, rccl()->GroupEnd());
	}
	// 4. the totals back to the ctxs that share a leader's device
	for (int i = 0; i < n_ctx; i++) {
		const int l = leader_of[i];
		if (l == i) continue;
		SK_HIP(c0, hipSetDevice(ctxs[l]->device));
		SK_HIP(c0, hipMemcpyAsync(ctxs[i]->bar.d_counts.get(), ctxs[l]->bar.d_counts.get(), (size_t)nc * 8, hipMemcpyDeviceToDevice, ctxs[l]->stream));
	}
	for (int k : leaders) { SK_HIP(c0, hipSetDevice(ctxs[k]->device)); SK_HIP(c0, hipStreamSynchronize(ctxs[k]->stream)); }
	return SK_OK;
}

}  // extern "C"

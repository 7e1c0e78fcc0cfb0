// sk_ctx.h — the context of the C-ABI units (sk_capi_*.cpp, sk_capi_comm.hip): the struct, the owner of its buffers, and what every
// entry point starts with (fail, bind, SK_HIP, the workspace, the chunk pipeline of the host-pointer forms).  Internal to the library,
// and to those units: the file calls (sk_bamfile*.cpp) go through the sk::ctx_* accessors of sk_internal.h.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and prototypes only: librccl is loaded with dlopen on first use (sk_capi_comm.hip)

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/seqkit_hip.h"
#include "sk_internal.h"
#include "sk_hoststage.h"

namespace sk {
// The owner of one device or page-locked host allocation: freed when it is reset, allocated over, moved over or destroyed, and nowhere
// else.  A failed alloc() leaves it empty and does not stay as the runtime's sticky last error.
template <class T>
struct DevMem {
	T *p = nullptr;
	bool pinned = false;
	DevMem() = default;
	DevMem(DevMem &&o) noexcept : p(o.p), pinned(o.pinned) { o.p = nullptr; }
	DevMem &operator=(DevMem &&o) noexcept { if (this != &o) { reset(); p = o.p; pinned = o.pinned; o.p = nullptr; } return *this; }
	~DevMem() { reset(); }
	T *get() const { return p; }
	explicit operator bool() const { return p != nullptr; }
	void reset() { if (p) { if (pinned) (void)hipHostFree(p); else (void)hipFree(p); p = nullptr; } }
	hipError_t alloc(size_t bytes, bool pin = false)
	{
		reset();
		pinned = pin;
		const hipError_t e = pin ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes);
		if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
		return e;
	}
};

// The streams and events of a ctx.  A base of sk_ctx, so that they are destroyed after every member: after every buffer is freed.
struct CtxLanes {
	hipStream_t stream = nullptr;
	hipStream_t stream2 = nullptr;     // second lane of the host entry points' chunk pipeline (H2D of chunk i+1 under kernel / D2H of chunk i)
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_pipe = nullptr;
	~CtxLanes()
	{
		if (ev0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
		if (ev_pipe) (void)hipEventDestroy(ev_pipe);
		if (stream2) (void)hipStreamDestroy(stream2);
		if (stream) (void)hipStreamDestroy(stream);
	}
};
}  // namespace sk

static constexpr int kManySlots = 8, kManyMax = 256;     // sk_fused_pass_many_dev: descriptor slots in the ring, batches per launch

// Each nested struct is one domain's state, read and written by one unit; a setter starts from `= {}`, which frees what the last one left.
struct sk_ctx : sk::CtxLanes {
	int device = 0;
	int n_cu = 256;
	std::string err;
	struct Barcodes {                      // sk_capi_barcodes.cpp: the table of sk_set_barcodes and the counters
		bool have_table = false;
		int S = 0, L = 0, W = 0, max_diff = 1;
		sk::DevMem<uint8_t> d_raw;
		sk::DevMem<uint32_t> d_onehot;
		sk::DevMem<uint8_t> d_lut;
		sk::DevMem<uint8_t> d_bs;
		int bs_bytes = 0, bs_mm_off = 0, G = 0;
		sk::DevMem<uint8_t> d_nbr;         // neighbourhood table of the sheet (sk_lut.h, demux_lut_kernel), when it has one: slots, then the ambiguity pairs
		sk::LutDev nbr{};
		std::vector<uint8_t> sheet;        // the sheet as given to sk_set_barcodes (the table is built from it on first use)
		bool nbr_tried = false;
		int64_t nbr_keys = 0, nbr_bytes = 0;
		sk::DevMem<unsigned long long> d_counts;        // u64[S+3]
		sk::DevMem<unsigned long long> d_counts_wide;   // TileArgs::counts_wide: 16 x (S+3) lines; folded into d_counts by fold_counts()
		bool wide_dirty = false;
		sk::DevMem<unsigned long long> d_count_rep;     // BarcodeDev::count_rep
		int count_rep_pitch = 0;
		size_t count_rep_set = 0;                       // u64 words of one set
	} bar;
	int detail_mode = SK_DETAIL_FULL;      // (sk_set_detail_mode: stays from one sheet to the next)
	// workspace for the host-pointer entry points
	sk::DevMem<uint8_t> ws;
	size_t ws_bytes = 0;
	// sk_fused_pass_many_dev: the batch descriptors of a many-batch launch travel through a ring of pinned slots
	struct Many {
		sk::DevMem<sk::ManyBatch> pin;
		hipEvent_t ev[kManySlots] = {};
		int next = 0;
		~Many() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
	} many;
	// buffers that stay with the ctx from one call to the next (sk::ctx_keep; sk_internal.h: sk::KeepSlot)
	struct Kept { sk::DevMem<void> m; size_t cap = 0; } kept[sk::kKeepSlots];
	void *ext = nullptr;               // an object another translation unit keeps with the ctx (sk_bamfile.h: Ranges, the file calls' mapped ranges and window state), and how to free it
	void (*ext_free)(void *) = nullptr;
	sk::Census *census = nullptr;
	ncclComm_t comm = nullptr;         // one-process-per-GPU communicator (sk_comm_init_rank)
	int comm_ranks = 0;
	struct Genome {                        // `fasta gc content`: the genome, resident
		sk::DevMem<uint8_t> d;
		int64_t len = 0;
	} genome;
	struct CountRegions {                  // `sam count` region tables
		int n_chr = 0;
		int64_t n_regions = 0;
		sk::DevMem<uint8_t> d;             // one allocation: chr_off, rstart, rend, rpmax, ridx, counts
		int32_t *chr_off = nullptr, *ridx = nullptr;
		uint32_t *rstart = nullptr, *rend = nullptr, *rpmax = nullptr, *region_frags = nullptr;
	} cnt;
	struct TargetRegions {                 // `sam statistics --on-target` region tables and counters
		int n_chr = 0;
		sk::DevMem<uint8_t> d;             // one allocation: chr_off, rstart, rpmax, the six counters
		int32_t *chr_off = nullptr;
		int64_t *rstart = nullptr, *rpmax = nullptr;
		unsigned long long *counters = nullptr;
	} ot;
};

namespace sk { extern thread_local std::string g_create_err; }      // sk_capi_ctx.cpp: what sk_last_error(NULL) says

static int fail(sk_ctx *c, int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	if (c) c->err = buf; else sk::g_create_err = buf;
	return code;
}

#define SK_HIP(c, call)                                                                            \
	do {                                                                                           \
		hipError_t e_ = (call);                                                                    \
		if (e_ != hipSuccess) return fail((c), SK_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
	} while (0)

static int bind(sk_ctx *c)
{
	SK_HIP(c, hipSetDevice(c->device));
	return SK_OK;
}

static int ensure_ws(sk_ctx *c, size_t bytes)
{
	if (bytes <= c->ws_bytes) return SK_OK;
	if (c->ws) { SK_HIP(c, hipStreamSynchronize(c->stream)); c->ws.reset(); c->ws_bytes = 0; }
	size_t want = bytes + (bytes >> 2);
	hipError_t e = c->ws.alloc(want);
	if (e != hipSuccess) { want = bytes; e = c->ws.alloc(want); }
	if (e != hipSuccess) return fail(c, SK_ERR_NOMEM, "device workspace of %zu bytes: %s", want, hipGetErrorString(e));
	c->ws_bytes = want;
	return SK_OK;
}

// The sheet's table as the kernels take it, and the fold of the wide counters that everything which reads or hands out the ctx's
// counters starts with (sk_capi_barcodes.cpp)
namespace sk {
BarcodeDev table_of(const sk_ctx *c);
int fold_counts(sk_ctx *c);
int ensure_neighbour_table(sk_ctx *c);
}  // namespace sk

// The host-pointer entry points cut a batch into chunks and run them as a two-deep software pipeline: chunk k uses
// stream (k & 1) and half (k & 1) of the workspace, so the H2D copies of chunk k+1 run under the kernel and the D2H
// copies of chunk k, and a half is reused only by the next chunk of the SAME stream (in order: no hazard).  Copies are
// true DMA when the caller's buffers are pinned (sk_malloc_pinned); pageable buffers work too, staged by the runtime.
// What a chunk stages is stated once per call, as a hoststage::Stage (sk_hoststage.h): begin() sizes the workspace from it, stage_in()
// carves the lane's half and queues the H2D copies of rows [r0, r0 + nr), stage_out() queues the D2H copies behind the launch.
using namespace hoststage;
struct ChunkPipe {
	sk_ctx *c;
	Stage &s;
	int64_t n = 0, r0 = 0, nr = 0;                             // the batch's rows; the chunk at hand is [r0, r0 + nr)
	int k = 0;
	ChunkPipe(sk_ctx *ctx, Stage &stage) : c(ctx), s(stage) {}
	int begin(int64_t rows, int64_t chunk, size_t shared_tail = 0)
	{
		s.plan(chunk, shared_tail);
		n = rows; nr = s.rows_at(0, n);
		if (int r = ensure_ws(c, s.total())) return r;
		SK_HIP(c, hipEventRecord(c->ev_pipe, c->stream));          // the second lane starts after whatever the ctx stream holds
		SK_HIP(c, hipStreamWaitEvent(c->stream2, c->ev_pipe, 0));
		return SK_OK;
	}
	bool more() const { return r0 < n; }
	void next() { k++; r0 += s.chunk(); nr = s.rows_at(r0, n); }
	hipStream_t st() const { return (k & 1) ? c->stream2 : c->stream; }
	uint8_t *ws() const { return c->ws.get() + (size_t)(k & 1) * s.half(); }
	uint8_t *tail() const { return c->ws.get() + s.tail_at(); }      // behind the two halves, used by every chunk (accumulators)
	int copies(Dir dir) const
	{
		hipError_t e = hipSuccess;
		s.each_copy(dir, r0, nr, [&](size_t at, uint8_t *host, size_t bytes) {
			if (e != hipSuccess) return;
			e = dir == kIn ? hipMemcpyAsync(ws() + at, host, bytes, hipMemcpyHostToDevice, st()) : hipMemcpyAsync(host, ws() + at, bytes, hipMemcpyDeviceToHost, st());
		});
		if (e != hipSuccess) return fail(c, SK_ERR_HIP, "hipMemcpyAsync (%s): %s", dir == kIn ? "host to device" : "device to host", hipGetErrorString(e));
		return SK_OK;
	}
	int stage_in() const { s.carve(ws()); return copies(kIn); }
	int stage_out() const { return copies(kOut); }
	int end()
	{
		SK_HIP(c, hipStreamSynchronize(c->stream2));
		SK_HIP(c, hipStreamSynchronize(c->stream));
		return SK_OK;
	}
};
static const size_t kPipeChunkBytes = 48u << 20;
// chunk sizes of the host entry points; SK_HOST_CHUNK_LOG2 (read per call) shrinks every one of them to 2^k bytes / records,
// so that tests walk many chunks, both lanes and both workspace halves with small inputs
static size_t pipe_chunk(size_t dflt)
{
	if (const char *e = getenv("SK_HOST_CHUNK_LOG2")) { const int lg = atoi(e); if (lg >= 6 && lg <= 30) return (size_t)1 << lg; }
	return dflt;
}
static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

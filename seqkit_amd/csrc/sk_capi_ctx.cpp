// sk_capi_ctx.cpp — the C-ABI of include/seqkit_hip.h, the context itself: its lifetime, its error text, memory and copies, the timer,
// and what the file calls see of it (sk_internal.h: sk::ctx_*).  The other units of the C-ABI: sk_capi_barcodes.cpp, sk_capi_comm.hip,
// sk_capi_fused.cpp, sk_capi_bam.cpp, sk_capi_misc.cpp.
// No CPU fallback lives here: without a GPU sk_create() fails and every other call needs a ctx.
#include "sk_ctx.h"

thread_local std::string sk::g_create_err;

namespace sk {
hipStream_t ctx_stream(sk_ctx *c) { return c->stream; }
hipStream_t ctx_stream2(sk_ctx *c) { return c->stream2; }
int ctx_n_cu(sk_ctx *c) { return c->n_cu; }
// a buffer of at least `bytes` that stays with the ctx (device memory or page-locked host memory); its contents are not kept when it
// has to grow.  nullptr + an error code in *rc when the allocation fails (the slot is then empty).
void *ctx_keep(sk_ctx *c, KeepSlot slot, size_t bytes, bool pinned, int *rc)
{
	*rc = SK_OK;
	auto &k = c->kept[slot];
	if (k.m && k.cap >= bytes && k.m.pinned == pinned) return k.m.get();
	k.cap = 0;
	const hipError_t e = k.m.alloc(bytes ? bytes : 1, pinned);
	if (e != hipSuccess) { *rc = fail(c, SK_ERR_NOMEM, "%zu bytes of %s memory: %s", bytes, pinned ? "page-locked" : "device", hipGetErrorString(e)); return nullptr; }
	k.cap = bytes;
	return k.m.get();
}
size_t ctx_kept_bytes(sk_ctx *c, KeepSlot slot) { return c->kept[slot].m ? c->kept[slot].cap : 0; }
void *ctx_ext(sk_ctx *c) { return c->ext; }
void ctx_set_ext(sk_ctx *c, void *p, void (*free_fn)(void *)) { c->ext = p; c->ext_free = free_fn; }
int ctx_bind(sk_ctx *c) { return bind(c); }
int ctx_fail(sk_ctx *c, int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	return fail(c, code, "%s", buf);
}
}  // namespace sk

extern "C" {

int sk_version(void) { return 0x000100; }

int sk_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

int sk_create(int device_id, sk_ctx **out)
{
	if (!out) return fail(nullptr, SK_ERR_INVALID, "sk_create: out is NULL");
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) return fail(nullptr, SK_ERR_NO_DEVICE, "no HIP device visible (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
	if (device_id < 0 || device_id >= n) return fail(nullptr, SK_ERR_NO_DEVICE, "device %d out of range (0..%d)", device_id, n - 1);
	hipDeviceProp_t prop;
	e = hipGetDeviceProperties(&prop, device_id);
	if (e != hipSuccess) return fail(nullptr, SK_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(nullptr, SK_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code objects only", device_id, prop.gcnArchName);
	sk_ctx *c = new sk_ctx();
	c->device = device_id;
	c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	if (const char *ev = getenv("SK_PLAN_CUS")) {      // tests: a smaller planning count, so capped grids loop at test sizes; never a larger one
		char *end = nullptr;
		const long v = strtol(ev, &end, 10);
		if (end != ev && *end == '\0' && v >= 1 && v <= (long)prop.multiProcessorCount) c->n_cu = (int)v;
	}
	e = hipSetDevice(device_id);
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
	if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_pipe, hipEventDisableTiming);
	if (e == hipSuccess) e = hipEventCreate(&c->ev0);
	if (e == hipSuccess) e = hipEventCreate(&c->ev1);
	if (e != hipSuccess) { int r = fail(nullptr, SK_ERR_HIP, "context setup: %s", hipGetErrorString(e)); delete c; return r; }
	*out = c;
	return SK_OK;
}

// What has an order or a side effect is done here; every buffer is freed by its owner (sk_ctx.h: DevMem) when the ctx is deleted, and the
// streams and events after them (CtxLanes).
void sk_destroy(sk_ctx *c)
{
	if (!c) return;
	(void)hipSetDevice(c->device);
	if (c->stream) (void)hipStreamSynchronize(c->stream);
	if (c->stream2) (void)hipStreamSynchronize(c->stream2);
	if (c->comm) (void)sk_comm_destroy(c);
	if (c->ext && c->ext_free) c->ext_free(c->ext);
	if (c->census) sk::census_destroy(c->census);
	delete c;
}

const char *sk_last_error(const sk_ctx *c) { return c ? c->err.c_str() : sk::g_create_err.c_str(); }

int sk_sync(sk_ctx *c)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	SK_HIP(c, hipStreamSynchronize(c->stream));
	return SK_OK;
}

void *sk_stream(sk_ctx *c) { return c ? (void *)c->stream : nullptr; }

int sk_planned_cus(sk_ctx *c) { return c ? c->n_cu : 0; }

int sk_malloc_device(sk_ctx *c, size_t bytes, void **out)
{
	if (!c || !out) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	*out = nullptr;
	hipError_t e = hipMalloc(out, bytes ? bytes : 1);
	if (e != hipSuccess) return fail(c, SK_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
	return SK_OK;
}
int sk_free_device(sk_ctx *c, void *p)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (p) SK_HIP(c, hipFree(p));
	return SK_OK;
}
// Pinned memory belongs to the process, not to a ctx (hipHostMallocPortable: page-locked for every device).  These two write
// NOTHING to the ctx — not even an error message: the hosts' worker threads call them on a ctx that another thread is running a
// pass on, and the message buffer of a ctx has one writer at a time — they return the code and sk_last_error is unchanged.
// They do make the ctx's device the calling thread's current one for the call (hipSetDevice is thread-local and touches no ctx
// state): on a thread that has no current device yet, the runtime would otherwise bring up a context on device 0 for the
// allocation.  The thread's own current device is put back before they return — a worker thread that also drives another ctx,
// another device or torch keeps launching where it was.
namespace {
struct ThreadDevice {              // the calling thread's current device for the lifetime of the object
	int saved = -1;
	bool ok;
	explicit ThreadDevice(int device)
	{
		if (hipGetDevice(&saved) != hipSuccess) { (void)hipGetLastError(); saved = -1; }
		ok = hipSetDevice(device) == hipSuccess;
		if (!ok) (void)hipGetLastError();
	}
	~ThreadDevice()
	{
		if (saved >= 0 && hipSetDevice(saved) != hipSuccess) (void)hipGetLastError();
	}
};
}  // namespace
int sk_malloc_pinned(sk_ctx *c, size_t bytes, void **out)
{
	if (!c || !out) return SK_ERR_INVALID;
	*out = nullptr;
	ThreadDevice td(c->device);
	if (!td.ok) return SK_ERR_HIP;
	if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return SK_ERR_NOMEM; }
	return SK_OK;
}
int sk_free_pinned(sk_ctx *c, void *p)
{
	if (!c) return SK_ERR_INVALID;
	if (!p) return SK_OK;
	ThreadDevice td(c->device);
	// (the pointer is freed even when the device could not be bound: portable pinned memory belongs to the process)
	if (hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); return SK_ERR_HIP; }
	return td.ok ? SK_OK : SK_ERR_HIP;
}
int sk_copy_h2d(sk_ctx *c, void *dst, const void *src, size_t bytes)
{
	if (!c || (bytes && (!dst || !src))) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (bytes) SK_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
	return SK_OK;
}
int sk_copy_d2h(sk_ctx *c, void *dst, const void *src, size_t bytes)
{
	if (!c || (bytes && (!dst || !src))) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	if (bytes) SK_HIP(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
	return SK_OK;
}

// ---- timing ----------------------------------------------------------------------------------------
int sk_timer_start(sk_ctx *c)
{
	if (!c) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	SK_HIP(c, hipEventRecord(c->ev0, c->stream));
	return SK_OK;
}

int sk_timer_stop(sk_ctx *c, float *ms)
{
	if (!c || !ms) return SK_ERR_INVALID;
	if (int r = bind(c)) return r;
	SK_HIP(c, hipEventRecord(c->ev1, c->stream));
	SK_HIP(c, hipEventSynchronize(c->ev1));
	SK_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
	return SK_OK;
}

}  // extern "C"

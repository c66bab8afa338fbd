// context.hip — the context behind a vkv_ctx handle (context.hpp): its arena, the per-stream scratch blocks, the cached device tables, the
// capture slots and the argument upload of vkv_render_batch that claims them, the start-order feedback targets and the tuning block, with the entry points that create, trim and destroy them.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>

#include "addr_tables.hpp"
#include "launchers.hpp"
#include "raymarch_args.hpp"        // sizeof(RayMarchArgs): what a batch upload holds
#include "../../include/vkvolume_amd_debug.h"

namespace vkv
{
int set_error(vkv_ctx *ctx, int code, const char *fmt, ...)
{
	if (ctx)
	{
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(ctx->error, sizeof(ctx->error), fmt, ap);
		va_end(ap);
	}
	return code;
}

VkvTuning tuning_of(vkv_ctx *ctx)
{
	std::lock_guard<std::mutex> lock(ctx->mutex);
	return ctx->tuning;
}

// `bytes` of device memory that stay valid until vkv_destroy (caller holds ctx->mutex).  Launch paths only take from the arena; set-up
// calls may fall back to hipMalloc.
// The arena has two regions: the first kScratchReserve scratch blocks (stream_scratch) and, behind them, the tables.  A renderer that
// keeps meeting new window sizes fills the TABLE region (a 1920x1080 schedule of 16x16 tiles costs 32 KiB per distinct size) - it can
// never take the room a new stream's scratch block needs, and vkv_trim gives the table region back.
static void *arena_take_table(vkv_ctx *ctx, size_t bytes, bool setup, bool *from_arena)
{
	const size_t need = (bytes + 255u) & ~(size_t) 255u;
	*from_arena       = false;
	if (ctx->arena && ctx->table_used + need <= ctx->arena_bytes - ctx->table_base)
	{
		void *p = ctx->arena.get() + ctx->table_base + ctx->table_used;
		ctx->table_used += need;
		*from_arena = true;
		return p;
	}
	if (!setup)
		return nullptr;
	DeviceMem p = device_alloc(need);
	if (!p)
		return nullptr;
	ctx->overflow.push_back(std::move(p));
	return ctx->overflow.back().get();
}

VkvStreamKey stream_key(hipStream_t stream)
{
	VkvStreamKey k;
	k.stream = stream;
	if (stream == hipStreamPerThread)
		k.thread = std::this_thread::get_id();
	return k;
}

StreamScratch stream_scratch(vkv_ctx *ctx, hipStream_t stream, bool setup)
{
	vkv_ctx::ScratchBlock *b = nullptr;
	{        // the block under ctx->mutex, its lock after: the lock order is "block, then ctx->mutex"
		std::lock_guard<std::mutex> lock(ctx->mutex);
		const VkvStreamKey          key = stream_key(stream);
		auto                        it  = ctx->scratch.find(key);
		if (it != ctx->scratch.end())
			b = it->second;
		else
		{
			uint8_t *const arena = ctx->arena.get();
			uint8_t *      p     = nullptr;
			if (!ctx->free_scratch.empty())
			{
				b = ctx->free_scratch.back();
				ctx->free_scratch.pop_back();
			}
			else if (arena && ctx->scratch_used + kScratchBytes <= ctx->table_base)
			{
				p = arena + ctx->scratch_used;
				ctx->scratch_used += kScratchBytes;
			}
			else if (setup)
			{        // more streams than the arena reserves blocks for: a set-up call may allocate (kept until vkv_destroy)
				DeviceMem q = device_alloc(kScratchBytes);
				if (q)
				{
					p = q.get();
					ctx->overflow_scratch.push_back(std::move(q));
				}
			}
			if (p)
			{
				b = new (std::nothrow) vkv_ctx::ScratchBlock;        // (out of host memory: the bytes stay unused until vkv_destroy)
				if (b)
				{
					b->p = p;
					ctx->scratch_blocks.emplace_back(b);
					const size_t index = (size_t) (p - arena) / kScratchBytes;        // (a block outside the arena: a huge index, no ring)
					if (ctx->upload_pool && p >= arena && index < kScratchReserve)
						for (uint32_t k = 0; k < vkv_ctx::kUploadRing; ++k)
						{        // the block's share of the pinned pool; a slot whose event cannot be created stays unused
							vkv_ctx::UploadSlot &u = b->upload[k];
							if ((u.done = event_create()))
								u.pinned = ctx->upload_pool.get() + (index * vkv_ctx::kUploadRing + k) * kUploadSlotBytes;
						}
				}
			}
			if (!b)
			{
				set_error(ctx, VKV_E_UNSUPPORTED, "no scratch block left for a new stream: the arena reserves %zu (call vkv_prepare_render for the stream at set-up "
				                                  "time, give finished streams back with vkv_release_stream, or raise VKV_ARENA_BYTES)", ctx->table_base / kScratchBytes);
				return StreamScratch{};
			}
			ctx->scratch.emplace(key, b);
		}
	}
	StreamScratch r;
	r.lock  = std::unique_lock<std::mutex>(b->lock);
	r.p     = b->p;
	r.block = b;
	return r;
}

// ---- the argument upload of vkv_render_batch ----
// The argument blocks go through the stream's scratch block: an earlier batch on the same stream has finished with it by the time the copy
// (same stream) runs, and the block's lock keeps other threads' writes into it (same stream) out from the copy to the launch.
static_assert(kMaxBatch * sizeof(RayMarchArgs) <= kScratchBytes - kBatchArgsOffset, "batch argument blocks must fit the stream scratch");
static_assert(kPullHeadsBytes + kMaxBatch * sizeof(RayMarchArgs) <= kCaptureSlotBytes, "a captured launch's upload must fit its pinned slot");
static_assert(kPullHeadsBytes + kMaxBatch * sizeof(RayMarchArgs) <= kUploadSlotBytes, "a launch's upload must fit a slot of the block's pinned ring");

// The upload is assembled once, in place, in a pinned slot of the block's ring: no pageable source that the runtime has to stage, nothing
// allocated.  A slot is free once the event behind the copy that read it has completed; with every slot still in flight (or none: a block
// beyond the reserve, a captured launch, which gets a slot of its own in commit) the upload comes from pageable memory - never a wait.
BatchUpload::BatchUpload(vkv_ctx *ctx, const StreamScratch &scratch, hipStream_t stream, size_t bytes)
    : ctx_(ctx), stream_(stream), bytes_(bytes), device_(scratch.p + kBatchArgsOffset - kPullHeadsBytes)
{
	hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
	capturing_                     = hipStreamIsCapturing(stream, &capture) == hipSuccess && capture == hipStreamCaptureStatusActive;
	vkv_ctx::ScratchBlock &b       = *scratch.block;
	for (uint32_t k = 0; k < vkv_ctx::kUploadRing && !capturing_ && !ring_slot_; ++k)
	{
		vkv_ctx::UploadSlot &u = b.upload[(b.upload_next + k) % vkv_ctx::kUploadRing];
		if (!u.pinned)
			continue;
		if (u.pending && hipEventQuery(u.done.get()) == hipSuccess)
			u.pending = false;
		if (!u.pending)
		{
			ring_slot_    = &u;
			b.upload_next = (b.upload_next + k + 1) % vkv_ctx::kUploadRing;
		}
	}
	(void) hipGetLastError();        // (a slot that is still being read answers hipErrorNotReady: not this launch's error)
	if (!ring_slot_)
		pageable_.resize(bytes);
	host_ = ring_slot_ ? ring_slot_->pinned : pageable_.data();
	std::memset(host_, 0, bytes);        // the counters, and every field fill_render_args leaves alone (an empty frame's block)
}

BatchUpload::BatchUpload(BatchUpload &&o)
    : ctx_(o.ctx_), stream_(o.stream_), bytes_(o.bytes_), capturing_(o.capturing_), ring_slot_(o.ring_slot_), pageable_(std::move(o.pageable_)), host_(o.host_),
      device_(o.device_), slot_(o.slot_), slot_taken_(o.slot_taken_)
{
	o.slot_taken_ = false;
}

BatchUpload::~BatchUpload()
{
	if (!slot_taken_)
		return;
	std::lock_guard<std::mutex> lock(ctx_->mutex);
	if (slot_ < ctx_->capture_slots.size())
		ctx_->capture_slots[slot_].in_use = false, ctx_->capture_slots[slot_].owner = VkvStreamKey{};
}

int BatchUpload::commit()
{
	const void *src = host_;
	if (capturing_)
	{
		// A stream that is being captured into a hipGraph records the copy's SOURCE POINTER and reads it at every replay, so the source has to
		// outlive the call; and the graph can be replayed on any stream, concurrently with other graphs and with live launches on the capture
		// stream, so it must not go through that stream's scratch block (whose users are serialised by the stream, which a replay elsewhere is
		// not).  A captured launch therefore gets a slot of its own - pinned source AND device target of the upload.  vkv_create set
		// kCaptureSlots slots aside, so that the usual capture allocates nothing; beyond them a slot is allocated here, with this thread's
		// capture mode relaxed for the calls (an allocation under the global / thread-local mode would invalidate the capture).  Slots return
		// with vkv_release_captured(stream), vkv_trim and vkv_destroy - or with this object, unless the launch was recorded (keep).
		std::lock_guard<std::mutex> lock(ctx_->mutex);
		vkv_ctx::CaptureSlot *      slot = nullptr;
		for (auto &c : ctx_->capture_slots)
			if (!c.in_use)
			{
				slot = &c;
				break;
			}
		if (!slot)
		{
			vkv_ctx::CaptureSlot c;
			void *               hp = nullptr, *dp = nullptr;
			hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
			(void) hipThreadExchangeStreamCaptureMode(&mode);
			const hipError_t ea = hipHostMalloc(&hp, kCaptureSlotBytes, hipHostMallocDefault);
			const hipError_t eb = ea == hipSuccess ? hipMalloc(&dp, kCaptureSlotBytes) : ea;
			const bool failed = ea != hipSuccess || eb != hipSuccess || !hp || !dp;
			if (failed && hp)
				(void) hipHostFree(hp);        // still inside the relaxed window: a free under the capture's own mode could invalidate it
			(void) hipThreadExchangeStreamCaptureMode(&mode);
			if (failed)
				return set_error(ctx_, VKV_E_UNSUPPORTED, "render_batch: no argument block for a captured launch: %s", hipGetErrorString(ea != hipSuccess ? ea : eb));
			c.pinned = static_cast<uint8_t *>(hp), c.device = static_cast<uint8_t *>(dp);
			c.own_pinned.reset(c.pinned), c.own_device.reset(c.device);        // the context's from here on
			ctx_->capture_slots.push_back(std::move(c));
			slot = &ctx_->capture_slots.back();
		}
		slot->in_use = true, slot->owner = stream_key(stream_);
		slot_ = (size_t) (slot - ctx_->capture_slots.data()), slot_taken_ = true;
		std::memcpy(slot->pinned, host_, bytes_);
		src     = slot->pinned;
		device_ = slot->device;
	}
	const hipError_t e = hipMemcpyAsync(device_, src, bytes_, hipMemcpyHostToDevice, stream_);
	if (e != hipSuccess)
		return set_error(ctx_, (int) e, "render_batch: argument upload: %s", hipGetErrorString(e));
	if (ring_slot_)
	{        // the slot is the copy's source until this event has completed; if it cannot be recorded, wait for the copy here
		if (hipEventRecord(ring_slot_->done.get(), stream_) == hipSuccess)
			ring_slot_->pending = true;
		else
			(void) hipStreamSynchronize(stream_);
	}
	return VKV_OK;
}

// Device copy of a new table: memory out of the arena, asynchronous upload from the entry's own host copy on the launch's stream, an
// event behind it for launches on other streams.  Caller holds ctx->mutex.  False (and nothing allocated that matters) when there is no room.
static bool table_upload(vkv_ctx *ctx, vkv_ctx::Table &t, hipStream_t s, bool setup)
{
	const size_t bytes = t.host.size() * sizeof(uint32_t);
	bool         from_arena = false;
	t.d                = static_cast<uint32_t *>(arena_take_table(ctx, bytes, setup, &from_arena));
	if (!t.d)
		return false;
	if (!(t.uploaded = event_create()))
		return false;        // (the arena bytes stay taken until the next vkv_trim: harmless)
	// The source of the asynchronous copy is the table's twin in the PINNED mirror of the table region (same offset): a copy from pageable
	// memory may block the enqueueing thread behind earlier work of the stream, which a launch must not do; the mirror lives as long as
	// the arena, so the source outlives the copy whatever happens to the entry.  A table a set-up call put outside the arena (hipMalloc
	// fallback) is copied from the entry's own vector and waited for right here.
	const void *src = t.host.data();
	if (from_arena && ctx->table_mirror)
	{
		uint8_t *m = ctx->table_mirror.get() + (reinterpret_cast<uint8_t *>(t.d) - (ctx->arena.get() + ctx->table_base));
		std::memcpy(m, t.host.data(), bytes);
		src = m;
	}
	const bool queued = hipMemcpyAsync(t.d, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
	if (!queued || hipEventRecord(t.uploaded.get(), s) != hipSuccess)
	{
		if (queued)
			(void) hipStreamSynchronize(s);        // the copy may still be reading its source: not while the caller deletes the entry
		t.uploaded.reset();
		return false;
	}
	t.upload_stream = s;
	if (setup || src == t.host.data())
	{        // a set-up call hands out finished tables (and a pageable source must not be left to an asynchronous copy)
		(void) hipEventSynchronize(t.uploaded.get());
		t.ready = true;
	}
	return true;
}

// the table for a launch on stream s: behind its upload (caller holds ctx->mutex)
static const uint32_t *table_on_stream(vkv_ctx::Table &t, hipStream_t s, bool setup)
{
	if (t.ready)
		return t.d;
	if (setup ? hipEventSynchronize(t.uploaded.get()) == hipSuccess : hipEventQuery(t.uploaded.get()) == hipSuccess)
	{
		t.ready = true;
		return t.d;
	}
	// (hipStreamPerThread is another stream in every thread: a launch on it waits for the upload even when the upload went through that handle)
	if ((s != t.upload_stream || s == hipStreamPerThread) && hipStreamWaitEvent(s, t.uploaded.get(), 0) != hipSuccess)
		return nullptr;
	return t.d;
}

constexpr size_t kMaxCachedTables = 1024;        // per kind; beyond that a launch runs without (never evicts: a launch may still read any of them)

const uint32_t *packed_addr_lut(vkv_ctx *ctx, int W, int H, int D, uint32_t *lut_y, uint32_t *lut_z, uint32_t *words, uint32_t *full, hipStream_t stream, bool setup)
{
	std::lock_guard<std::mutex> lock(ctx->mutex);
	for (auto &t : ctx->addr_luts)
		if (t->W == W && t->H == H && t->D == D)
		{
			*lut_y = t->lut_y, *lut_z = t->lut_z, *words = t->words, *full = t->full;
			return table_on_stream(t->table, stream, setup);
		}
	if (ctx->addr_luts.size() >= kMaxCachedTables)
		return nullptr;
	// two levels per axis: position inside a macro-brick (32 entries: padded index b & 31) and the macro-brick term (b >> 5); behind them the
	// per-voxel-index tables as a workgroup's LDS holds them (addr_tables.hpp), where a kernel can use them: offsets in units of two bytes
	// in 32 bits (a packed image of up to 8 GiB) and tables that fit the dynamic LDS a lean kernel may ask for
	const PackedDims pd = packed_dims(W, H, D);
	const bool       with_full = packed_bytes(pd) <= (1ull << 33) && ((size_t) W + 2 + (size_t) H + 2 + (size_t) D + 2) * 4 <= kMaxDynamicLds;
	std::unique_ptr<vkv_ctx::AddrLut> e(new (std::nothrow) vkv_ctx::AddrLut{W, H, D, 0, 0, 0, 0, {}});
	if (!e)
		return nullptr;
	const AddrTables t = build_addr_tables(W, H, D, pd.mx, pd.my, with_full, e->table.host);
	e->lut_y = t.lut_y, e->lut_z = t.lut_z, e->words = t.words, e->full = t.full;
	if (!table_upload(ctx, e->table, stream, setup))
		return nullptr;
	*lut_y = e->lut_y, *lut_z = e->lut_z, *words = e->words, *full = e->full;
	ctx->addr_luts.push_back(std::move(e));
	return ctx->addr_luts.back()->table.d;
}

const uint32_t *tile_start_order(vkv_ctx *ctx, uint32_t img_w, uint32_t img_h, uint32_t tile_w, uint32_t tile_h, uint32_t first, uint32_t stride, uint32_t count,
                                 hipStream_t stream, bool setup)
{
	if (count < 2)
		return nullptr;
	const uint32_t tiles_x = (img_w + tile_w - 1) / tile_w, tiles_y = (img_h + tile_h - 1) / tile_h;
	std::lock_guard<std::mutex> lock(ctx->mutex);
	const float mix_heavy_f = ctx->tuning.tile_mix_heavy, mix_spread_f = ctx->tuning.tile_mix_spread;
	for (auto &t : ctx->tile_orders)
		if (t->tiles_x == tiles_x && t->tiles_y == tiles_y && t->tile_w == tile_w && t->tile_h == tile_h && t->img_w == img_w && t->img_h == img_h && t->first == first &&
		    t->stride == stride && t->count == count && t->mix_heavy == mix_heavy_f && t->mix_spread == mix_spread_f)
			return table_on_stream(t->table, stream, setup);
	if (ctx->tile_orders.size() >= kMaxCachedTables)
		return nullptr;
	std::unique_ptr<vkv_ctx::TileOrder> e(
	    new (std::nothrow) vkv_ctx::TileOrder{tiles_x, tiles_y, tile_w, tile_h, img_w, img_h, first, stride, count, mix_heavy_f, mix_spread_f, {}});
	if (!e)
		return nullptr;
	e->table.host = start_order(img_w, img_h, tile_w, tile_h, first, stride, count, mix_heavy_f, mix_spread_f);
	if (!table_upload(ctx, e->table, stream, setup))
		return nullptr;
	ctx->tile_orders.push_back(std::move(e));
	return ctx->tile_orders.back()->table.d;
}

int check_launch(vkv_ctx *ctx, const char *what)
{
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess)
		return set_error(ctx, (int) e, "%s: %s", what, hipGetErrorString(e));
	return VKV_OK;
}

// the opacity-correction table (build_alpha_lut) out of the context's cache: it depends on two floats that change when a slider moves, not
// when the camera does
void cached_alpha_lut(vkv_ctx *ctx, const VkvTransferFunctionUniform &tf, float *lut)
{
	uint32_t factor_bits, sampling_bits;
	std::memcpy(&factor_bits, &tf.voxel_alpha_factor, 4), std::memcpy(&sampling_bits, &tf.sampling_factor, 4);
	{
		std::lock_guard<std::mutex> lock(ctx->mutex);
		for (const auto &e : ctx->alpha_luts)
			if (e.factor_bits == factor_bits && e.sampling_bits == sampling_bits)
			{
				std::memcpy(lut, e.lut, sizeof(e.lut));
				return;
			}
	}
	build_alpha_lut(tf, lut);        // (outside the lock; two threads that miss on the same key store the same bits)
	vkv_ctx::AlphaLut e;
	e.factor_bits = factor_bits, e.sampling_bits = sampling_bits;
	std::memcpy(e.lut, lut, sizeof(e.lut));
	std::lock_guard<std::mutex> lock(ctx->mutex);
	if (ctx->alpha_luts.size() < kAlphaLuts)
		ctx->alpha_luts.push_back(e);
	else
		ctx->alpha_luts[ctx->alpha_next++ % kAlphaLuts] = e;
}

// every cached table gone, the table region of the arena empty again (caller: the device is idle, ctx->mutex held or nobody else around)
static void drop_tables(vkv_ctx *ctx)
{
	ctx->tile_orders.clear();
	ctx->addr_luts.clear();
	ctx->overflow.clear();
	ctx->table_used = 0;
}

// the argument blocks of captured vkv_render_batch launches: the graphs that read them are the caller's, who promised not to replay them
static void drop_capture_blocks(vkv_ctx *ctx)
{
	auto &slots = ctx->capture_slots;
	slots.erase(std::remove_if(slots.begin(), slots.end(), [](const vkv_ctx::CaptureSlot &c) { return !c.pooled; }), slots.end());
	for (auto &c : slots)
		c.in_use = false, c.owner = VkvStreamKey{};
}

}        // namespace vkv

using namespace vkv;

extern "C" {

const char *vkv_version(void) { return "vkvolume_amd 0.1.0 (gfx950)"; }

int vkv_release_captured(vkv_ctx *ctx, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	std::lock_guard<std::mutex> lock(ctx->mutex);
	const VkvStreamKey          key = stream_key((hipStream_t) stream);
	for (auto &c : ctx->capture_slots)
		if (c.in_use && c.owner == key)
			c.in_use = false, c.owner = VkvStreamKey{};
	return VKV_OK;
}

int vkv_trim(vkv_ctx *ctx)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard      guard(ctx->device);
	// the lock first: the launch paths take it to look their tables up, so no launch can slip in between the wait and the drop
	std::lock_guard<std::mutex> lock(ctx->mutex);
	const hipError_t e = hipDeviceSynchronize();        // launches that still read a table
	if (e != hipSuccess)
		return set_error(ctx, (int) e, "trim: %s", hipGetErrorString(e));
	drop_tables(ctx);
	drop_capture_blocks(ctx);
	return VKV_OK;
}

int vkv_create(int device_ordinal, vkv_ctx **out_ctx)
{
	if (!out_ctx)
		return VKV_E_INVALID_ARGUMENT;
	*out_ctx  = nullptr;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_ordinal < 0 || device_ordinal >= count)
		return VKV_E_NO_DEVICE;
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess)
		return VKV_E_NO_DEVICE;
	if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !std::getenv("VKV_ALLOW_ANY_ARCH"))
		return VKV_E_NO_DEVICE;        // the code object is built for gfx950 only
	std::unique_ptr<vkv_ctx> ctx(new (std::nothrow) vkv_ctx());
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	ctx->device   = device_ordinal;
	ctx->cu_count = prop.multiProcessorCount;
	default_tuning(ctx->tuning, kMaxDynamicLds);
	{        // the arena every later launch carves its tables and scratch blocks out of (the one allocation of the render path)
		DeviceGuard guard(device_ordinal);
		if (!(ctx->arena = device_alloc(ctx->tuning.arena_bytes)))
			return VKV_E_NO_DEVICE;
		ctx->arena_bytes = ctx->tuning.arena_bytes;
		// scratch region: kScratchReserve blocks, at most half of a small arena; the tables get the rest and a pinned host mirror of it
		const size_t blocks = std::min<size_t>(kScratchReserve, ctx->arena_bytes / 2 / kScratchBytes);
		ctx->table_base = blocks * kScratchBytes, ctx->scratch_used = 0, ctx->table_used = 0;
		ctx->table_mirror = pinned_alloc(ctx->arena_bytes - ctx->table_base);        // (without it uploads fall back to the entry's own vector + a wait)
		PinnedMem cp = pinned_alloc((size_t) kCaptureSlots * kCaptureSlotBytes);
		DeviceMem cd = cp ? device_alloc((size_t) kCaptureSlots * kCaptureSlotBytes) : nullptr;
		if (cp && cd)
		{        // (without them a captured vkv_render_batch allocates its blocks during the capture)
			ctx->capture_pool = std::move(cp), ctx->capture_pool_device = std::move(cd);
			ctx->capture_slots.resize(kCaptureSlots);
			for (uint32_t i = 0; i < kCaptureSlots; ++i)
			{
				vkv_ctx::CaptureSlot &c = ctx->capture_slots[i];
				c.pinned = ctx->capture_pool.get() + (size_t) i * kCaptureSlotBytes, c.device = ctx->capture_pool_device.get() + (size_t) i * kCaptureSlotBytes, c.pooled = true;
			}
		}
		ctx->upload_pool = pinned_alloc(kScratchReserve * vkv_ctx::kUploadRing * kUploadSlotBytes);        // (without it vkv_render_batch uploads from pageable memory)
	}
	*out_ctx      = ctx.release();        // the caller's current device is left as it is: every entry point switches to ctx->device itself
	return VKV_OK;
}

void vkv_destroy(vkv_ctx *ctx)
{
	if (!ctx)
		return;
	DeviceGuard guard(ctx->device);
	(void) hipDeviceSynchronize();        // launches that still read the context's tables, scratch or feedback buffers
	delete ctx;
}

int vkv_get_tuning(const vkv_ctx *ctx, VkvTuning *out)
{
	if (!ctx || !out)
		return VKV_E_INVALID_ARGUMENT;
	*out = tuning_of(const_cast<vkv_ctx *>(ctx));
	return VKV_OK;
}

int vkv_set_tuning(vkv_ctx *ctx, const VkvTuning *tuning)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!tuning || tuning->struct_size != sizeof(VkvTuning))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "set_tuning: struct_size must be sizeof(VkvTuning) = %zu (start from vkv_get_tuning)", sizeof(VkvTuning));
	if (const char *why = tuning_problem(*tuning))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "set_tuning: %s", why);
	std::lock_guard<std::mutex> lock(ctx->mutex);
	const uint32_t              arena = ctx->tuning.arena_bytes;
	ctx->tuning                       = *tuning;
	ctx->tuning.arena_bytes           = arena;        // read-only
	clamp_tuning(ctx->tuning, kMaxDynamicLds);
	return VKV_OK;
}

int vkv_release_stream(vkv_ctx *ctx, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	std::lock_guard<std::mutex> lock(ctx->mutex);
	auto                        it = ctx->scratch.find(stream_key((hipStream_t) stream));        // hipStreamPerThread: the calling thread's block
	if (it != ctx->scratch.end())
	{
		ctx->free_scratch.push_back(it->second);
		ctx->scratch.erase(it);
	}
	return VKV_OK;
}

int vkv_register_target(vkv_ctx *ctx, const void *d_target, uint32_t image_width, uint32_t image_height, const VkvTileSchedule *tiles)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_target || !tiles || image_width == 0 || image_height == 0 || tiles->tile_width == 0 || tiles->tile_height == 0 || tiles->tile_stride == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "register_target: null pointer or zero size");
	(void) vkv_forget_target(ctx, d_target);        // a target has one state: registering it again replaces it
	if (tiles->tile_count == 0)
		return VKV_OK;
	const size_t        bytes = (size_t) tiles->tile_count * sizeof(uint32_t);
	DevicePtr<uint32_t> cost, order;
	void *              raw = nullptr;
	hipError_t          e   = hipMalloc(&raw, bytes);
	if (e == hipSuccess)
		cost.reset(static_cast<uint32_t *>(raw)), e = hipMalloc(&raw, bytes);
	if (e == hipSuccess)
		order.reset(static_cast<uint32_t *>(raw));
	std::vector<uint32_t> identity(tiles->tile_count);
	for (uint32_t i = 0; i < tiles->tile_count; ++i)
		identity[i] = i;
	// the order starts out as a valid permutation, the costs as zero; both are complete when this call returns
	if (e == hipSuccess)
		e = hipMemset(cost.get(), 0, bytes);
	if (e == hipSuccess)
		e = hipMemcpy(order.get(), identity.data(), bytes, hipMemcpyHostToDevice);
	const bool     whole   = tiles->rect.w == 0 || tiles->rect.h == 0;
	const uint32_t org_x = whole ? 0u : tiles->rect.x0 * tiles->tile_width, org_y = whole ? 0u : tiles->rect.y0 * tiles->tile_height;
	const uint32_t tiles_x = whole ? (image_width + tiles->tile_width - 1) / tiles->tile_width : tiles->rect.w;
	std::unique_ptr<vkv_ctx::TileFeedback> f(e != hipSuccess ? nullptr : new (std::nothrow) vkv_ctx::TileFeedback);
	if (!f)
		return set_error(ctx, e != hipSuccess ? (int) e : VKV_E_UNSUPPORTED, "register_target: %s", e != hipSuccess ? hipGetErrorString(e) : "out of memory");
	f->target = d_target, f->img_w = image_width, f->img_h = image_height, f->tile_w = tiles->tile_width, f->tile_h = tiles->tile_height;
	f->first = tiles->tile_first, f->stride = tiles->tile_stride, f->count = tiles->tile_count, f->org_x = org_x, f->org_y = org_y, f->tiles_x = tiles_x;
	f->d_cost = std::move(cost), f->d_order = std::move(order);
	load_feedback_code();        // the sort kernels' code object on this device now, not inside the first launch into the target
	std::lock_guard<std::mutex> lock(ctx->mutex);
	f->state.period = ctx->tuning.feedback_period;
	ctx->feedback.push_back(std::move(f));
	return VKV_OK;
}

int vkv_forget_target(vkv_ctx *ctx, const void *d_target)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard                            guard(ctx->device);
	std::unique_ptr<vkv_ctx::TileFeedback> f;
	{
		std::lock_guard<std::mutex> lock(ctx->mutex);
		for (size_t i = 0; i < ctx->feedback.size(); ++i)
			if (ctx->feedback[i]->target == d_target)
			{
				f = std::move(ctx->feedback[i]);
				ctx->feedback.erase(ctx->feedback.begin() + (long) i);
				break;
			}
	}
	if (f)
		(void) hipDeviceSynchronize();        // launches that still write costs or read the order (the entry is out of the list: no new ones)
	return VKV_OK;        // (and the entry goes with its buffers)
}

// ---- diagnostic entry points: include/vkvolume_amd_debug.h (not part of the drop-in boundary) ----
int vkv_debug_trace(vkv_ctx *ctx, void *d_buffer)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	ctx->d_trace = d_buffer;
	return VKV_OK;
}

int vkv_debug_tile_orders(vkv_ctx *ctx, const uint32_t *d_orders, uint32_t frames, uint32_t count)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	ctx->d_debug_orders = d_orders, ctx->debug_order_frames = d_orders ? frames : 0u, ctx->debug_order_count = count;
	return VKV_OK;
}

int vkv_debug_check(vkv_ctx *ctx, int32_t what, uint32_t first_bits, uint64_t count, uint64_t *d_mismatches, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_mismatches)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "check: null pointer");
	return launch_check_numerics(ctx, what, first_bits, count, reinterpret_cast<unsigned long long *>(d_mismatches), (hipStream_t) stream);
}

int vkv_debug_tf_scratch(vkv_ctx *ctx, uint32_t *d_out, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_out)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "debug_tf_scratch: null pointer");
	const StreamScratch scratch = stream_scratch(ctx, (hipStream_t) stream);
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	const hipError_t e = hipMemcpyAsync(d_out, scratch.p + kTfBitsOffset, (2048 + 8) * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t) stream);
	return e == hipSuccess ? VKV_OK : set_error(ctx, (int) e, "debug_tf_scratch: %s", hipGetErrorString(e));
}

const char *vkv_last_error(const vkv_ctx *ctx) { return ctx ? ctx->error : "null context"; }

}        // extern "C"

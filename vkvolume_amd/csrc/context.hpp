// context.hpp — the host-side context behind a vkv_ctx handle (context.hip owns it) and what the launchers take from it.  Host code only:
// the device-side definitions are vkv_device.hpp's.
// Device scratch is handed out PER STREAM (stream_scratch): calls on different streams never touch the same bytes.  Calls on one stream are
// ordered on the device, but an entry point enqueues several operations that pass data through the block (a bit table, argument blocks,
// queue heads), and two host threads enqueueing on the same stream could interleave them: each block has a lock, held by the entry point
// from its first write into the block to its last enqueue (stream_scratch returns the block locked).  hipStreamPerThread is one handle for
// a different stream in every thread: per-stream state is keyed by (handle, calling thread) for it (stream_key).  Lock order: a block's
// lock, then ctx->mutex briefly; ctx->mutex is never held while a block's lock is being taken.
//
// Device memory policy (include/vkvolume_amd.h, "Conventions"): vkv_create allocates one ARENA with two regions - the scratch blocks of
// up to kScratchReserve streams, and the small immutable tables a launch needs (tile start orders, address tables) - plus a pinned host
// mirror of the table region.  A table is written into the mirror and uploaded from there asynchronously on the stream of the launch that
// first needs it; launches on other streams are ordered behind that upload with an event until it has completed.  Nothing is freed or
// re-used while a launch could read it: tables stay until vkv_trim (a set-up call that waits for the device, then empties the region) or
// vkv_destroy; when the region is full a launch runs without the table.  Only set-up calls (vkv_prepare_render, vkv_register_target) fall
// back to hipMalloc when a region is full.
//
// Ownership: every allocation and event of the context is held by one of the move-only owners below and goes when its owner does - nothing
// is released by hand.  The order that matters: (1) the device is synchronised before anything a launch could read is freed (vkv_destroy
// and vkv_trim wait first; vkv_forget_target takes the entry out of the list under the mutex, THEN waits, then lets it go); (2) events go
// before the memory they guard - vkv_ctx's members are destroyed in reverse order of declaration, so the pools are declared in front of the
// blocks and tables whose events refer to them.
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../host/host_arith.hpp"
#include "vkv_device.hpp"

namespace vkv
{
struct DeviceFree { void operator()(void *p) const { (void) hipFree(p); } };
struct PinnedFree { void operator()(void *p) const { (void) hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void) hipEventDestroy(e); } };
template <class T> using DevicePtr = std::unique_ptr<T, DeviceFree>;
using DeviceMem = DevicePtr<uint8_t>;
using PinnedMem = std::unique_ptr<uint8_t, PinnedFree>;
using Event     = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
// null when the runtime refuses
inline DeviceMem device_alloc(size_t bytes) { void *p = nullptr; return DeviceMem(hipMalloc(&p, bytes) == hipSuccess ? static_cast<uint8_t *>(p) : nullptr); }
inline PinnedMem pinned_alloc(size_t bytes) { void *p = nullptr; return PinnedMem(hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? static_cast<uint8_t *>(p) : nullptr); }
inline Event     event_create() { hipEvent_t e = nullptr; return Event(hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? e : nullptr); }
}        // namespace vkv

// the key of a stream's state in the context: the handle, and for hipStreamPerThread also the calling thread
struct VkvStreamKey
{
	hipStream_t     stream = nullptr;
	std::thread::id thread;
	bool operator<(const VkvStreamKey &o) const { return stream != o.stream ? stream < o.stream : thread < o.thread; }
	bool operator==(const VkvStreamKey &o) const { return stream == o.stream && thread == o.thread; }
};

struct vkv_ctx
{
	int   device;
	int   cu_count;        // compute units of the device (grid of the resident-workgroup kernels)
	char  error[512] = "";
	void *d_trace = nullptr;        // diagnostic wave timeline buffer (vkv_debug_trace), normally null
	const uint32_t *d_debug_orders = nullptr;        // diagnostic per-frame tile start orders of vkv_render_batch (vkv_debug_tile_orders), normally null
	uint32_t        debug_order_frames = 0, debug_order_count = 0;
	std::mutex      mutex;
	VkvTuning       tuning;        // vkv_create: defaults + environment; vkv_set_tuning replaces it (read under the mutex, copied per call)
	// ---- device arena ----
	vkv::DeviceMem arena;
	size_t         arena_bytes = 0;
	size_t         table_base = 0;          // the arena's first table_base bytes are scratch blocks, the rest holds tables
	size_t         scratch_used = 0, table_used = 0;
	vkv::PinnedMem table_mirror;            // pinned host twin of the table region: the source of every asynchronous table upload
	std::vector<vkv::DeviceMem> overflow;                // hipMalloc blocks set-up calls took for tables when the region was full; dropped by vkv_trim
	std::vector<vkv::DeviceMem> overflow_scratch;        // ... for scratch blocks beyond the reserve
	// Argument blocks of vkv_render_batch launches captured into hipGraphs.  A captured launch owns a SLOT: a pinned host block (the graph's copy
	// node reads its source at every replay) and a device block of its own (the copy's target and the kernels' argument pointer: a graph may be
	// replayed on any stream, next to other graphs and to live launches, so it must not share the capture stream's scratch block).  kCaptureSlots
	// slots are set aside by vkv_create; later ones are allocated during the capture (and then own their two blocks).  A slot belongs to the
	// stream it was captured on until vkv_release_captured(stream), vkv_trim or vkv_destroy.
	struct CaptureSlot
	{
		uint8_t *      pinned = nullptr, *device = nullptr;
		VkvStreamKey   owner;
		bool           in_use = false, pooled = false;
		vkv::PinnedMem own_pinned;        // a slot that is not out of the pools
		vkv::DeviceMem own_device;
	};
	vkv::PinnedMem           capture_pool;
	vkv::DeviceMem           capture_pool_device;
	std::vector<CaptureSlot> capture_slots;
	// a stream's scratch block: kScratchBytes of device memory and the lock of the entry point that is passing data through it
	// upload: a small ring of pinned host slots (carved out of upload_pool by vkv_create, for the arena's blocks) in which vkv_render_batch
	// assembles the argument blocks it uploads into the block; a slot is taken again only after the event recorded behind the copy that read
	// it has completed (claimed under the block's lock).  A block without slots (beyond the reserve), or with every slot still being read,
	// uploads from pageable memory.
	struct UploadSlot
	{
		uint8_t *  pinned = nullptr;
		vkv::Event done;
		bool       pending = false;        // `done` has been recorded and not yet seen complete
	};
	static constexpr uint32_t kUploadRing = 4;
	struct ScratchBlock
	{
		uint8_t *  p = nullptr;
		std::mutex lock;
		UploadSlot upload[kUploadRing];
		uint32_t   upload_next = 0;
	};
	vkv::PinnedMem upload_pool;        // kScratchReserve x kUploadRing x kUploadSlotBytes
	// opacity-correction tables by the two floats they depend on (bit compare): a camera move re-uses them, a slider move adds one
	struct AlphaLut
	{
		uint32_t factor_bits, sampling_bits;
		float    lut[256];
	};
	std::vector<AlphaLut> alpha_luts;        // at most kAlphaLuts, replaced round robin
	uint32_t              alpha_next = 0;
	std::vector<std::unique_ptr<ScratchBlock>> scratch_blocks;        // every block the context has handed out (stable addresses)
	std::map<VkvStreamKey, ScratchBlock *>     scratch;               // stream -> its block
	std::vector<ScratchBlock *>                free_scratch;          // blocks given back by vkv_release_stream
	// an immutable device table with its host copy (the source of the asynchronous upload: it must outlive the call)
	struct Table
	{
		std::vector<uint32_t> host;
		uint32_t *            d = nullptr;        // in the arena, or in an `overflow` block
		vkv::Event            uploaded;           // recorded behind the upload
		hipStream_t           upload_stream = nullptr;
		bool                  ready = false;            // the upload is known to have completed: no more waits
	};
	// start orders of tile schedules (centre of the image first), built on first use and kept (heap objects: stable addresses)
	struct TileOrder
	{
		uint32_t tiles_x, tiles_y, tile_w, tile_h, img_w, img_h, first, stride, count;
		float    mix_heavy, mix_spread;
		Table    table;
	};
	std::vector<std::unique_ptr<TileOrder>> tile_orders;
	// per-axis address tables of the packed sampling image, per volume extent
	struct AddrLut
	{
		int      W, H, D;
		uint32_t lut_y, lut_z, words;
		uint32_t full;        // word offset of the per-voxel-index tables behind the two-level ones (addr_tables.hpp), 0 = none
		Table    table;
	};
	std::vector<std::unique_ptr<AddrLut>> addr_luts;
	// start-order feedback of the targets registered with vkv_register_target: the tile costs the last measured frame into the target left
	// behind and the buffer its longest-first order is written to (raymarch.hip, apply_feedback); heap objects, so their addresses stay valid
	struct TileFeedback
	{
		const void *target = nullptr;
		uint32_t    img_w = 0, img_h = 0, tile_w = 0, tile_h = 0, first = 0, stride = 0, count = 0;
		uint32_t    org_x = 0, org_y = 0, tiles_x = 0;        // the schedule's tile rectangle as the launcher sees it (pixels of its first tile, tile columns)
		vkv::DevicePtr<uint32_t> d_cost, d_order;
		vkv::FeedbackState       state;        // when to measure, when to use the order (feedback_step, ../host/host_arith.hpp)
	};
	std::vector<std::unique_ptr<TileFeedback>> feedback;
};

namespace vkv
{
int  set_error(vkv_ctx *ctx, int code, const char *fmt, ...);
int  check_launch(vkv_ctx *ctx, const char *what);
VkvStreamKey stream_key(hipStream_t stream);
// this stream's scratch block (out of the arena on first use, kept until vkv_release_stream / vkv_destroy), LOCKED until the object goes:
// an entry point keeps it from its first write into the block to its last enqueue.  p == nullptr + error set when there is no room.
struct StreamScratch
{
	uint8_t *                    p = nullptr;
	std::unique_lock<std::mutex> lock;
	vkv_ctx::ScratchBlock *      block = nullptr;        // its pinned upload ring (used under `lock`)
};
StreamScratch stream_scratch(vkv_ctx *ctx, hipStream_t stream, bool setup = false);
// The upload of a vkv_render_batch launch: `bytes` of the (zeroed) ticket counters of the pull kernel followed by the argument blocks, assembled
// in host() and brought to the device by commit().  Created under the lock of `scratch`, which the caller keeps until its last enqueue.
class BatchUpload
{
      public:
	BatchUpload(vkv_ctx *ctx, const StreamScratch &scratch, hipStream_t stream, size_t bytes);
	~BatchUpload();        // a capture slot whose launch was not recorded returns to the context
	BatchUpload(BatchUpload &&o);
	BatchUpload &operator=(BatchUpload &&) = delete;
	uint8_t *host() const { return host_; }
	// enqueues the copy; VKV_OK, or the error with the context's text set.  d_heads() and d_args() are valid after it.
	int       commit();
	uint32_t *d_heads() const { return reinterpret_cast<uint32_t *>(device_); }
	uint8_t * d_args() const;
	void      keep() { slot_taken_ = false; }        // the launch was recorded: the capture slot is the graph's until it is released
      private:
	vkv_ctx *            ctx_;
	hipStream_t          stream_;
	size_t               bytes_;
	bool                 capturing_;
	vkv_ctx::UploadSlot *ring_slot_ = nullptr;
	std::vector<uint8_t> pageable_;
	uint8_t *            host_, *device_;
	size_t               slot_ = 0;        // index of the capture slot taken by commit()
	bool                 slot_taken_ = false;
};
// start order of a tile schedule: entry indices sorted by the distance of the tile's centre from the image centre (device array of
// `count` uint32, cached per schedule shape); nullptr when the table cannot be allocated (the kernel then takes the tiles in order)
// Per-axis byte offsets of the packed sampling image: the offset of the footprint whose padded base texel is (bx, by, bz) is
// X(bx) + Y(by) + Z(bz) (the brick index and the position inside the brick are sums of per-axis terms), each in two levels:
// in-macro-brick term of b & 31 + macro-brick term of b >> 5.  Layout of the device array (uint32 words): in-macro tables of x, y, z
// at 0, 32, 64; macro terms of x at 96, of y at *lut_y, of z as 64-bit values at *lut_z (even), *words in all; behind them, at word *full
// (16-byte aligned; 0 = not built), the sums X[W + 2], Y[H + 2], Z[D + 2] per padded voxel index in units of two bytes, zero-padded to a multiple
// of 16 bytes: what a workgroup's LDS holds (stage_full_lut), built once per extent.  nullptr if it cannot be allocated.
// Both tables come out of the context's arena and are uploaded on `stream` when new (see vkv_ctx); `setup` = called from a set-up entry
// point: may fall back to hipMalloc when the arena is full.  nullptr when there is no room: the launch then runs without the table.
const uint32_t *packed_addr_lut(vkv_ctx *ctx, int W, int H, int D, uint32_t *lut_y, uint32_t *lut_z, uint32_t *words, uint32_t *full, hipStream_t stream, bool setup = false);
const uint32_t *tile_start_order(vkv_ctx *ctx, uint32_t img_w, uint32_t img_h, uint32_t tile_w, uint32_t tile_h, uint32_t first, uint32_t stride, uint32_t count,
                                 hipStream_t stream, bool setup = false);
VkvTuning tuning_of(vkv_ctx *ctx);        // a copy of the context's tuning block (taken under its mutex)
void      cached_alpha_lut(vkv_ctx *ctx, const VkvTransferFunctionUniform &tf, float *lut);        // the opacity-correction table out of the context's cache
constexpr size_t kScratchBytes     = 128 * 1024;
constexpr size_t kScratchReserve   = 16;          // scratch blocks the arena keeps for streams (2 MiB of the default 8 MiB)
constexpr uint32_t kCaptureSlots   = 32;          // vkv_render_batch launches one context may have captured into hipGraphs
constexpr size_t   kUploadSlotBytes = 64 * 1024;   // pinned slot of a scratch block's upload ring: the pull heads + VKV_MAX_BATCH argument blocks
constexpr size_t   kAlphaLuts = 8;
constexpr size_t   kCaptureSlotBytes = 96 * 1024;  // >= the pull heads + VKV_MAX_BATCH argument blocks (= the scratch block's argument area)
constexpr uint32_t kMaxDynamicLds  = 64 * 1024 - 1024;        // what a lean kernel may ask for as dynamic LDS (its tables; no hipFuncSetAttribute is called)
constexpr size_t kTfBitsOffset     = 0;           // 256*256 bits = 8 KiB: TF bit table of the map update / the voxel count (+ 8 words behind it: its column mask)
constexpr size_t kQueueHeadsOffset = 8192 + 64;       // 8 x u32 tile-queue heads of the persistent ray-march scheduler
constexpr size_t kTfRangesOffset   = 16 * 1024;       // 64 KiB: row-range ORs / ANDs of the bit table (cells.hip, k_tf_ranges), written and read
                                                      // within one occupancy-from-summary launch pair; shares bytes with the batch argument
                                                      // blocks below, which only a later launch on the same stream writes (stream order)
constexpr size_t kPullHeadsBytes   = 2048;        // 8 ticket counters of k_raymarch_lean_pull, kPullHeadStride words = 256 bytes apart (one memory channel each),
                                                  // directly in front of the argument blocks: one upload zeroes the counters and brings the arguments
constexpr size_t kBatchArgsOffset  = 32 * 1024 + kPullHeadsBytes;        // vkv_render_batch: kMaxBatch argument blocks
constexpr uint32_t kMaxBatch       = VKV_MAX_BATCH;
static_assert(kTfRangesOffset >= kQueueHeadsOffset + 32 && kTfRangesOffset + 4 * 2048 * 8 <= kScratchBytes, "the range table must fit the scratch block");
static_assert(8 * kPullHeadStride * sizeof(uint32_t) == kPullHeadsBytes, "the pull kernel's counters fill the bytes the upload zeroes");
inline uint8_t *BatchUpload::d_args() const { return device_ + kPullHeadsBytes; }

// Every device entry point runs on the context's device whatever the calling thread's current device is, and leaves the
// caller's current device as it found it.
struct DeviceGuard
{
	int  prev = -1;
	bool switched = false;
	explicit DeviceGuard(int device)
	{
		if (hipGetDevice(&prev) == hipSuccess && prev != device)
			switched = hipSetDevice(device) == hipSuccess;
	}
	~DeviceGuard()
	{
		if (switched)
			(void) hipSetDevice(prev);
	}
	DeviceGuard(const DeviceGuard &) = delete;
	DeviceGuard &operator=(const DeviceGuard &) = delete;
};
}        // namespace vkv

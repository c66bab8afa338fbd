// exchange.hip — the multi-GPU tile exchange: RCCL resolved at run time, the gather of every rank's tiles and the de-interleave of the
// gathered buffers into images (vkv_gather_tiles, vkv_assemble_frame(s), vkv_scatter_tiles).
#include <cstdlib>
#include <dlfcn.h>
#include <mutex>
#include <string>

#include "launchers.hpp"

using namespace vkv;

// ---- RCCL, resolved at run time (the library is not a link-time dependency of the product) ---------------------------------
namespace
{
typedef int (*nccl_gather_fn)(const void *, void *, size_t, int /* ncclDataType_t */, int, void * /* ncclComm_t */, hipStream_t);
typedef const char *(*nccl_error_fn)(int);
typedef int (*nccl_group_fn)(void);
struct Rccl
{
	void *         handle = nullptr;
	nccl_gather_fn gather = nullptr;
	nccl_error_fn  error  = nullptr;
	nccl_group_fn  group_start = nullptr, group_end = nullptr;
	bool           tried  = false;
	std::string    why;        // the loader's message when no library could be opened (dlerror() clears itself: captured once)
};
Rccl       g_rccl;
std::mutex g_rccl_mutex;

const Rccl &rccl()
{
	std::lock_guard<std::mutex> lock(g_rccl_mutex);
	if (g_rccl.tried)
		return g_rccl;
	g_rccl.tried = true;
	const char *override_path = std::getenv("VKV_RCCL_LIBRARY");
	void *      h             = nullptr;
	if (override_path && override_path[0])
		h = dlopen(override_path, RTLD_NOW | RTLD_LOCAL);
	// the copy the process already uses (the application's, or the one inside PyTorch): communicator and call must come from the same library
	for (const char *name : {"librccl.so.1", "librccl.so"})
		if (!h)
			h = dlopen(name, RTLD_NOW | RTLD_LOCAL | RTLD_NOLOAD);
	for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
		if (!h)
		{
			h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
			if (!h)
			{
				const char *msg = dlerror();
				g_rccl.why += (g_rccl.why.empty() ? "" : "; ");
				g_rccl.why += msg ? msg : name;
			}
		}
	if (h && !dlsym(h, "ncclGather"))
		g_rccl.why = "the RCCL library that was found does not export ncclGather";
	if (h)
	{
		g_rccl.handle = h;
		g_rccl.gather = reinterpret_cast<nccl_gather_fn>(dlsym(h, "ncclGather"));
		g_rccl.error  = reinterpret_cast<nccl_error_fn>(dlsym(h, "ncclGetErrorString"));
		g_rccl.group_start = reinterpret_cast<nccl_group_fn>(dlsym(h, "ncclGroupStart"));
		g_rccl.group_end   = reinterpret_cast<nccl_group_fn>(dlsym(h, "ncclGroupEnd"));
	}
	return g_rccl;
}

// the loaded library, or null with the error text of entry point `what` set
const Rccl *rccl_or_error(vkv_ctx *ctx, const char *what)
{
	const Rccl &r = rccl();
	if (!r.gather)
		set_error(ctx, VKV_E_UNSUPPORTED, "%s: no RCCL library with ncclGather could be loaded (%s)", what, r.why.empty() ? "librccl.so.1" : r.why.c_str());
	return r.gather ? &r : nullptr;
}
}        // namespace

extern "C" {

int vkv_scatter_tiles(vkv_ctx *ctx, const void *d_gathered, void *d_image, uint32_t image_width, uint32_t image_height, uint32_t tile_width,
                      uint32_t tile_height, const VkvTileRect *rect, uint32_t n_ranks, uint32_t rank_stride_tiles, uint32_t bytes_per_pixel, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_gathered || !d_image || !image_width || !image_height || !tile_width || !tile_height || !n_ranks)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "scatter_tiles: null pointer or zero size");
	VkvTileRect r;
	if (!resolve_rect(rect, image_width, image_height, tile_width, tile_height, r))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "scatter_tiles: the tile rectangle runs past the image");
	if ((uint64_t) rank_stride_tiles * n_ranks < (uint64_t) r.w * r.h)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "scatter_tiles: gathered buffer holds fewer tiles than the rectangle");
	return launch_scatter_tiles_frames(ctx, 1u, &d_image, &d_gathered, &r, &rank_stride_tiles, image_width, image_height, tile_width, tile_height, n_ranks,
	                                   bytes_per_pixel, (hipStream_t) stream);
}

int vkv_gather_tiles(vkv_ctx *ctx, const void *d_tiles, void *d_gathered, size_t bytes_per_rank, int32_t root, void *nccl_comm, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_tiles || !nccl_comm || root < 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "gather_tiles: null buffer / communicator or negative root");
	if (bytes_per_rank == 0)
		return VKV_OK;
	const Rccl *r = rccl_or_error(ctx, "gather_tiles");
	if (!r)
		return VKV_E_UNSUPPORTED;
	const int rc = r->gather(d_tiles, d_gathered, bytes_per_rank, 0 /* ncclInt8 / ncclChar */, root, nccl_comm, (hipStream_t) stream);
	if (rc != 0)
		return set_error(ctx, 1000 + rc, "gather_tiles: ncclGather: %s", r->error ? r->error(rc) : "error");
	return VKV_OK;
}

int vkv_assemble_frame(vkv_ctx *ctx, const void *d_tiles, void *d_gathered, void *d_image, uint32_t image_width, uint32_t image_height, uint32_t tile_width,
                       uint32_t tile_height, const VkvTileRect *rect, uint32_t n_ranks, uint32_t rank, uint32_t bytes_per_pixel, int32_t root, void *nccl_comm,
                       void *stream)
{
	return vkv_assemble_frames(ctx, d_tiles, d_gathered, &d_image, 1u, image_width, image_height, tile_width, tile_height, rect, n_ranks, rank, bytes_per_pixel, root, nullptr,
	                           nccl_comm, stream);
}

int vkv_assemble_frames(vkv_ctx *ctx, const void *d_tiles, void *d_gathered, void *const *d_images, uint32_t frames, uint32_t image_width, uint32_t image_height,
                        uint32_t tile_width, uint32_t tile_height, const VkvTileRect *rects, uint32_t n_ranks, uint32_t rank, uint32_t bytes_per_pixel, int32_t root,
                        const int32_t *roots, void *nccl_comm, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (n_ranks == 0 || rank >= n_ranks || frames == 0 || frames > VKV_MAX_BATCH)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: bad rank / n_ranks, or frames not in 1 .. %d", VKV_MAX_BATCH);
	if (!image_width || !image_height || !tile_width || !tile_height || (bytes_per_pixel != 4 && bytes_per_pixel != 16))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: zero size, or bytes_per_pixel not 4 or 16");
	// per frame: rectangle, owner, tiles per rank, where the frame starts in a rank's block
	VkvTileRect rect[VKV_MAX_BATCH];
	int32_t     owner[VKV_MAX_BATCH];
	uint32_t    tpr[VKV_MAX_BATCH];
	uint64_t    off[VKV_MAX_BATCH + 1];
	const bool  one_owner = roots == nullptr;        // the caller's choice: one gather of the whole block to `root`, or a group of gathers, one per frame
	bool        mine      = false;
	off[0] = 0;
	for (uint32_t f = 0; f < frames; ++f)
	{
		if (!resolve_rect(rects ? &rects[f] : nullptr, image_width, image_height, tile_width, tile_height, rect[f]))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: the tile rectangle of frame %u runs past the image", f);
		owner[f] = roots ? roots[f] : root;
		if (owner[f] < 0 || (uint32_t) owner[f] >= n_ranks)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: bad root %d of frame %u", owner[f], f);
		const uint64_t tiles = (uint64_t) rect[f].w * rect[f].h;
		tpr[f]     = (uint32_t) ((tiles + n_ranks - 1) / n_ranks);
		off[f + 1] = off[f] + tpr[f];
		if ((uint32_t) owner[f] == rank)
		{
			mine = true;
			if (!d_images || !d_images[f])
				return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: d_images[%u] is null on the frame's owner", f);
		}
	}
	if (off[frames] * n_ranks > 0xffffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "assemble_frames: too many tiles for one exchange");
	if (mine && !d_gathered)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: a rank that owns a frame needs d_gathered");
	const size_t   tile_bytes = (size_t) tile_width * tile_height * bytes_per_pixel;
	const uint8_t *tiles_b    = static_cast<const uint8_t *>(d_tiles);
	uint8_t *      gath_b     = static_cast<uint8_t *>(d_gathered);
	const void *   src[VKV_MAX_BATCH];
	uint32_t       stride[VKV_MAX_BATCH];
	if (one_owner)
	{
		// ONE collective for the whole launch: [frame][tiles] of every rank -> [rank][frame][tiles] on the owner
		const int rc = vkv_gather_tiles(ctx, d_tiles, d_gathered, (size_t) off[frames] * tile_bytes, owner[0], nccl_comm, stream);
		if (rc != VKV_OK)
			return rc;
		for (uint32_t f = 0; f < frames; ++f)
			src[f] = gath_b + (size_t) off[f] * tile_bytes, stride[f] = (uint32_t) off[frames];
	}
	else
	{
		// owners spread over the ranks: one gather per frame, all of them in ONE group (RCCL fuses the group's point-to-point transfers: every
		// owner receives at the same time over its own inbound links); frame f arrives as [rank][tpr(f) tiles] at tile n_ranks * off[f]
		if (!d_tiles || !nccl_comm)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "assemble_frames: null buffer / communicator");
		const Rccl *r = rccl_or_error(ctx, "assemble_frames");
		if (!r)
			return VKV_E_UNSUPPORTED;
		DeviceGuard guard(ctx->device);
		const bool  grouped = r->group_start && r->group_end;
		int         rc      = grouped ? r->group_start() : 0;
		for (uint32_t f = 0; f < frames && rc == 0; ++f)
			if (tpr[f])
				rc = r->gather(tiles_b + (size_t) off[f] * tile_bytes, (uint32_t) owner[f] == rank ? gath_b + (size_t) n_ranks * off[f] * tile_bytes : nullptr,
				              (size_t) tpr[f] * tile_bytes, 0 /* ncclInt8 / ncclChar */, owner[f], nccl_comm, (hipStream_t) stream);
		if (grouped)
		{
			const int rc2 = r->group_end();        // (always closed: an open group would swallow the caller's next collective)
			rc = rc ? rc : rc2;
		}
		if (rc != 0)
			return set_error(ctx, 1000 + rc, "assemble_frames: ncclGather group: %s", r->error ? r->error(rc) : "error");
		for (uint32_t f = 0; f < frames; ++f)
			src[f] = gath_b + (size_t) n_ranks * off[f] * tile_bytes, stride[f] = tpr[f];
	}
	if (!mine)
		return VKV_OK;
	// ONE de-interleave kernel for the frames this rank owns
	void *      img[VKV_MAX_BATCH];
	uint32_t    n = 0;
	for (uint32_t f = 0; f < frames; ++f)
		if ((uint32_t) owner[f] == rank)
			img[n] = d_images[f], src[n] = src[f], rect[n] = rect[f], stride[n] = stride[f], ++n;
	DeviceGuard guard(ctx->device);
	return launch_scatter_tiles_frames(ctx, n, img, src, rect, stride, image_width, image_height, tile_width, tile_height, n_ranks, bytes_per_pixel, (hipStream_t) stream);
}

}        // extern "C"

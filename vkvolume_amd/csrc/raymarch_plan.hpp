// raymarch_plan.hpp — what a ray-march launch decides on the host once its argument blocks are filled: the kernel a batch of frames shares,
// its grid, and whether a fill_outside rectangle is rendered as the whole-image schedule.  Pure functions of the argument blocks and the
// tuning block: no device, no context, no HIP header - plain host C++ like raymarch_args.hpp, so that tests/host_arith_driver.cpp can hold
// every decision to its rule.  Included by raymarch_inst.hpp (LeanChoice, wants_counts) and through it by raymarch.hip.
#pragma once

#include <stddef.h>
#include <string.h>

#include "raymarch_args.hpp"

namespace vkv
{

struct LeanChoice
{
	int    kind;        // 0 plain, 1 two-level tables, 2 full tables
	size_t lds;         // dynamic LDS bytes (lean_lds_bytes: the kernels' whole LDS layout lives in the dynamic segment)
};

// A launch may run the loop without the three per-pixel counters when nothing reads them: no counter buffer and not the frag's
// sample-count test output (frag:324-334 turns n_vol + n_dist into the colour - Test::NumTextureSamples is independent of ERT and of
// the skipping type in the reference's GUI, src/volume_render.cpp:539)
inline bool wants_counts(const RayMarchArgs &a) { return a.out_counts != nullptr || a.test == VKV_TEST_NUM_TEXTURE_SAMPLES; }

// VkvTileSchedule.fill_outside (the integrator's alone; checked by check_render_params: the whole rectangle, image-indexed outputs): the
// workgroups of a vkv_render_batch launch fill the tiles outside the rect_w x rect_h rectangle themselves, at most kFillPerTile each.  True
// when the launch renders the whole-image schedule of full_x x full_y tiles instead - the same frame either way: vkv_render (argument block
// by value: lean_block), the resident-workgroup schedulers (A/B switches), and a rectangle so small that its tiles could not fill the rest
// (a cheap frame anyway).
inline bool fill_outside_as_whole_image(bool batch, const VkvTuning &T, uint32_t full_x, uint32_t full_y, uint32_t rect_w, uint32_t rect_h)
{
	const uint64_t inside = (uint64_t) rect_w * rect_h;
	return !batch || T.scheduler == 1 || T.batch_mode == 1 || (uint64_t) full_x * full_y - inside > (uint64_t) kFillPerTile * inside;
}

// The launch of n filled frames (vkv_render_batch).  The frames share the tile SIZE; their tile counts may differ (every frame of a multi-GPU
// launch has its own screen rectangle): the grid is sized for the largest, a frame's surplus workgroups leave at once.  A frame without tiles
// (nblocks == 0: its argument block is only filled up to its tile count) takes no part in any decision.
struct BatchPlan
{
	uint32_t   max_tiles = 0;        // 0: nothing to launch
	uint32_t   ref = 0;              // the first frame with tiles
	bool       same_count = true;        // every frame has max_tiles tiles
	uint64_t   grid = 0;             // workgroups: the tile count padded to a multiple of 8 (ids are dealt round-robin to the XCDs) x blocks x frames
	bool       too_many = false;        // more than a launch takes (2^31 - 1)
	uint32_t   gpf = 0;              // groups of eight workgroups per frame when the frames run one after the other, 0 = interleaved
	LeanChoice choice = {0, 0};        // one kernel for all frames: the most general choice any of them needs
	bool       no_counts = true;        // no frame reads the per-pixel counters: the loop without them
	bool       pull = false;         // k_raymarch_lean_pull instead of k_raymarch_lean_batch
	uint64_t   units = 0;            // ... its 8x8 units
	uint32_t   pull_grid = 0;        // ... its resident workgroups
};

// choices[i]: choose_lean of frame i (read for frames with tiles only)
inline BatchPlan plan_batch(const RayMarchArgs *frames, const LeanChoice *choices, uint32_t n, const VkvTuning &T, int cu_count)
{
	BatchPlan p;
	for (uint32_t i = n; i-- > 0;)
		if (frames[i].nblocks)
		{
			p.max_tiles = frames[i].tile_count > p.max_tiles ? frames[i].tile_count : p.max_tiles;
			p.ref       = i;
		}
	if (p.max_tiles == 0)
		return p;
	p.choice = choices[p.ref];
	for (uint32_t i = 0; i < n; ++i)
	{
		const RayMarchArgs &a = frames[i];
		p.same_count = p.same_count && a.nblocks != 0 && a.tile_count == p.max_tiles;
		if (a.nblocks == 0)
			continue;
		p.no_counts = p.no_counts && !wants_counts(a);
		// frames that disagree about the tables: the kernel that works the footprint address out in registers serves them all
		if (choices[i].kind != choices[p.ref].kind || choices[i].lds != choices[p.ref].lds || a.lut_words != frames[p.ref].lut_words)
			p.choice = {0, 0};
	}
	p.grid     = (uint64_t) ((p.max_tiles + 7u) / 8u) * 8u * frames[0].blocks_per_tile * n;
	p.too_many = p.grid > 0x7fffffffull;
	// frames interleaved in groups of eight workgroups (default) or one frame after the other (VkvTuning.batch_sequential, A/B
	// switch: measured 0.183 vs 0.169 ms per frame on C3 with 8 frames per launch)
	const bool sequential = T.batch_sequential != 0;
	p.gpf                 = sequential ? (uint32_t) (p.grid / n / 8) : 0u;
	// VkvTuning.batch_mode = 1 (pull): resident workgroups whose waves pull 8x8 units from per-XCD ticket counters, possible when every frame
	// shares the LDS tables (same packed image and extents, TF tables, opacity table) and the tile count its tickets count.  Bit-identical;
	// measured on C3 with 8 frames per launch: the CU stays full (7 900 of 8 192 wave slots against 5 300) and everything but the last marching
	// tiles is done after 0.83 ms instead of 1.0, but those last tiles - the volume's silhouette, 100-250 iterations of cold probes - then run
	// 340 us with their four 8x8 units on four different CUs (150 us as one workgroup on one CU): 0.151 ms per frame against 0.137.  Not the default.
	p.pull  = T.batch_mode == 1 && !sequential && p.same_count;
	p.units = (uint64_t) p.max_tiles * frames[0].blocks_per_tile * 4u * n;
	for (uint32_t i = 1; i < n && p.pull; ++i)
	{
		const RayMarchArgs &a = frames[i], &b = frames[0];
		p.pull = a.packed == b.packed && a.tf_bits == b.tf_bits && a.tf == b.tf && a.addr_lut == b.addr_lut && a.W == b.W && a.H == b.H && a.D == b.D &&
		         memcmp(a.alpha_lut, b.alpha_lut, sizeof(a.alpha_lut)) == 0;
	}
	// eight workgroups of four waves fill a CU's 32 wave slots (the pull kernels are held to 64 VGPRs), never more than there are units / 4; should
	// fewer fit, the surplus workgroups start when others have finished and take what tickets are left
	const uint64_t resident = (uint64_t) 8 * (uint64_t) (cu_count > 1 ? cu_count : 1);
	const uint64_t want     = resident < (p.units + 3) / 4 ? resident : (p.units + 3) / 4;
	p.pull_grid             = (uint32_t) (want < 8 ? 8 : want);
	return p;
}

}        // namespace vkv

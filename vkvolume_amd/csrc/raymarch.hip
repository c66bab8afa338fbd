// raymarch.hip — launchers of the ray-march integrator (device code: raymarch_core.hpp and the headers it includes).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "raymarch_inst.hpp"
#include "launchers.hpp"
#include "render_args.hpp"

// ---------------------------------------------------------------------------------------------------------------
// Start order from measured costs: one workgroup per frame sorts the schedule entries 0 .. count - 1 by the cost the previous frame
// into the same target left in tile_cost, longest first (a counting sort over min(cost, 1023); entries of equal cost keep no
// particular order: any permutation renders the same frame, and tie orders measured the same), writes the order to order_out and
// clears the costs for the frame that is about to be rendered.  Centre-of-image-first is only a guess at "longest first": on C3 the tiles that finish
// last are the volume's silhouette.  With the measured order a launch of 8 frames takes 1.01 instead of 1.10 ms.
// ---------------------------------------------------------------------------------------------------------------
constexpr int kCostBins = 1024;

__device__ __forceinline__ void tile_order_from_cost(uint32_t *__restrict__ cost, uint32_t *__restrict__ order_out, uint32_t count)
{
	__shared__ uint32_t s_bin[kCostBins];        // histogram, then the next free position of every bin
	constexpr int       kPerThread = 40;         // 256 threads x 40 = 10 240 tiles per pass, costs kept in registers between the two passes
	for (int b = threadIdx.x; b < kCostBins; b += blockDim.x)
		s_bin[b] = 0;
	__syncthreads();
	for (uint32_t base = 0; base < count; base += 256u * kPerThread)
	{
		uint32_t c[kPerThread];
#pragma unroll
		for (int j = 0; j < kPerThread; ++j)
		{        // all loads of a thread in flight together (coalesced: consecutive threads, consecutive tiles)
			const uint32_t t = base + (uint32_t) j * 256u + threadIdx.x;
			c[j]             = t < count ? min(cost[t], (uint32_t) kCostBins - 1u) : 0xffffffffu;
		}
		// Half of a frame's tiles cost nothing (no ray of theirs marches): one LDS atomic per tile puts 4 000 of them on ONE address, which the
		// LDS serialises; the zero-cost tiles of a wave are counted with one ballot and one atomic by the wave's first such lane.  (Round 6,
		// the sort alone on 8 160 tiles: 23 us, of which 4.9 launch, ~5 the loads, 3.8 the histogram, 9.3 prefix + scatter - one workgroup is
		// a chain of latencies; it runs once per 8 launches and stream, 0.5 % of the frame time, and was left at that.)
#pragma unroll
		for (int j = 0; j < kPerThread; ++j)
		{
			const bool               zero = c[j] == 0u;
			const unsigned long long zm   = __ballot(zero);
			if (zero)
			{
				if ((zm & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0ull)
					atomicAdd(&s_bin[kCostBins - 1], (uint32_t) __popcll(zm));
			}
			else if (c[j] != 0xffffffffu)
				atomicAdd(&s_bin[kCostBins - 1 - c[j]], 1u);        // bin 0 = the dearest tiles
		}
		if (base + 256u * kPerThread >= count)
		{        // the common case (up to 10 240 tiles, a 2560 x 1024 frame): one pass, the scatter reuses the registers
			__syncthreads();
			if (threadIdx.x < 64)        // (workgroups of 256 threads: four waves find a place on a CU that render workgroups keep full)
			{        // exclusive prefix sum of the 1024 bins by one wave: 16 bins per lane
				uint32_t local[kCostBins / 64], sum = 0;
#pragma unroll
				for (int j = 0; j < kCostBins / 64; ++j)
					local[j] = s_bin[threadIdx.x * (kCostBins / 64) + j], sum += local[j];
				uint32_t incl = sum;
				for (int o = 1; o < 64; o <<= 1)
				{
					const uint32_t up = (uint32_t) __shfl_up((int) incl, o);
					if ((int) threadIdx.x >= o)
						incl += up;
				}
				uint32_t run = incl - sum;
#pragma unroll
				for (int j = 0; j < kCostBins / 64; ++j)
					s_bin[threadIdx.x * (kCostBins / 64) + j] = run, run += local[j];
			}
			__syncthreads();
			if (base == 0)
			{
#pragma unroll
				for (int j = 0; j < kPerThread; ++j)
				{
					const uint32_t           t    = (uint32_t) j * 256u + threadIdx.x;
					const bool               zero = c[j] == 0u;
					const unsigned long long zm   = __ballot(zero);
					if (zero)
					{        // the wave's zero-cost tiles take consecutive places behind one atomic (their costs are zero already)
						const unsigned long long below = zm & ((1ull << (threadIdx.x & 63u)) - 1ull);
						uint32_t                 first = 0;
						if (below == 0ull)
							first = atomicAdd(&s_bin[kCostBins - 1], (uint32_t) __popcll(zm));
						first = (uint32_t) __shfl((int) first, __ffsll((long long) zm) - 1);
						order_out[first + (uint32_t) __popcll(below)] = t;
					}
					else if (c[j] != 0xffffffffu)
					{
						order_out[atomicAdd(&s_bin[kCostBins - 1 - c[j]], 1u)] = t;
						cost[t] = 0;
					}
				}
				return;
			}
		}
	}
	// larger schedules: second pass over memory
	for (uint32_t t = threadIdx.x; t < count; t += blockDim.x)
	{
		const uint32_t pos = atomicAdd(&s_bin[kCostBins - 1 - min(cost[t], (uint32_t) kCostBins - 1u)], 1u);
		if (pos < count)        // always, unless somebody changed the costs between the two passes
			order_out[pos] = t;
		cost[t] = 0;
	}
}

__global__ void __launch_bounds__(256) k_tile_order_from_cost(uint32_t *__restrict__ cost, uint32_t *__restrict__ order_out, uint32_t count)
{
	tile_order_from_cost(cost, order_out, count);
}

// the frames of a batch whose argument block asks for it (order_out set)
__global__ void __launch_bounds__(256) k_tile_orders_from_cost(const RayMarchArgs *__restrict__ frames)
{
	const RayMarchArgs &A = frames[blockIdx.x];
	if (A.order_out)
		tile_order_from_cost(A.tile_cost, A.order_out, A.tile_count);
}

namespace vkv
{

LeanChoice choose_lean(const RayMarchArgs &a, const VkvTuning &T)
{
	const size_t lut_bytes = (size_t) a.lut_words * sizeof(uint32_t);
	if (!a.packed || !a.addr_lut || lut_bytes > kMaxLutBytes || !map_fits_u24((uint32_t) a.mw, (uint32_t) a.mh, (uint32_t) a.md))
		return {0, lean_lds_bytes(0, 0, a.W, a.H, a.D)};
	const bool        no_full  = T.address_tables < 2;        // A/B switch: two-level only
	const size_t      full_end = kFullLutWord * 4 + full_lut_bytes(a.W, a.H, a.D);        // from the start of RmLds
	// the full tables hold offsets in units of two bytes in 32 bits: a packed image of up to 8 GiB
	const bool        fits_u32 = packed_bytes(packed_dims(a.W, a.H, a.D)) <= (1ull << 33);
	if (!no_full && fits_u32 && a.lut_full != 0 && full_end <= (size_t) T.full_table_lds_limit)        // (lut_full: the prebuilt tables exist)
		return {2, lean_lds_bytes(2, a.lut_words, a.W, a.H, a.D)};
	return {1, lean_lds_bytes(1, a.lut_words, a.W, a.H, a.D)};
}

// (skipping type, early ray termination) -> the translation unit that holds the kernels of that pair: f(RayMarchLaunchers<SKIP, ERT>{});
// false for a bad skipping type
template <class F>
static bool with_launchers(int skip, bool ert, F &&f)
{
	switch (skip)
	{
		case VKV_SKIP_NONE: ert ? f(RayMarchLaunchers<VKV_SKIP_NONE, true>{}) : f(RayMarchLaunchers<VKV_SKIP_NONE, false>{}); return true;
		case VKV_SKIP_BLOCK: ert ? f(RayMarchLaunchers<VKV_SKIP_BLOCK, true>{}) : f(RayMarchLaunchers<VKV_SKIP_BLOCK, false>{}); return true;
		case VKV_SKIP_DISTANCE: ert ? f(RayMarchLaunchers<VKV_SKIP_DISTANCE, true>{}) : f(RayMarchLaunchers<VKV_SKIP_DISTANCE, false>{}); return true;
		case VKV_SKIP_ANISOTROPIC_DISTANCE: ert ? f(RayMarchLaunchers<VKV_SKIP_ANISOTROPIC_DISTANCE, true>{}) : f(RayMarchLaunchers<VKV_SKIP_ANISOTROPIC_DISTANCE, false>{}); return true;
		default: return false;
	}
}

// the start-order kernels of this file (vkv_register_target: the first launch into a registered target would load them otherwise)
void load_feedback_code()
{
	hipFuncAttributes at;
	(void) hipFuncGetAttributes(&at, reinterpret_cast<const void *>(&k_tile_order_from_cost));
}

// the conservative pixel bound of the clipped box (screen_bound: ../host/host_arith.cpp) as the kernel's cull rectangle
static void screen_bound_of_box(RayMarchArgs &a, const VkvTuning &T)
{
	a.cull_x0 = 0u, a.cull_x1 = ~0u, a.cull_y0 = 0u, a.cull_y1 = ~0u;
	if (!T.screen_cull)        // A/B switch
		return;
	double    b[4];
	const int kind = screen_bound(a.cam, a.dir00, a.ddx, a.ddy, a.plane_tex, b);
	if (kind == kScreenBoundNone)
		return;
	if (kind == kScreenBoundEmpty)
	{        // nothing of the clipped box is on screen: an empty bound
		a.cull_x0 = 1u, a.cull_x1 = 0u;
		return;
	}
	a.cull_x0 = b[0] <= 0.0 ? 0u : (uint32_t) b[0], a.cull_y0 = b[2] <= 0.0 ? 0u : (uint32_t) b[2];
	a.cull_x1 = b[1] >= 4.0e9 ? ~0u : (uint32_t) b[1], a.cull_y1 = b[3] >= 4.0e9 ? ~0u : (uint32_t) b[3];
}

// VkvRenderParams -> kernel arguments.  Returns VKV_OK with a.nblocks == 0 when the schedule is empty.
int fill_render_args(vkv_ctx *ctx, const VkvRenderParams *P, const float *alpha_lut, RayMarchArgs &a, hipStream_t s, const VkvTuning &T, bool setup, bool batch)
{
	bool whole_schedule = fill_shared_args(P, a);        // every tile of the image is scheduled (no rectangle, or a fill_outside rectangle rewritten below)
	for (int i = 0; i < 3; ++i)
		a.block_size[i] = P->ray_cast.block_size[i], a.block_rcp[i] = pow2_reciprocal(a.block_size[i]);
	a.block_pow2 = (a.block_rcp[0] != 0.0f && a.block_rcp[1] != 0.0f && a.block_rcp[2] != 0.0f) ? 1u : 0u;
	a.ord_lo0 = (div_ordinary(a.block_size[0]) && div_ordinary(a.block_size[1]) && div_ordinary(a.block_size[2])) ? ~0u : 0u;
	a.grad_modifier = P->transfer_function.grad_magnitude_modifier;
	a.grad = P->d_gradient, a.tf = P->d_transfer_function;
	a.tf_bits = P->d_transfer_function_bits;
	for (int i = 0; i < 8; ++i)
		a.maps[i] = P->d_distance_maps[i];
	a.in_depth = P->d_in_depth;        // whatever options.depth_attachment says (the direct renderers pass it only when that is set)
	a.blend    = P->blend_over_target != 0;
	a.fill_rgba8_rows = (a.out_rgba8 && !a.out_color && !a.out_counts && !a.out_depth && !a.blend && (a.img_w & 3u) == 0 && (((uintptr_t) a.out_rgba8) & 15u) == 0) ? 1u : 0u;
	{
		const VkvTileRect &r = P->tiles.rect;
		const uint32_t     full_x = (a.img_w + a.tile_w - 1) / a.tile_w, full_y = (a.img_h + a.tile_h - 1) / a.tile_h;
		a.fill_tiles = 0, a.img_tiles_x = full_x, a.rect_tx0 = a.rect_ty0 = a.rect_th = 0;
		if (!whole_schedule && P->tiles.fill_outside)
		{
			// fill_outside (the integrator's alone; checked by check_render_params: the whole rectangle, image-indexed outputs): the workgroups of a
			// vkv_render_batch launch fill the tiles outside the rectangle themselves; vkv_render (argument block by value: lean_block) and the
			// resident-wave schedulers (A/B switches) simply render the whole-image schedule - the same frame either way
			if (!batch || T.scheduler == 1 || T.batch_mode == 1 || (uint64_t) full_x * full_y - (uint64_t) r.w * r.h > (uint64_t) kFillPerTile * r.w * r.h)
			{        // (also a rectangle so small that its tiles could not fill the rest: a cheap frame anyway)
				whole_schedule = true;
				a.tile_count = full_x * full_y, a.tiles_x = full_x, a.org_x = a.org_y = 0u;
			}
			else
				a.fill_tiles = full_x * full_y - r.w * r.h, a.rect_tx0 = r.x0, a.rect_ty0 = r.y0, a.rect_th = r.h;
		}
	}
	// what every wave of the launch would otherwise work out for itself: the divisors of the deal as multiply-and-shift (tiles_x is final here)
	a.div_blocks_per_tile = uniform_div_of(a.blocks_per_tile), a.div_blocks_per_tile_x = uniform_div_of(a.blocks_per_tile_x);
	a.div_tiles_x = uniform_div_of(a.tiles_x), a.div_img_tiles_x = uniform_div_of(a.img_tiles_x), a.div_per_row = uniform_div_of(a.img_tiles_x - a.tiles_x);
	// the limits below and their messages are the integrator's own (the direct renderers' come from check_first_hit_params)
	const uint64_t nb   = (uint64_t) a.blocks_per_tile * a.tile_count;
	a.nblocks           = 0;
	if (nb == 0)
		return VKV_OK;
	if (nb > 0x3fffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "render: too many tiles for one launch");
	// output indices are 32-bit inside the kernel
	if ((uint64_t) a.img_w * a.img_h > 0xffffffffull / 4 || nb * 256 > 0xffffffffull / 4)
		return set_error(ctx, VKV_E_UNSUPPORTED, "render: frame too large for one launch");
	a.nblocks     = (uint32_t) nb;
	a.test        = P->options.test;
	a.queue_heads = nullptr;        // persistent scheduler: set at launch (per-stream scratch)
	a.tile_cost = nullptr, a.order_out = nullptr;        // start-order feedback: attached by the launchers
	a.trace       = reinterpret_cast<unsigned long long *>(ctx->d_trace);
	a.back        = (int) std::ceil(P->transfer_function.sampling_factor);
	a.clamp_always = T.clamp_always != 0 ? 1u : 0u;
	// shape of a wave's pixel patch: VkvTuning.wave_shape (A/B switch), or what the view asks for
	a.wave_pw_log2 = T.wave_shape == 4 ? 2u : (T.wave_shape == 8 ? 3u : (T.wave_shape == 16 ? 4u : wave_patch_log2(a.ddx, a.ddy, a.W, a.H, a.D)));
	{
		const float m[3] = {(float) a.mw, (float) a.mh, (float) a.md};
		const int   e[3] = {a.W, a.H, a.D};
		for (int k = 0; k < 3; ++k)
		{
			a.mapf[k] = m[k], a.mapb[k] = std::nextafterf(m[k], 0.0f);
			a.cells_per_unit[k] = P->options.skipping_type != VKV_SKIP_NONE ? cells_per_unit(e[k], a.block_size[k]) : 0.0f;
		}
		a.free_margin = clamp_free_margin(a.W, a.H, a.D);
	}
	a.addr_lut = nullptr, a.lut_y = a.lut_z = a.lut_words = a.lut_full = 0;
	if (a.packed && T.address_tables != 0)
		a.addr_lut = packed_addr_lut(ctx, a.W, a.H, a.D, &a.lut_y, &a.lut_z, &a.lut_words, &a.lut_full, s, setup);
	screen_bound_of_box(a, T);
	// Start order.  Whole-image schedules: centre of the image first (a cached table per schedule shape).  A schedule that holds every tile of a
	// tile rectangle computes the same kind of order in the kernel (start_entry: the rectangle's rings from the innermost outwards) - a table per
	// rectangle SIZE does not pay when the camera moves (every frame in flight its own 16 KB table through the scalar cache: +2 ... 4 % per frame
	// with 24 in flight, profiles/r6_rect_schedules.txt).  A rank's share of a rectangle (tile_stride > 1) starts in plain order.  A registered
	// target's measured order applies to all of them (apply_feedback).
	a.tile_order = (T.tile_order_linear || !whole_schedule) ? nullptr
	                                                         : tile_start_order(ctx, a.img_w, a.img_h, a.tile_w, a.tile_h, a.tile_first, a.tile_stride, a.tile_count, s, setup);
	a.order_h = 0;
	if (!whole_schedule && !T.tile_order_linear && a.tile_first == 0 && a.tile_stride == 1 && (uint64_t) a.tile_count == (uint64_t) a.tiles_x * P->tiles.rect.h)
		a.order_h = P->tiles.rect.h;
	for (int i = 0; i < 256; ++i)
		a.alpha_lut[i] = alpha_lut[i];
	return VKV_OK;
}

// Start-order feedback.  A renderer draws into the same target again and again with a camera that moves little from frame to frame,
// so the tiles that were expensive last time are expensive now: every marching wave leaves its iteration count in a per-target cost
// buffer (atomicMax per tile), and a small sort kernel behind the render (k_tile_orders_from_cost, one workgroup per frame, same stream)
// turns them into the longest-first order the next frame into that target starts its tiles in.  The per-target device state is created by
// vkv_register_target (a set-up call): a target that was never registered, the first frame into a registered one, and every frame when
// VkvTuning.feedback is 0, use the centre-of-image-first order.  Nothing is allocated, freed or waited for here.  Any order renders the
// same frame.  Returns true when `a` now asks for a sort (order_out set).
static bool apply_feedback(vkv_ctx *ctx, RayMarchArgs &a, hipStream_t s)
{
	(void) s;
	// costs are measured (and sorted behind the render) on the first frame into a target and then every `period`-th one: a camera that
	// moves little keeps the order good for a few frames, and the sort kernel + the cost atomics are then paid once per period
	const void *      target = a.out_rgba8 ? (const void *) a.out_rgba8 : (const void *) a.out_color;
	vkv_ctx::TileFeedback *     f = nullptr;
	std::lock_guard<std::mutex> lock(ctx->mutex);
	const uint32_t              period = ctx->tuning.feedback_period < 1u ? 1u : ctx->tuning.feedback_period;
	if (!ctx->tuning.feedback || !target || a.tile_count < 64 || ctx->d_debug_orders)
		return false;
	for (auto &e : ctx->feedback)
		if (e->target == target && e->img_w == a.img_w && e->img_h == a.img_h && e->tile_w == a.tile_w && e->tile_h == a.tile_h && e->first == a.tile_first &&
		    e->stride == a.tile_stride && e->count == a.tile_count && e->org_x == a.org_x && e->org_y == a.org_y && e->tiles_x == a.tiles_x)
		{
			f = e.get();
			break;
		}
	if (!f)
		return false;        // not registered (or registered for another schedule): centre-first
	// the view of this frame: central ray (normalised) and camera position in texture space.  Costs measured on a view that was more
	// than ~12 degrees away (or from a camera that has moved by more than a fifth of its distance to the volume's centre) say little
	// about this frame - an order sorted by them scatters the heavy tiles (measured: -3 % for targets that alternate between views
	// 45 degrees apart) - so such a frame starts centre-first.
	float dir[3], len2 = 0.0f;
	for (int i = 0; i < 3; ++i)
	{
		dir[i] = a.dir00[i] + 0.5f * ((float) a.img_w * a.ddx[i] + (float) a.img_h * a.ddy[i]);
		len2 += dir[i] * dir[i];
	}
	const float inv = len2 > 0.0f ? 1.0f / std::sqrt(len2) : 0.0f;
	float       cosine = 0.0f, moved2 = 0.0f, dist2 = 0.0f;
	for (int i = 0; i < 3; ++i)
	{
		dir[i] *= inv;
		cosine += dir[i] * f->view_dir[i];
		moved2 += (a.cam[i] - f->view_pos[i]) * (a.cam[i] - f->view_pos[i]);
		dist2 += (f->view_pos[i] - 0.5f) * (f->view_pos[i] - 0.5f);
	}
	const bool     stale   = f->has_cost && !(cosine >= 0.978f && moved2 <= 0.04f * dist2);
	const uint32_t since   = f->frames - f->measured_at;
	// Round 6: a target is only measured again while its camera holds still or moves slowly - this frame's view within the same ~12 degrees
	// of the PREVIOUS frame into the target.  A camera that moves fast between a target's frames (24 targets in flight and one degree per
	// frame: 6 - 72 degrees from one frame into a target to the next) cannot use a measured order, and measuring cost it 0.3 - 2.9 % (the
	// cost atomics of every measured frame, the sort behind it: profiles/r6_feedback_moving_camera.txt); now it pays for the first frame only.
	float prev_cos = 0.0f, prev_moved2 = 0.0f, prev_dist2 = 0.0f;
	for (int i = 0; i < 3; ++i)
	{
		prev_cos += dir[i] * f->prev_dir[i];
		prev_moved2 += (a.cam[i] - f->prev_pos[i]) * (a.cam[i] - f->prev_pos[i]);
		prev_dist2 += (f->prev_pos[i] - 0.5f) * (f->prev_pos[i] - 0.5f);
	}
	const bool steady = f->has_prev && prev_cos >= 0.978f && prev_moved2 <= 0.04f * prev_dist2;
	for (int i = 0; i < 3; ++i)
		f->prev_dir[i] = dir[i], f->prev_pos[i] = a.cam[i];
	f->has_prev        = true;
	const bool measure = !f->has_cost || (since >= f->period && steady);
	if (measure)
	{
		// a measurement whose order no frame could use (the target kept jumping between far views) doubles the distance to the next
		// one, up to 8 periods: such a target then pays next to nothing for the feedback it cannot use
		f->period      = (f->has_cost && f->used == 0) ? std::min(2u * f->period, 8u * period) : period;
		f->measured_at = f->frames;
		f->used        = 0;
	}
	++f->frames;
	if (f->has_cost && !stale)
	{
		a.tile_order = f->d_order.get();        // the order the last sort behind a frame into this target left
		++f->used;
	}
	if (!measure)
		return false;
	for (int i = 0; i < 3; ++i)
		f->view_dir[i] = dir[i], f->view_pos[i] = a.cam[i];
	a.tile_cost = f->d_cost.get();
	a.order_out = f->d_order.get();        // written by the sort that FOLLOWS this frame's render on the stream
	f->has_cost = true;
	return true;
}

int launch_render(vkv_ctx *ctx, const VkvRenderParams *P, const float *alpha_lut, hipStream_t s)
{
	const VkvTuning T = tuning_of(ctx);
	RayMarchArgs a;
	const int    rc = fill_render_args(ctx, P, alpha_lut, a, s, T, false, false);
	if (rc != VKV_OK || a.nblocks == 0)
		return rc;

	// scheduler: one lane per ray on static 8x8 tiles; VkvTuning.scheduler = 1 selects the lane-refilling persistent
	// waves (bit-identical output; measured 2.7x slower: the re-fill breaks the spatial coherence of a wave)
	const int   sched = T.scheduler == 1 ? (int) kSchedPersistent : (int) kSchedLean;

	const bool ert  = P->options.early_ray_termination != 0;
	const int  grad = !P->transfer_function.use_gradient ? 0 : (P->use_precomputed_gradient ? 1 : 2);
	// start-order feedback as in vkv_render_batch (with early ray termination only; the sort runs BEHIND the render on the stream): a
	// frame that runs alone also ends earlier when its long tiles start first (C3: 0.256 -> 0.246 ms)
	const bool sort = sched == (int) kSchedLean && ert && apply_feedback(ctx, a, s);
	int        rc2 = VKV_OK;
	if (!with_launchers(P->options.skipping_type, ert, [&](auto l) { rc2 = decltype(l)::single(ctx, sched, T, grad, a, s); }))
		rc2 = set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: bad skipping_type %d", P->options.skipping_type);
	if (rc2 == VKV_OK && sort)
	{
		hipLaunchKernelGGL(k_tile_order_from_cost, dim3(1), dim3(256), 0, s, a.tile_cost, a.order_out, a.tile_count);
		rc2 = check_launch(ctx, "render (start order)");
	}
	return rc2;
}

// vkv_prepare_render: everything a later launch of these parameter blocks on `s` takes from the context, created now (set-up call)
int prepare_render(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, hipStream_t s)
{
	const VkvTuning T = tuning_of(ctx);
	float           lut[256] = {};
	for (uint32_t i = 0; i < n; ++i)
	{
		RayMarchArgs a;
		int rc = fill_render_args(ctx, &P[i], lut, a, s, T, true, false);
		if (rc == VKV_OK && P[i].tiles.fill_outside)        // (a fill_outside schedule starts its tiles in another order in a batch launch: both tables)
			rc = fill_render_args(ctx, &P[i], lut, a, s, T, true, true);
		if (rc != VKV_OK)
			return rc;
		(void) with_launchers(P[i].options.skipping_type, P[i].options.early_ray_termination != 0, [](auto l) { decltype(l)::load(); });
	}
	load_feedback_code();
	if (!stream_scratch(ctx, s, true).p)
		return VKV_E_UNSUPPORTED;
	return VKV_OK;
}

// ---- several frames in one launch (vkv_render_batch) --------------------------------------------------------------
int launch_render_batch(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, const float *alpha_luts, hipStream_t s)
{
	// the argument blocks go through this stream's scratch buffer: an earlier batch on the same stream has finished with it by the
	// time the copy (same stream) runs, and the block's lock keeps other threads' writes into it (same stream) out from the copy to the
	// launch
	static_assert(kMaxBatch * sizeof(RayMarchArgs) <= kScratchBytes - kBatchArgsOffset, "batch argument blocks must fit the stream scratch");
	static_assert(kPullHeadsBytes + kMaxBatch * sizeof(RayMarchArgs) <= kCaptureSlotBytes, "a captured launch's upload must fit its pinned slot");
	static_assert(kPullHeadsBytes + kMaxBatch * sizeof(RayMarchArgs) <= kUploadSlotBytes, "a launch's upload must fit a slot of the block's pinned ring");
	const VkvTuning     T = tuning_of(ctx);
	const StreamScratch scratch = stream_scratch(ctx, s);
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
	const bool             capturing = hipStreamIsCapturing(s, &capture) == hipSuccess && capture == hipStreamCaptureStatusActive;
	// The upload - the (zeroed) ticket counters of the pull kernel, then the argument blocks - is assembled once, in place, in a pinned slot of
	// the block's ring: no pageable source that the runtime has to stage, nothing allocated.  A slot is free once the event behind the copy
	// that read it has completed; with every slot still in flight (or none: a block beyond the reserve, a captured launch, which has a slot
	// of its own below) the upload comes from pageable memory as before - never a wait.
	const size_t          upload_bytes = kPullHeadsBytes + n * sizeof(RayMarchArgs);
	vkv_ctx::UploadSlot * ring_slot = nullptr;
	for (uint32_t k = 0; k < vkv_ctx::kUploadRing && !capturing && !ring_slot; ++k)
	{
		vkv_ctx::UploadSlot &u = scratch.block->upload[(scratch.block->upload_next + k) % vkv_ctx::kUploadRing];
		if (!u.pinned)
			continue;
		if (u.pending && hipEventQuery(u.done.get()) == hipSuccess)
			u.pending = false;
		if (!u.pending)
		{
			ring_slot                  = &u;
			scratch.block->upload_next = (scratch.block->upload_next + k + 1) % vkv_ctx::kUploadRing;
		}
	}
	(void) hipGetLastError();        // (a slot that is still being read answers hipErrorNotReady: not this launch's error)
	std::vector<uint8_t> pageable;
	if (!ring_slot)
		pageable.resize(upload_bytes);
	uint8_t *const upload = ring_slot ? ring_slot->pinned : pageable.data();
	std::memset(upload, 0, upload_bytes);        // the counters, and every field fill_render_args leaves alone (an empty frame's block)
	RayMarchArgs *const host = reinterpret_cast<RayMarchArgs *>(upload + kPullHeadsBytes);
	for (uint32_t i = 0; i < n; ++i)
	{
		const int rc = fill_render_args(ctx, &P[i], alpha_luts + (size_t) i * 256, host[i], s, T, false, true);
		if (rc != VKV_OK)
			return rc;
		if (!host[i].packed)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: frame %u has no packed sampling image (d_packed_volume)", i);
		// the frames of a launch share the tile SIZE; their tile counts may differ (every frame of a multi-GPU launch has its own screen
		// rectangle): the grid is sized for the largest, a frame's surplus workgroups leave at once
		if (host[i].blocks_per_tile != host[0].blocks_per_tile)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: frame %u has a different tile size than frame 0", i);
		if (ctx->d_debug_orders && i < ctx->debug_order_frames && ctx->debug_order_count == host[i].tile_count)
			host[i].tile_order = ctx->d_debug_orders + (size_t) i * ctx->debug_order_count;        // diagnostic start orders
	}
	uint32_t max_tiles = 0, ref = 0;        // ref: the first frame with tiles (an empty frame's argument block is only filled up to its tile count)
	bool     same_count = true;
	for (uint32_t i = n; i-- > 0;)
	{
		max_tiles = std::max(max_tiles, host[i].nblocks ? host[i].tile_count : 0u);
		if (host[i].nblocks)
			ref = i;
	}
	if (max_tiles == 0)
		return VKV_OK;
	for (uint32_t i = 0; i < n; ++i)
		same_count = same_count && host[i].nblocks != 0 && host[i].tile_count == max_tiles;
	// measured start order only with early ray termination: without it every covered tile is about equally long, nothing is gained by
	// starting the longest first, and an order sorted by cost scatters neighbouring tiles (C3 without ERT: 0.394 against 0.373 ms per frame)
	bool any_sort = false;
	for (uint32_t i = 0; i < n && P[0].options.early_ray_termination != 0; ++i)
		any_sort = apply_feedback(ctx, host[i], s) || any_sort;
	RayMarchArgs *   d_frames = reinterpret_cast<RayMarchArgs *>(scratch.p + kBatchArgsOffset);
	uint32_t *       d_heads  = reinterpret_cast<uint32_t *>(scratch.p + kBatchArgsOffset - kPullHeadsBytes);
	const void *upload_src = upload;
	// a capture slot taken below returns to the context on every error path: only a launch that was recorded keeps it
	struct SlotGuard
	{
		vkv_ctx *ctx;
		size_t   index;
		bool     armed;
		~SlotGuard()
		{
			if (!armed)
				return;
			std::lock_guard<std::mutex> lock(ctx->mutex);
			if (index < ctx->capture_slots.size())
				ctx->capture_slots[index].in_use = false, ctx->capture_slots[index].owner = VkvStreamKey{};
		}
	} slot_guard{ctx, 0, false};
	{        // A stream that is being captured into a hipGraph records the copy's SOURCE POINTER and reads it at every replay: the block then has to
		 // outlive the call - a pinned slot the context keeps until vkv_trim / vkv_destroy
		if (capturing)
		{
			// A captured launch gets a slot of its own - pinned source AND device target of the upload: the graph can be replayed on any stream,
			// concurrently with other graphs and with live launches on the capture stream, so it must not go through that stream's scratch block
			// (whose users are serialised by the stream, which a replay elsewhere is not).  vkv_create set kCaptureSlots slots aside, so that the
			// usual capture allocates nothing; beyond them a slot is allocated here, with this thread's capture mode relaxed for the calls (an
			// allocation under the global / thread-local mode would invalidate the capture).  Slots return with vkv_release_captured(stream),
			// vkv_trim and vkv_destroy.
			std::lock_guard<std::mutex> lock(ctx->mutex);
			vkv_ctx::CaptureSlot *      slot = nullptr;
			for (auto &c : ctx->capture_slots)
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
					return set_error(ctx, VKV_E_UNSUPPORTED, "render_batch: no argument block for a captured launch: %s", hipGetErrorString(ea != hipSuccess ? ea : eb));
				c.pinned = static_cast<uint8_t *>(hp), c.device = static_cast<uint8_t *>(dp);
				c.own_pinned.reset(c.pinned), c.own_device.reset(c.device);        // the context's from here on
				ctx->capture_slots.push_back(std::move(c));
				slot = &ctx->capture_slots.back();
			}
			slot->in_use = true, slot->owner = stream_key(s);
			slot_guard.index = (size_t) (slot - ctx->capture_slots.data()), slot_guard.armed = true;
			std::memcpy(slot->pinned, upload, upload_bytes);
			upload_src = slot->pinned;
			d_heads    = reinterpret_cast<uint32_t *>(slot->device);
			d_frames   = reinterpret_cast<RayMarchArgs *>(slot->device + kPullHeadsBytes);
		}
	}
	const hipError_t e = hipMemcpyAsync(d_heads, upload_src, upload_bytes, hipMemcpyHostToDevice, s);
	if (e != hipSuccess)
		return set_error(ctx, (int) e, "render_batch: argument upload: %s", hipGetErrorString(e));
	if (ring_slot)
	{        // the slot is the copy's source until this event has completed; if it cannot be recorded, wait for the copy here
		if (hipEventRecord(ring_slot->done.get(), s) == hipSuccess)
			ring_slot->pending = true;
		else
			(void) hipStreamSynchronize(s);
	}
	const uint64_t grid = (uint64_t) ((max_tiles + 7u) / 8u) * 8u * host[0].blocks_per_tile * n;
	if (grid > 0x7fffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "render_batch: too many workgroups for one launch");
	const bool ert  = P[0].options.early_ray_termination != 0;
	const int  grad = !P[0].transfer_function.use_gradient ? 0 : (P[0].use_precomputed_gradient ? 1 : 2);
	// frames interleaved in groups of eight workgroups (default) or one frame after the other (VkvTuning.batch_sequential, A/B
	// switch: measured 0.183 vs 0.169 ms per frame on C3 with 8 frames per launch)
	const bool        sequential = T.batch_sequential != 0;
	const uint32_t    gpf        = sequential ? (uint32_t) (grid / n / 8) : 0u;
	LeanChoice        choice     = choose_lean(host[ref], T);
	bool              no_counts  = true;        // no frame reads the per-pixel counters (no counter buffer, no sample-count test output): the loop without them
	for (uint32_t i = 0; i < n; ++i)
		no_counts = no_counts && (host[i].nblocks == 0 || !wants_counts(host[i]));
	for (uint32_t i = 0; i < n; ++i)
	{        // one kernel for all frames: the most general choice any of them needs
		if (i == ref || host[i].nblocks == 0)
			continue;
		const LeanChoice c = choose_lean(host[i], T);
		if (c.kind != choice.kind || c.lds != choice.lds || host[i].lut_words != host[ref].lut_words)
			choice = {0, 0};
	}
	// VkvTuning.batch_mode = 1 (pull): resident workgroups whose waves pull 8x8 units from per-XCD ticket counters (k_raymarch_lean_pull), possible
	// when every frame shares the LDS tables (same packed image and extents, TF tables, opacity table).  Bit-identical; measured on C3 with 8
	// frames per launch: the CU stays full (7 900 of 8 192 wave slots against 5 300) and everything but the last marching tiles is done after
	// 0.83 ms instead of 1.0, but those last tiles - the volume's silhouette, 100-250 iterations of cold probes - then run 340 us with their
	// four 8x8 units on four different CUs (150 us as one workgroup on one CU): 0.151 ms per frame against 0.137.  Not the default.
	bool              pull      = T.batch_mode == 1 && !sequential && same_count;        // (its tickets count one tile count for every frame)
	const uint64_t    units     = (uint64_t) max_tiles * host[0].blocks_per_tile * 4u * n;
	for (uint32_t i = 1; i < n && pull; ++i)
	{
		const RayMarchArgs &a = host[i], &b = host[0];
		pull = a.packed == b.packed && a.tf_bits == b.tf_bits && a.tf == b.tf && a.addr_lut == b.addr_lut && a.W == b.W && a.H == b.H && a.D == b.D &&
		       std::memcmp(a.alpha_lut, b.alpha_lut, sizeof(a.alpha_lut)) == 0;
	}
	if (!with_launchers(P[0].options.skipping_type, ert, [&](auto l) {
		    if (pull)
			    decltype(l)::pull(ctx, grad, d_frames, n, d_heads, choice, units, s);
		    else
			    decltype(l)::batch(grad, d_frames, n, (uint32_t) grid, gpf, choice, no_counts, s);
	    }))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: bad skipping_type %d", P[0].options.skipping_type);
	// behind the render, on the same stream: the costs it measured become the start order of the next frames into these targets (the
	// sort is not in front of anybody's render this way; in front it cost 70 us per 20-frame block of three launches)
	if (any_sort)
		hipLaunchKernelGGL(k_tile_orders_from_cost, dim3(n), dim3(256), 0, s, d_frames);
	const int rc_launch = check_launch(ctx, "render_batch");
	slot_guard.armed = slot_guard.armed && rc_launch != VKV_OK;
	return rc_launch;
}

}        // namespace vkv

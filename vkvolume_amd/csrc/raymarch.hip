// raymarch.hip — launchers of the ray-march integrator (device code: raymarch_core.hpp and the headers it includes).
#include <algorithm>
#include <cmath>
#include <mutex>

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
			if (fill_outside_as_whole_image(batch, T, full_x, full_y, r.w, r.h))
			{
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
// same frame.  When a target is measured and when its order is used: feedback_step (../host/host_arith.cpp).  Returns true when `a` now
// asks for a sort (order_out set).
static bool apply_feedback(vkv_ctx *ctx, RayMarchArgs &a)
{
	const void *      target = a.out_rgba8 ? (const void *) a.out_rgba8 : (const void *) a.out_color;
	vkv_ctx::TileFeedback *     f = nullptr;
	std::lock_guard<std::mutex> lock(ctx->mutex);
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
	const FeedbackStep step = feedback_step(f->state, frame_view(a.dir00, a.ddx, a.ddy, a.cam, a.img_w, a.img_h), std::max(1u, ctx->tuning.feedback_period));
	if (step.use_order)
		a.tile_order = f->d_order.get();        // the order the last sort behind a frame into this target left
	if (step.measure)
	{
		a.tile_cost = f->d_cost.get();
		a.order_out = f->d_order.get();        // written by the sort that FOLLOWS this frame's render on the stream
	}
	return step.measure;
}

// the two options of a parameter block that select a kernel family: early ray termination, and grad = 0 unused, 1 precomputed map, 2 on the fly
struct RenderKind
{
	bool ert;
	int  grad;
};
static RenderKind render_kind(const VkvRenderParams &P)
{
	return {P.options.early_ray_termination != 0, !P.transfer_function.use_gradient ? 0 : (P.use_precomputed_gradient ? 1 : 2)};
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

	const RenderKind kind = render_kind(*P);
	// start-order feedback as in vkv_render_batch (with early ray termination only; the sort runs BEHIND the render on the stream): a
	// frame that runs alone also ends earlier when its long tiles start first (C3: 0.256 -> 0.246 ms)
	const bool sort = sched == (int) kSchedLean && kind.ert && apply_feedback(ctx, a);
	int        rc2 = VKV_OK;
	if (!with_launchers(P->options.skipping_type, kind.ert, [&](auto l) { rc2 = decltype(l)::single(ctx, sched, T, kind.grad, a, s); }))
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

// ---- several frames in one launch (vkv_render_batch; n <= kMaxBatch) -----------------------------------------------------------------
int launch_render_batch(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, const float *alpha_luts, hipStream_t s)
{
	const VkvTuning     T = tuning_of(ctx);
	const StreamScratch scratch = stream_scratch(ctx, s);        // locked until the last enqueue below
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	BatchUpload         upload(ctx, scratch, s, kPullHeadsBytes + n * sizeof(RayMarchArgs));
	RayMarchArgs *const host = reinterpret_cast<RayMarchArgs *>(upload.host() + kPullHeadsBytes);
	LeanChoice          choices[kMaxBatch] = {};
	for (uint32_t i = 0; i < n; ++i)
	{
		const int rc = fill_render_args(ctx, &P[i], alpha_luts + (size_t) i * 256, host[i], s, T, false, true);
		if (rc != VKV_OK)
			return rc;
		if (!host[i].packed)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: frame %u has no packed sampling image (d_packed_volume)", i);
		if (host[i].blocks_per_tile != host[0].blocks_per_tile)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: frame %u has a different tile size than frame 0", i);
		if (ctx->d_debug_orders && i < ctx->debug_order_frames && ctx->debug_order_count == host[i].tile_count)
			host[i].tile_order = ctx->d_debug_orders + (size_t) i * ctx->debug_order_count;        // diagnostic start orders
		if (host[i].nblocks)
			choices[i] = choose_lean(host[i], T);
	}
	const BatchPlan plan = plan_batch(host, choices, n, T, ctx->cu_count);
	if (plan.max_tiles == 0)
		return VKV_OK;
	const RenderKind kind = render_kind(P[0]);
	// measured start order only with early ray termination: without it every covered tile is about equally long, nothing is gained by
	// starting the longest first, and an order sorted by cost scatters neighbouring tiles (C3 without ERT: 0.394 against 0.373 ms per frame)
	bool any_sort = false;
	for (uint32_t i = 0; i < n && kind.ert; ++i)
		any_sort = apply_feedback(ctx, host[i]) || any_sort;
	const int rc = upload.commit();
	if (rc != VKV_OK)
		return rc;
	if (plan.too_many)
		return set_error(ctx, VKV_E_UNSUPPORTED, "render_batch: too many workgroups for one launch");
	const RayMarchArgs *const d_frames = reinterpret_cast<const RayMarchArgs *>(upload.d_args());
	if (!with_launchers(P[0].options.skipping_type, kind.ert, [&](auto l) {
		    if (plan.pull)
			    decltype(l)::pull(kind.grad, d_frames, n, upload.d_heads(), plan.choice, plan.pull_grid, s);
		    else
			    decltype(l)::batch(kind.grad, d_frames, n, (uint32_t) plan.grid, plan.gpf, plan.choice, plan.no_counts, s);
	    }))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: bad skipping_type %d", P[0].options.skipping_type);
	// behind the render, on the same stream: the costs it measured become the start order of the next frames into these targets (the
	// sort is not in front of anybody's render this way; in front it cost 70 us per 20-frame block of three launches)
	if (any_sort)
		hipLaunchKernelGGL(k_tile_orders_from_cost, dim3(n), dim3(256), 0, s, d_frames);
	const int rc_launch = check_launch(ctx, "render_batch");
	if (rc_launch == VKV_OK)
		upload.keep();
	return rc_launch;
}

}        // namespace vkv

// raymarch_persistent.hpp — the resident-wave scheduler (VkvTuning.scheduler = 1, not the default): k_raymarch_persistent, whose waves pull 8x8
// tiles from per-XCD queues and re-fill lanes whose rays have ended (ballot + mbcnt compaction), and the one-event-per-call loop body it runs
// (ray_event) with its LDS tables (stage_tables); bit-identical to the lean kernels, slower.  Included by raymarch_core.hpp, so that
// raymarch_inst.hpp (launch_one names the kernel) and tools/lab/raymarch_lab.hpp (ray_event, unit_pixel, stage_tables) find it there.
#pragma once

#include "raymarch_args.hpp"
#include "ray_setup.hpp"
#include "volume_sampling.hpp"

// ---------------------------------------------------------------------------------------------------------------
// One iteration of the frag's loop (frag:215-312): either one distance-map probe or one volume sample.
// Returns true when the ray has ended (ran past n_steps, or early ray termination).
// ---------------------------------------------------------------------------------------------------------------
template <int SKIP, bool ERT, int GRAD, bool PACKED>
__device__ __forceinline__ bool ray_event(const RayMarchArgs &A, Ray &R, const float *s_alpha, const float *s_unorm, const uint32_t *s_bits, bool tf_bits)
{
	const int   W = A.W, H = A.H, D = A.D;
	const int   i  = R.i;
	const float fi = (float) i;
	const float posx = __builtin_fmaf(fi, R.sx, R.ex), posy = __builtin_fmaf(fi, R.sy, R.ey), posz = __builtin_fmaf(fi, R.sz, R.ez);
	int         uix = 0, uiy = 0, uiz = 0;
	float       ux = 0, uy = 0, uz = 0;
	if (SKIP != VKV_SKIP_NONE)
	{        // frag:192, 220-221 (volume_to_distance_map_u is the same for every ray)
		const float kx = (float) W / A.block_size[0], ky = (float) H / A.block_size[1], kz = (float) D / A.block_size[2];
		ux = kx * posx, uy = ky * posy, uz = kz * posz;
		uix = i_clamp((int) ux, 0, A.mw - 1), uiy = i_clamp((int) uy, 0, A.mh - 1), uiz = i_clamp((int) uz, 0, A.md - 1);
	}
	const bool probe = SKIP != VKV_SKIP_NONE && !R.occupied && (uix != R.ulx || uiy != R.uly || uiz != R.ulz);        // frag:224

	// ---- issue phase --------------------------------------------------------------------------------------------
	// A wave usually holds probing and sampling lanes at once.  Issue this iteration's loads for BOTH kinds before either
	// is consumed (lanes of the other kind read a dummy address that every lane shares), so the probe's and the sample's
	// memory latencies overlap instead of adding up on the critical path of the wave.
	constexpr bool kHoist = PACKED && GRAD != 2 && SKIP != VKV_SKIP_NONE;
	uint32_t       dist_h = 0, q00 = 0, q10 = 0, q01 = 0, q11 = 0;
	float          hwx = 0, hwy = 0, hwz = 0;
	if (kHoist)
	{
		// a wave whose live lanes all probe (the empty space in front of the volume) or all sample skips the other kind's address
		// arithmetic and loads: wave-uniform scalar branches
		if (__ballot(probe) != 0ull)
		{
			const uint32_t cell = ((uint32_t) uiz * (uint32_t) A.mh + (uint32_t) uiy) * (uint32_t) A.mw + (uint32_t) uix;
			dist_h              = R.dmap[probe ? cell : 0u];
		}
		if (__ballot(!probe) != 0ull)
		{
			const uint8_t *fp = packed_footprint(A.packed, W, H, D, A.pmx, A.pmy, posx, posy, posz, hwx, hwy, hwz);
			const uint8_t *ba = probe ? A.packed : fp;
			q00 = *reinterpret_cast<const u32_align2 *>(ba);
			q10 = *reinterpret_cast<const u32_align2 *>(ba + 10);
			q01 = *reinterpret_cast<const u32_align2 *>(ba + 50);
			q11 = *reinterpret_cast<const u32_align2 *>(ba + 60);
		}
		// keep the five loads above the divergent consume code (the compiler would otherwise sink each into its branch)
		asm volatile("" : "+v"(dist_h), "+v"(q00), "+v"(q10), "+v"(q01), "+v"(q11));
	}

	if (probe)
	{        // frag:224-263
		++R.n_dist;
		uint32_t dist;
		if (kHoist)
			dist = dist_h;
		else
			dist = R.dmap[((uint32_t) uiz * (uint32_t) A.mh + (uint32_t) uiy) * (uint32_t) A.mw + (uint32_t) uix];
		// Both outcomes of the probe are computed and selected (no nested branch: the two groups of lanes would serialise):
		// dist > 0 skips forward (frag:236-247), dist == 0 marks the cell occupied and steps back (frag:248-262).
		// r = clamp(u_i - u, -1, 0) (frag:234); the operand is never NaN, so the median-of-three instruction gives the same
		// value as min(max(x, -1), 0)
		const float rx = __builtin_amdgcn_fmed3f((float) uix - ux, -1.0f, 0.0f);
		const float ry = __builtin_amdgcn_fmed3f((float) uiy - uy, -1.0f, 0.0f);
		const float rz = __builtin_amdgcn_fmed3f((float) uiz - uz, -1.0f, 0.0f);
		float       ax, ay, az;
		if (SKIP == VKV_SKIP_BLOCK)
		{        // frag:239: step(0, s) is 1 for s >= 0 (and for the impossible NaN), 0 for s < 0
			ax = (((R.six < 0.0f) ? 0.0f : 1.0f) + rx) * R.six;
			ay = (((R.siy < 0.0f) ? 0.0f : 1.0f) + ry) * R.siy;
			az = (((R.siz < 0.0f) ? 0.0f : 1.0f) + rz) * R.siz;
		}
		else
		{        // frag:242: step(0, -s) + sign(s) * dist is exactly dist for s > 0 and 1 - dist for s < 0 (s is never 0 or NaN:
			 // it is the reciprocal of a finite number)
			const float fd = (float) dist;
			ax = (((R.six > 0.0f) ? fd : 1.0f - fd) + rx) * R.six;
			ay = (((R.siy > 0.0f) ? fd : 1.0f - fd) + ry) * R.siy;
			az = (((R.siz > 0.0f) ? fd : 1.0f - fd) + rz) * R.siz;
		}
		if (ax != ax) ax = INFINITY;
		if (ay != ay) ay = INFINITY;
		if (az != az) az = INFINITY;
		float m = g_min(g_min(ax, ay), az);
		m       = (m < 1073741824.0f) ? m : 1073741824.0f;
		const int  i_skip = i + max(1, (int) __builtin_ceilf(m));
		const int  i_back = max(i - (int) __builtin_ceilf(A.sampling_factor), R.i_min);
		const bool empty  = dist > 0u;
		R.i               = empty ? i_skip : i_back;
		R.occupied        = !empty;
		R.ulx = empty ? R.ulx : uix, R.uly = empty ? R.uly : uiy, R.ulz = empty ? R.ulz : uiz;
		return R.i >= R.n_steps;
	}

	// frag:266-310
	++R.n_vol;
	uint32_t texel = 0;
	{
	float intensity, gradient = 1.0f;
	if (kHoist)
	{
		float unused;
		if (GRAD == 1)
			packed_filter<true>(q00, q10, q01, q11, hwx, hwy, hwz, intensity, gradient);
		else
			packed_filter<false>(q00, q10, q01, q11, hwx, hwy, hwz, intensity, unused);
	}
	else if (PACKED)
	{
		float unused;
		if (GRAD == 1)
			sample_packed<true>(A.packed, W, H, D, A.pmx, A.pmy, posx, posy, posz, intensity, gradient);
		else
			sample_packed<false>(A.packed, W, H, D, A.pmx, A.pmy, posx, posy, posz, intensity, unused);
	}
	else
	{
		intensity = sample_linear(A.vol, W, H, D, posx, posy, posz);
		if (GRAD == 1)
			gradient = sample_linear(A.grad, W, H, D, posx, posy, posz);
	}
	if (GRAD == 2)
	{        // frag:92-97
		const float dix = 1.0f / (float) W, diy = 1.0f / (float) H, diz = 1.0f / (float) D;
		float       t1, t2, t3, t4, unused;
		if (PACKED)
		{
			sample_packed<false>(A.packed, W, H, D, A.pmx, A.pmy, posx + dix, posy - diy, posz - diz, t1, unused);
			sample_packed<false>(A.packed, W, H, D, A.pmx, A.pmy, posx - dix, posy - diy, posz + diz, t2, unused);
			sample_packed<false>(A.packed, W, H, D, A.pmx, A.pmy, posx - dix, posy + diy, posz - diz, t3, unused);
			sample_packed<false>(A.packed, W, H, D, A.pmx, A.pmy, posx + dix, posy + diy, posz + diz, t4, unused);
		}
		else
		{
			t1 = sample_linear(A.vol, W, H, D, posx + dix, posy - diy, posz - diz);
			t2 = sample_linear(A.vol, W, H, D, posx - dix, posy - diy, posz + diz);
			t3 = sample_linear(A.vol, W, H, D, posx - dix, posy + diy, posz - diz);
			t4 = sample_linear(A.vol, W, H, D, posx + dix, posy + diy, posz + diz);
		}
		const float gx = (((t1 - t2) - t3) + t4) * 0.25f;
		const float gy = (((-t1 - t2) + t3) + t4) * 0.25f;
		const float gz = (((-t1 + t2) - t3) + t4) * 0.25f;
		const float len = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
		gradient = g_clamp(len * A.grad_modifier, 0.0f, 1.0f);
	}
	// get_color (transfer_function.glsl:35-38): NEAREST texel.  With the bit table the occupied test (frag:276) comes
	// from LDS and only occupied samples pay the dependent RGBA fetch.
	const uint32_t tidx  = (uint32_t) tf_texel(gradient) * 256u + (uint32_t) tf_texel(intensity);
	if (tf_bits)
	{
		if ((s_bits[tidx >> 5] >> (tidx & 31u)) & 1u)
			texel = reinterpret_cast<const uint32_t *>(A.tf)[tidx];
	}
	else
		texel = reinterpret_cast<const uint32_t *>(A.tf)[tidx];
	}
	const uint32_t ab = texel >> 24;
	R.occupied        = ab > 0;
	bool ended        = false;
	if (R.occupied)
	{
		if (SKIP != VKV_SKIP_NONE)
			R.ulx = uix, R.uly = uiy, R.ulz = uiz;
		const float a  = s_alpha[ab];        // frag:283
		// R8G8B8A8_UNORM -> float is exactly c / 255: read from the LDS table the workgroup filled with that division
		const float r_ = s_unorm[texel & 255u] * a, g_ = s_unorm[(texel >> 8) & 255u] * a, b_ = s_unorm[(texel >> 16) & 255u] * a;
		const float om = 1.0f - R.a;         // frag:287
		R.r = __builtin_fmaf(om, r_, R.r), R.g = __builtin_fmaf(om, g_, R.g), R.b = __builtin_fmaf(om, b_, R.b);
		R.a = __builtin_fmaf(om, a, R.a);
		if (a > 0.0f)
			R.first_hit = i;
		if (ERT && R.a > 0.99f)
		{        // frag:293-299
			R.a   = 1.0f;
			ended = true;
		}
	}
	else
		++R.n_empty;
	if (!ended)
	{
		R.i     = i + 1;
		R.i_min = R.i;
		ended   = R.i >= R.n_steps;
	}
	return ended;
}

// 8x8 work unit `u` (4 per 16x16 block of the tile schedule) + ray slot in the unit -> pixel and output index.
__device__ __forceinline__ bool unit_pixel(const RayMarchArgs &A, uint32_t u, uint32_t slot, uint32_t &px, uint32_t &py, uint32_t &o)
{
	const uint32_t b = u >> 2, w = u & 3u;
	const uint32_t k = b / A.blocks_per_tile, sb = b % A.blocks_per_tile;
	const uint32_t t = A.tile_first + k * A.tile_stride;
	const uint32_t lx = (sb % A.blocks_per_tile_x) * 16 + (w & 1) * 8 + (slot & 7);
	const uint32_t ly = (sb / A.blocks_per_tile_x) * 16 + (w >> 1) * 8 + (slot >> 3);
	px = A.org_x + (t % A.tiles_x) * A.tile_w + lx, py = A.org_y + (t / A.tiles_x) * A.tile_h + ly;
	o  = A.compact ? (k * A.tile_h + ly) * A.tile_w + lx : py * A.img_w + px;
	return px < A.img_w && py < A.img_h;
}

__device__ __forceinline__ void stage_tables(const RayMarchArgs &A, float *s_alpha, float *s_unorm, uint32_t *s_bits)
{
	for (int i = threadIdx.x; i < 256; i += blockDim.x)
	{
		s_alpha[i] = A.alpha_lut[i];
		s_unorm[i] = unorm8(i);        // exact IEEE division, once per workgroup
	}
	if (A.tf_bits)
		for (int i = threadIdx.x; i < 2048; i += blockDim.x)
			s_bits[i] = A.tf_bits[i];
	__syncthreads();
}
// ---------------------------------------------------------------------------------------------------------------
// Persistent scheduler.
// ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kInvalidUnit  = 0xffffffffu;
constexpr uint32_t kRefillLanes  = 16;        // re-fill a wave once this many lanes are idle

// Queue q owns the schedule's tiles k = q, q + 8, ... (same tile -> XCD mapping as the static scheduler); its v-th
// work unit is 8x8 sub-tile v % upt of its (v / upt)-th tile, upt = 4 * blocks_per_tile units per tile.
__device__ __forceinline__ uint32_t queue_units(const RayMarchArgs &A, uint32_t q)
{
	const uint32_t tiles = A.tile_count > q ? (A.tile_count - q + 7u) >> 3 : 0u;
	return tiles * A.blocks_per_tile * 4u;
}

// Pop one unit for this wave (wave-uniform result).  Starts at the wave's own queue and steals from the others once
// it is empty.  `q` is updated to the queue that delivered.
__device__ __forceinline__ uint32_t pop_unit(const RayMarchArgs &A, uint32_t &q)
{
	const uint32_t upt = A.blocks_per_tile * 4u;
	for (uint32_t tries = 0; tries < 8; ++tries)
	{
		uint32_t v = 0;
		if ((threadIdx.x & 63) == 0)
			v = atomicAdd(&A.queue_heads[q], 1u);
		v = __builtin_amdgcn_readfirstlane(v);
		if (v < queue_units(A, q))
			return ((v / upt) * 8u + q) * upt + v % upt;
		q = (q + 1) & 7u;
	}
	return kInvalidUnit;
}

template <int SKIP, bool ERT, int GRAD, bool PACKED>
__global__ void __launch_bounds__(256) k_raymarch_persistent(const RayMarchArgs A)
{
	__shared__ float    s_alpha[256], s_unorm[256];
	__shared__ uint32_t s_bits[2048];
	stage_tables(A, s_alpha, s_unorm, s_bits);
	const bool     tf_bits = A.tf_bits != nullptr;
	// blocks b and b + 8 share an XCD under the observed round-robin placement (speed only, never correctness)
	uint32_t q      = blockIdx.x & 7u;
	uint32_t unit   = pop_unit(A, q);
	uint32_t cursor = 0;        // next unassigned ray slot of `unit`
	bool     active = false;
	Ray      R;
	R.o = 0;

	for (;;)
	{
		uint64_t idle   = __ballot(!active);
		uint32_t n_idle = (uint32_t) __popcll(idle);
		// ---- re-fill: idle lanes take the next ray slots of the current unit, in lane order ----
		while (n_idle >= kRefillLanes && unit != kInvalidUnit)
		{
			const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) idle, 0u));
			const uint32_t take = min(n_idle, 64u - cursor);
			if (!active && rank < take)
			{
				uint32_t px, py, o;
				if (unit_pixel(A, unit, cursor + rank, px, py, o))
				{
					R.o    = o;
					active = ray_setup<SKIP>(A, px, py, R);
					if (!active)
						ray_finish(A, R, false);        // not covered / early-out / entry-exit test: result is final
				}
			}
			cursor += take;
			if (cursor == 64)
			{
				unit   = pop_unit(A, q);
				cursor = 0;
			}
			idle   = __ballot(!active);
			n_idle = (uint32_t) __popcll(idle);
		}
		if (n_idle == 64)
			break;        // nothing in flight and the queues are empty
		// ---- one event per active lane ----
		if (active)
		{
			if (ray_event<SKIP, ERT, GRAD, PACKED>(A, R, s_alpha, s_unorm, s_bits, tf_bits))
			{
				ray_finish(A, R, true);
				active = false;
			}
		}
	}
}

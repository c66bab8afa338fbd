// direct_render.hpp — what the direct renderers share: the maximum-intensity projection (k_mip), the isosurface (k_iso, §5.10),
// the slab (k_slab, §5.11) and the label render (k_labels, §5.21).  Device side: the deal of a launch's workgroups and lanes to pixels, the
// filtered intensity of one sample or of a
// group of samples, the max map's geometry, the grown-cell test and the exact skip step over the per-cell max map (vkv_max_map), the first-hit
// depth and the stores every kernel ends with.  Host side: the checks and the arguments of their four entry points.  k_mip keeps its own inline
// copy of the skip step: calling max_map_skip cost its skipping variant 1-2 % (§5.10).
#pragma once

#include <cmath>

#include "launchers.hpp"
#include "raymarch_args.hpp"
#include "ray_setup.hpp"
#include "render_args.hpp"
#include "volume_sampling.hpp"

// everything here is internal to the translation unit that includes it (no exported symbols)
namespace
{

// The deal of workgroups and lanes to pixels, the integrator's (lean_block): XCD x = id & 7 takes the schedule's tiles x, x + 8, ..., whose blocks
// are neighbouring ids on that XCD (L2 locality); a schedule that holds every tile of its rectangle starts them ring by ring from the middle
// (start_entry), so the long rays through the volume start first.  A workgroup is a 16x16 block of a tile, a wave the (1 << pw) pixels wide
// 64-pixel patch of it (pw = 2, 3, 4: 4x16, 8x8, 16x4).  false: this lane has no pixel; else pixel (px, py) and its output index o (compact:
// inside the launch's own tile buffer).  k_iso holds a written-out copy (iso.hip says why): keep the two in step.
__device__ __forceinline__ bool pixel_deal(const RayMarchArgs &A, uint32_t pw, uint32_t &px, uint32_t &py, uint32_t &o)
{
	const uint32_t x = blockIdx.x & 7u, idx = blockIdx.x >> 3;
	const uint32_t rank = (idx / A.blocks_per_tile) * 8u + x, sb = idx % A.blocks_per_tile;
	if (rank >= A.tile_count)
		return false;
	const uint32_t k_tile = A.order_h ? start_entry(A, rank) : rank;
	if (k_tile >= A.tile_count)
		return false;
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t bx = (w & ((16u >> pw) - 1u)) << pw, by = (w >> (4u - pw)) * (64u >> pw);
	const uint32_t t  = A.tile_first + k_tile * A.tile_stride;
	const uint32_t lx = (sb % A.blocks_per_tile_x) * 16u + bx + (lane & ((1u << pw) - 1u)), ly = (sb / A.blocks_per_tile_x) * 16u + by + (lane >> pw);
	px = A.org_x + (t % A.tiles_x) * A.tile_w + lx, py = A.org_y + (t / A.tiles_x) * A.tile_h + ly;
	o  = A.compact ? (k_tile * A.tile_h + ly) * A.tile_w + lx : py * A.img_w + px;
	return px < A.img_w && py < A.img_h;
}

// workgroups of a launch that pixel_deal serves: the schedule's tile count rounded up to a multiple of 8 (host)
uint32_t deal_grid(const RayMarchArgs &a) { return (a.tile_count + 7u) / 8u * 8u * a.blocks_per_tile; }

// the integrator's first_hit depth (ray_finish, frag:315-321) of the texture-space point (x, y, z): proj view model (p - 0.5, 1), z / w
__device__ __forceinline__ float first_hit_depth(const RayMarchArgs &A, float x, float y, float z)
{
	const float p[4] = {x - 0.5f, y - 0.5f, z - 0.5f, 1.0f};
	float       a4[4], b4[4], c4[4];
	mat4_mul_vec4(A.model, p, a4);
	mat4_mul_vec4(A.view, a4, b4);
	mat4_mul_vec4(A.proj, b4, c4);
	return c4[2] / c4[3];
}

// pixel o of an RGBA8 target (one non-temporal dword), and of the three counters of d_out_counts
__device__ __forceinline__ void store_rgba8_nt(uint8_t *base, size_t o, float r, float g, float b, float a)
{
	__builtin_nontemporal_store((uint32_t) quantise_rgba8(r) | ((uint32_t) quantise_rgba8(g) << 8) | ((uint32_t) quantise_rgba8(b) << 16) |
	                                ((uint32_t) quantise_rgba8(a) << 24),
	                            reinterpret_cast<uint32_t *>(base) + o);
}
__device__ __forceinline__ void store_counts(uint32_t *base, size_t o, uint32_t n_filt, uint32_t n_probe, uint32_t n_skip)
{
	base[o * 3 + 0] = n_filt, base[o * 3 + 1] = n_probe, base[o * 3 + 2] = n_skip;
}

template <bool PACKED>
__device__ __forceinline__ float mip_sample(const RayMarchArgs &A, float posx, float posy, float posz)
{
	if (PACKED)
	{
		float v, unused;
		sample_packed<false>(A.packed, A.W, A.H, A.D, A.pmx, A.pmy, posx, posy, posz, v, unused);
		return v;
	}
	return sample_linear(A.vol, A.W, A.H, A.D, posx, posy, posz);
}

// samples i .. i + G - 1 of a ray: every load first, then the filters (the same bits as mip_sample one by one)
constexpr int kDenseGroup = 4;
template <bool PACKED, int G>
__device__ __forceinline__ void mip_samples(const RayMarchArgs &A, const Ray &R, int i, float *v)
{
	if (PACKED)
	{
		uint32_t q[G][4];
		float    w[G][3];
#pragma unroll
		for (int j = 0; j < G; ++j)
		{
			const float    fi = (float) (i + j);
			const uint8_t *b  = packed_footprint(A.packed, A.W, A.H, A.D, A.pmx, A.pmy, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey),
			                                     __builtin_fmaf(fi, R.sz, R.ez), w[j][0], w[j][1], w[j][2]);
			q[j][0] = *reinterpret_cast<const u32_align2 *>(b);
			q[j][1] = *reinterpret_cast<const u32_align2 *>(b + 10);
			q[j][2] = *reinterpret_cast<const u32_align2 *>(b + 50);
			q[j][3] = *reinterpret_cast<const u32_align2 *>(b + 60);
		}
#pragma unroll
		for (int j = 0; j < G; ++j)
		{
			float unused;
			packed_filter<false>(q[j][0], q[j][1], q[j][2], q[j][3], w[j][0], w[j][1], w[j][2], v[j], unused);
		}
	}
	else
	{
#pragma unroll
		for (int j = 0; j < G; ++j)
		{
			const float fi = (float) (i + j);
			v[j] = sample_linear(A.vol, A.W, A.H, A.D, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey), __builtin_fmaf(fi, R.sz, R.ez));
		}
	}
}

// the largest value a sample can take (a footprint of 255s)
constexpr float kMaxSample = 255.0f * kInv255;

// c = the sampler's voxel coordinate of a sample on one axis; true when it lies in [lo - 1, lo + b): the sample then reads only voxels of the
// cell [lo, lo + b) grown by one voxel
__device__ __forceinline__ bool in_grown(float c, int lo, int b) { return c >= (float) (lo - 1) && c < (float) (lo + b); }

// the max map and its geometry in a kernel's arguments (fill_max_map_geometry); block 1 and cell 0 without a map
struct MaxMapGeometry
{
	const uint8_t *max_map;         // skipping variants only
	int            bx, by, bz;      // voxels per map cell per axis
	int            lcx, lcy, lcz;   // last map cell per axis that holds a voxel: (extent - 1) / block
	float          rbx, rby, rbz;   // 1 / block (finding the cell only; the skip itself is checked exactly)
};

// One probe of the skip step at sample i of n (position pos*).  When sample i enters a map cell other than `last_cell`, the cell's byte B is
// read (++n_probe); when B * kInv255 cannot reach `bound` (STRICT: B * kInv255 < bound; else B * kInv255 <= bound) and the sample lies in the
// grown cell, the result is the last index i + kk (kk >= 0, never past sample n - 1) of the samples i .. i + kk that lie in the grown cell,
// and last_cell is reset.  -1: filter sample i.
template <bool STRICT>
__device__ __forceinline__ int max_map_skip(const RayMarchArgs &A, const MaxMapGeometry &M, const Ray &R, int i, int n, float posx, float posy, float posz,
                                            float bound, uint32_t &last_cell, uint32_t &n_probe)
{
	const float fW = (float) A.W, fH = (float) A.H, fD = (float) A.D;
	// the sampler's own voxel coordinates of this sample (sample_linear / packed_footprint)
	const float cx = __builtin_fmaf(posx, fW, -0.5f), cy = __builtin_fmaf(posy, fH, -0.5f), cz = __builtin_fmaf(posz, fD, -0.5f);
	const int   mx = i_clamp((int) __builtin_floorf((cx + 0.5f) * M.rbx), 0, M.lcx);
	const int   my = i_clamp((int) __builtin_floorf((cy + 0.5f) * M.rby), 0, M.lcy);
	const int   mz = i_clamp((int) __builtin_floorf((cz + 0.5f) * M.rbz), 0, M.lcz);
	const uint32_t cell = ((uint32_t) mz * (uint32_t) A.mh + (uint32_t) my) * (uint32_t) A.mw + (uint32_t) mx;
	if (cell == last_cell)
		return -1;
	++n_probe;
	last_cell = cell;
	const int   lx = mx * M.bx, ly = my * M.by, lz = mz * M.bz;
	const float top = (float) M.max_map[cell] * kInv255;
	if (!((STRICT ? top < bound : top <= bound) && in_grown(cx, lx, M.bx) && in_grown(cy, ly, M.by) && in_grown(cz, lz, M.bz)))
		return -1;
	// samples i .. i + kk: the estimate aims a quarter voxel past the cell's edge (inside the half-voxel margin); the last one is checked exactly
	// below, and the sampler's coordinates are monotone in the sample index, so every sample between lies in the grown cell too
	const float sx = R.sx * fW, sy = R.sy * fH, sz = R.sz * fD;
	const float tx = sx > 0.0f ? ((float) (lx + M.bx) - 0.25f - cx) / sx : (sx < 0.0f ? ((float) lx - 0.75f - cx) / sx : INFINITY);
	const float ty = sy > 0.0f ? ((float) (ly + M.by) - 0.25f - cy) / sy : (sy < 0.0f ? ((float) ly - 0.75f - cy) / sy : INFINITY);
	const float tz = sz > 0.0f ? ((float) (lz + M.bz) - 0.25f - cz) / sz : (sz < 0.0f ? ((float) lz - 0.75f - cz) / sz : INFINITY);
	const float tm = g_min(g_min(tx, ty), g_min(tz, (float) (n - 1 - i)));
	int         kk = tm > 0.0f ? (int) tm : 0;
	if (kk > 0)
	{
		const float fl = (float) (i + kk);
		const float qx = __builtin_fmaf(__builtin_fmaf(fl, R.sx, R.ex), fW, -0.5f);
		const float qy = __builtin_fmaf(__builtin_fmaf(fl, R.sy, R.ey), fH, -0.5f);
		const float qz = __builtin_fmaf(__builtin_fmaf(fl, R.sz, R.ez), fD, -0.5f);
		if (!(in_grown(qx, lx, M.bx) && in_grown(qy, ly, M.by) && in_grown(qz, lz, M.bz)))
			kk = 0;
	}
	last_cell = ~0u;
	return i + kk;
}

// ---- host side: the checks and arguments vkv_render_mip, vkv_render_isosurface and vkv_render_slab share --------------------------------------------------

// the checks of the fields of P a MIP / isosurface call reads (`what`: the entry point's name in the messages), with the max map d_max_map
// (or null) and `has_output`: an output of the call's own options is set; VKV_OK or the code (nothing is enqueued before they pass).
// rays = false (vkv_render_slab): the call casts no rays, so it has no depth (options.depth_attachment and d_out_depth are unsupported) and
// reads no sampling_factor.  needs_volume = false (vkv_render_labels with shade == 0): the call reads no voxel, so d_volume may be null
int check_first_hit_params(vkv_ctx *ctx, const char *what, const VkvRenderParams *P, const uint8_t *d_max_map, bool has_output, bool rays = true,
                           bool needs_volume = true)
{
	if (P->blend_over_target)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: blend_over_target is not supported", what);
	if (P->tiles.fill_outside)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: tiles.fill_outside is not supported", what);
	if (P->options.test != VKV_TEST_NONE)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: test modes are not supported", what);
	if (!rays && (P->options.depth_attachment || P->d_out_depth))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: options.depth_attachment and d_out_depth are not supported", what);
	if (P->options.depth_attachment && !P->d_in_depth)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: options.depth_attachment needs d_in_depth", what);
	if (!extent_ok(P->volume_extent) || P->image_width == 0 || P->image_height == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: zero extent", what);
	if (needs_volume && !P->d_volume)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null volume", what);
	if (rays && !(P->transfer_function.sampling_factor > 0.0f))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: sampling_factor must be positive", what);
	if (d_max_map)
	{
		if (!map_extent_ok(P->volume_extent, P->map_extent))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: the max map needs a valid map_extent", what);
		if ((uint64_t) P->map_extent.width * P->map_extent.height * P->map_extent.depth > 0xffffffffull)
			return set_error(ctx, VKV_E_UNSUPPORTED, "%s: max maps with more than 2^32 cells are not supported", what);
	}
	if (const int rc = check_tile_schedule(ctx, what, P))
		return rc;
	if (const int rc = check_render_buffers(ctx, what, P, has_output))
		return rc;
	const VkvTileSchedule &t = P->tiles;
	const uint64_t nb = (uint64_t) (t.tile_width / 16) * (t.tile_height / 16) * t.tile_count;
	if (nb > 0x3fffffffull || (uint64_t) P->image_width * P->image_height > 0xffffffffull / 4 || nb * 256 > 0xffffffffull / 4)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: frame too large for one launch", what);
	return VKV_OK;
}

// VkvRenderParams -> the fields of RayMarchArgs the direct renderers' kernels read (the rest stays zero)
void fill_direct_args(const VkvRenderParams *P, RayMarchArgs &a)
{
	a                = RayMarchArgs{};
	const bool whole = fill_shared_args(P, a);
	a.in_depth       = P->options.depth_attachment ? P->d_in_depth : nullptr;        // null unless the attachment is on (the integrator passes it as it comes)
	a.nblocks        = a.blocks_per_tile * a.tile_count;        // (within the limits of check_first_hit_params, whose message a too large frame gets)
	a.test           = VKV_TEST_NONE;
	a.wave_pw_log2   = wave_patch_log2(a.ddx, a.ddy, a.W, a.H, a.D);        // the integrator's shape, without its VkvTuning.wave_shape override
	// a schedule over every tile of its rectangle starts in the integrator's ring order, computed (start_entry) for the whole image too: the
	// integrator reads its cached table there
	const uint32_t rows = whole ? (a.img_h + a.tile_h - 1) / a.tile_h : P->tiles.rect.h;
	a.order_h           = (a.tile_first == 0 && a.tile_stride == 1 && (uint64_t) a.tile_count == (uint64_t) a.tiles_x * rows) ? rows : 0u;
}

// the max map d_max_map (or null) of a call as its kernel reads it
void fill_max_map_geometry(const VkvRenderParams *P, const uint8_t *d_max_map, MaxMapGeometry &m)
{
	m.max_map = d_max_map;
	m.bx = m.by = m.bz = 1, m.lcx = m.lcy = m.lcz = 0, m.rbx = m.rby = m.rbz = 1.0f;
	if (d_max_map)
	{
		const VkvExtent3D e = P->volume_extent, me = P->map_extent;
		m.bx = (int) block_of(e.width, me.width), m.by = (int) block_of(e.height, me.height), m.bz = (int) block_of(e.depth, me.depth);
		m.lcx = (int) (e.width - 1) / m.bx, m.lcy = (int) (e.height - 1) / m.by, m.lcz = (int) (e.depth - 1) / m.bz;
		m.rbx = 1.0f / (float) m.bx, m.rby = 1.0f / (float) m.by, m.rbz = 1.0f / (float) m.bz;
	}
}

}        // namespace

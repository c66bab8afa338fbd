// max_map_skip.hpp — the sample path of the maximum-intensity projection (k_mip) that the isosurface (k_iso, §5.10) and the slab (k_slab, §5.11) share:
// the filtered intensity of one sample or of a group of samples, the grown-cell test, the exact skip step over the per-cell max map
// (vkv_max_map) as a helper, and the host-side checks and arguments of both entry points.  k_mip keeps its own inline copy of the skip step:
// calling max_map_skip cost its skipping variant 1-2 % (§5.10).  Included after raymarch_core.hpp.
#pragma once

#include <cmath>

// everything here is internal to the translation unit that includes it (no exported symbols)
namespace
{

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

// One probe of the skip step at sample i of n (position pos*).  When sample i enters a map cell other than `last_cell`, the cell's byte B is
// read (++n_probe); when B * kInv255 cannot reach `bound` (STRICT: B * kInv255 < bound; else B * kInv255 <= bound) and the sample lies in the
// grown cell, the result is the last index i + kk (kk >= 0, never past sample n - 1) of the samples i .. i + kk that lie in the grown cell,
// and last_cell is reset.  -1: filter sample i.  MM holds the max map and its geometry: max_map; bx, by, bz (voxels per cell); lcx, lcy, lcz
// (last cell per axis that holds a voxel); rbx, rby, rbz (1 / block: finding the cell only, the skip itself is checked exactly).
template <bool STRICT, typename MM>
__device__ __forceinline__ int max_map_skip(const RayMarchArgs &A, const MM &M, const Ray &R, int i, int n, float posx, float posy, float posz, float bound,
                                            uint32_t &last_cell, uint32_t &n_probe)
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

bool     extent_ok(VkvExtent3D e) { return e.width > 0 && e.height > 0 && e.depth > 0; }
bool     map_extent_ok(VkvExtent3D e, VkvExtent3D me) { return extent_ok(me) && me.width <= e.width && me.height <= e.height && me.depth <= e.depth; }
uint32_t block_of(uint32_t e, uint32_t m) { return (e + m - 1) / m; }

// the checks of the fields of P a MIP / isosurface call reads (`what`: the entry point's name in the messages), with the max map d_max_map
// (or null) and `has_output`: an output of the call's own options is set; VKV_OK or the code (nothing is enqueued before they pass).
// rays = false (vkv_render_slab): the call casts no rays, so it has no depth (options.depth_attachment and d_out_depth are unsupported) and
// reads no sampling_factor
int check_first_hit_params(vkv_ctx *ctx, const char *what, const VkvRenderParams *P, const uint8_t *d_max_map, bool has_output, bool rays = true)
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
	if (!P->d_volume)
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
	const VkvTileSchedule &t = P->tiles;
	if (t.tile_width == 0 || t.tile_height == 0 || (t.tile_width % 16) || (t.tile_height % 16) || t.tile_stride == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: tile size must be a positive multiple of 16 and tile_stride > 0", what);
	const uint64_t tiles_x = (P->image_width + t.tile_width - 1) / t.tile_width, tiles_y = (P->image_height + t.tile_height - 1) / t.tile_height;
	const bool     whole   = t.rect.w == 0 || t.rect.h == 0;
	if (!whole && ((uint64_t) t.rect.x0 + t.rect.w > tiles_x || (uint64_t) t.rect.y0 + t.rect.h > tiles_y))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: the schedule's tile rectangle runs past the image", what);
	const uint64_t scheduled = whole ? tiles_x * tiles_y : (uint64_t) t.rect.w * t.rect.h;
	if (t.tile_count && (uint64_t) t.tile_first + (uint64_t) (t.tile_count - 1) * t.tile_stride >= scheduled)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: tile schedule runs past the %s", what, whole ? "image" : "tile rectangle");
	if (P->d_packed_volume && ((uintptr_t) P->d_packed_volume & 255u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_packed_volume must be 256-byte aligned", what);
	if (!P->d_out_color && !P->d_out_rgba8 && !P->d_out_counts && !P->d_out_depth && !has_output)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: no output buffer", what);
	const uint64_t nb = (uint64_t) (t.tile_width / 16) * (t.tile_height / 16) * t.tile_count;
	if (nb > 0x3fffffffull || (uint64_t) P->image_width * P->image_height > 0xffffffffull / 4 || nb * 256 > 0xffffffffull / 4)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: frame too large for one launch", what);
	return VKV_OK;
}

// VkvRenderParams -> the fields of RayMarchArgs the MIP and isosurface kernels read (the rest stays zero)
void fill_mip_args(const VkvRenderParams *P, RayMarchArgs &a)
{
	a = RayMarchArgs{};
	for (int i = 0; i < 3; ++i)
		a.dir00[i] = P->ray_gen.dir00[i], a.ddx[i] = P->ray_gen.ddx[i], a.ddy[i] = P->ray_gen.ddy[i], a.cam[i] = P->ray_cast.camera_pos_tex[i];
	for (int i = 0; i < 4; ++i)
		a.plane_tex[i] = P->ray_cast.plane_tex[i];
	for (int i = 0; i < 16; ++i)
		a.model[i] = P->camera.model[i], a.view[i] = P->camera.camera_view[i], a.proj[i] = P->camera.camera_proj[i],
		a.view_proj_inv[i] = P->camera.camera_view_proj_inv[i], a.model_inv[i] = P->camera.model_inv[i];
	a.sampling_factor = P->transfer_function.sampling_factor;
	a.W = (int) P->volume_extent.width, a.H = (int) P->volume_extent.height, a.D = (int) P->volume_extent.depth;
	a.mw = (int) P->map_extent.width, a.mh = (int) P->map_extent.height, a.md = (int) P->map_extent.depth;
	a.vol    = P->d_volume;
	a.packed = static_cast<const uint8_t *>(P->d_packed_volume);
	{
		const PackedDims pd = packed_dims(a.W, a.H, a.D);
		a.pmx = pd.mx, a.pmy = pd.my;
	}
	a.out_color = P->d_out_color, a.out_rgba8 = P->d_out_rgba8, a.out_counts = P->d_out_counts, a.out_depth = P->d_out_depth;
	a.in_depth         = P->options.depth_attachment ? P->d_in_depth : nullptr;
	a.depth_attachment = P->options.depth_attachment != 0;
	a.img_w = P->image_width, a.img_h = P->image_height;
	a.tile_w = P->tiles.tile_width, a.tile_h = P->tiles.tile_height;
	a.tile_first = P->tiles.tile_first, a.tile_stride = P->tiles.tile_stride, a.tile_count = P->tiles.tile_count, a.compact = P->tiles.compact;
	const VkvTileRect &r     = P->tiles.rect;
	const bool         whole = r.w == 0 || r.h == 0;
	a.tiles_x                = whole ? (a.img_w + a.tile_w - 1) / a.tile_w : r.w;
	a.org_x = whole ? 0u : r.x0 * a.tile_w, a.org_y = whole ? 0u : r.y0 * a.tile_h;
	a.blocks_per_tile_x = a.tile_w / 16;
	a.blocks_per_tile   = a.blocks_per_tile_x * (a.tile_h / 16);
	a.nblocks           = a.blocks_per_tile * a.tile_count;
	a.test              = VKV_TEST_NONE;
	{        // shape of a wave's pixel patch, as the integrator picks it: voxels per pixel step in x against y
		double vx = 0.0, vy = 0.0;
		const double dim[3] = {(double) a.W, (double) a.H, (double) a.D};
		for (int k = 0; k < 3; ++k)
			vx += (double) a.ddx[k] * dim[k] * (double) a.ddx[k] * dim[k], vy += (double) a.ddy[k] * dim[k] * (double) a.ddy[k] * dim[k];
		const double q = (vx > 0.0 && vy > 0.0) ? std::sqrt(vx / vy) : 1.0;
		a.wave_pw_log2 = q >= 1.6 ? 2u : (q <= 1.0 / 1.6 ? 4u : 3u);        // 4x16, 16x4 or 8x8 pixels
	}
	// a schedule over every tile of its rectangle (the whole image or VkvTileSchedule.rect) starts in the integrator's ring order
	const uint32_t rows = whole ? (a.img_h + a.tile_h - 1) / a.tile_h : r.h;
	a.order_h           = (a.tile_first == 0 && a.tile_stride == 1 && (uint64_t) a.tile_count == (uint64_t) a.tiles_x * rows) ? rows : 0u;
}

// the max-map fields of a kernel's arguments (MipArgs, IsoArgs: what max_map_skip reads); block 1 and cell 0 without a map
template <typename MM>
void fill_max_map_geometry(const VkvRenderParams *P, const uint8_t *d_max_map, MM &m)
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

// mip.hip — maximum-intensity projection: the per-cell max map (vkv_max_map) and the MIP render (vkv_render_mip).  DESIGN.md §5.9 pins the
// definition and says why skipping over the max map gives the dense path's bits.
//
// Max map: one byte per occupancy-map cell, the largest voxel of the cell's voxel box grown by one voxel per side (clipped to the volume): every
// voxel a trilinear sample whose voxel coordinate lies within half a voxel of the cell can read.  One lane per cell, voxel rows read a dword at
// a time at any alignment (load4_clipped: nothing past a row's last byte).
//
// Render: the integrator's rays (ray_setup<VKV_SKIP_NONE>, unchanged), one lane per ray, a workgroup = 16x16 pixels dealt to the XCDs and
// started as the integrator's are, a wave = the 64-pixel patch shape the integrator picks for the view (4x16, 8x8 or 16x4).
// A sample is the integrator's filtered intensity (sample_linear, or sample_packed<false>: four footprint dwords).  The skipping variant reads
// the max-map byte of the cell a ray enters and jumps over the samples of that cell when the byte cannot beat max(threshold, best so far).
#include <algorithm>
#include <cmath>

#include "ray_setup.hpp"
#include "volume_sampling.hpp"
#include "direct_render.hpp"
#include "row_loads.hpp"

namespace
{

__device__ __forceinline__ uint32_t max_byte(uint32_t d) { return max(max(d & 255u, (d >> 8) & 255u), max((d >> 16) & 255u, d >> 24)); }

struct MaxMapArgs
{
	const uint8_t *vol;
	uint8_t *      map;
	int            W, H, D, mw, mh, bx, by, bz;
	int            cx0, cy0, cz0, ncx, ncy, ncz;        // the launch's cells
};

__global__ void __launch_bounds__(256) k_max_map(const MaxMapArgs a)
{
	const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (t >= (uint64_t) a.ncx * (uint64_t) a.ncy * (uint64_t) a.ncz)
		return;
	const int      cx = a.cx0 + (int) (t % (uint64_t) a.ncx);
	const uint64_t r  = t / (uint64_t) a.ncx;
	const int      cy = a.cy0 + (int) (r % (uint64_t) a.ncy), cz = a.cz0 + (int) (r / (uint64_t) a.ncy);
	uint32_t       m  = 0u;
	if (cx * a.bx < a.W && cy * a.by < a.H && cz * a.bz < a.D)        // (cells past the volume hold 0)
	{
		const int x0 = max(cx * a.bx - 1, 0), x1 = min(cx * a.bx + a.bx, a.W - 1);        // inclusive
		const int y0 = max(cy * a.by - 1, 0), y1 = min(cy * a.by + a.by, a.H - 1);
		const int z0 = max(cz * a.bz - 1, 0), z1 = min(cz * a.bz + a.bz, a.D - 1);
		for (int z = z0; z <= z1; ++z)
			for (int y = y0; y <= y1; ++y)
			{
				const uint8_t *row = a.vol + ((size_t) z * (size_t) a.H + (size_t) y) * (size_t) a.W;
				for (int x = x0; x <= x1; x += 4)
				{
					const int      nv = min(4, x1 + 1 - x);
					const uint32_t d  = load4_clipped(row, x, a.W) & (nv == 4 ? ~0u : ((1u << (8 * nv)) - 1u));
					m                 = max(m, max_byte(d));
				}
			}
	}
	a.map[((size_t) cz * (size_t) a.mh + (size_t) cy) * (size_t) a.mw + (size_t) cx] = (uint8_t) m;
}

struct MipArgs
{
	RayMarchArgs   A;               // the fields ray_setup, start_entry and the samplers read (fill_direct_args)
	float          threshold, window_max;
	float *        out_intensity;   // or null
	MaxMapGeometry mm;              // skipping variant only
};

// (the deal, the samplers, in_grown, the depth and the stores are in direct_render.hpp, shared with k_iso and k_slab.  The skip step below is written
// out here rather than calling max_map_skip: the shared helper's control flow cost the skipping variant 1-2 %)

template <bool PACKED, bool SKIP>
__global__ void __launch_bounds__(256) k_mip(const MipArgs M)
{
	const RayMarchArgs &A = M.A;
	const MaxMapGeometry &G = M.mm;
	// a wave's patch: the shape the integrator picks for the view (wave_patch_log2)
	uint32_t px, py, o;
	if (!pixel_deal(A, A.wave_pw_log2, px, py, o))
		return;
	Ray R;
	R.o                = o;
	const bool marched = ray_setup<VKV_SKIP_NONE>(A, px, py, R);
	float      best    = M.threshold;        // max(threshold, largest counted sample)
	int        k       = -1;                 // first index of the largest counted sample
	uint32_t   n_filt = 0, n_probe = 0, n_skip = 0;
	if (!SKIP && marched)
	{
		// dense: kDenseGroup samples per round, their footprint loads all issued before the first filter (memory-level parallelism: a lane has
		// nothing else to hide the gather latency behind); the groups are taken in order, so `k` stays the first index of the maximum
		const int n = R.n_steps;
		int       i = 0;
		for (; i + kDenseGroup <= n; i += kDenseGroup)
		{
			float v[kDenseGroup];
			mip_samples<PACKED, kDenseGroup>(A, R, i, v);
#pragma unroll
			for (int j = 0; j < kDenseGroup; ++j)
				if (v[j] > best)
					best = v[j], k = i + j;
		}
		for (; i < n; ++i)
		{
			const float fi = (float) i;
			const float v  = mip_sample<PACKED>(A, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey), __builtin_fmaf(fi, R.sz, R.ez));
			if (v > best)
				best = v, k = i;
		}
		n_filt = (uint32_t) n;
	}
	if (SKIP && marched)
	{
		// the skip step of max_map_skip<false> (direct_render.hpp), written out: keep the two in step
		const int   n  = R.n_steps;
		const float fW = (float) A.W, fH = (float) A.H, fD = (float) A.D;
		uint32_t    last_cell = ~0u;
		int         i         = 0;
		while (i < n)
		{
			const float fi   = (float) i;
			const float posx = __builtin_fmaf(fi, R.sx, R.ex), posy = __builtin_fmaf(fi, R.sy, R.ey), posz = __builtin_fmaf(fi, R.sz, R.ez);
			if (SKIP)
			{
				// the sampler's own voxel coordinates of this sample (sample_linear / packed_footprint)
				const float cx = __builtin_fmaf(posx, fW, -0.5f), cy = __builtin_fmaf(posy, fH, -0.5f), cz = __builtin_fmaf(posz, fD, -0.5f);
				const int   mx = i_clamp((int) __builtin_floorf((cx + 0.5f) * G.rbx), 0, G.lcx);
				const int   my = i_clamp((int) __builtin_floorf((cy + 0.5f) * G.rby), 0, G.lcy);
				const int   mz = i_clamp((int) __builtin_floorf((cz + 0.5f) * G.rbz), 0, G.lcz);
				const uint32_t cell = ((uint32_t) mz * (uint32_t) A.mh + (uint32_t) my) * (uint32_t) A.mw + (uint32_t) mx;
				if (cell != last_cell)
				{
					++n_probe;
					last_cell = cell;
					const int lx = mx * G.bx, ly = my * G.by, lz = mz * G.bz;
					if ((float) G.max_map[cell] * kInv255 <= best && in_grown(cx, lx, G.bx) && in_grown(cy, ly, G.by) && in_grown(cz, lz, G.bz))
					{
						// samples i .. i + kk: the estimate aims a quarter voxel past the cell's edge (inside the half-voxel margin); the last one is
						// checked exactly below, and the sampler's coordinates are monotone in the sample index, so every sample between lies in the
						// grown cell too
						const float sx = R.sx * fW, sy = R.sy * fH, sz = R.sz * fD;
						const float tx = sx > 0.0f ? ((float) (lx + G.bx) - 0.25f - cx) / sx : (sx < 0.0f ? ((float) lx - 0.75f - cx) / sx : INFINITY);
						const float ty = sy > 0.0f ? ((float) (ly + G.by) - 0.25f - cy) / sy : (sy < 0.0f ? ((float) ly - 0.75f - cy) / sy : INFINITY);
						const float tz = sz > 0.0f ? ((float) (lz + G.bz) - 0.25f - cz) / sz : (sz < 0.0f ? ((float) lz - 0.75f - cz) / sz : INFINITY);
						const float tm = g_min(g_min(tx, ty), g_min(tz, (float) (n - 1 - i)));
						int         kk = tm > 0.0f ? (int) tm : 0;
						if (kk > 0)
						{
							const float fl = (float) (i + kk);
							const float qx = __builtin_fmaf(__builtin_fmaf(fl, R.sx, R.ex), fW, -0.5f);
							const float qy = __builtin_fmaf(__builtin_fmaf(fl, R.sy, R.ey), fH, -0.5f);
							const float qz = __builtin_fmaf(__builtin_fmaf(fl, R.sz, R.ez), fD, -0.5f);
							if (!(in_grown(qx, lx, G.bx) && in_grown(qy, ly, G.by) && in_grown(qz, lz, G.bz)))
								kk = 0;
						}
						i += kk + 1;
						n_skip += (uint32_t) (kk + 1);
						last_cell = ~0u;
						continue;
					}
				}
			}
			const float v = mip_sample<PACKED>(A, posx, posy, posz);
			++n_filt;
			if (v > best)
				best = v, k = i;
			++i;
			if (SKIP && best >= kMaxSample)
			{        // nothing can beat it
				n_skip += (uint32_t) (n - i);
				break;
			}
		}
	}
	const size_t po = o;
	float        g = 0.0f, a = 0.0f, intensity = 0.0f;
	float        depth = A.depth_attachment ? A.in_depth[po] : 0.0f;        // what the integrator gives a pixel without colour
	if (k >= 0)
	{
		intensity = best;
		g         = M.window_max <= M.threshold ? 1.0f : g_clamp((best - M.threshold) / (M.window_max - M.threshold), 0.0f, 1.0f);
		a         = 1.0f;
		if (A.out_depth)
		{        // at sample k
			const float fk = (float) k;
			depth          = first_hit_depth(A, __builtin_fmaf(fk, R.sx, R.ex), __builtin_fmaf(fk, R.sy, R.ey), __builtin_fmaf(fk, R.sz, R.ez));
		}
	}
	if (A.out_color)
		store_float4_nt(A.out_color, po, g, g, g, a);
	if (A.out_rgba8)
		store_rgba8_nt(A.out_rgba8, po, g, g, g, a);
	if (M.out_intensity)
		__builtin_nontemporal_store(intensity, M.out_intensity + po);
	if (A.out_counts)
		store_counts(A.out_counts, po, n_filt, n_probe, n_skip);
	if (A.out_depth)
		__builtin_nontemporal_store(depth, A.out_depth + po);
}

// the checks of vkv_render_mip; VKV_OK or the code (nothing is enqueued before they pass)
int check_mip(vkv_ctx *ctx, const VkvRenderParams *P, const VkvMipOptions *M)
{
	if (!P || !M)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_mip: null params or options");
	if (M->flags != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_mip: flags must be 0");
	if (!std::isfinite(M->threshold) || std::isnan(M->window_max))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_mip: threshold must be finite and window_max not NaN");
	return check_first_hit_params(ctx, "render_mip", P, M->d_max_map, M->d_out_intensity != nullptr);
}

template <bool PACKED>
void launch_mip(const MipArgs &m, hipStream_t s)
{
	if (m.mm.max_map)
		hipLaunchKernelGGL((k_mip<PACKED, true>), dim3(deal_grid(m.A)), dim3(256), 0, s, m);
	else
		hipLaunchKernelGGL((k_mip<PACKED, false>), dim3(deal_grid(m.A)), dim3(256), 0, s, m);
}

}        // namespace

extern "C" {

int vkv_max_map(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, VkvExtent3D map_extent, const VkvBox *box, uint8_t *d_max_map, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_max_map || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "max_map: null pointer or bad extent");
	if (const int rc = check_box(ctx, "max_map", extent, box))
		return rc;
	MaxMapArgs a;
	a.vol = d_volume, a.map = d_max_map;
	a.W = (int) extent.width, a.H = (int) extent.height, a.D = (int) extent.depth, a.mw = (int) map_extent.width, a.mh = (int) map_extent.height;
	a.bx = (int) block_of(extent.width, map_extent.width), a.by = (int) block_of(extent.height, map_extent.height), a.bz = (int) block_of(extent.depth, map_extent.depth);
	if (box)
	{
		const VkvBox b = *box;
		// the cells whose grown voxel box [c b - 1, c b + b] meets [x0, x0 + width - 1]: ceil(x0 / b) - 1 <= c <= (x0 + width) / b, clamped to the map
		const uint32_t lo[3] = {b.x0, b.y0, b.z0}, n[3] = {b.width, b.height, b.depth}, bs[3] = {(uint32_t) a.bx, (uint32_t) a.by, (uint32_t) a.bz};
		const uint32_t me[3] = {map_extent.width, map_extent.height, map_extent.depth};
		int            c0[3], nc[3];
		for (int k = 0; k < 3; ++k)
		{
			const uint32_t up = (uint32_t) (((uint64_t) lo[k] + bs[k] - 1) / bs[k]);        // ceil(x0 / b)
			const uint32_t first = up > 0 ? up - 1 : 0u, last = std::min((uint32_t) (((uint64_t) lo[k] + n[k]) / bs[k]), me[k] - 1);
			c0[k] = (int) first, nc[k] = (int) (last - first + 1);
		}
		a.cx0 = c0[0], a.cy0 = c0[1], a.cz0 = c0[2], a.ncx = nc[0], a.ncy = nc[1], a.ncz = nc[2];
	}
	else
		a.cx0 = a.cy0 = a.cz0 = 0, a.ncx = (int) map_extent.width, a.ncy = (int) map_extent.height, a.ncz = (int) map_extent.depth;
	const uint64_t cells  = (uint64_t) a.ncx * a.ncy * a.ncz;
	const uint64_t groups = (cells + 255) / 256;
	if (groups > 0x7fffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "max_map: map too large for one launch");
	hipLaunchKernelGGL(k_max_map, dim3((uint32_t) groups), dim3(256), 0, (hipStream_t) stream, a);
	return check_launch(ctx, "max_map");
}

int vkv_render_mip(vkv_ctx *ctx, const VkvRenderParams *P, const VkvMipOptions *M, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int rc = check_mip(ctx, P, M);
	if (rc != VKV_OK)
		return rc;
	MipArgs m;
	fill_direct_args(P, m.A);
	if (m.A.nblocks == 0)
		return VKV_OK;
	m.threshold = M->threshold, m.window_max = M->window_max, m.out_intensity = M->d_out_intensity;
	fill_max_map_geometry(P, M->d_max_map, m.mm);
	if (m.A.packed)
		launch_mip<true>(m, (hipStream_t) stream);
	else
		launch_mip<false>(m, (hipStream_t) stream);
	return check_launch(ctx, "render_mip");
}

}        // extern "C"

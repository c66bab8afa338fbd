// slab.hip — oblique slices and thick slabs (vkv_render_slab): the plain filtered value on a plane through the volume, or the max, min or mean
// of a column of samples along the plane's normal (multi-planar reformatting).  DESIGN.md §5.11 pins every output to the bit and says why
// skipping over the max map (MAX only) gives the dense path's bits.
//
// No camera: pixel (x, y) has the base point p = fma(y, dv, fma(x, du, origin)) in texture space and the samples q_j = fma(j, dn, p),
// j = 0 .. samples - 1; a sample counts when q_j lies in [0, 1]^3.  fma is monotone in j, so per axis the counted indices are one range,
// found by bisection over the very test that defines it.  One lane per pixel, a workgroup = 16x16 pixels dealt to the XCDs and started as
// k_mip's are (mip.hip), a wave = an 8x8 pixel patch whatever the plane: the footprints of a thin slice then fall in neighbouring voxel rows
// and bricks.  A sample is the integrator's filtered intensity (mip_sample / mip_samples of direct_render.hpp); the skipping variant walks the
// column like a MIP ray with entry p and step dn (max_map_skip, bound = the best so far).
#include <cmath>

#include "raymarch_args.hpp"
#include "volume_sampling.hpp"
#include "direct_render.hpp"

namespace
{

struct SlabArgs
{
	RayMarchArgs   A;               // the fields start_entry and the samplers read (fill_direct_args); no ray is set up
	float          origin[3], du[3], dv[3], dn[3];
	int            samples;         // 1 .. 4096
	float          window_min, window_max;
	float *        out_value;       // or null
	MaxMapGeometry mm;              // skipping variant only
};

// the first j in [0, n] for which pred(fma(j, d, p)) holds (n: none); pred must turn from false to true once as j rises
template <typename Pred>
__device__ __forceinline__ int first_sample(float p, float d, int n, Pred pred)
{
	int a = 0, b = n;
	while (a < b)
	{
		const int m = (a + b) >> 1;
		if (pred(__builtin_fmaf((float) m, d, p)))
			b = m;
		else
			a = m + 1;
	}
	return a;
}

// the indices j in [lo, hi) of [0, n) with 0 <= fma(j, d, p) <= 1: q is monotone in j (rising for d >= 0, falling for d < 0; a correctly
// rounded fma keeps the order of the exact values), so each bound is one bisection over the defining comparison itself
__device__ __forceinline__ void counted_range(float p, float d, int n, int &lo, int &hi)
{
	int l, h;
	if (d >= 0.0f)
		l = first_sample(p, d, n, [](float q) { return q >= 0.0f; }), h = first_sample(p, d, n, [](float q) { return q > 1.0f; });
	else
		l = first_sample(p, d, n, [](float q) { return q <= 1.0f; }), h = first_sample(p, d, n, [](float q) { return q < 0.0f; });
	lo = max(lo, l), hi = min(hi, h);
}

template <bool PACKED, int MODE, bool SKIP>
__global__ void __launch_bounds__(256) k_slab(const SlabArgs S)
{
	static_assert(!SKIP || MODE == VKV_SLAB_MAX, "the max map bounds a maximum only");
	const RayMarchArgs &A = S.A;
	// a wave's patch: 8x8 pixels whatever the plane
	uint32_t px, py, o;
	if (!pixel_deal(A, 3u, px, py, o))
		return;
	const size_t po = o;
	// the column of this pixel as a ray: entry p, step dn
	Ray         R;
	const float fx = (float) px, fy = (float) py;
	R.ex = __builtin_fmaf(fy, S.dv[0], __builtin_fmaf(fx, S.du[0], S.origin[0]));
	R.ey = __builtin_fmaf(fy, S.dv[1], __builtin_fmaf(fx, S.du[1], S.origin[1]));
	R.ez = __builtin_fmaf(fy, S.dv[2], __builtin_fmaf(fx, S.du[2], S.origin[2]));
	R.sx = S.dn[0], R.sy = S.dn[1], R.sz = S.dn[2];
	int lo = 0, hi = S.samples;        // the counted samples: [lo, hi)
	counted_range(R.ex, R.sx, S.samples, lo, hi);
	counted_range(R.ey, R.sy, S.samples, lo, hi);
	counted_range(R.ez, R.sz, S.samples, lo, hi);
	float    best = MODE == VKV_SLAB_MIN ? INFINITY : -INFINITY;        // MAX / MIN: the extreme so far
	float    acc  = 0.0f;                                               // MEAN: the sum in rising order
	uint32_t n_filt = 0, n_probe = 0, n_skip = 0;
	auto     take = [&](float v) {
		if (MODE == VKV_SLAB_MAX)
			best = v > best ? v : best;
		else if (MODE == VKV_SLAB_MIN)
			best = v < best ? v : best;
		else
			acc = acc + v;
	};
	if (!SKIP && lo < hi)
	{
		// dense: kDenseGroup samples per round, their footprint loads all issued before the first filter; the groups are taken in order
		int i = lo;
		for (; i + kDenseGroup <= hi; i += kDenseGroup)
		{
			float v[kDenseGroup];
			mip_samples<PACKED, kDenseGroup>(A, R, i, v);
#pragma unroll
			for (int j = 0; j < kDenseGroup; ++j)
				take(v[j]);
		}
		for (; i < hi; ++i)
		{
			const float fi = (float) i;
			take(mip_sample<PACKED>(A, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey), __builtin_fmaf(fi, R.sz, R.ez)));
		}
		n_filt = (uint32_t) (hi - lo);
	}
	if (SKIP && lo < hi)
	{
		// a MIP ray over samples lo .. hi - 1 without a threshold: no byte is <= -inf, so the first counted sample is always filtered
		uint32_t last_cell = ~0u;
		int      i         = lo;
		while (i < hi)
		{
			const float fi   = (float) i;
			const float posx = __builtin_fmaf(fi, R.sx, R.ex), posy = __builtin_fmaf(fi, R.sy, R.ey), posz = __builtin_fmaf(fi, R.sz, R.ez);
			const int   last = max_map_skip<false>(A, S.mm, R, i, hi, posx, posy, posz, best, last_cell, n_probe);
			if (last >= 0)
			{
				n_skip += (uint32_t) (last + 1 - i);
				i = last + 1;
				continue;
			}
			take(mip_sample<PACKED>(A, posx, posy, posz));
			++n_filt;
			++i;
			if (best >= kMaxSample)
			{        // nothing can beat it
				n_skip += (uint32_t) (hi - i);
				break;
			}
		}
	}
	float g = 0.0f, a = 0.0f, value = 0.0f;
	if (lo < hi)
	{
		value = MODE == VKV_SLAB_MEAN ? acc / (float) (hi - lo) : best;
		g     = S.window_max <= S.window_min ? 1.0f : g_clamp((value - S.window_min) / (S.window_max - S.window_min), 0.0f, 1.0f);
		a     = 1.0f;
	}
	if (A.out_color)
		store_float4_nt(A.out_color, po, g, g, g, a);
	if (A.out_rgba8)
		store_rgba8_nt(A.out_rgba8, po, g, g, g, a);
	if (S.out_value)
		__builtin_nontemporal_store(value, S.out_value + po);
	if (A.out_counts)
		store_counts(A.out_counts, po, n_filt, n_probe, n_skip);
}

// the checks of vkv_render_slab; VKV_OK or the code (nothing is enqueued before they pass)
int check_slab(vkv_ctx *ctx, const VkvRenderParams *P, const VkvSlabOptions *S)
{
	if (!P || !S)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: null params or options");
	if (S->flags != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: flags must be 0");
	if (S->samples < 1 || S->samples > 4096)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: samples must be 1 .. 4096");
	if (S->mode != VKV_SLAB_MAX && S->mode != VKV_SLAB_MIN && S->mode != VKV_SLAB_MEAN)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: unknown mode");
	for (int c = 0; c < 3; ++c)
		if (!std::isfinite(S->origin[c]) || !std::isfinite(S->du[c]) || !std::isfinite(S->dv[c]) || !std::isfinite(S->dn[c]))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: origin, du, dv and dn must be finite");
	if (std::isnan(S->window_min) || std::isnan(S->window_max))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: window_min and window_max must not be NaN");
	if (S->d_max_map && S->mode != VKV_SLAB_MAX)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_slab: a max map bounds VKV_SLAB_MAX only");
	return check_first_hit_params(ctx, "render_slab", P, S->d_max_map, S->d_out_value != nullptr, false);
}

template <bool PACKED>
void launch_slab(const SlabArgs &a, int mode, bool skip, dim3 grid, hipStream_t s)
{
	const dim3 block(256);
	if (mode == VKV_SLAB_MAX && skip)
		hipLaunchKernelGGL((k_slab<PACKED, VKV_SLAB_MAX, true>), grid, block, 0, s, a);
	else if (mode == VKV_SLAB_MAX)
		hipLaunchKernelGGL((k_slab<PACKED, VKV_SLAB_MAX, false>), grid, block, 0, s, a);
	else if (mode == VKV_SLAB_MIN)
		hipLaunchKernelGGL((k_slab<PACKED, VKV_SLAB_MIN, false>), grid, block, 0, s, a);
	else
		hipLaunchKernelGGL((k_slab<PACKED, VKV_SLAB_MEAN, false>), grid, block, 0, s, a);
}

}        // namespace

extern "C" {

int vkv_render_slab(vkv_ctx *ctx, const VkvRenderParams *P, const VkvSlabOptions *S, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int rc = check_slab(ctx, P, S);
	if (rc != VKV_OK)
		return rc;
	SlabArgs a;
	fill_direct_args(P, a.A);
	if (a.A.nblocks == 0)
		return VKV_OK;
	a.A.out_depth = nullptr, a.A.in_depth = nullptr, a.A.depth_attachment = 0;        // (rejected when set)
	for (int c = 0; c < 3; ++c)
		a.origin[c] = S->origin[c], a.du[c] = S->du[c], a.dv[c] = S->dv[c], a.dn[c] = S->dn[c];
	a.samples = (int) S->samples, a.window_min = S->window_min, a.window_max = S->window_max, a.out_value = S->d_out_value;
	fill_max_map_geometry(P, S->d_max_map, a.mm);
	const dim3 grid(deal_grid(a.A));
	if (a.A.packed)
		launch_slab<true>(a, S->mode, S->d_max_map != nullptr, grid, (hipStream_t) stream);
	else
		launch_slab<false>(a, S->mode, S->d_max_map != nullptr, grid, (hipStream_t) stream);
	return check_launch(ctx, "render_slab");
}

}        // extern "C"

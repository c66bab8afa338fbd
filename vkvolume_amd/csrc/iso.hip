// iso.hip — shaded isosurface (vkv_render_isosurface): the first sample of a ray whose filtered intensity reaches `iso`, refined by bisection
// between it and the sample before, lit by a headlight.  DESIGN.md §5.10 pins every output to the bit and says why skipping over the max map
// gives the dense path's bits.
//
// Rays, workgroup deal, wave patch shape and samplers are k_mip's (mip.hip): ray_setup<VKV_SKIP_NONE>, one lane per ray, a workgroup = 16x16
// pixels dealt to the XCDs in the integrator's ring order, a wave = the integrator's 64-pixel patch shape, a sample = mip_sample / mip_samples.
// The dense variant filters kDenseGroup samples per round (their loads first) and stops after the round that holds the first hit; the skipping
// variant probes the max map once per cell entered (max_map_skip, strict: a cell is skipped when B * kInv255 < iso).  A hit lane then spends
// refine_steps filters on the bisection and four on the tetrahedron gradient (the integrator's GRAD == 2 taps, frag:92-97).
#include <cmath>

#include "ray_setup.hpp"
#include "volume_sampling.hpp"
#include "direct_render.hpp"

namespace
{

struct IsoArgs
{
	RayMarchArgs   A;               // the fields ray_setup, start_entry and the samplers read (fill_direct_args)
	float          iso;
	int            refine_steps;    // 0 .. 16
	float          base[3], ambient, diffuse, specular;
	uint32_t       shininess;       // 1 .. 1024
	float *        out_normal;      // or null
	MaxMapGeometry mm;              // skipping variant only
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
	return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

template <bool PACKED, bool SKIP>
__global__ void __launch_bounds__(256) k_iso(const IsoArgs I)
{
	const RayMarchArgs &A = I.A;
	// pixel_deal (direct_render.hpp), written out: keep the two in step.  Calling it cost the skipping variant 0.4-0.95 % on C4
	// (profiles/r9_direct_renderer_refactor.txt), the precedent being k_mip's skip step
	const uint32_t x = blockIdx.x & 7u, idx = blockIdx.x >> 3;
	const uint32_t rank = (idx / A.blocks_per_tile) * 8u + x, sb = idx % A.blocks_per_tile;
	if (rank >= A.tile_count)
		return;
	const uint32_t k_tile = A.order_h ? start_entry(A, rank) : rank;
	if (k_tile >= A.tile_count)
		return;
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63u, pw = A.wave_pw_log2;
	const uint32_t bx = (w & ((16u >> pw) - 1u)) << pw, by = (w >> (4u - pw)) * (64u >> pw);
	const uint32_t t  = A.tile_first + k_tile * A.tile_stride;
	const uint32_t lx = (sb % A.blocks_per_tile_x) * 16u + bx + (lane & ((1u << pw) - 1u)), ly = (sb / A.blocks_per_tile_x) * 16u + by + (lane >> pw);
	const uint32_t px = A.org_x + (t % A.tiles_x) * A.tile_w + lx, py = A.org_y + (t / A.tiles_x) * A.tile_h + ly;
	const uint32_t o  = A.compact ? (k_tile * A.tile_h + ly) * A.tile_w + lx : py * A.img_w + px;
	if (px >= A.img_w || py >= A.img_h)
		return;
	Ray R;
	R.o                = o;
	const bool  marched = ray_setup<VKV_SKIP_NONE>(A, px, py, R);
	const float iso     = I.iso;
	int         k       = -1;        // the first index with v_k >= iso
	uint32_t    n_filt = 0, n_probe = 0, n_skip = 0;
	if (!SKIP && marched)
	{
		// dense: kDenseGroup samples per round, their footprint loads issued before the first filter; the round that holds the first hit ends
		// the march (its samples past the hit are not counted)
		const int n = R.n_steps;
		int       i = 0;
		for (; i + kDenseGroup <= n; i += kDenseGroup)
		{
			float v[kDenseGroup];
			mip_samples<PACKED, kDenseGroup>(A, R, i, v);
			int hit = -1;
#pragma unroll
			for (int j = kDenseGroup - 1; j >= 0; --j)
				if (v[j] >= iso)
					hit = j;
			if (hit >= 0)
			{
				k = i + hit;
				break;
			}
		}
		if (k < 0)
			for (; i < n; ++i)
			{
				const float fi = (float) i;
				if (mip_sample<PACKED>(A, __builtin_fmaf(fi, R.sx, R.ex), __builtin_fmaf(fi, R.sy, R.ey), __builtin_fmaf(fi, R.sz, R.ez)) >= iso)
				{
					k = i;
					break;
				}
			}
		n_filt = k >= 0 ? (uint32_t) (k + 1) : (uint32_t) n;
	}
	if (SKIP && marched)
	{
		const int n         = R.n_steps;
		uint32_t  last_cell = ~0u;
		int       i         = 0;
		while (i < n)
		{
			const float fi   = (float) i;
			const float posx = __builtin_fmaf(fi, R.sx, R.ex), posy = __builtin_fmaf(fi, R.sy, R.ey), posz = __builtin_fmaf(fi, R.sz, R.ez);
			// a cell whose byte cannot reach iso: jump over its samples
			const int last = max_map_skip<true>(A, I.mm, R, i, n, posx, posy, posz, iso, last_cell, n_probe);
			if (last >= 0)
			{
				n_skip += (uint32_t) (last + 1 - i);
				i = last + 1;
				continue;
			}
			++n_filt;
			if (mip_sample<PACKED>(A, posx, posy, posz) >= iso)
			{
				k = i;
				break;
			}
			++i;
		}
	}
	const size_t po = o;
	float        cr = 0.0f, cg = 0.0f, cb = 0.0f, ca = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, nw = 0.0f;
	float        depth = A.depth_attachment ? A.in_depth[po] : 0.0f;        // what the integrator gives a pixel without colour
	if (k >= 0)
	{
		// refinement: bisection between samples k - 1 and k (t = 0 for a hit at the first sample)
		float th = 0.0f;
		if (k > 0)
		{
			float lo = (float) (k - 1);
			th       = (float) k;
			for (int j = 0; j < I.refine_steps; ++j)
			{
				const float mid = (lo + th) * 0.5f;
				if (mip_sample<PACKED>(A, __builtin_fmaf(mid, R.sx, R.ex), __builtin_fmaf(mid, R.sy, R.ey), __builtin_fmaf(mid, R.sz, R.ez)) >= iso)
					th = mid;
				else
					lo = mid;
			}
		}
		const float hx = __builtin_fmaf(th, R.sx, R.ex), hy = __builtin_fmaf(th, R.sy, R.ey), hz = __builtin_fmaf(th, R.sz, R.ez);
		if (A.out_depth)
			depth = first_hit_depth(A, hx, hy, hz);
		// gradient: the integrator's tetrahedron taps (raymarch_persistent.hpp, ray_event, GRAD == 2), in texture space
		const float dix = 1.0f / (float) A.W, diy = 1.0f / (float) A.H, diz = 1.0f / (float) A.D;
		const float t1  = mip_sample<PACKED>(A, hx + dix, hy - diy, hz - diz);
		const float t2  = mip_sample<PACKED>(A, hx - dix, hy - diy, hz + diz);
		const float t3  = mip_sample<PACKED>(A, hx - dix, hy + diy, hz - diz);
		const float t4  = mip_sample<PACKED>(A, hx + dix, hy + diy, hz + diz);
		const float gx  = (((t1 - t2) - t3) + t4) * 0.25f;
		const float gy  = (((-t1 - t2) + t3) + t4) * 0.25f;
		const float gz  = (((-t1 + t2) - t3) + t4) * 0.25f;
		const float gtx = gx * (float) A.W, gty = gy * (float) A.H, gtz = gz * (float) A.D;
		// world-space normal: transpose(model_inv[3x3]) * g_tex; row i of the transpose is column i of model_inv (column-major: mi[4i .. 4i + 2])
		const float *mi = A.model_inv;
		const float  wx = dot3(mi[0], mi[1], mi[2], gtx, gty, gtz), wy = dot3(mi[4], mi[5], mi[6], gtx, gty, gtz), wz = dot3(mi[8], mi[9], mi[10], gtx, gty, gtz);
		// view vector: -(model[3x3] * step), normalised
		const float *m  = A.model;
		float        vx = -dot3(m[0], m[4], m[8], R.sx, R.sy, R.sz), vy = -dot3(m[1], m[5], m[9], R.sx, R.sy, R.sz), vz = -dot3(m[2], m[6], m[10], R.sx, R.sy, R.sz);
		const float  vl = __builtin_sqrtf(dot3(vx, vy, vz, vx, vy, vz));
		vx = vx / vl, vy = vy / vl, vz = vz / vl;
		const float l2 = dot3(wx, wy, wz, wx, wy, wz);
		if (l2 == 0.0f || !__builtin_isfinite(l2))
			nx = vx, ny = vy, nz = vz;
		else
		{
			const float nl = __builtin_sqrtf(l2);
			nx = wx / nl, ny = wy / nl, nz = wz / nl;
			if (dot3(nx, ny, nz, vx, vy, vz) < 0.0f)
				nx = -nx, ny = -ny, nz = -nz;        // two-sided: the normal faces the camera
		}
		nw = 1.0f;
		// headlight: the half vector is v; spec = d^shininess by binary exponentiation, highest bit first (leading zero bits keep r = 1)
		const float d = g_clamp(dot3(nx, ny, nz, vx, vy, vz), 0.0f, 1.0f);
		float       r = 1.0f;
		for (int bit = 10; bit >= 0; --bit)
		{
			r = r * r;
			if ((I.shininess >> bit) & 1u)
				r = r * d;
		}
		const float L = (I.ambient + I.diffuse * d) + I.specular * r;
		cr = g_clamp(I.base[0] * L, 0.0f, 1.0f), cg = g_clamp(I.base[1] * L, 0.0f, 1.0f), cb = g_clamp(I.base[2] * L, 0.0f, 1.0f), ca = 1.0f;
	}
	if (A.out_color)
		store_float4_nt(A.out_color, po, cr, cg, cb, ca);
	if (A.out_rgba8)
		store_rgba8_nt(A.out_rgba8, po, cr, cg, cb, ca);
	if (I.out_normal)
		store_float4_nt(I.out_normal, po, nx, ny, nz, nw);
	if (A.out_counts)
		store_counts(A.out_counts, po, n_filt, n_probe, n_skip);
	if (A.out_depth)
		__builtin_nontemporal_store(depth, A.out_depth + po);
}

bool finite_nonneg(float x) { return std::isfinite(x) && x >= 0.0f; }

// the checks of vkv_render_isosurface; VKV_OK or the code (nothing is enqueued before they pass)
int check_iso(vkv_ctx *ctx, const VkvRenderParams *P, const VkvIsoOptions *I)
{
	if (!P || !I)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_isosurface: null params or options");
	if (I->flags != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_isosurface: flags must be 0");
	if (!std::isfinite(I->iso))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_isosurface: iso must be finite");
	if (I->refine_steps > 16)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_isosurface: refine_steps must be 0 .. 16");
	if (!finite_nonneg(I->base_color[0]) || !finite_nonneg(I->base_color[1]) || !finite_nonneg(I->base_color[2]) || !finite_nonneg(I->ambient) ||
	    !finite_nonneg(I->diffuse) || !finite_nonneg(I->specular))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_isosurface: base_color, ambient, diffuse and specular must be finite and >= 0");
	if (I->shininess < 1 || I->shininess > 1024)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_isosurface: shininess must be 1 .. 1024");
	return check_first_hit_params(ctx, "render_isosurface", P, I->d_max_map, I->d_out_normal != nullptr);
}

template <bool PACKED>
void launch_iso(const IsoArgs &a, hipStream_t s)
{
	if (a.mm.max_map)
		hipLaunchKernelGGL((k_iso<PACKED, true>), dim3(deal_grid(a.A)), dim3(256), 0, s, a);
	else
		hipLaunchKernelGGL((k_iso<PACKED, false>), dim3(deal_grid(a.A)), dim3(256), 0, s, a);
}

}        // namespace

extern "C" {

int vkv_render_isosurface(vkv_ctx *ctx, const VkvRenderParams *P, const VkvIsoOptions *I, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int rc = check_iso(ctx, P, I);
	if (rc != VKV_OK)
		return rc;
	IsoArgs a;
	fill_direct_args(P, a.A);
	if (a.A.nblocks == 0)
		return VKV_OK;
	a.iso = I->iso, a.refine_steps = (int) I->refine_steps, a.shininess = I->shininess, a.out_normal = I->d_out_normal;
	a.base[0] = I->base_color[0], a.base[1] = I->base_color[1], a.base[2] = I->base_color[2];
	a.ambient = I->ambient, a.diffuse = I->diffuse, a.specular = I->specular;
	fill_max_map_geometry(P, I->d_max_map, a.mm);
	if (a.A.packed)
		launch_iso<true>(a, (hipStream_t) stream);
	else
		launch_iso<false>(a, (hipStream_t) stream);
	return check_launch(ctx, "render_isosurface");
}

}        // extern "C"

// ray_setup.hpp — a ray from its pixel to its first loop position and from its last one to the frame: the per-ray set-up of the frag
// (ray_setup_impl / ray_setup / ray_clear), the finish with its stores (ray_finish), and the computed start order of a schedule's tiles
// (start_entry).  Every kernel of the integrator shares them (raymarch_core.hpp, raymarch_persistent.hpp), and so do the direct renderers
// (direct_render.hpp, mip.hip, iso.hip: the integrator's rays, unchanged).
#pragma once

#include "raymarch_args.hpp"
#include "volume_sampling.hpp"

// ---------------------------------------------------------------------------------------------------------------
// Correctly rounded fp32 division out of v_rcp_f32 - the sequence the compiler itself emits for `a / b` under
// -fhip-fp32-correctly-rounded-divide-sqrt, without its range scaling (v_div_scale / v_div_fmas) and special-case fix-up
// (v_div_fixup), which do nothing for "ordinary" operands (both magnitudes in [2^-40, 2^40]; a ZERO numerator is not ordinary - the
// refinement would lose the sign of -0 / d - and takes the IEEE path like everything else outside the range: div_ordinary_num):
//     r0 = rcp(d); e = fma(-d, r0, 1); r = fma(e, r0, r0)                          <- depends on the denominator only
//     q0 = a * r; q1 = fma(fma(-d, q0, a), r, q0); q = fma(fma(-d, q1, a), r, q1)
// The ray set-up divides three numerators by the same length (twice), by the same step count, takes three reciprocals of a
// direction ...: 22 divisions per covered ray, 13 % of a C3 frame.  Sharing r between the quotients of one denominator and dropping
// the scale / fix-up instructions leaves 149 of their 242 instructions, with the same bits: checked on the device against the IEEE
// division for every float as denominator (vkv_debug_check what = 2: reciprocals; what = 3: quotients with hashed numerators; what = 4:
// the dispatch itself with numerators +0 and -0).
// Operands outside the ordinary range (axis-parallel rays: 1 / 0; NaNs of a degenerate camera) send the whole wave through the
// plain IEEE set-up (ray_setup below), so the fast path never has to be right about them.
//
// The range test (round 10).  Both paths give the same bits wherever the fast one is valid, so the predicate that chooses between them only
// has to be SUFFICIENT: true only where every operand of every division is ordinary.  It is not kept per operand (28 times two compares and
// the scalar mask operations that fold them into a flag) but as one accumulated range per lane, OrdRange (vkv_device.hpp): the smallest and
// the largest magnitude of the operands as integers, two compares behind the last one, the ballot as before.  Its bounds are 2^-39 and 2^39,
// one binade inside div_ordinary's, and that slack is what lets operands be left out:
//   * the two lengths len = sqrt(fma(z, z, fma(y, y, x * x))).  With 2^-39 <= |x|, |y|, |z| <= 2^39 nothing under- or overflows, every term
//     is >= 0 and rounding is monotone, so x^2 (1 - 2^-24) <= fl(x * x) <= the sum <= 3 * 2^78 (1 + 2^-24)^3 and
//     2^-39 (1 - 2^-24) <= len <= 1.74 * 2^39: inside [2^-40, 2^40].
//   * the upper bound of a component of a normalised vector, q = a / len with len as above: |a| <= len (1 + 2^-23), so |q| < 2 and q is
//     neither inf nor NaN; only its lower bound can fail (ord_low).
//   * the three block sizes: the same for every ray of a launch, tested once on the host (RayMarchArgs.ord_lo0, fill_render_args).
// Everything else goes in: the numerators dx..dz, Bp and Ap, vx..vz, the step numerators (their denominator is a step count, 1 .. 2^24),
// the numerators and the quotients of the divisions by the block size.  The host program of tests/test_ray_setup_range_cpu.py checks
// "new implies old" for one operand over all 2^32 floats, for tuples with every special value in every position, and the two arguments above.
//
// Divisions by a block size that is a power of two (the application's and the benchmark's is 4): n / block is n * (1 / block) exactly, one
// multiplication instead of the eight instructions of recip_refined + div_by; RayMarchArgs.block_rcp holds the reciprocal per axis (0 for an
// axis that has none) and block_pow2 says that all three axes have one: one wave-uniform branch, three multiplications behind it, the
// divisions on its other side.  The IEEE path keeps `a / b`.
// ---------------------------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------------------------
// Ray generation + frag:147-210.  Returns true when the ray has to be marched; false when the pixel is finished
// already (not covered, grazing-ray early-out, or a RayEntry / RayExit test output) with its result in R.
// FAST: divisions through div_by / recip_exact; `ord` comes back as the range of their operands' magnitudes (when it is not ord_ok the caller
// repeats the set-up with FAST = false for the whole wave).
// ---------------------------------------------------------------------------------------------------------------
template <int SKIP, bool FAST>
__device__ __forceinline__ bool ray_setup_impl(const RayMarchArgs &A, uint32_t px, uint32_t py, Ray &R, OrdRange &ord)
{
	R.r = R.g = R.b = R.a = 0.0f;        // out_color = vec4(0) (frag:120)
	R.depth = 0.0f;                      // gl_FragDepth = 0 (frag:140)
	R.n_vol = R.n_dist = R.n_empty = 0;
	R.n_steps = 0, R.i = 0, R.i_min = 0, R.first_hit = 0, R.ul = 0;
	R.fragment = false;
	const int W = A.W, H = A.H, D = A.D;

	// ---- ray generation (replaces volume_render_clipped.vert + volume_render_plane_intersection.vert) ----------
	const float fx = (float) px + 0.5f, fy = (float) py + 0.5f;
	float       dx = __builtin_fmaf(fy, A.ddy[0], __builtin_fmaf(fx, A.ddx[0], A.dir00[0]));
	float       dy = __builtin_fmaf(fy, A.ddy[1], __builtin_fmaf(fx, A.ddx[1], A.dir00[1]));
	float       dz = __builtin_fmaf(fy, A.ddy[2], __builtin_fmaf(fx, A.ddx[2], A.dir00[2]));
	{
		const float len = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
		if (FAST)
		{
			ord_both(ord, dx, dy, dz);        // (len follows from them)
			const float r = recip_refined(len);
			dx = div_by(dx, len, r), dy = div_by(dy, len, r), dz = div_by(dz, len, r);
		}
		else
			dx /= len, dy /= len, dz /= len;
	}
	const float ox = A.cam[0], oy = A.cam[1], oz = A.cam[2];
	float       t_near = -INFINITY, t_far = INFINITY;
	bool        miss   = false;
	{
		const float dv[3] = {dx, dy, dz}, ov[3] = {ox, oy, oz};
#pragma unroll
		for (int a = 0; a < 3; ++a)
		{
			if (dv[a] == 0.0f)
			{
				if (ov[a] < 0.0f || ov[a] > 1.0f)
					miss = true;
			}
			else
			{
				float inv;
				if (FAST)
				{
					ord_low(ord, dv[a]);
					inv = recip_exact(dv[a]);
				}
				else
					inv = 1.0f / dv[a];
				const float ta = (0.0f - ov[a]) * inv, tb = (1.0f - ov[a]) * inv;
				t_near = g_max(t_near, g_min(ta, tb));
				t_far  = g_min(t_far, g_max(ta, tb));
			}
		}
	}
	if (miss)
		return false;
	const float Ap = __builtin_fmaf(A.plane_tex[2], oz, __builtin_fmaf(A.plane_tex[1], oy, A.plane_tex[0] * ox)) + A.plane_tex[3];
	const float Bp = __builtin_fmaf(A.plane_tex[2], dz, __builtin_fmaf(A.plane_tex[1], dy, A.plane_tex[0] * dx));
	if (!(Bp > 0.0f))
		return false;
	float t_plane;
	if (FAST)
	{
		ord_both(ord, Bp), ord_both(ord, Ap);        // (|0 - Ap| = |Ap|)
		t_plane = div_by(0.0f - Ap, Bp, recip_refined(Bp));
	}
	else
		t_plane = (0.0f - Ap) / Bp;
	const float t0      = g_max(t_near, t_plane);
	if (!(t0 < t_far))
		return false;
	const float ex = __builtin_fmaf(t0, dx, ox), ey = __builtin_fmaf(t0, dy, oy), ez = __builtin_fmaf(t0, dz, oz);        // ray_entry
	R.fragment = true;

	// ---- DEPTH_ATTACHMENT, frag:122-136: manual z-test of the front face against the scene depth (reverse-Z) ----
	float frag_depth = 0.0f, frag_depth_front = 0.0f, position[4] = {0, 0, 0, 0};
	if (A.depth_attachment)
	{
		const float pm[4] = {ex - 0.5f, ey - 0.5f, ez - 0.5f, 1.0f};        // position = proj * view * model * (ray_entry - 0.5) (clipped.vert:62)
		float       a4[4], b4[4];
		mat4_mul_vec4(A.model, pm, a4);
		mat4_mul_vec4(A.view, a4, b4);
		mat4_mul_vec4(A.proj, b4, position);
		frag_depth       = A.in_depth[R.o];
		frag_depth_front = position[2] / position[3];
		if (frag_depth > frag_depth_front)
		{        // discard
			R.fragment = false;
			return false;
		}
		R.depth = frag_depth;        // gl_FragDepth = frag_depth (frag:135)
	}

	// ---- frag:147-149 --------------------------------------------------------------------------------------
	float rdx, rdy, rdz;
	{
		const float vx = ex - ox, vy = ey - oy, vz = ez - oz;
		const float len = __builtin_sqrtf(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
		if (FAST)
		{
			ord_both(ord, vx, vy, vz);        // (len follows from them)
			const float r = recip_refined(len);
			rdx = div_by(vx, len, r), rdy = div_by(vy, len, r), rdz = div_by(vz, len, r);
		}
		else
			rdx = vx / len, rdy = vy / len, rdz = vz / len;
	}
	float xx, xy, xz, ray_distance;        // ray_exit
	{
		float ix, iy, iz;
		if (FAST)
		{
			ord_low(ord, rdx, rdy, rdz);
			ix = recip_exact(rdx), iy = recip_exact(rdy), iz = recip_exact(rdz);
		}
		else
			ix = 1.0f / rdx, iy = 1.0f / rdy, iz = 1.0f / rdz;
		const float tminx = -ex * ix, tminy = -ey * iy, tminz = -ez * iz;
		const float tmaxx = (1.0f - ex) * ix, tmaxy = (1.0f - ey) * iy, tmaxz = (1.0f - ez) * iz;
		const float t2x = g_max(tminx, tmaxx), t2y = g_max(tminy, tmaxy), t2z = g_max(tminz, tmaxz);
		const float tFar = g_min(g_min(t2x, t2y), t2z);
		xx = __builtin_fmaf(tFar, rdx, ex), xy = __builtin_fmaf(tFar, rdy, ey), xz = __builtin_fmaf(tFar, rdz, ez);
		const float vx = ex - xx, vy = ey - xy, vz = ez - xz;
		ray_distance = __builtin_sqrtf(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
	}
	if (A.depth_attachment)
	{        // frag:152-164: stop the ray where it meets the depth buffer
		const float clip[4] = {(position[0] * frag_depth) / frag_depth_front, (position[1] * frag_depth) / frag_depth_front,
		                       (position[2] * frag_depth) / frag_depth_front, position[3]};
		float       w4[4], m4[4];
		mat4_mul_vec4(A.view_proj_inv, clip, w4);
		w4[0] /= w4[3], w4[1] /= w4[3], w4[2] /= w4[3], w4[3] /= w4[3];
		mat4_mul_vec4(A.model_inv, w4, m4);
		const float ix = m4[0] + 0.5f, iy = m4[1] + 0.5f, iz = m4[2] + 0.5f;
		const float vx = ex - ix, vy = ey - iy, vz = ez - iz;
		const float dd = __builtin_sqrtf(__builtin_fmaf(vz, vz, __builtin_fmaf(vy, vy, vx * vx)));
		if (dd < ray_distance)
		{
			xx = ix, xy = iy, xz = iz;
			ray_distance = dd;
		}
	}
	if (A.test == VKV_TEST_RAY_ENTRY)
	{
		R.r = ex, R.g = ey, R.b = ez, R.a = 1.0f;
		return false;
	}
	if (A.test == VKV_TEST_RAY_EXIT)
	{
		R.r = xx, R.g = xy, R.b = xz, R.a = 1.0f;
		return false;
	}

	// ---- frag:176-187 --------------------------------------------------------------------------------------
	const int   dim_max = max(max(W, H), D);
	const float nf      = __builtin_ceilf((float) dim_max * ray_distance * A.sampling_factor);
	if (!(nf >= 2.0f && nf <= 16777216.0f))
		return false;
	float sx, sy, sz;
	{
		const float den = nf - 1.0f, nx = rdx * ray_distance, ny = rdy * ray_distance, nz = rdz * ray_distance;
		if (FAST)
		{
			ord_both(ord, nx, ny, nz);        // den is 1 .. 2^24
			const float r = recip_refined(den);
			sx = div_by(nx, den, r), sy = div_by(ny, den, r), sz = div_by(nz, den, r);
		}
		else
			sx = nx / den, sy = ny / den, sz = nz / den;
	}
	{
		const float qx = ex + sx, qy = ey + sy, qz = ez + sz;
		if (qx <= 0.0f || qy <= 0.0f || qz <= 0.0f || qx >= 1.0f || qy >= 1.0f || qz >= 1.0f)
			return false;
	}
	R.ex = ex, R.ey = ey, R.ez = ez, R.sx = sx, R.sy = sy, R.sz = sz;
	R.n_steps = (int) nf;

	// ---- frag:191-214 --------------------------------------------------------------------------------------
	R.six = R.siy = R.siz = 0.0f;
	R.dmap                = nullptr;
	if (SKIP != VKV_SKIP_NONE)
	{
		if (FAST)
		{
			const float nx = sx * (float) W, ny = sy * (float) H, nz = sz * (float) D;
			ord.lo = ord_min(ord.lo, A.ord_lo0);        // the block sizes: 0 when one of them is not ordinary
			ord_both(ord, nx, ny, nz);
			// (a power-of-two block: the product is the IEEE quotient, and it stays a normal number - nx is at least 2^-39 here, or `ord` fails)
			float tx, ty, tz;
			if (A.block_pow2 != 0u)        // (one wave-uniform branch for the three axes: a branch per axis costs what its multiplication saves)
				tx = nx * A.block_rcp[0], ty = ny * A.block_rcp[1], tz = nz * A.block_rcp[2];
			else
			{
				tx = div_by(nx, A.block_size[0], recip_refined(A.block_size[0]));
				ty = div_by(ny, A.block_size[1], recip_refined(A.block_size[1]));
				tz = div_by(nz, A.block_size[2], recip_refined(A.block_size[2]));
			}
			ord_both(ord, tx, ty, tz);
			R.six = recip_exact(tx), R.siy = recip_exact(ty), R.siz = recip_exact(tz);
		}
		else
		{
			R.six = 1.0f / ((sx * (float) W) / A.block_size[0]);
			R.siy = 1.0f / ((sy * (float) H) / A.block_size[1]);
			R.siz = 1.0f / ((sz * (float) D) / A.block_size[2]);
		}
		if (SKIP == VKV_SKIP_ANISOTROPIC_DISTANCE)
			R.dmap = A.maps[(rdz < 0 ? 1 : 0) + (rdy < 0 ? 2 : 0) + (rdx < 0 ? 4 : 0)];
		else
			R.dmap = A.maps[0];
	}
	R.i = 0, R.i_min = 0, R.ulx = R.uly = R.ulz = 0, R.ul = 0;
	R.occupied  = true;
	R.first_hit = R.n_steps;
	return true;
}

// The set-up every kernel calls: the fast divisions when every operand of every lane of the wave is ordinary, else (axis-parallel
// rays, degenerate cameras) the plain IEEE ones for the whole wave - the same bits either way.
template <int SKIP>
__device__ __forceinline__ bool ray_setup(const RayMarchArgs &A, uint32_t px, uint32_t py, Ray &R)
{
	OrdRange   ord     = {~0u, 0u};
	const bool marched = ray_setup_impl<SKIP, true>(A, px, py, R, ord);
	if (__builtin_amdgcn_ballot_w64(!ord_ok(ord)) == 0ull)
		return marched;
	OrdRange unused = {~0u, 0u};
	return ray_setup_impl<SKIP, false>(A, px, py, R, unused);
}

// the state ray_setup leaves behind for a pixel the volume's box does not cover
__device__ __forceinline__ void ray_clear(Ray &R)
{
	R.r = R.g = R.b = R.a = 0.0f;
	R.depth = 0.0f;
	R.n_vol = R.n_dist = R.n_empty = 0;
	R.n_steps = 0, R.i = 0, R.i_min = 0, R.first_hit = 0, R.ul = 0;
	R.fragment = false;
}

// frag:315-334 + the stores.  `marched` is false for pixels that never entered the loop.
__device__ __forceinline__ void ray_finish(const RayMarchArgs &A, Ray &R, bool marched)
{
	if (marched)
	{
		if (A.out_depth && R.a > 0.0f && R.first_hit < R.n_steps)
		{        // frag:315-321
			const float fi   = (float) R.first_hit;
			const float p[4] = {__builtin_fmaf(fi, R.sx, R.ex) - 0.5f, __builtin_fmaf(fi, R.sy, R.ey) - 0.5f, __builtin_fmaf(fi, R.sz, R.ez) - 0.5f, 1.0f};
			float       a4[4], b4[4], c4[4];
			mat4_mul_vec4(A.model, p, a4);
			mat4_mul_vec4(A.view, a4, b4);
			mat4_mul_vec4(A.proj, b4, c4);
			R.depth = c4[2] / c4[3];
		}
		if (A.test == VKV_TEST_NUM_TEXTURE_SAMPLES)
		{        // frag:324-334
			const int      dim_max     = max(max(A.W, A.H), A.D);
			const uint32_t n_steps_max = (uint32_t) (__builtin_ceilf((float) dim_max * __builtin_sqrtf(3.0f)) * A.sampling_factor);
			const float    v           = (float) (R.n_vol + R.n_dist) / (float) n_steps_max;
			R.r = R.g = R.b = v;
			R.a             = 1.0f;
		}
	}
	const size_t o = R.o;
	if (!R.fragment)
	{        // no fragment: an existing target stays as it is, a fresh one holds the clear values
		if (A.blend)
		{
			if (A.out_counts)
				A.out_counts[o * 3 + 0] = A.out_counts[o * 3 + 1] = A.out_counts[o * 3 + 2] = 0;
			return;
		}
		if (A.depth_attachment)
			R.depth = A.in_depth[o];
		// a fresh target gets the clear values (out_color = 0, counters 0: nothing was added to them since ray_setup / ray_clear)
		if (A.out_color)
			store_float4_nt(A.out_color, o, 0.0f, 0.0f, 0.0f, 0.0f);
		if (A.out_rgba8)
			__builtin_nontemporal_store(0u, reinterpret_cast<uint32_t *>(A.out_rgba8) + o);
		if (A.out_counts)
			A.out_counts[o * 3 + 0] = A.out_counts[o * 3 + 1] = A.out_counts[o * 3 + 2] = 0;
		if (A.out_depth)
			__builtin_nontemporal_store(R.depth, A.out_depth + o);
		return;
	}
	else if (A.blend)
	{        // blend state of the subpass (src/volume_render_subpass.cpp:176-190): rgb = src + (1 - src.a) * dst, a = src.a * (1 - src.a)
		const float om = 1.0f - R.a;
		if (A.out_color)
		{
			float4 d = reinterpret_cast<float4 *>(A.out_color)[o];
			d.x = __builtin_fmaf(om, d.x, R.r), d.y = __builtin_fmaf(om, d.y, R.g), d.z = __builtin_fmaf(om, d.z, R.b), d.w = R.a * om;
			reinterpret_cast<float4 *>(A.out_color)[o] = d;
		}
		if (A.out_rgba8)
		{
			const uint32_t d = reinterpret_cast<uint32_t *>(A.out_rgba8)[o];
			const float    r = __builtin_fmaf(om, unorm8(d & 255u), R.r), g = __builtin_fmaf(om, unorm8((d >> 8) & 255u), R.g),
			            b = __builtin_fmaf(om, unorm8((d >> 16) & 255u), R.b);
			reinterpret_cast<uint32_t *>(A.out_rgba8)[o] = (uint32_t) quantise_rgba8(r) | ((uint32_t) quantise_rgba8(g) << 8) |
			                                               ((uint32_t) quantise_rgba8(b) << 16) | ((uint32_t) quantise_rgba8(R.a * om) << 24);
		}
		if (A.out_counts)
		{
			A.out_counts[o * 3 + 0] = R.n_vol;
			A.out_counts[o * 3 + 1] = R.n_dist;
			A.out_counts[o * 3 + 2] = R.n_empty;
		}
		if (A.out_depth)
			A.out_depth[o] = R.depth;
		return;
	}
	if (A.out_color)
		store_float4_nt(A.out_color, o, R.r, R.g, R.b, R.a);
	// (non-temporal, like the float colour above and the depth below: the frame is not read again by this kernel, and its 8 MB per frame would otherwise push volume bricks out of the L2s:
	// 0.1157 -> 0.1139 ms per frame on C3)
	if (A.out_rgba8)
		__builtin_nontemporal_store((uint32_t) quantise_rgba8(R.r) | ((uint32_t) quantise_rgba8(R.g) << 8) |
		                                               ((uint32_t) quantise_rgba8(R.b) << 16) | ((uint32_t) quantise_rgba8(R.a) << 24), reinterpret_cast<uint32_t *>(A.out_rgba8) + o);
	if (A.out_counts)
	{
		A.out_counts[o * 3 + 0] = R.n_vol;
		A.out_counts[o * 3 + 1] = R.n_dist;
		A.out_counts[o * 3 + 2] = R.n_empty;
	}
	if (A.out_depth)
		__builtin_nontemporal_store(R.depth, A.out_depth + o);
}

// Computed start order of a schedule over a tile rectangle (RayMarchArgs.order_h; wave-uniform, once per workgroup, no table): which schedule
// entry is started r-th.  Ring by ring from the innermost ring of the w x h rectangle to its border (ring j = the tiles with j tiles between them
// and the nearest border; the rectangle inside ring j holds (w - 2j)(h - 2j) tiles, so the ring of rank r follows from a square root), inside a
// ring clockwise from its top left tile.  The volume's silhouette and the empty corners of the rectangle start last, as with the centre-first
// table of a whole-image schedule - but a rectangle's size changes with the camera, and a table per size does not pay (a camera that moves
// gives every frame in flight its own: profiles/r6_rect_schedules.txt).  Launches of 2 - 4 frames on one stream: -11 % against the plain order.
// Hands back the tile's column and row in the rectangle as well (tx, ty): the entry is ty * w + tx, and a caller that deals pixels needs them apart.
__device__ __forceinline__ uint32_t start_entry(const RayMarchArgs &A, uint32_t r, uint32_t &tx_out, uint32_t &ty_out)
{
	const int w = (int) A.tiles_x, h = (int) A.order_h, rings = (min(w, h) + 1) >> 1;
	auto      inner = [&](int j) { return (w - 2 * j > 0 && h - 2 * j > 0) ? (uint32_t) ((w - 2 * j) * (h - 2 * j)) : 0u; };        // tiles inside ring j - 1
	const float d = (float) (w - h);
	int         j = (int) (((float) (w + h) - __builtin_sqrtf(d * d + 4.0f * (float) r)) * 0.25f);
	j             = max(0, min(j, rings - 1));
#pragma unroll
	for (int it = 0; it < 2; ++it)        // the float estimate is off by one at most
	{
		if (j + 1 < rings && inner(j + 1) > r)
			++j;
		if (j > 0 && inner(j) <= r)
			--j;
	}
	const int wj = w - 2 * j, hj = h - 2 * j;
	int       q = (int) (r - inner(j + 1)), tx, ty;
	if (hj == 1 || q < wj)
		tx = j + q, ty = j;        // top edge, left to right (all of a one-row ring)
	else if ((q -= wj) < hj - 1)
		tx = j + wj - 1, ty = j + 1 + q;        // right edge, downwards
	else if ((q -= hj - 1) < wj - 1)
		tx = j + wj - 2 - q, ty = j + hj - 1;        // bottom edge, right to left
	else
		q -= wj - 1, tx = j, ty = j + hj - 2 - q;        // left edge, upwards
	tx_out = (uint32_t) __builtin_amdgcn_readfirstlane(tx), ty_out = (uint32_t) __builtin_amdgcn_readfirstlane(ty);
	return ty_out * (uint32_t) w + tx_out;
}
__device__ __forceinline__ uint32_t start_entry(const RayMarchArgs &A, uint32_t r)
{
	uint32_t tx, ty;
	return start_entry(A, r, tx, ty);
}

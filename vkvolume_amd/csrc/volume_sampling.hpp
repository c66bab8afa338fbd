// volume_sampling.hpp — the volume filters (sample_linear on the plain volume, packed_footprint / packed_filter / sample_packed on the packed
// image) and the small device helpers every renderer shares (mat4_mul_vec4, quantise_rgba8, store_float4_nt).  Included by ray_setup.hpp,
// raymarch_persistent.hpp and raymarch_core.hpp, and by the direct renderers (direct_render.hpp, mip.hip, iso.hip, slab.hip).
#pragma once

#include "vkv_device.hpp"

using namespace vkv;

// Linear filter, clamp-to-edge (sampler: src/volume_component.cpp:139-148); see DESIGN.md "Pinned numerics".
__device__ __forceinline__ float sample_linear(const uint8_t *__restrict__ tex, int W, int H, int D, float px, float py, float pz)
{
	const float cx = __builtin_fmaf(px, (float) W, -0.5f), cy = __builtin_fmaf(py, (float) H, -0.5f), cz = __builtin_fmaf(pz, (float) D, -0.5f);
	const float fx = __builtin_floorf(cx), fy = __builtin_floorf(cy), fz = __builtin_floorf(cz);
	const float wx = cx - fx, wy = cy - fy, wz = cz - fz;
	const int   ix = (int) fx, iy = (int) fy, iz = (int) fz;
	const int   x0 = i_clamp(ix, 0, W - 1), x1 = i_clamp(ix + 1, 0, W - 1);
	const int   y0 = i_clamp(iy, 0, H - 1), y1 = i_clamp(iy + 1, 0, H - 1);
	const int   z0 = i_clamp(iz, 0, D - 1), z1 = i_clamp(iz + 1, 0, D - 1);
	const size_t r00 = ((size_t) z0 * (size_t) H + (size_t) y0) * (size_t) W, r10 = ((size_t) z0 * (size_t) H + (size_t) y1) * (size_t) W;
	const size_t r01 = ((size_t) z1 * (size_t) H + (size_t) y0) * (size_t) W, r11 = ((size_t) z1 * (size_t) H + (size_t) y1) * (size_t) W;
	const float b000 = tex[r00 + x0], b100 = tex[r00 + x1];
	const float b010 = tex[r10 + x0], b110 = tex[r10 + x1];
	const float b001 = tex[r01 + x0], b101 = tex[r01 + x1];
	const float b011 = tex[r11 + x0], b111 = tex[r11 + x1];
	const float c00 = __builtin_fmaf(wx, b100 - b000, b000), c10 = __builtin_fmaf(wx, b110 - b010, b010);
	const float c01 = __builtin_fmaf(wx, b101 - b001, b001), c11 = __builtin_fmaf(wx, b111 - b011, b011);
	const float c0 = __builtin_fmaf(wy, c10 - c00, c00), c1 = __builtin_fmaf(wy, c11 - c01, c01);
	return __builtin_fmaf(wz, c1 - c0, c0) * kInv255;
}

// Same filter on the packed image: the whole 2x2x2 footprint of BOTH textures sits in one 256-byte brick, the x pair of
// a row is one (2-byte aligned) dword = (v0, g0, v1, g1).  Arithmetic identical to sample_linear, so results are too.
typedef uint32_t u32_align2 __attribute__((aligned(2)));

// address of the footprint's first dword + the three filter weights
__device__ __forceinline__ const uint8_t *packed_footprint(const uint8_t *__restrict__ P, int W, int H, int D, int pmx, int pmy, float px, float py, float pz,
                                                           float &wx, float &wy, float &wz)
{
	const float cx = __builtin_fmaf(px, (float) W, -0.5f), cy = __builtin_fmaf(py, (float) H, -0.5f), cz = __builtin_fmaf(pz, (float) D, -0.5f);
	const float fx = __builtin_floorf(cx), fy = __builtin_floorf(cy), fz = __builtin_floorf(cz);
	wx = cx - fx, wy = cy - fy, wz = cz - fz;
	const int bx = i_clamp((int) fx, -1, W) + 1, by = i_clamp((int) fy, -1, H) + 1, bz = i_clamp((int) fz, -1, D) + 1;
	// 32-bit brick index (macro-brick * 512 + brick-in-macro), one 64-bit shift for the byte offset
	const uint32_t macro = ((uint32_t) (bz >> 5) * (uint32_t) pmy + (uint32_t) (by >> 5)) * (uint32_t) pmx + (uint32_t) (bx >> 5);
	const uint32_t sub   = (uint32_t) ((((bz >> 2) & 7) << 6) | (((by >> 2) & 7) << 3) | ((bx >> 2) & 7));
	const uint32_t in    = (uint32_t) ((((bz & 3) * 5 + (by & 3)) * 5 + (bx & 3)) * 2);
	return P + (((uint64_t) (macro * 512u + sub)) << 8) + in;
}

// the four x-pair dwords (v0, g0, v1, g1) of rows (y0,z0), (y1,z0), (y0,z1), (y1,z1) -> filtered volume (and gradient) value
template <bool WANT_G>
__device__ __forceinline__ void packed_filter(uint32_t q00, uint32_t q10, uint32_t q01, uint32_t q11, float wx, float wy, float wz, float &out_v, float &out_g)
{
	{
		const float b000 = (float) (q00 & 255u), b100 = (float) ((q00 >> 16) & 255u);
		const float b010 = (float) (q10 & 255u), b110 = (float) ((q10 >> 16) & 255u);
		const float b001 = (float) (q01 & 255u), b101 = (float) ((q01 >> 16) & 255u);
		const float b011 = (float) (q11 & 255u), b111 = (float) ((q11 >> 16) & 255u);
		const float c00 = __builtin_fmaf(wx, b100 - b000, b000), c10 = __builtin_fmaf(wx, b110 - b010, b010);
		const float c01 = __builtin_fmaf(wx, b101 - b001, b001), c11 = __builtin_fmaf(wx, b111 - b011, b011);
		const float c0 = __builtin_fmaf(wy, c10 - c00, c00), c1 = __builtin_fmaf(wy, c11 - c01, c01);
		out_v = __builtin_fmaf(wz, c1 - c0, c0) * kInv255;
	}
	if (WANT_G)
	{
		const float b000 = (float) ((q00 >> 8) & 255u), b100 = (float) (q00 >> 24);
		const float b010 = (float) ((q10 >> 8) & 255u), b110 = (float) (q10 >> 24);
		const float b001 = (float) ((q01 >> 8) & 255u), b101 = (float) (q01 >> 24);
		const float b011 = (float) ((q11 >> 8) & 255u), b111 = (float) (q11 >> 24);
		const float c00 = __builtin_fmaf(wx, b100 - b000, b000), c10 = __builtin_fmaf(wx, b110 - b010, b010);
		const float c01 = __builtin_fmaf(wx, b101 - b001, b001), c11 = __builtin_fmaf(wx, b111 - b011, b011);
		const float c0 = __builtin_fmaf(wy, c10 - c00, c00), c1 = __builtin_fmaf(wy, c11 - c01, c01);
		out_g = __builtin_fmaf(wz, c1 - c0, c0) * kInv255;
	}
}

template <bool WANT_G>
__device__ __forceinline__ void sample_packed(const uint8_t *__restrict__ P, int W, int H, int D, int pmx, int pmy, float px, float py, float pz,
                                              float &out_v, float &out_g)
{
	float          wx, wy, wz;
	const uint8_t *b   = packed_footprint(P, W, H, D, pmx, pmy, px, py, pz, wx, wy, wz);
	const uint32_t q00 = *reinterpret_cast<const u32_align2 *>(b);
	const uint32_t q10 = *reinterpret_cast<const u32_align2 *>(b + 10);
	const uint32_t q01 = *reinterpret_cast<const u32_align2 *>(b + 50);
	const uint32_t q11 = *reinterpret_cast<const u32_align2 *>(b + 60);
	packed_filter<WANT_G>(q00, q10, q01, q11, wx, wy, wz, out_v, out_g);
}

__device__ __forceinline__ void mat4_mul_vec4(const float *m, const float *v, float *r)
{
#pragma unroll
	for (int i = 0; i < 4; ++i)
		r[i] = __builtin_fmaf(m[12 + i], v[3], __builtin_fmaf(m[8 + i], v[2], __builtin_fmaf(m[4 + i], v[1], m[i] * v[0])));
}

__device__ __forceinline__ uint8_t quantise_rgba8(float c) { return (uint8_t) __builtin_rintf(g_clamp(c, 0.0f, 1.0f) * 255.0f); }

// 16-byte non-temporal store of one RGBA32F pixel (an ext_vector so that it stays one global_store_dwordx4 nt)
__device__ __forceinline__ void store_float4_nt(float *base, size_t pixel, float r, float g, float b, float a)
{
	typedef float float4v __attribute__((ext_vector_type(4)));
	const float4v v = {r, g, b, a};
	__builtin_nontemporal_store(v, reinterpret_cast<float4v *>(base) + pixel);
}

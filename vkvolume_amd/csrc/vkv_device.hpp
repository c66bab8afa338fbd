// vkv_device.hpp — shared device-side definitions for the gfx950 kernels.
//
// The arithmetic below is the product's definition of the numerics the reference leaves to the Vulkan
// implementation (DESIGN.md "Pinned numerics"): fp32 only, no implicit contraction (the library is
// built with -ffp-contract=off), fused multiply-adds only where __builtin_fmaf is written out,
// IEEE-correct division and square root (-fhip-fp32-correctly-rounded-divide-sqrt).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vkvolume_amd.h"
#include "../host/host_arith.hpp"        // kInv255: the host derives thresholds with the kernels' constant

namespace vkv
{

// GLSL built-ins with specification semantics (min(x,y) = y<x ? y : x, ...).
__device__ __forceinline__ float g_min(float x, float y) { return (y < x) ? y : x; }
__device__ __forceinline__ float g_max(float x, float y) { return (x < y) ? y : x; }
__device__ __forceinline__ float g_clamp(float x, float lo, float hi) { return g_min(g_max(x, lo), hi); }
__device__ __forceinline__ float g_step(float edge, float x) { return (x < edge) ? 0.0f : 1.0f; }
__device__ __forceinline__ float g_sign(float x) { return (x > 0.0f) ? 1.0f : ((x < 0.0f) ? -1.0f : 0.0f); }
__device__ __forceinline__ int   i_clamp(int x, int lo, int hi) { return min(max(x, lo), hi); }

__device__ __forceinline__ size_t vidx(int x, int y, int z, int W, int H)
{
	return ((size_t) z * (size_t) H + (size_t) y) * (size_t) W + (size_t) x;
}

// R8_UNORM texel -> float: exactly byte / 255 (IEEE division).
__device__ __forceinline__ float unorm8(uint32_t b) { return (float) b / 255.0f; }

// NEAREST lookup coordinate of the 256-wide TF texture (sampler: src/volume_component.cpp:149-151).
__device__ __forceinline__ int tf_texel(float u) { return i_clamp((int) __builtin_floorf(u * 256.0f), 0, 255); }

// Tetrahedron gradient on integer texels, shaders/get_gradient_compute.glsl:12-20; returns the float in [0,1]
// before the UNORM store.  Term order k.xyy, k.yyx, k.yxy, k.xxx, sums left to right.
__device__ __forceinline__ float gradient_from_taps(float v1, float v2, float v3, float v4, float modifier)
{
	const float gx  = 0.25f * (((v1 - v2) - v3) + v4);
	const float gy  = 0.25f * (((-v1 - v2) + v3) + v4);
	const float gz  = 0.25f * (((-v1 + v2) - v3) + v4);
	const float len = __builtin_sqrtf((gx * gx + gy * gy) + gz * gz);
	return g_clamp(len * modifier, 0.0f, 1.0f);
}

__device__ __forceinline__ float gradient_on_the_fly(const uint8_t *__restrict__ vol, int W, int H, int D, int x, int y, int z, float modifier)
{
	const int   xm = max(x - 1, 0), xp = min(x + 1, W - 1);
	const int   ym = max(y - 1, 0), yp = min(y + 1, H - 1);
	const int   zm = max(z - 1, 0), zp = min(z + 1, D - 1);
	const float v1 = unorm8(vol[vidx(xp, ym, zm, W, H)]);
	const float v2 = unorm8(vol[vidx(xm, ym, zp, W, H)]);
	const float v3 = unorm8(vol[vidx(xm, yp, zm, W, H)]);
	const float v4 = unorm8(vol[vidx(xp, yp, zp, W, H)]);
	return gradient_from_taps(v1, v2, v3, v4, modifier);
}

// ---- correctly rounded fp32 division out of v_rcp_f32 (the ray set-up's 22 divisions per ray; see ray_setup.hpp) ----
__host__ __device__ __forceinline__ bool div_ordinary(float x)
{
	const float m = __builtin_fabsf(x);
	return m >= 0x1p-40f && m <= 0x1p40f;        // false for 0, denormals, huge values, inf and NaN
}
__host__ __device__ __forceinline__ bool div_ordinary_num(float x)
{        // (a zero numerator is NOT ordinary: the refinement loses the sign of -0 / d)
	return div_ordinary(x);
}
// The set-up's form of the same test: instead of one div_ordinary per operand (two compares and the mask bookkeeping that folds them into a
// flag), the smallest and the largest MAGNITUDE of all operands of a lane, as bit patterns without the sign - for those the integer order is
// the order of the magnitudes, with +-0 and the denormals at the bottom (below 0x00800000) and +-inf and every NaN at the top (from
// 0x7f800000) - and two compares at the end (ord_ok).  The bounds are one binade INSIDE div_ordinary's on either side, 2^-39 and 2^39: ord_ok
// then implies div_ordinary of every operand that went in, and of the few that are left out because they follow from operands that did (the
// length of a vector whose components went in: ray_setup.hpp gives the argument; tests/test_ray_setup_range_cpu.py checks all of it on the host).
struct OrdRange
{
	uint32_t lo, hi;        // smallest / largest magnitude so far; the host starts lo (RayMarchArgs.ord_lo0: ~0u, or 0 = "never ordinary")
};
constexpr uint32_t kOrdLoBits = 0x2c000000u, kOrdHiBits = 0x53000000u;        // 2^-39, 2^39
__host__ __device__ __forceinline__ uint32_t ord_mag(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7fffffffu; }
__host__ __device__ __forceinline__ uint32_t ord_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
__host__ __device__ __forceinline__ uint32_t ord_max(uint32_t a, uint32_t b) { return b > a ? b : a; }
// operands whose magnitude has to be tested on both sides
__host__ __device__ __forceinline__ void ord_both(OrdRange &r, float a)
{
	const uint32_t m = ord_mag(a);
	r.lo = ord_min(r.lo, m), r.hi = ord_max(r.hi, m);
}
__host__ __device__ __forceinline__ void ord_both(OrdRange &r, float a, float b, float c) { ord_both(r, a), ord_both(r, b), ord_both(r, c); }
// operands that are bounded above by construction (a component of a normalised vector: ray_setup.hpp): only the lower bound can fail.  NOT for
// an operand that can be inf or NaN.
__host__ __device__ __forceinline__ void ord_low(OrdRange &r, float a) { r.lo = ord_min(r.lo, ord_mag(a)); }
__host__ __device__ __forceinline__ void ord_low(OrdRange &r, float a, float b, float c) { ord_low(r, a), ord_low(r, b), ord_low(r, c); }
__host__ __device__ __forceinline__ bool ord_ok(const OrdRange &r) { return r.lo >= kOrdLoBits && r.hi <= kOrdHiBits; }

__device__ __forceinline__ float recip_refined(float d)
{
	const float r0 = __builtin_amdgcn_rcpf(d);
	const float e  = __builtin_fmaf(-d, r0, 1.0f);
	return __builtin_fmaf(e, r0, r0);
}
// a / d given r = recip_refined(d)
__host__ __device__ __forceinline__ float div_by(float a, float d, float r)
{
	const float q0 = a * r;
	const float q1 = __builtin_fmaf(__builtin_fmaf(-d, q0, a), r, q0);
	return __builtin_fmaf(__builtin_fmaf(-d, q1, a), r, q1);
}
// 1 / d (the same sequence with a = 1: q0 = r)
__device__ __forceinline__ float recip_exact(float d)
{
	const float r  = recip_refined(d);
	const float q1 = __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
	return __builtin_fmaf(__builtin_fmaf(-d, q1, 1.0f), r, q1);
}
// byte / 255 with the IEEE quotient's bits and without the division: div_by with the correctly rounded reciprocal as r (a constant; checked
// against the division for all 256 bytes on the host, tests/test_ray_setup_range_cpu.py, and 0 * r = 0 needs no special case: the byte is unsigned).
// For the tables a workgroup stages in front of its march loop (stage_tables_er); unorm8 stays the definition.
__host__ __device__ __forceinline__ float unorm8_staged(uint32_t b) { return div_by((float) b, 255.0f, kInv255); }

// A block size that is a power of two (the application's is 4): 1 / block is a float, and n * (1 / block) is the correctly rounded n / block -
// the IEEE quotient - for every n.  The host half of the set-up's divisions by the block size (fill_render_args): the exact reciprocal, or 0 when
// the block size is no power of two in [2^-39, 2^39] (the kernel then divides: ray_setup_impl).
__host__ __device__ __forceinline__ float pow2_reciprocal(float block)
{
	const uint32_t u = __builtin_bit_cast(uint32_t, block);
	if ((u & 0x807fffffu) != 0u || u < kOrdLoBits || u > kOrdHiBits)        // negative, a mantissa bit set, or outside the range (0, denormal, inf, NaN)
		return 0.0f;
	return __builtin_bit_cast(float, 0x7f000000u - u);        // 2^-(e - 127): exponent field 254 - e
}

// R8_UNORM store: round to nearest even.
__device__ __forceinline__ uint8_t store_unorm8(float g) { return (uint8_t) __builtin_rintf(g * 255.0f); }

// Four bytes of a voxel row as ONE dword, whatever the row's alignment (round 6: the tiled kernels no longer need W % 4 == 0).  Rows of a volume
// whose width is no multiple of 4 start at every byte alignment; global loads need none on gfx950 (the integrator's own footprint gathers are
// 2-byte aligned), the type only tells the compiler not to assume one.
typedef uint32_t u32_any_align __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t load_u32_any(const uint8_t *p) { return *reinterpret_cast<const u32_any_align *>(p); }
// Dword column dc (voxels 4 dc .. 4 dc + 3) of a row of W >= 4 voxels, dc < ceil(W / 4): the last, partial column of an odd width is read as the
// row's LAST four bytes and shifted down - nothing past the row is touched, the bytes of x >= W come back zero.
__device__ __forceinline__ uint32_t row_dword(const uint8_t *row, int dc, int W)
{
	const int x = 4 * dc;
	if (x + 4 <= W)
		return load_u32_any(row + x);
	return load_u32_any(row + (W - 4)) >> (8 * (x + 4 - W));
}

// analytic get_color (transfer_function.glsl:41-43) > 0
__device__ __forceinline__ bool analytic_occupied(float intensity, float gradient, float imin, float iinv, float gmin, float ginv)
{
	const float ai = g_clamp((intensity - imin) * iinv, 0.0f, 1.0f);
	const float ag = g_clamp((gradient - gmin) * ginv, 0.0f, 1.0f);
	return ai * ag > 0.0f;
}

// XCD-aware block remap: hardware deals consecutive block ids round-robin over the 8 XCDs, so give each XCD a
// contiguous range of logical ids (neighbouring screen tiles / slabs then share one L2).
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t nb)
{
	const uint32_t q = nb >> 3, r = nb & 7u, xcd = b & 7u, idx = b >> 3;
	return xcd * q + min(xcd, r) + idx;
}

// ---- transfer-function acceleration tables (vkv_transfer_function_tables), uint32 words ---------------------------------
// [0, 2048)     1 bit per texel of the 256x256 texture: alpha > 0 (row = gradient)
// [2048]        flags: kTfFlagSeparable = every texel is (b, b, b, b) with b = (uint8) clamp((ai[col] * ag[row]) * 255, 0, 255),
//               checked on the device for all 65536 texels with the arithmetic the integrator uses
// [2052, 2308)  ai[256] (float bits), [2308, 2564) ag[256]
constexpr uint32_t kTfFlagWord = 2048, kTfAiWord = 2052, kTfAgWord = 2308, kTfWords = 2564;
constexpr uint32_t kTfFlagSeparable = 1u;
static_assert(kTfWords == VKV_TF_BITS_WORDS, "include/vkvolume_amd.h and vkv_device.hpp disagree on the table size");

// the alpha byte of a separable greyscale transfer function (src/volume_component.cpp:246-261 builds exactly this product)
__host__ __device__ __forceinline__ uint32_t tf_separable_alpha(float ai, float ag)
{
	// ai, ag are in [0, 1] (k_tf_tables_init clamps them), so the product needs no clamp; the min keeps a table index in range whatever
	// the tables hold.  The flag that enables this path is only set after all 65536 texels were checked against exactly this function.
	const uint32_t b = (uint32_t) ((ai * ag) * 255.0f);
	return b < 255u ? b : 255u;
}

// ---- packed sampling layout (vkv_pack_volume) -------------------------------------------------------------------
// Padded index j in [0, W+2] holds voxel clamp(j-1, 0, W-1), so the clamp-to-edge footprint of texel index ix is always
// the pair (b, b+1) with b = clamp(ix, -1, W) + 1.  Brick (bx,by,bz) stores padded voxels [4b, 4b+4] per axis (5^3 with
// the apron) as interleaved (volume, gradient) byte pairs, x fastest: 250 bytes padded to 256.  Bricks are grouped
// 8x8x8 (one 128 KiB macro-brick = 32^3 voxels) so a ray's working set stays within a few pages.
struct PackedDims
{
	int bx, by, bz;        // bricks per axis
	int mx, my, mz;        // macro-bricks per axis
};

__host__ __device__ __forceinline__ PackedDims packed_dims(int W, int H, int D)
{
	PackedDims p;
	p.bx = ((W + 1) >> 2) + 1, p.by = ((H + 1) >> 2) + 1, p.bz = ((D + 1) >> 2) + 1;
	p.mx = (p.bx + 7) >> 3, p.my = (p.by + 7) >> 3, p.mz = (p.bz + 7) >> 3;
	return p;
}

__host__ __device__ __forceinline__ size_t packed_bytes(const PackedDims &p) { return (size_t) p.mx * p.my * p.mz * 512 * 256; }

__host__ __device__ __forceinline__ size_t packed_brick_offset(int bx, int by, int bz, int mx, int my)
{
	const size_t macro = ((size_t) (bz >> 3) * my + (size_t) (by >> 3)) * mx + (size_t) (bx >> 3);
	const size_t sub   = (size_t) (((bz & 7) << 6) | ((by & 7) << 3) | (bx & 7));
	return (macro * 512 + sub) * 256;
}

constexpr uint32_t kPullHeadStride = 64;        // uint32 words between two ticket counters of k_raymarch_lean_pull (256 bytes: one memory channel each; context.hpp)
}        // namespace vkv

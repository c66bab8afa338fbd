// gradient.hip — the gradient-magnitude map (vkv_gradient_map, and the grown box of a region update): one R8_UNORM byte per voxel from the
// four tetrahedron taps of shaders/gradient_map.comp:35-41.  Replaces ComputeGradientMap (src/compute_gradient_map.cpp).  Byte streaming
// bound by HBM / LDS bandwidth; no MFMA.
//
// k_gradient_map_tiled<ALIGNED> takes every volume of width >= 4 with use_gradient set.  k_gradient_map, a thread per voxel, takes the rest:
// widths below 4, use_gradient off (every byte 255), a modifier whose quarter is not a normal float, and volumes whose ten slices exceed
// 2^32 bytes.  k_check_numerics (vkv_debug_check) lives here because it checks this file's short sqrt and store against their definitions.
#include <algorithm>
#include <cmath>

#include "launchers.hpp"

using namespace vkv;

// One thread per voxel, x fastest so every load/store of a wave is one contiguous 64-byte row segment.
// The four taps sit on the (±1,±1,±1) tetrahedron, i.e. in four different (y,z) rows; L1/L2 absorb the
// 4x re-read (each byte is requested by the 4 voxels diagonal to it).
__global__ void __launch_bounds__(256) k_gradient_map(const uint8_t *__restrict__ vol, uint8_t *__restrict__ grad, int W, int H, int D,
                                                      int use_gradient, float modifier, uint32_t blocks_x, int x0, int y0, int z0, int x1, int y1)
{
	// grid.x = column blocks x 4-row groups of one z slice, grid.y = z (keeps every grid dimension x block size below 2^32
	// for 2048^3 and larger volumes); the grid covers the box [x0, x1) x [y0, y1) x [z0, z0 + grid.y) (the whole volume, or a region update's)
	const uint32_t bx = blockIdx.x % blocks_x;
	const int      x  = x0 + (int) (bx * 64 + (threadIdx.x & 63));
	const int      y  = y0 + (int) ((blockIdx.x / blocks_x) * 4 + (threadIdx.x >> 6)), z = z0 + (int) blockIdx.y;
	if (x >= x1 || y >= y1)
		return;
	float g = 1.0f;        // get_gradient_compute.glsl:6-7
	if (use_gradient)
		g = gradient_on_the_fly(vol, W, H, D, x, y, z, modifier);
	grad[vidx(x, y, z, W, H)] = store_unorm8(g);
}

// Correctly rounded sqrt for x == 0 or x normal with a normal root, from the reciprocal root (Markstein's final step): g = x * rsq(x) is
// within a few ulp, the residual x - g * g is exact in an fma, and g + residual * (0.5 * rsq) rounds to the nearest float of the true
// root.  Six instructions (v_max keeps x = 0 away from 0 * inf) where __builtin_sqrtf under -fhip-fp32-correctly-rounded-divide-sqrt
// takes sixteen (v_sqrt_f32, a one-ulp fix-up from two residual signs, rescaling of tiny inputs, inf / nan pass-through).  The
// gradient's sum of squares is 0 or >= ~1e-17 (squares of rounding residues of byte / 255 values).  vkv_debug_check (what = 0)
// compares it with __builtin_sqrtf for every float of a range; the GPU tests run it over 0 and all of [2^-90, 16).
__device__ __forceinline__ float sqrt_rn_normal(float x)
{
	const float y = __builtin_amdgcn_rsqf(__builtin_fmaxf(x, 0x1p-100f));
	const float g = x * y, h = 0.5f * y;
	return __builtin_fmaf(__builtin_fmaf(-g, g, x), h, g);
}

// R8_UNORM store of clamp(g, 0, 1) in one instruction: v_cvt_pk_u8_f32 rounds to nearest even and saturates to [0, 255], so fed
// g * 255 it equals store_unorm8(g_clamp(g, 0, 1)) for every non-NaN float (vkv_debug_check what = 1 runs over all of them).
__device__ __forceinline__ uint32_t store_unorm8_clamped(float g) { return __builtin_amdgcn_cvt_pk_u8_f32(g * 255.0f, 0u, 0u); }

// LDS-tiled version (the one the launcher uses for every width >= 4; until round 5 only for dword-aligned rows, W % 4 == 0): a workgroup computes 64 x 8 x 8 blocks of
// voxels from (64+8) x 10 x 10 halo tiles staged in LDS with coalesced dword loads, so every volume byte is fetched ~1.8x (mostly from
// L2) instead of 4x with byte gathers.
constexpr int kGradTileX = 64, kGradTileY = 8, kGradTileZ = 8, kGradPitch = 72;        // pitch = 64 + 4 texels of halo on each side
constexpr int kGradSegment = 10;                                                       // tiles one workgroup marches over

// byte store through a wave-uniform base (SGPR pair) and a 32-bit lane offset: no 64-bit vector address arithmetic per voxel
__device__ __forceinline__ void store_u8_uniform_base(uint8_t *base, uint32_t off, uint32_t value)
{
	asm volatile("global_store_byte %0, %1, %2" : : "v"(off), "v"(value), "s"(base) : "memory");
}

// (Measured in round 3 and dropped: TWO tiles of loads in flight - the tile after next requested as soon as the current one is staged:
// 0.670 against 0.654 ms on C3, 6.88 against 6.84 on C4: the loads are not what the arithmetic waits for.)
// A workgroup MARCHES along z over `seg` consecutive tiles with the next tile's dwords already in flight (held in registers) while the
// current one is computed: a workgroup that loads, waits, computes and leaves keeps too few bytes in flight per CU to cover the HBM
// latency (measured on the one-tile-per-workgroup kernel: neither the VALU nor the LDS busy more than half the time; 0.96 -> 0.85 ms
// on 1024 x 1024 x 795).  The tile holds 16-bit OFFSETS into the 256-entry table of b / 255 (4 b: the shift between the tap read and the
// table read is paid once per staged texel, not four times per voxel), two per half of a staged dword, which puts the texels of every
// group of four in the order 0, 2, 1, 3.
// ALIGNED: W % 4 == 0 and a dword-aligned volume - the staging loads are plain aligned dwords (scalar base + 32-bit lane offset addressing);
// otherwise (round 6) rows start at any alignment and the last column of a row may be partial: row_dword / load_u32_any, measured 11 - 18 %
// slower on aligned volumes (64-bit vector addresses per load), 2.4 x faster than the byte-wise kernel on odd ones.
template <bool ALIGNED>
__global__ void __launch_bounds__(256) k_gradient_map_tiled(const uint8_t *__restrict__ vol, uint8_t *__restrict__ grad, int W, int H, int D,
                                                            float modifier, uint32_t tiles_x, uint32_t tiles_y, uint32_t tiles_z, uint32_t seg,
                                                            uint32_t n_wgs, uint32_t tx0, uint32_t ty0, uint32_t tz0)
{
	// the launch covers tiles_x x tiles_y tiles from tile (tx0, ty0) and the z tiles tz0 .. tiles_z - 1 (0, 0, 0 and all tiles for the whole
	// volume; a region update passes the tiles its box touches: whole tiles are recomputed, the bytes outside the box come out as they were)
	constexpr int kRows = (kGradTileZ + 2) * (kGradTileY + 2), kCols = kGradPitch / 4, kIter = (kRows * kCols + 255) / 256;
	__shared__ __align__(16) uint16_t s_tile[kRows * kGradPitch];
	__shared__ float                  s_unorm[256];        // b / 255 (IEEE division, once per workgroup): a tap costs one LDS read, not four VALU
	s_unorm[threadIdx.x] = unorm8(threadIdx.x);
	const uint32_t t  = xcd_remap(blockIdx.x, n_wgs);
	const int      x0 = (int) (tx0 + t % tiles_x) * kGradTileX;
	const int      y0 = (int) (ty0 + (t / tiles_x) % tiles_y) * kGradTileY;
	const uint32_t k0 = tz0 + (t / (tiles_x * tiles_y)) * seg, k1 = min(k0 + seg, tiles_z);
	const int      wd = (W + 3) >> 2;        // dword columns of a row (round 6: the last one partial when W % 4 != 0; rows then start at any alignment)
	const float    quarter_modifier = 0.25f * modifier;
	// per-thread staging slots (100 rows x 18 dwords, 8 per thread): row / column of the tile are the same for every tile of the march,
	// only z moves; rows clamp in y and z, dword columns clamp in x
	int  row_xy[kIter], colc[kIter], rz[kIter];
	bool left[kIter], right[kIter];
#pragma unroll
	for (int j = 0; j < kIter; ++j)
	{
		const int d   = min((int) threadIdx.x + 256 * j, kRows * kCols - 1);
		const int row = d / kCols, col = d - row * kCols;
		const int gy = min(max(y0 - 1 + row % (kGradTileY + 2), 0), H - 1);
		const int gc = (x0 >> 2) - 1 + col;
		left[j] = gc < 0, right[j] = gc >= wd;        // clamp-to-edge in x: texel x = -1 is voxel 0, texel x = W is voxel W - 1
		row_xy[j] = gy * W, colc[j] = min(max(gc, 0), wd - 1);
		rz[j]     = row / (kGradTileY + 2) - 1;
	}
	const size_t plane = (size_t) H * (size_t) W;        // bytes of a z slice
	uint32_t     v[kIter];
	auto         fetch_edge = [&](uint32_t k) {
#pragma unroll
		for (int j = 0; j < kIter; ++j)
		{
			const int gz = min(max((int) k * kGradTileZ + rz[j], 0), D - 1);
			const uint8_t *row = vol + (size_t) gz * plane + (size_t) row_xy[j];
			uint32_t       w   = ALIGNED ? reinterpret_cast<const uint32_t *>(row)[colc[j]] : row_dword(row, colc[j], W);
			const int      nv  = W - 4 * colc[j];        // voxels of this column inside the row: 1 .. 3 in the last column of an odd width
			if (!ALIGNED && nv < 4)
				w |= (((w >> (8 * (nv - 1))) & 255u) * 0x01010101u) << (8 * nv);        // clamp-to-edge: the texels x >= W of the column are voxel W - 1
			w    = left[j] ? (w << 24) : w;
			v[j] = right[j] ? (w >> 24) : w;
		}
	};
	// tiles whose halo needs no clamp in x and z (nearly all of them): one wave-uniform base per tile and a constant 32-bit byte offset per
	// slot, i.e. no vector address arithmetic at all (10 slices of the volume stay below 2^32 bytes: checked by the launcher)
	uint32_t voff[kIter];
#pragma unroll
	for (int j = 0; j < kIter; ++j)
		voff[j] = (uint32_t) ((size_t) (rz[j] + 1) * plane + (size_t) row_xy[j] + (size_t) (4 * colc[j]));
	const bool inner_x = x0 > 0 && x0 + kGradTileX + 4 <= W;
	auto       fetch   = [&](uint32_t k) {
        if (inner_x && k > 0 && (int) (k + 1) * kGradTileZ < D)
        {
            const uint8_t *base = vol + ((size_t) k * kGradTileZ - 1) * plane;
#pragma unroll
            for (int j = 0; j < kIter; ++j)
            {
                uint32_t o = voff[j];
                asm volatile("" : "+v"(o));        // keeps the zero-extension next to the load: scalar base + 32-bit lane offset addressing
                v[j] = ALIGNED ? *reinterpret_cast<const uint32_t *>(base + o) : load_u32_any(base + o);
            }
        }
        else
            fetch_edge(k);
	};
	fetch(k0);
	const int      lx = threadIdx.x & 63, x = x0 + lx, ly0 = (int) (threadIdx.x >> 6) * 2;        // lane = x, each wave two y rows, all z
	const uint32_t off = (uint32_t) (y0 + ly0) * (uint32_t) W + (uint32_t) x, off1 = off + (uint32_t) W;        // inside one z slice (< 2^32 voxels)
	constexpr int  sy = kGradPitch, sz = (kGradTileY + 2) * kGradPitch;
	// position of texel i of a row in the tile (0, 2, 1, 3 within every four), for the lane's x - 1 and x + 1; texel x sits at column x - x0 + 4
	auto      column = [](int i) { return (i & ~3) | ((i & 1) << 1) | ((i >> 1) & 1); };
	const int cm = column(4 + lx - 1), cp = column(4 + lx + 1);
	for (uint32_t k = k0; k < k1; ++k)
	{
		__syncthreads();        // the previous tile has been read by everyone
#pragma unroll
		for (int j = 0; j < kIter; ++j)
			if ((int) threadIdx.x + 256 * j < kRows * kCols)
				reinterpret_cast<uint2 *>(s_tile)[threadIdx.x + 256 * j] = make_uint2((v[j] & 0x00ff00ffu) << 2, (v[j] & 0xff00ff00u) >> 6);
		__syncthreads();
		if (k + 1 < k1)
			fetch(k + 1);        // in flight during the arithmetic below
		const int z0 = (int) k * kGradTileZ;
		// the four taps of TWO voxels (rows ly0, ly0 + 1 of slice lz; k.xyy, k.yyx, k.yxy, k.xxx of get_gradient_compute.glsl:8-11): all reads
		// of a stage are issued before the first is used
		auto taps = [&](int lz, float(&a)[4], float(&b)[4]) {
			const int      r  = ((lz + 1) * (kGradTileY + 2) + (ly0 + 1)) * kGradPitch;
			const uint32_t a0 = s_tile[r + cp - sy - sz], a1 = s_tile[r + cm - sy + sz], a2 = s_tile[r + cm + sy - sz], a3 = s_tile[r + cp + sy + sz];
			const uint32_t b0 = s_tile[r + cp - sz], b1 = s_tile[r + cm + sz], b2 = s_tile[r + cm + 2 * sy - sz], b3 = s_tile[r + cp + 2 * sy + sz];
			__builtin_amdgcn_wave_barrier();
			auto at = [&](uint32_t o) { return *reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(s_unorm) + o); };
			a[0] = at(a0), a[1] = at(a1), a[2] = at(a2), a[3] = at(a3);
			b[0] = at(b0), b[1] = at(b1), b[2] = at(b2), b[3] = at(b3);
			__builtin_amdgcn_wave_barrier();
		};
		// get_gradient_compute.glsl:12-20, the operations of gradient_from_taps with the short exact sqrt.  The three factors 0.25 are
		// taken out: scaling by a power of two commutes with every rounding on the way (squares x 2^-4, their sums, the root x 2^-2;
		// nothing comes near the denormal range: the sum is 0 or >= ~1e-17), so sqrt(sum of (0.25 s)^2) * m == sqrt(sum of s^2) * (0.25 m)
		// bit for bit (quarter_modifier = 0.25 * modifier is exact as well).
		// (The empty asm statements keep the three chains scalar: the packed v_pk_add_f32 the compiler forms otherwise issue at 4.4 cycles
		// for two results, no faster than two full-rate scalar operations, and cost two v_mov to assemble their operands.)
		auto finish = [&](const float(&q)[4]) -> uint32_t {
			float tx = q[0] - q[1], ty = -q[0] - q[1];
			asm volatile("" : "+v"(tx));
			asm volatile("" : "+v"(ty));
			float       sx = (tx - q[2]) + q[3], sy_ = (ty + q[2]) + q[3];
			const float sz_ = ((-q[0] + q[1]) - q[2]) + q[3];
			asm volatile("" : "+v"(sx));
			asm volatile("" : "+v"(sy_));
			const float len = sqrt_rn_normal((sx * sx + sy_ * sy_) + sz_ * sz_);
			return store_unorm8_clamped(len * quarter_modifier);
		};
		uint8_t *gz = grad + (size_t) z0 * (size_t) W * (size_t) H;        // wave-uniform base, advanced per slice on the scalar unit
		if (x0 + kGradTileX <= W && y0 + kGradTileY <= H && z0 + kGradTileZ <= D)
		{        // interior tile: no masks, the eight slices unrolled
#pragma unroll
			for (int lz = 0; lz < kGradTileZ; ++lz)
			{
				float a[4], b[4];
				taps(lz, a, b);
				store_u8_uniform_base(gz, off, finish(a));
				store_u8_uniform_base(gz, off1, finish(b));
				gz += (size_t) W * (size_t) H;
			}
		}
		else if (x < W)
			for (int lz = 0; lz < kGradTileZ && z0 + lz < D; ++lz)
			{
				float a[4], b[4];
				taps(lz, a, b);
				if (y0 + ly0 < H)
					gz[off] = (uint8_t) finish(a);
				if (y0 + ly0 + 1 < H)
					gz[off1] = (uint8_t) finish(b);
				gz += (size_t) W * (size_t) H;
			}
	}
}

// vkv_debug_check: one float per thread, a mismatch counted with an atomic.
// what = 0: sqrt_rn_normal vs __builtin_sqrtf; what = 1: store_unorm8_clamped vs store_unorm8(g_clamp(., 0, 1));
// what = 2: recip_exact(x) vs 1.0f / x for every ordinary x (vkv_device.hpp; the others take the IEEE path in ray_setup by construction);
// what = 3: div_by(a, x, recip_refined(x)) vs a / x with eight hashed ordinary numerators per denominator x
// what = 4: numerators +0 and -0 must NOT take the reciprocal path (div_ordinary_num), and the quotient the dispatch delivers is the IEEE one
__global__ void __launch_bounds__(256) k_check_numerics(int what, uint32_t first_bits, uint64_t count, unsigned long long *mismatches)
{
	const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	if (i >= count)
		return;
	const uint32_t bits = first_bits + (uint32_t) i;
	const float    x    = __uint_as_float(bits);
	bool           bad  = false;
	if (what == 0)
		bad = __float_as_uint(sqrt_rn_normal(x)) != __float_as_uint(__builtin_sqrtf(x));
	else if (what == 1)
		bad = (uint8_t) store_unorm8_clamped(x) != store_unorm8(g_clamp(x, 0.0f, 1.0f));
	else if (what == 2)
		bad = div_ordinary(x) && __float_as_uint(recip_exact(x)) != __float_as_uint(1.0f / x);
	else if (what == 4)
	{        // the dispatch of ray_setup for a zero numerator: not "ordinary", so the quotient comes from the IEEE division - and it has to,
		 // the refined reciprocal path returns +0 for -0 / x (checked here too, so that nobody relaxes div_ordinary_num on the comment's word)
		const float zeros[2] = {0.0f, -0.0f};
		for (int k = 0; k < 2; ++k)
		{
			const float a = zeros[k];
			const bool  fast = div_ordinary(x) && div_ordinary_num(a);
			const float q    = fast ? div_by(a, x, recip_refined(x)) : a / x;
			bad = bad || fast || __float_as_uint(q) != __float_as_uint(a / x);
		}
	}
	else if (div_ordinary(x))
	{
		const float r = recip_refined(x);
		uint32_t    h = bits * 0x9e3779b9u + 0x7f4a7c15u;
		for (int k = 0; k < 8 && !bad; ++k)
		{
			h ^= h >> 15, h *= 0x2c1b3c6du, h ^= h >> 12, h *= 0x297a2d39u, h ^= h >> 15;
			// sign and mantissa from the hash, exponent 2^-40 .. 2^40 (biased 87 .. 167; the largest only with a zero mantissa)
			uint32_t a_bits = (h & 0x807fffffu) | ((87u + (h >> 23) % 81u) << 23);
			if (!div_ordinary(__uint_as_float(a_bits)))
				a_bits &= 0xff800000u;
			const float    a      = __uint_as_float(a_bits);
			bad                   = __float_as_uint(div_by(a, x, r)) != __float_as_uint(a / x);
		}
	}
	if (bad)
		atomicAdd(mismatches, 1ull);
}

namespace vkv
{

// the gradient of the voxels of the box [b.x0, b.x0 + b.width) x ... (inside e); launch_gradient_map: the whole volume
int launch_gradient_map_box(vkv_ctx *ctx, const uint8_t *d_vol, uint8_t *d_grad, VkvExtent3D e, const VkvBox &b, const VkvTransferFunctionUniform *tf,
                            hipStream_t s)
{
	const uint32_t blocks_x = (b.width + 63) / 64;
	if (e.depth > 65535u || (uint64_t) blocks_x * ((b.height + 3) / 4) > 0xffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "gradient_map: volume too large for one launch");
	// the tiled kernel folds the three factors 0.25 into the modifier: exact unless 0.25 * modifier is denormal (or the modifier no number)
	const float m_abs    = std::fabs(tf->grad_magnitude_modifier);
	const bool  m_normal = m_abs == 0.0f || (m_abs >= 1e-30f && m_abs <= 1e30f);
	// round 6: any width >= 4 and any alignment of the volume (the staging loads need none: row_dword / load_u32_any)
	if (tf->use_gradient && m_normal && e.width >= 4 && (uint64_t) e.width * e.height * (kGradTileZ + 2) <= 0xffffffffull)
	{
		// the tiles the box touches: [t0, t1) per axis
		const uint32_t tx0 = b.x0 / kGradTileX, ty0 = b.y0 / kGradTileY, tz0 = b.z0 / kGradTileZ;
		const uint64_t tx = (b.x0 + b.width + kGradTileX - 1) / kGradTileX - tx0, ty = (b.y0 + b.height + kGradTileY - 1) / kGradTileY - ty0,
		               tz1 = (b.z0 + b.depth + kGradTileZ - 1) / kGradTileZ, tz = tz1 - tz0;
		// kGradSegment tiles per workgroup, fewer when the volume would not give every CU its eight workgroups otherwise
		const uint64_t want = (uint64_t) 8 * (uint64_t) std::max(1, ctx->cu_count);
		uint32_t       seg  = (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(kGradSegment, tx * ty * tz / want));
		if (const uint32_t forced = tuning_of(ctx).gradient_segment)        // VkvTuning: lets a test march a small volume
			seg = std::min(forced, 255u);
		const uint64_t n_wgs = tx * ty * ((tz + seg - 1) / seg);
		if (n_wgs <= 0x7fffffffull)
		{
			if ((e.width & 3u) == 0 && (((uintptr_t) d_vol) & 3u) == 0)
				hipLaunchKernelGGL(k_gradient_map_tiled<true>, dim3((uint32_t) n_wgs), dim3(256), 0, s, d_vol, d_grad, (int) e.width, (int) e.height, (int) e.depth,
				                   tf->grad_magnitude_modifier, (uint32_t) tx, (uint32_t) ty, (uint32_t) tz1, seg, (uint32_t) n_wgs, tx0, ty0, tz0);
			else
				hipLaunchKernelGGL(k_gradient_map_tiled<false>, dim3((uint32_t) n_wgs), dim3(256), 0, s, d_vol, d_grad, (int) e.width, (int) e.height, (int) e.depth,
				                   tf->grad_magnitude_modifier, (uint32_t) tx, (uint32_t) ty, (uint32_t) tz1, seg, (uint32_t) n_wgs, tx0, ty0, tz0);
			return check_launch(ctx, "gradient_map");
		}
	}
	hipLaunchKernelGGL(k_gradient_map, dim3(blocks_x * ((b.height + 3) / 4), b.depth), dim3(256), 0, s, d_vol, d_grad, (int) e.width, (int) e.height,
	                   (int) e.depth, (int) (tf->use_gradient != 0), tf->grad_magnitude_modifier, blocks_x, (int) b.x0, (int) b.y0, (int) b.z0,
	                   (int) (b.x0 + b.width), (int) (b.y0 + b.height));
	return check_launch(ctx, "gradient_map");
}

int launch_gradient_map(vkv_ctx *ctx, const uint8_t *d_vol, uint8_t *d_grad, VkvExtent3D e, const VkvTransferFunctionUniform *tf, hipStream_t s)
{
	return launch_gradient_map_box(ctx, d_vol, d_grad, e, VkvBox{0, 0, 0, e.width, e.height, e.depth}, tf, s);
}

int launch_check_numerics(vkv_ctx *ctx, int what, uint32_t first_bits, uint64_t count, unsigned long long *d_mismatches, hipStream_t s)
{
	if (count == 0)
		return VKV_OK;
	if ((count + 255) / 256 > 0x7fffffffull || what < 0 || what > 4)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "check_numerics: bad arguments");
	hipLaunchKernelGGL(k_check_numerics, dim3((uint32_t) ((count + 255) / 256)), dim3(256), 0, s, what, first_bits, count, d_mismatches);
	return check_launch(ctx, "check_numerics");
}

}        // namespace vkv

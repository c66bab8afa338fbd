// pack.hip — the packed sampling image (vkv_pack_volume, and the bricks a region update touches): every 4^3 brick of the volume with its
// one-texel apron as 5^3 (intensity, gradient) texel pairs in 256 bytes, so that a trilinear footprint is a few dword loads of one brick
// (layout: vkv_device.hpp).  Byte streaming; no MFMA.
//
// k_pack_volume_tiled<BY, BZ, PITCH, ALIGNED> takes every volume of width >= 4 (gradient-off volumes too: grad null packs zero gradient
// bytes).  k_pack_volume, one 128-thread half-block per brick and a thread per texel, takes widths below 4 and brick grids too large for the
// tiled kernel's launch.
#include <algorithm>

#include "launchers.hpp"

using namespace vkv;

__global__ void __launch_bounds__(256) k_pack_volume(const uint8_t *__restrict__ vol, const uint8_t *__restrict__ grad, uint8_t *__restrict__ packed,
                                                     int W, int H, int D, PackedDims pd, int ox, int oy, int oz, int nbx, int nby, int nbz)
{
	// a workgroup packs 2 bricks that are neighbours in x; consecutive workgroups walk a 4 x 4 x 4 group of brick pairs
	// (8 x 4 x 4 bricks = 32 x 16 x 16 voxels) before moving on, so the overlapping 5^3 neighbourhoods are re-read from L1 / L2
	// and not from HBM (the first version walked whole brick rows and fetched every byte ~5x).  The launch packs the nbx x nby x nbz
	// bricks from brick (ox, oy, oz): all of them, or a region update's
	const uint32_t gx = (uint32_t) (nbx + 7) / 8, gy = (uint32_t) (nby + 3) / 4;        // groups per axis
	// workgroup ids are dealt round-robin to the 8 XCDs: XCD (id & 7) takes groups id&7, id&7 + 8, ... so a group stays in one L2;
	// grid.y = group layer in z (keeps grid.x * 256 below 2^32 for 2048^3)
	const uint32_t grp = ((blockIdx.x >> 3) >> 6) * 8u + (blockIdx.x & 7u), in = (blockIdx.x >> 3) & 63u;
	const int      lbx = (int) ((grp % gx) * 8 + (in & 3u) * 2 + (threadIdx.x >> 7));
	const int      lby = (int) ((grp / gx) * 4 + ((in >> 2) & 3u));
	const int      lbz = (int) (blockIdx.y * 4 + (in >> 4));
	const int      t  = threadIdx.x & 127;
	if (lbx >= nbx || lby >= nby || lbz >= nbz || grp >= gx * gy)
		return;
	const int bx = ox + lbx, by = oy + lby, bz = oz + lbz;
	uint16_t *dst = reinterpret_cast<uint16_t *>(packed + packed_brick_offset(bx, by, bz, pd.mx, pd.my));
	if (t >= 125)
	{
		dst[t] = 0;        // the 6 padding bytes
		return;
	}
	const int lx = t % 5, ly = (t / 5) % 5, lz = t / 25;
	const int x = min(max(bx * 4 + lx - 1, 0), W - 1), y = min(max(by * 4 + ly - 1, 0), H - 1), z = min(max(bz * 4 + lz - 1, 0), D - 1);
	const size_t   o = vidx(x, y, z, W, H);
	const uint32_t v = vol[o], g = grad ? grad[o] : 0u;
	dst[t] = (uint16_t) (v | (g << 8));
}

// LDS-staged version for dword-aligned rows (W % 4 == 0): a workgroup packs 8 x BY x BZ bricks from a 33 x (4 BY + 1) x (4 BZ + 1) texel
// tile that it stages with coalesced dword loads (volume and gradient once each), then writes the bricks as whole 256-byte lines.
// 8 x 4 x 4 (the launcher's choice for volumes of at least 16 bricks in y and z): every lane has 2 x 11 dwords in flight before the
// barrier (8 x 2 x 2: 2 x 3 - not enough outstanding bytes per CU to cover the HBM latency) and the apron re-read drops from 1.42 to 1.27.
template <int BY, int BZ, int PITCH, bool ALIGNED>        // ALIGNED: W % 4 == 0 and dword-aligned buffers (plain dword loads); else row_dword
__global__ void __launch_bounds__(256) k_pack_volume_tiled(const uint8_t *__restrict__ vol, const uint8_t *__restrict__ grad, uint8_t *__restrict__ packed,
                                                           int W, int H, int D, PackedDims pd, uint32_t groups_x, uint32_t gx0, uint32_t gy0, uint32_t gz0)
{
	// the grid covers groups_x x (grid.x / groups_x) x grid.y groups of 8 x BY x BZ bricks from group (gx0, gy0, gz0): all of them, or the
	// groups a region update touches (whole groups are re-packed; the bricks outside its footprint come out as they were)
	// tile: rows (jz, jy) of (v | g << 8) texels; staged dword column c (voxels 4 * (bx0 - 1 + c) ..) sits at texels 4c .. 4c + 3, so the
	// padded tile column jx (voxel x = 4 * bx0 - 1 + jx) is texel jx + 3; 36 texels staged, 33 used
	constexpr int kTX = PITCH, kRY = 4 * BY + 1, kRZ = 4 * BZ + 1, kRows = kRY * kRZ;
	__shared__ __align__(8) uint16_t s_tile[kRows * kTX];
	// x-neighbouring workgroups stage parts of the same 128-byte lines: consecutive groups go to one XCD (own L2)
	const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
	const int      bx0 = (int) (gx0 + bid % groups_x) * 8, by0 = (int) (gy0 + bid / groups_x) * BY, bz0 = (int) (gz0 + blockIdx.y) * BZ;
	const int wd  = (W + 3) >> 2;        // dword columns of a row; the last one partial when W % 4 != 0 (its texels x >= W are fixed up below)
	// ---- stage: row = (jz, jy) of the padded tile, 9 dwords per row starting one dword left of the tile; a lane's (row, column) advance by
	// constants from one of its loads to the next (256 = 28 * 9 + 4), so the divisions are done once
	{
		constexpr int kIter = (kRows * 9 + 255) / 256;        // all loads of a lane are in flight before its first LDS store
		uint32_t      v4[kIter], g4[kIter];
		const int     row0 = (int) threadIdx.x / 9, c0 = (int) threadIdx.x - row0 * 9;
		int           row = row0, c = c0;
#pragma unroll
		for (int j = 0; j < kIter; ++j)
		{
			const int r  = min(row, kRows - 1);
			const int ry = r % kRY, rz = r / kRY;
			const int y = min(max(by0 * 4 + ry - 1, 0), H - 1), z = min(max(bz0 * 4 + rz - 1, 0), D - 1);
			const int dc = min(max(bx0 - 1 + c, 0), wd - 1);
			const size_t o = ((size_t) z * H + y) * (size_t) W;
			v4[j]          = ALIGNED ? reinterpret_cast<const uint32_t *>(vol + o)[dc] : row_dword(vol + o, dc, W);
			g4[j]          = grad ? (ALIGNED ? reinterpret_cast<const uint32_t *>(grad + o)[dc] : row_dword(grad + o, dc, W)) : 0u;
			row += 28, c += 4;
			if (c >= 9)
				c -= 9, ++row;
		}
		row = row0, c = c0;
#pragma unroll
		for (int j = 0; j < kIter; ++j)
		{
			if (row < kRows)
			{
				// bytes (v0 v1 v2 v3), (g0 g1 g2 g3) -> texel pairs (v0 g0 v1 g1), (v2 g2 v3 g3): one byte permute each, one 8-byte LDS store
				const uint32_t lo = __builtin_amdgcn_perm(g4[j], v4[j], 0x05010400u), hi = __builtin_amdgcn_perm(g4[j], v4[j], 0x07030602u);
				if (kTX % 4 == 0)
					*reinterpret_cast<uint2 *>(&s_tile[row * kTX + 4 * c]) = make_uint2(lo, hi);
				else
				{
					*reinterpret_cast<uint32_t *>(&s_tile[row * kTX + 4 * c])     = lo;
					*reinterpret_cast<uint32_t *>(&s_tile[row * kTX + 4 * c + 2]) = hi;
				}
			}
			row += 28, c += 4;
			if (c >= 9)
				c -= 9, ++row;
		}
	}
	__syncthreads();
	// ---- clamp-to-edge in x (dword columns were clamped as a whole): x = -1 -> voxel 0, x >= W -> voxel W - 1
	if (bx0 == 0 || bx0 * 4 + 31 >= W)
	{
		for (int it = threadIdx.x; it < kRows * 33; it += 256)
		{
			const int row = it / 33, jx = it - row * 33;
			const int x = bx0 * 4 + jx - 1;
			if (x < 0)
				s_tile[row * kTX + jx + 3] = s_tile[row * kTX + 3 + 1 - bx0 * 4];
			else if (x >= W)
				s_tile[row * kTX + jx + 3] = s_tile[row * kTX + 3 + W - bx0 * 4];
		}
		__syncthreads();
	}
	// ---- write: 8 BY BZ bricks x 16 pieces of 16 bytes (a store instruction costs the same per lane whatever its width).  A lane keeps its
	// piece q of every brick it writes (bricks b, b + 16, ...), so the positions of its eight texels inside a brick's 5^3 block are computed once
	const int q = (int) threadIdx.x & 15;
	int       off[8];
#pragma unroll
	for (int k = 0; k < 8; ++k)
	{
		const int t = 8 * q + k;        // texel of the 5^3 brick, x fastest; 125..127 are padding
		const int lx = t % 5, ly = (t / 5) % 5, lz = t / 25;
		off[k]       = t < 125 ? (lz * kRY + ly) * kTX + lx + 3 : -1;
	}
#pragma unroll
	for (int j = 0; j < (8 * BY * BZ) / 16; ++j)
	{
		const int b  = ((int) threadIdx.x >> 4) + 16 * j;
		const int lbx = b & 7, lby = (b >> 3) % BY, lbz = (b >> 3) / BY;
		const int bx = bx0 + lbx, by = by0 + lby, bz = bz0 + lbz;
		if (bx >= pd.bx || by >= pd.by || bz >= pd.bz)
			continue;
		const int base = ((lbz * 4) * kRY + lby * 4) * kTX + lbx * 4;
		uint32_t  w[4] = {0, 0, 0, 0};
#pragma unroll
		for (int k = 0; k < 8; ++k)
			if (off[k] >= 0)
				w[k >> 1] |= (uint32_t) s_tile[base + off[k]] << (16 * (k & 1));
		// non-temporal: 3.6 GB that nobody reads before the kernel is over (1.31 -> 1.23 ms; non-temporal LOADS of the volume cost the apron's
		// L2 hits: 1.6 ms)
		typedef uint32_t v4u __attribute__((ext_vector_type(4)));
		v4u              val = {w[0], w[1], w[2], w[3]};
		__builtin_nontemporal_store(val, reinterpret_cast<v4u *>(packed + packed_brick_offset(bx, by, bz, pd.mx, pd.my)) + q);
	}
}

namespace vkv
{

// the bricks [b0, b1) per axis (packed_dims' brick grid); launch_pack_volume: all of them
int launch_pack_volume_bricks(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, const int b0[3], const int b1[3], void *d_packed,
                              hipStream_t s)
{
	const PackedDims pd = packed_dims((int) e.width, (int) e.height, (int) e.depth);
	if (e.width >= 4)        // round 6: any width and alignment (row_dword: the staging loads need none, an odd row's last column is shifted in)
	{
		const bool     big = pd.by >= 16 && pd.bz >= 16;
		const uint32_t t   = big ? 4u : 2u;
		const uint32_t gx0 = (uint32_t) b0[0] / 8, gy0 = (uint32_t) b0[1] / t, gz0 = (uint32_t) b0[2] / t;        // groups of 8 x t x t bricks touched
		const uint32_t gx = ((uint32_t) b1[0] + 7) / 8 - gx0, gy = ((uint32_t) b1[1] + t - 1) / t - gy0, gz = ((uint32_t) b1[2] + t - 1) / t - gz0;
		if ((uint64_t) gx * gy <= 0xffffffull && gz <= 65535u && (uint64_t) pd.mx * pd.my * pd.mz * 512 <= 0xffffffffull)
		{
			// row pitch 40 texels; 38 (19 banks, odd: no bank conflicts, 70 % of the LDS cycles otherwise) measured the same 1.34 ms: the
			// kernel follows its 5.3 GB of traffic, not the LDS or the VALU (50 % busy)
			const bool aligned = (e.width & 3u) == 0 && ((((uintptr_t) d_vol) | ((uintptr_t) d_grad)) & 3u) == 0;
#define VKV_PACK(T, A)                                                                                                                              \
	hipLaunchKernelGGL((k_pack_volume_tiled<T, T, 40, A>), dim3(gx * gy, gz), dim3(256), 0, s, d_vol, d_grad, (uint8_t *) d_packed, (int) e.width,     \
	                   (int) e.height, (int) e.depth, pd, gx, gx0, gy0, gz0)
			if (big)
			{
				if (aligned) VKV_PACK(4, true); else VKV_PACK(4, false);
			}
			else
			{
				if (aligned) VKV_PACK(2, true); else VKV_PACK(2, false);
			}
#undef VKV_PACK
			return check_launch(ctx, "pack_volume");
		}
	}
	const uint64_t   nb = (uint64_t) pd.bx * pd.by;        // bricks per z layer
	if (nb > 0xffffffull || pd.bz > 65535 || (uint64_t) pd.mx * pd.my * pd.mz * 512 > 0xffffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "pack_volume: volume too large");
	// macro-brick padding (bricks that exist only because of the 8x8x8 grouping) is never addressed by the sampler
	const int      nbx = b1[0] - b0[0], nby = b1[1] - b0[1], nbz = b1[2] - b0[2];
	const uint64_t groups = (uint64_t) ((nbx + 7) / 8) * ((nby + 3) / 4);        // per layer of 4 bricks in z
	if ((groups + 8) * 64 * 256 > 0xffffffffull || (nbz + 3) / 4 > 65535)
		return set_error(ctx, VKV_E_UNSUPPORTED, "pack_volume: volume too large");
	hipLaunchKernelGGL(k_pack_volume, dim3((uint32_t) (((groups + 7) / 8) * 8 * 64), (uint32_t) ((nbz + 3) / 4)), dim3(256), 0, s, d_vol, d_grad, (uint8_t *) d_packed, (int) e.width, (int) e.height,
	                   (int) e.depth, pd, b0[0], b0[1], b0[2], nbx, nby, nbz);
	return check_launch(ctx, "pack_volume");
}

int launch_pack_volume(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, void *d_packed, hipStream_t s)
{
	const PackedDims pd = packed_dims((int) e.width, (int) e.height, (int) e.depth);
	const int        b0[3] = {0, 0, 0}, b1[3] = {pd.bx, pd.by, pd.bz};
	return launch_pack_volume_bricks(ctx, d_vol, d_grad, e, b0, b1, d_packed, s);
}

}        // namespace vkv

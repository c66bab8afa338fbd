// box_domain.hpp — what every operation on a box of voxels shares (mesh.hip, mesh_indexed.hip, components.hip, edt.hip, and capi.hip for the
// host parts): the box a call means and the check of it, the max map as the kernels see it, and the BOX-LINEAR domain: kernels that are
// one-dimensional over i = ((z - z0) bh + (y - y0)) bw + (x - x0), one voxel per lane, a wave's 64 voxels one ENTRY (the tile: 64 x 1 x 1,
// wrapping over rows where the box is narrower).  The inside rule of all of them is iso_threshold() of ../host/host_arith.hpp.
#pragma once

#include <type_traits>

#include "launchers.hpp"

namespace vkv
{

// ---- host side: the box of a call
inline VkvBox whole_or(VkvExtent3D e, const VkvBox *box) { return box ? *box : VkvBox{0, 0, 0, e.width, e.height, e.depth}; }

// a valid extent and null (the whole volume) or a non-empty box inside it: what check_box() and the scratch-size functions accept
inline bool extent_and_box_ok(VkvExtent3D e, const VkvBox *box)
{
	if (!extent_ok(e))
		return false;
	return !(box && (box->width == 0 || box->height == 0 || box->depth == 0 || (uint64_t) box->x0 + box->width > e.width ||
	                 (uint64_t) box->y0 + box->height > e.height || (uint64_t) box->z0 + box->depth > e.depth));
}

// launch(std::true_type / std::false_type): a kernel's WIDE or narrow instance
template <typename Launch>
inline void dispatch_wide(bool wide, Launch launch)
{
	if (wide)
		launch(std::true_type{});
	else
		launch(std::false_type{});
}

// ---- the max map (vkv_max_map) of the volume, or none
struct MaxMap
{
	const uint8_t *map = nullptr;        // null: none
	int            bx = 1, by = 1, bz = 1, mw = 0, mh = 0;        // voxels per cell and the map's row and slice

	MaxMap() = default;
	MaxMap(const uint8_t *d_max_map, VkvExtent3D e, VkvExtent3D me) : map(d_max_map)        // me is read with a map only
	{
		if (d_max_map)
		{
			bx = (int) block_of(e.width, me.width), by = (int) block_of(e.height, me.height), bz = (int) block_of(e.depth, me.depth);
			mw = (int) me.width, mh = (int) me.height;
		}
	}

	// the index of the cell that holds the volume's voxel (x, y, z), and of the cell (cx, cy, cz), which is passed slowest first; T: the caller's coordinate type, int or uint32_t
	template <typename T>
	__device__ __forceinline__ size_t cell_of(T x, T y, T z) const
	{
		return cell(z / (T) bz, y / (T) by, x / (T) bx);
	}
	template <typename T>
	__device__ __forceinline__ size_t cell(T cz, T cy, T cx) const
	{
		return ((size_t) cz * (size_t) (T) mh + (size_t) cy) * (size_t) (T) mw + (size_t) cx;
	}
};

// ---- the box-linear domain
struct BoxLinear
{
	const uint8_t *vol;
	uint32_t       W, H;              // the volume's row and slice
	uint32_t       x0, y0, z0;        // the box's first voxel
	uint32_t       bw, bh, bd, n;        // the box's shape and its voxels
	uint32_t       thr;               // the smallest inside byte (iso_threshold); 256: none
};

struct BoxVoxel
{
	uint32_t i, lane, x, y, z;        // the box-linear index, the lane, the position in the box
	bool     valid;
};

__device__ __forceinline__ BoxVoxel box_voxel(const BoxLinear &G)
{
	BoxVoxel v;
	v.i     = blockIdx.x * 256u + threadIdx.x;        // at most 2^32 - 1: the grid has at most 2^24 workgroups
	v.lane  = threadIdx.x & 63u;
	v.valid = v.i < G.n;
	const uint32_t t = v.i / G.bw;
	v.x = v.i - t * G.bw, v.y = t % G.bh, v.z = t / G.bh;
	return v;
}

// where the voxel lies in a buffer of the volume's shape
__device__ __forceinline__ size_t box_address(const BoxLinear &G, const BoxVoxel &v)
{
	return ((size_t) (G.z0 + v.z) * (size_t) G.H + (size_t) (G.y0 + v.y)) * (size_t) G.W + (size_t) (G.x0 + v.x);
}

// a select kernel's body: every voxel of the box in dst becomes `fill` where replace(i) holds of its box-linear index, else its byte of src.
// In place works: a lane reads and writes its own byte only
template <typename Replace>
__device__ __forceinline__ void box_select(const BoxLinear &G, const uint8_t *src, uint8_t *dst, uint32_t fill, Replace replace)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)
		return;
	const size_t  a = box_address(G, v);
	const uint8_t b = src[a];
	dst[a]          = replace(v.i) ? (uint8_t) fill : b;
}

// ---- host side: what a box-linear call is dealt into
struct BoxLinearPlan
{
	uint32_t n, entries, wgs;        // voxels, entries of 64, workgroups of 256
};

// false: the extent or box is not accepted, or the box holds more than 2^32 - 1 voxels
inline bool box_linear_plan(VkvExtent3D e, const VkvBox *box, BoxLinearPlan &p)
{
	if (!extent_and_box_ok(e, box))
		return false;
	const VkvBox b = whole_or(e, box);
	if ((uint64_t) b.width * b.height > 0xffffffffull || (uint64_t) b.width * b.height * b.depth > 0xffffffffull)
		return false;
	p.n       = b.width * b.height * b.depth;
	p.entries = p.n / 64u + (p.n % 64u != 0u);        // n + 63 may wrap
	p.wgs     = (p.entries + 3u) / 4u;
	return true;
}

inline BoxLinear box_linear(const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, const BoxLinearPlan &p, float iso)
{
	BoxLinear G{};
	G.vol = d_vol, G.W = e.width, G.H = e.height, G.x0 = b.x0, G.y0 = b.y0, G.z0 = b.z0, G.bw = b.width, G.bh = b.height, G.bd = b.depth, G.n = p.n;
	G.thr = iso_threshold(iso);
	return G;
}

}        // namespace vkv

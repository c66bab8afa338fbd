// filter.hip — 3x3x3 filters of the uint8 volume (vkv_filter_volume): the binomial (1, 2, 1)^3 smoothing with one rounding
// and the median, both over the clamp-to-edge neighbourhood the samplers use.  Byte streaming; no MFMA.
//
// k_filter3<KIND, WIDE> takes every extent, alignment and box (WIDE: widths of at least 4, one dword load per row; narrower rows gather
// bytes).  A lane owns four x-adjacent voxels of one row and marches along z; a wave is 256 voxels of one row.  Per slice a lane loads the
// dword of its four voxels in its three rows, takes the columns x - 1 and x + 4 from its neighbour lanes, reduces the six columns over y
// and keeps that reduction for the three outputs that see the slice.  Clamp-to-edge is resolved by the loads, so the arithmetic has no
// bounds tests.  Everything is held two voxels per dword in 16-bit fields; nothing goes through LDS (the reuse across rows y +- 1 is the
// vector L1's) and nothing spills.
#include <algorithm>

#include "launchers.hpp"
#include "median27_network.hpp"

using namespace vkv;

constexpr int kFilterTileX = 256, kFilterTileY = 4;        // voxels of a workgroup per slice: 64 lanes x 4 voxels, 4 rows
constexpr int kFilterSegment = 18;                          // slices a workgroup marches over (it loads two more)
constexpr int kFilterAhead = 3;                             // slices whose loads are in flight during the arithmetic; a multiple of 3
static_assert(kFilterAhead % 3 == 0 && kFilterSegment % kFilterAhead == 0, "the march is unrolled over the loads in flight and the three reductions");

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

struct PackedU16Ops        // v_pk_min_u16 / v_pk_max_u16
{
	__device__ __forceinline__ u16x2 lo(u16x2 a, u16x2 b) const { return __builtin_elementwise_min(a, b); }
	__device__ __forceinline__ u16x2 hi(u16x2 a, u16x2 b) const { return __builtin_elementwise_max(a, b); }
};

// What a lane holds of one row: `d`, the voxels clamp(x .. x + 3, 0, W - 1) as one dword, and in the first and last lane of a wave `e`, the
// voxel clamp(x - 1) or clamp(x + 4) that no neighbouring lane holds.  WIDE (W >= 4): ONE dword load at min(x, W - 4), at any alignment; a
// lane whose dword would leave the row (over = x + 4 - W > 0 voxels) shifts the row's last dword down at consumption and repeats voxel
// W - 1.  Narrower rows gather their four bytes (over = 0).  Nothing outside the row is read.
struct RowBytes
{
	uint32_t d, e;
};

template <bool WIDE>
__device__ __forceinline__ RowBytes row_load(const uint8_t *row, int x, int W, uint32_t lane)
{
	RowBytes r;
	r.e = 0;
	if (lane == 0 || lane == 63)
		r.e = row[lane == 0 ? min(max(x - 1, 0), W - 1) : min(x + 4, W - 1)];
	if (WIDE)
		r.d = load_u32_any(row + min(x, W - 4));
	else
	{
		r.d = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			r.d |= (uint32_t) row[min(x + i, W - 1)] << (8 * i);
	}
	return r;
}

// the six columns x - 1 .. x + 4 as three dwords of two 16-bit fields: (x - 1, x), (x + 1, x + 2), (x + 3, x + 4).  Voxel x - 1 is the
// last byte of the lane below, voxel x + 4 the first of the lane above (v_mov_b32 wave_shr:1 / wave_shl:1; every lane of the wave takes
// part: lanes past the box or the row hold clamped voxels and only skip their store)
__device__ __forceinline__ void column_pairs(RowBytes r, int over, uint32_t lane, uint32_t (&p)[3])
{
	uint32_t d = r.d;
	if (over > 0)
	{
		const uint32_t last = (d >> 24) * 0x01010101u;
		d = over >= 4 ? last : (d >> (8 * over)) | (last << (8 * (4 - over)));
	}
	uint32_t below = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) d, 0x138, 0xf, 0xf, false);        // wave_shr:1
	uint32_t above = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) d, 0x130, 0xf, 0xf, false);        // wave_shl:1
	below = lane == 0 ? r.e << 24 : below;
	above = lane == 63 ? r.e : above;
	p[0] = __builtin_amdgcn_perm(below, d, 0x0c000c07u);
	p[1] = __builtin_amdgcn_perm(0u, d, 0x0c020c01u);
	p[2] = __builtin_amdgcn_perm(above, d, 0x0c040c03u);
}

// fields (lo.hi, hi.lo): the pair of columns between two neighbouring pairs
__device__ __forceinline__ uint32_t between(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_alignbit(hi, lo, 16); }

// what a lane keeps of one slice: the y reduction of its six columns
template <int KIND>
struct FilterSlice;
template <>
struct FilterSlice<VKV_FILTER_BINOMIAL3>
{
	uint32_t c[3];        // r(y - 1) + 2 r(y) + r(y + 1) per column, <= 1020
};
template <>
struct FilterSlice<VKV_FILTER_MEDIAN3>
{
	u16x2 t[3][3];        // the three y neighbours of every column, ascending
};

__device__ __forceinline__ void reduce_y(const uint32_t (&m)[3], const uint32_t (&o)[3], const uint32_t (&p)[3], FilterSlice<VKV_FILTER_BINOMIAL3> &s)
{
#pragma unroll
	for (int j = 0; j < 3; ++j)
		s.c[j] = m[j] + 2u * o[j] + p[j];
}

__device__ __forceinline__ void reduce_y(const uint32_t (&m)[3], const uint32_t (&o)[3], const uint32_t (&p)[3], FilterSlice<VKV_FILTER_MEDIAN3> &s)
{
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
		s.t[j][0] = __builtin_bit_cast(u16x2, m[j]), s.t[j][1] = __builtin_bit_cast(u16x2, o[j]), s.t[j][2] = __builtin_bit_cast(u16x2, p[j]);
		sort3(s.t[j][0], s.t[j][1], s.t[j][2], PackedU16Ops());
	}
}

// bytes 0 and 2 of a and of b: four 16-bit fields (values <= 255) as four voxels
__device__ __forceinline__ uint32_t low_bytes(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x06040200u); }

// the four voxels x .. x + 3 of slice z from the reductions of slices z - 1, z, z + 1
__device__ __forceinline__ uint32_t finish(const FilterSlice<VKV_FILTER_BINOMIAL3> &a, const FilterSlice<VKV_FILTER_BINOMIAL3> &b,
                                           const FilterSlice<VKV_FILTER_BINOMIAL3> &c)
{
	uint32_t q[3];        // the y-z sums, <= 4080
#pragma unroll
	for (int j = 0; j < 3; ++j)
		q[j] = a.c[j] + 2u * b.c[j] + c.c[j];
	// S <= 16320, S + 32 < 2^16: the fields never carry into each other; one rounding
	const uint32_t s01 = q[0] + 2u * between(q[0], q[1]) + q[1] + 0x00200020u;
	const uint32_t s23 = q[1] + 2u * between(q[1], q[2]) + q[2] + 0x00200020u;
	return low_bytes(s01 >> 6, s23 >> 6);        // byte 0 / 2 of (s >> 6): bits 6 .. 13 of each field
}

__device__ __forceinline__ uint32_t finish(const FilterSlice<VKV_FILTER_MEDIAN3> &a, const FilterSlice<VKV_FILTER_MEDIAN3> &b,
                                           const FilterSlice<VKV_FILTER_MEDIAN3> &c)
{
	const PackedU16Ops op;
	u16x2              s[3][9];        // the sorted y-z plane of every column
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
#pragma unroll
		for (int i = 0; i < 3; ++i)
			s[j][i] = a.t[j][i], s[j][3 + i] = b.t[j][i], s[j][6 + i] = c.t[j][i];
		merge_triples(s[j], op);
	}
	u16x2 m01[9], m12[9];        // columns (x, x + 1) and (x + 2, x + 3)
#pragma unroll
	for (int i = 0; i < 9; ++i)
	{
		m01[i] = __builtin_bit_cast(u16x2, between(__builtin_bit_cast(uint32_t, s[0][i]), __builtin_bit_cast(uint32_t, s[1][i])));
		m12[i] = __builtin_bit_cast(u16x2, between(__builtin_bit_cast(uint32_t, s[1][i]), __builtin_bit_cast(uint32_t, s[2][i])));
	}
	// voxels (x, x + 1) see the columns (x - 1, x), (x, x + 1), (x + 1, x + 2); voxels (x + 2, x + 3) the next three pairs
	const u16x2 o01 = median_of_sorted(s[0], m01, s[1], op), o23 = median_of_sorted(s[1], m12, s[2], op);
	return low_bytes(__builtin_bit_cast(uint32_t, o01), __builtin_bit_cast(uint32_t, o23));
}

// The launch covers the box [x0, x1) x [y0, y1) x [z0, z1) in tiles of kFilterTileX x kFilterTileY voxels and kFilterSegment slices.
template <int KIND, bool WIDE>
__global__ void __launch_bounds__(256) k_filter3(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int W, int H, int D, int x0, int y0, int z0,
                                                 int x1, int y1, int z1, uint32_t tiles_x, uint32_t tiles_y, uint32_t n_wgs)
{
	const uint32_t t = xcd_remap(blockIdx.x, n_wgs), lane = threadIdx.x & 63u;
	const int      xw = x0 + (int) (t % tiles_x) * kFilterTileX, x = xw + 4 * (int) lane;        // a wave is 256 voxels of one row
	const int      y = y0 + (int) ((t / tiles_x) % tiles_y) * kFilterTileY + (int) (threadIdx.x >> 6);
	const int      zs = z0 + (int) (t / (tiles_x * tiles_y)) * kFilterSegment, ze = min(zs + kFilterSegment, z1);
	if (xw >= x1 || y >= y1)        // whole waves only: the lanes exchange columns below (and there is no barrier anywhere)
		return;
	const size_t plane = (size_t) H * (size_t) W;
	const size_t rm = (size_t) max(y - 1, 0) * (size_t) W, ro = (size_t) y * (size_t) W, rp = (size_t) min(y + 1, H - 1) * (size_t) W;
	const int    over = WIDE ? x + 4 - W : 0;
	struct Rows
	{
		RowBytes m, o, p;
	};
	auto load = [&](int z) {
		const uint8_t *base = src + (size_t) min(max(z, 0), D - 1) * plane;
		return Rows{row_load<WIDE>(base + rm, x, W, lane), row_load<WIDE>(base + ro, x, W, lane), row_load<WIDE>(base + rp, x, W, lane)};
	};
	auto reduce = [&](const Rows &r) {
		uint32_t m[3], o[3], p[3];
		column_pairs(r.m, over, lane, m), column_pairs(r.o, over, lane, o), column_pairs(r.p, over, lane, p);
		FilterSlice<KIND> s;
		reduce_y(m, o, p, s);
		return s;
	};
	// kFilterAhead slices of loads are in flight during the arithmetic (a wave's step is far shorter than the memory latency); the loop is
	// unrolled over them and over the three reductions a, b, c, so that neither ring is ever copied
	const Rows r0 = load(zs - 1), r1 = load(zs);
	Rows       ring[kFilterAhead];
#pragma unroll
	for (int k = 0; k < kFilterAhead; ++k)
		ring[k] = load(zs + 1 + k);
	FilterSlice<KIND> red[3];
	red[0] = reduce(r0), red[1] = reduce(r1);
	uint8_t * out = dst + (size_t) zs * plane + ro + (size_t) x;
	const int n   = min(4, x1 - x);        // voxels of this lane inside the box: the last lane of a row may hold 1 .. 3, lanes past it none
	for (int zb = zs; zb < ze; zb += kFilterAhead)
	{
#pragma unroll
		for (int k = 0; k < kFilterAhead; ++k)
		{
			const int z = zb + k;
			if (z >= ze)        // wave-uniform
				break;
			red[(k + 2) % 3] = reduce(ring[k]);        // slice z + 1
			if (z + 1 + kFilterAhead <= ze)
				ring[k] = load(z + 1 + kFilterAhead);
			const uint32_t v = finish(red[k % 3], red[(k + 1) % 3], red[(k + 2) % 3]);
			if (n == 4)
				*reinterpret_cast<u32_any_align *>(out) = v;        // one dword at whatever alignment the row has
			else
				for (int i = 0; i < n; ++i)
					out[i] = (uint8_t) (v >> (8 * i));
			out += plane;
		}
	}
}

namespace vkv
{

bool filter_launch_ok(VkvExtent3D e)
{
	// int coordinates with room for a lane past the row (x + 4 * 64), and a one-dimensional grid
	const uint64_t tiles = (uint64_t) ((e.width + kFilterTileX - 1) / kFilterTileX) * ((e.height + kFilterTileY - 1) / kFilterTileY);
	if (e.width > 0x7fffff00u || e.height > 0x7fffff00u || e.depth > 0x7fffff00u || tiles > 0x7fffffffull)
		return false;
	return tiles * ((e.depth + kFilterSegment - 1) / kFilterSegment) <= 0x7fffffffull;
}

int launch_filter_volume(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, int kind, hipStream_t s)
{
	if (!filter_launch_ok(e))
		return set_error(ctx, VKV_E_UNSUPPORTED, "filter_volume: volume too large for one launch");
	const uint32_t tx = (b.width + kFilterTileX - 1) / kFilterTileX, ty = (b.height + kFilterTileY - 1) / kFilterTileY,
	               tz = (b.depth + kFilterSegment - 1) / kFilterSegment;
	const uint32_t n  = tx * ty * tz;        // <= the whole volume's tiles: checked above
	const int      x1 = (int) (b.x0 + b.width), y1 = (int) (b.y0 + b.height), z1 = (int) (b.z0 + b.depth);
	const bool     wide = e.width >= 4;        // the kernels' dword row loads
#define VKV_FILTER(K, WIDE_)                                                                                                                  \
	hipLaunchKernelGGL((k_filter3<K, WIDE_>), dim3(n), dim3(256), 0, s, d_src, d_dst, (int) e.width, (int) e.height, (int) e.depth, (int) b.x0, \
	                   (int) b.y0, (int) b.z0, x1, y1, z1, tx, ty, n)
	if (kind == VKV_FILTER_BINOMIAL3)
	{
		if (wide) VKV_FILTER(VKV_FILTER_BINOMIAL3, true); else VKV_FILTER(VKV_FILTER_BINOMIAL3, false);
	}
	else
	{
		if (wide) VKV_FILTER(VKV_FILTER_MEDIAN3, true); else VKV_FILTER(VKV_FILTER_MEDIAN3, false);
	}
#undef VKV_FILTER
	return check_launch(ctx, "filter_volume");
}

}        // namespace vkv

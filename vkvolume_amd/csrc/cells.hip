// cells.hip — per-cell summaries of the volume (vkv_cell_summary) and the occupancy map decided from them (vkv_occupancy_map_from_summary,
// vkv_update_transfer_function_from_summary).  DESIGN.md §5 "Cell summaries" pins the format and the decision rule and says why the rule is exact.
//
// Summary of a cell (16 bytes, cells in map order): i_lo, i_hi, g_lo, g_hi, g_at_i_hi, i_at_g_hi, flags (bit 0: the cell holds a voxel), 0,
// then a uint64 mask with bit (g >> 5) * 8 + (i >> 5) set for every (gradient byte g, intensity byte i) of the cell's voxels.
//
// Build: a workgroup owns up to 256 voxels in x - whole cells - of one cell slice and walks its cell rows; its four waves take every fourth voxel
// row of a cell row.  A lane loads four voxels per row at any alignment and reduces them in registers: the 16-bit keys (i << 8 | g) and
// (g << 8 | i) of two voxels per dword, under packed u16 min / max, give i_lo, i_hi with g_at_i_hi, g_lo, g_hi with i_at_g_hi; the mask bins
// come out of one SWAR expression per dword.  At the end of a cell row every lane merges its four voxels into the cells' LDS words with atomics.
//
// Classify: one lane per cell, one 16-byte load.  The two point tests read the bit table in LDS; the rectangle tests read a table of row-range
// ORs and ANDs (k_tf_ranges, in the stream's scratch block).  A cell the rule cannot decide goes onto the workgroup's LDS list, and the whole
// workgroup then evaluates the listed cells' voxels, one lane per (cell, voxel row, dword) - no lane waits on another lane's cell.
#include <algorithm>

#include "launchers.hpp"
#include "row_loads.hpp"

using namespace vkv;

namespace
{
constexpr int      kClassifyLanes = 256, kCellsPerLane = 4, kCellsPerGroup = kClassifyLanes * kCellsPerLane;
constexpr uint32_t kRangeLevels = 4;        // row ranges of 2, 4, 8 and 16 rows; a query covers up to 32 rows with two lookups

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
	return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

struct SummaryArgs
{
	const uint8_t *vol, *grad;        // grad null: every gradient byte is 255
	uint4 *        out;
	int            W, H, D, mw, mh, bx, by, bz;
	int            cx0, cy0, cz0, ncx, ncy;        // the launch's cells: [cx0, cx0 + ncx) x [cy0, cy0 + ncy) x [cz0, cz0 + gridDim.y)
	int            cpg, cyg;                       // cells in x per workgroup (<= 256), cell rows per workgroup
	uint32_t       groups_x;
};

__global__ void __launch_bounds__(256) k_cell_summary(const SummaryArgs a)
{
	__shared__ uint32_t s_igmin[256], s_gimin[256], s_igmax[256], s_gimax[256], s_mlo[256], s_mhi[256];
	const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)), lane = (int) (threadIdx.x & 63u);
	const int gx = (int) (blockIdx.x % a.groups_x), gy = (int) (blockIdx.x / a.groups_x);
	const int c_first = a.cx0 + gx * a.cpg, n_cells = min(a.cpg, a.cx0 + a.ncx - c_first);
	const int cz = a.cz0 + (int) blockIdx.y, cy_begin = a.cy0 + gy * a.cyg, cy_end = min(cy_begin + a.cyg, a.cy0 + a.ncy);
	const int x_begin = c_first * a.bx, x_end = min((c_first + n_cells) * a.bx, a.W);        // (x_begin >= W: cells past the volume)
	const int nz = min((cz + 1) * a.bz, a.D) - cz * a.bz;
	const size_t zs = (size_t) a.W * (size_t) a.H;
	for (int cy = cy_begin; cy < cy_end; ++cy)
	{
		for (int c = threadIdx.x; c < n_cells; c += 256)
			s_igmin[c] = 0xffffu, s_gimin[c] = 0xffffu, s_igmax[c] = 0u, s_gimax[c] = 0u, s_mlo[c] = 0u, s_mhi[c] = 0u;
		__syncthreads();
		const int ny = min((cy + 1) * a.by, a.H) - cy * a.by, n_rows = (ny > 0 && nz > 0) ? ny * nz : 0;
		if (wave < n_rows)
			for (int xs = x_begin; xs < x_end; xs += 256)        // one chunk unless a cell is wider than 256 voxels
			{
				const int x = xs + 4 * lane;
				if (x >= x_end)
					continue;
				uint32_t igmin0 = ~0u, igmin1 = ~0u, gimin0 = ~0u, gimin1 = ~0u, igmax0 = 0u, igmax1 = 0u, gimax0 = 0u, gimax1 = 0u;
				uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
				constexpr int kB = 4;        // rows per wave per round (a round repeats the last row where the cell row has fewer: min / max / OR are idempotent)
				for (int r0 = wave; r0 < n_rows; r0 += 4 * kB)
				{
					uint32_t v[kB], g[kB];
#pragma unroll
					for (int j = 0; j < kB; ++j)
					{
						const int    r   = min(r0 + 4 * j, n_rows - 1);
						const int    rz  = r / ny, ry = r - rz * ny;
						const size_t row = (size_t) (cz * a.bz + rz) * zs + (size_t) (cy * a.by + ry) * (size_t) a.W;
						v[j]             = load4_clipped(a.vol + row, x, a.W);
						g[j]             = a.grad ? load4_clipped(a.grad + row, x, a.W) : 0xffffffffu;
					}
#pragma unroll
					for (int j = 0; j < kB; ++j)
					{
						// packed keys of voxels (0, 1) and (2, 3): (i << 8 | g) and (g << 8 | i); v_perm bytes 0-3 = g, 4-7 = v
						const uint32_t ig01 = __builtin_amdgcn_perm(v[j], g[j], 0x05010400u), ig23 = __builtin_amdgcn_perm(v[j], g[j], 0x07030602u);
						const uint32_t gi01 = __builtin_amdgcn_perm(v[j], g[j], 0x01050004u), gi23 = __builtin_amdgcn_perm(v[j], g[j], 0x03070206u);
						igmin0 = pk_min_u16(igmin0, ig01), igmin1 = pk_min_u16(igmin1, ig23);
						gimin0 = pk_min_u16(gimin0, gi01), gimin1 = pk_min_u16(gimin1, gi23);
						igmax0 = pk_max_u16(igmax0, ig01), igmax1 = pk_max_u16(igmax1, ig23);
						gimax0 = pk_max_u16(gimax0, gi01), gimax1 = pk_max_u16(gimax1, gi23);
						const uint32_t idx = ((g[j] >> 2) & 0x38383838u) | ((v[j] >> 5) & 0x07070707u);        // per byte: (g >> 5) * 8 + (i >> 5)
						m0 |= 1ull << (idx & 63u), m1 |= 1ull << ((idx >> 8) & 63u), m2 |= 1ull << ((idx >> 16) & 63u), m3 |= 1ull << (idx >> 24);
					}
				}
#pragma unroll
				for (int p = 0; p < 4; ++p)
				{
					if (x + p >= x_end)
						break;
					const int      c  = (x + p) / a.bx - c_first;
					const uint32_t sh = 16u * (uint32_t) (p & 1);
					const uint32_t igmin = ((p < 2 ? igmin0 : igmin1) >> sh) & 0xffffu, gimin = ((p < 2 ? gimin0 : gimin1) >> sh) & 0xffffu;
					const uint32_t igmax = ((p < 2 ? igmax0 : igmax1) >> sh) & 0xffffu, gimax = ((p < 2 ? gimax0 : gimax1) >> sh) & 0xffffu;
					const uint64_t m     = p == 0 ? m0 : p == 1 ? m1 : p == 2 ? m2 : m3;
					atomicMin(&s_igmin[c], igmin), atomicMin(&s_gimin[c], gimin), atomicMax(&s_igmax[c], igmax), atomicMax(&s_gimax[c], gimax);
					atomicOr(&s_mlo[c], (uint32_t) m), atomicOr(&s_mhi[c], (uint32_t) (m >> 32));
				}
			}
		__syncthreads();
		uint4 *out = a.out + ((size_t) cz * (size_t) a.mh + (size_t) cy) * (size_t) a.mw;
		for (int c = threadIdx.x; c < n_cells; c += 256)
		{
			const int cx = c_first + c;
			uint4     w  = make_uint4(0u, 0u, 0u, 0u);
			if (n_rows > 0 && cx * a.bx < a.W)
			{
				const uint32_t igmin = s_igmin[c], gimin = s_gimin[c], igmax = s_igmax[c], gimax = s_gimax[c];
				w.x = (igmin >> 8) | (igmax & 0xff00u) | ((gimin >> 8) << 16) | ((gimax >> 8) << 24);        // i_lo, i_hi, g_lo, g_hi
				w.y = (igmax & 255u) | ((gimax & 255u) << 8) | (1u << 16);                                 // g_at_i_hi, i_at_g_hi, flags
				w.z = s_mlo[c], w.w = s_mhi[c];
			}
			out[cx] = w;
		}
		__syncthreads();        // (the next cell row re-initialises the words)
	}
}

// Row-range ORs and ANDs of the bit table: entry ((k - 1) * 2048 + r * 8 + ib) = (OR, AND) of words r * 8 + ib .. (r + 2^k - 1) * 8 + ib
// (rows past 255 clamped: never queried), k = 1 .. 4.  Thread 0 also clears the unresolved-cell counter of the classify launch behind it.
__global__ void __launch_bounds__(256) k_tf_ranges(const uint32_t *__restrict__ bits, uint2 *__restrict__ ranges, unsigned long long *unresolved)
{
	const uint32_t e = blockIdx.x * 256u + threadIdx.x;        // < 4 * 2048
	if (e == 0u && unresolved)
		*unresolved = 0ull;
	const uint32_t k = e / 2048u + 1u, r = (e % 2048u) >> 3, ib = e & 7u;
	uint32_t       o = 0u, n = ~0u;
	for (uint32_t j = 0; j < (1u << k); ++j)
	{
		const uint32_t w = bits[min(r + j, 255u) * 8u + ib];
		o |= w, n &= w;
	}
	ranges[e] = make_uint2(o, n);
}

struct ClassifyArgs
{
	const uint4 *        summary;
	const uint8_t *      vol, *grad;        // grad used only with use_gradient (else every voxel in gradient row 255)
	const uint32_t *     bits;
	const uint2 *        ranges;
	uint8_t *            map;
	unsigned long long * unresolved;        // optional
	uint64_t             n_cells;
	int                  W, H, D, mw, mh, bx, by, bz, use_gradient;
	int                  nd, upc;        // dwords per voxel row of a cell (ceil(bx / 4)), evaluation units per cell (nd * by * bz)
};

enum : uint32_t { kEmpty = 0u, kOccupied = 1u, kUnresolved = 2u };

__device__ __forceinline__ uint32_t tf_bit(const uint32_t *s_bits, uint32_t g, uint32_t i) { return (s_bits[g * 8u + (i >> 5)] >> (i & 31u)) & 1u; }

// the decision rule of DESIGN.md §5 for one summary
__device__ __forceinline__ uint32_t classify(const uint4 w, const uint32_t *s_bits, const uint2 *__restrict__ ranges, int use_gradient)
{
	if (!((w.y >> 16) & 1u))
		return kEmpty;        // no voxel
	uint32_t ilo = w.x & 255u, ihi = (w.x >> 8) & 255u, glo = (w.x >> 16) & 255u, ghi = w.x >> 24, gai = w.y & 255u, iag = (w.y >> 8) & 255u;
	uint64_t mask = (uint64_t) w.z | ((uint64_t) w.w << 32);
	if (!use_gradient)
	{        // every voxel in gradient row 255: the intensity bins of all gradient bins folded into bin 7
		glo = ghi = gai = 255u, iag = ihi;
		uint64_t f = mask | (mask >> 32);
		f |= f >> 16, f |= f >> 8;
		mask = (f & 255u) << 56;
	}
	if (tf_bit(s_bits, gai, ihi) | tf_bit(s_bits, ghi, iag))
		return kOccupied;        // those voxels exist
	bool any = false;
	while (mask)
	{
		const uint32_t b = (uint32_t) __builtin_ctzll(mask);
		mask &= mask - 1u;
		const uint32_t gb = b >> 3, ib = b & 7u;
		const uint32_t r0 = max(gb * 32u, glo), r1 = min(gb * 32u + 31u, ghi), c0 = max(ib * 32u, ilo), c1 = min(ib * 32u + 31u, ihi);
		const uint32_t cols = (~0u >> (31u - (c1 & 31u))) & (~0u << (c0 & 31u));
		uint32_t       o, n;
		const uint32_t len = r1 - r0 + 1u;
		if (len == 1u)
			o = n = s_bits[r0 * 8u + ib];
		else
		{
			const uint32_t k = min(31u - (uint32_t) __builtin_clz(len), kRangeLevels);
			const uint2    p = ranges[(k - 1u) * 2048u + r0 * 8u + ib], q = ranges[(k - 1u) * 2048u + (r1 + 1u - (1u << k)) * 8u + ib];
			o = p.x | q.x, n = p.y & q.y;
		}
		if ((n & cols) == cols)
			return kOccupied;        // every (g, i) of this rectangle is occupied, and some voxel lies in it
		any |= (o & cols) != 0u;
	}
	return any ? kUnresolved : kEmpty;
}

__global__ void __launch_bounds__(kClassifyLanes) k_occupancy_from_summary(const ClassifyArgs a)
{
	__shared__ uint32_t s_bits[2048];
	__shared__ uint32_t s_cx[kCellsPerGroup], s_cyz[kCellsPerGroup], s_local[kCellsPerGroup];
	__shared__ uint8_t  s_occ[kCellsPerGroup];
	__shared__ uint32_t s_n;
	for (int i = threadIdx.x; i < 2048; i += kClassifyLanes)
		s_bits[i] = a.bits[i];
	if (threadIdx.x == 0)
		s_n = 0u;
	__syncthreads();
	const uint64_t base = (uint64_t) blockIdx.x * kCellsPerGroup;
	uint4          w[kCellsPerLane];
#pragma unroll
	for (int k = 0; k < kCellsPerLane; ++k)
	{
		const uint64_t cell = base + (uint64_t) (k * kClassifyLanes + threadIdx.x);
		w[k]                = cell < a.n_cells ? a.summary[cell] : make_uint4(0u, 0u, 0u, 0u);
	}
#pragma unroll
	for (int k = 0; k < kCellsPerLane; ++k)
	{
		const uint32_t local = (uint32_t) (k * kClassifyLanes + threadIdx.x);
		const uint64_t cell  = base + local;
		if (cell >= a.n_cells)
			continue;
		const uint32_t d = classify(w[k], s_bits, a.ranges, a.use_gradient);
		if (d != kUnresolved)
		{
			a.map[cell] = d == kOccupied ? 0 : 255;        // OCCUPIED = 0, EMPTY = 255
			continue;
		}
		const uint64_t row = cell / (uint64_t) a.mw;
		const uint32_t n   = atomicAdd(&s_n, 1u);
		s_cx[n]    = (uint32_t) (cell - row * (uint64_t) a.mw);
		s_cyz[n]   = (uint32_t) (row % (uint64_t) a.mh) | ((uint32_t) (row / (uint64_t) a.mh) << 16);
		s_local[n] = local;
		s_occ[n]   = 0;
	}
	__syncthreads();
	const uint32_t n_list = s_n;
	if (n_list == 0u)
		return;
	if (threadIdx.x == 0 && a.unresolved)
		atomicAdd(a.unresolved, (unsigned long long) n_list);
	// the listed cells' voxels, as vkv_occupancy_map tests them: unit t = (cell t / upc, voxel row, dword of that row)
	const uint32_t total = n_list * (uint32_t) a.upc;
	const size_t   zs    = (size_t) a.W * (size_t) a.H;
	for (uint32_t t = threadIdx.x; t < total; t += kClassifyLanes)
	{
		const uint32_t k = t / (uint32_t) a.upc, u = t - k * (uint32_t) a.upc;
		const uint32_t r = u / (uint32_t) a.nd, dw = u - r * (uint32_t) a.nd, rz = r / (uint32_t) a.by, ry = r - rz * (uint32_t) a.by;
		const int      cx = (int) s_cx[k], cy = (int) (s_cyz[k] & 0xffffu), cz = (int) (s_cyz[k] >> 16);
		const int      y = cy * a.by + (int) ry, z = cz * a.bz + (int) rz, x = cx * a.bx + 4 * (int) dw, x_end = min(cx * a.bx + a.bx, a.W);
		if (y >= a.H || z >= a.D || x >= x_end)
			continue;
		const size_t   row = (size_t) z * zs + (size_t) y * (size_t) a.W;
		const uint32_t v   = load4_clipped(a.vol + row, x, a.W);
		const uint32_t g   = a.use_gradient ? load4_clipped(a.grad + row, x, a.W) : 0xffffffffu;
		const int      nv  = min(4, x_end - x);
		uint32_t       occ = 0u;
		for (int p = 0; p < nv; ++p)
			occ |= tf_bit(s_bits, (g >> (8 * p)) & 255u, (v >> (8 * p)) & 255u);
		if (occ)
			s_occ[k] = 1;        // benign race: every writer stores 1
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < n_list; k += kClassifyLanes)
		a.map[base + s_local[k]] = s_occ[k] ? 0 : 255;
}

}        // namespace

namespace vkv
{

// what the summary and classify launches can take (checked by the entry points before anything is enqueued)
bool cells_launch_ok(VkvExtent3D e, VkvExtent3D me)
{
	const uint64_t n_cells = (uint64_t) me.width * me.height * me.depth;
	const uint64_t bx = block_of(e.width, me.width), by = block_of(e.height, me.height), bz = block_of(e.depth, me.depth);
	return me.height <= 65535u && me.depth <= 65535u && (n_cells + kCellsPerGroup - 1) / kCellsPerGroup <= 0x7fffffffull &&
	       (bx + 3) / 4 * by * bz * kCellsPerGroup <= 0xffffffffull;        // (the classify kernel's 32-bit evaluation units)
}

// vkv_cell_summary after its argument checks: the cells that meet b (the whole map when b is null)
int launch_cell_summary(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, VkvExtent3D me, const VkvBox *b, void *d_summary,
                        hipStream_t s)
{
	SummaryArgs a;
	a.vol = d_vol, a.grad = d_grad, a.out = reinterpret_cast<uint4 *>(d_summary);
	a.W = (int) e.width, a.H = (int) e.height, a.D = (int) e.depth, a.mw = (int) me.width, a.mh = (int) me.height;
	a.bx = (int) block_of(e.width, me.width), a.by = (int) block_of(e.height, me.height), a.bz = (int) block_of(e.depth, me.depth);
	int ncz;
	if (b)
	{
		a.cx0 = (int) (b->x0 / a.bx), a.cy0 = (int) (b->y0 / a.by), a.cz0 = (int) (b->z0 / a.bz);
		a.ncx = (int) ((b->x0 + b->width - 1) / a.bx) - a.cx0 + 1, a.ncy = (int) ((b->y0 + b->height - 1) / a.by) - a.cy0 + 1;
		ncz   = (int) ((b->z0 + b->depth - 1) / a.bz) - a.cz0 + 1;
	}
	else
		a.cx0 = a.cy0 = a.cz0 = 0, a.ncx = (int) me.width, a.ncy = (int) me.height, ncz = (int) me.depth;
	a.cpg      = std::min(a.ncx, a.bx <= 256 ? 256 / a.bx : 1);
	a.groups_x = (uint32_t) ((a.ncx + a.cpg - 1) / a.cpg);
	// cell rows per workgroup: ~64 KB of voxel bytes behind each cell row's barriers, but at least 16 workgroups per CU in the launch
	const size_t row_bytes = (size_t) std::min(a.cpg * a.bx, 256) * a.by * a.bz * (d_grad ? 2 : 1);
	a.cyg = (int) std::min<size_t>(std::max<size_t>(1, (64 * 1024) / std::max<size_t>(1, row_bytes)), (size_t) a.ncy);
	const uint64_t want = (uint64_t) 16 * (uint64_t) std::max(1, ctx->cu_count);
	while (a.cyg > 1 && (uint64_t) a.groups_x * ((a.ncy + a.cyg - 1) / a.cyg) * ncz < want)
		a.cyg >>= 1;
	const uint64_t groups = (uint64_t) a.groups_x * (uint64_t) ((a.ncy + a.cyg - 1) / a.cyg);
	if (groups > 0x7fffffffull || ncz > 65535)
		return set_error(ctx, VKV_E_UNSUPPORTED, "cell_summary: map too large for one launch");
	hipLaunchKernelGGL(k_cell_summary, dim3((uint32_t) groups, (uint32_t) ncz), dim3(256), 0, s, a);
	return check_launch(ctx, "cell_summary");
}

// the occupancy map from the summary, with the bit table already in the stream's scratch block (the caller holds its lock): the range table
// behind it, then the classification.  use_gradient: tf->use_gradient (d_grad is then non-null: the entry points refuse the on-the-fly gradient)
int launch_occupancy_from_summary(vkv_ctx *ctx, const void *d_summary, const uint8_t *d_vol, const uint8_t *d_grad, bool use_gradient, uint8_t *scratch,
                                  VkvExtent3D e, uint8_t *d_map, VkvExtent3D me, uint64_t *d_unresolved, hipStream_t s)
{
	const uint32_t *d_bits     = reinterpret_cast<const uint32_t *>(scratch + kTfBitsOffset);
	uint2 *         d_ranges   = reinterpret_cast<uint2 *>(scratch + kTfRangesOffset);
	auto *         unresolved = reinterpret_cast<unsigned long long *>(d_unresolved);
	hipLaunchKernelGGL(k_tf_ranges, dim3(kRangeLevels * 2048 / 256), dim3(256), 0, s, d_bits, d_ranges, unresolved);
	ClassifyArgs a;
	a.summary = reinterpret_cast<const uint4 *>(d_summary), a.vol = d_vol, a.grad = d_grad, a.bits = d_bits, a.ranges = d_ranges, a.map = d_map;
	a.unresolved = unresolved, a.n_cells = (uint64_t) me.width * me.height * me.depth;
	a.W = (int) e.width, a.H = (int) e.height, a.D = (int) e.depth, a.mw = (int) me.width, a.mh = (int) me.height;
	a.bx = (int) block_of(e.width, me.width), a.by = (int) block_of(e.height, me.height), a.bz = (int) block_of(e.depth, me.depth);
	a.use_gradient = use_gradient ? 1 : 0;
	a.nd = (a.bx + 3) / 4, a.upc = a.nd * a.by * a.bz;
	const uint64_t groups = (a.n_cells + kCellsPerGroup - 1) / kCellsPerGroup;
	if (!cells_launch_ok(e, me))
		return set_error(ctx, VKV_E_UNSUPPORTED, "occupancy_map_from_summary: map too large for one launch");
	hipLaunchKernelGGL(k_occupancy_from_summary, dim3((uint32_t) groups), dim3(kClassifyLanes), 0, s, a);
	return check_launch(ctx, "occupancy_map_from_summary");
}

}        // namespace vkv

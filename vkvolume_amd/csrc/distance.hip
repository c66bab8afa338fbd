// distance.hip — the Chebyshev distance transforms of the occupancy map (vkv_distance_map, vkv_distance_map_anisotropic;
// shaders/distance_map.comp, distance_map_anisotropic.comp): out(p) = min over q of max(|q - p|, g(q)) one axis after the other, two-sided or
// towards one side per axis for the eight octant maps.  Replaces ComputeDistanceMap's transform passes (src/compute_distance_map.cpp:142-252).
//
// The x pass is k_dm_x_wave<MODE, C, VEC>: a wave per map row, the row in registers, rows of up to 2048 cells (distance_launch_ok; the entry
// points refuse longer rows before anything is enqueued).  The y and z passes are k_dm_rmq<MODE, XT, SEG>: range-minimum queries on a sparse
// table in LDS, for lines of any length.
#include <type_traits>

#include "launchers.hpp"

using namespace vkv;

// x pass for rows of up to 2048 cells: one WAVE per row, the row in registers (C cells per lane).
// Stage 0 of both shaders is the min-plus recurrence g = min(g_prev + 1, occ) (distance_map.comp:57-71 forward and backward in place,
// distance_map_anisotropic.comp:44-53 one-sided), whose closed form is
//     out(x) = min over q of (g(q) + |x - q|)            (one-sided: q >= x for dir > 0, q <= x for dir < 0),
// i.e. x + the running minimum of g(q) - q from the left, and the running minimum of g(q) + q from the right minus x: two scans - inside
// the lane over its C cells, across the lanes with six shuffle steps.  Exact for ANY byte input (not only 0 / 255 occupancy), like the
// recurrence.  Reads the whole row before it writes: dst may alias src.  MODE 0: two-sided -> dst; +1 / -1: one-sided -> dst;
// 2: dst = +1 result, dst2 = -1 result.  VEC: rows are dword-aligned (mw % 4 == 0, aligned pointers).
template <int MODE, int C, bool VEC>
__global__ void __launch_bounds__(256) k_dm_x_wave(const uint8_t *src, uint8_t *dst, uint8_t *dst2, int mw, uint32_t n_rows)
{
	// a wave takes kRows consecutive rows and has the loads of all of them in flight before it scans the first (one row is 256 bytes to 1 KB:
	// with one row per wave a CU keeps 8 KB in flight and the pass runs at 1.4 TB/s)
	constexpr int  kRows = C <= 8 ? 4 : (C <= 16 ? 2 : 1);        // (C = 32, rows of 1025 .. 2048 cells - round 6: a row is 1 - 2 KB, one per wave)
	const uint32_t row0  = (blockIdx.x * 4u + (threadIdx.x >> 6)) * kRows;
	if (row0 >= n_rows)
		return;        // wave-uniform
	const int     lane = (int) (threadIdx.x & 63u), x0 = lane * C;
	constexpr int kFar = 1 << 20;        // padding cells past the end of the row: never the minimum
	uint32_t      raw[kRows][C / 4];
	uint8_t       rawb[VEC ? 1 : kRows][VEC ? 1 : C];
#pragma unroll
	for (int r = 0; r < kRows; ++r)
	{
		const size_t ro = (size_t) min(row0 + (uint32_t) r, n_rows - 1u) * (size_t) mw;        // (rows past the end: the last row again, not stored)
		if (VEC)
		{
#pragma unroll
			for (int j = 0; j < C / 4; ++j)
				raw[r][j] = x0 + 4 * j < mw ? *reinterpret_cast<const uint32_t *>(src + ro + x0 + 4 * j) : 0u;
		}
		else
		{
#pragma unroll
			for (int i = 0; i < C; ++i)
				rawb[VEC ? 0 : r][VEC ? 0 : i] = x0 + i < mw ? src[ro + x0 + i] : (uint8_t) 0;
		}
	}
#pragma unroll
	for (int r = 0; r < kRows; ++r)
	{
		if (row0 + (uint32_t) r >= n_rows)
			break;        // wave-uniform
		const size_t ro = (size_t) (row0 + (uint32_t) r) * (size_t) mw;
		int          g[C];
#pragma unroll
		for (int i = 0; i < C; ++i)
		{
			const int v = VEC ? (int) ((raw[r][i / 4] >> (8 * (i & 3))) & 255u) : (int) rawb[VEC ? 0 : r][VEC ? 0 : i];
			g[i]        = x0 + i < mw ? v : kFar;
		}
		// running minimum of g(q) - q over q <= x (left candidates) and of g(q) + q over q >= x (right candidates), inside the lane
		int pre[C], suf[C];
		{
			int m = 2 * kFar;
#pragma unroll
			for (int i = 0; i < C; ++i)
				m = min(m, g[i] - (x0 + i)), pre[i] = m;
			m = 2 * kFar;
#pragma unroll
			for (int i = C - 1; i >= 0; --i)
				m = min(m, g[i] + (x0 + i)), suf[i] = m;
		}
		// exclusive scans over the lanes: `left` = minimum over all lower lanes, `right` = over all higher lanes
		int left = pre[C - 1], right = suf[0];
#pragma unroll
		for (int o = 1; o < 64; o <<= 1)
		{
			const int l = __shfl_up(left, o), rr = __shfl_down(right, o);
			left = lane >= o ? min(left, l) : left, right = lane + o < 64 ? min(right, rr) : right;
		}
		left = __shfl_up(left, 1), right = __shfl_down(right, 1);
		if (lane == 0)
			left = 2 * kFar;
		if (lane == 63)
			right = 2 * kFar;
		uint32_t wa[C / 4], wb[C / 4];
#pragma unroll
		for (int j = 0; j < C / 4; ++j)
		{
			wa[j] = 0, wb[j] = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b)
			{
				const int i = 4 * j + b, x = x0 + i;
				const int L = min(left, pre[i]) + x, R = min(right, suf[i]) - x;        // both <= g[i] <= 255 for cells of the row
				const int a = MODE == 0 ? min(L, R) : (MODE == -1 ? L : R);
				wa[j] |= (uint32_t) (a & 255) << (8 * b);
				wb[j] |= (uint32_t) (L & 255) << (8 * b);
			}
		}
		if (VEC)
		{
#pragma unroll
			for (int j = 0; j < C / 4; ++j)
				if (x0 + 4 * j < mw)
				{
					*reinterpret_cast<uint32_t *>(dst + ro + x0 + 4 * j) = wa[j];
					if (MODE == 2)
						*reinterpret_cast<uint32_t *>(dst2 + ro + x0 + 4 * j) = wb[j];
				}
		}
		else
		{
#pragma unroll
			for (int i = 0; i < C; ++i)
				if (x0 + i < mw)
				{
					dst[ro + x0 + i] = (uint8_t) (wa[i / 4] >> (8 * (i & 3)));
					if (MODE == 2)
						dst2[ro + x0 + i] = (uint8_t) (wb[i / 4] >> (8 * (i & 3)));
				}
		}
	}
}

// ---------------------------------------------------------------------------------------------
// Axis pass of the distance transform (x, y or z), every cell an independent lane of work.
// With m_r(p) = min of g over the candidates within r cells of p (a window that only grows with r),
//     out(p) = min over q of max(|q - p|, g(q)) = the smallest r with m_r(p) <= r
// (below that r every max(r, m_r) equals m_r > r; at it the value is r itself).  This is what the reference's zig-zag search
// (distance_map.comp:72-107, up to 2 x 255 reads per cell) and the anisotropic one-sided search (distance_map_anisotropic.comp:
// 55-91) compute.  The predicate is monotone in r and true at r = g(p), so 8 bisection steps settle a cell, each one a
// range-minimum query answered with two byte reads from a sparse table (level k = minima of 2^k consecutive cells) that the
// workgroup builds in LDS four cells per operation.  Results of neighbouring cells differ by at most one (two-sided) or follow
// from the neighbour with one window test (one-sided), so a thread bisects only the first cell of its run and walks the rest.
// History: a data-dependent search out of an LDS strip (1.4 ms for the three C3 passes), then an O(N) monotone-deque sweep per
// column (0.66 ms: 51 K serial sweeps whose LDS round trips sit on one dependency chain), now 0.13 ms.
// A workgroup takes XT lines and a run of the axis: the whole line when it fits SEG cells, else `ch` outputs plus 255 cells of
// halo on both sides (a candidate further away can never win: the result never exceeds g(p) <= 255).
// MODE 0: two-sided, +1 / -1: candidates at higher / lower index, 2: both one-sided results from one table (dst = +1,
// dst2 = -1; the anisotropic schedule always needs the pair).
// ---------------------------------------------------------------------------------------------
// byte-wise unsigned minimum of two packed dwords (no carries between the bytes)
__device__ __forceinline__ uint32_t min_u8x4(uint32_t a, uint32_t b)
{
	const uint32_t d  = (a | 0x80808080u) - (b & 0x7f7f7f7fu);                        // bit 7 of a byte: low 7 bits of a >= those of b
	const uint32_t ge = ((a & ~b) | (~(a ^ b) & d)) & 0x80808080u;                    // bit 7: a >= b
	const uint32_t m  = (ge - (ge >> 7)) | ge;                                        // 0xff where a >= b
	return (b & m) | (a & ~m);
}

// up to four independent passes of one launch (blockIdx.y picks one): the anisotropic schedule runs both y passes, then all four z passes,
// as one grid each
struct DmPasses
{
	const uint8_t *src[4];
	uint8_t *      dst[4], *dst2[4];
};

template <int MODE, int XT, int SEG, int THREADS = 256>
__global__ void __launch_bounds__(THREADS) k_dm_rmq(const DmPasses passes, uint32_t n_lines, int len, size_t axis_stride, size_t other_stride, uint32_t chunks_x,
                                                uint32_t chunks_p, int ch, int vec)
{
	// A line is one run of the axis; the workgroup owns lines cx * XT .. + XT (consecutive x) of group `other`; LDS index p * XT + line
	// (a dword = 4 lines of one cell row).  The levels of the sparse table, then one (MODE 2: two) level-sized result area for a coalesced
	// write-out.  src may be dst (in place) when a workgroup stages whole lines (chunks_p == 1): it reads only the cells it writes.
	// Levels 0 .. kTop: a query never spans more than the staged cells, and a window of up to 2^(kTop + 1) cells is covered by two blocks of
	// level kTop (its first and its last 2^kTop cells overlap or touch) - so 256 staged cells need levels 0..7, not 0..8: one level less to
	// build, and 20 KB instead of 22 for the anisotropic passes (8 workgroups per CU instead of 7)
	constexpr int kTop   = SEG <= 128 ? 6 : (SEG <= 256 ? 7 : 8);
	constexpr int kLevel = SEG * XT, kOut = (kTop + 1) * kLevel;
	__shared__ __align__(16) uint8_t s_t[(kTop + 1 + (MODE == 2 ? 2 : 1)) * kLevel];
	const uint8_t *src = passes.src[blockIdx.y];
	uint8_t *      dst = passes.dst[blockIdx.y], *dst2 = passes.dst2[blockIdx.y];
	// neighbouring line groups read and write parts of the same 128-byte lines: give each XCD (own L2) a contiguous range of them
	const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
	const uint32_t cx = bid % chunks_x, cp = (bid / chunks_x) % chunks_p, other = bid / (chunks_x * chunks_p);
	const int      out0 = (int) cp * ch, out1 = min(len, out0 + ch);
	const int      seg0 = max(0, out0 - 255), n = min(len, out1 + 255) - seg0;        // staged cells [seg0, seg0 + n), n <= SEG
	const int      t      = (int) threadIdx.x;
	const size_t   base   = (size_t) other * other_stride + (size_t) cx * XT + (size_t) seg0 * axis_stride;
	auto           at     = [](int p, int line) { return p * XT + line; };
	// staging / write-out: iteration q of a thread is cell (line, p): 256 / XT cell rows of XT lines at a time
	const int n_iter = (n + THREADS / XT - 1) / (THREADS / XT);
	auto      cell   = [&](int q, int &line, int &p) { line = t % XT, p = t / XT + q * (THREADS / XT); };
	using vec_t = typename std::conditional<XT == 16, uint4, typename std::conditional<XT == 8, uint2, uint32_t>::type>::type;        // the XT lines of one cell row
	// `vec`: every group of XT lines (one XT-byte row segment) is an aligned vector in memory and in the LDS layout - one load / store
	// instruction moves what XT byte-wide ones would
	if (vec)
	{
		for (int p = t; p < n; p += THREADS)
			*reinterpret_cast<vec_t *>(s_t + p * XT) = *reinterpret_cast<const vec_t *>(src + base + (size_t) p * axis_stride);
	}
	else
	{
		constexpr int kBatch = 8;        // loads in flight per thread
		for (int q0 = 0; q0 < n_iter; q0 += kBatch)
		{
			uint8_t v[kBatch];
#pragma unroll
			for (int j = 0; j < kBatch; ++j)
			{
				int line, p;
				cell(q0 + j, line, p);
				const bool ok = q0 + j < n_iter && p < n && cx * XT + (uint32_t) line < n_lines;
				v[j]          = ok ? src[base + (size_t) line + (size_t) p * axis_stride] : (uint8_t) 255;
			}
#pragma unroll
			for (int j = 0; j < kBatch; ++j)
			{
				int line, p;
				cell(q0 + j, line, p);
				if (q0 + j < n_iter && p < n)
					s_t[at(p, line)] = v[j];
			}
		}
	}
	__syncthreads();
	// ---- sparse table, four cells per operation ------------------------------------------------------------------
	for (int k = 1; k <= kTop && (1 << (k - 1)) < n; ++k)
	{
		const int       h = 1 << (k - 1);
		const uint32_t *a = reinterpret_cast<const uint32_t *>(s_t + (k - 1) * kLevel);
		uint32_t *      b = reinterpret_cast<uint32_t *>(s_t + k * kLevel);
		// dword = 4 lines of cell row p; the partner is the same dword h rows on
		constexpr int kDw = XT / 4;
		for (int e = t; e < n * kDw; e += THREADS)
		{
			const int      p = e / kDw;
			const uint32_t o = (p + h < n) ? a[e + h * kDw] : 0xffffffffu;
			b[e]             = min_u8x4(a[e], o);
		}
		__syncthreads();
	}
	// ---- results: each thread owns a run of consecutive cells of one line; the first by bisection, the rest by walking
	// (the result of a neighbouring cell differs by at most one, so one or two window tests settle each further cell)
	{
		constexpr int kRuns = THREADS / XT;
		const int     line  = t % XT, run = t / XT;
		const int     nout  = out1 - out0, rl = (nout + kRuns - 1) / kRuns;
		const int     pa = out0 - seg0 + run * rl, pb = min(pa + rl, out1 - seg0);        // [pa, pb)
		auto rmq = [&](int l, int r) -> uint32_t {
			const int      k  = min(31 - __builtin_clz((uint32_t) (r - l + 1)), kTop);
			const uint8_t *tk = s_t + k * kLevel;
			return min((uint32_t) tk[at(l, line)], (uint32_t) tk[at(r - (1 << k) + 1, line)]);
		};
		auto bisect = [&](int p, int dir) -> uint32_t {
			uint32_t lo = 0, hi = s_t[at(p, line)];
#pragma unroll
			for (int it = 0; it < 8; ++it)
			{
				const uint32_t mid = (lo + hi) >> 1;
				const int      l = dir == 1 ? p : max(p - (int) mid, 0);
				const int      r = dir == -1 ? p : min(p + (int) mid, n - 1);
				const bool     ok = rmq(l, r) <= mid;
				hi = ok ? mid : hi;
				lo = ok ? lo : mid + 1;
			}
			return hi;
		};
		if (pa < pb)
		{
			if (MODE == 0)
			{        // (measured and dropped: the run as two half runs with a bisection each, two chains side by side - C3 iso 0.099-0.109 ms against
				 // 0.087-0.092: the second bisection's 16 reads cost more than the shorter chain returns)
				uint32_t c               = bisect(pa, 0);
				s_t[kOut + at(pa, line)] = (uint8_t) c;
				for (int p = pa + 1; p < pb; ++p)
				{        // out(p) is c - 1, c or c + 1.  Radius c - 1 failed at p - 1, and the window of radius c - 1 at p is that window
					 // minus its first cell plus cell p + c - 1: it can only succeed through the new cell - one byte, no query.
					const int      e    = p + (int) c - 1;
					const bool     down = c >= 1u && e < n && (uint32_t) s_t[at(min(e, n - 1), line)] <= c - 1u;
					const uint32_t w0   = rmq(max(p - (int) c, 0), min(p + (int) c, n - 1));
					c                   = down ? c - 1u : (w0 <= c ? c : c + 1u);
					s_t[kOut + at(p, line)] = (uint8_t) c;
				}
			}
			if (MODE == 2)
			{        // both one-sided results of the run as ONE loop: the walk down (candidates at higher index, from pb - 1) and the walk up
				 // (candidates at lower index, from pa) are independent chains of dependent LDS round trips - side by side each hides the
				 // other's latency (as two loops the LDS stores between them keep the compiler from overlapping them)
				constexpr int o2 = kOut + kLevel;
				uint32_t lo1 = 0, hi1 = s_t[at(pb - 1, line)], lo2 = 0, hi2 = s_t[at(pa, line)];
#pragma unroll
				for (int it = 0; it < 8; ++it)
				{
					const uint32_t m1 = (lo1 + hi1) >> 1, m2 = (lo2 + hi2) >> 1;
					const uint32_t w1 = rmq(pb - 1, min(pb - 1 + (int) m1, n - 1)), w2 = rmq(max(pa - (int) m2, 0), pa);
					const bool     ok1 = w1 <= m1, ok2 = w2 <= m2;
					hi1 = ok1 ? m1 : hi1, lo1 = ok1 ? lo1 : m1 + 1;
					hi2 = ok2 ? m2 : hi2, lo2 = ok2 ? lo2 : m2 + 1;
				}
				uint32_t c1 = hi1, c2 = hi2;
				s_t[kOut + at(pb - 1, line)] = (uint8_t) c1;
				s_t[o2 + at(pa, line)]       = (uint8_t) c2;
				for (int j = 1; j < pb - pa; ++j)
				{
					const int      pd = pb - 1 - j, pu = pa + j;
					const uint32_t wd = c1 >= 1u ? rmq(pd + 1, min(pd + (int) c1, n - 1)) : 255u;
					const uint32_t wu = c2 >= 1u ? rmq(max(pu - (int) c2, 0), pu - 1) : 255u;
					const uint32_t gd = s_t[at(pd, line)], gu = s_t[at(pu, line)];
					const uint32_t Td = (c1 >= 1u && wd <= c1) ? c1 : c1 + 1u, Tu = (c2 >= 1u && wu <= c2) ? c2 : c2 + 1u;
					c1 = min(gd, Td), c2 = min(gu, Tu);
					s_t[kOut + at(pd, line)] = (uint8_t) c1;
					s_t[o2 + at(pu, line)]   = (uint8_t) c2;
				}
			}
			if (MODE == 1)
			{        // candidates at higher index: walk down; the candidates above p give c or c + 1, the cell itself g(p)
				uint32_t c                   = bisect(pb - 1, 1);
				s_t[kOut + at(pb - 1, line)] = (uint8_t) c;
				for (int p = pb - 2; p >= pa; --p)
				{
					const uint32_t w = c >= 1u ? rmq(p + 1, min(p + (int) c, n - 1)) : 255u;
					const uint32_t T = (c >= 1u && w <= c) ? c : c + 1u;
					c                = min((uint32_t) s_t[at(p, line)], T);
					s_t[kOut + at(p, line)] = (uint8_t) c;
				}
			}
			if (MODE == -1)
			{
				constexpr int o2             = kOut;
				uint32_t      c              = bisect(pa, -1);
				s_t[o2 + at(pa, line)]       = (uint8_t) c;
				for (int p = pa + 1; p < pb; ++p)
				{
					const uint32_t w = c >= 1u ? rmq(max(p - (int) c, 0), p - 1) : 255u;
					const uint32_t T = (c >= 1u && w <= c) ? c : c + 1u;
					c                = min((uint32_t) s_t[at(p, line)], T);
					s_t[o2 + at(p, line)] = (uint8_t) c;
				}
			}
		}
	}
	__syncthreads();
	if (vec)
	{
		for (int p = out0 - seg0 + t; p < out1 - seg0; p += THREADS)
		{
			const size_t o = base + (size_t) p * axis_stride;
			*reinterpret_cast<vec_t *>(dst + o) = *reinterpret_cast<const vec_t *>(s_t + kOut + p * XT);
			if (MODE == 2)
				*reinterpret_cast<vec_t *>(dst2 + o) = *reinterpret_cast<const vec_t *>(s_t + kOut + kLevel + p * XT);
		}
		return;
	}
	for (int q = 0; q < n_iter; ++q)
	{
		int line, p;
		cell(q, line, p);
		if (p < out0 - seg0 || p >= out1 - seg0 || cx * XT + (uint32_t) line >= n_lines)
			continue;
		const size_t o = base + (size_t) line + (size_t) p * axis_stride;
		dst[o]         = s_t[kOut + at(p, line)];
		if (MODE == 2)
			dst2[o] = s_t[kOut + kLevel + at(p, line)];
	}
}

namespace vkv
{

template <int MODE>
static int launch_dm_rmq_passes(vkv_ctx *ctx, int axis, const DmPasses &passes, uint32_t n_passes, VkvExtent3D me, hipStream_t s);
static bool dm_whole_lines(int axis, VkvExtent3D me) { return (axis == 1 ? me.height : me.depth) <= 512u; }        // a workgroup stages the whole line: in place is safe

// what the distance transforms can take in one launch: map rows of at most 2048 cells (the x pass)
bool distance_launch_ok(VkvExtent3D me) { return me.width <= 2048; }

// axis: 0 = x, 1 = y, 2 = z.  MODE 2 writes the +1 result to dst and the -1 result to dst2.  The x pass may run in place
// (a wave holds its whole row before it writes).
template <int MODE>
static int launch_dm_rmq(vkv_ctx *ctx, int axis, const uint8_t *src, uint8_t *dst, uint8_t *dst2, VkvExtent3D me, hipStream_t s)
{
	if (axis == 0)
	{        // one wave per row, the row in registers (k_dm_x_wave): rows of up to 2048 cells, and distance_launch_ok admits no longer ones
		const int      len    = (int) me.width;
		const uint32_t n_rows = me.height * me.depth;
		const bool     vec    = (me.width & 3u) == 0 && ((((uintptr_t) src) | ((uintptr_t) dst) | ((uintptr_t) dst2)) & 3u) == 0;
#define VKV_DM_XW(C)                                                                                                                            \
	do                                                                                                                                          \
	{                                                                                                                                           \
		const uint32_t rows_per_wg = 4u * ((C) <= 8 ? 4u : ((C) <= 16 ? 2u : 1u)); /* kRows of the kernel */                                    \
		const dim3     grid((n_rows + rows_per_wg - 1u) / rows_per_wg);                                                                         \
		if (vec)                                                                                                                                \
			hipLaunchKernelGGL((k_dm_x_wave<MODE, C, true>), grid, dim3(256), 0, s, src, dst, dst2, len, n_rows);                                \
		else                                                                                                                                    \
			hipLaunchKernelGGL((k_dm_x_wave<MODE, C, false>), grid, dim3(256), 0, s, src, dst, dst2, len, n_rows);                               \
	} while (0)
		if (len <= 256)
			VKV_DM_XW(4);
		else if (len <= 512)
			VKV_DM_XW(8);
		else if (len <= 1024)
			VKV_DM_XW(16);
		else
			VKV_DM_XW(32);        // up to 2048 cells (the widest map distance_launch_ok lets through)
#undef VKV_DM_XW
		return check_launch(ctx, "distance_map x pass");
	}
	DmPasses one = {};
	one.src[0] = src, one.dst[0] = dst, one.dst2[0] = dst2;
	return launch_dm_rmq_passes<MODE>(ctx, axis, one, 1, me, s);
}

// y (axis 1) or z (axis 2) pass over n_passes independent (src, dst, dst2) triples in one grid
template <int MODE>
static int launch_dm_rmq_passes(vkv_ctx *ctx, int axis, const DmPasses &passes, uint32_t n_passes, VkvExtent3D me, hipStream_t s)
{
	const size_t   sy = me.width, sz = (size_t) me.width * me.height;
	const int      len     = axis == 1 ? (int) me.height : (int) me.depth;
	const uint32_t other   = axis == 1 ? me.depth : me.height;
	const uint32_t n_lines = me.width;
	const size_t   as = axis == 1 ? sy : sz, os = axis == 1 ? sz : sy;
	uintptr_t      al = 0;
	for (uint32_t i = 0; i < n_passes; ++i)
		al |= (uintptr_t) passes.src[i] | (uintptr_t) passes.dst[i] | (uintptr_t) passes.dst2[i];
#define VKV_DM_RMQ(XT, SEG)                                                                                                                            \
	do                                                                                                                                                  \
	{                                                                                                                                                   \
		const int      ch       = len <= (SEG) ? len : (SEG) -510;                                                                                     \
		const uint32_t chunks_p = (uint32_t) ((len + ch - 1) / ch), chunks_x = (n_lines + (XT) -1) / (XT);                                              \
		if ((uint64_t) chunks_x * chunks_p * other > 0x7fffffffull)                                                                                     \
			return set_error(ctx, VKV_E_UNSUPPORTED, "distance_map: map too large for one launch");                                                     \
		const int vec = (me.width & ((XT) -1)) == 0 && (al & ((XT) -1)) == 0;                                                                           \
		hipLaunchKernelGGL((k_dm_rmq<MODE, XT, SEG>), dim3(chunks_x * chunks_p * other, n_passes), dim3(256), 0, s, passes, n_lines, len, as, os, chunks_x, \
		                   chunks_p, ch, vec);                                                                                                          \
	} while (0)
	// (measured and dropped: resident workgroups marching over several tiles with the next tile's cells prefetched into registers - 38 -> 44 us
	// per pass on C3; the CU already overlaps one workgroup's loads with the others' table building.  Round 4: WAVE-OWNED dword columns - a
	// wave builds the nine levels of 4 lines and answers their queries alone, two workgroup barriers instead of eleven - with workgroups of
	// 2 waves x 8 lines or 4 waves x 16 lines: bit-identical, C3 iso 0.102-0.117 ms against 0.087-0.092, aniso 0.41 against 0.30; the same
	// LDS then holds half as many waves per CU (14 against 32), and the walk's dependent LDS round trips need the waves more than the
	// barriers cost: profiles/r4_dm_variants.txt)
	if (len <= 128 && me.width > 16)
		VKV_DM_RMQ(16, 128);
	else if (len <= 256)        // (4 lines per workgroup here: C3 iso 0.112-0.115 ms against 0.087 - the wave slots, not the LDS, cap the CU at this size;
		                        // 16 lines x 512 threads, i.e. 16-byte row segments at the same waves per CU: the same 0.086-0.096 / 0.26 ms) 8 lines per workgroup: 20 KB of LDS instead of 40 (8 workgroups per CU, not 4) and runs of 8 cells per thread:
		VKV_DM_RMQ(8, 256);        // C3 42.6 -> 36.8 us per isotropic pass, 63 -> 47 us per anisotropic pass
	else if (len <= 512)        // whole line, no halo; 4 lines per workgroup: 22 KB of LDS instead of 45 (7 workgroups per CU, not 3): C4 iso 0.70 -> 0.64 ms,
		VKV_DM_RMQ(4, 512);        // aniso 3.11 -> 2.60 ms
	else
		VKV_DM_RMQ(8, 768);
#undef VKV_DM_RMQ
	return check_launch(ctx, "distance_map axis pass");
}

template <int MODE>
static int launch_dm_x(vkv_ctx *ctx, const uint8_t *src, uint8_t *dst, VkvExtent3D me, hipStream_t s)
{
	return launch_dm_rmq<MODE>(ctx, 0, src, dst, nullptr, me, s);
}

// axis: 1 = y, 2 = z
template <int MODE>
static int launch_dm_axis(vkv_ctx *ctx, int axis, const uint8_t *src, uint8_t *dst, VkvExtent3D me, hipStream_t s)
{
	return launch_dm_rmq<MODE>(ctx, axis, src, dst, nullptr, me, s);
}

static int dm_check_extent(vkv_ctx *ctx, VkvExtent3D me)
{
	if (me.width == 0 || me.height == 0 || me.depth == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "distance_map: zero map extent");
	if (!distance_launch_ok(me))
		return set_error(ctx, VKV_E_UNSUPPORTED, "distance_map: map rows longer than 2048 cells (LDS strip limit of the x pass)");
	return VKV_OK;
}

// src/compute_distance_map.cpp:142-175
int launch_distance_map(vkv_ctx *ctx, uint8_t *d_map, uint8_t *d_swap, VkvExtent3D me, hipStream_t s)
{
	int rc = dm_check_extent(ctx, me);
	if (rc) return rc;
	if ((rc = launch_dm_x<0>(ctx, d_map, d_map, me, s))) return rc;
	if ((rc = launch_dm_axis<0>(ctx, 1, d_map, d_swap, me, s))) return rc;
	return launch_dm_axis<0>(ctx, 2, d_swap, d_map, me, s);
}

// src/compute_distance_map.cpp:201-252 — same buffers, same order (stream order replaces the image barriers)
int launch_distance_map_anisotropic(vkv_ctx *ctx, uint8_t *const m[8], uint8_t *swap, VkvExtent3D me, hipStream_t s)
{
	int rc = dm_check_extent(ctx, me);
	if (rc) return rc;
	const uint8_t *occ = m[7];
	if (me.width <= 1024)
	{
		// Same results with 7 launches instead of 14: every pass answers its +1 and -1 queries from one table.  Buffers: the x
		// pass leaves x+ in m[3] and x- in m[7] (in place on the occupancy); y of x+ puts y+ into swap and y- into m[1], whose z
		// passes fill (m[2], m[3]) and then (m[0], m[1]); the x- half repeats this with m[4..7].
		if ((rc = launch_dm_rmq<2>(ctx, 0, occ, m[3], m[7], me, s))) return rc;
		if (dm_whole_lines(1, me) && dm_whole_lines(2, me))
		{        // Three launches: x; both y passes as one grid; all four z passes as one grid (every launch boundary costs a drain and a ramp-up
			 // of a grid that is only three rounds of workgroups deep).  No swap buffer: y of x+ (m[3]) goes to m[0] / m[2], y of x- (m[7]) to
			 // m[4] / m[6] (all four still free), and every z pass writes its + result IN PLACE over its source (a workgroup stages the whole
			 // lines it owns before it writes them) and its - result into the odd neighbour: m[1], m[3], m[5], m[7] (whose x results have
			 // been consumed by the y launch).
			DmPasses y = {}, z = {};
			for (int h = 0; h < 2; ++h)
			{
				uint8_t *const *q = m + 4 * h;
				y.src[h] = q[3], y.dst[h] = q[0], y.dst2[h] = q[2];
				for (int k = 0; k < 2; ++k)
					z.src[2 * h + k] = q[2 * k], z.dst[2 * h + k] = q[2 * k], z.dst2[2 * h + k] = q[2 * k + 1];
			}
			if ((rc = launch_dm_rmq_passes<2>(ctx, 1, y, 2, me, s))) return rc;
			return launch_dm_rmq_passes<2>(ctx, 2, z, 4, me, s);
		}
		for (int h = 0; h < 2; ++h)
		{
			uint8_t *const *q = m + 4 * h;
			if ((rc = launch_dm_rmq<2>(ctx, 1, q[3], swap, q[1], me, s))) return rc;
			if ((rc = launch_dm_rmq<2>(ctx, 2, q[1], q[2], q[3], me, s))) return rc;
			if ((rc = launch_dm_rmq<2>(ctx, 2, swap, q[0], q[1], me, s))) return rc;
		}
		return VKV_OK;
	}
	if ((rc = launch_dm_x<1>(ctx, occ, m[3], me, s))) return rc;                  // stage1(3, +1)
	if ((rc = launch_dm_axis<1>(ctx, 1, m[3], swap, me, s))) return rc;           // stage2(3, +1)
	if ((rc = launch_dm_axis<1>(ctx, 2, swap, m[0], me, s))) return rc;           // stage3(0, +1)
	if ((rc = launch_dm_axis<-1>(ctx, 2, swap, m[1], me, s))) return rc;          // stage3(1, -1)
	if ((rc = launch_dm_axis<-1>(ctx, 1, m[3], swap, me, s))) return rc;          // stage2(3, -1)
	if ((rc = launch_dm_axis<1>(ctx, 2, swap, m[2], me, s))) return rc;           // stage3(2, +1)
	if ((rc = launch_dm_axis<-1>(ctx, 2, swap, m[3], me, s))) return rc;          // stage3(3, -1)
	if ((rc = launch_dm_x<-1>(ctx, occ, m[7], me, s))) return rc;                 // stage1(7, -1) in place
	if ((rc = launch_dm_axis<1>(ctx, 1, m[7], swap, me, s))) return rc;           // stage2(7, +1)
	if ((rc = launch_dm_axis<1>(ctx, 2, swap, m[4], me, s))) return rc;           // stage3(4, +1)
	if ((rc = launch_dm_axis<-1>(ctx, 2, swap, m[5], me, s))) return rc;          // stage3(5, -1)
	if ((rc = launch_dm_axis<-1>(ctx, 1, m[7], swap, me, s))) return rc;          // stage2(7, -1)
	if ((rc = launch_dm_axis<1>(ctx, 2, swap, m[6], me, s))) return rc;           // stage3(6, +1)
	return launch_dm_axis<-1>(ctx, 2, swap, m[7], me, s);                         // stage3(7, -1)
}

// skipping_type's transform of the occupancy map (NONE and BLOCK use the raw 0/255 map: src/compute_distance_map.cpp:96-99)
int launch_map_transform(vkv_ctx *ctx, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D me, int skipping_type, hipStream_t s)
{
	if (skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE)
		return launch_distance_map_anisotropic(ctx, d_maps, d_swap, me, s);
	return skipping_type == VKV_SKIP_DISTANCE ? launch_distance_map(ctx, d_maps[0], d_swap, me, s) : VKV_OK;
}

}        // namespace vkv

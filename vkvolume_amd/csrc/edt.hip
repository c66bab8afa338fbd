// edt.hip — the exact squared Euclidean distance transform of the thresholded voxels of a box (vkv_distance_transform) and the pointwise
// select on it (vkv_select_by_distance): ball erosion, dilation, shells and margins; DESIGN.md §5.16.  (distance.hip is the Chebyshev
// transform of the occupancy CELLS, another metric on another grid.)  Integer work only: no MFMA, no floating point after the threshold, no
// square root.
//
// A voxel is a TARGET iff (byte >= thr) == (target == VKV_DISTANCE_TO_INSIDE), thr = iso_threshold(iso): the mesh's inside rule.  Every
// kernel is one-dimensional over the box-linear index of box_domain.hpp, i = ((z - z0) bh + (y - y0)) bw + (x - x0), one voxel per lane, so
// every access of every pass is coalesced along x; a wave's 64 voxels are one ENTRY, as in components.hip.  All values are squared distances
// CAPPED at `limit` (0xffffffff = VKV_DISTANCE_NONE when unlimited): min(limit, min_u (a_u + b)) = min(limit, min_u (min(limit, a_u) + b))
// for b >= 0, so capping after every pass gives the capped result, and the cap doubles as "no target in this row / column".
//   k_edt_bits   target bits by wave ballot, one 64-bit word per entry (scratch).  Reads the volume, 1 B per voxel.
//   k_edt_x      g(i) = min(limit, dx^2), dx = the distance along the voxel's own row to the nearest target bit: row_walk of edt_passes.hpp,
//                which edt_envelope.hip's x kernel calls too.  Reads the bits, writes the schedule's first buffer.
//   k_edt_axis   out(p) = min over p' of the line of (g(p') + (p - p')^2), for y (stride bw) and then for z (stride bw bh): from best = g(p)
//                it looks at p - d and p + d for d = 1, 2, ... while d^2 < best, four offsets at a time.  Reads one buffer, writes the OTHER (a line's outputs need
//                its inputs: not in place).  A pass over an axis of length 1 is not launched.
// BUFFERS.  The two 4-byte buffers are d_dist2 and the scratch block's, dealt out by EdtSchedule (edt_passes.hpp), which the three exact
// transforms share: the x pass writes the one that makes the last pass land in d_dist2.
// LOOP BOUNDS.  k_edt_x: row_walk's, with reach = ceil(sqrt(limit)) (65536 when unlimited).  k_edt_axis ends at the latest when neither p - d
// nor p + d lies in the line: d < len <= 32768 rounds.  No lane waits for another lane, wave or workgroup; no atomics.
// NO OVERFLOW.  Offsets along an axis are at most 32767, their squares at most 2^30 - 2^16 + 1; a true distance is at most 3 x 32767^2 =
// 3221028867 < 2^32 - 1.  No sum is formed before it is known to fit: a candidate g + d^2 replaces best only after g < best - d^2 was seen,
// with d^2 < best, so the difference does not wrap, a "none" g (the cap) never passes, and g + d^2 < best <= 2^32 - 1.  Box-linear
// indices: i - d stride and i + d stride lie in the line, hence in [0, n), n <= 2^32 - 1.
// No kernel uses scratch memory (tests/test_distance_cpu.py reads the listing).
#include "edt_passes.hpp"

using namespace vkv;

__global__ void __launch_bounds__(256) k_edt_bits(BoxLinear G, uint32_t outside, uint64_t *__restrict__ bits)        // outside 1: the targets are the outside voxels
{
	const BoxVoxel v = box_voxel(G);
	bool           t = false;
	if (v.valid)
		t = (G.vol[box_address(G, v)] >= G.thr) != (outside != 0u);
	const uint64_t m = __ballot(t);        // lanes past the box give 0: the last word's upper bits are no targets
	if (v.valid && v.lane == 0)
		bits[v.i >> 6] = m;
}

// the squared distance along the row, capped: a target further than reach = ceil(sqrt(limit)) away gives the cap anyway
__global__ void __launch_bounds__(256) k_edt_x(BoxLinear G, const uint64_t *__restrict__ bits, uint32_t *__restrict__ out, uint32_t limit, uint32_t reach)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)        // no wave-wide operation below
		return;
	const uint32_t dx = row_walk(G, v, bits, reach);
	// dx <= 32767 where a target was found: dx^2 < 2^30
	out[v.i] = dx == 0xffffffffu ? limit : min(dx * dx, limit);
}

constexpr uint32_t kEdtBatch = 4;

// one axis pass: p = the voxel's position on its line of `len` voxels `stride` apart
__global__ void __launch_bounds__(256) k_edt_axis(uint32_t n, uint32_t stride, uint32_t len, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n)
		return;
	const uint32_t p = (i / stride) % len, below = p, above = len - 1u - p;
	uint32_t       best = src[i];        // <= limit
	const uint32_t far  = max(below, above);
	// kEdtBatch offsets at a time, so that their loads are in flight together: of d .. d + 3 those are loaded that lie in the line and
	// whose d^2 is below best as it stands; best only falls, so what is not loaded could not have won, and what is loaded is a voxel of the line
	for (uint32_t d = 1; d <= far && d * d < best; d += kEdtBatch)        // d < len <= 32768: (d + 3)^2 < 2^31
	{
		uint32_t g[kEdtBatch];
#pragma unroll
		for (uint32_t k = 0; k < kEdtBatch; ++k)
		{
			const uint32_t dd = d + k;
			const uint64_t o  = (uint64_t) dd * stride;
			const bool     in = dd * dd < best, lo = in && dd <= below, hi = in && dd <= above;
			// without a branch, so that nothing waits between the loads: an offset that is not wanted reads the voxel itself
			const uint32_t a = src[i - (lo ? o : 0ull)], b = src[i + (hi ? o : 0ull)];
			g[k]             = min(lo ? a : 0xffffffffu, hi ? b : 0xffffffffu);
		}
#pragma unroll
		for (uint32_t k = 0; k < kEdtBatch; ++k)
		{
			const uint32_t d2 = (d + k) * (d + k);
			if (d2 < best && g[k] < best - d2)        // every voxel from d2 >= best on is at least that far away
				best = g[k] + d2;
		}
	}
	dst[i] = best;
}

__global__ void __launch_bounds__(256) k_edt_select(const uint8_t *src, uint8_t *dst, BoxLinear G, const uint32_t *__restrict__ dist2, uint32_t lo, uint32_t hi,
                                                    uint32_t fill)
{
	box_select(G, src, dst, fill, [&](uint32_t i) {
		const uint32_t d = dist2[i];
		return d >= lo && d <= hi;
	});
}

namespace vkv
{

size_t edt_scratch_bytes(VkvExtent3D e, const VkvBox *box)        // 0: the extent and box are not accepted
{
	EdtSchedule S;
	return S.lay(e, box, nullptr, nullptr) ? S.bytes() : 0;
}

bool edt_launch_ok(VkvExtent3D e, const VkvBox *box)
{
	EdtSchedule S;
	return S.lay(e, box, nullptr, nullptr);
}

int launch_distance_transform(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, uint32_t limit, void *d_scratch,
                              uint32_t *d_dist2, hipStream_t s)
{
	EdtSchedule S;
	if (const int rc = edt_schedule(ctx, "distance_transform", e, b, d_scratch, d_dist2, S))
		return rc;
	const BoxLinear G   = box_linear(d_vol, e, b, S.p, iso);
	uint32_t      reach = 0;        // the smallest r with r^2 >= limit: at most 65536
	while ((uint64_t) reach * reach < limit)
		++reach;
	hipLaunchKernelGGL(k_edt_bits, dim3(S.p.wgs), dim3(256), 0, s, G, target == VKV_DISTANCE_TO_OUTSIDE ? 1u : 0u, S.bits);
	hipLaunchKernelGGL(k_edt_x, dim3(S.p.wgs), dim3(256), 0, s, G, S.bits, S.cur, limit, reach);
	S.axes([&](const uint32_t *src, uint32_t *dst) { hipLaunchKernelGGL(k_edt_axis, dim3(S.p.wgs), dim3(256), 0, s, S.p.n, b.width, b.height, src, dst); },
	       [&](const uint32_t *src, uint32_t *dst) { hipLaunchKernelGGL(k_edt_axis, dim3(S.p.wgs), dim3(256), 0, s, S.p.n, b.width * b.height, b.depth, src, dst); });
	return check_launch(ctx, "distance_transform");
}

int launch_select_by_distance(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, const uint32_t *d_dist2, uint32_t lo,
                              uint32_t hi, uint32_t fill, hipStream_t s)
{
	EdtSchedule S;        // for its plan and its limits: no pass is scheduled
	if (const int rc = edt_schedule(ctx, "select_by_distance", e, b, nullptr, nullptr, S))
		return rc;
	const BoxLinear G = box_linear(d_src, e, b, S.p, 0.0f);        // thr is not read
	hipLaunchKernelGGL(k_edt_select, dim3(S.p.wgs), dim3(256), 0, s, d_src, d_dst, G, d_dist2, lo, hi, fill);
	return check_launch(ctx, "select_by_distance");
}

}        // namespace vkv

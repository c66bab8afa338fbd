// nearest.hip — the nearest-target (feature) transform of a box (vkv_nearest_target) and the gather that hands labels along it
// (vkv_propagate_labels); DESIGN.md §5.19.  d_nearest[v] = the SMALLEST BOX-LINEAR INDEX among the targets at the least weighted distance
// D(v) = min over the targets u of (wx dx)^2 + (wy dy)^2 + (wz dz)^2, or VKV_NEAREST_NONE where the box holds no target or D(v) >= limit.
// Targets, the box-linear domain, the weights, the cap and the scratch block are those of edt_envelope.hip (§5.18); the envelope pass
// with its invariants and tie rule, k_edt_bits' declaration and the schedule of the passes are edt_passes.hpp's, as is the row walk that
// k_near_x restates.  Integer work only.
// THE PASSES CARRY FEATURES, NOT DISTANCES.  The two ping-pong buffers are d_nearest and the uint32 buffer of the scratch block; a pass reads
// the feature stored at a position and recomputes g from it and the lane's own coordinates, so there is no third buffer.  NONE (0xffffffff)
// means "no target within the cap so far" in every format; a stored feature always has g < limit.
//   k_near_x          feature = x' of the nearest target of the row, the LEFT one on a tie: row_walk's walk, written out (the note at the
//                     kernel).  NONE where the row holds none within reach or (wx dx)^2 >= limit.
//   k_near_axis<1>    y: g(u) = (wx |x - x'|)^2 from the feature x' at (x, u); writes s mul + x' for the winning s, mul = 32768 (y' << 15 | x',
//                     30 bits, decoded without a division) when a z pass follows and mul = bw (the box-linear index) when it is the last.
//   k_near_axis<2>    z: g(u) = (wx |x - x'|)^2 + (wy |y - y'|)^2 from y' << 15 | x' (an x' alone where bh == 1: y' = 0); always the last pass:
//                     writes (s bh + y') bw + x'.
// With bh == bd == 1 the x pass is the last, and x' is the box-linear index.  The last pass that is launched lands in d_nearest and also
// writes d_dist2 = min(limit, D) if that was given: the value k_env_x / k_env_axis store.
// TIES.  Each pass gives a tie to the smaller coordinate along its own axis: the x walk to the left target, envelope_line to the smaller
// position.  Smallest z', then smallest y', then smallest x' is the smallest box-linear index (DESIGN.md §5.19 has the full argument).
// LOOP BOUNDS.  Those of row_walk and envelope_line.  k_propagate: no loop.  No lane waits for another lane, wave or workgroup; no atomics; no
// private arrays (ScratchSize 0, tests/test_nearest_cpu.py reads the listing).
// NO OVERFLOW.  The weights are admitted by edt_weights_fit (host_arith.hpp): every w (len - 1) <= 65535 and the sum of the three squares
// <= 0xfffffffe, so g, a sum of at most two such squares of in-box differences, is below 2^32, which is what envelope_line asks for.
// Coordinates are <= 32767 (15 bits): y' << 15 | x' < 2^30 and s mul + x' <= 32767 * 32768 + 32767 < 2^30 for mul = 32768; with mul = bw and
// in the z pass the value is a box-linear index < n <= 2^32 - 1, so no feature equals NONE.  k_propagate reads d_labels only at an index < n.
#include "edt_passes.hpp"

using namespace vkv;

#define NEAR_NONE 0xffffffffu

// row_walk (edt_passes.hpp) WRITTEN OUT, with the target's x' taken inside its two loops.  As a call of row_walk, which had to hand back on
// which side the winner lies, the kernel came to 884 bytes against 836 (18 VGPRs against 19, 32 SGPRs against 26), and in
// tools/time_nearest.py the salt-noise scene's vkv_nearest_target rows to the inside at limit none, weights (2, 2, 5), and to the outside at
// weights (1, 1, 1), with Volume.split_bodies on both scenes, lay 0.14 to 1.5 % above the previous library's median, outside its spread, in
// two sessions out of two (profiles/edt_family_refactor.txt).  A fix to the walk is made in row_walk AND here
__global__ void __launch_bounds__(256) k_near_x(BoxLinear G, const uint64_t *__restrict__ bits, uint32_t *__restrict__ out, uint32_t *__restrict__ dist,
                                                uint32_t limit, uint32_t reach, uint32_t w)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)        // no wave-wide operation below
		return;
	const uint32_t lo = v.i - min(v.x, reach), hi = v.i + min(G.bw - 1u - v.x, reach);        // lo <= i <= hi < n
	uint32_t       dx = 0xffffffffu, xt = 0;        // the distance along the row and the target's x'
	{        // the highest target bit in [lo, i]
		uint32_t wd = v.i >> 6;
		uint64_t m  = bits[wd] & (~0ull >> (63u - (v.i & 63u)));
		for (;;)        // wd falls to lo >> 6 at the latest
		{
			const bool last = wd == lo >> 6;
			if (last)
				m &= ~0ull << (lo & 63u);
			if (m)
			{
				dx = v.i - (wd * 64u + 63u - (uint32_t) __clzll((long long) m));
				xt = v.x - dx;
				break;
			}
			if (last)
				break;
			m = bits[--wd];
		}
	}
	if (dx != 0u)
	{        // the lowest target bit in [i, end]: nothing further than dx - 1 can win, so a tie stays with the left target.  end <= hi < n: no wrap
		const uint32_t end = v.i + min(hi - v.i, dx - 1u);
		uint32_t       wd  = v.i >> 6;
		uint64_t       m   = bits[wd] & (~0ull << (v.i & 63u));
		for (;;)        // wd rises to end >> 6 at the latest
		{
			const bool last = wd == end >> 6;
			if (last)
				m &= ~0ull >> (63u - (end & 63u));
			if (m)
			{
				dx = wd * 64u + (uint32_t) __builtin_ctzll(m) - v.i;
				xt = v.x + dx;
				break;
			}
			if (last)
				break;
			m = bits[++wd];
		}
	}
	// dx <= bw - 1 where a target was found: w dx <= 65535 (a weight above 65535 comes with bw == 1, dx == 0)
	const uint32_t wdx = w * (dx == 0xffffffffu ? 0u : dx);
	const bool     hit = dx != 0xffffffffu && wdx * wdx < limit;
	out[v.i]           = hit ? xt : NEAR_NONE;
	if (dist)        // the last pass: bh == bd == 1
		dist[v.i] = hit ? wdx * wdx : limit;
}

// what an axis pass knows of the box and of the passes before it
struct NearAxis
{
	uint32_t bw, bh;        // the box's row and rows per slice
	uint32_t wx, wy;        // the weights of the axes already done
	uint32_t mul;           // y pass: the feature written is s mul + x'
};

// g of a source feature (not NONE) for the lane at (x, y): below 2^32
template <int AXIS>
__device__ __forceinline__ uint32_t near_g(const NearAxis &A, uint32_t x, uint32_t y, uint32_t f)
{
	if (AXIS == 1)
		return edt_wd2(A.wx, x, f);
	return edt_wd2(A.wx, x, f & 0x7fffu) + edt_wd2(A.wy, y, f >> 15);
}

// a position carries the feature of the passes before it, or NONE; a stored feature has g < limit: the pass before stored none otherwise
template <int AXIS>
struct FeatureCarry
{
	NearAxis  A;
	uint32_t  x, y;        // the lane's coordinates on the axes already done
	uint32_t  limit;
	uint32_t *dist;        // null, or d_dist2 in the last pass

	__device__ __forceinline__ bool     skips(uint32_t e) const { return e == NEAR_NONE; }
	__device__ __forceinline__ uint32_t g(uint32_t e) const { return near_g<AXIS>(A, x, y, e); }
	struct Out
	{
		uint32_t feature, d2;
	};
	__device__ __forceinline__ Out none() const { return Out{NEAR_NONE, limit}; }
	// the winner's feature, extended by this axis's coordinate s
	__device__ __forceinline__ Out value(uint32_t s, uint32_t e, uint64_t f) const
	{
		if (f >= limit)
			return none();
		return Out{AXIS == 1 ? s * A.mul + e : (s * A.bh + (e >> 15)) * A.bw + (e & 0x7fffu), (uint32_t) f};
	}
	__device__ __forceinline__ void store(uint32_t *dst, uint32_t i, Out out) const
	{
		dst[i] = out.feature;
		if (dist)
			dist[i] = out.d2;
	}
};

// one axis pass: lane L owns line L of the n / len lines of `len` voxels `stride` apart; src and dst are the two feature buffers, never the
// same; dist: null, or d_dist2 in the last pass
template <int AXIS>
__global__ void __launch_bounds__(256) k_near_axis(uint32_t lines, uint32_t stride, uint32_t len, uint32_t w, uint32_t limit, NearAxis A,
                                                   const uint32_t *__restrict__ src, uint32_t *dst, uint32_t *__restrict__ dist)
{
	const uint32_t L = blockIdx.x * 256u + threadIdx.x;
	if (L >= lines)
		return;
	const uint32_t base = (L / stride) * stride * len + L % stride;        // the line's first voxel: below n
	const uint32_t x = L % A.bw, y = AXIS == 1 ? 0u : L / A.bw;            // z: L < bw bh
	envelope_line(base, stride, len, w, FeatureCarry<AXIS>{A, x, y, limit, dist}, src, dst);
}

// d_out[v] = d_labels[d_nearest[v]] where that index lies in the box and (masked: G.vol is given) the mask's voxel v is inside, else 0.
// VKV_NEAREST_NONE is no index of a box.  A lane writes its own element only; out overlaps neither input (the entry point's check)
__global__ void __launch_bounds__(256) k_propagate(BoxLinear G, const uint32_t *__restrict__ nearest, const uint32_t *__restrict__ labels,
                                                   uint32_t *__restrict__ out)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)
		return;
	const uint32_t f = nearest[v.i];
	uint32_t       r = 0;
	if (f < G.n && (!G.vol || G.vol[box_address(G, v)] >= G.thr))
		r = labels[f];
	out[v.i] = r;
}

namespace vkv
{

int launch_nearest_target(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, const uint32_t weights[3], uint32_t limit,
                          void *d_scratch, uint32_t *d_nearest, uint32_t *d_dist2, hipStream_t s)
{
	EdtSchedule S;
	if (const int rc = edt_schedule(ctx, "nearest_target", e, b, d_scratch, d_nearest, S))
		return rc;
	const BoxLinear G = box_linear(d_vol, e, b, S.p, iso);
	hipLaunchKernelGGL(k_edt_bits, dim3(S.p.wgs), dim3(256), 0, s, G, target == VKV_DISTANCE_TO_OUTSIDE ? 1u : 0u, S.bits);
	hipLaunchKernelGGL(k_near_x, dim3(S.p.wgs), dim3(256), 0, s, G, S.bits, S.cur, (S.y || S.z) ? nullptr : d_dist2, limit,
	                   edt_weighted_reach(limit, weights[0]), weights[0]);
	const NearAxis A{b.width, b.height, weights[0], weights[1], S.z ? 32768u : b.width};
	S.axes(
	    [&](const uint32_t *src, uint32_t *dst) {
		    const uint32_t lines = S.p.n / b.height;
		    hipLaunchKernelGGL(k_near_axis<1>, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, b.width, b.height, weights[1], limit, A, src, dst,
		                       S.z ? nullptr : d_dist2);
	    },
	    [&](const uint32_t *src, uint32_t *dst) {
		    const uint32_t lines = b.width * b.height;
		    hipLaunchKernelGGL(k_near_axis<2>, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, lines, b.depth, weights[2], limit, A, src, dst, d_dist2);
	    });
	return check_launch(ctx, "nearest_target");
}

int launch_propagate_labels(vkv_ctx *ctx, const uint32_t *d_nearest, const uint32_t *d_labels, uint32_t *d_out, VkvExtent3D e, const VkvBox &b,
                            const uint8_t *d_mask_vol, float mask_iso, hipStream_t s)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "propagate_labels: a box of more than 2^32 - 1 voxels");
	const BoxLinear G = box_linear(d_mask_vol, e, b, p, d_mask_vol ? mask_iso : 0.0f);        // vol null: no mask, thr is not read
	hipLaunchKernelGGL(k_propagate, dim3(p.wgs), dim3(256), 0, s, G, d_nearest, d_labels, d_out);
	return check_launch(ctx, "propagate_labels");
}

}        // namespace vkv

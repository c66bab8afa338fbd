// nearest.hip — the nearest-target (feature) transform of a box (vkv_nearest_target) and the gather that hands labels along it
// (vkv_propagate_labels); DESIGN.md §5.19.  d_nearest[v] = the SMALLEST BOX-LINEAR INDEX among the targets at the least weighted distance
// D(v) = min over the targets u of (wx dx)^2 + (wy dy)^2 + (wz dz)^2, or VKV_NEAREST_NONE where the box holds no target or D(v) >= limit.
// Targets, the box-linear domain, the weights, the cap and the scratch block are those of edt_envelope.hip (§5.18), which stays as it is,
// as does edt.hip: its k_edt_bits is launched from here through a declaration.  Integer work only.
// THE PASSES CARRY FEATURES, NOT DISTANCES.  The two ping-pong buffers are d_nearest and the uint32 buffer of the scratch block; a pass reads
// the feature stored at a position and recomputes g from it and the lane's own coordinates, so there is no third buffer.  NONE (0xffffffff)
// means "no target within the cap so far" in every format; a stored feature always has g < limit.
//   k_near_x          feature = x' of the nearest target of the row, the LEFT one on a tie: k_env_x's walk (the search to the right goes up to
//                     dx - 1 only).  NONE where the row holds none within reach or (wx dx)^2 >= limit.  The walk is repeated here a second
//                     time for §5.18's reason: shared through a header it changed k_edt_x's listing, and edt.hip's and edt_envelope.hip's
//                     code objects are not to change.
//   k_near_axis<1>    y: g(u) = (wx |x - x'|)^2 from the feature x' at (x, u); writes s mul + x' for the winning s, mul = 32768 (y' << 15 | x',
//                     30 bits, decoded without a division) when a z pass follows and mul = bw (the box-linear index) when it is the last.
//   k_near_axis<2>    z: g(u) = (wx |x - x'|)^2 + (wy |y - y'|)^2 from y' << 15 | x' (an x' alone where bh == 1: y' = 0); always the last pass:
//                     writes (s bh + y') bw + x'.
// With bh == bd == 1 the x pass is the last, and x' is the box-linear index.  The last pass that is launched lands in d_nearest and also
// writes d_dist2 = min(limit, D) if that was given: the value k_env_x / k_env_axis store.
// k_near_axis IS k_env_axis: one line per lane, consecutive lanes on consecutive x, the lower envelope as a stack of (s, t) built forward
// and read backward, the entry s | t << 15 of the stack IN THE DESTINATION LINE of the feature buffer (uint32, as there), the same
// inequalities: forward k <= u and dst is not yet written; backward k <= t_k <= u, and the store at u hits an entry only when u = k = t_k,
// the top, which is held in registers (s, t, its source feature fs and g(s)) and popped by that very step.
// TIES.  Each pass gives a tie to the smaller coordinate along its own axis: the x walk as said; the envelope because the pop test is a
// strict > (a parabola that only ties at t stays) and a range starts at 1 + floor(the crossing) (the older, smaller s keeps the crossing
// itself).  A popped s is strictly above u at t and everywhere after, and was above its predecessors before t: it wins nowhere, ties
// included.  Smallest z', then smallest y', then smallest x' is the smallest box-linear index (DESIGN.md §5.19 has the full argument).
// LOOP BOUNDS.  k_near_x: as k_env_x, at most min(bw, reach) / 64 + 2 words per side.  k_near_axis, per lane: every position is pushed at
// most once and popped at most once: at most 2 len forward iterations and len backward, len <= 32768.  k_propagate: no loop.  No lane waits
// for another lane, wave or workgroup; no atomics; no private arrays (ScratchSize 0, tests/test_nearest_cpu.py reads the listing).
// NO OVERFLOW.  The weights are admitted by edt_weights_fit (host_arith.hpp), unchanged: every w (len - 1) <= 65535 and the sum of the three
// squares <= 0xfffffffe, so g, a sum of at most two such squares of in-box differences, is below 2^32 and f = g + (w d)^2 below 2^33 in 64
// bits; numerator and denominator of the one division per push are §5.18's.  Coordinates are <= 32767 (15 bits): y' << 15 | x' < 2^30 and
// s mul + x' <= 32767 * 32768 + 32767 < 2^30 for mul = 32768; with mul = bw and in the z pass the value is a box-linear index < n <= 2^32 - 1,
// so no feature equals NONE.  Indices base + u stride lie in the line, hence in [0, n).  k_propagate reads d_labels only at an index < n.
#include <utility>

#include "box_domain.hpp"

using namespace vkv;

#define NEAR_NONE 0xffffffffu

// edt.hip's: target bits by wave ballot, one 64-bit word per entry
__global__ void k_edt_bits(BoxLinear G, uint32_t outside, uint64_t *__restrict__ bits);

// k_env_x's walk (a copy: see the head): the row's bits are [i - x, i - x + bw), of which [i - min(x, reach), i + min(bw - 1 - x, reach)] is searched
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

__device__ __forceinline__ uint32_t near_wd2(uint32_t w, uint32_t a, uint32_t b)
{
	const uint32_t wd = w * (a > b ? a - b : b - a);        // at most 65535
	return wd * wd;
}

// g of a source feature (not NONE) for the lane at (x, y): below 2^32
template <int AXIS>
__device__ __forceinline__ uint32_t near_g(const NearAxis &A, uint32_t x, uint32_t y, uint32_t f)
{
	if (AXIS == 1)
		return near_wd2(A.wx, x, f);
	return near_wd2(A.wx, x, f & 0x7fffu) + near_wd2(A.wy, y, f >> 15);
}

// f(p, i) = g(i) + (w (p - i))^2, below 2^33
__device__ __forceinline__ uint64_t near_f(uint32_t p, uint32_t i, uint32_t g, uint32_t w) { return (uint64_t) g + near_wd2(w, p, i); }

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
	const uint32_t x = L % A.bw, y = AXIS == 1 ? 0u : L / A.bw;            // the lane's coordinates on the axes already done (z: L < bw bh)
	const uint64_t w2 = (uint64_t) w * w;
	uint32_t       k = 0, s = 0, t = 0, gs = 0, fs = 0;        // entries on the stack, and the top entry with its source feature and g(s) while k > 0
	// forward: the lower envelope of the parabolas of the positions that hold a feature
	uint32_t next = src[base];
	for (uint32_t u = 0; u < len; ++u)
	{
		const uint32_t fu = next;
		if (u + 1u < len)
			next = src[base + (u + 1u) * stride];        // in flight while u is worked on
		if (fu == NEAR_NONE)
			continue;
		const uint32_t g = near_g<AXIS>(A, x, y, fu);        // below limit: the pass before stored no feature otherwise
		while (k > 0u && near_f(t, s, gs, w) > near_f(t, u, g, w))        // u is STRICTLY lower from t on: the top is never the lowest, nor ties
		{
			--k;
			if (k > 0u)
			{
				const uint32_t e = dst[base + (k - 1u) * stride];
				s = e & 0x7fffu, t = e >> 15;
				fs = src[base + s * stride];
				gs = near_g<AXIS>(A, x, y, fs);
			}
		}
		if (k == 0u)
			t = 0;
		else
		{        // the first position at which u is strictly lower than the top: 1 + floor(the crossing), the crossing >= t
			const uint64_t num = (uint64_t) g + w2 * (uint64_t) (u * u - s * s) - gs, den = 2ull * w2 * (u - s);
			const uint64_t q   = num / den;
			if (q >= len - 1u)
				continue;        // past the line's end
			t = (uint32_t) q + 1u;
		}
		s = u, gs = g, fs = fu;
		dst[base + k * stride] = s | t << 15;        // k <= u
		++k;
	}
	// backward: position u takes the feature of the top entry, extended by this axis's coordinate s; the top is popped where its range ends
	for (uint32_t u = len; u-- > 0u;)
	{
		uint32_t out = NEAR_NONE, d2 = limit;
		if (k > 0u)
		{
			const uint64_t f = near_f(u, s, gs, w);
			if (f < limit)
			{
				d2  = (uint32_t) f;
				out = AXIS == 1 ? s * A.mul + fs : (s * A.bh + (fs >> 15)) * A.bw + (fs & 0x7fffu);
			}
			if (u == t && --k > 0u)
			{        // entry k - 1 lies below position u: the store below does not touch it
				const uint32_t e = dst[base + (k - 1u) * stride];
				s = e & 0x7fffu, t = e >> 15;
				fs = src[base + s * stride];
				gs = near_g<AXIS>(A, x, y, fs);
			}
		}
		dst[base + u * stride] = out;
		if (dist)
			dist[base + u * stride] = d2;
	}
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
	BoxLinearPlan p;
	if (!edt_launch_ok(e, &b) || !box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "nearest_target: a box of more than 2^32 - 1 voxels or an axis above 32768");
	uint64_t     *bits  = static_cast<uint64_t *>(d_scratch);        // the block of edt_scratch_bytes(): [target bits][the second feature buffer]
	uint32_t     *other = reinterpret_cast<uint32_t *>(bits + p.entries);
	const BoxLinear G   = box_linear(d_vol, e, b, p, iso);
	const bool y = b.height > 1u, z = b.depth > 1u;
	uint32_t  *cur = (y != z) ? other : d_nearest, *nxt = (y != z) ? d_nearest : other;        // one further pass: it starts in the scratch block
	hipLaunchKernelGGL(k_edt_bits, dim3(p.wgs), dim3(256), 0, s, G, target == VKV_DISTANCE_TO_OUTSIDE ? 1u : 0u, bits);
	hipLaunchKernelGGL(k_near_x, dim3(p.wgs), dim3(256), 0, s, G, bits, cur, (y || z) ? nullptr : d_dist2, limit, edt_weighted_reach(limit, weights[0]),
	                   weights[0]);
	NearAxis A{b.width, b.height, weights[0], weights[1], z ? 32768u : b.width};
	if (y)
	{
		const uint32_t lines = p.n / b.height;
		hipLaunchKernelGGL(k_near_axis<1>, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, b.width, b.height, weights[1], limit, A, cur, nxt,
		                   z ? nullptr : d_dist2);
		std::swap(cur, nxt);
	}
	if (z)
	{
		const uint32_t lines = b.width * b.height;
		hipLaunchKernelGGL(k_near_axis<2>, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, lines, b.depth, weights[2], limit, A, cur, nxt, d_dist2);
		std::swap(cur, nxt);
	}
	return check_launch(ctx, "nearest_target");        // cur == d_nearest
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

// edt_envelope.hip — the squared Euclidean distance transform with an integer weight per axis (vkv_distance_transform_weighted), by lower
// envelopes; DESIGN.md §5.18.  d_dist2[v] = min(limit, min over the targets u of (wx dx)^2 + (wy dy)^2 + (wz dz)^2): voxel spacing as a ratio
// of small integers.  Targets, the box-linear domain, the two ping-pong buffers and the cap are those of edt.hip, which stays as it is: its
// k_edt_bits is launched from here (declared below), the other kernels are this file's.  Integer work only.
//   k_env_x      g(i) = min(limit, (wx dx)^2): k_edt_x's walk along the row's bits with reach = the smallest r with (wx r)^2 >= limit.
//   k_env_axis   out(p) = min(limit, min over p' of the line of g(p') + (w (p - p'))^2) for y (stride bw) and then z (stride bw bh).  ONE LINE
//                PER LANE, consecutive lanes on consecutive x: every lane of a wave is at the same position u of its line, so the wave's
//                loads and stores run along x.  Forward over u it builds the lower envelope of the parabolas f(p, i) = g(i) + (w (p - i))^2 as
//                a stack of (s, t): parabola s is the lowest from position t on, t strictly increasing from 0.  Backward over u it reads the
//                value off the top entry and pops where u == t.  A capped g(u) = limit is skipped: min(limit, limit + b) = limit.
// THE STACK LIVES IN THE OUTPUT LINE.  Entry k is the uint32 s | t << 15 (s, t <= 32767) at position k of the line in dst, which the backward
// sweep overwrites.  Forward: the entries hold distinct s < u, so k <= u, and dst is not yet written.  Backward: t is strictly increasing from
// t_0 = 0, so k <= t_k <= u for the top entry k; the store of out(u) hits an entry only when u = k = t_k: the top itself, which is held in
// registers and is popped by that very step.  So the call needs no scratch beyond vkv_distance_transform_scratch_bytes.
// LOOP BOUNDS.  k_env_x: as k_edt_x, at most min(bw, reach) / 64 + 2 words per side.  k_env_axis, per lane: every position is pushed at most
// once and popped at most once, so the forward sweep makes at most 2 len iterations (len steps of u plus len pops) and the backward sweep len,
// len <= 32768.  No lane waits for another lane, wave or workgroup; no atomics.
// NO OVERFLOW.  The entry point admits weights only where every w (len - 1) <= 65535 and the sum of their squares is at most 0xfffffffe
// (edt_weights_fit, host_arith.hpp): w d <= 65535 and (w d)^2 < 2^32 in 32 bits, g <= 0xffffffff, f = g + (w d)^2 < 2^33 in 64 bits.  The pop
// test compares two f and does not divide.  After the pops f(t_top, s_top) <= f(t_top, u), so the crossing of u with s_top lies at or above
// t_top >= 0: the numerator g(u) - g(s) + w^2 (u^2 - s^2) is non-negative (< 2^34, formed in 64 bits with g(s) subtracted last) and the
// denominator 2 w^2 (u - s) is below 2^33; ONE exact 64-bit division per push.  Indices base + u stride lie in the line, hence in [0, n).
// No kernel uses scratch memory (tests/test_distance_weighted_cpu.py reads the listing).
#include <utility>

#include "box_domain.hpp"

using namespace vkv;

// edt.hip's: target bits by wave ballot, one 64-bit word per entry
__global__ void k_edt_bits(BoxLinear G, uint32_t outside, uint64_t *__restrict__ bits);

// edt.hip's k_edt_x with a weight: the row's bits are [i - x, i - x + bw), of which [i - min(x, reach), i + min(bw - 1 - x, reach)] is searched.
// The walk is a copy: shared through a header it changed k_edt_x's listing, and edt.hip's code objects are not to change
__global__ void __launch_bounds__(256) k_env_x(BoxLinear G, const uint64_t *__restrict__ bits, uint32_t *__restrict__ out, uint32_t limit, uint32_t reach, uint32_t w)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)        // no wave-wide operation below
		return;
	const uint32_t lo = v.i - min(v.x, reach), hi = v.i + min(G.bw - 1u - v.x, reach);        // lo <= i <= hi < n
	uint32_t       dx = 0xffffffffu;
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
				break;
			}
			if (last)
				break;
			m = bits[--wd];
		}
	}
	if (dx != 0u)
	{        // the lowest target bit in [i, end]: nothing further than dx - 1 can win.  end <= hi < n: no wrap
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
				break;
			}
			if (last)
				break;
			m = bits[++wd];
		}
	}
	// dx <= bw - 1 where a target was found: w dx <= 65535 (a weight above 65535 comes with bw == 1, dx == 0)
	const uint32_t wdx = w * (dx == 0xffffffffu ? 0u : dx);
	out[v.i]           = dx == 0xffffffffu ? limit : min(wdx * wdx, limit);
}

// f(p, i) = g(i) + (w (p - i))^2, below 2^33
__device__ __forceinline__ uint64_t env_f(uint32_t p, uint32_t i, uint32_t g, uint32_t w)
{
	const uint32_t wd = w * (p > i ? p - i : i - p);        // at most 65535
	return (uint64_t) g + wd * wd;
}

// one axis pass: lane L owns line L of the n / len lines of `len` voxels `stride` apart; src and dst are the two distance buffers, never the same
__global__ void __launch_bounds__(256) k_env_axis(uint32_t lines, uint32_t stride, uint32_t len, uint32_t w, uint32_t limit, const uint32_t *__restrict__ src,
                                                  uint32_t *dst)
{
	const uint32_t L = blockIdx.x * 256u + threadIdx.x;
	if (L >= lines)
		return;
	const uint32_t base = (L / stride) * stride * len + L % stride;        // the line's first voxel: below n
	const uint64_t w2   = (uint64_t) w * w;
	uint32_t       k = 0, s = 0, t = 0, gs = 0;        // entries on the stack, and the top entry with g(s) while k > 0
	// forward: the lower envelope of the uncapped parabolas
	uint32_t next = src[base];
	for (uint32_t u = 0; u < len; ++u)
	{
		const uint32_t g = next;
		if (u + 1u < len)
			next = src[base + (u + 1u) * stride];        // in flight while u is worked on
		if (g >= limit)
			continue;
		while (k > 0u && env_f(t, s, gs, w) > env_f(t, u, g, w))        // u is lower from t on: the top is never the lowest
		{
			--k;
			if (k > 0u)
			{
				const uint32_t e = dst[base + (k - 1u) * stride];
				s = e & 0x7fffu, t = e >> 15;
				gs = src[base + s * stride];
			}
		}
		if (k == 0u)
			t = 0;
		else
		{        // the first position at which u is lower than the top: 1 + floor(the crossing), the crossing >= t
			const uint64_t num = (uint64_t) g + w2 * (uint64_t) (u * u - s * s) - gs, den = 2ull * w2 * (u - s);
			const uint64_t q   = num / den;
			if (q >= len - 1u)
				continue;        // past the line's end
			t = (uint32_t) q + 1u;
		}
		s = u, gs = g;
		dst[base + k * stride] = s | t << 15;        // k <= u
		++k;
	}
	// backward: position u takes its value from the top entry, which is popped where its range ends.  The bottom entry has t = 0: the stack
	// holds an entry until u = 0 is done.  Without an entry every g was the cap
	for (uint32_t u = len; u-- > 0u;)
	{
		uint32_t out = limit;
		if (k > 0u)
		{
			out = (uint32_t) min((uint64_t) limit, env_f(u, s, gs, w));
			if (u == t && --k > 0u)
			{        // entry k - 1 lies below position u: the store below does not touch it
				const uint32_t e = dst[base + (k - 1u) * stride];
				s = e & 0x7fffu, t = e >> 15;
				gs = src[base + s * stride];
			}
		}
		dst[base + u * stride] = out;
	}
}

namespace vkv
{

int launch_distance_transform_weighted(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, const uint32_t weights[3],
                                       uint32_t limit, void *d_scratch, uint32_t *d_dist2, hipStream_t s)
{
	BoxLinearPlan p;
	if (!edt_launch_ok(e, &b) || !box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "distance_transform_weighted: a box of more than 2^32 - 1 voxels or an axis above 32768");
	uint64_t     *bits  = static_cast<uint64_t *>(d_scratch);        // the block of edt_scratch_bytes(): [target bits][the second distance buffer]
	uint32_t     *other = reinterpret_cast<uint32_t *>(bits + p.entries);
	const BoxLinear G   = box_linear(d_vol, e, b, p, iso);
	const bool y = b.height > 1u, z = b.depth > 1u;
	uint32_t  *cur = (y != z) ? other : d_dist2, *nxt = (y != z) ? d_dist2 : other;        // one further pass: it starts in the scratch block
	hipLaunchKernelGGL(k_edt_bits, dim3(p.wgs), dim3(256), 0, s, G, target == VKV_DISTANCE_TO_OUTSIDE ? 1u : 0u, bits);
	hipLaunchKernelGGL(k_env_x, dim3(p.wgs), dim3(256), 0, s, G, bits, cur, limit, edt_weighted_reach(limit, weights[0]), weights[0]);
	if (y)
	{
		const uint32_t lines = p.n / b.height;
		hipLaunchKernelGGL(k_env_axis, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, b.width, b.height, weights[1], limit, cur, nxt);
		std::swap(cur, nxt);
	}
	if (z)
	{
		const uint32_t lines = b.width * b.height;
		hipLaunchKernelGGL(k_env_axis, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, lines, b.depth, weights[2], limit, cur, nxt);
		std::swap(cur, nxt);
	}
	return check_launch(ctx, "distance_transform_weighted");        // cur == d_dist2
}

}        // namespace vkv

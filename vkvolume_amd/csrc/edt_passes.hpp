// edt_passes.hpp — what the three exact distance transforms share (edt.hip, edt_envelope.hip, nearest.hip): the
// walk along a row's target bits (k_edt_x, k_env_x; k_near_x keeps a copy, noted there), the lower-envelope pass of one line (k_env_axis, k_near_axis<1>, <2>), the declaration
// of k_edt_bits, and on the host the schedule of the passes over the scratch block and the caller's buffer.  k_edt_axis (edt.hip) is another
// algorithm and is not here.  profiles/edt_family_refactor.txt has every kernel's figures against the copies this header replaced.
#pragma once

#include <utility>

#include "box_domain.hpp"

// edt.hip's: target bits by wave ballot, one 64-bit word per entry; launched by all three transforms
__global__ void k_edt_bits(vkv::BoxLinear G, uint32_t outside, uint64_t *__restrict__ bits);

namespace vkv
{

// ---- the x pass: the distance along the voxel's own row to the nearest target bit, 0xffffffff for none within `reach`.
// The row's bits are [i - x, i - x + bw), of which [i - min(x, reach), i + min(bw - 1 - x, reach)] is searched: clz / ctz in the
// lane's own word, then whole words outward, at most min(bw, reach) / 64 + 2 words per side.  TIES: the search to the right goes up to dx - 1
// only, so the left target keeps a tie.  No wave-wide operation: the caller has returned for a lane past the box
__device__ __forceinline__ uint32_t row_walk(const BoxLinear &G, const BoxVoxel &v, const uint64_t *__restrict__ bits, uint32_t reach)
{
	const uint32_t lo = v.i - min(v.x, reach), hi = v.i + min(G.bw - 1u - v.x, reach);        // lo <= i <= hi < n
	uint32_t       dx = 0xffffffffu;
	{        // the highest target bit in [lo, i]
		uint32_t w = v.i >> 6;
		uint64_t m = bits[w] & (~0ull >> (63u - (v.i & 63u)));
		for (;;)        // w falls to lo >> 6 at the latest
		{
			const bool last = w == lo >> 6;
			if (last)
				m &= ~0ull << (lo & 63u);
			if (m)
			{
				dx = v.i - (w * 64u + 63u - (uint32_t) __clzll((long long) m));
				break;
			}
			if (last)
				break;
			m = bits[--w];
		}
	}
	if (dx != 0u)
	{        // the lowest target bit in [i, end]: nothing further than dx - 1 can win.  end <= hi < n: no wrap
		const uint32_t end = v.i + min(hi - v.i, dx - 1u);
		uint32_t       w   = v.i >> 6;
		uint64_t       m   = bits[w] & (~0ull << (v.i & 63u));
		for (;;)        // w rises to end >> 6 at the latest
		{
			const bool last = w == end >> 6;
			if (last)
				m &= ~0ull >> (63u - (end & 63u));
			if (m)
			{
				dx = w * 64u + (uint32_t) __builtin_ctzll(m) - v.i;
				break;
			}
			if (last)
				break;
			m = bits[++w];
		}
	}
	return dx;        // <= bw - 1 <= 32767 where a target was found
}

// (w |a - b|)^2 for positions a, b of one axis: w |a - b| is at most 65535 (edt_weights_fit, host_arith.hpp), the square below 2^32
__device__ __forceinline__ uint32_t edt_wd2(uint32_t w, uint32_t a, uint32_t b)
{
	const uint32_t wd = w * (a > b ? a - b : b - a);
	return wd * wd;
}

// f(p, i) = g(i) + (w (p - i))^2, below 2^33
__device__ __forceinline__ uint64_t env_f(uint32_t p, uint32_t i, uint32_t g, uint32_t w)
{
	const uint32_t d2 = edt_wd2(w, p, i);        // first: g may still be on its way from memory
	return (uint64_t) g + d2;
}

// ---- an axis pass: out(p) = min over the positions p' of the line that take part of f(p, p') = g(p') + (w (p - p'))^2, for the line of `len`
// voxels `stride` apart that starts at `base`.  ONE LINE PER LANE, consecutive lanes on consecutive x: every lane of a wave is at the same
// position u of its line, so the wave's loads and stores run along x.  Forward over u it builds the lower envelope of the parabolas as a stack
// of (s, t): parabola s is the lowest from position t on, t strictly increasing from 0.  Backward over u it reads the value off the top entry
// and pops where u == t.  What a position holds is the Carry's business:
//   carry.skips(e)            the element e of src takes no part (a capped distance, no feature)
//   carry.g(e)                g of an element that takes part, below 2^32
//   carry.none(), carry.value(s, e, f), carry.store(dst, i, out)      the backward sweep's store at index i: none() where no position of
//                             the line takes part, else value() of the winning position s, which holds e, at f = f(u, s) < 2^33
// THE STACK LIVES IN THE OUTPUT LINE.  Entry k is the uint32 s | t << 15 (s, t <= 32767) at position k of the line in dst, which the backward
// sweep overwrites; src and dst are never the same buffer.  Forward: the entries hold distinct s < u, so k <= u, and dst is not yet written.
// Backward: t is strictly increasing from t_0 = 0, so k <= t_k <= u for the top entry k; the store at u hits an entry only when u = k = t_k:
// the top itself, which is held in registers (s, t, its element es and g(s)) and is popped by that very step.  So a pass needs no scratch.
// TIES go to the smaller position: the pop test is a strict > (a parabola that only ties at t stays) and a range starts at 1 + floor(the
// crossing) (the older, smaller s keeps the crossing itself).  A popped s is strictly above u at t and everywhere after, and was above its
// predecessors before t: it wins nowhere, ties included.
// LOOP BOUNDS.  Every position is pushed at most once and popped at most once: at most 2 len forward iterations (len steps of u plus len
// pops) and len backward, len <= 32768.  No lane waits for another lane, wave or workgroup; no atomics.
// NO OVERFLOW.  w (len - 1) <= 65535, so f = g + (w d)^2 < 2^33 in 64 bits.  The pop test compares two f and does not divide.  After the pops
// f(t_top, s_top) <= f(t_top, u), so the crossing of u with s_top lies at or above t_top >= 0: the numerator g(u) - g(s) + w^2 (u^2 - s^2) is
// non-negative (< 2^34, formed in 64 bits with g(s) subtracted last) and the denominator 2 w^2 (u - s) is below 2^33; ONE exact 64-bit
// division per push.  Indices base + u stride lie in the line, hence in [0, n).
// The body is plain statements on purpose: with the pop and f as local lambdas the three kernels grew by 28 to 72 bytes of code and the
// transforms ran 0.5 to 4 % slower; and env_f squares before it touches g because the other order cost k_env_axis 0.7 to 1 % where stacks are
// dense (profiles/edt_family_refactor.txt).
template <typename Carry>
__device__ __forceinline__ void envelope_line(uint32_t base, uint32_t stride, uint32_t len, uint32_t w, const Carry &carry, const uint32_t *__restrict__ src,
                                              uint32_t *dst)
{
	const uint64_t w2 = (uint64_t) w * w;
	uint32_t       k = 0, s = 0, t = 0, gs = 0, es = 0;        // entries on the stack, and the top entry with its element and g(s) while k > 0
	// forward: the lower envelope of the parabolas of the positions that take part
	uint32_t next = src[base];
	for (uint32_t u = 0; u < len; ++u)
	{
		const uint32_t eu = next;
		if (u + 1u < len)
			next = src[base + (u + 1u) * stride];        // in flight while u is worked on
		if (carry.skips(eu))
			continue;
		const uint32_t g = carry.g(eu);
		while (k > 0u && env_f(t, s, gs, w) > env_f(t, u, g, w))        // u is STRICTLY lower from t on: the top is never the lowest, nor ties
		{
			--k;
			if (k > 0u)
			{
				const uint32_t e = dst[base + (k - 1u) * stride];
				s = e & 0x7fffu, t = e >> 15;
				es = src[base + s * stride];
				gs = carry.g(es);
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
		s = u, gs = g, es = eu;
		dst[base + k * stride] = s | t << 15;        // k <= u
		++k;
	}
	// backward: position u takes its value from the top entry, which is popped where its range ends.  The bottom entry has t = 0: the stack
	// holds an entry until u = 0 is done
	for (uint32_t u = len; u-- > 0u;)
	{
		auto out = carry.none();
		if (k > 0u)
		{
			out = carry.value(s, es, env_f(u, s, gs, w));
			if (u == t && --k > 0u)
			{        // entry k - 1 lies below position u: the store below does not touch it
				const uint32_t e = dst[base + (k - 1u) * stride];
				s = e & 0x7fffu, t = e >> 15;
				es = src[base + s * stride];
				gs = carry.g(es);
			}
		}
		carry.store(dst, base + u * stride, out);
	}
}

// ---- host side: the schedule of a transform's passes.  The scratch block is [target bits: u64 x entries][the second buffer: u32 x voxels], an
// entry = 64 voxels: 4 bytes and one bit per voxel, the bits rounded up to 8 bytes.  The two 4-byte buffers are the caller's output and the
// block's; a y or z pass reads one and writes the OTHER (a line's outputs need its inputs), and a pass over an axis of length 1 is not
// launched.  PARITY: the x pass writes the buffer that makes the last pass land in the caller's, passes = 1 + y + z, so it starts in the
// scratch block when exactly one further pass runs.  Every pass writes every element of its output, so nothing depends on what the buffers
// held before, and two runs give the same bytes.  The family's own limit: no box axis above 32768 (positions fit 15 bits, squares 2^30)
struct EdtSchedule
{
	BoxLinearPlan p{};
	uint64_t     *bits = nullptr;
	uint32_t     *cur = nullptr, *nxt = nullptr;        // the x pass writes cur; each further pass reads cur, writes nxt, and the two swap
	bool          y = false, z = false;                 // which of the axis passes run

	// false: the extent and box are not accepted.  d_scratch null: for the size alone
	bool lay(VkvExtent3D e, const VkvBox *box, void *d_scratch, uint32_t *out)
	{
		if (!box_linear_plan(e, box, p))
			return false;
		const VkvBox b = whole_or(e, box);
		if (b.width > 32768u || b.height > 32768u || b.depth > 32768u)
			return false;
		y = b.height > 1u, z = b.depth > 1u;
		if (d_scratch)
		{
			bits            = static_cast<uint64_t *>(d_scratch);
			uint32_t *other = reinterpret_cast<uint32_t *>(bits + p.entries);
			cur = (y != z) ? other : out, nxt = (y != z) ? out : other;
		}
		return true;
	}
	size_t bytes() const { return 8 * (size_t) p.entries + 4 * (size_t) p.n; }

	// y then z: pass(src, dst) launches one; afterwards cur is the caller's buffer
	template <typename YPass, typename ZPass>
	void axes(YPass y_pass, ZPass z_pass)
	{
		if (y)
		{
			y_pass((const uint32_t *) cur, nxt);
			std::swap(cur, nxt);
		}
		if (z)
		{
			z_pass((const uint32_t *) cur, nxt);
			std::swap(cur, nxt);
		}
	}
};

// the launchers' opening: 0, or the one rejection under the entry point's name
inline int edt_schedule(vkv_ctx *ctx, const char *name, VkvExtent3D e, const VkvBox &b, void *d_scratch, uint32_t *out, EdtSchedule &S)
{
	if (S.lay(e, &b, d_scratch, out))
		return 0;
	return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a box of more than 2^32 - 1 voxels or an axis above 32768", name);
}

}        // namespace vkv

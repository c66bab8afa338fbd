// edt_envelope.hip — the squared Euclidean distance transform with an integer weight per axis (vkv_distance_transform_weighted), by lower
// envelopes; DESIGN.md §5.18.  d_dist2[v] = min(limit, min over the targets u of (wx dx)^2 + (wy dy)^2 + (wz dz)^2): voxel spacing as a ratio
// of small integers.  Targets, the box-linear domain and the cap are those of edt.hip; the row walk, the envelope pass with its invariants
// (the stack in the output line, loop bounds, no overflow, one exact 64-bit division per push), k_edt_bits' declaration and the schedule of
// the passes over the two ping-pong buffers are edt_passes.hpp's.  Integer work only.
//   k_env_x      g(i) = min(limit, (wx dx)^2): row_walk with reach = the smallest r with (wx r)^2 >= limit.
//   k_env_axis   out(p) = min(limit, min over p' of the line of g(p') + (w (p - p'))^2) for y (stride bw) and then z (stride bw bh): envelope_line
//                over capped distances.  A capped g(u) = limit is skipped: min(limit, limit + b) = limit.
// NO OVERFLOW.  The entry point admits weights only where every w (len - 1) <= 65535 and the sum of their squares is at most 0xfffffffe
// (edt_weights_fit, host_arith.hpp): w d <= 65535 and (w d)^2 < 2^32 in 32 bits, g <= 0xffffffff, which is what envelope_line asks for.
// No kernel uses scratch memory (tests/test_distance_weighted_cpu.py reads the listing).
#include "edt_passes.hpp"

using namespace vkv;

__global__ void __launch_bounds__(256) k_env_x(BoxLinear G, const uint64_t *__restrict__ bits, uint32_t *__restrict__ out, uint32_t limit, uint32_t reach, uint32_t w)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)        // no wave-wide operation below
		return;
	const uint32_t dx = row_walk(G, v, bits, reach);
	// dx <= bw - 1 where a target was found: w dx <= 65535 (a weight above 65535 comes with bw == 1, dx == 0)
	const uint32_t wdx = w * (dx == 0xffffffffu ? 0u : dx);
	out[v.i]           = dx == 0xffffffffu ? limit : min(wdx * wdx, limit);
}

// a position carries its capped distance: g is the value itself
struct DistanceCarry
{
	uint32_t limit;

	__device__ __forceinline__ bool     skips(uint32_t e) const { return e >= limit; }
	__device__ __forceinline__ uint32_t g(uint32_t e) const { return e; }
	__device__ __forceinline__ uint32_t none() const { return limit; }
	__device__ __forceinline__ uint32_t value(uint32_t, uint32_t, uint64_t f) const { return (uint32_t) min((uint64_t) limit, f); }
	__device__ __forceinline__ void     store(uint32_t *dst, uint32_t i, uint32_t out) const { dst[i] = out; }
};

// one axis pass: lane L owns line L of the n / len lines of `len` voxels `stride` apart; src and dst are the two distance buffers, never the same
__global__ void __launch_bounds__(256) k_env_axis(uint32_t lines, uint32_t stride, uint32_t len, uint32_t w, uint32_t limit, const uint32_t *__restrict__ src,
                                                  uint32_t *dst)
{
	const uint32_t L = blockIdx.x * 256u + threadIdx.x;
	if (L >= lines)
		return;
	const uint32_t base = (L / stride) * stride * len + L % stride;        // the line's first voxel: below n
	envelope_line(base, stride, len, w, DistanceCarry{limit}, src, dst);
}

namespace vkv
{

int launch_distance_transform_weighted(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, const uint32_t weights[3],
                                       uint32_t limit, void *d_scratch, uint32_t *d_dist2, hipStream_t s)
{
	EdtSchedule S;
	if (const int rc = edt_schedule(ctx, "distance_transform_weighted", e, b, d_scratch, d_dist2, S))
		return rc;
	const BoxLinear G = box_linear(d_vol, e, b, S.p, iso);
	hipLaunchKernelGGL(k_edt_bits, dim3(S.p.wgs), dim3(256), 0, s, G, target == VKV_DISTANCE_TO_OUTSIDE ? 1u : 0u, S.bits);
	hipLaunchKernelGGL(k_env_x, dim3(S.p.wgs), dim3(256), 0, s, G, S.bits, S.cur, limit, edt_weighted_reach(limit, weights[0]), weights[0]);
	const auto pass = [&](uint32_t lines, uint32_t stride, uint32_t len, uint32_t w, const uint32_t *src, uint32_t *dst) {
		hipLaunchKernelGGL(k_env_axis, dim3((lines + 255u) / 256u), dim3(256), 0, s, lines, stride, len, w, limit, src, dst);
	};
	S.axes([&](const uint32_t *src, uint32_t *dst) { pass(S.p.n / b.height, b.width, b.height, weights[1], src, dst); },
	       [&](const uint32_t *src, uint32_t *dst) { pass(b.width * b.height, b.width * b.height, b.depth, weights[2], src, dst); });
	return check_launch(ctx, "distance_transform_weighted");
}

}        // namespace vkv

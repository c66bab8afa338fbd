// host_arith.hpp — the library's pure host arithmetic (host_arith.cpp): what the .hip files of csrc call from it.  Plain C++, no HIP: the
// same sources link into a stand-alone program (tests/host_arith_driver.cpp).  The extern "C" helpers of include/vkvolume_amd.h that
// never touch a device (uniforms, transfer-function texture, loader, vkv_screen_tile_rect) are defined there as well.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/vkvolume_amd.h"

namespace vkv
{
static inline bool extent_ok(VkvExtent3D e) { return e.width > 0 && e.height > 0 && e.depth > 0; }
// ceil(volume / map) must reproduce a valid block size (src/compute_distance_map.cpp:110-113)
static inline bool map_extent_ok(VkvExtent3D e, VkvExtent3D me) { return extent_ok(me) && me.width <= e.width && me.height <= e.height && me.depth <= e.depth; }
// voxels per map cell on one axis: ceil(extent / map extent)
static inline uint32_t block_of(uint32_t e, uint32_t m) { return (e + m - 1) / m; }

// a byte as a sample value: f = (float) byte * kInv255
constexpr float kInv255 = 1.0f / 255.0f;
// The inside threshold of iso: the smallest byte b with (float) b * kInv255 >= iso (the renderer's hit rule on a voxel's own value; the product
// is monotone in b), 256 where there is none.  The meshes, the components and the distance transform all take their inside rule from here.
static inline uint32_t iso_threshold(float iso)
{
	uint32_t thr = 0;
	while (thr < 256u && !((float) thr * kInv255 >= iso))
		++thr;
	return thr;
}

// ---- vkv_distance_transform_weighted (csrc/edt_envelope.hip): what the entry point works out before it enqueues anything -----------------
// The weights (wx, wy, wz) are accepted for a box of (bw, bh, bd) voxels iff none is 0 and the largest value that can occur,
// sum over the axes of (w (len - 1))^2, is at most 0xfffffffe (one below VKV_DISTANCE_NONE).  No step wraps: each w (len - 1) is held to 65535 in 64 bits
// first, so each square is below 2^32 and the sum of three is formed in 64 bits.  An axis of length 1 admits every weight but 0.
bool edt_weights_fit(const uint32_t weights[3], uint32_t bw, uint32_t bh, uint32_t bd);
// the x pass's reach: the smallest r with (w r)^2 >= limit, w >= 1: a target further away along the row gives the cap anyway.  At most 65536
uint32_t edt_weighted_reach(uint32_t limit, uint32_t w);

// ---- launch-uniform arithmetic of the ray-march kernels, done once on the host (fill_render_args) ---------------------------------------
#if defined(__HIPCC__)        // (always inlined: a kernel built with target attributes of its own cannot inline a plain function, and a call costs it a stack)
#define VKV_HOST_DEVICE __host__ __device__ inline __attribute__((always_inline))
#else
#define VKV_HOST_DEVICE static inline
#endif
// Division of a u32 below 2^30 by a launch-uniform divisor d >= 1 without a division: q = mulhi(n << 2, mul) >> shift, with shift = ceil(log2 d)
// and mul = ceil(2^(30 + shift) / d), in [2^30, 2^31).  Exact: mul = (2^(30 + shift) + e) / d with 0 <= e < d <= 2^shift, so n * mul / 2^(30 + shift) =
// n / d + n e / (d 2^(30 + shift)), and the second term is below 1 / d for n < 2^30 - too small to carry n / d over the next integer.  d = 1 gives
// mul = 2^30, shift = 0: the same path (no special case, no correction round).  Numerators: fill_render_args admits at most 0x3fffffff blocks
// and 2^30 - 1 output indices per launch.  In a kernel both operands are wave-uniform: three scalar instructions for the quotient (shift, s_mul_hi_u32,
// shift) and a multiply and a subtraction for the remainder.  tests/test_uniform_div_cpu.py checks it against / and %.
struct UniformDiv
{
	uint32_t mul, shift;
};
constexpr uint32_t kUniformDivMax = 0x3fffffffu;        // the largest numerator
static inline UniformDiv uniform_div_of(uint32_t d)
{
	if (d == 0u)
		return {0u, 0u};        // a divisor nobody divides by (a launch with nothing to fill): the quotient is 0
	uint32_t shift = 0;
	while (shift < 31u && (1u << shift) < d)
		++shift;
	const uint64_t p = 1ull << (30u + shift);
	return {(uint32_t) ((p + d - 1u) / d), shift};
}
VKV_HOST_DEVICE uint32_t uniform_quot(uint32_t n, const UniformDiv &v) { return (uint32_t) (((uint64_t) (n << 2) * v.mul) >> 32) >> v.shift; }
// n = q * d + r
VKV_HOST_DEVICE void uniform_divmod(uint32_t n, uint32_t d, const UniformDiv &v, uint32_t &q, uint32_t &r)
{
	q = uniform_quot(n, v);
	r = n - q * d;
}
// frag:192 volume_to_distance_map_u, one axis: map cells per unit of the texture coordinate.  The kernels used to divide per wave; the host code
// is built with -ffp-contract=off and the device divides with correct rounding, so these are the same bits.  Kept as the plain expressions:
// tests/test_uniform_div_cpu.py holds them to that.
static inline float cells_per_unit(int extent, float block_size) { return (float) extent / block_size; }
// the clamp-free march loop's margin g (lean_free_wave): a quarter of a voxel of the longest axis, in texture coordinates
static inline float clamp_free_margin(int W, int H, int D)
{
	const int m = W > H ? (W > D ? W : D) : (H > D ? H : D);
	return 0.25f / (float) m;
}

// ---- start-order feedback: when a registered target is measured again and when its measured order may be used (raymarch.hip attaches the
// buffers; vkv_ctx::TileFeedback holds a state per target).  No device, no lock: the caller holds the context's mutex.
// the view of a frame: its central ray (normalised) and the camera position, both in texture space
struct FrameView
{
	float dir[3] = {0, 0, 0}, pos[3] = {0, 0, 0};
};
FrameView frame_view(const float dir00[3], const float ddx[3], const float ddy[3], const float cam[3], uint32_t img_w, uint32_t img_h);
struct FeedbackState
{
	bool      has_cost = false;        // a frame has been rendered into this target with the cost buffer attached
	uint32_t  frames = 0;              // frames rendered into this target so far
	uint32_t  measured_at = 0;         // value of `frames` at the last measured frame
	uint32_t  period = 8;              // frames until the next measurement (doubles while no frame can use the measured order)
	uint32_t  used = 0;                // frames since the last measurement that started in its order
	FrameView measured, prev;          // the view of the measured frame, and of the previous frame into the target (measured or not)
	bool      has_prev = false;
};
struct FeedbackStep
{
	bool use_order;        // start this frame's tiles in the order the last measurement left
	bool measure;          // attach the cost buffer to this frame and sort behind it
};
// one frame into the target; base_period = max(1, VkvTuning.feedback_period)
FeedbackStep feedback_step(FeedbackState &f, const FrameView &view, uint32_t base_period);

// Range checks of a tuning block, shared by vkv_set_tuning (which rejects a bad block) and default_tuning (which falls back to the
// built-in value of a field the environment set out of range).  Returns null when the block is fine, else what is wrong with it.
const char *tuning_problem(const VkvTuning &t);
// full_table_lds_limit at most max_dynamic_lds (what a kernel may ask for as dynamic LDS)
void clamp_tuning(VkvTuning &t, uint32_t max_dynamic_lds);
// defaults of the tuning block, then the environment (read HERE, once per context, and nowhere else)
void default_tuning(VkvTuning &t, uint32_t max_dynamic_lds);
// opacity-correction table keyed by the TF alpha byte (frag:283):
// lut[a] = clamp(voxel_alpha_factor * (1 - pow(1 - a/255, 1/sampling_factor)), 0, 1)
void build_alpha_lut(const VkvTransferFunctionUniform &tf, float *lut);
// the tile rectangle a caller passed (NULL / empty: every tile of the image), checked against the image; false = it runs past the image
bool resolve_rect(const VkvTileRect *rect, uint32_t image_width, uint32_t image_height, uint32_t tile_width, uint32_t tile_height, VkvTileRect &out);
// Start order of the schedule entries k = 0 .. count - 1 (entry k is tile first + k * stride of the image's tiles): by the distance of the
// tile's centre from the image centre, ties in index order; then the tile mix, in groups of eight.
std::vector<uint32_t> start_order(uint32_t img_w, uint32_t img_h, uint32_t tile_w, uint32_t tile_h, uint32_t first, uint32_t stride, uint32_t count,
                                  float mix_heavy, float mix_spread);
// Conservative pixel bound {x0, x1, y0, y1} of the clipped unit box as the kernel's ray generator sees it (host_arith.cpp explains it)
enum { kScreenBoundNone = 0 /* no statement */, kScreenBoundEmpty = 1 /* nothing can be seen */, kScreenBoundRect = 2 };
int screen_bound(const float cam[3], const float dir00[3], const float ddx[3], const float ddy[3], const float plane_tex[4], double out[4]);
// vkv_screen_tile_rect: the same bound in whole tiles
void screen_tile_rect(const VkvRayCastUniform *rc, const VkvRayGen *rg, uint32_t iw, uint32_t ih, uint32_t tw, uint32_t th, uint32_t align, VkvTileRect *out);
}        // namespace vkv

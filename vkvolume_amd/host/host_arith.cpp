// host_arith.cpp — the library's pure host arithmetic: the extern "C" helpers of include/vkvolume_amd.h that never touch a device, and what
// the context, the entry points and the ray-march launchers work out on the host (host_arith.hpp).  Plain C++, no HIP.
#include "host_arith.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>

#include "load_volume.h"
#include "vkv_math.hpp"

namespace vkv
{
// a tile mix that is not a number never compares equal to a cached schedule's: every launch would build a new table
static bool tile_mix_ok(const VkvTuning &t)
{
	return std::isfinite(t.tile_mix_heavy) && std::isfinite(t.tile_mix_spread) && t.tile_mix_heavy >= 0.0f && t.tile_mix_heavy <= 1.0f && t.tile_mix_spread >= 0.0f &&
	       t.tile_mix_spread <= 1.0f;
}

bool edt_weights_fit(const uint32_t weights[3], uint32_t bw, uint32_t bh, uint32_t bd)
{
	const uint32_t len[3] = {bw, bh, bd};
	uint64_t       sum    = 0;
	for (int a = 0; a < 3; ++a)
	{
		if (weights[a] == 0u || len[a] == 0u)
			return false;
		const uint64_t far = (uint64_t) weights[a] * (len[a] - 1u);        // below 2^64
		if (far > 65535u)
			return false;
		sum += far * far;        // three terms below 2^32
	}
	return sum <= 0xfffffffeull;
}

uint32_t edt_weighted_reach(uint32_t limit, uint32_t w)
{
	uint64_t root = 0;        // the smallest root with root^2 >= limit: at most 65536
	while (root * root < limit)
		++root;
	return (uint32_t) ((root + w - 1u) / w);        // (w r)^2 >= limit iff w r >= root
}

const char *tuning_problem(const VkvTuning &t)
{
	if (t.scheduler < 0 || t.scheduler > 1 || t.batch_mode < 0 || t.batch_mode > 1 || t.address_tables < 0 || t.address_tables > 2 || t.feedback_period == 0 ||
	    t.gradient_segment > 255u || t.clamp_always < 0 || t.clamp_always > 1 ||
	    (t.wave_shape != 0 && t.wave_shape != 4 && t.wave_shape != 8 && t.wave_shape != 16))
		return "field out of range";
	if (!tile_mix_ok(t))
		return "tile_mix_heavy / tile_mix_spread must be numbers in [0, 1]";
	return nullptr;
}

// the kernels request their whole LDS layout as dynamic LDS without raising the 64 KiB default limit: a larger figure would make every
// launch fail instead of choosing the smaller tables
void clamp_tuning(VkvTuning &t, uint32_t max_dynamic_lds) { t.full_table_lds_limit = std::min<uint32_t>(t.full_table_lds_limit, max_dynamic_lds); }

void default_tuning(VkvTuning &t, uint32_t max_dynamic_lds)
{
	std::memset(&t, 0, sizeof(t));
	t.struct_size          = (uint32_t) sizeof(VkvTuning);
	t.address_tables       = 2;
	t.full_table_lds_limit = 17920;        // = kFullLdsLimit (raymarch_core.hpp): 9 workgroups per CU
	t.screen_cull          = 1;
	t.feedback             = 1;
	t.feedback_period      = 8;
	t.arena_bytes          = 8u << 20;
	auto env = [](const char *name) -> const char * { const char *e = std::getenv(name); return (e && e[0]) ? e : nullptr; };
	if (const char *e = env("VKV_RAYMARCH_SCHEDULER"))
		t.scheduler = e[0] == 'p';
	if (const char *e = env("VKV_RAYMARCH_BATCH"))
		t.batch_mode = e[0] == 'p';
	if (const char *e = env("VKV_RAYMARCH_BATCH_ORDER"))
		t.batch_sequential = e[0] == 's';
	if (const char *e = env("VKV_RAYMARCH_TILE_ORDER"))
		t.tile_order_linear = e[0] == 'l';
	if (const char *e = env("VKV_RAYMARCH_LUT"))
		t.address_tables = e[0] == '0' ? 0 : (e[0] == '2' ? 1 : 2);
	if (const char *e = env("VKV_RAYMARCH_FULL_LIMIT"))
		t.full_table_lds_limit = (uint32_t) std::max(0l, std::atol(e));
	if (const char *e = env("VKV_RAYMARCH_CULL"))
		t.screen_cull = e[0] != '0';
	if (const char *e = env("VKV_RAYMARCH_FEEDBACK"))
		t.feedback = e[0] != '0';
	if (const char *e = env("VKV_RAYMARCH_FEEDBACK_PERIOD"))
		t.feedback_period = (uint32_t) std::max(1l, std::atol(e));
	if (const char *e = env("VKV_RAYMARCH_TILE_MIX"))
	{
		double h = 0.0, sp = 0.0;
		if (std::sscanf(e, "%lf,%lf", &h, &sp) == 2)
			t.tile_mix_heavy = (float) h, t.tile_mix_spread = (float) sp;
	}
	if (const char *e = env("VKV_GRADIENT_SEGMENT"))
		t.gradient_segment = (uint32_t) std::min(std::max(std::atol(e), 0l), 255l);
	if (const char *e = env("VKV_ARENA_BYTES"))
		t.arena_bytes = (uint32_t) std::min(std::max(std::atol(e), 1l << 20), 1l << 30);
	if (const char *e = env("VKV_RAYMARCH_CLAMP"))
		t.clamp_always = e[0] == 'a';
	if (const char *e = env("VKV_RAYMARCH_WAVE_SHAPE"))
	{
		const int v = std::atoi(e);
		t.wave_shape = (v == 4 || v == 8 || v == 16) ? v : 0;
	}
	// the environment gets the checks vkv_set_tuning applies: an out-of-range tile mix falls back to the built-in default of its group
	clamp_tuning(t, max_dynamic_lds);
	if (!tile_mix_ok(t))
		t.tile_mix_heavy = t.tile_mix_spread = 0.0f;
}

void build_alpha_lut(const VkvTransferFunctionUniform &tf, float *lut)
{
	const float sf_inv = 1.0f / tf.sampling_factor;
	for (int a = 0; a < 256; ++a)
	{
		const float v = tf.voxel_alpha_factor * (1.0f - std::pow(1.0f - (float) a / 255.0f, sf_inv));
		lut[a]        = std::min(std::max(v, 0.0f), 1.0f);
	}
}

bool resolve_rect(const VkvTileRect *rect, uint32_t image_width, uint32_t image_height, uint32_t tile_width, uint32_t tile_height, VkvTileRect &out)
{
	const uint32_t tiles_x = (image_width + tile_width - 1) / tile_width, tiles_y = (image_height + tile_height - 1) / tile_height;
	if (!rect || rect->w == 0 || rect->h == 0)
	{
		out = VkvTileRect{0u, 0u, tiles_x, tiles_y};
		return true;
	}
	out = *rect;
	return (uint64_t) rect->x0 + rect->w <= tiles_x && (uint64_t) rect->y0 + rect->h <= tiles_y;
}

std::vector<uint32_t> start_order(uint32_t img_w, uint32_t img_h, uint32_t tile_w, uint32_t tile_h, uint32_t first, uint32_t stride, uint32_t count,
                                  float mix_heavy_f, float mix_spread_f)
{
	const uint32_t tiles_x = (img_w + tile_w - 1) / tile_w;
	std::vector<std::pair<double, uint32_t>> key(count);
	for (uint32_t k = 0; k < count; ++k)
	{
		const uint64_t t  = (uint64_t) first + (uint64_t) k * stride;
		const double   cx = ((double) (t % tiles_x) + 0.5) * tile_w - 0.5 * img_w, cy = ((double) (t / tiles_x) + 0.5) * tile_h - 0.5 * img_h;
		key[k]            = {cx * cx + cy * cy, k};
	}
	std::stable_sort(key.begin(), key.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
	std::vector<uint32_t> order(count);
	for (uint32_t r = 0; r < count; ++r)
		order[r] = key[r].second;
	// experiment (VkvTuning.tile_mix_heavy / tile_mix_spread): the central <heavy share> of the tiles is spread evenly over the first
	// <spread> of the start order, the remaining (border) tiles fill the gaps and the end
	const double mix_heavy = mix_heavy_f, mix_spread = mix_spread_f;
	if (mix_heavy > 0.0 && mix_heavy < 1.0 && mix_spread >= mix_heavy && mix_spread <= 1.0)
	{
		// in groups of eight ranks: rank r runs on XCD r & 7, so a group gives every XCD one tile of the same kind
		const uint32_t groups = count / 8, nh = (uint32_t) (mix_heavy * groups), span = (uint32_t) (mix_spread * groups);
		std::vector<uint32_t> mixed;
		mixed.reserve(count);
		uint32_t h = 0, l = nh;
		for (uint32_t r = 0; r < groups; ++r)
		{
			// heavy group number h is due at position h * span / nh
			const bool     take_heavy = h < nh && ((uint64_t) h * span <= (uint64_t) r * nh || l >= groups);
			const uint32_t g          = take_heavy ? h++ : l++;
			for (uint32_t j = 0; j < 8; ++j)
				mixed.push_back(order[g * 8 + j]);
		}
		for (uint32_t r = groups * 8; r < count; ++r)
			mixed.push_back(order[r]);
		order.swap(mixed);
	}
	return order;
}

// Conservative pixel bound of what a frame's fragments can see: the unit box [0,1]^3 (texture space) cut by the clipping plane (kept side:
// dot(plane_tex.xyz, p) + plane_tex.w >= 0 - ray_setup_impl starts a ray at t0 = max(t_box_near, t_plane) and needs t0 < t_box_far, so every
// fragment's ray holds a point of that clipped box), as seen through the ray generator of the kernel: pixel (px, py) looks along
// dir00 + (px + 0.5) ddx + (py + 0.5) ddy from cam, so a point c is seen at the (fx, fy) with c - cam = g (dir00 + fx ddx + fy ddy), g > 0.
// The clipped box is convex and the map to (fx, fy) keeps convexity in front of the camera: the bound is the min / max over its VERTICES - the
// box corners on the kept side and the points where the plane cuts an edge (the plane is moved outwards by 1e-4 of its normal's length
// first: the device evaluates in fp32) -, widened by two pixels (the device evaluates the direction in fp32: it can disagree with this
// double-precision solve by a tiny fraction of a pixel).  A vertex at or behind the camera plane, or a degenerate generator, disables it
// (kScreenBoundNone); no vertex at all = nothing can be seen (kScreenBoundEmpty).  With the application's plane (through a point in front of the
// camera, facing away from it) every vertex lies in front of the camera, also for a camera inside the box: round 6 - the bound of the
// un-clipped box (rounds 2-5) gave up there.  Pixels outside cannot have a fragment, whatever the depth test does afterwards.
int screen_bound(const float cam[3], const float dir00[3], const float ddx[3], const float ddy[3], const float plane_tex[4], double out[4])
{
	// inverse of M = [ddx ddy dir00] (columns) by the adjugate
	const double M[3][3] = {{ddx[0], ddy[0], dir00[0]}, {ddx[1], ddy[1], dir00[1]}, {ddx[2], ddy[2], dir00[2]}};
	double       inv[3][3], scale = 0.0;
	for (int i = 0; i < 3; ++i)
		for (int j = 0; j < 3; ++j)
		{
			const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
			inv[j][i]    = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1];        // cofactor (i, j) -> adjugate (j, i)
			scale        = std::max(scale, std::fabs(M[i][j]));
		}
	const double det = M[0][0] * inv[0][0] + M[0][1] * inv[1][0] + M[0][2] * inv[2][0];
	if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * scale * scale * scale))
		return kScreenBoundNone;
	// vertices of the clipped box
	double    vert[8 + 12][3];
	int       n_vert = 0;
	double    sd[8];        // signed plane values of the corners (+ the outward shift)
	bool      clip = plane_tex != nullptr;
	if (clip)
	{
		const double pn = std::sqrt((double) plane_tex[0] * plane_tex[0] + (double) plane_tex[1] * plane_tex[1] + (double) plane_tex[2] * plane_tex[2]);
		if (!std::isfinite(pn) || !(pn > 0.0) || !std::isfinite((double) plane_tex[3]))
			clip = false;        // no usable plane: the whole box
		for (int c = 0; c < 8 && clip; ++c)
			sd[c] = (double) plane_tex[0] * (c & 1) + (double) plane_tex[1] * ((c >> 1) & 1) + (double) plane_tex[2] * ((c >> 2) & 1) + (double) plane_tex[3] + 1e-4 * pn;
	}
	for (int c = 0; c < 8; ++c)
		if (!clip || sd[c] >= 0.0)
			vert[n_vert][0] = (double) (c & 1), vert[n_vert][1] = (double) ((c >> 1) & 1), vert[n_vert][2] = (double) ((c >> 2) & 1), ++n_vert;
	if (clip)
		for (int c = 0; c < 8; ++c)
			for (int axis = 0; axis < 3; ++axis)
			{
				const int d = c | (1 << axis);
				if (d == c || (sd[c] >= 0.0) == (sd[d] >= 0.0))
					continue;        // (each edge once: from its corner with the axis bit clear) the plane does not cut this edge
				const double u = sd[c] / (sd[c] - sd[d]);
				for (int k = 0; k < 3; ++k)
					vert[n_vert][k] = (double) ((c >> k) & 1) + u * ((double) ((d >> k) & 1) - (double) ((c >> k) & 1));
				++n_vert;
			}
	if (n_vert == 0)
		return kScreenBoundEmpty;
	double lo_x = 1e300, hi_x = -1e300, lo_y = 1e300, hi_y = -1e300;
	for (int i = 0; i < n_vert; ++i)
	{
		const double v[3] = {vert[i][0] - cam[0], vert[i][1] - cam[1], vert[i][2] - cam[2]};
		const double fa = (inv[0][0] * v[0] + inv[0][1] * v[1] + inv[0][2] * v[2]) / det, fb = (inv[1][0] * v[0] + inv[1][1] * v[1] + inv[1][2] * v[2]) / det;
		const double g  = (inv[2][0] * v[0] + inv[2][1] * v[1] + inv[2][2] * v[2]) / det;
		if (!(g > 1e-6) || !std::isfinite(fa) || !std::isfinite(fb))
			return kScreenBoundNone;        // a vertex beside or behind the camera: its projection says nothing
		lo_x = std::min(lo_x, fa / g), hi_x = std::max(hi_x, fa / g), lo_y = std::min(lo_y, fb / g), hi_y = std::max(hi_y, fb / g);
	}
	// pixel p is sampled at p + 0.5
	out[0] = std::floor(lo_x - 0.5) - 2.0, out[1] = std::ceil(hi_x - 0.5) + 2.0, out[2] = std::floor(lo_y - 0.5) - 2.0, out[3] = std::ceil(hi_y - 0.5) + 2.0;
	if (out[1] < 0.0 || out[3] < 0.0 || out[0] > 4.0e9 || out[2] > 4.0e9)
		return kScreenBoundEmpty;        // off screen
	return kScreenBoundRect;
}

// vkv_screen_tile_rect: the same bound in whole tiles
void screen_tile_rect(const VkvRayCastUniform *rc, const VkvRayGen *rg, uint32_t iw, uint32_t ih, uint32_t tw, uint32_t th, uint32_t align, VkvTileRect *out)
{
	const uint32_t tiles_x = (iw + tw - 1) / tw, tiles_y = (ih + th - 1) / th;
	*out = VkvTileRect{0u, 0u, tiles_x, tiles_y};
	double    b[4];
	const int kind = screen_bound(rc->camera_pos_tex, rg->dir00, rg->ddx, rg->ddy, rc->plane_tex, b);
	if (kind == kScreenBoundNone)
		return;
	if (kind == kScreenBoundEmpty || b[0] >= (double) iw || b[2] >= (double) ih)
	{
		*out = VkvTileRect{0u, 0u, 1u, 1u};
		return;
	}
	const uint32_t x0 = b[0] <= 0.0 ? 0u : (uint32_t) b[0], y0 = b[2] <= 0.0 ? 0u : (uint32_t) b[2];
	const uint32_t x1 = b[1] >= (double) (iw - 1) ? iw - 1 : (uint32_t) b[1], y1 = b[3] >= (double) (ih - 1) ? ih - 1 : (uint32_t) b[3];        // inclusive
	const uint32_t q = align > 1 ? align : 1u;
	uint32_t       tx0 = (x0 / tw) / q * q, ty0 = (y0 / th) / q * q;
	uint32_t       tx1 = std::min(tiles_x, (x1 / tw + q) / q * q), ty1 = std::min(tiles_y, (y1 / th + q) / q * q);        // exclusive
	*out = VkvTileRect{tx0, ty0, tx1 - tx0, ty1 - ty0};
}

// ---- start-order feedback ---------------------------------------------------------------------------------------------------------
FrameView frame_view(const float dir00[3], const float ddx[3], const float ddy[3], const float cam[3], uint32_t img_w, uint32_t img_h)
{
	FrameView v;
	float     len2 = 0.0f;
	for (int i = 0; i < 3; ++i)
	{
		v.dir[i] = dir00[i] + 0.5f * ((float) img_w * ddx[i] + (float) img_h * ddy[i]);
		len2 += v.dir[i] * v.dir[i];
	}
	const float inv = len2 > 0.0f ? 1.0f / std::sqrt(len2) : 0.0f;
	for (int i = 0; i < 3; ++i)
		v.dir[i] *= inv, v.pos[i] = cam[i];
	return v;
}

// Costs measured on a view that was more than ~12 degrees away (or from a camera that has moved by more than a fifth of its distance to the
// volume's centre) say little about this frame - an order sorted by them scatters the heavy tiles (measured: -3 % for targets that alternate
// between views 45 degrees apart).
static bool view_close(const FrameView &v, const FrameView &to)
{
	float cosine = 0.0f, moved2 = 0.0f, dist2 = 0.0f;
	for (int i = 0; i < 3; ++i)
	{
		cosine += v.dir[i] * to.dir[i];
		moved2 += (v.pos[i] - to.pos[i]) * (v.pos[i] - to.pos[i]);
		dist2 += (to.pos[i] - 0.5f) * (to.pos[i] - 0.5f);
	}
	return cosine >= 0.978f && moved2 <= 0.04f * dist2;
}

// Costs are measured (and sorted behind the render) on the first frame into a target and then every `period`-th one: a camera that moves
// little keeps the order good for a few frames, and the sort kernel + the cost atomics are then paid once per period.  A frame whose view
// is not close to the MEASURED view (stale) starts centre-first.  A target is only measured again while its camera holds still or moves
// slowly - this frame's view close to the PREVIOUS frame into the target (steady): a camera that moves fast between a target's frames (24
// targets in flight and one degree per frame: 6 - 72 degrees from one frame into a target to the next) cannot use a measured order, and
// measuring cost it 0.3 - 2.9 % (profiles/r6_feedback_moving_camera.txt); it pays for the first frame only.
FeedbackStep feedback_step(FeedbackState &f, const FrameView &view, uint32_t base_period)
{
	const bool     stale  = f.has_cost && !view_close(view, f.measured);
	const uint32_t since  = f.frames - f.measured_at;
	const bool     steady = f.has_prev && view_close(view, f.prev);
	f.prev = view, f.has_prev = true;
	const bool measure = !f.has_cost || (since >= f.period && steady);
	if (measure)
	{
		// a measurement whose order no frame could use (the target kept jumping between far views) doubles the distance to the next
		// one, up to 8 periods: such a target then pays next to nothing for the feedback it cannot use
		f.period      = (f.has_cost && f.used == 0) ? std::min(2u * f.period, 8u * base_period) : base_period;
		f.measured_at = f.frames;
		f.used        = 0;
	}
	++f.frames;
	const bool use_order = f.has_cost && !stale;        // the order the last sort behind a frame into this target left
	if (use_order)
		++f.used;
	if (measure)
		f.measured = view, f.has_cost = true;        // (the new order is written by the sort that FOLLOWS this frame's render)
	return {use_order, measure};
}
}        // namespace vkv

using namespace vkv;

extern "C" {

// src/volume_component.cpp:226-240
int vkv_transfer_function_uniform(const VkvVolumeOptions *o, VkvTransferFunctionUniform *u)
{
	if (!o || !u)
		return VKV_E_INVALID_ARGUMENT;
	u->sampling_factor         = o->sampling_factor;
	u->voxel_alpha_factor      = o->voxel_alpha_factor;
	u->grad_magnitude_modifier = 1.0f;
	u->use_gradient            = o->gradient_max != o->gradient_min;
	u->intensity_min           = o->intensity_min;
	u->intensity_range_inv     = 1.0f / (o->intensity_max - o->intensity_min);
	u->gradient_min            = o->gradient_min;
	u->gradient_range_inv      = 1.0f / (o->gradient_max - o->gradient_min);
	return VKV_OK;
}

// src/volume_component.cpp:242-261
int vkv_transfer_function_texture(const VkvVolumeOptions *o, uint8_t *tex)
{
	if (!o || !tex)
		return VKV_E_INVALID_ARGUMENT;
	auto        clampf       = [](float x, float lo, float hi) { return std::min(std::max(x, lo), hi); };
	const float i_inv        = 1.0f / (o->intensity_max - o->intensity_min);
	const float g_inv        = 1.0f / (o->gradient_max - o->gradient_min);
	const bool  use_gradient = o->gradient_max != o->gradient_min;
	size_t      idx          = 0;
	for (int gi = 0; gi < 256; ++gi)
		for (int ii = 0; ii < 256; ++ii, ++idx)
		{
			const float   g = (float) gi, i = (float) ii;
			const float   alpha_i = clampf(((i / 255.0f) - o->intensity_min) * i_inv, 0.0f, 1.0f);
			const float   alpha_g = use_gradient ? clampf(((g / 255.0f) - o->gradient_min) * g_inv, 0.0f, 1.0f) : 1.0f;
			const uint8_t alpha   = static_cast<uint8_t>(clampf(alpha_i * alpha_g * 255, 0, 255));
			tex[idx * 4 + 0] = tex[idx * 4 + 1] = tex[idx * 4 + 2] = tex[idx * 4 + 3] = alpha;
		}
	return VKV_OK;
}

// src/volume_render_subpass.cpp:221-249
int vkv_build_uniforms(const float *view, const float *proj, const float *node_transform, const float *image_transform, float clip_distance,
                       uint32_t image_width, uint32_t image_height, VkvExtent3D ve, VkvExtent3D me, VkvCameraUniform *cam, VkvRayCastUniform *rc,
                       VkvRayGen *rg)
{
	if (!view || !proj || !node_transform || !image_transform || !cam || !rc || !rg || !extent_ok(ve) || !extent_ok(me) || image_width == 0 ||
	    image_height == 0)
		return VKV_E_INVALID_ARGUMENT;
	const mat4 V(view), P(proj), N(node_transform), I(image_transform);
	const mat4 model         = N * I;
	const mat4 model_inv     = inverse(model);
	const mat4 view_proj_inv = inverse(P * V);
	std::memcpy(cam->camera_view, V.m, 64);
	std::memcpy(cam->camera_proj, P.m, 64);
	std::memcpy(cam->camera_view_proj_inv, view_proj_inv.m, 64);
	std::memcpy(cam->model, model.m, 64);
	std::memcpy(cam->model_inv, model_inv.m, 64);

	const mat4 model_to_tex  = translate(vec3{0.5f, 0.5f, 0.5f});
	const mat4 global_to_tex = model_to_tex * model_inv;
	const mat4 view_inv      = inverse(V);
	const vec3 cam_pos_global{view_inv.at(0, 3), view_inv.at(1, 3), view_inv.at(2, 3)};
	const vec4 cam_pos_model = model_inv * vec4{cam_pos_global.x, cam_pos_global.y, cam_pos_global.z, 1.0f};
	const vec4 cam_pos_tex   = model_to_tex * vec4{cam_pos_model.x, cam_pos_model.y, cam_pos_model.z, 1.0f};
	const vec4 cam_dir4      = view_inv * vec4{0, 0, -1, 0};
	const vec3 cam_dir{cam_dir4.x, cam_dir4.y, cam_dir4.z};
	const vec4 plane{cam_dir.x, cam_dir.y, cam_dir.z,
	                 -clip_distance - (cam_pos_global.x * cam_dir.x + cam_pos_global.y * cam_dir.y + cam_pos_global.z * cam_dir.z)};
	const vec4 plane_tex = inverse_transpose(global_to_tex) * plane;
	rc->plane[0] = plane.x, rc->plane[1] = plane.y, rc->plane[2] = plane.z, rc->plane[3] = plane.w;
	rc->plane_tex[0] = plane_tex.x, rc->plane_tex[1] = plane_tex.y, rc->plane_tex[2] = plane_tex.z, rc->plane_tex[3] = plane_tex.w;
	rc->camera_pos_tex[0] = cam_pos_tex.x, rc->camera_pos_tex[1] = cam_pos_tex.y, rc->camera_pos_tex[2] = cam_pos_tex.z, rc->camera_pos_tex[3] = cam_pos_tex.w;
	rc->front_index   = (plane_tex.x < 0 ? 1 : 0) + (plane_tex.y < 0 ? 2 : 0) + (plane_tex.z < 0 ? 4 : 0);
	rc->block_size[0] = (float) block_of(ve.width, me.width);
	rc->block_size[1] = (float) block_of(ve.height, me.height);
	rc->block_size[2] = (float) block_of(ve.depth, me.depth);
	rc->block_size[3] = 0.0f;

	// Ray generator (replaces the rasteriser): in double precision from the same float matrices.  Unproject pixel-space
	// points (0,0), (1,0), (0,1) at two depths, express the direction in texture space and scale it to unit distance along
	// the view direction (plane_tex.xyz is that covector), which makes the direction affine in pixel coordinates.
	double PV[16], PVinv[16], Md[16], Minv[16];
	{
		const mat4 pv = P * V;        // product in float like the uniform above, inverted in double
		for (int i = 0; i < 16; ++i)
			PV[i] = pv.m[i], Md[i] = model.m[i];
		if (!invert4x4<double>(PV, PVinv) || !invert4x4<double>(Md, Minv))
			return VKV_E_INVALID_ARGUMENT;
	}
	auto mulv = [](const double *m, const double *v, double *r) {
		for (int i = 0; i < 4; ++i)
			r[i] = m[i] * v[0] + m[4 + i] * v[1] + m[8 + i] * v[2] + m[12 + i] * v[3];
	};
	double       dirs[3][3];
	const double pts[3][2] = {{0, 0}, {1, 0}, {0, 1}};
	for (int p = 0; p < 3; ++p)
	{
		const double nx = 2.0 * pts[p][0] / (double) image_width - 1.0, ny = 2.0 * pts[p][1] / (double) image_height - 1.0;
		const double c1[4] = {nx, ny, 1.0, 1.0}, c2[4] = {nx, ny, 0.25, 1.0};
		double       w1[4], w2[4], t1[4], t2[4];
		mulv(PVinv, c1, w1);
		mulv(PVinv, c2, w2);
		for (int i = 0; i < 3; ++i)
			w1[i] /= w1[3], w2[i] /= w2[3];
		w1[3] = w2[3] = 1.0;
		mulv(Minv, w1, t1);        // model space; the +0.5 translation cancels in the difference
		mulv(Minv, w2, t2);
		const double dx = t2[0] - t1[0], dy = t2[1] - t1[1], dz = t2[2] - t1[2];
		const double along = (double) plane_tex.x * dx + (double) plane_tex.y * dy + (double) plane_tex.z * dz;
		dirs[p][0] = dx / along, dirs[p][1] = dy / along, dirs[p][2] = dz / along;
	}
	for (int i = 0; i < 3; ++i)
	{
		rg->dir00[i] = (float) dirs[0][i];
		rg->ddx[i]   = (float) (dirs[1][i] - dirs[0][i]);
		rg->ddy[i]   = (float) (dirs[2][i] - dirs[0][i]);
	}
	rg->dir00[3] = rg->ddx[3] = rg->ddy[3] = 0.0f;
	return VKV_OK;
}

// ---- loader (host side; the C++ class throws, the C ABI returns codes) ------------------------------------------
int vkv_load_header(const char *filename_header, VkvVolumeHeader *out)
{
	if (!filename_header || !out)
		return VKV_E_INVALID_ARGUMENT;
	try
	{
		const LoadVolume::Header h = LoadVolume::load_header(filename_header);
		std::memset(out, 0, sizeof(*out));
		out->extent = h.extent;
		out->voxel_size[0] = h.voxel_size.x, out->voxel_size[1] = h.voxel_size.y, out->voxel_size[2] = h.voxel_size.z;
		out->normalisation_range[0] = h.normalisation_range[0], out->normalisation_range[1] = h.normalisation_range[1];
		std::strncpy(out->type, h.type.c_str(), sizeof(out->type) - 1);
		std::strncpy(out->endianness, h.endianness.c_str(), sizeof(out->endianness) - 1);
		std::memcpy(out->image_transform, h.image_transform.m, sizeof(out->image_transform));
		return VKV_OK;
	}
	catch (const std::exception &)
	{
		return VKV_E_IO;
	}
}

int vkv_load_data(const char *filename_data, const VkvVolumeHeader *header, uint8_t *out_voxels, size_t out_bytes)
{
	if (!filename_data || !header || !out_voxels)
		return VKV_E_INVALID_ARGUMENT;
	try
	{
		LoadVolume::Header h;
		h.extent                 = header->extent;
		h.normalisation_range[0] = header->normalisation_range[0], h.normalisation_range[1] = header->normalisation_range[1];
		h.type       = std::string(header->type, strnlen(header->type, sizeof(header->type)));
		h.endianness = std::string(header->endianness, strnlen(header->endianness, sizeof(header->endianness)));
		const std::vector<uint8_t> v = LoadVolume::load_data(filename_data, h);
		if (v.size() != out_bytes)
			return VKV_E_INVALID_ARGUMENT;
		std::memcpy(out_voxels, v.data(), v.size());
		return VKV_OK;
	}
	catch (const std::runtime_error &e)
	{
		return std::string(e.what()) == "unsupported image data type" ? VKV_E_INVALID_ARGUMENT : VKV_E_IO;
	}
	catch (const std::exception &)
	{
		return VKV_E_IO;
	}
}

int vkv_screen_tile_rect(const VkvRayCastUniform *ray_cast, const VkvRayGen *ray_gen, uint32_t image_width, uint32_t image_height, uint32_t tile_width,
                         uint32_t tile_height, uint32_t align_tiles, VkvTileRect *out_rect)
{
	if (!ray_cast || !ray_gen || !out_rect || !image_width || !image_height || !tile_width || !tile_height)
		return VKV_E_INVALID_ARGUMENT;
	screen_tile_rect(ray_cast, ray_gen, image_width, image_height, tile_width, tile_height, align_tiles, out_rect);
	return VKV_OK;
}

}        // extern "C"

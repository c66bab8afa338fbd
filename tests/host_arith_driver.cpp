// host_arith_driver.cpp — the library's pure host arithmetic (vkvolume_amd/host/host_arith.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer.  Built and run by tests/test_host_arith_cpu.py (CPU only, no HIP, nothing loaded into Python):
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined host_arith_driver.cpp
//         ../vkvolume_amd/host/host_arith.cpp ../vkvolume_amd/host/load_volume.cpp
// exit status 0 = every check passed (a sanitizer report aborts the process).  Expected values are worked out here from the definitions
// (tile centres, the pinhole projection, the opacity formula, the documented ranges), not by calling the code under test a second time.
// With the argument "iso_threshold" it instead prints kInv255's bits and, for every float32 bit pattern on stdin (hexadecimal, one per
// line), iso_threshold() of it: the test holds those against numpy.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../vkvolume_amd/host/host_arith.hpp"

using namespace vkv;

static int g_failed = 0;
#define CHECK(cond)                                                           \
	do                                                                        \
	{                                                                         \
		if (!(cond))                                                          \
		{                                                                     \
			std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
			++g_failed;                                                       \
		}                                                                     \
	} while (0)

static bool is_permutation_of_range(const std::vector<uint32_t> &v, uint32_t count)
{
	if (v.size() != count)
		return false;
	std::vector<char> seen(count, 0);
	for (uint32_t x : v)
	{
		if (x >= count || seen[x])
			return false;
		seen[x] = 1;
	}
	return true;
}

// ---- start order ------------------------------------------------------------------------------------------------------------
// entry k of a schedule is tile first + k * stride (row-major over the image's tiles); its key is the squared distance of the tile's
// centre from the image centre, in pixels
static double centre_distance2(uint32_t img_w, uint32_t img_h, uint32_t tw, uint32_t th, uint32_t first, uint32_t stride, uint32_t k)
{
	const uint32_t tiles_x = (img_w + tw - 1) / tw;
	const uint64_t t       = (uint64_t) first + (uint64_t) k * stride;
	const double   cx = ((double) (t % tiles_x) + 0.5) * tw - 0.5 * img_w, cy = ((double) (t / tiles_x) + 0.5) * th - 0.5 * img_h;
	return cx * cx + cy * cy;
}

// partial: odd image sizes, the last tile column and row are partial (no two tiles at the same distance); else whole tiles, where the image's
// symmetry gives every distance up to four times.  Returns the number of ties it met.
static uint32_t start_order_case(uint32_t tiles_x, uint32_t tiles_y, uint32_t first, uint32_t stride, bool partial)
{
	const uint32_t tw = 16, th = 32, img_w = tiles_x * tw - (partial ? 5 : 0), img_h = tiles_y * th - (partial ? 3 : 0), tiles = tiles_x * tiles_y;
	uint32_t       ties = 0;
	const uint32_t count = first < tiles ? (tiles - first + stride - 1) / stride : 0u;
	const std::vector<uint32_t> order = start_order(img_w, img_h, tw, th, first, stride, count, 0.0f, 0.0f);
	CHECK(is_permutation_of_range(order, count));
	for (size_t r = 1; r < order.size(); ++r)
	{
		const double a = centre_distance2(img_w, img_h, tw, th, first, stride, order[r - 1]), b = centre_distance2(img_w, img_h, tw, th, first, stride, order[r]);
		CHECK(a <= b);
		if (a == b)
		{
			CHECK(order[r - 1] < order[r]);        // ties keep index order
			++ties;
		}
	}
	return ties;
}

static void tile_mix_case(uint32_t count)
{
	// 10 x 7 tiles of 16 x 16, the first `count` of them
	const uint32_t img_w = 160, img_h = 112, t = 16;
	const std::vector<uint32_t> plain = start_order(img_w, img_h, t, t, 0, 1, count, 0.0f, 0.0f);
	const std::vector<uint32_t> mixed = start_order(img_w, img_h, t, t, 0, 1, count, 0.25f, 0.5f);
	CHECK(is_permutation_of_range(plain, count));
	CHECK(is_permutation_of_range(mixed, count));
	// 64 and 67 entries are 8 groups of eight: the central quarter is groups 0 and 1 (nh = 2), spread over the first half (span = 4) - heavy
	// group h is due at position h * span / nh = 0 and 2; the light groups 2 .. 7 fill the gaps and the end in their order
	CHECK(count / 8 == 8);
	const uint32_t group_at[8] = {0, 2, 1, 3, 4, 5, 6, 7};
	if (mixed.size() == count && plain.size() == count)
	{
		for (uint32_t r = 0; r < 8; ++r)
			for (uint32_t j = 0; j < 8; ++j)
				CHECK(mixed[r * 8 + j] == plain[group_at[r] * 8 + j]);        // groups of eight stay intact
		for (uint32_t r = 64; r < count; ++r)
			CHECK(mixed[r] == plain[r]);        // the tail count % 8 is unmoved
	}
	// a mix outside its valid range (0 < heavy < 1, heavy <= spread <= 1) leaves the plain order
	const float nan = std::numeric_limits<float>::quiet_NaN();
	const float bad[][2] = {{0.0f, 0.5f}, {1.0f, 1.0f}, {0.5f, 0.25f}, {0.25f, 1.5f}, {-0.25f, 0.5f}, {2.0f, 3.0f}, {nan, 0.5f}, {0.25f, nan}};
	for (const auto &b : bad)
		CHECK(start_order(img_w, img_h, t, t, 0, 1, count, b[0], b[1]) == plain);
}

// ---- screen bound -----------------------------------------------------------------------------------------------------------
struct Vec
{
	double x, y, z;
};
static Vec    sub(Vec a, Vec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static double dot(Vec a, Vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static Vec    cross(Vec a, Vec b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static Vec    unit(Vec a)
{
	const double n = std::sqrt(dot(a, a));
	return {a.x / n, a.y / n, a.z / n};
}

// a pinhole camera in texture space: pixel (px, py) looks along dir00 + (px + 0.5) ddx + (py + 0.5) ddy
struct Camera
{
	Vec      pos, f, r, u;
	double   tan_x, tan_y;
	uint32_t iw, ih;
	Camera(Vec position, Vec target, double fov_y_degrees, uint32_t w, uint32_t h) : pos(position), iw(w), ih(h)
	{
		f     = unit(sub(target, position));
		r     = unit(cross(f, std::fabs(f.y) > 0.9 ? Vec{1, 0, 0} : Vec{0, 1, 0}));
		u     = cross(r, f);
		tan_y = std::tan(fov_y_degrees * 3.14159265358979323846 / 360.0);
		tan_x = tan_y * (double) w / (double) h;
	}
	void generator(float cam[3], float dir00[3], float ddx[3], float ddy[3]) const
	{
		const double F[3] = {f.x, f.y, f.z}, R[3] = {r.x, r.y, r.z}, U[3] = {u.x, u.y, u.z}, P[3] = {pos.x, pos.y, pos.z};
		for (int i = 0; i < 3; ++i)
		{
			cam[i]   = (float) P[i];
			dir00[i] = (float) (F[i] - tan_x * R[i] - tan_y * U[i]);
			ddx[i]   = (float) (2.0 * tan_x / iw * R[i]);
			ddy[i]   = (float) (2.0 * tan_y / ih * U[i]);
		}
	}
	// where a point in front of the camera is seen, in continuous pixel coordinates (pixel p covers [p, p + 1))
	bool project(Vec p, double &fx, double &fy) const
	{
		const Vec    w = sub(p, pos);
		const double g = dot(w, f);
		if (!(g > 0.0))
			return false;
		fx = (dot(w, r) / (g * tan_x) + 1.0) * 0.5 * iw;
		fy = (dot(w, u) / (g * tan_y) + 1.0) * 0.5 * ih;
		return true;
	}
};

// the corners of the unit box on the kept side of the plane (dot(n, p) + w >= 0; no plane: all eight)
static std::vector<Vec> kept_corners(const float *plane)
{
	std::vector<Vec> v;
	for (int c = 0; c < 8; ++c)
	{
		const Vec p{(double) (c & 1), (double) ((c >> 1) & 1), (double) ((c >> 2) & 1)};
		if (!plane || (double) plane[0] * p.x + (double) plane[1] * p.y + (double) plane[2] * p.z + (double) plane[3] >= 0.0)
			v.push_back(p);
	}
	return v;
}

static void screen_bound_case(const Camera &cam, const float *plane, bool expect_tighter_than_box)
{
	float c[3], d0[3], dx[3], dy[3];
	cam.generator(c, d0, dx, dy);
	double b[4] = {0, 0, 0, 0}, whole[4] = {0, 0, 0, 0};
	CHECK(screen_bound(c, d0, dx, dy, plane, b) == kScreenBoundRect);
	CHECK(screen_bound(c, d0, dx, dy, nullptr, whole) == kScreenBoundRect);
	const std::vector<Vec> corners = kept_corners(plane);
	CHECK(!corners.empty());
	double lo_x = 1e300, hi_x = -1e300, lo_y = 1e300, hi_y = -1e300;
	for (const Vec &p : corners)
	{
		double fx = 0, fy = 0;
		CHECK(cam.project(p, fx, fy));
		// the pixel that sees the vertex lies inside the bound {x0, x1, y0, y1} (inclusive pixel indices)
		CHECK(std::floor(fx) >= b[0] && std::floor(fx) <= b[1] && std::floor(fy) >= b[2] && std::floor(fy) <= b[3]);
		lo_x = std::min(lo_x, fx), hi_x = std::max(hi_x, fx), lo_y = std::min(lo_y, fy), hi_y = std::max(hi_y, fy);
	}
	// the clipped box lies inside the box: so does its bound
	CHECK(b[0] >= whole[0] && b[1] <= whole[1] && b[2] >= whole[2] && b[3] <= whole[3]);
	if (!plane)        // all vertices are corners: the bound is their extent widened by two pixels and the rounding to whole pixels
		CHECK(b[0] >= lo_x - 4.0 && b[1] <= hi_x + 4.0 && b[2] >= lo_y - 4.0 && b[3] <= hi_y + 4.0);
	if (expect_tighter_than_box)
		CHECK((b[1] - b[0]) * (b[3] - b[2]) < (whole[1] - whole[0]) * (whole[3] - whole[2]));

	// the same in whole tiles
	VkvRayCastUniform rc;
	VkvRayGen         rg;
	std::memset(&rc, 0, sizeof(rc));
	std::memset(&rg, 0, sizeof(rg));
	for (int i = 0; i < 3; ++i)
		rc.camera_pos_tex[i] = c[i], rg.dir00[i] = d0[i], rg.ddx[i] = dx[i], rg.ddy[i] = dy[i];
	for (int i = 0; i < 4 && plane; ++i)
		rc.plane_tex[i] = plane[i];        // (all zero: no usable plane, the whole box)
	const uint32_t tw = 16, th = 32, tiles_x = (cam.iw + tw - 1) / tw, tiles_y = (cam.ih + th - 1) / th;
	for (uint32_t align : {1u, 4u})
	{
		VkvTileRect r{9, 9, 9, 9};
		CHECK(vkv_screen_tile_rect(&rc, &rg, cam.iw, cam.ih, tw, th, align, &r) == VKV_OK);
		CHECK(r.w >= 1 && r.h >= 1 && r.x0 + r.w <= tiles_x && r.y0 + r.h <= tiles_y);
		CHECK(r.x0 % align == 0 && r.y0 % align == 0);
		for (const Vec &p : corners)
		{
			double fx = 0, fy = 0;
			if (!cam.project(p, fx, fy))
				continue;
			// the tile of the pixel that sees the vertex, or of the image's edge pixel nearest to it
			const uint32_t px = (uint32_t) std::min(std::max(std::floor(fx), 0.0), (double) cam.iw - 1.0), py = (uint32_t) std::min(std::max(std::floor(fy), 0.0), (double) cam.ih - 1.0);
			CHECK(px / tw >= r.x0 && px / tw < r.x0 + r.w && py / th >= r.y0 && py / th < r.y0 + r.h);
		}
	}
}

static void screen_bound_tests()
{
	const Vec   centre{0.5, 0.5, 0.5};
	const float cut_x[4] = {1.0f, 0.0f, 0.0f, -0.5f};             // keeps x >= 0.5
	const float cut_diag[4] = {0.5f, -0.25f, 1.0f, -0.4f};       // an oblique cut
	const float keep_all[4] = {0.0f, 0.0f, 1.0f, 2.0f};          // a plane that cuts nothing
	const Camera cams[] = {Camera({0.5, 0.5, 3.5}, centre, 40.0, 640, 480), Camera({3.0, 2.0, -2.5}, centre, 30.0, 333, 517),
	                       Camera({-1.2, 0.3, 0.8}, centre, 60.0, 1920, 1080), Camera({0.6, 4.0, 0.4}, centre, 50.0, 256, 256),
	                       Camera({0.5, 0.5, 1.3}, centre, 90.0, 200, 120) /* close: the box runs past the image */};
	for (const Camera &cam : cams)
	{
		screen_bound_case(cam, nullptr, false);
		screen_bound_case(cam, keep_all, false);
		screen_bound_case(cam, cut_diag, false);
	}
	screen_bound_case(cams[0], cut_x, true);        // seen along z, half of the box is gone: half of the bound
	{        // a camera inside the box, no plane: vertices behind it, no statement, the whole image
		const Camera cam({0.4, 0.5, 0.6}, {0.9, 0.5, 0.1}, 60.0, 300, 200);
		float        c[3], d0[3], dx[3], dy[3];
		cam.generator(c, d0, dx, dy);
		double b[4];
		CHECK(screen_bound(c, d0, dx, dy, nullptr, b) == kScreenBoundNone);
		VkvRayCastUniform rc;
		VkvRayGen         rg;
		std::memset(&rc, 0, sizeof(rc));
		std::memset(&rg, 0, sizeof(rg));
		for (int i = 0; i < 3; ++i)
			rc.camera_pos_tex[i] = c[i], rg.dir00[i] = d0[i], rg.ddx[i] = dx[i], rg.ddy[i] = dy[i];
		VkvTileRect r{9, 9, 9, 9};
		CHECK(vkv_screen_tile_rect(&rc, &rg, 300, 200, 16, 16, 1, &r) == VKV_OK);
		CHECK(r.x0 == 0 && r.y0 == 0 && r.w == 19 && r.h == 13);
	}
	{        // the box behind the camera, with the application's plane (through a point in front of the camera, facing away from it): nothing is
		 // on the kept side, nothing can be seen, the 1 x 1 rectangle
		const Camera cam({0.5, 0.5, 3.0}, {0.5, 0.5, 9.0}, 60.0, 300, 200);
		float        c[3], d0[3], dx[3], dy[3];
		cam.generator(c, d0, dx, dy);
		const float plane[4] = {(float) cam.f.x, (float) cam.f.y, (float) cam.f.z, (float) (-1.0 - dot(cam.f, cam.pos))};        // dot(f, p - pos) >= 1
		CHECK(kept_corners(plane).empty());
		double b[4];
		CHECK(screen_bound(c, d0, dx, dy, plane, b) == kScreenBoundEmpty);
		VkvRayCastUniform rc;
		VkvRayGen         rg;
		std::memset(&rc, 0, sizeof(rc));
		std::memset(&rg, 0, sizeof(rg));
		for (int i = 0; i < 3; ++i)
			rc.camera_pos_tex[i] = c[i], rg.dir00[i] = d0[i], rg.ddx[i] = dx[i], rg.ddy[i] = dy[i];
		for (int i = 0; i < 4; ++i)
			rc.plane_tex[i] = plane[i];
		for (uint32_t align : {1u, 4u})
		{
			VkvTileRect r{9, 9, 9, 9};
			CHECK(vkv_screen_tile_rect(&rc, &rg, 300, 200, 16, 16, align, &r) == VKV_OK);
			CHECK(r.x0 == 0 && r.y0 == 0 && r.w == 1 && r.h == 1);
		}
		VkvTileRect r;
		CHECK(vkv_screen_tile_rect(nullptr, &rg, 300, 200, 16, 16, 1, &r) == VKV_E_INVALID_ARGUMENT);
		CHECK(vkv_screen_tile_rect(&rc, &rg, 300, 0, 16, 16, 1, &r) == VKV_E_INVALID_ARGUMENT);
	}
}

// ---- tuning -----------------------------------------------------------------------------------------------------------------
static const char *const kTuningVariables[] = {"VKV_RAYMARCH_SCHEDULER", "VKV_RAYMARCH_BATCH", "VKV_RAYMARCH_BATCH_ORDER", "VKV_RAYMARCH_TILE_ORDER", "VKV_RAYMARCH_LUT",
                                               "VKV_RAYMARCH_FULL_LIMIT", "VKV_RAYMARCH_CULL", "VKV_RAYMARCH_FEEDBACK", "VKV_RAYMARCH_FEEDBACK_PERIOD", "VKV_RAYMARCH_TILE_MIX",
                                               "VKV_GRADIENT_SEGMENT", "VKV_ARENA_BYTES", "VKV_RAYMARCH_CLAMP", "VKV_RAYMARCH_WAVE_SHAPE"};
constexpr uint32_t kLdsCap = 64 * 1024 - 1024;        // what the library passes: the dynamic LDS a kernel may ask for

// the documented defaults (include/vkvolume_amd.h, VkvTuning)
static VkvTuning documented_defaults()
{
	VkvTuning t;
	std::memset(&t, 0, sizeof(t));
	t.struct_size = (uint32_t) sizeof(VkvTuning), t.address_tables = 2, t.full_table_lds_limit = 17920, t.screen_cull = 1, t.feedback = 1, t.feedback_period = 8;
	t.arena_bytes = 8u << 20;
	return t;
}

// the tuning block with the environment holding only `name` = `value` (null: nothing set)
static VkvTuning tuning_with(const char *name, const char *value)
{
	for (const char *v : kTuningVariables)
		unsetenv(v);
	if (name)
		setenv(name, value, 1);
	VkvTuning t;
	std::memset(&t, 0xab, sizeof(t));
	default_tuning(t, kLdsCap);
	return t;
}

static bool same(const VkvTuning &a, const VkvTuning &b) { return std::memcmp(&a, &b, sizeof(VkvTuning)) == 0; }

static void tuning_tests()
{
	const VkvTuning d = documented_defaults();
	CHECK(same(tuning_with(nullptr, nullptr), d));
	CHECK(same(tuning_with("VKV_RAYMARCH_CULL", ""), d));        // an empty variable counts as unset
	CHECK(tuning_problem(d) == nullptr);
	size_t read = 0;
	// every variable is read: it changes its field and nothing else
#define FIELD(name, value, field, expected)            \
	do                                                 \
	{                                                  \
		VkvTuning want = d;                            \
		want.field     = expected;                     \
		CHECK(!same(want, d));                         \
		CHECK(same(tuning_with(name, value), want));   \
		++read;                                        \
	} while (0)
	FIELD("VKV_RAYMARCH_SCHEDULER", "persistent", scheduler, 1);
	FIELD("VKV_RAYMARCH_BATCH", "pull", batch_mode, 1);
	FIELD("VKV_RAYMARCH_BATCH_ORDER", "sequential", batch_sequential, 1);
	FIELD("VKV_RAYMARCH_TILE_ORDER", "linear", tile_order_linear, 1);
	FIELD("VKV_RAYMARCH_LUT", "0", address_tables, 0);
	FIELD("VKV_RAYMARCH_FULL_LIMIT", "1000", full_table_lds_limit, 1000u);
	FIELD("VKV_RAYMARCH_CULL", "0", screen_cull, 0);
	FIELD("VKV_RAYMARCH_FEEDBACK", "0", feedback, 0);
	FIELD("VKV_RAYMARCH_FEEDBACK_PERIOD", "3", feedback_period, 3u);
	{
		VkvTuning want      = d;
		want.tile_mix_heavy = 0.25f, want.tile_mix_spread = 0.5f;
		CHECK(same(tuning_with("VKV_RAYMARCH_TILE_MIX", "0.25,0.5"), want));
		++read;
	}
	FIELD("VKV_GRADIENT_SEGMENT", "7", gradient_segment, 7u);
	FIELD("VKV_ARENA_BYTES", "4194304", arena_bytes, 4u << 20);
	FIELD("VKV_RAYMARCH_CLAMP", "always", clamp_always, 1);
	FIELD("VKV_RAYMARCH_WAVE_SHAPE", "8", wave_shape, 8);
	CHECK(read == sizeof(kTuningVariables) / sizeof(kTuningVariables[0]));
	// values that map or clamp
	FIELD("VKV_RAYMARCH_LUT", "2", address_tables, 1);        // "2" = two-level tables = address_tables 1
	FIELD("VKV_RAYMARCH_FULL_LIMIT", "999999", full_table_lds_limit, kLdsCap);
	FIELD("VKV_RAYMARCH_FULL_LIMIT", "-5", full_table_lds_limit, 0u);
	FIELD("VKV_GRADIENT_SEGMENT", "999", gradient_segment, 255u);
	FIELD("VKV_ARENA_BYTES", "1", arena_bytes, 1u << 20);
	FIELD("VKV_ARENA_BYTES", "99999999999", arena_bytes, 1u << 30);
	FIELD("VKV_RAYMARCH_WAVE_SHAPE", "16", wave_shape, 16);
#undef FIELD
	CHECK(same(tuning_with("VKV_RAYMARCH_WAVE_SHAPE", "5"), d));
	CHECK(tuning_with("VKV_RAYMARCH_FEEDBACK_PERIOD", "0").feedback_period == 1u);
	// an out-of-range tile mix falls back to 0, 0
	for (const char *mix : {"2,3", "nan,0.5", "0.5,nan", "-0.5,0.5", "0.5,inf"})
		CHECK(same(tuning_with("VKV_RAYMARCH_TILE_MIX", mix), d));
	CHECK(same(tuning_with("VKV_RAYMARCH_TILE_MIX", "0.5"), d));        // (not two numbers: not read)
	for (const char *v : kTuningVariables)
		unsetenv(v);

	// tuning_problem: each field one step outside its range is rejected, the ends of the range are accepted
#define REJECT(field, value)                   \
	do                                         \
	{                                          \
		VkvTuning t = d;                       \
		t.field     = value;                   \
		CHECK(tuning_problem(t) != nullptr);   \
	} while (0)
#define ACCEPT(field, value)                   \
	do                                         \
	{                                          \
		VkvTuning t = d;                       \
		t.field     = value;                   \
		CHECK(tuning_problem(t) == nullptr);   \
	} while (0)
	const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
	REJECT(scheduler, -1); REJECT(scheduler, 2); ACCEPT(scheduler, 0); ACCEPT(scheduler, 1);
	REJECT(batch_mode, -1); REJECT(batch_mode, 2); ACCEPT(batch_mode, 1);
	REJECT(address_tables, -1); REJECT(address_tables, 3); ACCEPT(address_tables, 0); ACCEPT(address_tables, 2);
	REJECT(feedback_period, 0u); ACCEPT(feedback_period, 1u); ACCEPT(feedback_period, 0xffffffffu);
	REJECT(gradient_segment, 256u); ACCEPT(gradient_segment, 255u); ACCEPT(gradient_segment, 0u);
	REJECT(clamp_always, -1); REJECT(clamp_always, 2); ACCEPT(clamp_always, 1);
	for (int w : {-1, 1, 3, 5, 7, 9, 15, 17})
		REJECT(wave_shape, w);
	for (int w : {0, 4, 8, 16})
		ACCEPT(wave_shape, w);
	REJECT(tile_mix_heavy, std::nextafter(0.0f, -1.0f)); REJECT(tile_mix_heavy, std::nextafter(1.0f, 2.0f)); REJECT(tile_mix_heavy, nan); REJECT(tile_mix_heavy, inf);
	REJECT(tile_mix_spread, std::nextafter(0.0f, -1.0f)); REJECT(tile_mix_spread, std::nextafter(1.0f, 2.0f)); REJECT(tile_mix_spread, nan); REJECT(tile_mix_spread, -inf);
	ACCEPT(tile_mix_heavy, 1.0f); ACCEPT(tile_mix_spread, 1.0f); ACCEPT(tile_mix_heavy, 0.0f);
#undef REJECT
#undef ACCEPT
	VkvTuning t = d;
	t.full_table_lds_limit = 0xffffffffu;
	clamp_tuning(t, kLdsCap);
	CHECK(t.full_table_lds_limit == kLdsCap);
}

// ---- opacity table, tile rectangles -----------------------------------------------------------------------------------------------
static void alpha_lut_case(float voxel_alpha_factor, float sampling_factor)
{
	VkvTransferFunctionUniform tf;
	std::memset(&tf, 0, sizeof(tf));
	tf.voxel_alpha_factor = voxel_alpha_factor, tf.sampling_factor = sampling_factor;
	float lut[256 + 2];
	lut[0] = lut[257] = -77.0f;        // guards: 256 entries are written, no more
	build_alpha_lut(tf, lut + 1);
	CHECK(lut[0] == -77.0f && lut[257] == -77.0f);
	for (int a = 0; a < 256; ++a)
	{
		// frag:283 in float: clamp(voxel_alpha_factor * (1 - pow(1 - a / 255, 1 / sampling_factor)), 0, 1)
		const float exponent = 1.0f / sampling_factor;
		const float base     = 1.0f - (float) a / 255.0f;
		float       want     = voxel_alpha_factor * (1.0f - std::pow(base, exponent));
		want                 = want < 0.0f ? 0.0f : (want > 1.0f ? 1.0f : want);
		CHECK(lut[1 + a] == want);
		CHECK(lut[1 + a] >= 0.0f && lut[1 + a] <= 1.0f);
	}
	CHECK(lut[1] == 0.0f);
	CHECK(lut[256] == std::min(voxel_alpha_factor, 1.0f));        // a = 255: 1 - pow(0, e) = 1
}

static void resolve_rect_tests()
{
	// 100 x 50 pixels in tiles of 16 x 16: 7 x 4 tiles, the last column and row partial
	const uint32_t iw = 100, ih = 50, t = 16;
	VkvTileRect    out{9, 9, 9, 9};
	CHECK(resolve_rect(nullptr, iw, ih, t, t, out) && out.x0 == 0 && out.y0 == 0 && out.w == 7 && out.h == 4);
	for (const VkvTileRect &empty : {VkvTileRect{0, 0, 0, 0}, VkvTileRect{2, 1, 0, 3}, VkvTileRect{2, 1, 3, 0}})
	{
		out = VkvTileRect{9, 9, 9, 9};
		CHECK(resolve_rect(&empty, iw, ih, t, t, out) && out.x0 == 0 && out.y0 == 0 && out.w == 7 && out.h == 4);
	}
	for (const VkvTileRect &in : {VkvTileRect{0, 0, 7, 4}, VkvTileRect{6, 3, 1, 1}, VkvTileRect{2, 1, 5, 3}})
	{
		out = VkvTileRect{9, 9, 9, 9};
		CHECK(resolve_rect(&in, iw, ih, t, t, out) && out.x0 == in.x0 && out.y0 == in.y0 && out.w == in.w && out.h == in.h);
	}
	// one tile past either edge (and a sum that wraps in 32 bits)
	for (const VkvTileRect &past : {VkvTileRect{0, 0, 8, 4}, VkvTileRect{0, 0, 7, 5}, VkvTileRect{7, 0, 1, 1}, VkvTileRect{0, 4, 1, 1}, VkvTileRect{3, 1, 5, 3}, VkvTileRect{2, 2, 5, 3},
	                                VkvTileRect{0xffffffffu, 0, 2, 1}, VkvTileRect{0, 0xffffffffu, 1, 2}})
		CHECK(!resolve_rect(&past, iw, ih, t, t, out));
}

// "kInv255 <bits>", then one threshold per bit pattern read
static int iso_threshold_mode()
{
	uint32_t bits;
	std::memcpy(&bits, &kInv255, sizeof(bits));
	std::printf("kInv255 %08x\n", (unsigned) bits);
	unsigned in;
	while (std::scanf("%x", &in) == 1)
	{
		float iso;
		bits = in;
		std::memcpy(&iso, &bits, sizeof(iso));
		std::printf("%u\n", (unsigned) iso_threshold(iso));
	}
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 1 && std::strcmp(argv[1], "iso_threshold") == 0)
		return iso_threshold_mode();
	for (uint32_t stride_case = 0; stride_case < 2; ++stride_case)
	{        // whole schedules, and a rank's strided share of them
		const uint32_t first = stride_case ? 1u : 0u, stride = stride_case ? 3u : 1u;
		for (bool partial : {false, true})
		{
			start_order_case(1, 1, first, stride, partial);
			const uint32_t small = start_order_case(3, 2, first, stride, partial), large = start_order_case(11, 7, first, stride, partial);
			CHECK(partial ? small + large == 0 : (small > 0 && large > 0));        // the tie rule is exercised where ties exist
		}
	}
	tile_mix_case(64);
	tile_mix_case(67);
	screen_bound_tests();
	tuning_tests();
	alpha_lut_case(1.0f, 1.0f);
	alpha_lut_case(0.5f, 2.0f);
	alpha_lut_case(4.0f, 0.25f);
	resolve_rect_tests();
	VkvVolumeHeader header;
	CHECK(vkv_load_header("/nonexistent/volume.mhd", &header) == VKV_E_IO);        // the loader's C boundary links and turns the exception into a code
	CHECK(vkv_load_header(nullptr, &header) == VKV_E_INVALID_ARGUMENT);
	if (g_failed)
	{
		std::fprintf(stderr, "host arith driver: %d check(s) FAILED\n", g_failed);
		return 1;
	}
	std::printf("host arith driver: ok\n");
	return 0;
}

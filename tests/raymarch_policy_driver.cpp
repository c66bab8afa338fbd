// raymarch_policy_driver.cpp — the host-side decisions of the ray-march launchers under AddressSanitizer + UndefinedBehaviorSanitizer: the
// start-order feedback policy (frame_view, feedback_step: vkvolume_amd/host/host_arith.cpp) and the launch plan of vkv_render_batch
// (plan_batch, fill_outside_as_whole_image: vkvolume_amd/csrc/raymarch_plan.hpp).  Built and run by tests/test_raymarch_policy_cpu.py (CPU
// only, no HIP, nothing loaded into Python):
//     g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined raymarch_policy_driver.cpp
//         ../vkvolume_amd/host/host_arith.cpp ../vkvolume_amd/host/load_volume.cpp
// exit status 0 = every check passed.  Expected values are written out from the rules (which frame measures, which uses the order, what
// the grid is), not obtained by calling the code under test a second time.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../vkvolume_amd/csrc/raymarch_plan.hpp"

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

// ---- start-order feedback -----------------------------------------------------------------------------------------------------------
// a camera two units from the volume's centre (0.5, 0.5, 0.5), looking at it, `degrees` around the y axis: views 20 or more degrees
// apart are far by both rules (cos 20 = 0.94 < 0.978; moved 2 * 2 sin 10 = 0.69 > a fifth of the distance 2)
static FrameView orbit(double degrees)
{
	const double t = degrees * 3.14159265358979323846 / 180.0;
	FrameView    v;
	v.dir[0] = (float) -std::sin(t), v.dir[1] = 0.0f, v.dir[2] = (float) -std::cos(t);
	v.pos[0] = (float) (0.5 + 2.0 * std::sin(t)), v.pos[1] = 0.5f, v.pos[2] = (float) (0.5 + 2.0 * std::cos(t));
	return v;
}

static void frame_view_tests()
{
	{        // 4 x 2 pixels: the central ray is dir00 + 0.5 (4 ddx + 2 ddy) = (0, 0, 2), normalised (0, 0, 1); the position is the camera's
		const float     dir00[3] = {-1.0f, -1.0f, 2.0f}, ddx[3] = {0.5f, 0.0f, 0.0f}, ddy[3] = {0.0f, 1.0f, 0.0f}, cam[3] = {0.25f, -3.0f, 7.5f};
		const FrameView v = frame_view(dir00, ddx, ddy, cam, 4, 2);
		CHECK(v.dir[0] == 0.0f && v.dir[1] == 0.0f && v.dir[2] == 1.0f);
		CHECK(v.pos[0] == 0.25f && v.pos[1] == -3.0f && v.pos[2] == 7.5f);
	}
	{        // central ray (3, 4, 0): length 5, each component times 1 / 5 in float
		const float     dir00[3] = {1.0f, 4.0f, 0.0f}, ddx[3] = {0.5f, 0.0f, 0.0f}, ddy[3] = {0.0f, 0.0f, 0.0f}, cam[3] = {0.0f, 0.0f, 0.0f};
		const FrameView v = frame_view(dir00, ddx, ddy, cam, 8, 100);
		CHECK(v.dir[0] == 3.0f * (1.0f / 5.0f) && v.dir[1] == 4.0f * (1.0f / 5.0f) && v.dir[2] == 0.0f);
	}
	{        // no direction at all: zeros, not a division by zero
		const float     zero[3] = {0.0f, 0.0f, 0.0f};
		const FrameView v = frame_view(zero, zero, zero, zero, 16, 16);
		CHECK(v.dir[0] == 0.0f && v.dir[1] == 0.0f && v.dir[2] == 0.0f);
	}
}

static void feedback_static_camera()
{
	FeedbackState s;
	s.period = 8;        // (vkv_register_target: the tuning block's period)
	for (uint32_t i = 0; i <= 16; ++i)
	{
		const FeedbackStep r = feedback_step(s, orbit(30.0), 8);
		CHECK(r.measure == (i % 8 == 0));        // the first frame and every 8th
		CHECK(r.use_order == (i > 0));           // every frame but the first, the measuring ones included
		CHECK(s.period == 8 && s.frames == i + 1 && s.measured_at == i / 8 * 8 && s.has_cost && s.has_prev);
		CHECK(s.used == (i == 0 ? 0u : (i % 8 == 0 ? 1u : i % 8 + (i > 8 ? 1u : 0u))));        // frames in the order since the last measurement (that frame included)
	}
}

static void feedback_camera_jumps_once()
{
	FeedbackState s;
	for (uint32_t i = 0; i <= 24; ++i)
	{
		const FeedbackStep r = feedback_step(s, orbit(i == 0 ? 0.0 : 20.0), 8);
		// frames 1 .. 8 are stale (frame 8 is judged against the view measured on frame 0); 8 frames after the measurement the camera has been
		// steady since frame 2: measured, and as no frame used the first order the period doubles; 16 frames later again, period 8
		CHECK(r.measure == (i == 0 || i == 8 || i == 24));
		CHECK(r.use_order == (i >= 9));
		CHECK(s.period == (i < 8 ? 8u : (i < 24 ? 16u : 8u)));
	}
}

static void feedback_unused_measurements_saturate()
{
	// the camera jumps by 120 degrees right after every measurement and then holds still: each measurement finds that no frame used the last one
	const uint32_t measured[] = {0, 8, 24, 56, 120, 184, 248}, period_after[] = {8, 16, 32, 64, 64, 64, 64};
	FeedbackState  s;
	uint32_t       k = 0;
	for (uint32_t i = 0; i <= 248; ++i)
	{
		const FeedbackStep r = feedback_step(s, orbit(120.0 * (k % 3)), 8);
		CHECK(!r.use_order);
		CHECK(r.measure == (i == measured[k]));
		if (i == measured[k])
		{
			CHECK(s.period == period_after[k]);        // doubles up to 8 x the base period
			++k;                                       // the jump
		}
	}
	CHECK(k == 7);
}

static void feedback_alternating_views()
{
	for (uint32_t base : {8u, 1u})
	{
		FeedbackState s;
		for (uint32_t i = 0; i < 100; ++i)
		{
			const FeedbackStep r = feedback_step(s, orbit(i % 2 ? 45.0 : 0.0), base);
			CHECK(r.measure == (i == 0));                     // never steady: measured once
			CHECK(r.use_order == (i > 0 && i % 2 == 0));        // the frames at the measured view
		}
		CHECK(s.used == 49 && s.measured_at == 0);
	}
}

static void feedback_rule_boundaries()
{
	// the other view: central ray (1, 0, 0), camera 5 from the centre along z, so that a fifth of the distance is 1: 0.04f * 25 rounds to 1
	FrameView m;
	m.dir[0] = 1.0f, m.pos[0] = 0.5f, m.pos[1] = 0.5f, m.pos[2] = 5.5f;
	CHECK(0.04f * 25.0f == 1.0f);
	FrameView at_cos = m, past_cos = m, at_move = m, past_move = m;
	at_cos.dir[0] = 0.978f, past_cos.dir[0] = std::nextafterf(0.978f, 0.0f);        // the cosine is dir[0] * 1
	at_move.pos[0] = 1.5f, past_move.pos[0] = 0.5f + std::nextafterf(1.0f, 2.0f);        // moved^2 = 1 and the next float above
	CHECK(past_move.pos[0] - 0.5f == std::nextafterf(1.0f, 2.0f));
	const struct
	{
		const FrameView *view;
		bool             close;
	} cases[] = {{&m, true}, {&at_cos, true}, {&past_cos, false}, {&at_move, true}, {&past_move, false}};
	for (const auto &c : cases)
	{
		// against the MEASURED view: a measured state in the middle of its period; the previous frame was this very view
		FeedbackState s;
		s.has_cost = true, s.frames = 3, s.measured_at = 0, s.used = 2, s.measured = m, s.prev = *c.view, s.has_prev = true;
		FeedbackStep r = feedback_step(s, *c.view, 8);
		CHECK(r.use_order == c.close && !r.measure);
		CHECK(s.used == (c.close ? 3u : 2u) && s.frames == 4);
		// against the PREVIOUS frame's view: a measurement is due
		FeedbackState t;
		t.has_cost = true, t.frames = 8, t.measured_at = 0, t.used = 7, t.measured = *c.view, t.prev = m, t.has_prev = true;
		r = feedback_step(t, *c.view, 8);
		CHECK(r.measure == c.close);
		CHECK(t.measured_at == (c.close ? 8u : 0u));
		// ... and without a previous frame nothing is steady
		FeedbackState u = FeedbackState();
		u.has_cost = true, u.frames = 8, u.used = 7, u.measured = *c.view;
		CHECK(!feedback_step(u, *c.view, 8).measure && u.has_prev);
	}
}

static void feedback_base_period_one()
{
	// A static camera.  Frame 1 measures again and finds that no frame used the order measured on frame 0 (frame 0 itself had none to use):
	// the period doubles to 2 and frame 2 is the one steady frame that does not measure; frame 3 finds two users, the period is 1 again and
	// every later frame measures.
	FeedbackState s;
	s.period = 1;
	for (uint32_t i = 0; i < 40; ++i)
	{
		const FeedbackStep r = feedback_step(s, orbit(10.0), 1);
		CHECK(r.measure == (i != 2));
		CHECK(r.use_order == (i > 0));
		CHECK(s.period == (i == 1 || i == 2 ? 2u : 1u));
	}
}

// ---- the batch plan -----------------------------------------------------------------------------------------------------------------
static uint8_t g_memory[8];        // addresses to tell buffers apart (never read)

static VkvTuning tuning(int batch_mode = 0, int batch_sequential = 0)
{
	VkvTuning t;
	std::memset(&t, 0, sizeof(t));
	t.batch_mode = batch_mode, t.batch_sequential = batch_sequential;
	return t;
}

// a filled frame of `tiles` tiles of 32 x 32 pixels (four blocks)
static RayMarchArgs frame(uint32_t tiles)
{
	RayMarchArgs a;
	std::memset(&a, 0, sizeof(a));
	a.tile_count = tiles, a.blocks_per_tile = 4, a.nblocks = 4 * tiles;
	a.packed = g_memory, a.tf = g_memory + 1, a.tf_bits = reinterpret_cast<const uint32_t *>(g_memory + 4), a.addr_lut = reinterpret_cast<const uint32_t *>(g_memory);
	a.W = 64, a.H = 48, a.D = 32, a.lut_words = 120;
	for (int i = 0; i < 256; ++i)
		a.alpha_lut[i] = (float) i / 255.0f;
	return a;
}

static bool same(const LeanChoice &a, int kind, size_t lds) { return a.kind == kind && a.lds == lds; }

static void plan_tests()
{
	const LeanChoice full{2, 9000};
	const int        cus = 256;        // 8 x 256 = 2048 resident workgroups
	{        // one frame, 10 tiles: padded to 16, x 4 blocks
		const RayMarchArgs f[1] = {frame(10)};
		const LeanChoice   c[1] = {full};
		BatchPlan          p = plan_batch(f, c, 1, tuning(), cus);
		CHECK(p.max_tiles == 10 && p.ref == 0 && p.same_count && p.grid == 64 && !p.too_many && p.gpf == 0 && same(p.choice, 2, 9000) && p.no_counts && !p.pull);
		p = plan_batch(f, c, 1, tuning(1), cus);
		CHECK(p.pull && p.units == 10 * 4 * 4 && p.pull_grid == 40 && p.grid == 64);        // 160 units of 8 x 8, four per workgroup
		p = plan_batch(f, c, 1, tuning(0, 1), cus);
		CHECK(p.gpf == 8 && !p.pull);
	}
	for (uint32_t tiles : {16u, 17u})
	{        // three frames with the same tile count: a multiple of 8 as it is, 17 padded to 24
		const RayMarchArgs f[3] = {frame(tiles), frame(tiles), frame(tiles)};
		const LeanChoice   c[3] = {full, full, full};
		const uint32_t     padded = tiles == 16 ? 16 : 24;
		BatchPlan          p = plan_batch(f, c, 3, tuning(), cus);
		CHECK(p.max_tiles == tiles && p.ref == 0 && p.same_count && p.grid == padded * 4 * 3 && p.gpf == 0 && same(p.choice, 2, 9000) && p.no_counts && !p.pull);
		p = plan_batch(f, c, 3, tuning(1), cus);
		CHECK(p.pull && p.units == (uint64_t) tiles * 4 * 4 * 3 && p.pull_grid == tiles * 4 * 3);
		CHECK(plan_batch(f, c, 3, tuning(1), 4).pull_grid == 32);        // no more than eight per CU
		CHECK(plan_batch(f, c, 3, tuning(1), 0).pull_grid == 8);         // ... and at least eight
		// one frame after the other: groups of eight workgroups per frame, and no pull
		p = plan_batch(f, c, 3, tuning(1, 1), cus);
		CHECK(p.gpf == padded * 4 / 8 && !p.pull && p.grid == padded * 4 * 3);
	}
	{        // unequal tile counts: the largest sizes the grid; the pull kernel's tickets count one tile count for every frame
		const RayMarchArgs f[3] = {frame(10), frame(30), frame(20)};
		const LeanChoice   c[3] = {full, full, full};
		const BatchPlan    p = plan_batch(f, c, 3, tuning(1), cus);
		CHECK(p.max_tiles == 30 && p.ref == 0 && !p.same_count && p.grid == 32 * 4 * 3 && !p.pull && same(p.choice, 2, 9000));
	}
	{        // a leading empty frame: the reference is the first frame with tiles, whatever the empty frame's choice says
		RayMarchArgs f[3] = {frame(0), frame(12), frame(12)};
		f[0].lut_words = 0;
		const LeanChoice c[3] = {{7, 7}, full, full};
		const BatchPlan  p = plan_batch(f, c, 3, tuning(1), cus);
		CHECK(p.max_tiles == 12 && p.ref == 1 && !p.same_count && p.grid == 16 * 4 * 3 && !p.pull && same(p.choice, 2, 9000) && p.no_counts);
	}
	{        // nothing to launch
		const RayMarchArgs f[2] = {frame(0), frame(0)};
		const LeanChoice   c[2] = {full, full};
		CHECK(plan_batch(f, c, 2, tuning(), cus).max_tiles == 0);
	}
	for (int what = 0; what < 4; ++what)
	{        // frames that disagree about the tables in kind, LDS bytes or the length of the two-level tables: the plain kernel; an empty frame does not count
		RayMarchArgs f[3] = {frame(9), frame(9), frame(what == 3 ? 0 : 9)};
		LeanChoice   c[3] = {full, full, full};
		if (what == 0)
			c[2].kind = 1;
		if (what == 1)
			c[1].lds = 9016;
		if (what == 2)
			f[2].lut_words = 121;
		if (what == 3)
			c[2] = {0, 0}, f[2].lut_words = 0;
		const BatchPlan p = plan_batch(f, c, 3, tuning(), cus);
		CHECK(what == 3 ? same(p.choice, 2, 9000) : same(p.choice, 0, 0));
	}
	for (int what = 0; what < 3; ++what)
	{        // one frame reads the per-pixel counters: all run the loop with them; an empty frame's counter buffer does not count
		RayMarchArgs f[3] = {frame(9), frame(what == 2 ? 0 : 9), frame(9)};
		const LeanChoice c[3] = {full, full, full};
		if (what == 1)
			f[1].test = VKV_TEST_NUM_TEXTURE_SAMPLES;
		else
			f[1].out_counts = reinterpret_cast<uint32_t *>(g_memory);
		CHECK(plan_batch(f, c, 3, tuning(), cus).no_counts == (what == 2));
	}
	for (int what = -1; what < 8; ++what)
	{        // the pull kernel stages one set of LDS tables for all frames: each single difference forbids it
		RayMarchArgs f[3] = {frame(9), frame(9), frame(9)};
		const LeanChoice c[3] = {full, full, full};
		RayMarchArgs &   a = f[what & 1 ? 1 : 2];
		switch (what)
		{
			case 0: a.packed = g_memory + 2; break;
			case 1: a.tf_bits = nullptr; break;
			case 2: a.tf = g_memory + 3; break;
			case 3: a.addr_lut = nullptr; break;
			case 4: a.W = 65; break;
			case 5: a.H = 49; break;
			case 6: a.D = 33; break;
			case 7: a.alpha_lut[255] = std::nextafterf(1.0f, 0.0f); break;
			default: break;
		}
		CHECK(plan_batch(f, c, 3, tuning(1), cus).pull == (what < 0));
		CHECK(!plan_batch(f, c, 3, tuning(0), cus).pull);
	}
	for (uint32_t tiles : {0x1000000u - 8u, 0x1000000u})
	{        // 32 frames of 2^24 tiles x 4 blocks are 2^31 workgroups, one more than a launch takes
		std::vector<RayMarchArgs> f(32, frame(tiles));
		const std::vector<LeanChoice> c(32, full);
		const BatchPlan p = plan_batch(f.data(), c.data(), 32, tuning(), cus);
		CHECK(p.grid == (uint64_t) tiles * 4 * 32 && p.too_many == (tiles == 0x1000000u));
	}
}

static void fill_outside_tests()
{
	// an image of 10 x 10 tiles; a rendering tile fills at most kFillPerTile = 3 outside tiles
	CHECK(kFillPerTile == 3);
	CHECK(!fill_outside_as_whole_image(true, tuning(), 10, 10, 5, 5));        // 75 outside tiles, 25 inside: the workgroups fill them
	CHECK(fill_outside_as_whole_image(true, tuning(), 10, 10, 6, 4));         // 76 outside, 24 inside: too many
	CHECK(!fill_outside_as_whole_image(true, tuning(), 10, 10, 10, 10));      // nothing outside
	CHECK(fill_outside_as_whole_image(false, tuning(), 10, 10, 5, 5));        // vkv_render
	VkvTuning resident = tuning();
	resident.scheduler = 1;
	CHECK(fill_outside_as_whole_image(true, resident, 10, 10, 5, 5));          // the resident-wave scheduler
	CHECK(fill_outside_as_whole_image(true, tuning(1), 10, 10, 5, 5));         // the resident workgroups of the pull kernel
	CHECK(!fill_outside_as_whole_image(true, tuning(0, 1), 10, 10, 5, 5));     // (the frame order is no override)
	CHECK(fill_outside_as_whole_image(true, tuning(), 0x10000, 0x10000, 0x8000, 0x8000 - 1));        // 64-bit tile counts: 2^32 tiles, just under a quarter inside
	CHECK(!fill_outside_as_whole_image(true, tuning(), 0x10000, 0x10000, 0x8000, 0x8000));
}

int main()
{
	frame_view_tests();
	feedback_static_camera();
	feedback_camera_jumps_once();
	feedback_unused_measurements_saturate();
	feedback_alternating_views();
	feedback_rule_boundaries();
	feedback_base_period_one();
	plan_tests();
	fill_outside_tests();
	if (g_failed)
	{
		std::fprintf(stderr, "raymarch policy driver: %d check(s) FAILED\n", g_failed);
		return 1;
	}
	std::printf("raymarch policy driver: ok\n");
	return 0;
}

// C ABI of oracle/_ref/libvkv_ref.so: the reference's own shader text, compiled as C++ (glsl_shim.hpp + prep.py), run on the CPU over raw
// pointers.  The shaders themselves are in the generated sources; what CANNOT be compiled - the host's dispatch schedules - is restated here,
// each citing the lines of the reference it follows.  Own code, no shader text.  Test infrastructure only; not thread-safe (the shaders'
// resources are globals, as in GLSL).
#include "harness.hpp"

#include <cstdio>
#include <cstdlib>

#include "glsl_shim.hpp"
#undef in
#undef discard

static VkvRefCompFn g_comp[VKV_REF_COMP_COUNT];
static VkvRefFragFn g_frag[VKV_REF_FRAG_COUNT];

void vkv_ref_register_comp(int kind, VkvRefCompFn fn) { g_comp[kind] = fn; }
void vkv_ref_register_frag(int key, VkvRefFragFn fn) { g_frag[key] = fn; }

static uint32_t rnd_up(uint32_t a, uint32_t b) { return (a + b - 1) / b; } // rndUp of the reference's host code

static VkvRefCompFn comp(int kind)
{
	if (!g_comp[kind])
	{
		fprintf(stderr, "libvkv_ref: compute variant %d was not built\n", kind);
		abort();
	}
	return g_comp[kind];
}

extern "C" {

// 0: plain, 1: pinned (glsl_shim.hpp)
void vkv_ref_set_mode(int pinned) { glsl::g_pinned = pinned ? 1 : 0; }
int  vkv_ref_has_frag(int key) { return key >= 0 && key < VKV_REF_FRAG_COUNT && g_frag[key] != nullptr; }

// ComputeGradientMap::compute (src/compute_gradient_map.cpp): one dispatch of rndUp(extent, 8) groups per axis
void vkv_ref_gradient_map(const uint8_t *vol, uint8_t *grad, const int32_t extent[3], const VkvRefTransferFunction *tf, const uint8_t *tf_rgba8)
{
	VkvRefCompArgs a = {};
	a.image[0] = const_cast<uint8_t *>(vol), a.image[1] = grad;
	a.tf = tf, a.tf_rgba8 = tf_rgba8;
	for (int i = 0; i < 3; ++i)
		a.extent[i] = extent[i], a.groups[i] = rnd_up((uint32_t) extent[i], 8);
	comp(VKV_REF_COMP_GRADIENT)(&a);
}

// ComputeDistanceMap::computeOccupancy (src/compute_distance_map.cpp:103-140): block = rndUp(volume extent, map extent) (:110-113), pushed as
// ivec4(block, 0) (:136); dispatch of rndUp(map extent, 8) groups per axis (:137); the PRECOMPUTED_GRADIENT variant when a gradient map is bound
void vkv_ref_occupancy_map(const uint8_t *vol, const uint8_t *grad, const uint8_t *tf_rgba8, const VkvRefTransferFunction *tf,
                           const int32_t extent[3], uint8_t *map, const int32_t map_extent[3])
{
	VkvRefCompArgs a = {};
	a.image[0] = const_cast<uint8_t *>(vol), a.image[1] = const_cast<uint8_t *>(grad);
	a.tf = tf, a.tf_rgba8 = tf_rgba8, a.map = map;
	for (int i = 0; i < 3; ++i)
	{
		a.extent[i] = extent[i], a.map_extent[i] = map_extent[i];
		a.block[i]  = (int32_t) rnd_up((uint32_t) extent[i], (uint32_t) map_extent[i]);
		a.groups[i] = rnd_up((uint32_t) map_extent[i], 8);
	}
	comp(VKV_REF_COMP_OCCUPANCY + (grad ? 1 : 0))(&a);
}

static void distance_dispatch(int kind, uint8_t *dist, uint8_t *dist_swap, const int32_t e[3], uint32_t stage, int32_t dir)
{
	VkvRefCompArgs a = {};
	a.image[0] = dist, a.image[1] = dist_swap;
	a.stage = stage, a.dir = dir;
	for (int i = 0; i < 3; ++i)
		a.extent[i] = e[i];
	// stage 0: (height, depth) rows; stage 1: (width, depth); stage 2: (width, height)  (src/compute_distance_map.cpp:161, 167, 172; 206, 215, 225)
	const uint32_t gx = stage == 0 ? e[1] : e[0], gy = stage == 2 ? e[1] : e[2];
	a.groups[0] = rnd_up(gx, 8), a.groups[1] = rnd_up(gy, 8), a.groups[2] = 1;
	comp(kind)(&a);
}

// ComputeDistanceMap::computeDistance (src/compute_distance_map.cpp:142-175): stage 0 with BOTH bindings on the distance image (:156-157, the
// occupancy map transformed in place), stage 1 distance -> swap (:165-167), stage 2 swap -> distance (:171-172)
void vkv_ref_distance_map(uint8_t *map, uint8_t *swap, const int32_t e[3])
{
	distance_dispatch(VKV_REF_COMP_DISTANCE, map, map, e, 0, 0);
	distance_dispatch(VKV_REF_COMP_DISTANCE, map, swap, e, 1, 0);
	distance_dispatch(VKV_REF_COMP_DISTANCE, map, swap, e, 2, 0);
}

// ComputeDistanceMap::computeDistanceAnisotropic (src/compute_distance_map.cpp:177-252): the occupancy map is map 7 (:183).
// stage1(idx, dir): binding 0 = map idx, binding 1 = the occupancy map (:201-208); stage2(idx, dir): binding 0 = map idx, binding 1 = swap
// (:210-217); stage3(idx, dir): the same bindings, stage 2 of the shader (:219-227).  The fourteen dispatches of :238-252 in their order.
void vkv_ref_distance_map_anisotropic(uint8_t *const maps[8], uint8_t *swap, const int32_t e[3])
{
	static const struct
	{
		int     stage, idx;
		int32_t dir;
	} schedule[14] = {{1, 3, 1}, {2, 3, 1}, {3, 0, 1}, {3, 1, -1}, {2, 3, -1}, {3, 2, 1}, {3, 3, -1},
	                  {1, 7, -1}, {2, 7, 1}, {3, 4, 1}, {3, 5, -1}, {2, 7, -1}, {3, 6, 1}, {3, 7, -1}};
	for (int s = 0; s < 14; ++s)
	{
		uint8_t *other = schedule[s].stage == 1 ? maps[7] : swap;
		distance_dispatch(VKV_REF_COMP_DISTANCE_ANISO, maps[schedule[s].idx], other, e, (uint32_t) schedule[s].stage - 1, schedule[s].dir);
	}
}

// volume_render.frag for every covered pixel; `key` selects the #define variant (harness.hpp)
int vkv_ref_frag(int key, const VkvRefFragArgs *a)
{
	if (!vkv_ref_has_frag(key))
		return -1;
	g_frag[key](a);
	return 0;
}
}

// What the generated shader sources (oracle/_ref/gen/*.cpp) and harness.cpp share: the argument blocks of the C ABI and the registry
// through which each compiled variant announces its entry point.  Plain C types only; own code, no shader text.
#pragma once
#include <cstdint>

extern "C" {
struct VkvRefTransferFunction
{
	float    sampling_factor, voxel_alpha_factor, grad_magnitude_modifier;
	uint32_t use_gradient;
};

struct VkvRefCompArgs
{
	uint8_t *                     image[2]; // distance shaders: binding 0 `dist`, binding 1 `dist_swap`; gradient: volume, gradient map
	                                        // occupancy: volume, gradient map (or null)
	int32_t                       extent[3];
	uint8_t *                     map; // occupancy: the occupancy map
	int32_t                       map_extent[3];
	int32_t                       block[3];
	const uint8_t *               tf_rgba8; // 256 x 256 RGBA8
	const VkvRefTransferFunction *tf;
	uint32_t                      stage;
	int32_t                       dir;
	uint32_t                      groups[3]; // the dispatch, in work groups of 8 (x 8 (x 8))
};

struct VkvRefFragArgs
{
	const float *  entry; // [height][width][4]: rgb = the interpolant `ray_entry`, a > 0 where the rasteriser produces a fragment
	const float *  in_depth; // [height][width] scene depth (DEPTH_ATTACHMENT variants) or null
	int32_t        width, height;
	float          view[16], proj[16], view_proj_inv[16], model[16], model_inv[16];
	float          cam_pos_tex[4], block_size[4];
	VkvRefTransferFunction tf;
	const uint8_t *volume, *gradient, *tf_rgba8;
	int32_t        extent[3];
	const uint8_t *maps[8];
	int32_t        map_extent[3];
	float *        out_color;    // [height][width][4]
	uint32_t *     out_counts;   // [height][width][3]: volume samples, distance probes, empty samples
	float *        out_depth;    // [height][width]: gl_FragDepth
	uint8_t *      out_fragment; // [height][width]: 1 = a fragment was written (covered and not discarded)
};
}

typedef void (*VkvRefCompFn)(const VkvRefCompArgs *);
typedef void (*VkvRefFragFn)(const VkvRefFragArgs *);

// preprocessor constants: the runners select code with #if on them
#define VKV_REF_COMP_GRADIENT 0
#define VKV_REF_COMP_OCCUPANCY 1 // + 1 with PRECOMPUTED_GRADIENT
#define VKV_REF_COMP_DISTANCE 3
#define VKV_REF_COMP_DISTANCE_ANISO 4
#define VKV_REF_COMP_COUNT 5
#define VKV_REF_FRAG_COUNT 96 // skip (0..3) | no ERT << 2 | precomputed gradient << 3 | depth attachment << 4 | (show 0..2) << 5

void vkv_ref_register_comp(int kind, VkvRefCompFn fn);
void vkv_ref_register_frag(int key, VkvRefFragFn fn);

struct VkvRefRegisterComp
{
	VkvRefRegisterComp(int kind, VkvRefCompFn fn) { vkv_ref_register_comp(kind, fn); }
};
struct VkvRefRegisterFrag
{
	VkvRefRegisterFrag(int key, VkvRefFragFn fn) { vkv_ref_register_frag(key, fn); }
};

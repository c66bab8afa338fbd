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

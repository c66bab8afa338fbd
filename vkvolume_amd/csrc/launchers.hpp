// launchers.hpp — every function of the library that crosses a translation unit on the host side: the kernel launchers, the limits the
// entry points check before they enqueue anything, and the few helpers of raymarch.hip that capi.hip calls.  capi.hip and every file that
// defines one of them include it, so a changed signature is a compile error, not a link error.  All of them return VKV_OK or an error code
// with the context's error text set; `s` is the stream the work is enqueued on; device pointers are named d_*.
#pragma once

#include "vkv_device.hpp"

namespace vkv
{
// ---- gradient.hip
// vkv_gradient_map: the gradient of every voxel of e; _box: of the voxels of b (inside e)
int launch_gradient_map(vkv_ctx *ctx, const uint8_t *d_vol, uint8_t *d_grad, VkvExtent3D e, const VkvTransferFunctionUniform *tf, hipStream_t s);
int launch_gradient_map_box(vkv_ctx *ctx, const uint8_t *d_vol, uint8_t *d_grad, VkvExtent3D e, const VkvBox &b, const VkvTransferFunctionUniform *tf,
                            hipStream_t s);
// vkv_debug_check: device arithmetic `what` (0 .. 4) against its IEEE definition for `count` floats from bit pattern first_bits
int launch_check_numerics(vkv_ctx *ctx, int what, uint32_t first_bits, uint64_t count, unsigned long long *d_mismatches, hipStream_t s);

// ---- occupancy.hip
// what the occupancy pass (whole map or a region update's cells) can take in one launch
bool occupancy_launch_ok(VkvExtent3D e, VkvExtent3D me);
// what the voxel count can take
bool count_launch_ok(VkvExtent3D e);
// the occupancy bit table of an RGBA8 texture in d_bits (the stream's scratch block; the caller holds its lock); _columns: and the column
// mask behind it, i.e. what launch_occupancy_map takes as bits_ready
int launch_tf_bits(vkv_ctx *ctx, const uint8_t *d_tf, uint32_t *d_bits, hipStream_t s);
int launch_tf_bits_columns(vkv_ctx *ctx, const uint8_t *d_tf, uint32_t *d_bits, hipStream_t s);
// vkv_occupancy_map: every cell of the map.  bits_ready: d_bits already holds the bit table and its column mask; d_tf is then not read, and
// the map is filled by a kernel, not a memset
int launch_occupancy_map(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf,
                         VkvExtent3D e, uint8_t *d_map, VkvExtent3D me, hipStream_t s, uint32_t *d_bits, bool bits_ready = false);
// the cells [c0, c1) per axis of the map from the bit table in d_bits (ready); from_distance: d_map holds a distance transform of the
// occupancy and is first turned back into it
int launch_occupancy_map_cells(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, const VkvTransferFunctionUniform *tf, VkvExtent3D e,
                               uint8_t *d_map, VkvExtent3D me, const uint32_t c0[3], const uint32_t c1[3], bool from_distance, hipStream_t s,
                               uint32_t *d_bits);
// vkv_occupied_voxel_count: the analytic transfer function's occupied voxels into *d_count (d_bits as above)
int launch_occupied_voxel_count(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, const VkvTransferFunctionUniform *tf, VkvExtent3D e,
                                uint64_t *d_count, hipStream_t s, uint32_t *d_bits);

// ---- distance.hip
// what the distance transforms can take in one launch
bool distance_launch_ok(VkvExtent3D me);
// vkv_distance_map: d_map in place (d_swap: a buffer of the map's size); _anisotropic: the eight octant maps from the occupancy in d_maps[7]
int launch_distance_map(vkv_ctx *ctx, uint8_t *d_map, uint8_t *d_swap, VkvExtent3D me, hipStream_t s);
int launch_distance_map_anisotropic(vkv_ctx *ctx, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D me, hipStream_t s);
// skipping_type's transform of the occupancy map in d_maps[0] (anisotropic: d_maps[7]); nothing for NONE and BLOCK
int launch_map_transform(vkv_ctx *ctx, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D me, int skipping_type, hipStream_t s);

// ---- pack.hip
// vkv_pack_volume: every brick of the packed sampling image; _bricks: the bricks [b0, b1) per axis
int launch_pack_volume(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, void *d_packed, hipStream_t s);
int launch_pack_volume_bricks(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, const int b0[3], const int b1[3], void *d_packed,
                              hipStream_t s);

// ---- tf_tables.hip
// the integrator's tables of an RGBA8 texture (bit table, separable alpha tables, flag word); tf null: no separable claim
int launch_tf_tables(vkv_ctx *ctx, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf, uint32_t *d_tables, hipStream_t s);
// the texture, its tables and (d_bits non-null) the occupancy bit table + column mask from the uniform's fields alone
int launch_tf_build(vkv_ctx *ctx, const VkvTransferFunctionUniform *tf, uint8_t *d_tf, uint32_t *d_tables, uint32_t *d_bits, hipStream_t s);

// ---- volume_io.hip
// vkv_synth_volume: kind 0 = sphere, 1 (+ modifiers in the upper bits) = shells of `seed`
int launch_synth_volume(vkv_ctx *ctx, uint8_t *d_vol, VkvExtent3D e, uint32_t kind, uint32_t seed, hipStream_t s);
// the loader's conversion of n raw elements (VKV_VOXEL_* type, [lo, hi] -> [0, 255]); _box: of a box's elements into its voxels of the volume e
int launch_convert_volume(vkv_ctx *ctx, const void *d_raw, int type, bool big_endian, float lo, float hi, uint64_t n, uint8_t *d_out, hipStream_t s);
int launch_convert_box(vkv_ctx *ctx, const void *d_raw, int type, bool big_endian, float lo, float hi, const VkvBox &box, uint8_t *d_vol, VkvExtent3D e,
                       hipStream_t s);
// vkv_scatter_tiles: n frames (1 .. VKV_MAX_BATCH) of gathered per-rank tile buffers into their images
int launch_scatter_tiles_frames(vkv_ctx *ctx, uint32_t n, void *const *images, const void *const *srcs, const VkvTileRect *rects, const uint32_t *strides,
                                uint32_t iw, uint32_t ih, uint32_t tw, uint32_t th, uint32_t n_ranks, uint32_t bpp, hipStream_t s);

// ---- region.hip
// vkv_update_volume_region after the entry point's argument checks: convert the box, then its gradient, bricks, occupancy cells and the transform
int launch_update_volume_region(vkv_ctx *ctx, const void *d_src, int type, bool big_endian, float lo, float hi, const VkvBox &box, uint8_t *d_vol,
                                uint8_t *d_grad, void *d_packed, VkvExtent3D e, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf,
                                uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D me, int skipping_type, hipStream_t s);

// ---- histogram.hip
// vkv_volume_histogram after the entry point's argument checks; the occupied-voxel count of the analytic transfer function from a histogram
int launch_volume_histogram(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, const VkvBox &b, int mode, uint64_t *d_hist,
                            hipStream_t s);
int launch_histogram_occupied_count(vkv_ctx *ctx, const uint64_t *d_hist, const VkvTransferFunctionUniform *tf, uint64_t *d_count, hipStream_t s);

// ---- cells.hip
// what the summary and classify launches can take
bool cells_launch_ok(VkvExtent3D e, VkvExtent3D me);
// vkv_cell_summary: the cells that meet b (the whole map when b is null)
int launch_cell_summary(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, VkvExtent3D me, const VkvBox *b, void *d_summary,
                        hipStream_t s);
// the occupancy map from the summary, with the bit table already in the stream's scratch block `scratch` (the caller holds its lock)
int launch_occupancy_from_summary(vkv_ctx *ctx, const void *d_summary, const uint8_t *d_vol, const uint8_t *d_grad, bool use_gradient, uint8_t *scratch,
                                  VkvExtent3D e, uint8_t *d_map, VkvExtent3D me, uint64_t *d_unresolved, hipStream_t s);

// ---- filter.hip
// what the filter launch can take
bool filter_launch_ok(VkvExtent3D e);
// vkv_filter_volume after the entry point's argument checks: the voxels of b (inside e) of d_dst from d_src, kind a VkvFilterKind
int launch_filter_volume(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, int kind, hipStream_t s);

// ---- mesh.hip
// vkv_isosurface_mesh_scratch_bytes: 0 for an extent or box that is not accepted; what the launches can take (box null: the whole volume)
size_t mesh_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   mesh_launch_ok(VkvExtent3D e, const VkvBox *box);
// vkv_isosurface_mesh after the entry point's argument checks (b inside e; me is read with a max map only)
int launch_isosurface_mesh(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint8_t *d_max_map, VkvExtent3D me,
                           void *d_scratch, float *d_triangles, uint64_t capacity, uint64_t *d_counts, hipStream_t s);

// ---- raymarch.hip
// vkv_render /vkv_render_batch (n frames in one launch) after the entry point's argument checks
int launch_render(vkv_ctx *ctx, const VkvRenderParams *P, const float *alpha_lut, hipStream_t s);
int launch_render_batch(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, const float *alpha_luts, hipStream_t s);
// vkv_prepare_render: everything a later launch of these n parameter blocks on s takes from the context, created now
int prepare_render(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, hipStream_t s);
// vkv_screen_tile_rect: the screen bound of the volume's box in whole tiles
void screen_tile_rect(const VkvRayCastUniform *rc, const VkvRayGen *rg, uint32_t iw, uint32_t ih, uint32_t tw, uint32_t th, uint32_t align, VkvTileRect *out);
// loads the start-order kernels' code object on the current device (vkv_register_target)
void load_feedback_code();

// ---- checks of a VkvRenderParams that vkv_render / vkv_render_batch (capi.hip) and the direct renderers (direct_render.hpp) share.  Defined here
// (static: no symbol) because their callers are in different translation units; `what` is the entry point's name in the messages.
// The tile schedule: tile size a multiple of 16 and tile_stride > 0, the rectangle inside the image, the schedule inside the image or the
// rectangle.  (The fill_outside check sits between them, where vkv_render has always had it; the direct renderers reject fill_outside before.)
static int check_tile_schedule(vkv_ctx *ctx, const char *what, const VkvRenderParams *P)
{
	const VkvTileSchedule &t = P->tiles;
	if (t.tile_width == 0 || t.tile_height == 0 || (t.tile_width % 16) || (t.tile_height % 16) || t.tile_stride == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: tile size must be a positive multiple of 16 and tile_stride > 0", what);
	const uint64_t tiles_x = (P->image_width + t.tile_width - 1) / t.tile_width, tiles_y = (P->image_height + t.tile_height - 1) / t.tile_height;
	const bool     whole   = t.rect.w == 0 || t.rect.h == 0;
	if (!whole && ((uint64_t) t.rect.x0 + t.rect.w > tiles_x || (uint64_t) t.rect.y0 + t.rect.h > tiles_y))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: the schedule's tile rectangle runs past the image", what);
	if (t.fill_outside && !whole && (t.compact || t.tile_first != 0 || t.tile_stride != 1 || (uint64_t) t.tile_count != (uint64_t) t.rect.w * t.rect.h))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: fill_outside needs image-indexed outputs and the whole rectangle in one launch (tile_first 0, tile_stride 1)", what);
	const uint64_t scheduled = whole ? tiles_x * tiles_y : (uint64_t) t.rect.w * t.rect.h;
	if (t.tile_count && (uint64_t) t.tile_first + (uint64_t) (t.tile_count - 1) * t.tile_stride >= scheduled)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: tile schedule runs past the %s", what, whole ? "image" : "tile rectangle");
	return VKV_OK;
}
// The buffers: the packed image's alignment, and at least one output (own_output: an output of the entry point's own options is set)
static int check_render_buffers(vkv_ctx *ctx, const char *what, const VkvRenderParams *P, bool own_output)
{
	if (P->d_packed_volume && ((uintptr_t) P->d_packed_volume & 255u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_packed_volume must be 256-byte aligned", what);
	if (!P->d_out_color && !P->d_out_rgba8 && !P->d_out_counts && !P->d_out_depth && !own_output)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: no output buffer", what);
	return VKV_OK;
}
}        // namespace vkv

// capi.hip — the device entry points of include/vkvolume_amd.h: each checks its arguments and calls one launcher (launchers.hpp).  The
// context and its entry points are context.hip's, the multi-GPU exchange is exchange.hip's, the helpers that never touch a device
// are ../host/host_arith.cpp's.
#include <cmath>
#include <cstring>
#include <vector>

#include "box_domain.hpp"

namespace vkv
{
int check_box(vkv_ctx *ctx, const char *what, VkvExtent3D extent, const VkvBox *box)
{
	if (!box || extent_and_box_ok(extent, box))
		return VKV_OK;
	const VkvBox b = *box;
	if (b.width == 0 || b.height == 0 || b.depth == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: empty box", what);
	return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: box (%u, %u, %u) + (%u, %u, %u) outside the volume", what, b.x0, b.y0, b.z0, b.width, b.height, b.depth);
}

// skipping_type's maps: 8 for ANISOTROPIC_DISTANCE, else 1, and for the distance transforms a swap buffer that is none of them
static int check_map_buffers(vkv_ctx *ctx, const char *what, uint8_t *const d_maps[8], const uint8_t *d_swap, int32_t skipping_type)
{
	if (skipping_type < VKV_SKIP_NONE || skipping_type > VKV_SKIP_ANISOTROPIC_DISTANCE)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: bad skipping_type %d", what, (int) skipping_type);
	if (!d_maps)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null maps", what);
	const bool transform = skipping_type == VKV_SKIP_DISTANCE || skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE;
	const int  n         = skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE ? 8 : 1;
	if (transform && !d_swap)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null swap buffer", what);
	for (int i = 0; i < n; ++i)
		if (!d_maps[i] || (transform && d_maps[i] == d_swap))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: map %d %s", what, i, d_maps[i] ? "aliases the swap buffer" : "is null");
	return VKV_OK;
}

// the maps' buffers (VKV_E_INVALID_ARGUMENT), then the limits of the occupancy pass (from_summary: the classify launch) and of the transform
// (VKV_E_UNSUPPORTED): what an entry point that builds the maps checks before it enqueues anything (extent and map_extent are valid)
static int check_maps(vkv_ctx *ctx, const char *what, uint8_t *const d_maps[8], const uint8_t *d_swap, VkvExtent3D extent, VkvExtent3D map_extent,
                      int32_t skipping_type, bool from_summary = false)
{
	if (const int rc = check_map_buffers(ctx, what, d_maps, d_swap, skipping_type))
		return rc;
	if (!(from_summary ? cells_launch_ok(extent, map_extent) : occupancy_launch_ok(extent, map_extent)))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: map too large for one launch", what);
	if ((skipping_type == VKV_SKIP_DISTANCE || skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE) && !distance_launch_ok(map_extent))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: map rows too long for the distance transform", what);
	return VKV_OK;
}

// ---- a VkvRenderParams' checks that vkv_render / vkv_render_batch share with the direct renderers (direct_render.hpp) ----
// The tile schedule: tile size a multiple of 16 and tile_stride > 0, the rectangle inside the image, the schedule inside the image or the
// rectangle.  (The fill_outside check sits between them, where vkv_render has always had it; the direct renderers reject fill_outside before.)
int check_tile_schedule(vkv_ctx *ctx, const char *what, const VkvRenderParams *P)
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
int check_render_buffers(vkv_ctx *ctx, const char *what, const VkvRenderParams *P, bool own_output)
{
	if (P->d_packed_volume && ((uintptr_t) P->d_packed_volume & 255u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_packed_volume must be 256-byte aligned", what);
	if (!P->d_out_color && !P->d_out_rgba8 && !P->d_out_counts && !P->d_out_depth && !own_output)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: no output buffer", what);
	return VKV_OK;
}

// d_src and d_dst, each of extent's bytes, do not overlap, or (allow_equal: the call works in place) are the same buffer
static int check_in_place_or_disjoint(vkv_ctx *ctx, const char *what, const void *d_src, const void *d_dst, VkvExtent3D extent, bool allow_equal)
{
	const unsigned __int128 bytes = (unsigned __int128) extent.width * extent.height * extent.depth;
	const uint64_t          n     = bytes > ~0ull ? ~0ull : (uint64_t) bytes;
	const uintptr_t         a = (uintptr_t) d_src, b = (uintptr_t) d_dst;
	if ((allow_equal && a == b) || (a < b ? b - a : a - b) >= n)
		return VKV_OK;
	return set_error(ctx, VKV_E_INVALID_ARGUMENT,
	                 allow_equal ? "%s: d_src and d_dst overlap without being equal" : "%s: d_src and d_dst overlap (the filter does not run in place)", what);
}
// the transfer-function texture and its tables are read and written as dwords
static bool tf_pointers_aligned(const void *d_tf, const void *d_tables) { return (((uintptr_t) d_tf | (uintptr_t) d_tables) & 3u) == 0; }

// ---- what the four mesh extractors check alike (vkv_isosurface_mesh, _indexed, vkv_label_mesh, _indexed); each calls them in this order ----
// the pointers every call needs, iso, the box
// d_input: the volume or the labels; iso_when: null where iso is not read, else what follows "iso must be finite"
static int check_mesh_inputs(vkv_ctx *ctx, const char *what, const void *d_input, const void *d_scratch, const void *d_counts, VkvExtent3D extent, float iso,
                             const char *iso_when, const VkvBox *box)
{
	if (!d_input || !d_scratch || !d_counts || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null pointer or zero extent", what);
	if (iso_when && !std::isfinite(iso))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: iso must be finite%s", what, iso_when);
	return check_box(ctx, what, extent, box);
}
// the max map or the visibility map (`map_name`), where one is given
static int check_skip_map(vkv_ctx *ctx, const char *what, const char *map_name, const uint8_t *d_map, VkvExtent3D extent, VkvExtent3D map_extent)
{
	if (d_map && !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: the %s needs a valid map_extent", what, map_name);
	return VKV_OK;
}
// the colour table of the label meshes, the visibility map's need of it, and the map
static int check_label_table(vkv_ctx *ctx, const char *what, const uint32_t *d_colors, uint64_t table_entries, const uint8_t *d_visibility_map, VkvExtent3D extent,
                             VkvExtent3D map_extent)
{
	if (!d_colors && table_entries != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: a table of %llu entries needs d_colors", what, (unsigned long long) table_entries);
	if (d_visibility_map && !d_colors)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: a visibility map needs the d_colors it was built from", what);
	return check_skip_map(ctx, what, "visibility map", d_visibility_map, extent, map_extent);
}
// a capacity of `things` needs its outputs (`names`)
static int check_capacity(vkv_ctx *ctx, const char *what, uint64_t capacity, const char *things, bool have_outputs, const char *names)
{
	if (capacity != 0 && !have_outputs)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: a capacity of %llu %s needs %s", what, (unsigned long long) capacity, things, names);
	return VKV_OK;
}
// the indexed meshes' vertices: numbered in 32 bits, and written to d_vertices
static int check_vertex_capacity(vkv_ctx *ctx, const char *what, uint64_t capacity_vertices, const float *d_vertices)
{
	if (capacity_vertices > 0xffffffffull)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: a capacity of %llu vertices is past 32-bit indices; split the surface by boxes", what,
		                 (unsigned long long) capacity_vertices);
	return check_capacity(ctx, what, capacity_vertices, "vertices", d_vertices != nullptr, "d_vertices");
}
// any_dword: the bitwise or of the pointers that are read or written as dwords, `names`
static int check_mesh_alignment(vkv_ctx *ctx, const char *what, const void *d_scratch, const void *d_counts, uintptr_t any_dword, const char *names)
{
	if ((((uintptr_t) d_scratch | (uintptr_t) d_counts) & 7u) != 0 || (any_dword & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_scratch and d_counts must be 8-byte aligned, %s 4-byte aligned", what, names);
	return VKV_OK;
}
// labels: a label array's 2^32 - 1 voxels first; launch_ok: the unit's *_launch_ok
static int check_mesh_limits(vkv_ctx *ctx, const char *what, VkvExtent3D extent, const VkvBox *box, bool labels, bool (*launch_ok)(VkvExtent3D, const VkvBox *))
{
	if (labels && !components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a box of more than 2^32 - 1 voxels", what);
	if (!launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: volume too large for the launches", what);
	return VKV_OK;
}

}        // namespace vkv

using namespace vkv;

extern "C" {

int vkv_gradient_map(vkv_ctx *ctx, const uint8_t *d_volume, uint8_t *d_gradient, VkvExtent3D extent, const VkvTransferFunctionUniform *tf, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_gradient || !tf || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "gradient_map: null pointer or zero extent");
	return launch_gradient_map(ctx, d_volume, d_gradient, extent, tf, (hipStream_t) stream);
}

int vkv_occupancy_map(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf,
                      VkvExtent3D extent, uint8_t *d_map, VkvExtent3D map_extent, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_tf || !tf || !d_map || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "occupancy_map: null pointer or bad extent");
	const StreamScratch scratch = stream_scratch(ctx, (hipStream_t) stream);        // the bit table, written and read by the launches below
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	return launch_occupancy_map(ctx, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, (hipStream_t) stream,
	                            reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset));
}

int vkv_distance_map(vkv_ctx *ctx, uint8_t *d_map, uint8_t *d_swap, VkvExtent3D map_extent, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int rc = check_map_buffers(ctx, "distance_map", &d_map, d_swap, VKV_SKIP_DISTANCE);
	return rc != VKV_OK ? rc : launch_distance_map(ctx, d_map, d_swap, map_extent, (hipStream_t) stream);
}

int vkv_distance_map_anisotropic(vkv_ctx *ctx, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D map_extent, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int rc = check_map_buffers(ctx, "distance_map_anisotropic", d_maps, d_swap, VKV_SKIP_ANISOTROPIC_DISTANCE);
	return rc != VKV_OK ? rc : launch_distance_map_anisotropic(ctx, d_maps, d_swap, map_extent, (hipStream_t) stream);
}

// src/compute_distance_map.cpp:65-101: every argument is checked before the first launch
int vkv_compute_distance_map(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf,
                             VkvExtent3D extent, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D map_extent, int32_t skipping_type, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_tf || !tf || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "compute_distance_map: null pointer or bad extent");
	int rc = check_maps(ctx, "compute_distance_map", d_maps, d_swap, extent, map_extent, skipping_type);
	if (rc != VKV_OK)
		return rc;
	const hipStream_t   s       = (hipStream_t) stream;
	const StreamScratch scratch = stream_scratch(ctx, s);        // the bit table, written and read by the occupancy pass
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	uint8_t *occ = d_maps[skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE ? 7 : 0];
	if ((rc = launch_occupancy_map(ctx, d_volume, d_gradient, d_tf, tf, extent, occ, map_extent, s, reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset))) != VKV_OK)
		return rc;
	return launch_map_transform(ctx, d_maps, d_swap, map_extent, skipping_type, s);
}

int vkv_occupied_voxel_count(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, const VkvTransferFunctionUniform *tf, VkvExtent3D extent,
                             uint64_t *d_count, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !tf || !d_count || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "occupied_voxel_count: null pointer or zero extent");
	const StreamScratch scratch = stream_scratch(ctx, (hipStream_t) stream);
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	return launch_occupied_voxel_count(ctx, d_volume, d_gradient, tf, extent, d_count, (hipStream_t) stream, reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset));
}

int vkv_convert_volume(vkv_ctx *ctx, const void *d_raw, int32_t type, int32_t big_endian, float range_min, float range_max, uint64_t n_voxels,
                       uint8_t *d_out, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_raw || !d_out)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "convert_volume: null pointer");
	if ((type == VKV_VOXEL_UINT16 || type == VKV_VOXEL_INT16) && (((uintptr_t) d_raw) & 1u))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "convert_volume: 16-bit input must be 2-byte aligned");
	return launch_convert_volume(ctx, d_raw, type, big_endian != 0, range_min, range_max, n_voxels, d_out, (hipStream_t) stream);
}

size_t vkv_packed_volume_bytes(VkvExtent3D e)
{
	if (!extent_ok(e))
		return 0;
	return packed_bytes(packed_dims((int) e.width, (int) e.height, (int) e.depth));
}

int vkv_pack_volume(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent, void *d_packed, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_packed || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "pack_volume: null pointer or zero extent");
	if (((uintptr_t) d_packed & 255u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "pack_volume: d_packed must be 256-byte aligned");
	return launch_pack_volume(ctx, d_volume, d_gradient, extent, d_packed, (hipStream_t) stream);
}

int vkv_transfer_function_tables(vkv_ctx *ctx, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf, uint32_t *d_tables, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_tf || !d_tables)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "transfer_function_tables: null pointer");
	if (!tf_pointers_aligned(d_tf, d_tables))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "transfer_function_tables: pointers must be 4-byte aligned");
	return launch_tf_tables(ctx, d_tf, tf, d_tables, (hipStream_t) stream);
}

int vkv_transfer_function_bits(vkv_ctx *ctx, const uint8_t *d_tf, uint32_t *d_tables, void *stream)
{
	return vkv_transfer_function_tables(ctx, d_tf, nullptr, d_tables, stream);
}

int vkv_transfer_function_texture_device(vkv_ctx *ctx, const VkvVolumeOptions *options, uint8_t *d_tf, uint32_t *d_tables, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!options || !d_tf || !d_tables)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "transfer_function_texture_device: null pointer");
	if (!tf_pointers_aligned(d_tf, d_tables))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "transfer_function_texture_device: pointers must be 4-byte aligned");
	VkvTransferFunctionUniform tf;
	vkv_transfer_function_uniform(options, &tf);        // the same i_inv / g_inv the host texture is built with
	return launch_tf_build(ctx, &tf, d_tf, d_tables, nullptr, (hipStream_t) stream);
}

// src/volume_render.cpp:392-445 as one enqueue: every argument is checked before the first launch
int vkv_update_transfer_function(vkv_ctx *ctx, const VkvVolumeOptions *options, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent,
                                 uint8_t *d_tf, uint32_t *d_tables, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D map_extent,
                                 int32_t skipping_type, uint64_t *d_occupied_count, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!options || !d_volume || !d_tf || !d_tables || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_transfer_function: null pointer or bad extent");
	if (!tf_pointers_aligned(d_tf, d_tables))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_transfer_function: d_transfer_function and d_tables must be 4-byte aligned");
	int rc = check_maps(ctx, "update_transfer_function", d_maps, d_swap, extent, map_extent, skipping_type);
	if (rc != VKV_OK)
		return rc;
	if (d_occupied_count && !count_launch_ok(extent))
		return set_error(ctx, VKV_E_UNSUPPORTED, "update_transfer_function: volume too large for the voxel count");
	const hipStream_t   s       = (hipStream_t) stream;
	const StreamScratch scratch = stream_scratch(ctx, s);        // held until the occupancy pass is enqueued
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	uint32_t *d_bits = reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset);
	VkvTransferFunctionUniform tf;
	vkv_transfer_function_uniform(options, &tf);
	// the count first: it stages its own (analytic) bit table in the same scratch words that k_tf_build fills for the occupancy pass
	if (d_occupied_count && (rc = launch_occupied_voxel_count(ctx, d_volume, d_gradient, &tf, extent, d_occupied_count, s, d_bits)) != VKV_OK)
		return rc;
	if ((rc = launch_tf_build(ctx, &tf, d_tf, d_tables, d_bits, s)) != VKV_OK)
		return rc;
	uint8_t *occ = d_maps[skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE ? 7 : 0];
	if ((rc = launch_occupancy_map(ctx, d_volume, d_gradient, d_tf, &tf, extent, occ, map_extent, s, d_bits, true)) != VKV_OK)
		return rc;
	return launch_map_transform(ctx, d_maps, d_swap, map_extent, skipping_type, s);
}

// every argument is checked before the first launch (the volume's size limits by launch_update_volume_region)
int vkv_update_volume_region(vkv_ctx *ctx, const void *d_src, int32_t type, int32_t big_endian, float range_min, float range_max, const VkvBox *box,
                             uint8_t *d_volume, uint8_t *d_gradient, void *d_packed, VkvExtent3D extent, const uint8_t *d_tf,
                             const VkvTransferFunctionUniform *tf, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D map_extent, int32_t skipping_type,
                             void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_src || !box || !d_volume || !tf || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_volume_region: null pointer or zero extent");
	int rc = check_box(ctx, "update_volume_region", extent, box);
	if (rc != VKV_OK)
		return rc;
	if (type < VKV_VOXEL_UINT8 || type > VKV_VOXEL_INT16)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_volume_region: unsupported image data type %d", (int) type);
	if ((type == VKV_VOXEL_UINT16 || type == VKV_VOXEL_INT16) && (((uintptr_t) d_src) & 1u))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_volume_region: 16-bit input must be 2-byte aligned");
	if (d_packed && ((uintptr_t) d_packed & 255u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_volume_region: d_packed must be 256-byte aligned");
	if (d_maps)
	{
		if (!d_tf || !map_extent_ok(extent, map_extent))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_volume_region: null transfer function or bad map extent");
		if ((rc = check_maps(ctx, "update_volume_region", d_maps, d_swap, extent, map_extent, skipping_type)) != VKV_OK)
			return rc;
	}
	return launch_update_volume_region(ctx, d_src, type, big_endian != 0, range_min, range_max, *box, d_volume, d_gradient, d_packed, extent, d_tf, tf, d_maps,
	                                   d_swap, map_extent, skipping_type, (hipStream_t) stream);
}

// every argument is checked before the first launch
int vkv_volume_histogram(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent, const VkvBox *box, int32_t mode,
                         uint64_t *d_histogram, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_histogram || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "volume_histogram: null pointer or zero extent");
	if (const int rc = check_box(ctx, "volume_histogram", extent, box))
		return rc;
	if (mode < VKV_HISTOGRAM_SET || mode > VKV_HISTOGRAM_SUBTRACT)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "volume_histogram: bad mode %d", (int) mode);
	if (((uintptr_t) d_histogram & 7u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "volume_histogram: d_histogram must be 8-byte aligned");
	return launch_volume_histogram(ctx, d_volume, d_gradient, extent, whole_or(extent, box), mode, d_histogram, (hipStream_t) stream);
}

int vkv_histogram_occupied_count(vkv_ctx *ctx, const uint64_t *d_histogram, const VkvTransferFunctionUniform *tf, uint64_t *d_count, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_histogram || !tf || !d_count)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "histogram_occupied_count: null pointer");
	if ((((uintptr_t) d_histogram) | ((uintptr_t) d_count)) & 7u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "histogram_occupied_count: d_histogram and d_count must be 8-byte aligned");
	return launch_histogram_occupied_count(ctx, d_histogram, tf, d_count, (hipStream_t) stream);
}

// every argument is checked before the first launch (and before the device is touched)
int vkv_filter_volume(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box, int32_t kind, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_src || !d_dst || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "filter_volume: null pointer or zero extent");
	if (kind != VKV_FILTER_BINOMIAL3 && kind != VKV_FILTER_MEDIAN3)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "filter_volume: unknown kind %d", (int) kind);
	if (const int rc = check_box(ctx, "filter_volume", extent, box))
		return rc;
	if (!filter_launch_ok(extent))
		return set_error(ctx, VKV_E_UNSUPPORTED, "filter_volume: volume too large for one launch");
	if (const int rc = check_in_place_or_disjoint(ctx, "filter_volume", d_src, d_dst, extent, false))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_filter_volume(ctx, d_src, d_dst, extent, whole_or(extent, box), kind, (hipStream_t) stream);
}

size_t vkv_isosurface_mesh_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return mesh_scratch_bytes(extent, box); }

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_isosurface_mesh(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, const uint8_t *d_max_map,
                        VkvExtent3D map_extent, void *d_scratch, float *d_triangles, uint64_t capacity_triangles, uint64_t *d_counts, void *stream)
{
	const char *what = "isosurface_mesh";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_inputs(ctx, what, d_volume, d_scratch, d_counts, extent, iso, "", box))
		return rc;
	if (const int rc = check_skip_map(ctx, what, "max map", d_max_map, extent, map_extent))
		return rc;
	if (const int rc = check_capacity(ctx, what, capacity_triangles, "triangles", d_triangles != nullptr, "d_triangles"))
		return rc;
	if (const int rc = check_mesh_alignment(ctx, what, d_scratch, d_counts, (uintptr_t) d_triangles, "d_triangles"))
		return rc;
	if (const int rc = check_mesh_limits(ctx, what, extent, box, false, mesh_launch_ok))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_isosurface_mesh(ctx, d_volume, extent, whole_or(extent, box), iso, d_max_map, map_extent,
	                              d_scratch, d_triangles, capacity_triangles, d_counts, (hipStream_t) stream);
}

size_t vkv_isosurface_mesh_indexed_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return mesh_indexed_scratch_bytes(extent, box); }

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_isosurface_mesh_indexed(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, const uint8_t *d_max_map,
                                VkvExtent3D map_extent, void *d_scratch, float *d_vertices, float *d_normals, uint64_t capacity_vertices,
                                uint32_t *d_indices, uint64_t capacity_triangles, uint64_t *d_counts, void *stream)
{
	const char *what = "isosurface_mesh_indexed";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_inputs(ctx, what, d_volume, d_scratch, d_counts, extent, iso, "", box))
		return rc;
	if (const int rc = check_skip_map(ctx, what, "max map", d_max_map, extent, map_extent))
		return rc;
	if (const int rc = check_vertex_capacity(ctx, what, capacity_vertices, d_vertices))
		return rc;
	if (capacity_vertices == 0 && d_normals)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_normals needs a capacity of vertices", what);
	if (const int rc = check_capacity(ctx, what, capacity_triangles, "triangles", d_indices != nullptr, "d_indices"))
		return rc;
	if (const int rc = check_mesh_alignment(ctx, what, d_scratch, d_counts, (uintptr_t) d_vertices | (uintptr_t) d_normals | (uintptr_t) d_indices,
	                                        "d_vertices, d_normals and d_indices"))
		return rc;
	if (const int rc = check_mesh_limits(ctx, what, extent, box, false, mesh_indexed_launch_ok))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_isosurface_mesh_indexed(ctx, d_volume, extent, whole_or(extent, box), iso, d_max_map, map_extent, d_scratch, d_vertices, d_normals,
	                                      capacity_vertices, d_indices, capacity_triangles, d_counts, (hipStream_t) stream);
}

size_t vkv_label_mesh_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return label_mesh_scratch_bytes(extent, box); }

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_label_mesh(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors, uint64_t table_entries,
                   const uint8_t *d_volume, float iso, const uint8_t *d_visibility_map, VkvExtent3D map_extent, void *d_scratch,
                   float *d_triangles, uint32_t *d_triangle_labels, uint64_t capacity_triangles, uint64_t *d_counts, void *stream)
{
	const char *what = "label_mesh";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_inputs(ctx, what, d_labels, d_scratch, d_counts, extent, iso, d_volume ? " when d_volume is given" : nullptr, box))
		return rc;
	if (const int rc = check_label_table(ctx, what, d_colors, table_entries, d_visibility_map, extent, map_extent))
		return rc;
	if (const int rc = check_capacity(ctx, what, capacity_triangles, "triangles", d_triangles && d_triangle_labels, "d_triangles and d_triangle_labels"))
		return rc;
	if (const int rc = check_mesh_alignment(ctx, what, d_scratch, d_counts,
	                                        (uintptr_t) d_labels | (uintptr_t) d_colors | (uintptr_t) d_triangles | (uintptr_t) d_triangle_labels,
	                                        "d_labels, d_colors, d_triangles and d_triangle_labels"))
		return rc;
	if (const int rc = check_mesh_limits(ctx, what, extent, box, true, label_mesh_launch_ok))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_label_mesh(ctx, d_labels, extent, whole_or(extent, box), d_colors, table_entries, d_volume, iso, d_visibility_map, map_extent,
	                         d_scratch, d_triangles, d_triangle_labels, capacity_triangles, d_counts, (hipStream_t) stream);
}

size_t vkv_label_mesh_indexed_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return label_mesh_indexed_scratch_bytes(extent, box); }

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_label_mesh_indexed(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors, uint64_t table_entries,
                           const uint8_t *d_volume, float iso, const uint8_t *d_visibility_map, VkvExtent3D map_extent, void *d_scratch,
                           float *d_vertices, float *d_normals, uint32_t *d_vertex_labels, uint64_t capacity_vertices, uint32_t *d_indices,
                           uint32_t *d_triangle_labels, uint64_t capacity_triangles, uint64_t *d_counts, void *stream)
{
	const char *what = "label_mesh_indexed";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_inputs(ctx, what, d_labels, d_scratch, d_counts, extent, iso, d_volume ? " when d_volume is given" : nullptr, box))
		return rc;
	if (const int rc = check_label_table(ctx, what, d_colors, table_entries, d_visibility_map, extent, map_extent))
		return rc;
	if (const int rc = check_vertex_capacity(ctx, what, capacity_vertices, d_vertices))
		return rc;
	if (capacity_vertices == 0 && (d_normals || d_vertex_labels))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_normals and d_vertex_labels need a capacity of vertices", what);
	if (d_normals && !d_volume)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_normals needs the d_volume they are taken from", what);
	if (const int rc = check_capacity(ctx, what, capacity_triangles, "triangles", d_indices && d_triangle_labels, "d_indices and d_triangle_labels"))
		return rc;
	if (const int rc = check_mesh_alignment(ctx, what, d_scratch, d_counts,
	                                        (uintptr_t) d_labels | (uintptr_t) d_colors | (uintptr_t) d_vertices | (uintptr_t) d_normals |
	                                            (uintptr_t) d_vertex_labels | (uintptr_t) d_indices | (uintptr_t) d_triangle_labels,
	                                        "d_labels, d_colors, d_vertices, d_normals, d_vertex_labels, d_indices and d_triangle_labels"))
		return rc;
	if (const int rc = check_mesh_limits(ctx, what, extent, box, true, label_mesh_indexed_launch_ok))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_label_mesh_indexed(ctx, d_labels, extent, whole_or(extent, box), d_colors, table_entries, d_volume, iso, d_visibility_map, map_extent,
	                                 d_scratch, d_vertices, d_normals, d_vertex_labels, capacity_vertices, d_indices, d_triangle_labels, capacity_triangles,
	                                 d_counts, (hipStream_t) stream);
}

size_t vkv_mesh_adjacency_scratch_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles)
{
	return mesh_adjacency_bytes(capacity_vertices, capacity_triangles);
}

// what the three calls on an indexed mesh share: the 4-byte data pointers in `data`, the 8-byte d_counts and d_adjacency, the 32-bit capacities
static int check_mesh_post(vkv_ctx *ctx, const char *what, bool required, uintptr_t data, const char *data_names, const void *d_counts,
                           const void *d_adjacency, uint64_t capacity_vertices, uint64_t capacity_triangles)
{
	if (!required || !d_counts || !d_adjacency)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null pointer", what);
	if (data & 3u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: %s must be 4-byte aligned", what, data_names);
	if (((uintptr_t) d_counts | (uintptr_t) d_adjacency) & 7u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_counts and d_adjacency must be 8-byte aligned", what);
	if (capacity_vertices > 0xffffffffull || capacity_triangles > 0xffffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a capacity above 2^32 - 1 (indices are 32-bit)", what);
	return VKV_OK;
}

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_mesh_adjacency(vkv_ctx *ctx, const uint32_t *d_indices, uint64_t capacity_triangles, uint64_t capacity_vertices, const uint64_t *d_counts,
                       void *d_adjacency, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_post(ctx, "mesh_adjacency", d_indices != nullptr, (uintptr_t) d_indices, "d_indices", d_counts, d_adjacency,
	                                   capacity_vertices, capacity_triangles))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_mesh_adjacency(ctx, d_indices, capacity_triangles, capacity_vertices, d_counts, d_adjacency, (hipStream_t) stream);
}

int vkv_mesh_smooth(vkv_ctx *ctx, float *d_vertices, float *d_swap, uint64_t capacity_vertices, const uint64_t *d_counts, const void *d_adjacency,
                    const uint8_t *d_pinned, const float *factors, uint32_t n_passes, void *stream)
{
	const char *what = "mesh_smooth";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_post(ctx, what, d_vertices && d_swap, (uintptr_t) d_vertices | (uintptr_t) d_swap, "d_vertices and d_swap", d_counts,
	                                   d_adjacency, capacity_vertices, 0))
		return rc;
	if (d_vertices == d_swap)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_swap must be a buffer of its own", what);
	if (n_passes && !factors)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: %u passes without factors", what, n_passes);
	for (uint32_t i = 0; i < n_passes; ++i)
		if (!std::isfinite(factors[i]))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: factor %u is not finite", what, i);
	DeviceGuard guard(ctx->device);
	return launch_mesh_smooth(ctx, d_vertices, d_swap, capacity_vertices, d_counts, d_adjacency, d_pinned, factors, n_passes, (hipStream_t) stream);
}

int vkv_mesh_vertex_normals(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint32_t label,
                            uint64_t capacity_vertices, uint64_t capacity_triangles, const uint64_t *d_counts, const void *d_adjacency, float *d_normals,
                            void *stream)
{
	const char *what = "mesh_vertex_normals";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_mesh_post(ctx, what, d_vertices && d_indices && d_normals,
	                                   (uintptr_t) d_vertices | (uintptr_t) d_indices | (uintptr_t) d_triangle_labels | (uintptr_t) d_normals,
	                                   "d_vertices, d_indices, d_triangle_labels and d_normals", d_counts, d_adjacency, capacity_vertices, capacity_triangles))
		return rc;
	if (d_vertices == d_normals)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_normals must be a buffer of its own", what);
	DeviceGuard guard(ctx->device);
	return launch_mesh_vertex_normals(ctx, d_vertices, d_indices, d_triangle_labels, label, capacity_vertices, capacity_triangles, d_counts, d_adjacency,
	                                  d_normals, (hipStream_t) stream);
}

size_t vkv_mesh_decimate_scratch_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles, VkvExtent3D grid_extent)
{
	return mesh_decimate_bytes(capacity_vertices, capacity_triangles, grid_extent);
}

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_mesh_decimate(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint64_t capacity_vertices,
                      uint64_t capacity_triangles, const uint64_t *d_counts, const float *grid_origin, const float *grid_cell, VkvExtent3D grid_extent,
                      void *d_scratch, float *d_out_vertices, uint64_t out_capacity_vertices, uint32_t *d_out_indices, uint32_t *d_out_triangle_labels,
                      uint64_t out_capacity_triangles, uint32_t *d_vertex_map, uint64_t *d_out_counts, void *stream)
{
	const char *what = "mesh_decimate";
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_vertices || !d_indices || !d_counts || !grid_origin || !grid_cell || !d_scratch || !d_out_counts)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null pointer", what);
	if (((uintptr_t) d_vertices | (uintptr_t) d_indices | (uintptr_t) d_triangle_labels | (uintptr_t) d_out_vertices | (uintptr_t) d_out_indices |
	     (uintptr_t) d_out_triangle_labels | (uintptr_t) d_vertex_map) &
	    3u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT,
		                 "%s: d_vertices, d_indices, d_triangle_labels, d_out_vertices, d_out_indices, d_out_triangle_labels and d_vertex_map must be 4-byte aligned",
		                 what);
	if (((uintptr_t) d_counts | (uintptr_t) d_scratch | (uintptr_t) d_out_counts) & 7u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_counts, d_scratch and d_out_counts must be 8-byte aligned", what);
	if (grid_extent.width == 0 || grid_extent.height == 0 || grid_extent.depth == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: a grid of %u x %u x %u cells", what, grid_extent.width, grid_extent.height, grid_extent.depth);
	for (int a = 0; a < 3; ++a)
	{
		if (!std::isfinite(grid_cell[a]) || !(grid_cell[a] > 0.0f))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: grid_cell[%d] must be finite and positive", what, a);
		if (!std::isfinite(grid_origin[a]))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: grid_origin[%d] is not finite", what, a);
	}
	// every output that is given against every input, the scratch block and every other output
	const void *const inputs[]  = {d_vertices, d_indices, d_triangle_labels, d_counts, d_scratch};
	const void *const outputs[] = {d_out_vertices, d_out_indices, d_out_triangle_labels, d_vertex_map, d_out_counts};
	for (size_t o = 0; o < 5; ++o)
	{
		if (!outputs[o])
			continue;
		for (size_t i = 0; i < 5; ++i)
			if (outputs[o] == inputs[i])
				return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: every output must be a buffer of its own, not an input or the scratch block", what);
		for (size_t p = o + 1; p < 5; ++p)
			if (outputs[o] == outputs[p])
				return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: every output must be a buffer of its own, not another output", what);
	}
	if ((out_capacity_vertices != 0 && !d_out_vertices) || (out_capacity_triangles != 0 && (!d_out_indices || (d_triangle_labels && !d_out_triangle_labels))))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: an output capacity without its buffer", what);
	if (capacity_vertices > 0xffffffffull || capacity_triangles > 0xffffffffull || out_capacity_vertices > 0xffffffffull || out_capacity_triangles > 0xffffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a capacity above 2^32 - 1 (indices are 32-bit)", what);
	if (mesh_decimate_cells(grid_extent) == 0)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a grid of more than 2^32 - 1 cells", what);
	DeviceGuard guard(ctx->device);
	return launch_mesh_decimate(ctx, d_vertices, d_indices, d_triangle_labels, capacity_vertices, capacity_triangles, d_counts, grid_origin, grid_cell,
	                            grid_extent, d_scratch, d_out_vertices, out_capacity_vertices, d_out_indices, d_out_triangle_labels, out_capacity_triangles,
	                            d_vertex_map, d_out_counts, (hipStream_t) stream);
}

size_t vkv_label_components_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return components_scratch_bytes(extent, box); }

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_label_components(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t connectivity,
                         const uint8_t *d_max_map, VkvExtent3D map_extent, void *d_scratch, uint32_t *d_labels, uint32_t *d_sizes,
                         uint64_t capacity_components, uint64_t *d_counts, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_volume || !d_scratch || !d_labels || !d_counts || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: null pointer or zero extent");
	if (!std::isfinite(iso))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: iso must be finite");
	if (connectivity != VKV_CONNECT_6 && connectivity != VKV_CONNECT_14 && connectivity != VKV_CONNECT_26)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: unknown connectivity %d (6, 14 or 26)", (int) connectivity);
	if (const int rc = check_box(ctx, "label_components", extent, box))
		return rc;
	if (d_max_map && !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: the max map needs a valid map_extent");
	if (capacity_components > 0xffffffffull)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: a capacity of %llu components is past 32-bit labels", (unsigned long long) capacity_components);
	if (capacity_components != 0 && !d_sizes)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: a capacity of %llu components needs d_sizes", (unsigned long long) capacity_components);
	if ((((uintptr_t) d_scratch | (uintptr_t) d_counts) & 7u) != 0 || (((uintptr_t) d_labels | (uintptr_t) d_sizes) & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "label_components: d_scratch and d_counts must be 8-byte aligned, d_labels and d_sizes 4-byte aligned");
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "label_components: a box of more than 2^32 - 1 voxels; label it box by box");
	DeviceGuard guard(ctx->device);
	return launch_label_components(ctx, d_volume, extent, whole_or(extent, box), iso, connectivity, d_max_map, map_extent, d_scratch, d_labels, d_sizes,
	                               capacity_components, d_counts, (hipStream_t) stream);
}

// every argument is checked before the launch (and before the device is touched)
int vkv_select_components(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_labels,
                          const uint32_t *d_sizes, const uint64_t *d_counts, uint64_t min_voxels, uint64_t max_voxels, uint32_t fill, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_src || !d_dst || !d_labels || !d_counts || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components: null pointer or zero extent");
	if (const int rc = check_box(ctx, "select_components", extent, box))
		return rc;
	if (fill > 255u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components: fill %u is no byte", fill);
	if (min_voxels > max_voxels)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components: min_voxels %llu above max_voxels %llu", (unsigned long long) min_voxels,
		                 (unsigned long long) max_voxels);
	if ((((uintptr_t) d_labels | (uintptr_t) d_sizes) & 3u) != 0 || ((uintptr_t) d_counts & 7u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components: d_labels and d_sizes must be 4-byte aligned, d_counts 8-byte aligned");
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "select_components: a box of more than 2^32 - 1 voxels");
	if (const int rc = check_in_place_or_disjoint(ctx, "select_components", d_src, d_dst, extent, true))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_select_components(ctx, d_src, d_dst, extent, whole_or(extent, box), d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill,
	                                (hipStream_t) stream);
}

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_component_stats(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_labels, const uint64_t *d_counts,
                        VkvComponentStats *d_stats, uint64_t capacity_components, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_labels || !d_counts || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "component_stats: null pointer or zero extent");
	if (const int rc = check_box(ctx, "component_stats", extent, box))
		return rc;
	if (capacity_components > 0xffffffffull)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "component_stats: a capacity of %llu components is past 32-bit labels", (unsigned long long) capacity_components);
	if (capacity_components != 0 && !d_stats)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "component_stats: a capacity of %llu components needs d_stats", (unsigned long long) capacity_components);
	if (((uintptr_t) d_labels & 3u) != 0 || (((uintptr_t) d_counts | (uintptr_t) d_stats) & 7u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "component_stats: d_labels must be 4-byte aligned, d_counts and d_stats 8-byte aligned");
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "component_stats: a box of more than 2^32 - 1 voxels; measure it box by box");
	DeviceGuard guard(ctx->device);
	return launch_component_stats(ctx, d_volume, extent, whole_or(extent, box), d_labels, d_counts, d_stats, capacity_components, (hipStream_t) stream);
}

// every argument is checked before the launch (and before the device is touched)
int vkv_select_components_by_table(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_labels,
                                   const uint8_t *d_keep, uint64_t table_entries, uint32_t fill, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_src || !d_dst || !d_labels || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components_by_table: null pointer or zero extent");
	if (!d_keep && table_entries != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components_by_table: a table of %llu entries needs d_keep", (unsigned long long) table_entries);
	if (const int rc = check_box(ctx, "select_components_by_table", extent, box))
		return rc;
	if (fill > 255u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components_by_table: fill %u is no byte", fill);
	if (((uintptr_t) d_labels & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_components_by_table: d_labels must be 4-byte aligned");
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "select_components_by_table: a box of more than 2^32 - 1 voxels");
	if (const int rc = check_in_place_or_disjoint(ctx, "select_components_by_table", d_src, d_dst, extent, true))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_select_components_by_table(ctx, d_src, d_dst, extent, whole_or(extent, box), d_labels, d_keep, table_entries, fill, (hipStream_t) stream);
}

size_t vkv_distance_transform_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return edt_scratch_bytes(extent, box); }

// what vkv_distance_transform, vkv_distance_transform_weighted and vkv_nearest_target check alike (ctx is not null); 0: accepted so far.
// dist2_optional: vkv_nearest_target's d_dist2 may be null
static int check_distance_transform(vkv_ctx *ctx, const char *name, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target,
                                    uint32_t limit, void *d_scratch, uint32_t *d_dist2, bool dist2_optional = false)
{
	if (!d_volume || !d_scratch || (!d_dist2 && !dist2_optional) || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: null pointer or zero extent", name);
	if (!std::isfinite(iso))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: iso must be finite", name);
	if (target != VKV_DISTANCE_TO_INSIDE && target != VKV_DISTANCE_TO_OUTSIDE)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: unknown target %d", name, (int) target);
	if (limit == 0u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: limit 0 (VKV_DISTANCE_NONE: unlimited)", name);
	if (const int rc = check_box(ctx, name, extent, box))
		return rc;
	if (((uintptr_t) d_scratch & 7u) != 0 || ((uintptr_t) d_dist2 & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_scratch must be 8-byte aligned, d_dist2 4-byte aligned", name);
	if (!edt_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: a box of more than 2^32 - 1 voxels or an axis above 32768; transform it box by box", name);
	return VKV_OK;
}

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written
int vkv_distance_transform(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target, uint32_t limit,
                           void *d_scratch, uint32_t *d_dist2, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (const int rc = check_distance_transform(ctx, "distance_transform", d_volume, extent, box, iso, target, limit, d_scratch, d_dist2))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_distance_transform(ctx, d_volume, extent, whole_or(extent, box), iso, target, limit, d_scratch, d_dist2, (hipStream_t) stream);
}

// the same checks, then the weights (read here, on the host): none null or 0, and the largest value they can give fits below VKV_DISTANCE_NONE
int vkv_distance_transform_weighted(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target,
                                    const uint32_t weights[3], uint32_t limit, void *d_scratch, uint32_t *d_dist2, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!weights || weights[0] == 0u || weights[1] == 0u || weights[2] == 0u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "distance_transform_weighted: null weights or a weight of 0");
	if (const int rc = check_distance_transform(ctx, "distance_transform_weighted", d_volume, extent, box, iso, target, limit, d_scratch, d_dist2))
		return rc;
	const VkvBox b = whole_or(extent, box);
	if (!edt_weights_fit(weights, b.width, b.height, b.depth))
		return set_error(ctx, VKV_E_UNSUPPORTED, "distance_transform_weighted: weights (%u, %u, %u) can give a value above 0xfffffffe in this box", weights[0],
		                 weights[1], weights[2]);
	DeviceGuard guard(ctx->device);
	return launch_distance_transform_weighted(ctx, d_volume, extent, b, iso, target, weights, limit, d_scratch, d_dist2, (hipStream_t) stream);
}

// vkv_distance_transform_weighted's checks (the shared function, the weights), then the feature buffer: not null, 4-byte aligned, and apart
// from d_dist2 where that is given.  Both hold 4 bytes per voxel of the box
int vkv_nearest_target(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target, const uint32_t weights[3],
                       uint32_t limit, void *d_scratch, uint32_t *d_nearest, uint32_t *d_dist2, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!weights || weights[0] == 0u || weights[1] == 0u || weights[2] == 0u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "nearest_target: null weights or a weight of 0");
	if (!d_nearest || ((uintptr_t) d_nearest & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "nearest_target: d_nearest must be given and 4-byte aligned");
	if (const int rc = check_distance_transform(ctx, "nearest_target", d_volume, extent, box, iso, target, limit, d_scratch, d_dist2, true))
		return rc;
	const VkvBox b = whole_or(extent, box);
	if (!edt_weights_fit(weights, b.width, b.height, b.depth))
		return set_error(ctx, VKV_E_UNSUPPORTED, "nearest_target: weights (%u, %u, %u) can give a value above 0xfffffffe in this box", weights[0], weights[1],
		                 weights[2]);
	if (d_dist2)
	{        // edt_launch_ok: at most 2^32 - 1 voxels
		const uint64_t  bytes = 4ull * b.width * b.height * b.depth;
		const uintptr_t p = (uintptr_t) d_nearest, q = (uintptr_t) d_dist2;
		if ((p < q ? q - p : p - q) < bytes)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "nearest_target: d_nearest and d_dist2 overlap");
	}
	DeviceGuard guard(ctx->device);
	return launch_nearest_target(ctx, d_volume, extent, b, iso, target, weights, limit, d_scratch, d_nearest, d_dist2, (hipStream_t) stream);
}

// every argument is checked before the launch (and before the device is touched).  The call is a gather: d_out apart from both inputs
int vkv_propagate_labels(vkv_ctx *ctx, const uint32_t *d_nearest, const uint32_t *d_labels, uint32_t *d_out, VkvExtent3D extent, const VkvBox *box,
                         const uint8_t *d_mask_volume, float mask_iso, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_nearest || !d_labels || !d_out || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "propagate_labels: null pointer or zero extent");
	if (d_mask_volume && !std::isfinite(mask_iso))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "propagate_labels: mask_iso must be finite");
	if (const int rc = check_box(ctx, "propagate_labels", extent, box))
		return rc;
	if ((((uintptr_t) d_nearest | (uintptr_t) d_labels | (uintptr_t) d_out) & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "propagate_labels: d_nearest, d_labels and d_out must be 4-byte aligned");
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "propagate_labels: a box of more than 2^32 - 1 voxels");
	const VkvBox    b     = whole_or(extent, box);
	const uint64_t  bytes = 4ull * b.width * b.height * b.depth;
	const uintptr_t o     = (uintptr_t) d_out;
	for (const uintptr_t in : {(uintptr_t) d_nearest, (uintptr_t) d_labels})
		if ((o < in ? in - o : o - in) < bytes)
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "propagate_labels: d_out overlaps d_nearest or d_labels (a gather does not run in place)");
	DeviceGuard guard(ctx->device);
	return launch_propagate_labels(ctx, d_nearest, d_labels, d_out, extent, b, d_mask_volume, mask_iso, (hipStream_t) stream);
}

size_t vkv_geodesic_scratch_bytes(VkvExtent3D extent, const VkvBox *box) { return geodesic_scratch_bytes(extent, box); }

// every argument is checked before the first launch (and before the device is touched); nothing in the context is written.  `steps` is read
// here, on the host
int vkv_geodesic_propagate(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, const uint32_t *d_seeds,
                           const uint32_t steps[7], uint32_t limit, uint32_t rounds, int32_t resume, void *d_scratch, uint32_t *d_dist, uint32_t *d_labels,
                           uint64_t *d_counts, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (resume != 0 && resume != 1)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: resume %d is neither 0 nor 1", (int) resume);
	if (resume)
		d_seeds = nullptr;        // not read
	if (!d_volume || !d_scratch || !d_counts || !steps || (!d_seeds && !resume) || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: null pointer or zero extent");
	if (!d_dist && !d_labels)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: neither d_dist nor d_labels is given");
	if (!std::isfinite(iso))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: iso must be finite");
	if (limit == 0u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: limit 0 (VKV_GEODESIC_NONE: unlimited)");
	if (rounds == 0u || rounds > VKV_GEODESIC_MAX_ROUNDS)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: %u rounds (1 .. %d)", rounds, VKV_GEODESIC_MAX_ROUNDS);
	uint32_t largest = 0;
	for (int m = 0; m < 7; ++m)
		largest = steps[m] > largest ? steps[m] : largest;
	if (largest == 0u || largest > 65535u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: every step is 0, or a step is above 65535");
	if (const int rc = check_box(ctx, "geodesic_propagate", extent, box))
		return rc;
	if ((((uintptr_t) d_scratch | (uintptr_t) d_counts) & 7u) != 0 || (((uintptr_t) d_seeds | (uintptr_t) d_dist | (uintptr_t) d_labels) & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: d_scratch and d_counts must be 8-byte aligned, d_seeds, d_dist and d_labels 4-byte aligned");
	if (!components_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "geodesic_propagate: a box of more than 2^32 - 1 voxels");
	const VkvBox b = whole_or(extent, box);
	{        // the three arrays hold 4 bytes per voxel of the box; only d_labels == d_seeds may meet
		const uint64_t array = 4ull * b.width * b.height * b.depth, block = geodesic_scratch_bytes(extent, box);
		struct Range
		{
			uintptr_t p;
			uint64_t  bytes;
		} ranges[4] = {{(uintptr_t) d_seeds, array}, {(uintptr_t) d_dist, array}, {(uintptr_t) d_labels, array}, {(uintptr_t) d_scratch, block}};
		for (int i = 0; i < 4; ++i)
			for (int j = i + 1; j < 4; ++j)
			{
				const Range &lo = ranges[i].p <= ranges[j].p ? ranges[i] : ranges[j], &hi = ranges[i].p <= ranges[j].p ? ranges[j] : ranges[i];
				if (!lo.p || !hi.p || hi.p - lo.p >= lo.bytes || (i == 0 && j == 2 && lo.p == hi.p))
					continue;
				return set_error(ctx, VKV_E_INVALID_ARGUMENT, "geodesic_propagate: d_seeds, d_dist, d_labels and d_scratch overlap (only d_labels == d_seeds may)");
			}
	}
	DeviceGuard guard(ctx->device);
	return launch_geodesic_propagate(ctx, d_volume, extent, b, iso, d_seeds, steps, limit, rounds, resume != 0, d_scratch, d_dist, d_labels, d_counts,
	                                 (hipStream_t) stream);
}

// every argument is checked before the launch (and before the device is touched)
int vkv_select_by_distance(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_dist2, uint32_t lo,
                           uint32_t hi, uint32_t fill, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	if (!d_src || !d_dst || !d_dist2 || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_by_distance: null pointer or zero extent");
	if (const int rc = check_box(ctx, "select_by_distance", extent, box))
		return rc;
	if (fill > 255u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_by_distance: fill %u is no byte", fill);
	if (lo > hi)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_by_distance: lo %u above hi %u", lo, hi);
	if (((uintptr_t) d_dist2 & 3u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "select_by_distance: d_dist2 must be 4-byte aligned");
	if (!edt_launch_ok(extent, box))
		return set_error(ctx, VKV_E_UNSUPPORTED, "select_by_distance: a box of more than 2^32 - 1 voxels or an axis above 32768");
	if (const int rc = check_in_place_or_disjoint(ctx, "select_by_distance", d_src, d_dst, extent, true))
		return rc;
	DeviceGuard guard(ctx->device);
	return launch_select_by_distance(ctx, d_src, d_dst, extent, whole_or(extent, box), d_dist2, lo, hi, fill, (hipStream_t) stream);
}

// every argument is checked before the first launch
int vkv_cell_summary(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent, VkvExtent3D map_extent, const VkvBox *box,
                     void *d_summary, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !d_summary || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "cell_summary: null pointer or bad extent");
	if (((uintptr_t) d_summary & 15u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "cell_summary: d_summary must be 16-byte aligned");
	if (const int rc = check_box(ctx, "cell_summary", extent, box))
		return rc;
	if (!cells_launch_ok(extent, map_extent))
		return set_error(ctx, VKV_E_UNSUPPORTED, "cell_summary: map too large for one launch");
	return launch_cell_summary(ctx, d_volume, d_gradient, extent, map_extent, box, d_summary, (hipStream_t) stream);
}

// the checks the two summary-based map calls share (after their own null checks): check_maps with the classify launch's limits
static int check_from_summary(vkv_ctx *ctx, const char *what, const void *d_summary, const uint8_t *d_gradient, int32_t use_gradient, VkvExtent3D extent,
                              uint8_t *const d_maps[8], const uint8_t *d_swap, VkvExtent3D map_extent, int32_t skipping_type, const uint64_t *d_unresolved)
{
	if ((((uintptr_t) d_summary) & 15u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_summary must be 16-byte aligned", what);
	if ((((uintptr_t) d_unresolved) & 7u) != 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "%s: d_unresolved must be 8-byte aligned", what);
	if (const int rc = check_maps(ctx, what, d_maps, d_swap, extent, map_extent, skipping_type, true))
		return rc;
	if (use_gradient && !d_gradient)
		return set_error(ctx, VKV_E_UNSUPPORTED, "%s: the summary holds no on-the-fly gradient (use_gradient needs d_gradient)", what);
	return VKV_OK;
}

int vkv_occupancy_map_from_summary(vkv_ctx *ctx, const void *d_summary, const uint8_t *d_volume, const uint8_t *d_gradient, const uint8_t *d_tf,
                                   const VkvTransferFunctionUniform *tf, VkvExtent3D extent, uint8_t *d_map, VkvExtent3D map_extent, uint64_t *d_unresolved,
                                   void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_summary || !d_volume || !d_tf || !tf || !d_map || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "occupancy_map_from_summary: null pointer or bad extent");
	int rc = check_from_summary(ctx, "occupancy_map_from_summary", d_summary, d_gradient, tf->use_gradient, extent, &d_map, nullptr, map_extent,
	                            VKV_SKIP_NONE, d_unresolved);
	if (rc != VKV_OK)
		return rc;
	const hipStream_t   s       = (hipStream_t) stream;
	const StreamScratch scratch = stream_scratch(ctx, s);
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	if ((rc = launch_tf_bits(ctx, d_tf, reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset), s)) != VKV_OK)
		return rc;
	return launch_occupancy_from_summary(ctx, d_summary, d_volume, d_gradient, tf->use_gradient != 0, scratch.p, extent, d_map, map_extent, d_unresolved, s);
}

// vkv_update_transfer_function with the occupancy map from the summary and the count from the histogram: every argument is checked first
int vkv_update_transfer_function_from_summary(vkv_ctx *ctx, const VkvVolumeOptions *options, const uint8_t *d_volume, const uint8_t *d_gradient,
                                              VkvExtent3D extent, uint8_t *d_tf, uint32_t *d_tables, uint8_t *const d_maps[8], uint8_t *d_swap,
                                              VkvExtent3D map_extent, int32_t skipping_type, uint64_t *d_occupied_count, const void *d_summary,
                                              const uint64_t *d_histogram, uint64_t *d_unresolved, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!options || !d_volume || !d_tf || !d_tables || !d_maps || !d_summary || !extent_ok(extent) || !map_extent_ok(extent, map_extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_transfer_function_from_summary: null pointer or bad extent");
	if (!tf_pointers_aligned(d_tf, d_tables))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_transfer_function_from_summary: d_transfer_function and d_tables must be 4-byte aligned");
	if (d_occupied_count && !d_histogram)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_transfer_function_from_summary: d_occupied_count needs d_histogram");
	if ((((uintptr_t) d_occupied_count) | ((uintptr_t) d_histogram)) & 7u)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "update_transfer_function_from_summary: d_occupied_count and d_histogram must be 8-byte aligned");
	VkvTransferFunctionUniform tf;
	vkv_transfer_function_uniform(options, &tf);
	int rc = check_from_summary(ctx, "update_transfer_function_from_summary", d_summary, d_gradient, tf.use_gradient, extent, d_maps, d_swap, map_extent,
	                            skipping_type, d_unresolved);
	if (rc != VKV_OK)
		return rc;
	const hipStream_t   s       = (hipStream_t) stream;
	const StreamScratch scratch = stream_scratch(ctx, s);        // held until the classification is enqueued
	if (!scratch.p)
		return VKV_E_UNSUPPORTED;
	uint32_t *d_bits = reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset);
	if (d_occupied_count && (rc = launch_histogram_occupied_count(ctx, d_histogram, &tf, d_occupied_count, s)) != VKV_OK)
		return rc;
	if ((rc = launch_tf_build(ctx, &tf, d_tf, d_tables, d_bits, s)) != VKV_OK)
		return rc;
	uint8_t *occ = d_maps[skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE ? 7 : 0];
	if ((rc = launch_occupancy_from_summary(ctx, d_summary, d_volume, d_gradient, tf.use_gradient != 0, scratch.p, extent, occ, map_extent, d_unresolved,
	                                        s)) != VKV_OK)
		return rc;
	return launch_map_transform(ctx, d_maps, d_swap, map_extent, skipping_type, s);
}

// argument checks shared by vkv_render and vkv_render_batch
static int check_render_params(vkv_ctx *ctx, const VkvRenderParams *P)
{
	if (!P)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: null params");
	const VkvRenderOptions &o = P->options;
	if (o.depth_attachment && !P->d_in_depth)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: options.depth_attachment needs d_in_depth");
	if (o.test < VKV_TEST_NONE || o.test > VKV_TEST_NUM_TEXTURE_SAMPLES)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: bad test mode %d", o.test);
	if (o.skipping_type < VKV_SKIP_NONE || o.skipping_type > VKV_SKIP_ANISOTROPIC_DISTANCE)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: bad skipping_type %d", o.skipping_type);
	if (!extent_ok(P->volume_extent) || P->image_width == 0 || P->image_height == 0)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: zero extent");
	if (!P->d_volume || !P->d_transfer_function)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: null volume or transfer function");
	if (P->transfer_function.use_gradient && P->use_precomputed_gradient && !P->d_gradient)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: precomputed gradient requested but d_gradient is null");
	if (!(P->transfer_function.sampling_factor > 0.0f))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: sampling_factor must be positive");
	if (o.skipping_type != VKV_SKIP_NONE)
	{
		if (!map_extent_ok(P->volume_extent, P->map_extent))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: bad map extent");
		if ((uint64_t) P->map_extent.width * P->map_extent.height * P->map_extent.depth > 0xffffffffull)
			return set_error(ctx, VKV_E_UNSUPPORTED, "render: distance maps with more than 2^32 cells are not supported");
		if (P->map_extent.width >= (1u << 24) || P->map_extent.height >= (1u << 24) || P->map_extent.depth >= (1u << 24))
			return set_error(ctx, VKV_E_UNSUPPORTED, "render: distance map axes of 2^24 cells or more are not supported");
		const int n = o.skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE ? 8 : 1;
		for (int i = 0; i < n; ++i)
			if (!P->d_distance_maps[i])
				return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render: distance map %d is null", i);
	}
	if (const int rc = check_tile_schedule(ctx, "render", P))
		return rc;
	return check_render_buffers(ctx, "render", P, false);
}

int vkv_render(vkv_ctx *ctx, const VkvRenderParams *P, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	const int   rc = check_render_params(ctx, P);
	if (rc != VKV_OK)
		return rc;
	float lut[256];
	cached_alpha_lut(ctx, P->transfer_function, lut);
	return launch_render(ctx, P, lut, (hipStream_t) stream);
}

int vkv_render_batch(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t count, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!P || count == 0 || count > VKV_MAX_BATCH)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: count must be 1 .. %d", VKV_MAX_BATCH);
	std::vector<float> luts((size_t) count * 256);
	for (uint32_t i = 0; i < count; ++i)
	{
		const int rc = check_render_params(ctx, &P[i]);
		if (rc != VKV_OK)
			return rc;
		const VkvRenderParams &a = P[i], &b = P[0];
		if (a.options.skipping_type != b.options.skipping_type || (a.options.early_ray_termination != 0) != (b.options.early_ray_termination != 0) ||
		    (a.transfer_function.use_gradient != 0) != (b.transfer_function.use_gradient != 0) ||
		    (a.use_precomputed_gradient != 0) != (b.use_precomputed_gradient != 0))
			return set_error(ctx, VKV_E_INVALID_ARGUMENT, "render_batch: frame %u needs a different kernel variant than frame 0", i);
		// frames of the batch with the same two floats share one table (and one look at the cache)
		uint32_t same = i;
		for (uint32_t j = 0; j < i && same == i; ++j)
			if (std::memcmp(&P[j].transfer_function.voxel_alpha_factor, &a.transfer_function.voxel_alpha_factor, 4) == 0 &&
			    std::memcmp(&P[j].transfer_function.sampling_factor, &a.transfer_function.sampling_factor, 4) == 0)
				same = j;
		if (same != i)
			std::memcpy(luts.data() + (size_t) i * 256, luts.data() + (size_t) same * 256, 256 * sizeof(float));
		else
			cached_alpha_lut(ctx, a.transfer_function, luts.data() + (size_t) i * 256);
	}
	return launch_render_batch(ctx, P, count, luts.data(), (hipStream_t) stream);
}

int vkv_prepare_render(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t count, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!P || count == 0 || count > VKV_MAX_BATCH)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "prepare_render: count must be 1 .. %d", VKV_MAX_BATCH);
	for (uint32_t i = 0; i < count; ++i)
	{
		const int rc = check_render_params(ctx, &P[i]);
		if (rc != VKV_OK)
			return rc;
	}
	return prepare_render(ctx, P, count, (hipStream_t) stream);
}

int vkv_synth_volume(vkv_ctx *ctx, uint8_t *d_volume, VkvExtent3D extent, uint32_t kind, uint32_t seed, void *stream)
{
	if (!ctx)
		return VKV_E_INVALID_ARGUMENT;
	DeviceGuard guard(ctx->device);
	if (!d_volume || !extent_ok(extent))
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "synth_volume: null pointer or zero extent");
	return launch_synth_volume(ctx, d_volume, extent, kind, seed, (hipStream_t) stream);
}

}        // extern "C"

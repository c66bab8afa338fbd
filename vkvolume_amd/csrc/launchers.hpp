// launchers.hpp — every function of the library that crosses a translation unit on the host side: the kernel launchers, the limits the entry
// points check before they enqueue anything, the helpers of raymarch.hip that capi.hip and context.hip call, and the argument checks of capi.hip
// that other files share.  The entry points' files (capi.hip, context.hip, exchange.hip) and every file that defines one of them include it, so a
// changed signature is a compile error, not a link error.  All of them return VKV_OK or an error code with the context's error text set; `s` is
// the stream the work is enqueued on; device pointers are named d_*.  The context: context.hpp; host arithmetic without HIP: ../host/host_arith.hpp;
// what the box-of-voxels operations (mesh.hip .. edt.hip) share on both sides: box_domain.hpp (it includes this file) and fixed_scan.hpp.
#pragma once

#include "context.hpp"

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
// vkv_isosurface_mesh_scratch_bytes: 0 for an extent or box that is not accepted (extent_and_box_ok, box_domain.hpp, as for the three files
// below); what the launches can take (box null: the whole volume)
size_t mesh_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   mesh_launch_ok(VkvExtent3D e, const VkvBox *box);
// vkv_isosurface_mesh after the entry point's argument checks (b inside e; me is read with a max map only)
int launch_isosurface_mesh(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint8_t *d_max_map, VkvExtent3D me,
                           void *d_scratch, float *d_triangles, uint64_t capacity, uint64_t *d_counts, hipStream_t s);

// ---- mesh_indexed.hip
// vkv_isosurface_mesh_indexed_scratch_bytes, what its launches can take, and the call after the entry point's argument checks
size_t mesh_indexed_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   mesh_indexed_launch_ok(VkvExtent3D e, const VkvBox *box);
int launch_isosurface_mesh_indexed(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint8_t *d_max_map, VkvExtent3D me,
                                   void *d_scratch, float *d_vertices, float *d_normals, uint64_t capacity_vertices, uint32_t *d_indices,
                                   uint64_t capacity_triangles, uint64_t *d_counts, hipStream_t s);

// ---- label_mesh.hip
// vkv_label_mesh_scratch_bytes (0 for an extent or box that is not accepted, a box of more than 2^32 - 1 voxels included), what the launches
// can take, and vkv_label_mesh after the entry point's argument checks (b inside e; d_colors null: every non-zero label is visible; d_vol
// null: midpoints; me is read with a visibility map only)
size_t label_mesh_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   label_mesh_launch_ok(VkvExtent3D e, const VkvBox *box);
int launch_label_mesh(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D e, const VkvBox &b, const uint32_t *d_colors, uint64_t table_entries,
                      const uint8_t *d_vol, float iso, const uint8_t *d_visibility_map, VkvExtent3D me, void *d_scratch, float *d_triangles,
                      uint32_t *d_triangle_labels, uint64_t capacity, uint64_t *d_counts, hipStream_t s);

// ---- label_mesh_indexed.hip
// vkv_label_mesh_indexed_scratch_bytes (0 as for label_mesh_scratch_bytes), what the launches can take, and vkv_label_mesh_indexed after the
// entry point's argument checks (as launch_label_mesh; d_normals and d_vertex_labels may be null; a capacity of 0 enqueues no emit of its list)
size_t label_mesh_indexed_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   label_mesh_indexed_launch_ok(VkvExtent3D e, const VkvBox *box);
int launch_label_mesh_indexed(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D e, const VkvBox &b, const uint32_t *d_colors, uint64_t table_entries,
                              const uint8_t *d_vol, float iso, const uint8_t *d_visibility_map, VkvExtent3D me, void *d_scratch, float *d_vertices,
                              float *d_normals, uint32_t *d_vertex_labels, uint64_t capacity_vertices, uint32_t *d_indices, uint32_t *d_triangle_labels,
                              uint64_t capacity_triangles, uint64_t *d_counts, hipStream_t s);

// ---- mesh_smooth.hip
// vkv_mesh_adjacency_scratch_bytes (0 for a capacity above 2^32 - 1), and vkv_mesh_adjacency, vkv_mesh_smooth (factors: n_passes host floats,
// read now; d_pinned may be null) and vkv_mesh_vertex_normals (d_triangle_labels null: every used face) after the entry points' argument checks
size_t mesh_adjacency_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles);
int launch_mesh_adjacency(vkv_ctx *ctx, const uint32_t *d_indices, uint64_t capacity_triangles, uint64_t capacity_vertices, const uint64_t *d_counts,
                          void *d_adjacency, hipStream_t s);
int launch_mesh_smooth(vkv_ctx *ctx, float *d_vertices, float *d_swap, uint64_t capacity_vertices, const uint64_t *d_counts, const void *d_adjacency,
                       const uint8_t *d_pinned, const float *factors, uint32_t n_passes, hipStream_t s);
int launch_mesh_vertex_normals(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint32_t label,
                               uint64_t capacity_vertices, uint64_t capacity_triangles, const uint64_t *d_counts, const void *d_adjacency, float *d_normals,
                               hipStream_t s);

// ---- mesh_decimate.hip
// the cells of a clustering grid (0 for a zero axis or more than 2^32 - 1 cells), vkv_mesh_decimate_scratch_bytes (0 for such a grid or a
// capacity above 2^32 - 1), and vkv_mesh_decimate after the entry point's argument checks (grid_origin, grid_cell: 3 host floats each, read
// now; d_triangle_labels, d_vertex_map may be null; an output capacity of 0 enqueues no emit of its list)
uint64_t mesh_decimate_cells(VkvExtent3D grid);
size_t   mesh_decimate_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles, VkvExtent3D grid);
int launch_mesh_decimate(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint64_t capacity_vertices,
                         uint64_t capacity_triangles, const uint64_t *d_counts, const float *grid_origin, const float *grid_cell, VkvExtent3D grid,
                         void *d_scratch, float *d_out_vertices, uint64_t out_capacity_vertices, uint32_t *d_out_indices, uint32_t *d_out_triangle_labels,
                         uint64_t out_capacity_triangles, uint32_t *d_vertex_map, uint64_t *d_out_counts, hipStream_t s);

// ---- components.hip
// vkv_label_components_scratch_bytes (0 for an extent or box that is not accepted), what the launches can take (box_linear_plan: at most
// 2^32 - 1 voxels in the box), and vkv_label_components / vkv_select_components after the entry points' argument checks (b inside e)
size_t components_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   components_launch_ok(VkvExtent3D e, const VkvBox *box);
int launch_label_components(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int connectivity, const uint8_t *d_max_map,
                            VkvExtent3D me, void *d_scratch, uint32_t *d_labels, uint32_t *d_sizes, uint64_t capacity, uint64_t *d_counts, hipStream_t s);
int launch_select_components(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, const uint32_t *d_labels,
                             const uint32_t *d_sizes, const uint64_t *d_counts, uint64_t min_voxels, uint64_t max_voxels, uint32_t fill, hipStream_t s);

// ---- component_stats.hip
// vkv_component_stats (nothing is enqueued for a capacity of 0) and vkv_select_components_by_table after the entry points' argument checks
// (b inside e, components_launch_ok)
int launch_component_stats(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, const uint32_t *d_labels, const uint64_t *d_counts,
                           VkvComponentStats *d_stats, uint64_t capacity, hipStream_t s);
int launch_select_components_by_table(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, const uint32_t *d_labels,
                                      const uint8_t *d_keep, uint64_t table_entries, uint32_t fill, hipStream_t s);

// ---- edt.hip
// vkv_distance_transform_scratch_bytes (0 for an extent or box that is not accepted), what the launches can take (box_linear_plan and no box
// axis above 32768), and vkv_distance_transform / vkv_select_by_distance after the entry points' argument checks (b inside e)
size_t edt_scratch_bytes(VkvExtent3D e, const VkvBox *box);
bool   edt_launch_ok(VkvExtent3D e, const VkvBox *box);
int launch_distance_transform(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, uint32_t limit, void *d_scratch,
                              uint32_t *d_dist2, hipStream_t s);
int launch_select_by_distance(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, const uint32_t *d_dist2, uint32_t lo,
                              uint32_t hi, uint32_t fill, hipStream_t s);

// ---- edt_envelope.hip
// vkv_distance_transform_weighted after the entry point's argument checks (b inside e, edt_launch_ok, edt_weights_fit of host_arith.hpp); the
// scratch block is edt_scratch_bytes()
int launch_distance_transform_weighted(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, const uint32_t weights[3],
                                       uint32_t limit, void *d_scratch, uint32_t *d_dist2, hipStream_t s);

// ---- nearest.hip
// vkv_nearest_target after the entry point's argument checks (those of vkv_distance_transform_weighted; d_dist2 may be null), with the same
// scratch block, and vkv_propagate_labels after its checks (b inside e, components_launch_ok; d_mask_vol null: no mask)
int launch_nearest_target(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int target, const uint32_t weights[3], uint32_t limit,
                          void *d_scratch, uint32_t *d_nearest, uint32_t *d_dist2, hipStream_t s);
int launch_propagate_labels(vkv_ctx *ctx, const uint32_t *d_nearest, const uint32_t *d_labels, uint32_t *d_out, VkvExtent3D e, const VkvBox &b,
                            const uint8_t *d_mask_vol, float mask_iso, hipStream_t s);

// ---- geodesic.hip
// vkv_geodesic_scratch_bytes (0 for an extent or box that is not accepted) and vkv_geodesic_propagate after the entry point's argument checks
// (b inside e, components_launch_ok, steps and limit valid, rounds 1 .. VKV_GEODESIC_MAX_ROUNDS; d_seeds is not read on a resumed call)
size_t geodesic_scratch_bytes(VkvExtent3D e, const VkvBox *box);
int launch_geodesic_propagate(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint32_t *d_seeds, const uint32_t steps[7],
                              uint32_t limit, uint32_t rounds, bool resume, void *d_scratch, uint32_t *d_dist, uint32_t *d_labels, uint64_t *d_counts,
                              hipStream_t s);

// ---- raymarch.hip
// vkv_render /vkv_render_batch (n frames in one launch) after the entry point's argument checks
int launch_render(vkv_ctx *ctx, const VkvRenderParams *P, const float *alpha_lut, hipStream_t s);
int launch_render_batch(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, const float *alpha_luts, hipStream_t s);
// vkv_prepare_render: everything a later launch of these n parameter blocks on s takes from the context, created now
int prepare_render(vkv_ctx *ctx, const VkvRenderParams *P, uint32_t n, hipStream_t s);
// loads the start-order kernels' code object on the current device (vkv_register_target)
void load_feedback_code();

// ---- capi.hip: argument checks that entry points of several files share; `what` is the entry point's name in the messages
// VKV_OK for null (the whole volume) or a box inside extent (extent_and_box_ok, box_domain.hpp)
int check_box(vkv_ctx *ctx, const char *what, VkvExtent3D extent, const VkvBox *box);
// a VkvRenderParams' tile schedule and buffers (vkv_render / vkv_render_batch and the direct renderers, direct_render.hpp)
int check_tile_schedule(vkv_ctx *ctx, const char *what, const VkvRenderParams *P);
int check_render_buffers(vkv_ctx *ctx, const char *what, const VkvRenderParams *P, bool own_output);
}        // namespace vkv

// raymarch_args.hpp — the argument block of the ray-march kernels (RayMarchArgs) and the per-lane ray state (Ray), with the two constants of the
// launch interface.  No device function and no HIP header: it compiles as plain host C++.  Included by render_args.hpp (the host code that
// fills the block) and by every device header of the integrator (ray_setup.hpp, raymarch_persistent.hpp, raymarch_core.hpp).
#pragma once

#include <stdint.h>

#include "../host/host_arith.hpp"        // UniformDiv

constexpr int kTraceWords = 10;        // u64 words per wave of the diagnostic trace buffer
constexpr uint32_t kFillPerTile = 3;   // VkvTileSchedule.fill_outside: outside tiles a rendering tile fills at most (lean_block)

struct RayMarchArgs
{
	// ray generator + RayCastUniform
	float dir00[3], ddx[3], ddy[3];
	float cam[3];
	float plane_tex[4];
	float block_size[3];
	// the ray set-up's divisions by the block size (ray_setup.hpp): 1 / block_size per axis where that is exact (a power of two in range), else 0,
	// and block_pow2 != 0 when all three are; ord_lo0 = the start value of a lane's smallest operand magnitude - ~0u, or 0 when a block size is
	// outside the fast divisions' range
	float    block_rcp[3];
	uint32_t block_pow2, ord_lo0;
	// CameraUniform matrices needed for gl_FragDepth (frag:319)
	float model[16], view[16], proj[16];
	float view_proj_inv[16], model_inv[16];        // DEPTH_ATTACHMENT only (frag:154-156)
	// TransferFunctionUniform
	float sampling_factor, grad_modifier;
	// extents
	int W, H, D, mw, mh, md;
	const uint8_t * vol, *grad, *tf;
	const uint8_t * packed;         // vkv_pack_volume image (PACKED variants) or null
	int             pmx, pmy;       // macro-bricks per axis of the packed image
	const uint32_t *tf_bits;        // vkv_transfer_function_tables buffer (alpha>0 bit table, flags, separable alpha tables) or null
	const uint8_t * maps[8];
	float *         out_color;
	uint8_t *       out_rgba8;
	uint32_t *      out_counts;
	float *         out_depth;
	const float *   in_depth;           // scene depth (options.depth_attachment) or null
	uint32_t        depth_attachment, blend;
	uint32_t        img_w, img_h, tile_w, tile_h, tiles_x, tile_first, tile_stride, tile_count, compact;        // tiles_x: tile columns of the schedule's rectangle
	uint32_t        org_x, org_y;   // first pixel column / row of the schedule's tile rectangle (VkvTileSchedule.rect; 0, 0 = the whole image)
	// VkvTileSchedule.fill_outside (k_raymarch_lean*): fill_tiles = tiles of the image OUTSIDE the rectangle (0 = nothing to fill); the rendering
	// workgroups write the no-fragment result there, schedule entry k the outside tiles k, k + tile_count, ...
	uint32_t        fill_tiles, img_tiles_x, rect_tx0, rect_ty0, rect_th;
	uint32_t        fill_rgba8_rows;        // != 0: the only output is RGBA8, nothing is blended, image rows are 16-byte aligned - outside tiles are cleared with 16-byte stores
	uint32_t        blocks_per_tile_x, blocks_per_tile, nblocks;
	int             test;
	unsigned long long *trace;      // diagnostic (tools/wave_trace.py): kTraceWords x u64 per wave {t_start, t_end, iterations, unit, phase sums}, or null
	int             back;           // ceil(sampling_factor): the step back after a probe that found an occupied cell (frag:253)
	uint32_t        clamp_always;   // k_raymarch_lean: 1 = no clamp-free march loop (VkvTuning.clamp_always: A/B switch, same bits)
	float           mapf[3], mapb[3];        // k_raymarch_lean, clamp-free loop: the map extent as floats, and the largest floats below them
	// launch-uniform values the kernels used to derive in every wave, from the host (fill_render_args; helpers and their exactness: host_arith.hpp):
	// cells_per_unit = (float) extent / block_size per axis (frag:192; zeros without empty-space skipping), free_margin = the clamp-free loop's g,
	// and the schedule's integer divisions as multiply-and-shift (div_per_row: by img_tiles_x - tiles_x, the fill's tiles left and right of the rectangle)
	float           cells_per_unit[3], free_margin;
	vkv::UniformDiv div_blocks_per_tile, div_blocks_per_tile_x, div_tiles_x, div_img_tiles_x, div_per_row;
	uint32_t        wave_pw_log2;            // k_raymarch_lean: log2 of the width in pixels of a wave's 64-pixel patch (2, 3, 4: 4x16, 8x8, 16x4)
	const uint32_t *addr_lut;       // k_raymarch_lean: per-axis byte offsets of the packed image (packed_addr_lut, context.hpp), or null
	uint32_t        lut_y, lut_z, lut_words;        // word offsets of the y and z tables inside addr_lut and the length of the two-level tables
	uint32_t        lut_full;       // word offset inside addr_lut of the prebuilt per-voxel-index tables (16-byte aligned, zero-padded to 16 bytes), 0 = none
	uint32_t        cull_x0, cull_x1, cull_y0, cull_y1;        // k_raymarch_lean: pixels outside [x0, x1] x [y0, y1] cannot see the volume's box
	                                                           // (conservative screen bound from the launcher); 0, ~0, 0, ~0 = no bound
	const uint32_t *tile_order;     // k_raymarch_lean: the r-th tile to be started is schedule entry tile_order[r] (centre of the image first), or null
	// no tile_order and order_h != 0: the start order is computed (start_entry) - the rings of the schedule's tiles_x x order_h rectangle of tiles from the
	// innermost outwards (schedules that hold every tile of their rectangle)
	uint32_t        order_h;
	uint32_t *      queue_heads;        // persistent scheduler: 8 tile-queue heads (one per XCD label), zeroed per launch
	// start-order feedback (raymarch.hip, TileFeedback): every marching wave leaves max(its iteration count) in tile_cost[schedule entry];
	// before the next frame into the same target k_tile_order_from_cost turns the costs into a longest-first order (order_out = the
	// buffer tile_order then points to).  Both null when unused.
	uint32_t *      tile_cost;
	uint32_t *      order_out;
	float           alpha_lut[256];     // opacity correction keyed by the TF alpha byte (frag:283)
};

// Per-lane ray state (everything main() of the frag keeps across loop iterations).
struct Ray
{
	float          ex, ey, ez;         // ray_entry
	float          sx, sy, sz;         // step_volume
	float          six, siy, siz;      // step_dist_texel_inv (frag:195)
	const uint8_t *dmap;               // distance map of this ray (anisotropic: chosen by direction octant, frag:209)
	int            n_steps, i, i_min;
	int            ulx, uly, ulz;      // u_last_alpha
	uint32_t       ul;                 // u_last_alpha as a linear cell index (k_raymarch_er)
	int            first_hit;
	bool           occupied;
	float          r, g, b, a;         // out_color
	float          depth;
	uint32_t       n_vol, n_dist, n_empty;
	uint32_t       o;                  // output index of the pixel
	bool           fragment;           // false: no fragment for this pixel (not covered, or discarded by the depth test)
};

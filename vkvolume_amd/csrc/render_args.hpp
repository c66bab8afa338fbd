// render_args.hpp — VkvRenderParams -> the fields of RayMarchArgs that the integrator (fill_render_args, raymarch.hip) and the direct renderers
// (fill_direct_args, direct_render.hpp) fill alike, and the shape of a wave's pixel patch.  It
// defines host functions only: RayMarchArgs comes from raymarch_args.hpp (no device code), VkvRenderParams and packed_dims from vkv_device.hpp.
// Included by raymarch.hip and direct_render.hpp.
#pragma once

#include <cmath>

#include "vkv_device.hpp"
#include "raymarch_args.hpp"

using namespace vkv;

// everything here is internal to the translation unit that includes it (no exported symbols)
namespace
{

// log2 of the width of a wave's 64-pixel patch (2, 3, 4: 4x16, 8x8 or 16x4 pixels) for a view: voxels per pixel step in x against y
// (texture-space ray increments x the extent)
uint32_t wave_patch_log2(const float ddx[3], const float ddy[3], int W, int H, int D)
{
	double       vx = 0.0, vy = 0.0;
	const double dim[3] = {(double) W, (double) H, (double) D};
	for (int k = 0; k < 3; ++k)
		vx += (double) ddx[k] * dim[k] * (double) ddx[k] * dim[k], vy += (double) ddy[k] * dim[k] * (double) ddy[k] * dim[k];
	const double r = (vx > 0.0 && vy > 0.0) ? std::sqrt(vx / vy) : 1.0;
	return r >= 1.6 ? 2u : (r <= 1.0 / 1.6 ? 4u : 3u);
}

// The shared fields: ray generator, camera, plane and matrices, sampling_factor, extents, volume and packed image, the four common outputs,
// image and tile size, the schedule with its tile rectangle (all zero: the whole image; tiles are numbered row-major inside it) and the
// blocks of a tile.  Returns true when the schedule is over the whole image.  Everything else is the caller's.
bool fill_shared_args(const VkvRenderParams *P, RayMarchArgs &a)
{
	for (int i = 0; i < 3; ++i)
		a.dir00[i] = P->ray_gen.dir00[i], a.ddx[i] = P->ray_gen.ddx[i], a.ddy[i] = P->ray_gen.ddy[i], a.cam[i] = P->ray_cast.camera_pos_tex[i];
	for (int i = 0; i < 4; ++i)
		a.plane_tex[i] = P->ray_cast.plane_tex[i];
	for (int i = 0; i < 16; ++i)
		a.model[i] = P->camera.model[i], a.view[i] = P->camera.camera_view[i], a.proj[i] = P->camera.camera_proj[i],
		a.view_proj_inv[i] = P->camera.camera_view_proj_inv[i], a.model_inv[i] = P->camera.model_inv[i];
	a.sampling_factor = P->transfer_function.sampling_factor;
	a.W = (int) P->volume_extent.width, a.H = (int) P->volume_extent.height, a.D = (int) P->volume_extent.depth;
	a.mw = (int) P->map_extent.width, a.mh = (int) P->map_extent.height, a.md = (int) P->map_extent.depth;
	a.vol    = P->d_volume;
	a.packed = static_cast<const uint8_t *>(P->d_packed_volume);
	{
		const PackedDims pd = packed_dims(a.W, a.H, a.D);
		a.pmx = pd.mx, a.pmy = pd.my;
	}
	a.out_color = P->d_out_color, a.out_rgba8 = P->d_out_rgba8, a.out_counts = P->d_out_counts, a.out_depth = P->d_out_depth;
	a.depth_attachment = P->options.depth_attachment != 0;
	a.img_w = P->image_width, a.img_h = P->image_height;
	a.tile_w = P->tiles.tile_width, a.tile_h = P->tiles.tile_height;
	a.tile_first = P->tiles.tile_first, a.tile_stride = P->tiles.tile_stride, a.tile_count = P->tiles.tile_count, a.compact = P->tiles.compact;
	const VkvTileRect &r     = P->tiles.rect;
	const bool         whole = r.w == 0 || r.h == 0;
	a.tiles_x                = whole ? (a.img_w + a.tile_w - 1) / a.tile_w : r.w;
	a.org_x = whole ? 0u : r.x0 * a.tile_w, a.org_y = whole ? 0u : r.y0 * a.tile_h;
	a.blocks_per_tile_x = a.tile_w / 16;
	a.blocks_per_tile   = a.blocks_per_tile_x * (a.tile_h / 16);
	return whole;
}

}        // namespace

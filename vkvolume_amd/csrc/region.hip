// region.hip — vkv_update_volume_region: new voxels for a box of the volume, then only what they can change of the gradient map, the packed
// image and the occupancy map, then the whole-map transform.  No kernel of its own: it chains the launchers of volume_io.hip, gradient.hip,
// pack.hip, occupancy.hip and distance.hip.
#include <algorithm>

#include "launchers.hpp"

namespace vkv
{

// vkv_update_volume_region (include/vkvolume_amd.h), after the entry point's argument checks.  The size limits of every launch below are
// checked before the first one, so a call this rejects writes nothing.
int launch_update_volume_region(vkv_ctx *ctx, const void *d_src, int type, bool big_endian, float lo, float hi, const VkvBox &box, uint8_t *d_vol,
                                uint8_t *d_grad, void *d_packed, VkvExtent3D e, const uint8_t *d_tf, const VkvTransferFunctionUniform *tf,
                                uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D me, int skipping_type, hipStream_t s)
{
	const uint32_t ext[3] = {e.width, e.height, e.depth}, org[3] = {box.x0, box.y0, box.z0}, size[3] = {box.width, box.height, box.depth};
	// the box grown by one voxel per side and clamped to the volume: where the gradient can change (a voxel's gradient reads its +-1
	// neighbours), and with it the packed bricks and the occupancy cells
	uint32_t g0[3], g1[3];
	for (int a = 0; a < 3; ++a)
		g0[a] = org[a] > 0 ? org[a] - 1 : 0, g1[a] = std::min(org[a] + size[a] + 1, ext[a]);        // (org + size <= ext was checked in 64 bits)
	const VkvBox     grown = {g0[0], g0[1], g0[2], g1[0] - g0[0], g1[1] - g0[1], g1[2] - g0[2]};
	const PackedDims pd    = packed_dims((int) e.width, (int) e.height, (int) e.depth);
	// ---- limits (those of the whole-volume launchers: any volume they build can be updated)
	if (e.depth > 65535u || (uint64_t) ((e.width + 63) / 64) * ((e.height + 3) / 4) > 0xffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "update_volume_region: volume too large for one launch");
	if (d_packed && ((uint64_t) pd.mx * pd.my * pd.mz * 512 > 0xffffffffull || (uint64_t) pd.bx * pd.by > 0xffffffull))
		return set_error(ctx, VKV_E_UNSUPPORTED, "update_volume_region: pack_volume: volume too large");
	const bool aniso = skipping_type == VKV_SKIP_ANISOTROPIC_DISTANCE, transform = aniso || skipping_type == VKV_SKIP_DISTANCE;
	uint32_t   c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
	StreamScratch scratch;        // held from the bit table to the last map pass
	if (d_maps)
	{
		if (!occupancy_launch_ok(e, me) || (transform && !distance_launch_ok(me)))
			return set_error(ctx, VKV_E_UNSUPPORTED, "update_volume_region: map too large for one launch");
		const uint32_t mext[3] = {me.width, me.height, me.depth};
		for (int a = 0; a < 3; ++a)        // src/compute_distance_map.cpp:110-113; the cells that meet the grown box
		{
			const uint32_t blk = block_of(ext[a], mext[a]);
			c0[a] = g0[a] / blk, c1[a] = (g1[a] - 1) / blk + 1;
		}
		if (!(scratch = stream_scratch(ctx, s)).p)
			return VKV_E_UNSUPPORTED;
	}
	// ---- 1. convert the source box into the volume; 2. gradient of the grown box; 3. the bricks whose texels read a changed byte
	int rc = launch_convert_box(ctx, d_src, type, big_endian, lo, hi, box, d_vol, e, s);
	if (rc != VKV_OK)
		return rc;
	if (d_grad && (rc = launch_gradient_map_box(ctx, d_vol, d_grad, e, grown, tf, s)) != VKV_OK)
		return rc;
	if (d_packed)
	{
		// brick b reads voxels 4b - 1 .. 4b + 3 (clamped): the bricks [g0 / 4, (g1 - 1 + 1) / 4] per axis, and up to the last brick when the grown box
		// reaches the volume's far face (the apron bricks there read only the clamped last voxel)
		const int nb[3] = {pd.bx, pd.by, pd.bz};
		int       b0[3], b1[3];
		for (int a = 0; a < 3; ++a)
			b0[a] = (int) (g0[a] / 4), b1[a] = g1[a] == ext[a] ? nb[a] : std::min(nb[a], (int) (g1[a] / 4) + 1);
		if ((rc = launch_pack_volume_bricks(ctx, d_vol, d_grad, e, b0, b1, d_packed, s)) != VKV_OK)
			return rc;
	}
	if (!d_maps)
		return VKV_OK;
	// ---- 4. occupancy of the cells that meet the grown box, from the bit table of the texture (staged in the stream's scratch block)
	uint32_t *d_bits = reinterpret_cast<uint32_t *>(scratch.p + kTfBitsOffset);
	if ((rc = launch_tf_bits_columns(ctx, d_tf, d_bits, s)) != VKV_OK)
		return rc;
	uint8_t *occ = d_maps[aniso ? 7 : 0];
	if (c0[0] == 0 && c0[1] == 0 && c0[2] == 0 && c1[0] == me.width && c1[1] == me.height && c1[2] == me.depth)
		// every cell: the whole-map pass writes them all (its EMPTY fill is a kernel here)
		rc = launch_occupancy_map(ctx, d_vol, d_grad, d_tf, tf, e, occ, me, s, d_bits, true);
	else
		rc = launch_occupancy_map_cells(ctx, d_vol, d_grad, tf, e, occ, me, c0, c1, transform, s, d_bits);
	if (rc != VKV_OK)
		return rc;
	// ---- 5. the whole-map transform
	return launch_map_transform(ctx, d_maps, d_swap, me, skipping_type, s);
}

}        // namespace vkv

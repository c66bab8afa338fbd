// row_loads.hpp — device loads of voxel rows shared by cells.hip and mip.hip.
#pragma once

#include "vkv_device.hpp"

namespace vkv
{
// voxels x .. x + 3 of a row of W voxels (x < W) as one dword at any alignment; nothing past the row's last byte is read, the bytes of
// x + i >= W are zero
__device__ __forceinline__ uint32_t load4_clipped(const uint8_t *row, int x, int W)
{
	if (x + 4 <= W)
		return load_u32_any(row + x);
	if (W >= 4)
		return load_u32_any(row + (W - 4)) >> (8 * (x + 4 - W));
	uint32_t r = 0;
	for (int i = 0; x + i < W; ++i)
		r |= (uint32_t) row[x + i] << (8 * i);
	return r;
}
}        // namespace vkv

// addr_tables.hpp — host-only builder of the address tables of the packed sampling image (packed_addr_lut, context.hip).  Plain C++: no HIP
// header, so that a test driver built with the host compiler can include it (tests/test_addr_tables_cpu.py).
//
// Two-level tables (uint32 words): in-macro-brick terms of x, y, z at words 0, 32, 64 (padded index b & 31); macro-brick terms (b >> 5) of x
// at 96, of y at lut_y, of z as 64-bit values at lut_z (even).  Behind them, when asked for, the per-voxel-index tables a workgroup copies into
// its LDS (stage_full_lut, raymarch_core.hpp): X[W + 2], Y[H + 2], Z[D + 2], 32-bit offsets in units of two bytes, starting at word `full`
// (a multiple of 4: 16-byte aligned) and zero-padded to `full_words` (a multiple of 4).  Every full entry is the sum of its two two-level
// words shifted right by one, taken from the words written just above: the same integers by construction.
#pragma once

#include <stdint.h>

#include <vector>

namespace vkv
{
struct AddrTables
{
	uint32_t lut_y = 0, lut_z = 0, words = 0;        // two-level tables: word offsets of the y and z macro terms, their total length
	uint32_t full = 0, full_words = 0;               // per-voxel-index tables: first word and padded length (0, 0 = not built)
};

// mx, my: macro-bricks per axis of the packed image (packed_dims); with_full: append the per-voxel-index tables (only meaningful while the
// packed image is at most 8 GiB: the z term must fit 33 bits before the shift)
inline AddrTables build_addr_tables(int W, int H, int D, int mx, int my, bool with_full, std::vector<uint32_t> &h)
{
	AddrTables     t;
	const uint32_t nmx = (uint32_t) (W + 1) / 32 + 1, nmy = (uint32_t) (H + 1) / 32 + 1, nmz = (uint32_t) (D + 1) / 32 + 1;
	const uint32_t ny = 96 + nmx, nz = (ny + nmy + 1) & ~1u, total = nz + 2 * nmz;
	t.lut_y = ny, t.lut_z = nz, t.words = total;
	const uint32_t nx_full = (uint32_t) W + 2u, ny_full = (uint32_t) H + 2u, nz_full = (uint32_t) D + 2u;
	if (with_full)
		t.full = (total + 3u) & ~3u, t.full_words = (nx_full + ny_full + nz_full + 3u) & ~3u;
	h.assign((size_t) (with_full ? t.full + t.full_words : total), 0u);
	for (uint32_t j = 0; j < 32; ++j)
	{
		h[j]      = (((j >> 2) & 7u) << 8) + (j & 3u) * 2u;
		h[32 + j] = (((j >> 2) & 7u) << 11) + (j & 3u) * 10u;
		h[64 + j] = (((j >> 2) & 7u) << 14) + (j & 3u) * 50u;
	}
	for (uint32_t m = 0; m < nmx; ++m)
		h[96 + m] = m << 17;
	for (uint32_t m = 0; m < nmy; ++m)
		h[ny + m] = (m * (uint32_t) mx) << 17;
	for (uint32_t m = 0; m < nmz; ++m)
	{
		const uint64_t z = ((uint64_t) m * (uint64_t) my * (uint64_t) mx) << 17;
		h[nz + 2 * m] = (uint32_t) z, h[nz + 2 * m + 1] = (uint32_t) (z >> 32);
	}
	if (with_full)
	{
		uint32_t *fx = h.data() + t.full, *fy = fx + nx_full, *fz = fy + ny_full;
		for (uint32_t b = 0; b < nx_full; ++b)
			fx[b] = (h[b & 31u] + h[96u + (b >> 5)]) >> 1;
		for (uint32_t b = 0; b < ny_full; ++b)
			fy[b] = (h[32u + (b & 31u)] + h[ny + (b >> 5)]) >> 1;
		for (uint32_t b = 0; b < nz_full; ++b)
			fz[b] = (uint32_t) ((((((uint64_t) h[nz + 2u * (b >> 5) + 1u]) << 32) | h[nz + 2u * (b >> 5)]) + h[64u + (b & 31u)]) >> 1);
	}
	return t;
}
}        // namespace vkv

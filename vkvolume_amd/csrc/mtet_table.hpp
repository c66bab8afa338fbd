// mtet_table.hpp — the case table of marching tetrahedra on the Kuhn decomposition of a cube (vkv_isosurface_mesh, mesh.hip),
// computed at compile time from the definition.  Plain C++17 without device code: mesh.hip copies the table into constant memory and
// tests/mtet_driver.cpp prints it for the comparison with the numpy statement.
//
// Cube corner j = dx + 2 dy + 4 dz.  Tetrahedron t has the corners kMtetCorners[t] (its local vertices 0 .. 3 in that order): the path from
// corner 0 to corner 7 that adds the axes in a permutation's order; kMtetOdd[t] tells an odd permutation.  Mask m: bit i set = local vertex i
// inside.  An edge is a pair of local vertices; its mesh vertex is interpolated from the LOWER local vertex `a` to the higher one `b`, so that
// b - a is 0 or 1 per axis.  An entry holds its triangles' edges as cube corners a | b << 3, with the winding swap already applied.
#pragma once

#include <cstdint>

namespace vkv
{

constexpr int  kMtetCorners[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
constexpr bool kMtetOdd[6]        = {false, true, true, false, false, true};
// the masks whose triangles, as listed below, face the inside vertices on an even tetrahedron
constexpr uint32_t kMtetFlipMasks = 1u << 2 | 1u << 5 | 1u << 8 | 1u << 10 | 1u << 11 | 1u << 14;

struct alignas(8) MtetCase        // read as one 64-bit word: n | swap << 8 | e[k] << (16 + 8 k)
{
	uint8_t n;           // triangles: 0, 1 or 2
	uint8_t swap;        // the second and third vertex of each triangle were swapped
	uint8_t e[6];        // triangle k has the edges e[3 k .. 3 k + 2]: cube corners a | b << 3
};

struct MtetTable
{
	MtetCase c[6][16];
	uint8_t  count[256];        // triangles of a cube by its 8-bit corner mask: the sum over its six tetrahedra, at most 12
};

// the 4-bit mask of tetrahedron t from a cube's corner mask
constexpr uint32_t mtet_submask(int t, uint32_t corner_mask)
{
	uint32_t m = 0;
	for (int i = 0; i < 4; ++i)
		m |= ((corner_mask >> kMtetCorners[t][i]) & 1u) << i;
	return m;
}

constexpr MtetTable make_mtet_table()
{
	MtetTable T{};
	for (int t = 0; t < 6; ++t)
		for (uint32_t m = 0; m < 16; ++m)
		{
			int ins[4] = {}, out[4] = {}, ni = 0, no = 0;
			for (int i = 0; i < 4; ++i)
				if ((m >> i) & 1u)
					ins[ni++] = i;
				else
					out[no++] = i;
			int tri[2][3][2] = {}, n = 0;        // [triangle][vertex][end of its edge]
			if (ni == 1)
			{
				for (int k = 0; k < 3; ++k)
					tri[0][k][0] = ins[0], tri[0][k][1] = out[k];
				n = 1;
			}
			else if (ni == 3)
			{
				for (int k = 0; k < 3; ++k)
					tri[0][k][0] = ins[k], tri[0][k][1] = out[0];
				n = 1;
			}
			else if (ni == 2)
			{
				const int A[2] = {ins[0], out[0]}, B[2] = {ins[0], out[1]}, C[2] = {ins[1], out[1]}, D[2] = {ins[1], out[0]};
				for (int j = 0; j < 2; ++j)
				{
					tri[0][0][j] = A[j], tri[0][1][j] = B[j], tri[0][2][j] = C[j];
					tri[1][0][j] = A[j], tri[1][1][j] = C[j], tri[1][2][j] = D[j];
				}
				n = 2;
			}
			const bool swap = kMtetOdd[t] != (((kMtetFlipMasks >> m) & 1u) != 0);
			MtetCase & c    = T.c[t][m];
			c.n = (uint8_t) n, c.swap = (uint8_t) (n > 0 && swap);
			for (int k = 0; k < n; ++k)
				for (int v = 0; v < 3; ++v)
				{
					const int  w  = (swap && v > 0) ? 3 - v : v;
					const int *ed = tri[k][w];
					const int  lo = ed[0] < ed[1] ? ed[0] : ed[1], hi = ed[0] < ed[1] ? ed[1] : ed[0];        // by local index, not by side
					c.e[3 * k + v] = (uint8_t) (kMtetCorners[t][lo] | kMtetCorners[t][hi] << 3);
				}
		}
	for (uint32_t cm = 0; cm < 256; ++cm)
	{
		int n = 0;
		for (int t = 0; t < 6; ++t)
			n += T.c[t][mtet_submask(t, cm)].n;
		T.count[cm] = (uint8_t) n;
	}
	return T;
}

constexpr MtetTable kMtetTable = make_mtet_table();
static_assert(kMtetTable.count[0] == 0 && kMtetTable.count[255] == 0 && kMtetTable.count[1] == 6 && kMtetTable.count[0x0f] == 8 &&
                  kMtetTable.count[0x17] == 12,
              "corner 0 meets all six tetrahedra; corners 0, 1, 2, 4 inside cut every tetrahedron two and two: the most, twelve triangles");

}        // namespace vkv

// Prints the marching-tetrahedra case table of vkvolume_amd/csrc/mtet_table.hpp, the header mesh.hip copies into constant memory, for the
// entry-by-entry comparison with the numpy statement in tests/test_mesh_cpu.py.  Plain host C++ with its own main.
//   case <tetrahedron> <mask> <triangles> <swap> <a b of each edge, three edges per triangle>
//   count <corner mask> <triangles of the cube>
#include <cstdio>

#include "mtet_table.hpp"

int main()
{
	const vkv::MtetTable &T = vkv::kMtetTable;
	for (int t = 0; t < 6; ++t)
	{
		std::printf("tet %d %d %d %d %d %d\n", t, vkv::kMtetCorners[t][0], vkv::kMtetCorners[t][1], vkv::kMtetCorners[t][2], vkv::kMtetCorners[t][3],
		            (int) vkv::kMtetOdd[t]);
		for (int m = 0; m < 16; ++m)
		{
			const vkv::MtetCase &c = T.c[t][m];
			std::printf("case %d %d %d %d", t, m, (int) c.n, (int) c.swap);
			for (int k = 0; k < 3 * c.n; ++k)
				std::printf(" %d %d", c.e[k] & 7, c.e[k] >> 3);
			std::printf("\n");
		}
	}
	for (int cm = 0; cm < 256; ++cm)
		std::printf("count %d %d\n", cm, (int) T.count[cm]);
	std::printf("mtet ok\n");
	return 0;
}

// Driver of tests/test_addr_tables_cpu.py: prints the address tables packed_addr_lut builds for the extents on the command line.
// usage: addr_tables_driver W H D   ->   "lut_y lut_z words full full_words", then every table word, one per line
#include <cstdio>
#include <cstdlib>

#include "../vkvolume_amd/csrc/addr_tables.hpp"

int main(int argc, char **argv)
{
	if (argc != 4)
		return 2;
	const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), D = std::atoi(argv[3]);
	// macro-bricks per axis as packed_dims (vkv_device.hpp) counts them: bricks of 4 padded voxels, 8 bricks per macro-brick
	const int mx = ((((W + 1) >> 2) + 1) + 7) >> 3, my = ((((H + 1) >> 2) + 1) + 7) >> 3;
	std::vector<uint32_t> h;
	const vkv::AddrTables t = vkv::build_addr_tables(W, H, D, mx, my, true, h);
	std::printf("%u %u %u %u %u\n", t.lut_y, t.lut_z, t.words, t.full, t.full_words);
	for (uint32_t w : h)
		std::printf("%u\n", w);
	return 0;
}

// Exhaustive zero-one check of vkvolume_amd/csrc/median27_network.hpp (built and run by tests/test_filter_cpu.py with the host compiler).
// The network is instantiated on 64-bit bit slices, lo = AND and hi = OR: bit k of input word i is value i of the k-th of 64 zero/one inputs.
// All 2^27 inputs are run (inputs 0..5 vary inside a word, inputs 6..26 with the loop counter) and the output bit compared with the median
// of zeros and ones: 1 iff at least 14 of the 27 are 1.  A second mode checks the stages on their own: sort3 and merge_triples must sort.
#include <cstdint>
#include <cstdio>

#include "median27_network.hpp"

struct BitOps
{
	uint64_t lo(uint64_t a, uint64_t b) const { return a & b; }
	uint64_t hi(uint64_t a, uint64_t b) const { return a | b; }
};

static const uint64_t kLane[6] = {0xaaaaaaaaaaaaaaaaull, 0xccccccccccccccccull, 0xf0f0f0f0f0f0f0f0ull,
                                  0xff00ff00ff00ff00ull, 0xffff0000ffff0000ull, 0xffffffff00000000ull};

int main()
{
	const BitOps op;
	// the nine-sorter (three sort3 + merge_triples) on all 2^9 zero/one inputs: output i is 1 iff at least 9 - i inputs are 1
	for (uint32_t hi_bits = 0; hi_bits < 8; ++hi_bits)
	{
		uint64_t v[9];
		for (int i = 0; i < 9; ++i)
			v[i] = i < 6 ? kLane[i] : (((hi_bits >> (i - 6)) & 1u) ? ~0ull : 0ull);
		uint64_t in[9];
		for (int i = 0; i < 9; ++i)
			in[i] = v[i];
		for (int t = 0; t < 3; ++t)
			vkv::sort3(v[3 * t], v[3 * t + 1], v[3 * t + 2], op);
		vkv::merge_triples(v, op);
		for (int k = 0; k < 64; ++k)
		{
			int ones = 0;
			for (int i = 0; i < 9; ++i)
				ones += (int) ((in[i] >> k) & 1u);
			for (int i = 0; i < 9; ++i)
				if ((int) ((v[i] >> k) & 1u) != (i >= 9 - ones ? 1 : 0))
				{
					std::printf("nine-sorter: output %d wrong for input %u\n", i, (hi_bits << 6) | (uint32_t) k);
					return 1;
				}
		}
	}
	uint64_t checked = 0;
	for (uint32_t upper = 0; upper < (1u << 21); ++upper)
	{
		uint64_t v[27];
		int      upper_ones = 0;
		for (int i = 0; i < 6; ++i)
			v[i] = kLane[i];
		for (int i = 6; i < 27; ++i)
		{
			const uint32_t bit = (upper >> (i - 6)) & 1u;
			v[i] = bit ? ~0ull : 0ull;
			upper_ones += (int) bit;
		}
		const uint64_t got = vkv::median27(v, op);
		uint64_t       want = 0;
		for (int k = 0; k < 64; ++k)
			if (upper_ones + __builtin_popcount((unsigned) k) >= 14)
				want |= 1ull << k;
		if (got != want)
		{
			std::printf("median27: wrong for inputs with upper bits %u: got %016llx want %016llx\n", upper, (unsigned long long) got,
			            (unsigned long long) want);
			return 1;
		}
		checked += 64;
	}
	std::printf("median27 ok: %llu inputs\n", (unsigned long long) checked);
	return 0;
}

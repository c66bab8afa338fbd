// uniform_div_driver.cpp — host check of the launch-uniform arithmetic the ray-march kernels take from the host (vkvolume_amd/host/host_arith.hpp):
// UniformDiv (quotient and remainder against / and %) and the float helpers (against the plain expressions).  The functions are the ones the
// kernels compile: plain C++ here.  Built and run by tests/test_uniform_div_cpu.py; prints "uniform div driver: ok" or the first failures.
#include <stdint.h>
#include <stdio.h>

#include "../vkvolume_amd/host/host_arith.hpp"

using namespace vkv;

static uint64_t g_checked = 0;
static int      g_failed  = 0;

static void check(uint32_t n, uint32_t d, const UniformDiv &v)
{
	uint32_t q, r;
	uniform_divmod(n, d, v, q, r);
	++g_checked;
	if ((q != n / d || r != n % d || uniform_quot(n, v) != n / d) && g_failed++ < 10)
		printf("FAIL %u / %u: got %u rem %u, want %u rem %u (mul %u shift %u)\n", n, d, q, r, n / d, n % d, v.mul, v.shift);
}

static uint32_t hash32(uint32_t x)
{
	x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
	return x;
}

static void check_divisor(uint32_t d)
{
	const UniformDiv v = uniform_div_of(d);
	if (v.shift > 30u || v.mul < (1u << 30) || v.mul >= (1u << 31))        // (n << 2) * mul then fits 64 bits with room to spare
	{
		if (g_failed++ < 10)
			printf("FAIL divisor %u: mul %u shift %u out of range\n", d, v.mul, v.shift);
		return;
	}
	const uint32_t top = kUniformDivMax;        // the largest numerator the launch checks admit: 0x3fffffff blocks, 2^30 - 1 output indices
	const uint32_t fixed[] = {0u, 1u, d - 1u, d, d + 1u, (1u << 30) - 1u, top, top - 1u, top / d * d, top / d * d - 1u};
	for (uint32_t n : fixed)
		if (n <= top)
			check(n, d, v);
	for (uint32_t i = 0; i < 16; ++i)
	{        // multiples of d and their neighbours, for hashed factors k over the whole range of quotients
		const uint32_t kmax = top / d;
		const uint32_t k    = kmax == 0 ? 0 : 1u + hash32(d * 16u + i) % kmax;
		const uint64_t m    = (uint64_t) k * d;
		if (m >= 1 && m - 1 <= top)
			check((uint32_t) (m - 1), d, v);
		if (m <= top)
			check((uint32_t) m, d, v);
		if (m + 1 <= top)
			check((uint32_t) (m + 1), d, v);
	}
}

int main()
{
	static_assert(kUniformDivMax == 0x3fffffffu, "the numerator bound is the launch's block and output-index limit");
	for (uint32_t d = 1; d <= 65536u; ++d)
		check_divisor(d);
	for (uint32_t s = 17; s <= 30; ++s)        // beyond what a frame can hold: every power of two and its neighbours up to the numerator bound
		for (uint32_t d : {(1u << s) - 1u, 1u << s, (1u << s) + 1u})
			if (d <= kUniformDivMax)
				check_divisor(d);
	for (uint32_t d = 1; d <= 64u; ++d)
	{
		const UniformDiv v = uniform_div_of(d);
		for (uint32_t n = 0; n < (1u << 20); ++n)
			check(n, d, v);
	}
	{        // a divisor of 0 (nothing to divide: a launch that fills no tiles) gives quotient 0 and divides nothing by zero
		const UniformDiv v = uniform_div_of(0u);
		if (uniform_quot(12345u, v) != 0u && g_failed++ < 10)
			printf("FAIL divisor 0\n");
	}
	// the float helpers are the plain single-precision expressions (this file is built with -ffp-contract=off like the library)
	uint64_t floats = 0;
	for (int e = 1; e <= 2048; ++e)
		for (int b = 1; b <= 17; ++b)
		{
			const volatile float fe = (float) e, fb = (float) b;
			const float want = fe / fb, got = cells_per_unit(e, (float) b);
			++floats;
			if (__builtin_memcmp(&want, &got, 4) != 0 && g_failed++ < 10)
				printf("FAIL cells_per_unit(%d, %d): %a, want %a\n", e, b, got, want);
		}
	for (int e = 1; e <= 2048; ++e)
	{
		const int other[] = {1, e / 2 + 1, e};
		for (int a : other)
			for (int c : other)
			{
				const volatile float fm = (float) e, quarter = 0.25f;
				const float want = quarter / fm;
				const float got[] = {clamp_free_margin(e, a, c), clamp_free_margin(a, e, c), clamp_free_margin(a, c, e)};
				for (float x : got)
				{
					++floats;
					if (__builtin_memcmp(&want, &x, 4) != 0 && g_failed++ < 10)
						printf("FAIL clamp_free_margin with longest extent %d: %a, want %a\n", e, x, want);
				}
			}
	}
	printf("checked %llu divisions, %llu float values\n", (unsigned long long) g_checked, (unsigned long long) floats);
	if (g_failed)
	{
		printf("uniform div driver: %d FAILED\n", g_failed);
		return 1;
	}
	printf("uniform div driver: ok\n");
	return 0;
}

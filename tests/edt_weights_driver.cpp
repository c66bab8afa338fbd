// edt_weights_driver.cpp — host check of what vkv_distance_transform_weighted works out before it enqueues anything
// (vkvolume_amd/host/host_arith.cpp): edt_weights_fit, the bound on the largest value the weights can give in a box, against the same sum in
// 128-bit integers, and edt_weighted_reach, the x pass's reach, against its definition.  Built with AddressSanitizer and
// UndefinedBehaviorSanitizer and run by tests/test_distance_weighted_cpu.py; prints "edt weights driver: ok" or the first failures.
#include <stdint.h>
#include <stdio.h>

#include "../vkvolume_amd/host/host_arith.hpp"

using namespace vkv;

static int g_failed = 0;

static void expect(bool got, bool want, uint32_t wx, uint32_t wy, uint32_t wz, uint32_t bw, uint32_t bh, uint32_t bd)
{
	if (got != want && g_failed++ < 10)
		printf("FAIL weights (%u, %u, %u) on %u x %u x %u: %s, want %s\n", wx, wy, wz, bw, bh, bd, got ? "accepted" : "refused", want ? "accepted" : "refused");
}

static bool fit(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t bw, uint32_t bh, uint32_t bd)
{
	const uint32_t w[3] = {wx, wy, wz};
	return edt_weights_fit(w, bw, bh, bd);
}

// the definition, where nothing can wrap: three squares below 2^96 summed in 128 bits
static bool fit_wide(uint32_t wx, uint32_t wy, uint32_t wz, uint32_t bw, uint32_t bh, uint32_t bd)
{
	const uint32_t    w[3] = {wx, wy, wz}, len[3] = {bw, bh, bd};
	unsigned __int128 sum  = 0;
	for (int a = 0; a < 3; ++a)
	{
		if (w[a] == 0u)
			return false;
		const unsigned __int128 far = (unsigned __int128) w[a] * (len[a] - 1u);
		sum += far * far;
	}
	return sum <= 0xfffffffeu;
}

static uint32_t hash32(uint32_t x)
{
	x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
	return x;
}

int main()
{
	// the issue's cases
	expect(fit(2, 362, 362, 32768, 2, 2), true, 2, 362, 362, 32768, 2, 2);        // the largest value: 65534^2 + 2 x 362^2 = 4 294 967 244
	if ((uint64_t) 65534 * 65534 + 2ull * 362 * 362 != 4294967244ull && g_failed++ < 10)
		printf("FAIL the largest value of (2, 362, 362) on 32768 x 2 x 2\n");
	expect(fit(2, 363, 362, 32768, 2, 2), false, 2, 363, 362, 32768, 2, 2);
	expect(fit(3, 1, 1, 32768, 1, 1), false, 3, 1, 1, 32768, 1, 1);        // 3 x 32767 > 65535
	expect(fit(0xffffffffu, 1, 1, 1, 4, 4), true, 0xffffffffu, 1, 1, 1, 4, 4);        // an axis of length 1: len - 1 is 0
	expect(fit(0xffffffffu, 0xffffffffu, 0xffffffffu, 1, 1, 1), true, 0xffffffffu, 0xffffffffu, 0xffffffffu, 1, 1, 1);
	expect(fit(0, 1, 1, 4, 4, 4), false, 0, 1, 1, 4, 4, 4);
	expect(fit(1, 0, 1, 4, 1, 4), false, 1, 0, 1, 4, 1, 4);        // a weight of 0 on an axis of length 1 as well
	expect(fit(1, 1, 0, 4, 4, 4), false, 1, 1, 0, 4, 4, 4);
	expect(fit(1, 1, 1, 32768, 32768, 3), true, 1, 1, 1, 32768, 32768, 3);        // the unweighted call's largest box
	expect(fit(0xffffffffu, 1, 1, 0xffffffffu, 1, 1), false, 0xffffffffu, 1, 1, 0xffffffffu, 1, 1);        // the product needs 64 bits
	expect(fit(65536, 1, 1, 65537, 1, 1), false, 65536, 1, 1, 65537, 1, 1);        // 2^32: the square would wrap a 64-bit sum to 0 were it formed first
	expect(fit(37837, 37837, 37837, 2, 2, 2), true, 37837, 37837, 37837, 2, 2, 2);        // 3 x 37837^2 = 4 294 915 707
	expect(fit(37838, 37837, 37837, 2, 2, 2), false, 37838, 37837, 37837, 2, 2, 2);       // + 75 675: past 0xfffffffe
	// hashed weights and shapes around the bound, against 128 bits
	uint64_t checked = 0, accepted = 0;
	for (uint32_t i = 0; i < 400000u; ++i)
	{
		const uint32_t h0 = hash32(3u * i), h1 = hash32(3u * i + 1u), h2 = hash32(3u * i + 2u);
		uint32_t       len[3], w[3];
		for (int a = 0; a < 3; ++a)
		{
			const uint32_t h = a == 0 ? h0 : (a == 1 ? h1 : h2);
			len[a]           = (h & 3u) == 0u ? 1u : 1u + (h >> 2) % 32768u;        // a quarter of the axes have length 1
			const uint32_t far = len[a] - 1u;
			const uint32_t top = far == 0u ? 0xffffffffu : 65535u / far;        // the largest weight the axis admits
			w[a]             = (h >> 17 & 7u) == 0u ? top + (top != 0xffffffffu) : 1u + (h >> 20) % (top ? top : 1u);        // an eighth lies just past it
		}
		const bool got = fit(w[0], w[1], w[2], len[0], len[1], len[2]), want = fit_wide(w[0], w[1], w[2], len[0], len[1], len[2]);
		expect(got, want, w[0], w[1], w[2], len[0], len[1], len[2]);
		++checked, accepted += want;
	}
	if ((accepted < checked / 20 || accepted > checked - checked / 20) && g_failed++ < 10)
		printf("FAIL the hashed cases do not straddle the bound: %llu of %llu accepted\n", (unsigned long long) accepted, (unsigned long long) checked);
	// the reach: the smallest r with (w r)^2 >= limit
	uint64_t reaches = 0;
	auto     reach_ok = [&](uint32_t limit, uint32_t w) {
        const uint64_t r = edt_weighted_reach(limit, w);
        ++reaches;
        const bool enough = (unsigned __int128) w * r * w * r >= limit;
        const bool least  = r == 0 || (unsigned __int128) w * (r - 1) * w * (r - 1) < limit;
        if ((!enough || !least || r > 65536u) && g_failed++ < 10)
            printf("FAIL reach(limit %u, weight %u) = %llu\n", limit, w, (unsigned long long) r);
	};
	for (uint32_t limit = 1; limit <= 5000u; ++limit)
		for (uint32_t w = 1; w <= 70u; ++w)
			reach_ok(limit, w);
	for (uint32_t s = 1; s <= 65536u; s += 13u)        // around every 13th square, and the ends
		for (uint32_t w : {1u, 2u, 3u, 5u, 7u, 255u, 362u, 65535u, 65536u, 0xffffffffu})
			for (uint64_t limit : {(uint64_t) s * s - 1u, (uint64_t) s * s, (uint64_t) s * s + 1u})
				if (limit >= 1u && limit <= 0xffffffffull)
					reach_ok((uint32_t) limit, w);
	for (uint32_t w : {1u, 2u, 65535u, 0xffffffffu})
		for (uint32_t limit : {1u, 2u, 0xfffffffeu, 0xffffffffu})
			reach_ok(limit, w);
	if (edt_weighted_reach(0xffffffffu, 1u) != 65536u && g_failed++ < 10)
		printf("FAIL the unlimited reach of weight 1\n");
	printf("checked %llu weight sets (%llu accepted), %llu reaches\n", (unsigned long long) checked, (unsigned long long) accepted, (unsigned long long) reaches);
	if (g_failed)
	{
		printf("edt weights driver: %d FAILED\n", g_failed);
		return 1;
	}
	printf("edt weights driver: ok\n");
	return 0;
}

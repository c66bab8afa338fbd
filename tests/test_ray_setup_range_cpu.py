"""The ray set-up's range test and its division shortcuts (ray_setup.hpp, vkv_device.hpp), checked on the host: a stand-alone C++ program,
compiled here from the header's own host-callable functions (hipcc's host pass only: no GPU, no kernel), that exits non-zero on the first
property that fails.

  * one operand, all 2^32 bit patterns: the accumulated form (ord_both + ord_ok) implies div_ordinary; the one-sided form (ord_low) implies
    it for every operand below 2 in magnitude (what a component of a normalised vector is);
  * the accumulated form over 28-tuples (25 operands and the three block sizes of the host's field), random and with every special value
    (+-0, denormals, 2^+-39, 2^+-40 and their neighbours, +-inf, quiet and signalling NaN) in every position: true only when every operand
    passes div_ordinary;
  * the operands the set-up leaves out: for vectors with the same special values in every component, a passing range implies div_ordinary
    of the vector's length and of its normalised components;
  * n * pow2_reciprocal(b) has the bits of n / b for every float n and b in {1, 2, 4, 8, 16}; a block size that is no power of two in range
    has no reciprocal;
  * byte / 255 through the constant reciprocal (unorm8_staged) has the bits of the division for all 256 bytes.
The loops over all floats run on up to 16 threads: a few seconds."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as T

PROGRAM = r"""
#include "vkv_device.hpp"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

using namespace vkv;

static float    f_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool     same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || u_of(a) == u_of(b); }

// [first, last] of all bit patterns, split over the threads
template <typename F>
static uint64_t over_all_floats(F body)
{
	const unsigned          nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
	std::atomic<uint64_t>    bad{0};
	std::vector<std::thread> pool;
	for (unsigned t = 0; t < nt; ++t)
		pool.emplace_back([=, &bad]() {
			const uint64_t lo = (1ull << 32) * t / nt, hi = (1ull << 32) * (t + 1) / nt;
			uint64_t       n = 0;
			for (uint64_t u = lo; u < hi; ++u)
				n += body((uint32_t) u) ? 0 : 1;
			bad += n;
		});
	for (auto &th : pool)
		th.join();
	return bad.load();
}

static std::vector<float> specials()
{
	std::vector<float> s;
	const uint32_t     around[] = {0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, u_of(0x1p-40f), u_of(0x1p-39f), u_of(1.0f), u_of(2.0f),
	                               u_of(0x1p39f), u_of(0x1p40f), 0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0x7fa00000u, 0x7fffffffu};
	for (uint32_t a : around)
		for (int d = -1; d <= 1; ++d)
			for (uint32_t sign : {0u, 0x80000000u})
				s.push_back(f_of(((a + (uint32_t) d) & 0x7fffffffu) | sign));
	return s;
}

static int fail(const char *what, uint64_t n)
{
	printf("FAILED: %s (%llu cases)\n", what, (unsigned long long) n);
	return 1;
}

int main()
{
	// ---- one operand, every float ----
	uint64_t bad = over_all_floats([](uint32_t u) {
		const float x = f_of(u);
		OrdRange    r = {~0u, 0u};
		ord_both(r, x);
		OrdRange l = {~0u, 0u};
		ord_low(l, x);
		const bool both_implies = !ord_ok(r) || div_ordinary(x);
		const bool low_implies  = !(ord_ok(l) && std::fabs(x) < 2.0f) || div_ordinary(x);
		return both_implies && low_implies;
	});
	if (bad)
		return fail("one operand: the accumulated test does not imply div_ordinary", bad);
	{        // the new test is not vacuous: it accepts what a frame's operands look like
		OrdRange r = {~0u, 0u};
		ord_both(r, 1.0f, -0.25f, 1.0e-9f), ord_both(r, 3.0e9f), ord_low(r, -1.0e-7f);
		if (!ord_ok(r))
			return fail("ordinary operands rejected", 1);
	}

	// ---- 28-tuples: 25 operands and the three block sizes behind the host's field ----
	const std::vector<float> sp = specials();
	std::mt19937             rng(0x5e7u);
	auto                     ordinary_random = [&]() {        // magnitudes 2^-38 .. 2^38, either sign
        const uint32_t e = 127u - 38u + rng() % 77u;
        return f_of((rng() & 0x807fffffu) | (e << 23));
	};
	auto tuple_ok = [&](const float *v) {        // as the kernel accumulates it
		OrdRange r = {~0u, 0u};
		for (int i = 0; i < 25; ++i)
			ord_both(r, v[i]);
		r.lo = ord_min(r.lo, (div_ordinary(v[25]) && div_ordinary(v[26]) && div_ordinary(v[27])) ? ~0u : 0u);        // RayMarchArgs.ord_lo0
		return ord_ok(r);
	};
	auto old_ok = [&](const float *v) {
		bool ok = true;
		for (int i = 0; i < 28; ++i)
			ok = ok && div_ordinary(v[i]);
		return ok;
	};
	uint64_t accepted = 0;
	bad               = 0;
	for (int round = 0; round < 20000; ++round)
	{
		float v[28];
		for (float &x : v)
			x = (round & 1) ? ordinary_random() : f_of(rng());
		accepted += tuple_ok(v) ? 1 : 0;
		bad += (tuple_ok(v) && !old_ok(v)) ? 1 : 0;
	}
	for (int pos = 0; pos < 28; ++pos)
		for (float s : sp)
		{
			float v[28];
			for (float &x : v)
				x = ordinary_random();
			v[pos] = s;
			bad += (tuple_ok(v) && !old_ok(v)) ? 1 : 0;
			v[(pos + 7) % 28] = sp[rng() % sp.size()];        // and a second special value somewhere else
			bad += (tuple_ok(v) && !old_ok(v)) ? 1 : 0;
		}
	if (bad)
		return fail("tuples: accepted with an operand that fails div_ordinary", bad);
	if (accepted < 9000)
		return fail("tuples: ordinary tuples rejected", 10000 - accepted);

	// ---- the operands left out: a vector's length, and the upper bound of its normalised components ----
	bad               = 0;
	uint64_t vectors = 0;
	auto     vector_case = [&](float x, float y, float z) {
        const float len = std::sqrt(std::fma(z, z, std::fma(y, y, x * x)));
        const float q[3] = {x / len, y / len, z / len};
        OrdRange    r    = {~0u, 0u};
        ord_both(r, x, y, z);
        ord_low(r, q[0], q[1], q[2]);
        if (!ord_ok(r))
            return;
        ++vectors;
        if (!(div_ordinary(len) && div_ordinary(x) && div_ordinary(y) && div_ordinary(z) && div_ordinary(q[0]) && div_ordinary(q[1]) && div_ordinary(q[2])))
            ++bad;
	};
	for (float x : sp)
		for (float y : sp)
			for (float z : sp)
				vector_case(x, y, z);
	for (int round = 0; round < 200000; ++round)
	{
		float c[3];
		for (float &x : c)
			x = (rng() & 3u) ? ordinary_random() : sp[rng() % sp.size()];
		vector_case(c[0], c[1], c[2]);
	}
	if (bad)
		return fail("a vector passed whose length or normalised component fails div_ordinary", bad);
	if (vectors < 1000)
		return fail("no vector passed", 1);

	// ---- divisions by a power-of-two block size ----
	for (float b : {1.0f, 2.0f, 4.0f, 8.0f, 16.0f})
	{
		const float r = pow2_reciprocal(b);
		if (r == 0.0f || r * b != 1.0f)
			return fail("pow2_reciprocal of a power of two", 1);
		bad = over_all_floats([=](uint32_t u) {
			const float n = f_of(u);
			return same(n * r, n / b);
		});
		if (bad)
			return fail("n * (1 / block) differs from n / block", bad);
	}
	for (float b : {3.0f, 5.0f, 6.0f, 0.0f, -4.0f, 0x1p-41f, 0x1p41f, 0x1p-130f, INFINITY, NAN, 4.0000005f})
		if (pow2_reciprocal(b) != 0.0f)
			return fail("pow2_reciprocal accepts a block size it must not", 1);
	for (int e = -39; e <= 39; ++e)
		if (pow2_reciprocal(std::ldexp(1.0f, e)) != std::ldexp(1.0f, -e))
			return fail("pow2_reciprocal in range", 1);

	// ---- byte / 255 through the constant reciprocal ----
	for (uint32_t i = 0; i < 256; ++i)
		if (u_of(unorm8_staged(i)) != u_of((float) i / 255.0f))
			return fail("unorm8_staged differs from the division", i);

	printf("ok: %llu tuples and %llu vectors accepted\n", (unsigned long long) accepted, (unsigned long long) vectors);
	return 0;
}
"""


def test_range_predicate_and_division_shortcuts_on_the_host(tmp_path):
    hipcc = T.HIPCC if os.path.exists(T.HIPCC) else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    src, exe = tmp_path / "range_check.hip", tmp_path / "range_check"
    src.write_text(PROGRAM)
    # the host pass alone; the library's own floating-point flags (no contraction: fused multiply-adds only where written)
    cmd = [hipcc, "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "--cuda-host-only", "-I", T.CSRC, str(src), "-o", str(exe), "-pthread"]
    r = subprocess.run(cmd, cwd=T.CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:]

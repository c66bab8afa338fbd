// The exact distance family's pass schedule (edt_passes.hpp's EdtSchedule, which vkv_distance_transform_scratch_bytes and the three launchers
// share) on the host alone: for a handful of boxes the target bits and the second buffer must tile a block of exactly 8 entries + 4 n bytes,
// the passes must follow one another through the two buffers and the last one that runs must write the caller's, in all four combinations of
// (y runs, z runs), and a box the family does not take must be rejected with size 0.  Built by tests/test_distance_cpu.py from the header's
// host pass, with AddressSanitizer and UBSan; exits non-zero on the first difference.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "edt_passes.hpp"

using namespace vkv;

static int failures = 0;

static void expect(bool ok, const char *what, const VkvBox &b)
{
	if (ok)
		return;
	++failures;
	std::printf("FAIL %s: box %u x %u x %u at (%u, %u, %u)\n", what, b.width, b.height, b.depth, b.x0, b.y0, b.z0);
}

// edt.hip's edt_scratch_bytes()
static size_t scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	EdtSchedule S;
	return S.lay(e, box, nullptr, nullptr) ? S.bytes() : 0;
}

static void check(const VkvBox &b)
{
	const VkvExtent3D e{b.x0 + b.width, b.y0 + b.height, b.z0 + b.depth};
	const size_t      n = (size_t) b.width * b.height * b.depth, entries = (n + 63) / 64, want = 8 * entries + 4 * n;
	expect(scratch_bytes(e, &b) == want, "the size", b);
	std::vector<uint32_t> block(want / 4), out(n);        // the sanitizer's red zones stand behind them
	EdtSchedule           S;
	expect(S.lay(e, &b, block.data(), out.data()), "lay()", b);
	expect(S.p.n == n && S.p.entries == entries && S.bytes() == want, "the plan", b);
	expect(S.y == (b.height > 1u) && S.z == (b.depth > 1u), "which passes run", b);
	// the layout: [bits][the second buffer], the caller's buffer being the other of cur and nxt
	uint8_t  *base  = reinterpret_cast<uint8_t *>(block.data());
	uint32_t *other = S.cur == out.data() ? S.nxt : S.cur;
	expect((S.cur == out.data()) != (S.nxt == out.data()), "one of the two buffers is the caller's", b);
	expect(reinterpret_cast<uint8_t *>(S.bits) == base, "bits", b);
	expect(reinterpret_cast<uint8_t *>(other) == base + 8 * entries, "the second buffer follows the bits", b);
	expect(reinterpret_cast<uint8_t *>(other + n) == base + want, "the second buffer ends the block", b);
	std::fill(S.bits, S.bits + entries, ~0ull);        // every word of both parts can be written
	std::fill(other, other + n, 7u);
	// the passes: x writes cur, each further pass reads what the one before wrote and writes the other buffer
	const uint32_t *written = S.cur;
	int             passes  = 0;
	const auto      pass    = [&](const uint32_t *src, uint32_t *dst) {
		expect(src == written && dst != src && (dst == out.data() || dst == other), "a pass reads the last output and writes the other buffer", b);
		written = dst;
		++passes;
	};
	S.axes(pass, pass);
	expect(passes == (int) S.y + (int) S.z, "the number of axis passes", b);
	expect(written == out.data() && S.cur == out.data(), "the last pass writes the caller's buffer", b);
}

static void check_rejected(const VkvBox &b)
{
	const VkvExtent3D e{b.x0 + b.width, b.y0 + b.height, b.z0 + b.depth};
	EdtSchedule       S;
	uint32_t          word = 0;
	expect(!S.lay(e, &b, &word, &word) && scratch_bytes(e, &b) == 0, "rejected, size 0", b);
}

int main()
{
	check(VkvBox{0, 0, 0, 9, 1, 1});        // x alone
	check(VkvBox{0, 0, 0, 9, 5, 1});        // x, y
	check(VkvBox{0, 0, 0, 9, 1, 5});        // x, z
	check(VkvBox{0, 0, 0, 9, 5, 5});        // x, y, z
	check(VkvBox{0, 0, 0, 64, 1, 1});       // exactly one entry
	check(VkvBox{0, 0, 0, 65, 1, 1});       // one voxel more: two entries, 4 n not a multiple of 8
	check(VkvBox{3, 2, 1, 9, 5, 5});        // inside a larger volume
	check_rejected(VkvBox{0, 0, 0, 32769, 1, 1});
	check_rejected(VkvBox{0, 0, 0, 1, 32769, 1});
	check_rejected(VkvBox{0, 0, 0, 1, 1, 32769});
	check_rejected(VkvBox{0, 0, 0, 32768, 32768, 4});        // 2^32 voxels
	check_rejected(VkvBox{0, 0, 0, 9, 0, 5});                // an empty box
	const VkvBox all{0, 0, 0, 32768, 32768, 1};              // 2^30 voxels, accepted: only the size is asked for
	expect(scratch_bytes(VkvExtent3D{32768, 32768, 1}, nullptr) == 8 * ((size_t) 1 << 24) + 4 * ((size_t) 1 << 30), "the whole volume, null box", all);
	std::printf(failures ? "%d failures\n" : "edt schedule ok\n", failures);
	return failures ? 1 : 0;
}

// The mesh extractors' scratch layout (mesh_common.hpp's MeshScratch) against the sizes the C ABI promises, on the host alone: for a handful
// of plans bytes() must equal the stated formula, and sums / counts / local / behind must tile the block in order without a gap or an overlap.
// Built by tests/test_mesh_cpu.py from the header's host pass, with AddressSanitizer and UBSan; exits non-zero on the first difference.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "mesh_common.hpp"

using namespace vkv;

static int failures = 0;

static void expect(bool ok, const char *what, const VkvBox &b, uint32_t lists, size_t extra)
{
	if (ok)
		return;
	++failures;
	std::printf("FAIL %s: box %u x %u x %u, %u lists, %zu extra bytes\n", what, b.width, b.height, b.depth, lists, extra);
}

static void check(const VkvBox &b, bool voxels, uint32_t lists, size_t extra, uint32_t want_entries, uint32_t want_chunks)
{
	const VkvExtent3D e{b.x0 + b.width, b.y0 + b.height, b.z0 + b.depth};
	MeshPlan          p;
	expect(mesh_plan(e, b, p, voxels), "mesh_plan", b, lists, extra);
	expect(p.entries == want_entries && p.chunks == want_chunks, "entries and chunks", b, lists, extra);
	const size_t lists_bytes = (size_t) lists * (8 * (size_t) p.chunks + 8 * (size_t) p.entries);        // 8 and 16 bytes per chunk and entry
	const size_t want        = std::max<size_t>(16, (lists_bytes + extra + 7) & ~(size_t) 7);
	std::vector<uint64_t> block(want / 8);        // the sanitizer's red zones stand behind it
	const MeshScratch     S{p, lists, extra, block.data()};
	expect(S.bytes() == want, "bytes()", b, lists, extra);
	uint8_t *at = reinterpret_cast<uint8_t *>(block.data());
	for (uint32_t l = 0; l < lists; ++l, at += 8 * (size_t) p.chunks)
		expect(reinterpret_cast<uint8_t *>(S.sums(l)) == at, "sums()", b, lists, extra);
	for (uint32_t l = 0; l < lists; ++l, at += 8 * (size_t) p.entries)
		expect(reinterpret_cast<uint8_t *>(S.counts(l)) == at && reinterpret_cast<uint8_t *>(S.local(l)) == at + 4 * (size_t) p.entries, "counts() and local()", b,
		       lists, extra);
	expect(S.behind() == at && at + extra <= reinterpret_cast<uint8_t *>(block.data()) + want, "behind()", b, lists, extra);
	// every word of every part can be written
	for (uint32_t l = 0; l < lists; ++l)
	{
		std::fill(S.sums(l), S.sums(l) + p.chunks, 1ull);
		std::fill(S.counts(l), S.counts(l) + p.entries, 2u);
		std::fill(S.local(l), S.local(l) + p.entries, 3u);
	}
	std::fill(S.behind(), S.behind() + extra, (uint8_t) 4);
}

int main()
{
	for (uint32_t lists = 1; lists <= 2; ++lists)
		for (size_t extra : {(size_t) 0, (size_t) 5, (size_t) 4096})
		{
			check(VkvBox{0, 0, 0, 1, 5, 5}, false, lists, extra, 0, 0);              // no cube
			check(VkvBox{0, 0, 0, 1, 5, 5}, true, lists, extra, 0, 0);               // a box of width 1, dealt over voxels: still none
			check(VkvBox{3, 2, 1, 2, 2, 2}, false, lists, extra, 1, 1);              // one entry
			check(VkvBox{0, 0, 0, 257, 65, 65}, false, lists, extra, 4096, 1);       // exactly one chunk
			check(VkvBox{0, 0, 0, 2, 18, 242}, false, lists, extra, 4097, 2);        // one entry more
			check(VkvBox{0, 0, 0, 258, 2, 2}, true, lists, extra, 2 * 2 * 2, 1);     // voxels: 258 of them in two x segments, two rows, two slices
		}
	std::printf(failures ? "%d failures\n" : "mesh scratch layout ok\n", failures);
	return failures ? 1 : 0;
}

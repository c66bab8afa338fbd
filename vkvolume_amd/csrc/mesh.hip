// mesh.hip — the isosurface of the uint8 volume as a triangle list (vkv_isosurface_mesh): marching tetrahedra on the Kuhn
// decomposition of every cube, in a defined order, with an exact total and a prefix under a capacity.  Byte streaming; no MFMA.
//
// Three steps, four launches, no atomics:
//   k_mesh_count   a lane owns four x-adjacent cubes of one row and marches along z; a wave is 256 cubes of one row, a workgroup four rows
//                  and kMeshSegment slices.  Per slice a lane loads the dword of its voxels in its two rows, takes voxel x + 4 from the lane
//                  above, turns the ten voxels into inside bits and keeps them for the two cubes that see the slice.  A cube's 8-bit corner
//                  mask indexes the 256 triangle counts of mtet_table.hpp (in LDS); the wave's sum goes to the ENTRY of its 256 cubes: the
//                  entries lie in the output's order (x segment fastest, then row, then slice), which a three-dimensional tile does not.
//                  With a max map a workgroup whose cells all stay below iso writes zeros without reading a voxel.
//   k_mesh_scan_*  exclusive scan of the entries: each chunk of 4096 on its own (uint32), then the chunk sums by one workgroup (uint64),
//                  which also writes d_counts.  Both are fixed trees: the result does not depend on scheduling.
//   k_mesh_emit    a wave whose entries are all zero, or all start at or past the capacity, leaves at once; for every other entry it loads
//                  the two slices again, prefixes its lanes' counts and stores the triangles whose index is below the capacity (the case table in LDS).
// No kernel uses scratch memory (tests/test_mesh_cpu.py reads the listing).  The row loads, inside bits, corner mask, tile geometry, the
// vertex rule, the plan and the scratch layout live in mesh_common.hpp, and so does every step that the other three mesh extractors take as
// well: the empty tile's zero fill, the case table's staging, the wave's entries and their starts, the triangle store.  The scans' bodies are
// fixed_scan.hpp's.
#include "launchers.hpp"
#include "mesh_common.hpp"
#include "mtet_table.hpp"

using namespace vkv;

__constant__ MtetTable d_mtet = kMtetTable;

template <bool WIDE>
__global__ void __launch_bounds__(256) k_mesh_count(MeshGeom G, uint32_t *__restrict__ counts)
{
	__shared__ uint8_t lut[256];
	const MeshTile     T    = mesh_tile(G, G.ny, G.nz);
	const uint32_t     lane = threadIdx.x & 63u;
	if (G.mm.map && tile_is_empty(G, T, G.nx, G.ny))
	{
		zero_tile_counts(G, T, counts);
		return;
	}
	lut[threadIdx.x] = d_mtet.count[threadIdx.x];
	__syncthreads();
	if (T.yc >= G.ny)        // whole waves only: the lanes exchange voxels below
		return;
	const int    x = G.x0 + T.xc, nvalid = min(max(G.nx - T.xc, 0), 4);
	const size_t plane = (size_t) G.H * (size_t) G.W, row = (size_t) (G.y0 + T.yc) * (size_t) G.W;
	struct Rows
	{
		Row5 a, b;
	};
	auto load = [&](int zc) {
		const uint8_t *base = G.vol + (size_t) (G.z0 + zc) * plane + row;
		return Rows{row5<WIDE>(base, x, G.W, lane), row5<WIDE>(base + G.W, x, G.W, lane)};
	};
	auto bits = [&](const Rows &r) { return inside5(r.a, G.thr) | inside5(r.b, G.thr) << 8; };
	Rows     next = load(T.zc0 + 1);
	uint32_t q0   = bits(load(T.zc0)), e = T.e0;
	for (int zc = T.zc0; zc < T.zc1; ++zc, e += T.e_step)
	{
		const uint32_t q1 = bits(next);
		if (zc + 1 < T.zc1)        // wave-uniform; slice zc + 2 <= nz is a slice of the box
			next = load(zc + 2);
		uint32_t n = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			n += i < nvalid ? (uint32_t) lut[corner_mask(q0, q1, i)] : 0u;
		n = wave_sum(n);
		if (lane == 0)
			counts[e] = n;
		q0 = q1;
	}
}

__global__ void __launch_bounds__(256) k_mesh_scan_chunks(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                          uint32_t n_entries)
{
	scan_chunk(counts, local, sums, n_entries);
}

__global__ void __launch_bounds__(256) k_mesh_scan_total(uint64_t *__restrict__ sums, uint32_t n_chunks, uint64_t capacity, uint64_t *__restrict__ d_counts)
{
	scan_total(sums, n_chunks, capacity, d_counts);
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_mesh_emit(MeshGeom G, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                   const uint64_t *__restrict__ chunk_before, float iso, float *__restrict__ triangles, uint64_t capacity)
{
	__shared__ MtetTable tab;
	stage_mtet(tab, d_mtet);
	const MeshTile T    = mesh_tile(G, G.ny, G.nz);
	const uint32_t lane = threadIdx.x & 63u;
	if (T.yc >= G.ny)        // whole waves only; there is no barrier below
		return;
	// the wave's entries, one per lane: those with triangles that start below the capacity
	uint64_t start;
	uint64_t todo = wave_entries(T, lane, T.zc1, counts, local, chunk_before, capacity, start);
	if (todo == 0)
		return;
	const int    x = G.x0 + T.xc, y = G.y0 + T.yc, nvalid = min(max(G.nx - T.xc, 0), 4);
	const size_t plane = (size_t) G.H * (size_t) G.W, row = (size_t) y * (size_t) G.W;
	while (todo)        // wave-uniform
	{
		const int k = __ffsll((long long) todo) - 1;
		todo &= todo - 1;
		const int      zc = T.zc0 + k;
		const uint64_t at = entry_start(start, k);
		const uint8_t *base = G.vol + (size_t) (G.z0 + zc) * plane + row;
		const Row5     r[4] = {row5<WIDE>(base, x, G.W, lane), row5<WIDE>(base + G.W, x, G.W, lane), row5<WIDE>(base + plane, x, G.W, lane),
		                       row5<WIDE>(base + plane + G.W, x, G.W, lane)};
		const uint32_t q0 = inside5(r[0], G.thr) | inside5(r[1], G.thr) << 8, q1 = inside5(r[2], G.thr) | inside5(r[3], G.thr) << 8;
		CubeBytes      B;
#pragma unroll
		for (int j = 0; j < 4; ++j)
			B.v[j] = (uint64_t) r[j].d | (uint64_t) r[j].e << 32;
		uint32_t mine = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			mine += i < nvalid ? (uint32_t) tab.count[corner_mask(q0, q1, i)] : 0u;
		uint64_t idx = at + wave_exclusive(mine, lane);        // the cubes of a row lie in lane order
		if (mine == 0)
			continue;
#pragma unroll 1
		for (int i = 0; i < nvalid; ++i)
		{
			const uint32_t cm = corner_mask(q0, q1, i);
			if (tab.count[cm] == 0)
				continue;
#pragma unroll 1
			for (int t = 0; t < 6; ++t)
			{
				const uint32_t  p = (kMtetMid1 >> (4 * t)) & 7u, q = (kMtetMid2 >> (4 * t)) & 7u;
				const uint32_t  m = (cm & 1u) | ((cm >> p) & 1u) << 1 | ((cm >> q) & 1u) << 2 | (cm >> 7) << 3;
				const uint64_t  c = *reinterpret_cast<const uint64_t *>(&tab.c[t][m]);        // n, swap, e[0 .. 5]
				const int       n = (int) (c & 0xffu);
				for (int tri = 0; tri < n; ++tri, ++idx)
				{
					if (idx >= capacity)
						continue;
					float v[9];
#pragma unroll
					for (int j = 0; j < 3; ++j)
						edge_vertex(B, i, (uint32_t) (c >> (16 + 24 * tri + 8 * j)) & 0x3fu, x + i, y, G.z0 + zc, iso, v + 3 * j);
					store_triangle(triangles + 9 * idx, v);
				}
			}
		}
	}
}

namespace vkv
{

// MeshScratch with one list; 0: the extent and box are not accepted
size_t mesh_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	if (!extent_and_box_ok(e, box) || !mesh_plan(e, whole_or(e, box), p))
		return 0;
	return MeshScratch{p, 1, 0, nullptr}.bytes();
}

bool mesh_launch_ok(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	return mesh_plan(e, whole_or(e, box), p);
}

int launch_isosurface_mesh(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint8_t *d_max_map, VkvExtent3D me,
                           void *d_scratch, float *d_triangles, uint64_t capacity, uint64_t *d_counts, hipStream_t s)
{
	MeshPlan p;
	if (!mesh_plan(e, b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "isosurface_mesh: volume too large for the launches");
	const MeshScratch S{p, 1, 0, d_scratch};
	const MeshGeom    G = mesh_geom(d_vol, e, b, iso, d_max_map, me, p);
	const bool wide = e.width >= 4;        // the kernels' dword row loads
	if (p.entries)
	{
		dispatch_wide(wide, [&](auto w) { hipLaunchKernelGGL(k_mesh_count<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, G, S.counts(0)); });
		hipLaunchKernelGGL(k_mesh_scan_chunks, dim3(p.chunks), dim3(256), 0, s, S.counts(0), S.local(0), S.sums(0), p.entries);
	}
	hipLaunchKernelGGL(k_mesh_scan_total, dim3(1), dim3(256), 0, s, S.sums(0), p.chunks, capacity, d_counts);
	if (p.entries && capacity)
		dispatch_wide(wide, [&](auto w) {
			hipLaunchKernelGGL(k_mesh_emit<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, G, S.counts(0), S.local(0), S.sums(0), iso, d_triangles, capacity);
		});
	return check_launch(ctx, "isosurface_mesh");
}

}        // namespace vkv
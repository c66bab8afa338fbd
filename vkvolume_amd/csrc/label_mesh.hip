// label_mesh.hip — the surfaces of the visible bodies of a uint32 label array as a triangle list with one label per triangle (vkv_label_mesh,
// DESIGN.md §5.22): marching tetrahedra on the Kuhn decomposition of every cube, each tetrahedron cut once per visible label it touches, in a
// defined order, with an exact total and a prefix under a capacity.  Dword streaming; no MFMA.
//
// The steps are mesh.hip's: the tile geometry, the plan, the scratch layout, the empty tile's zero fill, the case table's staging, the wave's
// entries and the triangle store are mesh_common.hpp's, stated there once for the four extractors; what label_mesh_indexed.hip shares with
// this file alone is label_mesh_common.hpp's:
//   k_lmesh_count  a lane owns four x-adjacent cubes of one row and marches along z; a wave is 256 cubes of one row, a workgroup four rows and
//                  kMeshSegment slices.  Per slice a lane loads its four labels of its two rows as one 16-byte load each, takes label x + 4
//                  from the lane above and keeps the previous slice's two rows in registers.  Twenty equal labels end the lane's slice; a cube
//                  of eight equal labels gives nothing; otherwise the table is looked up once per distinct label of the cube (a hidden label
//                  becomes 0: it starts no group and is outside for every group), a cube with ONE visible label takes the isosurface's corner
//                  mask and its 256 triangle counts, and only the rest walks its six tetrahedra.  The wave's sum goes to the entry of its 256
//                  cubes.  With a visibility map a workgroup whose cells all hold 0 writes zeros without reading a label.
//   k_lmesh_scan_* fixed_scan.hpp's two scans; the second writes d_counts.
//   k_lmesh_emit   a wave whose entries are all zero, or all start at or past the capacity, leaves at once; for every other entry it loads the
//                  two slices again, prefixes its lanes' counts and walks cube, tetrahedron, group (only the local vertices that start one:
//                  trying all four cost 2.2 x the whole call) and triangle, storing the triangles and
//                  labels whose index is below the capacity.  The byte volume is read here only, by the waves and in the slices that emit:
//                  a dword per lane and row, asked for together with the labels.
// No kernel uses scratch memory or atomics (tests/test_label_mesh_cpu.py reads the listing).
#include "label_mesh_common.hpp"
#include "launchers.hpp"

using namespace vkv;

__constant__ MtetTable d_lmtet = kMtetTable;

template <bool WIDE>
__global__ void __launch_bounds__(256) k_lmesh_count(LabelGeom A, uint32_t *__restrict__ counts)
{
	__shared__ uint8_t lut[256];
	const MeshGeom &   G    = A.G;
	const MeshTile     T    = mesh_tile(G, G.ny, G.nz);
	const uint32_t     lane = threadIdx.x & 63u;
	if (G.mm.map && tile_is_empty(G, T, G.nx, G.ny))
	{
		zero_tile_counts(G, T, counts);
		return;
	}
	lut[threadIdx.x] = d_lmtet.count[threadIdx.x];
	__syncthreads();
	if (T.yc >= G.ny)        // whole waves only: the lanes exchange labels below
		return;
	const int    nvalid = min(max(G.nx - T.xc, 0), 4);
	const size_t plane = (size_t) A.bh * (size_t) A.bw, row = (size_t) T.yc * (size_t) A.bw;
	auto         load  = [&](int zc, Lab5 &a, Lab5 &b) {
        const uint32_t *base = A.labels + (size_t) zc * plane + row;
        a = lab5<WIDE>(base, T.xc, A.bw, lane), b = lab5<WIDE>(base + A.bw, T.xc, A.bw, lane);
	};
	CubeRows R;
	Lab5     na, nb;
	load(T.zc0, R.r[0], R.r[1]);
	load(T.zc0 + 1, na, nb);
	uint32_t e = T.e0;
	for (int zc = T.zc0; zc < T.zc1; ++zc, e += T.e_step)
	{
		R.r[2] = na, R.r[3] = nb;
		if (zc + 1 < T.zc1)        // wave-uniform; slice zc + 2 <= nz is a slice of the box
			load(zc + 2, na, nb);
		const uint32_t n = wave_sum(lane_count(A, lut, R, nvalid));
		if (lane == 0)
			counts[e] = n;
		R.r[0] = R.r[2], R.r[1] = R.r[3];
	}
}

__global__ void __launch_bounds__(256) k_lmesh_scan_chunks(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                           uint32_t n_entries)
{
	scan_chunk(counts, local, sums, n_entries);
}

__global__ void __launch_bounds__(256) k_lmesh_scan_total(uint64_t *__restrict__ sums, uint32_t n_chunks, uint64_t capacity, uint64_t *__restrict__ d_counts)
{
	scan_total(sums, n_chunks, capacity, d_counts);
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_lmesh_emit(LabelGeom A, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                    const uint64_t *__restrict__ chunk_before, float iso, float *__restrict__ triangles,
                                                    uint32_t *__restrict__ triangle_labels, uint64_t capacity)
{
	__shared__ MtetTable tab;
	stage_mtet(tab, d_lmtet);
	const MeshGeom &G    = A.G;
	const MeshTile  T    = mesh_tile(G, G.ny, G.nz);
	const uint32_t  lane = threadIdx.x & 63u;
	if (T.yc >= G.ny)        // whole waves only; there is no barrier below
		return;
	// the wave's entries, one per lane: those with triangles that start below the capacity
	uint64_t start;
	uint64_t todo = wave_entries(T, lane, T.zc1, counts, local, chunk_before, capacity, start);
	if (todo == 0)
		return;
	const int    nvalid = min(max(G.nx - T.xc, 0), 4);
	const size_t plane = (size_t) A.bh * (size_t) A.bw, row = (size_t) T.yc * (size_t) A.bw;
	while (todo)        // wave-uniform
	{
		const int k = __ffsll((long long) todo) - 1;
		todo &= todo - 1;
		const int       zc = T.zc0 + k;
		const uint64_t  at = entry_start(start, k);
		const uint32_t *base = A.labels + (size_t) zc * plane + row;
		CubeRows        R;
		R.r[0] = lab5<WIDE>(base, T.xc, A.bw, lane), R.r[1] = lab5<WIDE>(base + A.bw, T.xc, A.bw, lane);
		R.r[2] = lab5<WIDE>(base + plane, T.xc, A.bw, lane), R.r[3] = lab5<WIDE>(base + plane + A.bw, T.xc, A.bw, lane);
		// the bytes around the lane's cubes, asked for together with the labels: a second round trip after the counts costs more than the bytes
		CubeBytes B{};
		if (G.vol)        // wave-uniform
		{
			const size_t   vplane = (size_t) G.H * (size_t) G.W;
			const uint8_t *vrow   = G.vol + (size_t) (G.z0 + zc) * vplane + (size_t) (G.y0 + T.yc) * (size_t) G.W;
			const int      vx     = G.x0 + T.xc;
			B.v[0] = bytes5(vrow, vx, G.W, lane), B.v[1] = bytes5(vrow + G.W, vx, G.W, lane);
			B.v[2] = bytes5(vrow + vplane, vx, G.W, lane), B.v[3] = bytes5(vrow + vplane + G.W, vx, G.W, lane);
		}
		const uint32_t mine = lane_count(A, tab.count, R, nvalid);
		uint64_t       idx  = at + wave_exclusive(mine, lane);        // the cubes of a row lie in lane order
		if (mine == 0)
			continue;
#pragma unroll 1
		for (int i = 0; i < nvalid; ++i)
		{
			uint32_t c[8], dif = 0;        // cube_labels() and, below, cube_bytes() spelt out: through the calls "label full" measured 0.1 - 0.2 % slower
#pragma unroll
			for (int j = 0; j < 8; ++j)
			{
				const Lab5 &r = R.r[j >> 1];
				c[j]          = (j & 1) ? sel4(r.v[1], r.v[2], r.v[3], r.v[4], i) : sel4(r.v[0], r.v[1], r.v[2], r.v[3], i);
				dif |= c[j] ^ c[0];
			}
			if (dif == 0u)
				continue;
			uint32_t E[8];
			shown8(A, c, E);
			const int cx = G.x0 + T.xc + i, cy = G.y0 + T.yc, cz = G.z0 + zc;
			uint64_t  cb = 0;        // the cube's bytes, corner j in byte j: bytes i and i + 1 of row j >> 1
#pragma unroll
			for (int r = 0; r < 4; ++r)
				cb |= ((B.v[r] >> (8 * i)) & 0xffffull) << (16 * r);
#pragma unroll 1
			for (int t = 0; t < 6; ++t)
			{
				const uint32_t p = (kMtetMid1 >> (4 * t)) & 7u, q = (kMtetMid2 >> (4 * t)) & 7u;
				const uint32_t l0 = E[0], l1 = p == 1u ? E[1] : p == 2u ? E[2] : E[4], l2 = q == 3u ? E[3] : q == 5u ? E[5] : E[6], l3 = E[7];
				// the local vertices that start a group: a visible label that no lower vertex carries.  (label_mesh_indexed.hip walks the groups
				// by the same lines.  As one function template that takes the triangle's work it cost this kernel 4 VGPRs and 8 bytes of code)
				uint32_t starts = (l0 != 0u ? 1u : 0u) | (l1 != 0u && l1 != l0 ? 2u : 0u) | (l2 != 0u && l2 != l0 && l2 != l1 ? 4u : 0u) |
				                  (l3 != 0u && l3 != l0 && l3 != l1 && l3 != l2 ? 8u : 0u);
				while (starts)
				{
					const int g = __ffs((int) starts) - 1;
					starts &= starts - 1u;
					const uint32_t L  = sel4(l0, l1, l2, l3, g);
					const uint32_t m  = (l0 == L ? 1u : 0u) | (l1 == L ? 2u : 0u) | (l2 == L ? 4u : 0u) | (l3 == L ? 8u : 0u);
					const uint64_t cs = *reinterpret_cast<const uint64_t *>(&tab.c[t][m]);        // n, swap, e[0 .. 5]
					const int      n  = (int) (cs & 0xffu);
					for (int tri = 0; tri < n; ++tri, ++idx)
					{
						if (idx >= capacity)
							continue;
						float v[9];
#pragma unroll
						for (int j = 0; j < 3; ++j)
							label_edge_vertex(G.vol != nullptr, cb, (uint32_t) (cs >> (16 + 24 * tri + 8 * j)) & 0x3fu, cx, cy, cz, iso, v + 3 * j);
						store_triangle(triangles + 9 * idx, v);
						triangle_labels[idx]                   = L;
					}
				}
			}
		}
	}
}

namespace vkv
{

// the box's cubes dealt as mesh.hip deals them; false: not accepted, more than 2^32 - 1 voxels, or too large for the launches
static bool label_mesh_plan(VkvExtent3D e, const VkvBox *box, MeshPlan &p)
{
	return extent_and_box_ok(e, box) && components_launch_ok(e, box) && mesh_plan(e, whole_or(e, box), p);
}

// MeshScratch with one list; 0: the extent and box are not accepted
size_t label_mesh_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	if (!label_mesh_plan(e, box, p))
		return 0;
	return MeshScratch{p, 1, 0, nullptr}.bytes();
}

bool label_mesh_launch_ok(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	return label_mesh_plan(e, box, p);
}

int launch_label_mesh(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D e, const VkvBox &b, const uint32_t *d_colors, uint64_t table_entries,
                      const uint8_t *d_vol, float iso, const uint8_t *d_visibility_map, VkvExtent3D me, void *d_scratch, float *d_triangles,
                      uint32_t *d_triangle_labels, uint64_t capacity, uint64_t *d_counts, hipStream_t s)
{
	MeshPlan p;
	if (!mesh_plan(e, b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "label_mesh: volume too large for the launches");
	const MeshScratch S{p, 1, 0, d_scratch};
	const LabelGeom   A = label_geom(d_labels, e, b, d_colors, table_entries, d_vol, d_visibility_map, me, p);
	const bool wide = b.width >= 4;        // the kernels' 16-byte row loads
	if (p.entries)
	{
		dispatch_wide(wide, [&](auto w) { hipLaunchKernelGGL(k_lmesh_count<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, A, S.counts(0)); });
		hipLaunchKernelGGL(k_lmesh_scan_chunks, dim3(p.chunks), dim3(256), 0, s, S.counts(0), S.local(0), S.sums(0), p.entries);
	}
	hipLaunchKernelGGL(k_lmesh_scan_total, dim3(1), dim3(256), 0, s, S.sums(0), p.chunks, capacity, d_counts);
	if (p.entries && capacity)
		dispatch_wide(wide, [&](auto w) {
			hipLaunchKernelGGL(k_lmesh_emit<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, A, S.counts(0), S.local(0), S.sums(0), iso, d_triangles,
			                   d_triangle_labels, capacity);
		});
	return check_launch(ctx, "label_mesh");
}

}        // namespace vkv

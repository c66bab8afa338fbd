// mesh_indexed.hip — the isosurface of the uint8 volume as an indexed mesh (vkv_isosurface_mesh_indexed): the triangles of
// vkv_isosurface_mesh in their order as three vertex numbers each, one vertex per crossing tetrahedron edge, optionally with its gradient
// normal.  Byte streaming; no MFMA.
//
// Every tetrahedron edge of a cube runs from a corner a to a corner b with a & b == a, so it has one OWNER: the voxel at a and the direction
// d = a ^ b (1 .. 7).  The vertex list is the crossing edges by owner voxel, then d: numbering them takes the count / scan / emit of mesh.hip
// run over voxels, no hash, no sort, no atomics.  Tiles and entries are dealt over the box's VOXELS (one more per axis than its cubes: the
// far faces own the edges that lie in them); the entry of 256 x-adjacent voxels carries two counts, the triangles of the cubes that start
// there (zero on the far faces) and the crossing edges they own.  Both lists lie in entry order.
//   k_meshi_count          mesh.hip's count kernel with a second sum: a voxel's crossing mask is its cube's corner mask shifted down, flipped
//                          where the voxel is inside, and cut to the directions that stay in the box; its vertices are a popcount.
//   k_meshi_scan_*         the fixed-tree scans of fixed_scan.hpp, both lists in one launch each (blockIdx.y / blockIdx.x picks the list).
//   k_meshi_emit_vertices  per entry with vertices below the capacity: the four rows again, the lanes' counts prefixed, then position and
//                          (on request) normal of every crossing edge: twelve clamped byte gathers, for crossing edges only.
//   k_meshi_emit_indices   per entry with triangles below the capacity: a triangle of cube o names owners in the rows (y, y + 1) x (z, z + 1)
//                          at x and x + 1, and an owner's number is its entry's start + the crossing edges of the entry's earlier voxels + the
//                          rank of d in its mask.  The wave therefore loads the 3 x 3 rows (y .. y + 2) x (z .. z + 2), forms the four owner
//                          rows' masks and prefixes each over its lanes: nothing per voxel or lane group is kept in scratch, which stays at
//                          16 bytes per entry.  The owner at x + 4 is the lane above's first voxel (its mask and number come by wave_shl);
//                          for the last lane it is the first voxel of the NEXT entry of the row, whose vertices begin where this entry's
//                          end: the last lane's own number plus its own count; that voxel's mask takes one more byte per row.
// No kernel uses scratch memory (tests/test_mesh_indexed_cpu.py reads the listing).  mesh_common.hpp holds what label_mesh_indexed.hip takes
// as well: box_dirs(), central_differences(), store_normal(), and the emit kernels' opening (stage_mtet, wave_entries, entry_start).
#include "launchers.hpp"
#include "mesh_common.hpp"
#include "mtet_table.hpp"

using namespace vkv;

__constant__ MtetTable d_mtet_indexed = kMtetTable;

// bit d - 1 = the edge from a voxel in direction d crosses: corner d of its cube is inside and the voxel is not, or the reverse
__device__ __forceinline__ uint32_t crossing_mask(uint32_t cm) { return (cm >> 1) ^ ((cm & 1u) ? 0x7fu : 0u); }

// the crossing masks of the lane's four voxels xv .. xv + 3 of row (yv, zv), one per byte, from the inside bits of corner_mask()
__device__ __forceinline__ uint32_t owner_masks(const MeshGeom &G, uint32_t q0, uint32_t q1, int xv, int yv, int zv)
{
	uint32_t m = 0;
#pragma unroll
	for (int i = 0; i < 4; ++i)
		m |= (crossing_mask(corner_mask(q0, q1, i)) & box_dirs(G, xv + i, yv, zv)) << (8 * i);
	return m;
}

// One pass, both counts: tri_counts[e] = the triangles of the cubes that start at entry e's voxels, vert_counts[e] = the crossing edges they own.
template <bool WIDE>
__global__ void __launch_bounds__(256) k_meshi_count(MeshGeom G, uint32_t *__restrict__ tri_counts, uint32_t *__restrict__ vert_counts)
{
	__shared__ uint8_t lut[256];
	const int          vy = G.ny + 1, vz = G.nz + 1;
	const MeshTile     T    = mesh_tile(G, vy, vz);
	const uint32_t     lane = threadIdx.x & 63u;
	if (G.mm.map && tile_is_empty(G, T, G.nx + 1, vy))        // a cell below iso: its voxels and their neighbours are outside, no edge from them crosses
	{
		if (threadIdx.x < 4 * kMeshSegment)
		{
			const int yv = T.yc - (int) (threadIdx.x >> 6) + (int) (threadIdx.x & 3u), zv = T.zc0 + (int) (threadIdx.x >> 2);
			if (yv < vy && zv < T.zc1)
			{
				const uint32_t e = ((uint32_t) zv * (uint32_t) vy + (uint32_t) yv) * G.segs_x + T.xs;
				tri_counts[e] = 0u, vert_counts[e] = 0u;
			}
		}
		return;
	}
	lut[threadIdx.x] = d_mtet_indexed.count[threadIdx.x];
	__syncthreads();
	if (T.yc >= vy)        // whole waves only: the lanes exchange voxels below
		return;
	const int    x = G.x0 + T.xc, ncubes = T.yc < G.ny ? min(max(G.nx - T.xc, 0), 4) : 0;
	const size_t plane = (size_t) G.H * (size_t) G.W, row = (size_t) (G.y0 + T.yc) * (size_t) G.W;
	const size_t up = T.yc < G.ny ? (size_t) G.W : 0;        // the far face's rows stand in for the row past them: those directions are cut
	struct Rows
	{
		Row5 a, b;
	};
	auto load = [&](int zv) {
		const uint8_t *base = G.vol + (size_t) (G.z0 + min(zv, G.nz)) * plane + row;
		return Rows{row5<WIDE>(base, x, G.W, lane), row5<WIDE>(base + up, x, G.W, lane)};
	};
	auto bits = [&](const Rows &r) { return inside5(r.a, G.thr) | inside5(r.b, G.thr) << 8; };
	Rows     next = load(T.zc0 + 1);
	uint32_t q0   = bits(load(T.zc0)), e = T.e0;
	for (int zv = T.zc0; zv < T.zc1; ++zv, e += T.e_step)
	{
		const uint32_t q1 = bits(next);
		if (zv + 1 < T.zc1)        // wave-uniform
			next = load(zv + 2);
		uint32_t n = __builtin_popcount(owner_masks(G, q0, q1, T.xc, T.yc, zv)) << 16;        // at most 7 x 256 vertices, 12 x 256 triangles
		if (zv < G.nz)
		{
#pragma unroll
			for (int i = 0; i < 4; ++i)
				n += i < ncubes ? (uint32_t) lut[corner_mask(q0, q1, i)] : 0u;
		}
		n = wave_sum(n);
		if (lane == 0)
			tri_counts[e] = n & 0xffffu, vert_counts[e] = n >> 16;
		q0 = q1;
	}
}

// both lists' entries lie one behind the other: [counts, local] x 2 and [sums] x 2; blockIdx.y = the list
__global__ void __launch_bounds__(256) k_meshi_scan_chunks(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                           uint32_t n_entries, uint32_t n_chunks)
{
	const size_t list = blockIdx.y;
	scan_chunk(counts + 2 * list * n_entries, local + 2 * list * n_entries, sums + list * n_chunks, n_entries);
}

// workgroup 0: the triangles into d_counts[0, 1]; workgroup 1: the vertices into d_counts[2, 3]
__global__ void __launch_bounds__(256) k_meshi_scan_total(uint64_t *__restrict__ sums, uint32_t n_chunks, uint64_t capacity_triangles,
                                                          uint64_t capacity_vertices, uint64_t *__restrict__ d_counts)
{
	const size_t list = blockIdx.x;
	scan_total(sums + list * n_chunks, n_chunks, list ? capacity_vertices : capacity_triangles, d_counts + 2 * list);
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_meshi_emit_vertices(MeshGeom G, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                             const uint64_t *__restrict__ chunk_before, float iso, float *__restrict__ vertices,
                                                             float *__restrict__ normals, uint64_t capacity)
{
	const int      vy = G.ny + 1, vz = G.nz + 1;
	const MeshTile T    = mesh_tile(G, vy, vz);
	const uint32_t lane = threadIdx.x & 63u;
	if (T.yc >= vy)        // whole waves only; there is no barrier
		return;
	// the wave's entries, one per lane: those with vertices that start below the capacity
	uint64_t start;
	uint64_t todo = wave_entries(T, lane, T.zc1, counts, local, chunk_before, capacity, start);
	if (todo == 0)
		return;
	const int    x = G.x0 + T.xc, y = G.y0 + T.yc;
	const size_t plane = (size_t) G.H * (size_t) G.W, row = (size_t) y * (size_t) G.W;
	const size_t up = T.yc < G.ny ? (size_t) G.W : 0;
	while (todo)        // wave-uniform
	{
		const int k = __ffsll((long long) todo) - 1;
		todo &= todo - 1;
		const int      zv = T.zc0 + k, z = G.z0 + zv;
		const uint64_t at = entry_start(start, k);
		const uint8_t *base = G.vol + (size_t) z * plane + row;
		const size_t   back = zv < G.nz ? plane : 0;
		const Row5     r[4] = {row5<WIDE>(base, x, G.W, lane), row5<WIDE>(base + up, x, G.W, lane), row5<WIDE>(base + back, x, G.W, lane),
		                       row5<WIDE>(base + back + up, x, G.W, lane)};
		const uint32_t q0 = inside5(r[0], G.thr) | inside5(r[1], G.thr) << 8, q1 = inside5(r[2], G.thr) | inside5(r[3], G.thr) << 8;
		CubeBytes      B;
#pragma unroll
		for (int j = 0; j < 4; ++j)
			B.v[j] = (uint64_t) r[j].d | (uint64_t) r[j].e << 32;
		const uint32_t masks = owner_masks(G, q0, q1, T.xc, T.yc, zv), mine = __builtin_popcount(masks);
		uint64_t       idx   = at + wave_exclusive(mine, lane);
		if (mine == 0)
			continue;
#pragma unroll 1
		for (int i = 0; i < 4; ++i)
		{
			uint32_t m = (masks >> (8 * i)) & 0x7fu;
			for (; m; m &= m - 1, ++idx)
			{
				if (idx >= capacity)
					continue;
				const uint32_t d  = (uint32_t) __ffs((int) m);        // the direction: b = a + d, a = the voxel itself
				const float    fa = corner_value(B, i, 0u), fb = corner_value(B, i, d);
				const float    t  = (iso - fa) / (fb - fa);
				const int      X = x + i, bx = (int) (d & 1u), by = (int) ((d >> 1) & 1u), bz = (int) (d >> 2);
				float         *out = vertices + 3 * idx;
				out[0]             = bx ? (float) X + t : (float) X;
				out[1]             = by ? (float) y + t : (float) y;
				out[2]             = bz ? (float) z + t : (float) z;
				if (normals)
				{
					int ga[3], gb[3];
					central_differences(G, X, y, z, ga);
					central_differences(G, X + bx, y + by, z + bz, gb);
					store_normal(normals + 3 * idx, ga, gb, t);
				}
			}
		}
	}
}

// the six voxels x .. x + 5 of a row as inside bits; bit 5 only in the wave's last lane, which owns no lane above to ask
template <bool WIDE>
__device__ __forceinline__ uint32_t inside6(const uint8_t *row, int x, int W, uint32_t lane, uint32_t thr)
{
	uint32_t q = inside5(row5<WIDE>(row, x, W, lane), thr);
	if (lane == 63)
		q |= row[min(x + 5, W - 1)] >= thr ? 0x20u : 0u;
	return q;
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_meshi_emit_indices(MeshGeom G, const uint32_t *__restrict__ tri_counts, const uint32_t *__restrict__ tri_local,
                                                            const uint64_t *__restrict__ tri_before, const uint32_t *__restrict__ vert_local,
                                                            const uint64_t *__restrict__ vert_before, uint32_t *__restrict__ indices, uint64_t capacity)
{
	__shared__ MtetTable tab;
	stage_mtet(tab, d_mtet_indexed);
	const int      vy = G.ny + 1, vz = G.nz + 1;
	const MeshTile T    = mesh_tile(G, vy, vz);
	const uint32_t lane = threadIdx.x & 63u;
	if (T.yc >= G.ny)        // whole waves only; there is no barrier below.  The far face's rows start no cube
		return;
	uint64_t start;
	uint64_t todo = wave_entries(T, lane, min(T.zc1, G.nz), tri_counts, tri_local, tri_before, capacity, start);
	if (todo == 0)
		return;
	const int    x = G.x0 + T.xc, nvalid = min(max(G.nx - T.xc, 0), 4);
	const size_t W = (size_t) G.W, plane = (size_t) G.H * W;
	while (todo)        // wave-uniform
	{
		const int k = __ffsll((long long) todo) - 1;
		todo &= todo - 1;
		const int      zc = T.zc0 + k;
		const uint64_t at = entry_start(start, k);
		const uint32_t e  = T.e0 + (uint32_t) k * T.e_step;
		// inside bits of the rows (y .. y + 2) x (z .. z + 2), clamped to the box: what is clamped only feeds directions that box_dirs() cuts
		uint32_t Q[3][3];
#pragma unroll
		for (int zz = 0; zz < 3; ++zz)
#pragma unroll
			for (int yy = 0; yy < 3; ++yy)
				Q[zz][yy] = inside6<WIDE>(G.vol + (size_t) (G.z0 + min(zc + zz, G.nz)) * plane + (size_t) (G.y0 + min(T.yc + yy, G.ny)) * W, x, G.W, lane, G.thr);
		// the four owner rows r = oy + 2 oz: the masks of the lane's voxels and of voxel x + 4 (bits 32 ..), the number of the lane's first
		// vertex, and of voxel x + 4's.  (label_mesh_indexed.hip numbers owners by the same lines.  As shared functions over these arrays they
		// cost this kernel 16 to 24 bytes of code and two SGPRs for the row, and 16 KiB of LDS for the corner: the arrays left the registers)
		uint64_t m64[4];
		uint32_t first[4], above[4];
#pragma unroll
		for (int r = 0; r < 4; ++r)
		{
			const int      oy = r & 1, oz = r >> 1;
			const uint32_t q0 = Q[oz][oy] | Q[oz][oy + 1] << 8, q1 = Q[oz + 1][oy] | Q[oz + 1][oy + 1] << 8;
			const uint32_t m  = owner_masks(G, q0, q1, T.xc, T.yc + oy, zc + oz);
			const uint32_t er = e + (uint32_t) oy * G.segs_x + (uint32_t) oz * T.e_step;
			first[r]          = (uint32_t) vert_before[er / kScanChunk] + vert_local[er] + wave_exclusive((uint32_t) __builtin_popcount(m), lane);
			uint32_t m4       = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) m, 0x130, 0xf, 0xf, false) & 0x7fu;        // wave_shl:1
			above[r]          = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) first[r], 0x130, 0xf, 0xf, false);
			if (lane == 63)        // voxel x + 4 opens the next entry
			{
				m4       = crossing_mask(corner_mask(q0, q1, 4)) & box_dirs(G, T.xc + 4, T.yc + oy, zc + oz);
				above[r] = first[r] + (uint32_t) __builtin_popcount(m);        // where this entry's vertices end, the next entry's begin
			}
			m64[r] = (uint64_t) m | (uint64_t) m4 << 32;
		}
		uint32_t mine = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			mine += i < nvalid ? (uint32_t) tab.count[corner_mask(Q[0][0] | Q[0][1] << 8, Q[1][0] | Q[1][1] << 8, i)] : 0u;
		uint64_t idx = at + wave_exclusive(mine, lane);
		if (mine == 0)
			continue;
#pragma unroll 1
		for (int i = 0; i < nvalid; ++i)
		{
			const uint32_t cm = corner_mask(Q[0][0] | Q[0][1] << 8, Q[1][0] | Q[1][1] << 8, i);
			if (tab.count[cm] == 0)
				continue;
#pragma unroll 1
			for (int t = 0; t < 6; ++t)
			{
				const uint32_t p = (kMtetMid1 >> (4 * t)) & 7u, q = (kMtetMid2 >> (4 * t)) & 7u;
				const uint32_t m = (cm & 1u) | ((cm >> p) & 1u) << 1 | ((cm >> q) & 1u) << 2 | (cm >> 7) << 3;
				const uint64_t c = *reinterpret_cast<const uint64_t *>(&tab.c[t][m]);        // n, swap, e[0 .. 5]
				const int      n = (int) (c & 0xffu);
				for (int tri = 0; tri < n; ++tri, ++idx)
				{
					if (idx >= capacity)
						continue;
					uint32_t v[3];
#pragma unroll
					for (int j = 0; j < 3; ++j)
					{
						const uint32_t code = (uint32_t) (c >> (16 + 24 * tri + 8 * j)) & 0x3fu, a = code & 7u, d = a ^ (code >> 3);
						const uint32_t r = a >> 1, kx = (uint32_t) i + (a & 1u);        // the owner's row, and which of the lane's voxels: 4 = the lane above's
						const uint64_t mr = (r & 2u) ? ((r & 1u) ? m64[3] : m64[2]) : ((r & 1u) ? m64[1] : m64[0]);
						const uint32_t fr = (r & 2u) ? ((r & 1u) ? first[3] : first[2]) : ((r & 1u) ? first[1] : first[0]);
						const uint32_t ar = (r & 2u) ? ((r & 1u) ? above[3] : above[2]) : ((r & 1u) ? above[1] : above[0]);
						// the owner's vertices before direction d: in the lane's voxels before it and in its own mask below bit d - 1
						const uint64_t below = kx < 4u ? (1ull << (8u * kx + d - 1u)) - 1ull : ((1ull << (d - 1u)) - 1ull) << 32;
						v[j] = (kx < 4u ? fr : ar) + (uint32_t) __builtin_popcountll(mr & below);
					}
					uint32_t *out = indices + 3 * idx;
					out[0] = v[0], out[1] = v[1], out[2] = v[2];
				}
			}
		}
	}
}

namespace vkv
{

// MeshScratch with two lists, the triangles' before the vertices': 16 bytes per entry of 256 voxels; 0: the extent and box are not accepted
size_t mesh_indexed_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	if (!extent_and_box_ok(e, box) || !mesh_plan(e, whole_or(e, box), p, true))
		return 0;
	return MeshScratch{p, 2, 0, nullptr}.bytes();
}

bool mesh_indexed_launch_ok(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	return mesh_plan(e, whole_or(e, box), p, true);
}

int launch_isosurface_mesh_indexed(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint8_t *d_max_map, VkvExtent3D me,
                                   void *d_scratch, float *d_vertices, float *d_normals, uint64_t capacity_vertices, uint32_t *d_indices,
                                   uint64_t capacity_triangles, uint64_t *d_counts, hipStream_t s)
{
	MeshPlan p;
	if (!mesh_plan(e, b, p, true))
		return set_error(ctx, VKV_E_UNSUPPORTED, "isosurface_mesh_indexed: volume too large for the launches");
	const MeshScratch S{p, 2, 0, d_scratch};        // list 0: the triangles, list 1: the vertices
	const MeshGeom    G    = mesh_geom(d_vol, e, b, iso, d_max_map, me, p);
	const bool     wide   = e.width >= 4;        // the kernels' dword row loads
	if (p.entries)
	{
		dispatch_wide(wide, [&](auto w) { hipLaunchKernelGGL(k_meshi_count<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, G, S.counts(0), S.counts(1)); });
		hipLaunchKernelGGL(k_meshi_scan_chunks, dim3(p.chunks, 2), dim3(256), 0, s, S.counts(0), S.local(0), S.sums(0), p.entries, p.chunks);
	}
	hipLaunchKernelGGL(k_meshi_scan_total, dim3(2), dim3(256), 0, s, S.sums(0), p.chunks, capacity_triangles, capacity_vertices, d_counts);
	if (p.entries && capacity_vertices)
		dispatch_wide(wide, [&](auto w) {
			hipLaunchKernelGGL(k_meshi_emit_vertices<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, G, S.counts(1), S.local(1), S.sums(1), iso,
			                   d_vertices, d_normals, capacity_vertices);
		});
	if (p.entries && capacity_triangles)
		dispatch_wide(wide, [&](auto w) {
			hipLaunchKernelGGL(k_meshi_emit_indices<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, G, S.counts(0), S.local(0), S.sums(0), S.local(1), S.sums(1),
			                   d_indices, capacity_triangles);
		});
	return check_launch(ctx, "isosurface_mesh_indexed");
}

}        // namespace vkv

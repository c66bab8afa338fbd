// label_mesh_indexed.hip — the surfaces of the visible bodies of a uint32 label array as an indexed mesh (vkv_label_mesh_indexed, DESIGN.md
// §5.23): the triangles of vkv_label_mesh in their order as three vertex numbers and one label each, one vertex per crossing tetrahedron edge,
// on request with its gradient normal and with the two shown labels it separates.  Dword streaming; no MFMA.
//
// This is the product of mesh_indexed.hip and label_mesh.hip.  From the first: an edge belongs to the voxel at its lower corner a and the
// direction d = a ^ b, the vertex list is the crossing edges by owner voxel, then d, tiles and entries are dealt over the box's VOXELS, an
// entry of 256 x-adjacent voxels carries two counts, and an owner's number is its entry's start + the crossing edges of the entry's earlier
// voxels + the rank of d in its mask.  From the second: the row loads of labels, the table lookup once per distinct label of a cube, the
// triangle counts and the walk cube, tetrahedron, group, triangle.  "Crossing" here means shown(label(v)) != shown(label(v + d)).
// What is new: the count kernel keeps every voxel's crossing mask, one byte (7 bits) per voxel, rows padded to a multiple of 4, behind the
// entries in scratch.  The emit kernels number vertices from those bytes (a dword per lane and owner row) and read labels only for the 2 x 2
// rows their cubes need; recomputing the owners' masks as mesh_indexed.hip does would take 3 x 3 rows of five DWORDS per lane and table
// lookups for rows the cube walk never touches (DESIGN.md §5.23 has the argument).
//   k_lmeshi_count          per entry the triangles of the cubes that start there and the crossing edges they own, and the masks.  With a
//                           visibility map a workgroup whose cells all hold 0 writes zeros, masks included, without reading a label.
//   k_lmeshi_scan_*         the fixed-tree scans of fixed_scan.hpp, both lists in one launch each.
//   k_lmeshi_emit_vertices  per entry with vertices below the capacity: its masks, then position and (on request) normal and label pair of
//                           every crossing edge.  The volume's bytes are read here only; a pair is two label gathers per crossing edge.
//   k_lmeshi_emit_indices   per entry with triangles below the capacity: the masks of the four owner rows (y, y + 1) x (z, z + 1), each
//                           prefixed over the lanes, and label_mesh.hip's walk.  The owner at x + 4 is the lane above's first voxel; for the
//                           last lane it opens the NEXT entry of the row, whose vertices begin where this entry's end.
// No kernel uses scratch memory or atomics (tests/test_label_mesh_indexed_cpu.py reads the listing).  box_dirs(), central_differences(),
// store_normal() and the emit kernels' opening are mesh_common.hpp's; the argument block's builder is label_mesh_common.hpp's.
#include "label_mesh_common.hpp"
#include "launchers.hpp"

using namespace vkv;

__constant__ MtetTable d_lmtet_indexed = kMtetTable;

namespace
{

// the crossing masks in scratch: one byte per voxel of the box, rows of `stride` bytes (the box's width rounded up to 4) in (z, y) order
struct MaskRows
{
	uint8_t *at;
	uint32_t stride;
	int      rows;        // per slice: the box's height
	__device__ __forceinline__ uint8_t *row(int yv, int zv) const { return at + ((size_t) zv * (size_t) rows + (size_t) yv) * (size_t) stride; }
};

// bit d - 1 = the shown labels at corners 0 and d of a cube differ
__device__ __forceinline__ uint32_t crossing_mask(const uint32_t E[8])
{
	uint32_t m = 0;
#pragma unroll
	for (int d = 1; d < 8; ++d)
		m |= (E[d] != E[0] ? 1u : 0u) << (d - 1);
	return m;
}

// of the lane's voxels xv .. xv + 3 of row (yv, zv): the crossing masks, one per byte, and the triangles of the first ncubes cubes that start there
__device__ __forceinline__ void lane_edges(const LabelGeom &A, const uint8_t *lut, const CubeRows &R, int xv, int yv, int zv, int ncubes, uint32_t &masks,
                                           uint32_t &triangles)
{
	masks = 0u, triangles = 0u;
	uint32_t dif = 0;
#pragma unroll
	for (int j = 0; j < 4; ++j)
#pragma unroll
		for (int i = 0; i < 5; ++i)
			dif |= R.r[j].v[i] ^ R.r[0].v[0];
	if (dif == 0u)
		return;
#pragma unroll
	for (int i = 0; i < 4; ++i)
	{
		uint32_t c[8], d8 = 0;
#pragma unroll
		for (int j = 0; j < 8; ++j)
		{
			c[j] = R.r[j >> 1].v[i + (j & 1)];
			d8 |= c[j] ^ c[0];
		}
		if (d8 == 0u)
			continue;
		uint32_t E[8];
		shown8(A, c, E);
		masks |= (crossing_mask(E) & box_dirs(A.G, xv + i, yv, zv)) << (8 * i);
		if (i < ncubes)
			triangles += shown_cube_count(lut, E);
	}
}

// shown(L): L if the table shows it, else 0
__device__ __forceinline__ uint32_t shown1(const LabelGeom &A, uint32_t L)
{
	if (!A.colors)
		return L;
	return L - 1u < A.entries && (A.colors[L - 1u] >> 24) != 0u ? L : 0u;        // label 0 gives 2^32 - 1, which no table names
}

}        // namespace

// One pass: tri_counts[e] = the triangles of the cubes that start at entry e's voxels, vert_counts[e] = the crossing edges they own, and
// every voxel's crossing mask.
template <bool WIDE>
__global__ void __launch_bounds__(256) k_lmeshi_count(LabelGeom A, uint32_t *__restrict__ tri_counts, uint32_t *__restrict__ vert_counts, MaskRows M)
{
	__shared__ uint8_t lut[256];
	const MeshGeom &   G  = A.G;
	const int          vy = G.ny + 1, vz = G.nz + 1;
	const MeshTile     T    = mesh_tile(G, vy, vz);
	const uint32_t     lane = threadIdx.x & 63u;
	const bool         own  = T.xc < A.bw;        // the lane's four voxels begin inside the row: it owns a dword of masks
	if (G.mm.map && tile_is_empty(G, T, G.nx + 1, vy))        // a cell of 0: its voxels and their neighbours show nothing, no edge from them crosses
	{
		if (T.yc < vy)
		{
			uint32_t e = T.e0;
			for (int zv = T.zc0; zv < T.zc1; ++zv, e += T.e_step)
			{
				if (lane == 0)
					tri_counts[e] = 0u, vert_counts[e] = 0u;
				if (own)
					*reinterpret_cast<uint32_t *>(M.row(T.yc, zv) + T.xc) = 0u;
			}
		}
		return;
	}
	lut[threadIdx.x] = d_lmtet_indexed.count[threadIdx.x];
	__syncthreads();
	if (T.yc >= vy)        // whole waves only: the lanes exchange labels below
		return;
	const int    ncubes = T.yc < G.ny ? min(max(G.nx - T.xc, 0), 4) : 0;
	const size_t plane = (size_t) A.bh * (size_t) A.bw, row = (size_t) T.yc * (size_t) A.bw;
	const size_t up = T.yc < G.ny ? (size_t) A.bw : 0;        // the far face's rows stand in for the row past them: those directions are cut
	auto         load = [&](int zv, Lab5 &a, Lab5 &b) {
        const uint32_t *base = A.labels + (size_t) min(zv, G.nz) * plane + row;
        a = lab5<WIDE>(base, T.xc, A.bw, lane), b = lab5<WIDE>(base + up, T.xc, A.bw, lane);
	};
	CubeRows R;
	Lab5     na, nb;
	load(T.zc0, R.r[0], R.r[1]);
	load(T.zc0 + 1, na, nb);
	uint32_t e = T.e0;
	for (int zv = T.zc0; zv < T.zc1; ++zv, e += T.e_step)
	{
		R.r[2] = na, R.r[3] = nb;
		if (zv + 1 < T.zc1)        // wave-uniform
			load(zv + 2, na, nb);
		uint32_t masks, triangles;
		lane_edges(A, lut, R, T.xc, T.yc, zv, zv < G.nz ? ncubes : 0, masks, triangles);
		const uint32_t n = wave_sum(triangles | (uint32_t) __builtin_popcount(masks) << 16);        // at most 7 x 256 vertices, 24 x 256 triangles
		if (lane == 0)
			tri_counts[e] = n & 0xffffu, vert_counts[e] = n >> 16;
		if (own)
			*reinterpret_cast<uint32_t *>(M.row(T.yc, zv) + T.xc) = masks;
		R.r[0] = R.r[2], R.r[1] = R.r[3];
	}
}

// both lists' entries lie one behind the other: [counts, local] x 2 and [sums] x 2; blockIdx.y = the list
__global__ void __launch_bounds__(256) k_lmeshi_scan_chunks(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                            uint32_t n_entries, uint32_t n_chunks)
{
	const size_t list = blockIdx.y;
	scan_chunk(counts + 2 * list * n_entries, local + 2 * list * n_entries, sums + list * n_chunks, n_entries);
}

// workgroup 0: the triangles into d_counts[0, 1]; workgroup 1: the vertices into d_counts[2, 3]
__global__ void __launch_bounds__(256) k_lmeshi_scan_total(uint64_t *__restrict__ sums, uint32_t n_chunks, uint64_t capacity_triangles,
                                                           uint64_t capacity_vertices, uint64_t *__restrict__ d_counts)
{
	const size_t list = blockIdx.x;
	scan_total(sums + list * n_chunks, n_chunks, list ? capacity_vertices : capacity_triangles, d_counts + 2 * list);
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_lmeshi_emit_vertices(LabelGeom A, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                              const uint64_t *__restrict__ chunk_before, MaskRows M, float iso, float *__restrict__ vertices,
                                                              float *__restrict__ normals, uint32_t *__restrict__ vertex_labels, uint64_t capacity)
{
	const MeshGeom &G  = A.G;
	const int       vy = G.ny + 1, vz = G.nz + 1;
	const MeshTile  T    = mesh_tile(G, vy, vz);
	const uint32_t  lane = threadIdx.x & 63u;
	if (T.yc >= vy)        // whole waves only; there is no barrier
		return;
	// the wave's entries, one per lane: those with vertices that start below the capacity
	uint64_t start;
	uint64_t todo = wave_entries(T, lane, T.zc1, counts, local, chunk_before, capacity, start);
	if (todo == 0)
		return;
	const int    x = G.x0 + T.xc, y = G.y0 + T.yc;
	const size_t plane = (size_t) A.bh * (size_t) A.bw, row = (size_t) T.yc * (size_t) A.bw;
	const size_t vplane = (size_t) G.H * (size_t) G.W, vup = T.yc < G.ny ? (size_t) G.W : 0;
	while (todo)        // wave-uniform
	{
		const int k = __ffsll((long long) todo) - 1;
		todo &= todo - 1;
		const int      zv = T.zc0 + k, z = G.z0 + zv;
		const uint64_t at    = entry_start(start, k);
		const uint32_t masks = T.xc < A.bw ? *reinterpret_cast<const uint32_t *>(M.row(T.yc, zv) + T.xc) : 0u;
		// the far faces' rows stand in for the rows past them: what they hold only feeds directions that the masks do not have
		CubeBytes B{};
		if (G.vol)        // wave-uniform
		{
			const uint8_t *vrow  = G.vol + (size_t) z * vplane + (size_t) y * (size_t) G.W;
			const size_t   vback = zv < G.nz ? vplane : 0;
			B.v[0] = bytes5(vrow, x, G.W, lane), B.v[1] = bytes5(vrow + vup, x, G.W, lane);
			B.v[2] = bytes5(vrow + vback, x, G.W, lane), B.v[3] = bytes5(vrow + vback + vup, x, G.W, lane);
		}
		const uint32_t mine = __builtin_popcount(masks);
		uint64_t       idx  = at + wave_exclusive(mine, lane);
		if (mine == 0)
			continue;
#pragma unroll 1
		for (int i = 0; i < 4; ++i)
		{
			uint32_t m = (masks >> (8 * i)) & 0x7fu;
			if (m == 0u)
				continue;
			const uint64_t  cb = cube_bytes(B, i);
			const uint32_t *la = A.labels + (size_t) zv * plane + row + (size_t) (T.xc + i);        // the voxel's own label
			const int      X  = x + i;
			for (; m; m &= m - 1, ++idx)
			{
				if (idx >= capacity)
					continue;
				const uint32_t d = (uint32_t) __ffs((int) m);        // the direction: b = a + d, a = the voxel itself
				const float    t = label_edge_t(G.vol != nullptr, cb, 0u, d, iso);
				float          p[3];
				label_edge_vertex(t, d << 3, X, y, z, p);
				float *out = vertices + 3 * idx;
				out[0] = p[0], out[1] = p[1], out[2] = p[2];
				if (normals)
				{
					int ga[3], gb[3];
					central_differences(G, X, y, z, ga);
					central_differences(G, X + (int) (d & 1u), y + (int) ((d >> 1) & 1u), z + (int) (d >> 2), gb);
					store_normal(normals + 3 * idx, ga, gb, t);
				}
				if (vertex_labels)        // two gathers per crossing edge: rows of labels held for this alone cost more registers than the kernel has
				{
					const uint32_t own = shown1(A, la[0]), other = shown1(A, la[(size_t) (d >> 2) * plane + (size_t) ((d >> 1) & 1u) * (size_t) A.bw + (d & 1u)]);
					vertex_labels[2 * idx] = own, vertex_labels[2 * idx + 1] = other;
				}
			}
		}
	}
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_lmeshi_emit_indices(LabelGeom A, const uint32_t *__restrict__ tri_counts, const uint32_t *__restrict__ tri_local,
                                                             const uint64_t *__restrict__ tri_before, const uint32_t *__restrict__ vert_local,
                                                             const uint64_t *__restrict__ vert_before, MaskRows M, uint32_t *__restrict__ indices,
                                                             uint32_t *__restrict__ triangle_labels, uint64_t capacity)
{
	__shared__ MtetTable tab;
	stage_mtet(tab, d_lmtet_indexed);
	const MeshGeom &G  = A.G;
	const int       vy = G.ny + 1, vz = G.nz + 1;
	const MeshTile  T    = mesh_tile(G, vy, vz);
	const uint32_t  lane = threadIdx.x & 63u;
	if (T.yc >= G.ny)        // whole waves only; there is no barrier below.  The far face's rows start no cube
		return;
	uint64_t start;
	uint64_t todo = wave_entries(T, lane, min(T.zc1, G.nz), tri_counts, tri_local, tri_before, capacity, start);
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
		const uint32_t  e  = T.e0 + (uint32_t) k * T.e_step;
		const uint32_t *base = A.labels + (size_t) zc * plane + row;
		CubeRows        R;
		R.r[0] = lab5<WIDE>(base, T.xc, A.bw, lane), R.r[1] = lab5<WIDE>(base + A.bw, T.xc, A.bw, lane);
		R.r[2] = lab5<WIDE>(base + plane, T.xc, A.bw, lane), R.r[3] = lab5<WIDE>(base + plane + A.bw, T.xc, A.bw, lane);
		// the four owner rows r = oy + 2 oz: the masks of the lane's voxels and of voxel x + 4 (bits 32 ..), the number of the lane's first
		// vertex, and of voxel x + 4's.  (mesh_indexed.hip's lines, kept as a copy for the reason given there: as a shared function the
		// corner's rule put these arrays into 16 KiB of LDS here too)
		uint64_t m64[4];
		uint32_t first[4], above[4];
#pragma unroll
		for (int r = 0; r < 4; ++r)
		{
			const int      oy = r & 1, oz = r >> 1;
			const uint8_t *mr = M.row(T.yc + oy, zc + oz);
			const uint32_t m  = T.xc < A.bw ? *reinterpret_cast<const uint32_t *>(mr + T.xc) : 0u;
			const uint32_t er = e + (uint32_t) oy * G.segs_x + (uint32_t) oz * T.e_step;
			first[r]          = (uint32_t) vert_before[er / kScanChunk] + vert_local[er] + wave_exclusive((uint32_t) __builtin_popcount(m), lane);
			uint32_t m4       = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) m, 0x130, 0xf, 0xf, false) & 0x7fu;        // wave_shl:1
			above[r]          = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) first[r], 0x130, 0xf, 0xf, false);
			if (lane == 63)        // voxel x + 4 opens the next entry
			{
				m4       = T.xc + 4 < A.bw ? (uint32_t) mr[T.xc + 4] : 0u;
				above[r] = first[r] + (uint32_t) __builtin_popcount(m);        // where this entry's vertices end, the next entry's begin
			}
			m64[r] = (uint64_t) m | (uint64_t) m4 << 32;
		}
		const uint32_t mine = lane_count(A, tab.count, R, nvalid);
		uint64_t       idx  = at + wave_exclusive(mine, lane);        // the cubes of a row lie in lane order
		if (mine == 0)
			continue;
#pragma unroll 1
		for (int i = 0; i < nvalid; ++i)
		{
			uint32_t c[8], dif = 0;
			cube_labels(R, i, c);
#pragma unroll
			for (int j = 1; j < 8; ++j)
				dif |= c[j] ^ c[0];
			if (dif == 0u)
				continue;
			uint32_t E[8];
			shown8(A, c, E);
#pragma unroll 1
			for (int t = 0; t < 6; ++t)
			{
				const uint32_t p = (kMtetMid1 >> (4 * t)) & 7u, q = (kMtetMid2 >> (4 * t)) & 7u;
				const uint32_t l0 = E[0], l1 = p == 1u ? E[1] : p == 2u ? E[2] : E[4], l2 = q == 3u ? E[3] : q == 5u ? E[5] : E[6], l3 = E[7];
				// the local vertices that start a group: a visible label that no lower vertex carries (label_mesh.hip's walk, a copy: see there)
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
						uint32_t v[3];
#pragma unroll
						for (int j = 0; j < 3; ++j)
						{
							const uint32_t code = (uint32_t) (cs >> (16 + 24 * tri + 8 * j)) & 0x3fu, a = code & 7u, d = a ^ (code >> 3);
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
						triangle_labels[idx] = L;
					}
				}
			}
		}
	}
}

namespace vkv
{

// the box's voxels dealt as mesh_indexed.hip deals them; false: not accepted, more than 2^32 - 1 voxels, or too large for the launches
static bool label_mesh_indexed_plan(VkvExtent3D e, const VkvBox *box, MeshPlan &p)
{
	return extent_and_box_ok(e, box) && components_launch_ok(e, box) && mesh_plan(e, whole_or(e, box), p, true);
}

// the masks' row: the box's width rounded up to a dword, so that every lane's four voxels are one aligned dword
static uint32_t mask_stride(const VkvBox &b) { return (b.width + 3u) & ~3u; }

// one crossing-mask byte per voxel in rows of mask_stride(); none for a box without cubes
static size_t mask_bytes(const MeshPlan &p, const VkvBox &b) { return p.entries ? (size_t) mask_stride(b) * (size_t) b.height * (size_t) b.depth : 0; }

// MeshScratch with two lists as in mesh_indexed.hip, 16 bytes per entry of 256 voxels, and behind them the masks; 0: the extent and box are
// not accepted
size_t label_mesh_indexed_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	if (!label_mesh_indexed_plan(e, box, p))
		return 0;
	return MeshScratch{p, 2, mask_bytes(p, whole_or(e, box)), nullptr}.bytes();
}

bool label_mesh_indexed_launch_ok(VkvExtent3D e, const VkvBox *box)
{
	MeshPlan p;
	return label_mesh_indexed_plan(e, box, p);
}

int launch_label_mesh_indexed(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D e, const VkvBox &b, const uint32_t *d_colors, uint64_t table_entries,
                              const uint8_t *d_vol, float iso, const uint8_t *d_visibility_map, VkvExtent3D me, void *d_scratch, float *d_vertices,
                              float *d_normals, uint32_t *d_vertex_labels, uint64_t capacity_vertices, uint32_t *d_indices, uint32_t *d_triangle_labels,
                              uint64_t capacity_triangles, uint64_t *d_counts, hipStream_t s)
{
	MeshPlan p;
	if (!mesh_plan(e, b, p, true))
		return set_error(ctx, VKV_E_UNSUPPORTED, "label_mesh_indexed: volume too large for the launches");
	const MeshScratch S{p, 2, mask_bytes(p, b), d_scratch};        // list 0: the triangles, list 1: the vertices; behind them the masks
	const MaskRows    M{S.behind(), mask_stride(b), (int) b.height};
	const LabelGeom   A = label_geom(d_labels, e, b, d_colors, table_entries, d_vol, d_visibility_map, me, p);
	const bool wide = b.width >= 4;        // the kernels' 16-byte row loads
	if (p.entries)
	{
		dispatch_wide(wide, [&](auto w) { hipLaunchKernelGGL(k_lmeshi_count<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, A, S.counts(0), S.counts(1), M); });
		hipLaunchKernelGGL(k_lmeshi_scan_chunks, dim3(p.chunks, 2), dim3(256), 0, s, S.counts(0), S.local(0), S.sums(0), p.entries, p.chunks);
	}
	hipLaunchKernelGGL(k_lmeshi_scan_total, dim3(2), dim3(256), 0, s, S.sums(0), p.chunks, capacity_triangles, capacity_vertices, d_counts);
	if (p.entries && capacity_vertices)
		dispatch_wide(wide, [&](auto w) {
			hipLaunchKernelGGL(k_lmeshi_emit_vertices<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, A, S.counts(1), S.local(1), S.sums(1), M, iso,
			                   d_vertices, d_normals, d_vertex_labels, capacity_vertices);
		});
	if (p.entries && capacity_triangles)
		dispatch_wide(wide, [&](auto w) {
			hipLaunchKernelGGL(k_lmeshi_emit_indices<decltype(w)::value>, dim3(p.wgs), dim3(256), 0, s, A, S.counts(0), S.local(0), S.sums(0), S.local(1), S.sums(1), M,
			                   d_indices, d_triangle_labels, capacity_triangles);
		});
	return check_launch(ctx, "label_mesh_indexed");
}

}        // namespace vkv

// mesh_common.hpp — what the kernels of the four mesh extractors share: mesh.hip (vkv_isosurface_mesh), mesh_indexed.hip
// (vkv_isosurface_mesh_indexed) and, through label_mesh_common.hpp, label_mesh.hip and label_mesh_indexed.hip; DESIGN.md §5.13, §5.14, §5.22,
// §5.23.  Each step of the count / scan / emit pipeline is stated here once:
//   geometry   the tile (mesh_tile), the empty-tile test and the zero fill of its entries (tile_is_empty, zero_tile_counts), the row loads and
//              inside bits (row5, inside5), the corner mask (corner_mask)
//   emit       the table's staging (stage_mtet), the wave's entries and their starts (wave_entries, entry_start), edge_vertex, store_triangle
//   owners     of the indexed meshes: the directions that stay in the box (box_dirs), central_differences and store_normal
//   host       the plan (mesh_plan), the kernels' geometry block (mesh_geom), the scratch layout's size and pointers (MeshScratch)
// Four steps are NOT here and remain as copies in the kernels (the last three with a note at the copy), because as shared functions they changed a
// kernel's code size, registers or LDS (profiles/mesh_family_refactor.txt has the figures): the sum of a lane's four counts, the owner rows'
// numbering and a corner's vertex number in the two *_emit_indices kernels, and the label emits' walk over a tetrahedron's groups.
// The scans are fixed_scan.hpp's; the box, the max map and the WIDE dispatch are box_domain.hpp's.
#pragma once

#include "box_domain.hpp"
#include "fixed_scan.hpp"
#include "mtet_table.hpp"

namespace vkv
{

constexpr int      kMeshTileX = 256, kMeshTileY = 4;        // cubes of a workgroup per slice: 64 lanes x 4 cubes, 4 rows
constexpr int      kMeshSegment = 16;                       // slices of cubes a workgroup marches over (it loads one more)
static_assert(kMeshSegment <= 64, "a wave tests its entries one per lane");

// the middle corners of tetrahedron t (its local vertices 1 and 2; 0 and 3 are the cube's corners 0 and 7), one nibble per tetrahedron
constexpr uint32_t mtet_pack_corner(int local)
{
	uint32_t p = 0;
	for (int t = 0; t < 6; ++t)
		p |= (uint32_t) kMtetCorners[t][local] << (4 * t);
	return p;
}
constexpr uint32_t kMtetMid1 = mtet_pack_corner(1), kMtetMid2 = mtet_pack_corner(2);
static_assert(mtet_pack_corner(0) == 0u && mtet_pack_corner(3) == 0x777777u, "every tetrahedron runs from corner 0 to corner 7");

struct MeshGeom
{
	const uint8_t *vol;
	int            W, H, D;
	int            x0, y0, z0;        // the box's first voxel = the first cube's origin
	int            nx, ny, nz;        // cubes of the box per axis: its extent - 1
	uint32_t       segs_x, tiles_y, n_wgs;
	uint32_t       thr;               // the smallest inside byte (iso_threshold); 256: none
	MaxMap         mm;                // the max map or none
};

// What a lane holds of one row: `d`, the voxels x .. x + 3 (zero past the row's end), and `e`, voxel x + 4: the first byte of the lane above
// (v_mov_b32 wave_shl:1; every lane of the wave takes part), in the wave's last lane a byte load.  WIDE (W >= 4): one dword load at
// min(x, W - 4), at any alignment, shifted down where it was moved; narrower rows gather bytes.  Nothing outside the row is read; what is
// not a voxel of the row only reaches cubes that are not counted.
struct Row5
{
	uint32_t d, e;
};

template <bool WIDE>
__device__ __forceinline__ Row5 row5(const uint8_t *row, int x, int W, uint32_t lane)
{
	Row5 r;
	if (WIDE)
	{
		r.d            = load_u32_any(row + min(x, W - 4));
		const int over = x + 4 - W;
		if (over > 0)
			r.d = over >= 4 ? 0u : r.d >> (8 * over);
	}
	else
	{
		r.d = 0;
#pragma unroll
		for (int i = 0; i < 4; ++i)
			if (x + i < W)
				r.d |= (uint32_t) row[x + i] << (8 * i);
	}
	r.e = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) r.d, 0x130, 0xf, 0xf, false) & 0xffu;        // wave_shl:1
	if (lane == 63)
		r.e = row[min(x + 4, W - 1)];
	return r;
}

// bit i = voxel i of the five is inside: byte >= thr, which is (float) byte * kInv255 >= iso (the product is monotone in the byte).  Two
// 16-bit fields per dword: (b | 0x100) - thr lies in 0 .. 511 for thr <= 256 and has bit 8 set exactly when b >= thr.
__device__ __forceinline__ uint32_t inside5(Row5 r, uint32_t thr)
{
	const uint32_t k  = thr * 0x00010001u;
	const uint32_t ev = ((r.d & 0x00ff00ffu) | 0x01000100u) - k, od = (((r.d >> 8) & 0x00ff00ffu) | 0x01000100u) - k;
	const uint32_t m  = ((ev >> 8) & 0x00010001u) | ((od >> 7) & 0x00020002u);        // bits 0, 1, 16, 17: voxels 0, 1, 2, 3
	return ((m | m >> 14) & 0xfu) | (r.e >= thr ? 0x10u : 0u);
}

// the corner mask of the lane's cube i from the inside bits of its two slices, each (row y) | (row y + 1) << 8
__device__ __forceinline__ uint32_t corner_mask(uint32_t q0, uint32_t q1, int i)
{
	const uint32_t a = q0 >> i, b = q1 >> i;
	return (a & 3u) | ((a >> 6) & 0xcu) | (b & 3u) << 4 | ((b >> 6) & 0xcu) << 4;
}

struct MeshTile
{
	uint32_t xs;                 // x segment
	int      xc, yc, zc0, zc1;        // the lane's first cube and its row (yc may lie past the box), the slices [zc0, zc1), relative to the box
	uint32_t e0, e_step;         // the wave's entry of slice zc0 and the step to the next slice
};

// rows, slices: what the tiles are dealt over, the box's cubes (G.ny, G.nz) or its voxels (one more)
__device__ __forceinline__ MeshTile mesh_tile(const MeshGeom &G, int rows, int slices)
{
	const uint32_t t = xcd_remap(blockIdx.x, G.n_wgs), lane = threadIdx.x & 63u;
	MeshTile       T;
	T.xs     = t % G.segs_x;
	T.xc     = (int) T.xs * kMeshTileX + 4 * (int) lane;
	T.yc     = (int) ((t / G.segs_x) % G.tiles_y) * kMeshTileY + (int) (threadIdx.x >> 6);
	T.zc0    = (int) (t / (G.segs_x * G.tiles_y)) * kMeshSegment;
	T.zc1    = min(T.zc0 + kMeshSegment, slices);
	T.e_step = (uint32_t) rows * G.segs_x;
	T.e0     = ((uint32_t) T.zc0 * (uint32_t) rows + (uint32_t) T.yc) * G.segs_x + T.xs;
	return T;
}

// every map cell that holds a cube origin (cols = G.nx, rows = G.ny) or a voxel (one more each) of the workgroup's tile stays below iso
// (workgroup-uniform; a barrier inside)
__device__ __forceinline__ bool tile_is_empty(const MeshGeom &G, const MeshTile &T, int cols, int rows)
{
	const int xa = G.x0 + (int) T.xs * kMeshTileX, xb = G.x0 + min((int) T.xs * kMeshTileX + kMeshTileX, cols) - 1;
	const int yt = T.yc - (int) (threadIdx.x >> 6);
	const int ya = G.y0 + yt, yb = G.y0 + min(yt + kMeshTileY, rows) - 1;
	const int za = G.z0 + T.zc0, zb = G.z0 + T.zc1 - 1;
	const int cx = xa / G.mm.bx, cy = ya / G.mm.by, cz = za / G.mm.bz;
	const int ncx = xb / G.mm.bx - cx + 1, ncy = yb / G.mm.by - cy + 1, ncz = zb / G.mm.bz - cz + 1;
	int       any = 0;
	for (int i = (int) threadIdx.x; i < ncx * ncy * ncz; i += 256)
	{
		const int ix = i % ncx, iy = (i / ncx) % ncy, iz = i / (ncx * ncy);
		any |= G.mm.map[G.mm.cell(cz + iz, cy + iy, cx + ix)] >= G.thr;
	}
	return !__syncthreads_or(any);
}

// an empty tile's entries, where the tiles are dealt over the box's cubes and an entry holds one count: its 4 rows x kMeshSegment slices, one
// entry per thread
__device__ __forceinline__ void zero_tile_counts(const MeshGeom &G, const MeshTile &T, uint32_t *__restrict__ counts)
{
	if (threadIdx.x < 4 * kMeshSegment)
	{
		const int yc = T.yc - (int) (threadIdx.x >> 6) + (int) (threadIdx.x & 3u), zc = T.zc0 + (int) (threadIdx.x >> 2);
		if (yc < G.ny && zc < T.zc1)
			counts[((uint32_t) zc * (uint32_t) G.ny + (uint32_t) yc) * G.segs_x + T.xs] = 0u;
	}
}

// the case table into LDS, by all 256 threads, a barrier behind it: a cube's walk reads it once per tetrahedron, one after the other
__device__ __forceinline__ void stage_mtet(MtetTable &tab, const MtetTable &src)
{
	static_assert(sizeof(MtetTable) == 4 * 256 && alignof(MtetTable) >= 8, "one dword per thread; a case is read as one 64-bit word");
	reinterpret_cast<uint32_t *>(&tab)[threadIdx.x] = reinterpret_cast<const uint32_t *>(&src)[threadIdx.x];
	__syncthreads();
}

// The wave's entries, one per lane (those of the slices [T.zc0, zend)): the ballot of those that hold something and start below the capacity,
// and in `start` the lane's entry's first output index
__device__ __forceinline__ uint64_t wave_entries(const MeshTile &T, uint32_t lane, int zend, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                 const uint64_t *__restrict__ chunk_before, uint64_t capacity, uint64_t &start)
{
	start     = 0;
	bool work = false;
	if (T.zc0 + (int) lane < zend)
	{
		const uint32_t e = T.e0 + lane * T.e_step;
		start            = chunk_before[e / kScanChunk] + local[e];
		work             = counts[e] != 0u && start < capacity;
	}
	return __ballot(work);
}

// entry k's start, from lane k (k is wave-uniform).  Fetch it first in the entry's loop, ahead of the row loads: behind them the same two
// readlanes reordered the loop's code in two kernels
__device__ __forceinline__ uint64_t entry_start(uint64_t start, int k)
{
	const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) start, k), hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (start >> 32), k);
	return (uint64_t) hi << 32 | lo;
}

// the five voxels of row (j >> 1) & 3 = slice * 2 + row as one 64-bit value each; corner j of cube i is byte i + (j & 1) of it
struct CubeBytes
{
	uint64_t v[4];
};

__device__ __forceinline__ float corner_value(const CubeBytes &B, int i, uint32_t j)
{
	const uint64_t lo = (j & 2u) ? B.v[1] : B.v[0], hi = (j & 2u) ? B.v[3] : B.v[2];
	const uint64_t v  = (j & 4u) ? hi : lo;
	return (float) (uint32_t) ((v >> (8 * (i + (int) (j & 1u)))) & 0xffu) * kInv255;
}

// the vertex on the edge `code` = a | b << 3 of the cube with origin (cx, cy, cz): from a towards b, whoever is inside
__device__ __forceinline__ void edge_vertex(const CubeBytes &B, int i, uint32_t code, int cx, int cy, int cz, float iso, float *out)
{
	const uint32_t a = code & 7u, b = code >> 3, dif = a ^ b;
	const float    fa = corner_value(B, i, a), fb = corner_value(B, i, b);
	const float    t  = (iso - fa) / (fb - fa);
	const float    ax = (float) (cx + (int) (a & 1u)), ay = (float) (cy + (int) ((a >> 1) & 1u)), az = (float) (cz + (int) (a >> 2));
	out[0] = (dif & 1u) ? ax + t : ax;
	out[1] = (dif & 2u) ? ay + t : ay;
	out[2] = (dif & 4u) ? az + t : az;
}

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// a triangle's nine floats, 36 bytes at a 4-byte alignment: two 16-byte stores and a dword
__device__ __forceinline__ void store_triangle(float *out, const float v[9])
{
	*reinterpret_cast<f32x4_a4 *>(out)     = f32x4_a4{v[0], v[1], v[2], v[3]};
	*reinterpret_cast<f32x4_a4 *>(out + 4) = f32x4_a4{v[4], v[5], v[6], v[7]};
	out[8]                                 = v[8];
}

// ---- the indexed meshes: an edge's vertex belongs to the voxel at its lower corner a and the direction d = a ^ b
// the directions (bit d - 1) that stay in the box from its voxel (xv, yv, zv), relative to the box; none from a voxel past it along x
__device__ __forceinline__ uint32_t box_dirs(const MeshGeom &G, int xv, int yv, int zv)
{
	uint32_t m = xv > G.nx ? 0u : 0x7fu;
	m &= xv >= G.nx ? ~0x55u : ~0u;        // d with dx: 1, 3, 5, 7
	m &= yv >= G.ny ? ~0x66u : ~0u;        // d with dy: 2, 3, 6, 7
	m &= zv >= G.nz ? ~0x78u : ~0u;        // d with dz: 4 .. 7
	return m;
}

// G_c of the volume's voxel (X, Y, Z): the byte after minus the byte before along each axis, both clamped to the volume
__device__ __forceinline__ void central_differences(const MeshGeom &G, int X, int Y, int Z, int g[3])
{
	const size_t   W = (size_t) G.W, plane = (size_t) G.H * W;
	const uint8_t *p = G.vol + (size_t) Z * plane + (size_t) Y * W;
	g[0]             = (int) p[min(X + 1, G.W - 1)] - (int) p[max(X - 1, 0)];
	g[1]             = (int) G.vol[(size_t) Z * plane + (size_t) min(Y + 1, G.H - 1) * W + (size_t) X] - (int) G.vol[(size_t) Z * plane + (size_t) max(Y - 1, 0) * W + (size_t) X];
	g[2]             = (int) G.vol[(size_t) min(Z + 1, G.D - 1) * plane + (size_t) Y * W + (size_t) X] - (int) G.vol[(size_t) max(Z - 1, 0) * plane + (size_t) Y * W + (size_t) X];
}

// the normal of a vertex t of the way from a voxel with gradient ga to one with gb: minus the interpolated gradient
__device__ __forceinline__ void store_normal(float *out, const int ga[3], const int gb[3], float t)
{
#pragma unroll
	for (int c = 0; c < 3; ++c)
		out[c] = -((float) ga[c] + t * (float) (gb[c] - ga[c]));
}

// ---- host side: what a call is dealt into
struct MeshPlan
{
	uint32_t nx, ny, nz, segs_x, tiles_y, tiles_z, entries, chunks, wgs;
};

// false: too large for the launches (int coordinates with room for a lane past the row, 32-bit entry indices, one-dimensional grids).
// voxels: the tiles and entries are dealt over the box's voxels, one more per axis than its cubes (mesh_indexed.hip); none where it has no cube
inline bool mesh_plan(VkvExtent3D e, const VkvBox &b, MeshPlan &p, bool voxels = false)
{
	if (e.width > 0x7fffff00u || e.height > 0x7fffff00u || e.depth > 0x7fffff00u)
		return false;
	p    = MeshPlan{};
	p.nx = b.width - 1, p.ny = b.height - 1, p.nz = b.depth - 1;
	const uint32_t more = voxels && p.nx && p.ny && p.nz ? 1u : 0u, cx = p.nx + more, cy = p.ny + more, cz = voxels && !more ? 0u : p.nz + more;
	p.segs_x  = (cx + kMeshTileX - 1) / kMeshTileX;
	p.tiles_y = (cy + kMeshTileY - 1) / kMeshTileY;
	p.tiles_z = (cz + kMeshSegment - 1) / kMeshSegment;
	const uint64_t entries = (uint64_t) p.segs_x * cy, wgs = (uint64_t) p.segs_x * p.tiles_y;
	if (entries > 0x7fffffffull || entries * cz > 0x7fffffffull || wgs * p.tiles_z > 0x7fffffffull)
		return false;
	p.entries = (uint32_t) (entries * cz), p.wgs = (uint32_t) (wgs * p.tiles_z);
	p.chunks  = scan_chunks(p.entries);
	return true;
}

inline MeshGeom mesh_geom(const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint8_t *d_max_map, VkvExtent3D me, const MeshPlan &p)
{
	MeshGeom G{};
	G.vol = d_vol, G.W = (int) e.width, G.H = (int) e.height, G.D = (int) e.depth;
	G.x0 = (int) b.x0, G.y0 = (int) b.y0, G.z0 = (int) b.z0, G.nx = (int) p.nx, G.ny = (int) p.ny, G.nz = (int) p.nz;
	G.segs_x = p.segs_x, G.tiles_y = p.tiles_y, G.n_wgs = p.wgs;
	G.thr = iso_threshold(iso), G.mm = MaxMap(d_max_map, e, me);
	return G;
}

// A call's scratch block, its size and its pointers from one place: [chunk sums, then sums before: u64 x chunks] x lists, then [counts: u32 x
// entries][local prefix: u32 x entries] x lists (8 bytes per entry and list), then `extra` bytes of the unit's own; rounded up to 8, at least 16
struct MeshScratch
{
	MeshPlan p;
	uint32_t lists;
	size_t   extra;
	void    *base;        // null where only the size is asked for

	size_t bytes() const
	{
		const size_t n = ((size_t) lists * (8 * (size_t) p.chunks + 8 * (size_t) p.entries) + extra + 7) & ~(size_t) 7;
		return n < 16 ? 16 : n;
	}
	uint64_t *sums(uint32_t list) const { return static_cast<uint64_t *>(base) + (size_t) list * p.chunks; }
	uint32_t *counts(uint32_t list) const { return reinterpret_cast<uint32_t *>(sums(lists)) + 2 * (size_t) list * p.entries; }
	uint32_t *local(uint32_t list) const { return counts(list) + p.entries; }
	uint8_t  *behind() const { return reinterpret_cast<uint8_t *>(counts(lists)); }
};

}        // namespace vkv

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
// No kernel uses scratch memory (tests/test_mesh_cpu.py reads the listing).
#include <algorithm>

#include "launchers.hpp"
#include "mtet_table.hpp"

using namespace vkv;

constexpr int      kMeshTileX = 256, kMeshTileY = 4;        // cubes of a workgroup per slice: 64 lanes x 4 cubes, 4 rows
constexpr int      kMeshSegment = 16;                       // slices of cubes a workgroup marches over (it loads one more)
constexpr uint32_t kMeshScanChunk = 4096;                   // entries a scan workgroup takes: 256 threads x 16
static_assert(kMeshSegment <= 64, "a wave tests its entries one per lane");

__constant__ MtetTable d_mtet = kMtetTable;

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
	uint32_t       thr;               // the smallest byte b with (float) b * kInv255 >= iso; 256: none
	const uint8_t *map;               // the max map or null
	int            bx, by, bz, mw, mh;
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

__device__ __forceinline__ uint32_t wave_sum(uint32_t n)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		n += (uint32_t) __shfl_xor((int) n, o);
	return n;
}

struct MeshTile
{
	uint32_t xs;                 // x segment
	int      xc, yc, zc0, zc1;        // the lane's first cube and its row (yc may lie past the box), the slices [zc0, zc1), relative to the box
	uint32_t e0, e_step;         // the wave's entry of slice zc0 and the step to the next slice
};

__device__ __forceinline__ MeshTile mesh_tile(const MeshGeom &G)
{
	const uint32_t t = xcd_remap(blockIdx.x, G.n_wgs), lane = threadIdx.x & 63u;
	MeshTile       T;
	T.xs     = t % G.segs_x;
	T.xc     = (int) T.xs * kMeshTileX + 4 * (int) lane;
	T.yc     = (int) ((t / G.segs_x) % G.tiles_y) * kMeshTileY + (int) (threadIdx.x >> 6);
	T.zc0    = (int) (t / (G.segs_x * G.tiles_y)) * kMeshSegment;
	T.zc1    = min(T.zc0 + kMeshSegment, G.nz);
	T.e_step = (uint32_t) G.ny * G.segs_x;
	T.e0     = ((uint32_t) T.zc0 * (uint32_t) G.ny + (uint32_t) T.yc) * G.segs_x + T.xs;
	return T;
}

// every map cell that holds a cube origin of the workgroup's tile stays below iso (workgroup-uniform; a barrier inside)
__device__ __forceinline__ bool tile_is_empty(const MeshGeom &G, const MeshTile &T)
{
	const int xa = G.x0 + (int) T.xs * kMeshTileX, xb = G.x0 + min((int) T.xs * kMeshTileX + kMeshTileX, G.nx) - 1;
	const int yt = T.yc - (int) (threadIdx.x >> 6);
	const int ya = G.y0 + yt, yb = G.y0 + min(yt + kMeshTileY, G.ny) - 1;
	const int za = G.z0 + T.zc0, zb = G.z0 + T.zc1 - 1;
	const int cx = xa / G.bx, cy = ya / G.by, cz = za / G.bz;
	const int ncx = xb / G.bx - cx + 1, ncy = yb / G.by - cy + 1, ncz = zb / G.bz - cz + 1;
	int       any = 0;
	for (int i = (int) threadIdx.x; i < ncx * ncy * ncz; i += 256)
	{
		const int ix = i % ncx, iy = (i / ncx) % ncy, iz = i / (ncx * ncy);
		any |= G.map[((size_t) (cz + iz) * (size_t) G.mh + (size_t) (cy + iy)) * (size_t) G.mw + (size_t) (cx + ix)] >= G.thr;
	}
	return !__syncthreads_or(any);
}

template <bool WIDE>
__global__ void __launch_bounds__(256) k_mesh_count(MeshGeom G, uint32_t *__restrict__ counts)
{
	__shared__ uint8_t lut[256];
	const MeshTile     T    = mesh_tile(G);
	const uint32_t     lane = threadIdx.x & 63u;
	if (G.map && tile_is_empty(G, T))
	{
		if (threadIdx.x < 4 * kMeshSegment)
		{
			const int yc = T.yc - (int) (threadIdx.x >> 6) + (int) (threadIdx.x & 3u), zc = T.zc0 + (int) (threadIdx.x >> 2);
			if (yc < G.ny && zc < T.zc1)
				counts[((uint32_t) zc * (uint32_t) G.ny + (uint32_t) yc) * G.segs_x + T.xs] = 0u;
		}
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

// exclusive scan of v over the workgroup's 256 threads (Hillis-Steele in LDS: a fixed tree), its total in `total`
template <typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T *lds, T &total)
{
	const uint32_t i = threadIdx.x;
	T              s = v;
	lds[i]           = s;
	__syncthreads();
#pragma unroll
	for (uint32_t o = 1; o < 256; o <<= 1)
	{
		const T add = i >= o ? lds[i - o] : T(0);
		__syncthreads();
		s += add;
		lds[i] = s;
		__syncthreads();
	}
	total = lds[255];
	__syncthreads();
	return s - v;
}

// chunk c = entries [4096 c, 4096 c + 4096): local[e] = the sum of the chunk's entries before e, sums[c] = the chunk's sum
__global__ void __launch_bounds__(256) k_mesh_scan_chunks(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                          uint32_t n_entries)
{
	__shared__ uint32_t lds[256];
	constexpr uint32_t  kPer = kMeshScanChunk / 256;
	const uint32_t      first = blockIdx.x * kMeshScanChunk + threadIdx.x * kPer;
	uint32_t            c[kPer], mine = 0;
#pragma unroll
	for (uint32_t k = 0; k < kPer; ++k)
	{
		c[k] = first + k < n_entries ? counts[first + k] : 0u;
		mine += c[k];
	}
	uint32_t total;
	uint32_t before = block_exclusive_scan(mine, lds, total);
#pragma unroll
	for (uint32_t k = 0; k < kPer; ++k)
	{
		if (first + k < n_entries)
			local[first + k] = before;
		before += c[k];
	}
	if (threadIdx.x == 0)
		sums[blockIdx.x] = total;
}

// one workgroup: sums[c] becomes the sum of the chunks before c; counts[0] = the total, counts[1] = min(total, capacity)
__global__ void __launch_bounds__(256) k_mesh_scan_total(uint64_t *__restrict__ sums, uint32_t n_chunks, uint64_t capacity, uint64_t *__restrict__ d_counts)
{
	__shared__ uint64_t lds[256];
	uint64_t            carry = 0;
	for (uint32_t c0 = 0; c0 < n_chunks; c0 += 256)
	{
		const uint32_t c = c0 + threadIdx.x;
		const uint64_t v = c < n_chunks ? sums[c] : 0ull;
		uint64_t       total;
		const uint64_t before = block_exclusive_scan(v, lds, total);
		if (c < n_chunks)
			sums[c] = carry + before;
		carry += total;
	}
	if (threadIdx.x == 0)
	{
		d_counts[0] = carry;
		d_counts[1] = carry < capacity ? carry : capacity;
	}
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

template <bool WIDE>
__global__ void __launch_bounds__(256) k_mesh_emit(MeshGeom G, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ local,
                                                   const uint64_t *__restrict__ chunk_before, float iso, float *__restrict__ triangles, uint64_t capacity)
{
	// the case table in LDS: a cube's walk below reads it once per tetrahedron, one after the other
	__shared__ MtetTable tab;
	static_assert(sizeof(MtetTable) == 4 * 256 && alignof(MtetTable) >= 8, "one dword per thread; a case is read as one 64-bit word");
	reinterpret_cast<uint32_t *>(&tab)[threadIdx.x] = reinterpret_cast<const uint32_t *>(&d_mtet)[threadIdx.x];
	__syncthreads();
	const MeshTile T    = mesh_tile(G);
	const uint32_t lane = threadIdx.x & 63u;
	if (T.yc >= G.ny)        // whole waves only; there is no barrier below
		return;
	// the wave's entries, one per lane: those with triangles that start below the capacity
	uint64_t start = 0;
	bool     work  = false;
	if (T.zc0 + (int) lane < T.zc1)
	{
		const uint32_t e = T.e0 + lane * T.e_step;
		start            = chunk_before[e / kMeshScanChunk] + local[e];
		work             = counts[e] != 0u && start < capacity;
	}
	uint64_t todo = __ballot(work);
	if (todo == 0)
		return;
	const int    x = G.x0 + T.xc, y = G.y0 + T.yc, nvalid = min(max(G.nx - T.xc, 0), 4);
	const size_t plane = (size_t) G.H * (size_t) G.W, row = (size_t) y * (size_t) G.W;
	while (todo)        // wave-uniform
	{
		const int k = __ffsll((long long) todo) - 1;
		todo &= todo - 1;
		const int      zc = T.zc0 + k;
		const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) start, k), hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) (start >> 32), k);
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
		uint32_t incl = mine;        // inclusive prefix over the lanes: the cubes of a row lie in lane order
#pragma unroll
		for (int o = 1; o < 64; o <<= 1)
		{
			const uint32_t up = (uint32_t) __shfl_up((int) incl, o);
			incl += lane >= (uint32_t) o ? up : 0u;
		}
		uint64_t idx = ((uint64_t) hi << 32 | lo) + (incl - mine);
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
					float *out = triangles + 9 * idx;        // 36 bytes at a 4-byte alignment: two 16-byte stores and a dword
					*reinterpret_cast<f32x4_a4 *>(out)     = f32x4_a4{v[0], v[1], v[2], v[3]};
					*reinterpret_cast<f32x4_a4 *>(out + 4) = f32x4_a4{v[4], v[5], v[6], v[7]};
					out[8]                                 = v[8];
				}
			}
		}
	}
}

namespace vkv
{

namespace
{
struct MeshPlan
{
	uint32_t nx, ny, nz, segs_x, tiles_y, tiles_z, entries, chunks, wgs;
};

// false: too large for the launches (int coordinates with room for a lane past the row, 32-bit entry indices, one-dimensional grids)
bool mesh_plan(VkvExtent3D e, const VkvBox &b, MeshPlan &p)
{
	if (e.width > 0x7fffff00u || e.height > 0x7fffff00u || e.depth > 0x7fffff00u)
		return false;
	p         = MeshPlan{};
	p.nx      = b.width - 1, p.ny = b.height - 1, p.nz = b.depth - 1;
	p.segs_x  = (p.nx + kMeshTileX - 1) / kMeshTileX;
	p.tiles_y = (p.ny + kMeshTileY - 1) / kMeshTileY;
	p.tiles_z = (p.nz + kMeshSegment - 1) / kMeshSegment;
	const uint64_t entries = (uint64_t) p.segs_x * p.ny, wgs = (uint64_t) p.segs_x * p.tiles_y;
	if (entries > 0x7fffffffull || entries * p.nz > 0x7fffffffull || wgs * p.tiles_z > 0x7fffffffull)
		return false;
	p.entries = (uint32_t) (entries * p.nz), p.wgs = (uint32_t) (wgs * p.tiles_z);
	p.chunks  = (p.entries + kMeshScanChunk - 1) / kMeshScanChunk;
	return true;
}

VkvBox whole_or(VkvExtent3D e, const VkvBox *box) { return box ? *box : VkvBox{0, 0, 0, e.width, e.height, e.depth}; }
}        // namespace

// [chunk sums, then sums before: u64 x chunks][counts: u32 x entries][local prefix: u32 x entries]; 0: the extent and box are not accepted
size_t mesh_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	if (!extent_ok(e))
		return 0;
	if (box && (box->width == 0 || box->height == 0 || box->depth == 0 || (uint64_t) box->x0 + box->width > e.width ||
	            (uint64_t) box->y0 + box->height > e.height || (uint64_t) box->z0 + box->depth > e.depth))
		return 0;
	MeshPlan p;
	if (!mesh_plan(e, whole_or(e, box), p))
		return 0;
	return std::max<size_t>(16, 8 * (size_t) p.chunks + 8 * (size_t) p.entries);
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
	uint64_t *sums   = static_cast<uint64_t *>(d_scratch);
	uint32_t *counts = reinterpret_cast<uint32_t *>(sums + p.chunks), *local = counts + p.entries;
	MeshGeom  G{};
	G.vol = d_vol, G.W = (int) e.width, G.H = (int) e.height, G.D = (int) e.depth;
	G.x0 = (int) b.x0, G.y0 = (int) b.y0, G.z0 = (int) b.z0, G.nx = (int) p.nx, G.ny = (int) p.ny, G.nz = (int) p.nz;
	G.segs_x = p.segs_x, G.tiles_y = p.tiles_y, G.n_wgs = p.wgs;
	G.thr = 0;
	while (G.thr < 256u && !((float) G.thr * kInv255 >= iso))        // the renderer's hit rule on a voxel's own value
		++G.thr;
	G.map = d_max_map, G.bx = G.by = G.bz = 1, G.mw = G.mh = 0;
	if (d_max_map)
	{
		G.bx = (int) block_of(e.width, me.width), G.by = (int) block_of(e.height, me.height), G.bz = (int) block_of(e.depth, me.depth);
		G.mw = (int) me.width, G.mh = (int) me.height;
	}
	const bool wide = e.width >= 4;        // the kernels' dword row loads
	if (p.entries)
	{
		if (wide)
			hipLaunchKernelGGL(k_mesh_count<true>, dim3(p.wgs), dim3(256), 0, s, G, counts);
		else
			hipLaunchKernelGGL(k_mesh_count<false>, dim3(p.wgs), dim3(256), 0, s, G, counts);
		hipLaunchKernelGGL(k_mesh_scan_chunks, dim3(p.chunks), dim3(256), 0, s, counts, local, sums, p.entries);
	}
	hipLaunchKernelGGL(k_mesh_scan_total, dim3(1), dim3(256), 0, s, sums, p.chunks, capacity, d_counts);
	if (p.entries && capacity)
	{
		if (wide)
			hipLaunchKernelGGL(k_mesh_emit<true>, dim3(p.wgs), dim3(256), 0, s, G, counts, local, sums, iso, d_triangles, capacity);
		else
			hipLaunchKernelGGL(k_mesh_emit<false>, dim3(p.wgs), dim3(256), 0, s, G, counts, local, sums, iso, d_triangles, capacity);
	}
	return check_launch(ctx, "isosurface_mesh");
}

}        // namespace vkv

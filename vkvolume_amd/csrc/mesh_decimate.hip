// mesh_decimate.hip — vkv_mesh_decimate: an indexed mesh decimated by vertex clustering on a regular grid.  Every vertex falls
// into a cell, a cell's vertices become their mean, a face survives iff its three cells differ.  Count, scan, emit; dword gathers; no MFMA.
//
// The input is a MESH as mesh_smooth.hip reads it: nt = min(counts[1], capacity_triangles), nv = min(counts[3], capacity_vertices), a face is USED
// iff it is one of the first nt and its three indices are below nv.  Every kernel is launched for a capacity or for the grid and takes its bounds
// from d_counts, on the device.
//
// The one unordered sum, a cell's positions, runs in 64-bit fixed point, q(x) = (int64) rint((double) x * 2^24), with integer atomics: integer
// addition is associative, so neither the order of the atomics nor how a wave groups them can change a bit.
//
// The scratch block (caller memory, mesh_decimate_bytes()), NC = the grid's cells, FB = ceil(capacity_triangles / 256) face blocks:
//   [ sums i64 x 3 NC | count u32 x NC | number u32 x NC | cell_sums u64 per 4096 cells | face_count u32 x FB | face_local u32 x FB |
//     face_sums u64 per 4096 face blocks | cell_of u32 x capacity_vertices ]
//   k_mdec_clear          sums, count and number (first the mark) = 0 for every cell
//   k_mdec_accumulate     per vertex below nv: its cell into cell_of, q(p) and 1 into the cell's sums and count.  Extractor vertices come in voxel
//                         order, so neighbouring lanes mostly hold the same cell: a wave adds up each run of equal adjacent cells with shuffles
//                         and its first lane issues the run's four atomics.  A run that goes on in the next wave simply issues again there
//   k_mdec_classify       per face: surviving iff used and its three cells differ pairwise; number[cell] = 1 for its cells (every writer stores
//                         the same value); face_count[block] = the block's surviving faces, by ballots
//   k_mdec_scan_cells     fixed_scan.hpp's chunk scan over the marks: number[cell] = the marked cells before it in its chunk, kNone if unmarked
//   k_mdec_scan_faces     scan_chunk over face_count
//   k_mdec_scan_totals    scan_total over both chunk sums, which writes the four d_out_counts
//   k_mdec_emit_vertices  per marked cell below the capacity: the mean.  k_mdec_vertex_map: per vertex below nv its cell's number
//   k_mdec_emit_faces     per surviving face below the capacity: its cells' numbers and its label
// No kernel uses scratch memory (tests/test_mesh_decimate_cpu.py reads the listing).  Every cell read back from cell_of is compared with NC before
// it indexes anything.
#include "fixed_scan.hpp"
#include "launchers.hpp"

using namespace vkv;

namespace
{

constexpr double   kFix    = 16777216.0;              // 2^24
constexpr double   kInvFix = 1.0 / 16777216.0;        // exact
constexpr uint32_t kNone   = 0xffffffffu;             // no cell (there are at most 2^32 - 1), and in `number`: no surviving face names the cell

struct ClusterGrid
{
	float    origin[3], cell[3];
	uint32_t n[3];
};

// the scratch block's regions; the same arithmetic gives mesh_decimate_bytes()
struct Decimate
{
	long long *sums;
	uint32_t * count, *number, *face_count, *face_local, *cell_of;
	uint64_t * cell_sums, *face_sums;
	uint32_t   cv, ct, nc, cell_chunks, face_blocks, face_chunks;
	size_t     bytes;
	Decimate(void *base, uint64_t capacity_vertices, uint64_t capacity_triangles, uint64_t cells)
	    : cv((uint32_t) capacity_vertices), ct((uint32_t) capacity_triangles), nc((uint32_t) cells), cell_chunks((uint32_t) ((cells + kScanChunk - 1) / kScanChunk)),
	      face_blocks((uint32_t) ((capacity_triangles + 255) / 256)), face_chunks((face_blocks + kScanChunk - 1) / kScanChunk)        // in 64 bits: 2^32 - 1 are accepted
	{
		uint8_t *p    = static_cast<uint8_t *>(base);
		size_t   at   = 0;
		auto     take = [&](size_t n) {
            uint8_t *r = p + at;
            at += n;
            return r;
		};
		sums       = reinterpret_cast<long long *>(take((size_t) nc * 24));
		count      = reinterpret_cast<uint32_t *>(take((size_t) nc * 4));
		number     = reinterpret_cast<uint32_t *>(take((size_t) nc * 4));
		cell_sums  = reinterpret_cast<uint64_t *>(take((size_t) cell_chunks * 8));
		face_count = reinterpret_cast<uint32_t *>(take((size_t) face_blocks * 4));
		face_local = reinterpret_cast<uint32_t *>(take((size_t) face_blocks * 4));
		face_sums  = reinterpret_cast<uint64_t *>(take((size_t) face_chunks * 8));
		cell_of    = reinterpret_cast<uint32_t *>(take(((size_t) cv * 4 + 7) & ~(size_t) 7));
		bytes      = at;
	}
};

__device__ __forceinline__ uint32_t written(const uint64_t *__restrict__ counts, int which, uint32_t capacity)
{
	const uint64_t n = counts[which];
	return n < capacity ? (uint32_t) n : capacity;
}

__device__ __forceinline__ uint64_t global_index() { return (uint64_t) blockIdx.x * 256u + threadIdx.x; }

__device__ __forceinline__ long long fix(float x) { return (long long) __builtin_rint((double) x * kFix); }

// one subtraction, one correctly rounded division; NaN fails the first comparison and falls to 0
__device__ __forceinline__ uint32_t cell_on_axis(float p, float origin, float cell, uint32_t n)
{
	const float d = p - origin;
	const float u = d / cell;
	return u >= 0.0f ? (u < (float) n ? (uint32_t) u : n - 1u) : 0u;
}

// whether face t survives, and its three cells
__device__ __forceinline__ bool surviving(const uint32_t *__restrict__ indices, uint64_t t, uint32_t nt, uint32_t nv, const uint32_t *__restrict__ cell_of,
                                          uint32_t nc, uint32_t c[3])
{
	if (t >= nt)
		return false;
	const uint32_t i0 = indices[3 * t], i1 = indices[3 * t + 1], i2 = indices[3 * t + 2];
	if (i0 >= nv || i1 >= nv || i2 >= nv)
		return false;
	c[0] = cell_of[i0], c[1] = cell_of[i1], c[2] = cell_of[i2];
	if (c[0] >= nc || c[1] >= nc || c[2] >= nc)        // cannot be, while the counts stand still during the call
		return false;
	return c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
}

// the workgroup's 256 flags: how many are set in the threads before this one, and in all (ballots and four wave totals through LDS: a fixed tree)
__device__ __forceinline__ uint32_t flags_before(bool flag, uint32_t &total)
{
	__shared__ uint32_t per_wave[4];
	const uint32_t      lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t      set  = __ballot(flag);
	if (lane == 0)
		per_wave[wave] = (uint32_t) __popcll(set);
	__syncthreads();
	uint32_t before = (uint32_t) __popcll(set & ((1ull << lane) - 1ull));
	total           = 0;
#pragma unroll
	for (uint32_t w = 0; w < 4; ++w)
	{
		before += w < wave ? per_wave[w] : 0u;
		total += per_wave[w];
	}
	return before;
}

}        // namespace

__global__ void __launch_bounds__(256) k_mdec_clear(long long *__restrict__ sums, uint32_t *__restrict__ count, uint32_t *__restrict__ number, uint32_t nc)
{
	const uint64_t e = global_index();
	if (e >= nc)
		return;
	sums[3 * e] = 0, sums[3 * e + 1] = 0, sums[3 * e + 2] = 0;
	count[e] = 0u, number[e] = 0u;
}

__global__ void __launch_bounds__(256) k_mdec_accumulate(const float *__restrict__ vertices, const uint64_t *__restrict__ counts, uint32_t cv, ClusterGrid g,
                                                         long long *__restrict__ sums, uint32_t *__restrict__ count, uint32_t *__restrict__ cell_of)
{
	const uint32_t nv = written(counts, 3, cv);
	if ((uint64_t) blockIdx.x * 256u >= nv)        // the whole workgroup; below, every lane of a wave stays for the shuffles
		return;
	const uint64_t v    = global_index();
	const bool     live = v < nv;
	uint32_t       c    = kNone, k = 0;
	long long      s[3] = {0, 0, 0};
	if (live)
	{
		const float p[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
		const uint32_t a = cell_on_axis(p[0], g.origin[0], g.cell[0], g.n[0]), b = cell_on_axis(p[1], g.origin[1], g.cell[1], g.n[1]);
		c                = a + g.n[0] * (b + g.n[1] * cell_on_axis(p[2], g.origin[2], g.cell[2], g.n[2]));
		cell_of[v]       = c;
		s[0] = fix(p[0]), s[1] = fix(p[1]), s[2] = fix(p[2]), k = 1;
	}
	// runs of equal adjacent cells: a lane is a head if the lane before it holds another cell; the lanes past nv hold kNone and form a run of their own
	const uint32_t lane  = threadIdx.x & 63u;
	const uint32_t left  = (uint32_t) __shfl_up((int) c, 1);
	const bool     head  = lane == 0 || left != c;
	const uint64_t heads = __ballot(head);
	if (heads != ~0ull)        // wave-uniform: some run is longer than one lane
	{
		const uint64_t later = lane == 63 ? 0ull : heads >> (lane + 1);
		const uint32_t end   = later ? lane + 1 + (uint32_t) __builtin_ctzll(later) : 64u;        // the run's end
#pragma unroll
		for (uint32_t o = 1; o < 64; o <<= 1)        // after the step for o a lane holds the sum over [lane, min(lane + 2 o, end))
		{
			const long long t0 = __shfl_down(s[0], o), t1 = __shfl_down(s[1], o), t2 = __shfl_down(s[2], o);
			const uint32_t  tk = (uint32_t) __shfl_down((int) k, o);
			if (lane + o < end)
				s[0] += t0, s[1] += t1, s[2] += t2, k += tk;
		}
	}
	if (head && live)
	{
		atomicAdd(reinterpret_cast<unsigned long long *>(sums + 3 * (size_t) c), (unsigned long long) s[0]);
		atomicAdd(reinterpret_cast<unsigned long long *>(sums + 3 * (size_t) c + 1), (unsigned long long) s[1]);
		atomicAdd(reinterpret_cast<unsigned long long *>(sums + 3 * (size_t) c + 2), (unsigned long long) s[2]);
		atomicAdd(count + c, k);
	}
}

__global__ void __launch_bounds__(256) k_mdec_classify(const uint32_t *__restrict__ indices, const uint64_t *__restrict__ counts, uint32_t cv, uint32_t ct,
                                                       const uint32_t *__restrict__ cell_of, uint32_t nc, uint32_t *__restrict__ number,
                                                       uint32_t *__restrict__ face_count)
{
	uint32_t   c[3];
	const bool keep = surviving(indices, global_index(), written(counts, 1, ct), written(counts, 3, cv), cell_of, nc, c);
	if (keep)
		number[c[0]] = 1u, number[c[1]] = 1u, number[c[2]] = 1u;
	uint32_t total;
	(void) flags_before(keep, total);
	if (threadIdx.x == 0)
		face_count[blockIdx.x] = total;
}

// scan_chunk of fixed_scan.hpp over the marks, in place: a marked cell gets the marked cells before it in its chunk, an unmarked one kNone
__global__ void __launch_bounds__(256) k_mdec_scan_cells(uint32_t *__restrict__ number, uint64_t *__restrict__ cell_sums, uint32_t nc)
{
	__shared__ uint32_t lds[256];
	constexpr uint32_t  kPer  = kScanChunk / 256;
	const uint32_t      first = blockIdx.x * kScanChunk + threadIdx.x * kPer;
	uint32_t            mark[kPer], mine = 0;
#pragma unroll
	for (uint32_t k = 0; k < kPer; ++k)
	{
		mark[k] = first + k < nc ? number[first + k] : 0u;
		mine += mark[k];
	}
	uint32_t total;
	uint32_t before = block_exclusive_scan(mine, lds, total);
#pragma unroll
	for (uint32_t k = 0; k < kPer; ++k)
	{
		if (first + k < nc)
			number[first + k] = mark[k] ? before : kNone;
		before += mark[k];
	}
	if (threadIdx.x == 0)
		cell_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) k_mdec_scan_faces(const uint32_t *__restrict__ face_count, uint32_t *__restrict__ face_local,
                                                         uint64_t *__restrict__ face_sums, uint32_t face_blocks)
{
	scan_chunk(face_count, face_local, face_sums, face_blocks);
}

// workgroup 0: the faces' chunk sums and d_out_counts[0 .. 1]; workgroup 1: the cells' and d_out_counts[2 .. 3]
__global__ void __launch_bounds__(256) k_mdec_scan_totals(uint64_t *__restrict__ face_sums, uint32_t face_chunks, uint64_t capacity_triangles,
                                                          uint64_t *__restrict__ cell_sums, uint32_t cell_chunks, uint64_t capacity_vertices,
                                                          uint64_t *__restrict__ out_counts)
{
	if (blockIdx.x == 0)
		scan_total(face_sums, face_chunks, capacity_triangles, out_counts);
	else
		scan_total(cell_sums, cell_chunks, capacity_vertices, out_counts + 2);
}

__global__ void __launch_bounds__(256) k_mdec_emit_vertices(const long long *__restrict__ sums, const uint32_t *__restrict__ count, const uint32_t *__restrict__ number,
                                                            const uint64_t *__restrict__ cell_sums, uint32_t nc, float *__restrict__ out_vertices,
                                                            uint32_t capacity)
{
	const uint64_t e = global_index();
	if (e >= nc || number[e] == kNone)
		return;
	const uint64_t at = cell_sums[e / kScanChunk] + number[e];
	if (at >= capacity)
		return;
	const double k = (double) count[e];        // at least 1: a surviving face names the cell through a vertex in it
#pragma unroll
	for (int a = 0; a < 3; ++a)
		out_vertices[3 * at + a] = (float) ((double) sums[3 * e + a] / k * kInvFix);
}

__global__ void __launch_bounds__(256) k_mdec_vertex_map(const uint64_t *__restrict__ counts, uint32_t cv, const uint32_t *__restrict__ cell_of, uint32_t nc,
                                                         const uint32_t *__restrict__ number, const uint64_t *__restrict__ cell_sums,
                                                         uint32_t *__restrict__ vertex_map)
{
	const uint64_t v = global_index();
	if (v >= written(counts, 3, cv))
		return;
	const uint32_t c = cell_of[v];
	vertex_map[v]    = c < nc && number[c] != kNone ? (uint32_t) (cell_sums[c / kScanChunk] + number[c]) : kNone;
}

__global__ void __launch_bounds__(256) k_mdec_emit_faces(const uint32_t *__restrict__ indices, const uint32_t *__restrict__ triangle_labels,
                                                         const uint64_t *__restrict__ counts, uint32_t cv, uint32_t ct, const uint32_t *__restrict__ cell_of,
                                                         uint32_t nc, const uint32_t *__restrict__ number, const uint64_t *__restrict__ cell_sums,
                                                         const uint32_t *__restrict__ face_local, const uint64_t *__restrict__ face_sums,
                                                         uint32_t *__restrict__ out_indices, uint32_t *__restrict__ out_triangle_labels, uint32_t capacity)
{
	const uint64_t t = global_index();
	uint32_t       c[3], total;
	const bool     keep   = surviving(indices, t, written(counts, 1, ct), written(counts, 3, cv), cell_of, nc, c);
	const uint32_t before = flags_before(keep, total);
	if (!keep)
		return;
	const uint64_t at = face_sums[blockIdx.x / kScanChunk] + face_local[blockIdx.x] + before;
	if (at >= capacity)
		return;
#pragma unroll
	for (int j = 0; j < 3; ++j)
		out_indices[3 * at + j] = (uint32_t) (cell_sums[c[j] / kScanChunk] + number[c[j]]);        // the full numbering mod 2^32
	if (triangle_labels)
		out_triangle_labels[at] = triangle_labels[t];
}

namespace vkv
{

// the grid's cells; 0 for a zero axis or more than 2^32 - 1 of them
uint64_t mesh_decimate_cells(VkvExtent3D grid)
{
	if (grid.width == 0 || grid.height == 0 || grid.depth == 0)
		return 0;
	const uint64_t xy = (uint64_t) grid.width * grid.height;
	if (xy > 0xffffffffull || xy * grid.depth > 0xffffffffull)
		return 0;
	return xy * grid.depth;
}

// 32 per cell + 8 per 4096 cells + 8 per 256 triangles + 8 per 4096 x 256 triangles + 4 per vertex, rounded up to 8
size_t mesh_decimate_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles, VkvExtent3D grid)
{
	const uint64_t cells = mesh_decimate_cells(grid);
	if (capacity_vertices > 0xffffffffull || capacity_triangles > 0xffffffffull || cells == 0)
		return 0;
	return Decimate(nullptr, capacity_vertices, capacity_triangles, cells).bytes;
}

static uint32_t blocks_for(uint32_t n) { return (uint32_t) (((uint64_t) n + 255u) / 256u); }

int launch_mesh_decimate(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint64_t capacity_vertices,
                         uint64_t capacity_triangles, const uint64_t *d_counts, const float *grid_origin, const float *grid_cell, VkvExtent3D grid,
                         void *d_scratch, float *d_out_vertices, uint64_t out_capacity_vertices, uint32_t *d_out_indices, uint32_t *d_out_triangle_labels,
                         uint64_t out_capacity_triangles, uint32_t *d_vertex_map, uint64_t *d_out_counts, hipStream_t s)
{
	const Decimate D(d_scratch, capacity_vertices, capacity_triangles, mesh_decimate_cells(grid));
	ClusterGrid    g;
	for (int a = 0; a < 3; ++a)
		g.origin[a] = grid_origin[a], g.cell[a] = grid_cell[a];
	g.n[0] = grid.width, g.n[1] = grid.height, g.n[2] = grid.depth;
	const uint32_t out_cv = (uint32_t) out_capacity_vertices, out_ct = (uint32_t) out_capacity_triangles;
	hipLaunchKernelGGL(k_mdec_clear, dim3(blocks_for(D.nc)), dim3(256), 0, s, D.sums, D.count, D.number, D.nc);
	if (D.cv)
		hipLaunchKernelGGL(k_mdec_accumulate, dim3(blocks_for(D.cv)), dim3(256), 0, s, d_vertices, d_counts, D.cv, g, D.sums, D.count, D.cell_of);
	if (D.ct)
	{
		hipLaunchKernelGGL(k_mdec_classify, dim3(D.face_blocks), dim3(256), 0, s, d_indices, d_counts, D.cv, D.ct, D.cell_of, D.nc, D.number, D.face_count);
		hipLaunchKernelGGL(k_mdec_scan_faces, dim3(D.face_chunks), dim3(256), 0, s, D.face_count, D.face_local, D.face_sums, D.face_blocks);
	}
	hipLaunchKernelGGL(k_mdec_scan_cells, dim3(D.cell_chunks), dim3(256), 0, s, D.number, D.cell_sums, D.nc);
	hipLaunchKernelGGL(k_mdec_scan_totals, dim3(2), dim3(256), 0, s, D.face_sums, D.face_chunks, out_capacity_triangles, D.cell_sums, D.cell_chunks,
	                   out_capacity_vertices, d_out_counts);
	if (out_cv)
		hipLaunchKernelGGL(k_mdec_emit_vertices, dim3(blocks_for(D.nc)), dim3(256), 0, s, D.sums, D.count, D.number, D.cell_sums, D.nc, d_out_vertices, out_cv);
	if (d_vertex_map && D.cv)
		hipLaunchKernelGGL(k_mdec_vertex_map, dim3(blocks_for(D.cv)), dim3(256), 0, s, d_counts, D.cv, D.cell_of, D.nc, D.number, D.cell_sums, d_vertex_map);
	if (out_ct && D.ct)
		hipLaunchKernelGGL(k_mdec_emit_faces, dim3(D.face_blocks), dim3(256), 0, s, d_indices, d_triangle_labels, d_counts, D.cv, D.ct, D.cell_of, D.nc, D.number,
		                   D.cell_sums, D.face_local, D.face_sums, d_out_indices, d_out_triangle_labels, out_ct);
	return check_launch(ctx, "mesh_decimate");
}

}        // namespace vkv

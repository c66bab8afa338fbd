// mesh_smooth.hip — what is done to an indexed mesh after its extraction (vkv_mesh_adjacency, vkv_mesh_smooth, vkv_mesh_vertex_normals, DESIGN.md
// §5.24): the vertex adjacency of the used faces, built once per mesh; uniform-umbrella (Laplacian, Taubin lambda | mu) passes over it; and
// area-weighted vertex normals from the faces, of all faces or of one body's.  Dword gathers; no MFMA.
//
// A mesh is d_vertices (3 floats per vertex), d_indices (3 uint32 per triangle) and the four d_counts of the indexed extractors, read HERE, on
// the device: nt = min(counts[1], capacity_triangles), nv = min(counts[3], capacity_vertices), a face is USED iff it is one of the first nt and
// its three indices are below nv.  Every kernel is launched for the capacities and takes its bounds from d_counts.
//
// The sums over a vertex's neighbours and faces run in 64-bit fixed point, q(x) = (int64) rint((double) x * 2^24): integer addition is
// associative, so the order in which a segment lists them cannot change a bit, and no floating-point atomic appears.  The integer atomics of
// the build (a count and a fill cursor per vertex) decide only the order INSIDE a segment, which the sort then fixes.
//
// The adjacency block (caller memory, mesh_adjacency_bytes()):
//   [ head 4 x u64 | sums u64 per scan chunk | faces_of u32 x CV | local u32 x CV | degree u32 x CV | neighbours u32 x 6 CT | faces u32 x 3 CT ]
// head = { the corners of used faces, the same, CV, CT }.  Vertex v's segment starts at start(v) = sums[v / 4096] + local[v] in units of one
// corner: faces[start .. start + faces_of[v]) are its used faces, rising; neighbours[2 start .. 2 start + degree[v]) its neighbour set, rising
// (each corner brings the face's two other vertices; after the sort, duplicates and v itself are gone).  Everything that depends on CT lies
// behind what the smoothing pass reads, which is given CV alone.
//   k_madj_clear     faces_of and degree (the fill cursor) = 0 for the capacity, the head's two capacities
//   k_madj_faces     <false>: per used face an integer atomic add to each corner's faces_of
//   k_madj_scan_*    the fixed-tree scans of fixed_scan.hpp over faces_of
//   k_madj_faces     <true>: per used face and corner a slot from the vertex's cursor, the face and the two other vertices into it
//   k_madj_sort      per vertex: insertion sort of both segments, then the neighbours made a set; degree[v] = k(v).  Quadratic in the vertex's
//                    number of faces, by one lane: segments are short (at most 14 away from junctions in the extractors' meshes), and up to
//                    16 faces are sorted in the lane's column of LDS, more where they lie
//   k_msmooth_pass   per vertex: the gather of one pass.  k_msmooth_copy: the odd pass count's result back into d_vertices
//   k_mnormals       per vertex: the gather over its faces
// No kernel uses scratch memory (tests/test_mesh_smooth_cpu.py reads the listing).  A block built for other capacities, or changed counts,
// give unspecified values but no access outside a buffer: every index read from memory is compared with its bound before it is used.
#include "fixed_scan.hpp"
#include "launchers.hpp"

using namespace vkv;

namespace
{

constexpr double kFix    = 16777216.0;              // 2^24
constexpr double kInvFix = 1.0 / 16777216.0;        // exact

// the adjacency block's regions; the same arithmetic gives mesh_adjacency_bytes()
struct Adjacency
{
	uint64_t *head, *sums;
	uint32_t *faces_of, *local, *degree, *neighbours, *faces;
	uint32_t  cv, ct, chunks;
	size_t    bytes;
	Adjacency(void *base, uint64_t capacity_vertices, uint64_t capacity_triangles)
	    : cv((uint32_t) capacity_vertices), ct((uint32_t) capacity_triangles), chunks((uint32_t) ((capacity_vertices + kScanChunk - 1) / kScanChunk))        // in 64 bits: 2^32 - 1 vertices are accepted
	{
		const size_t per_vertex = ((size_t) cv * 4 + 7) & ~(size_t) 7;
		uint8_t *    p          = static_cast<uint8_t *>(base);
		size_t       at         = 0;
		auto         take       = [&](size_t n) {
            uint8_t *r = p + at;
            at += n;
            return r;
		};
		head       = reinterpret_cast<uint64_t *>(take(32));
		sums       = reinterpret_cast<uint64_t *>(take((size_t) chunks * 8));
		faces_of   = reinterpret_cast<uint32_t *>(take(per_vertex));
		local      = reinterpret_cast<uint32_t *>(take(per_vertex));
		degree     = reinterpret_cast<uint32_t *>(take(per_vertex));
		neighbours = reinterpret_cast<uint32_t *>(take((size_t) ct * 24));
		faces      = reinterpret_cast<uint32_t *>(take(((size_t) ct * 12 + 7) & ~(size_t) 7));
		bytes      = at;
	}
};

// what a gather kernel takes of the block
struct AdjacencyView
{
	const uint64_t *head, *sums;
	const uint32_t *faces_of, *local, *degree, *neighbours, *faces;
	uint32_t        cv, ct;
};

AdjacencyView view_of(const Adjacency &A) { return {A.head, A.sums, A.faces_of, A.local, A.degree, A.neighbours, A.faces, A.cv, A.ct}; }

__device__ __forceinline__ uint32_t written(const uint64_t *__restrict__ counts, int which, uint32_t capacity)
{
	const uint64_t n = counts[which];
	return n < capacity ? (uint32_t) n : capacity;
}

__device__ __forceinline__ uint64_t global_index() { return (uint64_t) blockIdx.x * 256u + threadIdx.x; }

__device__ __forceinline__ long long fix(float x) { return (long long) __builtin_rint((double) x * kFix); }

__device__ __forceinline__ float unfix(long long s) { return (float) ((double) s * kInvFix); }

// the block was built for these capacities (else its regions lie elsewhere)
__device__ __forceinline__ bool same_capacities(const AdjacencyView &A) { return A.head[2] == A.cv && A.head[3] == A.ct; }

__device__ __forceinline__ uint64_t least(uint64_t a, uint64_t b) { return a < b ? a : b; }

// start(v) in corners
__device__ __forceinline__ uint64_t segment_start(const AdjacencyView &A, uint32_t v) { return A.sums[v / kScanChunk] + A.local[v]; }

}        // namespace

__global__ void __launch_bounds__(256) k_madj_clear(uint32_t *__restrict__ faces_of, uint32_t *__restrict__ cursor, uint64_t *__restrict__ head, uint32_t cv,
                                                    uint32_t ct)
{
	const uint64_t v = global_index();
	if (v < cv)
		faces_of[v] = 0u, cursor[v] = 0u;
	if (v == 0)
		head[2] = cv, head[3] = ct;
}

// FILL false: faces_of[corner] += 1 per used face; true: the face and the corner's two other vertices into the corner's next slot
template <bool FILL>
__global__ void __launch_bounds__(256) k_madj_faces(const uint32_t *__restrict__ indices, const uint64_t *__restrict__ counts, uint32_t cv, uint32_t ct,
                                                    uint32_t *__restrict__ faces_of, const uint64_t *__restrict__ sums, const uint32_t *__restrict__ local,
                                                    uint32_t *__restrict__ cursor, uint32_t *__restrict__ neighbours, uint32_t *__restrict__ faces)
{
	const uint64_t t = global_index();
	if (t >= written(counts, 1, ct))
		return;
	const uint32_t nv = written(counts, 3, cv);
	const uint32_t i[3] = {indices[3 * t], indices[3 * t + 1], indices[3 * t + 2]};
	if (i[0] >= nv || i[1] >= nv || i[2] >= nv)
		return;
#pragma unroll
	for (int c = 0; c < 3; ++c)
	{
		if (!FILL)
		{
			atomicAdd(&faces_of[i[c]], 1u);
			continue;
		}
		const uint64_t at = sums[i[c] / kScanChunk] + local[i[c]] + atomicAdd(&cursor[i[c]], 1u);
		if (at >= 3ull * ct)        // cannot be, while the counts stand still between the two passes
			continue;
		faces[at]              = (uint32_t) t;
		neighbours[2 * at]     = i[(c + 1) % 3];
		neighbours[2 * at + 1] = i[(c + 2) % 3];
	}
}

__global__ void __launch_bounds__(256) k_madj_scan_chunks(const uint32_t *__restrict__ faces_of, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                          uint32_t cv)
{
	scan_chunk(faces_of, local, sums, cv);
}

__global__ void __launch_bounds__(256) k_madj_scan_total(uint64_t *__restrict__ sums, uint32_t chunks, uint64_t *__restrict__ head)
{
	scan_total(sums, chunks, ~0ull, head);
}

constexpr uint32_t kSortSlots = 32;        // the slots of a segment that a lane sorts in LDS: up to 16 faces, their 32 neighbour slots

// a lane's column of the workgroup's LDS block: element i of every lane in one row, so the lanes of a wave never share a bank
struct Column
{
	uint32_t *p;
	__device__ __forceinline__ uint32_t &operator[](uint32_t i) const { return p[i * 256u]; }
};

// ascending insertion sort of a[0 .. n) in place (a: a pointer into global memory or a Column)
template <typename Slots>
__device__ __forceinline__ void sort_segment(Slots a, uint32_t n)
{
	for (uint32_t i = 1; i < n; ++i)
	{
		const uint32_t x = a[i];
		uint32_t       j = i;
		for (; j > 0 && a[j - 1] > x; --j)
			a[j] = a[j - 1];
		a[j] = x;
	}
}

// the sorted a[0 .. n) made a set without v, in place; the slots behind it keep what they hold.  Returns its size
template <typename Slots>
__device__ __forceinline__ uint32_t make_set(Slots a, uint32_t n, uint32_t v)
{
	uint32_t k = 0;
	for (uint32_t i = 0; i < n; ++i)        // rising: a repeated neighbour follows itself
	{
		const uint32_t u = a[i];
		if (u == v || (k > 0 && a[k - 1] == u))
			continue;
		a[k++] = u;
	}
	return k;
}

// A segment of up to kSortSlots neighbour slots is sorted in the lane's LDS column (the dependent loads and stores of an insertion sort at
// LDS latency), a longer one where it lies, with the same result
__global__ void __launch_bounds__(256) k_madj_sort(const uint64_t *__restrict__ counts, uint32_t cv, uint32_t ct, const uint32_t *__restrict__ faces_of,
                                                   const uint64_t *__restrict__ sums, const uint32_t *__restrict__ local, uint32_t *__restrict__ degree,
                                                   uint32_t *__restrict__ neighbours, uint32_t *__restrict__ faces)
{
	__shared__ uint32_t lds[kSortSlots * 256];
	const uint64_t      v = global_index();
	if (v >= written(counts, 3, cv))        // there is no barrier below: a lane works in its own column
		return;
	const uint64_t start = sums[v / kScanChunk] + local[v], room = 3ull * ct;
	const uint32_t n     = start < room ? (uint32_t) least(faces_of[v], room - start) : 0u;
	uint32_t *     fa = faces + start, *nb = neighbours + 2 * start;
	uint32_t       k;
	if (2 * n <= kSortSlots)
	{
		const Column col{lds + threadIdx.x};
		for (uint32_t i = 0; i < n; ++i)
			col[i] = fa[i];
		sort_segment(col, n);
		for (uint32_t i = 0; i < n; ++i)
			fa[i] = col[i];
		for (uint32_t i = 0; i < 2 * n; ++i)
			col[i] = nb[i];
		sort_segment(col, 2 * n);
		k = make_set(col, 2 * n, (uint32_t) v);
		for (uint32_t i = 0; i < 2 * n; ++i)
			nb[i] = col[i];
	}
	else
	{
		sort_segment(fa, n);
		sort_segment(nb, 2 * n);
		k = make_set(nb, 2 * n, (uint32_t) v);
	}
	degree[v] = k;
}

// One Jacobi pass: dst[v] = src[v] + f (mean of src over N(v) - src[v]), the mean through the fixed-point sum; a vertex without neighbours
// or with pinned[v] != 0 keeps its bits
__global__ void __launch_bounds__(256) k_msmooth_pass(const float *__restrict__ src, float *__restrict__ dst, AdjacencyView A, const uint64_t *__restrict__ counts,
                                                      const uint8_t *__restrict__ pinned, float f)
{
	const uint64_t v  = global_index();
	const uint32_t nv = written(counts, 3, A.cv);
	if (v >= nv || A.head[2] != A.cv)
		return;
	float          p[3] = {src[3 * v], src[3 * v + 1], src[3 * v + 2]};
	const uint64_t room = 2 * least(A.head[0], 3 * A.head[3]), first = 2 * segment_start(A, (uint32_t) v);        // in neighbour slots
	const uint32_t k    = first < room ? (uint32_t) least(A.degree[v], room - first) : 0u;
	if (k != 0 && !(pinned && pinned[v]))
	{
		const uint32_t *nb = A.neighbours + first;
		long long       s[3] = {0, 0, 0};
		bool            ok = true;
		for (uint32_t i = 0; i < k; ++i)
		{
			uint32_t u = nb[i];
			if (u >= nv)        // cannot be in a block built from these counts: the vertex then stays
				ok = false, u = (uint32_t) v;
			s[0] += fix(src[3 * (size_t) u]), s[1] += fix(src[3 * (size_t) u + 1]), s[2] += fix(src[3 * (size_t) u + 2]);
		}
		if (ok)
		{
#pragma unroll
			for (int c = 0; c < 3; ++c)
			{
				const float m = (float) ((double) s[c] / (double) k * kInvFix);
				const float d = m - p[c];
				const float g = f * d;
				p[c]          = p[c] + g;
			}
		}
	}
	dst[3 * v] = p[0], dst[3 * v + 1] = p[1], dst[3 * v + 2] = p[2];
}

__global__ void __launch_bounds__(256) k_msmooth_copy(const float *__restrict__ src, float *__restrict__ dst, const uint64_t *__restrict__ counts, uint32_t cv)
{
	const uint64_t v = global_index();
	if (v >= written(counts, 3, cv))
		return;
	dst[3 * v] = src[3 * v], dst[3 * v + 1] = src[3 * v + 1], dst[3 * v + 2] = src[3 * v + 2];
}

// N(v) = the fixed-point sum of (p1 - p0) x (p2 - p0) over v's used faces (FILTER: those with triangle_labels[face] == label)
template <bool FILTER>
__global__ void __launch_bounds__(256) k_mnormals(const float *__restrict__ vertices, const uint32_t *__restrict__ indices,
                                                  const uint32_t *__restrict__ triangle_labels, uint32_t label, AdjacencyView A,
                                                  const uint64_t *__restrict__ counts, float *__restrict__ normals)
{
	const uint64_t v  = global_index();
	const uint32_t nv = written(counts, 3, A.cv), nt = written(counts, 1, A.ct);
	if (v >= nv || !same_capacities(A))
		return;
	const uint64_t start = segment_start(A, (uint32_t) v), room = least(A.head[0], 3ull * A.ct);
	const uint32_t n     = start < room ? (uint32_t) least(A.faces_of[v], room - start) : 0u;
	const uint32_t *fs   = A.faces + start;
	long long       s[3] = {0, 0, 0};
	for (uint32_t i = 0; i < n; ++i)
	{
		const uint32_t t = fs[i];
		if (t >= nt || (FILTER && triangle_labels[t] != label))
			continue;
		const uint32_t i0 = indices[3 * (size_t) t], i1 = indices[3 * (size_t) t + 1], i2 = indices[3 * (size_t) t + 2];
		if (i0 >= nv || i1 >= nv || i2 >= nv)
			continue;
		const float *p0 = vertices + 3 * (size_t) i0, *p1 = vertices + 3 * (size_t) i1, *p2 = vertices + 3 * (size_t) i2;
		const float  ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];        // e1
		const float  bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];        // e2
		// each component: two products, then one subtraction (no FMA: -ffp-contract=off)
		const float yz = ay * bz, zy = az * by, zx = az * bx, xz = ax * bz, xy = ax * by, yx = ay * bx;
		s[0] += fix(yz - zy), s[1] += fix(zx - xz), s[2] += fix(xy - yx);
	}
	normals[3 * v] = unfix(s[0]), normals[3 * v + 1] = unfix(s[1]), normals[3 * v + 2] = unfix(s[2]);
}

namespace vkv
{

// 32 + 8 per 4096 vertices + 3 x (4 per vertex, rounded up to 8) + 24 per triangle + 12 per triangle, rounded up to 8
size_t mesh_adjacency_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles)
{
	if (capacity_vertices > 0xffffffffull || capacity_triangles > 0xffffffffull)
		return 0;
	return Adjacency(nullptr, capacity_vertices, capacity_triangles).bytes;
}

static uint32_t blocks_for(uint32_t n) { return (uint32_t) (((uint64_t) n + 255u) / 256u); }

int launch_mesh_adjacency(vkv_ctx *ctx, const uint32_t *d_indices, uint64_t capacity_triangles, uint64_t capacity_vertices, const uint64_t *d_counts,
                          void *d_adjacency, hipStream_t s)
{
	const Adjacency A(d_adjacency, capacity_vertices, capacity_triangles);
	hipLaunchKernelGGL(k_madj_clear, dim3(A.cv ? blocks_for(A.cv) : 1u), dim3(256), 0, s, A.faces_of, A.degree, A.head, A.cv, A.ct);
	if (A.ct && A.cv)
		hipLaunchKernelGGL(k_madj_faces<false>, dim3(blocks_for(A.ct)), dim3(256), 0, s, d_indices, d_counts, A.cv, A.ct, A.faces_of, A.sums, A.local, A.degree,
		                   A.neighbours, A.faces);
	if (A.cv)
		hipLaunchKernelGGL(k_madj_scan_chunks, dim3(A.chunks), dim3(256), 0, s, A.faces_of, A.local, A.sums, A.cv);
	hipLaunchKernelGGL(k_madj_scan_total, dim3(1), dim3(256), 0, s, A.sums, A.chunks, A.head);
	if (A.ct && A.cv)
		hipLaunchKernelGGL(k_madj_faces<true>, dim3(blocks_for(A.ct)), dim3(256), 0, s, d_indices, d_counts, A.cv, A.ct, A.faces_of, A.sums, A.local, A.degree,
		                   A.neighbours, A.faces);
	if (A.cv)
		hipLaunchKernelGGL(k_madj_sort, dim3(blocks_for(A.cv)), dim3(256), 0, s, d_counts, A.cv, A.ct, A.faces_of, A.sums, A.local, A.degree, A.neighbours, A.faces);
	return check_launch(ctx, "mesh_adjacency");
}

int launch_mesh_smooth(vkv_ctx *ctx, float *d_vertices, float *d_swap, uint64_t capacity_vertices, const uint64_t *d_counts, const void *d_adjacency,
                       const uint8_t *d_pinned, const float *factors, uint32_t n_passes, hipStream_t s)
{
	// the smoothing pass reads nothing that lies behind the per-vertex regions, so the triangles' capacity is not needed to find them
	const Adjacency     A(const_cast<void *>(d_adjacency), capacity_vertices, 0);
	const AdjacencyView V = view_of(A);
	if (A.cv == 0)
		return VKV_OK;
	float *src = d_vertices, *dst = d_swap;
	for (uint32_t i = 0; i < n_passes; ++i)
	{
		hipLaunchKernelGGL(k_msmooth_pass, dim3(blocks_for(A.cv)), dim3(256), 0, s, src, dst, V, d_counts, d_pinned, factors[i]);
		float *t = src;
		src = dst, dst = t;
	}
	if (src != d_vertices)
		hipLaunchKernelGGL(k_msmooth_copy, dim3(blocks_for(A.cv)), dim3(256), 0, s, d_swap, d_vertices, d_counts, A.cv);
	return check_launch(ctx, "mesh_smooth");
}

int launch_mesh_vertex_normals(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint32_t label,
                               uint64_t capacity_vertices, uint64_t capacity_triangles, const uint64_t *d_counts, const void *d_adjacency, float *d_normals,
                               hipStream_t s)
{
	const Adjacency     A(const_cast<void *>(d_adjacency), capacity_vertices, capacity_triangles);
	const AdjacencyView V = view_of(A);
	if (A.cv == 0)
		return VKV_OK;
	if (d_triangle_labels)
		hipLaunchKernelGGL(k_mnormals<true>, dim3(blocks_for(A.cv)), dim3(256), 0, s, d_vertices, d_indices, d_triangle_labels, label, V, d_counts, d_normals);
	else
		hipLaunchKernelGGL(k_mnormals<false>, dim3(blocks_for(A.cv)), dim3(256), 0, s, d_vertices, d_indices, d_triangle_labels, label, V, d_counts, d_normals);
	return check_launch(ctx, "mesh_normals");
}

}        // namespace vkv

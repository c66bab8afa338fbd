// components.hip — connected components of the inside voxels of a box (vkv_label_components) and the size filter on them
// (vkv_select_components); DESIGN.md §5.15.  Integer work on bytes and labels; no MFMA, no floating point after the threshold.
//
// A voxel is inside iff byte >= thr (iso_threshold(iso): the mesh's inside rule).  Every kernel is one-dimensional over the box-linear index
// of box_domain.hpp, i = ((z - z0) bh + (y - y0)) bw + (x - x0), one voxel per lane; a wave's 64 voxels are one ENTRY (the tile:
// 64 x 1 x 1, wrapping over rows where the box is narrower).  d_labels doubles as the union-find's parent array until the last two kernels:
// parent[i] is the box-linear index of an ancestor of i in i's component; an outside voxel's cell holds its final 0 from the first kernel on and
// is never read: who is inside is told by the inside bits.
//   k_cc_init         inside bits by wave ballot (one 64-bit word per entry, in scratch); parent[i] = the first voxel of i's x-run inside
//                     the entry (a run of 64 inside voxels is linked without a single union), 0 for outside voxels.
//   k_cc_merge<CONN>  the unions that are left: the x seam between entries, and for every other forward offset o of the neighbourhood
//                     (2, 6 or 12) the pairs (v, v + o) that START an x-run of such pairs: where (v - ex, v - ex + o) is a pair too, v ~ v - ex
//                     and v + o ~ v - ex + o already hold along x, so that pair's union covers this one.  Lock-free union-find with atomicMin.
//   k_cc_flatten      parent[i] = find(i) for inside voxels; the root bits (parent[i] == i) by ballot, one more word per entry; per entry the
//                     number of roots and of inside voxels.
//   k_cc_scan_*       the fixed-tree scans of fixed_scan.hpp over the entries' root counts; K, min(K, capacity) and the inside count.
//   k_cc_rank_roots   a root's label is 1 + the roots before it: its entry's scan + the root bits below its lane.  Also zeroes the sizes.
//   k_cc_relabel      inside non-roots (by the two bit words) read their root's cell; sizes: a wave walks 32 entries, carries one pending
//                     (label, count) across them and adds the other labels once per entry: integer atomicAdd, far fewer than voxels or
//                     runs.  Where nothing is inside, the last three kernels touch no label at all.
//
// TERMINATION.  parent[i] <= i always: k_cc_init writes a run start <= i, atomicMin only lowers a cell (the union's hook and the path
// compression of cc_find_compress(), which writes a root found above i), k_cc_flatten stores find() <= the old value.  cc_find() follows a cell only to a strictly smaller index, and cc_union() ends or replaces its larger root a by a value < a:
// every loop strictly descends in the integers >= 0 and so ends, whatever other lanes do meanwhile.  No lane waits for another lane, wave or
// workgroup: no flag, no cross-workgroup barrier, no persistent kernel.
// COHERENCE.  Inside k_cc_merge and k_cc_flatten workgroups on different XCDs (separate L2s) touch the same parent cells: every read there
// is a relaxed agent-scope atomic load and every write an agent-scope atomic (min or store), so no value comes stale from another XCD's L2.
// Even a stale value would be a former content of the cell, i.e. an ancestor in the same component with a smaller index: find() from it
// still ends at a node of the component, and a union only ends on `old == a` (atomicMin returns the cell's true old content: a was a root
// and now hangs below b) or on a == b; otherwise it retries from the true old content.  Kernel boundaries order everything else.
// DETERMINISM.  The partition into components is unique, flattening makes parent[i] the component's smallest index (its first voxel),
// numbering is the rank of that voxel, sizes are integer sums: the bytes do not depend on the schedule.
// No kernel uses scratch memory (tests/test_components_cpu.py reads the listing).
#include <algorithm>

#include "box_domain.hpp"
#include "fixed_scan.hpp"

using namespace vkv;

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void     cc_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t cc_min(uint32_t *p, uint32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above i as far as this lane can see; every step goes to a strictly smaller index
__device__ __forceinline__ uint32_t cc_find(const uint32_t *parent, uint32_t i)
{
	for (;;)
	{
		const uint32_t a = cc_load(parent + i);
		if (a >= i)
			return i;
		i = a;
	}
}

// cc_find() that leaves i pointing at the root it found where the walk took more than one step: the root is an ancestor of i with a smaller
// index than the cell's content, so the cell only falls and parent[i] <= i holds; chains stay short however the roots were hooked
__device__ __forceinline__ uint32_t cc_find_compress(uint32_t *parent, uint32_t i)
{
	const uint32_t a = cc_load(parent + i);
	if (a >= i)
		return i;
	const uint32_t r = cc_find(parent, a);
	if (r != a)
		cc_min(parent + i, r);
	return r;
}

// joins the components of a and b: the larger root is hung below the smaller; a + b strictly falls from one round to the next
__device__ __forceinline__ void cc_union(uint32_t *parent, uint32_t a, uint32_t b)
{
	for (;;)
	{
		a = cc_find_compress(parent, a), b = cc_find_compress(parent, b);
		if (a == b)
			return;
		if (a < b)
		{
			const uint32_t t = a;
			a = b, b = t;
		}
		const uint32_t old = cc_min(parent + a, b);
		if (old >= a)        // a was a root (old == a) and now hangs below b
			return;
		a = old;        // somebody hung a below old < a meanwhile; the cell now holds min(old, b), and old and b are still to be joined
	}
}

__device__ __forceinline__ bool cc_bit(const uint64_t *bits, uint32_t j) { return (bits[j >> 6] >> (j & 63u)) & 1ull; }

__global__ void __launch_bounds__(256) k_cc_init(BoxLinear G, MaxMap M, uint32_t *__restrict__ parent, uint64_t *__restrict__ bits)
{
	const BoxVoxel v  = box_voxel(G);
	bool           in = false;
	if (v.valid)
	{
		bool look = true;
		if (M.map)        // a cell whose maximum stays below thr holds no inside voxel: none of its voxels is read
			look = M.map[M.cell_of(G.x0 + v.x, G.y0 + v.y, G.z0 + v.z)] >= G.thr;
		if (look)
			in = G.vol[box_address(G, v)] >= G.thr;
	}
	const uint64_t m      = __ballot(in);
	const uint64_t starts = (m & ~(m << 1)) | __ballot(in && v.x == 0);        // a run ends with its row
	if (v.valid)
	{
		uint32_t p = 0u;        // an outside voxel's label; nothing reads or writes the cell again
		if (in)
		{
			const uint64_t below = starts & (~0ull >> (63u - v.lane));        // never zero: a run's first voxel is a start
			p                    = v.i - (v.lane - (63u - (uint32_t) __clzll((long long) below)));
		}
		parent[v.i] = p;
		if (v.lane == 0)
			bits[v.i >> 6] = m;
	}
}

// the forward half of the neighbourhood without (1, 0, 0): the offsets whose voxel lies behind v in memory order
template <int CONN>
__device__ __forceinline__ constexpr bool cc_offset(int dx, int dy, int dz)
{
	const bool forward = dz > 0 || (dz == 0 && (dy > 0 || (dy == 0 && dx > 0)));
	if (!forward || (dx == 1 && dy == 0 && dz == 0))
		return false;
	if (CONN == VKV_CONNECT_6)
		return (dx != 0) + (dy != 0) + (dz != 0) == 1;
	if (CONN == VKV_CONNECT_14)
		return dx >= 0 && dy >= 0 && dz >= 0;
	return true;
}

template <int CONN>
__global__ void __launch_bounds__(256) k_cc_merge(BoxLinear G, uint32_t *parent, const uint64_t *__restrict__ bits)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid || !cc_bit(bits, v.i))        // no wave-wide operation below
		return;
	if (v.lane == 0 && v.x > 0 && cc_bit(bits, v.i - 1u))        // the x seam: the run goes on in the entry before
		cc_union(parent, v.i, v.i - 1u);
	const bool left = v.x > 0 && cc_bit(bits, v.i - 1u);
#pragma unroll
	for (int dz = 0; dz <= 1; ++dz)
#pragma unroll
		for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
			for (int dx = -1; dx <= 1; ++dx)
			{
				if (!cc_offset<CONN>(dx, dy, dz))
					continue;
				if ((dy < 0 && v.y == 0) || (dy > 0 && v.y + 1u >= G.bh) || (dz > 0 && v.z + 1u >= G.bd) || (dx < 0 && v.x == 0) || (dx > 0 && v.x + 1u >= G.bw))
					continue;        // connections run through the box only
				const uint32_t j = v.i + (uint32_t) dx + (uint32_t) dy * G.bw + (uint32_t) dz * G.bw * G.bh;        // mod 2^32; j lies in the box
				if (!cc_bit(bits, j))
					continue;
				// (v - ex, v - ex + o) is a pair as well: its union covers this one
				if (left && (int) v.x + dx > 0 && cc_bit(bits, j - 1u))
					continue;
				cc_union(parent, v.i, j);
			}
}

__global__ void __launch_bounds__(256) k_cc_flatten(uint32_t n, uint32_t *parent, const uint64_t *__restrict__ bits, uint64_t *__restrict__ root_bits,
                                                    uint32_t *__restrict__ counts)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
	const uint64_t ins = i < n ? bits[i >> 6] : 0ull;        // the entry's inside bits: an outside voxel's cell is not read
	bool           root = false;
	if ((ins >> lane) & 1ull)
	{
		const uint32_t p = cc_load(parent + i), r = cc_find(parent, p);        // p <= i
		if (r != p)
			cc_store(parent + i, r);        // r < p: the cell only falls.  Roots stay roots and non-roots non-roots throughout this kernel
		root = r == i;
	}
	const uint64_t roots = __ballot(root);
	if (lane == 0 && i < n)
	{
		root_bits[i >> 6] = roots;
		counts[i >> 6] = (uint32_t) __builtin_popcountll(roots) | (uint32_t) __builtin_popcountll(ins) << 16;
	}
}

// chunk c = entries [4096 c, 4096 c + 4096): local[e] = the roots of the chunk's entries before e, sums[c] = the chunk's roots, insums[c] =
// its inside voxels
__global__ void __launch_bounds__(256) k_cc_scan_chunks(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums,
                                                        uint64_t *__restrict__ insums, uint32_t n_entries)
{
	scan_chunk<true>(counts, local, sums, n_entries, insums);
}

// one workgroup: sums[c] becomes the roots of the chunks before c; d_counts = K, min(K, capacity), the inside voxels
__global__ void __launch_bounds__(256) k_cc_scan_total(uint64_t *__restrict__ sums, const uint64_t *__restrict__ insums, uint32_t n_chunks, uint64_t capacity,
                                                       uint64_t *__restrict__ d_counts)
{
	__shared__ uint64_t lds[256];
	scan_total(sums, n_chunks, capacity, d_counts);
	uint64_t mine = 0, total;
	for (uint32_t c = threadIdx.x; c < n_chunks; c += 256)
		mine += insums[c];
	(void) block_exclusive_scan(mine, lds, total);
	if (threadIdx.x == 0)
		d_counts[2] = total;
}

__global__ void __launch_bounds__(256) k_cc_rank_roots(uint32_t n, uint32_t *__restrict__ labels, const uint64_t *__restrict__ root_bits,
                                                       const uint32_t *__restrict__ local, const uint64_t *__restrict__ chunk_before,
                                                       uint32_t *__restrict__ sizes, const uint64_t *__restrict__ d_counts)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
	if (i >= n)
		return;
	if (sizes && i < d_counts[1])        // K <= n: there is a lane for every size
		sizes[i] = 0u;
	const uint32_t e = i >> 6;
	const uint64_t w = root_bits[e];
	if ((w >> lane) & 1ull)
		labels[i] = (uint32_t) chunk_before[e / kScanChunk] + local[e] + (uint32_t) __builtin_popcountll(w & ((1ull << lane) - 1ull)) + 1u;
}

// A wave walks kCcSpan consecutive entries and carries ONE pending (label, count) pair across them, so the label that dominates its 2048
// voxels costs one addition, however many runs it comes in; the other labels of an entry cost one addition each per entry.
constexpr uint32_t kCcSpan = 32;

__global__ void __launch_bounds__(256) k_cc_relabel(uint32_t n, uint32_t n_entries, uint32_t *labels, const uint64_t *__restrict__ bits,
                                                    const uint64_t *__restrict__ root_bits, uint32_t *__restrict__ sizes, const uint64_t *__restrict__ d_counts)
{
	const uint32_t lane = threadIdx.x & 63u, first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * kCcSpan;        // below 2^26 + 128
	const uint64_t known = sizes ? d_counts[1] : 0ull;
	uint32_t       pend = 0, pend_n = 0;        // wave-uniform
	for (uint32_t e = first; e < first + kCcSpan && e < n_entries; ++e)        // wave-uniform
	{
		const uint32_t i = e * 64u + lane;        // e < n_entries <= 2^26
		uint32_t       L = 0;
		if (i < n && ((bits[e] >> lane) & 1ull))        // an outside voxel holds its 0 since k_cc_init: its cell is not touched
		{
			if ((root_bits[e] >> lane) & 1ull)
				L = labels[i];        // a root: its cell was written by the kernel before and is not written here
			else
			{
				L         = labels[labels[i]];        // the cell names its root
				labels[i] = L;
			}
		}
		if (!sizes)        // uniform
			continue;
		uint64_t rest = __ballot(L != 0u && L <= known);
		if (pend)
		{
			const uint64_t m = __ballot(L == pend) & rest;
			pend_n += (uint32_t) __builtin_popcountll(m);
			rest &= ~m;
		}
		while (rest)        // wave-uniform; every round clears at least the leader's bit
		{
			const uint32_t Lx = (uint32_t) __shfl((int) L, __ffsll((long long) rest) - 1);
			const uint64_t m  = __ballot(L == Lx) & rest;
			const uint32_t c  = (uint32_t) __builtin_popcountll(m);
			rest &= ~m;
			if (!pend)
				pend = Lx, pend_n = c;
			else if (lane == 0)
				atomicAdd(sizes + (Lx - 1u), c);
		}
	}
	if (pend && lane == 0)
		atomicAdd(sizes + (pend - 1u), pend_n);
}

__global__ void __launch_bounds__(256) k_cc_select(const uint8_t *src, uint8_t *dst, BoxLinear G, const uint32_t *__restrict__ labels,
                                                   const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ d_counts, uint64_t min_voxels,
                                                   uint64_t max_voxels, uint32_t fill)
{
	box_select(G, src, dst, fill, [&](uint32_t i) {
		const uint32_t L = labels[i];
		if (L == 0 || !sizes || L > d_counts[1])        // a size that is not known removes nothing
			return false;
		const uint64_t s = sizes[L - 1u];
		return s < min_voxels || s > max_voxels;
	});
}

namespace vkv
{

// [the chunks' roots, then roots before: u64 x chunks][the chunks' inside voxels: u64 x chunks][inside bits: u64 x entries][root bits: u64 x
// entries][root and inside counts: u32 x entries][local prefix: u32 x entries], an entry = 64 voxels: 24 bytes per entry + 16 per chunk of
// 4096 entries, i.e. 3/8 byte per voxel; 0: the extent and box are not accepted
size_t components_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, box, p))
		return 0;
	return 16 * (size_t) scan_chunks(p.entries) + 24 * (size_t) p.entries;
}

bool components_launch_ok(VkvExtent3D e, const VkvBox *box)
{
	BoxLinearPlan p;
	return box_linear_plan(e, box, p);
}

int launch_label_components(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, int connectivity, const uint8_t *d_max_map,
                            VkvExtent3D me, void *d_scratch, uint32_t *d_labels, uint32_t *d_sizes, uint64_t capacity, uint64_t *d_counts, hipStream_t s)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "label_components: a box of more than 2^32 - 1 voxels; label it box by box");
	const uint32_t  chunks = scan_chunks(p.entries);
	uint64_t       *sums = static_cast<uint64_t *>(d_scratch), *insums = sums + chunks, *bits = insums + chunks, *root_bits = bits + p.entries;
	uint32_t       *counts = reinterpret_cast<uint32_t *>(root_bits + p.entries), *local = counts + p.entries;
	const BoxLinear G      = box_linear(d_vol, e, b, p, iso);
	hipLaunchKernelGGL(k_cc_init, dim3(p.wgs), dim3(256), 0, s, G, MaxMap(d_max_map, e, me), d_labels, bits);
	if (connectivity == VKV_CONNECT_6)
		hipLaunchKernelGGL(k_cc_merge<VKV_CONNECT_6>, dim3(p.wgs), dim3(256), 0, s, G, d_labels, bits);
	else if (connectivity == VKV_CONNECT_14)
		hipLaunchKernelGGL(k_cc_merge<VKV_CONNECT_14>, dim3(p.wgs), dim3(256), 0, s, G, d_labels, bits);
	else
		hipLaunchKernelGGL(k_cc_merge<VKV_CONNECT_26>, dim3(p.wgs), dim3(256), 0, s, G, d_labels, bits);
	hipLaunchKernelGGL(k_cc_flatten, dim3(p.wgs), dim3(256), 0, s, p.n, d_labels, bits, root_bits, counts);
	hipLaunchKernelGGL(k_cc_scan_chunks, dim3(chunks), dim3(256), 0, s, counts, local, sums, insums, p.entries);
	hipLaunchKernelGGL(k_cc_scan_total, dim3(1), dim3(256), 0, s, sums, insums, chunks, capacity, d_counts);
	uint32_t *sizes = capacity ? d_sizes : nullptr;        // no capacity: no size work
	hipLaunchKernelGGL(k_cc_rank_roots, dim3(p.wgs), dim3(256), 0, s, p.n, d_labels, root_bits, local, sums, sizes, d_counts);
	hipLaunchKernelGGL(k_cc_relabel, dim3((p.entries + 4 * kCcSpan - 1) / (4 * kCcSpan)), dim3(256), 0, s, p.n, p.entries, d_labels, bits, root_bits, sizes,
	                   d_counts);
	return check_launch(ctx, "label_components");
}

int launch_select_components(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, const uint32_t *d_labels,
                             const uint32_t *d_sizes, const uint64_t *d_counts, uint64_t min_voxels, uint64_t max_voxels, uint32_t fill, hipStream_t s)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "select_components: a box of more than 2^32 - 1 voxels");
	const BoxLinear G = box_linear(d_src, e, b, p, 0.0f);        // thr is not read
	hipLaunchKernelGGL(k_cc_select, dim3(p.wgs), dim3(256), 0, s, d_src, d_dst, G, d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill);
	return check_launch(ctx, "select_components");
}

}        // namespace vkv

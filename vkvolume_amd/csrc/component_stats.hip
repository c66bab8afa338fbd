// component_stats.hip — measurements of labelled components (vkv_component_stats) and the pointwise selection of components by a table
// (vkv_select_components_by_table); DESIGN.md §5.17.  Integer work on labels, coordinates and bytes: no floating point, no MFMA.
//
// Both are one-dimensional over the box-linear index of box_domain.hpp, i = ((z - z0) bh + (y - y0)) bw + (x - x0), one voxel per lane, a
// wave's 64 voxels one ENTRY.  written = min(d_counts[0], capacity) is read on the device by every kernel that needs it.
//   k_cs_init         the identities of the records [0, written): mins 0xffffffff, maxes and sums 0 (all four value fields 0 without a
//                     volume), as 8-byte stores; nothing beyond record `written` is touched.
//   k_cs_accumulate   a wave walks kCsSpan consecutive entries, as k_cc_relabel does.  The first counted label it meets becomes its PENDING
//                     label (wave-uniform); the lanes that carry it gather their voxels into per-lane partial records, which meet in ONE
//                     cross-lane reduction at the end of the span, however many runs the label came in.  The sixteen waves of a workgroup
//                     then put their pending labels side by side in LDS, and the waves that carry the same one send ONE set of atomics
//                     between them.  Every other counted label of an entry is found by ballot, its lanes reduced across the wave, and
//                     sent once per (wave, label, entry); a label that one lane alone carries is sent by that lane without a reduction.
//                     An entry without a counted label leaves after the ballot; the volume byte is loaded by lanes with a counted label only.
//   k_cs_select_table box_select with the table's verdict.
//
// POSITIONS.  A lane's position in the box is divided out once per span and then advanced per entry by the box-linear step of 64 voxels,
// (64 % bw, 64 / bw % bh, 64 / bw / bh), with one carry each into y and z: no division per voxel.  Partial records hold BOX coordinates;
// the box's origin is added when a record is sent, so what is stored are volume coordinates.
// WIDTHS.  A lane's and a wave's partial coordinate sums are 64 bits wide (a span of 2048 voxels at x = 4 M sums to 8.6e9); counts and the
// sums of bytes and squared bytes of a workgroup's 32768 voxels stay below 2^31 and are 32 bits wide until they are sent.
// CONTENTION.  Atomics on one record queue up behind one another, and a component that fills the volume meets every wave.  So equal pending
// labels are joined per workgroup (above), and a minimum or maximum is sent only where it would change the bound read beforehand (cs_send).
// UNIQUENESS.  Every field is an integer sum, minimum or maximum of per-voxel terms: it does not depend on the order of the atomics, so two
// runs give the same bytes.  The records are touched from all XCDs with relaxed agent-scope atomics, as the sizes of components.hip are.
// Cross-lane reductions are DPP steps inside rows of 16 and four v_readlane; they run under a full EXEC: every branch around them is wave-uniform,
// no lane leaves the loop early, and no wave leaves before the workgroup's one barrier.  No kernel uses scratch memory (tests/test_component_stats_cpu.py reads the listing).
#include <algorithm>

#include "box_domain.hpp"

using namespace vkv;

constexpr uint32_t kCsSpan = 32;        // entries per wave, as kCcSpan: 2048 voxels

struct CsPartial
{
	uint32_t n, sum_v, sum_v2;                  // voxels, bytes, squared bytes
	uint32_t x0, y0, z0, x1, y1, z1, v0, v1;        // minima and maxima
	uint64_t sx, sy, sz;
};

__device__ __forceinline__ CsPartial cs_identity()
{
	CsPartial p;
	p.n = p.sum_v = p.sum_v2 = 0u;
	p.x0 = p.y0 = p.z0 = p.v0 = 0xffffffffu;
	p.x1 = p.y1 = p.z1 = p.v1 = 0u;
	p.sx = p.sy = p.sz = 0ull;
	return p;
}

// one more voxel of the lane's own
__device__ __forceinline__ void cs_take(CsPartial &p, uint32_t x, uint32_t y, uint32_t z, uint32_t v)
{
	p.n += 1u, p.sum_v += v, p.sum_v2 += v * v;
	p.x0 = min(p.x0, x), p.y0 = min(p.y0, y), p.z0 = min(p.z0, z), p.v0 = min(p.v0, v);
	p.x1 = max(p.x1, x), p.y1 = max(p.y1, y), p.z1 = max(p.z1, z), p.v1 = max(p.v1, v);
	p.sx += x, p.sy += y, p.sz += z;
}

template <int CTRL>
__device__ __forceinline__ uint32_t cs_dpp(uint32_t v)
{
	return (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t cs_dpp(uint64_t v)
{
	return (uint64_t) cs_dpp<CTRL>((uint32_t) v) | (uint64_t) cs_dpp<CTRL>((uint32_t) (v >> 32)) << 32;
}
__device__ __forceinline__ uint32_t cs_lane(uint32_t v, int lane) { return (uint32_t) __builtin_amdgcn_readlane((int) v, lane); }
__device__ __forceinline__ uint64_t cs_lane(uint64_t v, int lane) { return (uint64_t) cs_lane((uint32_t) v, lane) | (uint64_t) cs_lane((uint32_t) (v >> 32), lane) << 32; }

// op over the wave's 64 values, wave-uniform: quad swaps, the half-row and row mirrors (every source lane exists), then one lane per row
template <typename T, typename Op>
__device__ __forceinline__ T cs_reduce(T v, Op op)
{
	v = op(v, cs_dpp<0xB1>(v));         // quad_perm [1, 0, 3, 2]
	v = op(v, cs_dpp<0x4E>(v));         // quad_perm [2, 3, 0, 1]
	v = op(v, cs_dpp<0x141>(v));        // row_half_mirror
	v = op(v, cs_dpp<0x140>(v));        // row_mirror
	return op(op(cs_lane(v, 0), cs_lane(v, 16)), op(cs_lane(v, 32), cs_lane(v, 48)));
}

// the lanes' partial records as one; a lane that holds the identity adds nothing
__device__ __forceinline__ CsPartial cs_wave(const CsPartial &p, bool values)
{
	const auto add = [](auto a, auto b) { return a + b; };
	const auto lo  = [](uint32_t a, uint32_t b) { return min(a, b); };
	const auto hi  = [](uint32_t a, uint32_t b) { return max(a, b); };
	CsPartial  w   = cs_identity();
	w.n            = cs_reduce(p.n, add);
	w.x0 = cs_reduce(p.x0, lo), w.y0 = cs_reduce(p.y0, lo), w.z0 = cs_reduce(p.z0, lo);
	w.x1 = cs_reduce(p.x1, hi), w.y1 = cs_reduce(p.y1, hi), w.z1 = cs_reduce(p.z1, hi);
	w.sx = cs_reduce(p.sx, add), w.sy = cs_reduce(p.sy, add), w.sz = cs_reduce(p.sz, add);
	if (values)        // uniform
	{
		w.sum_v = cs_reduce(p.sum_v, add), w.sum_v2 = cs_reduce(p.sum_v2, add);
		w.v0 = cs_reduce(p.v0, lo), w.v1 = cs_reduce(p.v1, hi);
	}
	return w;
}

__device__ __forceinline__ void cs_add(uint64_t *p, uint64_t v) { (void) __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cs_min(uint32_t *p, uint32_t v) { (void) __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cs_max(uint32_t *p, uint32_t v) { (void) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t cs_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one lane: the partial record p (box coordinates, p.n > 0) into label L's record (volume coordinates).  x0 + p.x1 < 2^32: the box lies in the extent.
// LOOK (the once-per-workgroup send; not the per-entry ones, whose labels are mostly small and which would wait for the answer every time):
// the record's bounds are read first and a minimum or maximum is sent only where it would change what was read.  A minimum only falls
// and a maximum only rises, so a bound that already covers ours still does, however old the value read is: the record ends the same, and a
// large component, whose waves would otherwise queue fourteen atomics each on the same two cache lines, queues six
template <bool LOOK>
__device__ __forceinline__ void cs_send(VkvComponentStats *stats, uint32_t L, const CsPartial &p, const BoxLinear &G, bool values)
{
	VkvComponentStats *r = stats + (L - 1u);
	const uint32_t     x0 = G.x0 + p.x0, y0 = G.y0 + p.y0, z0 = G.z0 + p.z0, x1 = G.x0 + p.x1, y1 = G.y0 + p.y1, z1 = G.z0 + p.z1;
	uint32_t           rx0 = 0xffffffffu, ry0 = 0xffffffffu, rz0 = 0xffffffffu, rv0 = 0xffffffffu, rx1 = 0u, ry1 = 0u, rz1 = 0u, rv1 = 0u;        // everything is sent
	if (LOOK)
	{
		rx0 = cs_load(&r->min_x), ry0 = cs_load(&r->min_y), rz0 = cs_load(&r->min_z), rx1 = cs_load(&r->max_x), ry1 = cs_load(&r->max_y), rz1 = cs_load(&r->max_z);
		if (values)
			rv0 = cs_load(&r->min_value), rv1 = cs_load(&r->max_value);
	}
	if (!LOOK || x0 < rx0)
		cs_min(&r->min_x, x0);
	if (!LOOK || y0 < ry0)
		cs_min(&r->min_y, y0);
	if (!LOOK || z0 < rz0)
		cs_min(&r->min_z, z0);
	if (!LOOK || x1 > rx1)
		cs_max(&r->max_x, x1);
	if (!LOOK || y1 > ry1)
		cs_max(&r->max_y, y1);
	if (!LOOK || z1 > rz1)
		cs_max(&r->max_z, z1);
	cs_add(&r->voxels, p.n);
	cs_add(&r->sum_x, p.sx + (uint64_t) p.n * G.x0), cs_add(&r->sum_y, p.sy + (uint64_t) p.n * G.y0), cs_add(&r->sum_z, p.sz + (uint64_t) p.n * G.z0);
	if (values)
	{
		if (!LOOK || p.v0 < rv0)
			cs_min(&r->min_value, p.v0);
		if (!LOOK || p.v1 > rv1)
			cs_max(&r->max_value, p.v1);
		cs_add(&r->sum_value, p.sum_v), cs_add(&r->sum_value2, p.sum_v2);
	}
}

// records [0, min(d_counts[0], capacity)) as ten 8-byte words each: (min_x, min_y) (min_z, max_x) (max_y, max_z) (min_value, max_value) and six sums
__global__ void __launch_bounds__(256) k_cs_init(uint2 *__restrict__ words, const uint64_t *__restrict__ d_counts, uint64_t capacity, uint32_t min_value)
{
	const uint64_t k = d_counts[0], total = (k < capacity ? k : capacity) * 10ull;        // below 2^36
	for (uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t) gridDim.x * 256u)
	{
		const uint32_t part = (uint32_t) (t % 10ull);
		uint2          w    = make_uint2(0u, 0u);
		if (part == 0u)
			w = make_uint2(0xffffffffu, 0xffffffffu);
		else if (part == 1u)
			w = make_uint2(0xffffffffu, 0u);
		else if (part == 3u)
			w = make_uint2(min_value, 0u);
		words[t] = w;
	}
}

// what the host divides once: the entries and the box-linear step of 64 voxels
struct CsWalk
{
	uint32_t n_entries, dx, dy, dz;        // dx < bw, dy < bh
};

// the position `step` voxels on, step = (dx, dy, dz) in box-linear terms with dx < bw and dy < bh: one carry into y, one into z
__device__ __forceinline__ void cs_advance(BoxVoxel &v, const BoxLinear &G, uint32_t dx, uint32_t dy, uint32_t dz)
{
	v.x += dx;
	const uint32_t cx = v.x >= G.bw ? 1u : 0u;
	v.x -= cx ? G.bw : 0u;
	v.y += dy + cx;        // below 2 bh
	const uint32_t cy = v.y >= G.bh ? 1u : 0u;
	v.y -= cy ? G.bh : 0u;
	v.z += dz + cy;
}

constexpr uint32_t kCsWaves = 16;        // waves per workgroup: 16 spans, 32768 voxels

__global__ void __launch_bounds__(64 * kCsWaves) k_cs_accumulate(BoxLinear G, CsWalk K, const uint32_t *__restrict__ labels, const uint64_t *__restrict__ d_counts,
                                                       uint64_t capacity, VkvComponentStats *stats)
{
	const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
	__shared__ uint32_t  s_pend[kCsWaves];
	__shared__ CsPartial s_part[kCsWaves];
	const uint32_t first = (blockIdx.x * kCsWaves + wave) * kCsSpan;        // below 2^26 + 512
	const uint64_t k = d_counts[0], known = k < capacity ? k : capacity;        // 0: no label is counted
	const bool     values = G.vol != nullptr;
	BoxVoxel       v;
	v.lane = lane, v.valid = true;
	v.i = first * 64u + lane;        // first < n_entries <= 2^26 wherever the loop below runs at all
	{
		const uint32_t t = v.i / G.bw;
		v.x = v.i - t * G.bw, v.y = t % G.bh, v.z = t / G.bh;
	}
	uint32_t  pend = 0u;        // wave-uniform
	CsPartial mine = cs_identity();        // this lane's voxels of the pending label
	for (uint32_t e = first; e < first + kCsSpan && e < K.n_entries; ++e)        // wave-uniform; at or above n_entries from the start: nothing to walk
	{
		const uint32_t L       = v.i < G.n ? labels[v.i] : 0u;        // only the last entry is short
		const bool     counted = L != 0u && L <= known;
		uint64_t       rest    = __ballot(counted);
		if (rest)
		{
			uint32_t b = 0u;
			if (counted && values)
				b = G.vol[box_address(G, v)];
			if (pend)
			{
				const bool same = counted && L == pend;
				if (same)
					cs_take(mine, v.x, v.y, v.z, b);
				rest &= ~__ballot(same);
			}
			while (rest)        // wave-uniform; every round clears at least the leader's bit
			{
				const uint32_t leader = (uint32_t) __ffsll((long long) rest) - 1u;
				const uint32_t Lx     = (uint32_t) __shfl((int) L, (int) leader);
				const bool     in     = counted && L == Lx;
				const uint64_t m      = __ballot(in);        // a subset of rest: a counted label that is not pending
				rest &= ~m;
				if (!pend)
				{
					pend = Lx;
					if (in)
						cs_take(mine, v.x, v.y, v.z, b);
					continue;
				}
				CsPartial one = cs_identity();
				if (in)
					cs_take(one, v.x, v.y, v.z, b);
				if ((m & (m - 1ull)) == 0ull)        // one lane alone: it holds the whole partial record
				{
					if (lane == leader)
						cs_send<false>(stats, Lx, one, G, values);
				}
				else
				{
					const CsPartial w = cs_wave(one, values);
					if (lane == 0u)
						cs_send<false>(stats, Lx, w, G, values);
				}
			}
		}
		v.i += 64u;        // the next entry; may wrap behind the last one, where it is not used
		cs_advance(v, G, K.dx, K.dy, K.dz);
	}
	// the workgroup's waves that carry the same pending label send as one: the first of them gathers the others' partial records, one per lane
	if (pend)
	{
		const CsPartial w = cs_wave(mine, values);
		if (lane == 0u)
			s_part[wave] = w;
	}
	if (lane == 0u)
		s_pend[wave] = pend;
	__syncthreads();        // every wave arrives: none has left
	if (!pend)
		return;
	const uint64_t same = __ballot(lane < kCsWaves && s_pend[lane < kCsWaves ? lane : 0u] == pend);        // bit `wave` is set
	if (same & ((1ull << wave) - 1ull))        // an earlier wave sends for this one
		return;
	CsPartial p = cs_identity();
	if ((same >> lane) & 1ull)
		p = s_part[lane];
	const CsPartial w = cs_wave(p, values);
	if (lane == 0u)
		cs_send<true>(stats, pend, w, G, values);
}

__global__ void __launch_bounds__(256) k_cs_select_table(const uint8_t *src, uint8_t *dst, BoxLinear G, const uint32_t *__restrict__ labels,
                                                         const uint8_t *__restrict__ keep, uint64_t table_entries, uint32_t fill)
{
	box_select(G, src, dst, fill, [&](uint32_t i) {
		const uint32_t L = labels[i];
		if (L == 0u || L > table_entries)        // what the table does not name is not removed
			return false;
		return keep[L - 1u] == 0u;
	});
}

namespace vkv
{

int launch_component_stats(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, const uint32_t *d_labels, const uint64_t *d_counts,
                           VkvComponentStats *d_stats, uint64_t capacity, hipStream_t s)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "component_stats: a box of more than 2^32 - 1 voxels; measure it box by box");
	if (capacity == 0)
		return VKV_OK;
	const BoxLinear G = box_linear(d_vol, e, b, p, 0.0f);        // thr is not read
	CsWalk          K{};
	K.n_entries = p.entries;
	K.dx = 64u % b.width, K.dy = 64u / b.width % b.height, K.dz = 64u / b.width / b.height;
	const uint64_t init_wgs = std::min<uint64_t>((capacity * 10ull + 255ull) / 256ull, 8192ull);
	hipLaunchKernelGGL(k_cs_init, dim3((uint32_t) init_wgs), dim3(256), 0, s, reinterpret_cast<uint2 *>(d_stats), d_counts, capacity, d_vol ? 0xffffffffu : 0u);
	hipLaunchKernelGGL(k_cs_accumulate, dim3((p.entries + kCsWaves * kCsSpan - 1) / (kCsWaves * kCsSpan)), dim3(64 * kCsWaves), 0, s, G, K, d_labels, d_counts, capacity, d_stats);
	return check_launch(ctx, "component_stats");
}

int launch_select_components_by_table(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D e, const VkvBox &b, const uint32_t *d_labels,
                                      const uint8_t *d_keep, uint64_t table_entries, uint32_t fill, hipStream_t s)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "select_components_by_table: a box of more than 2^32 - 1 voxels");
	const BoxLinear G = box_linear(d_src, e, b, p, 0.0f);        // thr is not read
	hipLaunchKernelGGL(k_cs_select_table, dim3(p.wgs), dim3(256), 0, s, d_src, d_dst, G, d_labels, d_keep, table_entries, fill);
	return check_launch(ctx, "select_components_by_table");
}

}        // namespace vkv

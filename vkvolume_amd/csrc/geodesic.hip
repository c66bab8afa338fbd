// geodesic.hip — the geodesic (in-mask) distance map of a box with chamfer step costs, and the label propagation that goes with it
// (vkv_geodesic_propagate); DESIGN.md §5.20.  key(v) = the lexicographic minimum of (cost, seed label) over all paths of moves from a seed to
// v through inside voxels of the box; a move to one of the 26 neighbours has the cost steps[|dx| + 2 |dy| + 4 |dz| - 1], 0: no such move.
// Integer work only.  The inside rule, "only the box exists" and the box-linear arrays are components.hip's.
// STATE.  One uint64 per voxel of the box in the scratch block, key = cost << 32 | label, read and written as ONE 64-bit value: a reader
// never sees a new cost next to an old label.  GEO_NONE (all ones) = not reached, and what every outside voxel holds throughout.  Behind the
// keys: a header (GeoHead) and two dirty flags per TILE of 8 x 8 x 8 voxels.
//   k_geo_init     keys from the seeds (label, cost 0), GEO_NONE elsewhere; every tile dirty for round 0; the header reset.
//   k_geo_round    once per round.  A workgroup of 512 lanes takes a tile (tiles beyond the grid in a stride loop), leaves it after reading
//                  its flag when that is 0, else loads the tile's keys with a one-voxel halo into LDS (10 x 10 x 10 entries, rows 24
//                  entries apart), one lane per voxel, and relaxes: key(v) <- min(key(v), key(u) + (c << 32)) over the 26 moves u -> v whose
//                  new cost stays below the limit.  A sweep is Jacobi: every lane reads its neighbours, a barrier, the lanes that improved
//                  write THEIR OWN entry, a barrier.  The loop ends with the first sweep that changes nothing, after at most 512 sweeps.
//                  Lanes whose key changed store it, and set a mark for every neighbour tile that has the voxel in its halo; the marks
//                  become the dirty flags of the NEXT round, and the round's "changed" word.  A tile that ran into the sweep bound marks
//                  itself.
//   k_geo_finish   keys split into d_dist / d_labels, the reached voxels counted (one integer atomicAdd per workgroup of 4096 voxels), d_counts[0] = the last
//                  round marked nothing, and the header's round counter moved on for a resumed call.
// ORDER-FREE.  Costs are positive, so a path's prefix under the limit is under the limit, and the cap drops nothing that counts.  Every value
// a voxel ever holds is the key of some path from a seed (or GEO_NONE): an upper bound of key(v) that only falls.  Relaxing in any order from
// any such values ends in the same fixed point, key(v) itself (tests/test_geodesic_cpu.py restates the scheme with
// shuffled tiles and stale halos and holds it to a heap Dijkstra).
// COHERENCE.  ONLY THE OWNING TILE WRITES A KEY.  The halo reads of a round race with the neighbours' stores of the same round; whatever is
// read is an earlier key of that voxel, hence a valid upper bound, and the neighbour's change marks this tile for the next round, which sees
// it across the kernel boundary.  Those loads and stores are relaxed agent-scope 64-bit atomics: nothing tears, nothing stale is served from
// another XCD's L2.  Flags, marks and the header are read only across kernel boundaries: round g reads dirty[g & 1] (each dirty tile clears
// its own, after a barrier) and changed[(g - 1) % 3], writes ones into dirty[(g + 1) & 1] and changed[g % 3], and clears changed[(g + 1) % 3].
// TERMINATION is structural.  The sweep loop is a `for` with the bound 512 = the tile's voxels (a shortest path inside a tile visits each
// voxel at most once, and a Jacobi sweep settles at least the next voxel of every such path); the tile loop strides over a fixed count.  No
// lane waits for another wave or workgroup; no persistent kernel.  EARLY EXIT: round g + 1 leaves at once where round g marked nothing.
// DETERMINISM.  The fixed point is unique (ties go to the smallest label inside the 64-bit minimum), the count is an integer sum.
// NO OVERFLOW.  A move is taken only from a key below (limit - c) << 32, so the new cost is below limit <= 0xffffffff and the 64-bit sum does
// not carry; GEO_NONE is above every such bound, so outside voxels, unreached voxels and halo entries beyond the box never propagate.
// Box-linear indices are below n <= 2^32 - 1; halo coordinates are checked against the box before anything is read.
// LDS.  ds_read_b64 is served per half wave over 64 dword banks.  A half wave is 8 x 4 voxels of a z slice: with rows 24 entries = 48 dwords
// apart the four rows start at banks 0, 48, 32, 16 and cover all 64 once: conflict-free for every offset (dx shifts all lanes alike).
// RESOURCES (gfx950 listing): k_geo_round 50 VGPRs, 19320 bytes of LDS (2400 keys + 2 sweep flags + 27 marks), no scratch memory, no private
// arrays; k_geo_init and k_geo_finish below 24 VGPRs, 0 and 16 bytes of LDS, no scratch memory (tests/test_geodesic_cpu.py reads the listing).
#include "box_domain.hpp"

using namespace vkv;

#define GEO_NONE 0xffffffffffffffffull

constexpr uint32_t kGeoEdge = 8, kGeoLanes = 512;        // a tile's edge and voxels
constexpr uint32_t kGeoHalo = kGeoEdge + 2, kGeoPitch = 24, kGeoSlab = kGeoHalo * kGeoPitch, kGeoLds = kGeoHalo * kGeoSlab;
constexpr uint32_t kGeoMaxGrid = 1u << 22;               // workgroups per launch; further tiles by stride
constexpr uint32_t kGeoStrips  = 16;                     // k_geo_finish: strips of 256 voxels per workgroup

// behind the keys in the scratch block, 32 bytes
struct GeoHead
{
	uint32_t epoch;             // the rounds run so far, mod 6 (parity for the dirty flags, mod 3 for `changed`)
	uint32_t changed[3];        // changed[g % 3] != 0: round g marked a tile
	uint32_t pad[4];
};

// the step table as the kernel takes it
struct GeoSteps
{
	uint64_t below[7];        // a neighbour's key below this may take the move of class m = index + 1: (limit - c) << 32; 0: no such move
	uint32_t c[7];
};

__device__ __forceinline__ uint64_t geo_load(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void     geo_store(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void     geo_raise(uint32_t *p) { __hip_atomic_store(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// lane i: voxel i's key; tile i's flags (there are at most as many tiles as voxels); lane 0: the header
__global__ void __launch_bounds__(256) k_geo_init(BoxLinear G, const uint32_t *__restrict__ seeds, uint64_t *__restrict__ keys, GeoHead *__restrict__ head,
                                                  uint32_t *__restrict__ dirty0, uint32_t *__restrict__ dirty1, uint32_t tiles)
{
	const BoxVoxel v = box_voxel(G);
	if (!v.valid)
		return;
	const uint32_t s = seeds[v.i];
	keys[v.i]        = (s != 0u && G.vol[box_address(G, v)] >= G.thr) ? (uint64_t) s : GEO_NONE;        // cost 0 is below every limit
	if (v.i < tiles)
		dirty0[v.i] = 1u, dirty1[v.i] = 0u;
	if (v.i == 0u)
		head->epoch = 0u, head->changed[0] = 0u, head->changed[1] = 0u, head->changed[2] = 1u;        // "round -1 changed something"
}

// one relaxation of `best` from the entry at lds[a + (dz, dy, dx)]
template <int DX, int DY, int DZ>
__device__ __forceinline__ void geo_relax(const GeoSteps &S, const uint64_t *lds, uint32_t a, uint64_t &best)
{
	constexpr int m = (DX != 0) + 2 * (DY != 0) + 4 * (DZ != 0);
	if (m == 0)
		return;
	const uint64_t below = S.below[m > 0 ? m - 1 : 0];
	if (below == 0ull)        // uniform
		return;
	const uint64_t k = lds[(int) a + DZ * (int) kGeoSlab + DY * (int) kGeoPitch + DX];
	if (k < below)
	{
		const uint64_t cand = k + ((uint64_t) S.c[m > 0 ? m - 1 : 0] << 32);        // no carry: the cost stays below the limit
		best                = cand < best ? cand : best;
	}
}

template <int DY, int DZ>
__device__ __forceinline__ void geo_relax_row(const GeoSteps &S, const uint64_t *lds, uint32_t a, uint64_t &best)
{
	geo_relax<-1, DY, DZ>(S, lds, a, best);
	geo_relax<0, DY, DZ>(S, lds, a, best);
	geo_relax<1, DY, DZ>(S, lds, a, best);
}

template <int DZ>
__device__ __forceinline__ void geo_relax_slab(const GeoSteps &S, const uint64_t *lds, uint32_t a, uint64_t &best)
{
	geo_relax_row<-1, DZ>(S, lds, a, best);
	geo_relax_row<0, DZ>(S, lds, a, best);
	geo_relax_row<1, DZ>(S, lds, a, best);
}

// round g = head->epoch + r of the state; tx, ty, tz: the tiles along the axes, tiles = tx ty tz
__global__ void __launch_bounds__(512) k_geo_round(BoxLinear G, GeoSteps S, uint32_t tx, uint32_t ty, uint32_t tiles, uint32_t r, uint64_t *keys, GeoHead *head,
                                                   uint32_t *dirty0, uint32_t *dirty1, uint64_t *__restrict__ d_counts)
{
	__shared__ uint64_t lds[kGeoLds];
	__shared__ uint32_t moved[2];        // moved[sweep & 1]: the sweep changed an entry
	__shared__ uint32_t mark[27];        // the neighbour tile (sz + 1) 9 + (sy + 1) 3 + sx + 1 has a changed voxel in its halo; 13: this tile
	const uint32_t tid = threadIdx.x;
	const uint32_t g   = head->epoch + r;        // the header's epoch is written by k_geo_init and k_geo_finish only
	uint32_t *cur = (g & 1u) ? dirty1 : dirty0, *nxt = (g & 1u) ? dirty0 : dirty1;
	const uint32_t before = head->changed[(g + 2u) % 3u];        // round g - 1's: nobody writes it in this round
	if (blockIdx.x == 0u && tid == 0u)
	{
		head->changed[(g + 1u) % 3u] = 0u;        // for round g + 1 to raise
		if (r == 0u)
			d_counts[1] = 0ull;        // for k_geo_finish to add to
	}
	if (before == 0u)        // uniform over the grid: the state is the fixed point, and no flag is set
		return;
	const uint32_t lx = tid & 7u, ly = (tid >> 3) & 7u, lz = tid >> 6;
	const uint32_t a  = ((lz + 1u) * kGeoHalo + ly + 1u) * kGeoPitch + lx + 1u;
	for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x)        // uniform
	{
		if (__builtin_amdgcn_readfirstlane((int) cur[t]) == 0)        // every lane reads the same word; only this workgroup writes it, below
			continue;
		const uint32_t tzc = t / (tx * ty), trem = t - tzc * (tx * ty), tyc = trem / tx, txc = trem - tyc * tx;
		const uint32_t x0 = txc * kGeoEdge, y0 = tyc * kGeoEdge, z0 = tzc * kGeoEdge;        // the tile's first voxel, in the box
		for (uint32_t e = tid; e < kGeoHalo * kGeoHalo * kGeoHalo; e += kGeoLanes)
		{
			const uint32_t hz = e / (kGeoHalo * kGeoHalo), hrem = e - hz * (kGeoHalo * kGeoHalo), hy = hrem / kGeoHalo, hx = hrem - hy * kGeoHalo;
			const uint32_t x = x0 + hx - 1u, y = y0 + hy - 1u, z = z0 + hz - 1u;        // mod 2^32: -1 is above every axis
			uint64_t       k = GEO_NONE;                                                // beyond the box nothing exists
			if (x < G.bw && y < G.bh && z < G.bd)
				k = geo_load(keys + ((z * G.bh + y) * G.bw + x));        // an index of the box: below n
			lds[(hz * kGeoHalo + hy) * kGeoPitch + hx] = k;
		}
		if (tid < 27u)
			mark[tid] = 0u;
		if (tid < 2u)
			moved[tid] = 0u;
		const uint32_t x = x0 + lx, y = y0 + ly, z = z0 + lz;
		const bool     own = x < G.bw && y < G.bh && z < G.bd;
		const uint32_t i   = own ? (z * G.bh + y) * G.bw + x : 0u;
		bool           in  = false;
		if (own)
			in = G.vol[((size_t) (G.z0 + z) * (size_t) G.H + (size_t) (G.y0 + y)) * (size_t) G.W + (size_t) (G.x0 + x)] >= G.thr;
		__syncthreads();
		if (tid == 0u)
			cur[t] = 0u;        // every lane has read it
		const uint64_t first = lds[a];
		uint64_t       mine  = first;
		bool           bound = true;
		for (uint32_t sweep = 0; sweep < kGeoLanes; ++sweep)        // uniform
		{
			uint64_t best = mine;
			if (in)
			{
				geo_relax_slab<-1>(S, lds, a, best);
				geo_relax_slab<0>(S, lds, a, best);
				geo_relax_slab<1>(S, lds, a, best);
			}
			__syncthreads();        // every read of the sweep is done
			if (best < mine)
			{
				mine = best, lds[a] = best;
				moved[sweep & 1u] = 1u;
			}
			if (tid == 0u)
				moved[(sweep + 1u) & 1u] = 0u;        // read before the barrier above, raised after the next one
			__syncthreads();
			if (moved[sweep & 1u] == 0u)
			{
				bound = false;
				break;
			}
		}
		if (mine != first)
		{
			geo_store(keys + i, mine);        // this lane's own voxel, of this workgroup's own tile
			const int bx = lx == 0u ? -1 : (lx == kGeoEdge - 1u ? 1 : 0), by = ly == 0u ? -1 : (ly == kGeoEdge - 1u ? 1 : 0),
			          bz = lz == 0u ? -1 : (lz == kGeoEdge - 1u ? 1 : 0);
#pragma unroll
			for (int k = 1; k < 8; ++k)        // the tiles that hold this voxel in their halo
			{
				if (((k & 1) && bx == 0) || ((k & 2) && by == 0) || ((k & 4) && bz == 0))
					continue;
				mark[(((k & 4) ? bz : 0) + 1) * 9 + (((k & 2) ? by : 0) + 1) * 3 + ((k & 1) ? bx : 0) + 1] = 1u;
			}
		}
		if (bound && tid == 0u)
			mark[13] = 1u;        // not settled within the bound: this tile goes on in the next round
		__syncthreads();
		if (tid < 27u && mark[tid] != 0u)
		{
			const uint32_t nx = txc + tid % 3u - 1u, ny = tyc + tid / 3u % 3u - 1u, nz = tzc + tid / 9u - 1u;        // mod 2^32
			if (nx < tx && ny < ty && nz < tiles / (tx * ty))
			{
				geo_raise(nxt + ((nz * ty + ny) * tx + nx));
				geo_raise(&head->changed[g % 3u]);
			}
		}
		__syncthreads();        // the LDS is the next tile's
	}
}

// rounds: those of this call; the last one was round head->epoch + rounds - 1
__global__ void __launch_bounds__(256) k_geo_finish(uint32_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ dist, uint32_t *__restrict__ labels,
                                                    GeoHead *head, uint32_t rounds, uint64_t *__restrict__ d_counts)
{
	__shared__ uint32_t waves[4];
	uint32_t            count = 0;        // wave-uniform: the reached voxels of this wave's strips
#pragma unroll 4
	for (uint32_t strip = 0; strip < kGeoStrips; ++strip)
	{
		const uint32_t i = (blockIdx.x * kGeoStrips + strip) * 256u + threadIdx.x;        // at most 2^32 - 1: the grid has at most 2^20 workgroups
		const uint64_t k = i < n ? keys[i] : GEO_NONE;
		if (i < n)
		{
			if (dist)
				dist[i] = (uint32_t) (k >> 32);        // GEO_NONE: VKV_GEODESIC_NONE
			if (labels)
				labels[i] = k == GEO_NONE ? 0u : (uint32_t) k;
		}
		count += (uint32_t) __builtin_popcountll(__ballot(k != GEO_NONE));
	}
	if ((threadIdx.x & 63u) == 0u)
		waves[threadIdx.x >> 6] = count;
	__syncthreads();
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (threadIdx.x == 0u && waves[0] + waves[1] + waves[2] + waves[3] != 0u)        // one atomic per 4096 voxels that hold a reached one
		atomicAdd((unsigned long long *) d_counts + 1, (unsigned long long) (waves[0] + waves[1] + waves[2] + waves[3]));
	if (i == 0u)        // the one lane that reads or writes the header here
	{
		const uint32_t last = head->epoch + rounds - 1u;
		d_counts[0]         = head->changed[last % 3u] == 0u ? 1ull : 0ull;
		head->epoch         = (last + 1u) % 6u;
	}
}

namespace vkv
{

static uint32_t geo_tiles_along(uint32_t len) { return len / kGeoEdge + (len % kGeoEdge != 0u); }

// [keys: u64 x voxels][GeoHead: 32 bytes][dirty flags: 2 x u32 x tiles], tiles = the product over the axes of ceil(len / 8): 8 bytes per voxel
// + 32 + 8 per tile; 0: the extent and box are not accepted
size_t geodesic_scratch_bytes(VkvExtent3D e, const VkvBox *box)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, box, p))
		return 0;
	const VkvBox b = whole_or(e, box);
	const size_t t = (size_t) geo_tiles_along(b.width) * geo_tiles_along(b.height) * geo_tiles_along(b.depth);        // at most 2^29 + ...: below n + 1
	return 8 * (size_t) p.n + sizeof(GeoHead) + 8 * t;
}

int launch_geodesic_propagate(vkv_ctx *ctx, const uint8_t *d_vol, VkvExtent3D e, const VkvBox &b, float iso, const uint32_t *d_seeds, const uint32_t steps[7],
                              uint32_t limit, uint32_t rounds, bool resume, void *d_scratch, uint32_t *d_dist, uint32_t *d_labels, uint64_t *d_counts,
                              hipStream_t s)
{
	BoxLinearPlan p;
	if (!box_linear_plan(e, &b, p))
		return set_error(ctx, VKV_E_UNSUPPORTED, "geodesic_propagate: a box of more than 2^32 - 1 voxels");
	const uint32_t  tx = geo_tiles_along(b.width), ty = geo_tiles_along(b.height), tz = geo_tiles_along(b.depth), tiles = tx * ty * tz;        // <= n
	uint64_t       *keys   = static_cast<uint64_t *>(d_scratch);
	GeoHead        *head   = reinterpret_cast<GeoHead *>(keys + p.n);
	uint32_t       *dirty0 = reinterpret_cast<uint32_t *>(head + 1), *dirty1 = dirty0 + tiles;
	const BoxLinear G      = box_linear(d_vol, e, b, p, iso);
	GeoSteps        S{};
	for (int m = 0; m < 7; ++m)
	{
		S.c[m]     = steps[m];
		S.below[m] = steps[m] != 0u && steps[m] < limit ? (uint64_t) (limit - steps[m]) << 32 : 0ull;
	}
	if (!resume)
		hipLaunchKernelGGL(k_geo_init, dim3(p.wgs), dim3(256), 0, s, G, d_seeds, keys, head, dirty0, dirty1, tiles);
	const uint32_t grid = tiles < kGeoMaxGrid ? tiles : kGeoMaxGrid;
	for (uint32_t r = 0; r < rounds; ++r)
		hipLaunchKernelGGL(k_geo_round, dim3(grid), dim3(kGeoLanes), 0, s, G, S, tx, ty, tiles, r, keys, head, dirty0, dirty1, d_counts);
	hipLaunchKernelGGL(k_geo_finish, dim3(p.n / (256u * kGeoStrips) + (p.n % (256u * kGeoStrips) != 0u)), dim3(256), 0, s, p.n, keys, d_dist, d_labels, head, rounds, d_counts);
	return check_launch(ctx, "geodesic_propagate");
}

}        // namespace vkv

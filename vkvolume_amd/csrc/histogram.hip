// histogram.hip — joint (gradient byte, intensity byte) histogram of a box of the volume (vkv_volume_histogram), and the
// occupied-voxel count of an analytic transfer function read off it (vkv_histogram_occupied_count).
//
// The histogram reads the two bytes per voxel that k_occupied_voxel_count reads.  A wave takes (row, 64-dword column) units of the box;
// each lane turns one dword of intensities and one of gradients into four keys g * 256 + i.  Equal keys of a lane are merged in registers,
// the keys equal to the wave's first active key are added once by one lane (ballot + popcount), and the rest go one LDS atomic per key.
// That keeps a constant or background-heavy volume from serialising 64 lanes on one address.
//
// Large boxes: one workgroup per CU with a private histogram of 65536 16-bit counters in 32768 LDS words (128 KiB), flushed at the end
// with one 64-bit device-scope atomic per non-zero bin.  Small boxes: the same loop adding straight to the 64-bit bins, so that a
// region update's few thousand voxels do not pay for clearing and scanning 128 KiB of LDS per workgroup.
#include <algorithm>

#include "launchers.hpp"

using namespace vkv;

namespace
{
constexpr uint32_t kHistBins  = VKV_HISTOGRAM_BINS;
constexpr uint32_t kHistWords = kHistBins / 2;        // LDS word w holds bin w in its low half and bin w + 32768 in its high half
constexpr int      kHistItems = 8;                    // units a wave loads per round
constexpr int      kHistLdsThreads = 1024, kHistGlobalThreads = 256;
// A 16-bit counter never wraps.  The lane whose returning add takes a half from below kHistSpill to kHistSpill or above moves kHistSpill
// from that half to the 64-bit bin, and every wave waits for its LDS operations and meets at a barrier once per round.  A round adds at
// most 16 waves x kHistItems units x 64 lanes x 4 voxels = 32768 voxels to a workgroup's counters, so a half that starts a round below
// kHistSpill stays at or below 0x7fff + 32768 = 0xffff while its spill is in flight, and ends the round below kHistSpill again.
constexpr uint32_t kHistSpill = 0x8000;
static_assert((kHistLdsThreads / 64) * kHistItems * 64 * 4 + (kHistSpill - 1) <= 0xffffu, "a round could wrap a 16-bit counter");
// boxes of at most this many voxels take the global-atomic path; larger ones get a workgroup per 2^kHistVoxelsPerGroupLog2 voxels, up to one per CU
constexpr uint64_t kHistGlobalMaxVoxels    = 1ull << 18;
constexpr int      kHistVoxelsPerGroupLog2 = 18;

struct HistArgs
{
	const uint8_t *     vol, *grad;        // the box's first voxel in the volume / the gradient map (grad null: gradient row 0)
	unsigned long long *hist;
	uint64_t            slice;             // W * H
	uint32_t            W, bw, bh, blocks_x, n_units;        // units: (row of the box, 64-dword column of that row), row-major
	int                 negate;                             // VKV_HISTOGRAM_SUBTRACT: bins receive 2^64 - count
};

__device__ __forceinline__ unsigned long long signed_count(uint32_t c, int negate) { return negate ? 0ull - (unsigned long long) c : (unsigned long long) c; }

// LDS: add c to the 16-bit counter of `key` and return the counter's value before the add (hist_spill checks it later, so that the adds of an
// item are all in flight before the first return is waited for); global: add c to the 64-bit bin
template <bool LDS>
__device__ __forceinline__ uint32_t hist_add(uint32_t *s_hist, const HistArgs &a, uint32_t key, uint32_t c)
{
	if (!LDS)
	{
		atomicAdd(&a.hist[key], signed_count(c, a.negate));
		return 0u;
	}
	const uint32_t sh = (key >> 15) << 4;
	return (atomicAdd(&s_hist[key & (kHistWords - 1)], c << sh) >> sh) & 0xffffu;
}

// the add that took the counter of `key` from `old` below kHistSpill to kHistSpill or above moves kHistSpill to the 64-bit bin
template <bool LDS>
__device__ __forceinline__ void hist_spill(uint32_t *s_hist, const HistArgs &a, uint32_t key, uint32_t c, uint32_t old)
{
	if (LDS && old < kHistSpill && old + c >= kHistSpill)
	{
		atomicSub(&s_hist[key & (kHistWords - 1)], kHistSpill << ((key >> 15) << 4));
		atomicAdd(&a.hist[key], signed_count(kHistSpill, a.negate));
	}
}

// sum over the wave of a per-lane count 0..7
__device__ __forceinline__ uint32_t wave_sum3(uint32_t m)
{
	return (uint32_t) __popcll(__ballot(m & 1u)) + 2u * (uint32_t) __popcll(__ballot(m & 2u)) + 4u * (uint32_t) __popcll(__ballot(m & 4u));
}

// the n (0..4) valid voxels of one lane: intensities in the bytes of v >> sh, gradients in those of g >> sh
template <bool LDS>
__device__ __forceinline__ void hist_item(uint32_t *s_hist, const HistArgs &a, uint32_t v, uint32_t g, uint32_t sh, int n)
{
	v >>= sh, g >>= sh;
	const unsigned long long active = __ballot(n > 0);
	if (active == 0ull)
		return;
	// the wave's first key: voxel 0 of its first active lane
	const int      first = __ffsll((long long) active) - 1;
	const uint32_t v0 = (uint32_t) __builtin_amdgcn_readlane((int) (v & 255u), first), g0 = (uint32_t) __builtin_amdgcn_readlane((int) (g & 255u), first);
	const uint32_t lead = (g0 << 8) | v0;
	// every valid voxel of the wave has that key (a background run, a constant volume): one add of the wave's voxel count
	const uint32_t valid = n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
	const bool     same  = (((v ^ (v0 * 0x01010101u)) | (g ^ (g0 * 0x01010101u))) & valid) == 0u;
	if (__ballot(!same) == 0ull)
	{
		const uint32_t total = wave_sum3((uint32_t) n);
		if ((int) __lane_id() == first)
			hist_spill<LDS>(s_hist, a, lead, total, hist_add<LDS>(s_hist, a, lead, total));
		return;
	}
	uint32_t k[4], c[4];
#pragma unroll
	for (int i = 0; i < 4; ++i)
		k[i] = (((g >> (8 * i)) & 255u) << 8) | ((v >> (8 * i)) & 255u), c[i] = i < n ? 1u : 0u;
	// a lane's equal keys: slot j's voxel goes to the first slot with its key (that slot is never one emptied before: its key would have
	// matched an earlier slot first)
#pragma unroll
	for (int j = 1; j < 4; ++j)
	{
		bool merged = false;
#pragma unroll
		for (int i = 0; i < j; ++i)
		{
			const bool m = !merged && k[j] == k[i];
			c[i] += m ? c[j] : 0u;
			merged = merged || m;
		}
		c[j] = merged ? 0u : c[j];
	}
	// the voxels with the lead key: one add of their count, by the first lane
	uint32_t m = 0;        // this lane's voxels with the lead key (one slot at most after the merge: 0..4)
#pragma unroll
	for (int i = 0; i < 4; ++i)
	{
		const bool e = k[i] == lead;
		m += e ? c[i] : 0u;
		c[i] = e ? 0u : c[i];
	}
	const uint32_t total = wave_sum3(m);
	const bool     leads = (int) __lane_id() == first;
	// every add of the item first, then the spill checks
	uint32_t old_lead = 0, old[4];
	if (leads)
		old_lead = hist_add<LDS>(s_hist, a, lead, total);
#pragma unroll
	for (int i = 0; i < 4; ++i)
		old[i] = c[i] ? hist_add<LDS>(s_hist, a, k[i], c[i]) : 0u;
	if (leads)
		hist_spill<LDS>(s_hist, a, lead, total, old_lead);
#pragma unroll
	for (int i = 0; i < 4; ++i)
		if (c[i])
			hist_spill<LDS>(s_hist, a, k[i], c[i], old[i]);
}

// Unit u's dword for this lane, without a branch, so that a round's loads are all in flight before the first is used: the last, partial
// column of a box row of bw >= 4 voxels reads the row's last four bytes (as row_dword) and sh shifts them down later; NARROW (bw < 4) boxes
// read bytes x = min(i, bw - 1).  Lanes past the row or units past the box load the box's first voxel and count nothing (n = 0).
template <bool NARROW>
__device__ __forceinline__ void hist_load(const HistArgs &a, uint64_t u, uint32_t lane, uint32_t &v, uint32_t &g, uint32_t &sh, int &n)
{
	const bool     in = u < a.n_units;
	const uint32_t uu = in ? (uint32_t) u : 0u;
	const uint32_t r = uu / a.blocks_x, cx = uu - r * a.blocks_x, y = r % a.bh, z = r / a.bh;
	const int      x  = 4 * (int) (cx * 64u + lane), bw = (int) a.bw;
	n                 = in ? max(0, min(4, bw - x)) : 0;
	const uint64_t o  = n > 0 ? (uint64_t) z * a.slice + (uint64_t) y * a.W + (uint64_t) (NARROW ? 0 : min(x, bw - 4)) : 0u;
	sh                = NARROW ? 0u : 8u * (uint32_t) (4 - n);
	if (NARROW)
	{
		v = g = 0u;
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
			v |= (uint32_t) a.vol[o + (uint64_t) min(i, bw - 1)] << (8 * i);
			g |= a.grad ? (uint32_t) a.grad[o + (uint64_t) min(i, bw - 1)] << (8 * i) : 0u;
		}
	}
	else
	{
		v = load_u32_any(a.vol + o);
		g = a.grad ? load_u32_any(a.grad + o) : 0u;
	}
}

// LDS: one workgroup of 1024 threads per CU with a private histogram; else 256 threads adding to the 64-bit bins.  A wave's units are
// base + wave + j * stride (j < kHistItems) for a workgroup-uniform base, so every wave of a workgroup runs the same number of rounds;
// the next round's dwords are requested before the current round's keys go to LDS.
template <bool LDS, bool NARROW>
__global__ void __launch_bounds__(LDS ? kHistLdsThreads : kHistGlobalThreads) k_volume_histogram(const HistArgs a)
{
	constexpr uint32_t kWaves = (LDS ? kHistLdsThreads : kHistGlobalThreads) / 64;
	__shared__ uint32_t s_hist[LDS ? kHistWords : 1];
	if (LDS)
	{
		for (uint32_t i = threadIdx.x; i < kHistWords / 4; i += kHistLdsThreads)
			reinterpret_cast<uint4 *>(s_hist)[i] = make_uint4(0u, 0u, 0u, 0u);
		__syncthreads();
	}
	const uint32_t wave   = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)), lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t) gridDim.x * kWaves, round = stride * kHistItems;
	uint32_t       v[kHistItems], g[kHistItems], sh[kHistItems];
	int            n[kHistItems];
	uint64_t       base = (uint64_t) blockIdx.x * kWaves;
#pragma unroll
	for (int j = 0; j < kHistItems; ++j)
		hist_load<NARROW>(a, base + wave + j * stride, lane, v[j], g[j], sh[j], n[j]);
	for (; base < a.n_units; base += round)
	{
		uint32_t nv[kHistItems], ng[kHistItems], nsh[kHistItems];
		int      nn[kHistItems];
#pragma unroll
		for (int j = 0; j < kHistItems; ++j)
			hist_load<NARROW>(a, base + round + wave + j * stride, lane, nv[j], ng[j], nsh[j], nn[j]);
#pragma unroll
		for (int j = 0; j < kHistItems; ++j)
			hist_item<LDS>(s_hist, a, v[j], g[j], sh[j], n[j]);
		if (LDS)        // every spill of the round has landed before any wave adds the next round's voxels
			asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
		for (int j = 0; j < kHistItems; ++j)
			v[j] = nv[j], g[j] = ng[j], sh[j] = nsh[j], n[j] = nn[j];
	}
	if (LDS)
	{        // the non-zero bins, lane-contiguous: each wave instruction covers 64 consecutive bins
		__syncthreads();
		for (uint32_t w = threadIdx.x; w < kHistWords; w += kHistLdsThreads)
		{
			const uint32_t x = s_hist[w];
			if (x & 0xffffu)
				atomicAdd(&a.hist[w], signed_count(x & 0xffffu, a.negate));
			if (x >> 16)
				atomicAdd(&a.hist[w + kHistWords], signed_count(x >> 16, a.negate));
		}
	}
}

__global__ void __launch_bounds__(256) k_histogram_clear(unsigned long long *__restrict__ hist)
{
	for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < kHistBins; i += gridDim.x * 256)
		hist[i] = 0ull;
}

// The bins whose analytic alpha is > 0 (k_tf_bits_analytic's rule: bit row g, or 255 without use_gradient), summed and STORED by one workgroup
__global__ void __launch_bounds__(1024) k_histogram_count(const unsigned long long *__restrict__ hist, unsigned long long *__restrict__ count, float imin,
                                                          float iinv, float gmin, float ginv, int use_gradient)
{
	__shared__ unsigned long long s_wave[16];
	unsigned long long n = 0;
#pragma unroll 16
	for (uint32_t b = threadIdx.x; b < kHistBins; b += 1024)
	{
		const unsigned long long h = hist[b];
		n += analytic_occupied(unorm8(b & 255u), unorm8(use_gradient ? b >> 8 : 255u), imin, iinv, gmin, ginv) ? h : 0ull;
	}
	for (int o = 32; o > 0; o >>= 1)
		n += __shfl_xor(n, o);
	if ((threadIdx.x & 63) == 0)
		s_wave[threadIdx.x >> 6] = n;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		unsigned long long t = 0;
		for (int w = 0; w < 16; ++w)
			t += s_wave[w];
		*count = t;
	}
}

}        // namespace

namespace vkv
{

// vkv_volume_histogram (include/vkvolume_amd.h), after the entry point's argument checks
int launch_volume_histogram(vkv_ctx *ctx, const uint8_t *d_vol, const uint8_t *d_grad, VkvExtent3D e, const VkvBox &b, int mode, uint64_t *d_hist,
                            hipStream_t s)
{
	const uint32_t blocks_x = ((b.width + 3) / 4 + 63) / 64;
	const uint64_t rows = (uint64_t) b.height * b.depth, units = rows * blocks_x, voxels = rows * b.width;
	if (units > 0xffffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "volume_histogram: box too large for one launch");
	const uint64_t first = ((uint64_t) b.z0 * e.height + b.y0) * e.width + b.x0;
	HistArgs       a;
	a.vol = d_vol + first, a.grad = d_grad ? d_grad + first : nullptr;
	a.hist = reinterpret_cast<unsigned long long *>(d_hist);
	a.slice = (uint64_t) e.width * e.height, a.W = e.width, a.bw = b.width, a.bh = b.height, a.blocks_x = blocks_x, a.n_units = (uint32_t) units;
	a.negate = mode == VKV_HISTOGRAM_SUBTRACT;
	if (mode == VKV_HISTOGRAM_SET)        // a kernel, not a memset node (vkv_update_transfer_function: memset nodes were unreliable under graph replay)
		hipLaunchKernelGGL(k_histogram_clear, dim3(64), dim3(256), 0, s, a.hist);
	if (voxels <= kHistGlobalMaxVoxels)
	{
		const uint64_t per_group = (uint64_t) (kHistGlobalThreads / 64) * kHistItems;
		const uint32_t groups    = (uint32_t) std::min<uint64_t>(1024, (units + per_group - 1) / per_group);
		if (b.width >= 4)
			hipLaunchKernelGGL((k_volume_histogram<false, false>), dim3(groups), dim3(kHistGlobalThreads), 0, s, a);
		else
			hipLaunchKernelGGL((k_volume_histogram<false, true>), dim3(groups), dim3(kHistGlobalThreads), 0, s, a);
	}
	else
	{
		const uint32_t groups = (uint32_t) std::min<uint64_t>((uint64_t) std::max(1, ctx->cu_count), std::max<uint64_t>(1, voxels >> kHistVoxelsPerGroupLog2));
		if (b.width >= 4)
			hipLaunchKernelGGL((k_volume_histogram<true, false>), dim3(groups), dim3(kHistLdsThreads), 0, s, a);
		else
			hipLaunchKernelGGL((k_volume_histogram<true, true>), dim3(groups), dim3(kHistLdsThreads), 0, s, a);
	}
	return check_launch(ctx, "volume_histogram");
}

int launch_histogram_occupied_count(vkv_ctx *ctx, const uint64_t *d_hist, const VkvTransferFunctionUniform *tf, uint64_t *d_count, hipStream_t s)
{
	hipLaunchKernelGGL(k_histogram_count, dim3(1), dim3(1024), 0, s, reinterpret_cast<const unsigned long long *>(d_hist),
	                   reinterpret_cast<unsigned long long *>(d_count), tf->intensity_min, tf->intensity_range_inv, tf->gradient_min, tf->gradient_range_inv,
	                   (int) (tf->use_gradient != 0));
	return check_launch(ctx, "histogram_occupied_count");
}

}        // namespace vkv

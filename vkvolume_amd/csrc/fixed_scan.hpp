// fixed_scan.hpp — the schedule-independent reductions of the kernels that count, scan and emit (mesh.hip, mesh_indexed.hip, components.hip):
// sums and prefixes over a wave, an exclusive scan over a workgroup, and the two-level scan of per-entry counts (each chunk of kScanChunk
// entries on its own in uint32, then the chunk sums by one workgroup in uint64).  All of them are fixed trees: the result does not depend on
// scheduling.  Device code only, and nothing about what is counted.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vkv
{

constexpr uint32_t kScanChunk = 4096;        // entries a scan workgroup takes: 256 threads x 16

// the chunks of `entries` entries (host)
inline uint32_t scan_chunks(uint32_t entries) { return (entries + kScanChunk - 1) / kScanChunk; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t n)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		n += (uint32_t) __shfl_xor((int) n, o);
	return n;
}

// exclusive prefix of n over the wave's lanes
__device__ __forceinline__ uint32_t wave_exclusive(uint32_t n, uint32_t lane)
{
	uint32_t incl = n;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1)
	{
		const uint32_t up = (uint32_t) __shfl_up((int) incl, o);
		incl += lane >= (uint32_t) o ? up : 0u;
	}
	return incl - n;
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

// chunk c = entries [4096 c, 4096 c + 4096), one workgroup: local[e] = the sum of the chunk's entries before e, sums[c] = the chunk's sum.
// PACKED: an entry carries two counts, the scanned one in its low 16 bits and a second one above them that is only summed, into sums_high[c]
template <bool PACKED = false>
__device__ __forceinline__ void scan_chunk(const uint32_t *__restrict__ counts, uint32_t *__restrict__ local, uint64_t *__restrict__ sums, uint32_t n_entries,
                                           uint64_t *__restrict__ sums_high = nullptr)
{
	__shared__ uint32_t lds[256];
	constexpr uint32_t  kPer  = kScanChunk / 256;
	const uint32_t      first = blockIdx.x * kScanChunk + threadIdx.x * kPer;
	uint32_t            c[kPer], mine = 0, mine_high = 0;
#pragma unroll
	for (uint32_t k = 0; k < kPer; ++k)
	{
		const uint32_t both = first + k < n_entries ? counts[first + k] : 0u;
		c[k]                = PACKED ? both & 0xffffu : both;
		mine += c[k], mine_high += both >> 16;
	}
	uint32_t total, total_high = 0;
	uint32_t before = block_exclusive_scan(mine, lds, total);
	if (PACKED)
		(void) block_exclusive_scan(mine_high, lds, total_high);
#pragma unroll
	for (uint32_t k = 0; k < kPer; ++k)
	{
		if (first + k < n_entries)
			local[first + k] = before;
		before += c[k];
	}
	if (threadIdx.x == 0)
	{
		sums[blockIdx.x] = total;
		if (PACKED)
			sums_high[blockIdx.x] = total_high;
	}
}

// one workgroup: sums[c] becomes the sum of the chunks before c; d_counts[0] = the total, d_counts[1] = min(total, capacity)
__device__ __forceinline__ void scan_total(uint64_t *__restrict__ sums, uint32_t n_chunks, uint64_t capacity, uint64_t *__restrict__ d_counts)
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

}        // namespace vkv

// volume_io.hip — how voxels and pixels get into place: the synthetic volumes (vkv_synth_volume), the loader's conversion of raw
// 8 / 16-bit elements on the device (whole volume, or the box of a region update) and the multi-GPU scatter of gathered tile buffers into
// the final images.  One thread per element (or 16 bytes of them); nothing here is on a frame's critical path.
#include <cmath>

#include "launchers.hpp"

using namespace vkv;

// ---------------------------------------------------------------------------------------------
// Synthetic volumes (DESIGN.md "Synthetic inputs")
// ---------------------------------------------------------------------------------------------
struct SynthShell
{
	float cx, cy, cz, irx, iry, irz, slope, amp, lo2, hi2;
};
constexpr int kSynthShells = 40;
struct SynthArgs
{
	SynthShell sh[kSynthShells];
};

__device__ __forceinline__ uint32_t synth_hash(uint32_t seed, uint32_t x, uint32_t y, uint32_t z)
{
	uint32_t h = seed ^ (x * 0x8da6b343u) ^ (y * 0xd8163841u) ^ (z * 0xcb1ab31fu);
	h ^= h >> 16;
	h *= 0x7feb352du;
	h ^= h >> 15;
	h *= 0x846ca68bu;
	h ^= h >> 16;
	return h;
}

__global__ void __launch_bounds__(256) k_synth_sphere(uint8_t *__restrict__ vol, int W, int H, int D, uint32_t blocks_x)
{
	const uint32_t bx = blockIdx.x % blocks_x;
	const int      x  = (int) (bx * 64 + (threadIdx.x & 63));
	const int      y  = (int) ((blockIdx.x / blocks_x) * 4 + (threadIdx.x >> 6)), z = (int) blockIdx.y;        // grid.y = z
	if (x >= W || y >= H)
		return;
	const float dm = (float) max(max(W, H), D);
	const float R0 = 0.375f * dm, R1 = 0.25f * dm;
	const float cx = ((float) W - 1.0f) * 0.5f, cy = ((float) H - 1.0f) * 0.5f, cz = ((float) D - 1.0f) * 0.5f;
	const float dx = (float) x - cx, dy = (float) y - cy, dz = (float) z - cz;
	const float r  = __builtin_sqrtf(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)));
	const float t  = g_clamp((R0 - r) / (R0 - R1), 0.0f, 1.0f);
	vol[vidx(x, y, z, W, H)] = (uint8_t) __builtin_rintf(255.0f * t);
}

__global__ void __launch_bounds__(256) k_synth_shells(uint8_t *__restrict__ vol, int W, int H, int D, uint32_t seed, uint32_t blocks_x, int n_shells, uint32_t noise_mod,
                                                      SynthArgs args)
{
	__shared__ SynthShell s_sh[kSynthShells];
	for (int i = threadIdx.x; i < kSynthShells * 10; i += 256)
		reinterpret_cast<float *>(s_sh)[i] = reinterpret_cast<const float *>(args.sh)[i];
	__syncthreads();
	const uint32_t bx = blockIdx.x % blocks_x;
	const int      x  = (int) (bx * 64 + (threadIdx.x & 63));
	const int      y  = (int) ((blockIdx.x / blocks_x) * 4 + (threadIdx.x >> 6)), z = (int) blockIdx.y;        // grid.y = z
	if (x >= W || y >= H)
		return;
	float best = 0.0f;
	for (int k = 0; k < n_shells; ++k)
	{
		const float dx = ((float) x - s_sh[k].cx) * s_sh[k].irx;
		const float dy = ((float) y - s_sh[k].cy) * s_sh[k].iry;
		const float dz = ((float) z - s_sh[k].cz) * s_sh[k].irz;
		const float q2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
		if (q2 > s_sh[k].lo2 && q2 < s_sh[k].hi2)
		{
			const float q   = __builtin_sqrtf(q2);
			const float val = s_sh[k].amp * (1.0f - __builtin_fabsf(q - 1.0f) * s_sh[k].slope);
			if (val > best)
				best = val;
		}
	}
	const uint32_t noise = synth_hash(seed, (uint32_t) x, (uint32_t) y, (uint32_t) z) % noise_mod;
	const uint32_t v     = (uint32_t) best + noise;
	vol[vidx(x, y, z, W, H)] = (uint8_t) min(v, 255u);
}

// ---------------------------------------------------------------------------------------------
// Loader conversion on the device (src/load_volume.cpp:151-169): 16 input bytes per thread
// ---------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ uint8_t normalise_voxel(T raw, bool swap, float lo, float hi)
{
	if (sizeof(T) == 2 && swap)
		raw = (T) (uint16_t) ((((uint16_t) raw) >> 8) | (((uint16_t) raw) << 8));
	const float x = ((float) raw - lo) / (hi - lo);
	const float a = (x < 1.0f) ? x : 1.0f;          // std::min(1.0f, x)
	const float t = (0.0f < a) ? a : 0.0f;          // std::max(0.0f, .)
	return (uint8_t) (255 * t);                      // truncation (load_volume.cpp:169)
}

template <typename T>
__global__ void __launch_bounds__(256) k_convert_volume(const T *__restrict__ raw, uint8_t *__restrict__ out, unsigned long long n, bool swap, float lo, float hi)
{
	constexpr int kPer = 16 / (int) sizeof(T);        // elements per 16-byte load
	const unsigned long long first = ((unsigned long long) blockIdx.x * 256 + threadIdx.x) * kPer;
	if (first >= n)
		return;
	if (first + kPer <= n && (((uintptr_t) raw) & 15u) == 0 && (((uintptr_t) out) & (kPer - 1)) == 0)
	{
		const uint4 q = *reinterpret_cast<const uint4 *>(raw + first);
		T           e[kPer];
		__builtin_memcpy(e, &q, 16);
		uint8_t o[kPer];
#pragma unroll
		for (int i = 0; i < kPer; ++i)
			o[i] = normalise_voxel<T>(e[i], swap, lo, hi);
		if (kPer == 16)
			*reinterpret_cast<uint4 *>(out + first) = *reinterpret_cast<const uint4 *>(o);
		else
			*reinterpret_cast<uint2 *>(out + first) = *reinterpret_cast<const uint2 *>(o);
	}
	else
		for (unsigned long long i = first; i < n && i < first + kPer; ++i)
			out[i] = normalise_voxel<T>(raw[i], swap, lo, hi);
}

// The same conversion for a box of the volume (vkv_update_volume_region): raw holds bw x bh x (rows / bh) elements, x fastest; element
// (x, y, z) goes to voxel (x0 + x, y0 + y, z0 + z).  A workgroup converts 256 elements of a row (`chunks_x` of them per row), grid-stride
// over the rows.
template <typename T>
__global__ void __launch_bounds__(256) k_convert_box(const T *__restrict__ raw, uint8_t *__restrict__ out, int W, int H, int x0, int y0, int z0, int bw,
                                                     int bh, unsigned long long rows, uint32_t chunks_x, bool swap, float lo, float hi)
{
	for (unsigned long long b = blockIdx.x; b < rows * chunks_x; b += gridDim.x)
	{
		const unsigned long long row = b / chunks_x;
		const int                x   = (int) (b - row * chunks_x) * 256 + (int) threadIdx.x;
		if (x >= bw)
			continue;
		const int y = (int) (row % (unsigned) bh), z = (int) (row / (unsigned) bh);
		out[vidx(x0 + x, y0 + y, z0 + z, W, H)] = normalise_voxel<T>(raw[row * (unsigned) bw + (unsigned) x], swap, lo, hi);
	}
}

// ---------------------------------------------------------------------------------------------
// Multi-GPU: de-interleave gathered compact tile buffers into the final image(s) (one thread per pixel, or per four RGBA8 pixels).
// blockIdx.z = frame of the launch; each frame has its own image, source ([rank][tiles], `stride` tiles between two ranks' buffers) and
// tile rectangle (tiles numbered row-major inside it, tile t on rank t % n_ranks as its (t / n_ranks)-th); pixels outside the rectangle
// are cleared, so the image is complete after the kernel.
// ---------------------------------------------------------------------------------------------
struct ScatterFrame
{
	void *      image;
	const void *src;
	uint32_t    rx0, ry0, rw, rh;        // the tile rectangle
	uint32_t    stride;                  // tiles between the buffers of two ranks
	uint32_t    pad;
};
struct ScatterFrames
{
	ScatterFrame f[VKV_MAX_BATCH];
};

template <typename T>
__global__ void __launch_bounds__(256) k_scatter_tiles_frames(const ScatterFrames frames, uint32_t iw, uint32_t ih, uint32_t tw, uint32_t th, uint32_t n_ranks)
{
	const uint32_t x = blockIdx.x * 64 + (threadIdx.x & 63);
	const uint32_t y = blockIdx.y * 4 + (threadIdx.x >> 6);
	if (x >= iw || y >= ih)
		return;
	const ScatterFrame &F  = frames.f[blockIdx.z];
	const uint32_t      tx = x / tw - F.rx0, ty = y / th - F.ry0;        // (wraps to a huge value left of / above the rectangle)
	T                   v  = {};
	if (tx < F.rw && ty < F.rh)
	{
		const uint32_t t    = ty * F.rw + tx;
		const uint32_t rank = t % n_ranks, k = t / n_ranks;
		v = static_cast<const T *>(F.src)[(((size_t) rank * F.stride + k) * th + (y % th)) * tw + (x % tw)];
	}
	static_cast<T *>(F.image)[(size_t) y * iw + x] = v;
}

namespace vkv
{

// --- synthetic volume: host builds the shell table (same definition as DESIGN.md "Synthetic inputs") ---
static uint64_t splitmix64(uint64_t *s)
{
	uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
	z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}
static float u01(uint64_t *s) { return (float) (splitmix64(s) >> 40) * (1.0f / 16777216.0f); }

int launch_synth_volume(vkv_ctx *ctx, uint8_t *d_vol, VkvExtent3D e, uint32_t kind, uint32_t seed, hipStream_t s)
{
	const uint32_t blocks_x = (e.width + 63) / 64;
	if (e.depth > 65535u || (uint64_t) blocks_x * ((e.height + 3) / 4) > 0xffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "synth_volume: volume too large for one launch");
	const dim3 grid(blocks_x * ((e.height + 3) / 4), e.depth);
	const int  W = (int) e.width, H = (int) e.height, D = (int) e.depth;
	if ((kind & 255u) == 0)
	{
		hipLaunchKernelGGL(k_synth_sphere, grid, dim3(256), 0, s, d_vol, W, H, D, blocks_x);
		return check_launch(ctx, "synth_volume");
	}
	if ((kind & 255u) != 1)
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "synth_volume: unknown kind %u", kind & 255u);
	// kind = 1 | shells << 8 | thickness << 16 | noise << 28: the first `shells` (0 = all 40) of the seed's shells, their thickness scaled by
	// thickness / 256 (12 bits, 0 = 1), hash noise 0 .. noise (4 bits, 0 = the default 0 .. 20)
	const uint32_t nq = (kind >> 8) & 255u, tq = (kind >> 16) & 0xfffu, noise_mod = (kind >> 28) ? (kind >> 28) + 1u : 21u;
	const int      n_shells = nq && nq < (uint32_t) kSynthShells ? (int) nq : kSynthShells;
	SynthArgs   args;
	uint64_t    st = (0x5EEDull << 32) | (uint64_t) seed;
	const float Wf = (float) e.width, Hf = (float) e.height, Df = (float) e.depth;
	const float dm = fmaxf(fmaxf(Wf, Hf), Df);
	const float th = (0.001f * dm + 1.0f) * (tq ? (float) tq * (1.0f / 256.0f) : 1.0f);
	for (int k = 0; k < kSynthShells; ++k)
	{
		SynthShell &sh = args.sh[k];
		sh.cx          = (0.15f + 0.70f * u01(&st)) * Wf;
		sh.cy          = (0.15f + 0.70f * u01(&st)) * Hf;
		sh.cz          = (0.15f + 0.70f * u01(&st)) * Df;
		const float r  = (0.05f + 0.13f * u01(&st)) * dm;
		const float rx = r * (0.7f + 0.6f * u01(&st));
		const float ry = r * (0.7f + 0.6f * u01(&st));
		const float rz = r * (0.7f + 0.6f * u01(&st));
		sh.irx = 1.0f / rx, sh.iry = 1.0f / ry, sh.irz = 1.0f / rz;
		sh.slope       = fminf(fminf(rx, ry), rz) / th;
		sh.amp         = 110.0f + 145.0f * u01(&st);
		const float w  = 1.0f / sh.slope + 0.001f;
		const float lo = 1.0f - w, hi = 1.0f + w;
		sh.lo2 = lo > 0.0f ? lo * lo : 0.0f;
		sh.hi2 = hi * hi;
	}
	hipLaunchKernelGGL(k_synth_shells, grid, dim3(256), 0, s, d_vol, W, H, D, seed, blocks_x, n_shells, noise_mod, args);
	return check_launch(ctx, "synth_volume");
}

// 16-bit elements of a file in this byte order need a swap (the device shares the host's byte order)
static bool swap_for(bool big_endian)
{
	const uint16_t probe = 1;
	return big_endian == (*reinterpret_cast<const uint8_t *>(&probe) == 1);
}

int launch_convert_volume(vkv_ctx *ctx, const void *d_raw, int type, bool big_endian, float lo, float hi, uint64_t n, uint8_t *d_out, hipStream_t s)
{
	const bool     swap           = swap_for(big_endian);
	const int      per            = (type == VKV_VOXEL_UINT16 || type == VKV_VOXEL_INT16) ? 8 : 16;
	const uint64_t blocks         = (n + (uint64_t) per * 256 - 1) / ((uint64_t) per * 256);
	if (blocks == 0)
		return VKV_OK;
	if (blocks > 0xffffffull)
		return set_error(ctx, VKV_E_UNSUPPORTED, "convert_volume: volume too large for one launch");
	const unsigned long long nn = n;
	switch (type)
	{
		case VKV_VOXEL_UINT8: hipLaunchKernelGGL(k_convert_volume<uint8_t>, dim3((uint32_t) blocks), dim3(256), 0, s, (const uint8_t *) d_raw, d_out, nn, swap, lo, hi); break;
		case VKV_VOXEL_INT8: hipLaunchKernelGGL(k_convert_volume<int8_t>, dim3((uint32_t) blocks), dim3(256), 0, s, (const int8_t *) d_raw, d_out, nn, swap, lo, hi); break;
		case VKV_VOXEL_UINT16: hipLaunchKernelGGL(k_convert_volume<uint16_t>, dim3((uint32_t) blocks), dim3(256), 0, s, (const uint16_t *) d_raw, d_out, nn, swap, lo, hi); break;
		case VKV_VOXEL_INT16: hipLaunchKernelGGL(k_convert_volume<int16_t>, dim3((uint32_t) blocks), dim3(256), 0, s, (const int16_t *) d_raw, d_out, nn, swap, lo, hi); break;
		default: return set_error(ctx, VKV_E_INVALID_ARGUMENT, "convert_volume: unsupported image data type %d", type);
	}
	return check_launch(ctx, "convert_volume");
}

// `n` frames (1 .. VKV_MAX_BATCH) described by images[f], srcs[f], rects[f] (a rectangle of whole tiles inside the image), strides[f]
int launch_scatter_tiles_frames(vkv_ctx *ctx, uint32_t n, void *const *images, const void *const *srcs, const VkvTileRect *rects, const uint32_t *strides, uint32_t iw,
                                uint32_t ih, uint32_t tw, uint32_t th, uint32_t n_ranks, uint32_t bpp, hipStream_t s)
{
	ScatterFrames fr{};
	bool          aligned = true;
	for (uint32_t f = 0; f < n; ++f)
	{
		fr.f[f] = ScatterFrame{images[f], srcs[f], rects[f].x0, rects[f].y0, rects[f].w, rects[f].h, strides[f], 0u};
		aligned = aligned && (((uintptr_t) images[f] | (uintptr_t) srcs[f]) & 15u) == 0;
	}
	if (bpp == 4 && (iw % 4) == 0 && (tw % 4) == 0 && aligned)
		// RGBA8: four pixels per thread (a 16-pixel tile row = 64 B = 4 threads)
		hipLaunchKernelGGL(k_scatter_tiles_frames<uint4>, dim3((iw / 4 + 63) / 64, (ih + 3) / 4, n), dim3(256), 0, s, fr, iw / 4, ih, tw / 4, th, n_ranks);
	else if (bpp == 4)
		hipLaunchKernelGGL(k_scatter_tiles_frames<uint32_t>, dim3((iw + 63) / 64, (ih + 3) / 4, n), dim3(256), 0, s, fr, iw, ih, tw, th, n_ranks);
	else if (bpp == 16)
		hipLaunchKernelGGL(k_scatter_tiles_frames<uint4>, dim3((iw + 63) / 64, (ih + 3) / 4, n), dim3(256), 0, s, fr, iw, ih, tw, th, n_ranks);
	else
		return set_error(ctx, VKV_E_INVALID_ARGUMENT, "scatter_tiles: bytes_per_pixel must be 4 or 16");
	return check_launch(ctx, "scatter_tiles");
}

// the same conversion for the elements of `box` (x fastest, box.width x box.height x box.depth of them) into the box's voxels of the volume e
int launch_convert_box(vkv_ctx *ctx, const void *d_raw, int type, bool big_endian, float lo, float hi, const VkvBox &box, uint8_t *d_vol, VkvExtent3D e,
                       hipStream_t s)
{
	const bool               swap = swap_for(big_endian);
	const unsigned long long rows = (unsigned long long) box.height * box.depth;
	const uint32_t chunks_x       = (box.width + 255) / 256;
	const uint32_t blocks         = (uint32_t) std::min<unsigned long long>(rows * chunks_x, 1ull << 20);
	const int      W = (int) e.width, H = (int) e.height, x0 = (int) box.x0, y0 = (int) box.y0, z0 = (int) box.z0, bw = (int) box.width, bh = (int) box.height;
#define VKV_CONVERT_BOX(T) hipLaunchKernelGGL(k_convert_box<T>, dim3(blocks), dim3(256), 0, s, (const T *) d_raw, d_vol, W, H, x0, y0, z0, bw, bh, rows, chunks_x, swap, lo, hi)
	switch (type)
	{
		case VKV_VOXEL_UINT8: VKV_CONVERT_BOX(uint8_t); break;
		case VKV_VOXEL_INT8: VKV_CONVERT_BOX(int8_t); break;
		case VKV_VOXEL_UINT16: VKV_CONVERT_BOX(uint16_t); break;
		default: VKV_CONVERT_BOX(int16_t); break;        // VKV_VOXEL_INT16 (the type was checked)
	}
#undef VKV_CONVERT_BOX
	return check_launch(ctx, "update_volume_region: convert");
}

}        // namespace vkv

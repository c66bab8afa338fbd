// slab_host_driver.cpp — one VolumeRenderSubpass::draw_slab frame through the C++ host mirror (tests/test_gpu_slab.py builds and runs it).
//   slab_host_driver W H D volume.raw slab.bin WIDTH HEIGHT SKIP BLOCK out_prefix
// volume.raw: W*H*D uint8 voxels; slab.bin: the bytes of a VkvSlabOptions (its pointers are ignored).  Writes out_prefix.rgba8, .value, .counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "volume_render_subpass.h"

namespace
{

std::vector<uint8_t> read_file(const std::string &name)
{
	std::vector<uint8_t> b;
	FILE *               f = std::fopen(name.c_str(), "rb");
	if (!f)
		throw std::runtime_error("cannot open " + name);
	uint8_t buf[65536];
	for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;)
		b.insert(b.end(), buf, buf + n);
	std::fclose(f);
	return b;
}

template <typename T>
void dump(const std::string &name, const T *device, size_t count, hipStream_t stream)
{
	std::vector<T> h(count);
	if (hipMemcpyAsync(h.data(), device, count * sizeof(T), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
		throw std::runtime_error("copy of " + name + " failed");
	FILE *f = std::fopen(name.c_str(), "wb");
	if (!f || std::fwrite(h.data(), sizeof(T), count, f) != count)
		throw std::runtime_error("cannot write " + name);
	std::fclose(f);
}

template <typename T>
T *device_alloc(size_t count)
{
	void *p = nullptr;
	if (hipMalloc(&p, count * sizeof(T)) != hipSuccess)
		throw std::runtime_error("hipMalloc failed");
	return static_cast<T *>(p);
}

}        // namespace

int main(int argc, char **argv)
{
	try
	{
		if (argc != 11)
			throw std::runtime_error("usage: slab_host_driver W H D volume.raw slab.bin WIDTH HEIGHT SKIP BLOCK out_prefix");
		const VkvExtent3D extent{(uint32_t) std::atoi(argv[1]), (uint32_t) std::atoi(argv[2]), (uint32_t) std::atoi(argv[3])};
		const auto        voxels = read_file(argv[4]);
		const auto        raw    = read_file(argv[5]);
		if (voxels.size() != (size_t) extent.width * extent.height * extent.depth || raw.size() != sizeof(VkvSlabOptions))
			throw std::runtime_error("volume or options file of the wrong size");
		VkvSlabOptions slab;
		std::memcpy(&slab, raw.data(), sizeof(slab));
		const uint32_t    width = (uint32_t) std::atoi(argv[6]), height = (uint32_t) std::atoi(argv[7]);
		const bool        skip   = std::atoi(argv[8]) != 0;
		const uint32_t    block  = (uint32_t) std::atoi(argv[9]);
		const std::string prefix = argv[10];

		vkv_ctx *ctx = nullptr;
		if (vkv_create(0, &ctx) != VKV_OK)
			throw std::runtime_error("no gfx950 device");
		hipStream_t stream = nullptr;
		if (hipStreamCreate(&stream) != hipSuccess)
			throw std::runtime_error("hipStreamCreate failed");
		DeviceContext dc{ctx, stream};
		Volume        volume("slab");
		volume.load_from_memory(dc, voxels.data(), extent, block);
		volume.set_image_transform(vkv::scale(vkv::vec3{(float) extent.width, (float) extent.height, (float) extent.depth}));
		if (skip)
			volume.build_max_map(dc);
		Camera              camera;        // a slab reads no camera: the identity will do
		VolumeRenderSubpass subpass(dc, {&volume}, camera, VolumeRenderSubpass::Options{});
		const size_t        n = (size_t) width * height;
		RenderTarget        target;
		target.width = width, target.height = height;
		target.rgba8  = device_alloc<uint8_t>(n * 4);
		target.counts = device_alloc<uint32_t>(n * 3);
		slab.d_max_map   = nullptr;
		slab.d_out_value = device_alloc<float>(n);
		subpass.draw_slab(target, slab, skip);
		dump(prefix + ".rgba8", target.rgba8, n * 4, stream);
		dump(prefix + ".value", slab.d_out_value, n, stream);
		dump(prefix + ".counts", target.counts, n * 3, stream);
		// without the max map a skipping MAX slab is an error of the caller
		bool threw = false;
		if (!skip && slab.mode == VKV_SLAB_MAX)
		{
			try
			{
				subpass.draw_slab(target, slab, true);
			}
			catch (const std::runtime_error &)
			{
				threw = true;
			}
			std::printf("skip without a max map: %s\n", threw ? "refused" : "accepted");
		}
		(void) hipStreamSynchronize(stream);
		(void) hipFree(target.rgba8), (void) hipFree(target.counts), (void) hipFree(slab.d_out_value);
		(void) hipStreamDestroy(stream);
		vkv_destroy(ctx);
		std::printf("slab: %ux%u pixels, %u samples, mode %d\n", width, height, slab.samples, slab.mode);
		return 0;
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "slab_host_driver: %s\n", e.what());
		return 1;
	}
}

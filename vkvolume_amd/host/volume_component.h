// volume_component.h — Volume, the reference's scene component that owns every per-volume GPU resource
// (src/volume_component.h:31-93).  Vulkan images become linear HIP device buffers; the RenderContext / CommandBuffer
// parameters become a DeviceContext (vkv context + HIP stream).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vkvolume_amd.h"
#include "transfer_function.h"
#include "vkv_math.hpp"

// Stand-in for vkb::RenderContext& / vkb::CommandBuffer& on this path: where to enqueue.
struct DeviceContext
{
	vkv_ctx *ctx    = nullptr;
	void *   stream = nullptr;        // hipStream_t
};

class Volume
{
  public:
	explicit Volume(const std::string &name);
	~Volume();
	Volume(const Volume &) = delete;
	Volume &operator=(const Volume &) = delete;

	// src/volume_component.cpp:55-153: header + data from disk, device buffers, volume upload.  Always returns true (errors throw).
	bool load_from_file(DeviceContext &dc, std::string filename, uint32_t distance_map_block_size = 4);
	// Same resource set-up from voxels already in host memory / generated on the device (offscreen driver, tests).
	bool load_from_memory(DeviceContext &dc, const uint8_t *voxels, VkvExtent3D extent, uint32_t distance_map_block_size = 4);
	bool load_synthetic(DeviceContext &dc, VkvExtent3D extent, uint32_t kind, uint32_t seed, uint32_t distance_map_block_size = 4);

	void set_image_transform(const vkv::mat4 &mat);
	void set_number_of_distance_maps(DeviceContext &dc, size_t n);        // grow-only (src/volume_component.cpp:155-184)

	// Volume::Options, src/volume_component.h:45-56 (same defaults)
	struct Options
	{
		float sampling_factor          = 1.0f;
		float voxel_alpha_factor       = 1.0f;
		bool  use_precomputed_gradient = true;
		float intensity_min            = 0.0f;
		float intensity_max            = 1.0f;
		float gradient_min             = 0.0f;
		float gradient_max             = 1.0f;
	} options;

	// Volume::Image: a device buffer instead of image + view + sampler
	struct Image
	{
		uint8_t *   data = nullptr;
		VkvExtent3D extent{0, 0, 0};
		uint32_t    bytes_per_texel = 1;
		size_t      size_bytes() const { return (size_t) extent.width * extent.height * extent.depth * bytes_per_texel; }
	};

	const Image &get_volume() const { return volume; }
	const Image &get_gradient() const { return gradient; }
	const Image &get_transfer_function() const { return transfer_function; }
	const Image &get_distance_map(size_t idx = 0) const { return distance_maps.at(idx); }
	const Image &get_distance_map_swap() const { return distance_map_swap; }
	size_t       get_number_of_distance_maps() const { return distance_maps.size(); }
	vkv::mat4 &  get_image_transform() { return image_transform; }
	const std::string &get_name() const { return name; }

	TransferFunctionUniform get_transfer_function_uniform();                 // src/volume_component.cpp:226-240
	void                    update_transfer_function_texture(DeviceContext &dc);        // src/volume_component.cpp:242-278
	// the same texture + tables built on the device (vkv_transfer_function_texture_device): no host loop, no upload, no wait
	void update_transfer_function_on_device(DeviceContext &dc);
	// VolumeRender::update_transfer_function (src/volume_render.cpp:392-445) as one enqueue (vkv_update_transfer_function): texture + tables,
	// occupancy and the transform of skipping_type (a VkvSkippingType) into the distance maps (grown as ComputeDistanceMap::compute grows them);
	// d_occupied_count != nullptr also receives the occupied-voxel count
	void update_transfer_function(DeviceContext &dc, int32_t skipping_type, uint64_t *d_occupied_count = nullptr);
	// New voxels for a box (vkv_update_volume_region): host_raw holds box.width * height * depth raw elements of `type` (a VkvVoxelType, x
	// fastest; a z-slab of a raw file), converted like the loader converts a file (byte order, normalisation range[0] .. range[1]); the
	// gradient, the packed image (if built) and the maps of skipping_type (if built) are rebuilt where the box reaches them, on dc.stream.
	// The raw bytes are staged in a device buffer the volume keeps (grown as needed); host_raw may be reused when the call returns.
	void update_region(DeviceContext &dc, VkvBox box, const void *host_raw, int32_t type, bool big_endian, const float range[2], int32_t skipping_type);
	// Joint (gradient byte, intensity byte) histogram of `box` (nullptr: the whole volume) into the VKV_HISTOGRAM_BINS uint64 bins at
	// d_histogram, set / added / subtracted as `mode` (a VkvHistogramMode) says (vkv_volume_histogram), on dc.stream; the gradient map is used
	// when options.use_precomputed_gradient is set, else every voxel counts in gradient row 0
	void histogram(DeviceContext &dc, uint64_t *d_histogram, const VkvBox *box = nullptr, int32_t mode = VKV_HISTOGRAM_SET);
	// Per-cell summaries of the occupancy map (vkv_cell_summary) of every cell (box == nullptr) or of the cells that meet `box`, into a device
	// buffer the volume allocates at the first call (build the whole summary first); built from the gradient map when
	// options.use_precomputed_gradient is set.  update_region keeps a built summary current (it rebuilds the update's box grown by one voxel).
	void cell_summary(DeviceContext &dc, const VkvBox *box = nullptr);
	const void *get_cell_summary() const { return cell_summary_buf; }
	// The max map (vkv_max_map: per occupancy cell the largest voxel of the cell grown by one voxel per side) of every cell (box == nullptr) or of
	// the cells whose grown box meets `box`, into a device buffer the volume allocates at the first call (build the whole map first).
	// update_region keeps a built map current.  VolumeRenderSubpass::draw_mip skips over it.
	void build_max_map(DeviceContext &dc, const VkvBox *box = nullptr);
	const uint8_t *get_max_map() const { return max_map_buf; }
	// update_transfer_function with the occupancy map decided from the summary (vkv_update_transfer_function_from_summary; call cell_summary
	// first): same texture, tables and maps.  d_occupied_count needs d_histogram (a histogram() of the volume); d_unresolved receives the
	// number of cells evaluated from their voxels
	void update_transfer_function_from_summary(DeviceContext &dc, int32_t skipping_type, uint64_t *d_occupied_count = nullptr,
	                                           const uint64_t *d_histogram = nullptr, uint64_t *d_unresolved = nullptr);

	// vkb::sg::Node stand-in: the node's world matrix (benchmark mode rescales it, src/volume_render.cpp:224-238)
	vkv::mat4 node_transform;

	// device-internal accelerators of the ray-marcher (see include/vkvolume_amd.h)
	void            pack(DeviceContext &dc);
	const void *    get_packed_volume() const { return packed; }
	const uint32_t *get_transfer_function_bits() const { return transfer_function_bits; }

  private:
	void allocate(DeviceContext &dc, VkvExtent3D extent, uint32_t block);
	void release();

	std::string        name;
	Image              volume, gradient, transfer_function;
	std::vector<Image> distance_maps;
	Image              distance_map_swap;
	void *             packed                 = nullptr;
	size_t             packed_bytes           = 0;
	uint32_t *         transfer_function_bits = nullptr;
	void *             region_staging         = nullptr;        // update_region's device copy of the raw box
	size_t             region_staging_bytes   = 0;
	void *             cell_summary_buf       = nullptr;        // cell_summary's VKV_CELL_SUMMARY_BYTES per occupancy cell
	uint8_t *          max_map_buf            = nullptr;        // build_max_map's byte per occupancy cell
	vkv::mat4          image_transform;
};

/*
 * vkvolume_amd.h — C ABI of the MI355X-native volume ray-caster hot path.
 *
 * This is the drop-in boundary: every entry point below replaces one
 * Vulkan dispatcher of the reference (LDeakin/VkVolume) and is what a maintainer's FFI
 * would bind.  Plain C types only: device pointers, sizes, POD structs, an opaque
 * context and a `void *stream` that is a `hipStream_t`.
 *
 * Conventions
 *   - every function returns 0 on success, a negative VKV_E_* code for argument /
 *     capability errors, or a positive `hipError_t` value when the HIP runtime failed;
 *   - device functions ENQUEUE on `stream` and do not synchronise (the reference's
 *     compute_submit() fence wait, src/volume_render.cpp:301-327, is the caller's job).
 *     They neither allocate device memory nor wait for the device once the SET-UP calls below
 *     (vkv_create, vkv_prepare_render, vkv_register_target; marked "set-up call") have seen the
 *     shapes, streams and targets they are used with: the small device tables a launch needs
 *     (tile start order, address tables, per-stream scratch) come out of an arena allocated by
 *     vkv_create and are uploaded asynchronously on the launch's stream from a pinned host copy;
 *     nothing is ever freed or re-used while a launch could still read it (only vkv_trim,
 *     vkv_forget_target, vkv_release_stream and vkv_destroy give device memory back, and they
 *     say what they wait for).  GROWTH: every distinct (frame size, tile schedule) and every
 *     distinct volume extent a context has rendered keeps one cached table (32 KiB for a
 *     1920x1080 frame of 16x16 tiles); the arena's table region (default 6 MiB of 8) holds
 *     ~190 such sizes.  When it is full, launches run without the table (plain tile order,
 *     address arithmetic in registers: the same bits, a few per cent slower) until vkv_trim
 *     empties it; the scratch blocks of streams have a region of their own (16 streams) and
 *     are never starved by tables;
 *   - THREADS: any number of host threads may call the device functions of one context at
 *     the same time, on their own streams or on a shared one (the null stream included).
 *     Per-stream device scratch has a lock that an entry point holds from its first write
 *     into the block to its last enqueue, so calls from several threads on ONE stream run
 *     in some order, each one whole.  hipStreamPerThread is a different stream in every
 *     thread: the context keeps its scratch block and captured-launch slots per (handle,
 *     calling thread), and vkv_release_stream / vkv_release_captured with that handle
 *     release the calling thread's.  vkv_last_error is ONE buffer per context: with
 *     several threads, rely on the return codes (the text may be another thread's).
 *     vkv_trim, vkv_forget_target and vkv_destroy must not run concurrently with launches
 *     (see there);
 *   - pointers named `d_*` are device pointers owned by the caller; POD structs are
 *     passed by const pointer and copied at call time;
 *   - volumes are dense uint8, x fastest: index = (z*height + y)*width + x
 *     (raw file order, src/volume_component.cpp:47-52); distance / occupancy maps the same;
 *   - ALIGNMENT: byte buffers may start at ANY byte - volumes, gradient maps, occupancy, distance and
 *     octant maps (each of the eight on its own), swap buffers, the 8-bit sources and the destinations
 *     of vkv_convert_volume / vkv_update_volume_region - so a caller may keep them all in one arena.
 *     RGBA8 render targets (d_out_rgba8) and the images and gathered tiles of vkv_scatter_tiles need
 *     the alignment of one pixel only (4 bytes, 16 for 16-byte pixels).  The launchers pick their
 *     vector variants from the pointers as well as from the extents; the results are the same bytes,
 *     and nothing before the first or past the last byte of a buffer is read or written
 *     (tests/test_gpu_pointer_alignment.py).  The exceptions are stated at the entry points:
 *     16-bit sources 2 bytes, d_transfer_function and d_tables of the transfer-function updates 4,
 *     counters, d_unresolved and d_histogram 8, d_summary 16, the packed image
 *     (vkv_pack_volume) 256;
 *   - matrices are column-major float[16] (glm::mat4 byte layout).
 */
#ifndef VKVOLUME_AMD_H
#define VKVOLUME_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VKV_OK 0
#define VKV_E_INVALID_ARGUMENT (-1) /* null pointer, zero extent, bad enum              */
#define VKV_E_UNSUPPORTED (-2)      /* e.g. map axis > 2048, volume too large for a launch */
#define VKV_E_NO_DEVICE (-3)        /* no HIP device / wrong architecture               */
#define VKV_E_IO (-4)               /* file errors of the loader                        */

#define VKV_TF_BITS_WORDS 2564      /* uint32 words of a vkv_transfer_function_tables() / _bits() buffer */

/* VkExtent3D stand-in (src/load_volume.h:31, src/volume_component.cpp:91-92). */
typedef struct VkvExtent3D
{
	uint32_t width, height, depth;
} VkvExtent3D;

/* TransferFunctionUniform, src/transfer_function.h:20-32 (32 bytes; the texture-path shaders read
 * the first 16, shaders/transfer_function.glsl:18-29). use_gradient is a VkBool32. */
typedef struct VkvTransferFunctionUniform
{
	float    sampling_factor;
	float    voxel_alpha_factor;
	float    grad_magnitude_modifier;
	uint32_t use_gradient;
	float    intensity_min;
	float    intensity_range_inv;
	float    gradient_min;
	float    gradient_range_inv;
} VkvTransferFunctionUniform;

/* Volume::Options, src/volume_component.h:45-56. */
typedef struct VkvVolumeOptions
{
	float    sampling_factor;          /* 1.0 */
	float    voxel_alpha_factor;       /* 1.0 */
	uint32_t use_precomputed_gradient; /* true */
	float    intensity_min;            /* 0.0 */
	float    intensity_max;            /* 1.0 */
	float    gradient_min;             /* 0.0 */
	float    gradient_max;             /* 1.0 */
} VkvVolumeOptions;

/* CameraUniform, src/volume_render_subpass.h:32-39 (320 bytes). */
typedef struct VkvCameraUniform
{
	float camera_view[16];
	float camera_proj[16];
	float camera_view_proj_inv[16];
	float model[16];
	float model_inv[16];
} VkvCameraUniform;

/* RayCastUniform, src/volume_render_subpass.h:46-53 (68 bytes). */
typedef struct VkvRayCastUniform
{
	float   plane[4];          /* clipping plane, global coordinates  */
	float   plane_tex[4];      /* clipping plane, texture coordinates */
	float   camera_pos_tex[4]; /* camera position, texture coordinates */
	float   block_size[4];     /* ceil(volume extent / map extent) per axis, as floats */
	int32_t front_index;
} VkvRayCastUniform;

/* Analytic pinhole ray generator.  It stands in for the rasteriser + the two vertex shaders
 * (shaders/volume_render_clipped.vert:50-65, shaders/volume_render_plane_intersection.vert:101-130):
 * the un-normalised texture-space direction of the ray through pixel (px, py) is
 *   dir = dir00 + (px + 0.5) * ddx + (py + 0.5) * ddy
 * which is exact for a pinhole camera.  vkv_build_uniforms() fills it from the matrices. */
typedef struct VkvRayGen
{
	float dir00[4];
	float ddx[4];
	float ddy[4];
} VkvRayGen;

/* VolumeRenderSubpass::SkippingType / Test / Options, src/volume_render_subpass.h:58-81. */
enum VkvSkippingType
{
	VKV_SKIP_NONE                 = 0,
	VKV_SKIP_BLOCK                = 1,
	VKV_SKIP_DISTANCE             = 2,
	VKV_SKIP_ANISOTROPIC_DISTANCE = 3
};

enum VkvTest
{
	VKV_TEST_NONE                = 0,
	VKV_TEST_RAY_ENTRY           = 1,
	VKV_TEST_RAY_EXIT            = 2,
	VKV_TEST_NUM_TEXTURE_SAMPLES = 3
};

typedef struct VkvRenderOptions
{
	int32_t skipping_type;         /* VKV_SKIP_DISTANCE */
	float   clip_distance;         /* 50.0 */
	int32_t early_ray_termination; /* true */
	int32_t depth_attachment;      /* false; true = DEPTH_ATTACHMENT variant: needs VkvRenderParams.d_in_depth */
	int32_t test;                  /* VKV_TEST_NONE */
} VkvRenderOptions;

/* A rectangle of screen tiles: x0, y0 = its first tile column / row, w x h tiles.  vkv_screen_tile_rect() derives the rectangle a frame's
 * fragments can lie in from the uniforms alone, so every rank of a multi-GPU frame arrives at the same one without talking. */
typedef struct VkvTileRect
{
	uint32_t x0, y0, w, h;
} VkvTileRect;

/* Screen tiling of one launch (single GPU: all tiles; multi GPU: every tile_stride-th tile).
 * The W×H image is cut into tiles of tile_width × tile_height pixels.  The SCHEDULED tiles are those of `rect` (rect.w == 0 or rect.h == 0:
 * every tile of the image), numbered row-major INSIDE the rectangle: tile t is column rect.x0 + t % rect.w, row rect.y0 + t / rect.w.
 * The launch renders tiles tile_first + k*tile_stride, k = 0 .. tile_count-1.  Pixels outside the rectangle are not touched by the launch
 * (vkv_scatter_tiles / vkv_assemble_frames clear them when they assemble a frame) unless fill_outside is set (single-GPU frames).
 * compact == 0: outputs are indexed by image pixel  (y*image_width + x);
 * compact != 0: outputs are indexed by (k*tile_height + ly)*tile_width + lx  (the per-rank
 *               buffer that is gathered over RCCL and de-interleaved by vkv_scatter_tiles); the
 *               slots of a partial tile's pixels beyond the image edge are never written.
 * The reference's rasteriser only shades fragments of the clipped box's faces (src/volume_render_subpass.cpp:262-293,
 * shaders/volume_render_clipped.vert:50-65): the rectangle is this build's counterpart - tiles no fragment can lie in are neither
 * scheduled nor exchanged. */
typedef struct VkvTileSchedule
{
	uint32_t    tile_width, tile_height; /* multiples of 16 (one 256-thread workgroup marches 16x16 pixels) */
	uint32_t    tile_first, tile_stride, tile_count;
	uint32_t    compact;
	VkvTileRect rect;                    /* all zero: the whole image */
	uint32_t    fill_outside;            /* single-GPU frames through a rectangle: != 0 = the launch ALSO writes the "no fragment" result (what a pixel whose ray
	                                        misses the box gets: clear values, or nothing with blend_over_target) to every pixel outside the rectangle, so the
	                                        frame is complete as with the whole-image schedule - without a workgroup per empty tile (each rendering workgroup
	                                        fills a share of the outside tiles).  Needs compact == 0 and the whole rectangle in this launch (tile_first 0,
	                                        tile_stride 1, tile_count rect.w * rect.h); the result equals the whole-image schedule's bit for bit. */
} VkvTileSchedule;

/* Everything VolumeRenderSubpass::draw binds for one volume
 * (src/volume_render_subpass.cpp:219-293) plus the output images. */
typedef struct VkvRenderParams
{
	VkvCameraUniform           camera;
	VkvRayCastUniform          ray_cast;
	VkvTransferFunctionUniform transfer_function;
	VkvRayGen                  ray_gen;
	VkvRenderOptions           options;
	uint32_t                   use_precomputed_gradient; /* PRECOMPUTED_GRADIENT variant */
	uint32_t                   image_width, image_height;
	VkvTileSchedule            tiles;
	VkvExtent3D                volume_extent;
	VkvExtent3D                map_extent;
	const uint8_t *            d_volume;                   /* R8_UNORM  W*H*D                */
	const uint8_t *            d_gradient;                 /* R8_UNORM  W*H*D, may be NULL when !use_precomputed_gradient */
	const uint8_t *            d_transfer_function;        /* RGBA8 256x256, row = gradient  */
	const uint8_t *            d_distance_maps[8];         /* [0] (or [0..7] anisotropic); unused for VKV_SKIP_NONE */
	const void *               d_packed_volume;            /* optional: vkv_pack_volume() image of d_volume (+ d_gradient); NULL = sample the linear buffers */
	const uint32_t *           d_transfer_function_bits;   /* optional: vkv_transfer_function_tables() of d_transfer_function; NULL = fetch the texel */
	float *                    d_out_color;                /* RGBA32F premultiplied, or NULL */
	uint8_t *                  d_out_rgba8;                /* RGBA8 round-to-nearest of the above, or NULL */
	uint32_t *                 d_out_counts;               /* 3 x u32 per pixel: volume samples, distance probes, empty samples; or NULL (the integrator then does not count) */
	float *                    d_out_depth;                /* gl_FragDepth (reverse-Z, 0 = far), or NULL */
	const float *              d_in_depth;                 /* options.depth_attachment: the scene depth the subpass reads as input attachment 0
	                                                          (frag:26, 122-165; reverse-Z), indexed like the outputs */
	uint32_t                   blend_over_target;          /* != 0: d_out_color / d_out_rgba8 hold the destination colour and the fragment is blended
	                                                          onto it with the subpass's blend state (volume_render_subpass.cpp:176-190):
	                                                          rgb = src + (1 - src.a) * dst, a = src.a * (1 - src.a); pixels without a fragment stay
	                                                          untouched.  0: every pixel of the schedule is overwritten (cleared to 0 first). */
} VkvRenderParams;

typedef struct vkv_ctx vkv_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* set-up call: allocates the context's device arena (VkvTuning.arena_bytes of the environment default, 8 MiB). */
int         vkv_create(int device_ordinal, vkv_ctx **out_ctx);
/* set-up call: waits for the device, then frees everything the context owns. */
void        vkv_destroy(vkv_ctx *ctx);
const char *vkv_last_error(const vkv_ctx *ctx);
const char *vkv_version(void);

/* Tuning switches of one context (A/B switches of the launchers; every setting renders the same bits).  vkv_create fills them from the
 * environment variables named below, ONCE; afterwards the environment is not consulted again: the behaviour of a linked library depends
 * on its context, not on the host's environment at first use.  vkv_set_tuning replaces the whole block (read it with vkv_get_tuning,
 * change fields, write it back); it applies to calls made after it returns. */
typedef struct VkvTuning
{
	uint32_t struct_size;              /* sizeof(VkvTuning): set by vkv_get_tuning, checked by vkv_set_tuning                       */
	int32_t  scheduler;                /* 0 lane = ray on static tiles (default); 1 persistent waves with lane re-fill   VKV_RAYMARCH_SCHEDULER=persistent */
	int32_t  batch_mode;               /* vkv_render_batch: 0 workgroup per tile (default); 1 resident workgroups pulling 8x8 units   VKV_RAYMARCH_BATCH=pull */
	int32_t  batch_sequential;         /* vkv_render_batch: 1 = frames one after the other instead of interleaved       VKV_RAYMARCH_BATCH_ORDER=sequential */
	int32_t  tile_order_linear;        /* 1 = tiles start in schedule order instead of centre-of-image first             VKV_RAYMARCH_TILE_ORDER=linear */
	int32_t  address_tables;           /* packed image: 0 none, 1 two-level LDS tables, 2 + one entry per voxel index (default)   VKV_RAYMARCH_LUT=0|2(two-level)|1 */
	uint32_t full_table_lds_limit;     /* LDS bytes per workgroup up to which the per-voxel tables are used (17920)       VKV_RAYMARCH_FULL_LIMIT */
	int32_t  screen_cull;              /* 1 = pixels outside the screen bound of the volume's box skip the ray set-up (default)   VKV_RAYMARCH_CULL=0 */
	int32_t  feedback;                 /* 1 = registered targets start their tiles in the order their last measured frame suggests (default)   VKV_RAYMARCH_FEEDBACK=0 */
	uint32_t feedback_period;          /* frames between two cost measurements of a target (8)                            VKV_RAYMARCH_FEEDBACK_PERIOD */
	int32_t  clamp_always;             /* 1 = the march loop never takes its clamp-free iterations (A/B switch, same bits)   VKV_RAYMARCH_CLAMP=always  */
	float    tile_mix_heavy;           /* experiment: central share of the tiles spread over the first tile_mix_spread of the order (0 = off)   VKV_RAYMARCH_TILE_MIX=h,s */
	float    tile_mix_spread;
	uint32_t gradient_segment;         /* vkv_gradient_map: tiles a workgroup marches in z; 0 = automatic                 VKV_GRADIENT_SEGMENT */
	int32_t  wave_shape;               /* width in pixels of a wave's 64-pixel patch: 0 automatic (4, 8 or 16 from the view: the shape that is most compact
	                                      in voxels), or 4 / 8 / 16 (A/B switch, same bits)                                 VKV_RAYMARCH_WAVE_SHAPE */
	uint32_t arena_bytes;              /* read-only: size of the device arena vkv_create allocated                        VKV_ARENA_BYTES */
} VkvTuning;
int vkv_get_tuning(const vkv_ctx *ctx, VkvTuning *out);
int vkv_set_tuning(vkv_ctx *ctx, const VkvTuning *tuning);

/* ---- host-side helpers (pure CPU, no device access) ------------------------------------------ */

/* Volume::get_transfer_function_uniform, src/volume_component.cpp:226-240. */
int vkv_transfer_function_uniform(const VkvVolumeOptions *options, VkvTransferFunctionUniform *out);

/* CPU half of Volume::update_transfer_function_texture, src/volume_component.cpp:242-261:
 * fills 256*256 RGBA8 texels (row = gradient, column = intensity). */
int vkv_transfer_function_texture(const VkvVolumeOptions *options, uint8_t *out_rgba8_256x256);

/* Uniform maths of VolumeRenderSubpass::draw, src/volume_render_subpass.cpp:221-249, plus the ray
 * generator.  view / proj (already vulkan-style, y flipped) / node_transform / image_transform are
 * column-major 4x4. */
int vkv_build_uniforms(const float *view, const float *proj, const float *node_transform, const float *image_transform,
                       float clip_distance, uint32_t image_width, uint32_t image_height,
                       VkvExtent3D volume_extent, VkvExtent3D map_extent,
                       VkvCameraUniform *out_camera, VkvRayCastUniform *out_ray_cast, VkvRayGen *out_ray_gen);

/* ---- device entry points ------------------------------------------------------------------- */

/* ComputeGradientMap::compute, src/compute_gradient_map.cpp:57-81 (shaders/gradient_map.comp). */
int vkv_gradient_map(vkv_ctx *ctx, const uint8_t *d_volume, uint8_t *d_gradient, VkvExtent3D extent,
                     const VkvTransferFunctionUniform *tf, void *stream);

/* ComputeDistanceMap::computeOccupancy, src/compute_distance_map.cpp:103-140
 * (shaders/occupancy_map.comp).  d_gradient == NULL selects the on-the-fly gradient variant. */
int vkv_occupancy_map(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient,
                      const uint8_t *d_transfer_function, const VkvTransferFunctionUniform *tf,
                      VkvExtent3D extent, uint8_t *d_map, VkvExtent3D map_extent, void *stream);

/* ComputeDistanceMap::computeDistance, src/compute_distance_map.cpp:142-175
 * (shaders/distance_map.comp): in-place on d_map (holding the occupancy map), d_swap is scratch. */
int vkv_distance_map(vkv_ctx *ctx, uint8_t *d_map, uint8_t *d_swap, VkvExtent3D map_extent, void *stream);

/* ComputeDistanceMap::computeDistanceAnisotropic, src/compute_distance_map.cpp:177-290
 * (shaders/distance_map_anisotropic.comp): occupancy in d_maps[7]; on return d_maps[k] is the map
 * for ray-direction octant k = (dz<0) + 2(dy<0) + 4(dx<0). */
int vkv_distance_map_anisotropic(vkv_ctx *ctx, uint8_t *const d_maps[8], uint8_t *d_swap,
                                 VkvExtent3D map_extent, void *stream);

/* ComputeDistanceMap::compute, src/compute_distance_map.cpp:65-101: occupancy into
 * d_maps[n-1] (n = 8 for anisotropic, else 1), then the transform selected by skipping_type.
 * Every argument is checked before anything is enqueued: a rejected call writes nothing. */
int vkv_compute_distance_map(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient,
                             const uint8_t *d_transfer_function, const VkvTransferFunctionUniform *tf,
                             VkvExtent3D extent, uint8_t *const d_maps[8], uint8_t *d_swap,
                             VkvExtent3D map_extent, int32_t skipping_type, void *stream);

/* ComputeOccupiedVoxelCount::compute + get_result, src/compute_occupied_voxel_count.cpp:88-156
 * (shaders/occupied_voxel_count.comp + occupied_voxel_count_reduce.comp): number of voxels whose ANALYTIC
 * transfer-function alpha (the uniform's min / range_inv fields, not the texture) is > 0, written to *d_count.
 * One pass: wave ballot + one 64-bit atomic per workgroup instead of the reference's multi-dispatch tree reduce. */
int vkv_occupied_voxel_count(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, const VkvTransferFunctionUniform *tf,
                             VkvExtent3D extent, uint64_t *d_count, void *stream);

/* LoadVolume::load_header / load_data, src/load_volume.cpp:33-86, :112-172 (host side). */
typedef struct VkvVolumeHeader
{
	VkvExtent3D extent;
	float       voxel_size[3];
	float       normalisation_range[2];
	char        type[16];
	char        endianness[16];
	float       image_transform[16];
} VkvVolumeHeader;
int vkv_load_header(const char *filename_header, VkvVolumeHeader *out);
int vkv_load_data(const char *filename_data, const VkvVolumeHeader *header, uint8_t *out_voxels, size_t out_bytes);

/* Device half of LoadVolume::load_data_impl (src/load_volume.cpp:151-169) for volumes whose raw file has been uploaded as
 * is: endianness conversion and normalisation to uint8, `(uint8) (255 * max(0, min(1, (v - min) / (max - min))))`, truncating.
 * d_raw holds n_voxels elements of `type`. */
enum VkvVoxelType
{
	VKV_VOXEL_UINT8  = 0,
	VKV_VOXEL_INT8   = 1,
	VKV_VOXEL_UINT16 = 2,
	VKV_VOXEL_INT16  = 3
};
int vkv_convert_volume(vkv_ctx *ctx, const void *d_raw, int32_t type, int32_t big_endian, float range_min, float range_max, uint64_t n_voxels,
                       uint8_t *d_out, void *stream);

/* Device-internal sampling layout of the volume (the counterpart of uploading into a VK_IMAGE_TILING_OPTIMAL image,
 * src/volume_component.cpp:68-83): 4x4x4-voxel bricks with a one-voxel apron, volume and gradient bytes interleaved,
 * clamp-to-edge baked in, bricks grouped 8x8x8.  Every trilinear footprint of both textures then lies inside one
 * 256-byte brick.  vkv_packed_volume_bytes() sizes the buffer; d_gradient may be NULL (gradient channel = 0).
 * Results of vkv_render are bit-identical with and without it. */
size_t vkv_packed_volume_bytes(VkvExtent3D extent);
int    vkv_pack_volume(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent, void *d_packed, void *stream);

/* Acceleration tables of the 256x256 TF texture for the integrator (device half of Volume::update_transfer_function_texture,
 * src/volume_component.cpp:262-278, next to the texture upload).  The buffer is VKV_TF_BITS_WORDS uint32:
 *   words [0, 2048)  1 bit per texel: alpha > 0 (row = gradient), so "voxel_occupied" (frag:276) comes from LDS and only occupied
 *                    samples fetch the RGBA texel;
 *   word 2048        flags; bit 0 = "separable greyscale": every texel equals (b, b, b, b) with
 *                    b = (uint8) clamp(alpha_i[column] * alpha_g[row] * 255, 0, 255) — the product the reference always builds
 *                    (src/volume_component.cpp:246-261).  alpha_i / alpha_g are derived from `tf` (intensity_min, *_range_inv,
 *                    use_gradient) and the claim is CHECKED on the device against all 65536 texels; when it holds the integrator
 *                    takes the texel from two 256-entry LDS tables (words 2052.., float) instead of a dependent global fetch.
 * tf == NULL (or vkv_transfer_function_bits) leaves the flag clear: any RGBA texture works through the generic path.
 * Rebuild the tables whenever the texture changes. */
int vkv_transfer_function_tables(vkv_ctx *ctx, const uint8_t *d_transfer_function, const VkvTransferFunctionUniform *tf,
                                 uint32_t *d_tables, void *stream);
int vkv_transfer_function_bits(vkv_ctx *ctx, const uint8_t *d_transfer_function, uint32_t *d_tables, void *stream);

/* CPU + device halves of Volume::update_transfer_function_texture (src/volume_component.cpp:242-278) on the device: the RGBA8 256x256
 * texture and the vkv_transfer_function_tables() buffer (separable flag set) from the options, in one launch - no host loop, no upload,
 * no wait.  Every texel equals what vkv_transfer_function_texture writes for the same options (a degenerate intensity window,
 * intensity_max == intensity_min, gives 0 where the host's product is NaN); every table word equals what vkv_transfer_function_tables
 * makes of that texture and vkv_transfer_function_uniform(options).  Both pointers 4-byte aligned. */
int vkv_transfer_function_texture_device(vkv_ctx *ctx, const VkvVolumeOptions *options, uint8_t *d_transfer_function, uint32_t *d_tables,
                                         void *stream);

/* VolumeRender::update_transfer_function, src/volume_render.cpp:392-445, as ONE enqueue on `stream`: (d_occupied_count != NULL) the
 * occupied-voxel count of vkv_occupied_voxel_count for the options' uniform (the reference's benchmark-mode submission, :400-416; it is
 * enqueued first because it stages its own bit table in the stream's scratch block), then the texture + tables of
 * vkv_transfer_function_texture_device, then the occupancy map and the transform of skipping_type into d_maps, as
 * vkv_compute_distance_map would build them from that texture (d_gradient == NULL: on-the-fly gradient, as there).  The occupancy pass
 * takes its bit table from the texture kernel instead of rebuilding it from the texture.  Every argument is checked before anything is
 * enqueued.  Capture: the call only enqueues kernels and memsets; the stream's scratch block comes out of the arena at its first use without
 * allocating, so after one direct call (or vkv_prepare_render) on `stream` the update can be captured into a hipGraph, with or without
 * the frames behind it.  A captured update replays with the options it was captured with: capture again when a slider moves. */
int vkv_update_transfer_function(vkv_ctx *ctx, const VkvVolumeOptions *options, const uint8_t *d_volume, const uint8_t *d_gradient,
                                 VkvExtent3D extent, uint8_t *d_transfer_function, uint32_t *d_tables, uint8_t *const d_maps[8],
                                 uint8_t *d_swap, VkvExtent3D map_extent, int32_t skipping_type, uint64_t *d_occupied_count, void *stream);

/* A box of voxels: [x0, x0 + width) x [y0, y0 + height) x [z0, z0 + depth). */
typedef struct VkvBox
{
	uint32_t x0, y0, z0, width, height, depth;
} VkvBox;

/* New voxels for a box of the volume, and every derived buffer rebuilt where the box reaches it - as ONE enqueue on `stream`:
 *   1. the width * height * depth raw elements of `type` at d_src (x fastest; a raw z-slab of a .header file is one) are converted as
 *      vkv_convert_volume converts them (endianness, normalisation to [range_min, range_max], truncating) into their place in d_volume;
 *   2. (d_gradient != NULL) the gradient of the box grown by one voxel per side, clamped to the volume (a voxel's gradient reads its +-1
 *      neighbours);
 *   3. (d_packed != NULL) every brick of the vkv_pack_volume image whose 5^3 texels read a changed volume or gradient byte (the clamped
 *      apron bricks on the volume's faces included), from d_volume and d_gradient (NULL: gradient channel 0, as there);
 *   4. (d_maps != NULL) the occupancy cells that meet the grown box, OCCUPIED or EMPTY, into the map that holds the occupancy, with the bit
 *      table of d_transfer_function staged in the stream's scratch block (d_gradient == NULL: the on-the-fly gradient, as in
 *      vkv_compute_distance_map).  `skipping_type` names what d_maps hold: NONE / BLOCK raw occupancy in d_maps[0], DISTANCE the Chebyshev
 *      map in d_maps[0], ANISOTROPIC the eight octant maps; a distance is 0 exactly where the cell is occupied, so the map holding the
 *      occupancy input (d_maps[0], d_maps[7] for ANISOTROPIC) is first turned back into occupancy;
 *   5. the whole-map transform of skipping_type, as vkv_compute_distance_map runs it.
 * PRECONDITION: before the call d_gradient, d_packed and d_maps hold what vkv_gradient_map, vkv_pack_volume and vkv_compute_distance_map
 * (with this tf, d_transfer_function, extent, map_extent and skipping_type) make of d_volume.  Then after the call they hold, byte for byte,
 * what those entry points make of the updated volume.
 * The box must lie inside `extent` and not be empty; 16-bit sources must be 2-byte aligned; d_packed 256-byte aligned; with d_maps the
 * maps the skipping type uses and d_transfer_function must be non-NULL, and DISTANCE / ANISOTROPIC need a d_swap that aliases no map.
 * Every argument is checked before anything is enqueued: a rejected call writes nothing.  Capture: the call enqueues kernels only (no
 * memset or copy nodes, no allocation, no host wait), so after one direct call (or vkv_prepare_render) on `stream` the update can be
 * captured into a hipGraph; it replays with the source pointer and box it was captured with. */
int vkv_update_volume_region(vkv_ctx *ctx, const void *d_src, int32_t type, int32_t big_endian, float range_min, float range_max, const VkvBox *box,
                             uint8_t *d_volume, uint8_t *d_gradient, void *d_packed, VkvExtent3D extent, const uint8_t *d_transfer_function,
                             const VkvTransferFunctionUniform *tf, uint8_t *const d_maps[8], uint8_t *d_swap, VkvExtent3D map_extent,
                             int32_t skipping_type, void *stream);

/* Joint histogram of (gradient byte, intensity byte): 65536 uint64 bins, bin g * 256 + i = the voxels with gradient byte g and intensity
 * byte i (row = gradient, as in the transfer-function texture).  One bin of a 2048^3 volume can exceed 2^32. */
#define VKV_HISTOGRAM_BINS 65536

enum VkvHistogramMode
{
	VKV_HISTOGRAM_SET      = 0, /* overwrite every bin with the box's counts          */
	VKV_HISTOGRAM_ADD      = 1, /* add the box's counts to the bins                   */
	VKV_HISTOGRAM_SUBTRACT = 2, /* subtract them, modulo 2^64 (ADD undoes it exactly) */
};

/* The histogram of the voxels of `box` (NULL: the whole volume) into d_histogram (VKV_HISTOGRAM_BINS uint64, 8-byte aligned), as `mode`
 * says.  d_gradient == NULL counts every voxel in gradient row 0: the intensity histogram of a volume without a precomputed gradient.
 * Every argument is checked before anything is enqueued: a null volume or histogram, a zero extent, an empty box or one not inside
 * `extent`, an unknown mode or a misaligned d_histogram return VKV_E_INVALID_ARGUMENT and write nothing.  The call only enqueues kernels
 * (SET clears the bins with a kernel, not a memset node), allocates nothing and does not wait, so after one direct call on `stream` it
 * can be captured into a hipGraph.
 * Keeping a histogram current across vkv_update_volume_region: before the update, SUBTRACT over the update's box grown by one voxel per
 * side and clamped to the volume (the gradient changes there); after it, ADD over the same grown box, on the same stream.  A cell summary
 * (vkv_cell_summary below) is kept current the same way: rebuild it over that grown box after the update. */
int vkv_volume_histogram(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent, const VkvBox *box, int32_t mode,
                         uint64_t *d_histogram, void *stream);

/* The sum of the bins of d_histogram whose ANALYTIC transfer-function alpha is > 0 (vkv_occupied_voxel_count's rule: bit row g when
 * tf->use_gradient is set, else 255), STORED to *d_count (8-byte aligned).  Equals vkv_occupied_voxel_count of the same volume and tf when
 * the histogram was built with the gradient map, or when tf->use_gradient is 0.  Limit: with use_gradient set and no gradient map,
 * vkv_occupied_voxel_count evaluates an on-the-fly float gradient, which the histogram does not hold.  One small launch; kernels only. */
int vkv_histogram_occupied_count(vkv_ctx *ctx, const uint64_t *d_histogram, const VkvTransferFunctionUniform *tf, uint64_t *d_count,
                                 void *stream);

/* Per-cell summaries: a transfer-function change decides most occupancy cells without reading a voxel (DESIGN.md §5 "Cell summaries").
 * Each cell of the occupancy map (block = ceil(extent / map_extent) per axis, voxels clipped to the volume) has 16 bytes, in map order (x fastest):
 *   bytes 0, 1   i_lo, i_hi: min / max intensity byte of the cell's voxels
 *   bytes 2, 3   g_lo, g_hi: min / max gradient byte (a summary built without a gradient map records 255 for every voxel)
 *   byte 4       g_at_i_hi: the largest gradient byte among the voxels whose intensity is i_hi
 *   byte 5       i_at_g_hi: the largest intensity byte among the voxels whose gradient is g_hi
 *   byte 6       flags: bit 0 = the cell holds at least one voxel (cells past the volume are all zero)
 *   byte 7       0
 *   bytes 8..15  mask (uint64, little-endian): bit (g >> 5) * 8 + (i >> 5) is set if some voxel has gradient byte g and intensity byte i.
 * Every field is a min, a max or an OR: a rebuild is byte-comparable. */
#define VKV_CELL_SUMMARY_BYTES 16

/* The summaries of every cell (box == NULL), or of every cell that meets `box`, into d_summary (16-byte aligned, map_extent cells x
 * VKV_CELL_SUMMARY_BYTES); a cell is rebuilt whole, from all of its voxels.  d_gradient == NULL records gradient byte 255 for every voxel.
 * Every argument is checked before anything is enqueued: a rejected call writes nothing.  Kernels only: no memset, no allocation, no
 * host wait, so after one direct call on `stream` it can be captured into a hipGraph.
 * Keeping a summary current across vkv_update_volume_region: after the update, call vkv_cell_summary over the update's box grown by one voxel
 * per side and clamped to the volume (the gradient changes there), on the same stream. */
int vkv_cell_summary(vkv_ctx *ctx, const uint8_t *d_volume, const uint8_t *d_gradient, VkvExtent3D extent, VkvExtent3D map_extent, const VkvBox *box,
                     void *d_summary, void *stream);

/* The occupancy map of vkv_occupancy_map with the same arguments, byte for byte, decided per cell from d_summary where the rule is certain
 * and from the cell's voxels where it is not.  d_unresolved (optional, 8-byte aligned) receives the number of cells evaluated from their
 * voxels, stored rather than accumulated.
 * PRECONDITION: d_summary was built by vkv_cell_summary from the current d_volume and d_gradient, with the same extent and map_extent and the
 * same NULL-ness of d_gradient.  A summary built with a gradient map serves both tf->use_gradient values.  tf->use_gradient with
 * d_gradient == NULL (the on-the-fly float gradient, which no summary byte can hold) returns VKV_E_UNSUPPORTED.
 * The call stages the bit table and a 64 KiB table of row-range ORs / ANDs in the stream's scratch block; checks, capture and "writes
 * nothing when rejected" as vkv_cell_summary. */
int vkv_occupancy_map_from_summary(vkv_ctx *ctx, const void *d_summary, const uint8_t *d_volume, const uint8_t *d_gradient,
                                   const uint8_t *d_transfer_function, const VkvTransferFunctionUniform *tf, VkvExtent3D extent, uint8_t *d_map,
                                   VkvExtent3D map_extent, uint64_t *d_unresolved, void *stream);

/* vkv_update_transfer_function with the occupancy map from d_summary (as vkv_occupancy_map_from_summary, same precondition and limits) and,
 * when d_occupied_count is given, the count from d_histogram (vkv_histogram_occupied_count; d_histogram is then required, and must have been
 * built with the gradient map whenever d_gradient is given): a counted slider move reads no voxel of a resolved cell.  Texture, tables, maps and
 * count equal those of vkv_update_transfer_function byte for byte.  d_unresolved as in vkv_occupancy_map_from_summary.  Every argument is
 * checked before anything is enqueued; kernels only, so after one direct call on `stream` it can be captured into a hipGraph. */
int vkv_update_transfer_function_from_summary(vkv_ctx *ctx, const VkvVolumeOptions *options, const uint8_t *d_volume, const uint8_t *d_gradient,
                                              VkvExtent3D extent, uint8_t *d_transfer_function, uint32_t *d_tables, uint8_t *const d_maps[8],
                                              uint8_t *d_swap, VkvExtent3D map_extent, int32_t skipping_type, uint64_t *d_occupied_count,
                                              const void *d_summary, const uint64_t *d_histogram, uint64_t *d_unresolved, void *stream);

/* VolumeRenderSubpass::prepare, src/volume_render_subpass.cpp:95-157 (where the reference builds its pipelines and descriptor layouts).
 * Set-up call: creates, for `count` parameter blocks as a later vkv_render / vkv_render_batch on `stream` will pass them, everything that
 * launch takes from the context: the stream's scratch block, the address tables of the packed image's extent, the tile start order of the
 * schedule - and from the HIP runtime: the code objects of the kernels those blocks select are loaded onto the device now (the runtime
 * loads a code object at the first use of one of its kernels, which allocates device memory and takes milliseconds); uploads are
 * waited for before it returns.  A launch that finds one of them missing still creates it on the fly out of the
 * arena with an asynchronous upload on its own stream (no device-wide wait; if the arena is exhausted the launch runs without the table:
 * plain tile order / address arithmetic in registers, same bits) - vkv_prepare_render only moves that work to set-up time.  Call it
 * before capturing `stream` into a hipGraph: a launch that still has to create a table records and queries an event, which a capture
 * does not allow.  Captured launches replay with the parameter blocks they were captured with (camera included: capture one graph per
 * view, or re-capture).  A captured vkv_render_batch owns a slot of the context - a pinned host block (the graph's copy node reads its
 * source at every replay) and a device block of its own (the copy's target and the kernels' argument pointer) - so graphs may be replayed on
 * any stream, next to each other and next to live launches.  32 slots are set aside by vkv_create (nothing is allocated during such a
 * capture), later ones are allocated during the capture (2 x 96 KiB, with the thread's capture mode relaxed for the calls).  A slot stays
 * with the stream it was captured on until vkv_release_captured(stream); vkv_trim and vkv_destroy free the slots and the tables the
 * captured launches point to: graphs captured before either call must not be launched after it. */
int vkv_prepare_render(vkv_ctx *ctx, const VkvRenderParams *params, uint32_t count, void *stream);

/* The graphs captured on `stream` so far have been destroyed (or will not be launched again): the slots their vkv_render_batch launches
 * own return to the context.  A renderer that re-captures when its camera moves calls this after hipGraphExecDestroy and before the next
 * capture; without it every capture takes new slots until vkv_trim.  Does not wait and frees nothing. */
int vkv_release_captured(vkv_ctx *ctx, void *stream);

/* Start-order feedback needs device state per render target (one uint32 cost and one uint32 order entry per tile of the
 * schedule): a renderer draws into the same swap-chain images again and again with a camera that moves little, so the tiles that took longest in the
 * last measured frame are started first in the next ones (any order renders the same bits).
 * vkv_register_target - set-up call: allocates and initialises that state for frames of image_width x image_height pixels rendered with
 *   tile schedule `tiles` into `d_target` (the d_out_rgba8 or, without one, d_out_color pointer of the parameter block).  Targets that
 *   were never registered are rendered in the centre-first order: vkv_render never allocates.  Registering a target again replaces
 *   its state (waits for the device first, like vkv_forget_target).
 * vkv_forget_target - set-up call: waits for the device (launches that still use the state), then frees it.  Like freeing the target
 *   itself, it must not run concurrently with a render into that target from another thread. */
int vkv_register_target(vkv_ctx *ctx, const void *d_target, uint32_t image_width, uint32_t image_height, const VkvTileSchedule *tiles);
int vkv_forget_target(vkv_ctx *ctx, const void *d_target);

/* Set-up call: waits for the device, then drops every cached table (tile start orders, address tables) and empties the arena's table
 * region; the next launches create what they need again (asynchronously, as on first use).  For a renderer whose window or volume sizes
 * keep changing: call it at a quiet point (a resize, a scene change) - like vkv_forget_target it must not run concurrently with a launch
 * from another thread.  Stream scratch blocks and registered targets are not touched.  Also returns the pinned argument blocks of launches
 * captured into hipGraphs (vkv_prepare_render): a graph captured before the call points to tables and blocks that are gone - re-capture. */
int vkv_trim(vkv_ctx *ctx);

/* Gives the 128 KiB scratch block vkv_render_batch / vkv_compute_distance_map / ... keep per HIP stream back to the context's pool.
 * Call it before destroying a stream that was handed to this context, when all work enqueued on it has completed (it does not wait).
 * For hipStreamPerThread it gives back the calling thread's block: call it from each thread that used the handle, before the thread ends. */
int vkv_release_stream(vkv_ctx *ctx, void *stream);

/* VolumeRenderSubpass::draw, src/volume_render_subpass.cpp:159-294 (shaders/volume_render.frag). */
int vkv_render(vkv_ctx *ctx, const VkvRenderParams *params, void *stream);

/* Several frames in ONE launch: `count` (1 .. VKV_MAX_BATCH) parameter blocks that share the kernel variant (skipping type, ERT,
 * gradient mode, test mode), have a packed sampling image and the same tile SIZE (the tile counts and rectangles of the schedules may
 * differ: the frames of a multi-GPU launch each have their own screen rectangle); cameras, volumes and output buffers may differ (stereo pairs, orbit sweeps, the per-rank tile sets of a multi-GPU frame, the reference's frames in flight).  The
 * frames advance side by side inside one grid, so the long tail of each is covered by the bulk of the others without relying on
 * several hardware queues.  Output buffers of different frames must not overlap.  Results are bit-identical to `count` vkv_render calls. */
#define VKV_MAX_BATCH 32
int vkv_render_batch(vkv_ctx *ctx, const VkvRenderParams *params, uint32_t count, void *stream);

/* The tile rectangle the fragments of a frame can lie in (pure CPU, double precision from the float uniforms: the same inputs give the
 * same rectangle on every rank).  The volume's box [0,1]^3 (texture space) is cut by the clipping plane (plane_tex: the kept side is
 * dot(plane_tex.xyz, p) + plane_tex.w >= 0, the side the integrator starts its rays on, frag:117 / volume_render_clipped.vert:56), the
 * vertices of the clipped box are solved through the ray generator (p - camera_pos_tex = g (dir00 + fx ddx + fy ddy)), and the pixel
 * bound of the (fx, fy), widened by two pixels, is rounded outwards to whole tiles and then to multiples of `align_tiles` tiles
 * (0 or 1: no alignment; a renderer whose camera moves aligns to e.g. 4 tiles so that the rectangle - and with it the feedback state of a
 * registered target - changes less often; a schedule over a whole rectangle computes its start order in the kernel, no table is cached per rectangle).  A pixel outside the rectangle cannot have a fragment, whatever
 * the depth test does afterwards.  The rectangle is never empty: a box that is off screen gives the 1 x 1 rectangle of tile (0, 0)
 * (a fixed, minimal exchange); a vertex at or behind the camera plane, or a degenerate generator, gives the whole image. */
int vkv_screen_tile_rect(const VkvRayCastUniform *ray_cast, const VkvRayGen *ray_gen, uint32_t image_width, uint32_t image_height,
                         uint32_t tile_width, uint32_t tile_height, uint32_t align_tiles, VkvTileRect *out_rect);

/* Root-rank de-interleave of gathered compact tile buffers into the W×H image (multi-GPU): the tiles of `rect` (NULL or w == 0: every
 * tile of the image; numbered row-major inside it as in VkvTileSchedule) were dealt round-robin to n_ranks ranks, tile t to rank
 * t % n_ranks as its (t / n_ranks)-th.  d_gathered holds the n_ranks compact buffers, `rank_stride_tiles` tiles apart (>= the
 * ceil(tiles / n_ranks) tiles a rank holds: when the frames of a launch travel as one block per rank the stride is the block's tile
 * count and the caller offsets d_gathered to the frame), bytes_per_pixel per pixel.  Pixels outside the rectangle are CLEARED to zero:
 * the image is complete after the call. */
int vkv_scatter_tiles(vkv_ctx *ctx, const void *d_gathered, void *d_image, uint32_t image_width,
                      uint32_t image_height, uint32_t tile_width, uint32_t tile_height, const VkvTileRect *rect,
                      uint32_t n_ranks, uint32_t rank_stride_tiles, uint32_t bytes_per_pixel, void *stream);

/* ---- multi-GPU exchange step --------------------------------------------------------------------------------
 * Rays are independent: a frame is cut into screen tiles dealt round-robin to the ranks (VkvTileSchedule: tile_first = rank,
 * tile_stride = n_ranks, compact = 1, rect = vkv_screen_tile_rect of the frame's uniforms), the volume is replicated, and the ONLY
 * exchange is the gather of every rank's compact tile buffer to the frame's owner, followed by vkv_scatter_tiles there.  One process (or
 * host thread) per GPU, one ncclComm_t each.
 *
 * vkv_gather_tiles enqueues that gather on `stream` with RCCL's ncclGather (rccl.h:745; 7 concurrent point-to-point transfers into
 * the root over xGMI): every rank sends bytes_per_rank bytes from d_tiles, the root receives n_ranks * bytes_per_rank bytes into
 * d_gathered (ignored elsewhere).  `nccl_comm` is the caller's ncclComm_t.  The RCCL library is resolved at run time: the copy
 * already loaded into the process if there is one (so the communicator and the call come from the same library), else librccl.so.1;
 * VKV_RCCL_LIBRARY=<path> overrides.  Returns VKV_E_UNSUPPORTED when no RCCL can be loaded, 1000 + ncclResult_t on RCCL errors. */
int vkv_gather_tiles(vkv_ctx *ctx, const void *d_tiles, void *d_gathered, size_t bytes_per_rank, int32_t root, void *nccl_comm, void *stream);

/* The whole exchange of one frame on `stream`: vkv_gather_tiles of this rank's ceil(tiles of rect / n_ranks) compact tiles to `root`, then
 * (on the root only) vkv_scatter_tiles of the gathered buffers into d_image.  d_gathered is scratch of n_ranks * ceil(tiles / n_ranks) *
 * tile_width * tile_height * bytes_per_pixel bytes on the root; d_image / d_gathered may be NULL on the other ranks. */
int vkv_assemble_frame(vkv_ctx *ctx, const void *d_tiles, void *d_gathered, void *d_image, uint32_t image_width, uint32_t image_height,
                       uint32_t tile_width, uint32_t tile_height, const VkvTileRect *rect, uint32_t n_ranks, uint32_t rank,
                       uint32_t bytes_per_pixel, int32_t root, void *nccl_comm, void *stream);

/* The exchange of a whole vkv_render_batch launch (what a C or C++ renderer binds for frames in flight).  Frame f has its own tile
 * rectangle rects[f] (NULL: every frame the whole image) and its own owner roots[f] (NULL: every frame `root`): with the owners of a
 * launch's frames spread over the ranks every GPU receives at once, over all of its inbound xGMI links, instead of one GPU receiving
 * everything.  tpr(f) = ceil(tiles of rects[f] / n_ranks) is what a rank renders of frame f (its VkvTileSchedule.tile_count, except on
 * the last ranks of a ragged deal, whose missing tile's slot travels unused).
 *   d_tiles     this rank's compact tiles of the launch, frames back to back: [frame f][tpr(f) tiles];
 *   d_gathered  scratch of n_ranks * sum_f tpr(f) tiles on every rank that owns a frame (its layout is the call's own business: [rank][frame]
 *               [tiles] after the one gather, [frame][rank][tiles] after the group);
 *   d_images    host array of `frames` device pointers (copied at call time); entry f is only read on the owner of frame f.
 * roots == NULL: ONE ncclGather of the launch's whole block to `root`.  roots != NULL: one ncclGather per frame, all inside ONE group
 * (ncclGroupStart / ncclGroupEnd: RCCL fuses the group's point-to-point transfers into one kernel).  Then, on every rank that owns a frame,
 * ONE de-interleave kernel for the frames it owns (pixels outside a frame's rectangle are cleared).
 * Every rank must pass the same frames, rects, roots. */
int vkv_assemble_frames(vkv_ctx *ctx, const void *d_tiles, void *d_gathered, void *const *d_images, uint32_t frames, uint32_t image_width,
                        uint32_t image_height, uint32_t tile_width, uint32_t tile_height, const VkvTileRect *rects, uint32_t n_ranks, uint32_t rank,
                        uint32_t bytes_per_pixel, int32_t root, const int32_t *roots, void *nccl_comm, void *stream);

/* ---- maximum-intensity projection ------------------------------------------------------------------------------
 * The per-cell max map: one byte per cell of map_extent (block = ceil(extent / map_extent) per axis, as for the occupancy map), in map order
 * (x fastest).  Each byte is the largest voxel of the cell's voxel box grown by ONE voxel on every side, clipped to the volume: every voxel that
 * a trilinear sample within half a voxel of the cell can read.  Cells past the volume hold 0.  box == NULL rebuilds every cell; a box rebuilds
 * every cell whose grown box meets it, so after vkv_update_volume_region(box) a vkv_max_map(box) on the same stream leaves the map byte-equal to
 * a full rebuild.  Every argument is checked before anything is enqueued: a rejected call writes nothing.  Kernels only: no memset, no
 * allocation, no host wait, so after one direct call on `stream` it can be captured into a hipGraph.  Voxel rows are read at any width and
 * alignment, never past the last row. */
int vkv_max_map(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, VkvExtent3D map_extent, const VkvBox *box, uint8_t *d_max_map,
                void *stream);

typedef struct VkvMipOptions
{
	float          threshold;       /* a sample counts if its filtered intensity is > threshold (finite; 1.0 or more: nothing counts)      */
	float          window_max;      /* grey level g = clamp((m - threshold) / (window_max - threshold), 0, 1); window_max <= threshold: g = 1 */
	const uint8_t *d_max_map;       /* vkv_max_map of d_volume with params->map_extent, or NULL (dense: every sample is filtered)          */
	float *        d_out_intensity; /* m per pixel (0 without a counted sample), indexed like the other outputs; or NULL                   */
	uint32_t       flags;           /* must be 0 */
} VkvMipOptions;

/* Maximum-intensity projection of one volume.  The rays and samples are vkv_render's with VKV_SKIP_NONE (ray generator, box, clipping plane,
 * options.depth_attachment with d_in_depth, transfer_function.sampling_factor, sample i at fma(i, step, entry)); a sample's value v_i is the
 * integrator's filtered intensity (linear buffer or d_packed_volume: the same bits).  v_i counts if v_i > threshold; m = the largest counted
 * v_i, k = the first index where v_i == m.  A pixel with a fragment and a counted sample gets d_out_intensity = m, RGBA32F (g, g, g, 1), RGBA8
 * its round-to-nearest, d_out_depth the reverse-Z depth of sample k (the integrator's first-hit formula).  Every other pixel gets what the
 * integrator gives a pixel without colour: clear colour, intensity 0, depth 0 (the scene depth under depth_attachment).  d_out_counts (3 x u32
 * per pixel): samples filtered, max-map bytes read, samples skipped; [0] + [2] is the ray's sample count on every path.
 * With d_max_map a ray jumps over the samples of a cell whose byte cannot beat max(threshold, its best so far), and stops once its best is
 * 255 / 255: the results equal the dense path's bit for bit (the argument is in DESIGN.md §5.9).
 * Read: camera, ray_cast, ray_gen, options.clip_distance (through the uniforms), options.depth_attachment / d_in_depth, sampling_factor,
 * volume_extent, map_extent (with a max map), d_volume, d_packed_volume, the outputs and `tiles` (whole image, rect, compact, strided: a
 * compact per-rank share assembles through vkv_scatter_tiles / vkv_assemble_frame as a render share does).  Ignored: skipping_type, distance
 * maps, transfer-function texture and tables, gradient, early_ray_termination.  VKV_E_UNSUPPORTED: blend_over_target, tiles.fill_outside,
 * options.test != VKV_TEST_NONE.  VKV_E_INVALID_ARGUMENT: a non-finite threshold or NaN window_max, a max map without a valid map_extent,
 * flags != 0, and what vkv_render rejects of the fields read.  Every argument is checked before anything is enqueued: a rejected call writes
 * nothing.  The call enqueues one kernel and nothing else (no scratch block, no table, no allocation, no host wait; the kernels use no
 * scratch memory), so after one direct call on `stream` it can be captured into a hipGraph; it replays with the parameters it was captured with. */
int vkv_render_mip(vkv_ctx *ctx, const VkvRenderParams *params, const VkvMipOptions *mip, void *stream);

/* ---- isosurface ------------------------------------------------------------------------------------------------- */
typedef struct VkvIsoOptions
{
	float          iso;             /* a sample hits if its filtered intensity v >= iso (finite; > 1: nothing hits; <= 0: the first sample hits) */
	uint32_t       refine_steps;    /* 0 .. 16 bisection steps between samples k - 1 and k                                                        */
	float          base_color[3];   /* surface colour, each finite and >= 0                                                                       */
	float          ambient, diffuse, specular; /* finite, >= 0                                                                                    */
	uint32_t       shininess;       /* 1 .. 1024, integer exponent of the specular term                                                           */
	const uint8_t *d_max_map;       /* vkv_max_map of d_volume with params->map_extent, or NULL (dense: every sample up to the hit is filtered)     */
	float *        d_out_normal;    /* 4 floats per pixel, indexed like the other outputs: world-space unit normal facing the camera, w = 1;      */
	                                /* zeros without a hit; or NULL                                                                                */
	uint32_t       flags;           /* must be 0 */
} VkvIsoOptions;

/* Shaded isosurface of one volume.  Rays, samples, clipping plane, options.depth_attachment with d_in_depth, sampling_factor and the filter
 * (linear buffer or d_packed_volume: the same bits) are vkv_render_mip's; e = the ray's entry, s = its step (texture space).  k = the first
 * sample index with v_k >= iso.  The hit parameter t is 0 for k == 0, else refine_steps bisection steps from lo = k - 1, hi = k (mid =
 * (lo + hi) * 0.5, filtered at fma(mid, s, e): hi = mid if v >= iso, else lo = mid; t = hi), the hit point p = fma(t, s, e).  A pixel with a hit
 * gets: d_out_depth the reverse-Z depth of p (the integrator's first-hit formula); the normal n from the integrator's tetrahedron gradient at p
 * (g_tex = (gx W, gy H, gz D), n = transpose(model_inv[3x3]) g_tex normalised, turned to face the view vector v = -(model[3x3] s) normalised;
 * v itself where that has no length); a headlight: d = clamp(n . v, 0, 1), L = (ambient + diffuse d) + specular d^shininess, RGBA32F
 * (clamp(base_color L, 0, 1), 1) and its RGBA8 round-to-nearest; d_out_normal (n, 1).  Every other pixel gets what the integrator gives a pixel
 * without colour: clear colour, depth 0 (the scene depth under depth_attachment), normal zeros.  Every step is IEEE arithmetic in an order
 * DESIGN.md §5.10 fixes, so every output is specified to the bit.  d_out_counts (3 x u32 per pixel): samples filtered, max-map bytes read,
 * samples skipped; [0] + [2] is k + 1 on a hit and the ray's sample count without one (refinement and gradient taps are not counted).
 * With d_max_map a ray jumps over the samples of a cell whose byte B gives B * kInv255 < iso and stops at its first hit: the results equal
 * the dense path's bit for bit.  VKV_E_UNSUPPORTED: blend_over_target, tiles.fill_outside, options.test != VKV_TEST_NONE.
 * VKV_E_INVALID_ARGUMENT: a non-finite iso, refine_steps > 16, a negative or non-finite colour or coefficient, shininess outside 1 .. 1024,
 * flags != 0, a max map without a valid map_extent, and what vkv_render_mip rejects of the fields read.  Every argument is checked before
 * anything is enqueued: a rejected call writes nothing.  One kernel launch and nothing else (no scratch, no table, no allocation, no host
 * wait), so after one direct call on `stream` it can be captured into a hipGraph.  Schedules as vkv_render_mip: whole image, rect, compact
 * strided shares that assemble through vkv_scatter_tiles. */
int vkv_render_isosurface(vkv_ctx *ctx, const VkvRenderParams *params, const VkvIsoOptions *iso, void *stream);

/* ---- oblique slices and thick slabs: multi-planar reformatting ------------------------------------------------------- */
enum VkvSlabMode { VKV_SLAB_MAX = 0, VKV_SLAB_MIN = 1, VKV_SLAB_MEAN = 2 };

typedef struct VkvSlabOptions
{
	float          origin[3];   /* texture coordinates ([0,1]^3 = the volume) of pixel (0, 0), sample 0 */
	float          du[3];       /* texture-space step per pixel column */
	float          dv[3];       /* texture-space step per pixel row    */
	float          dn[3];       /* texture-space step per slab sample  */
	uint32_t       samples;     /* 1 .. 4096 samples per pixel; 1 = a plain slice */
	int32_t        mode;        /* VkvSlabMode */
	float          window_min, window_max; /* grey g = clamp((value - window_min) / (window_max - window_min), 0, 1); window_max <= window_min: g = 1 */
	const uint8_t *d_max_map;   /* vkv_max_map of d_volume with params->map_extent, or NULL (dense); VKV_SLAB_MAX only */
	float *        d_out_value; /* the slab's value per pixel (0 without a counted sample), indexed like the other outputs; or NULL */
	uint32_t       flags;       /* must be 0 */
} VkvSlabOptions;

/* A plane through one volume, or a slab of finite thickness about it, without a camera.  Every step is fp32 IEEE arithmetic in this order:
 * pixel (x, y) has the base point p_c = fma((float) y, dv_c, fma((float) x, du_c, origin_c)) per component c, its samples lie at
 * q_c = fma((float) j, dn_c, p_c), j = 0 .. samples - 1, and sample j counts if 0 <= q_c <= 1 on all three axes (fma is monotone in j: the
 * counted indices are one contiguous range).  A sample's value v_j is the integrator's filtered intensity at q (linear buffer or
 * d_packed_volume: the same bits).  VKV_SLAB_MAX: the largest counted v_j; VKV_SLAB_MIN: the smallest; VKV_SLAB_MEAN: acc = 0, acc = acc + v_j
 * over the counted j in rising order, acc / (float) count.  A pixel with a counted sample gets d_out_value = that value, RGBA32F (g, g, g, 1)
 * and RGBA8 its round-to-nearest; every other pixel gets value 0 and colour zeros.  d_out_counts (3 x u32 per pixel): samples filtered,
 * max-map bytes read, samples skipped; [0] + [2] is the number of counted samples on every path, and [1] = [2] = 0 without a max map.
 * With d_max_map (VKV_SLAB_MAX only) a pixel's column walks like a MIP ray with entry p and step dn over the counted range: the samples of a
 * cell whose byte B gives B * kInv255 <= the best so far are jumped over (there is no best before the first filtered sample, so the first
 * counted sample is always filtered), and the walk stops once the best is 255 / 255: the results equal the dense path's bit for bit.
 * Read: image_width, image_height, `tiles` (whole image, rect, compact, strided: a compact per-rank share assembles through
 * vkv_scatter_tiles / vkv_assemble_frame as a MIP share does), volume_extent, map_extent (with a max map), d_volume, d_packed_volume,
 * d_out_color, d_out_rgba8, d_out_counts.  Ignored: camera, ray_cast, ray_gen, transfer function, gradient, distance maps, skipping_type (a
 * zero-filled camera is fine).  VKV_E_UNSUPPORTED: blend_over_target, tiles.fill_outside, options.test != VKV_TEST_NONE,
 * options.depth_attachment, a non-NULL d_out_depth.  VKV_E_INVALID_ARGUMENT: null params or slab, flags != 0, samples outside 1 .. 4096, an
 * unknown mode, a non-finite component of origin, du, dv or dn, a NaN window_min or window_max, d_max_map with a mode other than VKV_SLAB_MAX
 * or without a valid map_extent, no output at all, a null d_volume, a zero extent, and what vkv_render_mip rejects of `tiles`.  Every argument
 * is checked before anything is enqueued: a rejected call writes nothing.  One kernel launch and nothing else (no memset, no table, no
 * allocation, no host wait; the kernels use no scratch memory), so after one direct call on `stream` it can be captured into a hipGraph. */
int vkv_render_slab(vkv_ctx *ctx, const VkvRenderParams *params, const VkvSlabOptions *slab, void *stream);

/* ---- 3x3x3 filters of the uint8 volume --------------------------------------------------------------------------- */
enum VkvFilterKind { VKV_FILTER_BINOMIAL3 = 0, VKV_FILTER_MEDIAN3 = 1 };

/* d_dst = d_src filtered over each voxel's 3x3x3 neighbourhood; the result is an ordinary volume for every other entry point.
 * Neighbourhood: for a voxel (x, y, z) of a W x H x D volume, N is the 27 bytes src[clamp(z + dz, 0, D - 1)][clamp(y + dy, 0, H - 1)]
 * [clamp(x + dx, 0, W - 1)], dx, dy, dz in {-1, 0, 1}: clamp-to-edge, as the samplers do.  On a face a clamped neighbour counts as often as
 * it occurs; an axis of extent 1 gives three copies.
 * VKV_FILTER_BINOMIAL3: S = sum of w(dx) w(dy) w(dz) N with w = (1, 2, 1) (the weights sum to 64, S <= 16320), dst = (S + 32) >> 6: integer
 * arithmetic with ONE rounding at the end, not one per axis.  A constant volume is a fixed point.
 * VKV_FILTER_MEDIAN3: dst = the 14th smallest of the 27 bytes of N (index 13 after sorting).
 * box == NULL: every voxel of d_dst is written.  With a box exactly its voxels are written, at their volume positions in d_dst, from d_src's
 * box grown by one voxel and clamped; every other byte of d_dst is untouched.
 * Keeping a filtered copy current across vkv_update_volume_region(box) on the raw volume: after the update, vkv_filter_volume over that box
 * grown by one voxel per side and clipped to the volume, on the same stream, leaves the copy byte-equal to a full refilter.
 * d_src and d_dst may start at any byte; every extent is accepted, widths below 4 and axes of length 1 included; nothing before the first or
 * past the last byte of either buffer is read or written.  Every argument is checked before anything is enqueued, and a rejected call writes
 * nothing.  VKV_E_INVALID_ARGUMENT: a null ctx or pointer, a zero extent, an unknown kind, an empty box or one not inside `extent`, byte
 * ranges [d_src, d_src + n) and [d_dst, d_dst + n) (n = W H D) that overlap (an in-place stencil would read its own output).
 * VKV_E_UNSUPPORTED: a volume too large for one launch.  One kernel launch and nothing else (no memset or copy node, no allocation, no host
 * wait, no scratch block; the kernels use no scratch memory), so after one direct call on `stream` it can be captured into a hipGraph. */
int vkv_filter_volume(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box, int32_t kind, void *stream);

/* ---- isosurface meshes: marching tetrahedra ------------------------------------------------------------------------
 * The isosurface of the uint8 volume as a triangle list in a defined order, every step fp32 IEEE.  f(x, y, z) = (float) byte * kInv255; a
 * voxel is inside if f >= iso (the hit rule of vkv_render_isosurface).  Coordinates are voxel indices: voxel centres lie at integers.
 * Cubes: origins (x, y, z), 0 <= x < W - 1, 0 <= y < H - 1, 0 <= z < D - 1 (an axis of length 1 gives none); with a box only the cubes whose
 * eight voxels all lie in it.  Corner j = dx + 2 dy + 4 dz.  A cube's six tetrahedra, in this order, are the corners T0 = (0, 1, 3, 7),
 * T1 = (0, 1, 5, 7), T2 = (0, 2, 3, 7), T3 = (0, 2, 6, 7), T4 = (0, 4, 5, 7), T5 = (0, 4, 6, 7): the paths from corner 0 to corner 7 that add
 * the axes in a permutation's order; T1, T2, T5 come from odd permutations.  Neighbouring cubes cut their shared face alike.
 * Triangles of a tetrahedron: its local vertices are 0 .. 3 in the order listed; mask m has bit i set if local vertex i is inside; m = 0
 * and m = 15 give nothing.  With `ins` and `out` the inside and outside local vertices in rising order and an edge written as a pair:
 *   one inside vertex p:   [(p, out0), (p, out1), (p, out2)];        one outside vertex p:   [(ins0, p), (ins1, p), (ins2, p)];
 *   two and two, a, b = ins, c, d = out:  A = (a, c), B = (a, d), C = (b, d), D = (b, c);  [A, B, C] and [A, C, D].
 * The second and third vertex of each triangle are swapped iff (the tetrahedron is odd) XOR (m in {2, 5, 8, 10, 11, 14}); then
 * (v1 - v0) x (v2 - v0) points from the inside vertices towards the outside ones in all 6 x 14 cases.
 * Vertex on an edge (i, j): a = the voxel of the LOWER local index, b = the other (b - a is 0 or 1 per axis); t = (iso - f_a) / (f_b - f_a),
 * one subtraction each and a correctly rounded division, no clamp; component c is (float) a_c + t where b_c != a_c, else (float) a_c.  It
 * depends on the edge alone, so shared vertices are bit-equal and the mesh is watertight under exact comparison.  A voxel with f == iso gives
 * t = 0 or 1 and triangles of zero area; they are kept.
 * Order: by cube (x fastest, then y, then z), then tetrahedron 0 .. 5, then triangle; at most 12 per cube.  9 floats per triangle:
 * v0.xyz v1.xyz v2.xyz.
 * d_counts[0] = the exact total, whatever the capacity; d_counts[1] = min(total, capacity_triangles); d_triangles receives exactly the first
 * d_counts[1] triangles of the list and not one float beyond them.  capacity_triangles == 0 (d_triangles may be NULL) is the counting call:
 * no emit work is enqueued.  d_max_map (NULL: dense): vkv_max_map of d_volume with map_extent; a tile of cubes whose cells all hold a byte B
 * with B * kInv255 < iso is counted as empty without reading a voxel: the same bits.  d_scratch: vkv_isosurface_mesh_scratch_bytes(extent,
 * box) bytes (at least 16; 0 for an extent or box this call rejects), 8-byte aligned, the per-row-segment counts and their scan; its
 * contents mean nothing between calls.  d_counts must be 8-byte aligned, d_triangles 4-byte aligned; d_volume may start at any byte.
 * Kernels only (no allocation, no memset or copy node, no host wait, no atomics; the kernels use no scratch memory): after one direct call on
 * `stream` it can be captured into a hipGraph.  Two runs give the same bytes.  Nothing in the context is written.  Every argument is checked
 * before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_volume, d_scratch or d_counts, a
 * zero extent, a non-finite iso, an empty box or one not inside `extent`, a max map without a valid map_extent, a non-zero capacity with a
 * NULL d_triangles, a misaligned d_scratch, d_counts or d_triangles.  VKV_E_UNSUPPORTED: a volume too large for the launches.  Every extent
 * is accepted; nothing outside any buffer is read or written. */
size_t vkv_isosurface_mesh_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_isosurface_mesh(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, const uint8_t *d_max_map,
                        VkvExtent3D map_extent, void *d_scratch, float *d_triangles, uint64_t capacity_triangles, uint64_t *d_counts, void *stream);

/* ---- indexed isosurface meshes with vertex normals ---------------------------------------------------------------------
 * The same surface as a vertex list and three vertex numbers per triangle.  Everything not restated here is as for vkv_isosurface_mesh: f,
 * the inside rule, cubes, tetrahedra, case rules, winding, coordinates, the box rule, the max-map rule (a tile of VOXELS whose cells all stay
 * below iso owns no vertex and starts no triangle: the same bits), and that every argument is checked before anything is enqueued.
 * Vertex list.  An EDGE is a pair (voxel v, direction d = dx + 2 dy + 4 dz, 1 <= d <= 7; v + d means v + (dx, dy, dz)) with both v and v + d
 * inside the box, and every axis of the box at least 2 voxels long (an axis of length 1 gives no cubes and no edges).  These are exactly the
 * tetrahedron edges of the box's cubes: every such edge runs from a cube corner a to a corner b with a & b == a.  An edge is CROSSING if
 * inside(v) != inside(v + d).  The vertex list is the crossing edges ordered by v (x fastest, then y, then z), then by d rising: one vertex
 * per crossing edge.  Position: a = v, b = v + d, t = (iso - f_a) / (f_b - f_a), component c is (float) a_c + t where d has that axis, else
 * (float) a_c: the vertex rule above, so positions are bit-equal to the triangle list's.  Where a voxel equals iso exactly, several edges
 * give bit-equal positions; they stay separate vertices, as the triangle list keeps its triangles of zero area.  3 floats per vertex.
 * Normals (d_normals may be NULL: none are computed).  For a voxel p of the VOLUME, G_c(p) = (int) vol[p + e_c] - (int) vol[p - e_c], both
 * neighbours clamped to the volume (not to the box: a box's normals equal the whole volume's).  n_c = -((float) G_c(a) + t * (float) (G_c(b)
 * - G_c(a))) with a, b, t of the vertex: both integers are exact in fp32, then one multiplication, one addition (no FMA) and the sign flip.
 * Not normalised (the length is in bytes per two voxels), may be zero, points from the inside to the outside on a smooth field.  3 floats
 * per vertex, parallel to d_vertices.
 * Indices.  The triangles of vkv_isosurface_mesh in the same order, 3 x uint32 each (v0 v1 v2): the edge (a, b) of the cube with origin o is
 * the edge (o + a, a ^ b), and its index is that edge's position in the FULL vertex list, reduced mod 2^32; it depends on neither capacity.
 * d_counts holds four values: [0] = the total number of triangles, [1] = min([0], capacity_triangles), [2] = the total number of vertices,
 * [3] = min([2], capacity_vertices).  Exactly the first [1] triangles' indices and the first [3] vertices (and their normals, if asked for)
 * are written, and not one element beyond them.  A capacity of zero for either list (its pointers NULL or not) enqueues no emit for that
 * list; both zero is the counting call.  capacity_vertices may not exceed 0xffffffff, so a call with [2] == [3] has exact indices; a larger
 * surface is extracted box by box.  d_scratch: vkv_isosurface_mesh_indexed_scratch_bytes(extent, box) bytes (at least 16, a multiple of 8;
 * 0 for an extent or box this call rejects; 16 bytes per 256 x-adjacent voxels of a row of the box), 8-byte aligned; its contents mean
 * nothing between calls.  d_volume may start at any byte; every extent is accepted; nothing outside any buffer is read or written.
 * Kernels only (no allocation, no memset or copy node, no host wait, no atomics; the kernels use no scratch memory): two runs give the same
 * bytes, and after one direct call on `stream` it can be captured into a hipGraph.  Nothing in the context is written.  A rejected call
 * writes nothing.  VKV_E_INVALID_ARGUMENT: everything vkv_isosurface_mesh rejects (a null ctx, d_volume, d_scratch or d_counts, a zero
 * extent, a non-finite iso, an empty box or one not inside `extent`, a max map without a valid map_extent), capacity_vertices > 0xffffffff,
 * a non-zero capacity_vertices with a NULL d_vertices or capacity_triangles with a NULL d_indices, d_normals with capacity_vertices == 0, a
 * d_vertices, d_normals or d_indices that is not 4-byte aligned, a d_counts or d_scratch that is not 8-byte aligned.  VKV_E_UNSUPPORTED: a
 * volume too large for the launches.
 * Not here: smoothing, and normals from the faces instead of the volume, are vkv_mesh_smooth and vkv_mesh_vertex_normals (DESIGN.md
 * §5.24); decimation is vkv_mesh_decimate.  They take this call's buffers and d_counts as they are. */
size_t vkv_isosurface_mesh_indexed_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_isosurface_mesh_indexed(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, const uint8_t *d_max_map,
                                VkvExtent3D map_extent, void *d_scratch, float *d_vertices, float *d_normals, uint64_t capacity_vertices,
                                uint32_t *d_indices, uint64_t capacity_triangles, uint64_t *d_counts, void *stream);

/* ---- connected components and island removal ---------------------------------------------------------------------------
 * vkv_label_components numbers the connected components of the inside voxels of a box; vkv_select_components keeps or fills them by size.
 * Inside rule: the mesh's.  f = (float) byte * kInv255, and a voxel is inside iff f >= iso.
 * Voxels and connections.  Only the voxels of `box` take part (NULL: the whole volume), and connections run only through voxels of the box.
 * Two inside voxels are adjacent if their offset (dx, dy, dz) lies in the neighbourhood `connectivity`:
 *   VKV_CONNECT_6:  the six unit offsets;
 *   VKV_CONNECT_14: +-(dx, dy, dz) with dx, dy, dz in {0, 1}, not all zero.  These are exactly the tetrahedron edges of vkv_isosurface_mesh
 *                   (cube corners a, b with a & b == a), so the components are precisely the bodies that the mesh's surface separates;
 *   VKV_CONNECT_26: every offset in {-1, 0, 1}^3 except zero.
 * A component is a class of the transitive closure of adjacency.
 * Labels.  d_labels has the box's shape, box.width x box.height x box.depth with x fastest (NULL box: the volume's shape); every element is
 * written.  0: an outside voxel; k in 1 .. K: component k.  Components are numbered in the order of their first voxel, i.e. their smallest
 * box-linear index i = ((z - z0) bh + (y - y0)) bw + (x - x0): the numbering of scipy.ndimage.label with the matching structure.
 * Sizes.  d_sizes[k - 1] = the voxel count of component k for k <= d_counts[1]; not one element beyond that is written.  With
 * capacity_components == 0 d_sizes may be NULL and no size work is enqueued.
 * Counts.  d_counts[0] = K, exact whatever the capacity; d_counts[1] = min(K, capacity_components); d_counts[2] = the number of inside voxels.
 * d_max_map (NULL: dense): vkv_max_map of d_volume with map_extent; the voxels of a cell that holds a byte B with B * kInv255 < iso get label
 * 0 without being read: the same bits as the dense path.  The map is consulted per voxel, so all it saves is the voxel's own byte read, one
 * of the five bytes per voxel the call moves; it is measured to be no faster than the dense path.
 * d_scratch: vkv_label_components_scratch_bytes(extent, box) bytes, 8-byte aligned: 24 bytes per 64 voxels of the box (rounded up) plus 16
 * bytes per 262144 voxels (rounded up), three eighths of a byte per voxel; 0 for an extent or box this call rejects.  Its contents mean
 * nothing between calls.
 * Kernels only (no allocation, no memset or copy node, no host wait; the kernels use no scratch memory, and none waits for another lane, wave
 * or workgroup): after one direct call on `stream` it can be captured into a hipGraph.  Integer atomics (minimum, addition) are used where the
 * result does not depend on their order: two runs give the same bytes in d_labels, d_sizes and d_counts.  Nothing in the context is written.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_volume,
 * d_scratch, d_labels or d_counts, a zero extent, a non-finite iso, an unknown connectivity, an empty box or one not inside `extent`, a max
 * map without a valid map_extent, a non-zero capacity with a NULL d_sizes, a d_labels or d_sizes that is not 4-byte aligned, a d_counts or
 * d_scratch that is not 8-byte aligned, a capacity_components above 0xffffffff.  VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels
 * (labels are uint32; a larger volume goes box by box).  d_volume may start at any byte; every extent is accepted, widths below 4 and axes
 * of length 1 included; nothing outside any buffer is read or written.
 *
 * vkv_select_components: pointwise, one kernel launch.  For every voxel v of the box, at its volume position in d_dst, with L = d_labels[v]
 * (the box's shape, as written by vkv_label_components for the same box): L == 0: dst = src; L > d_counts[1] (its size is not known): dst =
 * src, what is not known is not removed; otherwise dst = src if min_voxels <= d_sizes[L - 1] <= max_voxels, else dst = fill.  Bytes of d_dst
 * outside the box are untouched.  d_counts is read on the device: no host wait.  d_sizes may be NULL where d_counts[1] is 0 (nothing is
 * removed then).  d_dst == d_src is allowed (in place); any other overlap of [d_src, d_src + W H D) and [d_dst, d_dst + W H D) is
 * VKV_E_INVALID_ARGUMENT, as are a null ctx, d_src, d_dst, d_labels or d_counts, a zero extent, an empty box or one not inside `extent`,
 * fill > 255, min_voxels > max_voxels, a d_labels or d_sizes that is not 4-byte aligned and a d_counts that is not 8-byte aligned.
 * VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels.  The result is an ordinary volume for every other entry point. */
#define VKV_CONNECT_6 6
#define VKV_CONNECT_14 14
#define VKV_CONNECT_26 26
size_t vkv_label_components_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_label_components(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t connectivity,
                         const uint8_t *d_max_map, VkvExtent3D map_extent, void *d_scratch, uint32_t *d_labels, uint32_t *d_sizes,
                         uint64_t capacity_components, uint64_t *d_counts, void *stream);
int vkv_select_components(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_labels,
                          const uint32_t *d_sizes, const uint64_t *d_counts, uint64_t min_voxels, uint64_t max_voxels, uint32_t fill, void *stream);

/* ---- measurements of labelled components and selection by table ----------------------------------------------------------
 * vkv_component_stats writes one record per label: bounding box, voxel count, coordinate sums (the centroid) and, with a volume, the
 * smallest and largest byte and the sums of bytes and squared bytes (mean and variance).  vkv_select_components_by_table keeps or fills
 * components by a table of one byte per label, so any rule computed from the records is applied on the device: neither the labels nor the
 * voxels leave it.
 * Inputs.  d_labels has the box's shape, box.width x box.height x box.depth with x fastest (NULL box: the volume's shape), as written by
 * vkv_label_components for the same box; any array of that shape whose values lie in 0 .. d_counts[0] is accepted as well, so a caller's own
 * segmentation can be measured.  Of d_counts only d_counts[0], the number of labels, is read, and it is read on the device: no host wait.
 * What is written.  written = min(d_counts[0], capacity_components).  The records d_stats[0 .. written) are written completely, record
 * k - 1 for label k; not one byte beyond them is touched.  Voxels with label 0 and voxels with a label above `written` are ignored.
 * A record.  min_* / max_*: the inclusive bounding box of the label's voxels in VOLUME coordinates (the box's origin is added), voxels: their
 * number, sum_x, sum_y, sum_z: the sums of their volume coordinates (centroid = sum / voxels), min_value, max_value, sum_value, sum_value2:
 * the smallest and the largest of their bytes of d_volume, the sum of the bytes and the sum of their squares (mean = sum_value / voxels,
 * variance = sum_value2 / voxels - mean^2).  A label that no voxel carries gets voxels = 0, sums 0, mins 0xffffffff and maxes 0.  d_volume ==
 * NULL is allowed: the four value fields of every written record are then 0 and no byte of a volume is read.  No sum can overflow: the box
 * holds fewer than 2^32 voxels, every coordinate is below 2^32 and a squared byte is below 2^16, so every sum stays below 2^64.
 * Kernels only (no allocation, no memset or copy node, no host wait; no scratch buffer is needed, the kernels use no scratch memory, and none
 * waits for another lane, wave or workgroup): after one direct call on `stream` it can be captured into a hipGraph.  Integer atomics
 * (addition, minimum, maximum) are used where the result does not depend on their order: two runs give the same bytes.  Nothing in the
 * context is written.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_labels
 * or d_counts, a null d_stats with a non-zero capacity, a zero extent, an empty box or one not inside `extent`, a d_labels that is not
 * 4-byte aligned, a d_counts or d_stats that is not 8-byte aligned, a capacity_components above 0xffffffff.  VKV_E_UNSUPPORTED: a box of more
 * than 2^32 - 1 voxels.  capacity_components == 0 is VKV_OK and enqueues nothing.  d_volume may start at any byte; every extent is
 * accepted, widths below 4 and axes of length 1 included; nothing outside any buffer is read or written.
 *
 * vkv_select_components_by_table: pointwise, one kernel launch.  For every voxel v of the box, at its volume position in d_dst, with L =
 * d_labels[v] (the box's shape): L == 0 or L > table_entries: dst = src, what the table does not name is not removed; d_keep[L - 1] != 0:
 * dst = src; d_keep[L - 1] == 0: dst = fill.  Bytes of d_dst outside the box are untouched.  d_keep (table_entries bytes, any alignment) may
 * be NULL with table_entries == 0.  d_dst == d_src is allowed (in place); any other overlap of [d_src, d_src + W H D) and [d_dst, d_dst + W
 * H D) is VKV_E_INVALID_ARGUMENT, as are a null ctx, d_src, d_dst or d_labels, a null d_keep with table_entries != 0, a zero extent, an
 * empty box or one not inside `extent`, fill > 255 and a d_labels that is not 4-byte aligned.  VKV_E_UNSUPPORTED: a box of more than 2^32 - 1
 * voxels.  The result is an ordinary volume for every other entry point. */
typedef struct VkvComponentStats {        /* 80 bytes, 8-byte aligned; offsets 0 4 8 | 12 16 20 | 24 28 | 32 | 40 48 56 | 64 72 */
    uint32_t min_x, min_y, min_z;         /* bounding box, VOLUME coordinates, inclusive */
    uint32_t max_x, max_y, max_z;
    uint32_t min_value, max_value;        /* the component's smallest and largest byte of d_volume */
    uint64_t voxels;
    uint64_t sum_x, sum_y, sum_z;         /* sums of volume coordinates: centroid = sum / voxels */
    uint64_t sum_value, sum_value2;       /* sum of bytes and of squared bytes: mean and variance */
} VkvComponentStats;
int vkv_component_stats(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_labels,
                        const uint64_t *d_counts, VkvComponentStats *d_stats, uint64_t capacity_components, void *stream);
int vkv_select_components_by_table(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box,
                                   const uint32_t *d_labels, const uint8_t *d_keep, uint64_t table_entries, uint32_t fill, void *stream);

/* ---- exact Euclidean distance transform and ball morphology ---------------------------------------------------------------
 * vkv_distance_transform writes the exact squared Euclidean distance of every voxel of a box to the nearest TARGET voxel of the box;
 * vkv_select_by_distance fills the voxels whose distance lies in a range: ball erosion and dilation (hence opening and closing), shells,
 * margins.  (vkv_distance_map is something else: the Chebyshev transform of the occupancy CELLS that the ray-march skips by.)
 * Inside rule: the mesh's.  f = (float) byte * kInv255, and a voxel is inside iff f >= iso.
 * Voxels.  Only the voxels of `box` exist (NULL: the whole volume): nothing beyond the box counts as inside or as outside.
 * Targets.  VKV_DISTANCE_TO_INSIDE: the inside voxels of the box; VKV_DISTANCE_TO_OUTSIDE: its outside voxels.
 * Output.  d_dist2 has the box's shape, box.width x box.height x box.depth with x fastest (NULL box: the volume's shape); every element is
 * written: d_dist2[v] = min(limit, min over the target voxels u of the box of |v - u|^2), |v - u|^2 = dx^2 + dy^2 + dz^2 in voxel units, an
 * integer: 0 on a target voxel, and `limit` everywhere where the box holds no target voxel.  limit == VKV_DISTANCE_NONE (0xffffffff) means
 * unlimited (a true distance is at most 3 x 32767^2 < 0xffffffff); limit == 0 is invalid.  All arithmetic is integer and compares squares:
 * no square root, no float, so the result is unique and two runs give the same bytes.  A limited transform costs less: the work per voxel
 * grows with the distance found, and the limit cuts it (morphology by radius^2 r2 needs limit = r2 + 1 only).
 * d_scratch: vkv_distance_transform_scratch_bytes(extent, box) bytes, 8-byte aligned: 8 bytes per 64 voxels of the box (rounded up), the
 * target bits, plus 4 bytes per voxel of the box, the second distance buffer: 4 B and one bit per voxel; 0 for an extent or box this call
 * rejects.  Its contents mean nothing between calls.
 * Kernels only (no allocation, no memset or copy node, no host wait, no atomics; the kernels use no scratch memory, and none waits for another
 * lane, wave or workgroup): after one direct call on `stream` it can be captured into a hipGraph.  Nothing in the context is written.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_volume,
 * d_scratch or d_dist2, a zero extent, a non-finite iso, an unknown target, limit == 0, an empty box or one not inside `extent`, a d_dist2
 * that is not 4-byte aligned, a d_scratch that is not 8-byte aligned.  VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels or with an axis
 * above 32768 (a larger volume goes box by box).  d_volume may start at any byte; every extent is accepted, widths below 4 and axes of
 * length 1 included; nothing outside any buffer is read or written.
 *
 * vkv_select_by_distance: pointwise, one kernel launch.  For every voxel v of the box, at its volume position in d_dst: dst = fill if lo <=
 * d_dist2[v] <= hi (d_dist2: the box's shape, as written by vkv_distance_transform for the same box), else dst = src.  Bytes of d_dst outside
 * the box are untouched.  Erosion by a ball of radius^2 r2: VKV_DISTANCE_TO_OUTSIDE, then (lo, hi, fill) = (1, r2, a byte below iso);
 * dilation: VKV_DISTANCE_TO_INSIDE, then (1, r2, a byte at or above iso); an opening is an erosion and a dilation of its result, a closing the
 * reverse.  Since nothing exists beyond the box, an erosion does not eat at the box's faces (scipy's border_value=1).  d_dst == d_src is
 * allowed (in place); any other overlap of [d_src, d_src + W H D) and [d_dst, d_dst + W H D) is VKV_E_INVALID_ARGUMENT, as are a null ctx,
 * d_src, d_dst or d_dist2, a zero extent, an empty box or one not inside `extent`, fill > 255, lo > hi and a d_dist2 that is not 4-byte
 * aligned.  VKV_E_UNSUPPORTED: as above.  The result is an ordinary volume for every other entry point. */
#define VKV_DISTANCE_NONE 0xffffffffu
enum VkvDistanceTarget { VKV_DISTANCE_TO_INSIDE = 0, VKV_DISTANCE_TO_OUTSIDE = 1 };
size_t vkv_distance_transform_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_distance_transform(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target,
                           uint32_t limit, void *d_scratch, uint32_t *d_dist2, void *stream);
int vkv_select_by_distance(vkv_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, VkvExtent3D extent, const VkvBox *box,
                           const uint32_t *d_dist2, uint32_t lo, uint32_t hi, uint32_t fill, void *stream);

/* ---- the distance transform with a weight per axis: voxel spacing ---------------------------------------------------------
 * vkv_distance_transform_weighted is vkv_distance_transform for voxels that are not cubes: `weights` is a HOST pointer to three integers
 * (wx, wy, wz), read during the call, and
 *   d_dist2[v] = min(limit, min over the target voxels u of the box of (wx dx)^2 + (wy dy)^2 + (wz dz)^2),
 * an integer again, so the result is unique and two runs give the same bytes.  A scan of 0.5 x 0.5 x 1.25 mm voxels takes (2, 2, 5): the
 * values are squared distances in units of 0.25 mm.  Everything else is as above: the inside rule, the targets, only the box exists, the
 * box-shaped output with every element written, `limit` everywhere where the box holds no target, VKV_DISTANCE_NONE for unlimited, limit == 0
 * invalid.  With weights (1, 1, 1) the bytes are those of vkv_distance_transform.  The result feeds vkv_select_by_distance unchanged; lo and
 * hi are then in weighted units (an erosion by r^2 removes what lies within sum (w_a k_a)^2 <= r^2 of the outside).
 * d_scratch: the SAME block, vkv_distance_transform_scratch_bytes(extent, box) bytes, 8-byte aligned; one allocation serves both calls.
 * The y and z passes build the lower envelope of each line's parabolas (one line per lane; the envelope's stack lives in the line of the
 * output that it is about to overwrite), so the cost does not grow with the distance found, as that of vkv_distance_transform does: this
 * call is the one for large or unlimited distances, the other one for small limits (README.md has the measured crossover).
 * Kernels only (no allocation, no memset or copy node, no host wait, no atomics; the kernels use no scratch memory, and none waits for another
 * lane, wave or workgroup): after one direct call on `stream` it can be captured into a hipGraph.  Nothing in the context is written.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: everything that
 * vkv_distance_transform rejects so, a null `weights` and a weight of 0.  VKV_E_UNSUPPORTED: everything that vkv_distance_transform rejects
 * so, and weights whose largest possible value does not fit: the sum over the axes of (w_a (len_a - 1))^2, len the box's shape, must be at
 * most 0xfffffffe, with every w_a (len_a - 1) at most 65535 (an axis of length 1 admits every weight but 0). */
int vkv_distance_transform_weighted(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target,
                                    const uint32_t weights[3], uint32_t limit, void *d_scratch, uint32_t *d_dist2, void *stream);

/* ---- the nearest-target (feature) transform and label propagation --------------------------------------------------------
 * vkv_nearest_target says not how far the nearest target is but WHICH it is.  The inside rule, the targets, "only the box exists", `weights`
 * (a HOST pointer, read during the call) and `limit` are exactly those of vkv_distance_transform_weighted.  With D(v) the least
 * (wx dx)^2 + (wy dy)^2 + (wz dz)^2 over the box's targets, d_nearest (uint32, the box's shape, every element written) is
 *   d_nearest[v] = the SMALLEST BOX-LINEAR INDEX ((z' - z0) height + (y' - y0)) width + (x' - x0) among the targets at distance D(v)
 *                  if the box holds a target and D(v) < limit,
 *                  VKV_NEAREST_NONE otherwise.
 * A box holds at most 2^32 - 1 voxels, so no index equals VKV_NEAREST_NONE; a target voxel's nearest target is itself.  The tie rule makes
 * the answer unique: two runs, and any two correct implementations, give the same bytes.  d_dist2 may be NULL; otherwise it receives
 * min(limit, D(v)), byte for byte what vkv_distance_transform_weighted writes.
 * d_scratch: the SAME block, vkv_distance_transform_scratch_bytes(extent, box) bytes, 8-byte aligned: the passes carry features, not
 * distances, between d_nearest and the block's uint32 buffer.  Kernels only (no allocation, no memset or copy node, no host wait, no
 * atomics, no scratch memory, no lane waits for another): after one direct call on `stream` it can be captured into a hipGraph.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  The codes are those of
 * vkv_distance_transform_weighted; also VKV_E_INVALID_ARGUMENT: a null d_nearest, a d_nearest or a non-NULL d_dist2 that is not 4-byte
 * aligned, and a d_dist2 that overlaps d_nearest.
 *
 * vkv_propagate_labels is the gather that every use of d_nearest comes to.  All three arrays have the box's shape (uint32, 4-byte aligned):
 *   d_out[v] = 0                          if d_nearest[v] == VKV_NEAREST_NONE, or is any other value >= the box's voxels (nothing is read),
 *            = 0                          if d_mask_volume is given and voxel v of it is outside (the inside rule, with mask_iso),
 *            = d_labels[d_nearest[v]]     otherwise.
 * d_mask_volume == NULL: no mask, and no byte of a volume is read.  d_out may overlap neither d_labels nor d_nearest (the call is a gather):
 * VKV_E_INVALID_ARGUMENT, as are a null array, a bad box, a misaligned array and (with a mask) a mask_iso that is not finite;
 * VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels.  One launch.  With d_labels of vkv_label_components the result is a label array
 * with values in 0 .. K, which vkv_component_stats and vkv_select_components_by_table take unchanged.  Erode, label, vkv_nearest_target of
 * the eroded volume, propagate with the original volume as the mask: touching bodies split at full size ("nearest" is Euclidean, not
 * geodesic). */
#define VKV_NEAREST_NONE 0xffffffffu
int vkv_nearest_target(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, int32_t target,
                       const uint32_t weights[3], uint32_t limit, void *d_scratch, uint32_t *d_nearest, uint32_t *d_dist2, void *stream);
int vkv_propagate_labels(vkv_ctx *ctx, const uint32_t *d_nearest, const uint32_t *d_labels, uint32_t *d_out, VkvExtent3D extent,
                         const VkvBox *box, const uint8_t *d_mask_volume, float mask_iso, void *stream);

/* ---- geodesic distance and label propagation inside the mask ---------------------------------------------------------------
 * vkv_geodesic_propagate answers "how far is this voxel from a seed THROUGH the inside voxels, and from which seed": the geodesic distance map
 * with chamfer step costs, and the labels that travel with it.  Every other distance of this header crosses walls; this one does not.
 * The inside rule, "only the voxels of `box` exist" and the box-shaped arrays (x fastest) are those of vkv_label_components.
 * Moves.  From an inside voxel to an inside voxel of the box at an offset (dx, dy, dz) in {-1, 0, 1}^3 other than 0.  The offset's class is
 * m = |dx| + 2 |dy| + 4 |dz|, 1 .. 7, and the move costs steps[m - 1]; `steps` is a HOST pointer to seven integers, read during the call.  A
 * cost of 0 means that this class of move does not exist.  Both ends inside is all a move needs: a diagonal move may pass between two outside
 * voxels, so with every class present the mask's connectivity is VKV_CONNECT_26.  (1, 1, 0, 1, 0, 0, 0) counts 6-connected steps;
 * (3, 3, 4, 3, 4, 4, 5) is the 3-4-5 chamfer (distances in thirds of a voxel); a table made from the voxel spacing gives a length.
 * Seeds.  d_seeds (uint32, the box's shape): a non-zero value on an inside voxel makes it a seed with that value as its label; non-zero
 * values on outside voxels are ignored.
 * The result.  key(v) = the lexicographic minimum of (cost, seed label) over all paths of moves from a seed to v, the cost of a path being the
 * sum of its moves': of all seeds at the least cost the SMALLEST LABEL wins, so the answer is unique.  v is REACHED iff that least cost is
 * below `limit`; VKV_GEODESIC_NONE (0xffffffff) means unlimited, so a stored cost is at most 0xfffffffe; limit == 0 is invalid.  Costs are
 * summed in 64 bits.  Either output may be NULL, not both; every element of a given output is written:
 *   d_dist[v]   = the least cost, VKV_GEODESIC_NONE where v is not reached or outside,
 *   d_labels[v] = that label, 0 where v is not reached or outside.
 * Rounds.  The work is done in rounds, each one kernel over tiles of 8 x 8 x 8 voxels: a tile whose surroundings changed in the round before
 * relaxes its voxels until nothing in it changes.  A body is settled after about as many rounds as the longest shortest path crosses tiles.
 * resume == 0: the state is set up from d_seeds, then `rounds` rounds (1 .. VKV_GEODESIC_MAX_ROUNDS) run, then the outputs are written.
 * resume == 1: d_seeds is not read and may be NULL; d_scratch holds the state an earlier call left for the same volume, box, iso, steps and
 * limit (the caller's promise); the call runs `rounds` more rounds and writes the outputs again.
 * d_counts (2 x uint64): d_counts[0] = 1 iff the last round that did any work left no tile to be relaxed again, i.e. the state is the fixed
 * point, else 0; d_counts[1] = the reached voxels.  While d_counts[0] is 0 the outputs are upper bounds whose bytes are not specified; once it
 * is 1 they are the definition's, further rounds cost an empty launch each and change nothing, and two runs give the same bytes.
 * d_scratch: vkv_geodesic_scratch_bytes(extent, box) bytes, 8-byte aligned: 8 bytes per voxel of the box (cost and label, kept as ONE 64-bit
 * value) + 32 + 8 per tile, the tiles being ceil(width / 8) ceil(height / 8) ceil(depth / 8) of the box; 0 for an extent or box this call
 * rejects.  Between a call and the call that resumes it the block is the state and must be left alone.
 * d_labels == d_seeds is allowed (labels grow in place); any other overlap among d_seeds, d_dist, d_labels (4 bytes per voxel of the box each)
 * and the scratch block is VKV_E_INVALID_ARGUMENT.
 * Kernels only (no allocation, no memset or copy node, no host wait; the host never reads a flag; the kernels use no scratch memory, and no
 * lane waits for another wave or workgroup): after one direct call on `stream` it can be captured into a hipGraph.  Keys are exchanged
 * between workgroups by relaxed 64-bit atomic loads and stores, the count is an integer atomic sum.  Nothing in the context is written.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_volume,
 * d_scratch, d_counts or steps, a null d_seeds with resume == 0, both outputs null, a zero extent, an empty box or one not inside `extent`, a
 * non-finite iso, limit == 0, rounds == 0 or above VKV_GEODESIC_MAX_ROUNDS, a resume other than 0 and 1, seven steps of 0, a step above
 * 65535, a d_seeds, d_dist or d_labels that is not 4-byte aligned, a d_counts or d_scratch that is not 8-byte aligned, the overlaps above.
 * VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels.  d_volume may start at any byte; every extent is accepted, axes of length 1
 * included; nothing outside any buffer is read or written. */
#define VKV_GEODESIC_NONE 0xffffffffu
#define VKV_GEODESIC_MAX_ROUNDS 1024
size_t vkv_geodesic_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_geodesic_propagate(vkv_ctx *ctx, const uint8_t *d_volume, VkvExtent3D extent, const VkvBox *box, float iso, const uint32_t *d_seeds,
                           const uint32_t steps[7], uint32_t limit, uint32_t rounds, int32_t resume, void *d_scratch, uint32_t *d_dist,
                           uint32_t *d_labels, uint64_t *d_counts, void *stream);

/* ---- label volumes as pictures: per-label colours, pick buffer, exact skipping ---------------------------------------------
 * What vkv_label_components, vkv_propagate_labels, vkv_geodesic_propagate and the calls built on them produce is a uint32 label array of the
 * shape of a box (x fastest; box == NULL: of the volume; at most 2^32 - 1 voxels).  These two calls show it: every body in its own colour,
 * bodies switched off by a table entry, and the label under each pixel.
 * Visible.  d_colors holds table_entries words of uint32; entry L - 1 belongs to label L (the convention of vkv_select_components_by_table);
 * R is bits 0-7, G bits 8-15, B bits 16-23, A bits 24-31.  visible(L) iff 1 <= L <= table_entries and the A byte of d_colors[L - 1] is not 0.
 * Alpha only switches a label on or off: a visible label is opaque.  Label 0 and every label the table does not name are never visible.
 * Voxel of a texture-space point q, per axis: c = fma(q, (float) extent, -0.5f) (the samplers' own coordinate), v = clamp((int) floorf(c +
 * 0.5f), 0, extent - 1).  label(q) = 0 if that voxel lies outside `box`, else d_labels[((z - z0) bh + (y - y0)) bw + (x - x0)].
 *
 * vkv_label_visibility_map: one byte per cell of map_extent, the geometry of vkv_max_map.  A cell holds 255 if any voxel of the cell's voxel
 * box, grown by one voxel per side and clipped to the volume, lies in `box` and carries a visible label; otherwise, and past the volume, 0.
 * Every cell is written.  The map depends on the labels and on the table: rebuild it after either changes.  Kernels only (one launch: no
 * memset, no allocation, no host wait, no scratch block; the kernel uses no scratch memory), so after one direct call on `stream` it can be
 * captured into a hipGraph.  Every argument is checked before anything is enqueued, and a rejected call writes nothing.
 * VKV_E_INVALID_ARGUMENT: a null ctx, d_labels or d_map, a null d_colors with table_entries != 0, a d_labels or d_colors that is not 4-byte
 * aligned, a zero extent, a map_extent that is not valid for it, an empty box or one not inside `extent`.  VKV_E_UNSUPPORTED: a box of more
 * than 2^32 - 1 voxels, a map too large for one launch. */
int vkv_label_visibility_map(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors,
                             uint64_t table_entries, VkvExtent3D map_extent, uint8_t *d_map, void *stream);

typedef struct VkvLabelRenderOptions
{
	const uint32_t *d_labels;         /* the labels of `box`, uint32, 4-byte aligned                                                              */
	const VkvBox *  box;              /* HOST pointer, read during the call; NULL: the whole volume                                               */
	const uint32_t *d_colors;         /* table_entries colour words, 4-byte aligned; may be NULL with table_entries == 0 (nothing is visible)     */
	uint64_t        table_entries;
	uint32_t        refine_steps;     /* 0 .. 16 bisection steps between samples k - 1 and k                                                      */
	uint32_t        shade;            /* 0: the table's colour as it is (d_volume is not read and may be NULL); 1: lit by the isosurface's headlight */
	float           ambient, diffuse, specular; /* finite, >= 0 (checked with shade == 0 too)                                                    */
	uint32_t        shininess;        /* 1 .. 1024                                                                                                */
	const uint8_t * d_visibility_map; /* vkv_label_visibility_map of d_labels, box and d_colors with params->map_extent, or NULL (dense)         */
	uint32_t *      d_out_label;      /* the label under each pixel, indexed like the other outputs; 0 without a hit; or NULL: the pick buffer    */
	float *         d_out_normal;     /* as VkvIsoOptions.d_out_normal; zeros with shade == 0; or NULL                                            */
	uint32_t        flags;            /* must be 0 */
} VkvLabelRenderOptions;

/* The first visible label along each ray.  Rays, samples q_i = fma(i, s, e), clipping plane, options.depth_attachment with d_in_depth,
 * sampling_factor, the tile schedules (whole image, rect, compact strided shares that assemble through vkv_scatter_tiles) and what is
 * unsupported are vkv_render_isosurface's.  k = the first i with visible(label(q_i)).  t = 0 for k == 0, else the isosurface's bisection
 * between k - 1 and k on the predicate visible(label(fma(mid, s, e))): hi = mid where it holds, else lo = mid; t = hi.  p = fma(t, s, e),
 * L = label(p), visible by construction.  A pixel with a hit gets d_out_label = L, d_out_depth the first-hit depth of p, and base_c =
 * (float) byte_c * kInv255 of d_colors[L - 1].  shade == 0: RGBA32F (base, 1), normal zeros; RGBA8 is then exactly the table's bytes with
 * A = 255.  shade == 1: the normal n from the isosurface's tetrahedron gradient of d_volume (linear or packed: the same bits) at p, its
 * headlight term L_light in its order of operations, RGBA32F (clamp(base L_light, 0, 1), 1), d_out_normal (n, 1).  RGBA8 is the
 * round-to-nearest of the colour.  Every other pixel gets what the isosurface gives a pixel without a hit, and label 0.  d_out_counts (3 x
 * u32 per pixel): samples looked up on the march, map bytes read, samples skipped; [0] + [2] is k + 1 on a hit and the ray's sample count
 * without one (refinement and gradient taps are not counted).
 * With d_visibility_map a ray jumps over the samples of a cell whose byte is 0: the results equal the dense path's bit for bit (a sample in
 * the grown cell has its voxel in the grown box the byte covers: DESIGN.md §5.21).  A map built for other labels or another table breaks that.
 * VKV_E_INVALID_ARGUMENT: null params or options, null d_labels, null d_colors with table_entries != 0, misaligned d_labels or d_colors, an
 * empty box or one not inside volume_extent, shade > 1, shade == 1 without d_volume, flags != 0, refine_steps > 16, a negative or non-finite
 * coefficient, shininess outside 1 .. 1024, a map without a valid map_extent, no output at all, and what vkv_render_isosurface rejects of the
 * fields read.  VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels, blend_over_target, tiles.fill_outside, options.test != VKV_TEST_NONE.
 * Every argument is checked before anything is enqueued: a rejected call writes nothing.  One kernel launch and nothing else (no scratch
 * block, no table, no allocation, no host wait; the kernels use no scratch memory), so after one direct call on `stream` it can be captured
 * into a hipGraph. */
int vkv_render_labels(vkv_ctx *ctx, const VkvRenderParams *params, const VkvLabelRenderOptions *labels, void *stream);

/* ---- label volumes as meshes: one closed surface per visible body -----------------------------------------------------------
 * vkv_label_mesh: the surfaces of the visible bodies of a label array as a triangle list in a defined order, with one uint32 label per
 * triangle.  Everything not restated here is vkv_isosurface_mesh's: the cubes whose eight voxels lie in `box`, the corner numbering, the six
 * tetrahedra in their order and their local vertices, the triangles of a mask m and the winding swap (odd tetrahedron XOR m in {2, 5, 8, 10,
 * 11, 14}), the coordinates, the order by cube (x fastest, then y, then z) and then tetrahedron, 9 floats per triangle.
 * Labels.  d_labels has the shape of `box` (x fastest; box == NULL: of the volume), 4-byte aligned.  visible(L) is vkv_render_labels' rule:
 * 1 <= L <= table_entries and the A byte of d_colors[L - 1] is not 0.  For this call only, d_colors == NULL with table_entries == 0 means
 * "every non-zero label is visible" (a table that shows nothing would give an empty mesh).
 * Per tetrahedron.  Walk its local vertices 0 .. 3.  Each visible label L that has not appeared at a lower local vertex of this tetrahedron
 * starts a group, so the groups are ordered by the first local vertex that carries L.  For each group, bit i of m is set if local vertex i
 * carries exactly L; the triangles of case m are emitted with the isosurface's winding ("inside" = "carries L"), each tagged L in
 * d_triangle_labels.  Hidden and zero labels start no group and are outside for every group.  A tetrahedron gives at most 4 triangles (label
 * patterns 1+1+1+1, 2+1+1 and 2+2 give 4; 3+1 gives 2), a cube at most 24.
 * Vertex on an edge (i, j) of local vertices: a = the voxel of the lower local index, b = the other; it depends on the edge alone, never on
 * L.  If d_volume is not NULL and (f_a >= iso) != (f_b >= iso), t = (iso - f_a) / (f_b - f_a), exactly the isosurface's operations (f =
 * (float) byte * kInv255); otherwise t = 0.5f.  Component c is (float) a_c + t where b differs from a, else (float) a_c.  iso is ignored
 * when d_volume is NULL.
 * Consequences.  Two bodies that touch share bit-equal vertices on their interface, and the triangles of each label are watertight under
 * exact comparison wherever the body does not touch a face of the box.  If label != 0 exactly where a voxel is inside, the outer surface has
 * the isosurface's own vertices.  For the labels of vkv_label_components(.., VKV_CONNECT_14) at `iso`, with d_volume and the same iso, the
 * triangle list equals vkv_isosurface_mesh's bit for bit, in the same order, with the same total (every tetrahedron edge is a 14-neighbour
 * pair, so the inside corners of a tetrahedron share one label): d_triangle_labels is then the split of that mesh by body.
 * d_counts[0] = the exact total, d_counts[1] = min(total, capacity_triangles).  Exactly the first d_counts[1] triangles and their labels are
 * written, and not one element beyond.  capacity_triangles == 0 is the counting call: d_triangles and d_triangle_labels may be NULL and no
 * emit is enqueued.  d_scratch: vkv_label_mesh_scratch_bytes(extent, box) bytes (at least 16, a multiple of 8; 0 for an extent or box the
 * call rejects), 8-byte aligned, contents undefined afterwards.
 * d_visibility_map (NULL: dense) is vkv_label_visibility_map of the same labels, box and table, with map_extent: a tile of cubes whose
 * cells all hold 0 is counted empty without reading a label, and gives the same bits (a cube whose origin lies in a cell has its eight
 * voxels in that cell grown by one).  With d_colors == NULL a map is rejected: no table it could have been built from means "all visible".
 * Kernels only (count, two scans, emit: no allocation, memset or copy node, no host wait, no atomics; the kernels use no scratch memory), so
 * after one direct call on `stream` it can be captured into a hipGraph; two runs give the same bytes; nothing in the context is written.
 * Every argument is checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_labels,
 * d_scratch or d_counts, a zero extent, an empty box or one not inside `extent`, a non-finite iso with a d_volume, a null d_colors with
 * table_entries != 0, a non-zero capacity with a null d_triangles or d_triangle_labels, a map with a null d_colors or without a valid
 * map_extent, a d_labels, d_colors, d_triangles or d_triangle_labels that is not 4-byte aligned, a d_scratch or d_counts that is not 8-byte
 * aligned.  VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels, or one too large for the launches.  Every extent is accepted, widths
 * below 4 and axes of length 1 included; d_volume may start at any byte; nothing outside any buffer is read or written.
 * Not here: the faces of the box stay open, as the isosurface mesh's do, so a body that touches a face is open there (clear the border
 * first, or pass labels with a box one voxel larger).  The indexed variant, with normals, is vkv_label_mesh_indexed below. */
size_t vkv_label_mesh_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_label_mesh(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors, uint64_t table_entries,
                   const uint8_t *d_volume, float iso, const uint8_t *d_visibility_map, VkvExtent3D map_extent, void *d_scratch,
                   float *d_triangles, uint32_t *d_triangle_labels, uint64_t capacity_triangles, uint64_t *d_counts, void *stream);

/* ---- label volumes as indexed meshes: shared vertices, normals, and what lies across ------------------------------------------
 * vkv_label_mesh_indexed: the surfaces of vkv_label_mesh as a vertex list and three vertex numbers per triangle.  Everything not restated
 * here is vkv_label_mesh's: the labels' shape (that of `box`) and the visible(L) rule, with d_colors == NULL && table_entries == 0 meaning
 * "every non-zero label is visible"; cubes, tetrahedra, groups per tetrahedron, case masks, winding and triangle order; the vertex rule (t from
 * the volume where it crosses iso between the edge's voxels, else 0.5f); that every argument is checked before anything is enqueued and a
 * rejected call writes nothing.  Write shown(L) = L if visible(L), else 0.
 * Vertex list.  An EDGE is a pair (voxel v, direction d = dx + 2 dy + 4 dz, 1 <= d <= 7; v + d means v + (dx, dy, dz)) with both v and v + d
 * inside the box, and every axis of the box at least 2 voxels long: vkv_isosurface_mesh_indexed's definition.  An edge is CROSSING iff
 * shown(label(v)) != shown(label(v + d)): two different hidden labels do not cross, and neither does a hidden label against 0.  The vertex
 * list is the crossing edges ordered by v (x fastest, then y, then z), then by d rising: one vertex per crossing edge.  Position: the vertex
 * rule with a = v, b = v + d, so positions are bit-equal to the triangle list's; 3 floats per vertex.  Every triangle vertex of
 * vkv_label_mesh lies on a crossing edge, and every crossing edge carries a vertex of at least one triangle (DESIGN.md §5.23 proves both),
 * so the list has no orphans.  Two bodies that meet on an edge share that one vertex.
 * Normals (d_normals may be NULL: none are computed; with d_normals, d_volume is required).  Exactly vkv_isosurface_mesh_indexed's: G_c(p)
 * = (int) vol[p + e_c] - (int) vol[p - e_c] from the VOLUME's bytes, both neighbours clamped to the volume; n_c = -((float) G_c(a) + t *
 * (float) (G_c(b) - G_c(a))) with the vertex's own t (0.5f where the volume does not cross): one multiplication, one addition, no FMA.  3
 * floats per vertex, not normalised.  What they are worth: on a body's outer surface, where the labels follow the volume, they are the
 * isosurface's smooth normal.  On an interface inside the material they follow the volume and not the bodies, and their sign there suits
 * neither body by construction: orient them per triangle (vkvolume_amd.mesh.oriented_corner_normals).
 * Vertex labels (d_vertex_labels may be NULL: none).  Two uint32 per vertex: shown(label(v)), then shown(label(v + d)).  They differ by
 * definition and at most one is 0.  A triangle tagged L has L in the pair of each of its three vertices; the other member is what lies
 * across the surface there, 0 meaning free surface.
 * Indices.  The triangles of vkv_label_mesh in its order, 3 x uint32 each (v0 v1 v2): the edge (a, b) of the cube with origin o is the edge
 * (o + a, a ^ b), and its index is that edge's position in the FULL vertex list, reduced mod 2^32; it depends on neither capacity.
 * d_triangle_labels is as in vkv_label_mesh, one uint32 per triangle.
 * d_counts holds four values: [0] = the total number of triangles, [1] = min([0], capacity_triangles), [2] = the total number of vertices,
 * [3] = min([2], capacity_vertices).  Exactly the first [1] triangles' indices and labels and the first [3] vertices (and their normals and
 * label pairs, if asked for) are written, and not one element beyond them.  A capacity of zero for either list (its pointers NULL or not)
 * enqueues no emit for that list; both zero is the counting call.  capacity_vertices may not exceed 0xffffffff, so a call with [2] == [3]
 * has exact indices; a larger surface is extracted box by box.  d_scratch: vkv_label_mesh_indexed_scratch_bytes(extent, box) bytes (at least
 * 16, a multiple of 8; 0 for an extent or box this call rejects; 16 bytes per 256 x-adjacent voxels of a row of the box and one byte per
 * voxel, rows rounded up to 4 voxels), 8-byte aligned; its contents mean nothing between calls.
 * d_visibility_map (NULL: dense) is vkv_label_visibility_map of the same labels, box and table, with map_extent: a tile of VOXELS whose
 * cells all hold 0 owns no vertex and starts no triangle, and gives the same bits (v + d lies in v's cell grown by one).  With d_colors ==
 * NULL a map is rejected.
 * Kernels only (no allocation, no memset or copy node, no host wait, no atomics; the kernels use no scratch memory): two runs give the same
 * bytes, and after one direct call on `stream` it can be captured into a hipGraph.  Nothing in the context is written.
 * VKV_E_INVALID_ARGUMENT: everything vkv_label_mesh rejects (a null ctx, d_labels, d_scratch or d_counts, a zero extent, an empty box or
 * one not inside `extent`, a non-finite iso with a d_volume, a null d_colors with table_entries != 0, a map with a null d_colors or without
 * a valid map_extent), capacity_vertices > 0xffffffff, a non-zero capacity_vertices with a NULL d_vertices, a non-zero capacity_triangles
 * with a NULL d_indices or d_triangle_labels, d_normals or d_vertex_labels with capacity_vertices == 0, d_normals without d_volume, a
 * d_labels, d_colors, d_vertices, d_normals, d_vertex_labels, d_indices or d_triangle_labels that is not 4-byte aligned, a d_scratch or
 * d_counts that is not 8-byte aligned.  VKV_E_UNSUPPORTED: a box of more than 2^32 - 1 voxels, or one too large for the launches.  Every
 * extent is accepted, widths below 4 and axes of length 1 included; d_volume may start at any byte; nothing outside any buffer is read or
 * written.
 * Not here: the box's faces stay open, the normals come from the volume and not from the labels, and nothing is decimated.  Smoothing, and
 * normals from the faces of one body, are vkv_mesh_smooth and vkv_mesh_vertex_normals below: they take this call's buffers and d_counts as
 * they are. */
size_t vkv_label_mesh_indexed_scratch_bytes(VkvExtent3D extent, const VkvBox *box);
int vkv_label_mesh_indexed(vkv_ctx *ctx, const uint32_t *d_labels, VkvExtent3D extent, const VkvBox *box, const uint32_t *d_colors, uint64_t table_entries,
                           const uint8_t *d_volume, float iso, const uint8_t *d_visibility_map, VkvExtent3D map_extent, void *d_scratch,
                           float *d_vertices, float *d_normals, uint32_t *d_vertex_labels, uint64_t capacity_vertices, uint32_t *d_indices,
                           uint32_t *d_triangle_labels, uint64_t capacity_triangles, uint64_t *d_counts, void *stream);

/* ---- indexed meshes after their extraction: adjacency, Taubin smoothing, normals from the faces --------------------------------
 * A MESH is d_vertices (3 floats per vertex), d_indices (3 uint32 per triangle) and the four-value d_counts that vkv_isosurface_mesh_indexed
 * and vkv_label_mesh_indexed write.  d_counts is read ON THE DEVICE: no call here waits for the host.  nt = min(d_counts[1],
 * capacity_triangles), nv = min(d_counts[3], capacity_vertices).  USED FACES: the first nt triangles whose three indices are all below nv; a
 * truncated extraction names vertices past its capacity, and those faces contribute nothing and are never dereferenced.
 * NEIGHBOUR SET.  N(v) = { u != v : some used face holds both u and v }.  A set: a neighbour reached through several faces counts once, the
 * interface faces that a label mesh emits twice with opposite winding included.  k(v) = |N(v)|.
 * Fixed point.  q(x) = (int64) rint((double) x * 2^24), rounding half to even.  Every sum below is a sum of such integers in int64, so the
 * order of summation cannot matter and the results are pinned to the bit; no floating-point atomic is used.
 * vkv_mesh_adjacency builds, once per mesh, what the other two calls gather through: per vertex its neighbour set and its used faces, both
 * rising.  It lives in d_adjacency, vkv_mesh_adjacency_scratch_bytes(capacity_vertices, capacity_triangles) bytes of caller memory, 8-byte
 * aligned: 32 + 8 * ceil(capacity_vertices / 4096) + 3 * roundup8(4 * capacity_vertices) + 24 * capacity_triangles + roundup8(12 *
 * capacity_triangles); 0 for a capacity above 0xffffffff.  Its layout is the library's (mesh_smooth.hip states it); it stays valid while
 * d_indices and d_counts stay as they were, for any positions.  Steps: count per vertex (integer atomics), the fixed-tree scan, fill (an integer
 * atomic cursor per vertex), then each vertex's segment sorted and made a set in place by one lane: the cost is quadratic in a vertex's number
 * of faces, which is at most 14 away from junctions in the extractors' meshes and is not bounded for a mesh from elsewhere.
 * vkv_mesh_smooth runs n_passes Jacobi passes of the uniform umbrella operator, pass i with the factor factors[i] (a HOST array, read during the
 * call; Taubin smoothing is lambda, mu, lambda, mu, ...).  Every vertex reads the previous pass's positions.  One pass with factor f, for each
 * component c of vertex v at p: S = the sum over u in N(v) of q(p_u,c) in int64; m = (float) ((double) S / (double) k * 2^-24); p' = p + f *
 * (m - p) as three separately rounded fp32 operations (subtract, multiply, add; no FMA).  A vertex with k = 0, or with d_pinned[v] != 0
 * (d_pinned: one byte per vertex, NULL: none), keeps its bits.  After the call the result is in d_vertices for every pass count, zero
 * included; d_swap (capacity_vertices x 3 floats, not d_vertices) holds nothing of meaning.  Rows past nv are written in neither buffer.
 * Bodies of a label mesh that share an interface vertex see it move once, so they stay closed against each other under exact comparison.
 * Positions with |x| > 2^20 or non-finite give unspecified values, but never an access outside a buffer.
 * vkv_mesh_vertex_normals: area-weighted vertex normals from the faces.  For a used face (i0, i1, i2) with positions p0, p1, p2: e1 = p1 - p0,
 * e2 = p2 - p0 in fp32, n = e1 x e2 with n_x = e1_y * e2_z - e1_z * e2_y, n_y = e1_z * e2_x - e1_x * e2_z, n_z = e1_x * e2_y - e1_y * e2_x,
 * each the two products in that order, each rounded, then one subtraction (no FMA).  N(v)_c = (float) ((double) (the sum of q(n_c)) * 2^-24)
 * over the used faces that hold v, or with d_triangle_labels (one uint32 per triangle; NULL: no filter, `label` is ignored) over those with
 * d_triangle_labels[face] == label.  A face that holds v more than once has n = 0 exactly, so how often it is counted cannot matter.
 * Not normalised; zero where nothing contributes.  Over all faces an interior interface vertex of a label mesh sums to exactly zero, since its
 * faces come in opposite pairs; per label it gets that body's outward normal, and the two bodies' normals there are exact negatives.  Rows
 * past nv are not written.  The sums are defined while they stay below 2^63: face normals up to 2^20 in every component at the least.
 * All three calls: kernels only (no allocation, no memset or copy node, no host wait; the kernels use no scratch memory), so after one direct
 * call on `stream` they can be captured into a hipGraph (the factors are then the capture's); two runs give the same bytes in every output and
 * in d_adjacency; nothing in the context is written.  Every kernel is launched for the capacities and takes its bounds from d_counts.  The
 * capacities, d_indices and d_counts given to vkv_mesh_smooth and vkv_mesh_vertex_normals are those of the vkv_mesh_adjacency call; other
 * values give unspecified results, but every index read from memory is compared with its bound before it is used.  Every argument is
 * checked before anything is enqueued, and a rejected call writes nothing.  VKV_E_INVALID_ARGUMENT: a null ctx, d_indices, d_counts,
 * d_adjacency, d_vertices, d_swap or d_normals where the call takes one; a d_vertices, d_swap, d_indices, d_triangle_labels or d_normals that
 * is not 4-byte aligned, a d_counts or d_adjacency that is not 8-byte aligned; d_swap or d_normals equal to d_vertices; n_passes != 0 with
 * NULL factors; a non-finite factor.  VKV_E_UNSUPPORTED: a capacity above 0xffffffff.
 * Not here: cotangent or feature-preserving weights, smoothing during extraction.  Decimation is vkv_mesh_decimate below. */
size_t vkv_mesh_adjacency_scratch_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles);
int vkv_mesh_adjacency(vkv_ctx *ctx, const uint32_t *d_indices, uint64_t capacity_triangles, uint64_t capacity_vertices, const uint64_t *d_counts,
                       void *d_adjacency, void *stream);
int vkv_mesh_smooth(vkv_ctx *ctx, float *d_vertices, float *d_swap, uint64_t capacity_vertices, const uint64_t *d_counts, const void *d_adjacency,
                    const uint8_t *d_pinned, const float *factors, uint32_t n_passes, void *stream);
int vkv_mesh_vertex_normals(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint32_t label,
                            uint64_t capacity_vertices, uint64_t capacity_triangles, const uint64_t *d_counts, const void *d_adjacency,
                            float *d_normals, void *stream);

/* ---- indexed meshes decimated by vertex clustering ------------------------------------------------------------------------
 * Rossignac-Borrel clustering on a regular grid: every vertex falls into a cell, a cell's vertices become one vertex at their mean, and a
 * triangle survives if and only if its three cells differ.  The answer is unique and the same bytes come back twice.
 * Input: a MESH as above (d_vertices, d_indices, the four d_counts read ON THE DEVICE, the two capacities; nt, nv and USED FACES as above; a
 * truncated extraction is a valid input), and optionally d_triangle_labels (one uint32 per triangle; NULL: none).
 * Grid: grid_origin and grid_cell are 3 HOST floats each, read during the call; grid_extent holds the cell counts n_x, n_y, n_z.
 * Cell of a vertex at p, per axis a, in fp32: u = (p_a - origin_a) / cell_a, one subtraction and one correctly rounded division; c_a = u >= 0 ?
 * (u < (float) n_a ? (uint32) u : n_a - 1) : 0.  Positions outside the grid fall into its border cells, NaN falls to 0 by that comparison, and
 * nothing indexes out of range.  Cell id = c_x + n_x (c_y + n_y c_z).
 * Output faces: the used faces whose three cells are pairwise distinct, in input order, 3 x uint32 each: the new numbers of the three cells.
 * d_out_triangle_labels receives their labels in parallel when d_triangle_labels is given (else it is not touched).  Faces that become
 * duplicates of one another are kept: the interface faces of a label mesh come in opposite pairs and stay so.
 * Output vertices: one per cell that at least one surviving face names, in rising cell id; no output vertex is an orphan.  A cell's new number
 * is its position in that FULL list, reduced mod 2^32 in the faces; it depends on neither output capacity.  Position, per component:
 * (float) ((double) S / (double) k * 2^-24), where S is the int64 sum of q(p) (q as above: rint(x * 2^24)) over ALL of the first nv input
 * vertices in the cell, used by a face or not, and k is their number.  The sums are integer atomics, no floating-point atomic is used; they
 * are defined while they stay below 2^63: positions up to 2^20 in magnitude with up to 2^18 vertices in one cell at the least.  Non-finite
 * positions give unspecified values in their cell, but never an access outside a buffer.
 * Closedness.  If over the used input faces every directed edge a -> b occurs as often as b -> a, the same holds for the output faces: bodies
 * of a label mesh stay closed, also against each other, since the vertex they share is one vertex afterwards.
 * d_vertex_map (NULL: none): one uint32 per input vertex v < nv, the new number of v's cell, or 0xffffffff where no surviving face names that
 * cell; rows past nv are not written.  It carries per-vertex attributes such as label pairs over.
 * d_out_counts: [0] = the surviving faces, [1] = min([0], out_capacity_triangles), [2] = the output vertices, [3] = min([2],
 * out_capacity_vertices): the output is again a MESH for the calls above and for another vkv_mesh_decimate.  Exactly the first [1] faces (and
 * labels) and the first [3] vertices are written, and not one element beyond them.  A capacity of zero for either list enqueues no emit for that
 * list; both zero is the counting call.
 * d_scratch: vkv_mesh_decimate_scratch_bytes(capacity_vertices, capacity_triangles, grid_extent) bytes of caller memory, 8-byte aligned: with C
 * = n_x n_y n_z cells and B = ceil(capacity_triangles / 256), 32 * C + 8 * ceil(C / 4096) + 8 * B + 8 * ceil(B / 4096) + roundup8(4 *
 * capacity_vertices); 0 for what the call rejects.  Per cell three int64 sums, a count and a mark that becomes the number; per input vertex
 * its cell; the scan blocks.  Its contents mean nothing between calls.
 * Kernels only (a clear kernel; no allocation, no memset or copy node, no host wait; the kernels use no scratch memory): after one direct call
 * on `stream` it can be captured into a hipGraph (the grid is then the capture's).  Two runs give the same bytes in every output.  Nothing in
 * the context is written.  Every argument is checked before anything is enqueued, and a rejected call writes nothing.
 * VKV_E_INVALID_ARGUMENT: a null ctx, d_vertices, d_indices, d_counts, grid_origin, grid_cell, d_scratch or d_out_counts; a d_vertices,
 * d_indices, d_triangle_labels, d_out_vertices, d_out_indices, d_out_triangle_labels or d_vertex_map that is not 4-byte aligned, a d_counts,
 * d_scratch or d_out_counts that is not 8-byte aligned; a zero grid axis; a cell size that is not finite and positive; a non-finite origin;
 * an output (d_out_vertices, d_out_indices, d_out_triangle_labels, d_vertex_map, d_out_counts) equal to an input (d_vertices, d_indices,
 * d_triangle_labels, d_counts), to d_scratch or to another output; a non-zero
 * out_capacity_vertices with a NULL d_out_vertices, a non-zero out_capacity_triangles with a NULL d_out_indices or, with labels, a NULL
 * d_out_triangle_labels.  VKV_E_UNSUPPORTED: one of the four capacities above 0xffffffff; more than 0xffffffff cells.
 * Not here: quadric error metrics, edge collapse, removal of duplicate faces on the device (vkvolume_amd.mesh.drop_duplicate_faces does it
 * on the host), feature preservation. */
size_t vkv_mesh_decimate_scratch_bytes(uint64_t capacity_vertices, uint64_t capacity_triangles, VkvExtent3D grid_extent);
int vkv_mesh_decimate(vkv_ctx *ctx, const float *d_vertices, const uint32_t *d_indices, const uint32_t *d_triangle_labels, uint64_t capacity_vertices,
                      uint64_t capacity_triangles, const uint64_t *d_counts, const float *grid_origin, const float *grid_cell, VkvExtent3D grid_extent,
                      void *d_scratch, float *d_out_vertices, uint64_t out_capacity_vertices, uint32_t *d_out_indices, uint32_t *d_out_triangle_labels,
                      uint64_t out_capacity_triangles, uint32_t *d_vertex_map, uint64_t *d_out_counts, void *stream);

/* Deterministic synthetic uint8 volume, generated on the device. kind 0 = soft
 * sphere (config C1), kind 1 = ellipsoid shells + hash noise (configs C2..C5).  The shells take three knobs in the upper bits of `kind`
 * (kind = 1 | shells << 8 | thickness << 16 | noise << 28): only the first `shells` (1 .. 39; 0 = all 40) of the seed's shells, their
 * thickness scaled by thickness / 256 (12 bits; 0 = 1.0), the hash noise 0 .. noise (4 bits; 0 = the default 0 .. 20) -
 * tools/benchmark_sweep.py tunes the occupied-voxel share of its scenes to the reference's datasets with them. */
int vkv_synth_volume(vkv_ctx *ctx, uint8_t *d_volume, VkvExtent3D extent, uint32_t kind, uint32_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VKVOLUME_AMD_H */

"""ctypes mirror of ``include/vkvolume_amd.h`` (struct layouts and enums only; loads no library).

Each class cites the header struct it mirrors; the header cites the reference file:line.
"""
import ctypes as C

VKV_OK = 0
VKV_E_INVALID_ARGUMENT = -1
VKV_E_UNSUPPORTED = -2
VKV_E_NO_DEVICE = -3
VKV_E_IO = -4
TF_BITS_WORDS = 2564  # VKV_TF_BITS_WORDS
MAX_BATCH = 32  # VKV_MAX_BATCH

# VolumeRenderSubpass::SkippingType / Test (src/volume_render_subpass.h:58-72)
SKIP_NONE, SKIP_BLOCK, SKIP_DISTANCE, SKIP_ANISOTROPIC_DISTANCE = 0, 1, 2, 3
VOXEL_TYPES = {"uint8_t": 0, "int8_t": 1, "uint16_t": 2, "int16_t": 3}  # VkvVoxelType by LoadVolume::Header::type
TEST_NONE, TEST_RAY_ENTRY, TEST_RAY_EXIT, TEST_NUM_TEXTURE_SAMPLES = 0, 1, 2, 3
HISTOGRAM_BINS = 65536  # VKV_HISTOGRAM_BINS: bin g * 256 + i = voxels with gradient byte g and intensity byte i
HISTOGRAM_SET, HISTOGRAM_ADD, HISTOGRAM_SUBTRACT = 0, 1, 2  # VkvHistogramMode
CELL_SUMMARY_BYTES = 16  # VKV_CELL_SUMMARY_BYTES: one occupancy cell's summary (vkv_cell_summary)


class Extent3D(C.Structure):
    """VkvExtent3D"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32)]

    def __init__(self, width=0, height=0, depth=0):
        super().__init__(int(width), int(height), int(depth))

    def as_tuple(self):
        return (self.width, self.height, self.depth)

    @property
    def count(self):
        return self.width * self.height * self.depth


class Box(C.Structure):
    """VkvBox: voxels [x0, x0 + width) x [y0, y0 + height) x [z0, z0 + depth)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("z0", C.c_uint32),
                ("width", C.c_uint32), ("height", C.c_uint32), ("depth", C.c_uint32)]

    def __init__(self, x0=0, y0=0, z0=0, width=0, height=0, depth=0):
        super().__init__(int(x0), int(y0), int(z0), int(width), int(height), int(depth))


class TransferFunctionUniform(C.Structure):
    """VkvTransferFunctionUniform (src/transfer_function.h:20-32)"""
    _fields_ = [("sampling_factor", C.c_float), ("voxel_alpha_factor", C.c_float),
                ("grad_magnitude_modifier", C.c_float), ("use_gradient", C.c_uint32),
                ("intensity_min", C.c_float), ("intensity_range_inv", C.c_float),
                ("gradient_min", C.c_float), ("gradient_range_inv", C.c_float)]


class VolumeOptions(C.Structure):
    """VkvVolumeOptions (Volume::Options, src/volume_component.h:45-56)"""
    _fields_ = [("sampling_factor", C.c_float), ("voxel_alpha_factor", C.c_float),
                ("use_precomputed_gradient", C.c_uint32), ("intensity_min", C.c_float),
                ("intensity_max", C.c_float), ("gradient_min", C.c_float), ("gradient_max", C.c_float)]

    def __init__(self, sampling_factor=1.0, voxel_alpha_factor=1.0, use_precomputed_gradient=True,
                 intensity_min=0.0, intensity_max=1.0, gradient_min=0.0, gradient_max=1.0):
        super().__init__(sampling_factor, voxel_alpha_factor, 1 if use_precomputed_gradient else 0,
                         intensity_min, intensity_max, gradient_min, gradient_max)


class CameraUniform(C.Structure):
    """VkvCameraUniform (src/volume_render_subpass.h:32-39)"""
    _fields_ = [("camera_view", C.c_float * 16), ("camera_proj", C.c_float * 16),
                ("camera_view_proj_inv", C.c_float * 16), ("model", C.c_float * 16),
                ("model_inv", C.c_float * 16)]


class RayCastUniform(C.Structure):
    """VkvRayCastUniform (src/volume_render_subpass.h:46-53)"""
    _fields_ = [("plane", C.c_float * 4), ("plane_tex", C.c_float * 4), ("camera_pos_tex", C.c_float * 4),
                ("block_size", C.c_float * 4), ("front_index", C.c_int32)]


class RayGen(C.Structure):
    """VkvRayGen"""
    _fields_ = [("dir00", C.c_float * 4), ("ddx", C.c_float * 4), ("ddy", C.c_float * 4)]


class RenderOptions(C.Structure):
    """VkvRenderOptions (VolumeRenderSubpass::Options, src/volume_render_subpass.h:74-81)"""
    _fields_ = [("skipping_type", C.c_int32), ("clip_distance", C.c_float), ("early_ray_termination", C.c_int32),
                ("depth_attachment", C.c_int32), ("test", C.c_int32)]

    def __init__(self, skipping_type=SKIP_DISTANCE, clip_distance=50.0, early_ray_termination=True,
                 depth_attachment=False, test=TEST_NONE):
        super().__init__(skipping_type, clip_distance, 1 if early_ray_termination else 0,
                         1 if depth_attachment else 0, test)


class TileRect(C.Structure):
    """VkvTileRect: x0, y0 = first tile column / row, w x h tiles (all zero: the whole image)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]

    def as_tuple(self):
        return (self.x0, self.y0, self.w, self.h)

    @property
    def tiles(self):
        return self.w * self.h


class TileSchedule(C.Structure):
    """VkvTileSchedule"""
    _fields_ = [("tile_width", C.c_uint32), ("tile_height", C.c_uint32), ("tile_first", C.c_uint32),
                ("tile_stride", C.c_uint32), ("tile_count", C.c_uint32), ("compact", C.c_uint32), ("rect", TileRect),
                ("fill_outside", C.c_uint32)]


class RenderParams(C.Structure):
    """VkvRenderParams"""
    _fields_ = [("camera", CameraUniform), ("ray_cast", RayCastUniform),
                ("transfer_function", TransferFunctionUniform), ("ray_gen", RayGen), ("options", RenderOptions),
                ("use_precomputed_gradient", C.c_uint32), ("image_width", C.c_uint32), ("image_height", C.c_uint32),
                ("tiles", TileSchedule), ("volume_extent", Extent3D), ("map_extent", Extent3D),
                ("d_volume", C.c_void_p), ("d_gradient", C.c_void_p), ("d_transfer_function", C.c_void_p),
                ("d_distance_maps", C.c_void_p * 8), ("d_packed_volume", C.c_void_p),
                ("d_transfer_function_bits", C.c_void_p), ("d_out_color", C.c_void_p), ("d_out_rgba8", C.c_void_p),
                ("d_out_counts", C.c_void_p), ("d_out_depth", C.c_void_p), ("d_in_depth", C.c_void_p),
                ("blend_over_target", C.c_uint32)]



class MipOptions(C.Structure):
    """VkvMipOptions (vkv_render_mip): threshold, grey window, optional max map (vkv_max_map), optional intensity output, flags (0)"""
    _fields_ = [("threshold", C.c_float), ("window_max", C.c_float), ("d_max_map", C.c_void_p), ("d_out_intensity", C.c_void_p),
                ("flags", C.c_uint32)]


class IsoOptions(C.Structure):
    """VkvIsoOptions (vkv_render_isosurface): iso value, bisection steps, headlight shading (base colour, ambient, diffuse, specular,
    shininess), optional max map (vkv_max_map), optional normal output, flags (0)"""
    _fields_ = [("iso", C.c_float), ("refine_steps", C.c_uint32), ("base_color", C.c_float * 3), ("ambient", C.c_float), ("diffuse", C.c_float),
                ("specular", C.c_float), ("shininess", C.c_uint32), ("d_max_map", C.c_void_p), ("d_out_normal", C.c_void_p), ("flags", C.c_uint32)]


class LabelRenderOptions(C.Structure):
    """VkvLabelRenderOptions (vkv_render_labels): the labels (uint32, the shape of ``box``; a NULL box: of the volume), the colour table
    (entry L - 1: R | G << 8 | B << 16 | A << 24, alpha 0 hides the label), bisection steps, shade (0: the table's colour; 1: the
    isosurface's headlight with ambient, diffuse, specular, shininess), optional visibility map (vkv_label_visibility_map), optional label
    and normal outputs, flags (0).  ``box`` is a host pointer: assign ctypes.pointer(an abi.Box), which the structure keeps alive."""
    _fields_ = [("d_labels", C.c_void_p), ("box", C.POINTER(Box)), ("d_colors", C.c_void_p), ("table_entries", C.c_uint64),
                ("refine_steps", C.c_uint32), ("shade", C.c_uint32), ("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float),
                ("shininess", C.c_uint32), ("d_visibility_map", C.c_void_p), ("d_out_label", C.c_void_p), ("d_out_normal", C.c_void_p),
                ("flags", C.c_uint32)]


SLAB_MAX, SLAB_MIN, SLAB_MEAN = 0, 1, 2  # VkvSlabMode
FILTER_BINOMIAL3, FILTER_MEDIAN3 = 0, 1  # VkvFilterKind
CONNECT_6, CONNECT_14, CONNECT_26 = 6, 14, 26  # VKV_CONNECT_*: the neighbourhoods of vkv_label_components
DISTANCE_TO_INSIDE, DISTANCE_TO_OUTSIDE = 0, 1  # VkvDistanceTarget: the target voxels of vkv_distance_transform
DISTANCE_NONE = 0xffffffff  # VKV_DISTANCE_NONE: no limit
NEAREST_NONE = 0xffffffff  # VKV_NEAREST_NONE: vkv_nearest_target found no target (within the limit)
GEODESIC_NONE = 0xffffffff  # VKV_GEODESIC_NONE: vkv_geodesic_propagate did not reach the voxel; as a limit: unlimited
GEODESIC_MAX_ROUNDS = 1024  # VKV_GEODESIC_MAX_ROUNDS: the rounds of one vkv_geodesic_propagate call


class ComponentStats(C.Structure):
    """VkvComponentStats (vkv_component_stats): one label's bounding box (volume coordinates, inclusive), smallest and largest byte, voxel
    count, coordinate sums, sum of bytes and of squared bytes; 80 bytes"""
    _fields_ = [("min_x", C.c_uint32), ("min_y", C.c_uint32), ("min_z", C.c_uint32), ("max_x", C.c_uint32), ("max_y", C.c_uint32),
                ("max_z", C.c_uint32), ("min_value", C.c_uint32), ("max_value", C.c_uint32), ("voxels", C.c_uint64), ("sum_x", C.c_uint64),
                ("sum_y", C.c_uint64), ("sum_z", C.c_uint64), ("sum_value", C.c_uint64), ("sum_value2", C.c_uint64)]


COMPONENT_STATS_BYTES = 80  # sizeof(VkvComponentStats)
# the same 80 bytes as a numpy structured dtype (numpy itself is imported where it is used: this module loads nothing)
COMPONENT_STATS_FIELDS = [(name, "<u4" if ctype is C.c_uint32 else "<u8") for name, ctype in ComponentStats._fields_]


def component_stats_dtype():
    """numpy's structured dtype of VkvComponentStats: the fields of ComponentStats at the C offsets, itemsize 80"""
    import numpy as np
    return np.dtype(COMPONENT_STATS_FIELDS, align=True)


class SlabOptions(C.Structure):
    """VkvSlabOptions (vkv_render_slab): the plane (origin, du, dv) and the slab's sample step dn in texture space, samples per pixel, mode
    (SLAB_MAX / SLAB_MIN / SLAB_MEAN), grey window, optional max map (SLAB_MAX only), optional value output, flags (0)"""
    _fields_ = [("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("dn", C.c_float * 3), ("samples", C.c_uint32),
                ("mode", C.c_int32), ("window_min", C.c_float), ("window_max", C.c_float), ("d_max_map", C.c_void_p), ("d_out_value", C.c_void_p),
                ("flags", C.c_uint32)]


class Tuning(C.Structure):
    """VkvTuning"""
    _fields_ = [("struct_size", C.c_uint32), ("scheduler", C.c_int32), ("batch_mode", C.c_int32), ("batch_sequential", C.c_int32),
                ("tile_order_linear", C.c_int32), ("address_tables", C.c_int32), ("full_table_lds_limit", C.c_uint32),
                ("screen_cull", C.c_int32), ("feedback", C.c_int32), ("feedback_period", C.c_uint32), ("clamp_always", C.c_int32),
                ("tile_mix_heavy", C.c_float), ("tile_mix_spread", C.c_float), ("gradient_segment", C.c_uint32),
                ("wave_shape", C.c_int32), ("arena_bytes", C.c_uint32)]


class VolumeHeader(C.Structure):
    """VkvVolumeHeader (LoadVolume::Header, src/load_volume.h:29-39)"""
    _fields_ = [("extent", Extent3D), ("voxel_size", C.c_float * 3), ("normalisation_range", C.c_float * 2),
                ("type", C.c_char * 16), ("endianness", C.c_char * 16), ("image_transform", C.c_float * 16)]


def full_frame_tiles(image_width, image_height, tile_width=16, tile_height=16, rank=0, world=1, compact=False, rect=None, fill_outside=False):
    """Tile schedule of one rank: every ``world``-th tile starting at ``rank`` (interleaved screen tiles) of the whole image or, with
    ``rect`` (a TileRect, e.g. from lib.screen_tile_rect), of that tile rectangle.  ``fill_outside`` (one rank, image-indexed outputs): the
    launch also writes the no-fragment result outside the rectangle - the whole frame without a workgroup per empty tile."""
    if rect is not None and rect.w and rect.h:
        total, r = rect.w * rect.h, TileRect(rect.x0, rect.y0, rect.w, rect.h)
    else:
        tiles_x = (image_width + tile_width - 1) // tile_width
        tiles_y = (image_height + tile_height - 1) // tile_height
        total, r = tiles_x * tiles_y, TileRect(0, 0, 0, 0)
    count = (total - rank + world - 1) // world if total > rank else 0
    return TileSchedule(tile_width, tile_height, rank, world, count, 1 if compact else 0, r, 1 if (fill_outside and r.w and not compact and world == 1) else 0)


def whole_image_rect(image_width, image_height, tile_width=16, tile_height=16):
    return TileRect(0, 0, (image_width + tile_width - 1) // tile_width, (image_height + tile_height - 1) // tile_height)

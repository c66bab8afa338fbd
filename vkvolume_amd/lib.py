"""ctypes binding of ``csrc/libvkvolume_amd.so`` (the C ABI of ``include/vkvolume_amd.h``).

There is no fallback: if the shared library is missing or a call fails, a ``VkvError`` is raised.
"""
import ctypes as C
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VKV_LIB_PATH") or os.path.join(_HERE, "csrc", "libvkvolume_amd.so")  # override: kernel experiments only

# every symbol include/vkvolume_amd.h declares
EXPORTS = [
    "vkv_create", "vkv_destroy", "vkv_last_error", "vkv_version",
    "vkv_transfer_function_uniform", "vkv_transfer_function_texture", "vkv_build_uniforms",
    "vkv_gradient_map", "vkv_occupancy_map", "vkv_distance_map", "vkv_distance_map_anisotropic",
    "vkv_compute_distance_map", "vkv_render", "vkv_render_batch", "vkv_scatter_tiles", "vkv_synth_volume",
    "vkv_packed_volume_bytes", "vkv_pack_volume", "vkv_transfer_function_bits", "vkv_transfer_function_tables",
    "vkv_occupied_voxel_count", "vkv_load_header", "vkv_load_data", "vkv_convert_volume", "vkv_gather_tiles", "vkv_assemble_frame",
    "vkv_assemble_frames", "vkv_get_tuning", "vkv_set_tuning", "vkv_prepare_render", "vkv_register_target", "vkv_forget_target",
    "vkv_release_stream", "vkv_trim", "vkv_release_captured", "vkv_screen_tile_rect",
    "vkv_transfer_function_texture_device", "vkv_update_transfer_function", "vkv_update_volume_region",
    "vkv_volume_histogram", "vkv_histogram_occupied_count",
    "vkv_cell_summary", "vkv_occupancy_map_from_summary", "vkv_update_transfer_function_from_summary",
    "vkv_max_map", "vkv_render_mip", "vkv_render_isosurface", "vkv_render_slab", "vkv_filter_volume",
    "vkv_isosurface_mesh_scratch_bytes", "vkv_isosurface_mesh",
    "vkv_isosurface_mesh_indexed_scratch_bytes", "vkv_isosurface_mesh_indexed",
    "vkv_label_components_scratch_bytes", "vkv_label_components", "vkv_select_components",
    "vkv_component_stats", "vkv_select_components_by_table",
    "vkv_distance_transform_scratch_bytes", "vkv_distance_transform", "vkv_select_by_distance",
]
# include/vkvolume_amd_debug.h (diagnostics: tools/ and the exhaustive numerics tests)
DEBUG_EXPORTS = ["vkv_debug_trace", "vkv_debug_tile_orders", "vkv_debug_check", "vkv_debug_tf_scratch"]


class VkvError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("vkvolume_amd error %d: %s" % (code, message))
        self.code = code


_LIB = None


def _maps_array(d_maps):
    """the d_maps[8] argument of the C ABI: the given map pointers padded with NULL; None passes a NULL array"""
    return None if d_maps is None else (C.c_void_p * 8)(*(list(d_maps) + [None] * (8 - len(d_maps))))


def load():
    """Load the HIP library (once).  Raises VkvError if it has not been built — there is no CPU path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise VkvError(abi.VKV_E_NO_DEVICE, "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                            "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # torch bundles its own HIP runtime (same soname as /opt/rocm's).  It must be the one already mapped when this
    # library is dlopen()ed, so that streams and device pointers handed over from torch belong to the same runtime.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    P = C.POINTER
    L.vkv_create.argtypes = [C.c_int, P(vp)]
    L.vkv_destroy.argtypes = [vp]
    L.vkv_destroy.restype = None
    L.vkv_last_error.argtypes = [vp]
    L.vkv_last_error.restype = C.c_char_p
    L.vkv_version.restype = C.c_char_p
    L.vkv_transfer_function_uniform.argtypes = [P(abi.VolumeOptions), P(abi.TransferFunctionUniform)]
    L.vkv_transfer_function_texture.argtypes = [P(abi.VolumeOptions), vp]
    L.vkv_build_uniforms.argtypes = [vp, vp, vp, vp, C.c_float, u32, u32, abi.Extent3D, abi.Extent3D,
                                     P(abi.CameraUniform), P(abi.RayCastUniform), P(abi.RayGen)]
    L.vkv_gradient_map.argtypes = [vp, vp, vp, abi.Extent3D, P(abi.TransferFunctionUniform), vp]
    L.vkv_occupancy_map.argtypes = [vp, vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, vp, abi.Extent3D, vp]
    L.vkv_distance_map.argtypes = [vp, vp, vp, abi.Extent3D, vp]
    L.vkv_distance_map_anisotropic.argtypes = [vp, P(vp), vp, abi.Extent3D, vp]
    L.vkv_compute_distance_map.argtypes = [vp, vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, P(vp), vp,
                                           abi.Extent3D, i32, vp]
    L.vkv_render.argtypes = [vp, P(abi.RenderParams), vp]
    L.vkv_render_batch.argtypes = [vp, P(abi.RenderParams), C.c_uint32, vp]
    L.vkv_gather_tiles.argtypes = [vp, vp, vp, C.c_size_t, i32, vp, vp]
    L.vkv_assemble_frame.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, P(abi.TileRect), u32, u32, u32, i32, vp, vp]
    L.vkv_scatter_tiles.argtypes = [vp, vp, vp, u32, u32, u32, u32, P(abi.TileRect), u32, u32, u32, vp]
    L.vkv_assemble_frames.argtypes = [vp, vp, vp, P(vp), u32, u32, u32, u32, u32, P(abi.TileRect), u32, u32, u32, i32, P(i32), vp, vp]
    L.vkv_screen_tile_rect.argtypes = [P(abi.RayCastUniform), P(abi.RayGen), u32, u32, u32, u32, u32, P(abi.TileRect)]
    L.vkv_get_tuning.argtypes = [vp, P(abi.Tuning)]
    L.vkv_set_tuning.argtypes = [vp, P(abi.Tuning)]
    L.vkv_prepare_render.argtypes = [vp, P(abi.RenderParams), u32, vp]
    L.vkv_register_target.argtypes = [vp, vp, u32, u32, P(abi.TileSchedule)]
    L.vkv_forget_target.argtypes = [vp, vp]
    L.vkv_release_stream.argtypes = [vp, vp]
    L.vkv_trim.argtypes = [vp]
    L.vkv_release_captured.argtypes = [vp, vp]
    L.vkv_debug_trace.argtypes = [vp, vp]
    L.vkv_debug_tile_orders.argtypes = [vp, vp, u32, u32]
    L.vkv_debug_check.argtypes = [vp, i32, u32, C.c_uint64, vp, vp]
    L.vkv_synth_volume.argtypes = [vp, vp, abi.Extent3D, u32, u32, vp]
    L.vkv_packed_volume_bytes.argtypes = [abi.Extent3D]
    L.vkv_packed_volume_bytes.restype = C.c_size_t
    L.vkv_pack_volume.argtypes = [vp, vp, vp, abi.Extent3D, vp, vp]
    L.vkv_transfer_function_bits.argtypes = [vp, vp, vp, vp]
    L.vkv_transfer_function_tables.argtypes = [vp, vp, P(abi.TransferFunctionUniform), vp, vp]
    L.vkv_occupied_voxel_count.argtypes = [vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, vp, vp]
    L.vkv_transfer_function_texture_device.argtypes = [vp, P(abi.VolumeOptions), vp, vp, vp]
    L.vkv_update_transfer_function.argtypes = [vp, P(abi.VolumeOptions), vp, vp, abi.Extent3D, vp, vp, P(vp), vp, abi.Extent3D, i32, vp, vp]
    L.vkv_update_volume_region.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float, P(abi.Box), vp, vp, vp, abi.Extent3D, vp,
                                           P(abi.TransferFunctionUniform), P(vp), vp, abi.Extent3D, i32, vp]
    L.vkv_volume_histogram.argtypes = [vp, vp, vp, abi.Extent3D, P(abi.Box), i32, vp, vp]
    L.vkv_histogram_occupied_count.argtypes = [vp, vp, P(abi.TransferFunctionUniform), vp, vp]
    L.vkv_cell_summary.argtypes = [vp, vp, vp, abi.Extent3D, abi.Extent3D, P(abi.Box), vp, vp]
    L.vkv_occupancy_map_from_summary.argtypes = [vp, vp, vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, vp, abi.Extent3D, vp, vp]
    L.vkv_update_transfer_function_from_summary.argtypes = [vp, P(abi.VolumeOptions), vp, vp, abi.Extent3D, vp, vp, P(vp), vp, abi.Extent3D, i32, vp,
                                                            vp, vp, vp, vp]
    L.vkv_max_map.argtypes = [vp, vp, abi.Extent3D, abi.Extent3D, P(abi.Box), vp, vp]
    L.vkv_render_mip.argtypes = [vp, P(abi.RenderParams), P(abi.MipOptions), vp]
    L.vkv_render_isosurface.argtypes = [vp, P(abi.RenderParams), P(abi.IsoOptions), vp]
    L.vkv_render_slab.argtypes = [vp, P(abi.RenderParams), P(abi.SlabOptions), vp]
    L.vkv_filter_volume.argtypes = [vp, vp, vp, abi.Extent3D, P(abi.Box), i32, vp]
    L.vkv_isosurface_mesh_scratch_bytes.argtypes = [abi.Extent3D, P(abi.Box)]
    L.vkv_isosurface_mesh_scratch_bytes.restype = C.c_size_t
    L.vkv_isosurface_mesh.argtypes = [vp, vp, abi.Extent3D, P(abi.Box), C.c_float, vp, abi.Extent3D, vp, vp, C.c_uint64, vp, vp]
    L.vkv_isosurface_mesh_indexed_scratch_bytes.argtypes = [abi.Extent3D, P(abi.Box)]
    L.vkv_isosurface_mesh_indexed_scratch_bytes.restype = C.c_size_t
    L.vkv_isosurface_mesh_indexed.argtypes = [vp, vp, abi.Extent3D, P(abi.Box), C.c_float, vp, abi.Extent3D, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp]
    L.vkv_label_components_scratch_bytes.argtypes = [abi.Extent3D, P(abi.Box)]
    L.vkv_label_components_scratch_bytes.restype = C.c_size_t
    L.vkv_label_components.argtypes = [vp, vp, abi.Extent3D, P(abi.Box), C.c_float, i32, vp, abi.Extent3D, vp, vp, vp, C.c_uint64, vp, vp]
    L.vkv_select_components.argtypes = [vp, vp, vp, abi.Extent3D, P(abi.Box), vp, vp, vp, C.c_uint64, C.c_uint64, u32, vp]
    L.vkv_component_stats.argtypes = [vp, vp, abi.Extent3D, P(abi.Box), vp, vp, vp, C.c_uint64, vp]
    L.vkv_select_components_by_table.argtypes = [vp, vp, vp, abi.Extent3D, P(abi.Box), vp, vp, C.c_uint64, u32, vp]
    L.vkv_distance_transform_scratch_bytes.argtypes = [abi.Extent3D, P(abi.Box)]
    L.vkv_distance_transform_scratch_bytes.restype = C.c_size_t
    L.vkv_distance_transform.argtypes = [vp, vp, abi.Extent3D, P(abi.Box), C.c_float, i32, u32, vp, vp, vp]
    L.vkv_select_by_distance.argtypes = [vp, vp, vp, abi.Extent3D, P(abi.Box), vp, u32, u32, u32, vp]
    L.vkv_debug_tf_scratch.argtypes = [vp, vp, vp]
    L.vkv_convert_volume.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float, C.c_uint64, vp, vp]
    L.vkv_load_header.argtypes = [C.c_char_p, P(abi.VolumeHeader)]
    L.vkv_load_data.argtypes = [C.c_char_p, P(abi.VolumeHeader), vp, C.c_size_t]
    for name in EXPORTS + DEBUG_EXPORTS:
        getattr(L, name)  # AttributeError here means the library does not export what the headers declare
    _LIB = L
    return L


class Context:
    """RAII wrapper of ``vkv_ctx`` for one device."""

    def __init__(self, device=0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.vkv_create(int(device), C.byref(h))
        if rc != 0:
            raise VkvError(rc, "vkv_create(device=%d) failed (no gfx950 device?)" % device)
        self.handle = h
        self.device = device

    def close(self):
        if getattr(self, "handle", None):
            self._lib.vkv_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != 0:
            raise VkvError(rc, self._lib.vkv_last_error(self.handle).decode(errors="replace"))

    # ---- device entry points (pointers are ints / None; stream is a hipStream_t handle as int) ----
    def gradient_map(self, d_volume, d_gradient, extent, tf, stream=0):
        self.check(self._lib.vkv_gradient_map(self.handle, d_volume, d_gradient, extent, C.byref(tf), stream))

    def occupancy_map(self, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, stream=0):
        self.check(self._lib.vkv_occupancy_map(self.handle, d_volume, d_gradient, d_tf, C.byref(tf), extent, d_map,
                                               map_extent, stream))

    def distance_map(self, d_map, d_swap, map_extent, stream=0):
        self.check(self._lib.vkv_distance_map(self.handle, d_map, d_swap, map_extent, stream))

    def distance_map_anisotropic(self, d_maps, d_swap, map_extent, stream=0):
        self.check(self._lib.vkv_distance_map_anisotropic(self.handle, _maps_array(d_maps), d_swap, map_extent, stream))

    def compute_distance_map(self, d_volume, d_gradient, d_tf, tf, extent, d_maps, d_swap, map_extent, skipping_type, stream=0):
        self.check(self._lib.vkv_compute_distance_map(self.handle, d_volume, d_gradient, d_tf, C.byref(tf), extent, _maps_array(d_maps),
                                                      d_swap, map_extent, skipping_type, stream))

    def render(self, params, stream=0):
        self.check(self._lib.vkv_render(self.handle, C.byref(params), stream))

    def render_batch(self, params_list, stream=0):
        """vkv_render_batch: several frames (same kernel variant, same tile-schedule size) in one launch."""
        arr = (abi.RenderParams * len(params_list))(*params_list)
        self.check(self._lib.vkv_render_batch(self.handle, arr, len(params_list), stream))

    def gather_tiles(self, d_tiles, d_gathered, bytes_per_rank, root, nccl_comm, stream=0):
        self.check(self._lib.vkv_gather_tiles(self.handle, d_tiles, d_gathered, bytes_per_rank, root, nccl_comm, stream))

    def assemble_frame(self, d_tiles, d_gathered, d_image, image_size, tile_size, n_ranks, rank, bytes_per_pixel, root, nccl_comm, stream=0, rect=None):
        """vkv_assemble_frame: ncclGather of the compact tile buffers (the tiles of `rect`, a TileRect; None = the whole image) to `root` +
        de-interleave there, on `stream`."""
        self.check(self._lib.vkv_assemble_frame(self.handle, d_tiles, d_gathered, d_image, image_size[0], image_size[1], tile_size[0], tile_size[1],
                                                None if rect is None else C.byref(rect), n_ranks, rank, bytes_per_pixel, root, nccl_comm, stream))

    def assemble_frames(self, d_tiles, d_gathered, d_images, n_frames, image_size, tile_size, n_ranks, rank, bytes_per_pixel, root, nccl_comm, stream=0,
                        rects=None, roots=None):
        """vkv_assemble_frames: the exchange of a whole launch - frame f with tile rectangle rects[f] (None: the whole image) to its owner
        roots[f] (None: all to `root`, ONE ncclGather of the launch's block; else one group of gathers) + one de-interleave kernel on every owner
        (d_images: n_frames image pointers, entry f read on the owner of frame f only; None on ranks that own nothing)."""
        arr = (C.c_void_p * n_frames)(*d_images) if d_images is not None else None
        rarr = (abi.TileRect * n_frames)(*rects) if rects is not None else None
        oarr = (C.c_int32 * n_frames)(*roots) if roots is not None else None
        self.check(self._lib.vkv_assemble_frames(self.handle, d_tiles, d_gathered, arr, n_frames, image_size[0], image_size[1], tile_size[0], tile_size[1],
                                                 rarr, n_ranks, rank, bytes_per_pixel, root, oarr, nccl_comm, stream))

    # ---- set-up calls ----
    def get_tuning(self):
        t = abi.Tuning()
        self.check(self._lib.vkv_get_tuning(self.handle, C.byref(t)))
        return t

    def set_tuning(self, **fields):
        """read-modify-write of the context's VkvTuning block: ctx.set_tuning(scheduler=1)"""
        t = self.get_tuning()
        for k, v in fields.items():
            if not hasattr(t, k):
                raise AttributeError("VkvTuning has no field %r" % k)
            setattr(t, k, v)
        self.check(self._lib.vkv_set_tuning(self.handle, C.byref(t)))
        return t

    def prepare_render(self, params_list, stream=0):
        arr = (abi.RenderParams * len(params_list))(*params_list)
        self.check(self._lib.vkv_prepare_render(self.handle, arr, len(params_list), stream))

    def register_target(self, d_target, image_size, tiles):
        self.check(self._lib.vkv_register_target(self.handle, d_target, image_size[0], image_size[1], C.byref(tiles)))

    def forget_target(self, d_target):
        self.check(self._lib.vkv_forget_target(self.handle, d_target))

    def release_stream(self, stream):
        self.check(self._lib.vkv_release_stream(self.handle, stream))

    def trim(self):
        """vkv_trim: wait for the device, drop every cached table, empty the arena's table region"""
        self.check(self._lib.vkv_trim(self.handle))

    def release_captured(self, stream):
        """vkv_release_captured: the argument slots of the vkv_render_batch launches captured on `stream` return to the context"""
        self.check(self._lib.vkv_release_captured(self.handle, stream))

    def render_rc(self, params, stream=0):
        """Like render() but returns the status code instead of raising (error-path tests)."""
        return self._lib.vkv_render(self.handle, C.byref(params), stream)

    def scatter_tiles(self, d_gathered, d_image, image_size, tile_size, n_ranks, rank_stride_tiles, bytes_per_pixel, stream=0, rect=None):
        self.check(self._lib.vkv_scatter_tiles(self.handle, d_gathered, d_image, image_size[0], image_size[1], tile_size[0],
                                               tile_size[1], None if rect is None else C.byref(rect), n_ranks, rank_stride_tiles, bytes_per_pixel, stream))

    def synth_volume(self, d_volume, extent, kind, seed, stream=0):
        self.check(self._lib.vkv_synth_volume(self.handle, d_volume, extent, kind, seed, stream))

    def packed_volume_bytes(self, extent):
        return int(self._lib.vkv_packed_volume_bytes(extent))

    def pack_volume(self, d_volume, d_gradient, extent, d_packed, stream=0):
        self.check(self._lib.vkv_pack_volume(self.handle, d_volume, d_gradient, extent, d_packed, stream))

    def transfer_function_bits(self, d_tf, d_bits, stream=0):
        self.check(self._lib.vkv_transfer_function_bits(self.handle, d_tf, d_bits, stream))

    def transfer_function_tables(self, d_tf, tf, d_tables, stream=0):
        self.check(self._lib.vkv_transfer_function_tables(self.handle, d_tf, None if tf is None else C.byref(tf), d_tables, stream))

    def transfer_function_texture_device(self, options, d_tf, d_tables, stream=0):
        """vkv_transfer_function_texture_device: the TF texture + the integrator's tables from `options`, on the device (no host loop, no wait)"""
        self.check(self._lib.vkv_transfer_function_texture_device(self.handle, C.byref(options), d_tf, d_tables, stream))

    def update_transfer_function(self, options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                 d_count=None, stream=0):
        """vkv_update_transfer_function: [count,] texture + tables, occupancy and the transform of skipping_type, as one enqueue"""
        self.check(self.update_transfer_function_rc(options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                                    d_count, stream))

    def update_transfer_function_rc(self, options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                    d_count=None, stream=0):
        """Like update_transfer_function() but returns the status code (error-path tests); d_maps None passes a NULL array."""
        return self._lib.vkv_update_transfer_function(self.handle, None if options is None else C.byref(options), d_volume, d_gradient, extent, d_tf,
                                                      d_tables, _maps_array(d_maps), d_swap, map_extent, skipping_type, d_count, stream)

    def update_volume_region(self, d_src, voxel_type, big_endian, range_min, range_max, box, d_volume, d_gradient, d_packed, extent, d_tf, tf, d_maps,
                             d_swap, map_extent, skipping_type, stream=0):
        """vkv_update_volume_region: convert a box of raw voxels into the volume and rebuild the gradient, packed bricks, occupancy cells it
        reaches and the distance transform, as one enqueue; d_gradient / d_packed / d_maps None skip that output"""
        self.check(self.update_volume_region_rc(d_src, voxel_type, big_endian, range_min, range_max, box, d_volume, d_gradient, d_packed, extent, d_tf,
                                                tf, d_maps, d_swap, map_extent, skipping_type, stream))

    def update_volume_region_rc(self, d_src, voxel_type, big_endian, range_min, range_max, box, d_volume, d_gradient, d_packed, extent, d_tf, tf,
                                d_maps, d_swap, map_extent, skipping_type, stream=0):
        """Like update_volume_region() but returns the status code (error-path tests); box / tf / d_maps None pass NULL."""
        return self._lib.vkv_update_volume_region(self.handle, d_src, int(voxel_type), 1 if big_endian else 0, range_min, range_max,
                                                  None if box is None else C.byref(box), d_volume, d_gradient, d_packed, extent, d_tf,
                                                  None if tf is None else C.byref(tf), _maps_array(d_maps), d_swap, map_extent, skipping_type, stream)

    def volume_histogram(self, d_volume, d_gradient, extent, box, mode, d_histogram, stream=0):
        """vkv_volume_histogram: the (gradient byte, intensity byte) histogram of `box` (None: the whole volume) into the 65536 uint64 bins
        at d_histogram, set, added or subtracted as `mode` says; d_gradient None counts every voxel in gradient row 0"""
        self.check(self.volume_histogram_rc(d_volume, d_gradient, extent, box, mode, d_histogram, stream))

    def volume_histogram_rc(self, d_volume, d_gradient, extent, box, mode, d_histogram, stream=0):
        """Like volume_histogram() but returns the status code (error-path tests)."""
        return self._lib.vkv_volume_histogram(self.handle, d_volume, d_gradient, extent, None if box is None else C.byref(box), int(mode),
                                              d_histogram, stream)

    def histogram_occupied_count(self, d_histogram, tf, d_count, stream=0):
        """vkv_histogram_occupied_count: the bins whose analytic transfer-function alpha is > 0, summed into *d_count (stored, not added)"""
        self.check(self.histogram_occupied_count_rc(d_histogram, tf, d_count, stream))

    def histogram_occupied_count_rc(self, d_histogram, tf, d_count, stream=0):
        return self._lib.vkv_histogram_occupied_count(self.handle, d_histogram, None if tf is None else C.byref(tf), d_count, stream)

    def cell_summary(self, d_volume, d_gradient, extent, map_extent, box, d_summary, stream=0):
        """vkv_cell_summary: the 16-byte summaries of every occupancy cell (box None), or of the cells that meet `box`, into d_summary;
        d_gradient None records gradient byte 255 for every voxel"""
        self.check(self.cell_summary_rc(d_volume, d_gradient, extent, map_extent, box, d_summary, stream))

    def cell_summary_rc(self, d_volume, d_gradient, extent, map_extent, box, d_summary, stream=0):
        """Like cell_summary() but returns the status code (error-path tests)."""
        return self._lib.vkv_cell_summary(self.handle, d_volume, d_gradient, extent, map_extent, None if box is None else C.byref(box), d_summary, stream)

    def max_map(self, d_volume, extent, map_extent, box, d_max_map, stream=0):
        """vkv_max_map: per cell of map_extent the largest voxel of the cell grown by one voxel per side (box None: every cell; else the
        cells whose grown box meets `box`)"""
        self.check(self.max_map_rc(d_volume, extent, map_extent, box, d_max_map, stream))

    def max_map_rc(self, d_volume, extent, map_extent, box, d_max_map, stream=0):
        return self._lib.vkv_max_map(self.handle, d_volume, extent, map_extent, None if box is None else C.byref(box), d_max_map, stream)

    def render_mip(self, params, mip, stream=0):
        """vkv_render_mip: maximum-intensity projection of params' volume with the abi.MipOptions `mip`"""
        self.check(self.render_mip_rc(params, mip, stream))

    def render_mip_rc(self, params, mip, stream=0):
        return self._lib.vkv_render_mip(self.handle, None if params is None else C.byref(params), None if mip is None else C.byref(mip), stream)

    def render_isosurface(self, params, iso, stream=0):
        """vkv_render_isosurface: shaded isosurface of params' volume with the abi.IsoOptions `iso`"""
        self.check(self.render_isosurface_rc(params, iso, stream))

    def render_isosurface_rc(self, params, iso, stream=0):
        return self._lib.vkv_render_isosurface(self.handle, None if params is None else C.byref(params), None if iso is None else C.byref(iso), stream)

    def render_slab(self, params, slab, stream=0):
        """vkv_render_slab: an oblique slice or thick slab (max / min / mean) of params' volume with the abi.SlabOptions `slab`"""
        self.check(self.render_slab_rc(params, slab, stream))

    def render_slab_rc(self, params, slab, stream=0):
        return self._lib.vkv_render_slab(self.handle, None if params is None else C.byref(params), None if slab is None else C.byref(slab), stream)

    def isosurface_mesh(self, d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_triangles, capacity, d_counts, stream=0):
        """vkv_isosurface_mesh: the marching-tetrahedra triangles of `box` (None: the whole volume) at `iso` in their defined order; d_counts
        (2 x uint64) = the total and min(total, capacity); d_triangles the first min(total, capacity) triangles, 9 floats each.  d_max_map /
        map_extent None: dense.  d_scratch: mesh_scratch_bytes(extent, box) bytes."""
        self.check(self.isosurface_mesh_rc(d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_triangles, capacity, d_counts, stream))

    def isosurface_mesh_rc(self, d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_triangles, capacity, d_counts, stream=0):
        """Like isosurface_mesh() but returns the status code (error-path tests)."""
        return self._lib.vkv_isosurface_mesh(self.handle, d_volume, extent, None if box is None else C.byref(box), float(iso), d_max_map,
                                             abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_triangles, int(capacity),
                                             d_counts, stream)

    def isosurface_mesh_indexed(self, d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_vertices, d_normals, capacity_vertices,
                                d_indices, capacity_triangles, d_counts, stream=0):
        """vkv_isosurface_mesh_indexed: the surface of isosurface_mesh() as a vertex list (one vertex per crossing edge, 3 floats; d_normals
        None or as many gradient normals) and 3 x uint32 vertex numbers per triangle; d_counts (4 x uint64) = the triangles, those written,
        the vertices, those written.  d_scratch: mesh_indexed_scratch_bytes(extent, box) bytes."""
        self.check(self.isosurface_mesh_indexed_rc(d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_vertices, d_normals,
                                                   capacity_vertices, d_indices, capacity_triangles, d_counts, stream))

    def isosurface_mesh_indexed_rc(self, d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_vertices, d_normals, capacity_vertices,
                                   d_indices, capacity_triangles, d_counts, stream=0):
        """Like isosurface_mesh_indexed() but returns the status code (error-path tests)."""
        return self._lib.vkv_isosurface_mesh_indexed(self.handle, d_volume, extent, None if box is None else C.byref(box), float(iso), d_max_map,
                                                     abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_vertices, d_normals,
                                                     int(capacity_vertices), d_indices, int(capacity_triangles), d_counts, stream)

    def label_components(self, d_volume, extent, box, iso, connectivity, d_max_map, map_extent, d_scratch, d_labels, d_sizes, capacity_components,
                         d_counts, stream=0):
        """vkv_label_components: d_labels (uint32, the shape of `box`; None: of the volume) = 0 for an outside voxel, else the number 1 .. K of
        its connected component under `connectivity` (abi.CONNECT_*), numbered by first voxel; d_sizes[k - 1] = the voxels of component k for
        the first min(K, capacity_components); d_counts (3 x uint64) = K, the sizes written, the inside voxels.  d_scratch:
        components_scratch_bytes(extent, box) bytes."""
        self.check(self.label_components_rc(d_volume, extent, box, iso, connectivity, d_max_map, map_extent, d_scratch, d_labels, d_sizes,
                                            capacity_components, d_counts, stream))

    def label_components_rc(self, d_volume, extent, box, iso, connectivity, d_max_map, map_extent, d_scratch, d_labels, d_sizes, capacity_components,
                            d_counts, stream=0):
        """Like label_components() but returns the status code (error-path tests)."""
        return self._lib.vkv_label_components(self.handle, d_volume, extent, None if box is None else C.byref(box), float(iso), int(connectivity),
                                              d_max_map, abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_labels, d_sizes,
                                              int(capacity_components), d_counts, stream)

    def select_components(self, d_src, d_dst, extent, box, d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill=0, stream=0):
        """vkv_select_components: the voxels of `box` of d_dst = d_src, but `fill` where the voxel's component (d_labels, d_sizes, d_counts of
        label_components() for the same box) has fewer than min_voxels or more than max_voxels voxels; d_dst may be d_src"""
        self.check(self.select_components_rc(d_src, d_dst, extent, box, d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill, stream))

    def select_components_rc(self, d_src, d_dst, extent, box, d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill=0, stream=0):
        """Like select_components() but returns the status code (error-path tests)."""
        return self._lib.vkv_select_components(self.handle, d_src, d_dst, extent, None if box is None else C.byref(box), d_labels, d_sizes, d_counts,
                                               int(min_voxels), int(max_voxels), int(fill), stream)

    def component_stats(self, d_volume, extent, box, d_labels, d_counts, d_stats, capacity_components, stream=0):
        """vkv_component_stats: d_stats (abi.ComponentStats records, 80 bytes each) = for every label 1 .. min(d_counts[0],
        capacity_components) of d_labels (uint32, the shape of `box`; None: of the volume) its bounding box in volume coordinates, voxel
        count and coordinate sums and, unless d_volume is None, the smallest and largest byte and the sums of bytes and squared bytes"""
        self.check(self.component_stats_rc(d_volume, extent, box, d_labels, d_counts, d_stats, capacity_components, stream))

    def component_stats_rc(self, d_volume, extent, box, d_labels, d_counts, d_stats, capacity_components, stream=0):
        """Like component_stats() but returns the status code (error-path tests)."""
        return self._lib.vkv_component_stats(self.handle, d_volume, extent, None if box is None else C.byref(box), d_labels, d_counts, d_stats,
                                             int(capacity_components), stream)

    def select_components_by_table(self, d_src, d_dst, extent, box, d_labels, d_keep, table_entries, fill=0, stream=0):
        """vkv_select_components_by_table: the voxels of `box` of d_dst = d_src, but `fill` where the voxel's label L (d_labels, uint32, the
        box's shape) has d_keep[L - 1] == 0 (one byte per label, table_entries of them; labels beyond the table are kept); d_dst may be d_src"""
        self.check(self.select_components_by_table_rc(d_src, d_dst, extent, box, d_labels, d_keep, table_entries, fill, stream))

    def select_components_by_table_rc(self, d_src, d_dst, extent, box, d_labels, d_keep, table_entries, fill=0, stream=0):
        """Like select_components_by_table() but returns the status code (error-path tests)."""
        return self._lib.vkv_select_components_by_table(self.handle, d_src, d_dst, extent, None if box is None else C.byref(box), d_labels, d_keep,
                                                        int(table_entries), int(fill), stream)

    def distance_transform(self, d_volume, extent, box, iso, target, limit, d_scratch, d_dist2, stream=0):
        """vkv_distance_transform: d_dist2 (uint32, the shape of `box`; None: of the volume) = min(limit, the squared Euclidean distance to
        the nearest target voxel of the box), the targets being the voxels at or above `iso` (abi.DISTANCE_TO_INSIDE) or below it
        (abi.DISTANCE_TO_OUTSIDE); limit None or abi.DISTANCE_NONE: unlimited.  d_scratch: distance_transform_scratch_bytes(extent, box)
        bytes."""
        self.check(self.distance_transform_rc(d_volume, extent, box, iso, target, limit, d_scratch, d_dist2, stream))

    def distance_transform_rc(self, d_volume, extent, box, iso, target, limit, d_scratch, d_dist2, stream=0):
        """Like distance_transform() but returns the status code (error-path tests)."""
        return self._lib.vkv_distance_transform(self.handle, d_volume, extent, None if box is None else C.byref(box), float(iso), int(target),
                                                abi.DISTANCE_NONE if limit is None else int(limit), d_scratch, d_dist2, stream)

    def select_by_distance(self, d_src, d_dst, extent, box, d_dist2, lo, hi, fill, stream=0):
        """vkv_select_by_distance: the voxels of `box` of d_dst = `fill` where lo <= d_dist2 <= hi (distance_transform() of the same box),
        else d_src; d_dst may be d_src"""
        self.check(self.select_by_distance_rc(d_src, d_dst, extent, box, d_dist2, lo, hi, fill, stream))

    def select_by_distance_rc(self, d_src, d_dst, extent, box, d_dist2, lo, hi, fill, stream=0):
        """Like select_by_distance() but returns the status code (error-path tests)."""
        return self._lib.vkv_select_by_distance(self.handle, d_src, d_dst, extent, None if box is None else C.byref(box), d_dist2, int(lo), int(hi),
                                                int(fill), stream)

    def filter_volume(self, d_src, d_dst, extent, box, kind, stream=0):
        """vkv_filter_volume: the voxels of `box` (None: every voxel) of d_dst = the 3x3x3 filter `kind` (abi.FILTER_*) of d_src"""
        self.check(self.filter_volume_rc(d_src, d_dst, extent, box, kind, stream))

    def filter_volume_rc(self, d_src, d_dst, extent, box, kind, stream=0):
        """Like filter_volume() but returns the status code (error-path tests)."""
        return self._lib.vkv_filter_volume(self.handle, d_src, d_dst, extent, None if box is None else C.byref(box), int(kind), stream)

    def occupancy_map_from_summary(self, d_summary, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, d_unresolved=None, stream=0):
        """vkv_occupancy_map_from_summary: vkv_occupancy_map's map, decided from the cell summaries where they are certain; d_unresolved
        receives the number of cells evaluated from their voxels"""
        self.check(self.occupancy_map_from_summary_rc(d_summary, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, d_unresolved, stream))

    def occupancy_map_from_summary_rc(self, d_summary, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, d_unresolved=None, stream=0):
        return self._lib.vkv_occupancy_map_from_summary(self.handle, d_summary, d_volume, d_gradient, d_tf, None if tf is None else C.byref(tf), extent,
                                                        d_map, map_extent, d_unresolved, stream)

    def update_transfer_function_from_summary(self, options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                              d_count, d_summary, d_histogram, d_unresolved=None, stream=0):
        """vkv_update_transfer_function_from_summary: update_transfer_function() with the occupancy from the cell summaries and the count
        (d_count not None) from the histogram"""
        self.check(self.update_transfer_function_from_summary_rc(options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent,
                                                                 skipping_type, d_count, d_summary, d_histogram, d_unresolved, stream))

    def update_transfer_function_from_summary_rc(self, options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                                 d_count, d_summary, d_histogram, d_unresolved=None, stream=0):
        """Like update_transfer_function_from_summary() but returns the status code; d_maps None passes a NULL array."""
        return self._lib.vkv_update_transfer_function_from_summary(self.handle, None if options is None else C.byref(options), d_volume, d_gradient,
                                                                   extent, d_tf, d_tables, _maps_array(d_maps), d_swap, map_extent, skipping_type, d_count,
                                                                   d_summary, d_histogram, d_unresolved, stream)

    def debug_tf_scratch(self, d_out, stream=0):
        """vkv_debug_tf_scratch: the bit table + column mask (2056 words) in `stream`'s scratch block, copied to d_out"""
        self.check(self._lib.vkv_debug_tf_scratch(self.handle, d_out, stream))

    def occupied_voxel_count(self, d_volume, d_gradient, tf, extent, d_count, stream=0):
        self.check(self._lib.vkv_occupied_voxel_count(self.handle, d_volume, d_gradient, C.byref(tf), extent, d_count, stream))

    def convert_volume(self, d_raw, voxel_type, big_endian, range_min, range_max, n_voxels, d_out, stream=0):
        self.check(self._lib.vkv_convert_volume(self.handle, d_raw, voxel_type, 1 if big_endian else 0, range_min, range_max, n_voxels, d_out, stream))

    def last_error(self):
        return self._lib.vkv_last_error(self.handle).decode(errors="replace")


# ---- host helpers (no device needed) --------------------------------------------------------------

def transfer_function_uniform(options):
    out = abi.TransferFunctionUniform()
    rc = load().vkv_transfer_function_uniform(C.byref(options), C.byref(out))
    if rc != 0:
        raise VkvError(rc, "vkv_transfer_function_uniform")
    return out


def transfer_function_texture(options):
    import numpy as np
    tex = np.zeros((256, 256, 4), np.uint8)
    rc = load().vkv_transfer_function_texture(C.byref(options), tex.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise VkvError(rc, "vkv_transfer_function_texture")
    return tex


def build_uniforms(view, proj, node_transform, image_transform, clip_distance, image_size, volume_extent, map_extent):
    import numpy as np
    cam, rc_, rg = abi.CameraUniform(), abi.RayCastUniform(), abi.RayGen()
    mats = [np.ascontiguousarray(m, np.float32).reshape(16) for m in (view, proj, node_transform, image_transform)]
    rc = load().vkv_build_uniforms(*[m.ctypes.data_as(C.c_void_p) for m in mats], clip_distance, image_size[0], image_size[1],
                                   volume_extent, map_extent, C.byref(cam), C.byref(rc_), C.byref(rg))
    if rc != 0:
        raise VkvError(rc, "vkv_build_uniforms")
    return cam, rc_, rg


def screen_tile_rect(ray_cast, ray_gen, image_size, tile_size=(16, 16), align_tiles=1):
    """vkv_screen_tile_rect: the tile rectangle the fragments of a frame with these uniforms can lie in (pure CPU; every rank derives the same)"""
    out = abi.TileRect()
    rc = load().vkv_screen_tile_rect(C.byref(ray_cast), C.byref(ray_gen), image_size[0], image_size[1], tile_size[0], tile_size[1], align_tiles, C.byref(out))
    if rc != 0:
        raise VkvError(rc, "vkv_screen_tile_rect")
    return out


def load_header(path):
    """LoadVolume::load_header; raises RuntimeError with the reference's message on failure."""
    h = abi.VolumeHeader()
    if load().vkv_load_header(os.fsencode(path), C.byref(h)) != 0:
        raise RuntimeError("Failed to open header file")
    return h


def load_data(path, header):
    """LoadVolume::load_data → uint8 array [D, H, W]."""
    import numpy as np
    e = header.extent
    out = np.empty((e.depth, e.height, e.width), np.uint8)
    rc = load().vkv_load_data(os.fsencode(path), C.byref(header), out.ctypes.data_as(C.c_void_p), out.nbytes)
    if rc != 0:
        raise RuntimeError("load_data failed (%d)" % rc)
    return out


def mesh_scratch_bytes(extent, box=None):
    """vkv_isosurface_mesh_scratch_bytes: the scratch vkv_isosurface_mesh needs for `box` (None: the whole volume) of `extent`; 0 for an extent
    or box the call rejects"""
    return int(load().vkv_isosurface_mesh_scratch_bytes(extent, None if box is None else C.byref(box)))


def components_scratch_bytes(extent, box=None):
    """vkv_label_components_scratch_bytes: the scratch vkv_label_components needs for `box` (None: the whole volume) of `extent`; 0 for an
    extent or box the call rejects (a box of more than 2^32 - 1 voxels included)"""
    return int(load().vkv_label_components_scratch_bytes(extent, None if box is None else C.byref(box)))


def distance_transform_scratch_bytes(extent, box=None):
    """vkv_distance_transform_scratch_bytes: the scratch vkv_distance_transform needs for `box` (None: the whole volume) of `extent`: 4 bytes
    per voxel and 8 per 64 voxels; 0 for an extent or box the call rejects (more than 2^32 - 1 voxels or an axis above 32768 included)"""
    return int(load().vkv_distance_transform_scratch_bytes(extent, None if box is None else C.byref(box)))


def mesh_indexed_scratch_bytes(extent, box=None):
    """vkv_isosurface_mesh_indexed_scratch_bytes: the scratch vkv_isosurface_mesh_indexed needs for `box` (None: the whole volume) of `extent`;
    0 for an extent or box the call rejects"""
    return int(load().vkv_isosurface_mesh_indexed_scratch_bytes(extent, None if box is None else C.byref(box)))

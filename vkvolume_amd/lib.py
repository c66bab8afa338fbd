"""ctypes binding of ``csrc/libvkvolume_amd.so`` (the C ABI of ``include/vkvolume_amd.h``).

There is no fallback: if the shared library is missing or a call fails, a ``VkvError`` is raised.
"""
import ctypes as C
import functools
import os

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VKV_LIB_PATH") or os.path.join(_HERE, "csrc", "libvkvolume_amd.so")  # override: kernel experiments only


def _signatures():
    """One row per entry point, in the order of a C prototype: (result type, symbol, argument types, debug).  A pointer to a struct is
    P(its abi mirror), which takes an instance, a byref of one or None; VkvExtent3D goes by value, so a missing or swapped entry would
    shift every later argument: tests/test_binding_cpu.py holds each row to the headers."""
    vp, u32, i32, u64, f32, size, INT, text, P = (C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.c_float, C.c_size_t, C.c_int, C.c_char_p,
                                                  C.POINTER)

    def row(restype, symbol, *argtypes, debug=False):
        return restype, symbol, list(argtypes), debug

    return [
        # include/vkvolume_amd.h
        row(INT, "vkv_create", INT, P(vp)),
        row(None, "vkv_destroy", vp),
        row(text, "vkv_last_error", vp),
        row(text, "vkv_version"),
        row(INT, "vkv_transfer_function_uniform", P(abi.VolumeOptions), P(abi.TransferFunctionUniform)),
        row(INT, "vkv_transfer_function_texture", P(abi.VolumeOptions), vp),
        row(INT, "vkv_build_uniforms", vp, vp, vp, vp, f32, u32, u32, abi.Extent3D, abi.Extent3D, P(abi.CameraUniform), P(abi.RayCastUniform),
            P(abi.RayGen)),
        row(INT, "vkv_gradient_map", vp, vp, vp, abi.Extent3D, P(abi.TransferFunctionUniform), vp),
        row(INT, "vkv_occupancy_map", vp, vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, vp, abi.Extent3D, vp),
        row(INT, "vkv_distance_map", vp, vp, vp, abi.Extent3D, vp),
        row(INT, "vkv_distance_map_anisotropic", vp, P(vp), vp, abi.Extent3D, vp),
        row(INT, "vkv_compute_distance_map", vp, vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, P(vp), vp, abi.Extent3D, i32, vp),
        row(INT, "vkv_render", vp, P(abi.RenderParams), vp),
        row(INT, "vkv_render_batch", vp, P(abi.RenderParams), u32, vp),
        row(INT, "vkv_scatter_tiles", vp, vp, vp, u32, u32, u32, u32, P(abi.TileRect), u32, u32, u32, vp),
        row(INT, "vkv_synth_volume", vp, vp, abi.Extent3D, u32, u32, vp),
        row(size, "vkv_packed_volume_bytes", abi.Extent3D),
        row(INT, "vkv_pack_volume", vp, vp, vp, abi.Extent3D, vp, vp),
        row(INT, "vkv_transfer_function_bits", vp, vp, vp, vp),
        row(INT, "vkv_transfer_function_tables", vp, vp, P(abi.TransferFunctionUniform), vp, vp),
        row(INT, "vkv_occupied_voxel_count", vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, vp, vp),
        row(INT, "vkv_load_header", text, P(abi.VolumeHeader)),
        row(INT, "vkv_load_data", text, P(abi.VolumeHeader), vp, size),
        row(INT, "vkv_convert_volume", vp, vp, i32, i32, f32, f32, u64, vp, vp),
        row(INT, "vkv_gather_tiles", vp, vp, vp, size, i32, vp, vp),
        row(INT, "vkv_assemble_frame", vp, vp, vp, vp, u32, u32, u32, u32, P(abi.TileRect), u32, u32, u32, i32, vp, vp),
        row(INT, "vkv_assemble_frames", vp, vp, vp, P(vp), u32, u32, u32, u32, u32, P(abi.TileRect), u32, u32, u32, i32, P(i32), vp, vp),
        row(INT, "vkv_get_tuning", vp, P(abi.Tuning)),
        row(INT, "vkv_set_tuning", vp, P(abi.Tuning)),
        row(INT, "vkv_prepare_render", vp, P(abi.RenderParams), u32, vp),
        row(INT, "vkv_register_target", vp, vp, u32, u32, P(abi.TileSchedule)),
        row(INT, "vkv_forget_target", vp, vp),
        row(INT, "vkv_release_stream", vp, vp),
        row(INT, "vkv_trim", vp),
        row(INT, "vkv_release_captured", vp, vp),
        row(INT, "vkv_screen_tile_rect", P(abi.RayCastUniform), P(abi.RayGen), u32, u32, u32, u32, u32, P(abi.TileRect)),
        row(INT, "vkv_transfer_function_texture_device", vp, P(abi.VolumeOptions), vp, vp, vp),
        row(INT, "vkv_update_transfer_function", vp, P(abi.VolumeOptions), vp, vp, abi.Extent3D, vp, vp, P(vp), vp, abi.Extent3D, i32, vp, vp),
        row(INT, "vkv_update_volume_region", vp, vp, i32, i32, f32, f32, P(abi.Box), vp, vp, vp, abi.Extent3D, vp, P(abi.TransferFunctionUniform),
            P(vp), vp, abi.Extent3D, i32, vp),
        row(INT, "vkv_volume_histogram", vp, vp, vp, abi.Extent3D, P(abi.Box), i32, vp, vp),
        row(INT, "vkv_histogram_occupied_count", vp, vp, P(abi.TransferFunctionUniform), vp, vp),
        row(INT, "vkv_cell_summary", vp, vp, vp, abi.Extent3D, abi.Extent3D, P(abi.Box), vp, vp),
        row(INT, "vkv_occupancy_map_from_summary", vp, vp, vp, vp, vp, P(abi.TransferFunctionUniform), abi.Extent3D, vp, abi.Extent3D, vp, vp),
        row(INT, "vkv_update_transfer_function_from_summary", vp, P(abi.VolumeOptions), vp, vp, abi.Extent3D, vp, vp, P(vp), vp, abi.Extent3D, i32,
            vp, vp, vp, vp, vp),
        row(INT, "vkv_max_map", vp, vp, abi.Extent3D, abi.Extent3D, P(abi.Box), vp, vp),
        row(INT, "vkv_render_mip", vp, P(abi.RenderParams), P(abi.MipOptions), vp),
        row(INT, "vkv_render_isosurface", vp, P(abi.RenderParams), P(abi.IsoOptions), vp),
        row(INT, "vkv_render_slab", vp, P(abi.RenderParams), P(abi.SlabOptions), vp),
        row(INT, "vkv_filter_volume", vp, vp, vp, abi.Extent3D, P(abi.Box), i32, vp),
        row(size, "vkv_isosurface_mesh_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_isosurface_mesh", vp, vp, abi.Extent3D, P(abi.Box), f32, vp, abi.Extent3D, vp, vp, u64, vp, vp),
        row(size, "vkv_isosurface_mesh_indexed_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_isosurface_mesh_indexed", vp, vp, abi.Extent3D, P(abi.Box), f32, vp, abi.Extent3D, vp, vp, vp, u64, vp, u64, vp, vp),
        row(size, "vkv_label_components_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_label_components", vp, vp, abi.Extent3D, P(abi.Box), f32, i32, vp, abi.Extent3D, vp, vp, vp, u64, vp, vp),
        row(INT, "vkv_select_components", vp, vp, vp, abi.Extent3D, P(abi.Box), vp, vp, vp, u64, u64, u32, vp),
        row(INT, "vkv_component_stats", vp, vp, abi.Extent3D, P(abi.Box), vp, vp, vp, u64, vp),
        row(INT, "vkv_select_components_by_table", vp, vp, vp, abi.Extent3D, P(abi.Box), vp, vp, u64, u32, vp),
        row(size, "vkv_distance_transform_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_distance_transform", vp, vp, abi.Extent3D, P(abi.Box), f32, i32, u32, vp, vp, vp),
        row(INT, "vkv_select_by_distance", vp, vp, vp, abi.Extent3D, P(abi.Box), vp, u32, u32, u32, vp),
        row(INT, "vkv_distance_transform_weighted", vp, vp, abi.Extent3D, P(abi.Box), f32, i32, P(u32), u32, vp, vp, vp),
        row(INT, "vkv_nearest_target", vp, vp, abi.Extent3D, P(abi.Box), f32, i32, P(u32), u32, vp, vp, vp, vp),
        row(INT, "vkv_propagate_labels", vp, vp, vp, vp, abi.Extent3D, P(abi.Box), vp, f32, vp),
        row(size, "vkv_geodesic_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_geodesic_propagate", vp, vp, abi.Extent3D, P(abi.Box), f32, vp, P(u32), u32, u32, i32, vp, vp, vp, vp, vp),
        row(INT, "vkv_label_visibility_map", vp, vp, abi.Extent3D, P(abi.Box), vp, u64, abi.Extent3D, vp, vp),
        row(INT, "vkv_render_labels", vp, P(abi.RenderParams), P(abi.LabelRenderOptions), vp),
        row(size, "vkv_label_mesh_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_label_mesh", vp, vp, abi.Extent3D, P(abi.Box), vp, u64, vp, f32, vp, abi.Extent3D, vp, vp, vp, u64, vp, vp),
        row(size, "vkv_label_mesh_indexed_scratch_bytes", abi.Extent3D, P(abi.Box)),
        row(INT, "vkv_label_mesh_indexed", vp, vp, abi.Extent3D, P(abi.Box), vp, u64, vp, f32, vp, abi.Extent3D, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp),
        row(size, "vkv_mesh_adjacency_scratch_bytes", u64, u64),
        row(INT, "vkv_mesh_adjacency", vp, vp, u64, u64, vp, vp, vp),
        row(INT, "vkv_mesh_smooth", vp, vp, vp, u64, vp, vp, vp, P(f32), u32, vp),
        row(INT, "vkv_mesh_vertex_normals", vp, vp, vp, vp, u32, u64, u64, vp, vp, vp, vp),
        row(size, "vkv_mesh_decimate_scratch_bytes", u64, u64, abi.Extent3D),
        row(INT, "vkv_mesh_decimate", vp, vp, vp, vp, u64, u64, vp, P(f32), P(f32), abi.Extent3D, vp, vp, u64, vp, vp, u64, vp, vp, vp),
        # include/vkvolume_amd_debug.h (diagnostics: tools/ and the exhaustive numerics tests)
        row(INT, "vkv_debug_trace", vp, vp, debug=True),
        row(INT, "vkv_debug_tile_orders", vp, vp, u32, u32, debug=True),
        row(INT, "vkv_debug_check", vp, i32, u32, u64, vp, vp, debug=True),
        row(INT, "vkv_debug_tf_scratch", vp, vp, vp, debug=True),
    ]


SIGNATURES = _signatures()
EXPORTS = [symbol for _, symbol, _, debug in SIGNATURES if not debug]  # every symbol include/vkvolume_amd.h declares
DEBUG_EXPORTS = [symbol for _, symbol, _, debug in SIGNATURES if debug]  # and include/vkvolume_amd_debug.h


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
    for restype, symbol, argtypes, _ in SIGNATURES:
        f = getattr(L, symbol)  # AttributeError here means the library does not export what the headers declare
        f.restype, f.argtypes = restype, argtypes
    _LIB = L
    return L


def _raising(rc_method):
    """The raising form ``x`` of a Context method ``x_rc`` that returns a status code: the same parameters and the docstring written on
    ``x_rc``, a VkvError with the context's message for a status other than 0.  ``x_rc`` keeps a line that says how it differs."""
    name = rc_method.__name__[:-len("_rc")]

    @functools.wraps(rc_method)  # (inspect.signature follows __wrapped__)
    def method(self, *args, **kwargs):
        self.check(rc_method(self, *args, **kwargs))

    method.__name__, method.__qualname__ = name, rc_method.__qualname__[:-len("_rc")]
    rc_method.__doc__ = "Like %s() but returns the status code instead of raising (error-path tests)." % name
    return method


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
            raise VkvError(rc, self.last_error())

    def last_error(self):
        return self._lib.vkv_last_error(self.handle).decode(errors="replace")

    # ---- device entry points (pointers are ints / None; stream is a hipStream_t handle as int; a struct parameter takes the abi object, or
    # None for NULL).  Where error-path tests need the status code, the body is written once as x_rc and x is derived from it. ----
    def gradient_map(self, d_volume, d_gradient, extent, tf, stream=0):
        self.check(self._lib.vkv_gradient_map(self.handle, d_volume, d_gradient, extent, tf, stream))

    def occupancy_map(self, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, stream=0):
        self.check(self._lib.vkv_occupancy_map(self.handle, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, stream))

    def distance_map(self, d_map, d_swap, map_extent, stream=0):
        self.check(self._lib.vkv_distance_map(self.handle, d_map, d_swap, map_extent, stream))

    def distance_map_anisotropic(self, d_maps, d_swap, map_extent, stream=0):
        self.check(self._lib.vkv_distance_map_anisotropic(self.handle, _maps_array(d_maps), d_swap, map_extent, stream))

    def compute_distance_map(self, d_volume, d_gradient, d_tf, tf, extent, d_maps, d_swap, map_extent, skipping_type, stream=0):
        self.check(self._lib.vkv_compute_distance_map(self.handle, d_volume, d_gradient, d_tf, tf, extent, _maps_array(d_maps), d_swap, map_extent,
                                                      skipping_type, stream))

    def render_rc(self, params, stream=0):
        return self._lib.vkv_render(self.handle, params, stream)

    render = _raising(render_rc)

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
                                                rect, n_ranks, rank, bytes_per_pixel, root, nccl_comm, stream))

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
        self.check(self._lib.vkv_set_tuning(self.handle, t))
        return t

    def prepare_render(self, params_list, stream=0):
        arr = (abi.RenderParams * len(params_list))(*params_list)
        self.check(self._lib.vkv_prepare_render(self.handle, arr, len(params_list), stream))

    def register_target(self, d_target, image_size, tiles):
        self.check(self._lib.vkv_register_target(self.handle, d_target, image_size[0], image_size[1], tiles))

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

    def scatter_tiles(self, d_gathered, d_image, image_size, tile_size, n_ranks, rank_stride_tiles, bytes_per_pixel, stream=0, rect=None):
        self.check(self._lib.vkv_scatter_tiles(self.handle, d_gathered, d_image, image_size[0], image_size[1], tile_size[0], tile_size[1], rect,
                                               n_ranks, rank_stride_tiles, bytes_per_pixel, stream))

    def synth_volume(self, d_volume, extent, kind, seed, stream=0):
        self.check(self._lib.vkv_synth_volume(self.handle, d_volume, extent, kind, seed, stream))

    def packed_volume_bytes(self, extent):
        return self._lib.vkv_packed_volume_bytes(extent)

    def pack_volume(self, d_volume, d_gradient, extent, d_packed, stream=0):
        self.check(self._lib.vkv_pack_volume(self.handle, d_volume, d_gradient, extent, d_packed, stream))

    def transfer_function_bits(self, d_tf, d_bits, stream=0):
        self.check(self._lib.vkv_transfer_function_bits(self.handle, d_tf, d_bits, stream))

    def transfer_function_tables(self, d_tf, tf, d_tables, stream=0):
        self.check(self._lib.vkv_transfer_function_tables(self.handle, d_tf, tf, d_tables, stream))

    def transfer_function_texture_device(self, options, d_tf, d_tables, stream=0):
        """vkv_transfer_function_texture_device: the TF texture + the integrator's tables from `options`, on the device (no host loop, no wait)"""
        self.check(self._lib.vkv_transfer_function_texture_device(self.handle, options, d_tf, d_tables, stream))

    def update_transfer_function_rc(self, options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                    d_count=None, stream=0):
        """vkv_update_transfer_function: [count,] texture + tables, occupancy and the transform of skipping_type, as one enqueue"""
        return self._lib.vkv_update_transfer_function(self.handle, options, d_volume, d_gradient, extent, d_tf, d_tables, _maps_array(d_maps), d_swap,
                                                      map_extent, skipping_type, d_count, stream)

    update_transfer_function = _raising(update_transfer_function_rc)

    def update_volume_region_rc(self, d_src, voxel_type, big_endian, range_min, range_max, box, d_volume, d_gradient, d_packed, extent, d_tf, tf,
                                d_maps, d_swap, map_extent, skipping_type, stream=0):
        """vkv_update_volume_region: convert a box of raw voxels into the volume and rebuild the gradient, packed bricks, occupancy cells it
        reaches and the distance transform, as one enqueue; d_gradient / d_packed / d_maps None skip that output"""
        return self._lib.vkv_update_volume_region(self.handle, d_src, int(voxel_type), 1 if big_endian else 0, range_min, range_max, box, d_volume,
                                                  d_gradient, d_packed, extent, d_tf, tf, _maps_array(d_maps), d_swap, map_extent, skipping_type, stream)

    update_volume_region = _raising(update_volume_region_rc)

    def volume_histogram_rc(self, d_volume, d_gradient, extent, box, mode, d_histogram, stream=0):
        """vkv_volume_histogram: the (gradient byte, intensity byte) histogram of `box` (None: the whole volume) into the 65536 uint64 bins
        at d_histogram, set, added or subtracted as `mode` says; d_gradient None counts every voxel in gradient row 0"""
        return self._lib.vkv_volume_histogram(self.handle, d_volume, d_gradient, extent, box, int(mode), d_histogram, stream)

    volume_histogram = _raising(volume_histogram_rc)

    def histogram_occupied_count_rc(self, d_histogram, tf, d_count, stream=0):
        """vkv_histogram_occupied_count: the bins whose analytic transfer-function alpha is > 0, summed into *d_count (stored, not added)"""
        return self._lib.vkv_histogram_occupied_count(self.handle, d_histogram, tf, d_count, stream)

    histogram_occupied_count = _raising(histogram_occupied_count_rc)

    def cell_summary_rc(self, d_volume, d_gradient, extent, map_extent, box, d_summary, stream=0):
        """vkv_cell_summary: the 16-byte summaries of every occupancy cell (box None), or of the cells that meet `box`, into d_summary;
        d_gradient None records gradient byte 255 for every voxel"""
        return self._lib.vkv_cell_summary(self.handle, d_volume, d_gradient, extent, map_extent, box, d_summary, stream)

    cell_summary = _raising(cell_summary_rc)

    def max_map_rc(self, d_volume, extent, map_extent, box, d_max_map, stream=0):
        """vkv_max_map: per cell of map_extent the largest voxel of the cell grown by one voxel per side (box None: every cell; else the
        cells whose grown box meets `box`)"""
        return self._lib.vkv_max_map(self.handle, d_volume, extent, map_extent, box, d_max_map, stream)

    max_map = _raising(max_map_rc)

    def render_mip_rc(self, params, mip, stream=0):
        """vkv_render_mip: maximum-intensity projection of params' volume with the abi.MipOptions `mip`"""
        return self._lib.vkv_render_mip(self.handle, params, mip, stream)

    render_mip = _raising(render_mip_rc)

    def render_isosurface_rc(self, params, iso, stream=0):
        """vkv_render_isosurface: shaded isosurface of params' volume with the abi.IsoOptions `iso`"""
        return self._lib.vkv_render_isosurface(self.handle, params, iso, stream)

    render_isosurface = _raising(render_isosurface_rc)

    def render_slab_rc(self, params, slab, stream=0):
        """vkv_render_slab: an oblique slice or thick slab (max / min / mean) of params' volume with the abi.SlabOptions `slab`"""
        return self._lib.vkv_render_slab(self.handle, params, slab, stream)

    render_slab = _raising(render_slab_rc)

    def isosurface_mesh_rc(self, d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_triangles, capacity, d_counts, stream=0):
        """vkv_isosurface_mesh: the marching-tetrahedra triangles of `box` (None: the whole volume) at `iso` in their defined order; d_counts
        (2 x uint64) = the total and min(total, capacity); d_triangles the first min(total, capacity) triangles, 9 floats each.  d_max_map /
        map_extent None: dense.  d_scratch: mesh_scratch_bytes(extent, box) bytes."""
        return self._lib.vkv_isosurface_mesh(self.handle, d_volume, extent, box, iso, d_max_map,
                                             abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_triangles, capacity, d_counts,
                                             stream)

    isosurface_mesh = _raising(isosurface_mesh_rc)

    def isosurface_mesh_indexed_rc(self, d_volume, extent, box, iso, d_max_map, map_extent, d_scratch, d_vertices, d_normals, capacity_vertices,
                                   d_indices, capacity_triangles, d_counts, stream=0):
        """vkv_isosurface_mesh_indexed: the surface of isosurface_mesh() as a vertex list (one vertex per crossing edge, 3 floats; d_normals
        None or as many gradient normals) and 3 x uint32 vertex numbers per triangle; d_counts (4 x uint64) = the triangles, those written,
        the vertices, those written.  d_scratch: mesh_indexed_scratch_bytes(extent, box) bytes."""
        return self._lib.vkv_isosurface_mesh_indexed(self.handle, d_volume, extent, box, iso, d_max_map,
                                                     abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_vertices, d_normals,
                                                     capacity_vertices, d_indices, capacity_triangles, d_counts, stream)

    isosurface_mesh_indexed = _raising(isosurface_mesh_indexed_rc)

    def label_components_rc(self, d_volume, extent, box, iso, connectivity, d_max_map, map_extent, d_scratch, d_labels, d_sizes, capacity_components,
                            d_counts, stream=0):
        """vkv_label_components: d_labels (uint32, the shape of `box`; None: of the volume) = 0 for an outside voxel, else the number 1 .. K of
        its connected component under `connectivity` (abi.CONNECT_*), numbered by first voxel; d_sizes[k - 1] = the voxels of component k for
        the first min(K, capacity_components); d_counts (3 x uint64) = K, the sizes written, the inside voxels.  d_scratch:
        components_scratch_bytes(extent, box) bytes."""
        return self._lib.vkv_label_components(self.handle, d_volume, extent, box, iso, int(connectivity), d_max_map,
                                              abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_labels, d_sizes,
                                              capacity_components, d_counts, stream)

    label_components = _raising(label_components_rc)

    def select_components_rc(self, d_src, d_dst, extent, box, d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill=0, stream=0):
        """vkv_select_components: the voxels of `box` of d_dst = d_src, but `fill` where the voxel's component (d_labels, d_sizes, d_counts of
        label_components() for the same box) has fewer than min_voxels or more than max_voxels voxels; d_dst may be d_src"""
        return self._lib.vkv_select_components(self.handle, d_src, d_dst, extent, box, d_labels, d_sizes, d_counts, min_voxels, max_voxels, fill, stream)

    select_components = _raising(select_components_rc)

    def component_stats_rc(self, d_volume, extent, box, d_labels, d_counts, d_stats, capacity_components, stream=0):
        """vkv_component_stats: d_stats (abi.ComponentStats records, 80 bytes each) = for every label 1 .. min(d_counts[0],
        capacity_components) of d_labels (uint32, the shape of `box`; None: of the volume) its bounding box in volume coordinates, voxel
        count and coordinate sums and, unless d_volume is None, the smallest and largest byte and the sums of bytes and squared bytes"""
        return self._lib.vkv_component_stats(self.handle, d_volume, extent, box, d_labels, d_counts, d_stats, capacity_components, stream)

    component_stats = _raising(component_stats_rc)

    def select_components_by_table_rc(self, d_src, d_dst, extent, box, d_labels, d_keep, table_entries, fill=0, stream=0):
        """vkv_select_components_by_table: the voxels of `box` of d_dst = d_src, but `fill` where the voxel's label L (d_labels, uint32, the
        box's shape) has d_keep[L - 1] == 0 (one byte per label, table_entries of them; labels beyond the table are kept); d_dst may be d_src"""
        return self._lib.vkv_select_components_by_table(self.handle, d_src, d_dst, extent, box, d_labels, d_keep, table_entries, fill, stream)

    select_components_by_table = _raising(select_components_by_table_rc)

    def distance_transform_rc(self, d_volume, extent, box, iso, target, limit, d_scratch, d_dist2, stream=0):
        """vkv_distance_transform: d_dist2 (uint32, the shape of `box`; None: of the volume) = min(limit, the squared Euclidean distance to
        the nearest target voxel of the box), the targets being the voxels at or above `iso` (abi.DISTANCE_TO_INSIDE) or below it
        (abi.DISTANCE_TO_OUTSIDE); limit None or abi.DISTANCE_NONE: unlimited.  d_scratch: distance_transform_scratch_bytes(extent, box)
        bytes."""
        return self._lib.vkv_distance_transform(self.handle, d_volume, extent, box, iso, int(target),
                                                abi.DISTANCE_NONE if limit is None else int(limit), d_scratch, d_dist2, stream)

    distance_transform = _raising(distance_transform_rc)

    def select_by_distance_rc(self, d_src, d_dst, extent, box, d_dist2, lo, hi, fill, stream=0):
        """vkv_select_by_distance: the voxels of `box` of d_dst = `fill` where lo <= d_dist2 <= hi (distance_transform() of the same box),
        else d_src; d_dst may be d_src"""
        return self._lib.vkv_select_by_distance(self.handle, d_src, d_dst, extent, box, d_dist2, lo, hi, fill, stream)

    select_by_distance = _raising(select_by_distance_rc)

    def distance_transform_weighted_rc(self, d_volume, extent, box, iso, target, weights, limit, d_scratch, d_dist2, stream=0):
        """vkv_distance_transform_weighted: distance_transform() with integer weights (wx, wy, wz): d_dist2 = min(limit, the least
        (wx dx)^2 + (wy dy)^2 + (wz dz)^2 to a target voxel of the box); the same scratch block.  Returns the status code: there is no raising
        form (the public surface admits new names only as _rc), so callers write ctx.check(ctx.distance_transform_weighted_rc(...)).
        weights None passes NULL (error-path tests)."""
        return self._lib.vkv_distance_transform_weighted(self.handle, d_volume, extent, box, iso, int(target),
                                                         None if weights is None else (C.c_uint32 * 3)(*(int(w) for w in weights)),
                                                         abi.DISTANCE_NONE if limit is None else int(limit), d_scratch, d_dist2, stream)

    def nearest_target_rc(self, d_volume, extent, box, iso, target, weights, limit, d_scratch, d_nearest, d_dist2=None, stream=0):
        """vkv_nearest_target: d_nearest (uint32, the shape of `box`) = the smallest box-linear index among the targets at the least
        (wx dx)^2 + (wy dy)^2 + (wz dz)^2 from each voxel, abi.NEAREST_NONE where the box holds no target or that distance is >= limit;
        d_dist2 (None: not wanted) = distance_transform_weighted_rc()'s bytes.  Targets, weights, limit and the scratch block
        (distance_transform_scratch_bytes) are that call's.  Returns the status code: there is no raising form (the public surface admits
        new names only as _rc), so callers write ctx.check(ctx.nearest_target_rc(...)).  weights None passes NULL (error-path tests)."""
        return self._lib.vkv_nearest_target(self.handle, d_volume, extent, box, iso, int(target),
                                            None if weights is None else (C.c_uint32 * 3)(*(int(w) for w in weights)),
                                            abi.DISTANCE_NONE if limit is None else int(limit), d_scratch, d_nearest, d_dist2, stream)

    def propagate_labels_rc(self, d_nearest, d_labels, d_out, extent, box, d_mask_volume=None, mask_iso=0.0, stream=0):
        """vkv_propagate_labels: d_out = d_labels[d_nearest] per voxel of `box` (three uint32 arrays of its shape), 0 where d_nearest is
        abi.NEAREST_NONE (or any value >= the box's voxels) or where voxel v of d_mask_volume (None: no mask) is below mask_iso; d_out
        overlaps neither input.  Returns the status code, as nearest_target_rc()."""
        return self._lib.vkv_propagate_labels(self.handle, d_nearest, d_labels, d_out, extent, box, d_mask_volume, mask_iso, stream)

    def geodesic_propagate_rc(self, d_volume, extent, box, iso, d_seeds, steps, limit, rounds, resume, d_scratch, d_dist, d_labels, d_counts, stream=0):
        """vkv_geodesic_propagate: the geodesic distance map of `box` through the inside voxels (>= iso) from the seeds (d_seeds, uint32, the
        box's shape: non-zero = a seed with that label) with the move costs `steps` (seven integers, class |dx| + 2 |dy| + 4 |dz| - 1; 0: no
        such move): d_dist = the least cost below `limit` (None or abi.GEODESIC_NONE: unlimited), abi.GEODESIC_NONE where not reached;
        d_labels = the smallest label at that cost, 0 where not reached; either may be None.  `rounds` rounds (1 .. abi.GEODESIC_MAX_ROUNDS)
        from the seeds (resume False) or from the state that an earlier call left in d_scratch (resume True; d_seeds may be None).  d_counts
        (2 x uint64) = 1 once the state is the fixed point, the reached voxels.  d_scratch: geodesic.scratch_bytes(extent, box) bytes.
        Returns the status code: there is no raising form (the public surface admits new names only as _rc), so callers write
        ctx.check(ctx.geodesic_propagate_rc(...)).  steps None passes NULL and resume may be any integer (error-path tests)."""
        return self._lib.vkv_geodesic_propagate(self.handle, d_volume, extent, box, iso, d_seeds,
                                                None if steps is None else (C.c_uint32 * 7)(*(int(c) for c in steps)),
                                                abi.GEODESIC_NONE if limit is None else int(limit), int(rounds), int(resume), d_scratch, d_dist, d_labels,
                                                d_counts, stream)

    def label_visibility_map_rc(self, d_labels, extent, box, d_colors, table_entries, map_extent, d_map, stream=0):
        """vkv_label_visibility_map: per cell of map_extent 255 where a voxel of the cell grown by one voxel per side carries a visible label
        (d_labels: uint32, the shape of `box`; None: of the volume; d_colors: table_entries colour words, entry L - 1 for label L, alpha 0
        hides), else 0.  Returns the status code: there is no raising form (the public surface admits new names only as _rc), so callers
        write ctx.check(ctx.label_visibility_map_rc(...))."""
        return self._lib.vkv_label_visibility_map(self.handle, d_labels, extent, box, d_colors, int(table_entries), map_extent, d_map, stream)

    def render_labels_rc(self, params, labels, stream=0):
        """vkv_render_labels: the first visible label along each ray of params, coloured by its table entry, with the
        abi.LabelRenderOptions `labels`.  Returns the status code, as label_visibility_map_rc()."""
        return self._lib.vkv_render_labels(self.handle, params, labels, stream)

    def label_mesh_rc(self, d_labels, extent, box, d_colors, table_entries, d_volume, iso, d_visibility_map, map_extent, d_scratch, d_triangles,
                      d_triangle_labels, capacity, d_counts, stream=0):
        """vkv_label_mesh: the surfaces of the visible bodies of d_labels (uint32, the shape of `box`; None: of the volume) as
        marching-tetrahedra triangles in their defined order, each tetrahedron cut once per visible label it touches; d_triangle_labels one
        uint32 label per triangle; d_counts (2 x uint64) = the total and min(total, capacity).  d_colors None with table_entries 0: every
        non-zero label is visible.  d_volume None: vertices at edge midpoints (iso is ignored); else interpolated where the volume crosses
        iso.  d_visibility_map / map_extent None: dense.  d_scratch: labels.mesh_scratch_bytes(extent, box) bytes.  Returns the status
        code, as label_visibility_map_rc()."""
        return self._lib.vkv_label_mesh(self.handle, d_labels, extent, box, d_colors, int(table_entries), d_volume, iso, d_visibility_map,
                                        abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_triangles, d_triangle_labels,
                                        capacity, d_counts, stream)

    def label_mesh_indexed_rc(self, d_labels, extent, box, d_colors, table_entries, d_volume, iso, d_visibility_map, map_extent, d_scratch, d_vertices,
                              d_normals, d_vertex_labels, capacity_vertices, d_indices, d_triangle_labels, capacity_triangles, d_counts, stream=0):
        """vkv_label_mesh_indexed: the surfaces of label_mesh_rc() as a vertex list (one vertex per crossing edge, 3 floats; d_normals None or
        as many gradient normals of d_volume; d_vertex_labels None or two uint32 per vertex, the shown labels on either side) and 3 x uint32
        vertex numbers plus one uint32 label per triangle; d_counts (4 x uint64) = the triangles, those written, the vertices, those written.
        d_scratch: labels.mesh_indexed_scratch_bytes(extent, box) bytes.  Returns the status code, as label_visibility_map_rc()."""
        return self._lib.vkv_label_mesh_indexed(self.handle, d_labels, extent, box, d_colors, int(table_entries), d_volume, iso, d_visibility_map,
                                                abi.Extent3D(0, 0, 0) if map_extent is None else map_extent, d_scratch, d_vertices, d_normals,
                                                d_vertex_labels, capacity_vertices, d_indices, d_triangle_labels, capacity_triangles, d_counts, stream)

    def mesh_adjacency_rc(self, d_indices, capacity_triangles, capacity_vertices, d_counts, d_adjacency, stream=0):
        """vkv_mesh_adjacency: per vertex of an indexed mesh (d_indices: 3 x uint32 per triangle; d_counts: the 4 x uint64 of the indexed
        extractors, read on the device) its neighbour set and its used faces, into d_adjacency (mesh.adjacency_scratch_bytes(capacity_vertices,
        capacity_triangles) bytes); built once per mesh for mesh_smooth_rc() and mesh_vertex_normals_rc().  Returns the status code, as
        label_visibility_map_rc()."""
        return self._lib.vkv_mesh_adjacency(self.handle, d_indices, int(capacity_triangles), int(capacity_vertices), d_counts, d_adjacency, stream)

    def mesh_smooth_rc(self, d_vertices, d_swap, capacity_vertices, d_counts, d_adjacency, d_pinned, factors, stream=0):
        """vkv_mesh_smooth: one uniform-umbrella pass per entry of `factors` (host floats; Taubin: lambda, mu, lambda, mu, ...; None passes NULL
        with zero passes) over the first min(d_counts[3], capacity_vertices) rows of d_vertices, in place; d_swap: as many floats; d_pinned None
        or one byte per vertex, non-zero: the vertex stays.  `factors` may be a (pointer, count) pair (error-path tests).  Returns the status
        code, as label_visibility_map_rc()."""
        if isinstance(factors, tuple):
            array, n = factors
        else:
            n = 0 if factors is None else len(factors)
            array = (C.c_float * n)(*(float(f) for f in factors)) if n else None
        return self._lib.vkv_mesh_smooth(self.handle, d_vertices, d_swap, int(capacity_vertices), d_counts, d_adjacency, d_pinned, array, n, stream)

    def mesh_vertex_normals_rc(self, d_vertices, d_indices, d_triangle_labels, label, capacity_vertices, capacity_triangles, d_counts, d_adjacency,
                               d_normals, stream=0):
        """vkv_mesh_vertex_normals: d_normals (3 floats per vertex) = the area-weighted sum of (p1 - p0) x (p2 - p0) over each vertex's used
        faces, or with d_triangle_labels (not None) over those tagged `label`; not normalised.  d_adjacency: of mesh_adjacency_rc() for the
        same mesh.  Returns the status code, as label_visibility_map_rc()."""
        return self._lib.vkv_mesh_vertex_normals(self.handle, d_vertices, d_indices, d_triangle_labels, int(label), int(capacity_vertices),
                                                 int(capacity_triangles), d_counts, d_adjacency, d_normals, stream)

    def mesh_decimate_rc(self, d_vertices, d_indices, d_triangle_labels, capacity_vertices, capacity_triangles, d_counts, grid_origin, grid_cell,
                         grid_extent, d_scratch, d_out_vertices, out_capacity_vertices, d_out_indices, d_out_triangle_labels, out_capacity_triangles,
                         d_vertex_map, d_out_counts, stream=0):
        """vkv_mesh_decimate: the indexed mesh (d_counts: the 4 x uint64 of the indexed extractors, read on the device) clustered on the grid
        of grid_extent cells of size grid_cell from grid_origin (three host floats each; None passes NULL): one output vertex per cell that a
        surviving face names, the faces whose three cells differ, their labels when d_triangle_labels is given, d_vertex_map (None or one
        uint32 per input vertex) and the four d_out_counts.  d_scratch: mesh_decimate_scratch_bytes() bytes.  Returns the status code, as
        label_visibility_map_rc()."""
        origin = None if grid_origin is None else (C.c_float * 3)(*(float(x) for x in grid_origin))
        cell = None if grid_cell is None else (C.c_float * 3)(*(float(x) for x in grid_cell))
        return self._lib.vkv_mesh_decimate(self.handle, d_vertices, d_indices, d_triangle_labels, int(capacity_vertices), int(capacity_triangles), d_counts,
                                           origin, cell, grid_extent, d_scratch, d_out_vertices, int(out_capacity_vertices), d_out_indices,
                                           d_out_triangle_labels, int(out_capacity_triangles), d_vertex_map, d_out_counts, stream)

    def filter_volume_rc(self, d_src, d_dst, extent, box, kind, stream=0):
        """vkv_filter_volume: the voxels of `box` (None: every voxel) of d_dst = the 3x3x3 filter `kind` (abi.FILTER_*) of d_src"""
        return self._lib.vkv_filter_volume(self.handle, d_src, d_dst, extent, box, int(kind), stream)

    filter_volume = _raising(filter_volume_rc)

    def occupancy_map_from_summary_rc(self, d_summary, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent, d_unresolved=None, stream=0):
        """vkv_occupancy_map_from_summary: vkv_occupancy_map's map, decided from the cell summaries where they are certain; d_unresolved
        receives the number of cells evaluated from their voxels"""
        return self._lib.vkv_occupancy_map_from_summary(self.handle, d_summary, d_volume, d_gradient, d_tf, tf, extent, d_map, map_extent,
                                                        d_unresolved, stream)

    occupancy_map_from_summary = _raising(occupancy_map_from_summary_rc)

    def update_transfer_function_from_summary_rc(self, options, d_volume, d_gradient, extent, d_tf, d_tables, d_maps, d_swap, map_extent, skipping_type,
                                                 d_count, d_summary, d_histogram, d_unresolved=None, stream=0):
        """vkv_update_transfer_function_from_summary: update_transfer_function() with the occupancy from the cell summaries and the count
        (d_count not None) from the histogram"""
        return self._lib.vkv_update_transfer_function_from_summary(self.handle, options, d_volume, d_gradient, extent, d_tf, d_tables,
                                                                   _maps_array(d_maps), d_swap, map_extent, skipping_type, d_count, d_summary,
                                                                   d_histogram, d_unresolved, stream)

    update_transfer_function_from_summary = _raising(update_transfer_function_from_summary_rc)

    def debug_tf_scratch(self, d_out, stream=0):
        """vkv_debug_tf_scratch: the bit table + column mask (2056 words) in `stream`'s scratch block, copied to d_out"""
        self.check(self._lib.vkv_debug_tf_scratch(self.handle, d_out, stream))

    def occupied_voxel_count(self, d_volume, d_gradient, tf, extent, d_count, stream=0):
        self.check(self._lib.vkv_occupied_voxel_count(self.handle, d_volume, d_gradient, tf, extent, d_count, stream))

    def convert_volume(self, d_raw, voxel_type, big_endian, range_min, range_max, n_voxels, d_out, stream=0):
        self.check(self._lib.vkv_convert_volume(self.handle, d_raw, voxel_type, 1 if big_endian else 0, range_min, range_max, n_voxels, d_out, stream))


# ---- host helpers (no device needed) --------------------------------------------------------------

def _host_call(symbol, *args):
    """an entry point that takes no context, so has no vkv_last_error: VkvError(status, symbol) unless it returns 0"""
    rc = getattr(load(), symbol)(*args)
    if rc != 0:
        raise VkvError(rc, symbol)


def transfer_function_uniform(options):
    out = abi.TransferFunctionUniform()
    _host_call("vkv_transfer_function_uniform", options, C.byref(out))
    return out


def transfer_function_texture(options):
    import numpy as np
    tex = np.zeros((256, 256, 4), np.uint8)
    _host_call("vkv_transfer_function_texture", options, tex.ctypes.data_as(C.c_void_p))
    return tex


def build_uniforms(view, proj, node_transform, image_transform, clip_distance, image_size, volume_extent, map_extent):
    import numpy as np
    cam, rc_, rg = abi.CameraUniform(), abi.RayCastUniform(), abi.RayGen()
    mats = [np.ascontiguousarray(m, np.float32).reshape(16) for m in (view, proj, node_transform, image_transform)]
    _host_call("vkv_build_uniforms", *[m.ctypes.data_as(C.c_void_p) for m in mats], clip_distance, image_size[0], image_size[1], volume_extent,
               map_extent, C.byref(cam), C.byref(rc_), C.byref(rg))
    return cam, rc_, rg


def screen_tile_rect(ray_cast, ray_gen, image_size, tile_size=(16, 16), align_tiles=1):
    """vkv_screen_tile_rect: the tile rectangle the fragments of a frame with these uniforms can lie in (pure CPU; every rank derives the same)"""
    out = abi.TileRect()
    _host_call("vkv_screen_tile_rect", ray_cast, ray_gen, image_size[0], image_size[1], tile_size[0], tile_size[1], align_tiles, C.byref(out))
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
    rc = load().vkv_load_data(os.fsencode(path), header, out.ctypes.data_as(C.c_void_p), out.nbytes)
    if rc != 0:
        raise RuntimeError("load_data failed (%d)" % rc)
    return out


# the four scratch sizes: a size_t result comes back as an int, and `box` None is NULL
def mesh_scratch_bytes(extent, box=None):
    """vkv_isosurface_mesh_scratch_bytes: the scratch vkv_isosurface_mesh needs for `box` (None: the whole volume) of `extent`; 0 for an extent
    or box the call rejects"""
    return load().vkv_isosurface_mesh_scratch_bytes(extent, box)


def components_scratch_bytes(extent, box=None):
    """vkv_label_components_scratch_bytes: the scratch vkv_label_components needs for `box` (None: the whole volume) of `extent`; 0 for an
    extent or box the call rejects (a box of more than 2^32 - 1 voxels included)"""
    return load().vkv_label_components_scratch_bytes(extent, box)


def distance_transform_scratch_bytes(extent, box=None):
    """vkv_distance_transform_scratch_bytes: the scratch vkv_distance_transform needs for `box` (None: the whole volume) of `extent`: 4 bytes
    per voxel and 8 per 64 voxels; 0 for an extent or box the call rejects (more than 2^32 - 1 voxels or an axis above 32768 included)"""
    return load().vkv_distance_transform_scratch_bytes(extent, box)


def mesh_indexed_scratch_bytes(extent, box=None):
    """vkv_isosurface_mesh_indexed_scratch_bytes: the scratch vkv_isosurface_mesh_indexed needs for `box` (None: the whole volume) of `extent`;
    0 for an extent or box the call rejects"""
    return load().vkv_isosurface_mesh_indexed_scratch_bytes(extent, box)

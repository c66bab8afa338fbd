"""ctypes/numpy front-end of ``oracle/_ref/libvkv_ref.so``: the reference's OWN compute shaders and fragment shader, compiled as C++ for the CPU
by ``make -C oracle ref`` (oracle/glsl_host/).  The library exists only where the reference's sources were present at build time; it is
never committed.  ``available()`` says whether it is there.  Same array conventions as ``vkv_oracle.py``.

TEST INFRASTRUCTURE ONLY: tests/test_reference_text_cpu.py pins the oracle to it, tests/golden/make_reference_vectors.py records its outputs.
"""
import ctypes as C
import os

import numpy as np

from vkvolume_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(_HERE, "_ref", "libvkv_ref.so")
_LIB = None

PLAIN, PINNED = 0, 1  # the two arithmetic modes of oracle/glsl_host/glsl_shim.hpp
SHOW_NONE, SHOW_RAY_ENTRY, SHOW_RAY_EXIT = 0, 1, 2


class TransferFunction(C.Structure):
    """VkvRefTransferFunction (oracle/glsl_host/harness.hpp)"""
    _fields_ = [("sampling_factor", C.c_float), ("voxel_alpha_factor", C.c_float), ("grad_magnitude_modifier", C.c_float),
                ("use_gradient", C.c_uint32)]


class FragArgs(C.Structure):
    """VkvRefFragArgs (oracle/glsl_host/harness.hpp)"""
    _fields_ = [("entry", C.c_void_p), ("in_depth", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("view", C.c_float * 16), ("proj", C.c_float * 16), ("view_proj_inv", C.c_float * 16), ("model", C.c_float * 16),
                ("model_inv", C.c_float * 16), ("cam_pos_tex", C.c_float * 4), ("block_size", C.c_float * 4), ("tf", TransferFunction),
                ("volume", C.c_void_p), ("gradient", C.c_void_p), ("tf_rgba8", C.c_void_p), ("extent", C.c_int32 * 3),
                ("maps", C.c_void_p * 8), ("map_extent", C.c_int32 * 3), ("out_color", C.c_void_p), ("out_counts", C.c_void_p),
                ("out_depth", C.c_void_p), ("out_fragment", C.c_void_p)]


def available():
    return os.path.exists(PATH)


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(PATH)
        vp, i3 = C.c_void_p, C.POINTER(C.c_int32)
        L.vkv_ref_set_mode.argtypes = [C.c_int]
        L.vkv_ref_has_frag.argtypes = [C.c_int]
        L.vkv_ref_gradient_map.argtypes = [vp, vp, i3, C.POINTER(TransferFunction), vp]
        L.vkv_ref_occupancy_map.argtypes = [vp, vp, vp, C.POINTER(TransferFunction), i3, vp, i3]
        L.vkv_ref_distance_map.argtypes = [vp, vp, i3]
        L.vkv_ref_distance_map_anisotropic.argtypes = [C.POINTER(vp), vp, i3]
        L.vkv_ref_frag.argtypes = [C.c_int, C.POINTER(FragArgs)]
        _LIB = L
    return _LIB


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _extent(a):
    d, h, w = a.shape
    return (C.c_int32 * 3)(w, h, d)


def _tf(tf):
    return TransferFunction(tf.sampling_factor, tf.voxel_alpha_factor, tf.grad_magnitude_modifier, tf.use_gradient)


def set_mode(mode):
    lib().vkv_ref_set_mode(mode)


def gradient_map(vol, tf, tf_tex=None):
    """gradient_map.comp over vol uint8 [D,H,W] -> uint8 [D,H,W]"""
    vol = np.ascontiguousarray(vol, np.uint8)
    grad = np.full_like(vol, 0xA5)  # every byte must be written
    tex = np.zeros((256, 256, 4), np.uint8) if tf_tex is None else np.ascontiguousarray(tf_tex, np.uint8)  # declared by the shader, never sampled
    lib().vkv_ref_gradient_map(_ptr(vol), _ptr(grad), _extent(vol), C.byref(_tf(tf)), _ptr(tex))
    return grad


def occupancy_map(vol, grad, tf_tex, tf, block, map_extent_override=None):
    """occupancy_map.comp (its PRECOMPUTED_GRADIENT variant when `grad` is given) with the host's block size and dispatch"""
    vol = np.ascontiguousarray(vol, np.uint8)
    grad = None if grad is None else np.ascontiguousarray(grad, np.uint8)
    tex = np.ascontiguousarray(tf_tex, np.uint8)
    d, h, w = vol.shape
    me = map_extent_override.as_tuple() if map_extent_override is not None else tuple((v + block - 1) // block for v in (w, h, d))
    out = np.full((me[2], me[1], me[0]), 0xA5, np.uint8)
    lib().vkv_ref_occupancy_map(_ptr(vol), _ptr(grad), _ptr(tex), C.byref(_tf(tf)), _extent(vol), _ptr(out), _extent(out))
    return out


def distance_map(occ):
    """distance_map.comp, three dispatches, in place"""
    m = np.ascontiguousarray(occ, np.uint8).copy()
    swap = np.zeros_like(m)
    lib().vkv_ref_distance_map(_ptr(m), _ptr(swap), _extent(m))
    return m


def distance_map_anisotropic(occ):
    """distance_map_anisotropic.comp, fourteen dispatches -> uint8 [8,md,mh,mw]"""
    occ = np.ascontiguousarray(occ, np.uint8)
    maps = np.zeros((8,) + occ.shape, np.uint8)
    maps[7] = occ
    swap = np.zeros_like(occ)
    ptrs = (C.c_void_p * 8)(*[maps[i].ctypes.data for i in range(8)])
    lib().vkv_ref_distance_map_anisotropic(ptrs, _ptr(swap), _extent(occ))
    return maps


def compute_distance_map(vol, grad, tf_tex, tf, block, skipping_type):
    """ComputeDistanceMap::compute: occupancy, then the transform of the skipping type -> [n_maps, md, mh, mw]"""
    occ = occupancy_map(vol, grad, tf_tex, tf, block)
    if skipping_type == abi.SKIP_BLOCK:
        return occ[None].copy()
    if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE:
        return distance_map_anisotropic(occ)
    return distance_map(occ)[None].copy()


def frag_key(skipping_type, early_ray_termination, precomputed_gradient, depth_attachment, show=SHOW_NONE):
    return skipping_type | ((0 if early_ray_termination else 1) << 2) | ((1 if precomputed_gradient else 0) << 3) | \
        ((1 if depth_attachment else 0) << 4) | (show << 5)


class FragResult:
    def __init__(self, color, counts, depth, fragment):
        self.color, self.counts, self.depth, self.fragment = color, counts, depth, fragment


def frag(params, entry, vol, grad, tf_tex, maps, in_depth=None, show=SHOW_NONE, mode=PINNED):
    """volume_render.frag for every pixel with entry[..., 3] > 0.  `params`: the abi.RenderParams of the frame (uniforms and options: the
    #define variant follows from options and use_precomputed_gradient); `entry`: float32 [h, w, 4], rgb = the interpolant ray_entry."""
    o = params.options
    precomputed = bool(params.use_precomputed_gradient) and grad is not None
    key = frag_key(o.skipping_type, bool(o.early_ray_termination), precomputed, bool(o.depth_attachment), show)
    assert lib().vkv_ref_has_frag(key), "variant %d was not built" % key
    entry = np.ascontiguousarray(entry, np.float32)
    h, w = entry.shape[:2]
    vol, tex = np.ascontiguousarray(vol, np.uint8), np.ascontiguousarray(tf_tex, np.uint8)
    a = FragArgs()
    keep = [entry, vol, tex]
    a.entry, a.width, a.height = entry.ctypes.data, w, h
    if o.depth_attachment:
        in_depth = np.ascontiguousarray(in_depth, np.float32)
        keep.append(in_depth)
        a.in_depth = in_depth.ctypes.data
    cam = params.camera
    for dst, src in ((a.view, cam.camera_view), (a.proj, cam.camera_proj), (a.view_proj_inv, cam.camera_view_proj_inv), (a.model, cam.model),
                     (a.model_inv, cam.model_inv)):
        for i in range(16):
            dst[i] = src[i]
    for i in range(4):
        a.cam_pos_tex[i], a.block_size[i] = params.ray_cast.camera_pos_tex[i], params.ray_cast.block_size[i]
    a.tf = _tf(params.transfer_function)
    a.volume, a.tf_rgba8, a.extent = vol.ctypes.data, tex.ctypes.data, _extent(vol)
    if precomputed:
        grad = np.ascontiguousarray(grad, np.uint8)
        keep.append(grad)
        a.gradient = grad.ctypes.data
    if o.skipping_type != abi.SKIP_NONE:
        for i in range(len(maps)):
            m = np.ascontiguousarray(maps[i], np.uint8)
            keep.append(m)
            a.maps[i] = m.ctypes.data
        a.map_extent = _extent(maps[0])
    color, counts = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 3), np.uint32)
    depth, fragment = np.zeros((h, w), np.float32), np.zeros((h, w), np.uint8)
    a.out_color, a.out_counts, a.out_depth, a.out_fragment = color.ctypes.data, counts.ctypes.data, depth.ctypes.data, fragment.ctypes.data
    set_mode(mode)
    try:
        rc = lib().vkv_ref_frag(key, C.byref(a))
    finally:
        set_mode(PINNED)
    assert rc == 0
    del keep
    return FragResult(color, counts, depth, fragment.astype(bool))

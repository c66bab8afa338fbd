"""CPU: the device-side transfer-function update (vkv_transfer_function_texture_device, vkv_update_transfer_function) is declared, exported
and bound, and the column-mask claim its kernel is built on holds for the host texture: column i of the 256x256 texture has an occupied
texel iff (uint8) (a_i[i] * max_g a_g[g] * 255) > 0."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from vkvolume_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vkv_transfer_function_texture_device", "vkv_update_transfer_function"]


def option_sets(n_random=200, seed=0x7F0):
    """The option sets both TF-update test files run: the app's TF, defaults, gradient off, a narrow and an inverted window, a degenerate
    intensity window (a slider can reach it) and `n_random` seeded random sets - windows of any sign and width, degenerate ones on texel
    centres (where the host product is NaN), the gradient switched off now and then."""
    sets = [("app", T.APP_TF), ("defaults", {}), ("gradient_off", dict(intensity_min=0.2, intensity_max=0.7, gradient_min=0.3, gradient_max=0.3)),
            ("narrow", dict(intensity_min=0.5, intensity_max=0.505, gradient_min=0.1, gradient_max=0.11)),
            ("inverted", dict(intensity_min=0.8, intensity_max=0.3, gradient_min=0.4, gradient_max=0.05)),
            ("degenerate", dict(intensity_min=0.5, intensity_max=0.5)),
            ("degenerate_on_texel", dict(intensity_min=np.float32(100) / np.float32(255), intensity_max=np.float32(100) / np.float32(255),
                                         gradient_min=0.0, gradient_max=0.2))]
    rng = np.random.default_rng(seed)
    for k in range(n_random):
        imin = float(rng.uniform(-0.3, 1.2))
        r = rng.random()
        if r < 0.1:
            imin = float(np.float32(rng.integers(0, 256)) / np.float32(255))
            imax = imin
        elif r < 0.2:
            imax = imin + float(rng.choice([1e-3, -1e-3, 1e-6]))
        else:
            imax = imin + float(rng.uniform(-1.0, 1.2))
        gmin = float(rng.uniform(-0.2, 0.8))
        gmax = gmin if rng.random() < 0.15 else gmin + float(rng.uniform(-0.6, 0.9))
        sets.append(("random%d" % k, dict(intensity_min=imin, intensity_max=imax, gradient_min=gmin, gradient_max=gmax,
                                          sampling_factor=float(rng.uniform(0.5, 3.0)), voxel_alpha_factor=float(rng.uniform(0.1, 1.0)))))
    return sets


def axis_alpha(lo, inv):
    """The kernel's a_i / a_g (k_tf_tables_init's arithmetic) in float32: comparison clamps, NaN passes through."""
    x = np.arange(256, dtype=np.float32) / np.float32(255.0)
    with np.errstate(invalid="ignore", over="ignore"):
        a = (x - np.float32(lo)) * np.float32(inv)
    a = np.where(a < np.float32(0), np.float32(0), a)
    return np.where(np.float32(1) < a, np.float32(1), a).astype(np.float32)


def test_new_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    debug = open(os.path.join(ROOT, "include", "vkvolume_amd_debug.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in lib.EXPORTS
    assert re.search(r"\bint\s+vkv_debug_tf_scratch\s*\(", debug) and "vkv_debug_tf_scratch" in lib.DEBUG_EXPORTS
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in NEW + ["vkv_debug_tf_scratch"]:
        assert re.search(r"\b%s$" % name, out, flags=re.M), name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.vkv_transfer_function_texture_device.argtypes) == 5
    assert len(L.vkv_update_transfer_function.argtypes) == 13
    assert L.vkv_update_transfer_function.argtypes[4] is abi.Extent3D and L.vkv_update_transfer_function.argtypes[9] is abi.Extent3D
    assert L.vkv_update_transfer_function.argtypes[10] is C.c_int32


def test_argument_errors_need_no_device():
    """A null context is refused before anything touches the HIP runtime."""
    L = lib.load()
    opt = abi.VolumeOptions()
    assert L.vkv_transfer_function_texture_device(None, C.byref(opt), None, None, None) == abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_update_transfer_function(None, C.byref(opt), None, None, abi.Extent3D(4, 4, 4), None, None, None, None, abi.Extent3D(1, 1, 1),
                                          abi.SKIP_DISTANCE, None, None) == abi.VKV_E_INVALID_ARGUMENT


@pytest.mark.parametrize("name,opts", option_sets(), ids=[n for n, _ in option_sets()])
def test_column_mask_from_the_largest_gradient_alpha(name, opts):
    o = abi.VolumeOptions(**opts)
    tex = lib.transfer_function_texture(o)
    assert np.array_equal(tex[..., 0], tex[..., 3]) and np.array_equal(tex[..., 1], tex[..., 3]) and np.array_equal(tex[..., 2], tex[..., 3])
    columns = (tex[..., 3] > 0).any(axis=0)  # what k_tf_columns ORs out of the bit table
    u = lib.transfer_function_uniform(o)
    ai = axis_alpha(u.intensity_min, u.intensity_range_inv)
    ag = axis_alpha(u.gradient_min, u.gradient_range_inv) if u.use_gradient else np.ones(256, np.float32)
    ag_max = np.float32(np.nanmax(ag)) if not np.isnan(ag).all() else np.float32(0)
    with np.errstate(invalid="ignore"):
        p = (ai * ag_max) * np.float32(255.0)
        claim = np.where(np.isnan(p), 0, np.trunc(np.nan_to_num(p))) > 0
    assert np.array_equal(claim, columns), "columns %s" % np.nonzero(claim != columns)[0]
    # the texel itself is the separable product with NaN -> 0 (the device's definition of the degenerate window)
    with np.errstate(invalid="ignore"):
        prod = (ai[None, :] * ag[:, None]) * np.float32(255.0)
    expect = np.where(np.isnan(prod), 0, np.trunc(np.nan_to_num(prod))).astype(np.uint8)
    assert np.array_equal(expect, tex[..., 3])

"""The definitions of vkv_distance_transform and vkv_select_by_distance (include/vkvolume_amd.h) restated in numpy, twice:
edt2_brute_np() (brute force over the target voxels) and edt2_np() (a min-plus pass per axis, the kernels' own decomposition), and
select_by_distance_np(); and what can be shown of them without a GPU.  Both statements are scipy.ndimage.distance_transform_edt squared
(read exactly, through return_indices) wherever a target exists and the definition (`limit` everywhere) where none does, which scipy leaves
undefined; erosion and dilation by the select ranges of the header are scipy's binary_erosion(border_value=1) and binary_dilation with the
ball for r^2 in {1, 2, 3, 4, 9, 10}, opening and closing the composed calls; Volume.ball_radius2 is floor(radius^2); the entry points are
declared, exported and bound, the scratch formula is the header's and within the issue's bound, and the kernels of edt.hip use no scratch
memory.  tests/test_gpu_distance.py holds the kernels to edt2_np() and select_by_distance_np() bit for bit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_components_cpu import inside_np
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xffffffff
TO_INSIDE, TO_OUTSIDE = 0, 1
RADII2 = (1, 2, 3, 4, 9, 10)


def targets_np(vol_dhw, iso, target, box=None):
    """the target voxels of the box (x0, y0, z0, w, h, d): its inside voxels (the mesh's rule) or its outside ones"""
    inside = inside_np(vol_dhw, iso, box)
    return inside if target == TO_INSIDE else ~inside


def edt2_brute_np(vol_dhw, iso, target=TO_INSIDE, limit=None, box=None):
    """d_dist2 [d, h, w] uint32 of the header's sentence: min(limit, min over the target voxels u of the box of |v - u|^2), by brute force
    over the target voxels in int64; limit None: VKV_DISTANCE_NONE.  Targets x voxels work: for small volumes"""
    limit = NONE if limit is None else int(limit)
    t = targets_np(vol_dhw, iso, target, box)
    best = np.full(t.shape, limit, np.int64)
    zz, yy, xx = np.indices(t.shape, dtype=np.int64, sparse=True)
    pts = np.argwhere(t)
    step = max(1, (1 << 22) // max(t.size, 1))        # blocks of targets: [block, d, h, w] stays small
    for k in range(0, len(pts), step):
        p = pts[k:k + step].astype(np.int64)
        d2 = ((zz[None] - p[:, 0, None, None, None]) ** 2 + (yy[None] - p[:, 1, None, None, None]) ** 2 + (xx[None] - p[:, 2, None, None, None]) ** 2)
        best = np.minimum(best, d2.min(axis=0))
    return best.astype(np.uint32)


def edt2_np(vol_dhw, iso, target=TO_INSIDE, limit=None, box=None):
    """the same values one axis after the other (axis length x voxels work: the reference of the GPU tests): g = the squared distance
    along x (none: a value above every sum), then out(p) = min over p' of g(p') + (p - p')^2 along y and along z, capped at the end;
    int64, so nothing wraps"""
    limit = NONE if limit is None else int(limit)
    t = targets_np(vol_dhw, iso, target, box)
    far = np.int64(1) << 40
    g = np.where(t, 0, far).astype(np.int64)
    for axis in (2, 1, 0):
        n = g.shape[axis]
        out = g.copy()
        for d in range(1, n):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            lo, hi = tuple(lo), tuple(hi)
            out[hi] = np.minimum(out[hi], g[lo] + d * d)
            out[lo] = np.minimum(out[lo], g[hi] + d * d)
        g = out
    return np.minimum(g, limit).astype(np.uint32)


def select_by_distance_np(src_dhw, dist2, lo, hi, fill, box=None, dst=None):
    """vkv_select_by_distance: `dst` (None: a copy of src) with the box's voxels written"""
    src = np.ascontiguousarray(src_dhw, np.uint8)
    out = src.copy() if dst is None else dst.copy()
    x0, y0, z0, w, h, d = (0, 0, 0) + src.shape[::-1] if box is None else box
    assert dist2.shape == (d, h, w) and dist2.dtype == np.uint32
    sub = src[z0:z0 + d, y0:y0 + h, x0:x0 + w].copy()
    sub[(dist2 >= lo) & (dist2 <= hi)] = fill
    out[z0:z0 + d, y0:y0 + h, x0:x0 + w] = sub
    return out


def erode_np(vol, iso, r2, fill=0, box=None):
    return select_by_distance_np(vol, edt2_np(vol, iso, TO_OUTSIDE, r2 + 1, box), 1, r2, fill, box)


def dilate_np(vol, iso, r2, fill=255, box=None):
    return select_by_distance_np(vol, edt2_np(vol, iso, TO_INSIDE, r2 + 1, box), 1, r2, fill, box)


def ball_structure(r2):
    r = int(np.floor(np.sqrt(r2)))
    z, y, x = np.indices((2 * r + 1,) * 3) - r
    return z * z + y * y + x * x <= r2


def random_mask_volume(rng, shape, density):
    return np.where(rng.random(shape) < density, 200, 17).astype(np.uint8)


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def scipy_edt2(targets):
    """scipy's EDT to the nearest True voxel, squared from the returned indices: exact integers"""
    from scipy import ndimage
    idx = ndimage.distance_transform_edt(~targets, return_distances=False, return_indices=True)
    grid = np.indices(targets.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(axis=0)


@pytest.mark.parametrize("target", [TO_INSIDE, TO_OUTSIDE])
def test_both_statements_are_scipys_edt_squared(target):
    rng = np.random.default_rng(11 + target)
    for k in range(40):
        shape = tuple(int(s) for s in rng.integers(1, 12, size=3))
        density = (0.02, 0.1, 0.5, 0.9)[k % 4]
        vol = random_mask_volume(rng, shape, density)
        t = targets_np(vol, 0.5, target)
        for limit in (None, 1, 2, 9, 10, 100000):
            a, b = edt2_brute_np(vol, 0.5, target, limit), edt2_np(vol, 0.5, target, limit)
            assert a.dtype == np.uint32 and a.shape == shape and np.array_equal(a, b), (shape, density, limit)
            cap = NONE if limit is None else limit
            if t.any():
                assert np.array_equal(a, np.minimum(scipy_edt2(t), cap)), (shape, density, limit)
            else:
                assert (a == cap).all()        # scipy is undefined here; the definition is not
            assert np.array_equal(a == 0, t)


def test_no_target_gives_the_limit_everywhere_and_a_single_target_its_offsets():
    vol = np.full((3, 4, 5), 17, np.uint8)
    for limit, cap in ((None, NONE), (1, 1), (7, 7)):
        for f in (edt2_brute_np, edt2_np):
            assert (f(vol, 0.5, TO_INSIDE, limit) == cap).all() and (f(vol, 0.5, TO_OUTSIDE, limit) == 0).all()
    vol[2, 3, 4] = 200
    z, y, x = np.indices(vol.shape)
    want = (z - 2) ** 2 + (y - 3) ** 2 + (x - 4) ** 2
    for f in (edt2_brute_np, edt2_np):
        assert np.array_equal(f(vol, 0.5), want) and np.array_equal(f(vol, 0.5, limit=6), np.minimum(want, 6))


def test_a_box_is_transformed_as_the_cropped_array():
    vol = random_mask_volume(np.random.default_rng(5), (7, 8, 9), 0.1)
    box = (2, 1, 3, 5, 6, 3)
    crop = np.ascontiguousarray(vol[3:6, 1:7, 2:7])
    for target in (TO_INSIDE, TO_OUTSIDE):
        got = edt2_np(vol, 0.5, target, None, box)
        assert got.shape == (3, 6, 5) and np.array_equal(got, edt2_np(crop, 0.5, target)) and np.array_equal(got, edt2_brute_np(vol, 0.5, target, None, box))
    lonely = np.full((4, 4, 4), 17, np.uint8)
    lonely[0, 0, 0] = 200        # the only target lies outside the box: every element is the limit
    assert (edt2_np(lonely, 0.5, TO_INSIDE, 50, (1, 1, 1, 3, 3, 3)) == 50).all() and (edt2_np(lonely, 0.5, TO_INSIDE, None, (1, 1, 1, 3, 3, 3)) == NONE).all()


def test_the_inside_rule_is_the_meshes():
    from tests.test_mesh_cpu import KINV255
    vol = np.arange(256, dtype=np.uint8).reshape(1, 1, 256)
    for iso in (0.0, 0.2, 0.5, 128 * float(KINV255), 1.0, 1.5, -1.0):
        thr = next((b for b in range(256) if np.float32(b) * KINV255 >= np.float32(iso)), 256)
        assert np.array_equal(edt2_np(vol, iso, TO_INSIDE, 1)[0, 0] == 0, np.arange(256) >= thr)
        assert np.array_equal(edt2_np(vol, iso, TO_OUTSIDE, 1)[0, 0] == 0, np.arange(256) < thr)


def test_select_by_distance_np():
    vol = np.arange(10, dtype=np.uint8).reshape(1, 1, 10) + 100
    d2 = np.array([0, 1, 4, 9, 16, 9, 4, 1, 0, NONE], np.uint32).reshape(1, 1, 10)
    assert select_by_distance_np(vol, d2, 1, 4, 7)[0, 0].tolist() == [100, 7, 7, 103, 104, 105, 7, 7, 108, 109]
    assert select_by_distance_np(vol, d2, 0, NONE, 7)[0, 0].tolist() == [7] * 10
    assert np.array_equal(select_by_distance_np(vol, d2, 17, NONE - 1, 7), vol)
    fresh = np.full((1, 1, 10), 0xA5, np.uint8)
    out = select_by_distance_np(vol, d2[:, :, 2:5], 9, 9, 7, box=(2, 0, 0, 3, 1, 1), dst=fresh)
    assert out[0, 0].tolist() == [0xA5, 0xA5, 102, 7, 104] + [0xA5] * 5


# ---- morphology -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r2", RADII2)
def test_erosion_and_dilation_are_scipys_with_the_ball(r2):
    from scipy import ndimage
    ball = ball_structure(r2)
    assert ball.sum() == {1: 7, 2: 19, 3: 27, 4: 33, 9: 123, 10: 147}[r2]
    rng = np.random.default_rng(r2)
    for k in range(12):
        shape = tuple(int(s) for s in rng.integers(1, 14, size=3))
        vol = random_mask_volume(rng, shape, (0.05, 0.5, 0.95)[k % 3])
        inside = vol >= 128
        assert np.array_equal(erode_np(vol, 0.5, r2) >= 128, ndimage.binary_erosion(inside, structure=ball, border_value=1)), (shape, "erode")
        assert np.array_equal(dilate_np(vol, 0.5, r2) >= 128, ndimage.binary_dilation(inside, structure=ball)), (shape, "dilate")
        opened, closed = dilate_np(erode_np(vol, 0.5, r2), 0.5, r2), erode_np(dilate_np(vol, 0.5, r2), 0.5, r2)
        assert np.array_equal(opened >= 128, ndimage.binary_dilation(ndimage.binary_erosion(inside, structure=ball, border_value=1), structure=ball)), shape
        assert np.array_equal(closed >= 128, ndimage.binary_erosion(ndimage.binary_dilation(inside, structure=ball), structure=ball, border_value=1)), shape
        # only the voxels that change sides are written; the others keep their bytes
        e = erode_np(vol, 0.5, r2, fill=3)
        assert set(np.unique(e)) <= {3, 17, 200} and np.array_equal(e == 3, inside & ~(erode_np(vol, 0.5, r2) >= 128))


def test_radius_to_radius2_rule():
    f = V.Volume.ball_radius2
    assert [f(radius=r) for r in (1, 1.0, np.sqrt(2), 1.5, np.sqrt(3), 2, 3, 3.2, 10)] == [1, 1, 2, 2, 2, 4, 9, 10, 100]        # sqrt(3)^2 = 2.9999999999999996
    assert f(radius=1.7320508075688774) == 3 and f(radius=1.42) == 2 and f(radius2=10) == 10 and f(radius2=1) == 1
    for kw in (dict(), dict(radius=1, radius2=1), dict(radius=0.5), dict(radius=-2), dict(radius2=0), dict(radius2=2.5), dict(radius=float("nan")), dict(radius2=NONE)):
        with pytest.raises(ValueError):
            f(**kw)


# ---- entry points ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"#define\s+VKV_DISTANCE_NONE\s+0xffffffffu\b", header)
    assert re.search(r"enum\s+VkvDistanceTarget\s*\{\s*VKV_DISTANCE_TO_INSIDE\s*=\s*0,\s*VKV_DISTANCE_TO_OUTSIDE\s*=\s*1\s*\}", header)
    assert (abi.DISTANCE_TO_INSIDE, abi.DISTANCE_TO_OUTSIDE, abi.DISTANCE_NONE) == (0, 1, NONE)
    assert re.search(r"\bsize_t\s+vkv_distance_transform_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_distance_transform\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*float iso,\s*"
                     r"int32_t target,\s*uint32_t limit,\s*void\s*\*d_scratch,\s*uint32_t\s*\*d_dist2,\s*void\s*\*stream\)", header)
    assert re.search(r"\bint\s+vkv_select_by_distance\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_src,\s*uint8_t\s*\*d_dst,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"const uint32_t\s*\*d_dist2,\s*uint32_t lo,\s*uint32_t hi,\s*uint32_t fill,\s*void\s*\*stream\)", header)
    assert "max_map" not in header[header.index("exact Euclidean distance transform"):header.index("#define VKV_DISTANCE_NONE")]        # no max-map option
    L = lib.load()
    names = {"vkv_distance_transform", "vkv_distance_transform_scratch_bytes", "vkv_select_by_distance"}
    assert names <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert all(re.search(r"\b%s$" % n, out, flags=re.M) for n in names)
    at = L.vkv_distance_transform.argtypes
    assert len(at) == 10 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[5] is C.c_int32 and at[6] is C.c_uint32
    at = L.vkv_select_by_distance.argtypes
    assert len(at) == 10 and at[3] is abi.Extent3D and at[6] is C.c_uint32 and at[7] is C.c_uint32 and at[8] is C.c_uint32
    assert L.vkv_distance_transform_scratch_bytes.restype is C.c_size_t
    assert callable(lib.Context.distance_transform) and callable(lib.Context.distance_transform_rc)
    assert callable(lib.Context.select_by_distance) and callable(lib.Context.select_by_distance_rc)
    assert callable(lib.distance_transform_scratch_bytes) and callable(V.Volume.distance_transform)
    assert all(callable(getattr(V.Volume, n)) for n in ("erode", "dilate", "open", "close"))


def test_scratch_bytes_and_bad_arguments_without_a_device():
    L = lib.load()
    for extent in ((1, 1, 1), (64, 1, 1), (65, 1, 1), (258, 5, 19), (2, 66, 65), (1024, 1024, 795), (32768, 1, 1), (1, 32768, 3), (2, 2, 32768)):
        w, h, d = extent
        n = w * h * d
        want = 4 * n + 8 * ((n + 63) // 64)        # the header's formula
        got = lib.distance_transform_scratch_bytes(abi.Extent3D(w, h, d))
        assert got == want and want % 4 == 0 and want <= 4 * n + n // 8 + 8, extent        # 4 B and one bit per voxel, plus a constant
    e = abi.Extent3D(258, 5, 19)
    assert 40 == lib.distance_transform_scratch_bytes(e, abi.Box(1, 1, 1, 2, 2, 2)) < lib.distance_transform_scratch_bytes(e)
    assert lib.distance_transform_scratch_bytes(abi.Extent3D(0, 5, 19)) == 0
    assert lib.distance_transform_scratch_bytes(e, abi.Box(257, 0, 0, 2, 1, 1)) == 0 and lib.distance_transform_scratch_bytes(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    for too_long in (abi.Extent3D(32769, 1, 1), abi.Extent3D(1, 32769, 1), abi.Extent3D(1, 1, 32769), abi.Extent3D(0xffffffff, 1, 1)):
        assert lib.distance_transform_scratch_bytes(too_long) == 0        # an axis above 32768
    assert lib.distance_transform_scratch_bytes(abi.Extent3D(32769, 4, 4), abi.Box(1, 0, 0, 32768, 4, 4)) == 4 * (1 << 19) + (1 << 16)        # the BOX's axes count
    big = abi.Extent3D(32768, 32768, 4)        # 2^32 voxels: one too many
    assert lib.distance_transform_scratch_bytes(big) == 0 and lib.distance_transform_scratch_bytes(abi.Extent3D(32768, 32768, 3)) > 0
    assert lib.distance_transform_scratch_bytes(big, abi.Box(5, 5, 0, 3, 3, 2)) == 4 * 18 + 8
    buf = (C.c_uint64 * 128)()
    a = C.addressof(buf)
    bad = abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_distance_transform(None, a, abi.Extent3D(4, 4, 4), None, 0.5, 0, 5, a + 64, a + 512, None) == bad
    assert L.vkv_select_by_distance(None, a, a, abi.Extent3D(4, 4, 4), None, a + 512, 1, 4, 0, None) == bad
    assert not any(buf)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("edt.hip", tmp_path / "edt.s")
    for name in ("k_edt_bits", "k_edt_x", "k_edt_axis", "k_edt_select"):
        assert len([k for k in kernels if name in k]) == 1, sorted(kernels)
    assert len(kernels) == 4
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)
    # the row walk is edt_passes.hpp's: no more registers than the copy it replaced had
    assert [v["NumVgprs"] for k, v in kernels.items() if "k_edt_x" in k][0] <= 18, kernels


def test_the_pass_schedule_tiles_the_scratch_block_and_ends_in_the_callers_buffer_under_asan_and_ubsan(tmp_path):
    """EdtSchedule, which vkv_distance_transform_scratch_bytes and the launchers of the three exact transforms share: its size against
    8 entries + 4 n, its pointers against the size, the passes' buffers in all four combinations of (y runs, z runs), and the boxes it rejects
    (tests/edt_schedule_driver.cpp, the header's host pass: no GPU, no kernel)"""
    hipcc = T.HIPCC if os.path.exists(T.HIPCC) else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path / "edt_schedule_driver"
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-I", T.CSRC, os.path.join(ROOT, "tests", "edt_schedule_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "edt schedule ok", r.stdout[-2000:]

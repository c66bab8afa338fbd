"""The definition of vkv_distance_transform_weighted (include/vkvolume_amd.h) restated in numpy, twice:
edt2_weighted_brute_np() (brute force over the target voxels) and edt2_weighted_np() (a min-plus pass per axis with (w d)^2, the reference of
tests/test_gpu_distance_weighted.py), both scipy.ndimage.distance_transform_edt(sampling=weights) squared (read exactly, through
return_indices) and, with weights (1, 1, 1), tests/test_distance_cpu.py's edt2_np; the kernel's envelope pass restated in Python
(tests/edt_envelope_ref.py with the distance carry: the stack packed into the output line, the top entry held aside, every intermediate held
to its stated range) against the min-plus line; the bound predicate and the x pass's reach of host_arith.cpp in a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/edt_weights_driver.cpp); the entry point declared, exported and bound; Volume.spacing_weights; the
listing of edt_envelope.hip; and weights=None staying on vkv_distance_transform.  No device is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_binding_cpu import HANDLE, context
from tests.edt_envelope_ref import DistanceCarry, envelope_line_py
from tests.test_distance_cpu import NONE, TO_INSIDE, TO_OUTSIDE, edt2_np, random_mask_volume, targets_np
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vkvolume_amd", "host")


def edt2_weighted_brute_np(vol_dhw, iso, weights, target=TO_INSIDE, limit=None, box=None):
    """d_dist2 [d, h, w] uint32 of the header's sentence: min(limit, min over the target voxels u of the box of (wx dx)^2 + (wy dy)^2 +
    (wz dz)^2), by brute force over the target voxels in int64; weights = (wx, wy, wz); limit None: VKV_DISTANCE_NONE"""
    limit = NONE if limit is None else int(limit)
    wx, wy, wz = (int(w) for w in weights)
    t = targets_np(vol_dhw, iso, target, box)
    best = np.full(t.shape, limit, np.int64)
    zz, yy, xx = np.indices(t.shape, dtype=np.int64, sparse=True)
    for z, y, x in np.argwhere(t):
        best = np.minimum(best, (wz * (zz - z)) ** 2 + (wy * (yy - y)) ** 2 + (wx * (xx - x)) ** 2)
    return best.astype(np.uint32)


def edt2_weighted_np(vol_dhw, iso, weights, target=TO_INSIDE, limit=None, box=None):
    """the same values one axis after the other, as edt2_np with (w d)^2: g = 0 on a target and a value above every sum elsewhere, then
    out(p) = min over p' of g(p') + (w (p - p'))^2 along x, y and z, capped at the end; int64, so nothing wraps"""
    limit = NONE if limit is None else int(limit)
    t = targets_np(vol_dhw, iso, target, box)
    g = np.where(t, 0, np.int64(1) << 40).astype(np.int64)
    for axis, w in zip((2, 1, 0), weights):
        n = g.shape[axis]
        out = g.copy()
        for d in range(1, n):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, n - d), slice(d, n)
            lo, hi = tuple(lo), tuple(hi)
            out[hi] = np.minimum(out[hi], g[lo] + (int(w) * d) ** 2)
            out[lo] = np.minimum(out[lo], g[hi] + (int(w) * d) ** 2)
        g = out
    return np.minimum(g, limit).astype(np.uint32)


def scipy_edt2_weighted(targets, weights):
    """scipy's EDT with sampling to the nearest True voxel, squared from the returned indices in integers: exact"""
    from scipy import ndimage
    idx = ndimage.distance_transform_edt(~targets, sampling=[float(w) for w in weights[::-1]], return_distances=False, return_indices=True)
    w = np.array(weights[::-1], np.int64).reshape(3, 1, 1, 1)
    return ((w * (idx.astype(np.int64) - np.indices(targets.shape))) ** 2).sum(axis=0)


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [TO_INSIDE, TO_OUTSIDE])
def test_both_statements_are_scipys_edt_with_sampling_squared(target):
    rng = np.random.default_rng(31 + target)
    for k in range(60):
        shape = tuple(int(s) for s in rng.integers(1, 14, size=3))
        weights = tuple(int(w) for w in rng.integers(1, 8, size=3))
        density = (0.01, 0.1, 0.5)[k % 3]
        vol = random_mask_volume(rng, shape, density)
        t = targets_np(vol, 0.5, target)
        for limit in (None, 1, 10, 100000):
            a, b = edt2_weighted_brute_np(vol, 0.5, weights, target, limit), edt2_weighted_np(vol, 0.5, weights, target, limit)
            assert a.dtype == np.uint32 and a.shape == shape and np.array_equal(a, b), (shape, weights, density, limit)
            cap = NONE if limit is None else limit
            if t.any():
                assert np.array_equal(a, np.minimum(scipy_edt2_weighted(t, weights), cap)), (shape, weights, density, limit)
            else:
                assert (a == cap).all()        # scipy is undefined here; the definition is not
            assert np.array_equal(a == 0, t)


def test_unit_weights_are_the_unweighted_statement_and_no_target_gives_the_limit():
    rng = np.random.default_rng(7)
    for k in range(12):
        shape = tuple(int(s) for s in rng.integers(1, 12, size=3))
        vol = random_mask_volume(rng, shape, (0.02, 0.3)[k % 2])
        for target in (TO_INSIDE, TO_OUTSIDE):
            for limit in (None, 2, 9):
                want = edt2_np(vol, 0.5, target, limit)
                assert np.array_equal(edt2_weighted_np(vol, 0.5, (1, 1, 1), target, limit), want)
                assert np.array_equal(edt2_weighted_brute_np(vol, 0.5, (1, 1, 1), target, limit), want)
    vol = np.full((3, 4, 5), 17, np.uint8)
    for limit, cap in ((None, NONE), (1, 1), (7, 7)):
        for f in (edt2_weighted_brute_np, edt2_weighted_np):
            assert (f(vol, 0.5, (2, 2, 5), TO_INSIDE, limit) == cap).all() and (f(vol, 0.5, (2, 2, 5), TO_OUTSIDE, limit) == 0).all()
    vol[2, 3, 4] = 200
    z, y, x = np.indices(vol.shape)
    want = (5 * (z - 2)) ** 2 + (3 * (y - 3)) ** 2 + (2 * (x - 4)) ** 2
    box = (1, 1, 0, 4, 3, 3)
    for f in (edt2_weighted_brute_np, edt2_weighted_np):
        assert np.array_equal(f(vol, 0.5, (2, 3, 5)), want) and np.array_equal(f(vol, 0.5, (2, 3, 5), limit=30), np.minimum(want, 30))
        assert np.array_equal(f(vol, 0.5, (2, 3, 5), box=box), want[0:3, 1:4, 1:5])


# ---- the envelope pass of edt_envelope.hip ------------------------------------------------------------------------------------------------
def min_plus_line(g, w, limit):
    n = len(g)
    return [min([limit] + [g[i] + (w * (p - i)) ** 2 for i in range(n) if g[i] < limit]) for p in range(n)]


def test_the_envelope_pass_in_python_is_the_min_plus_line():
    rng = np.random.default_rng(2024)
    kinds = ("all cap", "no cap", "mixed", "sparse")
    for case in range(6000):
        n = 1 if case % 10 == 0 else int(rng.integers(1, 48))
        w = int(rng.integers(1, 8))
        limit = (NONE, int(rng.integers(1, 12)), int(rng.integers(12, 4000)))[case % 3]
        kind = kinds[(case // 3) % 4]
        top = min(limit, (4000, 50, 100000)[(case // 12) % 3])
        if kind == "all cap":
            g = [limit] * n
        else:
            g = [int(v) for v in rng.integers(0, top, size=n)]        # below the cap
            if kind != "no cap":
                share = 0.5 if kind == "mixed" else 0.9
                g = [limit if rng.random() < share else v for v in g]
        assert envelope_line_py(g, w, DistanceCarry(limit)) == min_plus_line(g, w, limit), (g, w, limit)


def test_the_envelope_pass_at_the_longest_line_and_the_largest_values():
    n = 32768
    for w, limit, g in ((1, NONE, {0: 0}), (2, NONE, {n - 1: 4294967244 - (2 * (n - 1)) ** 2}), (1, NONE, {0: 7, n - 1: 0}), (2, 0xfffffffe, {0: 0, 5: 1, n - 1: 3}),
                        (1, 1000, {100: 0, 20000: 999}), (1, NONE, {})):
        line = [limit] * n
        for i, v in g.items():
            line[i] = v
        got = np.array(envelope_line_py(line, w, DistanceCarry(limit)), np.int64)
        p = np.arange(n, dtype=np.int64)
        want = np.full(n, limit, np.int64)
        for i, v in g.items():
            want = np.minimum(want, v + (w * (p - i)) ** 2)
        assert np.array_equal(got, want), (w, limit, g)
    # every position on the stack: a line of zeros, and a parabola-shaped line whose every entry survives
    for line in ([0] * 3000, [(i - 1500) ** 2 // 7 for i in range(3000)]):
        assert envelope_line_py(line, 1, DistanceCarry(NONE)) == min_plus_line(line, 1, NONE)


# ---- the bound predicate and the reach --------------------------------------------------------------------------------------------------
def test_the_bound_predicate_and_the_reach_in_a_stand_alone_program(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "edt_weights_driver")
    build = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g", "-Wall"]
    sources = [os.path.join(ROOT, "tests", "edt_weights_driver.cpp"), os.path.join(HOST, "host_arith.cpp"), os.path.join(HOST, "load_volume.cpp")]
    subprocess.check_call(build + sources + ["-o", exe])
    r = subprocess.run([exe], env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "edt weights driver: ok" in r.stdout, r.stdout[-4000:]


# ---- entry point --------------------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bint\s+vkv_distance_transform_weighted\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"float iso,\s*int32_t target,\s*const uint32_t weights\[3\],\s*uint32_t limit,\s*void\s*\*d_scratch,\s*uint32_t\s*\*d_dist2,\s*void\s*\*stream\)",
                     header)
    assert "vkv_distance_transform_weighted_scratch_bytes" not in header        # one scratch block for both calls
    L = lib.load()
    assert "vkv_distance_transform_weighted" in lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\bvkv_distance_transform_weighted$", out, flags=re.M)
    at = L.vkv_distance_transform_weighted.argtypes
    assert len(at) == 11 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[5] is C.c_int32
    assert at[6] is C.POINTER(C.c_uint32) and at[7] is C.c_uint32 and L.vkv_distance_transform_weighted.restype is C.c_int
    assert callable(lib.Context.distance_transform_weighted_rc) and not hasattr(lib.Context, "distance_transform_weighted")
    buf = (C.c_uint64 * 128)()
    a = C.addressof(buf)
    w = (C.c_uint32 * 3)(2, 2, 5)
    assert L.vkv_distance_transform_weighted(None, a, abi.Extent3D(4, 4, 4), None, 0.5, 0, w, 5, a + 64, a + 512, None) == abi.VKV_E_INVALID_ARGUMENT
    assert not any(buf) and list(w) == [2, 2, 5]


def test_the_binding_passes_the_weights_as_three_uint32():
    ctx, rec = context()
    e = abi.Extent3D(40, 50, 60)
    assert ctx.distance_transform_weighted_rc(10, e, None, 0.5, abi.DISTANCE_TO_OUTSIDE, (2, 2, 5), None, 11, 12, 99) == 0
    assert rec.last("vkv_distance_transform_weighted") == (HANDLE, 10, bytes(e), None, 0.5, abi.DISTANCE_TO_OUTSIDE, [2, 2, 5], abi.DISTANCE_NONE, 11, 12, 99)
    ctx.distance_transform_weighted_rc(10, e, None, 0.5, abi.DISTANCE_TO_INSIDE, None, 7, 11, 12)
    assert rec.last("vkv_distance_transform_weighted") == (HANDLE, 10, bytes(e), None, 0.5, abi.DISTANCE_TO_INSIDE, None, 7, 11, 12, 0)


# ---- Volume.spacing_weights ---------------------------------------------------------------------------------------------------------------
def test_spacing_weights():
    f = V.Volume.spacing_weights
    assert f((0.5, 0.5, 1.25)) == ((2, 2, 5), 0.25)
    assert f((1, 1, 1)) == ((1, 1, 1), 1.0)
    assert f((1.25, 0.5, 0.5)) == ((5, 2, 2), 0.25) and f((0.3, 0.3, 0.9)) == ((1, 1, 3), 0.3)
    assert f((0.7, 0.7, 1.0)) == ((7, 7, 10), 0.7 / 7)        # m = 7 is exact
    # the fallback: 1 : sqrt(2) has no exact ratio.  With max_weight 10, m runs to 7 (w_z = round(7 sqrt 2) = 10; m = 8 would need 11); the
    # relative errors of w_z / m against sqrt(2) are 1 : 0.29, 3/2 : 0.061, 4/3 : 0.057, 6/4 : 0.061, 7/5 : 0.0101, 8/6 : 0.057, 10/7 : 0.0102
    weights, unit = f((1.0, 1.0, 2.0 ** 0.5), max_weight=10)
    assert weights == (5, 5, 7) and unit == 1.0 / 5
    assert f((1.0, 1.0, 2.0 ** 0.5), max_weight=10, rel_tol=0.07) == ((2, 2, 3), 0.5)        # the FIRST m within the tolerance, not the best
    assert f((1.0, 1.0, 2.0 ** 0.5), max_weight=64)[0] == (29, 29, 41)        # 41 / 29 is within 1e-3 (0.03 %); 17 / 12 (0.17 %) is not
    assert f((2.0, 3.0, 1.0), max_weight=3) == ((2, 3, 1), 1.0)
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, float("inf")), (1, float("nan"), 1), (1, 1), (1, 1, 1, 1), "abc", (1, 1, 100.0)):
        with pytest.raises(ValueError):
            f(bad)
    assert f((1, 1, 100.0), max_weight=100) == ((1, 1, 100), 1.0)


# ---- the listing ----------------------------------------------------------------------------------------------------------------------------
def test_the_envelope_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("edt_envelope.hip", tmp_path / "edt_envelope.s")
    for name in ("k_env_x", "k_env_axis"):
        assert len([k for k in kernels if name in k]) == 1, sorted(kernels)
    assert len(kernels) == 2        # k_edt_bits is edt.hip's: declared here, defined there
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)
    # the walk and the envelope pass are edt_passes.hpp's: no more registers than the copies they replaced had
    for name, vgprs in (("k_env_x", 18), ("k_env_axis", 22)):
        assert [v["NumVgprs"] for k, v in kernels.items() if name in k][0] <= vgprs, (name, kernels)


# ---- weights=None keeps the old path ------------------------------------------------------------------------------------------------------
@pytest.fixture
def stub_volume(monkeypatch):
    """a Volume of 12 x 5 x 4 host bytes on a context whose library records the calls"""
    ctx, rec = context()
    monkeypatch.setattr(V, "_stream", lambda: 99)
    v = V.Volume(ctx, device=torch.device("cpu"))
    v.volume = torch.full((4, 5, 12), 200, dtype=torch.uint8)
    v.extent = abi.Extent3D(12, 5, 4)
    return v, rec


def test_weights_none_stays_on_the_unweighted_call(stub_volume):
    v, rec = stub_volume
    v.distance_transform(0.5, to="outside", limit=7)
    for name in ("erode", "dilate", "open", "close"):
        getattr(v, name)(0.5, radius2=4)
        getattr(v, name)(0.5, radius2=4, weights=None)
    assert len(rec.calls["vkv_distance_transform"]) == 1 + 2 * (1 + 1 + 2 + 2) and "vkv_distance_transform_weighted" not in rec.calls
    assert rec.calls["vkv_distance_transform"][0][5:7] == (abi.DISTANCE_TO_OUTSIDE, 7)
    assert rec.calls["vkv_distance_transform"][1][5:7] == (abi.DISTANCE_TO_OUTSIDE, 5)        # erode: limit radius2 + 1


def test_weights_take_the_weighted_call_with_the_same_scratch(stub_volume):
    v, rec = stub_volume
    d = v.distance_transform(0.5, limit=30, box=((1, 1, 1), (3, 2, 2)), weights=(2, 2, 5))
    assert d.dtype == torch.uint32 and tuple(d.shape) == (2, 2, 3)
    call = rec.last("vkv_distance_transform_weighted")
    assert call[0] == HANDLE and call[3] == bytes(abi.Box(1, 1, 1, 3, 2, 2)) and call[5:8] == (abi.DISTANCE_TO_INSIDE, [2, 2, 5], 30) and call[10] == 99
    v.open(0.5, radius=5, weights=np.array([2, 2, 5]))
    assert [c[5:8] for c in rec.calls["vkv_distance_transform_weighted"][1:]] == [(abi.DISTANCE_TO_OUTSIDE, [2, 2, 5], 26), (abi.DISTANCE_TO_INSIDE, [2, 2, 5], 26)]
    assert "vkv_distance_transform" not in rec.calls and len(rec.calls["vkv_select_by_distance"]) == 2
    assert rec.calls["vkv_select_by_distance"][0][6:9] == (1, 25, 0)
    for bad in ((2, 2), (2, 2, 0), (1, 1, 1.5), (1, 1, -1), (1, 1, 2 ** 32), "xyz", 3):
        with pytest.raises(ValueError):
            v.distance_transform(0.5, weights=bad)
        with pytest.raises(ValueError):
            v.erode(0.5, radius=2, weights=bad)
    v.ctx._lib.status = abi.VKV_E_UNSUPPORTED        # a status other than 0 raises: the check is the caller's
    with pytest.raises(lib.VkvError, match="recorded message"):
        v.distance_transform(0.5, weights=(2, 2, 5))

"""CPU: vkv_filter_volume (3x3x3 binomial and median of the uint8 volume) is declared, exported and bound and refuses bad
arguments before anything touches the HIP runtime; the numpy restatements binomial3_np and median3_np (what tests/test_gpu_filter.py compares
the kernels with, byte for byte) each against an independent second statement; the filters' properties; the Volume.filter wrapper; the
selection network of the median (vkvolume_amd/csrc/median27_network.hpp, the very templates the kernel instantiates) on all 2^27 zero/one
inputs, which by the zero-one principle proves it for every input; and no kernel of filter.hip uses scratch memory."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as T
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = (1, 2, 1)


# ---- the restatements ------------------------------------------------------------------------------------------------------------------
def neighbours(vol):
    """the 27 shifted, edge-clamped copies of vol (D, H, W): [(dz, dy, dx), copy]"""
    vol = np.asarray(vol)
    d, h, w = vol.shape
    out = []
    for dz in (-1, 0, 1):
        zi = np.clip(np.arange(d) + dz, 0, d - 1)
        for dy in (-1, 0, 1):
            yi = np.clip(np.arange(h) + dy, 0, h - 1)
            for dx in (-1, 0, 1):
                xi = np.clip(np.arange(w) + dx, 0, w - 1)
                out.append(((dz, dy, dx), vol[np.ix_(zi, yi, xi)]))
    return out


def binomial3_np(vol):
    """(S + 32) >> 6 with S the (1, 2, 1)^3 weighted integer sum of the 27 clamped neighbours: one rounding"""
    s = np.zeros(np.asarray(vol).shape, np.int64)
    for (dz, dy, dx), n in neighbours(vol):
        s += WEIGHTS[dz + 1] * WEIGHTS[dy + 1] * WEIGHTS[dx + 1] * n.astype(np.int64)
    assert s.max() <= 16320
    return ((s + 32) >> 6).astype(np.uint8)


def median3_np(vol):
    """index 13 of the 27 clamped neighbours after sorting"""
    return np.sort(np.stack([n for _, n in neighbours(vol)]), axis=0)[13]


def binomial3_separable(vol):
    """second statement: three (1, 2, 1) passes over the edge-padded volume in int32, then the one rounding"""
    p = np.pad(np.asarray(vol).astype(np.int32), 1, mode="edge")
    p = p[:-2] + 2 * p[1:-1] + p[2:]
    p = p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:]
    p = p[:, :, :-2] + 2 * p[:, :, 1:-1] + p[:, :, 2:]
    return ((p + 32) >> 6).astype(np.uint8)


def median3_by_counting(vol):
    """second statement: per voxel the smallest b with count(N <= b) >= 14"""
    n = np.stack([c for _, c in neighbours(vol)]).astype(np.int32)
    out = np.full(n.shape[1:], -1, np.int32)
    for b in range(256):
        hit = (out < 0) & ((n <= b).sum(axis=0) >= 14)
        out[hit] = b
    assert out.min() >= 0
    return out.astype(np.uint8)


def contents(kind, shape_dhw, seed):
    """the test volumes of both filter test files: uniform random bytes, all 255, a 0 / 255 checkerboard, two values, isolated 255s in zeros"""
    rng = np.random.default_rng(seed)
    d, h, w = shape_dhw
    if kind == "random":
        return rng.integers(0, 256, size=shape_dhw, dtype=np.uint8)
    if kind == "all255":
        return np.full(shape_dhw, 255, np.uint8)
    if kind == "checker":
        z, y, x = np.indices(shape_dhw)
        return (((x + y + z) & 1) * 255).astype(np.uint8)
    if kind == "two":
        return np.where(rng.random(shape_dhw) < 0.5, 37, 200).astype(np.uint8)
    if kind == "salt":
        v = np.zeros(shape_dhw, np.uint8)
        v[::3, ::3, ::3] = 255        # no two within one neighbourhood of each other's centre: at most 8 of any 27
        return v
    raise ValueError(kind)


CONTENTS = ("random", "all255", "checker", "two", "salt")
SHAPES = [(5, 6, 7), (1, 6, 7), (6, 1, 7), (6, 7, 1), (1, 1, 9), (1, 1, 1), (2, 2, 2), (3, 9, 4)]


# ---- entry point -----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bVKV_FILTER_BINOMIAL3\s*=\s*%d\b" % abi.FILTER_BINOMIAL3, header)
    assert re.search(r"\bVKV_FILTER_MEDIAN3\s*=\s*%d\b" % abi.FILTER_MEDIAN3, header)
    assert re.search(r"\bint\s+vkv_filter_volume\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_src,\s*uint8_t\s*\*d_dst,\s*VkvExtent3D extent,\s*"
                     r"const VkvBox\s*\*box,\s*int32_t kind,\s*void\s*\*stream\)", header)
    L = lib.load()
    assert "vkv_filter_volume" in lib.EXPORTS
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\bvkv_filter_volume$", out, flags=re.M)
    at = L.vkv_filter_volume.argtypes
    assert len(at) == 7 and at[3] is abi.Extent3D and at[4] is C.POINTER(abi.Box) and at[5] is C.c_int32
    assert callable(lib.Context.filter_volume) and callable(lib.Context.filter_volume_rc) and callable(V.Volume.filter)


def test_bad_arguments_are_rejected_without_a_device():
    """no context exists without a device, so every call carries a null ctx besides its own fault: what is shown is that each returns
    VKV_E_INVALID_ARGUMENT without entering the HIP runtime (tests/test_gpu_filter.py repeats them with a live context and a sentinel)"""
    L = lib.load()
    e = abi.Extent3D(4, 4, 4)
    buf = (C.c_uint8 * 192)()
    a = C.addressof(buf)
    inside, outside, empty = abi.Box(0, 0, 0, 1, 1, 1), abi.Box(3, 0, 0, 2, 1, 1), abi.Box(0, 0, 0, 0, 1, 1)
    bad = abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_filter_volume(None, None, None, e, None, abi.FILTER_BINOMIAL3, None) == bad
    assert L.vkv_filter_volume(None, a, a + 64, e, C.byref(inside), abi.FILTER_MEDIAN3, None) == bad        # null ctx alone
    assert L.vkv_filter_volume(None, a, a + 63, e, None, abi.FILTER_MEDIAN3, None) == bad                   # overlap by one byte
    assert L.vkv_filter_volume(None, a + 63, a, e, None, abi.FILTER_MEDIAN3, None) == bad
    assert L.vkv_filter_volume(None, a, a, e, None, abi.FILTER_BINOMIAL3, None) == bad                      # in place
    assert L.vkv_filter_volume(None, a, a + 64, e, C.byref(outside), abi.FILTER_BINOMIAL3, None) == bad
    assert L.vkv_filter_volume(None, a, a + 64, e, C.byref(empty), abi.FILTER_BINOMIAL3, None) == bad
    assert L.vkv_filter_volume(None, a, a + 64, e, None, 2, None) == bad
    assert L.vkv_filter_volume(None, a, a + 64, e, None, -1, None) == bad
    assert L.vkv_filter_volume(None, a, a + 64, abi.Extent3D(4, 0, 4), None, abi.FILTER_BINOMIAL3, None) == bad
    assert bytes(buf) == bytes(192)


# ---- the Volume wrapper ----------------------------------------------------------------------------------------------------------------
class FakeContext:
    """records the calls the wrapper makes instead of entering the library"""
    device = 0

    def __init__(self):
        self.calls = []

    def filter_volume(self, *args):
        self.calls.append(args)


def fake_volume(monkeypatch):
    monkeypatch.setattr(V, "_stream", lambda: 0)  # no HIP stream without a device
    ctx = FakeContext()
    v = V.Volume(ctx, device=torch.device("cpu"))
    v.volume = torch.zeros((3, 4, 5), dtype=torch.uint8)
    v.extent = abi.Extent3D(5, 4, 3)
    return v, ctx


def test_volume_filter_wrapper_passes_buffers_box_and_ping_pongs(monkeypatch):
    v, ctx = fake_volume(monkeypatch)
    before = v.volume
    out = v.filter(abi.FILTER_MEDIAN3)
    assert out.shape == v.volume.shape and out.dtype == torch.uint8 and v.volume is before
    (src, dst, ext, box, kind, _), = ctx.calls
    assert src == v.volume.data_ptr() and dst == out.data_ptr() and ext.as_tuple() == (5, 4, 3) and box is None and kind == abi.FILTER_MEDIAN3
    mine = torch.zeros_like(v.volume)
    assert v.filter(abi.FILTER_BINOMIAL3, out=mine, box=((1, 2, 0), (4, 2, 3))) is mine
    b = ctx.calls[-1][3]
    assert isinstance(b, abi.Box) and (b.x0, b.y0, b.z0, b.width, b.height, b.depth) == (1, 2, 0, 4, 2, 3) and ctx.calls[-1][1] == mine.data_ptr()
    for passes in (2, 3):
        del ctx.calls[:]
        res = v.filter(abi.FILTER_BINOMIAL3, passes=passes, out=mine)
        assert res is mine and len(ctx.calls) == passes
        assert ctx.calls[0][0] == v.volume.data_ptr() and ctx.calls[-1][1] == mine.data_ptr()
        for prev, cur in zip(ctx.calls, ctx.calls[1:]):
            assert cur[0] == prev[1] and cur[1] != cur[0]        # each pass reads what the last wrote, never in place
        assert all(c[1] != v.volume.data_ptr() for c in ctx.calls)


def test_volume_filter_wrapper_rejects_bad_arguments(monkeypatch):
    v, ctx = fake_volume(monkeypatch)
    with pytest.raises(ValueError, match="unknown kind"):
        v.filter(2)
    with pytest.raises(ValueError, match="passes"):
        v.filter(abi.FILTER_MEDIAN3, passes=0)
    with pytest.raises(ValueError, match="needs `out`"):
        v.filter(abi.FILTER_MEDIAN3, box=((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="one pass"):
        v.filter(abi.FILTER_MEDIAN3, passes=2, out=torch.zeros_like(v.volume), box=((0, 0, 0), (1, 1, 1)))
    for bad in (torch.zeros((3, 4, 5), dtype=torch.int8), torch.zeros((3, 4, 6), dtype=torch.uint8), torch.zeros((3, 4, 10), dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError, match="contiguous"):
            v.filter(abi.FILTER_MEDIAN3, out=bad)
    assert ctx.calls == []


# ---- two statements of each filter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_two_statements_of_each_filter_agree(shape):
    for k, kind in enumerate(CONTENTS):
        vol = contents(kind, shape, seed=100 + k)
        what = "%s %s" % (kind, shape)
        assert np.array_equal(binomial3_np(vol), binomial3_separable(vol)), what
        assert np.array_equal(median3_np(vol), median3_by_counting(vol)), what


def test_one_rounding_differs_from_one_per_axis():
    """the definition is pinned: rounding after every axis gives other bytes on random data"""
    vol = contents("random", (6, 7, 8), seed=7)
    p = np.pad(vol.astype(np.int32), 1, mode="edge")
    p = (p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2
    p = (p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:] + 2) >> 2
    p = (p[:, :, :-2] + 2 * p[:, :, 1:-1] + p[:, :, 2:] + 2) >> 2
    assert not np.array_equal(p.astype(np.uint8), binomial3_np(vol))


# ---- properties ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 5, 6), (1, 3, 2)])
def test_properties(shape):
    for c in (0, 1, 127, 254, 255):
        vol = np.full(shape, c, np.uint8)
        assert np.array_equal(binomial3_np(vol), vol) and np.array_equal(median3_np(vol), vol)
    salt = np.zeros((7, 7, 7), np.uint8)
    salt[::3, ::3, ::3] = 255
    assert salt.any() and not median3_np(salt).any()        # isolated 255s in zeros disappear
    two = contents("two", (5, 6, 7), seed=3)
    assert set(np.unique(median3_np(two))) <= {37, 200}


# ---- the selection network -------------------------------------------------------------------------------------------------------------
def test_median_network_is_proven_on_all_zero_one_inputs(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "median27_driver"
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-I", T.CSRC, os.path.join(ROOT, "tests", "median27_driver.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "median27 ok: %d inputs" % (1 << 27) in r.stdout
    # the kernel instantiates these very templates, not a copy
    src = open(os.path.join(T.CSRC, "filter.hip")).read()
    assert '#include "median27_network.hpp"' in src
    for stage in ("sort3(", "merge_triples(", "median_of_sorted("):
        assert stage in src, stage
    assert "net_cx" not in src and "elementwise_min" in src and "elementwise_max" in src


# ---- no scratch ------------------------------------------------------------------------------------------------------------------------
def test_filter_kernels_use_no_scratch(tmp_path):
    kernels = T.kernel_listing("filter.hip", tmp_path / "filter.s")
    names = [k for k in kernels if "k_filter3" in k]
    assert len(names) == 4, sorted(kernels)  # two kinds x (WIDE, narrow)
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)

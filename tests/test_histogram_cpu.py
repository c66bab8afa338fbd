"""CPU: the histogram entry points (vkv_volume_histogram, vkv_histogram_occupied_count) are declared, exported and bound and refuse null
arguments before anything touches the HIP runtime; the Python wrappers' box, mode and shape handling; and a numpy restatement of the bin and
count rule against the oracle's transfer-function uniform and occupied-voxel count."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vkv_volume_histogram", "vkv_histogram_occupied_count")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"#define\s+VKV_HISTOGRAM_BINS\s+65536\b", header) and abi.HISTOGRAM_BINS == 65536
    for name, value in (("SET", abi.HISTOGRAM_SET), ("ADD", abi.HISTOGRAM_ADD), ("SUBTRACT", abi.HISTOGRAM_SUBTRACT)):
        assert re.search(r"\bVKV_HISTOGRAM_%s\s*=\s*%d\b" % (name, value), header)
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert name in lib.EXPORTS
        assert re.search(r"\b%s$" % name, out, flags=re.M)
    at = L.vkv_volume_histogram.argtypes
    assert len(at) == 8 and at[3] is abi.Extent3D and at[4] is C.POINTER(abi.Box) and at[5] is C.c_int32
    at = L.vkv_histogram_occupied_count.argtypes
    assert len(at) == 5 and at[2] is C.POINTER(abi.TransferFunctionUniform)


def test_null_arguments_are_rejected_without_a_device():
    L = lib.load()
    box = abi.Box(0, 0, 0, 1, 1, 1)
    tf = abi.TransferFunctionUniform()
    assert L.vkv_volume_histogram(None, None, None, abi.Extent3D(4, 4, 4), C.byref(box), abi.HISTOGRAM_SET, None, None) == abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_volume_histogram(None, None, None, abi.Extent3D(4, 4, 4), None, 7, None, None) == abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_histogram_occupied_count(None, None, C.byref(tf), None, None) == abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_histogram_occupied_count(None, None, None, None, None) == abi.VKV_E_INVALID_ARGUMENT


class FakeContext:
    """records the calls the wrappers make instead of entering the library"""
    device = 0

    def __init__(self):
        self.calls = []

    def volume_histogram(self, *args):
        self.calls.append(("volume_histogram",) + args)

    def histogram_occupied_count(self, *args):
        self.calls.append(("histogram_occupied_count",) + args)


def fake_volume(monkeypatch, use_gradient=True):
    monkeypatch.setattr(V, "_stream", lambda: 0)  # no HIP stream without a device
    ctx = FakeContext()
    v = V.Volume(ctx, device=torch.device("cpu"))
    v.options.use_precomputed_gradient = 1 if use_gradient else 0
    v.volume = torch.zeros((3, 4, 5), dtype=torch.uint8)
    v.gradient = torch.zeros((3, 4, 5), dtype=torch.uint8) if use_gradient else None
    v.extent = abi.Extent3D(5, 4, 3)
    return v, ctx


def test_volume_histogram_wrapper_passes_box_mode_and_buffers(monkeypatch):
    v, ctx = fake_volume(monkeypatch)
    out = v.histogram()
    assert out.shape == (256, 256) and out.dtype == torch.int64
    (name, d_vol, d_grad, ext, box, mode, d_hist, _), = ctx.calls
    assert name == "volume_histogram" and box is None and mode == abi.HISTOGRAM_SET
    assert d_vol == v.volume.data_ptr() and d_grad == v.gradient.data_ptr() and d_hist == out.data_ptr() and ext.as_tuple() == (5, 4, 3)
    assert v.histogram(out=out, box=((1, 2, 0), (4, 2, 3)), mode=abi.HISTOGRAM_SUBTRACT) is out
    box = ctx.calls[-1][4]
    assert isinstance(box, abi.Box) and (box.x0, box.y0, box.z0, box.width, box.height, box.depth) == (1, 2, 0, 4, 2, 3)
    assert ctx.calls[-1][5] == abi.HISTOGRAM_SUBTRACT
    b = abi.Box(0, 1, 2, 1, 1, 1)
    v.histogram(out=out, box=b, mode=abi.HISTOGRAM_ADD)
    assert ctx.calls[-1][4] is b and ctx.calls[-1][5] == abi.HISTOGRAM_ADD
    v2, ctx2 = fake_volume(monkeypatch, use_gradient=False)
    v2.histogram()
    assert ctx2.calls[-1][2] is None  # no gradient map: every voxel in row 0


def test_volume_histogram_wrapper_rejects_bad_arguments(monkeypatch):
    v, ctx = fake_volume(monkeypatch)
    with pytest.raises(ValueError, match="unknown mode"):
        v.histogram(mode=3)
    with pytest.raises(ValueError, match="need `out`"):
        v.histogram(mode=abi.HISTOGRAM_ADD)
    for bad in (torch.zeros((256, 256), dtype=torch.int32), torch.zeros(65536, dtype=torch.int64), torch.zeros((256, 512), dtype=torch.int64)[:, ::2]):
        with pytest.raises(ValueError, match="contiguous"):
            v.histogram(out=bad)
    with pytest.raises(ValueError):
        v.occupied_count_from_histogram(torch.zeros(100, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        v.occupied_count_from_histogram(torch.zeros((256, 256), dtype=torch.int64), torch.zeros(1, dtype=torch.float32))
    assert ctx.calls == []
    hist, count = torch.zeros((256, 256), dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    v.occupied_count_from_histogram(hist, count)
    (name, d_hist, tf, d_count, _), = ctx.calls
    assert name == "histogram_occupied_count" and d_hist == hist.data_ptr() and d_count == count.data_ptr()
    assert isinstance(tf, abi.TransferFunctionUniform)


def histogram(vol, grad):
    key = vol.astype(np.int64).reshape(-1) + (grad.astype(np.int64).reshape(-1) << 8 if grad is not None else 0)
    return np.bincount(key, minlength=abi.HISTOGRAM_BINS).astype(np.uint64).reshape(256, 256)


def histogram_count(hist, tf):
    """bit row g (or 255 without use_gradient), alpha from the uniform's min and range_inv in float32: clamp((x - min) * range_inv, 0, 1)"""
    f = np.float32
    b = np.arange(256, dtype=np.float32) / f(255.0)
    with np.errstate(invalid="ignore"):  # a degenerate window: 0 * inf is NaN, and NaN > 0 is false, as on the device
        ai = np.clip((b - f(tf.intensity_min)) * f(tf.intensity_range_inv), f(0), f(1)).astype(np.float32)
        ag = np.clip((b - f(tf.gradient_min)) * f(tf.gradient_range_inv), f(0), f(1)).astype(np.float32)
    if not tf.use_gradient:
        ag = np.full(256, ag[255], np.float32)
    with np.errstate(invalid="ignore"):
        occupied = (ag[:, None] * ai[None, :]) > 0
    return int(hist[occupied].sum())


@pytest.mark.parametrize("opts", [dict(), T.APP_TF, dict(intensity_min=0.4, intensity_max=0.8, gradient_min=0.0, gradient_max=0.0),
                                  dict(intensity_min=0.2, intensity_max=0.8, gradient_min=0.06, gradient_max=0.12),
                                  dict(intensity_min=0.5, intensity_max=0.5), dict(intensity_min=0.3, intensity_max=0.3, gradient_min=0.0, gradient_max=0.2)])
def test_bin_and_count_rule_against_the_oracle(opts):
    tf = O.transfer_function_uniform(abi.VolumeOptions(**opts))
    for seed, shape in ((1, (37, 29, 23)), (2, (64, 48, 40))):
        vol = T.random_volume(shape, seed, sparsity=0.5)
        grad = O.gradient_map(vol, tf)
        h = histogram(vol, grad)
        assert int(h.sum()) == vol.size and h[grad[0, 0, 0], vol[0, 0, 0]] >= 1
        assert histogram_count(h, tf) == O.occupied_voxel_count(vol, grad, tf)
        if not tf.use_gradient:  # without use_gradient the row does not matter: the intensity histogram (row 0) gives the same count
            assert histogram_count(histogram(vol, None), tf) == O.occupied_voxel_count(vol, None, tf)

"""GPU: the joint (gradient byte, intensity byte) histogram of the volume (vkv_volume_histogram) bin for bin against np.bincount / torch.bincount
of g * 256 + i, over tiny, odd, misaligned, random, synthetic, constant and C3-size volumes, boxes and the three modes; the occupied-voxel count
read off it (vkv_histogram_occupied_count) against vkv_occupied_voxel_count; a histogram kept across vkv_update_volume_region; streams,
hipGraph capture, argument checks, the Python wrapper and the driver."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_gpu_volume_region import SOURCES, State, make_source
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vkvolume_amd", "csrc", "vkv_offscreen")
BINS = abi.HISTOGRAM_BINS
C3 = ((1024, 1024, 795), 0xC0FFEE03)  # bench.py's "c3" workload: kind 1 shells
# the transfer functions of the count comparisons: the defaults, the application's, the windows test_host_cpu.py uses, a degenerate intensity
# window, and use_gradient 0 (gradient_min == gradient_max)
TF_CASES = [dict(), T.APP_TF, dict(intensity_min=0.4, intensity_max=0.8, gradient_min=0.0, gradient_max=0.0),
            dict(intensity_min=0.2, intensity_max=0.8, gradient_min=0.06, gradient_max=0.12),
            dict(sampling_factor=2.5, voxel_alpha_factor=0.3, intensity_min=0.5, intensity_max=0.5),
            dict(intensity_min=0.3, intensity_max=0.3, gradient_min=0.0, gradient_max=0.2),
            dict(intensity_min=0.05, intensity_max=0.6, gradient_min=0.1, gradient_max=0.1)]


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def ext_of(vol):
    d, h, w = vol.shape
    return abi.Extent3D(w, h, d)


def device_hist(ctx, vol, grad, box=None, mode=abi.HISTOGRAM_SET, out=None, ext=None):
    out = torch.zeros(BINS, dtype=torch.int64, device="cuda") if out is None else out
    ctx.volume_histogram(ptr(vol), ptr(grad), ext_of(vol) if ext is None else ext, box, mode, ptr(out), st())
    return out


def np_hist(vol, grad):
    """the reference: bincount of g * 256 + i (uint64 bins viewed as int64)"""
    key = np.asarray(vol, np.int64).reshape(-1)
    if grad is not None:
        key = key + (np.asarray(grad, np.int64).reshape(-1) << 8)
    return np.bincount(key, minlength=BINS).astype(np.int64)


def torch_hist(vol, grad, chunk=64):
    """the reference for volumes too large for the host: torch.bincount on the device, slab by slab"""
    out = torch.zeros(BINS, dtype=torch.int64, device="cuda")
    for z in range(0, vol.shape[0], chunk):
        key = vol[z:z + chunk].reshape(-1).to(torch.int64)
        if grad is not None:
            key += grad[z:z + chunk].reshape(-1).to(torch.int64) << 8
        out += torch.bincount(key, minlength=BINS)
        del key
    return out


def gradient_of(ctx, vol, opts=T.APP_TF):
    grad = torch.zeros_like(vol)
    ctx.gradient_map(ptr(vol), ptr(grad), ext_of(vol), lib.transfer_function_uniform(abi.VolumeOptions(**opts)), st())
    return grad


def synth(ctx, whd, kind, seed):
    w, h, d = whd
    vol = torch.empty((d, h, w), dtype=torch.uint8, device="cuda")
    ctx.synth_volume(ptr(vol), abi.Extent3D(w, h, d), kind, seed, st())
    return vol


def check_whole(ctx, vol, grad_too=True):
    """whole volume, with the gradient map and with d_gradient = NULL, against np.bincount"""
    vn = vol.cpu().numpy()
    for grad in ([gradient_of(ctx, vol)] if grad_too else []) + [None]:
        got = device_hist(ctx, vol, grad).cpu().numpy()
        want = np_hist(vn, None if grad is None else grad.cpu().numpy())
        assert np.array_equal(got, want), "grad %s: %d bins differ" % (grad is not None, int((got != want).sum()))
        assert got.sum() == vn.size


# ---- 1. whole volumes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whd", [(1, 1, 1), (3, 5, 7), (4, 4, 4), (65, 3, 2), (257, 9, 5)])
def test_tiny_and_odd_volumes(ctx, whd):
    w, h, d = whd
    check_whole(ctx, torch.from_numpy(T.random_volume(whd, w * 131 + h * 7 + d)).cuda())


@pytest.mark.parametrize("width", range(1, 10))
def test_widths_1_to_9_at_every_byte_offset(ctx, width):
    """volume and gradient at byte offsets 0..3 inside larger allocations, each ending where its allocation ends"""
    h, d = 7, 5
    n = width * h * d
    rng = np.random.default_rng(width)
    vol_np = rng.integers(0, 256, size=(d, h, width), dtype=np.uint8)
    grad_np = rng.integers(0, 256, size=(d, h, width), dtype=np.uint8)
    for ov in range(4):
        for og in range(4):
            vb = torch.zeros(ov + n, dtype=torch.uint8, device="cuda")
            gb = torch.zeros(og + n, dtype=torch.uint8, device="cuda")
            vol, grad = vb[ov:].view(d, h, width), gb[og:].view(d, h, width)
            vol.copy_(torch.from_numpy(vol_np)), grad.copy_(torch.from_numpy(grad_np))
            for g, gn in ((grad, grad_np), (None, None)):
                got = device_hist(ctx, vol, g).cpu().numpy()
                assert np.array_equal(got, np_hist(vol_np, gn)), "offsets %d / %d, gradient %s" % (ov, og, g is not None)


def test_synthetic_64_kind_0(ctx):
    check_whole(ctx, synth(ctx, (64, 64, 64), 0, 0xC0FFEE01))


def test_random_493x311x97(ctx):
    check_whole(ctx, torch.from_numpy(T.random_volume((493, 311, 97), 4931, sparsity=0.6)).cuda())


def test_c3_synthetic_scene(ctx):
    vol = synth(ctx, C3[0], 1, C3[1])
    for grad in (gradient_of(ctx, vol), None):
        assert torch.equal(device_hist(ctx, vol, grad), torch_hist(vol, grad))


# ---- 2. boxes -------------------------------------------------------------------------------------------------------------------------
def boxes_of(ext, rng, n_random):
    W, H, D = ext
    out = [abi.Box(0, 0, 0, W, H, D), abi.Box(0, 0, 0, 1, 1, 1), abi.Box(W - 1, H - 1, D - 1, 1, 1, 1), abi.Box(W // 2, H // 3, D // 4, 1, 1, 1)]
    out += [abi.Box(0, 0, 0, 1, H, D), abi.Box(W - 1, 0, 0, 1, H, D), abi.Box(0, 0, 0, W, 1, D), abi.Box(0, H - 1, 0, W, 1, D),  # the six faces
            abi.Box(0, 0, 0, W, H, 1), abi.Box(0, 0, D - 1, W, H, 1)]
    out += [abi.Box(W - 3, 1, 2, 3, H - 2, D - 3), abi.Box(1, 0, 0, W - 2, H, D)]  # narrow and nearly full
    for _ in range(n_random):
        w, h, d = [int(rng.integers(1, n + 1)) for n in (W, H, D)]
        out.append(abi.Box(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), int(rng.integers(0, D - d + 1)), w, h, d))
    return out


@pytest.mark.parametrize("whd", [(61, 47, 29), (211, 190, 97), (40, 300, 300)])
def test_boxes(ctx, whd):
    """random boxes, boxes on each face, single voxels and the full extent (small boxes take the global-atomic path, large ones LDS; the
    40-wide volume also has 1-3 voxel wide boxes of more than 2^18 voxels)"""
    rng = np.random.default_rng(sum(whd))
    vol = torch.from_numpy(T.random_volume(whd, sum(whd), sparsity=0.3)).cuda()
    grad = gradient_of(ctx, vol)
    vn, gn = vol.cpu().numpy(), grad.cpu().numpy()
    for b in boxes_of(whd, rng, 24):
        sl = np.s_[b.z0:b.z0 + b.depth, b.y0:b.y0 + b.height, b.x0:b.x0 + b.width]
        for g, gs in ((grad, gn[sl]), (None, None)):
            got = device_hist(ctx, vol, g, box=b).cpu().numpy()
            assert np.array_equal(got, np_hist(vn[sl], gs)), "box %s, gradient %s" % ((b.x0, b.y0, b.z0, b.width, b.height, b.depth), g is not None)


# ---- 3. modes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whd", [(37, 29, 23), (160, 128, 64)])
def test_modes(ctx, whd):
    vol = torch.from_numpy(T.random_volume(whd, 77, sparsity=0.5)).cuda()
    grad = gradient_of(ctx, vol)
    want = torch.from_numpy(np_hist(vol.cpu().numpy(), grad.cpu().numpy())).cuda()
    h = torch.randint(-2 ** 62, 2 ** 62, (BINS,), dtype=torch.int64, device="cuda")  # garbage
    assert torch.equal(device_hist(ctx, vol, grad, out=h), want)
    device_hist(ctx, vol, grad, mode=abi.HISTOGRAM_ADD, out=h)
    assert torch.equal(h, 2 * want)
    device_hist(ctx, vol, grad, mode=abi.HISTOGRAM_SUBTRACT, out=h)
    device_hist(ctx, vol, grad, mode=abi.HISTOGRAM_SUBTRACT, out=h)
    assert torch.equal(h, torch.zeros_like(h))
    device_hist(ctx, vol, grad, mode=abi.HISTOGRAM_SUBTRACT, out=h)  # below zero: 2^64 - count, i.e. -count as int64
    assert torch.equal(h, -want)
    device_hist(ctx, vol, grad, mode=abi.HISTOGRAM_ADD, out=h)
    assert torch.equal(h, torch.zeros_like(h))


# ---- 4. contention and overflow -------------------------------------------------------------------------------------------------------
def test_constant_c3_volume(ctx):
    """one bin = 833 617 920: every workgroup's 16-bit counter of that bin spills many times"""
    vol = torch.full(C3[0][::-1], 77, dtype=torch.uint8, device="cuda")
    grad = gradient_of(ctx, vol)
    assert int(grad.max().item()) == 0
    for g, b in ((grad, 77), (None, 77)):
        h = device_hist(ctx, vol, g).cpu().numpy()
        assert h[b] == 1024 * 1024 * 795 == 833617920 and h.sum() == h[b]


def test_constant_volume_bin_above_2_to_32(ctx):
    """2048 x 2048 x 1025 voxels of one value, no gradient: one bin = 4 299 161 600 > 2^32"""
    vol = torch.full((1025, 2048, 2048), 201, dtype=torch.uint8, device="cuda")
    h = device_hist(ctx, vol, None).cpu().numpy()
    assert h[201] == 4299161600 > 2 ** 32 and h.sum() == h[201]
    del vol
    torch.cuda.empty_cache()


def test_uniform_random_bytes_fill_every_bin(ctx):
    g = torch.Generator(device="cuda").manual_seed(5)
    vol = torch.randint(0, 256, (256, 512, 512), dtype=torch.uint8, device="cuda", generator=g)
    grad = torch.randint(0, 256, (256, 512, 512), dtype=torch.uint8, device="cuda", generator=g)
    got = device_hist(ctx, vol, grad)
    assert int((got > 0).sum().item()) == BINS
    assert torch.equal(got, torch_hist(vol, grad))


def test_two_value_checkerboard(ctx):
    d, h, w = 100, 200, 300
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    vn = np.where((x + y + z) % 2 == 0, 10, 200).astype(np.uint8)
    check_whole(ctx, torch.from_numpy(vn).cuda())


# ---- 5. count -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vol_kind", ["c2_synthetic", "random"])
def test_count_equals_occupied_voxel_count(ctx, vol_kind):
    if vol_kind == "c2_synthetic":
        vol = synth(ctx, (416, 512, 112), 1, 0xC0FFEE02)
    else:
        vol = torch.from_numpy(T.random_volume((301, 203, 97), 11, sparsity=0.5)).cuda()
    ext = ext_of(vol)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    seen = []
    for opts in TF_CASES:
        tf = lib.transfer_function_uniform(abi.VolumeOptions(**opts))
        grad = gradient_of(ctx, vol, opts)
        for g in (grad, None):
            if g is None and tf.use_gradient:
                continue  # the documented limit: the on-the-fly float gradient is not in the histogram
            h = device_hist(ctx, vol, g)
            counts.fill_(-1)
            ctx.occupied_voxel_count(ptr(vol), ptr(g), tf, ext, ptr(counts[0:1]), st())
            ctx.histogram_occupied_count(ptr(h), tf, ptr(counts[1:2]), st())
            a, b = counts.tolist()
            assert a == b, "%s use_gradient %d gradient %s: %d != %d" % (opts, tf.use_gradient, g is not None, a, b)
            assert 0 <= a <= vol.numel()
            seen.append(a)
    assert max(seen) > 0 and min(seen) < vol.numel() and len(set(seen)) > 3


def test_count_is_stored_not_added(ctx):
    vol = torch.from_numpy(T.random_volume((50, 40, 30), 3)).cuda()
    h = device_hist(ctx, vol, gradient_of(ctx, vol))
    tf = lib.transfer_function_uniform(abi.VolumeOptions(**T.APP_TF))
    c = torch.full((1,), 123456789, dtype=torch.int64, device="cuda")
    ctx.histogram_occupied_count(ptr(h), tf, ptr(c), st())
    first = int(c.item())
    ctx.histogram_occupied_count(ptr(h), tf, ptr(c), st())
    assert int(c.item()) == first < 50 * 40 * 30


# ---- 6. a histogram kept across region updates ----------------------------------------------------------------------------------------
def grown(box, ext):
    org, size, e = (box.x0, box.y0, box.z0), (box.width, box.height, box.depth), ext.as_tuple()
    g0 = [max(o - 1, 0) for o in org]
    g1 = [min(o + s + 1, n) for o, s, n in zip(org, size, e)]
    return abi.Box(*g0, *[b - a for a, b in zip(g0, g1)])


@pytest.mark.parametrize("skip", [abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_histogram_kept_across_region_updates(ctx, skip):
    rng = np.random.default_rng(skip)
    vol = torch.from_numpy(T.random_volume((83, 61, 47), 300 + skip, sparsity=0.6)).cuda()
    state = State(ctx, vol, 4, T.APP_TF, "map", True, skip)
    hist = device_hist(ctx, state.vol, state.grad)
    for i in range(12):
        W, H, D = state.ext.as_tuple()
        w, h, d = [int(rng.integers(1, n // (2 if i % 3 else 1) + 1)) for n in (W, H, D)]
        box = abi.Box(int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), int(rng.integers(0, D - d + 1)), w, h, d)
        source = SOURCES[i % len(SOURCES)]
        src = make_source(rng, source, box, empty_share=0.5)
        g = grown(box, state.ext)
        device_hist(ctx, state.vol, state.grad, box=g, mode=abi.HISTOGRAM_SUBTRACT, out=hist)
        state.update(src, source, box)
        device_hist(ctx, state.vol, state.grad, box=g, mode=abi.HISTOGRAM_ADD, out=hist)
    assert torch.equal(hist, device_hist(ctx, state.vol, state.grad))
    assert torch.equal(hist, torch.from_numpy(np_hist(state.vol.cpu().numpy(), state.grad.cpu().numpy())).cuda())
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    ctx.occupied_voxel_count(ptr(state.vol), ptr(state.grad), state.tf, state.ext, ptr(counts[0:1]), st())
    ctx.histogram_occupied_count(ptr(hist), state.tf, ptr(counts[1:2]), st())
    a, b = counts.tolist()
    assert a == b > 0


# ---- 7. streams and graphs ------------------------------------------------------------------------------------------------------------
def test_histogram_and_count_captured_into_a_graph(ctx):
    vol = torch.from_numpy(T.random_volume((200, 150, 100), 21, sparsity=0.5)).cuda()
    grad = gradient_of(ctx, vol)
    tf = lib.transfer_function_uniform(abi.VolumeOptions(**T.APP_TF))
    hist = torch.zeros(BINS, dtype=torch.int64, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        ctx.volume_histogram(ptr(vol), ptr(grad), ext_of(vol), None, abi.HISTOGRAM_SET, ptr(hist), s.cuda_stream)
        ctx.histogram_occupied_count(ptr(hist), tf, ptr(count), s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ctx.volume_histogram(ptr(vol), ptr(grad), ext_of(vol), None, abi.HISTOGRAM_SET, ptr(hist), s.cuda_stream)
        ctx.histogram_occupied_count(ptr(hist), tf, ptr(count), s.cuda_stream)
    torch.cuda.synchronize()
    results = []
    for seed in (21, 22):
        if seed != 21:  # the volume rewritten in place, then the graph replayed
            vol.copy_(torch.from_numpy(T.random_volume((200, 150, 100), seed, sparsity=0.2)))
            grad.copy_(gradient_of(ctx, vol))
        hist.fill_(-7), count.fill_(-7)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (hist.clone(), int(count.item()))
        ref_h = device_hist(ctx, vol, grad)
        ref_c = torch.zeros(1, dtype=torch.int64, device="cuda")
        ctx.histogram_occupied_count(ptr(ref_h), tf, ptr(ref_c), st())
        assert torch.equal(got[0], ref_h) and got[1] == int(ref_c.item()), "replay with seed %d" % seed
        results.append(got[1])
    assert results[0] != results[1]
    del g


def test_two_volumes_on_two_streams(ctx):
    vols = [torch.from_numpy(T.random_volume((300, 250, 120), 40 + i, sparsity=0.3 * i)).cuda() for i in range(2)]
    grads = [gradient_of(ctx, v) for v in vols]
    want = [device_hist(ctx, v, g) for v, g in zip(vols, grads)]
    outs = [torch.full((BINS,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(3):
        for i in range(2):
            with torch.cuda.stream(streams[i]):
                ctx.volume_histogram(ptr(vols[i]), ptr(grads[i]), ext_of(vols[i]), None, abi.HISTOGRAM_SET, ptr(outs[i]), streams[i].cuda_stream)
        torch.cuda.synchronize()
        for i in range(2):
            assert torch.equal(outs[i], want[i]), "stream %d, repetition %d" % (i, rep)
            outs[i].fill_(-1)
    assert not torch.equal(want[0], want[1])


# ---- 8. argument checks ---------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_write_nothing(ctx):
    vol = torch.from_numpy(T.random_volume((20, 10, 6), 8)).cuda()
    grad = gradient_of(ctx, vol)
    e = ext_of(vol)
    buf = torch.full((BINS + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    h = buf[:BINS]
    misaligned = buf.data_ptr() + 4
    S = abi.HISTOGRAM_SET
    cases = [(None, ptr(grad), e, None, S, ptr(h)), (ptr(vol), ptr(grad), e, None, S, None), (ptr(vol), ptr(grad), abi.Extent3D(0, 10, 6), None, S, ptr(h)),
             (ptr(vol), ptr(grad), abi.Extent3D(20, 10, 0), None, S, ptr(h)), (ptr(vol), ptr(grad), e, abi.Box(0, 0, 0, 0, 1, 1), S, ptr(h)),
             (ptr(vol), ptr(grad), e, abi.Box(0, 0, 0, 1, 0, 1), S, ptr(h)), (ptr(vol), ptr(grad), e, abi.Box(0, 0, 0, 1, 1, 0), S, ptr(h)),
             (ptr(vol), ptr(grad), e, abi.Box(19, 0, 0, 2, 1, 1), S, ptr(h)), (ptr(vol), ptr(grad), e, abi.Box(0, 9, 0, 1, 2, 1), S, ptr(h)),
             (ptr(vol), ptr(grad), e, abi.Box(0, 0, 6, 1, 1, 1), S, ptr(h)), (ptr(vol), ptr(grad), e, abi.Box(0xFFFFFFFF, 0, 0, 2, 1, 1), S, ptr(h)),
             (ptr(vol), ptr(grad), e, None, 3, ptr(h)), (ptr(vol), ptr(grad), e, None, -1, ptr(h)),
             (ptr(vol), ptr(grad), e, None, abi.HISTOGRAM_ADD, misaligned)]
    before = buf.clone()
    for i, args in enumerate(cases):
        assert ctx.volume_histogram_rc(*args, st()) == abi.VKV_E_INVALID_ARGUMENT, "case %d" % i
        assert ctx.last_error().startswith("volume_histogram")
    tf = lib.transfer_function_uniform(abi.VolumeOptions(**T.APP_TF))
    for args in [(None, tf, ptr(buf[BINS:])), (ptr(h), None, ptr(buf[BINS:])), (ptr(h), tf, None), (misaligned, tf, ptr(buf[BINS:])),
                 (ptr(h), tf, misaligned)]:
        assert ctx.histogram_occupied_count_rc(*args, st()) == abi.VKV_E_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ---- 9. interfaces --------------------------------------------------------------------------------------------------------------------
def test_volume_wrapper_equals_the_c_call(ctx):
    for pre in (True, False):
        v = V.Volume(ctx)
        v.options = abi.VolumeOptions(**T.APP_TF)
        v.options.use_precomputed_gradient = 1 if pre else 0
        v.load_synthetic((96, 80, 72), 1, 0xC0FFEE06)
        if pre:
            V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
        hist = v.histogram()
        assert hist.shape == (256, 256) and hist.dtype == torch.int64
        assert torch.equal(hist.view(-1), device_hist(ctx, v.volume, v.gradient if pre else None))
        if not pre:
            assert int(hist[1:].sum().item()) == 0  # every voxel in gradient row 0
        box = ((5, 6, 7), (40, 30, 20))
        part = v.histogram(box=box)
        assert torch.equal(part.view(-1), device_hist(ctx, v.volume, v.gradient if pre else None, box=abi.Box(5, 6, 7, 40, 30, 20)))
        v.histogram(out=hist, box=box, mode=abi.HISTOGRAM_SUBTRACT)
        v.histogram(out=hist, box=abi.Box(5, 6, 7, 40, 30, 20), mode=abi.HISTOGRAM_ADD)
        assert torch.equal(hist.view(-1), device_hist(ctx, v.volume, v.gradient if pre else None))
        d_count = torch.zeros(2, dtype=torch.int64, device="cuda")
        v.occupied_count_from_histogram(hist, d_count[0:1])
        tf = v.get_transfer_function_uniform()
        ctx.occupied_voxel_count(ptr(v.volume), ptr(v.gradient if pre else None), tf, v.extent, ptr(d_count[1:2]), st())
        if pre or not tf.use_gradient:
            assert d_count[0].item() == d_count[1].item() > 0


def test_driver_writes_the_histogram_and_its_count(ctx, tmp_path):
    assert os.path.exists(EXE), "vkv_offscreen not built (run __graft_entry__.build())"
    out = subprocess.run([EXE, "--synthetic=96x80x72:1:5", "--width=64", "--height=64", "--benchmark=2", "--skipmode=2", "--histogram=h.bin"],
                         cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()
    text = out.stdout.decode()
    m_occ = re.search(r"Occupied voxels: ([\d\.e\-\+]+)%", text)
    m_hist = re.search(r"Occupied voxels \(histogram\): ([\d\.e\-\+]+)%", text)
    assert m_occ and m_hist, text
    assert m_hist.group(1) == m_occ.group(1)
    bins = np.fromfile(tmp_path / "h.bin", dtype="<u8")
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(**T.APP_TF)
    v.load_synthetic((96, 80, 72), 1, 5)
    V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
    want = v.histogram().view(-1).cpu().numpy().view(np.uint64)
    assert bins.shape == (BINS,) and np.array_equal(bins, want)

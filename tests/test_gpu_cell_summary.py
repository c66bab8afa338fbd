"""GPU: per-cell summaries (vkv_cell_summary) byte for byte against the numpy restatement over odd widths, odd offsets, blocks 1-8 and map
extents past the volume, with and without a gradient map; the occupancy map decided from them (vkv_occupancy_map_from_summary) byte for byte
against vkv_occupancy_map, with the unresolved-cell count against the restated rule; the whole slider-move update against
vkv_update_transfer_function; summaries kept across vkv_update_volume_region; graphs, streams, argument errors and the driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_cell_summary_cpu import UNRESOLVED, bits_words, classify_np, occupancy_np, summary_np
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vkvolume_amd", "csrc", "vkv_offscreen")
SB = abi.CELL_SUMMARY_BYTES
TF_CASES = [dict(), T.APP_TF, dict(intensity_min=0.4, intensity_max=0.8, gradient_min=0.0, gradient_max=0.0),
            dict(intensity_min=0.2, intensity_max=0.8, gradient_min=0.06, gradient_max=0.12),
            dict(intensity_min=0.5, intensity_max=0.5),  # degenerate intensity window
            dict(intensity_min=0.3, intensity_max=0.3, gradient_min=0.0, gradient_max=0.2),
            dict(intensity_min=0.05, intensity_max=0.6, gradient_min=0.1, gradient_max=0.1),  # use_gradient 0
            dict(intensity_min=1.0, intensity_max=1.0, gradient_min=1.0, gradient_max=1.0),  # nothing occupied
            dict(intensity_min=-1.0, intensity_max=0.0, gradient_min=-1.0, gradient_max=0.0)]  # everything occupied


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def ext(w, h, d):
    return abi.Extent3D(w, h, d)


def at_offset(arr, off):
    """a CUDA copy of `arr` that starts `off` bytes past an allocation's start (odd alignments of the rows)"""
    buf = torch.zeros(arr.size + off + 16, dtype=torch.uint8, device="cuda")
    t = buf[off:off + arr.size].view(arr.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(arr)))
    return t


def device_summary(ctx, vol, grad, me, box=None, out=None):
    d, h, w = vol.shape
    out = torch.full((me[0] * me[1] * me[2], SB), 0xA5, dtype=torch.uint8, device="cuda") if out is None else out
    ctx.cell_summary(ptr(vol), ptr(grad), ext(w, h, d), ext(*me), box, ptr(out), st())
    torch.cuda.synchronize()
    return out


def tf_of(opts):
    o = abi.VolumeOptions(**opts)
    return o, lib.transfer_function_uniform(o), lib.transfer_function_texture(o)


def bits_of_texture(tex):
    return np.asarray(tex).reshape(256, 256, 4)[..., 3] > 0


def gradient_of(ctx, vol, opts=T.APP_TF):
    d, h, w = vol.shape
    grad = torch.zeros_like(vol)
    ctx.gradient_map(ptr(vol), ptr(grad), ext(w, h, d), lib.transfer_function_uniform(abi.VolumeOptions(**opts)), st())
    return grad


def maps_pair(ctx, vol, grad, tex_t, tf, me, summ):
    """(vkv_occupancy_map, vkv_occupancy_map_from_summary, unresolved) for one texture"""
    d, h, w = vol.shape
    n = me[0] * me[1] * me[2]
    ref = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    got = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    unres = torch.full((1,), 12345, dtype=torch.int64, device="cuda")
    ctx.occupancy_map(ptr(vol), ptr(grad), ptr(tex_t), tf, ext(w, h, d), ptr(ref), ext(*me), st())
    ctx.occupancy_map_from_summary(ptr(summ), ptr(vol), ptr(grad), ptr(tex_t), tf, ext(w, h, d), ptr(got), ext(*me), ptr(unres), st())
    torch.cuda.synchronize()
    return ref.cpu().numpy(), got.cpu().numpy(), int(unres.item())


# ---- 1. summary bytes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 5, 4), (5, 7, 6), (6, 9, 5), (7, 4, 3), (33, 17, 9), (66, 20, 11), (131, 9, 7), (300, 5, 6), (1029, 3, 2)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_grad", [True, False])
def test_summary_bytes_equal_the_restatement(ctx, shape, with_grad):
    w, h, d = shape
    rng = np.random.default_rng(w * 7 + h)
    vol_np = rng.integers(0, 256, (d, h, w)).astype(np.uint8)
    grad_np = rng.integers(0, 256, (d, h, w)).astype(np.uint8)
    for off in (0, 1, 2, 3):
        vol = at_offset(vol_np, off)
        grad = at_offset(grad_np, (off + 1) % 4) if with_grad else None
        for b in range(1, 9):
            me = tuple(min(e, (e + b - 1) // b) for e in (w, h, d))
            got = device_summary(ctx, vol, grad, me).cpu().numpy()
            want = summary_np(vol_np, grad_np if with_grad else None, me)
            assert np.array_equal(got, want), "offset %d block %d: %d cells differ" % (off, b, int((got != want).any(-1).sum()))
        # map extents past the volume (ceil(extent / block) + 1: the last cells hold no voxel and are all zero), and one cell per axis
        for me in [tuple(min(e, (e + b - 1) // b + 1) for e in (w, h, d)) for b in (3, 4)] + [(1, 1, 1)]:
            got = device_summary(ctx, vol, grad, me).cpu().numpy()
            assert np.array_equal(got, summary_np(vol_np, grad_np if with_grad else None, me)), me


def test_summary_of_a_box_rebuilds_exactly_the_cells_it_meets(ctx):
    rng = np.random.default_rng(5)
    w, h, d, b = 45, 38, 29, 4
    me = tuple((e + b - 1) // b for e in (w, h, d))
    vol_np = rng.integers(0, 256, (d, h, w)).astype(np.uint8)
    vol = torch.from_numpy(vol_np).cuda()
    want = summary_np(vol_np, None, me).reshape(me[2], me[1], me[0], SB)
    for box in (abi.Box(0, 0, 0, 1, 1, 1), abi.Box(5, 9, 3, 7, 1, 13), abi.Box(44, 37, 28, 1, 1, 1), abi.Box(0, 0, 0, w, h, d)):
        out = torch.full((me[0] * me[1] * me[2], SB), 0xA5, dtype=torch.uint8, device="cuda")
        got = device_summary(ctx, vol, None, me, box=box, out=out).cpu().numpy().reshape(me[2], me[1], me[0], SB)
        cx = slice(box.x0 // b, (box.x0 + box.width - 1) // b + 1)
        cy = slice(box.y0 // b, (box.y0 + box.height - 1) // b + 1)
        cz = slice(box.z0 // b, (box.z0 + box.depth - 1) // b + 1)
        assert np.array_equal(got[cz, cy, cx], want[cz, cy, cx])
        untouched = np.ones(got.shape[:3], bool)
        untouched[cz, cy, cx] = False
        assert (got[untouched] == 0xA5).all()


# ---- 2. the map and the unresolved count ----------------------------------------------------------------------------------------------
def scenes(ctx):
    w, h, d = 97, 70, 53
    shells = torch.empty((d, h, w), dtype=torch.uint8, device="cuda")
    ctx.synth_volume(ptr(shells), ext(w, h, d), 1, 0xC0FFEE03, st())
    noise = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (d, h, w)).astype(np.uint8)).cuda()
    const = torch.full((d, h, w), 77, dtype=torch.uint8, device="cuda")
    return {"shells": shells, "noise": noise, "constant": const}


@pytest.mark.parametrize("block", [2, 4, 6])
@pytest.mark.parametrize("with_grad", [True, False])
def test_map_from_summary_equals_the_occupancy_map(ctx, block, with_grad):
    for name, vol in scenes(ctx).items():
        d, h, w = vol.shape
        me = tuple((e + block - 1) // block for e in (w, h, d))
        grad = gradient_of(ctx, vol) if with_grad else None
        summ = device_summary(ctx, vol, grad, me)
        vol_np, grad_np = vol.cpu().numpy(), None if grad is None else grad.cpu().numpy()
        summ_np = summ.cpu().numpy()
        assert np.array_equal(summ_np, summary_np(vol_np, grad_np, me))
        for opts in TF_CASES:
            _, tf, tex = tf_of(opts)
            if tf.use_gradient and not with_grad:
                continue  # the on-the-fly gradient: refused (test_argument_errors_write_nothing)
            tex_t = torch.from_numpy(np.ascontiguousarray(tex)).cuda()
            ref, got, unres = maps_pair(ctx, vol, grad, tex_t, tf, me, summ)
            assert np.array_equal(got, ref), "%s %r: %d cells differ" % (name, opts, int((got != ref).sum()))
            bits = bits_of_texture(tex)
            assert unres == int((classify_np(summ_np, bits, tf.use_gradient) == UNRESOLVED).sum()), (name, opts)
            assert np.array_equal(ref, occupancy_np(vol_np, grad_np, bits, tf.use_gradient, me).reshape(-1))


@pytest.mark.parametrize("seed", range(4))
def test_map_from_summary_of_a_random_texture(ctx, seed):
    rng = np.random.default_rng(100 + seed)
    w, h, d = int(rng.integers(4, 90)), int(rng.integers(1, 40)), int(rng.integers(1, 30))
    vol_np = rng.integers(0, 256, (d, h, w)).astype(np.uint8)
    grad_np = (vol_np // 3 + rng.integers(0, 40, (d, h, w))).astype(np.uint8)
    vol, grad = at_offset(vol_np, seed), at_offset(grad_np, 3 - seed)
    tex = np.zeros((256, 256, 4), np.uint8)
    for k in range(4):  # arbitrary tables: noise of several densities, then blocks
        tex[..., 3] = (rng.random((256, 256)) < (0.002, 0.05, 0.5, 0.99)[k]) * rng.integers(1, 256)
        if k == 3:
            tex[..., 3] = 0
            tex[40:90, 100:220, 3] = 9
        tex_t = torch.from_numpy(tex.copy()).cuda()
        for b in (1, 3, 4, 8):
            me = tuple(min(e, (e + b - 1) // b) for e in (w, h, d))
            summ = device_summary(ctx, vol, grad, me)
            for use_gradient in (1, 0):
                tf = lib.transfer_function_uniform(abi.VolumeOptions(**T.APP_TF))
                tf.use_gradient = use_gradient
                ref, got, unres = maps_pair(ctx, vol, grad, tex_t, tf, me, summ)
                assert np.array_equal(got, ref), (k, b, use_gradient)
                assert unres == int((classify_np(summ.cpu().numpy(), tex[..., 3] > 0, use_gradient) == UNRESOLVED).sum())
    assert bits_words(tex[..., 3] > 0).shape == (2048,)


# ---- 3. the whole update ---------------------------------------------------------------------------------------------------------------
def make_volume(ctx, vol_dhw, opts, block, precomputed=True):
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(use_precomputed_gradient=precomputed, **opts)
    v.load_from_array(vol_dhw, block)
    if precomputed:
        V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
    return v


def snapshot(v):
    torch.cuda.synchronize()
    return [m.cpu().numpy() for m in v.distance_maps], v.transfer_function.cpu().numpy(), v.transfer_function_bits.cpu().numpy()


def poison(v):
    for m in v.distance_maps:
        m.fill_(0x5A)
    v.transfer_function.fill_(0x5A)
    v.transfer_function_bits.fill_(-1)


@pytest.mark.parametrize("skipping_type", [abi.SKIP_NONE, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
@pytest.mark.parametrize("precomputed", [True, False])
def test_update_from_summary_equals_the_update(ctx, skipping_type, precomputed):
    for i, opts in enumerate([T.APP_TF, dict(T.APP_TF, intensity_min=0.35), TF_CASES[6], TF_CASES[4]]):
        if precomputed is False and lib.transfer_function_uniform(abi.VolumeOptions(**opts)).use_gradient:
            continue
        v = make_volume(ctx, O.synth_volume((96, 80, 72), 1, 0xC0FFEE02 + i), opts, (4, 3, 5, 2)[i], precomputed)
        ref_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        v.update_transfer_function(skipping_type, ref_count)
        ref = snapshot(v)
        poison(v)
        v.build_cell_summary()
        hist = v.histogram()
        count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        unres = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        v.update_transfer_function_from_summary(skipping_type, count, hist, unres)
        got = snapshot(v)
        assert len(got[0]) == (8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1)
        for k, (a, b) in enumerate(zip(got[0], ref[0])):
            assert np.array_equal(a, b), "map %d" % k
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert int(count.item()) == int(ref_count.item())
        assert 0 <= int(unres.item()) <= v.distance_maps[0].numel()


# ---- 4. region edits ------------------------------------------------------------------------------------------------------------------
def test_summary_kept_across_region_updates(ctx):
    rng = np.random.default_rng(11)
    w, h, d = 83, 61, 47
    v = make_volume(ctx, O.synth_volume((w, h, d), 1, 0xC0FFEE09), T.APP_TF, 4)
    v.update_transfer_function_texture()
    V.ComputeDistanceMap(ctx).compute(v, v.get_transfer_function_uniform(), abi.SKIP_ANISOTROPIC_DISTANCE)
    v.build_cell_summary()
    me = v.map_extent
    for origin, size in (((0, 0, 0), (1, 1, 1)), ((10, 20, 5), (17, 9, 13)), ((82, 60, 46), (1, 1, 1)), ((40, 0, 30), (43, 61, 1))):
        box = rng.integers(0, 256, (size[2], size[1], size[0])).astype(np.uint8)
        v.update_region(origin, box, abi.SKIP_ANISOTROPIC_DISTANCE)  # rebuilds the grown box of the summary
        torch.cuda.synchronize()
        full = device_summary(ctx, v.volume, v.gradient, (me.width, me.height, me.depth))
        assert torch.equal(v.cell_summary, full)
        tf = v.get_transfer_function_uniform()
        n = me.width * me.height * me.depth
        ref = torch.empty(n, dtype=torch.uint8, device="cuda")
        got = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctx.occupancy_map(ptr(v.volume), ptr(v.gradient), ptr(v.transfer_function), tf, v.extent, ptr(ref), me, st())
        ctx.occupancy_map_from_summary(ptr(v.cell_summary), ptr(v.volume), ptr(v.gradient), ptr(v.transfer_function), tf, v.extent, ptr(got), me,
                                       None, st())
        torch.cuda.synchronize()
        assert torch.equal(got, ref)


# ---- 5. hipGraph and streams ----------------------------------------------------------------------------------------------------------
def test_update_from_summary_captured_into_a_graph(ctx):
    v = make_volume(ctx, O.synth_volume((96, 80, 72), 1, 0xC0FFEE06), dict(T.APP_TF, intensity_min=0.13), 4)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # one direct call on the capture stream: its scratch block, the maps and the summary exist
        v.build_cell_summary()
        hist = v.histogram()
        v.update_transfer_function_from_summary(abi.SKIP_ANISOTROPIC_DISTANCE)
    torch.cuda.synchronize()
    count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    unres = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        v.update_transfer_function_from_summary(abi.SKIP_ANISOTROPIC_DISTANCE, count, hist, unres)
    torch.cuda.synchronize()
    for seed in (0xC0FFEE06, 0xC0FFEE07):  # the second replay after the volume, its gradient, summary and histogram changed in place
        if seed != 0xC0FFEE06:
            v.volume.copy_(torch.from_numpy(O.synth_volume((96, 80, 72), 1, seed)))
            V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
            v.build_cell_summary()
            v.histogram(out=hist)
        poison(v)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got, got_count = snapshot(v), int(count.item())
        poison(v)
        ref_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE, ref_count)
        ref = snapshot(v)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(got[1], ref[1]) and got_count == int(ref_count.item()) and int(unres.item()) >= 0
    del g
    ctx.release_stream(s.cuda_stream)


def test_two_volumes_on_two_streams(ctx):
    vols = [make_volume(ctx, O.synth_volume((96, 80, 72), 1, 0xC0FFEE08 + i), dict(T.APP_TF, intensity_min=0.1 + 0.05 * i), 4) for i in range(2)]
    serial = []
    for v in vols:
        v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE)
        serial.append(snapshot(v))
        v.build_cell_summary()
        poison(v)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for v, s in zip(vols, streams):
            with torch.cuda.stream(s):
                v.update_transfer_function_from_summary(abi.SKIP_ANISOTROPIC_DISTANCE)
    torch.cuda.synchronize()
    for v, ref in zip(vols, serial):
        got = snapshot(v)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    for s in streams:
        ctx.release_stream(s.cuda_stream)


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(ctx):
    w, h, d = 20, 16, 12
    vol = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (d, h, w)).astype(np.uint8)).cuda()
    grad = gradient_of(ctx, vol)
    e, me = ext(w, h, d), ext(5, 4, 3)
    n = 5 * 4 * 3
    summ = torch.full((n + 1, SB), 0xA5, dtype=torch.uint8, device="cuda")
    mp = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    tex = torch.from_numpy(np.ascontiguousarray(lib.transfer_function_texture(abi.VolumeOptions(**T.APP_TF)))).cuda()
    tf = lib.transfer_function_uniform(abi.VolumeOptions(**T.APP_TF))
    inv, uns = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED
    S = ptr(summ)
    torch.cuda.synchronize()
    assert ctx.cell_summary_rc(ptr(vol), ptr(grad), e, me, None, None, st()) == inv
    assert ctx.cell_summary_rc(None, ptr(grad), e, me, None, S, st()) == inv
    assert ctx.cell_summary_rc(ptr(vol), ptr(grad), e, me, None, S + 8, st()) == inv  # misaligned
    assert ctx.cell_summary_rc(ptr(vol), ptr(grad), e, ext(21, 4, 3), None, S, st()) == inv  # map wider than the volume
    assert ctx.cell_summary_rc(ptr(vol), ptr(grad), e, ext(0, 4, 3), None, S, st()) == inv
    assert ctx.cell_summary_rc(ptr(vol), ptr(grad), e, me, abi.Box(15, 0, 0, 6, 1, 1), S, st()) == inv  # past the volume
    assert ctx.cell_summary_rc(ptr(vol), ptr(grad), e, me, abi.Box(0, 0, 0, 0, 1, 1), S, st()) == inv  # empty
    M = ptr(mp)
    assert ctx.occupancy_map_from_summary_rc(None, ptr(vol), ptr(grad), ptr(tex), tf, e, M, me, None, st()) == inv
    assert ctx.occupancy_map_from_summary_rc(S + 4, ptr(vol), ptr(grad), ptr(tex), tf, e, M, me, None, st()) == inv
    assert ctx.occupancy_map_from_summary_rc(S, ptr(vol), ptr(grad), None, tf, e, M, me, None, st()) == inv
    assert ctx.occupancy_map_from_summary_rc(S, ptr(vol), ptr(grad), ptr(tex), tf, e, M, ext(5, 17, 3), None, st()) == inv
    assert ctx.occupancy_map_from_summary_rc(S, ptr(vol), ptr(grad), ptr(tex), tf, e, M, me, M + 3, st()) == inv  # misaligned d_unresolved
    assert ctx.occupancy_map_from_summary_rc(S, ptr(vol), None, ptr(tex), tf, e, M, me, None, st()) == uns  # on-the-fly gradient
    o = abi.VolumeOptions(use_precomputed_gradient=True, **T.APP_TF)
    maps = [M] * 8
    tables = torch.zeros(abi.TF_BITS_WORDS, dtype=torch.int32, device="cuda")
    swap = torch.zeros(n, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    hist = torch.zeros(65536, dtype=torch.int64, device="cuda")
    args = lambda **k: dict(dict(options=o, d_volume=ptr(vol), d_gradient=ptr(grad), extent=e, d_tf=ptr(tex), d_tables=ptr(tables), d_maps=[M],  # noqa: E731
                                 d_swap=ptr(swap), map_extent=me, skipping_type=abi.SKIP_NONE, d_count=None, d_summary=S, d_histogram=None,
                                 d_unresolved=None), **k)
    bad = [args(d_summary=None), args(d_summary=S + 1), args(d_count=ptr(cnt)), args(d_count=ptr(cnt) + 4, d_histogram=ptr(hist)),
           args(d_histogram=ptr(hist) + 2, d_count=ptr(cnt)), args(skipping_type=7), args(d_maps=None), args(skipping_type=abi.SKIP_DISTANCE, d_swap=None),
           args(skipping_type=abi.SKIP_DISTANCE, d_swap=M), args(d_tables=ptr(tables) + 2), args(map_extent=ext(21, 1, 1)), args(options=None)]
    for a in bad:
        assert ctx.update_transfer_function_from_summary_rc(**a) == inv, a
    assert ctx.update_transfer_function_from_summary_rc(**args(d_gradient=None)) == uns
    # map rows too long for the distance transform: refused before the count, the texture or the classification is enqueued
    e2 = ext(2049, 1, 1)
    vol2 = torch.zeros((1, 1, 2049), dtype=torch.uint8, device="cuda")
    summ2 = torch.zeros((2049, SB), dtype=torch.uint8, device="cuda")
    tex2 = torch.full((256, 256, 4), 7, dtype=torch.uint8, device="cuda")
    tables2 = torch.full((abi.TF_BITS_WORDS,), 7, dtype=torch.int32, device="cuda")
    cnt2 = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    map2, swap2 = (torch.full((2049,), 7, dtype=torch.uint8, device="cuda") for _ in range(2))
    rc = ctx.update_transfer_function_from_summary_rc(**args(d_volume=ptr(vol2), d_gradient=ptr(vol2), extent=e2, d_tf=ptr(tex2), d_tables=ptr(tables2),
                                                            d_maps=[ptr(map2)], d_swap=ptr(swap2), map_extent=e2, skipping_type=abi.SKIP_DISTANCE,
                                                            d_count=ptr(cnt2), d_summary=ptr(summ2), d_histogram=ptr(hist)))
    assert rc == uns, rc
    err = ctx.last_error()
    torch.cuda.synchronize()
    assert (summ == 0xA5).all() and (mp == 0x5A).all() and (tables == 0).all() and (swap == 0).all()
    assert all((t == 7).all() for t in (tex2, tables2, cnt2, map2, swap2))
    assert err.startswith("update_transfer_function_from_summary:"), err


# ---- 7. the C++ driver -----------------------------------------------------------------------------------------------------------------
def test_offscreen_tf_drag_summary_frames_equal_device(tmp_path):
    assert os.path.exists(EXE), "vkv_offscreen not built (run __graft_entry__.build())"
    frames = {}
    for path in ("device", "summary"):
        out = tmp_path / ("%s.raw" % path)
        r = subprocess.run([EXE, "--width=192", "--height=128", "--skipmode=3", "--synthetic=72x64x56:1:7", "--tf-drag=4", "--tf-path=%s" % path,
                            "--dump-rgba8=%s" % out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "tf-drag %s: 4 moves" % path in r.stdout, r.stdout
        frames[path] = out.read_bytes()
        if path == "summary":
            assert "tf-drag summary: unresolved cells" in r.stdout, r.stdout
    assert len(frames["device"]) == 192 * 128 * 4 and frames["device"] == frames["summary"]
    assert any(frames["device"])

"""GPU: the transfer-function update on the device (vkv_transfer_function_texture_device, vkv_update_transfer_function) against the
blocking host path (CPU texture, upload, wait, vkv_transfer_function_tables, vkv_compute_distance_map): texture, tables, scratch bit table,
maps, count and frames bit for bit; queued slider moves, hipGraph capture, two streams, the C++ mirror and the argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_gpu_parity import compare_render, gpu_render
from tests.test_tf_update_cpu import option_sets
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vkvolume_amd", "csrc", "vkv_offscreen")
SCRATCH_WORDS = 2048 + 8


def st():
    return torch.cuda.current_stream().cuda_stream


def words(t):
    return t.cpu().numpy().view(np.uint32)


def tiny_volume():
    d_vol = torch.from_numpy(np.arange(64, dtype=np.uint8).reshape(4, 4, 4) * 4).cuda()
    return d_vol, abi.Extent3D(4, 4, 4), abi.Extent3D(1, 1, 1)


def host_tf(ctx, opt, d_vol, ext, mext):
    """The existing path: host texture, vkv_transfer_function_tables, and the bit table k_tf_bits + k_tf_columns leave in the scratch."""
    tex = lib.transfer_function_texture(opt)
    d_tex = torch.from_numpy(tex).cuda()
    d_tab = torch.full((abi.TF_BITS_WORDS,), -1, dtype=torch.int32, device="cuda")
    ctx.transfer_function_tables(d_tex.data_ptr(), lib.transfer_function_uniform(opt), d_tab.data_ptr(), st())
    d_map = torch.empty(1, dtype=torch.uint8, device="cuda")
    ctx.occupancy_map(d_vol.data_ptr(), None, d_tex.data_ptr(), lib.transfer_function_uniform(opt), ext, d_map.data_ptr(), mext, st())
    d_scr = torch.full((SCRATCH_WORDS,), -1, dtype=torch.int32, device="cuda")
    ctx.debug_tf_scratch(d_scr.data_ptr(), st())
    return tex, words(d_tab), words(d_scr)


def device_tf(ctx, opt, d_vol, ext, mext):
    d_tex = torch.full((256, 256, 4), 0x5A, dtype=torch.uint8, device="cuda")
    d_tab = torch.full((abi.TF_BITS_WORDS,), -1, dtype=torch.int32, device="cuda")
    d_map = torch.empty(1, dtype=torch.uint8, device="cuda")
    ctx.update_transfer_function(opt, d_vol.data_ptr(), None, ext, d_tex.data_ptr(), d_tab.data_ptr(), [d_map.data_ptr()], None, mext, abi.SKIP_BLOCK,
                                 None, st())
    d_scr = torch.full((SCRATCH_WORDS,), -1, dtype=torch.int32, device="cuda")
    ctx.debug_tf_scratch(d_scr.data_ptr(), st())
    # the texture-only entry point writes the same texture and tables
    d_tex2 = torch.full((256, 256, 4), 0xA5, dtype=torch.uint8, device="cuda")
    d_tab2 = torch.zeros((abi.TF_BITS_WORDS,), dtype=torch.int32, device="cuda")
    ctx.transfer_function_texture_device(opt, d_tex2.data_ptr(), d_tab2.data_ptr(), st())
    tex = d_tex.cpu().numpy()
    assert np.array_equal(tex, d_tex2.cpu().numpy()) and np.array_equal(words(d_tab), words(d_tab2))
    return tex, words(d_tab), words(d_scr)


# ---- 1. texture, tables, scratch bit table ------------------------------------------------------------------------------------------
def test_texture_tables_and_scratch_bits_bit_exact(ctx):
    d_vol, ext, mext = tiny_volume()
    bad = []
    for name, opts in option_sets():
        opt = abi.VolumeOptions(**opts)
        h_tex, h_tab, h_scr = host_tf(ctx, opt, d_vol, ext, mext)
        d_tex, d_tab, d_scr = device_tf(ctx, opt, d_vol, ext, mext)
        if not np.array_equal(d_tex, h_tex):
            bad.append("%s: %d texels differ" % (name, int((d_tex != h_tex).any(-1).sum())))
        if not np.array_equal(d_tab, h_tab):
            bad.append("%s: table words %s differ" % (name, np.nonzero(d_tab != h_tab)[0][:8]))
        if not np.array_equal(d_scr, h_scr):
            bad.append("%s: scratch words %s differ" % (name, np.nonzero(d_scr != h_scr)[0][:8]))
    assert not bad, "\n".join(bad[:20])


def test_degenerate_window_texel_is_zero(ctx):
    """intensity_max == intensity_min on a texel centre: the host product there is NaN and (uint8) NaN is 0 on x86-64; the device writes 0."""
    x = np.float32(100) / np.float32(255)
    opt = abi.VolumeOptions(intensity_min=x, intensity_max=x, gradient_min=0.0, gradient_max=0.2)
    d_vol, ext, mext = tiny_volume()
    tex, tab, _ = device_tf(ctx, opt, d_vol, ext, mext)
    assert (tex[:, 100] == 0).all() and (tex[52:, 101:, 3] == 255).all() and (tex[:, :100] == 0).all()
    assert np.isnan(tab[2052 + 100:2052 + 101].view(np.float32)).all()


# ---- 2. maps and count ------------------------------------------------------------------------------------------------------------
def make_volume(ctx, vol_dhw, opts, grad_mode, block):
    v = V.Volume(ctx)
    o = dict(opts)
    if grad_mode == "off":
        o["gradient_min"] = o["gradient_max"] = 0.25
    v.options = abi.VolumeOptions(use_precomputed_gradient=grad_mode == "precomputed", **o)
    v.load_from_array(vol_dhw, block)
    V.default_scene(v)
    if grad_mode == "precomputed":
        V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
    return v


def host_update(ctx, v, skipping_type):
    v.update_transfer_function_texture()
    V.ComputeDistanceMap(ctx).compute(v, v.get_transfer_function_uniform(), skipping_type)


def snapshot(v):
    torch.cuda.synchronize()
    return ([m.cpu().numpy() for m in v.distance_maps], v.transfer_function.cpu().numpy(), v.transfer_function_bits.cpu().numpy())


def poison(v):
    for m in v.distance_maps:
        m.fill_(0x5A)
    v.transfer_function.fill_(0x5A)
    v.transfer_function_bits.fill_(-1)


def check_maps_and_count(ctx, vol, opts, grad_mode, block, skipping_type):
    v = make_volume(ctx, vol, opts, grad_mode, block)
    host_update(ctx, v, skipping_type)
    h_maps, h_tex, h_tab = snapshot(v)
    grad = v.gradient if v.options.use_precomputed_gradient else None
    h_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ctx.occupied_voxel_count(v.volume.data_ptr(), None if grad is None else grad.data_ptr(), v.get_transfer_function_uniform(), v.extent,
                             h_count.data_ptr(), st())
    poison(v)
    d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    v.update_transfer_function(skipping_type, d_count)
    d_maps, d_tex, d_tab = snapshot(v)
    assert len(d_maps) == len(h_maps) == (8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1)
    for k, (a, b) in enumerate(zip(d_maps, h_maps)):
        assert np.array_equal(a, b), "map %d: %d cells differ" % (k, int((a != b).sum()))
    assert np.array_equal(d_tex, h_tex) and np.array_equal(d_tab, h_tab)
    assert int(d_count.item()) == int(h_count.item())
    return v


SKIPS = [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE]


@pytest.mark.parametrize("skipping_type", SKIPS)
@pytest.mark.parametrize("grad_mode", ["precomputed", "on_the_fly", "off"])
@pytest.mark.parametrize("shape,block,seed", [((73, 64, 57), 2, 1), ((4, 5, 6), 3, 2), ((96, 80, 72), 4, 3), ((130, 70, 41), 5, 4), ((64, 64, 64), 6, 5)])
def test_maps_and_count_bit_exact(ctx, skipping_type, grad_mode, shape, block, seed):
    vol = O.synth_volume(shape, 1, 0xC0FFEE00 + seed) if seed % 2 else T.random_volume(shape, seed, sparsity=0.6)
    opts = dict(intensity_min=0.05 * seed, intensity_max=0.9, gradient_min=0.0, gradient_max=0.2)
    check_maps_and_count(ctx, vol, opts, grad_mode, block, skipping_type)


@pytest.mark.parametrize("skipping_type", [abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
def test_maps_and_count_bit_exact_c3_size(ctx, skipping_type):
    w, h, d = 1024, 1024, 795
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(**T.APP_TF)
    v.load_synthetic((w, h, d), 1, 0xC0FFEE03)
    vol = v.volume
    del v
    check_maps_and_count(ctx, vol, T.APP_TF, "precomputed", 4, skipping_type)


# ---- 3. frames ----------------------------------------------------------------------------------------------------------------------
def draw(ctx, v, skipping_type, size=(160, 96), az=30.0, rgba8=None, counts=None):
    ro = abi.RenderOptions(skipping_type=skipping_type, clip_distance=1.0)
    sp = V.VolumeRenderSubpass(ctx, v, ro, size)
    view, proj = T.orbit(az, image_size=size)
    p = sp.make_params(view, proj)
    own = rgba8 is None
    if own:
        rgba8 = torch.zeros((size[1], size[0], 4), dtype=torch.uint8, device="cuda")
        counts = torch.zeros((size[1], size[0], 3), dtype=torch.int32, device="cuda")
    sp.draw(p, rgba8=rgba8, counts=counts)
    return rgba8, counts


@pytest.mark.parametrize("skipping_type", SKIPS)
def test_frames_after_device_update_equal_host_update(ctx, skipping_type):
    vol = O.synth_volume((96, 80, 72), 1, 0xC0FFEE02)
    v = make_volume(ctx, vol, T.APP_TF, "precomputed", 4)
    host_update(ctx, v, skipping_type)
    h = [t.cpu().numpy() for t in draw(ctx, v, skipping_type)]
    poison(v)
    v.update_transfer_function(skipping_type)
    d = [t.cpu().numpy() for t in draw(ctx, v, skipping_type)]
    assert h[1][..., 0].sum() > 0
    assert np.array_equal(d[0], h[0]) and np.array_equal(d[1], h[1])


def test_frame_after_device_update_matches_oracle(ctx):
    scene = T.OracleScene(O.synth_volume((96, 80, 72), 1, 0xC0FFEE02), abi.VolumeOptions(**T.APP_TF), 4)
    v = V.Volume(ctx)
    v.options = scene.options
    v.load_from_array(scene.vol, scene.block, scene.image_transform)
    v.node_transform = scene.node_transform
    V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
    v.update_transfer_function(abi.SKIP_DISTANCE)
    size = (128, 80)
    view, proj = T.orbit(40.0, image_size=size)
    params = scene.params(view, proj, size, abi.RenderOptions(skipping_type=abi.SKIP_DISTANCE, clip_distance=1.0))
    ref = scene.render(params)
    assert ref.counts[..., 0].sum() > 0
    compare_render(gpu_render(ctx, v, params), ref, "device TF update")


# ---- 4. queued slider moves -----------------------------------------------------------------------------------------------------
def slider(k):
    return 0.04 + 0.03 * k


def test_queued_slider_moves_without_host_waits(ctx):
    vol = O.synth_volume((96, 80, 72), 1, 0xC0FFEE05)
    v = make_volume(ctx, vol, T.APP_TF, "precomputed", 4)
    host_update(ctx, v, abi.SKIP_DISTANCE)
    draw(ctx, v, abi.SKIP_DISTANCE)  # packs the volume: nothing below allocates
    torch.cuda.synchronize()
    size = (160, 96)
    outs = [(torch.zeros((size[1], size[0], 4), dtype=torch.uint8, device="cuda"), torch.zeros((size[1], size[0], 3), dtype=torch.int32, device="cuda"))
            for _ in range(8)]
    for k in range(8):  # 8 moves, each followed by its frame, no sync in between
        v.options.intensity_min = slider(k)
        v.update_transfer_function(abi.SKIP_DISTANCE)
        draw(ctx, v, abi.SKIP_DISTANCE, size, rgba8=outs[k][0], counts=outs[k][1])
    torch.cuda.synchronize()
    for k in range(8):
        v.options.intensity_min = slider(k)
        host_update(ctx, v, abi.SKIP_DISTANCE)
        h = [t.cpu().numpy() for t in draw(ctx, v, abi.SKIP_DISTANCE, size)]
        assert np.array_equal(outs[k][0].cpu().numpy(), h[0]) and np.array_equal(outs[k][1].cpu().numpy(), h[1]), "move %d" % k
    assert not np.array_equal(outs[0][1].cpu().numpy(), outs[7][1].cpu().numpy())


# ---- 5. hipGraph ---------------------------------------------------------------------------------------------------------------------
def test_update_and_frame_captured_into_a_graph(ctx):
    size = (160, 96)
    v = make_volume(ctx, O.synth_volume((96, 80, 72), 1, 0xC0FFEE06), T.APP_TF, "precomputed", 4)
    v.options.intensity_min = 0.13
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_ANISOTROPIC_DISTANCE, clip_distance=1.0), size)
    view, proj = T.orbit(50.0, image_size=size)
    rgba8 = torch.zeros((size[1], size[0], 4), dtype=torch.uint8, device="cuda")
    counts = torch.zeros((size[1], size[0], 3), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # one direct call on the capture stream: its scratch block, the maps and the packed image exist
        v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE)
        p = sp.make_params(view, proj)
        p.d_out_rgba8, p.d_out_counts = rgba8.data_ptr(), counts.data_ptr()
        ctx.prepare_render([p], s.cuda_stream)
    torch.cuda.synchronize()

    def direct():
        torch.cuda.synchronize()
        poison(v)
        v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE)
        sp.draw(p, rgba8=rgba8, counts=counts)
        torch.cuda.synchronize()
        return rgba8.cpu().numpy(), counts.cpu().numpy()

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE)
        sp.draw(p, rgba8=rgba8, counts=counts)
    torch.cuda.synchronize()
    results = []
    for seed in (0xC0FFEE06, 0xC0FFEE07):  # the second replay after the volume buffer was overwritten in place (a time-varying volume)
        if seed != 0xC0FFEE06:
            v.volume.copy_(torch.from_numpy(O.synth_volume((96, 80, 72), 1, seed)))
            V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())  # also re-packs
        poison(v)
        rgba8.zero_(), counts.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = (rgba8.cpu().numpy(), counts.cpu().numpy())
        ref = direct()
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), "replay with seed %#x" % seed
        assert ref[1][..., 0].sum() > 0
        results.append(ref)
    assert not np.array_equal(results[0][1], results[1][1])
    del g
    ctx.release_stream(s.cuda_stream)


# ---- 6. two streams ----------------------------------------------------------------------------------------------------------------
def test_two_volumes_on_two_streams(ctx):
    vols = [make_volume(ctx, O.synth_volume((96, 80, 72), 1, 0xC0FFEE08 + i), dict(T.APP_TF, intensity_min=0.1 + 0.05 * i), "precomputed", 4)
            for i in range(2)]
    serial = []
    for v in vols:
        v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE)
        serial.append(snapshot(v))
    for v in vols:
        poison(v)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for rep in range(3):
        for v, s in zip(vols, streams):
            with torch.cuda.stream(s):
                v.update_transfer_function(abi.SKIP_ANISOTROPIC_DISTANCE)
    torch.cuda.synchronize()
    for v, ref in zip(vols, serial):
        got = snapshot(v)
        for a, b in zip(got[0], ref[0]):
            assert np.array_equal(a, b)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    for s in streams:
        ctx.release_stream(s.cuda_stream)


# ---- 7. C++ mirror -------------------------------------------------------------------------------------------------------------------
def test_offscreen_tf_drag_host_and_device_frames_equal(tmp_path):
    assert os.path.exists(EXE), "vkv_offscreen not built (run __graft_entry__.build())"
    frames = {}
    for path in ("host", "device"):
        out = tmp_path / ("%s.raw" % path)
        r = subprocess.run([EXE, "--width=192", "--height=128", "--skipmode=3", "--synthetic=72x64x56:1:7", "--tf-drag=4", "--tf-path=%s" % path,
                            "--dump-rgba8=%s" % out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "tf-drag %s: 4 moves" % path in r.stdout, r.stdout
        frames[path] = out.read_bytes()
    assert len(frames["host"]) == 192 * 128 * 4 and frames["host"] == frames["device"]
    assert any(frames["host"])


# ---- 8. argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(ctx):
    E = abi.VKV_E_INVALID_ARGUMENT
    d_vol = torch.from_numpy(O.synth_volume((16, 16, 16), 1, 3)).cuda()
    ext, mext = abi.Extent3D(16, 16, 16), abi.Extent3D(4, 4, 4)
    tex = torch.full((256, 256, 4), 7, dtype=torch.uint8, device="cuda")
    tab = torch.full((abi.TF_BITS_WORDS + 1,), 7, dtype=torch.int32, device="cuda")
    maps = [torch.full((4, 4, 4), 7, dtype=torch.uint8, device="cuda") for _ in range(8)]
    swap = torch.full((4, 4, 4), 7, dtype=torch.uint8, device="cuda")
    cnt = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    opt = abi.VolumeOptions(**T.APP_TF)
    mp = [m.data_ptr() for m in maps]
    ok = dict(options=opt, d_volume=d_vol.data_ptr(), d_gradient=None, extent=ext, d_tf=tex.data_ptr(), d_tables=tab.data_ptr(), d_maps=mp,
              d_swap=swap.data_ptr(), map_extent=mext, skipping_type=abi.SKIP_ANISOTROPIC_DISTANCE, d_count=cnt.data_ptr(), stream=st())
    cases = [dict(options=None), dict(d_volume=None), dict(d_tf=None), dict(d_tables=None), dict(d_maps=None), dict(d_maps=mp[:7] + [None]),
             dict(d_swap=None), dict(d_swap=mp[3]), dict(skipping_type=4), dict(skipping_type=-1), dict(d_tables=tab.data_ptr() + 2),
             dict(d_tf=tex.data_ptr() + 1), dict(extent=abi.Extent3D(0, 16, 16)), dict(map_extent=abi.Extent3D(17, 4, 4))]
    torch.cuda.synchronize()
    for c in cases:
        a = dict(ok, **c)
        assert ctx.update_transfer_function_rc(**a) == E, c
    assert ctx._lib.vkv_transfer_function_texture_device(ctx.handle, None, tex.data_ptr(), tab.data_ptr(), st()) == E
    assert ctx._lib.vkv_transfer_function_texture_device(ctx.handle, C.byref(opt), None, tab.data_ptr(), st()) == E
    assert ctx._lib.vkv_transfer_function_texture_device(ctx.handle, C.byref(opt), tex.data_ptr(), tab.data_ptr() + 2, st()) == E
    # launch limits are checked up front as well: map rows too long for the distance transform, too many map layers for the occupancy pass
    limited, errors = [], []
    for shape, skip in (((2049, 1, 1), abi.SKIP_DISTANCE), ((2049, 1, 1), abi.SKIP_ANISOTROPIC_DISTANCE), ((1, 1, 65536), abi.SKIP_NONE)):
        e = abi.Extent3D(*shape)
        vol = torch.zeros(shape[::-1], dtype=torch.uint8, device="cuda")
        bufs = [torch.full(shape[::-1], 7, dtype=torch.uint8, device="cuda") for _ in range(9)]  # 8 maps + swap
        limited += bufs
        rc = ctx.update_transfer_function_rc(**dict(ok, d_volume=vol.data_ptr(), extent=e, d_maps=[b.data_ptr() for b in bufs[:8]],
                                                    d_swap=bufs[8].data_ptr(), map_extent=e, skipping_type=skip))
        assert rc == abi.VKV_E_UNSUPPORTED, (shape, skip, rc)
        errors.append(ctx.last_error())
    torch.cuda.synchronize()
    assert (tex == 7).all() and (tab == 7).all() and (swap == 7).all() and (cnt == 7).all() and all((m == 7).all() for m in maps)
    assert all((b == 7).all() for b in limited)
    assert all(m.startswith("update_transfer_function:") for m in errors), errors
    # the same arguments without the fault go through
    ctx.update_transfer_function(**ok)
    torch.cuda.synchronize()
    assert not (tab == 7).all() and int(cnt.item()) != 7

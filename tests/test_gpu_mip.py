"""GPU: maximum-intensity projection.  vkv_max_map byte for byte against max_map_np (odd widths, row offsets, blocks 1-8, map extents past the
volume) and kept current across vkv_update_volume_region; the dense MIP against mip_np bit for bit on every pixel (intensity, colour, RGBA8,
depth, sample count); the max-map MIP against the dense MIP bit for bit over
thresholds, sampling factors, cameras (outside, inside with the clipping plane, axis-parallel), depth attachment, packed / linear sampling and
schedules (whole image, rect, compact strided through vkv_scatter_tiles); fewer samples behind a bright object; rejected calls; hipGraph replay;
two streams; the offscreen driver."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_mip_cpu import max_map_np, max_map_skip_np, mip_np, rays_np, samples_np
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vkvolume_amd", "csrc", "vkv_offscreen")
SIZE = (48, 40)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def st():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def make_volume(ctx, vol_dhw, block=4, packed=True):
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(use_precomputed_gradient=0, intensity_min=0.1, intensity_max=1.0, gradient_min=0.0, gradient_max=0.2,
                                  sampling_factor=1.0, voxel_alpha_factor=1.0)
    v.load_from_array(vol_dhw, distance_map_block_size=block)
    V.default_scene(v)
    v.use_packed = packed
    v.build_max_map()
    return v


def subpass(v, azimuth=30.0, elevation=20.0, radius=150.0, size=SIZE, sampling_factor=1.0, clip=50.0, depth_attachment=False, tiles=None):
    sp = V.VolumeRenderSubpass(v.ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, clip_distance=clip, early_ray_termination=0,
                                                           depth_attachment=1 if depth_attachment else 0), size)
    view, proj = T.orbit(azimuth, elevation, radius, image_size=size)
    p = sp.make_params(view, proj, tiles=tiles)
    p.transfer_function.sampling_factor = sampling_factor
    return sp, p


def outputs(size, n_pixels=None, fill=None):
    w, h = size
    n = w * h if n_pixels is None else n_pixels
    o = dict(color=torch.empty((n, 4), dtype=torch.float32, device="cuda"), rgba8=torch.empty((n, 4), dtype=torch.uint8, device="cuda"),
             intensity=torch.empty(n, dtype=torch.float32, device="cuda"), depth=torch.empty(n, dtype=torch.float32, device="cuda"),
             counts=torch.empty((n, 3), dtype=torch.int32, device="cuda"))
    for t in o.values():
        t.fill_(7 if fill is None else fill)
    return o


def draw(sp, p, thr, wmax, skip, size=SIZE, in_depth=None, n_pixels=None):
    o = outputs(size, n_pixels)
    sp.draw_mip(abi.RenderParams.from_buffer_copy(p), thr, wmax, color=o["color"], rgba8=o["rgba8"], intensity=o["intensity"], depth=o["depth"],
                counts=o["counts"], skip=skip, in_depth=in_depth)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in o.items()}


def assert_same_bits(a, b, what=""):
    for k in ("color", "rgba8", "intensity", "depth"):
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), (what, k)
    ca, cb = a["counts"].astype(np.int64), b["counts"].astype(np.int64)
    assert np.array_equal(ca[:, 0] + ca[:, 2], cb[:, 0]), (what, "counts")  # a = skipping, b = dense
    assert np.all(cb[:, 1] == 0) and np.all(cb[:, 2] == 0), (what, "dense counts")


def assert_matches_numpy(got, ref, what=""):
    """the dense MIP against mip_np, bit for bit on every pixel: intensity, colour, RGBA8, depth and the sample count"""
    n = got["intensity"].size
    for k in ("intensity", "color", "depth"):
        assert np.array_equal(got[k].reshape(n, -1).view(np.uint32), np.ascontiguousarray(ref[k], np.float32).reshape(n, -1).view(np.uint32)), (what, k)
    assert np.array_equal(got["rgba8"], ref["rgba8"].reshape(n, 4)), (what, "rgba8")
    assert np.array_equal(got["counts"][:, 0].astype(np.int64), ref["n_steps"].reshape(-1)), (what, "counts")
    assert np.all(got["counts"][:, 1:] == 0), (what, "counts")


def scene_volume(shape=(37, 29, 23), seed=5):
    return O.synth_volume(shape, 1, seed)


# ---- max map ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(13, 7, 5), (37, 29, 23), (64, 48, 40), (10, 3, 3)])
def test_max_map_equals_numpy(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    vol = rng.integers(0, 256, shape[::-1], dtype=np.uint8)
    vol[vol < 200] //= 4  # structure: a few bright voxels in dim ones
    w, h, d = shape
    n = vol.size
    base = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    extents = [tuple(-(-x // b) for x in shape) for b in range(1, 9)] + [(min(w, 7), min(h, 3), min(d, 2)), (w, 1, 1)]
    for off in (0, 1, 3):  # row offsets: the volume at every byte alignment
        base[off:off + n].copy_(torch.from_numpy(vol.reshape(-1)))
        for me in extents:
            out = torch.full((me[2], me[1], me[0]), 0xAB, dtype=torch.uint8, device="cuda")
            ctx.max_map(base.data_ptr() + off, abi.Extent3D(*shape), abi.Extent3D(*me), None, ptr(out), st())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), max_map_np(vol, me)), (shape, me, off)


def test_max_map_past_the_volume_is_zero(ctx):
    vol = np.full((3, 3, 10), 9, np.uint8)
    d_vol = torch.from_numpy(vol).cuda()
    out = torch.full((1, 1, 7), 0xAB, dtype=torch.uint8, device="cuda")
    ctx.max_map(ptr(d_vol), abi.Extent3D(10, 3, 3), abi.Extent3D(7, 1, 1), None, ptr(out), st())
    torch.cuda.synchronize()
    assert list(out.cpu().numpy()[0, 0]) == [9, 9, 9, 9, 9, 0, 0]


def test_max_map_kept_current_across_volume_region_updates(ctx):
    rng = np.random.default_rng(11)
    for block in (1, 3, 4, 8):
        vol = scene_volume((45, 33, 27), 9)
        v = make_volume(ctx, vol, block=block)
        for origin, size in (((0, 0, 0), (5, 4, 3)), ((17, 9, 20), (11, 13, 7)), ((44, 32, 26), (1, 1, 1)), ((3, 30, 0), (40, 3, 27))):
            box = rng.integers(0, 256, size[::-1], dtype=np.uint8)
            v.update_region(origin, box, abi.SKIP_NONE)
            x, y, z = origin
            vol[z:z + size[2], y:y + size[1], x:x + size[0]] = box
            torch.cuda.synchronize()
            me = v.map_extent
            got = v.max_map.cpu().numpy()
            assert np.array_equal(v.volume.cpu().numpy(), vol)
            full = torch.empty_like(v.max_map)
            ctx.max_map(ptr(v.volume), v.extent, me, None, ptr(full), st())
            torch.cuda.synchronize()
            assert np.array_equal(got, full.cpu().numpy()), (block, origin)
            assert np.array_equal(got, max_map_np(vol, (me.width, me.height, me.depth))), (block, origin)


# ---- render -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("cam", [(30.0, 20.0, 150.0, 50.0), (200.0, -35.0, 120.0, 50.0), (60.0, 10.0, 12.0, 1.0)])
def test_dense_mip_matches_numpy(ctx, packed, cam):
    vol = scene_volume()
    v = make_volume(ctx, vol, packed=packed)
    az, el, radius, clip = cam
    for sf, thr, wmax in ((1.0, 0.2, 0.8), (2.3, 0.0, 1.0), (0.5, 0.5, 0.5)):
        sp, p = subpass(v, az, el, radius, sampling_factor=sf, clip=clip)
        got = draw(sp, p, thr, wmax, skip=False)
        ref = mip_np(p, vol, abi.MipOptions(threshold=thr, window_max=wmax))
        assert ref["found"].sum() > 50
        assert_matches_numpy(got, ref, (cam, sf, thr))


@pytest.mark.parametrize("packed", [True, False])
def test_max_map_mip_equals_dense_bit_for_bit(ctx, packed):
    vol = scene_volume()
    v = make_volume(ctx, vol, packed=packed)
    # outside, behind and below, inside the volume (the clipping plane starts the rays), axis-parallel views (odd image: a centre ray)
    cams = [(30.0, 20.0, 150.0, 50.0, SIZE), (200.0, -35.0, 120.0, 50.0, SIZE), (60.0, 10.0, 12.0, 1.0, SIZE), (0.0, 0.0, 150.0, 50.0, (47, 33)),
            (90.0, 0.0, 150.0, 50.0, (47, 33)), (180.0, 0.0, 20.0, 1.0, (33, 33))]
    skipped = 0
    for az, el, radius, clip, size in cams:
        for sf in (0.5, 1.0, 2.3):
            sp, p = subpass(v, az, el, radius, size=size, sampling_factor=sf, clip=clip)
            for thr in (0.0, 0.3, 0.99, 1.0):
                dense = draw(sp, p, thr, 0.9, skip=False, size=size)
                fast = draw(sp, p, thr, 0.9, skip=True, size=size)
                assert_same_bits(fast, dense, (az, el, radius, sf, thr))
                skipped += int(fast["counts"][:, 2].sum())
                if thr == 1.0:
                    assert np.all(dense["rgba8"] == 0) and np.all(dense["intensity"] == 0)
    assert skipped > 0


def test_depth_attachment(ctx):
    vol = scene_volume()
    v = make_volume(ctx, vol)
    w, h = SIZE
    rng = np.random.default_rng(2)
    for packed in (True, False):
        v.use_packed = packed
        sp0, p0 = subpass(v, 30.0, 20.0, 150.0)
        sp, p = subpass(v, 30.0, 20.0, 150.0, depth_attachment=True)
        # a scene depth between the volume's front and back for half the pixels, far (0) elsewhere
        probe = draw(sp0, p0, 0.0, 1.0, skip=False)
        zs = probe["depth"][probe["rgba8"][:, 3] == 255]
        lo, hi = float(zs.min()), float(zs.max())
        scene = np.where(rng.random(w * h) < 0.5, rng.uniform(lo, hi, w * h), 0.0).astype(np.float32)
        d_scene = torch.from_numpy(scene).cuda()
        for thr in (0.0, 0.3):
            dense = draw(sp, p, thr, 0.7, skip=False, in_depth=d_scene)
            fast = draw(sp, p, thr, 0.7, skip=True, in_depth=d_scene)
            assert_same_bits(fast, dense, ("depth attachment", packed, thr))
            ref = mip_np(p, vol, abi.MipOptions(threshold=thr, window_max=0.7), in_depth=scene)
            assert_matches_numpy(dense, ref, ("depth attachment", packed, thr))
            none = dense["rgba8"][:, 3] == 0
            assert np.array_equal(dense["depth"][none].view(np.uint32), scene[none].view(np.uint32))  # the scene depth where nothing counts


def test_schedules_rect_and_compact_strided(ctx):
    vol = scene_volume((64, 56, 48), 3)
    v = make_volume(ctx, vol)
    size = (200, 136)
    w, h = size
    sp, p = subpass(v, 40.0, 15.0, 180.0, size=size)
    whole = {s: draw(sp, p, 0.2, 0.9, skip=s, size=size) for s in (False, True)}
    rect = lib.screen_tile_rect(p.ray_cast, p.ray_gen, size)
    assert 0 < rect.w * rect.h < ((w + 15) // 16) * ((h + 15) // 16)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = ((xs // 16 >= rect.x0) & (xs // 16 < rect.x0 + rect.w) & (ys // 16 >= rect.y0) & (ys // 16 < rect.y0 + rect.h)).reshape(-1)
    for skip in (False, True):
        pr = abi.RenderParams.from_buffer_copy(p)
        pr.tiles = abi.full_frame_tiles(w, h, rect=rect)
        got = draw(sp, pr, 0.2, 0.9, skip=skip, size=size)
        for k in ("rgba8", "intensity", "depth", "color"):
            assert np.array_equal(got[k][inside], whole[skip][k][inside]), ("rect", skip, k)
            assert np.all(got[k][~inside] == 7), ("rect writes outside", k)
        # three ranks, compact, strided over the rectangle, assembled by vkv_scatter_tiles
        n_ranks, n_tiles = 3, rect.w * rect.h
        tpr = -(-n_tiles // n_ranks)
        gathered = torch.zeros((n_ranks, tpr * 256, 4), dtype=torch.uint8, device="cuda")
        gathered_i = torch.zeros((n_ranks, tpr * 256), dtype=torch.float32, device="cuda")
        for r in range(n_ranks):
            pk = abi.RenderParams.from_buffer_copy(p)
            pk.tiles = abi.full_frame_tiles(w, h, rank=r, world=n_ranks, compact=True, rect=rect)
            sp.draw_mip(pk, 0.2, 0.9, rgba8=gathered[r], intensity=gathered_i[r], skip=skip)
        img = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
        img_i = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
        ctx.scatter_tiles(ptr(gathered), ptr(img), size, (16, 16), n_ranks, tpr, 4, st(), rect)
        ctx.scatter_tiles(ptr(gathered_i), ptr(img_i), size, (16, 16), n_ranks, tpr, 4, st(), rect)
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy().reshape(-1, 4), whole[skip]["rgba8"]), ("compact", skip)
        assert np.array_equal(img_i.cpu().numpy().reshape(-1).view(np.uint32), whole[skip]["intensity"].view(np.uint32)), ("compact", skip)
    assert_same_bits(whole[True], whole[False], "whole")


@pytest.mark.parametrize("tile,rect", [((16, 16), (2, 1, 3, 3)), ((32, 16), (0, 1, 3, 3))])
@pytest.mark.parametrize("stretch,patch", [(4.0, 2), (0.25, 4)])
def test_compact_strided_share_of_an_inner_rectangle_matches_numpy(ctx, tile, rect, stretch, patch):
    """the deal of workgroups and lanes to pixels: every second tile, from the second, of a tile rectangle off the origin that reaches the
    image's partial last column and row, into compact buffers; views whose waves take 4x16 and 16x4 pixel patches"""
    shape, size = (24, 20, 16), (72, 56)
    w, h = size
    vol = scene_volume(shape, 7)
    v = make_volume(ctx, vol)
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, clip_distance=50.0, early_ray_termination=0), size)
    p = sp.make_params(*T.stretched_orbit(30.0, 20.0, 40.0, size, stretch))
    assert T.wave_patch_log2(p) == patch
    p.tiles = abi.full_frame_tiles(w, h, tile[0], tile[1], rank=1, world=2, compact=True, rect=abi.TileRect(*rect))
    assert (p.tiles.tile_first, p.tiles.tile_stride, p.tiles.compact, p.tiles.tile_count) == (1, 2, 1, 4)
    ci, ii = T.compact_pixels(size, p.tiles)
    assert np.any(ii % w >= w - w % tile[0]) and np.any(ii // w >= h - h % tile[1]) and ci.size < 4 * tile[0] * tile[1]
    R = rays_np(p)
    S = samples_np(vol, R)
    thr, wmax = 0.2, 0.8
    ref = mip_np(p, vol, abi.MipOptions(threshold=thr, window_max=wmax), S=S)
    assert R["marched"][ii].sum() > 100 and ref["found"].reshape(-1)[ii].sum() > 100
    n = 4 * tile[0] * tile[1]
    dense = draw(sp, p, thr, wmax, skip=False, size=size, n_pixels=n)
    fast = draw(sp, p, thr, wmax, skip=True, size=size, n_pixels=n)
    at = (tile, rect, stretch)
    ref_at = {k: np.ascontiguousarray(a).reshape(w * h, -1)[ii] for k, a in ref.items() if k in ("intensity", "color", "depth", "rgba8", "n_steps")}
    assert_matches_numpy({k: a[ci] for k, a in dense.items()}, ref_at, at)
    assert_same_bits({k: a[ci] for k, a in fast.items()}, {k: a[ci] for k, a in dense.items()}, at)
    me = v.map_extent
    walk = max_map_skip_np(p, vol, max_map_np(vol, (me.width, me.height, me.depth)), thr, False, R, S)
    for j, key in enumerate(("n_filt", "n_probe", "n_skip")):
        assert np.array_equal(fast["counts"][ci, j].astype(np.int64), walk[key][ii]), (at, key)
    assert walk["n_skip"][ii].sum() > 0
    rest = np.ones(n, bool)
    rest[ci] = False        # the tiles' pixels past the image
    for k in dense:
        assert np.all(dense[k][rest] == 7) and np.all(fast[k][rest] == 7), (at, k)


def test_bright_object_in_front_filters_fewer_samples(ctx):
    D = H = W = 48
    vol = np.zeros((D, H, W), np.uint8)
    vol[:, :, :] = (O.synth_volume((W, H, D), 1, 4) // 3)  # dim structure everywhere
    for sl in (np.s_[:4], np.s_[-4:]):  # a bright shell, four voxels deep: every ray meets it first, whatever the view
        vol[sl] = 255
        vol[:, sl] = 255
        vol[:, :, sl] = 255
    v = make_volume(ctx, vol)
    sp, p = subpass(v, 30.0, 20.0, 150.0)
    dense = draw(sp, p, 0.1, 1.0, skip=False)
    fast = draw(sp, p, 0.1, 1.0, skip=True)
    assert_same_bits(fast, dense, "bright front")
    assert fast["counts"][:, 0].sum() < 0.6 * dense["counts"][:, 0].sum()
    assert fast["counts"][:, 1].sum() > 0


def test_rejected_calls_write_nothing(ctx):
    v = make_volume(ctx, scene_volume())
    sp, p = subpass(v)
    o = outputs(SIZE, fill=0x5A)

    def call(params, mip):
        params.d_out_color, params.d_out_rgba8, params.d_out_counts, params.d_out_depth = ptr(o["color"]), ptr(o["rgba8"]), ptr(o["counts"]), ptr(o["depth"])
        mip.d_out_intensity = ptr(o["intensity"])
        return ctx.render_mip_rc(params, mip, st())

    def good():
        return abi.MipOptions(threshold=0.2, window_max=0.8, d_max_map=ptr(v.max_map), flags=0)

    U, I = abi.VKV_E_UNSUPPORTED, abi.VKV_E_INVALID_ARGUMENT
    cases = []
    q = abi.RenderParams.from_buffer_copy(p); q.blend_over_target = 1; cases.append((q, good(), U, "render_mip: blend_over_target"))
    q = abi.RenderParams.from_buffer_copy(p); q.tiles.fill_outside = 1; cases.append((q, good(), U, "render_mip: tiles.fill_outside"))
    q = abi.RenderParams.from_buffer_copy(p); q.options.test = abi.TEST_RAY_ENTRY; cases.append((q, good(), U, "render_mip: test modes"))
    m = good(); m.threshold = float("nan"); cases.append((abi.RenderParams.from_buffer_copy(p), m, I, "render_mip: threshold must be finite"))
    m = good(); m.window_max = float("nan"); cases.append((abi.RenderParams.from_buffer_copy(p), m, I, "render_mip: threshold must be finite"))
    m = good(); m.flags = 1; cases.append((abi.RenderParams.from_buffer_copy(p), m, I, "render_mip: flags must be 0"))
    q = abi.RenderParams.from_buffer_copy(p); q.map_extent = abi.Extent3D(0, 0, 0); cases.append((q, good(), I, "render_mip: the max map needs a valid map_extent"))
    q = abi.RenderParams.from_buffer_copy(p); q.options.depth_attachment = 1; q.d_in_depth = None
    cases.append((q, good(), I, "render_mip: options.depth_attachment needs d_in_depth"))
    for q, m, code, message in cases:
        assert call(q, m) == code and ctx.last_error().startswith(message), (message, ctx.last_error())
    assert ctx.render_mip_rc(None, good(), st()) == I and ctx.last_error().startswith("render_mip: null params or options")
    assert ctx.render_mip_rc(p, None, st()) == I and ctx.last_error().startswith("render_mip: null params or options")
    # max map: bad extents, empty box, box outside
    mm = torch.full((4,), 0x5A, dtype=torch.uint8, device="cuda")
    e = v.extent
    for args, message in (((ptr(v.volume), e, abi.Extent3D(0, 1, 1), None), "max_map: null pointer or bad extent"),
                          ((ptr(v.volume), e, abi.Extent3D(e.width + 1, 1, 1), None), "max_map: null pointer or bad extent"),
                          ((ptr(v.volume), e, abi.Extent3D(2, 2, 1), abi.Box(0, 0, 0, 0, 1, 1)), "max_map: empty box"),
                          ((ptr(v.volume), e, abi.Extent3D(2, 2, 1), abi.Box(e.width - 1, 0, 0, 2, 1, 1)), "max_map: box ("),
                          ((None, e, abi.Extent3D(2, 2, 1), None), "max_map: null pointer or bad extent")):
        assert ctx.max_map_rc(*args, ptr(mm), st()) == I and ctx.last_error().startswith(message), (message, ctx.last_error())
    torch.cuda.synchronize()
    for k, t in o.items():
        assert np.all(t.cpu().numpy() == 0x5A), k
    assert np.all(mm.cpu().numpy() == 0x5A)


def test_hipgraph_replay_equals_direct_call(ctx):
    v = make_volume(ctx, scene_volume())
    sp, p = subpass(v)
    for skip in (True, False):
        direct = draw(sp, p, 0.2, 0.8, skip=skip)
        o = outputs(SIZE)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            sp.draw_mip(abi.RenderParams.from_buffer_copy(p), 0.2, 0.8, color=o["color"], rgba8=o["rgba8"], intensity=o["intensity"],
                        depth=o["depth"], counts=o["counts"], skip=skip)  # one direct call on the stream first
        s.synchronize()
        for t in o.values():
            t.fill_(7)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            sp.draw_mip(abi.RenderParams.from_buffer_copy(p), 0.2, 0.8, color=o["color"], rgba8=o["rgba8"], intensity=o["intensity"],
                        depth=o["depth"], counts=o["counts"], skip=skip)
        torch.cuda.synchronize()
        for t in o.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        got = {k: t.cpu().numpy() for k, t in o.items()}
        for k in got:
            assert np.array_equal(got[k], direct[k]), (skip, k)
        del g


def test_two_streams_give_the_same_results(ctx):
    v = make_volume(ctx, scene_volume())
    sp, p = subpass(v)
    ref = draw(sp, p, 0.3, 0.9, skip=True)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [outputs(SIZE) for _ in streams]
    for _ in range(3):
        for s, o in zip(streams, outs):
            with torch.cuda.stream(s):
                sp.draw_mip(abi.RenderParams.from_buffer_copy(p), 0.3, 0.9, color=o["color"], rgba8=o["rgba8"], intensity=o["intensity"],
                            depth=o["depth"], counts=o["counts"], skip=True)
    torch.cuda.synchronize()
    for o in outs:
        for k, t in o.items():
            assert np.array_equal(t.cpu().numpy(), ref[k]), k


def test_offscreen_mip_frame_equals_python_path(ctx, tmp_path):
    assert os.path.exists(EXE), "vkv_offscreen not built (run __graft_entry__.build())"
    w, h = 160, 96
    shape, kind, seed = (72, 60, 48), 1, 11
    frames = {}
    for mode in ("skip", "dense"):
        args = [EXE, "--width=%d" % w, "--height=%d" % h, "--synthetic=%dx%dx%d:%d:%d" % (*shape, kind, seed), "--azimuth=40", "--elevation=15",
                "--mip=0.25,0.8", "--benchmark=3", "--dump-rgba8=%s" % (tmp_path / (mode + ".raw")), "--dump-counts=%s" % (tmp_path / (mode + ".counts")),
                "--dump-params=%s" % (tmp_path / "params.raw")] + (["--mip-dense"] if mode == "dense" else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "mip: 3 frames" in r.stdout, r.stdout
        frames[mode] = np.fromfile(tmp_path / (mode + ".raw"), np.uint8).reshape(h * w, 4)
        frames[mode + "_counts"] = np.fromfile(tmp_path / (mode + ".counts"), np.uint32).reshape(h * w, 3)
    assert np.array_equal(frames["skip"], frames["dense"])
    assert np.array_equal(frames["skip_counts"][:, 0] + frames["skip_counts"][:, 2], frames["dense_counts"][:, 0])
    # the Python path with the driver's own uniforms (dumped parameter block) over the same synthetic volume
    pd = abi.RenderParams.from_buffer_copy(open(tmp_path / "params.raw", "rb").read())
    vol = O.synth_volume(shape, kind, seed)
    v = make_volume(ctx, vol)
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=pd.options.skipping_type, clip_distance=pd.options.clip_distance), (w, h))
    p = sp.make_params(None, None, uniforms=(pd.camera, pd.ray_cast, pd.ray_gen))
    p.transfer_function = pd.transfer_function
    got = draw(sp, p, 0.25, 0.8, skip=True, size=(w, h))
    assert (got["rgba8"][:, 3] == 255).sum() > 100
    assert np.array_equal(got["rgba8"], frames["skip"])

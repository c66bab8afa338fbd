"""GPU: shaded isosurface.  The dense isosurface against iso_np bit for bit (colour, RGBA8, depth, normal, counters; packed / linear sampling,
three cameras, refine_steps 0 / 4 / 16, odd volume shapes); the max-map isosurface against the dense one bit for bit over iso values and map
blocks, with fewer samples filtered where there is empty space; a world-space sphere on an anisotropic, rotated grid (normals radial,
hits on the radius, the headlight term against the eye); depth attachment; the max map kept current across vkv_update_volume_region; schedules (rect, compact strided through
vkv_scatter_tiles); rejected calls; hipGraph replay; two streams; the offscreen driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_iso_cpu import iso_np, iso_options
from tests.test_mip_cpu import max_map_np, max_map_skip_np, rays_np, samples_np
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "vkvolume_amd", "csrc", "vkv_offscreen")
SIZE = (48, 40)
KEYS = ("color", "rgba8", "depth", "normal")


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


def make_volume(ctx, vol_dhw, block=4, packed=True, voxel_size=(1.0, 1.0, 1.0), axis_angle=(1.0, 0.0, 0.0, 0.0)):
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(use_precomputed_gradient=0, intensity_min=0.1, intensity_max=1.0, gradient_min=0.0, gradient_max=0.2,
                                  sampling_factor=1.0, voxel_alpha_factor=1.0)
    v.load_from_array(vol_dhw, distance_map_block_size=block)
    V.default_scene(v, voxel_size=voxel_size, axis_angle=axis_angle)
    v.use_packed = packed
    v.build_max_map()
    return v


def subpass(v, azimuth=30.0, elevation=20.0, radius=150.0, size=SIZE, sampling_factor=1.0, clip=50.0, depth_attachment=False):
    sp = V.VolumeRenderSubpass(v.ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, clip_distance=clip, early_ray_termination=0,
                                                           depth_attachment=1 if depth_attachment else 0), size)
    view, proj = T.orbit(azimuth, elevation, radius, image_size=size)
    p = sp.make_params(view, proj)
    p.transfer_function.sampling_factor = sampling_factor
    return sp, p


def outputs(n, fill=7):
    o = dict(color=torch.empty((n, 4), dtype=torch.float32, device="cuda"), rgba8=torch.empty((n, 4), dtype=torch.uint8, device="cuda"),
             depth=torch.empty(n, dtype=torch.float32, device="cuda"), normal=torch.empty((n, 4), dtype=torch.float32, device="cuda"),
             counts=torch.empty((n, 3), dtype=torch.int32, device="cuda"))
    for t in o.values():
        t.fill_(fill)
    return o


def draw(sp, p, iso, skip, size=SIZE, in_depth=None, **kw):
    o = outputs(size[0] * size[1])
    sp.draw_iso(abi.RenderParams.from_buffer_copy(p), iso, color=o["color"], rgba8=o["rgba8"], depth=o["depth"], normal=o["normal"],
                counts=o["counts"], skip=skip, in_depth=in_depth, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in o.items()}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)
    ca, cb = a["counts"].astype(np.int64), b["counts"].astype(np.int64)
    assert np.array_equal(ca[:, 0] + ca[:, 2], cb[:, 0]), (what, "counts")  # a = skipping, b = dense
    assert np.all(cb[:, 1] == 0) and np.all(cb[:, 2] == 0), (what, "dense counts")


def assert_matches_numpy(got, ref, what=""):
    """the dense isosurface against iso_np, bit for bit on every pixel: colour, RGBA8, depth, normal and the sample count"""
    n = got["counts"].shape[0]
    for key in KEYS:
        assert np.array_equal(bits(got[key].reshape(n, -1)), bits(np.ascontiguousarray(ref[key]).reshape(n, -1))), (what, key)
    k = ref["k"].reshape(-1)
    assert np.array_equal(got["counts"][:, 0].astype(np.int64), np.where(k >= 0, k + 1, ref["n_steps"].reshape(-1))), (what, "counts")
    assert np.all(got["counts"][:, 1:] == 0), (what, "counts")


def scene_volume(shape=(37, 29, 23), seed=5):
    return O.synth_volume(shape, 1, seed)


def kw_of(o):
    return dict(refine_steps=o.refine_steps, base_color=tuple(o.base_color), ambient=o.ambient, diffuse=o.diffuse, specular=o.specular,
                shininess=o.shininess)


# ---- dense against the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("cam", [(30.0, 20.0, 150.0, 50.0), (200.0, -35.0, 120.0, 50.0), (60.0, 10.0, 12.0, 1.0)])
def test_dense_iso_matches_numpy_bit_for_bit(ctx, packed, cam):
    az, el, radius, clip = cam
    for shape, seed in (((37, 29, 23), 5), ((31, 18, 27), 8)):
        vol = scene_volume(shape, seed)
        v = make_volume(ctx, vol, packed=packed)
        for sf, opts in ((1.0, iso_options(0.3, 4)), (2.3, iso_options(0.2, 16, (0.9, 0.6, 0.3), 0.05, 0.7, 0.5, 7)),
                         (0.5, iso_options(0.5, 0, (1.0, 1.0, 1.0), 0.2, 0.6, 0.0, 1))):
            sp, p = subpass(v, az, el, radius, sampling_factor=sf, clip=clip)
            got = draw(sp, p, opts.iso, skip=False, **kw_of(opts))
            ref = iso_np(p, vol, opts)
            found = ref["found"].reshape(-1)
            assert found.sum() > 50, (cam, shape, sf)
            assert_matches_numpy(got, ref, (cam, shape, sf))
            assert np.all(got["normal"][~found] == 0)


# ---- skipping against dense --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("packed", [True, False])
def test_max_map_iso_equals_dense_bit_for_bit(ctx, packed):
    vol = scene_volume()
    skipped = 0
    for block in (2, 4, 7):
        v = make_volume(ctx, vol, block=block, packed=packed)
        cams = [(30.0, 20.0, 150.0, 50.0, SIZE), (200.0, -35.0, 120.0, 50.0, SIZE), (60.0, 10.0, 12.0, 1.0, SIZE), (90.0, 0.0, 150.0, 50.0, (47, 33))]
        for az, el, radius, clip, size in cams:
            for sf in (0.5, 1.0, 2.3):
                sp, p = subpass(v, az, el, radius, size=size, sampling_factor=sf, clip=clip)
                for iso in (0.0, 0.1, 0.3, 0.7, 1.0, 1.01):
                    dense = draw(sp, p, iso, skip=False, size=size)
                    fast = draw(sp, p, iso, skip=True, size=size)
                    assert_same_bits(fast, dense, (block, az, el, radius, sf, iso))
                    skipped += int(fast["counts"][:, 2].sum())
                    if iso > 1.0:
                        assert np.all(dense["rgba8"] == 0) and np.all(dense["normal"] == 0)
    assert skipped > 0


def test_empty_space_filters_fewer_samples(ctx):
    D = H = W = 48
    vol = np.zeros((D, H, W), np.uint8)
    zz, yy, xx = np.mgrid[0:D, 0:H, 0:W]
    r = np.sqrt((xx - 23.5) ** 2 + (yy - 23.5) ** 2 + (zz - 23.5) ** 2)
    vol[:] = np.clip(128 + 24 * (12 - r), 0, 255).astype(np.uint8)  # a ball of radius 12 in empty space
    v = make_volume(ctx, vol)
    sp, p = subpass(v, 30.0, 20.0, 150.0)
    dense = draw(sp, p, 0.5, skip=False)
    fast = draw(sp, p, 0.5, skip=True)
    assert_same_bits(fast, dense, "empty space")
    assert (dense["rgba8"][:, 3] == 255).sum() > 100
    assert fast["counts"][:, 0].sum() < 0.5 * dense["counts"][:, 0].sum()
    assert fast["counts"][:, 1].sum() > 0


# ---- physics: a sphere on an anisotropic, rotated grid -----------------------------------------------------------------------------------

def test_sphere_on_anisotropic_rotated_grid_has_radial_normals(ctx):
    """Independent of iso_np: the normal must be radial and the headlight term must be n . (eye - hit) / |eye - hit|.  The grid's voxels are
    twice as long in z and the volume is turned 30 degrees about (1, 1, 0), so model[3x3] is neither diagonal nor symmetric: the normal through
    model_inv's transpose and the view vector through model's columns each give other results with the matrix read the other way."""
    W, H, D = 48, 40, 24
    voxel, axis_angle = (1.0, 1.0, 2.0), (1.0, 1.0, 0.0, 30.0)
    size = (96, 80)
    v = make_volume(ctx, np.zeros((D, H, W), np.uint8), voxel_size=voxel, axis_angle=axis_angle)
    sp, p = subpass(v, 35.0, 25.0, 160.0, size=size)
    M = np.asarray(p.camera.model, np.float64).reshape(4, 4).T  # row-major: world = M (p_tex - 0.5, 1)
    A3 = M[:3, :3]
    assert np.abs(A3 - np.diag(np.diag(A3))).max() > 0.1 * np.abs(A3).max() and np.abs(A3 - A3.T).max() > 0.1 * np.abs(A3).max()
    centre = M[:3, 3]
    # world position of every voxel centre
    zz, yy, xx = np.mgrid[0:D, 0:H, 0:W]
    q = np.stack([(xx + 0.5) / W - 0.5, (yy + 0.5) / H - 0.5, (zz + 0.5) / D - 0.5], -1)
    world = q @ A3.T + centre
    dist = np.linalg.norm(world - centre, axis=-1)
    vx_world = np.linalg.norm(A3 @ np.diag([1.0 / W, 1.0 / H, 1.0 / D]), axis=0)  # world length of one voxel per axis
    radius = 0.35 * float(np.linalg.norm(A3 @ np.array([0.0, 0.0, 1.0])))  # a sphere well inside the box
    slope = 24.0 / vx_world.min()  # bytes per world unit: a linear field of distance, 24 per (short) voxel
    vol = np.clip(np.rint(128 + slope * (radius - dist)), 0, 255).astype(np.uint8)
    v = make_volume(ctx, vol, voxel_size=voxel, axis_angle=axis_angle)
    sp, p = subpass(v, 35.0, 25.0, 160.0, size=size)
    # diffuse only, white: the red channel is the headlight term d = clamp(n . v, 0, 1)
    got = draw(sp, p, 128.0 / 255.0, skip=True, size=size, refine_steps=12, ambient=0.0, diffuse=1.0, specular=0.0)
    hit = got["rgba8"][:, 3] == 255
    assert hit.sum() > 500
    # the hit point: the ray through the pixel (the integrator's rays) at the device's depth
    from tests.test_mip_cpu import rays_np
    R = rays_np(p)
    e = np.stack(R["e"], -1).astype(np.float64)
    s = np.stack(R["s"], -1).astype(np.float64)
    cam = p.camera
    view = np.asarray(cam.camera_view, np.float64).reshape(4, 4).T
    Mv = np.asarray(cam.camera_proj, np.float64).reshape(4, 4).T @ view @ M
    d = got["depth"].astype(np.float64)
    with np.errstate(all="ignore"):  # (rays that miss the box carry NaNs)
        h0 = np.concatenate([e - 0.5, np.ones((len(e), 1))], -1) @ Mv.T
        h1 = np.concatenate([s, np.zeros((len(e), 1))], -1) @ Mv.T
        tau = (d * h0[:, 3] - h0[:, 2]) / (h1[:, 2] - d * h1[:, 3])  # z(tau) / w(tau) = depth
        pw = np.concatenate([e + tau[:, None] * s - 0.5, np.ones((len(e), 1))], -1) @ M.T
    rad = pw[:, :3] - centre
    r_hit = np.linalg.norm(rad, axis=1)
    assert np.all(np.abs(r_hit[hit] - radius) <= vx_world.max()), float(np.abs(r_hit[hit] - radius).max())
    n = got["normal"][:, :3].astype(np.float64)
    assert np.allclose(np.linalg.norm(n[hit], axis=1), 1.0, atol=1e-5)
    cosang = np.sum(n[hit] * rad[hit], axis=1) / r_hit[hit]
    worst = np.degrees(np.arccos(np.clip(cosang, -1, 1))).max()
    assert worst < 6.0, worst
    # the view vector: from the hit towards the eye (the camera's position in world space), against the device's shading
    eye = np.linalg.inv(view)[:3, 3]
    to_eye = eye - pw[:, :3]
    to_eye /= np.linalg.norm(to_eye, axis=1, keepdims=True)
    want_d = np.clip(np.sum(n * to_eye, axis=1), 0, 1)
    assert np.abs(got["color"][hit, 0] - want_d[hit]).max() < 1e-3, float(np.abs(got["color"][hit, 0] - want_d[hit]).max())


# ---- depth attachment, map updates, schedules --------------------------------------------------------------------------------------------

def test_depth_attachment(ctx):
    vol = scene_volume()
    v = make_volume(ctx, vol)
    w, h = SIZE
    rng = np.random.default_rng(2)
    for packed in (True, False):
        v.use_packed = packed
        sp0, p0 = subpass(v, 30.0, 20.0, 150.0)
        sp, p = subpass(v, 30.0, 20.0, 150.0, depth_attachment=True)
        probe = draw(sp0, p0, 0.3, skip=False)
        hit0 = probe["rgba8"][:, 3] == 255
        zs = probe["depth"][hit0]
        lo, hi = float(zs.min()), float(zs.max())
        scene = np.where(rng.random(w * h) < 0.5, rng.uniform(lo, hi, w * h), 0.0).astype(np.float32)
        d_scene = torch.from_numpy(scene).cuda()
        dense = draw(sp, p, 0.3, skip=False, in_depth=d_scene)
        fast = draw(sp, p, 0.3, skip=True, in_depth=d_scene)
        assert_same_bits(fast, dense, ("depth attachment", packed))
        opts = iso_options(0.3)
        ref = iso_np(p, vol, opts, in_depth=scene)
        assert_matches_numpy(dense, ref, ("depth attachment", packed))
        hit = dense["rgba8"][:, 3] == 255
        none = ~hit
        assert np.array_equal(dense["depth"][none].view(np.uint32), scene[none].view(np.uint32))  # the scene depth where nothing hits
        # reverse-Z: a hit is never behind the scene depth, and some hits of the frame without the scene are gone
        assert np.all(dense["depth"][hit] >= scene[hit])
        assert (hit0 & ~hit).sum() > 0


def test_max_map_kept_current_across_volume_region_updates(ctx):
    rng = np.random.default_rng(11)
    vol = scene_volume((45, 33, 27), 9)
    v = make_volume(ctx, vol, block=4)
    sp, p = subpass(v, 40.0, 15.0, 150.0)
    for origin, size in (((0, 0, 0), (5, 4, 3)), ((17, 9, 10), (11, 13, 7)), ((3, 30, 0), (40, 3, 27))):
        box = rng.integers(0, 256, size[::-1], dtype=np.uint8)
        v.update_region(origin, box, abi.SKIP_NONE)  # rebuilds the max map over the box (vkv_max_map(box))
        x, y, z = origin
        vol[z:z + size[2], y:y + size[1], x:x + size[0]] = box
        torch.cuda.synchronize()
        for iso in (0.3, 0.8):
            dense = draw(sp, p, iso, skip=False)
            fast = draw(sp, p, iso, skip=True)
            assert_same_bits(fast, dense, (origin, iso))
            ref = iso_np(p, vol, iso_options(iso))
            assert_matches_numpy(dense, ref, (origin, iso))


def test_schedules_rect_and_compact_strided(ctx):
    vol = scene_volume((64, 56, 48), 3)
    v = make_volume(ctx, vol)
    size = (200, 136)
    w, h = size
    sp, p = subpass(v, 40.0, 15.0, 180.0, size=size)
    whole = {s: draw(sp, p, 0.3, skip=s, size=size) for s in (False, True)}
    rect = lib.screen_tile_rect(p.ray_cast, p.ray_gen, size)
    assert 0 < rect.w * rect.h < ((w + 15) // 16) * ((h + 15) // 16)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = ((xs // 16 >= rect.x0) & (xs // 16 < rect.x0 + rect.w) & (ys // 16 >= rect.y0) & (ys // 16 < rect.y0 + rect.h)).reshape(-1)
    for skip in (False, True):
        pr = abi.RenderParams.from_buffer_copy(p)
        pr.tiles = abi.full_frame_tiles(w, h, rect=rect)
        got = draw(sp, pr, 0.3, skip=skip, size=size)
        for k in KEYS:
            assert np.array_equal(got[k][inside], whole[skip][k][inside]), ("rect", skip, k)
            assert np.all(got[k][~inside] == 7), ("rect writes outside", k)
        # three ranks, compact, strided over the rectangle, assembled by vkv_scatter_tiles
        n_ranks, n_tiles = 3, rect.w * rect.h
        tpr = -(-n_tiles // n_ranks)
        gathered = torch.zeros((n_ranks, tpr * 256, 4), dtype=torch.uint8, device="cuda")
        gathered_n = torch.zeros((n_ranks, tpr * 256, 4), dtype=torch.float32, device="cuda")
        for r in range(n_ranks):
            pk = abi.RenderParams.from_buffer_copy(p)
            pk.tiles = abi.full_frame_tiles(w, h, rank=r, world=n_ranks, compact=True, rect=rect)
            sp.draw_iso(pk, 0.3, rgba8=gathered[r], normal=gathered_n[r], skip=skip)
        img = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
        img_n = torch.full((h, w, 4), 7.0, dtype=torch.float32, device="cuda")
        ctx.scatter_tiles(ptr(gathered), ptr(img), size, (16, 16), n_ranks, tpr, 4, st(), rect)
        ctx.scatter_tiles(ptr(gathered_n), ptr(img_n), size, (16, 16), n_ranks, tpr, 16, st(), rect)
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy().reshape(-1, 4), whole[skip]["rgba8"]), ("compact", skip)
        assert np.array_equal(img_n.cpu().numpy().reshape(-1, 4).view(np.uint32), whole[skip]["normal"].view(np.uint32)), ("compact", skip)
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
    opts = iso_options(0.7, 5)
    ref = iso_np(p, vol, opts, S=S)
    assert R["marched"][ii].sum() > 100 and (ref["k"].reshape(-1)[ii] >= 0).sum() > 100
    n = 4 * tile[0] * tile[1]
    frames = {}
    for skip in (False, True):
        o = outputs(n)
        sp.draw_iso(abi.RenderParams.from_buffer_copy(p), opts.iso, color=o["color"], rgba8=o["rgba8"], depth=o["depth"], normal=o["normal"],
                    counts=o["counts"], skip=skip, **kw_of(opts))
        torch.cuda.synchronize()
        frames[skip] = {k: t.cpu().numpy() for k, t in o.items()}
    dense, fast = frames[False], frames[True]
    at = (tile, rect, stretch)
    ref_at = {k: np.ascontiguousarray(ref[k]).reshape(w * h, -1)[ii] for k in KEYS + ("k", "n_steps")}
    assert_matches_numpy({k: a[ci] for k, a in dense.items()}, ref_at, at)
    assert_same_bits({k: a[ci] for k, a in fast.items()}, {k: a[ci] for k, a in dense.items()}, at)
    me = v.map_extent
    walk = max_map_skip_np(p, vol, max_map_np(vol, (me.width, me.height, me.depth)), opts.iso, True, R, S)
    for j, key in enumerate(("n_filt", "n_probe", "n_skip")):
        assert np.array_equal(fast["counts"][ci, j].astype(np.int64), walk[key][ii]), (at, key)
    rest = np.ones(n, bool)
    rest[ci] = False        # the tiles' pixels past the image
    for k in dense:
        assert np.all(dense[k][rest] == 7) and np.all(fast[k][rest] == 7), (at, k)


# ---- the call's guarantees ---------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(ctx):
    v = make_volume(ctx, scene_volume())
    sp, p = subpass(v)
    o = outputs(SIZE[0] * SIZE[1], fill=0x5A)

    def call(params, iso):
        params.d_out_color, params.d_out_rgba8, params.d_out_counts, params.d_out_depth = ptr(o["color"]), ptr(o["rgba8"]), ptr(o["counts"]), ptr(o["depth"])
        iso.d_out_normal = ptr(o["normal"])
        return ctx.render_isosurface_rc(params, iso, st())

    def good():
        g = iso_options(0.3)
        g.d_max_map = ptr(v.max_map)
        return g

    U, I = abi.VKV_E_UNSUPPORTED, abi.VKV_E_INVALID_ARGUMENT
    cases = []
    P = lambda: abi.RenderParams.from_buffer_copy(p)  # noqa: E731
    q = P(); q.blend_over_target = 1; cases.append((q, good(), U, "blend_over_target"))
    q = P(); q.tiles.fill_outside = 1; cases.append((q, good(), U, "tiles.fill_outside"))
    q = P(); q.options.test = abi.TEST_RAY_ENTRY; cases.append((q, good(), U, "test modes"))
    for field, value, message in (("iso", float("nan"), "iso must be finite"), ("iso", float("inf"), "iso must be finite"),
                                  ("refine_steps", 17, "refine_steps must be"), ("ambient", -0.1, "base_color, ambient"),
                                  ("diffuse", float("nan"), "base_color, ambient"), ("specular", float("inf"), "base_color, ambient"),
                                  ("shininess", 0, "shininess must be"), ("shininess", 1025, "shininess must be"), ("flags", 1, "flags must be 0")):
        m = good(); setattr(m, field, value); cases.append((P(), m, I, message))
    for c in (0, 1, 2):
        for value in (-1.0, float("nan")):
            m = good(); m.base_color[c] = value; cases.append((P(), m, I, "base_color, ambient"))
    q = P(); q.map_extent = abi.Extent3D(0, 0, 0); cases.append((q, good(), I, "the max map needs a valid map_extent"))
    q = P(); q.options.depth_attachment = 1; q.d_in_depth = None; cases.append((q, good(), I, "options.depth_attachment needs d_in_depth"))
    q = P(); q.transfer_function.sampling_factor = 0.0; cases.append((q, good(), I, "sampling_factor must be positive"))
    for q, m, code, message in cases:
        assert call(q, m) == code and ctx.last_error().startswith("render_isosurface: " + message), (message, ctx.last_error())
    assert ctx.render_isosurface_rc(None, good(), st()) == I and ctx.last_error().startswith("render_isosurface: null params or options")
    assert ctx.render_isosurface_rc(p, None, st()) == I and ctx.last_error().startswith("render_isosurface: null params or options")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert np.all(t.cpu().numpy() == 0x5A), k


def test_hipgraph_replay_equals_direct_call(ctx):
    v = make_volume(ctx, scene_volume())
    sp, p = subpass(v)
    for skip in (True, False):
        direct = draw(sp, p, 0.3, skip=skip)
        o = outputs(SIZE[0] * SIZE[1])
        s = torch.cuda.Stream()

        def call():
            sp.draw_iso(abi.RenderParams.from_buffer_copy(p), 0.3, color=o["color"], rgba8=o["rgba8"], depth=o["depth"], normal=o["normal"],
                        counts=o["counts"], skip=skip)
        with torch.cuda.stream(s):
            call()  # one direct call on the stream first
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        torch.cuda.synchronize()
        for t in o.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for k, t in o.items():
            assert np.array_equal(t.cpu().numpy(), direct[k]), (skip, k)
        del g


def test_two_streams_give_the_same_results(ctx):
    v = make_volume(ctx, scene_volume())
    sp, p = subpass(v)
    ref = draw(sp, p, 0.3, skip=True)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [outputs(SIZE[0] * SIZE[1]) for _ in streams]
    for _ in range(3):
        for s, o in zip(streams, outs):
            with torch.cuda.stream(s):
                sp.draw_iso(abi.RenderParams.from_buffer_copy(p), 0.3, color=o["color"], rgba8=o["rgba8"], depth=o["depth"], normal=o["normal"],
                            counts=o["counts"], skip=True)
    torch.cuda.synchronize()
    for o in outs:
        for k, t in o.items():
            assert np.array_equal(t.cpu().numpy(), ref[k]), k


def test_offscreen_iso_frame_equals_python_path(ctx, tmp_path):
    assert os.path.exists(EXE), "vkv_offscreen not built (run __graft_entry__.build())"
    w, h = 160, 96
    shape, kind, seed = (72, 60, 48), 1, 11
    frames = {}
    for mode in ("skip", "dense"):
        args = [EXE, "--width=%d" % w, "--height=%d" % h, "--synthetic=%dx%dx%d:%d:%d" % (*shape, kind, seed), "--azimuth=40", "--elevation=15",
                "--iso=0.3,6", "--benchmark=3", "--dump-rgba8=%s" % (tmp_path / (mode + ".raw")), "--dump-counts=%s" % (tmp_path / (mode + ".counts")),
                "--dump-params=%s" % (tmp_path / "params.raw")] + (["--iso-dense"] if mode == "dense" else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "iso: 3 frames" in r.stdout, r.stdout
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
    got = draw(sp, p, 0.3, skip=True, size=(w, h), refine_steps=6)
    assert (got["rgba8"][:, 3] == 255).sum() > 100
    assert np.array_equal(got["rgba8"], frames["skip"])

"""GPU: oblique slices and thick slabs (vkv_render_slab).  Every output of the device (value, RGBA32F, RGBA8, counters) against slab_np and,
with the max map, slab_skip_np bit for bit: three modes, packed / linear sampling, 1 / 2 / 17 / 256 samples, axial presets and random oblique
planes, odd extents, a one-voxel-thick volume, planes partly and wholly outside the box, image sizes that are no multiple of 16, grey windows;
the sparse scene of tests/test_slab_cpu.py (skipping must skip); schedules (rect, compact strided through vkv_scatter_tiles); the max map kept
current across vkv_update_volume_region; rejected calls; hipGraph replay; the C++ host mirror's draw_slab."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_mip_cpu import max_map_np
from tests.test_slab_cpu import random_plane, slab_np, slab_options, slab_params, slab_samples_np, slab_skip_np, sparse_scene
from vkvolume_amd import abi, camera, lib, volume as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vkvolume_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MODES = (abi.SLAB_MAX, abi.SLAB_MIN, abi.SLAB_MEAN)
KEYS = ("value", "color", "rgba8")


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


def bound(v, size, tiles=None):
    """the parameter block of a slab: a zero-filled camera, uniforms and transfer function; image size, schedule, extents and the volume's
    buffers only"""
    e, me = v.extent, v.map_extent
    p = slab_params((e.width, e.height, e.depth), size, map_extent=(me.width, me.height, me.depth))
    if tiles is not None:
        p.tiles = tiles
    sp = V.VolumeRenderSubpass(v.ctx, v, abi.RenderOptions(), size)
    return sp, sp.bind(p)


def outputs(n, fill=7):
    o = dict(value=torch.empty(n, dtype=torch.float32, device="cuda"), color=torch.empty((n, 4), dtype=torch.float32, device="cuda"),
             rgba8=torch.empty((n, 4), dtype=torch.uint8, device="cuda"), counts=torch.empty((n, 3), dtype=torch.int32, device="cuda"))
    for t in o.values():
        t.fill_(fill)
    return o


def plane_of(o):
    return (tuple(o.origin), tuple(o.du), tuple(o.dv), tuple(o.dn))


def draw_into(sp, p, o, skip, out):
    sp.draw_slab(abi.RenderParams.from_buffer_copy(p), plane_of(o), samples=o.samples, mode=o.mode, window=(o.window_min, o.window_max), skip=skip,
                 color=out.get("color"), rgba8=out.get("rgba8"), value=out.get("value"), counts=out.get("counts"))


def draw(sp, p, o, skip, n=None):
    out = outputs(p.image_width * p.image_height if n is None else n)
    draw_into(sp, p, o, skip, out)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in out.items()}


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_matches(got, ref, what, counts=None):
    """the device's frame against the restatement, bit for bit; counts: the expected (n, 3) counters (default: dense, (counted, 0, 0))"""
    n = got["counts"].shape[0]
    for k in KEYS:
        assert np.array_equal(bits(got[k].reshape(n, -1)), bits(np.ascontiguousarray(ref[k]).reshape(n, -1))), (what, k)
    if counts is None:
        counts = np.stack([ref["count"], np.zeros(n, np.int64), np.zeros(n, np.int64)], -1)
    assert np.array_equal(got["counts"].astype(np.int64), counts), (what, "counts")


def scene_volume(shape=(33, 20, 17), seed=5):
    return O.synth_volume(shape, 1, seed)


# ---- the device against the restatements -------------------------------------------------------------------------------------------------

def _planes(rng, ext, size):
    """(name, plane, sample counts): axial presets (a slice inside, one grazing the far face) and random oblique planes, one wholly outside"""
    w, h, d = ext
    out = [("axial", camera.slab_plane(ext, axis="z", index=d // 2, image_size=size), (1, 2, 17, 256)),
           ("axial far face", camera.slab_plane(ext, axis="z", index=d - 0.5, image_size=size, sample_voxels=0.5), (1, 17)),
           ("coronal", camera.slab_plane(ext, axis="y", index=h // 3, image_size=size, sample_voxels=0.25), (2, 256)),
           ("outside", camera.slab_plane(ext, axis="x", index=-4.0, image_size=size), (1, 2))]
    for i in range(3):
        out.append(("oblique %d" % i, random_plane(rng, ext, size), (1, 2, 17, 256)))
    return out


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("shape,size", [((33, 20, 17), (37, 23)), ((24, 19, 1), (50, 31)), ((16, 16, 16), (16, 16))])
def test_slab_matches_numpy_bit_for_bit(ctx, packed, shape, size):
    vol = scene_volume(shape, 5 + shape[0])
    v = make_volume(ctx, vol, block=4, packed=packed)
    me = (v.map_extent.width, v.map_extent.height, v.map_extent.depth)
    mm = max_map_np(vol, me)
    assert np.array_equal(v.max_map.cpu().numpy(), mm)
    sp, p = bound(v, size)
    rng = np.random.default_rng(shape[0] * 7 + 1)
    windows = [(0.0, 1.0), (0.2, 0.6), (0.5, 0.5), (0.7, 0.3), (-1.0, 0.25)]
    counted = outside = partly = 0
    for name, plane, sample_counts in _planes(rng, shape, size):
        for ns in sample_counts:
            window = windows[(ns + len(name)) % len(windows)]
            o = slab_options(plane, samples=ns, window=window)
            S = slab_samples_np(p, vol, o)
            for mode in MODES:
                o.mode = mode
                ref = slab_np(p, vol, o, S)
                assert_matches(draw(sp, p, o, skip=False), ref, (name, ns, mode, "dense"))
            o.mode = abi.SLAB_MAX
            fast = slab_skip_np(p, vol, mm, o, S)
            assert_matches(draw(sp, p, o, skip=True), fast, (name, ns, "skip"), counts=fast["counts"])
            c = ref["count"]
            counted += int(c.sum())
            outside += int((c == 0).all())
            partly += int((c == 0).any() and (c > 0).any())
    assert counted > 5000 and outside >= 1 and partly >= 1, (counted, outside, partly)


def test_sparse_scene_skips_at_least_half_of_the_samples(ctx):
    vol, p0, o = sparse_scene()
    for packed in (True, False):
        v = make_volume(ctx, vol, block=4, packed=packed)
        sp, p = bound(v, (p0.image_width, p0.image_height))
        dense = draw(sp, p, o, skip=False)
        fast = draw(sp, p, o, skip=True)
        ref = slab_np(p, vol, o)
        assert_matches(dense, ref, ("sparse dense", packed))
        for k in KEYS:
            assert np.array_equal(bits(fast[k]), bits(dense[k])), ("sparse", packed, k)
        fc = fast["counts"].astype(np.int64)
        assert np.array_equal(fc[:, 0] + fc[:, 2], ref["count"])
        counted = int(ref["count"].sum())
        print("sparse scene, packed %s: %d of %d counted samples skipped, %d bytes read" % (packed, fc[:, 2].sum(), counted, fc[:, 1].sum()))
        assert fc[:, 2].sum() >= 0.5 * counted, (int(fc[:, 2].sum()), counted)
        walk = slab_skip_np(p, vol, max_map_np(vol, (12, 12, 12)), o)
        assert np.array_equal(fc, walk["counts"])


# ---- schedules, map updates ---------------------------------------------------------------------------------------------------------------

def test_schedules_rect_and_compact_strided(ctx):
    vol = scene_volume((64, 56, 48), 3)
    v = make_volume(ctx, vol)
    size = (200, 136)
    w, h = size
    rng = np.random.default_rng(21)
    plane = camera.slab_plane((64, 56, 48), (30.0, 28.0, 22.0), rng.standard_normal(3), rng.standard_normal(3), size, pixel_voxels=0.45,
                              thickness_voxels=12.0, sample_voxels=0.75)
    sp, p = bound(v, size)
    for mode, skip in ((abi.SLAB_MAX, True), (abi.SLAB_MAX, False), (abi.SLAB_MEAN, False)):
        o = slab_options(plane, mode=mode, window=(0.1, 0.8))
        whole = draw(sp, p, o, skip=skip)
        assert (whole["rgba8"][:, 3] == 255).sum() > 1000 and (whole["rgba8"][:, 3] == 0).sum() > 100
        if not skip:
            assert_matches(whole, slab_np(p, vol, o), ("whole", mode))
        # a rectangle of tiles touches only its pixels
        rect = abi.TileRect(2, 1, 7, 5)
        ys, xs = np.mgrid[0:h, 0:w]
        inside = ((xs // 16 >= rect.x0) & (xs // 16 < rect.x0 + rect.w) & (ys // 16 >= rect.y0) & (ys // 16 < rect.y0 + rect.h)).reshape(-1)
        _, pr = bound(v, size, abi.full_frame_tiles(w, h, rect=rect))
        got = draw(sp, pr, o, skip=skip)
        for k in KEYS + ("counts",):
            assert np.array_equal(got[k][inside], whole[k][inside]), ("rect", mode, skip, k)
            assert np.all(got[k][~inside] == 7), ("rect writes outside", k)
        # compact strided shares of 2 and 8 virtual ranks, assembled by vkv_scatter_tiles
        n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
        for n_ranks in (2, 8):
            tpr = -(-n_tiles // n_ranks)
            g8 = torch.zeros((n_ranks, tpr * 256, 4), dtype=torch.uint8, device="cuda")
            gv = torch.zeros((n_ranks, tpr * 256), dtype=torch.float32, device="cuda")
            for r in range(n_ranks):
                _, pk = bound(v, size, abi.full_frame_tiles(w, h, rank=r, world=n_ranks, compact=True))
                draw_into(sp, pk, o, skip, dict(rgba8=g8[r], value=gv[r]))
            img8 = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
            imgv = torch.full((h, w), 7.0, dtype=torch.float32, device="cuda")
            ctx.scatter_tiles(ptr(g8), ptr(img8), size, (16, 16), n_ranks, tpr, 4, st())
            ctx.scatter_tiles(ptr(gv), ptr(imgv), size, (16, 16), n_ranks, tpr, 4, st())
            torch.cuda.synchronize()
            assert np.array_equal(img8.cpu().numpy().reshape(-1, 4), whole["rgba8"]), ("compact", n_ranks, mode, skip)
            assert np.array_equal(imgv.cpu().numpy().reshape(-1).view(np.uint32), whole["value"].view(np.uint32)), ("compact", n_ranks, mode, skip)


@pytest.mark.parametrize("tile,rect", [((16, 16), (2, 1, 3, 3)), ((32, 16), (0, 1, 3, 3))])
def test_compact_strided_share_of_an_inner_rectangle_matches_numpy(ctx, tile, rect):
    """the deal of workgroups and lanes to pixels (8x8 patches): every second tile, from the second, of a tile rectangle off the origin that
    reaches the image's partial last column and row, into compact buffers"""
    shape, size = (24, 20, 16), (72, 56)
    w, h = size
    vol = scene_volume(shape, 7)
    v = make_volume(ctx, vol)
    tiles = abi.full_frame_tiles(w, h, tile[0], tile[1], rank=1, world=2, compact=True, rect=abi.TileRect(*rect))
    assert (tiles.tile_first, tiles.tile_stride, tiles.compact, tiles.tile_count) == (1, 2, 1, 4)
    sp, p = bound(v, size, tiles)
    ci, ii = T.compact_pixels(size, tiles)
    assert np.any(ii % w >= w - w % tile[0]) and np.any(ii // w >= h - h % tile[1]) and ci.size < 4 * tile[0] * tile[1]
    rng = np.random.default_rng(33)
    plane = camera.slab_plane(shape, (12.0, 10.0, 8.0), rng.standard_normal(3), rng.standard_normal(3), size, pixel_voxels=0.4, thickness_voxels=9.0,
                              sample_voxels=0.75)
    n = 4 * tile[0] * tile[1]
    rest = np.ones(n, bool)
    rest[ci] = False        # the tiles' pixels past the image
    me = v.map_extent
    mm = max_map_np(vol, (me.width, me.height, me.depth))
    for mode, skip in ((abi.SLAB_MEAN, False), (abi.SLAB_MAX, False), (abi.SLAB_MAX, True)):
        o = slab_options(plane, mode=mode, window=(0.1, 0.8))
        S = slab_samples_np(p, vol, o)
        ref = slab_skip_np(p, vol, mm, o, S) if skip else slab_np(p, vol, o, S)
        assert (ref["count"][ii] > 0).sum() > 100
        got = draw(sp, p, o, skip=skip, n=n)
        ref_at = {k: np.ascontiguousarray(ref[k]).reshape(w * h, -1)[ii] for k in KEYS}
        ref_at["count"] = ref["count"][ii]
        assert_matches({k: a[ci] for k, a in got.items()}, ref_at, (tile, rect, mode, skip), counts=ref["counts"][ii] if skip else None)
        if skip:
            assert ref["counts"][ii, 2].sum() > 0
        for k in got:
            assert np.all(got[k][rest] == 7), (tile, rect, mode, skip, k)


def test_max_map_kept_current_across_volume_region_updates(ctx):
    rng = np.random.default_rng(11)
    vol = scene_volume((45, 33, 27), 9)
    v = make_volume(ctx, vol, block=4)
    size = (44, 36)
    sp, p = bound(v, size)
    me = (v.map_extent.width, v.map_extent.height, v.map_extent.depth)
    for origin, bsize in (((0, 0, 0), (5, 4, 3)), ((17, 9, 10), (11, 13, 7)), ((3, 30, 0), (40, 3, 27))):
        box = rng.integers(0, 256, bsize[::-1], dtype=np.uint8)
        v.update_region(origin, box, abi.SKIP_NONE)  # vkv_update_volume_region(box), then vkv_max_map(box) on the stream
        x, y, z = origin
        vol[z:z + bsize[2], y:y + bsize[1], x:x + bsize[0]] = box
        # a slab through the box: centred on it, along a random normal
        centre = [o + 0.5 * (s - 1) for o, s in zip(origin, bsize)]
        plane = camera.slab_plane((45, 33, 27), centre, rng.standard_normal(3), rng.standard_normal(3), size, pixel_voxels=0.8,
                                  thickness_voxels=20.0, sample_voxels=0.6)
        o = slab_options(plane)
        S = slab_samples_np(p, vol, o)
        ref = slab_np(p, vol, o, S)
        assert ref["count"].sum() > 1000
        assert_matches(draw(sp, p, o, skip=False), ref, (origin, "dense"))
        fast = slab_skip_np(p, vol, max_map_np(vol, me), o, S)
        assert_matches(draw(sp, p, o, skip=True), fast, (origin, "skip"), counts=fast["counts"])


# ---- the call's guarantees ---------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(ctx):
    vol = scene_volume()
    v = make_volume(ctx, vol)
    size = (37, 23)
    sp, p = bound(v, size)
    n = size[0] * size[1]
    o = outputs(n, fill=0x5A)
    depth = torch.full((n,), 0x5A, dtype=torch.float32, device="cuda")
    plane = camera.slab_plane((33, 20, 17), axis="z", index=8, image_size=size, thickness_voxels=6.0)

    def good(mode=abi.SLAB_MAX, with_map=True):
        g = slab_options(plane, mode=mode)
        g.d_max_map = ptr(v.max_map) if with_map else None
        g.d_out_value = ptr(o["value"])
        return g

    def P():
        q = abi.RenderParams.from_buffer_copy(p)
        q.d_out_color, q.d_out_rgba8, q.d_out_counts = ptr(o["color"]), ptr(o["rgba8"]), ptr(o["counts"])
        return q

    U, I = abi.VKV_E_UNSUPPORTED, abi.VKV_E_INVALID_ARGUMENT
    cases = []
    q = P(); q.blend_over_target = 1; cases.append((q, good(), U, "blend_over_target"))
    q = P(); q.tiles.fill_outside = 1; cases.append((q, good(), U, "tiles.fill_outside"))
    q = P(); q.options.test = abi.TEST_RAY_ENTRY; cases.append((q, good(), U, "test modes"))
    q = P(); q.options.depth_attachment = 1; q.d_in_depth = ptr(depth); cases.append((q, good(), U, "options.depth_attachment and d_out_depth"))
    q = P(); q.d_out_depth = ptr(depth); cases.append((q, good(), U, "options.depth_attachment and d_out_depth"))
    for field, value, message in (("flags", 1, "flags must be 0"), ("samples", 0, "samples must be"), ("samples", 4097, "samples must be"),
                                  ("mode", 3, "unknown mode"), ("mode", -1, "unknown mode"), ("window_min", float("nan"), "window_min and window_max"),
                                  ("window_max", float("nan"), "window_min and window_max")):
        m = good(); setattr(m, field, value); cases.append((P(), m, I, message))
    for field in ("origin", "du", "dv", "dn"):
        for c in (0, 1, 2):
            for value in (float("nan"), float("inf"), -float("inf")):
                m = good(); getattr(m, field)[c] = value; cases.append((P(), m, I, "origin, du, dv and dn must be finite"))
    cases.append((P(), good(abi.SLAB_MIN), I, "a max map bounds VKV_SLAB_MAX only"))   # a max map with a mode other than MAX
    cases.append((P(), good(abi.SLAB_MEAN), I, "a max map bounds VKV_SLAB_MAX only"))
    q = P(); q.map_extent = abi.Extent3D(0, 0, 0); cases.append((q, good(), I, "the max map needs a valid map_extent"))
    q = P(); q.map_extent = abi.Extent3D(34, 5, 5); cases.append((q, good(), I, "the max map needs a valid map_extent"))
    q = P(); q.d_out_color = q.d_out_rgba8 = q.d_out_counts = None; m = good(); m.d_out_value = None; cases.append((q, m, I, "no output buffer"))
    q = P(); q.d_volume = None; cases.append((q, good(), I, "null volume"))
    q = P(); q.volume_extent = abi.Extent3D(33, 0, 17); cases.append((q, good(), I, "zero extent"))
    q = P(); q.image_width = 0; cases.append((q, good(), I, "zero extent"))
    # what vkv_render_mip rejects of `tiles`
    q = P(); q.tiles.tile_width = 24; cases.append((q, good(), I, "tile size must be"))
    q = P(); q.tiles.tile_height = 0; cases.append((q, good(), I, "tile size must be"))
    q = P(); q.tiles.tile_stride = 0; cases.append((q, good(), I, "tile size must be"))
    q = P(); q.tiles.tile_count = q.tiles.tile_count + 1; cases.append((q, good(), I, "tile schedule runs past the image"))
    q = P(); q.tiles.rect = abi.TileRect(1, 1, 3, 2); cases.append((q, good(), I, "the schedule's tile rectangle runs past the image"))
    q = P(); q.tiles = abi.full_frame_tiles(*size, rect=abi.TileRect(2, 1, 2, 2)); cases.append((q, good(), I, "the schedule's tile rectangle runs past the image"))
    for i, (q, m, code, message) in enumerate(cases):
        assert ctx.render_slab_rc(q, m, st()) == code and ctx.last_error().startswith("render_slab: " + message), (i, message, ctx.last_error())
    assert ctx.render_slab_rc(None, good(), st()) == I and ctx.last_error().startswith("render_slab: null params or options")
    assert ctx.render_slab_rc(P(), None, st()) == I and ctx.last_error().startswith("render_slab: null params or options")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert np.all(t.cpu().numpy() == 0x5A), k
    assert np.all(depth.cpu().numpy() == 0x5A)
    # the same blocks are accepted once mended (the cases above fail for the reason they name)
    assert ctx.render_slab_rc(P(), good(), st()) == abi.VKV_OK
    assert ctx.render_slab_rc(P(), good(abi.SLAB_MIN, with_map=False), st()) == abi.VKV_OK
    torch.cuda.synchronize()
    # the Python wrapper: a skipping MAX slab without the volume's max map
    v2 = V.Volume(ctx)
    v2.options = v.options
    v2.load_from_array(vol)
    V.default_scene(v2)
    sp2, p2 = bound(v2, size)
    with pytest.raises(RuntimeError, match="max map"):
        sp2.draw_slab(p2, plane, samples=plane["samples"], value=o["value"])
    sp2.draw_slab(p2, plane, samples=plane["samples"], mode=abi.SLAB_MIN, value=o["value"])  # MIN needs none
    torch.cuda.synchronize()


def test_hipgraph_replay_equals_direct_call(ctx):
    vol = scene_volume()
    v = make_volume(ctx, vol)
    size = (37, 23)
    sp, p = bound(v, size)
    plane = random_plane(np.random.default_rng(3), (33, 20, 17), size, samples=24)
    for mode, skip in ((abi.SLAB_MAX, True), (abi.SLAB_MEAN, False)):
        o = slab_options(plane, mode=mode)
        direct = draw(sp, p, o, skip=skip)
        assert (direct["rgba8"][:, 3] == 255).sum() > 50
        out = outputs(size[0] * size[1])
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            draw_into(sp, p, o, skip, out)  # one direct call on the stream first
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            draw_into(sp, p, o, skip, out)
        torch.cuda.synchronize()
        for t in out.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for k, t in out.items():
            assert np.array_equal(t.cpu().numpy(), direct[k]), (mode, skip, k)
        del g


# ---- the C++ host mirror -----------------------------------------------------------------------------------------------------------------

def test_host_mirror_draw_slab_equals_the_c_abi(ctx, tmp_path):
    exe = str(tmp_path / "slab_host_driver")
    host = os.path.join(ROOT, "vkvolume_amd", "host")
    subprocess.run([HIPCC, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", host, "-x", "c++",
                    os.path.join(ROOT, "tests", "slab_host_driver.cpp"), "-o", exe, "-L", CSRC, "-lvkvolume_amd", "-Wl,-rpath," + CSRC,
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=600)
    shape, size = (33, 20, 17), (37, 23)
    vol = scene_volume(shape)
    vol.tofile(tmp_path / "vol.raw")
    v = make_volume(ctx, vol)
    sp, p = bound(v, size)
    plane = random_plane(np.random.default_rng(4), shape, size, samples=19)
    for mode, skip in ((abi.SLAB_MAX, True), (abi.SLAB_MIN, False)):
        o = slab_options(plane, mode=mode, window=(0.1, 0.7))
        (tmp_path / "slab.bin").write_bytes(bytes(o))
        r = subprocess.run([exe, *[str(x) for x in shape], str(tmp_path / "vol.raw"), str(tmp_path / "slab.bin"), str(size[0]), str(size[1]),
                            "1" if skip else "0", "4", str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert "slab: 37x23 pixels, 19 samples, mode %d" % mode in r.stdout, r.stdout
        got = draw(sp, p, o, skip=skip)
        assert (got["rgba8"][:, 3] == 255).sum() > 50
        assert np.array_equal(np.fromfile(tmp_path / "out.rgba8", np.uint8).reshape(-1, 4), got["rgba8"])
        assert np.array_equal(np.fromfile(tmp_path / "out.value", np.uint32), got["value"].view(np.uint32))
        assert np.array_equal(np.fromfile(tmp_path / "out.counts", np.uint32).reshape(-1, 3), got["counts"].astype(np.uint32))
    # a skipping MAX slab without Volume::build_max_map is refused by the mirror
    o = slab_options(plane, mode=abi.SLAB_MAX)
    (tmp_path / "slab.bin").write_bytes(bytes(o))
    r = subprocess.run([exe, *[str(x) for x in shape], str(tmp_path / "vol.raw"), str(tmp_path / "slab.bin"), str(size[0]), str(size[1]), "0", "4",
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "skip without a max map: refused" in r.stdout, (r.stdout, r.stderr)

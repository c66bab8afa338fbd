"""GPU: label volumes as pictures.  The dense label render against labels_np bit for bit (label, colour, RGBA8, depth, normal, counters;
three cameras, whole volume and box, shaded from the packed and the linear volume and unshaded, sampling factors, refine_steps 0 / 4 / 16,
tables with every, the odd, the even and the unnamed labels hidden, two volume shapes); the visibility map against max_map_np; the
skipping render against the dense one bit for bit, and no longer so with the map of another table; depth attachment; schedules (rect,
compact strided through vkv_scatter_tiles); pick; rejected calls; hipGraph replay; the chain from the device's own labelling."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_labels_render_cpu import (BOX, CAMERAS, INSIDE_CAMERA, SIZE, label_options, labels_np, scene, tables, visibility_map_np)
from tests.test_mip_cpu import max_map_skip_np
from vkvolume_amd import abi, labels as LB, lib, volume as V

pytestmark = pytest.mark.gpu
KEYS = ("label", "color", "rgba8", "depth", "normal")
LIGHTS = [dict(refine_steps=4), dict(refine_steps=16, ambient=0.05, diffuse=0.7, specular=0.5, shininess=7),
          dict(refine_steps=0, ambient=0.2, diffuse=0.6, specular=0.0, shininess=1)]


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
    v.load_from_array(np.array(vol_dhw), distance_map_block_size=block)
    V.default_scene(v)
    v.use_packed = packed
    return v


def subpass(v, cam=CAMERAS[0], size=SIZE, sampling_factor=1.0, depth_attachment=False):
    az, el, radius, clip = cam
    sp = V.VolumeRenderSubpass(v.ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, clip_distance=clip, early_ray_termination=0,
                                                           depth_attachment=1 if depth_attachment else 0), size)
    view, proj = T.orbit(az, el, radius, image_size=size)
    p = sp.make_params(view, proj)
    p.transfer_function.sampling_factor = sampling_factor
    return sp, p


def abox(box):
    """the abi.Box of a test's (x0, y0, z0, w, h, d); None stays None"""
    return None if box is None else abi.Box(*box)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def outputs(n, fill=7):
    o = dict(label=torch.empty(n, dtype=torch.int32, device="cuda"), color=torch.empty((n, 4), dtype=torch.float32, device="cuda"),
             rgba8=torch.empty((n, 4), dtype=torch.uint8, device="cuda"), depth=torch.empty(n, dtype=torch.float32, device="cuda"),
             normal=torch.empty((n, 4), dtype=torch.float32, device="cuda"), counts=torch.empty((n, 3), dtype=torch.int32, device="cuda"))
    for t in o.values():
        t.fill_(fill)
    return o


def draw(sp, p, d_labels, d_colors, box, skip, size=SIZE, in_depth=None, **kw):
    o = outputs(size[0] * size[1])
    sp.draw_labels(abi.RenderParams.from_buffer_copy(p), d_labels, d_colors, box=abox(box), color=o["color"], rgba8=o["rgba8"], label=o["label"],
                   depth=o["depth"], normal=o["normal"], counts=o["counts"], skip=skip, in_depth=in_depth, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in o.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.int32) else a


def assert_matches_numpy(got, ref, what=""):
    """the dense label render against labels_np, bit for bit on every pixel: label, colour, RGBA8, depth, normal and the sample count"""
    n = got["counts"].shape[0]
    for key in KEYS:
        assert np.array_equal(bits(got[key]).reshape(n, -1), bits(ref[key]).reshape(n, -1)), (what, key)
    k = ref["k"].reshape(-1)
    assert np.array_equal(got["counts"][:, 0].astype(np.int64), np.where(k >= 0, k + 1, ref["n_steps"].reshape(-1))), (what, "counts")
    assert np.all(got["counts"][:, 1:] == 0), (what, "counts")


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in KEYS)


def assert_skip_equals_dense(fast, dense, what=""):
    for k in KEYS:
        assert np.array_equal(bits(fast[k]), bits(dense[k])), (what, k)
    cf, cd = fast["counts"].astype(np.int64), dense["counts"].astype(np.int64)
    assert np.array_equal(cf[:, 0] + cf[:, 2], cd[:, 0]), (what, "counts")
    assert np.all(cd[:, 1] == 0) and np.all(cd[:, 2] == 0), (what, "dense counts")


def kw_of(light, shade):
    return dict(shade=bool(shade), **light)


def opts_of(light, shade):
    return label_options(shade=1 if shade else 0, **light)


# ---- dense against the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box", [None, BOX], ids=["whole", "box"])
@pytest.mark.parametrize("cam", CAMERAS + [INSIDE_CAMERA], ids=["front", "back", "inside"])
def test_dense_render_matches_numpy_bit_for_bit(ctx, cam, box):
    vol, lab, k_labels = scene(box=box)
    tabs = tables(k_labels)
    d_lab = dev(lab)
    volumes = {packed: make_volume(ctx, vol, packed=packed) for packed in (True, False)}
    # (sampling factor, light, shade, packed, table): every value of each axis at least once
    cases = [(1.0, LIGHTS[0], 1, True, "all"), (2.3, LIGHTS[1], 1, False, "odd_hidden"), (0.5, LIGHTS[2], 0, True, "even_hidden"),
             (1.0, LIGHTS[1], 0, False, "short"), (2.3, LIGHTS[2], 1, True, "short"), (0.5, LIGHTS[0], 1, False, "all")]
    for sf, light, shade, packed, name in cases:
        sp, p = subpass(volumes[packed], cam, sampling_factor=sf)
        colors = tabs[name]
        got = draw(sp, p, d_lab, dev(colors), box, skip=False, **kw_of(light, shade))
        ref = labels_np(p, lab, box, colors, opts_of(light, shade), vol=vol)
        found = ref["found"].reshape(-1)
        assert found.sum() > 30, (cam, sf, name)
        assert_matches_numpy(got, ref, (cam, box, sf, shade, packed, name))
        assert np.all(got["label"][~found] == 0) and np.all(got["rgba8"][~found] == 0)
        if name == "all" and cam is not INSIDE_CAMERA:
            assert len(np.unique(got["label"][found])) >= 20
        if name == "short":
            assert got["label"].max() <= colors.size


def test_dense_render_of_a_second_shape(ctx):
    shape = (31, 18, 27)
    vol, lab, k_labels = scene(shape, 8)
    assert k_labels > 10
    tabs = tables(k_labels)
    v = make_volume(ctx, vol)
    for cam, name, shade in ((CAMERAS[0], "all", 1), (CAMERAS[1], "odd_hidden", 0)):
        sp, p = subpass(v, cam, sampling_factor=1.0)
        got = draw(sp, p, dev(lab), dev(tabs[name]), None, skip=False, shade=bool(shade))
        ref = labels_np(p, lab, None, tabs[name], label_options(shade=shade), vol=vol)
        assert ref["found"].sum() > 10
        assert_matches_numpy(got, ref, (shape, cam, name))


# ---- the visibility map ------------------------------------------------------------------------------------------------------------------

def device_map(ctx, lab, shape_whd, box, colors, map_extent, fill=0x5A):
    me = abi.Extent3D(*map_extent)
    out = torch.full((me.depth, me.height, me.width), fill, dtype=torch.uint8, device="cuda")
    d_lab, d_col = dev(lab), dev(colors)
    ctx.check(ctx.label_visibility_map_rc(ptr(d_lab), abi.Extent3D(*shape_whd), None if box is None else abi.Box(*box), ptr(d_col) if colors.size else None,
                                          colors.size, me, ptr(out), st()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_visibility_map_matches_max_map_np(ctx):
    shape = (37, 29, 23)
    ext = lambda b: tuple(-(-e // bb) for e, bb in zip(shape, b))  # noqa: E731
    maps = [ext((1, 1, 1)), ext((4, 4, 4)), ext((3, 5, 2)), (30, 6, 12)]  # the last: block 2 in x, cells 19 .. 29 past the volume
    boxes = [None, BOX, (5, 7, 9, 1, 1, 1), (2, 3, 1, 17, 11, 13)]  # whole, the scene's box, one voxel, a box not aligned to any cell
    seen = set()
    for box in boxes:
        vol, lab, k_labels = scene(box=box)
        for name, colors in tables(max(k_labels, 1)).items():
            for me in maps:
                got = device_map(ctx, lab, shape, box, colors, me)
                want = visibility_map_np(lab, box, vol.shape, colors, me)
                assert np.array_equal(got, want), (box, name, me)
                seen |= set(np.unique(got))
        # an all-hidden table and an empty one give all zeros
        hidden = LB.color_table(max(k_labels, 1), hidden=range(1, max(k_labels, 1) + 1))
        assert not device_map(ctx, lab, shape, box, hidden, maps[1]).any()
        assert not device_map(ctx, lab, shape, box, np.zeros(0, np.uint32), maps[1]).any()
    assert seen == {0, 255}
    # the one-voxel box reaches exactly the cells whose grown box holds the voxel
    lab1 = np.ones((1, 1, 1), np.uint32)
    got = device_map(ctx, lab1, shape, (5, 7, 9, 1, 1, 1), LB.color_table(1), ext((4, 4, 4)))
    want = np.zeros_like(got)
    want[2, 1:3, 1] = 255  # x = 5: cell 1 (3 .. 8); y = 7: cells 1 (3 .. 8) and 2 (7 .. 12); z = 9: cell 2 (7 .. 12)
    assert np.array_equal(got, want)
    # a volume of width 3
    rng = np.random.default_rng(4)
    narrow = (3, 9, 7)
    lab = (rng.integers(0, 6, narrow[::-1]) * (rng.random(narrow[::-1]) < 0.2)).astype(np.uint32)
    colors = LB.color_table(5, hidden=(2, 4))
    for me in ((3, 9, 7), (1, 3, 2), (2, 2, 4)):
        assert np.array_equal(device_map(ctx, lab, narrow, None, colors, me), visibility_map_np(lab, None, narrow[::-1], colors, me)), me


# ---- skipping against dense --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("box", [None, BOX], ids=["whole", "box"])
def test_skipping_equals_dense_bit_for_bit(ctx, box):
    vol, lab, k_labels = scene(box=box)
    tabs = tables(k_labels)
    d_lab = dev(lab)
    skipped = 0
    for block in (2, 4, 7):
        v = make_volume(ctx, vol, block=block)
        for name in ("all", "odd_hidden", "even_hidden", "short"):
            d_col = dev(tabs[name])
            v.build_label_visibility_map(d_lab, d_col, box=abox(box))
            for cam, sf, light, shade in ((CAMERAS[0], 1.0, LIGHTS[0], 1), (CAMERAS[1], 2.3, LIGHTS[1], 0), (INSIDE_CAMERA, 0.5, LIGHTS[2], 1)):
                sp, p = subpass(v, cam, sampling_factor=sf)
                dense = draw(sp, p, d_lab, d_col, box, skip=False, **kw_of(light, shade))
                fast = draw(sp, p, d_lab, d_col, box, skip=True, **kw_of(light, shade))
                assert_skip_equals_dense(fast, dense, (block, name, cam, sf))
                skipped += int(fast["counts"][:, 2].sum())
                if block == 4 and cam is CAMERAS[0]:
                    # the counters are the numpy walk's
                    ref = labels_np(p, lab, box, tabs[name], opts_of(light, shade), vol=vol)
                    me = v.map_extent
                    vis = visibility_map_np(lab, box, vol.shape, tabs[name], (me.width, me.height, me.depth))
                    walk = max_map_skip_np(p, vol, vis, 1.0, True, ref["R"], ref["S"])
                    for j, key in enumerate(("n_filt", "n_probe", "n_skip")):
                        assert np.array_equal(fast["counts"][:, j].astype(np.int64), walk[key]), (name, key)
                    assert fast["counts"][:, 2].sum() > 0
    assert skipped > 0


def test_map_and_table_must_be_in_step(ctx):
    """skipping over the map of ANOTHER table is wrong, and the comparison shows it: with the odd labels hidden, the map built for the table
    that hides the even ones marks cells empty that hold the visible bodies"""
    vol, lab, k_labels = scene()
    tabs = tables(k_labels)
    v = make_volume(ctx, vol, block=1)  # one voxel per cell: a cell's byte speaks for 27 voxels, so the two tables' maps differ in many cells
    d_lab, d_odd, d_even = dev(lab), dev(tabs["odd_hidden"]), dev(tabs["even_hidden"])
    sp, p = subpass(v, CAMERAS[0])
    dense = draw(sp, p, d_lab, d_odd, None, skip=False)
    v.build_label_visibility_map(d_lab, d_odd)
    assert same_bits(draw(sp, p, d_lab, d_odd, None, skip=True), dense)
    v.build_label_visibility_map(d_lab, d_even)
    wrong = draw(sp, p, d_lab, d_odd, None, skip=True)
    assert not same_bits(wrong, dense) and (bits(wrong["depth"]) != bits(dense["depth"])).sum() >= 5


# ---- depth attachment and schedules ------------------------------------------------------------------------------------------------------

def test_depth_attachment(ctx):
    vol, lab, k_labels = scene()
    colors = tables(k_labels)["all"]
    d_lab, d_col = dev(lab), dev(colors)
    v = make_volume(ctx, vol)
    v.build_label_visibility_map(d_lab, d_col)
    w, h = SIZE
    rng = np.random.default_rng(2)
    sp0, p0 = subpass(v)
    sp, p = subpass(v, depth_attachment=True)
    probe = draw(sp0, p0, d_lab, d_col, None, skip=False)
    hit0 = probe["label"] != 0
    zs = probe["depth"][hit0]
    scene_depth = np.where(rng.random(w * h) < 0.5, rng.uniform(float(zs.min()), float(zs.max()), w * h), 0.0).astype(np.float32)
    d_scene = torch.from_numpy(scene_depth).cuda()
    dense = draw(sp, p, d_lab, d_col, None, skip=False, in_depth=d_scene)
    fast = draw(sp, p, d_lab, d_col, None, skip=True, in_depth=d_scene)
    assert_skip_equals_dense(fast, dense, "depth attachment")
    ref = labels_np(p, lab, None, colors, label_options(), vol=vol, in_depth=scene_depth)
    assert_matches_numpy(dense, ref, "depth attachment")
    hit = dense["label"] != 0
    assert np.array_equal(dense["depth"][~hit].view(np.uint32), scene_depth[~hit].view(np.uint32))  # the scene depth where nothing hits
    assert np.all(dense["depth"][hit] >= scene_depth[hit])  # reverse-Z: a hit is never behind the scene
    assert (hit0 & ~hit).sum() > 0


def test_schedules_rect_and_compact_strided(ctx):
    vol, lab, k_labels = scene((64, 56, 48), 3)
    colors = tables(k_labels)["odd_hidden"]
    d_lab, d_col = dev(lab), dev(colors)
    v = make_volume(ctx, vol)
    v.build_label_visibility_map(d_lab, d_col)
    size = (200, 136)
    w, h = size
    sp, p = subpass(v, (40.0, 15.0, 180.0, 50.0), size=size)
    whole = {s: draw(sp, p, d_lab, d_col, None, skip=s, size=size) for s in (False, True)}
    assert_skip_equals_dense(whole[True], whole[False], "whole")
    assert (whole[False]["label"] != 0).sum() > 300
    rect = lib.screen_tile_rect(p.ray_cast, p.ray_gen, size)
    assert 0 < rect.w * rect.h < ((w + 15) // 16) * ((h + 15) // 16)
    ys, xs = np.mgrid[0:h, 0:w]
    inside = ((xs // 16 >= rect.x0) & (xs // 16 < rect.x0 + rect.w) & (ys // 16 >= rect.y0) & (ys // 16 < rect.y0 + rect.h)).reshape(-1)
    for skip in (False, True):
        pr = abi.RenderParams.from_buffer_copy(p)
        pr.tiles = abi.full_frame_tiles(w, h, rect=rect)
        got = draw(sp, pr, d_lab, d_col, None, skip=skip, size=size)
        for k in KEYS:
            assert np.array_equal(got[k][inside], whole[skip][k][inside]), ("rect", skip, k)
            assert np.all(got[k][~inside] == 7), ("rect writes outside", k)
        # three ranks, compact, strided over the rectangle, assembled by vkv_scatter_tiles
        n_ranks, n_tiles = 3, rect.w * rect.h
        tpr = -(-n_tiles // n_ranks)
        gathered = torch.zeros((n_ranks, tpr * 256, 4), dtype=torch.uint8, device="cuda")
        gathered_l = torch.zeros((n_ranks, tpr * 256), dtype=torch.int32, device="cuda")
        for r in range(n_ranks):
            pk = abi.RenderParams.from_buffer_copy(p)
            pk.tiles = abi.full_frame_tiles(w, h, rank=r, world=n_ranks, compact=True, rect=rect)
            sp.draw_labels(pk, d_lab, d_col, rgba8=gathered[r], label=gathered_l[r], skip=skip)
        img = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda")
        img_l = torch.full((h, w), 7, dtype=torch.int32, device="cuda")
        ctx.scatter_tiles(ptr(gathered), ptr(img), size, (16, 16), n_ranks, tpr, 4, st(), rect)
        ctx.scatter_tiles(ptr(gathered_l), ptr(img_l), size, (16, 16), n_ranks, tpr, 4, st(), rect)
        torch.cuda.synchronize()
        assert np.array_equal(img.cpu().numpy().reshape(-1, 4), whole[skip]["rgba8"]), ("compact", skip)
        assert np.array_equal(img_l.cpu().numpy().reshape(-1), whole[skip]["label"]), ("compact", skip)


def test_pick_equals_the_label_image(ctx):
    vol, lab, k_labels = scene(box=BOX)
    colors = tables(k_labels)["odd_hidden"]
    d_lab, d_col = dev(lab), dev(colors)
    v = make_volume(ctx, vol)
    sp, p = subpass(v)
    frame = draw(sp, p, d_lab, d_col, BOX, skip=False, shade=False)
    w, h = SIZE
    label = frame["label"].view(np.uint32).reshape(h, w)
    depth = frame["depth"].reshape(h, w)
    hits, misses = np.argwhere(label != 0), np.argwhere(label == 0)
    assert len(hits) >= 10 and len(misses) >= 2
    picks = [hits[i] for i in np.linspace(0, len(hits) - 1, 10).astype(int)] + [misses[0], misses[-1]]
    assert any(x >= 32 for _, x in picks) and any(y >= 32 for y, _ in picks)  # tiles off the origin, the partial last column included
    for y, x in picks:
        got_label, got_depth = sp.pick(p, d_lab, d_col, int(x), int(y), box=abox(BOX))
        assert got_label == int(label[y, x]) and np.float32(got_depth).view(np.uint32) == depth[y, x].view(np.uint32), (x, y)
    with pytest.raises(ValueError):
        sp.pick(p, d_lab, d_col, w, 0, box=abox(BOX))


# ---- the calls' guarantees ---------------------------------------------------------------------------------------------------------------

def test_rejected_calls_write_nothing(ctx):
    vol, lab, k_labels = scene()
    colors = tables(k_labels)["all"]
    d_lab, d_col = dev(lab), dev(colors)
    v = make_volume(ctx, vol)
    vis = v.build_label_visibility_map(d_lab, d_col).clone()
    sp, p = subpass(v)
    o = outputs(SIZE[0] * SIZE[1], fill=0x5A)
    U, I = abi.VKV_E_UNSUPPORTED, abi.VKV_E_INVALID_ARGUMENT

    def good():
        return abi.LabelRenderOptions(d_labels=ptr(d_lab), box=None, d_colors=ptr(d_col), table_entries=colors.size, refine_steps=4, shade=1,
                                      ambient=0.1, diffuse=0.8, specular=0.3, shininess=32, d_visibility_map=ptr(vis), d_out_label=ptr(o["label"]),
                                      d_out_normal=ptr(o["normal"]), flags=0)

    def call(params, options):
        params.d_out_color, params.d_out_rgba8, params.d_out_counts, params.d_out_depth = ptr(o["color"]), ptr(o["rgba8"]), ptr(o["counts"]), ptr(o["depth"])
        return ctx.render_labels_rc(params, options, st())

    P = lambda: abi.RenderParams.from_buffer_copy(p)  # noqa: E731
    assert call(P(), good()) == 0  # the unbroken call is accepted ...
    torch.cuda.synchronize()
    assert (o["label"] != 0x5A).any()
    for t in o.values():
        t.fill_(0x5A)  # ... and every broken one below must leave the fill
    cases = []
    q = P(); q.blend_over_target = 1; cases.append((q, good(), U, "blend_over_target"))
    q = P(); q.tiles.fill_outside = 1; cases.append((q, good(), U, "tiles.fill_outside"))
    q = P(); q.options.test = abi.TEST_RAY_ENTRY; cases.append((q, good(), U, "test modes"))
    for field, value, message in (("d_labels", None, "null d_labels"), ("d_colors", None, "a table of"), ("d_labels", ptr(d_lab) + 2, "d_labels and d_colors must be"),
                                  ("d_colors", ptr(d_col) + 1, "d_labels and d_colors must be"), ("shade", 2, "shade must be"), ("flags", 1, "flags must be 0"),
                                  ("refine_steps", 17, "refine_steps must be"), ("ambient", -0.1, "ambient, diffuse"), ("diffuse", float("nan"), "ambient, diffuse"),
                                  ("specular", float("inf"), "ambient, diffuse"), ("shininess", 0, "shininess must be"), ("shininess", 1025, "shininess must be")):
        m = good(); setattr(m, field, value); cases.append((P(), m, I, message))
    for bad_box, message in ((abi.Box(0, 0, 0, 0, 5, 5), "empty box"), (abi.Box(30, 0, 0, 8, 5, 5), "box (30, 0, 0)"), (abi.Box(0, 0, 23, 1, 1, 1), "box (0, 0, 23)")):
        m = good(); m.box = C.pointer(bad_box); cases.append((P(), m, I, message))
    q = P(); q.d_volume = None; cases.append((q, good(), I, "null volume"))  # shade == 1 reads the volume
    q = P(); q.map_extent = abi.Extent3D(0, 0, 0); cases.append((q, good(), I, "the max map needs a valid map_extent"))
    q = P(); q.options.depth_attachment = 1; q.d_in_depth = None; cases.append((q, good(), I, "options.depth_attachment needs d_in_depth"))
    q = P(); q.transfer_function.sampling_factor = 0.0; cases.append((q, good(), I, "sampling_factor must be positive"))
    q = P(); q.tiles.tile_width = 24; cases.append((q, good(), I, "tile size must be"))
    for q, m, code, message in cases:
        assert call(q, m) == code and ctx.last_error().startswith("render_labels: " + message), (message, ctx.last_error())
    # no output at all
    q, m = P(), good()
    m.d_out_label = m.d_out_normal = None
    assert ctx.render_labels_rc(q, m, st()) == I and ctx.last_error().startswith("render_labels: no output buffer")
    assert ctx.render_labels_rc(None, good(), st()) == I and ctx.last_error().startswith("render_labels: null params or options")
    assert ctx.render_labels_rc(p, None, st()) == I and ctx.last_error().startswith("render_labels: null params or options")
    # a box of 2^32 voxels or more (nothing that large is allocated: the call is rejected before it reads a byte)
    q = P(); q.volume_extent = abi.Extent3D(2048, 2048, 1024); q.map_extent = abi.Extent3D(512, 512, 256)
    assert call(q, good()) == U and ctx.last_error().startswith("render_labels: a box of more than 2^32 - 1 voxels")
    # the visibility map's own rejections
    ext, me = v.extent, v.map_extent
    probe = torch.full((me.depth, me.height, me.width), 0x5A, dtype=torch.uint8, device="cuda")
    vm = lambda **kw: ctx.label_visibility_map_rc(**{**dict(d_labels=ptr(d_lab), extent=ext, box=None, d_colors=ptr(d_col), table_entries=colors.size,  # noqa: E731
                                                           map_extent=me, d_map=ptr(probe), stream=st()), **kw})
    for kw, code, message in ((dict(d_labels=None), I, "null d_labels"), (dict(d_colors=None), I, "a table of"), (dict(d_map=None), I, "null d_map or bad extent"),
                              (dict(d_labels=ptr(d_lab) + 1), I, "d_labels and d_colors must be"), (dict(extent=abi.Extent3D(0, 29, 23)), I, "null d_map or bad extent"),
                              (dict(map_extent=abi.Extent3D(40, 8, 6)), I, "null d_map or bad extent"), (dict(box=abi.Box(0, 0, 0, 0, 1, 1)), I, "empty box"),
                              (dict(box=abi.Box(36, 0, 0, 2, 1, 1)), I, "box (36, 0, 0)"),
                              (dict(extent=abi.Extent3D(2048, 2048, 1024), map_extent=abi.Extent3D(512, 512, 256)), U, "a box of more than 2^32 - 1 voxels")):
        assert vm(**kw) == code and ctx.last_error().startswith("label_visibility_map: " + message), (kw, ctx.last_error())
    torch.cuda.synchronize()
    for k, t in o.items():
        assert np.all(t.cpu().numpy() == 0x5A), k
    assert np.all(probe.cpu().numpy() == 0x5A)
    # shade == 0 reads no voxel: a null volume is accepted and gives the unshaded frame
    q, m = P(), good()
    q.d_volume = q.d_packed_volume = None
    m.shade = 0
    assert call(q, m) == 0, ctx.last_error()
    torch.cuda.synchronize()
    ref = labels_np(p, lab, None, colors, label_options(shade=0))
    assert np.array_equal(o["label"].cpu().numpy().view(np.uint32), ref["label"].reshape(-1))
    assert np.array_equal(o["rgba8"].cpu().numpy(), ref["rgba8"].reshape(-1, 4))


def test_hipgraph_replay_equals_direct_call(ctx):
    vol, lab, k_labels = scene()
    d_lab = dev(lab)
    table = tables(k_labels)["odd_hidden"]
    d_col = dev(table)
    v = make_volume(ctx, vol)
    sp, p = subpass(v)
    for skip in (True, False):
        v.build_label_visibility_map(d_lab, d_col)
        direct = draw(sp, p, d_lab, d_col, None, skip=skip)
        direct_map = v.label_visibility_map.cpu().numpy().copy()
        o = outputs(SIZE[0] * SIZE[1])
        s = torch.cuda.Stream()

        def call():
            v.build_label_visibility_map(d_lab, d_col)
            sp.draw_labels(abi.RenderParams.from_buffer_copy(p), d_lab, d_col, color=o["color"], rgba8=o["rgba8"], label=o["label"], depth=o["depth"],
                           normal=o["normal"], counts=o["counts"], skip=skip)
        with torch.cuda.stream(s):
            call()  # one direct call on the stream first
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call()
        torch.cuda.synchronize()
        for t in o.values():
            t.fill_(7)
        v.label_visibility_map.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for k, t in o.items():
            assert np.array_equal(t.cpu().numpy(), direct[k]), (skip, k)
        assert np.array_equal(v.label_visibility_map.cpu().numpy(), direct_map)
        del g


def test_end_to_end_from_the_device_labelling(ctx):
    vol, lab, k_labels = scene()
    v = make_volume(ctx, vol)
    d_lab, _, counts = v.label_components(0.5, connectivity=6, sizes=False)
    k = int(counts[0].item())
    assert k == k_labels and np.array_equal(d_lab.cpu().numpy().view(np.uint32), lab)
    hidden = list(range(1, k + 1, 3))
    table = LB.color_table(k, seed=9, hidden=hidden)
    d_col = torch.from_numpy(table).cuda()
    v.build_label_visibility_map(d_lab, d_col)
    sp, p = subpass(v)
    got = draw(sp, p, d_lab, d_col, None, skip=True, shade=False)
    shown = set(np.unique(got["label"].view(np.uint32))) - {0}
    assert len(shown) >= 10 and shown <= set(range(1, k + 1)) - set(hidden)
    hit = got["label"] != 0
    word = table[got["label"][hit].astype(np.int64) - 1]
    assert np.array_equal(got["rgba8"][hit].view(np.uint32).reshape(-1), word)  # unshaded: the table's bytes, alpha 255
    # toggling on the device: switch the shown bodies off and the hidden ones on, rebuild the map, draw again
    LB.set_visible(d_col, sorted(shown), False)
    LB.set_visible(d_col, hidden, True)
    v.build_label_visibility_map(d_lab, d_col)
    again = draw(sp, p, d_lab, d_col, None, skip=True, shade=False)
    assert same_bits(again, draw(sp, p, d_lab, d_col, None, skip=False, shade=False))
    assert not (set(np.unique(again["label"].view(np.uint32))) & shown)

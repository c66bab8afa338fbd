"""GPU: the launch-uniform arguments of the ray-march kernels (RayMarchArgs.cells_per_unit, free_margin, the UniformDiv divisors of the deal and
the batch kernel's frame / group split) against the CPU oracle, at the smallest shapes that reach each divisor.

Volume 40 x 36 x 28, frame 112 x 80, two cameras; per-axis block sizes (4, 4, 4), (3, 5, 6) and (8, 2, 16).  (A depth of 28 voxels has no map
extent whose block size is 16 - two cells give 14 - so that scene keeps the two-cell map and sets the uniform's block size to 16 itself: the
oracle and the kernels take the value from the uniform alike.)  Every case compares RGBA8 and the three counters with the oracle's bit for bit.
  * tile sizes 16 x 16, 32 x 16, 32 x 32, 48 x 32 (three blocks per tile row: a divisor that is no power of two); the frame's edge tiles are partial
    for all but the first;
  * fill_outside rectangles within kFillPerTile = 3: touching the top-left corner, interior, touching the bottom-right corner, one tile column
    narrower than the image (one outside tile per row), the whole image minus one tile row; with 32 x 16 and 48 x 32 tiles as well; the complete frame,
    through the general fill and through the 16-byte stores of an RGBA8-only launch.  Such a rectangle has to hold every tile the box is seen in, so
    these frames look from further away (the box covers 3 x 3 tiles) and the picture is moved by whole tiles to where the rectangle is;
  * launches of 1, 2, 3, 5, 6 and 7 frames whose frames have different tile counts (whole image, a rectangle with fill_outside, a plain rectangle),
    interleaved and with VkvTuning.batch_sequential;
  * a rank's share (tile_first = 1, tile_stride = 3, compact), through vkv_render_batch and vkv_render;
  * a registered target rendered twice - the second frame starts its tiles in the measured order (128 x 128 here: the feedback takes part from
    64 tiles on, and 112 x 80 has 35);
  * a launch with a depth output, and vkv_render (the single-frame kernel) with 48 x 32 tiles."""
import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_gpu_parity import DEPTH_TOL, make_gpu_volume
from tests.test_gpu_ray_setup_paths import AxisBlockScene
from vkvolume_amd import abi, lib, volume as V

pytestmark = pytest.mark.gpu

SHAPE = (40, 36, 28)
SIZE = (112, 80)
MAPS = {(4, 4, 4): (10, 9, 7), (3, 5, 6): (14, 8, 5), (8, 2, 16): (5, 18, 2)}        # block sizes -> map extent
AZIMUTHS = (33.0, 205.0)
TILE_SIZES = ((16, 16), (32, 16), (32, 32), (48, 32))
OPTS = dict(skipping_type=abi.SKIP_DISTANCE, clip_distance=1.0)


@pytest.fixture(scope="module")
def scenes(ctx):
    """per block size: the oracle scene, the device volume with its distance map, and a cache of oracle frames"""
    vol = O.synth_volume(SHAPE, 1, 0x11A265)
    out = {}
    for block, map_whd in MAPS.items():
        scene = AxisBlockScene(vol, abi.VolumeOptions(**T.APP_TF), map_whd)
        v, tf = make_gpu_volume(ctx, scene)
        me = scene.map_extent
        v.map_extent = me
        v.distance_map_swap = torch.empty((me.depth, me.height, me.width), dtype=torch.uint8, device="cuda")
        v.distance_maps = []
        V.ComputeDistanceMap(ctx).compute(v, tf, abi.SKIP_DISTANCE)
        assert np.array_equal(v.distance_maps[0].cpu().numpy(), scene.maps(abi.SKIP_DISTANCE)[0])
        out[block] = (scene, v, {})
    return out


FAR = 300.0        # orbit radius at which the box covers 3 x 3 tiles of 16 x 16 (the fill_outside rectangles must hold the whole box)


def frame_params(scene, block, cam, tiles, size=SIZE, radius=150.0, pan=(0, 0)):
    """the frame of camera `cam` at orbit radius `radius`, its picture moved right / down by `pan` pixels (the ray generator's first direction moves)"""
    ro = abi.RenderOptions(**OPTS)
    assert ro.early_ray_termination
    view, proj = T.orbit(AZIMUTHS[cam], radius=radius, image_size=size)
    p = scene.params(view, proj, size, ro, tiles=tiles)
    for k in range(3):
        p.ray_cast.block_size[k] = float(block[k])        # (8, 2, 16): see the module's docstring; the others have this value already
        p.ray_gen.dir00[k] = p.ray_gen.dir00[k] - (pan[0] * p.ray_gen.ddx[k] + pan[1] * p.ray_gen.ddy[k])
    return p


def oracle_frame(scenes, block, cam, tiles=None, key="whole", size=SIZE, radius=150.0, pan=(0, 0)):
    """the oracle's frame of camera `cam`, computed once per (camera, schedule kind, size, view); a whole-image frame does not depend on the tile size"""
    scene, _, cache = scenes[block]
    k = (cam, key, size, radius, pan)
    if k not in cache:
        t = tiles if tiles is not None else abi.full_frame_tiles(size[0], size[1])
        ref = scene.render(frame_params(scene, block, cam, t, size, radius, pan), want_rgba8=True)
        assert int((ref.counts[..., 0] > 0).sum()) > 50 and int(ref.counts[..., 1].sum()) > 0, "the view marches and probes"
        cache[k] = ref
    return cache[k]


def launch(ctx, v, plist, with_counts=True, with_depth=False, single=False):
    """the frames of plist in one vkv_render_batch launch (or one vkv_render each); buffers start from zero like the oracle's"""
    st = torch.cuda.current_stream().cuda_stream
    outs, qs = [], []
    for p in plist:
        size = (p.image_width, p.image_height)
        shape = (p.tiles.tile_count * p.tiles.tile_width * p.tiles.tile_height,) if p.tiles.compact else (size[1], size[0])
        o = dict(rgba8=torch.zeros(shape + (4,), dtype=torch.uint8, device="cuda"),
                 counts=torch.zeros(shape + (3,), dtype=torch.int32, device="cuda") if with_counts else None,
                 depth=torch.zeros(shape, dtype=torch.float32, device="cuda") if with_depth else None)
        q = abi.RenderParams.from_buffer_copy(V.VolumeRenderSubpass(ctx, v, p.options, size).bind(p))
        q.d_out_color, q.d_out_rgba8 = None, o["rgba8"].data_ptr()
        q.d_out_counts = o["counts"].data_ptr() if with_counts else None
        q.d_out_depth = o["depth"].data_ptr() if with_depth else None
        outs.append(o), qs.append(q)
    if single:
        for q in qs:
            ctx.render(q, st)
    else:
        ctx.render_batch(qs, st)
    torch.cuda.synchronize()
    return [{k: (None if t is None else t.cpu().numpy()) for k, t in o.items()} for o in outs]


def assert_frame(got, ref, what):
    assert np.array_equal(got["rgba8"], ref.rgba8), "%s: RGBA8 differs in %d pixels" % (what, int((got["rgba8"] != ref.rgba8).any(-1).sum()))
    if got["counts"] is not None:
        assert np.array_equal(got["counts"].astype(np.uint32), ref.counts), "%s: counters differ in %d pixels" % (
            what, int((got["counts"].astype(np.uint32) != ref.counts).any(-1).sum()))


@pytest.mark.parametrize("tile", TILE_SIZES, ids=lambda t: "%dx%d" % t)
@pytest.mark.parametrize("block", sorted(MAPS), ids=lambda b: "block%d_%d_%d" % b)
def test_tile_sizes_against_the_oracle(ctx, scenes, block, tile):
    scene, v, _ = scenes[block]
    tiles = abi.full_frame_tiles(SIZE[0], SIZE[1], tile[0], tile[1])
    if tile != (16, 16):
        assert SIZE[0] % tile[0] != 0 or SIZE[1] % tile[1] != 0        # partial edge tiles
    plist = [frame_params(scene, block, cam, tiles) for cam in (0, 1)]
    assert tuple(plist[0].ray_cast.block_size)[:3] == tuple(float(b) for b in block)
    for with_counts in (True, False):        # the kernels with and without the per-pixel counters
        for cam, got in enumerate(launch(ctx, v, plist, with_counts=with_counts)):
            assert_frame(got, oracle_frame(scenes, block, cam), "block %s tile %s camera %d counts %d" % (block, tile, cam, with_counts))


# (tile size, rectangle x0, y0, w, h): 7 x 5 tiles of 16 x 16, 4 x 5 of 32 x 16, 3 x 3 of 48 x 32
FILL_RECTS = [((16, 16), (0, 0, 4, 3)), ((16, 16), (2, 1, 3, 3)), ((16, 16), (3, 2, 4, 3)), ((16, 16), (1, 1, 6, 3)), ((16, 16), (0, 1, 6, 3)),
              ((16, 16), (0, 1, 7, 4)), ((16, 16), (0, 0, 7, 4)), ((32, 16), (1, 1, 2, 3)), ((48, 32), (0, 0, 2, 2)), ((48, 32), (1, 1, 2, 2))]


@pytest.mark.parametrize("tile,rect", FILL_RECTS, ids=lambda x: "x".join(str(i) for i in x))
def test_fill_outside_rectangles_complete_the_frame(ctx, scenes, tile, rect):
    block = (3, 5, 6)
    scene, v, _ = scenes[block]
    full_x, full_y = -(-SIZE[0] // tile[0]), -(-SIZE[1] // tile[1])
    inside = rect[2] * rect[3]
    assert rect[0] + rect[2] <= full_x and rect[1] + rect[3] <= full_y and 0 < full_x * full_y - inside <= 3 * inside        # the workgroups fill: kFillPerTile
    tiles = abi.full_frame_tiles(SIZE[0], SIZE[1], tile[0], tile[1], rect=abi.TileRect(*rect), fill_outside=True)
    assert tiles.fill_outside == 1 and tiles.tile_count == inside
    # a fill_outside rectangle holds every tile the box can be seen in: the picture is moved by whole tiles until the box's own rectangle starts at the
    # schedule's first tile
    plist, pans = [], []
    for cam in (0, 1):
        box = lib.screen_tile_rect(*[getattr(frame_params(scene, block, cam, tiles, radius=FAR), f) for f in ("ray_cast", "ray_gen")], SIZE, tile, 1)
        pan = ((rect[0] - box.x0) * tile[0], (rect[1] - box.y0) * tile[1])
        p = frame_params(scene, block, cam, tiles, radius=FAR, pan=pan)
        moved = lib.screen_tile_rect(p.ray_cast, p.ray_gen, SIZE, tile, 1)
        assert moved.w > 0 and moved.x0 >= rect[0] and moved.y0 >= rect[1] and moved.x0 + moved.w <= rect[0] + rect[2] and moved.y0 + moved.h <= rect[1] + rect[3], (
            moved.as_tuple(), rect)
        plist.append(p), pans.append(pan)
    for with_counts in (True, False):        # False: RGBA8 alone, the outside tiles cleared with 16-byte stores
        for cam, got in enumerate(launch(ctx, v, plist, with_counts=with_counts)):
            ref = oracle_frame(scenes, block, cam, radius=FAR, pan=pans[cam])
            assert_frame(got, ref, "tile %s rect %s camera %d counts %d" % (tile, rect, cam, with_counts))


@pytest.mark.parametrize("sequential", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 7])
def test_batch_launches_of_frames_with_different_tile_counts(ctx, scenes, n, sequential):
    block = (4, 4, 4)
    scene, v, _ = scenes[block]
    rect = abi.TileRect(2, 1, 4, 3)
    kinds = {"whole": abi.full_frame_tiles(SIZE[0], SIZE[1]),                                              # 35 tiles
             "fill": abi.full_frame_tiles(SIZE[0], SIZE[1], rect=rect, fill_outside=True),                 # 12 tiles, the complete frame
             "rect": abi.full_frame_tiles(SIZE[0], SIZE[1], rect=abi.TileRect(1, 0, 5, 4))}                # 20 tiles, the rest untouched
    order = ["fill", "whole", "rect", "whole", "fill", "rect", "whole"][:n]
    plist = [frame_params(scene, block, i % 2, kinds[k], radius=FAR) for i, k in enumerate(order)]
    for p in plist:        # the box lies inside the fill_outside rectangle
        box = lib.screen_tile_rect(p.ray_cast, p.ray_gen, SIZE, (16, 16), 1)
        assert box.x0 >= rect.x0 and box.y0 >= rect.y0 and box.x0 + box.w <= rect.x0 + rect.w and box.y0 + box.h <= rect.y0 + rect.h, box.as_tuple()
    if n > 1:
        assert len({p.tiles.tile_count for p in plist}) > 1
    ctx.set_tuning(batch_sequential=sequential)
    try:
        got = launch(ctx, v, plist)
    finally:
        ctx.set_tuning(batch_sequential=0)
    for i, k in enumerate(order):
        ref = oracle_frame(scenes, block, i % 2, kinds[k], "whole" if k == "fill" else k, radius=FAR)
        assert_frame(got[i], ref, "%d frames, sequential %d, frame %d (%s)" % (n, sequential, i, k))


@pytest.mark.parametrize("single", [False, True], ids=["batch", "vkv_render"])
def test_a_ranks_share_of_the_tiles(ctx, scenes, single):
    block = (3, 5, 6)
    scene, v, _ = scenes[block]
    tiles = abi.full_frame_tiles(SIZE[0], SIZE[1], rank=1, world=3, compact=True)
    assert (tiles.tile_first, tiles.tile_stride, tiles.compact, tiles.tile_count) == (1, 3, 1, 12)
    plist = [frame_params(scene, block, cam, tiles) for cam in (0, 1)]
    for cam, got in enumerate(launch(ctx, v, plist, single=single)):
        assert_frame(got, oracle_frame(scenes, block, cam, tiles, "share"), "share of rank 1 of 3, camera %d" % cam)


def test_a_registered_target_rendered_twice(ctx, scenes):
    block = (4, 4, 4)
    scene, v, _ = scenes[block]
    size = (128, 128)        # 64 tiles: the smallest schedule whose start order is measured
    p = frame_params(scene, block, 0, abi.full_frame_tiles(size[0], size[1]), size)
    ref = oracle_frame(scenes, block, 0, size=size)
    target = torch.zeros((size[1], size[0], 4), dtype=torch.uint8, device="cuda")
    q = abi.RenderParams.from_buffer_copy(V.VolumeRenderSubpass(ctx, v, p.options, size).bind(p))
    q.d_out_color, q.d_out_rgba8, q.d_out_counts, q.d_out_depth = None, target.data_ptr(), None, None
    st = torch.cuda.current_stream().cuda_stream
    ctx.register_target(target.data_ptr(), size, q.tiles)
    try:
        for frame in range(3):        # the first measures the tile costs, the following ones start in the measured order
            target.zero_()
            ctx.render_batch([q], st)
            torch.cuda.synchronize()
            assert np.array_equal(target.cpu().numpy(), ref.rgba8), "frame %d into the registered target" % frame
    finally:
        ctx.forget_target(target.data_ptr())


def test_a_launch_with_a_depth_output(ctx, scenes):
    block = (8, 2, 16)
    scene, v, _ = scenes[block]
    tiles = abi.full_frame_tiles(SIZE[0], SIZE[1], 32, 16)
    plist = [frame_params(scene, block, cam, tiles) for cam in (0, 1)]
    for cam, got in enumerate(launch(ctx, v, plist, with_depth=True)):
        ref = oracle_frame(scenes, block, cam)
        assert_frame(got, ref, "depth output, camera %d" % cam)
        assert float(np.abs(got["depth"] - ref.depth).max()) <= DEPTH_TOL


def test_the_single_frame_kernel(ctx, scenes):
    block = (3, 5, 6)
    scene, v, _ = scenes[block]
    for tile in ((48, 32), (32, 16)):
        tiles = abi.full_frame_tiles(SIZE[0], SIZE[1], tile[0], tile[1])
        plist = [frame_params(scene, block, cam, tiles) for cam in (0, 1)]
        for cam, got in enumerate(launch(ctx, v, plist, single=True)):
            assert_frame(got, oracle_frame(scenes, block, cam), "vkv_render, tile %s, camera %d" % (tile, cam))

"""GPU: every path of the ray set-up (ray_setup.hpp) against the oracle on frames small enough for a few seconds.

Volume 32 x 32 x 24; frames 64 x 48 and 40 x 24 (ragged edge tiles).  Per-axis block sizes (4, 4, 4) and (2, 4, 8) - powers of two: the
set-up multiplies by the exact reciprocal - (5, 4, 6) and (3, 3, 3) - it divides.  All four skipping types with and without early ray
termination, through vkv_render and vkv_render_batch (3 frames, with and without d_out_counts).  Cameras: a generic one; one whose rays
through one pixel column and one pixel row are exactly axis-parallel, so that some lanes of a wave fail the range test and the wave repeats the
set-up with the IEEE divisions; one inside the box; one turned away (no fragment anywhere).  Each frame against the oracle: the three
counters and RGBA8 bit for bit, float colour and depth within the parity tests' tolerances.  One MIP, one isosurface and one slab frame of
the same size against their numpy restatements (they share the set-up)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_gpu_parity import COLOR_TOL, DEPTH_TOL, compare_render, gpu_render, make_gpu_volume
from vkvolume_amd import abi, camera, volume as V

pytestmark = pytest.mark.gpu

SHAPE = (32, 32, 24)
SIZES = ((64, 48), (40, 24))
MAPS = {(4, 4, 4): (8, 8, 6), (2, 4, 8): (16, 8, 3), (3, 3, 3): (11, 11, 8), (5, 4, 6): (7, 8, 4)}        # block sizes -> map extent


class AxisBlockScene(T.OracleScene):
    """an oracle scene whose map extent is given per axis (block size = ceil(volume extent / map extent))"""

    def __init__(self, vol, options, map_whd):
        super().__init__(vol, options, 4)
        self.map_extent = abi.Extent3D(*map_whd)

    def maps(self, skipping_type):
        if skipping_type not in self._maps:
            me = self.map_extent
            maps = np.zeros((8, me.depth, me.height, me.width), np.uint8)
            swap = np.zeros((me.depth, me.height, me.width), np.uint8)
            ptrs = (C.c_void_p * 8)(*[maps[i].ctypes.data for i in range(8)])
            O.lib().vkvo_compute_distance_map(O._ptr(self.vol), O._ptr(self.grad), O._ptr(self.tex), C.byref(self.tf), self.extent, ptrs, O._ptr(swap),
                                              me, skipping_type)
            self._maps[skipping_type] = maps[:8 if skipping_type == abi.SKIP_ANISOTROPIC_DISTANCE else 1].copy()
        return self._maps[skipping_type]


@pytest.fixture(scope="module")
def scenes(ctx):
    """per block size: the oracle scene and the device volume with the map extent that gives it"""
    vol = O.synth_volume(SHAPE, 1, 0x5E7)
    out = {}
    for block, map_whd in MAPS.items():
        scene = AxisBlockScene(vol, abi.VolumeOptions(**T.APP_TF), map_whd)
        v, tf = make_gpu_volume(ctx, scene)
        me = scene.map_extent
        v.map_extent = me
        v.distance_map_swap = torch.empty((me.depth, me.height, me.width), dtype=torch.uint8, device="cuda")
        v.distance_maps = []
        out[block] = (scene, v, tf)
    return out


def cameras(scene, size, opts):
    """(name, RenderParams) of the four cameras"""
    w, h = size
    view, proj = T.orbit(33.0, image_size=size)
    generic = scene.params(view, proj, size, opts)
    # rays (x, y, 1) / 64 around the box's axis, every term a dyadic fraction: the ray through pixel (w / 2, h / 2) is (0, 0, 1) exactly, its pixel
    # column has x = 0 and its pixel row y = 0 - 1 / 0 in the box test
    axis = abi.RenderParams.from_buffer_copy(generic)
    s = 1.0 / 64.0
    for k in range(3):
        axis.ray_gen.ddx[k], axis.ray_gen.ddy[k] = (s, 0.0, 0.0)[k], (0.0, s, 0.0)[k]
        axis.ray_gen.dir00[k] = (-(w / 2 + 0.5) * s, -(h / 2 + 0.5) * s, 1.0)[k]
        axis.ray_cast.camera_pos_tex[k] = (0.5, 0.5, -2.0)[k]
    for k in range(4):
        axis.ray_cast.plane_tex[k] = (0.0, 0.0, 1.0, 1.5)[k]
    assert np.float32(axis.ray_gen.dir00[0]) + np.float32(w / 2 + 0.5) * np.float32(s) == 0.0
    inside = abi.RenderParams.from_buffer_copy(generic)
    for k in range(3):
        inside.ray_cast.camera_pos_tex[k] = (0.4, 0.55, 0.45)[k]
    inside.ray_cast.plane_tex[3] = -sum(inside.ray_cast.plane_tex[k] * inside.ray_cast.camera_pos_tex[k] for k in range(3)) - 0.01        # just in front of the eye
    away = abi.RenderParams.from_buffer_copy(generic)
    for k in range(3):
        away.ray_gen.dir00[k], away.ray_gen.ddx[k], away.ray_gen.ddy[k] = -generic.ray_gen.dir00[k], -generic.ray_gen.ddx[k], -generic.ray_gen.ddy[k]
    return [("generic", generic), ("axis-parallel", axis), ("inside", inside), ("away", away)]


def check_batch(ctx, v, plist, refs, with_counts, label):
    """the frames of plist in one vkv_render_batch launch against the oracle's"""
    size = (plist[0].image_width, plist[0].image_height)
    sp = V.VolumeRenderSubpass(ctx, v, plist[0].options, size)
    outs, qs = [], []
    for p in plist:
        o = dict(color=torch.full((size[1], size[0], 4), -1.0, dtype=torch.float32, device="cuda"),
                 depth=torch.full((size[1], size[0]), -1.0, dtype=torch.float32, device="cuda"),
                 rgba8=torch.full((size[1], size[0], 4), 7, dtype=torch.uint8, device="cuda"),
                 counts=torch.full((size[1], size[0], 3), 9, dtype=torch.int32, device="cuda") if with_counts else None)
        q = abi.RenderParams.from_buffer_copy(sp.bind(p))
        q.d_out_color, q.d_out_depth, q.d_out_rgba8 = o["color"].data_ptr(), o["depth"].data_ptr(), o["rgba8"].data_ptr()
        q.d_out_counts = o["counts"].data_ptr() if with_counts else None
        outs.append(o), qs.append(q)
    ctx.render_batch(qs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i, (o, ref) in enumerate(zip(outs, refs)):
        what = "%s batch frame %d counts %d" % (label, i, with_counts)
        if with_counts:
            assert np.array_equal(o["counts"].cpu().numpy().astype(np.uint32), ref.counts), what
        assert np.array_equal(o["rgba8"].cpu().numpy(), ref.rgba8), what
        assert float(np.abs(o["color"].cpu().numpy() - ref.color).max()) <= COLOR_TOL, what
        assert float(np.abs(o["depth"].cpu().numpy() - ref.depth).max()) <= DEPTH_TOL, what


@pytest.mark.parametrize("ert", [True, False])
@pytest.mark.parametrize("skipping_type", [abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE])
@pytest.mark.parametrize("block", sorted(MAPS))
def test_set_up_paths_against_the_oracle(ctx, scenes, block, skipping_type, ert):
    scene, v, tf = scenes[block]
    V.ComputeDistanceMap(ctx).compute(v, tf, skipping_type)
    if skipping_type != abi.SKIP_NONE:
        assert np.array_equal(v.distance_maps[0].cpu().numpy(), scene.maps(skipping_type)[0])
    opts = abi.RenderOptions(skipping_type=skipping_type, clip_distance=1.0, early_ray_termination=ert)
    for size in SIZES:
        cams = cameras(scene, size, opts)
        assert tuple(cams[0][1].ray_cast.block_size)[:3] == tuple(float(b) for b in block)
        refs = []
        for name, p in cams:
            ref = scene.render(p, want_rgba8=True)
            refs.append(ref)
            marched = int((ref.counts[..., 0] > 0).sum())
            assert (marched == 0) if name == "away" else (marched > size[0] * size[1] // 8), (name, marched)
            label = "block %s mode %d ert %d %s %dx%d" % (block, skipping_type, ert, name, size[0], size[1])
            got = gpu_render(ctx, v, p, want_rgba8=True)
            compare_render(got, ref, label)
            assert np.array_equal(got[3], ref.rgba8), label
        for with_counts in (True, False):
            check_batch(ctx, v, [p for _, p in cams[:3]], refs[:3], with_counts, "block %s mode %d ert %d %dx%d" % (block, skipping_type, ert, size[0], size[1]))


def test_direct_renderers_share_the_set_up(ctx):
    """one MIP, one isosurface and one slab frame of 64 x 48 against their numpy restatements, bit for bit"""
    from tests import test_gpu_iso as GI, test_gpu_mip as GM, test_gpu_slab as GS
    from tests.test_iso_cpu import iso_np, iso_options
    from tests.test_mip_cpu import mip_np
    from tests.test_slab_cpu import slab_np, slab_options
    size = SIZES[0]
    vol = O.synth_volume(SHAPE, 1, 0x5E7)
    v = GM.make_volume(ctx, vol)
    sp, p = GM.subpass(v, size=size)
    ref = mip_np(p, vol, abi.MipOptions(threshold=0.2, window_max=0.8))
    assert ref["found"].sum() > 50
    GM.assert_matches_numpy(GM.draw(sp, p, 0.2, 0.8, skip=False, size=size), ref, "mip")
    v = GI.make_volume(ctx, vol)
    sp, p = GI.subpass(v, size=size)
    opts = iso_options(0.3, 4)
    ref = iso_np(p, vol, opts)
    assert ref["found"].sum() > 50
    GI.assert_matches_numpy(GI.draw(sp, p, opts.iso, skip=False, size=size, **GI.kw_of(opts)), ref, "iso")
    v = GS.make_volume(ctx, vol)
    sp, p = GS.bound(v, size)
    o = slab_options(camera.slab_plane(SHAPE, axis="z", index=SHAPE[2] // 2, image_size=size), samples=17, window=(0.0, 1.0))
    ref = slab_np(p, vol, o)
    assert int(ref["count"].sum()) > 50
    GS.assert_matches(GS.draw(sp, p, o, skip=False), ref, "slab")

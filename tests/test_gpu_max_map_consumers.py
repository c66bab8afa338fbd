"""GPU: the seeded sweep of the max map's geometry (tests/test_gpu_max_map_sweep.py does it for the ray renderers) through the four other
entry points that skip over the map, each with cell arithmetic of its own: vkv_isosurface_mesh and vkv_isosurface_mesh_indexed (tile_is_empty,
dealt over cubes and over voxels), vkv_label_components (the per-voxel cell test of k_cc_init) and vkv_render_slab in MAX mode (max_map_skip
along a camera-less column).  VKV_TEST_FUZZ_SEEDS=n draws per family; the recipe is tests/test_max_map_consumers_cpu.py's
(draw_consumer_geometry: widths of one to three x-segments of the 256-cube tile, around 256 + 8 lanes, thin heights and depths; a map extent
per axis: block 1, blocks 2-9, one cell, cells past the volume; six kinds of content; isos on and beside the map's own bytes), where the
skipping of mesh and labels, which have no counters, is predicted and required not to be vacuous.  Per draw:
  1. vkv_max_map equals max_map_np;
  2. vkv_isosurface_mesh through the map equals the dense call byte for byte, counts included, the dense call equals mesh_np, and the call
     through the map with capacity total // 2 gives the exact prefix;
  3. vkv_isosurface_mesh_indexed likewise against indexed_np, with and without normals, with each capacity short in turn;
  4. vkv_label_components under 6, 14 and 26 likewise against components_np, and with a short capacity;
  5. (test_slab_sweep) the MAX slab on a random oblique plane: skip equals dense on value, colour and RGBA8 bits, dense equals slab_np, the
     three counters equal the restated walk's pixel by pixel, and every skipping family skipped samples;
  6. on half the draws a box whose origins are 0, a cell edge, a cell edge +- 1 or anything: 2-4 on the box against the cropped array;
  7. on the other half a box of the device volume is overwritten, vkv_max_map(box) must leave the WHOLE map equal to max_map_np of the new
     volume, and 2 is repeated on the new volume through that map.
Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole; all guards must be intact and the volume
unchanged, so nothing here relies on, or can cause, a fault."""
import os

import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_components_cpu import components_np
from tests.test_gpu_components import check as check_labels
from tests.test_gpu_mesh import FILL, ext_of, st
from tests.test_gpu_mesh import check as check_soup
from tests.test_gpu_mesh_indexed import check as check_indexed
from tests.test_gpu_mesh_indexed import guard_damage
from tests.test_gpu_slab import KEYS, assert_matches, bits
from tests.test_max_map_consumers_cpu import DEFAULT_SEEDS, FAMILIES, SKIPPING, draw_box, draw_consumer_geometry, draw_isos, seed_of, slab_of
from tests.test_mesh_cpu import mesh_np
from tests.test_mesh_indexed_cpu import indexed_np
from tests.test_mip_cpu import max_map_np
from tests.test_slab_cpu import slab_np, slab_samples_np, slab_skip_np
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu
SEEDS = int(os.environ.get("VKV_TEST_FUZZ_SEEDS", str(DEFAULT_SEEDS)))
CONNECTIVITIES = (6, 14, 26)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def assert_guards(handles, what):
    for name, h in handles:
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)


def same_arrays(a, b, what):
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), what


def consumers(ctx, vol, me, iso, box, what, max_map=None, soup_only=False, short=True):
    """checks 2-4 of one (volume, map extent, iso, box): dense against numpy, through the map against numpy and against the dense bytes,
    short capacities through the map"""
    iso = float(iso)
    kw = dict(box=box, map_extent=me, max_map=max_map)
    want = mesh_np(vol, iso, box)
    dense = check_soup(ctx, vol, iso, want, box=box, what=what + ": mesh, dense")
    fast = check_soup(ctx, vol, iso, want, what=what + ": mesh, max map", **kw)
    same_arrays(dense, fast, what + ": mesh, max map against dense")
    if short:
        check_soup(ctx, vol, iso, want, capacity=len(want) // 2, what=what + ": mesh, max map, half the capacity", **kw)
    if soup_only:
        return
    want = indexed_np(vol, iso, box)
    nv, nt = len(want[0]), len(want[2])
    dense = check_indexed(ctx, vol, iso, want, box=box, what=what + ": indexed, dense")
    fast = check_indexed(ctx, vol, iso, want, what=what + ": indexed, max map", **kw)
    same_arrays(dense, fast, what + ": indexed, max map against dense")
    check_indexed(ctx, vol, iso, want, normals=False, what=what + ": indexed, max map, no normals", **kw)
    if short:
        check_indexed(ctx, vol, iso, want, cap_v=nv // 2, normals=nv // 2 > 0, what=what + ": indexed, max map, vertices short", **kw)        # (normals need room)
        check_indexed(ctx, vol, iso, want, cap_t=nt // 2, normals=False, what=what + ": indexed, max map, triangles short", **kw)
    crop = vol if box is None else np.ascontiguousarray(vol[box[2]:box[2] + box[5], box[1]:box[1] + box[4], box[0]:box[0] + box[3]])
    for c in CONNECTIVITIES:
        want = components_np(crop, iso, c)
        dense = check_labels(ctx, vol, iso, c, want, box=box, what=what + ": labels %d, dense" % c)
        fast = check_labels(ctx, vol, iso, c, want, what=what + ": labels %d, max map" % c, **kw)
        same_arrays(dense, fast, what + ": labels %d, max map against dense" % c)
        if short:
            check_labels(ctx, vol, iso, c, want, cap=int(want[2][0]) // 2, what=what + ": labels %d, max map, short capacity" % c, **kw)


@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("family", FAMILIES)
def test_max_map_consumers_sweep(ctx, family, seed):
    rng = np.random.default_rng(seed_of(family, seed))
    g = draw_consumer_geometry(rng, family)
    vol, me, shape = g["vol"], g["map_extent"], g["shape"]
    what = "%s seed %d, %s, map %s (blocks %s)" % (family, seed, shape, me, g["blocks"])
    # 1. the map of this extent
    d_vol, h_vol = T.guarded(vol, 0, 0x00, "cuda")
    d_map, h_map = T.guarded((me[2], me[1], me[0]), 0, FILL, "cuda")
    handles = [("d_volume", h_vol), ("d_max_map", h_map)]
    ctx.max_map(d_vol.data_ptr(), ext_of(vol), abi.Extent3D(*me), None, d_map.data_ptr(), st())
    torch.cuda.synchronize()
    assert_guards(handles, what)
    mm = max_map_np(vol, me)
    assert np.array_equal(d_map.cpu().numpy(), mm) and np.array_equal(d_vol.cpu().numpy(), vol), what + ": vkv_max_map"
    isos = draw_isos(rng, mm)
    slab_of(rng, g)        # (test_slab_sweep's part of the draw: the same stream of numbers as tests/test_max_map_consumers_cpu.py)
    # 2-4. the whole volume
    for iso in isos:
        consumers(ctx, vol, me, iso, None, "%s, iso %r" % (what, float(iso)))
    if rng.random() < 0.5:
        # 6. a box
        box = draw_box(rng, shape, g["blocks"])
        for iso in isos:
            consumers(ctx, vol, me, iso, box, "%s, box %s, iso %r" % (what, box, float(iso)), short=False)
    else:
        # 7. new bytes in a box of the device volume, the map rebuilt over that box alone
        x0, y0, z0, bw, bh, bd = draw_box(rng, shape, g["blocks"])
        new = vol.copy()
        new[z0:z0 + bd, y0:y0 + bh, x0:x0 + bw] = rng.integers(0, 256, (bd, bh, bw), dtype=np.uint8)
        d_vol.copy_(torch.from_numpy(new))
        ctx.max_map(d_vol.data_ptr(), ext_of(vol), abi.Extent3D(*me), abi.Box(x0, y0, z0, bw, bh, bd), d_map.data_ptr(), st())
        torch.cuda.synchronize()
        assert_guards(handles, what)
        updated = d_map.cpu().numpy()
        at = "%s, box %s rewritten" % (what, (x0, y0, z0, bw, bh, bd))
        assert np.array_equal(updated, max_map_np(new, me)) and np.array_equal(d_vol.cpu().numpy(), new), at + ": vkv_max_map(box)"
        for iso in isos:
            consumers(ctx, new, me, iso, None, "%s, iso %r" % (at, float(iso)), max_map=updated, soup_only=True)


# ---- 5. the MAX slab ---------------------------------------------------------------------------------------------------------------------
def draw_slab(ctx, p, o, d_vol, d_map, handles, what):
    """the four outputs of ONE vkv_render_slab call on guarded buffers pre-filled with FILL; d_map None: dense"""
    n = p.image_width * p.image_height
    out, hs = {}, list(handles)
    for key, shape, dtype in (("value", (n,), np.float32), ("color", (n, 4), np.float32), ("rgba8", (n, 4), np.uint8), ("counts", (n, 3), np.int32)):
        out[key], h = T.guarded(shape, 0, FILL, "cuda", dtype=dtype)
        hs.append((key, h))
    q = abi.RenderParams.from_buffer_copy(p)
    q.d_volume = d_vol.data_ptr()
    q.d_out_color, q.d_out_rgba8, q.d_out_counts = out["color"].data_ptr(), out["rgba8"].data_ptr(), out["counts"].data_ptr()
    s = abi.SlabOptions.from_buffer_copy(o)
    s.d_max_map = None if d_map is None else d_map.data_ptr()
    s.d_out_value = out["value"].data_ptr()
    ctx.render_slab(q, s, st())
    torch.cuda.synchronize()
    assert_guards(hs, what)
    return {k: t.cpu().numpy() for k, t in out.items()}


@pytest.mark.parametrize("family", FAMILIES)
def test_slab_sweep(ctx, family):
    skipped_gpu = skipped_walk = 0
    for seed in range(SEEDS):
        rng = np.random.default_rng(seed_of(family, seed))
        g = draw_consumer_geometry(rng, family)
        vol, me = g["vol"], g["map_extent"]
        mm = max_map_np(vol, me)
        draw_isos(rng, mm)
        p, o = slab_of(rng, g)
        what = "%s seed %d, %s, map %s, %d samples" % (family, seed, g["shape"], me, o.samples)
        d_vol, h_vol = T.guarded(vol, 0, 0x00, "cuda")
        d_map, h_map = T.guarded((me[2], me[1], me[0]), 0, FILL, "cuda")
        handles = [("d_volume", h_vol), ("d_max_map", h_map)]
        ctx.max_map(d_vol.data_ptr(), ext_of(vol), abi.Extent3D(*me), None, d_map.data_ptr(), st())
        dense = draw_slab(ctx, p, o, d_vol, None, handles, what + ": dense")
        fast = draw_slab(ctx, p, o, d_vol, d_map, handles, what + ": skip")
        assert np.array_equal(d_map.cpu().numpy(), mm) and np.array_equal(d_vol.cpu().numpy(), vol), what
        for k in KEYS:
            assert np.array_equal(bits(fast[k]), bits(dense[k])), (what, k, "skip against dense")
        S = slab_samples_np(p, vol, o)
        assert_matches(dense, slab_np(p, vol, o, S), what + ": dense")
        walk = slab_skip_np(p, vol, mm, o, S)
        assert_matches(fast, walk, what + ": skip", counts=walk["counts"])
        skipped_gpu += int(fast["counts"][:, 2].astype(np.int64).sum())
        skipped_walk += int(walk["counts"][:, 2].sum())
    assert skipped_gpu == skipped_walk
    if family in SKIPPING and SEEDS >= DEFAULT_SEEDS:
        assert skipped_gpu > 0 and skipped_walk > 0, family

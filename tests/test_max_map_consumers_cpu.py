"""The draw recipe of tests/test_gpu_max_map_consumers.py (the max map's geometry swept through vkv_isosurface_mesh,
vkv_isosurface_mesh_indexed, vkv_label_components and the MAX slab), and the proof, without a GPU, that the sweep is not vacuous.

Mesh and labels have no counters, so their skipping is predicted here: tile_empty_np restates the tile-empty rule of mesh_common.hpp (a tile
is 256 x 4 x 16 cubes, or voxels for the indexed list, of the box; it is empty when every map cell that holds one of its origins is below the
inside threshold), cell_below_np the per-voxel cell test of the labels.  For the families that have something to skip, at least a third of the
(draw, iso, list kind) pairs at the default seeds must have an empty tile, a kept tile and a surface; at least a third of the (draw, iso)
pairs a cell below the threshold and an inside voxel; and the restated slab walk must skip samples.  These are conditions on the recipe."""
import numpy as np
import pytest

from tests.test_max_map_skip_cpu import _map_axis, bound_candidates, place_bright_voxels
from tests.test_mip_cpu import INV255, max_map_np
from tests.test_slab_cpu import random_plane, slab_options, slab_params, slab_skip_np

F = np.float32
FAMILIES = ("blobs", "bright_voxels", "plateau", "random", "all_255", "all_0")
SKIPPING = ("blobs", "bright_voxels", "plateau")        # the families with something to skip; the others are controls
DEFAULT_SEEDS = 6
MAX_VOXELS = 300000
TILE = (256, 4, 16)        # kMeshTileX, kMeshTileY, kMeshSegment
SLAB_IMAGE = (40, 28)


def seed_of(family, seed):
    return 47000 + 100 * seed + FAMILIES.index(family)


def blocks_of(shape, me):
    """block_of per axis: ceil(extent / map extent)"""
    return tuple(-(-e // m) for e, m in zip(shape, me))


def _thin(rng, lo, hi):
    x = int(rng.integers(lo, hi + 1))
    return 2 if rng.random() < 0.1 else x


def draw_consumer_geometry(rng, family):
    """one draw: dict shape (w, h, d), vol (d, h, w) uint8, map_extent (w, h, d), blocks.  Widths of one to three x-segments of the 256-cube
    tile (2-64, around 256 + 8 lanes, 65-600), heights of up to ten tile rows and depths of up to four segments, at most MAX_VOXELS voxels"""
    r = rng.random()
    if r < 0.4:
        w = int(rng.integers(2, 65))
    elif r < 0.6:
        w = int(rng.integers(255, 262))
    else:
        w = int(rng.integers(65, 601))
    while True:
        h, d = _thin(rng, 2, 40), _thin(rng, 2, 50)
        if w * h * d <= MAX_VOXELS:
            break
    shape = (w, h, d)
    while True:
        me = tuple(_map_axis(rng, e) for e in shape)
        blocks = blocks_of(shape, me)
        if family != "plateau" or all(b <= max(e // 3, 1) for b, e in zip(blocks, shape)):        # the plateau: several cells per axis
            break
    if family == "blobs":        # dim noise with one to three small bright balls
        vol = rng.integers(0, 60, (d, h, w), dtype=np.uint8)
        z, y, x = np.indices((d, h, w)).astype(np.float64)
        for _ in range(int(rng.integers(1, 4))):
            cx, cy, cz = (float(rng.uniform(0, e - 1)) for e in shape)
            radius = float(rng.uniform(1.5, 4.0))
            dist = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
            vol = np.maximum(vol, np.clip((radius - dist) * 60 + 128, 0, 255).astype(np.uint8))
    elif family == "bright_voxels":
        vol = rng.integers(0, 24, (d, h, w), dtype=np.uint8)
        place_bright_voxels(rng, vol, shape, blocks)
    elif family == "plateau":
        plateau = int(rng.integers(1, 255))
        vol = rng.integers(0, plateau, (d, h, w), dtype=np.uint8) // 2
        x0, y0, z0 = (int(rng.integers(0, e)) for e in shape)
        vol[z0:z0 + int(rng.integers(1, d + 1)), y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = plateau
    elif family == "random":
        vol = rng.integers(0, 256, (d, h, w), dtype=np.uint8)
    elif family == "all_255":
        vol = np.full((d, h, w), 255, np.uint8)
    elif family == "all_0":
        vol = np.zeros((d, h, w), np.uint8)
    else:
        raise ValueError(family)
    return dict(shape=shape, vol=vol, map_extent=me, blocks=blocks)


def draw_isos(rng, mm):
    """two random candidates of bound_candidates (the map's bytes as floats, their float neighbours, 0, 1, 1.01) and the map's largest byte: a
    tie with a cell on every draw"""
    cand = bound_candidates(mm)
    return [cand[int(rng.integers(0, len(cand)))] for _ in range(2)] + [F(int(mm.max())) * INV255]


def draw_box(rng, shape, blocks):
    """(x0, y0, z0, w, h, d): each origin 0, a cell edge, a cell edge +- 1 or anything; each size 1 .. the rest of the axis"""
    origin, size = [], []
    for e, b in zip(shape, blocks):
        edge = int(rng.integers(0, -(-e // b))) * b
        o = int(rng.choice([0, edge, edge - 1, edge + 1, int(rng.integers(0, e))]))
        o = min(max(o, 0), e - 1)
        origin.append(o)
        size.append(int(rng.integers(1, e - o + 1)))
    return tuple(origin) + tuple(size)


def thr_of(iso):
    """the smallest byte that is inside at iso (256: none): mesh_geom's loop"""
    thr = 0
    while thr < 256 and not F(thr) * INV255 >= F(iso):
        thr += 1
    return thr


def tile_empty_np(shape, mm, iso, box=None, voxels=False):
    """bool [tiles z, tiles y, tiles x]: the tiles of the box's cubes (voxels: of its voxels, the indexed list) that the kernels skip"""
    x0, y0, z0, bw, bh, bd = (0, 0, 0) + tuple(shape) if box is None else box
    n = [bw - 1, bh - 1, bd - 1]
    if voxels:
        n = [c + 1 for c in n] if min(n) > 0 else [0, 0, 0]
    md, mh, mw = mm.shape
    blocks = blocks_of(shape, (mw, mh, md))
    below = mm < thr_of(iso)
    counts = [-(-c // t) for c, t in zip(n, TILE)]
    if min(n) <= 0:
        return np.zeros((0, 0, 0), bool)
    out = np.zeros(counts[::-1], bool)
    cells = []
    for axis, (o, c, t, b) in enumerate(zip((x0, y0, z0), n, TILE, blocks)):
        cells.append([slice((o + k * t) // b, (o + min(k * t + t, c) - 1) // b + 1) for k in range(counts[axis])])
    for tz, sz in enumerate(cells[2]):
        for ty, sy in enumerate(cells[1]):
            for tx, sx in enumerate(cells[0]):
                out[tz, ty, tx] = below[sz, sy, sx].all()
    return out


def cell_below_np(shape, mm, iso):
    """bool (d, h, w): the voxels that vkv_label_components does not read (their cell's byte is below the threshold)"""
    md, mh, mw = mm.shape
    bx, by, bz = blocks_of(shape, (mw, mh, md))
    w, h, d = shape
    below = mm < thr_of(iso)
    return below[np.arange(d)[:, None, None] // bz, np.arange(h)[None, :, None] // by, np.arange(w)[None, None, :] // bx]


def inside_of(vol, iso):
    return vol.astype(F) * INV255 >= F(iso)


def slab_of(rng, g):
    """(params, options) of the draw's MAX slab: a random oblique plane of the draw's extent, the map extent the drawn one"""
    p = slab_params(g["shape"], SLAB_IMAGE, map_extent=g["map_extent"])
    plane = random_plane(rng, g["shape"], SLAB_IMAGE)
    return p, slab_options(plane, samples=plane["samples"])


def draws(family, seeds=DEFAULT_SEEDS):
    for seed in range(seeds):
        rng = np.random.default_rng(seed_of(family, seed))
        g = draw_consumer_geometry(rng, family)
        mm = max_map_np(g["vol"], g["map_extent"])
        yield rng, g, mm, draw_isos(rng, mm)


# ---- the recipe -------------------------------------------------------------------------------------------------------------------------
def test_the_recipe_draws_what_it_says():
    widths, thin, past, block1, one_cell, per_axis = [], 0, 0, 0, 0, 0
    for family in FAMILIES:
        for rng, g, mm, isos in draws(family, 40):
            w, h, d = g["shape"]
            assert 2 <= w <= 600 and 2 <= h <= 40 and 2 <= d <= 50 and w * h * d <= MAX_VOXELS
            assert g["vol"].shape == (d, h, w) and g["vol"].dtype == np.uint8 and len(isos) == 3
            widths.append(w)
            thin += int(h == 2 or d == 2)
            past += int(any((e - 1) // b < m - 1 for e, b, m in zip(g["shape"], g["blocks"], g["map_extent"])))
            block1 += int(1 in g["blocks"])
            one_cell += int(1 in g["map_extent"])
            per_axis += int(len(set(g["blocks"])) > 1)
            box = draw_box(rng, g["shape"], g["blocks"])
            assert all(o >= 0 and s >= 1 and o + s <= e for o, s, e in zip(box[:3], box[3:], g["shape"]))
    widths = np.array(widths)
    n = len(widths)
    assert (widths <= 64).sum() > n / 4 and ((widths >= 255) & (widths <= 261)).sum() > n / 8 and (widths > 261).sum() > n / 6
    assert thin > n / 10 and past > n / 10 and block1 > n / 10 and one_cell > n / 10 and per_axis > n / 2


def test_the_tile_rule_on_a_hand_made_map():
    """300 x 9 x 20, blocks (4, 3, 4): cubes 299 x 8 x 19 = 2 x 2 x 2 tiles, voxels 300 x 9 x 20 = 2 x 3 x 2; one bright voxel in the far corner
    cell (x 296 .. 299, y 6 .. 8, z 16 .. 19), away from that cell's faces, so that only that cell's byte rises"""
    shape = (300, 9, 20)
    vol = np.zeros((20, 9, 300), np.uint8)
    vol[17, 8, 299] = 200
    mm = max_map_np(vol, (75, 3, 5))
    assert (mm != 0).sum() == 1 and mm[4, 2, 74] == 200
    empty = tile_empty_np(shape, mm, 0.5)
    assert empty.shape == (2, 2, 2) and not empty[1, 1, 1] and empty.sum() == 7        # cube rows 4 .. 7 lie in the cells of rows 3 .. 5 and 6 .. 8
    empty = tile_empty_np(shape, mm, 0.5, voxels=True)
    assert empty.shape == (2, 3, 2) and not empty[1, 1, 1] and not empty[1, 2, 1] and empty.sum() == 10        # voxel row 8 is a tile of its own
    assert tile_empty_np(shape, mm, float(F(200) * INV255)).sum() == 7 and tile_empty_np(shape, mm, float(np.nextafter(F(200) * INV255, F(2)))).all()
    assert tile_empty_np(shape, mm, 0.0).sum() == 0
    # boxes: one tile whose last cube origins (298, 7, 18) lie in the bright cell; one that ends before it; one without a cube
    box = (255, 5, 14, 45, 4, 6)
    assert tile_empty_np(shape, mm, 0.5, box).shape == (1, 1, 1) and not tile_empty_np(shape, mm, 0.5, box)[0, 0, 0]
    assert tile_empty_np(shape, mm, 0.5, (255, 5, 14, 42, 4, 6)).all()        # cube origins up to x = 295: the cell before
    assert tile_empty_np(shape, mm, 0.5, (255, 5, 14, 41, 4, 6), voxels=True).all() and not tile_empty_np(shape, mm, 0.5, (255, 5, 14, 42, 4, 6), voxels=True).any()
    assert tile_empty_np(shape, mm, 0.5, (0, 0, 0, 290, 5, 14)).shape == (1, 1, 2) and tile_empty_np(shape, mm, 0.5, (0, 0, 0, 290, 5, 14)).all()
    assert tile_empty_np(shape, mm, 0.5, (0, 0, 0, 1, 9, 20)).size == 0 and tile_empty_np(shape, mm, 0.5, (0, 0, 0, 1, 9, 20), voxels=True).size == 0
    below = cell_below_np(shape, mm, 0.5)
    assert below.shape == vol.shape and below.sum() == 300 * 9 * 20 - 4 * 3 * 4
    assert not below[16, 6, 296] and not below[19, 8, 299] and below[15, 6, 296] and below[16, 5, 296] and below[16, 6, 295]


@pytest.mark.parametrize("family", FAMILIES)
def test_the_sweep_skips_tiles_and_keeps_tiles(family):
    pairs = good = 0
    for rng, g, mm, isos in draws(family):
        for iso in isos:
            inside = inside_of(g["vol"], iso)
            surface = bool(inside.any() and not inside.all())
            for voxels in (False, True):
                empty = tile_empty_np(g["shape"], mm, iso, voxels=voxels)
                pairs += 1
                good += int(surface and bool(empty.any()) and not bool(empty.all()))
    print("%s: %d of %d (draw, iso, list kind) pairs have an empty tile, a kept tile and a surface" % (family, good, pairs))
    assert pairs == 6 * DEFAULT_SEEDS
    if family in SKIPPING:
        assert 3 * good >= pairs, (family, good, pairs)
    elif family != "random":        # (random bytes: a thin tile of block-1 cells can miss the map's largest byte)
        assert good == 0, (family, good)


@pytest.mark.parametrize("family", SKIPPING)
def test_the_sweep_skips_cells_of_the_labels(family):
    pairs = good = 0
    for rng, g, mm, isos in draws(family):
        for iso in isos:
            pairs += 1
            good += int(bool(cell_below_np(g["shape"], mm, iso).any()) and bool(inside_of(g["vol"], iso).any()))
    print("%s: %d of %d (draw, iso) pairs have a cell below the threshold and an inside voxel" % (family, good, pairs))
    assert 3 * good >= pairs, (family, good, pairs)


@pytest.mark.parametrize("family", SKIPPING)
def test_the_slab_walk_skips(family):
    skipped = 0
    for rng, g, mm, isos in draws(family):
        p, o = slab_of(rng, g)
        skipped += int(slab_skip_np(p, g["vol"], mm, o)["counts"][:, 2].sum())
    assert skipped > 0, family

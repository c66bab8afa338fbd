"""The exactness argument of max-map skipping (DESIGN.md §5.9 point 2, §5.10) without a GPU: the skip walk restated in numpy
(max_map_skip_np) over many geometries gives the dense restatement's result exactly, and every sample it skips is at most the byte of the
cell it was skipped by.  The geometry families (draw_geometry) are shared with tests/test_gpu_max_map_sweep.py: volume shapes with axes 1
and 2 voxels thick, map extents chosen per axis (block 1, blocks 2-9, one cell per axis, cells past the volume), six kinds of content,
anisotropic and rotated voxel grids, cameras outside, inside behind the clipping plane and exactly axis-parallel, sampling factors that put
many samples or less than one into a cell, and bounds on, and one float either side of, the bytes of the map."""
import numpy as np
import pytest

from oracle import vkv_oracle as O
from tests.test_iso_cpu import iso_walk_dense
from tests.test_mip_cpu import INV255, max_map_np, max_map_skip_np, mip_walk_dense, params_np, rays_np, samples_np

F = np.float32
FAMILIES = ("random", "synth", "bright_voxels", "plateau", "all_255", "all_0")
SAMPLING = (0.3, 0.5, 1.0, 2.3, 4.0)


def _axis(rng, lo=1, hi=64):
    r = rng.random()
    if r < 0.15:
        return 1
    if r < 0.3:
        return 2
    x = int(rng.integers(max(lo, 3), hi + 1))
    return min(x | 1, hi) if rng.random() < 0.6 else x  # mostly odd widths


def _map_axis(rng, e):
    """a map extent for an axis of e voxels: block 1, blocks 2-9, one cell (the whole axis), or any count (cells past the volume)"""
    r = rng.random()
    if r < 0.15:
        return e
    if r < 0.55:
        return -(-e // int(rng.integers(2, 10)))
    if r < 0.7:
        return 1
    return int(rng.integers(1, e + 1))


def bound_candidates(mm):
    """threshold / iso values: B * kInv255 for the bytes B of the map, their float neighbours, 0, 1 and 1.01"""
    vals = [F(0), F(1), F(1.01)]
    for b in np.unique(mm):
        x = F(b) * INV255
        vals += [x, np.nextafter(x, F(-1)), np.nextafter(x, F(2))]
    return vals


def place_bright_voxels(rng, vol, shape, blocks):
    """1 .. 11 bright voxels (100 .. 255) written into vol (d, h, w): on the faces, edges and corners of cells of `blocks` voxels, at their
    centres, and one voxel outside a cell's own box (clamped to the volume)"""
    for _ in range(int(rng.integers(1, 12))):
        c = [int(rng.integers(0, -(-e // b))) for e, b in zip(shape, blocks)]
        pos = []
        for ci, b, e in zip(c, blocks, shape):
            lo = ci * b
            pos.append(min(max(int(rng.choice([lo, lo + b - 1, lo - 1, lo + b, lo + b // 2])), 0), e - 1))
        vol[pos[2], pos[1], pos[0]] = int(rng.integers(100, 256))


def draw_geometry(rng, family, max_extent=64):
    """one draw of the sweep: dict shape (w, h, d), vol (d, h, w) uint8, map_extent (w, h, d), voxel_size, axis_angle, camera (azimuth,
    elevation, radius, clip), axis_parallel, sampling_factor, and plateau (the plateau's byte, or None)"""
    axis_parallel = rng.random() < 0.2
    if rng.random() < 0.05:
        shape = (1, 1, 1)
    else:
        shape = tuple(_axis(rng, hi=max_extent) for _ in range(3))
    w, h, d = shape
    me = tuple(_map_axis(rng, e) for e in shape)
    bx, by, bz = (-(-e // m) for e, m in zip(shape, me))
    plateau = None
    if family == "random":
        vol = rng.integers(0, 256, (d, h, w), dtype=np.uint8)
        if rng.random() < 0.5:
            vol[vol < 200] //= 4  # a few bright voxels in dim ones
    elif family == "synth":
        vol = O.synth_volume(shape, int(rng.integers(0, 2)), int(rng.integers(1, 1 << 30)))
    elif family == "bright_voxels":
        # a dim background, bright voxels on the faces, edges and corners of cells and one voxel outside a cell's own box
        vol = rng.integers(0, 24, (d, h, w), dtype=np.uint8)
        place_bright_voxels(rng, vol, shape, (bx, by, bz))
    elif family == "plateau":
        plateau = int(rng.integers(1, 255))
        vol = rng.integers(0, plateau, (d, h, w), dtype=np.uint8) // 2
        x0, y0, z0 = (int(rng.integers(0, e)) for e in shape)
        vol[z0:z0 + int(rng.integers(1, d + 1)), y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = plateau
    elif family == "all_255":
        vol = np.full((d, h, w), 255, np.uint8)
    elif family == "all_0":
        vol = np.zeros((d, h, w), np.uint8)
    else:
        raise ValueError(family)
    if axis_parallel:
        voxel, aa = (1.0, 1.0, 1.0), (1.0, 0.0, 0.0, 0.0)
        cam = (float(rng.choice([0.0, 90.0, 180.0, 270.0])), 0.0, 150.0, 50.0)
    else:
        voxel = (1.0, 1.0, 1.0) if rng.random() < 0.4 else tuple(float(x) for x in rng.uniform(0.4, 2.5, 3))
        aa = (1.0, 0.0, 0.0, 0.0) if rng.random() < 0.4 else tuple(float(x) for x in rng.standard_normal(3)) + (float(rng.uniform(-180, 180)),)
        if rng.random() < 0.3:  # inside the volume: the clipping plane starts the rays
            cam = (float(rng.uniform(0, 360)), float(rng.uniform(-40, 40)), float(rng.uniform(8.0, 20.0)), 1.0)
        else:
            cam = (float(rng.uniform(0, 360)), float(rng.uniform(-60, 60)), 150.0, 50.0)
    sf = float(rng.choice(SAMPLING))
    if max(shape) * sf < 4:  # (a ray needs two samples to be marched)
        sf = 4.0
    return dict(shape=shape, vol=vol, map_extent=me, voxel_size=voxel, axis_angle=aa, camera=cam, axis_parallel=axis_parallel,
                sampling_factor=sf, plateau=plateau)


def draw_bounds(rng, g, mm, count=2):
    """`count` random candidates, the plateau's byte for that family, and the largest byte of the map (a tie with every cell's bound)"""
    cand = bound_candidates(mm)
    vals = [cand[int(rng.integers(0, len(cand)))] for _ in range(count)]
    if g["plateau"] is not None:
        vals[0] = F(g["plateau"]) * INV255
    return vals + [F(int(mm.max())) * INV255]


def check_walks(p, vol, mm, thresholds, isos, in_depth=None):
    """the skip walks of both renderers against the dense restatement on the rays of p; the totals of skipped samples (MIP, iso)"""
    R = rays_np(p, in_depth)
    S = samples_np(vol, R)
    n = R["n_steps"]
    skipped = [0, 0]
    for strict, bounds in ((False, thresholds), (True, isos)):
        for b in bounds:
            w = max_map_skip_np(p, vol, mm, b, strict, R, S)
            if strict:
                k = iso_walk_dense(S["v"], n, b)
                assert np.array_equal(w["k"], k), ("iso", b)
                assert np.array_equal(w["n_filt"] + w["n_skip"], np.where(k >= 0, k + 1, n)), ("iso", b)
            else:
                best, k = mip_walk_dense(S["v"], n, b)
                assert np.array_equal(w["k"], k), ("mip", b)
                assert np.array_equal(w["best"].view(np.uint32), best.view(np.uint32)), ("mip", b)
                assert np.array_equal(w["n_filt"] + w["n_skip"], n), ("mip", b)
            sk = w["skipped"]
            assert np.all(S["v"][sk] <= w["skip_top"][sk]), ("a skipped sample exceeds its cell's byte", strict, b)
            assert np.all(S["live"][sk])
            skipped[int(strict)] += int(sk.sum())
    return skipped


@pytest.mark.parametrize("family", FAMILIES)
def test_skip_walk_equals_dense_over_geometries(family):
    rng = np.random.default_rng(FAMILIES.index(family) * 1000 + 77)
    totals = [0, 0]
    marched = 0
    for case in range(40):
        g = draw_geometry(rng, family, max_extent=24)
        size = (21, 15) if g["axis_parallel"] else (20, 16)
        az, el, radius, clip = g["camera"]
        p = params_np(g["shape"], image_size=size, azimuth=az, elevation=el, radius=radius, sampling_factor=g["sampling_factor"],
                      map_extent=g["map_extent"], voxel_size=g["voxel_size"], axis_angle=g["axis_angle"], clip=clip)
        mm = max_map_np(g["vol"], g["map_extent"])
        marched += int(rays_np(p)["marched"].sum())
        s = check_walks(p, g["vol"], mm, draw_bounds(rng, g, mm), draw_bounds(rng, g, mm))
        totals = [a + b for a, b in zip(totals, s)]
    assert marched > 1000
    assert totals[0] > 0 and totals[1] > 0, totals

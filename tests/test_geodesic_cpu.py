"""The definition of vkv_geodesic_propagate (include/vkvolume_amd.h) restated in numpy, and held to itself.  Three
statements: geodesic_np() is a heap Dijkstra on 64-bit keys (cost << 32 | label) with the cap applied during the search;
geodesic_sweeps_np() relaxes the whole box along the 26 shifted arrays until nothing changes (the reference of the larger GPU shapes);
geodesic_brute_np() is the definition itself: one scipy.sparse.csgraph.dijkstra(min_only=True) per distinct label in float64 (exact below
2^53), the least cost, the smallest label that attains it, and the cap applied AT THE END, so the prefix argument ("a path's prefix under
the limit is under the limit") is tested, not assumed.  geodesic_rounds_np() is the kernels' scheme: tiles, dirty flags, tiles in shuffled
order, halos taken at random from the start-of-round snapshot or from the live array, Jacobi sweeps with the tile's voxel count as their
bound.  Then contents BUILT FOR TIES, which are asserted to tie from the brute statement, the scenes whose point is shown from scipy and
numpy alone (a fragment across a gap, a diagonal staircase), chamfer_steps(), the entry points declared, exported and bound, the calls the
Volume methods issue, and the listing of geodesic.hip.  No device is touched."""
import ctypes as C
import heapq
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_binding_cpu import HANDLE, Recorder, context
from tests.test_distance_cpu import ball_structure, inside_np, random_mask_volume
from tests.test_nearest_cpu import bridge_scene, split_bodies_np, weighted_ball_structure
from vkvolume_amd import abi, geodesic, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xffffffff
NONE64 = np.uint64(0xffffffffffffffff)
U32 = np.uint64(32)
CHAMFER, STEPS_6, STEPS_26 = (3, 3, 4, 3, 4, 4, 5), (1, 1, 0, 1, 0, 0, 0), (1, 1, 1, 1, 1, 1, 1)
SPACING_STEPS = geodesic.chamfer_steps((0.5, 0.5, 1.25))[0]        # (3, 3, 4, 8, 8, 8, 9)
BIG_STEPS = (65535, 7, 65535, 1, 65535, 9, 65535)
TABLES = (CHAMFER, STEPS_6, STEPS_26, SPACING_STEPS, BIG_STEPS)
OFFSETS = [(dz, dy, dx, abs(dx) + 2 * abs(dy) + 4 * abs(dz)) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def crop(a, box):
    if box is None:
        return a
    x0, y0, z0, w, h, d = box
    return a[z0:z0 + d, y0:y0 + h, x0:x0 + w]


def seed_keys(vol_dhw, iso, seeds, box=None):
    """(inside [d, h, w] of the box, keys [d, h, w] uint64): label (cost 0) on inside voxels with a non-zero seed value, NONE64 elsewhere;
    `seeds` has the box's shape"""
    inside = inside_np(vol_dhw, iso, box)
    seeds = np.asarray(seeds).astype(np.uint32)
    assert seeds.shape == inside.shape
    return inside, np.where(inside & (seeds != 0), seeds.astype(np.uint64), NONE64)


def split_keys(keys):
    """(d_dist, d_labels) of a key array"""
    return (keys >> U32).astype(np.uint32), np.where(keys == NONE64, 0, keys & np.uint64(NONE)).astype(np.uint32)


# ---- heap Dijkstra on 64-bit keys ---------------------------------------------------------------------------------------------------------
def geodesic_np(vol_dhw, iso, seeds, steps, limit=None, box=None):
    """(d_dist, d_labels): Dijkstra over the keys cost << 32 | label as Python integers; a move is taken only where the new cost is below
    the limit"""
    limit = NONE if limit is None else int(limit)
    inside, keys = seed_keys(vol_dhw, iso, seeds, box)
    d, h, w = inside.shape
    best = {}
    heap = [(int(k), int(i)) for i, k in enumerate(keys.ravel()) if k != NONE64]
    for k, i in heap:
        best[i] = k
    heapq.heapify(heap)
    ins = inside.ravel()
    while heap:
        k, i = heapq.heappop(heap)
        if best[i] != k:
            continue
        z, y, x = i // (h * w), i // w % h, i % w
        for dz, dy, dx, m in OFFSETS:
            c = steps[m - 1]
            zz, yy, xx = z + dz, y + dy, x + dx
            if c == 0 or not (0 <= zz < d and 0 <= yy < h and 0 <= xx < w):
                continue
            j = (zz * h + yy) * w + xx
            if not ins[j] or (k >> 32) + c >= limit:
                continue
            cand = k + (c << 32)
            if cand < best.get(j, 1 << 64):
                best[j] = cand
                heapq.heappush(heap, (cand, j))
    out = np.full(d * h * w, NONE64, np.uint64)
    for i, k in best.items():
        out[i] = k
    return split_keys(out.reshape(d, h, w))


# ---- whole-box sweeps -------------------------------------------------------------------------------------------------------------------
def relax_np(padded, inside, steps, limit, in_place):
    """one sweep over the interior of `padded` (uint64, one entry of NONE64 around it): every inside voxel takes the minimum of its key and
    of key(u) + (c << 32) over the moves u -> v whose new cost is below the limit.  in_place False: Jacobi, every move reads the keys
    from before the sweep (the kernel's sweep); True: each of the 26 directions reads what the directions before it wrote (fewer sweeps)"""
    limit = np.uint64(limit)
    d, h, w = inside.shape
    src = padded if in_place else padded.copy()
    core = padded[1:-1, 1:-1, 1:-1]
    for dz, dy, dx, m in OFFSETS:
        c = int(steps[m - 1])
        if c == 0:
            continue
        nb = src[1 - dz:1 - dz + d, 1 - dy:1 - dy + h, 1 - dx:1 - dx + w]        # the key of u = v - offset
        ok = inside & ((nb >> U32) + np.uint64(c) < limit)        # at most 2^32 + 65534: no wrap; NONE64 never passes
        cand = np.where(ok, nb + np.uint64(c << 32), NONE64)
        np.minimum(core, cand, out=core)
    return padded


def geodesic_sweeps_np(vol_dhw, iso, seeds, steps, limit=None, box=None, sweeps=False):
    """(d_dist, d_labels) by whole-box min-plus sweeps over the 26 shifted uint64 arrays until a sweep changes nothing"""
    limit = NONE if limit is None else int(limit)
    inside, keys = seed_keys(vol_dhw, iso, seeds, box)
    padded = np.full(tuple(s + 2 for s in inside.shape), NONE64, np.uint64)
    padded[1:-1, 1:-1, 1:-1] = keys
    count = 0
    while True:
        before = padded.copy()
        relax_np(padded, inside, steps, limit, in_place=True)
        count += 1
        if np.array_equal(before, padded):
            break
    out = split_keys(padded[1:-1, 1:-1, 1:-1].copy())
    return out + (count,) if sweeps else out


# ---- the definition -------------------------------------------------------------------------------------------------------------------------
def geodesic_brute_np(vol_dhw, iso, seeds, steps, limit=None, box=None, ties=False):
    """(d_dist, d_labels) of the header's sentences: per distinct label the least path cost from its seeds to every voxel (scipy's Dijkstra
    on the graph of moves, float64: exact), then the least cost over the labels, the smallest label that attains it, and at the END the
    cap.  ties=True: also the number of reached voxels at which more than one label attains the least cost"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    limit = NONE if limit is None else int(limit)
    inside, keys = seed_keys(vol_dhw, iso, seeds, box)
    d, h, w = inside.shape
    n = d * h * w
    index = np.arange(n).reshape(d, h, w)
    rows, cols, costs = [], [], []
    for dz, dy, dx, m in OFFSETS:
        c = steps[m - 1]
        if c == 0:
            continue
        a = (slice(max(0, -dz), d - max(0, dz)), slice(max(0, -dy), h - max(0, dy)), slice(max(0, -dx), w - max(0, dx)))        # u
        b = (slice(max(0, dz), d - max(0, -dz)), slice(max(0, dy), h - max(0, -dy)), slice(max(0, dx), w - max(0, -dx)))        # v = u + offset
        both = inside[a] & inside[b]
        rows.append(index[a][both]), cols.append(index[b][both]), costs.append(np.full(int(both.sum()), float(c)))
    graph = csr_matrix((np.concatenate(costs), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)) if rows else csr_matrix((n, n))
    flat = keys.ravel()
    labels = sorted(set(int(k) for k in flat[flat != NONE64]))
    least = np.full(n, np.inf)
    winner = np.zeros(n, np.uint32)
    attained = np.zeros(n, np.int64)
    for label in labels:        # increasing: a later label takes a voxel only where it is strictly cheaper
        cost = dijkstra(graph, directed=True, indices=np.flatnonzero(flat == np.uint64(label)), min_only=True)
        attained = np.where(cost < least, 1, attained + ((cost == least) & np.isfinite(cost)))
        winner = np.where(cost < least, np.uint32(label), winner)
        least = np.minimum(least, cost)
    reached = least < limit
    dist = np.where(reached, least, NONE).astype(np.uint32).reshape(d, h, w)
    out = dist, np.where(reached, winner, 0).astype(np.uint32).reshape(d, h, w)
    return out + (int((reached & (attained > 1)).sum()),) if ties else out


# ---- the kernels' scheme --------------------------------------------------------------------------------------------------------------------
def geodesic_rounds_np(vol_dhw, iso, seeds, steps, limit=None, box=None, tile=(8, 8, 8), rng=None, bound=None, rounds=None, state=None):
    """(d_dist, d_labels, info): k_geo_init / k_geo_round / k_geo_finish.  tile: (edge z, edge y, edge x); the dirty tiles of a round run in
    shuffled order, each loading its own keys and, entry by entry at random, its halo from the round's start or from the live array (what a
    racing load can return), sweeping (Jacobi) until nothing changes or `bound` sweeps (None: the tile's voxels) are done, storing its
    changed keys and marking the tiles that hold one of them in their halo, itself where the bound was hit.  rounds None: until no tile is
    dirty.  info: rounds run, the most sweeps of any tile, the tiles that hit the bound, whether the state is the fixed point, the state"""
    rng = np.random.default_rng(0) if rng is None else rng
    limit = NONE if limit is None else int(limit)
    inside, keys = seed_keys(vol_dhw, iso, seeds if state is None else np.zeros(inside_np(vol_dhw, iso, box).shape, np.uint32), box)
    shape = np.array(inside.shape)
    edge = np.array(tile)
    grid = tuple(int(g) for g in -(-shape // edge))
    bound = int(edge.prod()) if bound is None else bound
    if state is None:
        dirty = np.ones(grid, bool)
    else:
        keys, dirty = state[0].copy(), state[1].copy()
    pad_in = np.zeros(tuple(shape + 2), bool)
    pad_in[1:-1, 1:-1, 1:-1] = inside
    done, most, hits = 0, 0, 0
    while dirty.any() and (rounds is None or done < rounds):
        padded = np.full(tuple(shape + 2), NONE64, np.uint64)        # the live array, with nothing beyond the box
        padded[1:-1, 1:-1, 1:-1] = keys
        snapshot = padded.copy()
        nxt = np.zeros(grid, bool)
        todo = np.argwhere(dirty)
        rng.shuffle(todo)
        for t in todo:
            lo = t * edge
            hi = np.minimum(lo + edge, shape)
            halo = tuple(slice(int(a), int(b) + 2) for a, b in zip(lo, hi))        # in padded coordinates: the tile and one entry around it
            local = np.where(rng.random(tuple(int(b - a) + 2 for a, b in zip(lo, hi))) < 0.5, padded[halo], snapshot[halo])
            own = tuple(slice(int(a) + 1, int(b) + 1) for a, b in zip(lo, hi))
            local[1:-1, 1:-1, 1:-1] = padded[own]        # only this tile writes them
            first = local[1:-1, 1:-1, 1:-1].copy()
            tile_in = pad_in[own]
            hit = True
            for sweep in range(bound):
                before = local[1:-1, 1:-1, 1:-1].copy()
                relax_np(local, tile_in, steps, limit, in_place=False)
                most = max(most, sweep + 1)
                if np.array_equal(before, local[1:-1, 1:-1, 1:-1]):
                    hit = False
                    break
            changed = local[1:-1, 1:-1, 1:-1] != first
            padded[own] = local[1:-1, 1:-1, 1:-1]
            for s in itertools.product((-1, 0, 1), repeat=3):        # the tiles that hold a changed voxel in their halo
                face = tuple(slice(None) if k == 0 else (slice(0, 1) if k < 0 else slice(int(e) - 1, int(e))) for k, e in zip(s, edge))
                u = t + s
                if any(s) and (u >= 0).all() and (u < grid).all() and changed[face].any():
                    nxt[tuple(u)] = True
            if hit:
                hits += 1
                nxt[tuple(t)] = True
        keys = padded[1:-1, 1:-1, 1:-1].copy()
        dirty = nxt
        done += 1
    info = {"rounds": done, "most sweeps": most, "bound hits": hits, "converged": not dirty.any(), "state": (keys, dirty)}
    return split_keys(keys) + (info,)


# ---- contents ---------------------------------------------------------------------------------------------------------------------------------
def random_case(rng, case):
    """(vol, seeds, steps, limit) of a seeded small box: axes 1 .. 9, a mask of one of four densities, one to four labels on a few voxels"""
    shape = tuple(int(s) for s in rng.integers(1, 10, size=3))
    if case % 7 == 0:
        shape = tuple(1 if rng.random() < 0.5 else s for s in shape)
    vol = random_mask_volume(rng, shape, (0.35, 0.6, 0.9, 1.0)[(case // 3) % 4])
    labels = rng.integers(1, 5)
    seeds = np.where(rng.random(shape) < (0.02, 0.1, 0.3)[case % 3], rng.integers(1, labels + 1, size=shape), 0).astype(np.uint32)
    if case % 11 == 0:
        seeds[seeds == 1] = NONE        # the largest label
    steps = TABLES[case % len(TABLES)]
    limit = (None, min(c for c in steps if c), int(rng.integers(2, 40)))[(case // 5) % 3]
    return vol, seeds, steps, limit


def mirrored_seeds(shape, axis, first_small):
    """a full mask and two seeds mirrored about the middle plane of `axis` (odd), labels 5 and 9: which of them comes first in memory is
    `first_small`"""
    vol = np.full(shape, 200, np.uint8)
    seeds = np.zeros(shape, np.uint32)
    a, b = [s // 2 for s in shape], [s // 2 for s in shape]
    a[axis], b[axis] = 0, shape[axis] - 1
    seeds[tuple(a)], seeds[tuple(b)] = (5, 9) if first_small else (9, 5)
    return vol, seeds


def checkerboard_seeds(shape, seed=0):
    rng = np.random.default_rng(seed)
    vol = np.full(shape, 200, np.uint8)
    z, y, x = np.indices(shape)
    seeds = np.where((x + y + z) % 2 == 0, rng.integers(1, 6, size=shape), 0).astype(np.uint32)
    return vol, seeds


def extreme_labels(shape):
    """label 0xffffffff at the first voxel against label 1 at the last, in a full mask"""
    vol = np.full(shape, 200, np.uint8)
    seeds = np.zeros(shape, np.uint32)
    seeds.flat[0], seeds.flat[-1] = NONE, 1
    return vol, seeds


def staircase(n, anti=False):
    """the voxels (i, i, i) of an n^3 box (anti: (n - 1 - i, i, i) in x): connected by xyz moves only; the seed, label 7, at i = 0"""
    vol = np.full((n, n, n), 17, np.uint8)
    seeds = np.zeros((n, n, n), np.uint32)
    i = np.arange(n)
    vol[i, i, n - 1 - i if anti else i] = 200
    seeds[0, 0, n - 1 if anti else 0] = 7
    return vol, seeds


def serpentine(w=40, h=40, d=3):
    """a path that runs along x, steps one row up at the end and runs back, rows 0, 2, 4, ... of the middle slice: w h / 2 + h / 2 voxels long"""
    vol = np.full((d, h, w), 17, np.uint8)
    for y in range(0, h, 2):
        vol[d // 2, y, :] = 200
        if y + 1 < h:
            vol[d // 2, y + 1, w - 1 if (y // 2) % 2 == 0 else 0] = 200
    seeds = np.zeros((d, h, w), np.uint32)
    seeds[d // 2, 0, 0] = 3
    return vol, seeds


def gap_scene():
    """bridge_scene() of tests/test_nearest_cpu.py and a detached ball of radius 1 (thinner than the erosion by radius 2) centred at x = 1:
    the voxel x = 3 between it and the left body (which starts at x = 4) is outside"""
    vol, bridge = bridge_scene()
    z, y, x = np.indices(vol.shape)
    ball = (x - 1) ** 2 + (y - 10) ** 2 + (z - 10) ** 2 <= 1
    assert not (ball & (vol >= 128)).any()
    return np.where(ball, 200, vol).astype(np.uint8), bridge, ball


def split_bodies_geodesic_np(vol, iso, r2, connectivity=6, weights=None):
    """Volume.split_bodies(metric="geodesic") with scipy.ndimage: the erosion and the cores of split_bodies_np, then the cores' labels
    propagated through the original inside voxels with chamfer_steps(weights), unlimited: (labels, K)"""
    from scipy import ndimage
    inside = inside_np(vol, iso)
    eroded = ndimage.binary_erosion(inside, structure=weighted_ball_structure(r2, weights), border_value=1)
    core, k = ndimage.label(eroded, structure=ndimage.generate_binary_structure(3, {6: 1, 26: 3}[connectivity]))
    return geodesic_sweeps_np(vol, iso, core.astype(np.uint32), geodesic.chamfer_steps(weights)[0])[1], k


# ---- the statements against one another -----------------------------------------------------------------------------------------------------
def check_statements(vol, seeds, steps, limit, what, rounds_rng=None, tile=(8, 8, 8)):
    want_d, want_l, ties = geodesic_brute_np(vol, 0.5, seeds, steps, limit, ties=True)
    for f in (geodesic_np, geodesic_sweeps_np):
        got_d, got_l = f(vol, 0.5, seeds, steps, limit)
        assert got_d.dtype == np.uint32 and got_l.dtype == np.uint32
        assert np.array_equal(got_d, want_d), (f.__name__, what, np.argwhere(got_d != want_d)[:4].tolist())
        assert np.array_equal(got_l, want_l), (f.__name__, what, np.argwhere(got_l != want_l)[:4].tolist())
    if rounds_rng is not None:
        got_d, got_l, info = geodesic_rounds_np(vol, 0.5, seeds, steps, limit, tile=tile, rng=rounds_rng)
        assert np.array_equal(got_d, want_d) and np.array_equal(got_l, want_l), ("rounds", what, tile)
        assert info["converged"] and info["bound hits"] == 0 and info["most sweeps"] <= int(np.prod(tile)), (what, info["most sweeps"])
    inside = vol >= 128
    assert (want_d[~inside] == NONE).all() and (want_l[~inside] == 0).all() and ((want_d == NONE) == (want_l == 0)).all(), what
    assert (want_d[want_d != NONE] < (NONE if limit is None else limit)).all(), what
    return ties


def test_the_three_statements_agree_on_random_boxes():
    """axes 1 .. 9, the five step tables, limits none / the least step / 2 .. 39, four densities, one to four labels, label 0xffffffff; the
    kernels' scheme with 8 x 8 x 8 tiles on every fourth case and with 2 x 3 x 4 tiles on every fourth"""
    rng = np.random.default_rng(520)
    tied = reached = 0
    for case in range(600):
        vol, seeds, steps, limit = random_case(rng, case)
        tile = None if case % 2 else ((8, 8, 8), (2, 3, 4))[case // 2 % 2]
        tied += check_statements(vol, seeds, steps, limit, (case, vol.shape, steps, limit), rounds_rng=rng if tile else None, tile=tile or (8, 8, 8))
        reached += int((geodesic_sweeps_np(vol, 0.5, seeds, steps, limit)[1] != 0).sum())
    assert tied > 500 and reached > 20000


def test_the_cap_applied_at_the_end_is_the_cap_applied_on_the_way():
    """the prefix argument on its own: at every limit the capped search equals the unlimited result cut at the limit"""
    rng = np.random.default_rng(7)
    for case in range(60):
        vol, seeds, steps, _ = random_case(rng, case)
        full_d, full_l = geodesic_np(vol, 0.5, seeds, steps)
        for limit in (1, 2, 5, 11, 40, 65535, 70000):
            d, lab = geodesic_np(vol, 0.5, seeds, steps, limit)
            keep = full_d < limit
            assert np.array_equal(d, np.where(keep, full_d, NONE)) and np.array_equal(lab, np.where(keep, full_l, 0)), (case, limit)


# ---- the kernels' scheme ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [(8, 8, 8), (4, 4, 4), (1, 2, 3)], ids=lambda t: "%dx%dx%d" % t)
def test_rounds_with_shuffled_tiles_and_stale_halos_equal_dijkstra(tile):
    rng = np.random.default_rng(99 + tile[0])
    for case in range(24):
        shape = tuple(int(s) for s in rng.integers(1, 21 if min(tile) >= 4 else 9, size=3))        # small tiles: many of them
        vol = random_mask_volume(rng, shape, (0.35, 0.6, 0.9)[case % 3])
        seeds = np.where(rng.random(shape) < 0.01, rng.integers(1, 4, size=shape), 0).astype(np.uint32)
        seeds.flat[int(rng.integers(0, seeds.size))] = 2
        steps, limit = TABLES[case % len(TABLES)], (None, 30, 100000)[case % 3]
        want = geodesic_np(vol, 0.5, seeds, steps, limit)
        for repeat in range(2):        # another order, other halos: the same fixed point
            got_d, got_l, info = geodesic_rounds_np(vol, 0.5, seeds, steps, limit, tile=tile, rng=rng)
            assert np.array_equal(got_d, want[0]) and np.array_equal(got_l, want[1]), (case, shape, tile)
            assert info["bound hits"] == 0 and info["most sweeps"] <= int(np.prod(tile))


def test_a_tile_that_hits_the_sweep_bound_stays_dirty_and_the_result_is_the_same():
    vol, seeds = serpentine(16, 16, 1)
    want = geodesic_np(vol, 0.5, seeds, STEPS_6)
    got_d, got_l, info = geodesic_rounds_np(vol, 0.5, seeds, STEPS_6, bound=5)        # far fewer sweeps than the path needs in a tile
    assert info["bound hits"] > 0 and info["converged"] and np.array_equal(got_d, want[0]) and np.array_equal(got_l, want[1])
    assert int(want[0][vol >= 128].max()) == int((vol >= 128).sum()) - 1 == 16 * 8 + 8 - 1        # one path: 8 rows of 16 and 8 connecting voxels


def test_rounds_resume_from_the_state_and_report_convergence_only_at_the_fixed_point():
    vol = np.full((1, 1, 200), 200, np.uint8)
    seeds = np.zeros((1, 1, 200), np.uint32)
    seeds[0, 0, 0] = 4
    want = geodesic_np(vol, 0.5, seeds, CHAMFER)
    state, calls, early = None, 0, 0
    while True:
        d, lab, info = geodesic_rounds_np(vol, 0.5, seeds, CHAMFER, rounds=1, state=state)
        state, calls = info["state"], calls + 1
        if info["converged"]:
            break
        early += 1
        assert (d >= want[0]).all()        # upper bounds on the way
    assert early >= 24 and calls <= 27 and np.array_equal(d, want[0]) and np.array_equal(lab, want[1])        # 25 tiles along x
    assert int(want[0][0, 0, 199]) == 3 * 199


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["z", "y", "x"])
def test_the_plane_between_mirrored_seeds_takes_the_smaller_label_whichever_comes_first(axis):
    shape = [5, 7, 9]
    shape[axis] = (9, 7, 11)[axis]
    for first_small in (True, False):
        vol, seeds = mirrored_seeds(tuple(shape), axis, first_small)
        for steps in TABLES:
            ties = check_statements(vol, seeds, steps, None, ("mirrored", axis, first_small, steps), rounds_rng=np.random.default_rng(1), tile=(4, 4, 4))
            assert ties >= shape[(axis + 1) % 3] * shape[(axis + 2) % 3]        # the whole middle plane ties ...
            labels = geodesic_np(vol, 0.5, seeds, steps)[1]
            plane = labels[tuple(shape[axis] // 2 if a == axis else slice(None) for a in range(3))]
            assert (plane == 5).all(), (axis, first_small, steps)        # ... and goes to label 5


def test_a_checkerboard_of_seeds_and_the_extreme_labels_tie_and_resolve_to_the_smallest():
    for k, shape in enumerate([(5, 7, 9), (3, 3, 3), (1, 7, 5), (1, 1, 9), (8, 8, 8)]):
        vol, seeds = checkerboard_seeds(shape, seed=k)
        for steps in TABLES:
            assert check_statements(vol, seeds, steps, None, ("checkerboard", shape, steps), rounds_rng=np.random.default_rng(k), tile=(2, 3, 4)) > 0
    for shape in [(1, 1, 9), (3, 5, 7), (9, 9, 9)]:
        vol, seeds = extreme_labels(shape)
        for steps in (CHAMFER, STEPS_26):
            assert check_statements(vol, seeds, steps, None, ("extreme", shape, steps), rounds_rng=np.random.default_rng(3)) > 0
            d, lab = geodesic_np(vol, 0.5, seeds, steps)
            assert set(np.unique(lab).tolist()) == {1, NONE} and int(lab.flat[0]) == NONE and int(d.flat[0]) == 0
            middle = tuple(s // 2 for s in shape)
            assert int(lab[middle]) == 1        # equally far from both: the smaller label


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_fragment_across_a_gap_is_labelled_by_the_euclidean_split_and_not_by_the_geodesic_one():
    from scipy import ndimage
    vol, bridge, ball = gap_scene()
    inside = vol >= 128
    assert ndimage.label(inside, structure=np.ones((3, 3, 3)))[1] == 2 and ball.sum() == 7        # the bodies with their bridge, and the fragment
    eroded = ndimage.binary_erosion(inside, structure=ball_structure(4), border_value=1)
    assert not (eroded & ball).any() and ndimage.label(eroded)[1] == 2        # the fragment vanished whole; two cores
    euclid, k = split_bodies_np(vol, 0.5, 4)
    geo, kg = split_bodies_geodesic_np(vol, 0.5, 4)
    assert k == kg == 2
    assert (euclid[ball] == 1).all() and (geo[ball] == 0).all()        # the nearest core across the gap, against no core at all
    core = ndimage.label(eroded)[0]
    assert np.array_equal(euclid[eroded], core[eroded]) and np.array_equal(geo[eroded], core[eroded])        # they agree on both cores
    differ = euclid != geo
    assert differ.any() and differ[ball].all()
    assert np.array_equal(geo != 0, inside & ~ball) and set(geo[bridge].tolist()) == {1, 2}        # everything connected to a core is labelled
    sizes = ndimage.sum_labels(np.ones_like(geo), geo, index=[1, 2])
    assert sizes[0] + sizes[1] == inside.sum() - ball.sum() and sizes[0] == sizes[1]        # the scene is symmetric about x = 19.5
    assert np.array_equal(geo, geodesic_np(vol, 0.5, core.astype(np.uint32), CHAMFER)[1])


def test_a_diagonal_staircase_is_connected_under_the_chamfer_and_unreachable_under_six_steps():
    for anti in (False, True):
        vol, seeds = staircase(9, anti)
        i = np.arange(9)
        on = (i, i, 8 - i if anti else i)
        d, lab = geodesic_np(vol, 0.5, seeds, CHAMFER)
        assert np.array_equal(d[on], 5 * i) and (lab[on] == 7).all() and int((lab != 0).sum()) == 9
        d, lab = geodesic_np(vol, 0.5, seeds, STEPS_6)
        assert int((lab != 0).sum()) == 1 and int(d[on][0]) == 0 and (d[on][1:] == NONE).all()
        d, lab = geodesic_np(vol, 0.5, seeds, (0, 0, 0, 0, 0, 0, 2), limit=9)        # the xyz class alone, and a limit: costs 0 2 4 6 8
        assert np.array_equal(d[on], np.where(2 * i < 9, 2 * i, NONE))
        for steps in (CHAMFER, STEPS_6):
            check_statements(vol, seeds, steps, None, ("staircase", anti, steps), rounds_rng=np.random.default_rng(5), tile=(4, 4, 4))


def test_seeds_on_outside_voxels_no_seed_and_a_box():
    rng = np.random.default_rng(11)
    vol = random_mask_volume(rng, (6, 7, 8), 0.7)
    seeds = np.where(vol < 128, 9, 0).astype(np.uint32)        # on outside voxels only
    for f in (geodesic_np, geodesic_sweeps_np, geodesic_brute_np):
        d, lab = f(vol, 0.5, seeds, CHAMFER)
        assert (d == NONE).all() and (lab == 0).all()
        d, lab = f(vol, 0.5, np.zeros_like(seeds), CHAMFER)
        assert (d == NONE).all() and (lab == 0).all()
    box = (1, 2, 1, 6, 4, 4)
    everywhere = np.full(vol.shape, 200, np.uint8)        # the box's surroundings are inside: they do not exist
    everywhere[2:4, 3:5, 3:5] = 17
    seeds = np.zeros((4, 4, 6), np.uint32)
    seeds[0, 0, 0] = 3
    cropped = np.ascontiguousarray(crop(everywhere, box))
    for f in (geodesic_np, geodesic_sweeps_np, geodesic_brute_np):
        got = f(everywhere, 0.5, seeds, CHAMFER, box=box)
        want = f(cropped, 0.5, seeds, CHAMFER)
        assert got[0].shape == (4, 4, 6) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- chamfer_steps --------------------------------------------------------------------------------------------------------------------------------
def test_chamfer_steps():
    assert geodesic.chamfer_steps() == ((3, 3, 4, 3, 4, 4, 5), 1.0 / 3.0)
    assert geodesic.chamfer_steps((1, 1, 1)) == ((3, 3, 4, 3, 4, 4, 5), 1.0 / 3.0) and geodesic.chamfer_steps((2.0, 2.0, 2.0))[1] == 2.0 / 3.0
    steps, unit = geodesic.chamfer_steps((0.5, 0.5, 1.25))
    want = [int(np.floor(3 * np.sqrt(sum(s * s for a, s in enumerate((0.5, 0.5, 1.25)) if m >> a & 1)) / 0.5 + 0.5)) for m in range(1, 8)]
    assert list(steps) == want == [3, 3, 4, 8, 8, 8, 9] and unit == 0.5 / 3
    assert geodesic.chamfer_steps((2, 2, 5))[0] == steps        # integer weights of the same ratio
    assert geodesic.chamfer_steps((1, 1, 21845))[0][3] == 65535
    for bad in ((1, 1), (1, 1, 0), (1, -1, 1), (1, 1, float("inf")), (1, 1, float("nan")), "xyz", (1, 1, 21846)):
        with pytest.raises(ValueError):
            geodesic.chamfer_steps(bad)
    assert (geodesic.NONE, geodesic.MAX_ROUNDS, geodesic.CHAMFER_345, geodesic.STEPS_6, geodesic.STEPS_26) == (NONE, 1024, CHAMFER, STEPS_6, STEPS_26)


# ---- entry points -------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"#define VKV_GEODESIC_NONE 0xffffffffu", header) and abi.GEODESIC_NONE == 0xffffffff
    assert re.search(r"#define VKV_GEODESIC_MAX_ROUNDS 1024\b", header) and abi.GEODESIC_MAX_ROUNDS == 1024
    assert re.search(r"\bsize_t\s+vkv_geodesic_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_geodesic_propagate\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*float iso,\s*"
                     r"const uint32_t\s*\*d_seeds,\s*const uint32_t steps\[7\],\s*uint32_t limit,\s*uint32_t rounds,\s*int32_t resume,\s*void\s*\*d_scratch,\s*"
                     r"uint32_t\s*\*d_dist,\s*uint32_t\s*\*d_labels,\s*uint64_t\s*\*d_counts,\s*void\s*\*stream\)", header)
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in ("vkv_geodesic_propagate", "vkv_geodesic_scratch_bytes"):
        assert name in lib.EXPORTS and re.search(r"\b%s$" % name, out, flags=re.M)
    at = L.vkv_geodesic_propagate.argtypes
    assert len(at) == 15 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[6] is C.POINTER(C.c_uint32)
    assert at[7] is C.c_uint32 and at[8] is C.c_uint32 and at[9] is C.c_int32 and L.vkv_geodesic_propagate.restype is C.c_int
    assert L.vkv_geodesic_scratch_bytes.restype is C.c_size_t
    assert callable(lib.Context.geodesic_propagate_rc) and not hasattr(lib.Context, "geodesic_propagate")
    assert not hasattr(lib, "geodesic_scratch_bytes") and not hasattr(lib, "chamfer_steps")        # they live in vkvolume_amd/geodesic.py
    buf = (C.c_uint64 * 256)()
    a = C.addressof(buf)
    steps = (C.c_uint32 * 7)(*CHAMFER)
    assert L.vkv_geodesic_propagate(None, a, abi.Extent3D(4, 4, 4), None, 0.5, a + 256, steps, 5, 1, 0, a + 1024, a + 512, a + 768, a + 64, None) == abi.VKV_E_INVALID_ARGUMENT
    assert not any(buf) and list(steps) == list(CHAMFER)


def test_the_scratch_size_is_the_documented_formula():
    for w, h, d in [(1, 1, 1), (8, 8, 8), (9, 8, 8), (17, 9, 10), (70, 66, 65), (70000, 1, 1), (1024, 1024, 795), (65536, 65535, 1)]:
        tiles = -(-w // 8) * -(-h // 8) * -(-d // 8)
        assert geodesic.scratch_bytes(abi.Extent3D(w, h, d)) == 8 * w * h * d + 32 + 8 * tiles, (w, h, d)
    e = abi.Extent3D(40, 50, 60)
    assert geodesic.scratch_bytes(e, abi.Box(3, 4, 5, 17, 9, 10)) == 8 * 17 * 9 * 10 + 32 + 8 * 3 * 2 * 2
    assert geodesic.scratch_bytes(e, abi.Box(3, 4, 5, 38, 9, 10)) == 0 and geodesic.scratch_bytes(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    assert geodesic.scratch_bytes(abi.Extent3D(0, 4, 4)) == 0 and geodesic.scratch_bytes(abi.Extent3D(65536, 65536, 1)) == 0        # 2^32 voxels


def test_the_binding_passes_the_arguments_in_the_headers_order():
    ctx, rec = context()
    e = abi.Extent3D(40, 50, 60)
    assert ctx.geodesic_propagate_rc(10, e, None, 0.5, 11, CHAMFER, None, 64, False, 12, 13, 14, 15, 99) == 0
    assert rec.last("vkv_geodesic_propagate") == (HANDLE, 10, bytes(e), None, 0.5, 11, list(CHAMFER), abi.GEODESIC_NONE, 64, 0, 12, 13, 14, 15, 99)
    b = abi.Box(1, 2, 3, 4, 5, 6)
    ctx.geodesic_propagate_rc(10, e, b, 0.25, None, None, 7, 1024, True, 12, None, 14, 15)
    assert rec.last("vkv_geodesic_propagate") == (HANDLE, 10, bytes(e), bytes(b), 0.25, None, None, 7, 1024, 1, 12, None, 14, 15, 0)
    ctx.geodesic_propagate_rc(10, e, b, 0.25, 11, STEPS_6, 7, 3, 2, 12, 13, None, 15)
    assert rec.last("vkv_geodesic_propagate")[6:10] == ([1, 1, 0, 1, 0, 0, 0], 7, 3, 2)


class CountingRecorder(Recorder):
    """a Recorder whose vkv_geodesic_propagate writes d_counts (host memory here) as the device would: converged from call `after` on"""

    def __init__(self, after):
        super().__init__()
        self.after = after

    def __getattr__(self, name):
        call = super().__getattr__(name)
        if name != "vkv_geodesic_propagate":
            return call

        def propagate(*args):
            rc = call(*args)
            done = len(self.calls[name]) >= self.after
            (C.c_uint64 * 2).from_address(args[13])[:] = [1 if done else 0, 123]
            return rc
        return propagate


@pytest.fixture
def stub_volume(monkeypatch):
    """a Volume of 12 x 5 x 4 host bytes on a context whose library records the calls; geodesic calls converge from the third on"""
    ctx, _ = context()
    ctx._lib = rec = CountingRecorder(3)
    monkeypatch.setattr(V, "_stream", lambda: 99)
    v = V.Volume(ctx, device=torch.device("cpu"))
    v.volume = torch.full((4, 5, 12), 200, dtype=torch.uint8)
    v.extent = abi.Extent3D(12, 5, 4)
    return v, rec


def test_volume_methods_make_the_calls_the_docstrings_name(stub_volume):
    v, rec = stub_volume
    seeds = torch.zeros((4, 5, 12), dtype=torch.int32).view(torch.uint32)
    name = "vkv_geodesic_propagate"
    labels, dist, counts = v.geodesic_propagate(seeds, 0.5, rounds=7)        # exactly one call, whatever counts says
    assert len(rec.calls[name]) == 1 and labels.dtype == dist.dtype == torch.uint32 and tuple(labels.shape) == tuple(dist.shape) == (4, 5, 12)
    call = rec.last(name)
    assert call[1] == v.volume.data_ptr() and call[3] is None and call[4] == 0.5 and call[5] == seeds.data_ptr()
    assert call[6:10] == (list(CHAMFER), abi.GEODESIC_NONE, 7, 0) and call[11:] == (dist.data_ptr(), labels.data_ptr(), counts.data_ptr(), 99)
    assert counts.dtype == torch.int64 and counts.tolist() == [0, 123]
    rec.calls.clear()
    box_seeds = seeds[:2, :2, :3].contiguous()
    labels, dist, counts = v.geodesic_propagate(box_seeds, 0.5, steps=STEPS_6, limit=30, box=((1, 1, 1), (3, 2, 2)), distance=False)        # 64, then resumed 128, 256
    assert dist is None and tuple(labels.shape) == (2, 2, 3) and counts.tolist() == [1, 123]
    calls = rec.calls[name]
    assert [c[8:10] for c in calls] == [(64, 0), (128, 1), (256, 1)] and [c[5] for c in calls] == [box_seeds.data_ptr(), None, None]
    assert all(c[3] == bytes(abi.Box(1, 1, 1, 3, 2, 2)) and c[6:8] == ([1, 1, 0, 1, 0, 0, 0], 30) and c[11] is None and c[10] == calls[0][10] for c in calls)
    rec.after = 9        # 64, 128, 256, 512, then 1024 each
    rec.calls.clear()
    v.geodesic_propagate(seeds, 0.5)
    assert [c[8] for c in rec.calls[name]] == [64, 128, 256, 512, 1024, 1024, 1024, 1024, 1024]
    # grow_from_points: labels i + 1 at (x, y, z), the first of equal points
    rec.after = 1
    rec.calls.clear()
    captured = {}
    original = V.Volume.geodesic_propagate

    def spy(self, seeds, *args, **kw):
        captured["seeds"], captured["kw"] = seeds.clone(), kw
        return original(self, seeds, *args, **kw)
    V.Volume.geodesic_propagate = spy
    try:
        v.grow_from_points([(3, 2, 1), (11, 4, 3), (3, 2, 1)], 0.5, limit=20, rounds=5)
        want = np.zeros((4, 5, 12), np.int32)
        want[1, 2, 3], want[3, 4, 11] = 1, 2
        assert np.array_equal(captured["seeds"].numpy(), want) and captured["kw"]["limit"] == 20 and captured["kw"]["rounds"] == 5
        v.grow_from_points([(3, 2, 1)], 0.5, box=((2, 1, 1), (4, 3, 2)))
        assert tuple(captured["seeds"].shape) == (2, 3, 4) and int(captured["seeds"][0, 1, 1]) == 1 and int(captured["seeds"].sum()) == 1
        for outside in [(12, 0, 0), (0, 5, 0), (0, 0, 4), (-1, 0, 0)]:
            with pytest.raises(ValueError):
                v.grow_from_points([outside], 0.5)
        with pytest.raises(ValueError):
            v.grow_from_points([(1, 1, 1)], 0.5, box=((2, 1, 1), (4, 3, 2)))
    finally:
        V.Volume.geodesic_propagate = original
    assert rec.last(name)[8:10] == (64, 0)
    for bad in (dict(steps=(1, 1, 1)), dict(limit=0), dict(limit=2 ** 32), dict(rounds=0), dict(rounds=1025), dict(rounds=1.5)):
        with pytest.raises(ValueError):
            v.geodesic_propagate(seeds, 0.5, **bad)
    with pytest.raises(ValueError):
        v.geodesic_propagate(seeds[:2], 0.5)


def test_split_bodies_issues_todays_calls_by_default_and_the_geodesic_ones_on_request(stub_volume):
    v, rec = stub_volume

    def new_calls(f):
        before = {k: len(c) for k, c in rec.calls.items()}
        out = f()
        return out, {k: len(c) - before.get(k, 0) for k, c in rec.calls.items() if len(c) - before.get(k, 0)}

    today = {"vkv_distance_transform": 1, "vkv_select_by_distance": 1, "vkv_label_components": 1, "vkv_nearest_target": 1, "vkv_propagate_labels": 1}
    for kw in ({}, {"metric": "euclidean"}):
        (out, counts), new = new_calls(lambda: v.split_bodies(0.5, radius=2, **kw))
        assert new == today and out.dtype == torch.uint32 and counts.dtype == torch.int64 and tuple(counts.shape) == (3,)
        assert rec.last("vkv_nearest_target")[7] == abi.DISTANCE_NONE and rec.last("vkv_propagate_labels")[6:8] == (v.volume.data_ptr(), 0.5)
    rec.after = len(rec.calls.get("vkv_geodesic_propagate", [])) + 2
    (out, counts), new = new_calls(lambda: v.split_bodies(0.5, radius=2, metric="geodesic"))
    assert new == {"vkv_distance_transform": 1, "vkv_select_by_distance": 1, "vkv_label_components": 1, "vkv_geodesic_propagate": 2}
    first, second = rec.calls["vkv_geodesic_propagate"][-2:]
    assert first[1] == v.volume.data_ptr() and first[5] == rec.last("vkv_label_components")[9] and first[6:10] == (list(CHAMFER), abi.GEODESIC_NONE, 64, 0)
    assert second[5] is None and second[8:10] == (128, 1) and first[11] is None and first[12] == out.data_ptr() and tuple(counts.shape) == (3,)
    rec.after = 0
    (out, counts), new = new_calls(lambda: v.split_bodies(0.5, radius2=30, weights=(2, 2, 5), metric="geodesic"))
    assert new == {"vkv_distance_transform_weighted": 1, "vkv_select_by_distance": 1, "vkv_label_components": 1, "vkv_geodesic_propagate": 1}
    assert rec.last("vkv_geodesic_propagate")[6] == [3, 3, 4, 8, 8, 8, 9]
    with pytest.raises(ValueError):
        v.split_bodies(0.5, radius=2, metric="manhattan")


# ---- the listing ----------------------------------------------------------------------------------------------------------------------------------
def test_the_geodesic_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("geodesic.hip", tmp_path / "geodesic.s")
    for name in ("k_geo_init", "k_geo_round", "k_geo_finish"):
        assert len([k for k in kernels if name in k]) == 1, sorted(kernels)
    assert len(kernels) == 3
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)

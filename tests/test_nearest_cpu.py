"""The definition of vkv_nearest_target and vkv_propagate_labels (include/vkvolume_amd.h) restated in numpy, three times:
nearest_brute_np() is the definition (an int64 distance matrix from the voxels to the targets, the targets in box-linear order, argmin's
first occurrence = the smallest box-linear index); nearest_separable_np() restates the kernels pass by pass (min-plus per line with a
first-occurrence argmin per axis, the intermediate formats x' and y' << 15 | x', the reference of tests/test_gpu_nearest.py); near_line_py()
is tests/edt_envelope_ref.py with the feature carry: k_near_axis statement by statement with the stack-in-line inequalities as assertions.  The two restatements are held to the
definition on seeded small boxes, among them contents BUILT FOR TIES, which are asserted to tie: the separable tie argument is proved here,
not assumed.  Then scipy's distance_transform_edt(return_indices=True), the numpy statements of propagate / expand_labels / split_bodies
with scipy.ndimage, one fixed bridge scene, the entry points declared, exported and bound, and the listing of nearest.hip.  No device is
touched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_binding_cpu import HANDLE, context
from tests.edt_envelope_ref import feature_line_py as near_line_py
from tests.test_distance_cpu import NONE, TO_INSIDE, TO_OUTSIDE, ball_structure, inside_np, random_mask_volume, targets_np
from tests.test_distance_weighted_cpu import edt2_weighted_np
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = np.int64(1) << 40        # above every sum and every limit


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def nearest_brute_np(vol_dhw, iso, weights, target=TO_INSIDE, limit=None, box=None, ties=False):
    """(d_nearest, d_dist2) [d, h, w] uint32 of the header's sentences.  The distance matrix [voxels, targets] in int64, the targets in
    box-linear order: argmin takes the first occurrence, which is the smallest box-linear index.  ties=True: also the number of voxels with
    more than one nearest target"""
    limit = NONE if limit is None else int(limit)
    wx, wy, wz = (int(w) for w in weights)
    t = targets_np(vol_dhw, iso, target, box)
    idx = np.flatnonzero(t.ravel())        # increasing: box-linear order
    if idx.size == 0:
        out = np.full(t.shape, NONE, np.uint32), np.full(t.shape, limit, np.uint32)
        return out + (0,) if ties else out
    z, y, x = (a.ravel().astype(np.int64) for a in np.indices(t.shape))
    m = (wz * (z[:, None] - z[idx][None])) ** 2 + (wy * (y[:, None] - y[idx][None])) ** 2 + (wx * (x[:, None] - x[idx][None])) ** 2
    first = m.argmin(axis=1)
    best = m[np.arange(m.shape[0]), first]
    nearest = np.where(best < limit, idx[first], NONE).astype(np.uint32).reshape(t.shape)
    dist = np.minimum(best, limit).astype(np.uint32).reshape(t.shape)
    if ties:
        return nearest, dist, int(((m == best[:, None]).sum(axis=1) > 1).sum())
    return nearest, dist


def _min_plus_first(g, axis, w):
    """(the least g(u) + (w (p - u))^2 over u along `axis`, the SMALLEST u that attains it) for every position p, in int64"""
    n = g.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = n
    u = np.arange(n, dtype=np.int64).reshape(shape)
    best, arg = np.empty_like(g), np.empty_like(g)
    for p in range(n):
        c = g + (int(w) * (u - p)) ** 2
        a = c.argmin(axis=axis)        # first occurrence: the smaller coordinate on a tie
        sl = [slice(None)] * 3
        sl[axis] = p
        best[tuple(sl)] = np.take_along_axis(c, np.expand_dims(a, axis), axis).squeeze(axis)
        arg[tuple(sl)] = a
    return best, arg


def nearest_separable_np(vol_dhw, iso, weights, target=TO_INSIDE, limit=None, box=None):
    """(d_nearest, d_dist2) as nearest.hip computes them: the x pass stores x' of the row's nearest target (the left one of two), the y pass
    y' << 15 | x' (or the box-linear index where no z pass follows), the z pass the box-linear index; every pass reads the feature,
    recomputes g from it, and stores NONE where its value is >= limit.  A pass along an axis of length 1 is not run"""
    limit = NONE if limit is None else int(limit)
    wx, wy, wz = (int(w) for w in weights)
    t = targets_np(vol_dhw, iso, target, box)
    d, h, w = t.shape
    z, y, x = np.indices(t.shape, dtype=np.int64, sparse=True)
    # x
    val, arg = _min_plus_first(np.where(t, 0, FAR).astype(np.int64), 2, wx)
    feat = np.where(val < limit, arg, NONE).astype(np.int64)
    if h > 1:
        g = np.where(feat == NONE, FAR, (wx * (x - feat)) ** 2)
        val, arg = _min_plus_first(g, 1, wy)
        src = np.take_along_axis(feat, arg, 1)        # the winner's source feature
        mul = 32768 if d > 1 else w
        feat = np.where(val < limit, arg * mul + src, NONE).astype(np.int64)
    if d > 1:
        assert feat[feat != NONE].max(initial=0) < 1 << 30
        g = np.where(feat == NONE, FAR, (wx * (x - (feat & 0x7fff))) ** 2 + (wy * (y - (feat >> 15))) ** 2)
        val, arg = _min_plus_first(g, 0, wz)
        src = np.take_along_axis(feat, arg, 0)
        feat = np.where(val < limit, (arg * h + (src >> 15)) * w + (src & 0x7fff), NONE).astype(np.int64)
    return feat.astype(np.uint32), np.minimum(val, limit).astype(np.uint32)


# ---- k_near_axis on whole boxes -----------------------------------------------------------------------------------------------------------
def nearest_kernels_py(vol_dhw, iso, weights, target=TO_INSIDE, limit=None, box=None):
    """the launcher of nearest.hip with near_line_py for the y and z passes (the x pass, a bit walk, is nearest_separable_np's)"""
    limit = NONE if limit is None else int(limit)
    wx, wy, wz = (int(a) for a in weights)
    t = targets_np(vol_dhw, iso, target, box)
    d, h, w = t.shape
    val, arg = _min_plus_first(np.where(t, 0, FAR).astype(np.int64), 2, wx)
    feat = np.where(val < limit, arg, NONE).astype(np.int64)
    dist = np.minimum(val, limit)
    if h > 1:
        mul = 32768 if d > 1 else w
        out, dist = np.empty_like(feat), np.empty_like(feat)
        for z in range(d):
            for x in range(w):
                a, b = near_line_py([int(v) for v in feat[z, :, x]], wy, limit, lambda fv: (wx * abs(x - fv)) ** 2, lambda s, fv: s * mul + fv)
                out[z, :, x], dist[z, :, x] = a, b
        feat = out
    if d > 1:
        out, dist = np.empty_like(feat), np.empty_like(feat)
        for y in range(h):
            for x in range(w):
                a, b = near_line_py([int(v) for v in feat[:, y, x]], wz, limit,
                                    lambda fv: (wx * abs(x - (fv & 0x7fff))) ** 2 + (wy * abs(y - (fv >> 15))) ** 2,
                                    lambda s, fv: (s * h + (fv >> 15)) * w + (fv & 0x7fff))
                out[:, y, x], dist[:, y, x] = a, b
        feat = out
    return feat.astype(np.uint32), dist.astype(np.uint32)


# ---- contents built for ties ------------------------------------------------------------------------------------------------------------
TIE_CONTENTS = ("faces x", "faces y", "faces z", "corners", "checkerboard", "random 0.5")


def tie_contents(kind, shape_dhw, seed=0):
    """bytes 200 (inside) and 17 (outside): targets on the two faces of an axis (a tie in the middle plane where that axis is odd), all
    eight corners, a checkerboard, random 0.5"""
    vol = np.full(shape_dhw, 17, np.uint8)
    if kind == "faces x":
        vol[:, :, 0] = vol[:, :, -1] = 200
    elif kind == "faces y":
        vol[:, 0, :] = vol[:, -1, :] = 200
    elif kind == "faces z":
        vol[0, :, :] = vol[-1, :, :] = 200
    elif kind == "corners":
        vol[::max(shape_dhw[0] - 1, 1), ::max(shape_dhw[1] - 1, 1), ::max(shape_dhw[2] - 1, 1)] = 200
    elif kind == "checkerboard":
        z, y, x = np.indices(shape_dhw)
        vol[(x + y + z) % 2 == 0] = 200
    elif kind == "random 0.5":
        vol[np.random.default_rng(seed).random(shape_dhw) < 0.5] = 200
    else:
        raise KeyError(kind)
    return vol


def check_against_the_definition(vol, weights, target, limit, what, kernels=False):
    want_n, want_d, ties = nearest_brute_np(vol, 0.5, weights, target, limit, ties=True)
    for f in (nearest_separable_np,) + ((nearest_kernels_py,) if kernels else ()):
        got_n, got_d = f(vol, 0.5, weights, target, limit)
        assert got_n.dtype == np.uint32 and got_d.dtype == np.uint32
        assert np.array_equal(got_n, want_n), (f.__name__, what, np.argwhere(got_n != want_n)[:4].tolist())
        assert np.array_equal(got_d, want_d), (f.__name__, what)
    assert np.array_equal(want_d, edt2_weighted_np(vol, 0.5, weights, target, limit)), what
    # the distance AT the returned index is the distance
    hit = want_n != NONE
    zz, yy, xx = np.indices(vol.shape, dtype=np.int64)
    i = want_n[hit].astype(np.int64)
    h, w = vol.shape[1:]
    at = (weights[2] * (zz[hit] - i // (h * w))) ** 2 + (weights[1] * (yy[hit] - i // w % h)) ** 2 + (weights[0] * (xx[hit] - i % w)) ** 2
    assert np.array_equal(at, want_d[hit].astype(np.int64)) and targets_np(vol, 0.5, target).ravel()[i].all(), what
    cap = NONE if limit is None else limit
    assert (want_d[~hit] == cap).all(), what
    return ties


def limits_of(case, rng):
    return (None, int(rng.integers(1, 12)), int(rng.integers(12, 400)))[case % 3]


def test_both_restatements_are_the_definition_on_random_boxes():
    """axes 1 .. 9, weights 1 .. 7, limits none / small / mid, both targets, three densities; the statement-by-statement kernels on every fifth"""
    rng = np.random.default_rng(519)
    tied = 0
    for case in range(1500):
        shape = tuple(int(s) for s in rng.integers(1, 10, size=3))
        if case % 7 == 0:
            shape = tuple(1 if rng.random() < 0.5 else s for s in shape)        # axes of length 1: passes that are not run
        weights = tuple(int(a) for a in rng.integers(1, 8, size=3))
        vol = random_mask_volume(rng, shape, (0.02, 0.15, 0.5)[(case // 3) % 3])
        tied += check_against_the_definition(vol, weights, (TO_INSIDE, TO_OUTSIDE)[case % 2], limits_of(case, rng), (case, shape, weights), kernels=case % 5 == 0)
    assert tied > 1000


@pytest.mark.parametrize("content", TIE_CONTENTS, ids=lambda c: c.replace(" ", "_"))
def test_contents_built_for_ties_tie_and_both_restatements_resolve_them_as_the_definition(content):
    rng = np.random.default_rng(77)
    shapes = [(5, 7, 9), (9, 5, 7), (7, 9, 5), (3, 3, 3), (1, 7, 5), (5, 1, 7), (7, 5, 1), (1, 1, 9), (9, 1, 1), (1, 9, 1), (4, 6, 8)]
    for k, shape in enumerate(shapes):
        vol = tie_contents(content, shape, seed=k)
        for weights in ((1, 1, 1), (2, 2, 5), (3, 7, 1), tuple(int(a) for a in rng.integers(1, 8, size=3))):
            for target in (TO_INSIDE, TO_OUTSIDE):
                for limit in (None, min(weights) ** 2 + 1, 60):
                    ties = check_against_the_definition(vol, weights, target, limit, (content, shape, weights, target, limit), kernels=k < 4)
                    # an odd axis between two faces has a middle plane, an odd axis between corners a middle voxel on an edge; in a
                    # checkerboard an outside voxel has two inside neighbours along x, and random 0.5 ties by sheer number
                    odd = {"faces x": shape[2] % 2 == 1, "faces y": shape[1] % 2 == 1, "faces z": shape[0] % 2 == 1,
                           "corners": any(s % 2 == 1 for s in shape)}.get(content, True)
                    if target == TO_INSIDE and limit is None and min(shape) >= 3 and odd:
                        assert ties > 0, (content, shape, weights)        # else the tie rule is not being tested
    # the tie rule read off directly: the middle plane between two faces belongs to the LOWER face, along every axis
    for axis, content in ((2, "faces x"), (1, "faces y"), (0, "faces z")):
        vol = tie_contents(content, (5, 5, 5))
        n, _ = nearest_separable_np(vol, 0.5, (1, 1, 1))
        zyx = np.stack(np.unravel_index(n.astype(np.int64), vol.shape))
        assert (zyx[axis][tuple(slice(None) if a != axis else 2 for a in range(3))] == 0).all()
    vol = tie_contents("corners", (3, 3, 3))
    assert int(nearest_separable_np(vol, 0.5, (1, 1, 1))[0][1, 1, 1]) == 0 and nearest_brute_np(vol, 0.5, (1, 1, 1), ties=True)[2] == 19


def test_near_line_py_is_the_min_plus_line_with_the_smallest_position():
    """the y pass on single lines: source features x' (or NONE) under a lane at x; the reference takes the first of equal values"""
    rng = np.random.default_rng(2025)
    for case in range(4000):
        n = 1 if case % 10 == 0 else int(rng.integers(1, 40))
        w, wx, x = int(rng.integers(1, 8)), int(rng.integers(1, 8)), int(rng.integers(0, 12))
        limit = (NONE, int(rng.integers(1, 30)), int(rng.integers(30, 4000)))[case % 3]
        share = (0.0, 0.5, 0.9, 1.0)[(case // 3) % 4]
        g_of = lambda fv: (wx * abs(x - fv)) ** 2  # noqa: E731
        src = [NONE if rng.random() < share else int(rng.integers(0, 12)) for _ in range(n)]
        src = [NONE if fv != NONE and g_of(fv) >= limit else fv for fv in src]        # what the pass before stores
        dst, dist = near_line_py(src, w, limit, g_of, lambda s, fv: s << 15 | fv)
        for p in range(n):
            vals = [(g_of(src[u]) + (w * (p - u)) ** 2, u) for u in range(n) if src[u] != NONE]
            best = min(vals, default=(limit, 0))        # tuples: the smallest u of equal values
            if best[0] < limit:
                assert (dst[p], dist[p]) == (best[1] << 15 | src[best[1]], best[0]), (case, p, src, w, limit)
            else:
                assert (dst[p], dist[p]) == (NONE, limit), (case, p, src, w, limit)


def test_near_line_py_at_the_longest_line():
    n = 32768
    for w, limit, feats in ((1, NONE, {0: 0}), (2, NONE, {n - 1: 5}), (1, NONE, {0: 3, n - 1: 0}), (1, 1000, {100: 0, 20000: 2}), (1, NONE, {})):
        src = [NONE] * n
        for i, v in feats.items():
            src[i] = v
        dst, dist = near_line_py(src, w, limit, lambda fv: fv * fv, lambda s, fv: s << 15 | fv)
        p = np.arange(n, dtype=np.int64)
        want_d, want_f = np.full(n, limit, np.int64), np.full(n, NONE, np.int64)
        for i, v in sorted(feats.items()):
            d = v * v + (w * (p - i)) ** 2
            better = (d < want_d) & (d < limit)
            want_d[better], want_f[better] = d[better], i << 15 | v
        assert np.array_equal(np.array(dst, np.int64), want_f) and np.array_equal(np.array(dist, np.int64), want_d), (w, limit, feats)
    line = [0] * 3000        # every position on the stack
    dst, dist = near_line_py(line, 1, NONE, lambda fv: 0, lambda s, fv: s)
    assert dst == list(range(3000)) and dist == [0] * 3000


# ---- scipy ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [TO_INSIDE, TO_OUTSIDE])
def test_against_scipys_feature_transform(target):
    """the distance at scipy's index equals the distance at ours everywhere; the indices are equal where the nearest target is unique"""
    from scipy import ndimage
    rng = np.random.default_rng(61 + target)
    unique_seen = 0
    for k in range(60):
        shape = tuple(int(s) for s in rng.integers(1, 10, size=3))
        weights = tuple(int(a) for a in rng.integers(1, 8, size=3))
        vol = random_mask_volume(rng, shape, (0.02, 0.1, 0.5)[k % 3])
        t = targets_np(vol, 0.5, target)
        if not t.any():
            continue        # scipy is undefined here; the definition is not (test_no_target_...)
        idx = ndimage.distance_transform_edt(~t, sampling=[float(a) for a in weights[::-1]], return_distances=False, return_indices=True).astype(np.int64)
        wv = np.array(weights[::-1], np.int64).reshape(3, 1, 1, 1)
        d_scipy = ((wv * (idx - np.indices(shape))) ** 2).sum(axis=0)
        nearest, dist = nearest_separable_np(vol, 0.5, weights, target)
        ours = np.stack(np.unravel_index(nearest.astype(np.int64), shape))
        d_ours = ((wv * (ours - np.indices(shape))) ** 2).sum(axis=0)
        assert np.array_equal(d_scipy, d_ours) and np.array_equal(d_ours, dist.astype(np.int64))
        z, y, x = (a.ravel().astype(np.int64) for a in np.indices(shape))
        tz, ty, tx = np.nonzero(t)
        m = (weights[2] * (z[:, None] - tz[None])) ** 2 + (weights[1] * (y[:, None] - ty[None])) ** 2 + (weights[0] * (x[:, None] - tx[None])) ** 2
        unique = ((m == m.min(axis=1, keepdims=True)).sum(axis=1) == 1).reshape(shape)
        assert np.array_equal(ours[:, unique], idx[:, unique])
        unique_seen += int(unique.sum())
    assert unique_seen > 1000


def test_no_target_a_single_target_a_limit_and_a_box():
    vol = np.full((3, 4, 5), 17, np.uint8)
    for f in (nearest_brute_np, nearest_separable_np, nearest_kernels_py):
        for limit, cap in ((None, NONE), (7, 7)):
            n, d = f(vol, 0.5, (2, 2, 5), TO_INSIDE, limit)
            assert (n == NONE).all() and (d == cap).all()
            n, d = f(vol, 0.5, (2, 2, 5), TO_OUTSIDE, limit)        # every voxel is a target: its own index
            assert np.array_equal(n.ravel(), np.arange(60)) and (d == 0).all()
    vol[2, 3, 4] = 200
    z, y, x = np.indices(vol.shape)
    want = (5 * (z - 2)) ** 2 + (3 * (y - 3)) ** 2 + (2 * (x - 4)) ** 2
    box = (1, 1, 0, 4, 3, 3)
    for f in (nearest_brute_np, nearest_separable_np, nearest_kernels_py):
        n, d = f(vol, 0.5, (2, 3, 5))
        assert (n == 59).all() and np.array_equal(d, want)
        n, d = f(vol, 0.5, (2, 3, 5), limit=30)
        assert np.array_equal(n, np.where(want < 30, 59, NONE)) and np.array_equal(d, np.minimum(want, 30))
        n, d = f(vol, 0.5, (2, 3, 5), box=box)        # the target at (3, 2, 2) of the box: index (2 * 3 + 2) * 4 + 3
        assert n.shape == (3, 3, 4) and (n == 35).all() and np.array_equal(d, want[0:3, 1:4, 1:5])


# ---- propagate, expand_labels, split_bodies -----------------------------------------------------------------------------------------------
def propagate_labels_np(nearest, labels, mask_inside=None):
    """vkv_propagate_labels: labels.ravel()[nearest] where nearest is an index of the box and the mask (None: none) is inside, else 0"""
    n = nearest.size
    ok = nearest < n
    out = np.where(ok, labels.ravel()[np.where(ok, nearest, 0)], 0).astype(np.uint32)
    return out if mask_inside is None else np.where(mask_inside, out, 0).astype(np.uint32)


def weighted_ball_structure(r2, weights):
    """§5.16's ball, and §5.18's with weights: the offsets with sum (w_a k_a)^2 <= r2"""
    if weights is None:
        return ball_structure(r2)
    rx, ry, rz = (int(np.floor(np.sqrt(r2))) // a for a in weights)
    z, y, x = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    return (weights[0] * x) ** 2 + (weights[1] * y) ** 2 + (weights[2] * z) ** 2 <= r2


def expand_labels_np(vol, iso, labels, r2=None, weights=None, mask_inside=None):
    """Volume.expand_labels: the labels of the inside voxels grown into what lies within r2 (None: everywhere)"""
    nearest, _ = nearest_separable_np(vol, iso, weights or (1, 1, 1), TO_INSIDE, None if r2 is None else r2 + 1)
    return propagate_labels_np(nearest, labels, mask_inside)


def split_bodies_np(vol, iso, r2, connectivity=6, weights=None):
    """Volume.split_bodies with scipy.ndimage: binary_erosion by the ball (border_value=1: nothing beyond the array is outside), label (the
    numbering of vkv_label_components), then the nearest core by the tie rule, masked by the original inside voxels: (labels, K)"""
    from scipy import ndimage
    inside = inside_np(vol, iso)
    eroded = ndimage.binary_erosion(inside, structure=weighted_ball_structure(r2, weights), border_value=1)
    core, k = ndimage.label(eroded, structure=ndimage.generate_binary_structure(3, {6: 1, 26: 3}[connectivity]))
    nearest, _ = nearest_separable_np(np.where(eroded, 255, 0).astype(np.uint8), 0.5, weights or (1, 1, 1), TO_INSIDE)
    return propagate_labels_np(nearest, core.astype(np.uint32), inside), k


def bridge_scene():
    """two balls of radius 6 joined by a bridge 2 voxels thick in 40 x 20 x 20 (bytes 200 inside, 17 outside), and the bridge's voxels
    between the balls"""
    z, y, x = np.indices((20, 20, 40))
    balls = ((x - 10) ** 2 + (y - 10) ** 2 + (z - 10) ** 2 <= 36) | ((x - 29) ** 2 + (y - 10) ** 2 + (z - 10) ** 2 <= 36)
    bridge = (x >= 10) & (x <= 29) & (y >= 9) & (y <= 10) & (z >= 9) & (z <= 10)
    return np.where(balls | bridge, 200, 17).astype(np.uint8), bridge & ~balls


def test_propagate_labels_np():
    labels = np.arange(100, 124, dtype=np.uint32).reshape(2, 3, 4)
    nearest = np.array([0, 23, NONE, 24, 5, 0xfffffffe] * 4, np.uint32).reshape(2, 3, 4)
    out = propagate_labels_np(nearest, labels)
    assert out.dtype == np.uint32 and out.ravel()[:6].tolist() == [100, 123, 0, 0, 105, 0]
    mask = np.zeros((2, 3, 4), bool)
    mask[0, 0, 1] = True
    assert propagate_labels_np(nearest, labels, mask).ravel().tolist() == [0, 123] + [0] * 22


def test_the_bridge_scene_from_scipy_alone():
    """one component at first, two after the erosion by radius 2; scipy's own feature transform hands the cores' labels back: they cover
    exactly the original mask, and the bridge is divided between labels 1 and 2"""
    from scipy import ndimage
    vol, bridge = bridge_scene()
    inside = vol >= 128
    assert ndimage.label(inside)[1] == 1 and bridge.sum() == 6 + 3 * 8        # x = 17 .. 22 on the balls' axis row, 16 .. 23 on the three beside it
    eroded = ndimage.binary_erosion(inside, structure=ball_structure(4), border_value=1)
    core, k = ndimage.label(eroded)
    assert k == 2 and not (eroded & bridge).any()
    idx = ndimage.distance_transform_edt(~eroded, return_distances=False, return_indices=True)
    full = np.where(inside, core[tuple(idx)], 0)
    assert np.array_equal(full != 0, inside)
    assert set(full[bridge].tolist()) == {1, 2} and (full[bridge] == 1).sum() == (full[bridge] == 2).sum() == 15
    # and the numpy statement of Volume.split_bodies says the same (the scene is symmetric about x = 19.5: no voxel of it ties between cores)
    got, kk = split_bodies_np(vol, 0.5, 4)
    assert kk == 2 and np.array_equal(got, full.astype(np.uint32))
    sizes = ndimage.sum_labels(np.ones_like(got), got, index=[1, 2])
    assert sizes[0] == sizes[1] == inside.sum() // 2


def test_expand_labels_np_is_the_dilation_with_the_nearest_label():
    from scipy import ndimage
    rng = np.random.default_rng(5)
    vol = random_mask_volume(rng, (9, 11, 13), 0.03)
    inside = vol >= 128
    labels = ndimage.label(inside)[0].astype(np.uint32)
    for r2 in (1, 2, 9):
        out = expand_labels_np(vol, 0.5, labels, r2)
        assert np.array_equal(out != 0, ndimage.binary_dilation(inside, structure=ball_structure(r2))) and np.array_equal(out[inside], labels[inside])
    out = expand_labels_np(vol, 0.5, labels)
    assert (out != 0).all()        # unlimited: the Voronoi regions
    mask = rng.random(vol.shape) < 0.5
    assert np.array_equal(expand_labels_np(vol, 0.5, labels, 9, mask_inside=mask), np.where(mask, expand_labels_np(vol, 0.5, labels, 9), 0))


# ---- entry points -------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"#define VKV_NEAREST_NONE 0xffffffffu", header) and abi.NEAREST_NONE == 0xffffffff
    assert re.search(r"\bint\s+vkv_nearest_target\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*float iso,\s*"
                     r"int32_t target,\s*const uint32_t weights\[3\],\s*uint32_t limit,\s*void\s*\*d_scratch,\s*uint32_t\s*\*d_nearest,\s*uint32_t\s*\*d_dist2,\s*"
                     r"void\s*\*stream\)", header)
    assert re.search(r"\bint\s+vkv_propagate_labels\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint32_t\s*\*d_nearest,\s*const uint32_t\s*\*d_labels,\s*uint32_t\s*\*d_out,\s*"
                     r"VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*const uint8_t\s*\*d_mask_volume,\s*float mask_iso,\s*void\s*\*stream\)", header)
    assert "vkv_nearest_target_scratch_bytes" not in header        # one scratch block for the three calls
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in ("vkv_nearest_target", "vkv_propagate_labels"):
        assert name in lib.EXPORTS and re.search(r"\b%s$" % name, out, flags=re.M)
    at = L.vkv_nearest_target.argtypes
    assert len(at) == 12 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[5] is C.c_int32
    assert at[6] is C.POINTER(C.c_uint32) and at[7] is C.c_uint32 and L.vkv_nearest_target.restype is C.c_int
    at = L.vkv_propagate_labels.argtypes
    assert len(at) == 9 and at[4] is abi.Extent3D and at[5] is C.POINTER(abi.Box) and at[7] is C.c_float and L.vkv_propagate_labels.restype is C.c_int
    for name in ("nearest_target", "propagate_labels"):
        assert callable(getattr(lib.Context, name + "_rc")) and not hasattr(lib.Context, name)
    buf = (C.c_uint64 * 256)()
    a = C.addressof(buf)
    w = (C.c_uint32 * 3)(2, 2, 5)
    assert L.vkv_nearest_target(None, a, abi.Extent3D(4, 4, 4), None, 0.5, 0, w, 5, a + 64, a + 512, a + 1024, None) == abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_propagate_labels(None, a, a + 512, a + 1024, abi.Extent3D(4, 4, 4), None, None, 0.5, None) == abi.VKV_E_INVALID_ARGUMENT
    assert not any(buf) and list(w) == [2, 2, 5]


def test_the_binding_passes_the_arguments_in_the_headers_order():
    ctx, rec = context()
    e = abi.Extent3D(40, 50, 60)
    assert ctx.nearest_target_rc(10, e, None, 0.5, abi.DISTANCE_TO_OUTSIDE, (2, 2, 5), None, 11, 12, 13, 99) == 0
    assert rec.last("vkv_nearest_target") == (HANDLE, 10, bytes(e), None, 0.5, abi.DISTANCE_TO_OUTSIDE, [2, 2, 5], abi.DISTANCE_NONE, 11, 12, 13, 99)
    ctx.nearest_target_rc(10, e, None, 0.5, abi.DISTANCE_TO_INSIDE, None, 7, 11, 12)
    assert rec.last("vkv_nearest_target") == (HANDLE, 10, bytes(e), None, 0.5, abi.DISTANCE_TO_INSIDE, None, 7, 11, 12, None, 0)
    b = abi.Box(1, 2, 3, 4, 5, 6)
    assert ctx.propagate_labels_rc(20, 21, 22, e, b, 23, 0.25, 99) == 0
    assert rec.last("vkv_propagate_labels") == (HANDLE, 20, 21, 22, bytes(e), bytes(b), 23, 0.25, 99)
    ctx.propagate_labels_rc(20, 21, 22, e, None)
    assert rec.last("vkv_propagate_labels") == (HANDLE, 20, 21, 22, bytes(e), None, None, 0.0, 0)


@pytest.fixture
def stub_volume(monkeypatch):
    """a Volume of 12 x 5 x 4 host bytes on a context whose library records the calls"""
    ctx, rec = context()
    monkeypatch.setattr(V, "_stream", lambda: 99)
    v = V.Volume(ctx, device=torch.device("cpu"))
    v.volume = torch.full((4, 5, 12), 200, dtype=torch.uint8)
    v.extent = abi.Extent3D(12, 5, 4)
    return v, rec


def test_volume_methods_make_the_calls_the_docstrings_name(stub_volume):
    v, rec = stub_volume
    n = v.nearest_target(0.5)
    assert n.dtype == torch.uint32 and tuple(n.shape) == (4, 5, 12)
    call = rec.last("vkv_nearest_target")
    assert call[5:8] == (abi.DISTANCE_TO_INSIDE, [1, 1, 1], abi.DISTANCE_NONE) and call[10] is None and call[11] == 99        # weights None: (1, 1, 1)
    n, d = v.nearest_target(0.5, to="outside", limit=30, box=((1, 1, 1), (3, 2, 2)), weights=(2, 2, 5), distance=True)
    assert tuple(n.shape) == tuple(d.shape) == (2, 2, 3) and d.dtype == torch.uint32
    call = rec.last("vkv_nearest_target")
    assert call[3] == bytes(abi.Box(1, 1, 1, 3, 2, 2)) and call[5:8] == (abi.DISTANCE_TO_OUTSIDE, [2, 2, 5], 30) and call[9] == n.data_ptr() and call[10] == d.data_ptr()
    labels = torch.zeros((4, 5, 12), dtype=torch.int32).view(torch.uint32)
    out = v.expand_labels(labels, 0.5, radius=2)
    assert out.dtype == torch.uint32 and rec.last("vkv_nearest_target")[5:8] == (abi.DISTANCE_TO_INSIDE, [1, 1, 1], 5)        # limit r2 + 1
    call = rec.last("vkv_propagate_labels")
    assert call[2] == labels.data_ptr() and call[3] == out.data_ptr() and call[6] is None
    v.expand_labels(labels, 0.5, mask=v)
    assert rec.last("vkv_nearest_target")[7] == abi.DISTANCE_NONE and rec.last("vkv_propagate_labels")[6:8] == (v.volume.data_ptr(), 0.5)
    v.expand_labels(labels, 0.5, radius2=3, mask=v, mask_iso=0.25, weights=(1, 1, 2))
    assert rec.last("vkv_nearest_target")[6:8] == ([1, 1, 2], 4) and rec.last("vkv_propagate_labels")[7] == 0.25
    before = {k: len(c) for k, c in rec.calls.items()}
    out, counts = v.split_bodies(0.5, radius=2)
    new = {k: len(c) - before.get(k, 0) for k, c in rec.calls.items() if len(c) - before.get(k, 0)}
    assert new == {"vkv_distance_transform": 1, "vkv_select_by_distance": 1, "vkv_label_components": 1, "vkv_nearest_target": 1, "vkv_propagate_labels": 1}
    assert rec.last("vkv_nearest_target")[7] == abi.DISTANCE_NONE and rec.last("vkv_nearest_target")[1] != v.volume.data_ptr()        # the eroded volume, unlimited
    assert rec.last("vkv_propagate_labels")[6:8] == (v.volume.data_ptr(), 0.5) and out.dtype == torch.uint32 and counts.dtype == torch.int64
    for bad in ((2, 2), (2, 2, 0), "xyz"):
        with pytest.raises(ValueError):
            v.nearest_target(0.5, weights=bad)
    with pytest.raises(ValueError):
        v.nearest_target(0.5, to="nowhere")
    with pytest.raises(ValueError):
        v.expand_labels(labels[:2], 0.5)
    v.ctx._lib.status = abi.VKV_E_UNSUPPORTED        # a status other than 0 raises: the check is the caller's
    with pytest.raises(lib.VkvError, match="recorded message"):
        v.nearest_target(0.5)


# ---- the listing ----------------------------------------------------------------------------------------------------------------------------
def test_the_nearest_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("nearest.hip", tmp_path / "nearest.s")
    for name, count in (("k_near_x", 1), ("k_near_axis", 2), ("k_propagate", 1)):
        assert len([k for k in kernels if name in k]) == count, sorted(kernels)
    assert len(kernels) == 4        # k_edt_bits is edt.hip's: declared here, defined there
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)
    # the envelope pass is edt_passes.hpp's: no more registers than the copy it replaced had (k_near_x keeps its own walk)
    for name, vgprs in (("k_near_x", 19), ("k_near_axisILi1E", 26), ("k_near_axisILi2E", 28)):
        assert [v["NumVgprs"] for k, v in kernels.items() if name in k][0] <= vgprs, (name, kernels)

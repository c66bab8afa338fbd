"""CPU: what tests/test_gpu_far_boxes.py stands on.  That module runs every box-of-voxels operation on a box of a few tens of thousands of
voxels inside a volume of just over 2^32 bytes, where the whole volume cannot come to the host; its reference is the suite's numpy statement
of the operation evaluated on a WINDOW: the box grown by the halo the operation reads, clamped to the volume, with the box translated into
it and `origin` saying where the window lies.  The halos:
  "box"    nothing beyond the box exists for the operation;
  "voxel"  one voxel per side (the filter's neighbours, the indexed mesh's normals);
  "cells"  whole map cells, two per side (a cell reads one voxel of its neighbour; the cells beside the box's own are written too).
Here, without a GPU and without a large allocation:
  (a) every window reference equals the statement on a whole mid-sized volume with the box inside, for boxes that touch each face and none:
      the halo is enough;
  (b) every reference on the real contents differs from the reference on a window that holds the surround fill everywhere - what a kernel
      whose address wrapped to the start of the buffer would read: a wrap is visible.  (vkv_propagate_labels without a mask and
      vkv_label_visibility_map read no voxel of the volume: they form no volume address, and their references are asserted to be the same);
  (c) every *_scratch_bytes function gives, for each large extent and box, what it gives for the box in its window volume;
  (d) the references and make_aux take the parameters that tests/box_ops_fuzz.py draws as keywords; with the defaults every reference of a
      large case has the bytes it had before they did (a table of digests)."""
import functools

import numpy as np
import pytest

from tests.test_cell_summary_cpu import summary_np
from tests.test_component_stats_cpu import component_stats_np, select_by_table_np
from tests.test_components_cpu import components_np, inside_np, select_np
from tests.test_distance_cpu import TO_INSIDE, TO_OUTSIDE, edt2_np, select_by_distance_np
from tests.test_distance_weighted_cpu import edt2_weighted_np
from tests.test_filter_cpu import binomial3_np, median3_np
from tests.test_geodesic_cpu import CHAMFER, NONE as GEO_NONE, geodesic_sweeps_np
from tests.test_label_mesh_cpu import label_mesh_np
from tests.test_labels_render_cpu import visibility_map_np
from tests.test_mesh_cpu import mesh_np
from tests.test_mesh_indexed_cpu import indexed_np
from tests.test_mip_cpu import max_map_np
from tests.test_nearest_cpu import nearest_separable_np, propagate_labels_np
from vkvolume_amd import abi, geodesic, labels as LB, lib

ISO = 0.5
FILLS = (0x00, 0xFF)
WEIGHTS = (2, 2, 5)
EVERYTHING = 2 ** 64 - 1

# ---- the large volumes and their boxes (width, height, depth), (x0, y0, z0, w, h, d) -----------------------------------------------------
EXTENTS = {
    "A": (1000, 1000, 4400),        # voxel (296, 967, 4294) has byte offset exactly 2^32, in the middle of a row
    "B": (2, 65536, 32800),         # z * H reaches 2 149 515 264 > 2^31; width 2: the narrow-row paths
    "C": (65536, 33000, 2),         # y * W reaches 2 162 622 464 > 2^31, and the plane is above 2^31
}
CASES = (        # (name, extent, box, the seed of its contents)
    ("A-straddle", "A", (281, 960, 4290, 70, 21, 9), 1001),        # holds the voxel at offset 2^32: rows on both sides, one across
    ("A-far", "A", (930, 979, 4381, 70, 21, 19), 1002),            # touches the three far faces
    ("B-far", "B", (0, 65515, 32781, 2, 21, 19), 1003),
    ("C-far", "C", (65466, 32979, 0, 70, 21, 2), 1004),
)
CASE = {c[0]: c for c in CASES}


def blocks_of(extent):
    """voxels per map cell and axis: 4, where that divides the axis (else 5, else the axis): every cell is whole"""
    return tuple(4 if e % 4 == 0 else 5 if e % 5 == 0 else e for e in extent)


def map_extent_of(extent):
    return tuple(e // b for e, b in zip(extent, blocks_of(extent)))


def box_contents(shape_dhw, seed):
    """contents("random 0.5", shape, seed) of tests/test_gpu_distance.py: bytes 200 (inside at ISO) and 17"""
    return np.where(np.random.default_rng(seed).random(shape_dhw) < 0.5, 200, 17).astype(np.uint8)


def window(extent, box, halo):
    """(origin (x, y, z), size (w, h, d), the box inside the window) of the window of `box` in a volume of `extent` for the halo kind"""
    lo, hi = [], []
    for e, b, x0, n in zip(extent, blocks_of(extent), box[:3], box[3:]):
        if halo == "cells":
            lo.append(max(x0 // b - 2, 0) * b)
            hi.append((min((x0 + n) // b + 2, e // b - 1) + 1) * b)
        else:
            r = {"box": 0, "voxel": 1}[halo]
            lo.append(max(x0 - r, 0))
            hi.append(min(x0 + n + r, e))
    origin = tuple(lo)
    return origin, tuple(h - l for l, h in zip(lo, hi)), tuple(x - o for x, o in zip(box[:3], origin)) + tuple(box[3:])


def window_array(extent, box, halo, contents, fill):
    """(the window as a host array holding the surround fill and the box's contents, its origin, the box inside it)"""
    origin, (w, h, d), wbox = window(extent, box, halo)
    vol = np.full((d, h, w), fill, np.uint8)
    x0, y0, z0, bw, bh, bd = wbox
    vol[z0:z0 + bd, y0:y0 + bh, x0:x0 + bw] = contents
    return vol, origin, wbox


def crop(vol, box):
    x0, y0, z0, w, h, d = box
    return np.ascontiguousarray(vol[z0:z0 + d, y0:y0 + h, x0:x0 + w])


# ---- the inputs an operation takes besides the volume: made from the box's contents, the same whatever surrounds the box ------------------
def keep_table(rng, k, mode="some"):
    """one byte per label: which labels a table keeps (or shows): "some" of them at random, "all" or "none" of them"""
    n = max(k, 1)
    return {"some": rng.integers(0, 2, size=n), "all": np.ones(n, np.int64), "none": np.zeros(n, np.int64)}[mode].astype(np.uint8)


def make_aux(contents, seed, iso=ISO, connectivity=6, weights=WEIGHTS, target=TO_INSIDE, limit=None, dist_limit=10, keep="some", colors="some",
             seed_density=0.03):
    """the keywords are tests/box_ops_fuzz.py's drawn parameters; their defaults are what the large cases use"""
    rng = np.random.default_rng(seed + 50000)
    labels, sizes, counts = components_np(contents, iso, connectivity)
    k = int(counts[0])
    nearest, _ = nearest_separable_np(contents, iso, weights, target, limit)
    return dict(
        labels=labels, sizes=sizes, counts=counts,
        keep=keep_table(rng, k, keep),
        colors=(keep_table(rng, k, colors).astype(np.uint32) * np.uint32(0xFF000000)) | np.uint32(0x00C08040),
        dist2=edt2_np(contents, iso, target, dist_limit),
        nearest=nearest,
        plabels=rng.integers(1, 2 ** 32, size=contents.shape, dtype=np.uint64).astype(np.uint32),
        seeds=np.where(rng.random(contents.shape) < seed_density, rng.integers(1, 6, size=contents.shape), 0).astype(np.uint32))


# ---- the references: f(vol, box, origin, aux, blocks, **parameters) -> {name: array}; vol holds the box at `box` and lies at `origin` in the real
# volume.  The parameters are keywords whose defaults are the large cases' constants; tests/box_ops_fuzz.py draws them, and gives every
# reference the whole drawn set, so each takes what it knows and ignores the rest (**_).
# (a name that starts with "_" is not an output: "_at" says where the arrays lie in the real volume's map, in cells (z, y, x); "_cap*" is the
# capacity the call is to be given, where the parameters set one)
def _map_extent(vol, blocks, me=None):
    return tuple(e // b for e, b in zip(vol.shape[::-1], blocks)) if me is None else tuple(me)


def _cells(vol, box, origin, b, lo_hi, me=None):
    """the slices (z, y, x) into vol's own map of the cells lo_hi(x0, n, b) names per axis, in the real volume's map, and their first cell.
    me: the map extent of a volume that is its own window (origin 0), whose last cells need not be whole"""
    d, h, w = vol.shape
    extent = (w, h, d)
    if me is None:
        assert all(e % k == 0 and o % k == 0 for e, k, o in zip(extent, b, origin)), "the window is made of whole cells"
        me = tuple(e // k for e, k in zip(extent, b))
    else:
        assert tuple(origin) == (0, 0, 0) and all(-(-e // m) == k for e, m, k in zip(extent, me, b)), "blocks are ceil(extent / map extent)"
    sl, at = [], []
    for axis in range(3):
        first, last = lo_hi(box[axis] + origin[axis], box[3 + axis], b[axis])        # in the real map; the window ends where the map does, or later
        first, last = max(first, origin[axis] // b[axis]), min(last, origin[axis] // b[axis] + me[axis] - 1)
        sl.append(slice(first - origin[axis] // b[axis], last + 1 - origin[axis] // b[axis]))
        at.append(first)
    return tuple(sl[::-1]), np.array(at[::-1], np.int64)


def capacity_of(cap, total):
    """a capacity parameter: None (the large cases: nothing is cut, and the call gets total + 5), a number, or a function of the total"""
    return None if cap is None else int(cap(total) if callable(cap) else cap)


def cut(want, counts, pairs):
    """cuts the lists of a reference at their capacities: pairs of (capacity parameter, index of the total in counts, the lists' names); the
    element of counts after a total is what is written"""
    for n, (cap, at, names) in enumerate(pairs):
        c = capacity_of(cap, int(counts[at]))
        if c is not None:
            counts[at + 1] = min(int(counts[at]), c)
            want["_cap%d" % n] = c
            for name in names:
                want[name] = want[name][:c]
    want["counts"] = counts
    return want


def ref_max_map_box(vol, box, origin, aux, blocks, me=None, **_):
    """vkv_max_map(box): the cells whose voxel box grown by one voxel meets the box: ceil(x0 / b) - 1 .. (x0 + n) / b, clamped to the map"""
    sl, at = _cells(vol, box, origin, blocks, lambda x0, n, b: (max(-(-x0 // b) - 1, 0), (x0 + n) // b), me)
    return {"cells": np.ascontiguousarray(max_map_np(vol, _map_extent(vol, blocks, me))[sl]), "_at": at}


def ref_max_map_whole(vol, box, origin, aux, blocks, me=None, **_):
    """vkv_max_map of the whole volume, around the box: the cells of the box and one more per side"""
    sl, at = _cells(vol, box, origin, blocks, lambda x0, n, b: (max(x0 // b - 1, 0), (x0 + n - 1) // b + 1), me)
    return {"cells": np.ascontiguousarray(max_map_np(vol, _map_extent(vol, blocks, me))[sl]), "_at": at}


def ref_cell_summary(vol, box, origin, aux, blocks, me=None, **_):
    """vkv_cell_summary(box), no gradient: the cells that hold a voxel of the box"""
    sl, at = _cells(vol, box, origin, blocks, lambda x0, n, b: (x0 // b, (x0 + n - 1) // b), me)
    mw, mh, md = me = _map_extent(vol, blocks, me)
    return {"cells": np.ascontiguousarray(summary_np(vol, None, me).reshape(md, mh, mw, 16)[sl]), "_at": at}


def ref_visibility_map(vol, box, origin, aux, blocks, me=None, **_):
    """vkv_label_visibility_map writes the whole map: here the window's cells; every other cell sees no voxel of the box and holds 0"""
    sl, at = _cells(vol, box, origin, blocks, lambda x0, n, b: (x0 // b - 2, (x0 + n) // b + 2), me)
    vis = visibility_map_np(aux["labels"], box, vol.shape, aux["colors"], _map_extent(vol, blocks, me))
    return {"cells": np.ascontiguousarray(vis[sl]), "_at": at}


def ref_histogram(vol, box, origin, aux, blocks, mode=0, before=0, **_):
    """mode: abi.HISTOGRAM_SET, _ADD or _SUBTRACT (0, 1, 2); before: what every bin held"""
    counts = np.bincount(crop(vol, box).reshape(-1).astype(np.int64), minlength=65536).astype(np.uint64)
    with np.errstate(over="ignore"):
        hist = {0: counts, 1: np.uint64(before) + counts, 2: np.uint64(before) - counts}[mode]
    return {"hist": hist.view(np.int64)}


def ref_filter(statement):
    return lambda vol, box, origin, aux, blocks, **_: {"dst": crop(statement(vol), box)}


def ref_mesh(vol, box, origin, aux, blocks, iso=ISO, cap=None, **_):
    tri = mesh_np(vol, iso, box, origin)
    return cut({"triangles": tri}, np.array([len(tri), len(tri)], np.uint64), [(cap, 0, ("triangles",))])


def ref_mesh_indexed(vol, box, origin, aux, blocks, iso=ISO, cap=None, cap_vertices=None, **_):
    v, n, f = indexed_np(vol, iso, box, origin)
    return cut({"vertices": v, "normals": n, "indices": f.astype(np.uint32)}, np.array([len(f), len(f), len(v), len(v)], np.uint64),
               [(cap, 0, ("indices",)), (cap_vertices, 2, ("vertices", "normals"))])


def ref_components(connectivity):
    def ref(vol, box, origin, aux, blocks, iso=ISO, connectivity=connectivity, cap=None, **_):
        labels, sizes, counts = components_np(vol, iso, connectivity, box)
        return cut({"labels": labels, "sizes": sizes}, counts, [(cap, 0, ("sizes",))])
    return ref


def ref_select_components(vol, box, origin, aux, blocks, lo=3, hi=EVERYTHING, fill=9, **_):
    return {"dst": select_np(crop(vol, box), aux["labels"], aux["sizes"], int(aux["counts"][1]), lo, hi, fill)}


def ref_component_stats(vol, box, origin, aux, blocks, cap=None, **_):
    """the records as bytes; the statement's coordinates are the array's, the call's the real volume's: exact integers, moved by `origin`"""
    k = int(aux["counts"][0])
    c = capacity_of(cap, k)
    rec = component_stats_np(vol, aux["labels"], k, k + 5 if c is None else c, box)
    some = rec["voxels"] > 0
    for axis, o in zip("xyz", origin):
        for f in ("min_", "max_"):
            rec[f + axis][some] += np.uint32(o)
        rec["sum_" + axis] += rec["voxels"] * np.uint64(o)
    want = {"records": np.frombuffer(rec.tobytes(), np.uint8).copy()}
    if c is not None:
        want["_cap0"] = c
    return want


def ref_select_by_table(vol, box, origin, aux, blocks, fill=7, **_):
    return {"dst": select_by_table_np(crop(vol, box), aux["labels"], aux["keep"], fill)}


DISTANCE_CALLS = tuple((target, limit) for target in (TO_INSIDE, TO_OUTSIDE) for limit in (None, 10))


def rejected(shape, names):
    """the reference of a call that the header rejects (a limit of 0): nothing of any output is written"""
    return {name: np.zeros((0,) + tuple(shape[1:]), np.uint32) for name in names}


def ref_distance(vol, box, origin, aux, blocks, iso=ISO, calls=DISTANCE_CALLS, **_):
    shape = box[:2:-1]
    return {"to %d limit %s" % (t, l): rejected(shape, "d")["d"] if l == 0 else edt2_np(vol, iso, t, l, box) for t, l in calls}


def ref_select_by_distance(vol, box, origin, aux, blocks, lo=1, hi=9, fill=255, **_):
    return {"dst": select_by_distance_np(crop(vol, box), aux["dist2"], lo, hi, fill)}


def ref_distance_weighted(vol, box, origin, aux, blocks, iso=ISO, weights=WEIGHTS, limit=None, **_):
    if limit == 0:
        return rejected(box[:2:-1], ["to %d" % t for t in (TO_INSIDE, TO_OUTSIDE)])
    return {"to %d" % t: edt2_weighted_np(vol, iso, weights, t, limit, box) for t in (TO_INSIDE, TO_OUTSIDE)}


def ref_nearest(vol, box, origin, aux, blocks, iso=ISO, weights=WEIGHTS, target=TO_INSIDE, limit=None, **_):
    if limit == 0:
        return rejected(box[:2:-1], ("nearest", "dist2"))
    nearest, dist2 = nearest_separable_np(vol, iso, weights, target, limit, box)
    return {"nearest": nearest, "dist2": dist2}


def ref_propagate(masked):
    def ref(vol, box, origin, aux, blocks, iso=ISO, **_):
        return {"out": propagate_labels_np(aux["nearest"], aux["plabels"], inside_np(vol, iso, box) if masked else None)}
    return ref


def ref_geodesic(vol, box, origin, aux, blocks, iso=ISO, steps=CHAMFER, limit=None, **_):
    if limit == 0:
        return dict(rejected(box[:2:-1], ("dist", "labels")), counts=np.zeros(0, np.uint64))
    dist, labels = geodesic_sweeps_np(vol, iso, aux["seeds"], steps, limit, box)
    return {"dist": dist, "labels": labels, "counts": np.array([1, int((dist != GEO_NONE).sum())], np.uint64)}


def ref_label_mesh(vol, box, origin, aux, blocks, iso=ISO, cap=None, table=False, **_):
    """table: with aux["colors"] as the colour table (else every label is shown)"""
    tri, lab = label_mesh_np(aux["labels"], aux["colors"] if table else None, vol, iso, box, origin)
    return cut({"triangles": tri, "triangle_labels": lab}, np.array([len(tri), len(tri)], np.uint64), [(cap, 0, ("triangles", "triangle_labels"))])


# name: (halo, reference, the operation reads voxels of the volume)
REFERENCES = {
    "max_map_box": ("cells", ref_max_map_box, True),
    "max_map_whole": ("cells", ref_max_map_whole, True),
    "cell_summary": ("cells", ref_cell_summary, True),
    "histogram": ("box", ref_histogram, True),
    "filter_binomial": ("voxel", ref_filter(binomial3_np), True),
    "filter_median": ("voxel", ref_filter(median3_np), True),
    "mesh": ("box", ref_mesh, True),
    "mesh_indexed": ("voxel", ref_mesh_indexed, True),
    "components_6": ("box", ref_components(6), True),
    "components_26": ("box", ref_components(26), True),
    "select_components": ("box", ref_select_components, True),
    "component_stats": ("box", ref_component_stats, True),
    "select_by_table": ("box", ref_select_by_table, True),
    "distance": ("box", ref_distance, True),
    "select_by_distance": ("box", ref_select_by_distance, True),
    "distance_weighted": ("box", ref_distance_weighted, True),
    "nearest": ("box", ref_nearest, True),
    "propagate": ("box", ref_propagate(False), False),
    "propagate_masked": ("box", ref_propagate(True), True),
    "geodesic": ("box", ref_geodesic, True),
    "visibility_map": ("cells", ref_visibility_map, False),
    "label_mesh": ("box", ref_label_mesh, True),
}


def same(a, b):
    """two references agree: the same names, shapes, types and bits"""
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(contents, aux) of a large case"""
    _, _, box, seed = CASE[name]
    contents = box_contents((box[5], box[4], box[3]), seed)
    return contents, make_aux(contents, seed)


@functools.lru_cache(maxsize=None)
def reference(name, op, fill):
    """the window reference of operation `op` on the large case `name` under the surround fill"""
    _, extent, box, _ = CASE[name]
    contents, aux = case_inputs(name)
    halo, ref, _ = REFERENCES[op]
    vol, origin, wbox = window_array(EXTENTS[extent], box, halo, contents, fill)
    return ref(vol, wbox, origin, aux, blocks_of(EXTENTS[extent]))


# ---- (a) the halo is enough -----------------------------------------------------------------------------------------------------------------
MID = (40, 30, 20)        # blocks (4, 5, 4): a map of 10 x 6 x 5 cells
MID_BOXES = {"the low faces": (0, 0, 0, 13, 9, 7), "the far faces": (27, 21, 13, 13, 9, 7), "no face": (13, 11, 6, 14, 9, 7), "x0 and z1": (0, 7, 14, 9, 11, 6),
             "on cell edges": (8, 10, 4, 12, 10, 8), "one cell in": (4, 5, 4, 13, 9, 7)}


@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill_%02x" % f)
@pytest.mark.parametrize("where", sorted(MID_BOXES), ids=lambda b: b.replace(" ", "_"))
def test_the_window_reference_is_the_statement_on_the_whole_volume(where, fill):
    box = MID_BOXES[where]
    assert blocks_of(MID) == (4, 5, 4)
    contents = box_contents((box[5], box[4], box[3]), 7)
    aux = make_aux(contents, 7)
    whole = np.full(MID[::-1], fill, np.uint8)
    whole[box[2]:box[2] + box[5], box[1]:box[1] + box[4], box[0]:box[0] + box[3]] = contents
    for op, (halo, ref, _) in REFERENCES.items():
        vol, origin, wbox = window_array(MID, box, halo, contents, fill)
        if halo != "box":
            assert np.array_equal(vol, whole[origin[2]:origin[2] + vol.shape[0], origin[1]:origin[1] + vol.shape[1], origin[0]:origin[0] + vol.shape[2]])
        want, got = ref(whole, box, (0, 0, 0), aux, blocks_of(MID)), ref(vol, wbox, origin, aux, blocks_of(MID))
        assert same(got, want), "%s, box %s: the window %s at %s gives another reference than the whole volume" % (op, where, vol.shape, origin)
    # and the visibility map holds nothing outside the window
    origin, size, _ = window(MID, box, "cells")
    vis = visibility_map_np(aux["labels"], box, whole.shape, aux["colors"], map_extent_of(MID))
    assert vis.any()
    b = blocks_of(MID)
    vis[origin[2] // b[2]:(origin[2] + size[2]) // b[2], origin[1] // b[1]:(origin[1] + size[1]) // b[1], origin[0] // b[0]:(origin[0] + size[0]) // b[0]] = 0
    assert not vis.any()


def test_the_windows_of_the_large_cases():
    for name, extent, box, _ in CASES:
        e = EXTENTS[extent]
        assert e[0] * e[1] * e[2] > 2 ** 32 and all(a + n <= m for a, n, m in zip(box[:3], box[3:], e)), name
        assert blocks_of(e) == tuple(min(4, m) for m in e)
        for halo in ("box", "voxel", "cells"):
            origin, size, wbox = window(e, box, halo)
            assert all(o + w == x for o, w, x in zip(origin, wbox[:3], box[:3])) and wbox[3:] == box[3:]
            assert all(o + s <= m for o, s, m in zip(origin, size, e)) and size[0] * size[1] * size[2] < 200000
    (w, h, _), (x0, y0, z0, bw, bh, bd) = EXTENTS["A"], CASE["A-straddle"][2]
    assert (4294 * h + 967) * w + 296 == 2 ** 32 and x0 <= 296 < x0 + bw and y0 <= 967 < y0 + bh and z0 <= 4294 < z0 + bd
    assert (z0 * h + y0) * w + x0 < 2 ** 32 < ((z0 + bd - 1) * h + y0 + bh - 1) * w + x0 + bw - 1
    assert (EXTENTS["B"][2] - 1) * EXTENTS["B"][1] > 2 ** 31 and (EXTENTS["C"][1] - 1) * EXTENTS["C"][0] > 2 ** 31 and EXTENTS["C"][0] * EXTENTS["C"][1] > 2 ** 31
    # 70 x 21 x 19: 110 box-linear workgroups of 256 voxels, mesh tiles of 4 rows and 16 slices of cubes, geodesic tiles of 8 x 8 x 8
    assert -(-70 * 21 * 19 // 256) == 110 and (-(-20 // 4), -(-18 // 16)) == (5, 2) and -(-70 // 8) * -(-21 // 8) * -(-19 // 8) == 81


# ---- (b) a wrapped address is visible ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", FILLS, ids=lambda f: "fill_%02x" % f)
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_the_reference_differs_from_that_of_the_surround_fill_alone(name, fill):
    _, extent, box, _ = CASE[name]
    contents, aux = case_inputs(name)
    for op, (halo, ref, reads_volume) in REFERENCES.items():
        vol, origin, wbox = window_array(EXTENTS[extent], box, halo, np.full(contents.shape, fill, np.uint8), fill)
        assert (vol == fill).all()
        blank = ref(vol, wbox, origin, aux, blocks_of(EXTENTS[extent]))
        assert same(blank, reference(name, op, fill)) == (not reads_volume), "%s, %s, fill %#x" % (op, name, fill)


# ---- (c) host planning does not depend on the surroundings ------------------------------------------------------------------------------------
SCRATCH = {"mesh": (lib.mesh_scratch_bytes, "box"), "mesh_indexed": (lib.mesh_indexed_scratch_bytes, "voxel"), "components": (lib.components_scratch_bytes, "box"),
           "distance": (lib.distance_transform_scratch_bytes, "box"), "geodesic": (geodesic.scratch_bytes, "box"), "label_mesh": (LB.mesh_scratch_bytes, "box")}


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_scratch_sizes_are_those_of_the_box_in_its_window(name):
    _, extent, box, _ = CASE[name]
    n = box[3] * box[4] * box[5]
    for what, (scratch_bytes, halo) in SCRATCH.items():
        for kind in (halo, "cells"):
            _, size, wbox = window(EXTENTS[extent], box, kind)
            big = scratch_bytes(abi.Extent3D(*EXTENTS[extent]), abi.Box(*box))
            assert big > 0 and big == scratch_bytes(abi.Extent3D(*size), abi.Box(*wbox)), (what, name, kind)
            assert big == scratch_bytes(abi.Extent3D(*box[3:]), None), (what, name, "the box as a volume of its own")
    assert lib.distance_transform_scratch_bytes(abi.Extent3D(*EXTENTS[extent]), abi.Box(*box)) == 4 * n + 8 * ((n + 63) // 64)


# ---- (d) the references are those of the commit before the keywords came ----------------------------------------------------------------------
# sha256 (16 hex digits) over every large case and both fills of the reference's arrays (name, type, shape, bytes, names sorted), taken before
# ref_* and make_aux got keyword parameters: with the defaults nothing of what tests/test_gpu_far_boxes.py compares with has moved
DIGESTS = {
    "max_map_box": "14ce6904bbcba3d9",
    "max_map_whole": "ef9aa2acb85d09cd",
    "cell_summary": "c928f8533700b31a",
    "histogram": "1f670722138d722e",
    "filter_binomial": "1265231a39e7d6d8",
    "filter_median": "6e6ff7264509b838",
    "mesh": "f278bb0da90f7b92",
    "mesh_indexed": "7c17677b02139fb0",
    "components_6": "7ce96b4340f47260",
    "components_26": "55cbf1f64e7e0717",
    "select_components": "867f61501ef83f82",
    "component_stats": "8023391245e45684",
    "select_by_table": "c710ee5e05ad6df2",
    "distance": "22b4809379b93dc4",
    "select_by_distance": "e6e40738efe0e979",
    "distance_weighted": "c5ba6f2ca456f35e",
    "nearest": "5dc60b4eb8785eb4",
    "propagate": "3ecfd87c5fcd317f",
    "propagate_masked": "e0b11f1a4e611713",
    "geodesic": "b5636e19cbfa3cc0",
    "visibility_map": "47d46dcc8baf1130",
    "label_mesh": "633f6683f22425a2",
}


@pytest.mark.parametrize("op", sorted(REFERENCES))
def test_the_references_of_the_large_cases_keep_their_bytes(op):
    import hashlib
    h = hashlib.sha256()
    for name, _, _, _ in CASES:
        for fill in FILLS:
            r = reference(name, op, fill)
            for k in sorted(r):
                h.update(("%s|%s|%s|" % (k, r[k].dtype.str, r[k].shape)).encode())
                h.update(r[k].tobytes())
    assert h.hexdigest()[:16] == DIGESTS[op], op

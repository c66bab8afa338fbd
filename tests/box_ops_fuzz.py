"""The draw recipe of tests/test_gpu_box_ops_fuzz.py: every box-of-voxels operation of the volume-processing family on small drawn volumes,
with every parameter the header accepts drawn as well.  draw(op, seed) gives a case as a plain dict (it is printed in every assertion
message) and the case follows from (op, seed) alone; volume(case), inputs(case, vol) and reference(case, vol, aux) make the host arrays and
the expected outputs from the numpy statements of the suite, through the references of tests/test_far_boxes_cpu.py.  Nothing here needs a
GPU; tests/test_box_ops_fuzz_cpu.py checks the recipe (determinism, coverage, agreement of independent statements, mutants).

Stratified axes.  A hand-picked test walks one axis at a time; a plain random draw leaves coverage to chance.  Here every axis of the case
has n classes, and
  - the extent's axes take class seed mod n with n = 5 (width), 2 (height), 3 (depth): pairwise coprime, so any 30 consecutive seeds hold
    every combination, and the 12 default seeds hold a narrow, a one-wave and a three-segment width and two or more tiles in y and in z;
  - seed mod 6 == 5 has no box; the ten other seeds of a dozen take, per axis, two permutations of the five box classes, drawn for the
    dozen so that every class falls on an axis long enough for it (_box_plan), and x0 mod 4 = j mod 4 where the class leaves x0 free, j
    numbering the boxed seeds;
  - every other axis (contents, iso, connectivity, limit, weights, capacities, map, ...) takes class perm[seed mod n], where perm is a
    permutation of the n classes drawn from (op, axis, seed div n): every n consecutive seeds hold every class of every axis, whatever
    the other axes do, and different axes with the same n do not march in step.
tests/test_box_ops_fuzz_cpu.py asserts the coverage that follows, per operation, for the default seeds."""
import functools
import zlib

import numpy as np

from tests import test_far_boxes_cpu as FB
from tests import mesh_smooth_ref as MS
from tests.test_components_cpu import components_np, inside_np
from tests.test_distance_cpu import TO_INSIDE, TO_OUTSIDE, edt2_np, select_by_distance_np
from tests.test_geodesic_cpu import TABLES as STEP_TABLES
from tests.test_label_mesh_indexed_cpu import label_indexed_np
from tests.test_max_map_consumers_cpu import thr_of
from tests.test_mip_cpu import INV255
from tests.test_nearest_cpu import nearest_separable_np, propagate_labels_np

F = np.float32
DEFAULT_SEEDS = 12
MAX_VOLUME, MAX_BOX = 60000, 35000        # voxels: every statement stays below a second
EVERYTHING = FB.EVERYTHING

# operation: (the reference of tests/test_far_boxes_cpu.py, takes a box, what it does with a map: None, "reads" one, "writes" its cells)
OPS = {
    "max_map_box": ("max_map_box", True, "writes"),
    "max_map_whole": ("max_map_whole", False, "writes"),
    "cell_summary": ("cell_summary", True, "writes"),
    "histogram": ("histogram", True, None),
    "filter_binomial": ("filter_binomial", True, None),
    "filter_median": ("filter_median", True, None),
    "mesh": ("mesh", True, "reads"),
    "mesh_indexed": ("mesh_indexed", True, "reads"),
    "components": ("components_6", True, "reads"),
    "select_components": ("select_components", True, None),
    "component_stats": ("component_stats", True, None),
    "select_by_table": ("select_by_table", True, None),
    "distance": ("distance", True, None),
    "select_by_distance": ("select_by_distance", True, None),
    "distance_weighted": ("distance_weighted", True, None),
    "nearest": ("nearest", True, None),
    "propagate": ("propagate", True, None),
    "propagate_masked": ("propagate_masked", True, None),
    "geodesic": ("geodesic", True, None),
    "visibility_map": ("visibility_map", True, "writes"),
    "label_mesh": ("label_mesh", True, "reads"),              # the map is vkv_label_visibility_map's, built on the device from the same table
    "label_mesh_indexed": ("label_mesh_indexed", True, "reads"),
    "chain_mesh": ("chain_mesh", True, None),                  # components -> indexed label mesh -> adjacency -> smooth -> normals
    "chain_split": ("chain_split", True, None),                # distance -> erode -> components -> nearest -> propagate, masked
}

WIDTHS = ((1, 3), (4, 7), (60, 68), (250, 262), (510, 520))        # the narrow-row kernels, one wave, one, two and three x segments of 256
HEIGHTS = ((1, 9), (63, 66))                                       # rows per workgroup are 4
DEPTHS = ((1, 3), (15, 19), (33, 37))                              # mesh segment 16, filter segment 18
BOX_CLASSES = ("low", "high", "inner", "whole", "thin")            # from face 0, reaching the far face, touching neither, the axis, one voxel
CONTENTS = ("two_bytes", "arbitrary", "salt", "balls", "uniform", "threshold")        # uniform: all inside and all outside, by turns
SURROUNDS = ("zero", "ff", "arbitrary", "two_bytes", "threshold")
ISOS = ("byte", "below_byte", "above_byte", "one", "low_edge", "above_one")              # low_edge: 0.0 and a negative value, by turns
CONNECTIVITIES = (6, 14, 26)
TARGETS = (TO_INSIDE, TO_OUTSIDE)
LIMITS = ("none", "one", "small", "above_diagonal", "zero")                  # zero: the header rejects it
WEIGHTS = ("ones", "spacing", "odd", "bound")                      # (1, 1, 1), (2, 2, 5), (1, 3, 7), just under what the header accepts
SIZE_BOUNDS = ("empty", "everything", "from_3", "window")
DISTANCE_BOUNDS = ("shell", "targets", "all", "far")
TABLE_MODES = ("some", "all", "none")
ROUNDS = (1, 3, 16)
CAPACITIES = ("plus_5", "total", "minus_1", "between", "one", "zero")
MAPS = ("none", "blocks", "any")                                   # no map; ceil(e / block), blocks 2 .. 6; any count of cells (some past the volume)
GUARDS = (0x00, 0xFF, 0xA5)
HISTOGRAM_MODES = (0, 1, 2)


def _rng(*key):
    return np.random.default_rng([zlib.crc32(str(k).encode()) for k in key])


def _pick(op, axis, index, classes, dull=0):
    """the class of `axis` for seed `index`: every n consecutive seeds take the n classes in an order drawn from (op, axis, index div n).
    dull: the last `dull` classes are those that leave little to compute (nothing inside, a rejected limit, a capacity of 0, every label
    hidden); they go to the edge seeds of the n first (_edge: a volume one voxel thick, which has little to compute already), so
    that the dull classes of all axes fall together and the other seeds keep a surface, bodies and distances to work on"""
    n = len(classes)
    rng = _rng("class", op, axis, index // n)
    if not dull:
        return classes[int(rng.permutation(n)[index % n])]
    seeds = list(range(index // n * n, index // n * n + n))
    keys = rng.random(n)
    order = sorted(seeds, key=lambda s: (not _edge(op, s), keys[s % n]))
    numbers = [n - dull + int(k) for k in rng.permutation(dull)] + [int(k) for k in rng.permutation(n - dull)]
    return classes[dict(zip(order, numbers))[index]]


def _edge(op, seed):
    """the seed's volume is one voxel thick on some axis"""
    return min(extent_of(op, seed)) == 1


def in_class(cls, x0, n, e):
    """the box (x0, n) on an axis of e voxels is of the class; a short axis makes a box several things at once (one voxel is thin AND whole)"""
    return {"whole": n == e, "thin": n == 1, "low": x0 == 0 and n < e, "high": x0 > 0 and x0 + n == e, "inner": x0 > 0 and x0 + n < e}[cls]


def _origins(cls, e):
    """the x0 the class admits on an axis of e voxels (none: the axis is too short for it)"""
    if cls in ("whole", "low"):
        return [0] if cls == "whole" or e >= 2 else []
    if cls == "thin":
        return list(range(e))
    if cls == "high":
        return list(range(1, max(e - 1, 2))) if e >= 2 else []
    return list(range(1, max(e - 2, 2))) if e >= 3 else []        # inner


def _near(cls, e):
    """the origins of _origins that _box_axis draws from: on a long axis only the first eighth, but for a thin box"""
    return [x for x in _origins(cls, e) if x <= max(e // 8, 3) or cls == "thin"]


def _box_axis(rng, cls, e, residue=None):
    """(x0, n) of the class on an axis of e voxels, the whole axis where it is too short for the class; residue: x0 mod 4, where the class
    leaves the origin free and one fits"""
    origins = _origins(cls, e)
    if not origins:
        return 0, e
    slack = max(e // 8, 3)        # a box on a long axis covers most of it: the wide extents are there for their boxes
    near = _near(cls, e)
    fit = [x for x in near if residue is not None and x % 4 == residue]
    x0 = int(rng.choice(fit or near))
    if cls in ("whole", "thin", "high"):
        return x0, {"whole": e, "thin": 1, "high": e - x0}[cls]
    most = e - x0 - 1        # low and inner stop short of the far face
    return x0, int(rng.integers(max(min(2, most), most - slack), most + 1))


def extent_of(op, seed):
    """(w, h, d): class seed mod n of each axis; the other axes shrink when one is long"""
    rng = _rng("extent", op, seed)
    w, h, d = (int(rng.integers(lo, hi + 1)) for lo, hi in (WIDTHS[seed % 5], HEIGHTS[seed % 2], DEPTHS[seed % 3]))
    if seed % 5 == 0:        # the short classes take their lengths in turn: 1, 2, 3 all occur, and a length of 1 not more often than it must
        w = 1 + (seed // 5 + 1) % 3
    if seed % 2 == 0:
        h = 1 + (seed // 2 * 4 + 5) % 9
    if seed % 3 == 0:
        d = 1 + (seed // 3 + 1) % 3
    if w * h * d > MAX_VOLUME:
        d = max(1, min(d, MAX_VOLUME // (w * h)))
    return w, h, d


def _classes(rng, lengths):
    """a permutation of the five box classes for five axes of these lengths, each class on an axis long enough for it where there is one"""
    free, out = list(range(5)), [None] * 5
    for cls in ("inner",) + tuple(rng.permutation(("low", "high"))) + tuple(rng.permutation(("thin", "whole"))):
        fits = [i for i in free if _origins(cls, lengths[i])] or free
        out[free.pop(free.index(fits[int(rng.integers(len(fits)))]))] = str(cls)
    return out


@functools.lru_cache(maxsize=None)
def _box_plan(op, dozen):
    """the box classes per axis of the ten boxed seeds of a dozen, {seed: (class x, class y, class z)}: two permutations of the five classes
    per axis, drawn again until every class lies on an axis long enough for it, every x0 mod 4 can be had (the extents are known: they
    follow from the seeds), the widest axis has a box that is not thin, and the thin classes fall on the volumes that are one voxel thick
    themselves but for one box, a single plane inside a thicker volume (a thin box has no cubes): each dozen of seeds holds every class on
    every axis by construction, and most of it has a surface"""
    seeds = [s for s in range(12 * dozen, 12 * dozen + 12) if s % 6 != 5]
    extents = [extent_of(op, s) for s in seeds]
    rng, best = _rng("boxes", op, dozen), None
    for _ in range(500):
        plan = [_classes(rng, [e[a] for e in extents[:5]]) + _classes(rng, [e[a] for e in extents[5:]]) for a in range(3)]
        short = sum(not _origins(plan[a][i], extents[i][a]) for a in range(3) for i in range(10))
        residues = {i % 4 for i in range(10) if any(x % 4 == i % 4 for x in _near(plan[0][i], extents[i][0]))}
        narrow = all(plan[0][i] == "thin" for i in range(10) if extents[i][0] == max(e[0] for e in extents))        # the widest axis has a wide box
        # thin boxes go to the volumes that are thin themselves, but for one plane inside a volume that is not
        thin = [sum(plan[a][i] == "thin" for a in range(3)) for i in range(10) if min(extents[i]) > 1]
        score = short + 4 - len(residues) + narrow + (1 not in thin) + max(0, sum(t > 0 for t in thin) - 1)
        if best is None or score < best[0]:
            best = (score, plan)
        if best[0] == 0:
            break
    return {s: tuple(best[1][a][i] for a in range(3)) for i, s in enumerate(seeds)}


def draw(op, seed):
    """the case (op, seed) as a plain dict"""
    _, takes_box, map_use = OPS[op]
    rng = _rng("draw", op, seed)
    pick = lambda axis, classes, dull=0: _pick(op, axis, seed, classes, dull)        # noqa: E731
    extent = extent_of(op, seed)
    # ---- box
    j = seed - seed // 6
    box = classes = None
    if takes_box and seed % 6 != 5:
        classes = _box_plan(op, seed // 12)[seed]
        (x0, bw), (y0, bh), (z0, bd) = (_box_axis(rng, c, e, j % 4 if a == 0 else None) for a, (c, e) in enumerate(zip(classes, extent)))
        box = [x0, y0, z0, bw, bh, bd]
        for a in (2, 1, 0):        # too many voxels: shorten z, then y, then x, on the side that keeps the axis's class; at last z whatever its class
            rest = box[3] * box[4] * box[5] // box[3 + a]
            if box[3] * box[4] * box[5] > MAX_BOX and classes[a] in ("low", "high", "inner"):
                n = max(min(2, box[3 + a]), MAX_BOX // rest)
                box[a] += box[3 + a] - n if classes[a] == "high" else 0
                box[3 + a] = n
        if box[3] * box[4] * box[5] > MAX_BOX:
            box[5] = max(1, MAX_BOX // (box[3] * box[4]))
        box = tuple(box)
        classes = tuple(c if in_class(c, box[a], box[3 + a], extent[a]) else [k for k in BOX_CLASSES if in_class(k, box[a], box[3 + a], extent[a])][0]
                        for a, c in enumerate(classes))
    shape = box[3:] if box else extent
    # ---- iso and contents
    contents, iso_class = pick("contents", CONTENTS, 2), pick("iso", ISOS, 2)
    if seed // 6 % 4 != 3:        # in three of four sixes of seeds the contents without a surface fall on the isos without one: more cases have a surface
        pair = _rng("pair", op, seed // 6)
        contents = CONTENTS[int(np.concatenate([pair.permutation(4), 4 + pair.permutation(2)])[ISOS.index(iso_class)])]
    if contents == "uniform":
        contents = ("inside", "outside")[seed // len(CONTENTS) % 2]
    if iso_class == "low_edge":
        iso_class = ("zero", "negative")[seed // len(ISOS) % 2]
    byte = (17 if iso_class == "above_byte" else 200) if contents == "two_bytes" else int(rng.integers(1, 255))        # 200 at, or 17 just below, the threshold
    x = F(byte) * INV255
    iso = {"byte": x, "below_byte": np.nextafter(x, F(-1)), "above_byte": np.nextafter(x, F(2)), "zero": F(0), "negative": F(-0.25), "one": F(1),
           "above_one": F(1.01)}[iso_class]
    # ---- the parameters of the calls
    weights_class, limit_class = pick("weights", WEIGHTS), pick("limit", LIMITS, 1)
    weights = {"ones": (1, 1, 1), "spacing": (2, 2, 5), "odd": (1, 3, 7), "bound": tuple(37837 // max(n - 1, 1) for n in shape)}[weights_class]
    used = weights if op in ("distance_weighted", "nearest", "propagate", "propagate_masked") else (1, 1, 1)
    diagonal = sum((wa * (n - 1)) ** 2 for wa, n in zip(used, shape))
    reach = [int(v) for v in rng.integers(0, 3, 3)]        # small: a distance that occurs, so that a voxel lies exactly at the limit
    small = sum((wa * k) ** 2 for wa, k in zip(used, reach)) or used[0] ** 2
    limit = {"none": None, "zero": 0, "one": 1, "small": min(small, 0xfffffffe), "above_diagonal": min(diagonal + 1 + int(rng.integers(0, 9)), 0xfffffffe)}[limit_class]
    steps = tuple(int(c) for c in pick("steps", STEP_TABLES))
    if op == "geodesic" and limit_class == "above_diagonal":        # above every path: 65535 per move and a move per voxel
        limit = 0xfffffffe
    if op == "geodesic" and limit_class == "small":        # the cost of a path of one to four moves
        limit = sum(int(rng.choice([c for c in steps if c])) for _ in range(int(rng.integers(1, 5))))
    target = pick("target", TARGETS)
    bounds_class = pick("bounds", DISTANCE_BOUNDS if op == "select_by_distance" else SIZE_BOUNDS)
    lo, hi = {"empty": (0, 0), "everything": (1, EVERYTHING), "from_3": (3, EVERYTHING), "window": (2, int(rng.integers(2, 60))),
              "shell": (1, int(rng.integers(1, 20))), "targets": (0, 0), "all": (0, 0xffffffff), "far": (10, 0xffffffff)}[bounds_class]
    map_class = pick("map", {"reads": MAPS, "writes": MAPS[1:] if op == "max_map_whole" else MAPS[1:2], None: MAPS[:1]}[map_use])
    me = None
    if map_class == "blocks":
        me = tuple(-(-e // int(rng.integers(2, 7))) for e in extent)
    elif map_class == "any":
        me = tuple(int(rng.integers(1, e + 1)) for e in extent)
    caps = {name: (pick(name, CAPACITIES, 2), round(float(rng.random()), 6)) for name in ("cap", "cap_vertices")}
    params = dict(
        iso=float(iso), connectivity=pick("connectivity", CONNECTIVITIES), target=target, limit=limit, weights=weights, lo=lo, hi=hi,
        fill=int(rng.integers(0, 256)), calls=((target, limit), (1 - target, None)), steps=steps,
        rounds=pick("rounds", ROUNDS), max_calls=400, in_place=bool(pick("in_place", (False, True))), mode=pick("mode", HISTOGRAM_MODES),
        table=bool(pick("table", (False, True))), use_map=me is not None and map_use == "reads", me=me,
        keep=pick("keep", TABLE_MODES, 1), colors=pick("colors", TABLE_MODES, 1))
    if op in ("label_mesh", "label_mesh_indexed") and me is not None:        # a visibility map needs the table it was built from
        params["table"] = True
    threshold = thr_of(iso)
    params.update(r2=int(rng.integers(1, 10)), erode_fill=params["fill"] % threshold if 0 < threshold < 256 else params["fill"],
                  passes=int(rng.integers(0, 6)), pinned=round(float(rng.choice((0.0, 0.2, 1.0))), 1), normals_label=round(float(rng.random()), 6))
    prefill = int(rng.integers(0, 256))
    params["before"] = prefill * 0x0101010101010101
    return dict(op=op, seed=seed, extent=extent, box=box, box_classes=classes,
                contents=contents, surround=pick("surround", SURROUNDS), iso_class=iso_class, byte=byte, threshold=threshold, limit_class=limit_class,
                weights_class=weights_class, bounds_class=bounds_class, map_class=map_class, caps=caps, params=params,
                guard=pick("guard", GUARDS), prefill=prefill, offsets=int(rng.integers(0, 2 ** 31)))


def offset_of(case, name):
    """by how many times its alignment the buffer `name` of the case starts past a 256-byte boundary: 0 .. 15"""
    return zlib.crc32(("%d %s" % (case["offsets"], name)).encode()) % 16


def whole_box(case):
    return case["box"] or (0, 0, 0) + tuple(case["extent"])


def blocks_of(case):
    me = case["params"]["me"]
    return (1, 1, 1) if me is None else tuple(-(-e // m) for e, m in zip(case["extent"], me))


def _bytes(rng, kind, shape, thr, byte):
    """contents of a kind for the threshold byte thr (0 .. 256: the smallest byte that is inside)"""
    top, under = min(thr, 255), max(thr - 1, 0)
    if kind == "two_bytes":
        return np.where(rng.random(shape) < 0.5, 200, 17).astype(np.uint8)
    if kind == "arbitrary":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if kind == "salt":
        return np.where(rng.random(shape) < 0.01, rng.integers(top, 256, shape), rng.integers(0, under + 1, shape)).astype(np.uint8)
    if kind == "balls":        # two to four smooth balls that cross the threshold byte
        z, y, x = np.indices(shape).astype(np.float64)
        field = np.zeros(shape)
        for _ in range(int(rng.integers(2, 5))):
            c = [float(rng.uniform(-1, n)) for n in shape]
            radius = float(rng.uniform(1.5, 5.0))
            field = np.maximum(field, (radius - np.sqrt((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2)) * 30 + min(thr, 230))
        return np.clip(field, 0, 255).astype(np.uint8)
    if kind == "inside":
        return rng.integers(top, 256, shape).astype(np.uint8)
    if kind == "outside":
        return rng.integers(0, under + 1, shape).astype(np.uint8)
    if kind == "threshold":
        return np.full(shape, top, np.uint8)
    if kind in ("zero", "ff"):
        return np.full(shape, 0 if kind == "zero" else 255, np.uint8)
    raise ValueError(kind)


def volume(case):
    """the host volume [d, h, w]: the surround, and the box's contents drawn apart from it"""
    w, h, d = case["extent"]
    x0, y0, z0, bw, bh, bd = whole_box(case)
    vol = _bytes(_rng("surround", case["op"], case["seed"]), case["surround"], (d, h, w), case["threshold"], case["byte"])
    vol[z0:z0 + bd, y0:y0 + bh, x0:x0 + bw] = _bytes(_rng("contents", case["op"], case["seed"]), case["contents"], (bd, bh, bw), case["threshold"], case["byte"])
    return vol


def capacity(case, name):
    cls, u = case["caps"][name]
    return {"plus_5": lambda t: t + 5, "total": lambda t: t, "minus_1": lambda t: max(t - 1, 0), "one": lambda t: 1, "zero": lambda t: 0,
            "between": lambda t: int(u * t)}[cls]


def parameters(case):
    """the keywords for the reference and for the call"""
    return dict(case["params"], cap=capacity(case, "cap"), cap_vertices=capacity(case, "cap_vertices"))


def inputs(case, vol):
    """make_aux of the box's contents with the case's parameters: the inputs of the calls that take labels, sizes, distances, tables, seeds"""
    p = case["params"]
    aux = FB.make_aux(FB.crop(vol, whole_box(case)), 1000 * case["seed"] + 7, iso=p["iso"], connectivity=p["connectivity"], weights=p["weights"], target=p["target"],
                      limit=p["limit"] or None, dist_limit=p["limit"] or 25, keep=p["keep"], colors=p["colors"])
    if case["op"] == "select_components":        # the sizes as a labelling with the drawn capacity left them
        k = int(aux["counts"][0])
        aux["counts"][1] = min(k, capacity(case, "cap")(k))
        aux["sizes"] = aux["sizes"][:int(aux["counts"][1])]
    return aux


# ---- the calls the far-box table lacks, in the form of its references ----------------------------------------------------------------------
def ref_label_mesh_indexed(vol, box, origin, aux, blocks, iso=FB.ISO, cap=None, cap_vertices=None, table=False, **_):
    v, n, pairs, f, fl = label_indexed_np(aux["labels"], aux["colors"] if table else None, vol, iso, box)
    return FB.cut({"vertices": v, "normals": n, "vertex_labels": pairs, "indices": f.astype(np.uint32), "triangle_labels": fl},
                  np.array([len(f), len(f), len(v), len(v)], np.uint64), [(cap, 0, ("indices", "triangle_labels")), (cap_vertices, 2, ("vertices", "normals", "vertex_labels"))])


def taubin_factors(passes):
    return [float(f) for f in MS.taubin(0.5, -0.53, 3)[:passes]]


def pinned_mask(share, n, seed):
    """one byte per vertex, non-zero = pinned: any non-zero byte pins"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < share, rng.integers(1, 256, n), 0).astype(np.uint8)


def ref_chain_mesh(vol, box, origin, aux, blocks, iso=FB.ISO, connectivity=6, cap=None, cap_vertices=None, passes=4, pinned=0.0, normals_label=0.5, **_):
    """the bodies of the box as smoothed indexed meshes with normals from the faces, by the numpy chain of tests/mesh_smooth_ref.py: the
    extraction is cut at its capacities and everything after it sees the cut lists, as the device calls do through d_counts"""
    labels, _, ccounts = components_np(vol, iso, connectivity, box)
    v, _, _, f, fl = label_indexed_np(labels, None, vol, iso, box)
    want = FB.cut({"vertices": v, "indices": f.astype(np.uint32), "triangle_labels": fl}, np.array([len(f), len(f), len(v), len(v)], np.uint64),
                  [(cap, 0, ("indices", "triangle_labels")), (cap_vertices, 2, ("vertices",))])
    counts, cap_t, cap_v = [int(c) for c in want["counts"]], want["_cap0"], want["_cap1"]
    mask = pinned_mask(pinned, max(cap_v, 1), len(v))
    label = 1 + int(normals_label * int(ccounts[0]))
    smooth = MS.smooth_np(want["vertices"], f[:cap_t], taubin_factors(passes), counts=counts, pinned=mask[:counts[3]]) if counts[3] else want["vertices"]
    want.update(vertices=smooth, labels=labels, component_counts=ccounts[[0, 2]],
                normals=MS.vertex_normals_np(smooth, f[:cap_t], None, 0, counts=counts),
                normals_of_label=MS.vertex_normals_np(smooth, f[:cap_t], fl[:cap_t], label, counts=counts))
    want["_pinned"], want["_label"] = mask, label
    return want


def ref_chain_split(vol, box, origin, aux, blocks, iso=FB.ISO, connectivity=6, r2=4, erode_fill=0, **_):
    """Volume.split_bodies step by step from the statements: erode by the ball of r2, label the cores, the nearest core, its label where the
    ORIGINAL volume is inside.  tests/test_box_ops_fuzz_cpu.py holds it to split_bodies_np (scipy) where that applies"""
    dist2 = edt2_np(vol, iso, TO_OUTSIDE, r2 + 1, box)
    eroded = vol.copy()
    x0, y0, z0, w, h, d = box
    eroded[z0:z0 + d, y0:y0 + h, x0:x0 + w] = select_by_distance_np(FB.crop(vol, box), dist2, 1, r2, erode_fill)
    core, _, counts = components_np(eroded, iso, connectivity, box)
    nearest, _ = nearest_separable_np(eroded, iso, (1, 1, 1), TO_INSIDE, None, box)
    return {"dist2": dist2, "eroded": FB.crop(eroded, box), "core": core, "counts": counts[[0, 2]], "nearest": nearest,
            "out": propagate_labels_np(nearest, core, inside_np(vol, iso, box))}


REFERENCES = dict(FB.REFERENCES, label_mesh_indexed=("voxel", ref_label_mesh_indexed, True), chain_mesh=("voxel", ref_chain_mesh, True),
                  chain_split=("box", ref_chain_split, True))


def reference(case, vol, aux, references=None):
    """the expected outputs; references: a table like REFERENCES (tests/test_box_ops_fuzz_cpu.py passes mutants)"""
    _, ref, _ = (references or REFERENCES)[OPS[case["op"]][0]]
    return ref(vol, whole_box(case), (0, 0, 0), aux, blocks_of(case), **parameters(case))

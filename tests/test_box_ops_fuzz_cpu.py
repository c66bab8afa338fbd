"""CPU: the recipe of tests/box_ops_fuzz.py itself, which tests/test_gpu_box_ops_fuzz.py only executes.
  (a) draw() is deterministic, and every drawn case passes the library's own pure-host checks (the scratch-size functions give no 0, the
      weights are inside the header's bound, the box inside the extent, the map extent valid for its geometry);
  (b) coverage: over the default seeds every operation meets every class of every axis of the recipe - conditions on the recipe;
  (c) where the suite has two independent statements of an operation they agree on the default-seed cases small enough for the slow one;
  (d) mutants: a fuzz that cannot fail is worth nothing, and a broken kernel must not run on a shared machine, so the STATEMENTS are broken
      here, each in the way a kernel plausibly is.  For every mutant at least one default-seed case of the named operation gives a result
      that differs from the true statement's in what the GPU module compares; the seed is on record in profiles/box_ops_fuzz.txt."""
import numpy as np
import pytest

from tests import box_ops_fuzz as Z
from tests import test_far_boxes_cpu as FB
from tests.test_component_stats_cpu import component_stats_np
from tests.test_components_cpu import components_np, inside_np
from tests.test_distance_cpu import TO_OUTSIDE, edt2_brute_np, edt2_np
from tests.test_filter_cpu import binomial3_np, median3_np
from tests.test_geodesic_cpu import geodesic_brute_np, geodesic_rounds_np, geodesic_sweeps_np
from tests.test_label_mesh_cpu import label_mesh_loop, label_mesh_np
from tests.test_mesh_cpu import mesh_loop, mesh_np
from tests.test_nearest_cpu import nearest_brute_np, nearest_separable_np, split_bodies_np
from vkvolume_amd import abi, geodesic, labels as LB, lib

SEEDS = range(Z.DEFAULT_SEEDS)
BOXED = sorted(op for op, (_, takes_box, _) in Z.OPS.items() if takes_box)
F = np.float32


def built(op, seed, _cache={}):
    """(case, volume, inputs, reference) of a default-seed case, made once"""
    if (op, seed) not in _cache:
        case = Z.draw(op, seed)
        vol = Z.volume(case)
        aux = Z.inputs(case, vol)
        for a in (vol,) + tuple(aux.values()):
            a.setflags(write=False)
        _cache[(op, seed)] = (case, vol, aux, Z.reference(case, vol, aux))
    return _cache[(op, seed)]


# ---- (a) determinism and the library's host checks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(Z.OPS))
def test_draw_is_deterministic_and_the_library_accepts_every_case(op):
    sizes = (lib.mesh_scratch_bytes, lib.mesh_indexed_scratch_bytes, lib.components_scratch_bytes, lib.distance_transform_scratch_bytes,
             geodesic.scratch_bytes, LB.mesh_scratch_bytes, LB.mesh_indexed_scratch_bytes)
    for seed in SEEDS:
        case = Z.draw(op, seed)
        assert case == Z.draw(op, seed) and repr(case) == repr(Z.draw(op, seed)), (op, seed)
        assert np.array_equal(Z.volume(case), Z.volume(case))
        (w, h, d), box, p = case["extent"], Z.whole_box(case), case["params"]
        assert w * h * d <= Z.MAX_VOLUME and (case["box"] is None or box[3] * box[4] * box[5] <= Z.MAX_BOX), case
        assert all(n >= 1 and x0 >= 0 and x0 + n <= e for x0, n, e in zip(box[:3], box[3:], case["extent"])), case
        e, abox = abi.Extent3D(w, h, d), None if case["box"] is None else abi.Box(*case["box"])
        for scratch_bytes in sizes:
            assert scratch_bytes(e, abox) > 0, (scratch_bytes.__name__, case)
        terms = [wa * (n - 1) for wa, n in zip(p["weights"], box[3:])]
        assert min(p["weights"]) >= 1 and max(terms) <= 65535 and sum(t * t for t in terms) <= 0xfffffffe, case
        assert p["lo"] <= p["hi"] and 0 <= p["fill"] <= 255 and p["connectivity"] in (6, 14, 26) and 1 <= p["rounds"] <= abi.GEODESIC_MAX_ROUNDS, case
        assert max(p["steps"]) <= 65535 and any(p["steps"]), case
        if p["me"] is not None:
            assert all(1 <= m <= n for m, n in zip(p["me"], case["extent"])), case
            if Z.OPS[op][2] == "writes" and case["box"] is not None:        # a rebuilt cell holds a voxel: what a box rebuilds past the volume is not stated
                assert all((m - 1) * b < n for m, b, n in zip(p["me"], Z.blocks_of(case), case["extent"])), case
        assert 0 <= Z.offset_of(case, "d_volume") <= 15 and case["guard"] in Z.GUARDS


def test_other_seeds_give_other_cases():
    assert Z.draw("mesh", 0) != Z.draw("mesh", 1) and Z.draw("mesh", 0)["params"] != Z.draw("nearest", 0)["params"]


# ---- (b) coverage of the default seeds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", BOXED)
def test_the_default_seeds_cover_every_class(op):
    cases = [built(op, seed)[0] for seed in SEEDS]
    boxed = [c for c in cases if c["box"] is not None]
    assert len(boxed) < len(cases), "no case without a box"
    for axis in range(3):
        assert {c["box_classes"][axis] for c in boxed} == set(Z.BOX_CLASSES), (op, "xyz"[axis])
    assert {c["box"][0] % 4 for c in boxed} == {0, 1, 2, 3}, op
    widths = [Z.whole_box(c)[3] for c in cases]
    assert min(widths) < 4 and any(4 <= w <= 64 for w in widths) and any(w > 256 for w in widths) and any(w > 512 for w in [c["extent"][0] for c in cases]), (op, widths)
    assert any(Z.whole_box(c)[4] >= 5 for c in cases) and any(Z.whole_box(c)[5] >= 19 for c in cases), (op, "two tiles in y and in z")
    assert any(c["threshold"] == 256 for c in cases), (op, "threshold 256")
    assert any(c["threshold"] < 256 and (FB.crop(built(op, c["seed"])[1], Z.whole_box(c)) == c["threshold"]).any() for c in cases), (op, "a voxel at the threshold byte")
    for name in ("cap", "cap_vertices"):
        assert {c["caps"][name][0] for c in cases} == set(Z.CAPACITIES), (op, name)
    if Z.OPS[op][2] == "reads":
        assert {c["map_class"] for c in cases} == set(Z.MAPS), op
    assert {c["params"]["connectivity"] for c in cases} == set(Z.CONNECTIVITIES) and {c["params"]["target"] for c in cases} == set(Z.TARGETS), op
    assert {c["limit_class"] for c in cases} == set(Z.LIMITS) and {c["weights_class"] for c in cases} == set(Z.WEIGHTS), op
    assert {c["contents"] for c in cases} >= set(Z.CONTENTS) - {"uniform"} and {c["contents"] for c in cases} & {"inside", "outside"}, op
    assert {c["iso_class"] for c in cases} >= set(Z.ISOS) - {"low_edge"}, op
    assert {c["guard"] for c in cases} == set(Z.GUARDS) and {c["params"]["rounds"] for c in cases} == set(Z.ROUNDS), op
    assert {c["params"]["in_place"] for c in cases} == {False, True} and {c["params"]["mode"] for c in cases} == set(Z.HISTOGRAM_MODES), op
    assert {c["params"]["keep"] for c in cases} == set(Z.TABLE_MODES) == {c["params"]["colors"] for c in cases}, op


# ---- (c) independent statements agree on the drawn cases ---------------------------------------------------------------------------------------
def same(a, b):
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.astype(x.dtype).tobytes() for x, y in zip(a, b))


def small(case, most):
    box = Z.whole_box(case)
    return box[3] * box[4] * box[5] <= most


@pytest.mark.parametrize("seed", SEEDS)
def test_the_independent_statements_agree(seed):
    from scipy import ndimage
    done = 0
    case, vol, aux, want = built("distance", seed)
    box, p = Z.whole_box(case), case["params"]
    if small(case, 3000):
        for target, limit in p["calls"]:
            if limit != 0:
                assert same(edt2_np(vol, p["iso"], target, limit, box), edt2_brute_np(vol, p["iso"], target, limit, box)), case
                done += 1
    case, vol, aux, want = built("nearest", seed)
    box, p = Z.whole_box(case), case["params"]
    if small(case, 3000) and p["limit"] != 0:
        assert same(nearest_separable_np(vol, p["iso"], p["weights"], p["target"], p["limit"], box), nearest_brute_np(vol, p["iso"], p["weights"], p["target"], p["limit"], box)), case
        done += 1
    case, vol, aux, want = built("mesh", seed)
    if small(case, 1500):
        assert same(mesh_np(vol, case["params"]["iso"], Z.whole_box(case)), mesh_loop(vol, case["params"]["iso"], Z.whole_box(case))), case
        done += 1
    case, vol, aux, want = built("label_mesh", seed)
    if small(case, 1500):
        colors, box = aux["colors"] if case["params"]["table"] else None, Z.whole_box(case)
        assert same(label_mesh_np(aux["labels"], colors, vol, case["params"]["iso"], box), label_mesh_loop(aux["labels"], colors, vol, case["params"]["iso"], box)), case
        done += 1
    case, vol, aux, want = built("geodesic", seed)
    box, p = Z.whole_box(case), case["params"]
    if small(case, 3000) and p["limit"] != 0:
        assert same(geodesic_sweeps_np(vol, p["iso"], aux["seeds"], p["steps"], p["limit"], box), geodesic_brute_np(vol, p["iso"], aux["seeds"], p["steps"], p["limit"], box)), case
        done += 1
    case, vol, aux, want = built("components", seed)
    p = case["params"]
    if p["connectivity"] in (6, 26):
        labels, k = ndimage.label(inside_np(vol, p["iso"], Z.whole_box(case)), structure=ndimage.generate_binary_structure(3, {6: 1, 26: 3}[p["connectivity"]]))
        assert same(want["labels"], labels) and int(want["counts"][0]) == k, case
        done += 1
    case, vol, aux, want = built("chain_split", seed)
    p = case["params"]
    if p["connectivity"] in (6, 26) and 0 < case["threshold"] < 256 and p["erode_fill"] < case["threshold"]:
        labels, k = split_bodies_np(FB.crop(vol, Z.whole_box(case)), p["iso"], p["r2"], p["connectivity"])
        assert same(want["out"], labels) and int(want["counts"][0]) == k, case
        done += 1
    assert done or seed % 6 == 5, "nothing was compared"        # the seeds without a box have the largest boxes


# ---- (d) mutants ------------------------------------------------------------------------------------------------------------------------------
def differs(a, b):
    """two references differ in what tests/test_gpu_box_ops_fuzz.py compares: the outputs, and the capacities it passes"""
    return a.keys() != b.keys() or any((a[k] != b[k]) if not isinstance(a[k], np.ndarray) else
                                       (a[k].shape != np.asarray(b[k]).shape or a[k].tobytes() != np.asarray(b[k]).astype(a[k].dtype).tobytes()) for k in a)


def with_parameters(**changed):
    """the reference with some parameters replaced; a value may be a function of the case"""
    def mutant(case, vol, aux, want):
        params = {k: v(case) if callable(v) else v for k, v in changed.items()}
        return Z.reference(dict(case, params=dict(case["params"], **params)), vol, aux)
    return mutant


def with_statements(**replaced):
    """the reference with some of the numpy statements that tests/test_far_boxes_cpu.py calls replaced"""
    def mutant(case, vol, aux, want):
        saved = {name: getattr(FB, name) for name in replaced}
        try:
            for name, f in replaced.items():
                setattr(FB, name, f(saved[name]))
            return Z.reference(case, vol, aux)
        finally:
            for name, f in saved.items():
                setattr(FB, name, f)
    return mutant


def next_up(case):
    return float(np.nextafter(F(case["params"]["iso"]), F(np.inf)))        # f > iso is f >= the next float


def filter_clamped_to_the_box(statement):
    return lambda case, vol, aux, want: {"dst": statement(FB.crop(vol, Z.whole_box(case)))}


def relative_to_the_box(names):
    def mutant(case, vol, aux, want):
        out = dict(want)
        for name in names:
            out[name] = (want[name].reshape(-1, 3) - np.array(Z.whole_box(case)[:3], np.float32)).reshape(want[name].shape)
        return out
    return mutant


def cube_of(tri):
    """the cube a triangle of the list comes from, near enough: the floor of its smallest coordinates"""
    return np.floor(tri.reshape(len(tri), 3, 3).min(axis=1)).astype(np.int64)


def whole_entries_only(case, vol, aux, want):
    """the capacity cut drops the cube that does not fit whole, instead of stopping at the triangle"""
    full = mesh_np(vol, case["params"]["iso"], Z.whole_box(case))
    n = int(want["counts"][1])
    if n == 0 or n == len(full) or not np.array_equal(cube_of(full[n - 1:n]), cube_of(full[n:n + 1])):
        return want
    keep = n - int((cube_of(full[:n]) == cube_of(full[n:n + 1])).all(axis=1)[::-1].cumprod().sum())
    return dict(want, triangles=full[:keep], counts=np.array([len(full), keep], np.uint64))


def normals_clamped_to_the_box(case, vol, aux, want):
    box = Z.whole_box(case)
    return Z.reference(case, FB.crop(vol, box), aux) if case["box"] is None else dict(
        want, normals=FB.ref_mesh_indexed(FB.crop(vol, box), (0, 0, 0) + box[3:], box[:3], aux, None, **Z.parameters(case))["normals"])


def voxels_rule_on_a_thin_box(case, vol, aux, want):
    """a box one voxel thick owns the crossing edges that lie in it, where the header says that it has none"""
    box = Z.whole_box(case)
    if min(box[3:]) > 1:
        return want
    inside = inside_np(vol, case["params"]["iso"], box)
    edges = sum(int((inside[:inside.shape[0] - dz, :inside.shape[1] - dy, :inside.shape[2] - dx] != inside[dz:, dy:, dx:]).sum())
                for dz in (0, 1) for dy in (0, 1) for dx in (0, 1) if (dz, dy, dx) != (0, 0, 0) and dz < inside.shape[0] and dy < inside.shape[1] and dx < inside.shape[2])
    counts = want["counts"].copy()
    counts[2], counts[3] = edges, min(edges, want["_cap1"])
    return dict(want, counts=counts)


def ranked_by_size(components):
    def statement(vol, iso, connectivity=6, box=None, capacity=None):
        labels, sizes, counts = components(vol, iso, connectivity, box, capacity)
        order = np.argsort(-np.bincount(labels.reshape(-1), minlength=int(counts[0]) + 1)[1:].astype(np.int64), kind="stable")
        rank = np.zeros(int(counts[0]) + 1, np.uint32)
        rank[order + 1] = np.arange(1, int(counts[0]) + 1)
        return rank[labels], sizes, counts
    return statement


def sizes_not_cut(case, vol, aux, want):
    p = case["params"]
    return dict(want, sizes=components_np(vol, p["iso"], p["connectivity"], Z.whole_box(case))[1])


def stats_relative_to_the_box(case, vol, aux, want):
    box = Z.whole_box(case)
    return FB.ref_component_stats(FB.crop(vol, box), (0, 0, 0) + box[3:], (0, 0, 0), aux, None, **Z.parameters(case))


def a_record_at_the_capacity(case, vol, aux, want):
    k, cap = int(aux["counts"][0]), want["_cap0"]
    rec = component_stats_np(vol, aux["labels"], k, cap + 1, Z.whole_box(case))
    return dict(want, records=np.frombuffer(rec.tobytes(), np.uint8).copy())


def limit_included(case):
    limit = case["params"]["limit"]
    return limit + 1 if limit else limit


def nearest_limit_included(case, vol, aux, want):
    """D(v) <= limit still names a target, where the header asks D(v) < limit; the distances are the same"""
    p = case["params"]
    if not p["limit"]:
        return want
    return dict(want, nearest=nearest_separable_np(vol, p["iso"], p["weights"], p["target"], p["limit"] + 1, Z.whole_box(case))[0])


def the_largest_index_of_equals(case, vol, aux, want):
    p, box = case["params"], Z.whole_box(case)
    if p["limit"] == 0:
        return want
    flipped = np.ascontiguousarray(FB.crop(vol, box)[::-1, ::-1, ::-1])
    nearest, _ = nearest_separable_np(flipped, p["iso"], p["weights"][:3], p["target"], p["limit"])
    nearest = nearest[::-1, ::-1, ::-1]
    return dict(want, nearest=np.where(nearest == abi.NEAREST_NONE, nearest, np.uint32(nearest.size - 1) - nearest).astype(np.uint32))


def outside_beyond_the_box(case, vol, aux, want):
    """TO_OUTSIDE as the distance to the complement of the inside voxels in all of space: what lies beyond the box counts as outside"""
    p, box = case["params"], Z.whole_box(case)
    if case["threshold"] == 0:
        return want
    padded = np.pad(FB.crop(vol, box), 1, constant_values=0)
    out = dict(want)
    for target, limit in p["calls"]:
        if target == TO_OUTSIDE and limit != 0:
            out["to %d limit %s" % (target, limit)] = np.ascontiguousarray(edt2_np(padded, p["iso"], target, limit)[1:-1, 1:-1, 1:-1])
    return out


def one_round_too_few(case, vol, aux, want):
    """the state one round before the first that holds the fixed point, reported as settled"""
    p, box = case["params"], Z.whole_box(case)
    if p["limit"] == 0 or not small(case, 20000):
        return want
    state, before = None, None
    for _ in range(200):
        dist, labels, info = geodesic_rounds_np(vol, p["iso"], aux["seeds"], p["steps"], p["limit"], box, rounds=1, state=state)
        if same(dist, want["dist"]) and same(labels, want["labels"]):
            break
        state, before = info["state"], (dist, labels)
    return want if before is None else dict(want, dist=before[0], labels=before[1], counts=np.array([1, int((before[0] != abi.GEODESIC_NONE).sum())], np.uint64))


def cells_without_the_overlap(case, vol, aux, want):
    """the map holds each cell's own largest voxel, without the voxel of overlap into the next cell: the cubes whose origin lies in a cell
    below the threshold are skipped, though a corner in the next cell is inside"""
    me, box, iso = case["params"]["me"], Z.whole_box(case), case["params"]["iso"]
    full = mesh_np(vol, iso, box)
    if me is None or not len(full) or case["threshold"] == 256:
        return want
    d, h, w = vol.shape
    blocks = Z.blocks_of(case)
    pad = np.zeros((me[2] * blocks[2], me[1] * blocks[1], me[0] * blocks[0]), np.uint8)
    pad[:d, :h, :w] = vol
    own = pad.reshape(me[2], blocks[2], me[1], blocks[1], me[0], blocks[0]).max(axis=(1, 3, 5))
    o = np.minimum(cube_of(full), np.array([box[0] + box[3] - 2, box[1] + box[4] - 2, box[2] + box[5] - 2]))
    kept = full[own[o[:, 2] // blocks[2], o[:, 1] // blocks[1], o[:, 0] // blocks[0]] >= case["threshold"]]
    cap = want["_cap0"]
    return dict(want, triangles=kept[:cap], counts=np.array([len(kept), min(len(kept), cap)], np.uint64))


def fill_outside_the_box(case, vol, aux, want):
    """the fill also lands on the byte after the box's last voxel, where the buffer has one: the GPU module asks that every byte of the output
    outside the box keeps what it held (the pre-fill; in place, the volume's byte), so the mutant shows where that differs from the fill"""
    x0, y0, z0, w, h, d = Z.whole_box(case)
    i = ((z0 + d - 1) * vol.shape[1] + y0 + h - 1) * vol.shape[2] + x0 + w
    if i >= vol.size:
        return want
    held = int(vol.reshape(-1)[i]) if case["params"]["in_place"] else case["prefill"]
    return want if held == case["params"]["fill"] else dict(want, _outside=(i, case["params"]["fill"]))


# name: (the operations it applies to, the mutant: f(case, vol, aux, want) -> another reference)
MUTANTS = {
    "filters clamp at the box's faces": (("filter_binomial", "filter_median"), None),
    "inside is > at the threshold byte": (("components", "distance", "propagate_masked", "mesh"), with_parameters(iso=next_up, calls=lambda c: c["params"]["calls"])),
    "mesh coordinates relative to the box": (("mesh", "label_mesh"), relative_to_the_box(("triangles",))),
    "indexed mesh coordinates relative to the box": (("mesh_indexed", "label_mesh_indexed"), relative_to_the_box(("vertices",))),
    "a capacity cut drops the whole entry": (("mesh",), whole_entries_only),
    "indexed normals clamped to the box": (("mesh_indexed",), normals_clamped_to_the_box),
    "the voxels rule on a box one voxel thick": (("mesh_indexed",), voxels_rule_on_a_thin_box),
    "26-connectivity where 14 or 6 was asked": (("components",), with_parameters(connectivity=26)),
    "components ranked by size": (("components",), with_statements(components_np=ranked_by_size)),
    "sizes not cut at the capacity": (("components",), sizes_not_cut),
    "stats coordinates relative to the box": (("component_stats",), stats_relative_to_the_box),
    "a record written at index capacity": (("component_stats",), a_record_at_the_capacity),
    "limit compared with <= for the nearest target": (("nearest",), nearest_limit_included),
    "limit compared with <= for the geodesic reach": (("geodesic",), with_parameters(limit=limit_included)),
    "unweighted on one axis": (("distance_weighted", "nearest"), with_parameters(weights=lambda c: c["params"]["weights"][:2] + (1,))),
    "the largest index of equally near targets": (("nearest",), the_largest_index_of_equals),
    "TO_OUTSIDE counts what lies beyond the box": (("distance",), outside_beyond_the_box),
    "geodesic: one round too few reported as settled": (("geodesic",), one_round_too_few),
    "map cells without the one-voxel overlap": (("mesh",), cells_without_the_overlap),
    "select fills outside the box": (("select_components", "select_by_table", "select_by_distance"), fill_outside_the_box),
}


def mutant_of(name, op):
    ops, mutant = MUTANTS[name]
    if mutant is None:
        mutant = filter_clamped_to_the_box({"filter_binomial": binomial3_np, "filter_median": median3_np}[op])
    return mutant


def killers(name, op):
    """the default seeds at which the mutant's result differs from the true statement's"""
    out = []
    for seed in SEEDS:
        case, vol, aux, want = built(op, seed)
        if differs(want, mutant_of(name, op)(case, vol, aux, want)):
            out.append(seed)
    return out


@pytest.mark.parametrize("name,op", [(name, op) for name, (ops, _) in MUTANTS.items() for op in ops], ids=lambda v: v.replace(" ", "_"))
def test_a_default_seed_tells_the_mutant_from_the_statement(name, op):
    seeds = killers(name, op)
    print("%s, %s: seeds %s" % (name, op, seeds))
    assert seeds, "no default seed of %s distinguishes the mutant '%s'" % (op, name)

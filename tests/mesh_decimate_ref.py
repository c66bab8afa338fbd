"""The definition of vkv_mesh_decimate (include/vkvolume_amd.h) restated in numpy: the cell rule in float32, the cells that
surviving faces name through np.unique, and a cell's sum as np.add.at on Python integers of q(x) = rint(x * 2^24), so no width can bind.
tests/test_mesh_decimate_cpu.py holds it to a second, sort-based statement and to the properties the issue names; tests/test_gpu_mesh_decimate.py
holds the kernels to it bit for bit.  The meshes both files use are built here, once."""
import functools

import numpy as np

from tests import mesh_smooth_ref as R

NONE = 0xffffffff
CELLS = (2.0, 3.0, (2.0, 3.0, 5.0))        # the cell sizes of both test files


def grid_of(origin, cell, grid):
    """(origin float32 [3], cell float32 [3], counts int [3])"""
    return (np.asarray(origin, np.float32).reshape(3), np.broadcast_to(np.asarray(cell, np.float32), (3,)).copy(), tuple(int(n) for n in grid))


def cells_np(vertices, origin, cell, grid):
    """the cell id of every vertex, int64: per axis u = (p - origin) / cell in float32, c = u >= 0 ? (u < (float) n ? (uint32) u : n - 1) : 0"""
    origin, cell, grid = grid_of(origin, cell, grid)
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = p - origin
        u = d / cell
    assert d.dtype == np.float32 and u.dtype == np.float32
    n = np.array(grid, np.int64)
    nf = np.array(grid, np.uint64).astype(np.float32)
    with np.errstate(all="ignore"):
        inside = (u >= 0) & (u < nf)
        c = np.where(u >= 0, np.where(u < nf, np.where(inside, u, 0).astype(np.int64), n - 1), 0)
    return c[:, 0] + n[0] * (c[:, 1] + n[1] * c[:, 2])


def mean_np(total, k):
    """(float) ((double) S / (double) k * 2^-24) for arrays of Python integers S and counts k"""
    return (np.asarray(total, object).astype(np.float64) / np.asarray(k, np.float64) * (1.0 / R.FIX)).astype(np.float32)


def decimate_np(vertices, faces, origin, cell, grid, counts=None, face_labels=None, capacity_vertices=None, capacity_triangles=None):
    """The whole answer, before any output capacity: a dict of ``vertices`` [V, 3] float32, ``faces`` [T, 3] int64 (the full numbering),
    ``labels`` [T] or None, ``vertex_map`` [nv] uint32 and ``kept`` (the surviving faces' input numbers).  d_out_counts is [T, min(T,
    capacity), V, min(V, capacity)], and a short capacity keeps a prefix of each list."""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    f_all = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    nv, nt = R.bounds(len(p), len(f_all), counts, capacity_vertices, capacity_triangles)
    cell_of = cells_np(p[:nv], origin, cell, grid)
    f, number = R.used_faces(f_all, nv, nt)
    fc = cell_of[f] if len(f) else np.zeros((0, 3), np.int64)
    keep = (fc[:, 0] != fc[:, 1]) & (fc[:, 1] != fc[:, 2]) & (fc[:, 0] != fc[:, 2])
    named = np.unique(fc[keep])        # rising cell id
    new_faces = np.searchsorted(named, fc[keep])
    # every vertex below nv counts in its cell's mean, used by a face or not
    at = np.searchsorted(named, cell_of)
    at_safe = np.minimum(at, max(len(named) - 1, 0))
    in_named = (at < len(named)) & (named[at_safe] == cell_of) if len(named) else np.zeros(nv, bool)
    total = np.zeros((len(named), 3), object)
    total[...] = 0
    k = np.zeros(len(named), np.int64)
    with np.errstate(all="ignore"):        # a non-finite position: its cell's mean is unspecified
        q = R.q(p[:nv]).astype(object)
    np.add.at(total, at[in_named], q[in_named])
    np.add.at(k, at[in_named], 1)
    return {
        "vertices": mean_np(total, k[:, None]) if len(named) else np.zeros((0, 3), np.float32),
        "faces": new_faces.reshape(-1, 3).astype(np.int64),
        "labels": None if face_labels is None else np.asarray(face_labels).reshape(-1)[number[keep]].astype(np.uint32),
        "vertex_map": np.where(in_named, at_safe, NONE).astype(np.uint32),
        "kept": number[keep],
    }


def directed_edge_balance(faces):
    """{(a, b): occurrences of a -> b minus those of b -> a} without the zero entries: empty iff every directed edge is met as often as its
    reverse"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    balance = {}
    for a, b in e.tolist():
        if a == b:
            continue
        key, sign = ((a, b), 1) if a < b else ((b, a), -1)
        balance[key] = balance.get(key, 0) + sign
    return {k: v for k, v in balance.items() if v}


def grid_for(vertices, cell):
    """cluster_grid's rule for the integer box about the vertices: origin lo - 0.25, cells up to hi + 0.25 at the least"""
    p = np.asarray(vertices, np.float64).reshape(-1, 3)
    lo, hi = np.floor(p.min(axis=0)), np.ceil(p.max(axis=0))
    cell = np.broadcast_to(np.asarray(cell, np.float64), (3,))
    return (lo - 0.25).astype(np.float32), cell.astype(np.float32), tuple(int(max(1, np.ceil((h - l + 0.25) / c))) for l, h, c in zip(lo, hi, cell))


# ---- the meshes of both test files ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ball():
    """(vertices, faces int64, face labels) of one closed ball, radius 9 in 24^3, wholly inside its box: label_indexed_np() at midpoints"""
    from tests.test_label_mesh_indexed_cpu import label_indexed_np
    vertices, _, _, faces, face_labels = label_indexed_np(R.split_ball_labels(cut=0))
    for a in (vertices, faces, face_labels):
        a.setflags(write=False)
    return vertices, faces, face_labels


def fan(n, spread):
    """a fan of n triangles about vertex 0: the hub at (9, 9, 9), the rim's n vertices on a short arc within `spread` of (1, 1, 1), so that
    for a cell size above `spread` all rim vertices share one cell and every face collapses, and for a small one runs of them do"""
    t = np.linspace(0.0, 1.0, n)
    rim = np.stack([1 + spread * t, 1 + spread * t * t, 1 + spread * np.sqrt(t)], axis=1)
    vertices = np.concatenate([np.array([[9.0, 9.0, 9.0]]), rim]).astype(np.float32)
    faces = np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1)
    return vertices, faces

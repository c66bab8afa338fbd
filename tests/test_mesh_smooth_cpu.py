"""What can be shown of vkv_mesh_adjacency, vkv_mesh_smooth and vkv_mesh_vertex_normals (include/vkvolume_amd.h) without a
GPU.  The numpy restatement of tests/mesh_smooth_ref.py (edges -> np.unique -> np.add.at on int64) is held to a second statement through
scipy.sparse matrices; its results do not depend on the order of the faces, and a face repeated with reversed winding changes nothing; on a
radius-9 ball split into two labels Taubin smoothing keeps each body's volume better than Laplacian smoothing, both lower the spread of the
free surface's radii, and the bodies keep naming one row per interface vertex; over all faces an interior interface vertex has the normal
zero and per label two exact negatives; the entry points are declared, exported and bound; the scratch-byte formula is the header's; a null
context is rejected; the kernels of mesh_smooth.hip use no scratch memory.  tests/test_gpu_mesh_smooth.py holds the kernels to the
restatement bit for bit.

No context exists without a device, so of the rejections only the null context can be asked here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import helpers as T
from tests import mesh_smooth_ref as R
from vkvolume_amd import abi, lib, mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAUBIN = R.taubin(0.5, -0.53, 10)
LAPLACE = np.full(10, 0.5, np.float32)


def same_u32(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.flatnonzero(a.view(np.uint32).reshape(-1) != b.view(np.uint32).reshape(-1))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %d: %r != %r" % (what, len(bad), a.size, bad[0], a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


# ---- the second statement ------------------------------------------------------------------------------------------------------------------
def sparse_smooth(vertices, faces, factors, nv=None, nt=None, pinned=None):
    """the adjacency as a 0 / 1 scipy.sparse matrix without a diagonal; a pass is one integer matrix product"""
    p = np.array(vertices, np.float32, copy=True)
    nv, nt = len(p) if nv is None else nv, len(faces) if nt is None else nt
    f = np.asarray(faces, np.int64)[:nt]
    f = f[(f < nv).all(axis=1)]
    rows = np.concatenate([f[:, a] for a in range(3) for b in range(3) if a != b])
    cols = np.concatenate([f[:, b] for a in range(3) for b in range(3) if a != b])
    A = sp.coo_matrix((np.ones(len(rows), np.int64), (rows, cols)), shape=(nv, nv)).tocsr()
    A.setdiag(0)
    A.eliminate_zeros()
    A.data[:] = 1
    k = np.asarray(A.sum(axis=1)).reshape(-1)
    move = (k > 0) if pinned is None else (k > 0) & (np.asarray(pinned)[:nv] == 0)
    for factor in np.asarray(factors, np.float32):
        S = A @ np.rint(p[:nv].astype(np.float64) * 2.0 ** 24).astype(np.int64)
        assert S.dtype == np.int64
        for v in np.flatnonzero(move):
            for c in range(3):
                m = np.float32(float(S[v, c]) / float(k[v]) * 2.0 ** -24)
                p[v, c] = np.float32(p[v, c] + np.float32(factor * np.float32(m - p[v, c])))
    return p, k


def sparse_normals(vertices, faces, face_labels=None, label=0):
    p = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64)
    if face_labels is not None:
        f = f[np.asarray(face_labels) == label]
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])        # float32 in, float32 out: numpy's cross is products and differences
    assert n.dtype == np.float32
    B = sp.coo_matrix((np.ones(3 * len(f), np.int64), (f.reshape(-1), np.repeat(np.arange(len(f)), 3))), shape=(len(p), len(f))).tocsr()
    S = B @ np.rint(n.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    return (S.astype(np.float64) * 2.0 ** -24).astype(np.float32)


@pytest.mark.parametrize("name", sorted(R.small_meshes()))
def test_restatement_against_sparse_matrices_on_the_small_meshes(name):
    vertices, faces = R.small_meshes()[name]
    for factors in ([], [0.5], [0.5, -0.53], TAUBIN[:5]):
        want, k = sparse_smooth(vertices, faces, factors)
        same_u32(R.smooth_np(vertices, faces, factors), want, "%s, %d passes" % (name, len(factors)))
    pairs = R.neighbour_pairs(faces, len(vertices), len(faces))
    assert np.array_equal(np.bincount(pairs[:, 0], minlength=len(vertices)), k)
    same_u32(R.vertex_normals_np(vertices, faces), sparse_normals(vertices, faces), name + ": normals")
    if name == "isolated vertex":
        assert k[4] == 0 and np.array_equal(R.smooth_np(vertices, faces, TAUBIN)[4], vertices[4])
        assert not R.vertex_normals_np(vertices, faces)[4].any()
    if name == "fan of 100":
        assert k[0] == 100 and (k[1:] == 3).all()
    if name == "three faces on one edge":
        assert k.tolist() == [4, 4, 2, 2, 2]
    if name == "degenerate faces":
        assert k.tolist() == [2, 2, 3, 1]        # (0, 0, 1) links 0 and 1 once, (2, 3, 3) links 2 and 3


def test_restatement_against_sparse_matrices_on_the_split_ball():
    vertices, pairs, faces, face_labels, _ = R.extracted("split ball")
    assert (len(vertices), len(faces)) == (5573, 13064)
    want, k = sparse_smooth(vertices, faces, TAUBIN[:3])
    assert (k.min(), k.max()) == (4, 11)
    same_u32(R.smooth_np(vertices, faces, TAUBIN[:3]), want, "three passes")
    for labels, label in ((None, 0), (face_labels, 1), (face_labels, 2)):
        same_u32(R.vertex_normals_np(want, faces, labels, label), sparse_normals(want, faces, labels, label), "normals, label %d" % label)


def test_counts_and_capacities_decide_the_used_faces():
    vertices, _, faces, _, _ = R.extracted("junction")
    nv, nt = len(vertices) - 300, len(faces) - 500
    counts = [len(faces), nt, len(vertices), nv]
    assert (faces[:nt] >= nv).any()        # some of the faces kept name a vertex that was cut: they are not used
    got = R.smooth_np(vertices, faces, TAUBIN[:2], counts=counts)
    same_u32(got[:nv], sparse_smooth(vertices, faces, TAUBIN[:2], nv, nt)[0][:nv], "truncated")
    same_u32(got[nv:], vertices[nv:], "rows past nv")
    assert len(R.vertex_normals_np(vertices, faces, counts=counts)) == nv
    # capacities below the counts: the capacities win
    assert np.array_equal(R.smooth_np(vertices, faces, TAUBIN[:2], counts=[len(faces), len(faces), len(vertices), len(vertices)], capacity_vertices=nv,
                                      capacity_triangles=nt).view(np.uint32), got.view(np.uint32))


# ---- order and repetition --------------------------------------------------------------------------------------------------------------
def test_the_order_of_the_faces_does_not_matter():
    vertices, _, faces, face_labels, _ = R.extracted("split ball")
    want = R.smooth_np(vertices, faces, TAUBIN)
    normals = [R.vertex_normals_np(want, faces, face_labels, L) for L in (1, 2)]
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(faces))
        rolled = np.stack([np.roll(f, s) for f, s in zip(faces[order], np.random.default_rng(seed).integers(0, 3, len(faces)))])
        same_u32(R.smooth_np(vertices, faces[order], TAUBIN), want, "permuted faces")
        same_u32(R.smooth_np(vertices, rolled, TAUBIN), want, "permuted faces, rotated corners")
        for L in (1, 2):
            same_u32(R.vertex_normals_np(want, faces[order], face_labels[order], L), normals[L - 1], "normals of permuted faces")


def test_a_face_repeated_with_reversed_winding_changes_nothing():
    vertices, _, faces, _, _ = R.extracted("junction")
    want = R.smooth_np(vertices, faces, TAUBIN[:4])
    more = np.concatenate([faces, faces[::7, ::-1], faces[::11]])
    same_u32(R.smooth_np(vertices, more, TAUBIN[:4]), want, "repeated faces")
    # and the label mesh does that by itself: every interface face is there twice
    tri = np.sort(faces, axis=1)
    assert len(np.unique(tri, axis=0)) < len(tri)


# ---- what smoothing is for -------------------------------------------------------------------------------------------------------------
def body_volume(vertices, faces, face_labels, label):
    tri = vertices[faces[face_labels == label]].astype(np.float64)
    return float(np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum() / 6.0)


def test_taubin_keeps_the_volume_and_both_smooth_the_split_ball():
    vertices, pairs, faces, face_labels, labels = R.extracted("split ball")
    free = (pairs == 0).any(axis=1)
    centre = np.full(3, (labels.shape[0] - 1) / 2.0)
    spread = lambda p: float(np.linalg.norm(p[free].astype(np.float64) - centre, axis=1).std())  # noqa: E731
    laplace, taubin = R.smooth_np(vertices, faces, LAPLACE), R.smooth_np(vertices, faces, TAUBIN)
    for L in (1, 2):
        v0, vl, vt = (body_volume(p, faces, face_labels, L) for p in (vertices, laplace, taubin))
        print("label %d: volume %.2f, Laplacian %.2f, Taubin %.2f" % (L, v0, vl, vt))
        assert abs(vt - v0) < abs(vl - v0)
    print("spread of the free surface's radii: %.3f, Laplacian %.3f, Taubin %.3f" % (spread(vertices), spread(laplace), spread(taubin)))
    assert spread(laplace) < spread(vertices) and spread(taubin) < spread(vertices)
    # interface vertices remain single rows: each body's interface faces name the same rows, so the bodies stay closed against each other
    interface = np.flatnonzero((pairs != 0).all(axis=1))
    used = [np.unique(faces[face_labels == L]) for L in (1, 2)]
    assert len(interface) > 900 and set(interface.tolist()) == set(used[0].tolist()) & set(used[1].tolist())
    assert not np.array_equal(taubin[interface], vertices[interface])        # and they did move
    for L in (1, 2):        # closed: every directed edge of the body has its opposite
        f = faces[face_labels == L]
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert set(map(tuple, e.tolist())) == set(map(tuple, e[:, ::-1].tolist()))


def interior_interface(pairs, faces):
    """the interface vertices all of whose neighbours are interface vertices too"""
    interface = (pairs != 0).all(axis=1)
    near = R.neighbour_pairs(faces, len(pairs), len(faces))
    touched = np.zeros(len(pairs), bool)
    np.logical_or.at(touched, near[:, 0], ~interface[near[:, 1]])
    return interface & ~touched


@pytest.mark.parametrize("smoothed", [False, True], ids=["midpoints", "smoothed"])
def test_interface_normals_cancel_over_all_faces_and_oppose_per_label(smoothed):
    vertices, pairs, faces, face_labels, _ = R.extracted("split ball")
    if smoothed:
        vertices = R.smooth_np(vertices, faces, TAUBIN)
    inside = interior_interface(pairs, faces)
    assert inside.sum() > 800
    every = R.vertex_normals_np(vertices, faces)
    one, two = (R.vertex_normals_np(vertices, faces, face_labels, L) for L in (1, 2))
    assert not every[inside].any()
    assert np.array_equal(one[inside], -two[inside]) and (one[inside, 0] > 1).all()        # body 1 lies below the cut at x = 12: its normal is +x
    free = (pairs == 0).any(axis=1)
    assert (np.einsum("ij,ij->i", every[free].astype(np.float64), vertices[free].astype(np.float64) - 11.5) > 0).all()        # outward on the ball


def test_boundary_vertices_finds_the_rim_of_a_body_that_leaves_the_box():
    vertices, _, faces, _, _ = R.extracted("box cut")
    rim = M.boundary_vertices(faces, len(vertices))
    assert rim.dtype == bool and rim.shape == (len(vertices),) and np.array_equal(rim, R.boundary_vertices_np(faces, len(vertices)))
    assert rim.sum() > 20 and (vertices[rim, 0] == 0).all() and not rim[vertices[:, 0] > 0].any()        # the open face x = 0
    for name in ("split ball", "junction"):
        v, _, f, _, _ = R.extracted(name)
        assert not M.boundary_vertices(f, len(v)).any()
    assert M.boundary_vertices(faces, len(vertices) - 100).sum() > rim[:len(vertices) - 100].sum()        # cutting vertices opens the surface
    assert M.boundary_vertices(np.zeros((0, 3), np.int64), 5).tolist() == [False] * 5
    pinned = R.smooth_np(vertices, faces, TAUBIN, pinned=rim)
    assert np.array_equal(pinned[rim], vertices[rim]) and not np.array_equal(R.smooth_np(vertices, faces, TAUBIN)[rim], vertices[rim])


# ---- entry points ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bsize_t\s+vkv_mesh_adjacency_scratch_bytes\s*\(\s*uint64_t capacity_vertices,\s*uint64_t capacity_triangles\)", header)
    assert re.search(r"\bint\s+vkv_mesh_adjacency\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint32_t\s*\*d_indices,\s*uint64_t capacity_triangles,\s*"
                     r"uint64_t capacity_vertices,\s*const uint64_t\s*\*d_counts,\s*void\s*\*d_adjacency,\s*void\s*\*stream\)", header)
    assert re.search(r"\bint\s+vkv_mesh_smooth\s*\(\s*vkv_ctx\s*\*ctx,\s*float\s*\*d_vertices,\s*float\s*\*d_swap,\s*uint64_t capacity_vertices,\s*"
                     r"const uint64_t\s*\*d_counts,\s*const void\s*\*d_adjacency,\s*const uint8_t\s*\*d_pinned,\s*const float\s*\*factors,\s*"
                     r"uint32_t n_passes,\s*void\s*\*stream\)", header)
    assert re.search(r"\bint\s+vkv_mesh_vertex_normals\s*\(\s*vkv_ctx\s*\*ctx,\s*const float\s*\*d_vertices,\s*const uint32_t\s*\*d_indices,\s*"
                     r"const uint32_t\s*\*d_triangle_labels,\s*uint32_t label,\s*uint64_t capacity_vertices,\s*uint64_t capacity_triangles,\s*"
                     r"const uint64_t\s*\*d_counts,\s*const void\s*\*d_adjacency,\s*float\s*\*d_normals,\s*void\s*\*stream\)", header)
    assert "nothing is smoothed" not in header and header.count("vkv_mesh_smooth and") >= 2        # both extractors' blocks point here
    names = ["vkv_mesh_adjacency_scratch_bytes", "vkv_mesh_adjacency", "vkv_mesh_smooth", "vkv_mesh_vertex_normals"]
    L = lib.load()
    assert set(names) <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in names:
        assert re.search(r"\b%s$" % name, out, flags=re.M), name
    assert L.vkv_mesh_adjacency_scratch_bytes.restype is C.c_size_t and L.vkv_mesh_adjacency_scratch_bytes.argtypes == [C.c_uint64, C.c_uint64]
    at = L.vkv_mesh_smooth.argtypes
    assert len(at) == 10 and at[3] is C.c_uint64 and at[7] is C.POINTER(C.c_float) and at[8] is C.c_uint32
    at = L.vkv_mesh_vertex_normals.argtypes
    assert len(at) == 11 and at[4] is C.c_uint32 and at[5] is C.c_uint64 and at[6] is C.c_uint64
    assert len(L.vkv_mesh_adjacency.argtypes) == 7
    for name in ("mesh_adjacency_rc", "mesh_smooth_rc", "mesh_vertex_normals_rc"):
        assert callable(getattr(lib.Context, name))
    for name in ("smooth", "vertex_normals", "boundary_vertices", "build_adjacency", "adjacency_scratch_bytes"):
        assert callable(getattr(M, name))


def test_the_binding_passes_factors_as_a_float_array():
    from tests.test_binding_cpu import HANDLE, context
    ctx, rec = context()
    assert ctx.mesh_smooth_rc(10, 11, 100, 12, 13, None, [0.5, -0.53], 99) == 0
    assert rec.last("vkv_mesh_smooth") == (HANDLE, 10, 11, 100, 12, 13, None, [0.5, C.c_float(-0.53).value], 2, 99)
    ctx.mesh_smooth_rc(10, 11, 100, 12, 13, 14, None)
    assert rec.last("vkv_mesh_smooth") == (HANDLE, 10, 11, 100, 12, 13, 14, None, 0, 0)
    ctx.mesh_smooth_rc(10, 11, 100, 12, 13, 14, (None, 3))
    assert rec.last("vkv_mesh_smooth") == (HANDLE, 10, 11, 100, 12, 13, 14, None, 3, 0)
    ctx.mesh_adjacency_rc(10, 200, 100, 12, 13, 99)
    assert rec.last("vkv_mesh_adjacency") == (HANDLE, 10, 200, 100, 12, 13, 99)
    ctx.mesh_vertex_normals_rc(10, 11, None, 2, 100, 200, 12, 13, 14)
    assert rec.last("vkv_mesh_vertex_normals") == (HANDLE, 10, 11, None, 2, 100, 200, 12, 13, 14, 0)


def test_scratch_bytes_and_the_null_context_without_a_device():
    L = lib.load()
    size = L.vkv_mesh_adjacency_scratch_bytes
    up8 = lambda n: (n + 7) & ~7  # noqa: E731
    for cv, ct in ((0, 0), (1, 0), (0, 1), (1, 1), (3, 5), (4095, 7), (4096, 8), (4097, 9), (5573, 13064), (55_000_000, 110_000_001), (0xffffffff, 0xffffffff)):
        want = 32 + 8 * ((cv + 4095) // 4096) + 3 * up8(4 * cv) + 24 * ct + up8(12 * ct)
        assert size(cv, ct) == want == M.adjacency_scratch_bytes(cv, ct), (cv, ct)
        assert want % 8 == 0 and want >= 32
    assert size(1 << 32, 1) == 0 == M.adjacency_scratch_bytes(1 << 32, 1) and size(1, 1 << 32) == 0 == M.adjacency_scratch_bytes(1, 1 << 32)
    buf = (C.c_uint64 * 64)()
    a = C.addressof(buf)
    bad = abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_mesh_adjacency(None, a, 1, 3, a + 64, a + 128, None) == bad
    assert L.vkv_mesh_smooth(None, a, a + 64, 3, a + 128, a + 192, None, None, 0, None) == bad
    assert L.vkv_mesh_vertex_normals(None, a, a + 64, None, 0, 3, 1, a + 128, a + 192, a + 256, None) == bad
    assert not any(buf)


def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("mesh_smooth.hip", tmp_path / "mesh_smooth.s")
    for name, n in (("k_madj_clear", 1), ("k_madj_faces", 2), ("k_madj_scan", 2), ("k_madj_sort", 1), ("k_msmooth_pass", 1), ("k_msmooth_copy", 1),
                    ("k_mnormals", 2)):
        assert len([k for k in kernels if name in k]) == n, (name, sorted(kernels))
    assert len(kernels) == 10
    for k, v in kernels.items():
        print(k, v)
        assert v.get("ScratchSize") == 0, (k, v)
        assert v.get("NumVgprs") <= 64, (k, v)        # gathers hide their latency behind other waves: full occupancy
    text = open(tmp_path / "mesh_smooth.s").read()
    assert not re.search(r"atomic\w*_f(32|64)|atomic_pk_add", text)        # integer atomics only
    assert not re.search(r"\bv_(fma|fmac|mad|mac)_f32", text)        # the fp32 steps are rounded one by one

"""The definitions of vkv_mesh_adjacency, vkv_mesh_smooth and vkv_mesh_vertex_normals (include/vkvolume_amd.h) restated in
numpy: used faces, the neighbour SET through np.unique of the edges, and every sum as np.add.at on int64 of q(x) = rint(x * 2^24).
tests/test_mesh_smooth_cpu.py holds it to a second statement and to the properties the issue measured; tests/test_gpu_mesh_smooth.py holds the
kernels to it bit for bit.  The test meshes both files use are built here, once."""
import functools

import numpy as np

FIX = float(1 << 24)


def q(x):
    """(int64) rint((double) x * 2^24), half to even"""
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * FIX).astype(np.int64)


def bounds(n_vertices, n_faces, counts=None, capacity_vertices=None, capacity_triangles=None):
    """(nv, nt): min(counts[3], capacity_vertices), min(counts[1], capacity_triangles); a missing one is the array's length"""
    cv = n_vertices if capacity_vertices is None else capacity_vertices
    ct = n_faces if capacity_triangles is None else capacity_triangles
    return (cv, ct) if counts is None else (min(int(counts[3]), cv), min(int(counts[1]), ct))


def used_faces(faces, nv, nt):
    """(the used faces [m, 3] int64, their numbers [m]): the first nt whose three indices are all below nv"""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)[:nt]
    keep = np.flatnonzero((f < nv).all(axis=1))
    return f[keep], keep


def neighbour_pairs(faces, nv, nt):
    """the directed pairs (v, u), u in N(v), each once, sorted by v then u: [e, 2] int64"""
    f, _ = used_faces(faces, nv, nt)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.concatenate([e, e[:, ::-1]])
    e = e[e[:, 0] != e[:, 1]]
    return np.unique(e, axis=0) if len(e) else e.reshape(0, 2)


def smooth_np(vertices, faces, factors, counts=None, pinned=None, capacity_vertices=None, capacity_triangles=None):
    """the vertices after one pass per factor; rows past nv are returned as given"""
    p = np.array(vertices, np.float32, copy=True).reshape(-1, 3)
    nv, nt = bounds(len(p), len(np.asarray(faces).reshape(-1, 3)), counts, capacity_vertices, capacity_triangles)
    pairs = neighbour_pairs(faces, nv, nt)
    k = np.bincount(pairs[:, 0], minlength=max(nv, 1))[:nv]
    move = k > 0
    if pinned is not None:
        move &= np.asarray(pinned).reshape(-1)[:nv] == 0
    for f in np.asarray(factors, np.float32).reshape(-1):
        s = np.zeros((nv, 3), np.int64)
        np.add.at(s, pairs[:, 0], q(p[pairs[:, 1]]))
        with np.errstate(all="ignore"):
            m = (s.astype(np.float64) / k[:, None].astype(np.float64) * (1.0 / FIX)).astype(np.float32)
        d = m - p[:nv]
        g = np.float32(f) * d
        new = p[:nv] + g
        assert new.dtype == np.float32 and g.dtype == np.float32 and d.dtype == np.float32
        p[:nv] = np.where(move[:, None], new, p[:nv])
    return p


def face_normals_np(vertices, faces):
    """e1 x e2 in fp32 per face of `faces` [m, 3]: two rounded products and one subtraction per component"""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    e1, e2 = p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    assert n.dtype == np.float32
    return n


def vertex_normals_np(vertices, faces, face_labels=None, label=0, counts=None, capacity_vertices=None, capacity_triangles=None):
    """[nv, 3] float32: the fixed-point sum of the face normals over each vertex's used faces, of those tagged `label` with face_labels"""
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    nv, nt = bounds(len(p), len(np.asarray(faces).reshape(-1, 3)), counts, capacity_vertices, capacity_triangles)
    f, number = used_faces(faces, nv, nt)
    if face_labels is not None:
        keep = np.asarray(face_labels).reshape(-1)[number] == label
        f = f[keep]
    s = np.zeros((nv, 3), np.int64)
    qn = q(face_normals_np(p, f))
    for c in range(3):
        np.add.at(s, f[:, c], qn)
    return (s.astype(np.float64) * (1.0 / FIX)).astype(np.float32)


def boundary_vertices_np(faces, n_vertices):
    """the vertices on an edge that exactly one face holds (undirected, a face counted once per edge)"""
    f, _ = used_faces(faces, n_vertices, len(np.asarray(faces).reshape(-1, 3)))
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    e = e[e[:, 0] != e[:, 1]]
    edges, n = np.unique(e, axis=0, return_counts=True) if len(e) else (e.reshape(0, 2), np.zeros(0, np.int64))
    mask = np.zeros(n_vertices, bool)
    mask[edges[n == 1].reshape(-1)] = True
    return mask


def taubin(lam, mu, iterations):
    return np.array([lam, mu] * iterations, np.float32)


# ---- the meshes of both test files ---------------------------------------------------------------------------------------------------------
def split_ball_labels(n=24, radius=9.0, cut=12):
    """a ball of `radius` about the centre of n^3 voxels, label 1 where x < cut, else 2"""
    z, y, x = np.indices((n, n, n)).astype(np.float64)
    c = (n - 1) / 2.0
    inside = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= radius * radius
    return np.where(inside, np.where(x < cut, 1, 2), 0).astype(np.uint32)


def junction_labels(n=14):
    """three sectors around the line x = y = 6 in a zero border"""
    z, y, x = np.indices((n, n, n))
    labels = np.where(x < 6, 1, np.where(y < 6, 2, 3)).astype(np.uint32)
    labels[[0, -1]] = 0
    labels[:, [0, -1]] = 0
    labels[:, :, [0, -1]] = 0
    return labels


def box_cut_labels(n=12):
    """one body that leaves the box through its x = 0 face: the extraction leaves it open there"""
    labels = np.zeros((n, n, n), np.uint32)
    labels[3:9, 2:8, 0:7] = 1
    return labels


@functools.lru_cache(maxsize=None)
def extracted(name):
    """(vertices, vertex label pairs, faces int64, face labels, labels) of label_indexed_np() at midpoints for one of the label arrays above"""
    from tests.test_label_mesh_indexed_cpu import label_indexed_np
    labels = {"split ball": split_ball_labels, "junction": junction_labels, "box cut": box_cut_labels}[name]()
    vertices, _, pairs, faces, face_labels = label_indexed_np(labels)
    for a in (vertices, pairs, faces, face_labels, labels):
        a.setflags(write=False)
    return vertices, pairs, faces, face_labels, labels


def small_meshes():
    """{name: (vertices float32 [v, 3], faces int64 [n, 3])}: the hand-made cases"""
    rng = np.random.default_rng(5)
    out = {}
    tet = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) + np.float32(0.3)
    out["tetrahedron"] = (tet, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64))
    out["isolated vertex"] = (np.concatenate([tet, np.array([[5, 6, 7]], np.float32)]), out["tetrahedron"][1])
    out["three faces on one edge"] = (rng.random((5, 3), np.float32) * 4, np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], np.int64))
    out["reversed duplicate"] = (rng.random((4, 3), np.float32) * 4, np.array([[0, 1, 2], [2, 1, 0], [1, 2, 3], [0, 1, 2]], np.int64))
    out["degenerate faces"] = (rng.random((4, 3), np.float32) * 4, np.array([[0, 0, 1], [1, 2, 1], [2, 3, 3], [0, 1, 2]], np.int64))
    for n in (16, 17, 100):        # 16 faces about a vertex are the most the build sorts in LDS; 17 and 100 are sorted where they lie
        angle = np.linspace(0, 2 * np.pi, n + 1)[:-1]
        rim = np.stack([3 * np.cos(angle), 3 * np.sin(angle), 0.2 * np.sin(5 * angle)], axis=1)
        fan = np.concatenate([np.array([[0.1, -0.2, 1.0]]), rim]).astype(np.float32)
        out["fan of %d" % n] = (fan, np.stack([np.zeros(n, np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1))
    return out

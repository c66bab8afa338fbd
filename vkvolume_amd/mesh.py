"""What to do with the triangles of Volume.extract_isosurface / vkv_isosurface_mesh on the host: numpy only, nothing here is pinned to the bit.

``tri`` is always an [n, 3, 3] float32 array (triangle, vertex, xyz) in voxel-index coordinates, voxel centres at integers (a device tensor's
``.cpu().numpy()``).  Triangles wind so that (v1 - v0) x (v2 - v0) points from the inside (f >= iso) to the outside.  The indexed form of
Volume.extract_isosurface_indexed / vkv_isosurface_mesh_indexed is ``vertices`` [v, 3] float32 and ``faces`` [n, 3] of vertex numbers (any
integer type; a torch.uint32 tensor's ``.cpu().numpy()``): unindex() turns it into ``tri``, write_ply() stores it, and the coordinate maps take
a vertex array as well.  Volume.extract_label_mesh / vkv_label_mesh adds ``tri_labels``, one uint32 label per triangle: split_by_label()
groups the triangles by body, body_measures() gives each body's area and volume, and write_ply(face_colors=label_face_colors(...)) stores all
bodies in one coloured file.  Volume.extract_label_mesh_indexed / vkv_label_mesh_indexed gives the bodies as ONE indexed mesh with
``face_labels``, volume normals and ``vertex_labels`` (the two shown labels a vertex separates): body_submesh() cuts one body out,
oriented_corner_normals() turns the normals to each face's side, contact_areas() sums what touches what.
"""
import struct

import numpy as np


def _tri(tri):
    tri = np.ascontiguousarray(tri, np.float32)
    if tri.ndim != 3 or tri.shape[1:] != (3, 3):
        raise ValueError("triangles must have the shape [n, 3, 3], not %s" % (tri.shape,))
    return tri


def _whd(extent):
    if hasattr(extent, "width"):
        return np.array([extent.width, extent.height, extent.depth], np.float32)
    return np.asarray(extent, np.float32).reshape(3)


def _points(p):
    """triangles [n, 3, 3] or vertices [v, 3]"""
    p = np.ascontiguousarray(p, np.float32)
    return p if p.ndim == 2 and p.shape[1] == 3 else _tri(p)


def to_texture(tri, extent):
    """voxel-index coordinates -> texture coordinates ([0, 1]^3 = the volume): (p + 0.5) / extent, ``extent`` = (W, H, D) or an abi.Extent3D;
    ``tri``: triangles [n, 3, 3] or vertices [v, 3]"""
    return (_points(tri) + np.float32(0.5)) / _whd(extent)


def to_model(tri, extent, matrix):
    """voxel-index coordinates -> the space ``matrix`` maps the volume's centred unit cube into: matrix * (texture - 0.5).  ``matrix``: a
    column-major 4 x 4 as vkvolume_amd.camera builds them (memory order m[col][row]), e.g. Volume.image_transform or node * image.
    ``tri``: triangles [n, 3, 3] or vertices [v, 3]."""
    local = to_texture(tri, extent).astype(np.float64) - 0.5
    m = np.asarray(matrix, np.float64).reshape(4, 4)
    return (local @ m[:3, :3] + m[3, :3]).astype(np.float32)


def weld(tri):
    """(vertices [v, 3] float32, faces [n, 3] int64): vertices with the same bit pattern become one (-0.0 and 0.0 differ; the extraction never
    produces -0.0).  Shared vertices of an extracted surface ARE bit-equal, so no tolerance is involved.  Vertices come in order of first use."""
    tri = _tri(tri)
    keys = tri.reshape(-1, 3).view(np.uint32)
    packed = np.ascontiguousarray(keys).view([("", np.uint32)] * 3).reshape(-1)
    _, first, inverse = np.unique(packed, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")        # unique() sorts by value; renumber by first use
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    return tri.reshape(-1, 3)[first[order]].copy(), rank[inverse.reshape(-1)].reshape(-1, 3).astype(np.int64)


def unindex(vertices, faces):
    """the triangle list [n, 3, 3] float32 of an indexed mesh: vertices[faces]"""
    vertices = np.ascontiguousarray(vertices, np.float32)
    faces = np.asarray(faces)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("vertices must have the shape [v, 3] and faces [n, 3], not %s and %s" % (vertices.shape, faces.shape))
    return np.ascontiguousarray(vertices[faces.astype(np.int64)])


def drop_degenerate(tri):
    """the triangles with three bitwise distinct vertices (a voxel whose value equals iso exactly collapses edges onto it)"""
    tri = _tri(tri)
    b = tri.view(np.uint32)
    same = lambda i, j: (b[:, i] == b[:, j]).all(axis=1)  # noqa: E731
    return tri[~(same(0, 1) | same(1, 2) | same(0, 2))]


def face_normals(tri):
    """unit (v1 - v0) x (v2 - v0) per triangle, zeros for a triangle without area"""
    tri = _tri(tri).astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.0), 0.0).astype(np.float32)


def write_stl(path, tri, header=b"vkvolume_amd isosurface"):
    """binary STL: 80 header bytes, uint32 count, per triangle the face normal, three vertices (float32, little endian) and a zero uint16"""
    tri = _tri(tri)
    rec = np.zeros(len(tri), np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["n"], rec["v"] = face_normals(tri), tri
    with open(path, "wb") as f:
        f.write(bytes(header)[:80].ljust(80, b"\0"))
        f.write(struct.pack("<I", len(tri)))
        f.write(rec.tobytes())


def split_by_label(tri, tri_labels):
    """The triangles of Volume.extract_label_mesh / vkv_label_mesh grouped by body: ``(labels, starts, tri_sorted)``.  ``labels``: the
    distinct triangle labels in ascending order; ``tri_sorted``: the triangles sorted by label, stably, so that each body keeps the
    extraction's order; the body ``labels[k]`` is ``tri_sorted[starts[k]:starts[k + 1]]`` (``starts`` has one entry more than ``labels``)."""
    tri = _tri(tri)
    tri_labels = np.asarray(tri_labels).reshape(-1)
    if len(tri_labels) != len(tri):
        raise ValueError("%d labels for %d triangles" % (len(tri_labels), len(tri)))
    order = np.argsort(tri_labels, kind="stable")
    labels, first = np.unique(tri_labels[order], return_index=True)
    return labels, np.append(first, len(tri)).astype(np.int64), np.ascontiguousarray(tri[order])


def body_measures(tri, tri_labels, n_labels):
    """``(area, volume)`` of the bodies 1 .. n_labels, two float64 arrays of n_labels entries (entry L - 1: label L): the sum of the
    triangle areas, and the enclosed volume by the divergence theorem, sum of v0 . (v1 x v2) / 6, which is exact for a closed surface and
    positive for the extraction's winding.  Triangles with label 0 or above n_labels are ignored.  Voxel units: scale by the spacing for
    physical ones."""
    t = _tri(tri).astype(np.float64)
    tri_labels = np.asarray(tri_labels).reshape(-1).astype(np.int64)
    if len(tri_labels) != len(t):
        raise ValueError("%d labels for %d triangles" % (len(tri_labels), len(t)))
    keep = (tri_labels >= 1) & (tri_labels <= int(n_labels))
    t, at = t[keep], tri_labels[keep] - 1
    cross = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    area = np.bincount(at, weights=0.5 * np.linalg.norm(cross, axis=1), minlength=int(n_labels))
    volume = np.bincount(at, weights=np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])) / 6.0, minlength=int(n_labels))
    return area, volume


def _indexed(vertices, faces):
    vertices = np.ascontiguousarray(vertices, np.float32)
    faces = np.asarray(faces)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("vertices must have the shape [v, 3] and faces [n, 3], not %s and %s" % (vertices.shape, faces.shape))
    return vertices, faces.astype(np.int64)


def body_submesh(vertices, faces, face_labels, label, normals=None):
    """One body of Volume.extract_label_mesh_indexed / vkv_label_mesh_indexed as a mesh of its own: ``(vertices, faces, normals)`` with the
    faces tagged ``label`` in their order, the vertices they use compacted in the list's order, the faces renumbered (int64), and the
    normals of those vertices (None without ``normals``).  Interface vertices are copied into every body that uses them."""
    vertices, faces = _indexed(vertices, faces)
    face_labels = np.asarray(face_labels).reshape(-1)
    if len(face_labels) != len(faces):
        raise ValueError("%d labels for %d faces" % (len(face_labels), len(faces)))
    if normals is not None:
        normals = np.ascontiguousarray(normals, np.float32)
        if normals.shape != vertices.shape:
            raise ValueError("normals must have the vertices' shape %s, not %s" % (vertices.shape, normals.shape))
    own = faces[face_labels == label]
    used = np.zeros(len(vertices), bool)
    used[own.reshape(-1)] = True
    number = np.cumsum(used, dtype=np.int64) - 1
    return vertices[used], number[own], None if normals is None else normals[used]


def oriented_corner_normals(vertices, faces, normals):
    """[n, 3, 3] float32, one normal per face corner: the vertex normal, negated where its dot product with the face's (v1 - v0) x (v2 - v0)
    is negative.  The normals of vkv_label_mesh_indexed follow the volume; on an interface between two bodies their sign suits neither, and
    the faces of the two bodies wind against each other: this gives each face the normals on its own side."""
    vertices, faces = _indexed(vertices, faces)
    normals = np.ascontiguousarray(normals, np.float32)
    if normals.shape != vertices.shape:
        raise ValueError("normals must have the vertices' shape %s, not %s" % (vertices.shape, normals.shape))
    tri = vertices[faces].astype(np.float64)
    face = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    corner = normals[faces]
    against = np.einsum("nkc,nc->nk", corner.astype(np.float64), face) < 0
    return np.where(against[:, :, None], -corner, corner).astype(np.float32)


MIXED = 0xffffffff        # contact_areas(): the three vertices of a face do not agree on what lies across


def contact_areas(vertices, faces, face_labels, vertex_labels):
    """What each body touches, from the label pairs of vkv_label_mesh_indexed: ``(across, areas)``.  ``across`` [n] uint32: per face the
    label on its other side, the common other member of its three vertices' pairs (0: nothing, the free surface), or MIXED where they
    differ (a face next to a junction of three bodies).  ``areas``: {(label, across): the summed area of those faces} in voxel units,
    float.  An interface appears twice, as (L, K) from body L's faces and as (K, L) from body K's, with equal areas."""
    vertices, faces = _indexed(vertices, faces)
    face_labels = np.asarray(face_labels).reshape(-1).astype(np.int64)
    pairs = np.asarray(vertex_labels).astype(np.int64)
    if len(face_labels) != len(faces):
        raise ValueError("%d labels for %d faces" % (len(face_labels), len(faces)))
    if pairs.shape != (len(vertices), 2):
        raise ValueError("vertex_labels must have the shape (%d, 2), not %s" % (len(vertices), pairs.shape))
    p = pairs[faces]        # [n, 3, 2]
    own = face_labels[:, None]
    if not ((p[:, :, 0] == own) | (p[:, :, 1] == own)).all():
        raise ValueError("a face's label is missing from a pair of one of its vertices")
    other = np.where(p[:, :, 0] == own, p[:, :, 1], p[:, :, 0])
    across = np.where((other[:, 0] == other[:, 1]) & (other[:, 1] == other[:, 2]), other[:, 0], MIXED)
    tri = vertices[faces].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    keys, inverse = np.unique(np.stack([face_labels, across], axis=1), axis=0, return_inverse=True)
    sums = np.bincount(inverse.reshape(-1), weights=area, minlength=len(keys))
    return across.astype(np.uint32), {(int(k[0]), int(k[1])): float(s) for k, s in zip(keys, sums)}


def label_face_colors(tri_labels, table):
    """[n, 3] uint8 RGB per triangle from a colour table of vkvolume_amd.labels (entry L - 1 for label L); black for a label the table
    does not name"""
    tri_labels = np.asarray(tri_labels).reshape(-1).astype(np.int64)
    table = np.asarray(table, np.uint32).reshape(-1)
    named = (tri_labels >= 1) & (tri_labels <= len(table))
    words = np.where(named, table[np.where(named, tri_labels - 1, 0)] if len(table) else 0, 0).astype(np.uint32)
    return np.stack([words & 255, (words >> 8) & 255, (words >> 16) & 255], axis=1).astype(np.uint8)


def write_ply(path, vertices, faces, normals=None, face_colors=None):
    """binary little-endian PLY: per vertex x y z (and nx ny nz with ``normals`` [v, 3]) as float32, per face a uchar 3 and three uint32
    (and red green blue as uchar with ``face_colors`` [n, 3] uint8, e.g. label_face_colors() of a labels.color_table palette)"""
    vertices = np.ascontiguousarray(vertices, np.float32)
    faces = np.asarray(faces)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3:
        raise ValueError("vertices must have the shape [v, 3] and faces [n, 3], not %s and %s" % (vertices.shape, faces.shape))
    names = ["x", "y", "z"]
    columns = [vertices]
    if normals is not None:
        normals = np.ascontiguousarray(normals, np.float32)
        if normals.shape != vertices.shape:
            raise ValueError("normals must have the vertices' shape %s, not %s" % (vertices.shape, normals.shape))
        names += ["nx", "ny", "nz"]
        columns.append(normals)
    header = ["ply", "format binary_little_endian 1.0", "comment vkvolume_amd isosurface", "element vertex %d" % len(vertices)]
    header += ["property float %s" % n for n in names]
    header += ["element face %d" % len(faces), "property list uchar uint vertex_indices"]
    fields = [("n", "u1"), ("v", "<u4", 3)]
    if face_colors is not None:
        face_colors = np.asarray(face_colors)
        if face_colors.shape != (len(faces), 3) or face_colors.dtype != np.uint8:
            raise ValueError("face_colors must be a uint8 array of shape (%d, 3), not %s %s" % (len(faces), face_colors.dtype, face_colors.shape))
        header += ["property uchar red", "property uchar green", "property uchar blue"]
        fields.append(("c", "u1", 3))
    header.append("end_header")
    rec = np.zeros(len(faces), np.dtype(fields))
    rec["n"], rec["v"] = 3, faces
    if face_colors is not None:
        rec["c"] = face_colors
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.concatenate(columns, axis=1).astype("<f4").tobytes())
        f.write(rec.tobytes())

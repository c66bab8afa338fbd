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

Three functions work ON THE DEVICE and ARE pinned to the bit (vkv_mesh_adjacency, vkv_mesh_smooth, vkv_mesh_vertex_normals):
build_adjacency(), smooth() and vertex_normals() take an indexed mesh as torch device tensors, with the extraction's ``counts`` tensor if its
capacities were given, and never wait for the host.  boundary_vertices() is the host helper that finds what callers will want pinned.
decimate() (vkv_mesh_decimate) clusters such a mesh's vertices on a regular grid, cluster_grid() lays that grid over a box
of voxels, and drop_duplicate_faces() is the host helper for the duplicates that clustering keeps.
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


# ---- on the device: adjacency, smoothing, normals from the faces -----------------------------------------------------------

def adjacency_scratch_bytes(capacity_vertices, capacity_triangles):
    """vkv_mesh_adjacency_scratch_bytes, and the header's formula: 32 + 8 per 4096 vertices + 3 x (4 per vertex, rounded up to 8) + 24 per
    triangle + (12 per triangle, rounded up to 8); 0 for a capacity above 2^32 - 1"""
    cv, ct = int(capacity_vertices), int(capacity_triangles)
    if cv > 0xffffffff or ct > 0xffffffff:
        return 0
    up8 = lambda n: (n + 7) & ~7  # noqa: E731
    return 32 + 8 * ((cv + 4095) // 4096) + 3 * up8(4 * cv) + 24 * ct + up8(12 * ct)


def _device_mesh(name, vertices, faces, counts):
    """the checks the three device calls share; (capacity_vertices, capacity_triangles, counts as a device tensor, the stream)"""
    import torch
    if not (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2 and vertices.shape[1] == 3
            and vertices.is_contiguous()):
        raise ValueError("mesh.%s: vertices must be a contiguous [v, 3] float32 device tensor" % name)
    if not (isinstance(faces, torch.Tensor) and faces.device == vertices.device and faces.dtype in (torch.uint32, torch.int32) and faces.dim() == 2
            and faces.shape[1] == 3 and faces.is_contiguous()):
        raise ValueError("mesh.%s: faces must be a contiguous [n, 3] uint32 (or int32) tensor on the vertices' device" % name)
    cv, ct = int(vertices.shape[0]), int(faces.shape[0])
    if counts is None:
        counts = torch.tensor([ct, ct, cv, cv], dtype=torch.int64).to(vertices.device)
    elif not (isinstance(counts, torch.Tensor) and counts.device == vertices.device and counts.dtype in (torch.int64, torch.uint64) and counts.numel() == 4
              and counts.is_contiguous()):
        raise ValueError("mesh.%s: counts must be the extraction's four 64-bit counts on the vertices' device" % name)
    return cv, ct, counts, torch.cuda.current_stream(vertices.device).cuda_stream


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


class Adjacency:
    """build_adjacency()'s result: the device block and the mesh it belongs to (its faces, counts and capacities)"""

    def __init__(self, block, faces, counts, capacity_vertices, capacity_triangles):
        self.block, self.faces, self.counts = block, faces, counts
        self.capacity_vertices, self.capacity_triangles = capacity_vertices, capacity_triangles


def build_adjacency(ctx, vertices, faces, counts=None):
    """vkv_mesh_adjacency on the current stream: per vertex its neighbour set and its faces, built once per mesh for smooth() and
    vertex_normals() (``adjacency=``).  ``vertices`` [v, 3] float32 and ``faces`` [n, 3] torch.uint32 are device tensors as
    Volume.extract_label_mesh_indexed / extract_isosurface_indexed return them; ``counts``: their int64 counts tensor when they were extracted
    with ``capacity=`` (it is read on the device), None when every row is meant.  Only the vertices' number is used here."""
    import torch
    cv, ct, counts, stream = _device_mesh("build_adjacency", vertices, faces, counts)
    block = torch.empty((adjacency_scratch_bytes(cv, ct) // 8,), dtype=torch.int64, device=vertices.device)
    # an empty face list still gets a pointer: the call reads nothing through it
    ctx.check(ctx.mesh_adjacency_rc(_ptr(faces) if ct else block.data_ptr(), ct, cv, counts.data_ptr(), block.data_ptr(), stream))
    return Adjacency(block, faces, counts, cv, ct)


def _adjacency_for(name, ctx, vertices, faces, counts, adjacency):
    if adjacency is None:
        return build_adjacency(ctx, vertices, faces, counts)
    if adjacency.capacity_vertices != vertices.shape[0] or adjacency.capacity_triangles != faces.shape[0]:
        raise ValueError("mesh.%s: the adjacency was built for another mesh" % name)
    return adjacency


def smooth(ctx, vertices, faces, counts=None, lam=0.5, mu=-0.53, iterations=10, pinned=None, adjacency=None):
    """vkv_mesh_smooth on the current stream: ``iterations`` Taubin iterations (a pass with factor ``lam``, then one with ``mu``; ``mu`` None:
    ``iterations`` passes of ``lam`` alone, plain Laplacian smoothing, which shrinks) of the uniform umbrella operator over the mesh's used
    faces.  Returns the smoothed vertices as a new [v, 3] float32 device tensor (rows past the counts' vertices are copies); pinned to the bit,
    no host wait.  A vertex shared by two bodies of a label mesh moves once, for both.  ``pinned``: None or a [v] bool / uint8 tensor (or
    array: boundary_vertices()), non-zero rows stay.  ``adjacency``: build_adjacency() of the same mesh, to build it once for several calls."""
    import torch
    cv, ct, counts, stream = _device_mesh("smooth", vertices, faces, counts)
    adjacency = _adjacency_for("smooth", ctx, vertices, faces, counts, adjacency)
    if pinned is not None:
        pinned = torch.as_tensor(np.ascontiguousarray(pinned).astype(np.uint8) if isinstance(pinned, np.ndarray) else pinned)
        pinned = pinned.to(device=vertices.device, dtype=torch.uint8).contiguous()
        if pinned.shape != (cv,):
            raise ValueError("mesh.smooth: pinned must have one entry per vertex row (%d), not %s" % (cv, tuple(pinned.shape)))
    factors = [float(lam)] * int(iterations) if mu is None else [float(lam), float(mu)] * int(iterations)
    out, swap = vertices.clone(), torch.empty_like(vertices)
    if cv:
        ctx.check(ctx.mesh_smooth_rc(out.data_ptr(), swap.data_ptr(), cv, adjacency.counts.data_ptr(), adjacency.block.data_ptr(), _ptr(pinned), factors,
                                     stream))
    return out


def vertex_normals(ctx, vertices, faces, counts=None, face_labels=None, label=0, adjacency=None):
    """vkv_mesh_vertex_normals on the current stream: a new [v, 3] float32 device tensor, per vertex the sum of (v1 - v0) x (v2 - v0) over its
    used faces (area-weighted, NOT normalised, zero where nothing contributes; rows past the counts' vertices are zero); pinned to the bit,
    no host wait.  ``face_labels`` ([n] torch.uint32) with ``label``: only the faces of that body, which gives an interface vertex of a label
    mesh that body's outward normal; over all faces such a vertex sums to exactly zero.  Valid for the positions given: call it after
    smooth().  ``adjacency``: build_adjacency() of the same mesh."""
    import torch
    cv, ct, counts, stream = _device_mesh("vertex_normals", vertices, faces, counts)
    adjacency = _adjacency_for("vertex_normals", ctx, vertices, faces, counts, adjacency)
    if face_labels is not None and not (isinstance(face_labels, torch.Tensor) and face_labels.device == vertices.device and face_labels.shape == (ct,)
                                        and face_labels.dtype in (torch.uint32, torch.int32) and face_labels.is_contiguous()):
        raise ValueError("mesh.vertex_normals: face_labels must be a contiguous [n] uint32 tensor on the vertices' device")
    normals = torch.zeros_like(vertices)
    if cv:
        ctx.check(ctx.mesh_vertex_normals_rc(vertices.data_ptr(), _ptr(faces) if ct else adjacency.block.data_ptr(), _ptr(face_labels) if ct else None,
                                             label, cv, ct, adjacency.counts.data_ptr(), adjacency.block.data_ptr(), normals.data_ptr(), stream))
    return normals


# ---- on the device: decimation by vertex clustering ---------------------------------------------------------------------------

def decimate_scratch_bytes(capacity_vertices, capacity_triangles, grid):
    """vkv_mesh_decimate_scratch_bytes, and the header's formula: with C = nx * ny * nz cells and B = ceil(triangles / 256), 32 per cell + 8
    per 4096 cells + 8 per B + 8 per 4096 B + (4 per vertex, rounded up to 8); 0 for a capacity or a cell count above 2^32 - 1 or a zero axis.
    ``grid``: (nx, ny, nz) or an abi.Extent3D."""
    cv, ct = int(capacity_vertices), int(capacity_triangles)
    nx, ny, nz = (grid.width, grid.height, grid.depth) if hasattr(grid, "width") else (int(n) for n in grid)
    cells = nx * ny * nz
    if cv > 0xffffffff or ct > 0xffffffff or cells == 0 or cells > 0xffffffff:
        return 0
    blocks = (ct + 255) // 256
    return 32 * cells + 8 * ((cells + 4095) // 4096) + 8 * blocks + 8 * ((blocks + 4095) // 4096) + ((4 * cv + 7) & ~7)


def cluster_grid(extent_or_box, cell=2.0):
    """``(origin, cell, counts)`` of a clustering grid that covers a box of voxels: three float32 each for origin and cell size, three ints for
    the cells per axis.  ``extent_or_box``: (W, H, D), an abi.Extent3D (the whole volume) or an abi.Box; ``cell``: one number or three, in
    voxels.  The origin is ``lo - 0.25`` per axis: with integer cell sizes neither integer coordinates (voxel centres) nor half-integers (where
    the vertices of a label mesh without a volume sit) lie on a cell boundary.  The cells reach to ``lo + length - 0.75`` at the least, past
    the last voxel centre at ``lo + length - 1``."""
    if hasattr(extent_or_box, "x0"):
        b = extent_or_box
        lo, length = (b.x0, b.y0, b.z0), (b.width, b.height, b.depth)
    else:
        lo, length = (0, 0, 0), tuple(int(n) for n in _whd(extent_or_box))
    return _cluster_grid(lo, length, cell)


def _cluster_grid(lo, length, cell):
    size = np.broadcast_to(np.asarray(cell, np.float32), (3,)).copy()
    if not (np.isfinite(size).all() and (size > 0).all()):
        raise ValueError("mesh.cluster_grid: cell sizes must be finite and positive, not %s" % (cell,))
    origin = np.asarray(lo, np.float32) - np.float32(0.25)
    counts = tuple(max(1, int(np.ceil((n - 0.75) / float(s)))) for n, s in zip(length, size))
    return origin, size, counts


def decimate(ctx, vertices, faces, counts=None, face_labels=None, cell=2.0, origin=None, grid=None, capacity=None):
    """vkv_mesh_decimate on the current stream: vertex clustering.  Every vertex falls into a cell of a regular grid, a cell's vertices become
    their mean, a face survives iff its three cells differ; pinned to the bit, no host wait.  ``vertices``, ``faces``, ``counts`` as for
    smooth(); ``face_labels``: None or the [n] torch.uint32 labels.  The grid: ``cell`` (one number or three), ``origin`` (three numbers) and
    ``grid`` (the cells per axis), as cluster_grid(volume.extent, cell) returns them: with them the call never waits for the host.  With
    ``grid`` None, ``origin`` and ``counts`` must be None too (every row is then meant, so every row is a position), and the grid is
    cluster_grid's for the integer box about the vertices, which reads their range on the host and so WAITS for it.
    ``capacity``: None sizes the outputs by the inputs (they can only shrink), or (vertices, triangles).  Returns ``(vertices, faces,
    face_labels or None, counts, vertex_map)``: new device tensors; ``counts`` the four int64 counts of the result, which with the first
    three is a mesh for build_adjacency(), smooth(), vertex_normals() and decimate(); ``vertex_map`` [v] torch.uint32, per input vertex the
    new number of its cell, 0xffffffff where no surviving face names it (and past the counts' vertices)."""
    import torch
    from . import abi
    if grid is None and (origin is not None or counts is not None):        # rows past the counts hold no positions to take a range of
        raise ValueError("mesh.decimate: an origin, or a mesh with counts, needs the grid's cell counts (mesh.cluster_grid)")
    cv, ct, counts, stream = _device_mesh("decimate", vertices, faces, counts)
    if face_labels is not None and not (isinstance(face_labels, torch.Tensor) and face_labels.device == vertices.device and face_labels.shape == (ct,)
                                        and face_labels.dtype in (torch.uint32, torch.int32) and face_labels.is_contiguous()):
        raise ValueError("mesh.decimate: face_labels must be a contiguous [n] uint32 tensor on the vertices' device")
    if grid is None:
        if cv:
            lo = np.floor(vertices.min(dim=0).values.cpu().numpy()).astype(np.int64)
            hi = np.ceil(vertices.max(dim=0).values.cpu().numpy()).astype(np.int64)
        else:
            lo = hi = np.zeros(3, np.int64)
        origin, cell, grid = _cluster_grid(lo, hi - lo + 1, cell)        # lo may be negative, which a box cannot be
    else:
        cell = np.broadcast_to(np.asarray(cell, np.float32), (3,))
        origin = np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(3)
    nx, ny, nz = (grid.width, grid.height, grid.depth) if hasattr(grid, "width") else (int(n) for n in grid)
    extent = abi.Extent3D(nx, ny, nz)
    out_cv, out_ct = (cv, ct) if capacity is None else (int(capacity[0]), int(capacity[1]))
    nbytes = decimate_scratch_bytes(cv, ct, (nx, ny, nz))
    if nbytes == 0:
        raise ValueError("mesh.decimate: a grid of %d x %d x %d cells" % (nx, ny, nz))
    dev = vertices.device
    scratch = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    out_vertices = torch.zeros((out_cv, 3), dtype=torch.float32, device=dev)
    out_faces = torch.zeros((out_ct, 3), dtype=torch.int32, device=dev).view(torch.uint32)
    out_labels = None if face_labels is None else torch.zeros((out_ct,), dtype=torch.int32, device=dev).view(torch.uint32)
    vertex_map = torch.full((cv,), -1, dtype=torch.int32, device=dev).view(torch.uint32)
    out_counts = torch.zeros((4,), dtype=torch.int64, device=dev)
    # empty lists still get a pointer: the call reads nothing through it
    ctx.check(ctx.mesh_decimate_rc(_ptr(vertices) or scratch.data_ptr(), _ptr(faces) or scratch.data_ptr(), _ptr(face_labels), cv, ct, counts.data_ptr(),
                                   origin, cell, extent, scratch.data_ptr(), _ptr(out_vertices), out_cv, _ptr(out_faces), _ptr(out_labels), out_ct,
                                   _ptr(vertex_map), out_counts.data_ptr(), stream))
    return out_vertices, out_faces, out_labels, out_counts, vertex_map


def drop_duplicate_faces(faces, face_labels=None):
    """On the host: the faces without those that repeat an earlier one, up to rotation of the three vertex numbers and with the same label;
    the first of each stays, in order.  A face with the opposite winding is another face: the opposite pairs of a label mesh's interfaces
    stay.  Returns ``faces`` (int64), or ``(faces, face_labels)`` with labels.  decimate() keeps duplicates; this removes them."""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    key = f
    for r in (f[:, [1, 2, 0]], f[:, [2, 0, 1]]):        # the least of the three rotations, as a triple
        less = (r[:, 0] < key[:, 0]) | ((r[:, 0] == key[:, 0]) & ((r[:, 1] < key[:, 1]) | ((r[:, 1] == key[:, 1]) & (r[:, 2] < key[:, 2]))))
        key = np.where(less[:, None], r, key)
    if face_labels is not None:
        face_labels = np.asarray(face_labels).reshape(-1)
        if len(face_labels) != len(f):
            raise ValueError("%d labels for %d faces" % (len(face_labels), len(f)))
        key = np.concatenate([key, face_labels.astype(np.int64)[:, None]], axis=1)
    keep = np.sort(np.unique(key, axis=0, return_index=True)[1]) if len(f) else np.zeros(0, np.int64)
    return f[keep] if face_labels is None else (f[keep], face_labels[keep])


def boundary_vertices(faces, n_vertices):
    """[n_vertices] bool, on the host: the vertices on an edge that exactly one face holds, i.e. the rim of an open surface: where a body
    leaves the box (the extractors leave the box's faces open) and the seams of a box-by-box extraction.  Pin them in smooth(), or the rim
    shrinks and the seams part.  ``faces`` [n, 3]: any integer array (a tensor's ``.cpu().numpy()``); faces that name a vertex at or past
    n_vertices (a truncated extraction) are not used, as on the device."""
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    f = f[(f < int(n_vertices)).all(axis=1)]
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    e = e[e[:, 0] != e[:, 1]]
    mask = np.zeros(int(n_vertices), bool)
    if len(e):
        edges, n = np.unique(e, axis=0, return_counts=True)
        mask[edges[n == 1].reshape(-1)] = True
    return mask

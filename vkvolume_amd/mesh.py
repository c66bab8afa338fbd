"""What to do with the triangles of Volume.extract_isosurface / vkv_isosurface_mesh on the host: numpy only, nothing here is pinned to the bit.

``tri`` is always an [n, 3, 3] float32 array (triangle, vertex, xyz) in voxel-index coordinates, voxel centres at integers (a device tensor's
``.cpu().numpy()``).  Triangles wind so that (v1 - v0) x (v2 - v0) points from the inside (f >= iso) to the outside.
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


def to_texture(tri, extent):
    """voxel-index coordinates -> texture coordinates ([0, 1]^3 = the volume): (p + 0.5) / extent, ``extent`` = (W, H, D) or an abi.Extent3D"""
    return (_tri(tri) + np.float32(0.5)) / _whd(extent)


def to_model(tri, extent, matrix):
    """voxel-index coordinates -> the space ``matrix`` maps the volume's centred unit cube into: matrix * (texture - 0.5).  ``matrix``: a
    column-major 4 x 4 as vkvolume_amd.camera builds them (memory order m[col][row]), e.g. Volume.image_transform or node * image."""
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

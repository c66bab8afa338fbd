"""Camera matrices for the offscreen driver (stand-in for the vkb free camera the reference gets from
Vulkan-Samples, src/volume_render.cpp:169; pose and fov are this build's own definition).

All matrices are column-major 4x4 stored as numpy float32 arrays of shape (4, 4) in *memory order*
``m[col][row]`` — i.e. ``m.reshape(16)`` is the glm::mat4 byte layout the C ABI expects.
"""
import math

import numpy as np


def _colmajor(rows):
    """rows: 4x4 nested list in mathematical (row, col) order → column-major float32 [col][row]."""
    return np.ascontiguousarray(np.array(rows, np.float64).T, np.float32)


def look_at(eye, centre, up=(0.0, 1.0, 0.0)):
    """glm::lookAtRH"""
    eye, centre, up = (np.asarray(v, np.float64) for v in (eye, centre, up))
    f = centre - eye
    f /= np.linalg.norm(f)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    return _colmajor([[s[0], s[1], s[2], -s.dot(eye)],
                      [u[0], u[1], u[2], -u.dot(eye)],
                      [-f[0], -f[1], -f[2], f.dot(eye)],
                      [0, 0, 0, 1]])


def perspective_vulkan(fov_y_deg, aspect, near=0.1, far=1000.0):
    """vkb::PerspectiveCamera::get_projection (reverse-Z: glm::perspectiveRH_ZO(fov, aspect, far, near)) followed by
    vkb::vulkan_style_projection (y flipped), as used at src/volume_render_subpass.cpp:224."""
    t = math.tan(math.radians(fov_y_deg) / 2.0)
    zn, zf = far, near  # swapped on purpose
    return _colmajor([[1.0 / (aspect * t), 0, 0, 0],
                      [0, -1.0 / t, 0, 0],
                      [0, 0, zf / (zn - zf), -(zf * zn) / (zf - zn)],
                      [0, 0, -1, 0]])


def scale(s):
    s = np.broadcast_to(np.asarray(s, np.float64), (3,))
    return _colmajor([[s[0], 0, 0, 0], [0, s[1], 0, 0], [0, 0, s[2], 0], [0, 0, 0, 1]])


def rotate(angle_deg, axis):
    """glm::rotate(angle, axis)"""
    a = math.radians(angle_deg)
    c, s = math.cos(a), math.sin(a)
    n = np.asarray(axis, np.float64)
    n = n / np.linalg.norm(n)
    t = (1 - c) * n
    r = np.array([[c + t[0] * n[0], t[1] * n[0] - s * n[2], t[2] * n[0] + s * n[1], 0],
                  [t[0] * n[1] + s * n[2], c + t[1] * n[1], t[2] * n[1] - s * n[0], 0],
                  [t[0] * n[2] - s * n[1], t[1] * n[2] + s * n[0], c + t[2] * n[2], 0],
                  [0, 0, 0, 1]])
    return _colmajor(r)


def matmul(a, b):
    """column-major product a*b"""
    return np.ascontiguousarray((a.astype(np.float64).T @ b.astype(np.float64).T).T, np.float32)


def image_transform(voxel_size, extent_whd, axis_angle=(1.0, 0.0, 0.0, 0.0)):
    """LoadVolume::load_header's image_transform = rotate(angle, axis) * scale(voxel_size * extent)
    (src/load_volume.cpp:82-83)."""
    size = np.asarray(voxel_size, np.float64) * np.asarray(extent_whd, np.float64)
    return matmul(rotate(axis_angle[3], axis_angle[:3]), scale(size))


def benchmark_node_transform(image_xf, scale_factor=100.0):
    """Benchmark-mode node scale: the longest physical edge becomes ``scale_factor`` units
    (src/volume_render.cpp:224-238 rescales by the rotated physical size; SURVEY.md §8d keeps aspect)."""
    m = image_xf.astype(np.float64).T[:3, :3]
    longest = max(np.linalg.norm(m[:, i]) for i in range(3))
    return scale(scale_factor / longest)


def orbit_camera(azimuth_deg, elevation_deg, radius, centre=(0.0, 0.0, 0.0)):
    """Camera on a sphere around ``centre`` looking at it (8 azimuths, elevation 20 deg)."""
    az, el = math.radians(azimuth_deg), math.radians(elevation_deg)
    eye = np.asarray(centre, np.float64) + radius * np.array([math.cos(el) * math.sin(az), math.sin(el),
                                                              math.cos(el) * math.cos(az)])
    return look_at(eye, centre)


def slab_plane(extent_whd, centre_voxel=None, normal=None, up=None, image_size=None, pixel_voxels=1.0, thickness_voxels=0.0, sample_voxels=1.0,
               axis=None, index=None):
    """The plane of a slice or slab for vkv_render_slab (VolumeRenderSubpass.draw_slab), pure numpy: a dict with ``origin``, ``du``, ``dv``,
    ``dn`` (float32, texture coordinates), ``samples`` = max(1, round(thickness_voxels / sample_voxels) + 1) and ``image_size``.

    Voxel space: voxel i of an axis has its centre at coordinate i (the sampler's voxel coordinate), so the texture coordinate of voxel
    coordinate c is (c + 0.5) / extent.  The frame is orthonormal in voxel space: n = ``normal`` normalised, v = ``up`` made orthogonal to n
    and normalised (image rows advance along v), u = v x n (image columns advance along u).  A pixel step is ``pixel_voxels`` long, a sample
    step ``sample_voxels`` along n; the image is centred on ``centre_voxel`` (default: the volume's centre) and the slab on the plane.

    ``axis`` = "x" | "y" | "z" with ``index`` = k: slice k of that axis, one pixel per voxel, columns and rows along the remaining axes in
    x, y, z order (axis z: du = (1/W, 0, 0), dv = (0, 1/H, 0), origin_z = (k + 0.5) / D; image (W, H) unless ``image_size`` is given), dn
    along the axis."""
    ext = np.asarray(extent_whd, np.float64)
    if axis is not None:
        a = "xyz".index(axis)
        cu, cv = [c for c in range(3) if c != a]
        n, u, v = np.zeros(3), np.zeros(3), np.zeros(3)
        n[a], u[cu], v[cv] = 1.0, 1.0, 1.0
        if image_size is None:
            image_size = (int(ext[cu]), int(ext[cv]))
        if centre_voxel is None:
            centre_voxel = (ext - 1.0) * 0.5
        centre = np.asarray(centre_voxel, np.float64).copy()
        if index is not None:
            centre[a] = float(index)
    else:
        n = np.asarray(normal, np.float64)
        n = n / np.linalg.norm(n)
        v = np.asarray(up, np.float64)
        v = v - np.dot(v, n) * n
        if not np.linalg.norm(v) > 0.0:
            raise ValueError("slab_plane: up is parallel to normal")
        v = v / np.linalg.norm(v)
        u = np.cross(v, n)
        centre = (ext - 1.0) * 0.5 if centre_voxel is None else np.asarray(centre_voxel, np.float64)
    w, h = image_size
    samples = max(1, int(round(thickness_voxels / sample_voxels)) + 1)
    du_v, dv_v, dn_v = u * pixel_voxels, v * pixel_voxels, n * sample_voxels
    origin_v = centre - 0.5 * (w - 1) * du_v - 0.5 * (h - 1) * dv_v - 0.5 * (samples - 1) * dn_v
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    return dict(origin=f32((origin_v + 0.5) / ext), du=f32(du_v / ext), dv=f32(dv_v / ext), dn=f32(dn_v / ext), samples=samples,
                image_size=(int(w), int(h)))

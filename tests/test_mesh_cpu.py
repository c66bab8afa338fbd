"""The definition of vkv_isosurface_mesh (include/vkvolume_amd.h, DESIGN.md §5.13: marching tetrahedra on the Kuhn decomposition, every step
fp32 IEEE) restated twice in numpy, and what can be shown of it without a GPU: the two statements agree to the bit, the winding rule is right in
all 6 x 14 cases, the surfaces of a ball, a torus and a zero-bordered random volume are closed, oriented 2-manifolds with the expected counts,
the header's compile-time case table (mtet_table.hpp, printed by tests/mtet_driver.cpp) equals numpy's entry for entry, the kernels of mesh.hip
use no scratch memory, and vkvolume_amd.mesh welds, filters and writes what it is given.  tests/test_gpu_mesh.py holds the kernels to
mesh_np() bit for bit."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from vkvolume_amd import abi, lib, mesh as M, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINV255 = np.float32(1.0) / np.float32(255.0)
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))  # cube corners j = dx + 2 dy + 4 dz
ODD = (False, True, True, False, False, True)
FLIP = (2, 5, 8, 10, 11, 14)


def tet_triangles(t, m):
    """the triangles of tetrahedron t under mask m: a list of three edges each, an edge a pair of LOCAL vertices as the definition writes it"""
    ins, out = [i for i in range(4) if m >> i & 1], [i for i in range(4) if not m >> i & 1]
    if len(ins) == 1:
        tris = [[(ins[0], out[0]), (ins[0], out[1]), (ins[0], out[2])]]
    elif len(ins) == 3:
        tris = [[(ins[0], out[0]), (ins[1], out[0]), (ins[2], out[0])]]
    elif len(ins) == 2:
        (a, b), (c, d) = ins, out
        A, B, Cc, D = (a, c), (a, d), (b, d), (b, c)
        tris = [[A, B, Cc], [A, Cc, D]]
    else:
        return []
    if ODD[t] != (m in FLIP):
        tris = [[v0, v2, v1] for v0, v1, v2 in tris]
    return tris


def case_table():
    """{(t, m): (swap, [(a, b) cube corners of every edge, three per triangle])}, a from the lower local index"""
    table = {}
    for t in range(6):
        for m in range(16):
            edges = [(TETS[t][min(e)], TETS[t][max(e)]) for tri in tet_triangles(t, m) for e in tri]
            table[t, m] = (int(bool(edges) and ODD[t] != (m in FLIP)), edges)
    return table


def _crop(vol, box):
    vol = np.ascontiguousarray(vol, np.uint8)
    if box is None:
        return vol, (0, 0, 0)
    x0, y0, z0, w, h, d = box
    return vol[z0:z0 + d, y0:y0 + h, x0:x0 + w], (x0, y0, z0)


def mesh_np(vol_dhw, iso, box=None, origin=(0, 0, 0)):
    """vectorised statement: [n, 3, 3] float32, all cubes at once, then sorted into the defined order.  box = (x0, y0, z0, w, h, d);
    origin: where voxel (0, 0, 0) of vol_dhw lies in the volume whose coordinates the vertices carry (vol_dhw is a window cut from it)"""
    vol, first = _crop(vol_dhw, box)
    origin = tuple(int(a) + int(b) for a, b in zip(first, origin))
    iso = np.float32(iso)
    f = vol.astype(np.float32) * KINV255
    inside = f >= iso
    d, h, w = vol.shape
    if min(d, h, w) < 2:
        return np.zeros((0, 3, 3), np.float32)
    corner = lambda a, j: a[(j >> 2):d - 1 + (j >> 2), (j >> 1 & 1):h - 1 + (j >> 1 & 1), (j & 1):w - 1 + (j & 1)]  # noqa: E731
    table = case_table()
    keys, tris = [], []
    for t in range(6):
        sub = sum(corner(inside, TETS[t][i]).astype(np.int64) << i for i in range(4))
        for m in range(1, 15):
            _, edges = table[t, m]
            z, y, x = np.nonzero(sub == m)
            if len(z) == 0:
                continue
            cube = (z * (h - 1) + y) * (w - 1) + x
            for k in range(len(edges) // 3):
                out = np.empty((len(z), 3, 3), np.float32)
                for v in range(3):
                    a, b = edges[3 * k + v]
                    pa = [x + (a & 1), y + (a >> 1 & 1), z + (a >> 2)]
                    pb = [x + (b & 1), y + (b >> 1 & 1), z + (b >> 2)]
                    fa, fb = f[pa[2], pa[1], pa[0]], f[pb[2], pb[1], pb[0]]
                    tt = (iso - fa) / (fb - fa)
                    assert tt.dtype == np.float32
                    for c in range(3):
                        ac = (pa[c] + origin[c]).astype(np.float32)
                        out[:, v, c] = ac + tt if (a ^ b) >> c & 1 else ac
                keys.append((cube * 6 + t) * 2 + k)
                tris.append(out)
    if not keys:
        return np.zeros((0, 3, 3), np.float32)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys)
    return np.ascontiguousarray(tris[order])


def mesh_loop(vol_dhw, iso, box=None):
    """plain statement: cube by cube in the defined order, straight from the definition's sentences (no table)"""
    vol, origin = _crop(vol_dhw, box)
    iso = np.float32(iso)
    d, h, w = vol.shape
    value = lambda p: np.float32(vol[p[2], p[1], p[0]]) * KINV255  # noqa: E731
    out = []
    for z in range(d - 1):
        for y in range(h - 1):
            for x in range(w - 1):
                for t in range(6):
                    pos = [(x + (j & 1), y + (j >> 1 & 1), z + (j >> 2)) for j in TETS[t]]
                    m = sum(1 << i for i in range(4) if value(pos[i]) >= iso)
                    for tri in tet_triangles(t, m):
                        verts = []
                        for i, j in tri:
                            a, b = pos[min(i, j)], pos[max(i, j)]
                            fa, fb = value(a), value(b)
                            tt = (iso - fa) / (fb - fa)
                            verts.append([np.float32(a[c] + origin[c]) + tt if b[c] != a[c] else np.float32(a[c] + origin[c]) for c in range(3)])
                        out.append(verts)
    return np.array(out, np.float32).reshape(-1, 3, 3)


def same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, "%s: %s triangles, expected %s" % (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(g, w), "%s: %d floats differ, first at (triangle, vertex, axis) %s: got %s want %s" % (
        what, int((g != w).sum()), np.argwhere(g != w)[:4].tolist(), got[g != w][:4].tolist(), want[g != w][:4].tolist())


# ---- the test volumes (float64 formulas truncated to uint8) -------------------------------------------------------------------------------
def ball(n=12, centre=5.5, radius=4.0):
    z, y, x = np.indices((n, n, n)).astype(np.float64)
    dist = np.sqrt((x - centre) ** 2 + (y - centre) ** 2 + (z - centre) ** 2)
    return np.clip((radius - dist) * 60 + 128, 0, 255).astype(np.uint8)


def torus(n=14):
    z, y, x = np.indices((n, n, n)).astype(np.float64)
    dist = np.sqrt((np.sqrt((x - 6.5) ** 2 + (y - 6.5) ** 2) - 4) ** 2 + (z - 6.5) ** 2)
    return np.clip((1.6 - dist) * 80 + 128, 0, 255).astype(np.uint8)


def bordered_random(shape_dhw=(6, 7, 9), seed=11):
    vol = np.zeros(shape_dhw, np.uint8)
    vol[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).integers(0, 256, size=tuple(s - 2 for s in shape_dhw), dtype=np.uint8)
    return vol


def mesh_contents(kind, shape_dhw, seed):
    """the contents of tests/test_gpu_mesh.py"""
    d, h, w = shape_dhw
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, size=shape_dhw, dtype=np.uint8)
    if kind == "ball":
        z, y, x = np.indices(shape_dhw).astype(np.float64)
        r = np.sqrt(((x - (w - 1) / 2) / max(w, 2)) ** 2 + ((y - (h - 1) / 2) / max(h, 2)) ** 2 + ((z - (d - 1) / 2) / max(d, 2)) ** 2)
        return np.clip((0.35 - r) * 900 + 128, 0, 255).astype(np.uint8)
    if kind == "below":
        return np.full(shape_dhw, 17, np.uint8)
    if kind == "above":
        return np.full(shape_dhw, 200, np.uint8)
    assert kind == "voxel"
    vol = np.zeros(shape_dhw, np.uint8)
    vol[d // 2, h // 2, w // 2] = 255
    return vol


MESH_CONTENTS = ("random", "ball", "below", "above", "voxel")


def directed_edges(faces):
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    return e[:, 0] * (faces.max() + 1) + e[:, 1], e


def closed_and_oriented(tri):
    """every directed edge of the bitwise-welded mesh occurs once and its reverse once; returns (vertices, undirected edges, faces)"""
    vertices, faces = M.weld(tri)
    keys, e = directed_edges(faces)
    assert len(np.unique(keys)) == len(keys), "a directed edge occurs twice"
    rev = e[:, 1] * (faces.max() + 1) + e[:, 0]
    assert np.array_equal(np.sort(keys), np.sort(rev)), "a directed edge lacks its reverse"
    assert len(keys) % 2 == 0
    return len(vertices), len(keys) // 2, len(faces)


def signed_volume(tri):
    t = tri.astype(np.float64)
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


# ---- entry point -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bsize_t\s+vkv_isosurface_mesh_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_isosurface_mesh\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"float iso,\s*const uint8_t\s*\*d_max_map,\s*VkvExtent3D map_extent,\s*void\s*\*d_scratch,\s*float\s*\*d_triangles,\s*"
                     r"uint64_t capacity_triangles,\s*uint64_t\s*\*d_counts,\s*void\s*\*stream\)", header)
    L = lib.load()
    assert {"vkv_isosurface_mesh", "vkv_isosurface_mesh_scratch_bytes"} <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\bvkv_isosurface_mesh$", out, flags=re.M) and re.search(r"\bvkv_isosurface_mesh_scratch_bytes$", out, flags=re.M)
    at = L.vkv_isosurface_mesh.argtypes
    assert len(at) == 12 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[9] is C.c_uint64
    assert callable(lib.Context.isosurface_mesh) and callable(lib.Context.isosurface_mesh_rc) and callable(V.Volume.extract_isosurface)


def test_scratch_bytes_and_bad_arguments_without_a_device():
    """no context exists without a device, so every call carries a null ctx besides its own fault (tests/test_gpu_mesh.py repeats them with a live
    context and sentinels); the scratch size is host arithmetic"""
    L = lib.load()
    e = abi.Extent3D(258, 5, 19)
    assert lib.mesh_scratch_bytes(e) >= 16 and lib.mesh_scratch_bytes(e) % 8 == 0
    assert lib.mesh_scratch_bytes(abi.Extent3D(1, 5, 19)) >= 16 and lib.mesh_scratch_bytes(abi.Extent3D(1, 1, 1)) >= 16        # no cubes, still a buffer
    assert lib.mesh_scratch_bytes(e, abi.Box(1, 1, 1, 2, 2, 2)) <= lib.mesh_scratch_bytes(e)
    assert lib.mesh_scratch_bytes(abi.Extent3D(0, 5, 19)) == 0
    assert lib.mesh_scratch_bytes(e, abi.Box(257, 0, 0, 2, 1, 1)) == 0 and lib.mesh_scratch_bytes(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    assert lib.mesh_scratch_bytes(abi.Extent3D(0x80000000, 2, 2)) == 0
    buf = (C.c_uint64 * 64)()
    a = C.addressof(buf)
    none = abi.Extent3D(0, 0, 0)
    assert L.vkv_isosurface_mesh(None, a, abi.Extent3D(4, 4, 4), None, 0.5, None, none, a + 64, None, 0, a + 256, None) == abi.VKV_E_INVALID_ARGUMENT


# ---- the two statements ------------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 6, 7), (1, 6, 7), (6, 1, 7), (6, 7, 1), (2, 2, 2), (2, 3, 2), (3, 2, 5), (1, 1, 1), (4, 3, 6)]  # (depth, height, width)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_two_statements_agree_to_the_bit(shape):
    for seed, iso in ((0, 0.5), (1, 0.25), (2, 0.9), (3, 1.5), (4, 0.0)):
        vol = np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)
        a, b = mesh_np(vol, iso), mesh_loop(vol, iso)
        same_bits(a, b, "%s iso %g" % (shape, iso))
        if min(shape) < 2 or iso > 1.0 or iso <= 0.0:
            assert len(a) == 0
        assert len(a) <= 12 * max(shape[0] - 1, 0) * max(shape[1] - 1, 0) * max(shape[2] - 1, 0)


def test_a_box_is_the_cropped_volume_shifted():
    vol = np.random.default_rng(5).integers(0, 256, size=(5, 6, 7), dtype=np.uint8)
    box = (2, 1, 1, 4, 3, 3)
    a, b = mesh_np(vol, 0.5, box), mesh_loop(vol, 0.5, box)
    same_bits(a, b, "box")
    shifted = mesh_np(vol[1:4, 1:4, 2:6], 0.5) + np.array([2, 1, 1], np.float32)        # integer shifts of a_c + t are NOT exact in general
    assert len(a) == len(shifted) and np.allclose(a, shifted, atol=1e-5)
    assert len(mesh_np(vol, 0.5, (3, 0, 0, 1, 6, 5))) == 0


def test_a_voxel_equal_to_iso_gives_degenerate_triangles_and_both_statements_still_agree():
    iso = np.float32(128) * KINV255
    vol = np.random.default_rng(6).integers(120, 137, size=(4, 5, 6), dtype=np.uint8)
    vol[1:3, 2, 3] = 128
    assert (vol == 128).any()
    a = mesh_np(vol, iso)
    same_bits(a, mesh_loop(vol, iso), "iso on a voxel's value")
    kept = M.drop_degenerate(a)
    assert 0 < len(kept) < len(a)
    assert not np.isnan(a).any() and a.min() >= 0


# ---- winding -----------------------------------------------------------------------------------------------------------------------------
def test_winding_points_from_inside_to_outside_in_all_cases():
    cases = 0
    for t in range(6):
        pos = np.array([[j & 1, j >> 1 & 1, j >> 2] for j in TETS[t]], np.float64)
        # the permutation's parity, from the path itself: the axes it adds, in order
        axes = [int(np.argmax(pos[i + 1] - pos[i])) for i in range(3)]
        parity = sum(1 for i in range(3) for j in range(i) if axes[j] > axes[i]) % 2
        assert bool(parity) == ODD[t] and sorted(axes) == [0, 1, 2]
        for m in range(1, 15):
            ins, out = [i for i in range(4) if m >> i & 1], [i for i in range(4) if not m >> i & 1]
            direction = pos[out].mean(axis=0) - pos[ins].mean(axis=0)
            tris = tet_triangles(t, m)
            assert len(tris) == (2 if len(ins) == 2 else 1)
            for tri in tris:
                v = [(pos[i] + pos[j]) / 2 for i, j in tri]
                normal = np.cross(v[1] - v[0], v[2] - v[0])
                assert np.linalg.norm(normal) > 0 and np.dot(normal, direction) > 0, (t, m, tri)
            cases += 1
    assert cases == 6 * 14


# ---- surfaces ----------------------------------------------------------------------------------------------------------------------------
def test_ball_is_a_closed_oriented_sphere_with_the_expected_counts():
    tri = mesh_np(ball(), 0.5)
    assert len(tri) == 1824
    v, e, f = closed_and_oriented(tri)
    assert (v, e, f) == (914, 2736, 1824) and v - e + f == 2
    assert signed_volume(tri) > 0
    # roughly the ball it was made from: radius 4 at byte 128, iso 0.5 = byte 127.5
    assert abs(signed_volume(tri) - 4.0 / 3.0 * np.pi * 4.0 ** 3) < 0.05 * 268.1
    same_bits(tri[:200], mesh_loop(ball(), 0.5)[:200], "ball")


def test_torus_is_closed_with_euler_characteristic_zero():
    tri = mesh_np(torus(), 0.5)
    assert len(tri) == 2272
    v, e, f = closed_and_oriented(tri)
    assert v - e + f == 0 and signed_volume(tri) > 0


def test_zero_bordered_random_bytes_give_a_closed_oriented_surface():
    vol = bordered_random()
    assert vol.shape == (6, 7, 9)
    tri = mesh_np(vol, 0.5)
    assert len(tri) > 0
    closed_and_oriented(tri)
    assert signed_volume(tri) > 0
    same_bits(tri, mesh_loop(vol, 0.5), "bordered random")


# ---- the header's table ------------------------------------------------------------------------------------------------------------------
def parse_driver(text):
    tets, cases, counts = {}, {}, {}
    for line in text.splitlines():
        w = line.split()
        if w and w[0] == "tet":
            tets[int(w[1])] = (tuple(int(x) for x in w[2:6]), bool(int(w[6])))
        elif w and w[0] == "case":
            n = int(w[3])
            e = [int(x) for x in w[5:]]
            assert len(e) == 6 * n
            cases[int(w[1]), int(w[2])] = (int(w[4]), [(e[2 * i], e[2 * i + 1]) for i in range(3 * n)])
        elif w and w[0] == "count":
            counts[int(w[1])] = int(w[2])
    return tets, cases, counts


def check_driver_output(text):
    assert "mtet ok" in text
    tets, cases, counts = parse_driver(text)
    assert tets == {t: (TETS[t], ODD[t]) for t in range(6)}
    want = case_table()
    assert set(cases) == set(want)
    for key in sorted(want):
        assert cases[key] == want[key], (key, cases[key], want[key])
    for cm in range(256):
        n = sum(len(want[t, sum((cm >> TETS[t][i] & 1) << i for i in range(4))][1]) // 3 for t in range(6))
        assert counts[cm] == n, (cm, counts[cm], n)
    assert max(counts.values()) == 12


def test_header_table_equals_numpy_entry_for_entry(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = os.path.join(ROOT, "tests", "mtet_driver.cpp")
    for name, extra in (("mtet_driver", []), ("mtet_driver_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = tmp_path / name
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror"] + extra + ["-I", T.CSRC, src, "-o", str(exe)])
        r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:]
        check_driver_output(r.stdout)
    # the kernels read this very table, not a copy
    text = open(os.path.join(T.CSRC, "mesh.hip")).read()
    assert '#include "mtet_table.hpp"' in text and "d_mtet = kMtetTable" in text


def test_scratch_layout_matches_the_promised_sizes_under_asan_and_ubsan(tmp_path):
    """MeshScratch, which the four extractors' *_scratch_bytes() and launchers share: its size against the formulas of include/vkvolume_amd.h and
    its pointers against the size, for plans without a cube, with one entry and with 4096 and 4097 (tests/mesh_scratch_driver.cpp, the header's
    host pass: no GPU, no kernel)"""
    hipcc = T.HIPCC if os.path.exists(T.HIPCC) else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path / "mesh_scratch_driver"
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=undefined", "-I", T.CSRC, os.path.join(ROOT, "tests", "mesh_scratch_driver.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "mesh scratch layout ok", r.stdout[-2000:]


def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("mesh.hip", tmp_path / "mesh.s")
    assert len([k for k in kernels if "k_mesh_count" in k]) == 2 and len([k for k in kernels if "k_mesh_emit" in k]) == 2, sorted(kernels)  # WIDE, narrow
    assert len([k for k in kernels if "k_mesh_scan" in k]) == 2, sorted(kernels)
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)


# ---- vkvolume_amd.mesh -------------------------------------------------------------------------------------------------------------------
def read_stl(path):
    data = open(path, "rb").read()
    (n,) = struct.unpack_from("<I", data, 80)
    assert len(data) == 84 + 50 * n
    normals, tris = np.empty((n, 3), np.float32), np.empty((n, 3, 3), np.float32)
    for i in range(n):
        rec = struct.unpack_from("<12fH", data, 84 + 50 * i)
        normals[i], tris[i] = rec[:3], np.array(rec[3:12]).reshape(3, 3)
        assert rec[12] == 0
    return data[:80], normals, tris


def test_write_stl_round_trips(tmp_path):
    tri = mesh_np(ball(), 0.5)
    path = tmp_path / "ball.stl"
    M.write_stl(str(path), tri)
    header, normals, back = read_stl(str(path))
    assert header.startswith(b"vkvolume_amd") and not header.startswith(b"solid")
    same_bits(back, tri, "stl")
    centre = np.float32(5.5)
    outward = tri.mean(axis=1) - centre
    assert (np.einsum("ij,ij->i", normals, outward) > 0).all()        # a bright ball: the normals point away from its centre
    assert np.allclose(np.linalg.norm(normals, axis=1), 1.0, atol=1e-5)
    M.write_stl(str(path), np.zeros((0, 3, 3), np.float32))
    assert len(read_stl(str(path))[2]) == 0


def test_weld_drop_degenerate_and_the_coordinate_maps():
    tri = mesh_np(ball(), 0.5)
    vertices, faces = M.weld(tri)
    assert vertices.shape == (914, 3) and faces.shape == (1824, 3) and faces.min() == 0 and faces.max() == 913
    same_bits(vertices[faces], tri, "weld")
    assert (np.diff(np.unique(faces.reshape(-1), return_index=True)[1]) > 0).all()        # numbered by first use
    assert len(M.drop_degenerate(tri)) == 1824
    flat = tri.copy()
    flat[3, 2] = flat[3, 0]
    flat[7, 1] = flat[7, 2]
    assert len(M.drop_degenerate(flat)) == 1822
    tex = M.to_texture(tri, (12, 12, 12))
    assert tex.dtype == np.float32 and np.array_equal(tex, (tri + np.float32(0.5)) / np.float32(12))
    assert np.array_equal(M.to_texture(tri, abi.Extent3D(12, 12, 12)), tex)
    from vkvolume_amd import camera
    xf = camera.image_transform((1.0, 2.0, 0.5), (12, 12, 12))
    model = M.to_model(tri, (12, 12, 12), xf)
    assert np.allclose(model, (tex - 0.5) * np.array([12.0, 24.0, 6.0], np.float32), atol=1e-5)
    with pytest.raises(ValueError):
        M.weld(np.zeros((4, 3), np.float32))

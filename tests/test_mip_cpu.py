"""Maximum-intensity projection without a GPU: the ctypes mirror of VkvMipOptions against the C header, the two facts the skipping path's
exactness rests on (every lerp of the filter lies between its endpoints; x * kInv255 is monotone), the numpy restatements of
vkv_max_map (max_map_np) and of the dense MIP (mip_np) on analytic volumes, and the compiled MIP kernels' listing (no scratch).

max_map_np and mip_np are the references tests/test_gpu_mip.py compares the device against."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vkvolume_amd import abi, lib
from vkvolume_amd.abi import MipOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vkvolume_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
F = np.float32
INV255 = F(1.0) / F(255.0)


# ---- numpy restatements ---------------------------------------------------------------------------------------------------------------

def max_map_np(vol, map_extent):
    """vkv_max_map: per cell of map_extent (w, h, d) the largest voxel of the cell's voxel box grown by one voxel per side, clipped to the
    volume; cells past the volume hold 0.  vol is (D, H, W) uint8; the result is (md, mh, mw) uint8."""
    D, H, W = vol.shape
    mw, mh, md = map_extent
    bx, by, bz = -(-W // mw), -(-H // mh), -(-D // md)
    g = vol.copy()
    for axis in range(3):  # grown by one voxel: the max over each voxel's clipped +-1 neighbourhood, axis by axis
        lo = np.concatenate([np.take(g, [0], axis), np.take(g, range(g.shape[axis] - 1), axis)], axis)
        hi = np.concatenate([np.take(g, range(1, g.shape[axis]), axis), np.take(g, [g.shape[axis] - 1], axis)], axis)
        g = np.maximum(g, np.maximum(lo, hi))
    pad = np.zeros((md * bz, mh * by, mw * bx), np.uint8)  # cells past the volume read only the zero padding
    pad[:D, :H, :W] = g
    return pad.reshape(md, bz, mh, by, mw, bx).max(axis=(1, 3, 5))


def _fma(a, b, c):
    """fp32 fma through float64 (the product of two floats is exact in float64)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _gmin(x, y):
    return np.where(y < x, y, x)


def _gmax(x, y):
    return np.where(x < y, y, x)


def _mat4_mul(m, v):
    """mat4_mul_vec4 of raymarch_core.hpp: m column-major float[16], v four arrays"""
    m = np.asarray(m, F)
    return [_fma(m[12 + i], v[3], _fma(m[8 + i], v[2], _fma(m[4 + i], v[1], F(m[i]) * v[0]))) for i in range(4)]


def sample_linear_np(vol, px, py, pz):
    """sample_linear of raymarch_core.hpp: clamp-to-edge trilinear filter, lerps as fma(w, b - a, a), times kInv255"""
    D, H, W = vol.shape
    cx, cy, cz = _fma(px, F(W), F(-0.5)), _fma(py, F(H), F(-0.5)), _fma(pz, F(D), F(-0.5))
    fx, fy, fz = np.floor(cx), np.floor(cy), np.floor(cz)
    wx, wy, wz = cx - fx, cy - fy, cz - fz
    ix, iy, iz = fx.astype(np.int64), fy.astype(np.int64), fz.astype(np.int64)
    x0, x1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1)
    y0, y1 = np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    z0, z1 = np.clip(iz, 0, D - 1), np.clip(iz + 1, 0, D - 1)
    b = lambda z, y, x: vol[z, y, x].astype(F)  # noqa: E731
    c00 = _fma(wx, b(z0, y0, x1) - b(z0, y0, x0), b(z0, y0, x0))
    c10 = _fma(wx, b(z0, y1, x1) - b(z0, y1, x0), b(z0, y1, x0))
    c01 = _fma(wx, b(z1, y0, x1) - b(z1, y0, x0), b(z1, y0, x0))
    c11 = _fma(wx, b(z1, y1, x1) - b(z1, y1, x0), b(z1, y1, x0))
    c0, c1 = _fma(wy, c10 - c00, c00), _fma(wy, c11 - c01, c01)
    return _fma(wz, c1 - c0, c0) * INV255


def rays_np(p, in_depth=None):
    """ray_setup<VKV_SKIP_NONE> (IEEE divisions) for every pixel of the whole image of RenderParams p: dict of per-pixel arrays (row-major,
    image_height x image_width flattened) fragment, marched, entry e, step s, n_steps, and the depth a pixel without colour gets."""
    w, h = p.image_width, p.image_height
    W, H, D = p.volume_extent.width, p.volume_extent.height, p.volume_extent.depth
    py_, px_ = np.mgrid[0:h, 0:w]
    fx, fy = px_.reshape(-1).astype(F) + F(0.5), py_.reshape(-1).astype(F) + F(0.5)
    rg, rc = p.ray_gen, p.ray_cast
    with np.errstate(all="ignore"):
        d = [_fma(fy, F(rg.ddy[a]), _fma(fx, F(rg.ddx[a]), F(rg.dir00[a]))) for a in range(3)]
        ln = np.sqrt(_fma(d[2], d[2], _fma(d[1], d[1], d[0] * d[0])))
        d = [x / ln for x in d]
        o = [F(rc.camera_pos_tex[a]) for a in range(3)]
        n = fx.size
        t_near, t_far = np.full(n, -np.inf, F), np.full(n, np.inf, F)
        miss = np.zeros(n, bool)
        for a in range(3):
            zero = d[a] == 0
            if o[a] < 0 or o[a] > 1:
                miss |= zero
            inv = F(1.0) / d[a]
            ta, tb = (F(0.0) - o[a]) * inv, (F(1.0) - o[a]) * inv
            t_near = np.where(zero, t_near, _gmax(t_near, _gmin(ta, tb)))
            t_far = np.where(zero, t_far, _gmin(t_far, _gmax(ta, tb)))
        pt = [F(x) for x in rc.plane_tex]
        Ap = _fma(pt[2], o[2], _fma(pt[1], o[1], pt[0] * o[0])) + pt[3]
        Bp = _fma(pt[2], d[2], _fma(pt[1], d[1], pt[0] * d[0]))
        t_plane = (F(0.0) - Ap) / Bp
        t0 = _gmax(t_near, t_plane)
        frag = ~miss & (Bp > 0) & (t0 < t_far)
        e = [_fma(t0, d[a], o[a]) for a in range(3)]
        cam = p.camera
        no_colour_depth = np.zeros(n, F)
        if p.options.depth_attachment:
            zd = np.asarray(in_depth, F).reshape(-1)
            no_colour_depth = zd.copy()
            pm = [e[0] - F(0.5), e[1] - F(0.5), e[2] - F(0.5), np.ones(n, F)]
            pos = _mat4_mul(cam.camera_proj, _mat4_mul(cam.camera_view, _mat4_mul(cam.model, pm)))
            front = pos[2] / pos[3]
            frag &= ~(zd > front)
        v = [e[a] - o[a] for a in range(3)]
        ln2 = np.sqrt(_fma(v[2], v[2], _fma(v[1], v[1], v[0] * v[0])))
        rd = [x / ln2 for x in v]
        iv = [F(1.0) / x for x in rd]
        t2 = [_gmax(-e[a] * iv[a], (F(1.0) - e[a]) * iv[a]) for a in range(3)]
        tfar = _gmin(_gmin(t2[0], t2[1]), t2[2])
        x = [_fma(tfar, rd[a], e[a]) for a in range(3)]
        vv = [e[a] - x[a] for a in range(3)]
        dist = np.sqrt(_fma(vv[2], vv[2], _fma(vv[1], vv[1], vv[0] * vv[0])))
        if p.options.depth_attachment:
            clip = [(pos[0] * zd) / front, (pos[1] * zd) / front, (pos[2] * zd) / front, pos[3]]
            w4 = _mat4_mul(cam.camera_view_proj_inv, clip)
            w4 = [w4[0] / w4[3], w4[1] / w4[3], w4[2] / w4[3], w4[3] / w4[3]]
            m4 = _mat4_mul(cam.model_inv, w4)
            ii = [m4[a] + F(0.5) for a in range(3)]
            dv = [e[a] - ii[a] for a in range(3)]
            dd = np.sqrt(_fma(dv[2], dv[2], _fma(dv[1], dv[1], dv[0] * dv[0])))
            dist = np.where(dd < dist, dd, dist)
        nf = np.ceil(F(max(W, H, D)) * dist * F(p.transfer_function.sampling_factor))
        ok = frag & (nf >= 2) & (nf <= 16777216)
        den = nf - F(1.0)
        s = [(rd[a] * dist) / den for a in range(3)]
        for a in range(3):
            q = e[a] + s[a]
            ok &= ~((q <= 0) | (q >= 1))
        ok &= np.isfinite(nf)
    n_steps = np.where(ok, nf, 0).astype(np.int64)
    return dict(fragment=frag, marched=ok, e=e, s=s, n_steps=n_steps, no_colour_depth=no_colour_depth)


def mip_np(p, vol, mip, in_depth=None):
    """The dense MIP of DESIGN.md §5.9 for the whole image of RenderParams p and MipOptions mip (threshold, window_max) over the (D, H, W)
    uint8 volume: dict of (h, w) arrays intensity, color (h, w, 4), rgba8 (h, w, 4), depth, n_steps, and second (the largest counted sample
    other than at index k, -inf if none: depth is only well defined where the top two differ)."""
    assert isinstance(mip, MipOptions) and mip.flags == 0
    threshold, window_max = F(mip.threshold), F(mip.window_max)
    R = rays_np(p, in_depth)
    w, h = p.image_width, p.image_height
    n = R["n_steps"]
    thr = F(threshold)
    best = np.full(n.size, thr, F)
    k = np.full(n.size, -1, np.int64)
    second = np.full(n.size, -np.inf, F)
    e, s = R["e"], R["s"]
    for i in range(int(n.max()) if n.size else 0):
        live = i < n
        fi = F(i)
        with np.errstate(all="ignore"):
            v = sample_linear_np(vol, _fma(fi, s[0], e[0]), _fma(fi, s[1], e[1]), _fma(fi, s[2], e[2]))
        v = np.where(live, v, F(0))
        up = live & (v > best)
        counted = live & (v > thr)
        second = np.where(up, np.where(k >= 0, best, second), np.where(counted, _gmax(second, v), second))
        best = np.where(up, v, best)
        k = np.where(up, i, k)
    found = k >= 0
    intensity = np.where(found, best, F(0))
    if window_max <= threshold:
        g = np.ones(n.size, F)
    else:
        g = np.clip((best - thr) / (F(window_max) - thr), F(0), F(1)).astype(F)
    g = np.where(found, g, F(0))
    a = np.where(found, F(1), F(0))
    color = np.stack([g, g, g, a], -1)
    rgba8 = np.rint(np.clip(color, 0, 1) * F(255)).astype(np.uint8)
    depth = R["no_colour_depth"].copy()
    if found.any():
        fk = k.astype(F)
        pm = [_fma(fk, s[0], e[0]) - F(0.5), _fma(fk, s[1], e[1]) - F(0.5), _fma(fk, s[2], e[2]) - F(0.5), np.ones(n.size, F)]
        cam = p.camera
        c4 = _mat4_mul(cam.camera_proj, _mat4_mul(cam.camera_view, _mat4_mul(cam.model, pm)))
        with np.errstate(all="ignore"):
            depth = np.where(found, c4[2] / c4[3], depth)
    shp = (h, w)
    return dict(intensity=intensity.reshape(shp), color=color.reshape(h, w, 4), rgba8=rgba8.reshape(h, w, 4), depth=depth.reshape(shp).astype(F),
                n_steps=n.reshape(shp), second=second.reshape(shp), found=found.reshape(shp))


# ---- a scene without the device: uniforms from the C helper -----------------------------------------------------------------------------

def params_np(extent_whd, image_size=(48, 40), azimuth=30.0, elevation=20.0, radius=150.0, sampling_factor=1.0, block=4):
    """RenderParams of an orbit camera through lib.build_uniforms (pure CPU)"""
    from vkvolume_amd import camera
    w, h, d = extent_whd
    ext = abi.Extent3D(w, h, d)
    mext = abi.Extent3D(-(-w // block), -(-h // block), -(-d // block))
    image_t = camera.image_transform((1.0, 1.0, 1.0), (w, h, d), (1.0, 0.0, 0.0, 0.0))
    node_t = camera.benchmark_node_transform(image_t)
    view, proj = camera.orbit_camera(azimuth, elevation, radius), camera.perspective_vulkan(60.0, image_size[0] / image_size[1])
    cam, rc, rg = lib.build_uniforms(view, proj, node_t, image_t, 50.0, image_size, ext, mext)
    p = abi.RenderParams()
    p.camera, p.ray_cast, p.ray_gen = cam, rc, rg
    p.transfer_function.sampling_factor = sampling_factor
    p.image_width, p.image_height = image_size
    p.tiles = abi.full_frame_tiles(*image_size)
    p.volume_extent, p.map_extent = ext, mext
    return p


# ---- tests ------------------------------------------------------------------------------------------------------------------------------

def test_mip_options_mirror_matches_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkvolume_amd.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(VkvMipOptions));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(VkvMipOptions, %s));\n' % (f, f) for f, _ in abi.MipOptions._fields_) +
                   "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().split("\n") if line.strip())
    assert int(out.pop("sizeof")) == C.sizeof(abi.MipOptions)
    assert len(out) == 5
    for f, _ in abi.MipOptions._fields_:
        assert int(out[f]) == getattr(abi.MipOptions, f).offset, f


def test_every_lerp_of_the_filter_lies_between_its_endpoints():
    # all byte pairs (a, b) and a dense set of weights in [0, 1), fp32 fma(w, b - a, a) through an exactly rounded float64 evaluation
    a, b = np.meshgrid(np.arange(256, dtype=F), np.arange(256, dtype=F), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    ws = np.concatenate([np.linspace(0, 1, 4097, dtype=F)[:-1], np.nextafter(F(1), F(0), dtype=F)[None],
                         np.random.default_rng(7).random(2048).astype(F)])
    for w in ws:
        w = F(w)
        if w >= 1:
            continue
        v = _fma(w, b - a, a)
        assert np.all((v >= lo) & (v <= hi)), float(w)
    # nested: a lerp of two values that lie between bytes lies between those bytes too (fma is correctly rounded and monotone)
    vals = np.arange(256, dtype=F) * INV255
    assert np.all(np.diff(vals) > 0), "x * kInv255 is not strictly increasing over 0..255"
    assert F(255) * INV255 <= F(1.0)


def test_max_map_np_on_analytic_volumes():
    # a ramp along x: a cell's byte is its grown box's last column
    W, H, D = 13, 7, 6
    vol = np.broadcast_to((np.arange(W, dtype=np.uint8) * 10)[None, None, :], (D, H, W)).copy()
    mm = max_map_np(vol, (4, 2, 2))  # block 4, 4, 3
    for cx in range(4):
        assert np.all(mm[:, :, cx] == 10 * min(cx * 4 + 4, W - 1))
    # a single bright voxel reaches the cells whose grown box holds it, nothing else
    vol = np.zeros((8, 8, 8), np.uint8)
    vol[4, 3, 5] = 200
    mm = max_map_np(vol, (4, 4, 4))  # block 2: cell c covers voxels 2c, 2c + 1, grown 2c - 1 .. 2c + 2
    hit = lambda c, v: 2 * c - 1 <= v <= 2 * c + 2  # noqa: E731
    want = np.array([[[200 if hit(cz, 4) and hit(cy, 3) and hit(cx, 5) else 0 for cx in range(4)] for cy in range(4)] for cz in range(4)], np.uint8)
    assert np.array_equal(mm, want)
    # map extents past the volume: block 2 over 10 voxels with 7 cells leaves cells 5 and 6 outside
    vol = np.full((3, 3, 10), 9, np.uint8)
    mm = max_map_np(vol, (7, 1, 1))
    assert list(mm[0, 0]) == [9, 9, 9, 9, 9, 0, 0]
    # the restatement against the definition, cell by cell, on random bytes
    rng = np.random.default_rng(3)
    vol = rng.integers(0, 256, (9, 11, 13), dtype=np.uint8)
    for me in ((4, 3, 3), (13, 11, 9), (5, 6, 7), (2, 2, 1)):
        mm = max_map_np(vol, me)
        bx, by, bz = -(-13 // me[0]), -(-11 // me[1]), -(-9 // me[2])
        for cz in range(me[2]):
            for cy in range(me[1]):
                for cx in range(me[0]):
                    if cx * bx >= 13 or cy * by >= 11 or cz * bz >= 9:
                        want = 0
                    else:
                        want = vol[max(cz * bz - 1, 0):cz * bz + bz + 1, max(cy * by - 1, 0):cy * by + by + 1, max(cx * bx - 1, 0):cx * bx + bx + 1].max()
                    assert mm[cz, cy, cx] == want, (me, cx, cy, cz)


def test_mip_np_on_analytic_volumes():
    # a single bright voxel in an empty volume: exactly the pixels whose rays pass near it count, their m is the filter's peak there
    W = H = D = 16
    vol = np.zeros((D, H, W), np.uint8)
    vol[8, 8, 8] = 255
    p = params_np((W, H, D), image_size=(32, 32), azimuth=0.0, elevation=0.0)
    r = mip_np(p, vol, MipOptions(threshold=0.0, window_max=1.0))
    assert r["found"].sum() > 0
    assert r["found"].sum() < 0.25 * r["found"].size
    assert float(r["intensity"].max()) <= 1.0
    assert np.all(r["rgba8"][..., 3][r["found"]] == 255) and np.all(r["rgba8"][~r["found"]] == 0)
    # the brightest pixel looks straight through the voxel's neighbourhood
    assert float(r["intensity"].max()) > 0.3
    # threshold above every sample: nothing counts
    r1 = mip_np(p, vol, MipOptions(threshold=1.0, window_max=1.0))
    assert not r1["found"].any() and np.all(r1["intensity"] == 0)
    # a ramp in z: every covered ray's maximum is its sample nearest the bright end, within one sample's step of the exact value
    z = np.arange(D, dtype=np.float64)
    vol = np.broadcast_to(np.round(z * 255 / (D - 1)).astype(np.uint8)[:, None, None], (D, H, W)).copy()
    p = params_np((W, H, D), image_size=(24, 24), azimuth=20.0, elevation=10.0)
    r = mip_np(p, vol, MipOptions(threshold=0.0, window_max=0.5))
    R = rays_np(p)
    m = R["marched"].reshape(24, 24)
    assert m.sum() > 100
    # the ramp is linear in z between voxel centres and clamped outside: the largest sample of a ray is the filtered value at its largest z
    e, s, n = R["e"], R["s"], R["n_steps"]
    zs = np.maximum(e[2], _fma((n - 1).astype(F), s[2], e[2]))
    want = np.clip((zs.astype(np.float64) * D - 0.5), 0, D - 1) * (255 / (D - 1)) / 255
    got = r["intensity"].reshape(-1)
    sel = R["marched"] & (r["found"].reshape(-1))
    assert np.allclose(got[sel], want[sel], atol=2.5 / 255)
    # grey window: g = clamp((m - 0) / 0.5, 0, 1)
    g = r["color"][..., 0].reshape(-1)
    assert np.allclose(g[sel], np.clip(got[sel] / np.float32(0.5), 0, 1), atol=1e-6)


def test_mip_kernels_use_no_scratch(tmp_path):
    if not os.path.exists(HIPCC) and shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^FLAGS\s*:=\s*(.*)$", text, flags=re.M)
    flags = [f.replace("$(ARCH)", "gfx950") for f in m.group(1).split() if not f.startswith("$(")]
    out = str(tmp_path / "mip.s")
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc"] + flags + ["--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, "mip.hip"), "-o", out]
    subprocess.run(cmd, check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
    kernels, name = {}, None
    for line in open(out):
        mm = re.match(r"^(_Z\w+):", line)
        if mm:
            name = mm.group(1)
        mm = re.match(r";\s*ScratchSize:\s*(\d+)", line)
        if mm and name:
            kernels[name] = int(mm.group(1))
    mip = {k: v for k, v in kernels.items() if "k_mip" in k}
    assert len(mip) == 4, kernels
    assert any("k_max_map" in k for k in kernels), kernels
    assert all(v == 0 for v in kernels.values()), kernels

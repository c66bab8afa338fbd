"""Maximum-intensity projection without a GPU: the ctypes mirror of VkvMipOptions against the C header, the two facts the skipping path's
exactness rests on (every lerp of the filter lies between its endpoints; x * kInv255 is monotone), the numpy restatements of
vkv_max_map (max_map_np) and of the dense MIP (mip_np) on analytic volumes, the correctly rounded fp32 fma of the restatements (_fma)
against an exact one, and the compiled MIP kernels' listing (no scratch).

max_map_np and mip_np are the references tests/test_gpu_mip.py compares the device against; max_map_skip_np restates the skip walk of both
renderers (tests/test_max_map_skip_cpu.py, tests/test_gpu_max_map_sweep.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from vkvolume_amd import abi, lib
from vkvolume_amd.abi import MipOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    """fp32 fma, correctly rounded: the product of two floats is exact in float64 (24 + 24 bits), TwoSum gives the rounding error of the
    float64 sum exactly, and the sum rounded to odd (53 >= 2 * 24 + 2 bits) then rounds to the float32 nearest the exact value.  (A plain
    float64 sum rounded twice can land on a float32 tie the exact value is not on.)  Non-finite operands give float64's inf / NaN."""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.asarray(s).view(np.uint64) & np.uint64(1)) == 0
        fix = np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return np.asarray(s).astype(F)


def _gmin(x, y):
    return np.where(y < x, y, x)


def _gmax(x, y):
    return np.where(x < y, y, x)


def _mat4_mul(m, v):
    """mat4_mul_vec4 of volume_sampling.hpp: m column-major float[16], v four arrays"""
    m = np.asarray(m, F)
    return [_fma(m[12 + i], v[3], _fma(m[8 + i], v[2], _fma(m[4 + i], v[1], F(m[i]) * v[0]))) for i in range(4)]


def sample_linear_np(vol, px, py, pz):
    """sample_linear of volume_sampling.hpp: clamp-to-edge trilinear filter, lerps as fma(w, b - a, a), times kInv255"""
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


def samples_np(vol, R):
    """every sample of every ray of rays_np's R: (rays, max n_steps) arrays v (the filtered intensity, 0 past a ray's n_steps) and cx, cy,
    cz (the sampler's voxel coordinates fma(pos, extent, -0.5) of each sample)"""
    D, H, W = vol.shape
    n, e, s = R["n_steps"], R["e"], R["s"]
    m = int(n.max()) if n.size else 0
    live = np.arange(m)[None, :] < n[:, None]
    fi = np.arange(m, dtype=F)[None, :]
    with np.errstate(all="ignore"):
        pos = [np.where(live, _fma(fi, s[a][:, None], e[a][:, None]), F(0.5)) for a in range(3)]  # (the dead samples read the centre)
        v = np.where(live, sample_linear_np(vol, *pos), F(0))
        cx, cy, cz = _fma(pos[0], F(W), F(-0.5)), _fma(pos[1], F(H), F(-0.5)), _fma(pos[2], F(D), F(-0.5))
    return dict(v=v, cx=cx, cy=cy, cz=cz, live=live)


def mip_walk_dense(v, n, threshold):
    """the dense MIP over a samples_np matrix: best (threshold if nothing counts) and k (the first index of the largest sample > threshold,
    -1 if none)"""
    best = np.full(n.size, F(threshold), F)
    k = np.full(n.size, -1, np.int64)
    for i in range(v.shape[1]):
        up = (i < n) & (v[:, i] > best)
        best = np.where(up, v[:, i], best)
        k = np.where(up, i, k)
    return best, k


def mip_np(p, vol, mip, in_depth=None, S=None):
    """The dense MIP of DESIGN.md §5.9 for the whole image of RenderParams p and MipOptions mip (threshold, window_max) over the (D, H, W)
    uint8 volume: dict of (h, w) arrays intensity, color (h, w, 4), rgba8 (h, w, 4), depth, n_steps, k (the first index of the largest
    counted sample, -1: none) and found.  S: samples_np of the same rays, if already at hand."""
    assert isinstance(mip, MipOptions) and mip.flags == 0
    threshold, window_max = F(mip.threshold), F(mip.window_max)
    R = rays_np(p, in_depth)
    w, h = p.image_width, p.image_height
    n = R["n_steps"]
    thr = F(threshold)
    e, s = R["e"], R["s"]
    best, k = mip_walk_dense((samples_np(vol, R) if S is None else S)["v"], n, thr)
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
                n_steps=n.reshape(shp), k=k.reshape(shp), found=found.reshape(shp))


KMAX_SAMPLE = F(255) * INV255  # kMaxSample of mip.hip: the largest value a sample can take


def max_map_geometry_np(extent_whd, map_extent_whd):
    """fill_max_map_geometry: per axis the block ceil(extent / map extent), the last cell that holds a voxel (extent - 1) / block, and
    1 / block as a float"""
    b = [-(-e // m) for e, m in zip(extent_whd, map_extent_whd)]
    return b, [(e - 1) // bb for e, bb in zip(extent_whd, b)], [F(1) / F(bb) for bb in b]


def _in_grown(c, lo, b):
    """in_grown of max_map_skip.hpp: c in [lo - 1, lo + b)"""
    return (c >= (lo - 1).astype(F)) & (c < (lo + b).astype(F))


def max_map_skip_np(p, vol, max_map, bound, strict, R=None, S=None):
    """The skip walk of the max-map MIP (strict=False: mip.hip's inline step, bound = the threshold) or of the max-map isosurface (strict=True:
    max_map_skip<true>, bound = iso) over the (md, mh, mw) max map and p.map_extent, with the device's float32 operations in order,
    vectorised over the rays of the whole image.  Per sample i of a ray: the cell of its voxel coordinates (clamped to the last cell that
    holds a voxel); on entering a cell other than the last probed one, a probe; when the byte cannot reach the bound (MIP: B * kInv255 <=
    max(threshold, best so far); iso: B * kInv255 < iso) and the sample lies in the grown cell, samples i .. i + kk are skipped (kk from the
    per-axis IEEE estimate, 0 unless sample i + kk lies in the grown cell too) and the next sample probes again.  Otherwise the sample is
    filtered; the MIP stops at kMaxSample (the rest counts as skipped), the isosurface at its hit.

    Returns a dict of flat per-ray arrays: best (MIP: max(threshold, largest sample)), k (MIP: first index of the largest sample > threshold;
    iso: first index of a sample >= iso; -1: none), n_filt, n_probe, n_skip (the kernel's counters), and skipped (rays, max n_steps) bool /
    skip_top (the byte value B * kInv255 of the cell each skipped sample was skipped by)."""
    if R is None:
        R = rays_np(p)
    if S is None:
        S = samples_np(vol, R)
    D, H, W = vol.shape
    me = (p.map_extent.width, p.map_extent.height, p.map_extent.depth)
    (bx, by, bz), (lcx, lcy, lcz), (rbx, rby, rbz) = max_map_geometry_np((W, H, D), me)
    mw, mh = me[0], me[1]
    n = R["n_steps"]
    N, M = S["v"].shape
    cx, cy, cz = S["cx"], S["cy"], S["cz"]
    # per sample, as the probe at that sample computes it: the cell, its byte, the grown-cell test, and the last index the skip would reach
    with np.errstate(all="ignore"):
        cell_of = lambda c, rb, lc: np.clip(np.floor((c + F(0.5)) * rb).clip(-2 ** 30, 2 ** 30).astype(np.int64), 0, lc)  # noqa: E731
        mx, my, mz = cell_of(cx, rbx, lcx), cell_of(cy, rby, lcy), cell_of(cz, rbz, lcz)
        cell = (mz * mh + my) * mw + mx
        top = max_map.reshape(-1)[cell].astype(F) * INV255
        lx, ly, lz = mx * bx, my * by, mz * bz
        grown = _in_grown(cx, lx, bx) & _in_grown(cy, ly, by) & _in_grown(cz, lz, bz)
        fW, fH, fD = F(W), F(H), F(D)

        def t_axis(step, scale, c, lo, b):
            sv = (step * scale)[:, None]
            up = ((lo + b).astype(F) - F(0.25) - c) / sv
            dn = (lo.astype(F) - F(0.75) - c) / sv
            return np.where(sv > 0, up, np.where(sv < 0, dn, F(np.inf))).astype(F)
        s = R["s"]
        tx, ty, tz = t_axis(s[0], fW, cx, lx, bx), t_axis(s[1], fH, cy, ly, by), t_axis(s[2], fD, cz, lz, bz)
        idx = np.arange(M)[None, :]
        rest = (n[:, None] - 1 - idx).astype(F)
        tm = _gmin(_gmin(tx, ty), _gmin(tz, rest))
        kk = np.where(tm > 0, np.floor(np.where(tm > 0, tm, F(0))).astype(np.int64), 0)
        j = np.clip(idx + kk, 0, max(M - 1, 0))
        rows = np.arange(N)[:, None]
        q_ok = _in_grown(cx[rows, j], lx, bx) & _in_grown(cy[rows, j], ly, by) & _in_grown(cz[rows, j], lz, bz)
        last = idx + np.where((kk > 0) & ~q_ok, 0, kk)
    # the walk: one event per active ray and round (a skip, or one filtered sample)
    v = S["v"]
    best = np.full(N, F(bound), F)
    k = np.full(N, -1, np.int64)
    i = np.zeros(N, np.int64)
    last_cell = np.full(N, -1, np.int64)
    n_filt, n_probe, n_skip = (np.zeros(N, np.int64) for _ in range(3))
    skip_start = np.zeros((N, M + 1), np.int64)
    skip_top = np.full((N, M), np.nan, F)
    done = i >= n
    while True:
        r = np.nonzero(~done)[0]
        if r.size == 0:
            break
        ii = i[r]
        c = cell[r, ii]
        probe = c != last_cell[r]
        n_probe[r] += probe
        last_cell[r] = np.where(probe, c, last_cell[r])
        t = top[r, ii]
        low = t < best[r] if strict else t <= best[r]
        sk = probe & low & grown[r, ii]
        # skips
        rs, i0, i1 = r[sk], ii[sk], last[r[sk], ii[sk]]
        n_skip[rs] += i1 + 1 - i0
        np.add.at(skip_start, (rs, i0), 1)
        np.add.at(skip_start, (rs, i1 + 1), -1)
        skip_top[rs, i0] = t[sk]
        i[rs] = i1 + 1
        last_cell[rs] = -1
        # filtered samples
        rf, fi = r[~sk], ii[~sk]
        n_filt[rf] += 1
        x = v[rf, fi]
        if strict:
            hit = x >= best[rf]
            k[rf[hit]] = fi[hit]
            done[rf[hit]] = True
        else:
            up = x > best[rf]
            best[rf] = np.where(up, x, best[rf])
            k[rf] = np.where(up, fi, k[rf])
            stop = best[rf] >= KMAX_SAMPLE
            n_skip[rf[stop]] += n[rf[stop]] - (fi[stop] + 1)
            done[rf[stop]] = True
        i[rf] = fi + 1
        done |= i >= n
    skipped = np.cumsum(skip_start, axis=1)[:, :M] > 0
    # the byte each skipped sample was skipped by: the one recorded at the start of its run
    start = np.where(~np.isnan(skip_top), np.arange(M)[None, :], -1)
    run = np.maximum.accumulate(start, axis=1)
    skip_top = np.where(skipped, skip_top[np.arange(N)[:, None], np.maximum(run, 0)], np.nan)
    return dict(best=best, k=k, n_filt=n_filt, n_probe=n_probe, n_skip=n_skip, skipped=skipped, skip_top=skip_top)


# ---- a scene without the device: uniforms from the C helper -----------------------------------------------------------------------------

def params_np(extent_whd, image_size=(48, 40), azimuth=30.0, elevation=20.0, radius=150.0, sampling_factor=1.0, block=4, map_extent=None,
              voxel_size=(1.0, 1.0, 1.0), axis_angle=(1.0, 0.0, 0.0, 0.0), clip=50.0):
    """RenderParams of an orbit camera through lib.build_uniforms (pure CPU); map_extent (w, h, d) overrides the one of `block`"""
    from vkvolume_amd import camera
    w, h, d = extent_whd
    ext = abi.Extent3D(w, h, d)
    mext = abi.Extent3D(*map_extent) if map_extent is not None else abi.Extent3D(-(-w // block), -(-h // block), -(-d // block))
    image_t = camera.image_transform(voxel_size, (w, h, d), axis_angle)
    node_t = camera.benchmark_node_transform(image_t)
    view, proj = camera.orbit_camera(azimuth, elevation, radius), camera.perspective_vulkan(60.0, image_size[0] / image_size[1])
    cam, rc, rg = lib.build_uniforms(view, proj, node_t, image_t, clip, image_size, ext, mext)
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
    kernels = {k: v["ScratchSize"] for k, v in T.kernel_listing("mip.hip", tmp_path / "mip.s").items()}
    mip = {k: v for k, v in kernels.items() if "k_mip" in k}
    assert len(mip) == 4, kernels
    assert any("k_max_map" in k for k in kernels), kernels
    assert all(v == 0 for v in kernels.values()), kernels


def test_fma_is_correctly_rounded():
    from tests.golden.frag_literal import _fma as fma_exact
    u = 2.0 ** -23
    cases = []
    for e1 in (-20, -3, 0, 1, 7, 30):
        for e2 in (-40, -5, 0, 2, 11):
            a, b, c = (1 + u) * 2.0 ** e1, 2.0 ** -24 * (1 - u) * 2.0 ** e2, (1 + u) * 2.0 ** (e1 + e2)
            # a * b + c lies just below a float32 tie, on which the float64 sum lands: rounding twice gives the even neighbour above
            cases += [(a, b, c), (-a, b, -c), (a, -b, -c), (b, a, c)]
    a, b, c = (np.array(x, F) for x in zip(*cases))
    got = _fma(a, b, c)
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    twice = (a.astype(np.float64) * b + c).astype(F)
    assert np.all(twice != want), "the constructed triples no longer show double rounding"
    assert _fma(F(1 + u), F(2.0 ** -24 * (1 - u)), F(1 + u)) == F(1 + u)
    # random operands over a wide range of exponents (normal float32 results), with sums that cancel
    rng = np.random.default_rng(17)
    m = 20000
    a = (rng.standard_normal(m) * 2.0 ** rng.integers(-30, 30, m)).astype(F)
    b = (rng.standard_normal(m) * 2.0 ** rng.integers(-30, 30, m)).astype(F)
    c = np.where(rng.random(m) < 0.3, -(a.astype(np.float64) * b), rng.standard_normal(m) * 2.0 ** rng.integers(-60, 60, m)).astype(F)
    c[:200] = 1.0
    b[:200] = (rng.integers(1, 1 << 24, 200) * 2.0 ** -48).astype(F)  # products near half an ulp of c
    got = _fma(a, b, c)
    want = np.array([fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F)
    ok = np.isfinite(want) & ((want == 0) | (np.abs(want) >= np.finfo(F).tiny))
    assert ok.sum() > 0.95 * m
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))
    # zeros (their signs as IEEE fma gives them) and the non-finite cases rays_np feeds it
    for x, y, z, r in ((0.0, 5.0, 0.0, 0.0), (-0.0, 5.0, 0.0, 0.0), (-0.0, 5.0, -0.0, -0.0), (0.0, -5.0, -0.0, -0.0), (2.0, 3.0, -6.0, 0.0),
                       (np.inf, 2.0, 1.0, np.inf), (np.inf, -2.0, 1.0, -np.inf), (1.0, 2.0, -np.inf, -np.inf), (np.inf, 0.0, 1.0, np.nan),
                       (np.inf, 1.0, -np.inf, np.nan), (np.nan, 1.0, 1.0, np.nan), (1.0, 1.0, np.nan, np.nan), (3e38, 3e38, 0.0, np.inf)):
        g = _fma(F(x), F(y), F(z))
        assert g.dtype == F
        if np.isnan(r):
            assert np.isnan(g), (x, y, z)
        else:
            assert g == r and np.signbit(g) == np.signbit(r), (x, y, z, g)
    # arrays of every shape broadcast as before
    assert _fma(np.ones((3, 1), F), np.ones(4, F), F(1)).shape == (3, 4)

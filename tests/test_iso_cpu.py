"""Isosurface without a GPU: the ctypes mirror of VkvIsoOptions against the C header, the numpy restatement of DESIGN.md §5.10 (iso_np) and
its own checks on analytic volumes, and the compiled isosurface kernels' listing (no scratch).

iso_np is the reference tests/test_gpu_iso.py compares the device against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_mip_cpu import _fma, _gmax, _gmin, _mat4_mul, params_np, rays_np, sample_linear_np, samples_np
from vkvolume_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def iso_options(iso, refine_steps=4, base_color=(1.0, 1.0, 1.0), ambient=0.1, diffuse=0.8, specular=0.3, shininess=32):
    return abi.IsoOptions(iso=iso, refine_steps=refine_steps, base_color=(C.c_float * 3)(*base_color), ambient=ambient, diffuse=diffuse,
                          specular=specular, shininess=shininess, flags=0)


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------------

def _dot3(a, b):
    """dot3 of iso.hip: fma(a2, b2, fma(a1, b1, a0 * b0))"""
    return _fma(a[2], b[2], _fma(a[1], b[1], F(a[0]) * b[0]))


def _clamp01(x):
    """g_clamp(x, 0, 1) of the device: g_min(g_max(x, 0), 1) with its select semantics"""
    return _gmin(_gmax(x, F(0)), F(1))


def power_bits(d, shininess):
    """d^shininess by binary exponentiation over bits 10 .. 0 (highest first; leading zero bits keep r = 1)"""
    r = np.ones_like(np.asarray(d, F))
    for bit in range(10, -1, -1):
        r = r * r
        if (shininess >> bit) & 1:
            r = r * d
    return r


def iso_walk_dense(v, n, iso):
    """the dense isosurface's hit over a samples_np matrix: the first index of a sample >= iso (-1: none)"""
    if v.shape[1] == 0:
        return np.full(n.size, -1, np.int64)
    hit = (np.arange(v.shape[1])[None, :] < n[:, None]) & (v >= F(iso))
    return np.where(hit.any(axis=1), hit.argmax(axis=1), -1).astype(np.int64)


def iso_np(p, vol, o, in_depth=None, S=None):
    """The isosurface of DESIGN.md §5.10 for the whole image of RenderParams p and IsoOptions o over the (D, H, W) uint8 volume: dict of
    (h, w)-shaped arrays color (h, w, 4), rgba8 (h, w, 4), depth, normal (h, w, 4), k (-1: no hit), t, n_steps, and the flat per-pixel
    hit point / refined value (for the self-checks).  S: samples_np of the same rays, if already at hand."""
    assert isinstance(o, abi.IsoOptions) and o.flags == 0
    R = rays_np(p, in_depth)
    w, h = p.image_width, p.image_height
    n = R["n_steps"]
    e, s = R["e"], R["s"]
    N = n.size
    iso = F(o.iso)
    D, H, W = vol.shape
    k = iso_walk_dense((samples_np(vol, R) if S is None else S)["v"], n, iso)
    with np.errstate(all="ignore"):
        found = k >= 0
        # refinement
        lo, hi = (k - 1).astype(F), k.astype(F)
        for _ in range(int(o.refine_steps)):
            mid = (lo + hi) * F(0.5)
            v = sample_linear_np(vol, _fma(mid, s[0], e[0]), _fma(mid, s[1], e[1]), _fma(mid, s[2], e[2]))
            up = v >= iso
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        t = np.where(k > 0, hi, F(0)).astype(F)
        P = [_fma(t, s[a], e[a]) for a in range(3)]
        v_hit = sample_linear_np(vol, *P)
        cam = p.camera
        c4 = _mat4_mul(cam.camera_proj, _mat4_mul(cam.camera_view, _mat4_mul(cam.model, [P[0] - F(0.5), P[1] - F(0.5), P[2] - F(0.5), np.ones(N, F)])))
        depth = np.where(found, c4[2] / c4[3], R["no_colour_depth"]).astype(F)
        # gradient: the tetrahedron taps
        dix, diy, diz = F(1) / F(W), F(1) / F(H), F(1) / F(D)
        t1 = sample_linear_np(vol, P[0] + dix, P[1] - diy, P[2] - diz)
        t2 = sample_linear_np(vol, P[0] - dix, P[1] - diy, P[2] + diz)
        t3 = sample_linear_np(vol, P[0] - dix, P[1] + diy, P[2] - diz)
        t4 = sample_linear_np(vol, P[0] + dix, P[1] + diy, P[2] + diz)
        gx = (((t1 - t2) - t3) + t4) * F(0.25)
        gy = (((-t1 - t2) + t3) + t4) * F(0.25)
        gz = (((-t1 + t2) - t3) + t4) * F(0.25)
        g = [gx * F(W), gy * F(H), gz * F(D)]
        mi, m = np.asarray(cam.model_inv, F), np.asarray(cam.model, F)
        nw = [_dot3(mi[4 * i:4 * i + 3], g) for i in range(3)]
        v = [-_dot3((m[i], m[4 + i], m[8 + i]), s) for i in range(3)]
        vl = np.sqrt(_dot3(v, v))
        v = [x / vl for x in v]
        l2 = _dot3(nw, nw)
        degenerate = (l2 == 0) | ~np.isfinite(l2)
        nl = np.sqrt(l2)
        nn = [x / nl for x in nw]
        flip = _dot3(nn, v) < 0
        nn = [np.where(degenerate, v[a], np.where(flip, -nn[a], nn[a])) for a in range(3)]
        d = _clamp01(_dot3(nn, v))
        spec = power_bits(d, int(o.shininess))
        L = (F(o.ambient) + F(o.diffuse) * d) + F(o.specular) * spec
        rgb = [_clamp01(F(o.base_color[c]) * L) for c in range(3)]
    zero = np.zeros(N, F)
    color = np.stack([np.where(found, rgb[0], zero), np.where(found, rgb[1], zero), np.where(found, rgb[2], zero), np.where(found, F(1), zero)], -1)
    rgba8 = np.rint(np.clip(color, 0, 1) * F(255)).astype(np.uint8)
    normal = np.stack([np.where(found, nn[0], zero), np.where(found, nn[1], zero), np.where(found, nn[2], zero), np.where(found, F(1), zero)], -1)
    return dict(color=color.reshape(h, w, 4), rgba8=rgba8.reshape(h, w, 4), depth=depth.reshape(h, w), normal=normal.astype(F).reshape(h, w, 4),
                k=k.reshape(h, w), t=t.reshape(h, w), n_steps=n.reshape(h, w), found=found.reshape(h, w), v_hit=v_hit, d=d, view=v)


# ---- tests ------------------------------------------------------------------------------------------------------------------------------

def test_iso_options_mirror_matches_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkvolume_amd.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(VkvIsoOptions));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(VkvIsoOptions, %s));\n' % (f, f) for f, _ in abi.IsoOptions._fields_) +
                   "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().split("\n") if line.strip())
    assert int(out.pop("sizeof")) == C.sizeof(abi.IsoOptions)
    assert len(out) == 10
    for f, _ in abi.IsoOptions._fields_:
        assert int(out[f]) == getattr(abi.IsoOptions, f).offset, f
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bint\s+vkv_render_isosurface\s*\(", header)


def test_binary_exponentiation_equals_repeated_multiplication():
    d = np.concatenate([np.linspace(0, 1, 257, dtype=F), np.random.default_rng(1).random(256).astype(F)])
    for e in range(1, 9):  # small exponents: r = d, d*d, (d*d)*d, ((d*d)*(d*d)) ... : the same roundings as the chain below for e <= 3
        want = d.copy()
        for _ in range(e - 1):
            want = want * d
        got = power_bits(d, e)
        if e <= 3:
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), e
        assert np.allclose(got, want, rtol=4 * e * 2.0 ** -24, atol=0), e
    assert np.all(power_bits(F(1), 1024) == 1) and np.all(power_bits(d, 1) == d)
    assert np.all(power_bits(F(0.5), 10) == F(0.5) ** 10)  # powers of two are exact


def test_constant_volume_hits_at_the_first_sample_facing_the_camera():
    W, H, D = 12, 10, 9
    vol = np.full((D, H, W), 200, np.uint8)
    p = params_np((W, H, D), image_size=(32, 24), azimuth=25.0, elevation=15.0)
    r = iso_np(p, vol, iso_options(0.5))
    R = rays_np(p)
    m = R["marched"].reshape(24, 32)
    assert m.sum() > 100
    assert np.all(r["k"][m] == 0) and np.all(r["k"][~m] == -1)
    assert np.all(r["t"][m] == 0)
    # a constant field has no gradient: n = v, d = 1 (to the rounding of v . v), L = ambient + diffuse + specular (clamped)
    nrm = r["normal"].reshape(-1, 4)
    sel = R["marched"]
    for a in range(3):
        assert np.array_equal(nrm[sel, a], r["view"][a][sel])
    assert np.all(np.abs(r["d"][sel] - 1) <= 2.0 ** -22)
    assert np.all(r["color"].reshape(-1, 4)[sel, :3] == 1) and np.all(r["rgba8"].reshape(-1, 4)[sel] == 255)
    assert np.all(r["rgba8"].reshape(-1, 4)[~sel] == 0) and np.all(nrm[~sel] == 0)
    # a darker surface: L = 0.1 + 0.8 + 0.3 = 1.2 times 0.25
    r2 = iso_options(0.5, base_color=(0.25, 0.5, 1.0))
    c = iso_np(p, vol, r2)["color"].reshape(-1, 4)[sel]
    assert np.allclose(c[:, 0], 0.25 * 1.2, rtol=1e-5) and np.allclose(c[:, 1], 0.5 * 1.2, rtol=1e-5) and np.all(c[:, 2] == 1)
    # above every sample: nothing hits; at or below zero: the first sample hits
    assert not iso_np(p, vol, iso_options(1.01))["found"].any()
    assert np.all(iso_np(p, np.zeros_like(vol), iso_options(0.0))["k"][m] == 0)


def test_refined_hit_lies_between_the_samples_and_reaches_iso():
    # a ramp along z seen from the low end: rays cross the iso level once, inside the volume
    W, H, D = 16, 16, 16
    z = np.arange(D, dtype=np.float64)
    vol = np.broadcast_to(np.round(z * 255 / (D - 1)).astype(np.uint8)[:, None, None], (D, H, W)).copy()
    p = params_np((W, H, D), image_size=(24, 24), azimuth=200.0, elevation=10.0)
    for steps in (0, 4, 16):
        r = iso_np(p, vol, iso_options(0.45, refine_steps=steps))
        k, t, found = r["k"].reshape(-1), r["t"].reshape(-1), r["found"].reshape(-1)
        assert found.sum() > 50
        inner = found & (k > 0)
        assert inner.sum() > 20
        assert np.all(t[inner] >= k[inner] - 1) and np.all(t[inner] <= k[inner])
        assert np.all(r["v_hit"][found] >= F(0.45))
        if steps == 0:
            assert np.array_equal(t[found], k[found].astype(F))
        # the hit's normal is the ramp's: unit length, on the camera's side
        nrm = r["normal"].reshape(-1, 4)[found]
        assert np.allclose(np.linalg.norm(nrm[:, :3].astype(np.float64), axis=1), 1, atol=1e-5)
        assert np.all(nrm[:, 3] == 1)
    # more steps bring the hit nearer the crossing: the refined value approaches iso from above
    v0 = iso_np(p, vol, iso_options(0.45, refine_steps=0))["v_hit"]
    v16 = iso_np(p, vol, iso_options(0.45, refine_steps=16))["v_hit"]
    f = iso_np(p, vol, iso_options(0.45, refine_steps=0))["found"].reshape(-1)
    assert np.all(v16[f] <= v0[f]) and float(np.mean(v16[f] - F(0.45))) < float(np.mean(v0[f] - F(0.45)))


def test_iso_kernels_use_no_scratch(tmp_path):
    kernels = {k: v["ScratchSize"] for k, v in T.kernel_listing("iso.hip", tmp_path / "iso.s").items()}
    iso = {k: v for k, v in kernels.items() if "k_iso" in k}
    assert len(iso) == 4, kernels
    assert all(v == 0 for v in iso.values()), kernels

"""Oblique slices and thick slabs (vkv_render_slab) without a GPU: the ctypes mirror of VkvSlabOptions against the C header,
the numpy restatement of the definition (slab_np) with its self-checks on analytic volumes, the skip walk over the max map restated through
max_map_skip_np (slab_skip_np) against the dense restatement over many geometries and on a sparse scene, camera.slab_plane, and the compiled
slab kernels' listing (no scratch, one kernel per combination the launcher can select).

slab_np and slab_skip_np are the references tests/test_gpu_slab.py compares the device against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_mip_cpu import INV255, KMAX_SAMPLE, _fma, max_map_np, max_map_skip_np, sample_linear_np
from vkvolume_amd import abi, camera, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
MODES = (abi.SLAB_MAX, abi.SLAB_MIN, abi.SLAB_MEAN)


# ---- parameter blocks ------------------------------------------------------------------------------------------------------------------

def slab_params(extent_whd, image_size, block=4, map_extent=None):
    """the RenderParams a slab reads: image size, whole-image schedule, extents; camera, uniforms and transfer function stay zero"""
    w, h, d = extent_whd
    p = abi.RenderParams()
    p.image_width, p.image_height = image_size
    p.tiles = abi.full_frame_tiles(*image_size)
    p.volume_extent = abi.Extent3D(w, h, d)
    p.map_extent = abi.Extent3D(*map_extent) if map_extent is not None else abi.Extent3D(-(-w // block), -(-h // block), -(-d // block))
    return p


def slab_options(plane, samples=None, mode=abi.SLAB_MAX, window=(0.0, 1.0)):
    """abi.SlabOptions of a camera.slab_plane dict (or any dict with origin, du, dv, dn); samples defaults to the plane's"""
    vec = lambda a: (C.c_float * 3)(*[float(x) for x in a])  # noqa: E731
    return abi.SlabOptions(origin=vec(plane["origin"]), du=vec(plane["du"]), dv=vec(plane["dv"]), dn=vec(plane["dn"]),
                           samples=int(plane.get("samples", 1) if samples is None else samples), mode=int(mode), window_min=float(window[0]),
                           window_max=float(window[1]), flags=0)


# ---- numpy restatements ----------------------------------------------------------------------------------------------------------------

def slab_samples_np(p, vol, o):
    """every sample of every pixel of the whole image: q (three (pixels, samples) arrays: fma(j, dn, fma(y, dv, fma(x, du, origin)))), counted
    (0 <= q <= 1 on all axes, tested per sample), v (the filtered intensity of the counted samples, 0 elsewhere) and the base points"""
    w, h = p.image_width, p.image_height
    ys, xs = np.mgrid[0:h, 0:w]
    fx, fy = xs.reshape(-1).astype(F), ys.reshape(-1).astype(F)
    base = [_fma(fy, F(o.dv[c]), _fma(fx, F(o.du[c]), F(o.origin[c]))) for c in range(3)]
    fj = np.arange(o.samples, dtype=F)[None, :]
    q = [_fma(fj, F(o.dn[c]), base[c][:, None]) for c in range(3)]
    counted = np.ones(q[0].shape, bool)
    for c in range(3):
        counted &= (q[c] >= F(0)) & (q[c] <= F(1))
    pos = [np.where(counted, q[c], F(0.5)) for c in range(3)]  # (the samples that do not count read the centre)
    v = np.where(counted, sample_linear_np(vol, *pos), F(0))
    return dict(q=q, pos=pos, counted=counted, v=v, base=base)


def _grey(value, found, o):
    wmin, wmax = F(o.window_min), F(o.window_max)
    if wmax <= wmin:
        g = np.ones(value.shape, F)
    else:
        with np.errstate(all="ignore"):
            g = np.clip((value - wmin) / (wmax - wmin), F(0), F(1)).astype(F)
    g = np.where(found, g, F(0))
    a = np.where(found, F(1), F(0))
    color = np.stack([g, g, g, a], -1)
    return color, np.rint(np.clip(color, 0, 1) * F(255)).astype(np.uint8)


def slab_np(p, vol, o, S=None):
    """vkv_render_slab of DESIGN.md §5.11 for the whole image of RenderParams p and SlabOptions o over the (D, H, W) uint8 volume, dense: dict
    of flat per-pixel arrays value, color (n, 4), rgba8 (n, 4), count (the counted samples) and lo, hi (the counted indices are lo .. hi - 1;
    asserted contiguous)"""
    assert isinstance(o, abi.SlabOptions) and o.flags == 0 and 1 <= o.samples <= 4096 and o.mode in MODES
    if S is None:
        S = slab_samples_np(p, vol, o)
    counted, v = S["counted"], S["v"]
    count = counted.sum(axis=1)
    found = count > 0
    lo = np.where(found, counted.argmax(axis=1), 0)
    hi = lo + count
    j = np.arange(o.samples)[None, :]
    assert np.array_equal(counted, (j >= lo[:, None]) & (j < hi[:, None])), "the counted samples of a pixel are not one range"
    if o.mode == abi.SLAB_MAX:
        value = np.where(counted, v, F(-np.inf)).max(axis=1)
    elif o.mode == abi.SLAB_MIN:
        value = np.where(counted, v, F(np.inf)).min(axis=1)
    else:
        acc = np.zeros(count.size, F)
        for i in range(o.samples):  # in rising order; a sample that does not count adds +0, which changes no bit of a sum >= 0
            acc = (acc + np.where(counted[:, i], v[:, i], F(0))).astype(F)
        with np.errstate(all="ignore"):
            value = acc / count.astype(F)
    value = np.where(found, value, F(0)).astype(F)
    color, rgba8 = _grey(value, found, o)
    return dict(value=value, color=color, rgba8=rgba8, count=count, lo=lo, hi=hi)


def slab_skip_np(p, vol, max_map, o, S=None):
    """The skipping MAX slab: every pixel's column walks like a MIP ray with e = the base point, s = dn over its counted range, through
    max_map_skip_np (bound -inf: there is no best before the first filtered sample).  The walk's sample index is counted from the first
    counted sample; positions, voxel coordinates and values are those of the absolute index, as the kernel computes them.  Returns slab_np's
    arrays plus counts (n, 3): samples filtered, max-map bytes read, samples skipped."""
    assert o.mode == abi.SLAB_MAX
    if S is None:
        S = slab_samples_np(p, vol, o)
    D, H, W = vol.shape
    dense = slab_np(p, vol, o, S)
    lo, count = dense["lo"], dense["count"]
    n_pix = count.size
    M = int(count.max()) if n_pix else 0
    if M == 0:
        return dict(dense, counts=np.zeros((n_pix, 3), np.int64))
    col = np.arange(M)[None, :]
    live = col < count[:, None]
    take = np.minimum(lo[:, None] + col, o.samples - 1)
    rows = np.arange(n_pix)[:, None]
    pos = [np.where(live, S["pos"][c][rows, take], F(0.5)) for c in range(3)]
    Sw = dict(v=np.where(live, S["v"][rows, take], F(0)), live=live, cx=_fma(pos[0], F(W), F(-0.5)), cy=_fma(pos[1], F(H), F(-0.5)),
              cz=_fma(pos[2], F(D), F(-0.5)))
    R = dict(n_steps=count.astype(np.int64), s=[np.full(n_pix, F(o.dn[c]), F) for c in range(3)])
    w = max_map_skip_np(p, vol, max_map, F(-np.inf), False, R, Sw)
    found = count > 0
    value = np.where(found, w["best"], F(0)).astype(F)
    color, rgba8 = _grey(value, found, o)
    return dict(value=value, color=color, rgba8=rgba8, count=count, lo=lo, hi=dense["hi"],
                counts=np.stack([w["n_filt"], w["n_probe"], w["n_skip"]], -1), skipped=w["skipped"], skip_top=w["skip_top"], walk_v=Sw["v"])


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------

def random_plane(rng, extent_whd, image_size, samples=None):
    """an oblique plane through (or near, or beside) the volume: random normal and up, centre within 0.7 extents of the volume's centre,
    pixel and sample steps of 0.3 .. 1.6 voxels"""
    ext = np.asarray(extent_whd, np.float64)
    n = rng.standard_normal(3)
    up = rng.standard_normal(3)
    centre = (ext - 1) * 0.5 + rng.uniform(-0.7, 0.7, 3) * ext
    sv = float(rng.uniform(0.3, 1.6))
    k = int(rng.integers(1, 40)) if samples is None else samples
    return camera.slab_plane(extent_whd, centre, n, up, image_size, pixel_voxels=float(rng.uniform(0.3, 1.6)), thickness_voxels=(k - 1) * sv,
                             sample_voxels=sv)


def sparse_scene():
    """a bright ball of radius 12 (a quarter of the extent) in a zero background of 48^3 voxels, map block 4, an axial slab that spans the
    volume at one sample per voxel centre: (vol, params, options)"""
    D = H = W = 48
    zz, yy, xx = np.mgrid[0:D, 0:H, 0:W]
    r = np.sqrt((xx - 23.5) ** 2 + (yy - 23.5) ** 2 + (zz - 23.5) ** 2)
    vol = np.where(r <= 12.0, np.clip(250 - 10 * r, 0, 255), 0).astype(np.uint8)
    plane = camera.slab_plane((W, H, D), axis="z", index=(D - 1) * 0.5, thickness_voxels=D - 1)
    assert plane["samples"] == D
    return vol, slab_params((W, H, D), plane["image_size"], block=4), slab_options(plane)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- tests -----------------------------------------------------------------------------------------------------------------------------

def test_slab_options_mirror_matches_the_header(tmp_path):
    fields = [f for f, _ in abi.SlabOptions._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkvolume_amd.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(VkvSlabOptions));\n'
                   '  printf("modes %d%d%d\\n", VKV_SLAB_MAX, VKV_SLAB_MIN, VKV_SLAB_MEAN);\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(VkvSlabOptions, %s));\n' % (f, f) for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().split("\n") if line.strip())
    assert int(out.pop("sizeof")) == C.sizeof(abi.SlabOptions)
    assert out.pop("modes") == "%d%d%d" % (abi.SLAB_MAX, abi.SLAB_MIN, abi.SLAB_MEAN) == "012"
    assert len(out) == 11 == len(fields)
    for f in fields:
        assert int(out[f]) == getattr(abi.SlabOptions, f).offset, f
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bint\s+vkv_render_slab\s*\(\s*vkv_ctx\s*\*ctx,\s*const VkvRenderParams\s*\*params,\s*const VkvSlabOptions\s*\*slab,\s*void\s*\*stream\)",
                     header)
    assert "vkv_render_slab" in lib.EXPORTS


@pytest.mark.parametrize("axis", ["z", "y", "x"])
def test_axis_presets_on_power_of_two_extents_return_the_voxels(axis):
    rng = np.random.default_rng(4)
    W, H, D = 32, 16, 8
    vol = rng.integers(0, 256, (D, H, W), dtype=np.uint8)
    a = "xyz".index(axis)
    for k in (0, 3, (W, H, D)[a] - 1):
        plane = camera.slab_plane((W, H, D), axis=axis, index=k)
        assert plane["samples"] == 1
        p = slab_params((W, H, D), plane["image_size"])
        w, h = plane["image_size"]
        want = {"z": lambda: vol[k], "y": lambda: vol[:, k, :], "x": lambda: vol[:, :, k]}[axis]()
        assert want.shape == (h, w)
        for mode in MODES:
            r = slab_np(p, vol, slab_options(plane, mode=mode))
            assert np.all(r["count"] == 1)
            assert np.array_equal(bits(r["value"].reshape(h, w)), bits(want.astype(F) * INV255)), (axis, k, mode)
            assert np.array_equal(r["rgba8"][:, 0].reshape(h, w), np.rint(np.clip(want.astype(F) * INV255, 0, 1) * F(255)).astype(np.uint8))
            assert np.all(r["rgba8"][:, 3] == 255)


def test_full_depth_slabs_equal_the_column_extremes_and_mean_of_a_constant():
    rng = np.random.default_rng(5)
    W, H, D = 16, 8, 32
    vol = rng.integers(0, 256, (D, H, W), dtype=np.uint8)
    plane = camera.slab_plane((W, H, D), axis="z", index=(D - 1) * 0.5, thickness_voxels=D - 1)
    assert plane["samples"] == D and plane["image_size"] == (W, H)
    p = slab_params((W, H, D), (W, H))
    r = slab_np(p, vol, slab_options(plane, mode=abi.SLAB_MAX))
    assert np.all(r["count"] == D)
    assert np.array_equal(bits(r["value"].reshape(H, W)), bits(vol.max(axis=0).astype(F) * INV255))
    r = slab_np(p, vol, slab_options(plane, mode=abi.SLAB_MIN))
    assert np.array_equal(bits(r["value"].reshape(H, W)), bits(vol.min(axis=0).astype(F) * INV255))
    # MEAN of a constant volume is the constant: exactly for 0; for c * kInv255 within the rounding of the n - 1 additions (each partial sum
    # is rounded once: relative error <= (n - 1) * 2^-24 to first order) and of the division
    r = slab_np(p, np.zeros((D, H, W), np.uint8), slab_options(plane, mode=abi.SLAB_MEAN))
    assert np.all(r["value"] == 0) and np.all(r["rgba8"][:, :3] == 0) and np.all(r["rgba8"][:, 3] == 255)
    const = np.full((D, H, W), 77, np.uint8)
    r = slab_np(p, const, slab_options(plane, mode=abi.SLAB_MEAN))
    assert np.allclose(r["value"], float(F(77) * INV255), rtol=(D + 1) * 2.0 ** -24, atol=0)
    prng = np.random.default_rng(6)
    seen = 0
    for _ in range(8):
        pl = random_plane(prng, (W, H, D), (20, 12), samples=23)
        r = slab_np(slab_params((W, H, D), (20, 12)), const, slab_options(pl, mode=abi.SLAB_MEAN))
        f = r["count"] > 0
        seen += int(f.sum())
        assert np.allclose(r["value"][f], float(F(77) * INV255), rtol=24 * 2.0 ** -24, atol=0)
        assert np.all(r["value"][~f] == 0)
    assert seen > 200


def test_planes_outside_and_partly_outside_the_volume():
    rng = np.random.default_rng(8)
    W, H, D = 20, 17, 9
    vol = rng.integers(1, 256, (D, H, W), dtype=np.uint8)  # no zero voxel: a counted sample has a value > 0
    size = (24, 18)
    p = slab_params((W, H, D), size)
    # wholly outside: an axial plane below the volume, and one a slab's thickness above it
    for index, thick in ((-3.0, 0.0), (D + 6.0, 4.0), (-0.51, 0.0)):
        plane = camera.slab_plane((W, H, D), axis="z", index=index, thickness_voxels=thick, image_size=size)
        for mode in MODES:
            r = slab_np(p, vol, slab_options(plane, mode=mode))
            assert np.all(r["count"] == 0) and np.all(r["value"] == 0) and np.all(r["color"] == 0) and np.all(r["rgba8"] == 0)
    # grazing the faces: texture coordinate exactly 0 and exactly 1 count (power-of-two width and height: the in-plane positions are exact)
    gw, gh = 16, 8
    gvol = rng.integers(1, 256, (D, gh, gw), dtype=np.uint8)
    for index in (-0.5, D - 0.5):
        plane = camera.slab_plane((gw, gh, D), axis="z", index=index)
        assert plane["origin"][2] == (F(0) if index < 0 else F(1))
        r = slab_np(slab_params((gw, gh, D), (gw, gh)), gvol, slab_options(plane))
        assert np.all(r["count"] == 1)
        assert np.array_equal(bits(r["value"].reshape(gh, gw)), bits(gvol[0 if index < 0 else D - 1].astype(F) * INV255))
    # oblique, partly outside: zeros exactly where no sample counts
    partly = 0
    for _ in range(12):
        plane = random_plane(rng, (W, H, D), size)
        for mode in MODES:
            o = slab_options(plane, mode=mode, window=(0.0, 0.5))
            r = slab_np(p, vol, o)
            none = r["count"] == 0
            assert np.all(r["value"][none] == 0) and np.all(r["rgba8"][none] == 0) and np.all(r["color"][none] == 0)
            assert np.all(r["value"][~none] > 0) and np.all(r["rgba8"][~none][:, 3] == 255) and np.all(r["color"][~none][:, 3] == 1)
        partly += int(none.any() and (~none).any())
    assert partly >= 4


def test_counted_samples_are_one_range_over_random_planes():
    rng = np.random.default_rng(9)
    vol = np.zeros((5, 6, 7), np.uint8)
    counted_some = 0
    for case in range(60):
        ext = tuple(int(x) for x in rng.integers(1, 40, 3))
        size = (int(rng.integers(1, 30)), int(rng.integers(1, 30)))
        plane = random_plane(rng, ext, size, samples=int(rng.choice([1, 2, 17, 64, 256])))
        if case % 5 == 0:  # steps with zero components, and tiny ones
            plane["dn"] = plane["dn"] * np.array([0, 1, rng.choice([0, 1e-6])], F)
        o = slab_options(plane)
        S = slab_samples_np(slab_params((7, 6, 5), size), vol, o)
        c = S["counted"]
        count = c.sum(axis=1)
        first = np.where(count > 0, c.argmax(axis=1), 0)
        j = np.arange(o.samples)[None, :]
        assert np.array_equal(c, (j >= first[:, None]) & (j < (first + count)[:, None])), case
        counted_some += int(count.sum() > 0)
    assert counted_some > 30


def _skip_equals_dense(p, vol, mm, o, what):
    S = slab_samples_np(p, vol, o)
    dense = slab_np(p, vol, o, S)
    fast = slab_skip_np(p, vol, mm, o, S)
    for k in ("value", "color", "rgba8"):
        assert np.array_equal(bits(fast[k]), bits(dense[k])), (what, k)
    c = fast["counts"]
    assert np.array_equal(c[:, 0] + c[:, 2], dense["count"]), what
    assert np.all(c[:, 0][dense["count"] > 0] >= 1), what  # the first counted sample is always filtered
    if "skipped" in fast:
        sk = fast["skipped"]
        assert np.all(fast["walk_v"][sk] <= fast["skip_top"][sk]), (what, "a skipped sample exceeds its cell's byte")
    return int(c[:, 2].sum()), int(dense["count"].sum())


@pytest.mark.parametrize("family", ["random", "bright_voxels", "blobs"])
def test_skip_walk_equals_dense_over_geometries(family):
    rng = np.random.default_rng(["random", "bright_voxels", "blobs"].index(family) * 100 + 31)
    skipped = counted = 0
    for case in range(36):
        ext = tuple(int(x) | 1 if rng.random() < 0.7 else int(x) for x in rng.integers(1, 30, 3))  # mostly odd extents
        w, h, d = ext
        block = int(rng.integers(2, 7))
        me = tuple(-(-e // block) for e in ext)
        if family == "random":
            vol = rng.integers(0, 256, (d, h, w), dtype=np.uint8)
            vol[vol < 200] //= 4
        elif family == "bright_voxels":
            vol = rng.integers(0, 16, (d, h, w), dtype=np.uint8)
            for _ in range(int(rng.integers(1, 8))):
                vol[int(rng.integers(0, d)), int(rng.integers(0, h)), int(rng.integers(0, w))] = int(rng.integers(100, 256))
        else:
            zz, yy, xx = np.mgrid[0:d, 0:h, 0:w]
            c = rng.uniform(0, 1, 3) * (w, h, d)
            r = np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2)
            vol = np.clip(255 - 40 * r, 0, 255).astype(np.uint8)
        mm = max_map_np(vol, me)
        size = (int(rng.integers(5, 22)), int(rng.integers(5, 22)))
        p = slab_params(ext, size, map_extent=me)
        kind = case % 4
        if kind == 3:  # axis presets grazing a face, slab towards the inside and past the far face
            axis = "xyz"[int(rng.integers(0, 3))]
            e = ext["xyz".index(axis)]
            plane = camera.slab_plane(ext, axis=axis, index=float(rng.choice([-0.5, e - 0.5, 0.0, e - 1.0])), image_size=size)
            sign = F(1) if rng.random() < 0.5 else F(-1)
            plane["dn"] = plane["dn"] * sign * F(rng.choice([0.5, 1.0, 1.0 / 3.0]))
            samples = int(rng.integers(1, 3 * e + 2))
        else:
            plane = random_plane(rng, ext, size)
            samples = plane["samples"] if kind else int(rng.choice([1, 2, 17, 120]))
        s, c = _skip_equals_dense(p, vol, mm, slab_options(plane, samples=samples), (family, case, ext, block))
        skipped, counted = skipped + s, counted + c
    assert counted > 2000, counted
    assert skipped > 0 or family == "random", (counted, skipped)  # (bright noise in every cell leaves nothing to skip)


def test_skip_walk_skips_on_the_sparse_scene():
    vol, p, o = sparse_scene()
    assert o.samples == 48 and vol.max() >= 200 and (vol > 0).mean() < 0.08
    mm = max_map_np(vol, (p.map_extent.width, p.map_extent.height, p.map_extent.depth))
    skipped, counted = _skip_equals_dense(p, vol, mm, o, "sparse")
    assert counted == 48 * 48 * 48
    assert skipped >= 0.5 * counted, (skipped, counted)
    assert float(slab_np(p, vol, o)["value"].max()) <= float(KMAX_SAMPLE)


def test_slab_plane_frames():
    rng = np.random.default_rng(12)
    for _ in range(40):
        ext = rng.integers(1, 300, 3).astype(np.float64)
        size = (int(rng.integers(1, 200)), int(rng.integers(1, 200)))
        centre = rng.uniform(-20, 320, 3)
        pv, sv = float(rng.uniform(0.1, 3.0)), float(rng.uniform(0.1, 3.0))
        thick = float(rng.uniform(0, 30))
        pl = camera.slab_plane(tuple(int(e) for e in ext), centre, rng.standard_normal(3), rng.standard_normal(3), size, pixel_voxels=pv,
                               thickness_voxels=thick, sample_voxels=sv)
        assert all(pl[k].dtype == F and pl[k].shape == (3,) for k in ("origin", "du", "dv", "dn"))
        assert pl["samples"] == max(1, int(round(thick / sv)) + 1) and pl["image_size"] == size
        u, v, n = (pl[k].astype(np.float64) * ext for k in ("du", "dv", "dn"))  # back in voxel space
        for a, b in ((u, v), (u, n), (v, n)):
            assert abs(np.dot(a, b)) <= 1e-6 * np.linalg.norm(a) * np.linalg.norm(b) + 1e-12
        assert np.isclose(np.linalg.norm(u), pv, rtol=1e-6) and np.isclose(np.linalg.norm(v), pv, rtol=1e-6)
        assert np.isclose(np.linalg.norm(n), sv, rtol=1e-6)
        assert np.dot(np.cross(u, v), n) > 0  # du x dv points along dn
        # the image centre, at the slab's middle sample, maps to centre_voxel (voxel coordinate c <-> texture (c + 0.5) / extent)
        mid = (pl["origin"].astype(np.float64) + 0.5 * (size[0] - 1) * pl["du"] + 0.5 * (size[1] - 1) * pl["dv"] + 0.5 * (pl["samples"] - 1) * pl["dn"])
        scale = np.abs(centre).max() + np.abs(ext).max() + 200 * pv + 40 * sv
        assert np.allclose(mid * ext - 0.5, centre, rtol=0, atol=2e-5 * scale)
    with pytest.raises(ValueError):
        camera.slab_plane((8, 8, 8), (4, 4, 4), (0, 0, 1), (0, 0, 2), (8, 8))
    # the presets, exactly
    W, H, D = 40, 24, 10
    k = 7
    z = camera.slab_plane((W, H, D), axis="z", index=k)
    assert z["image_size"] == (W, H) and z["samples"] == 1
    assert np.array_equal(z["origin"], np.array([0.5 / W, 0.5 / H, (k + 0.5) / D], F))
    assert np.array_equal(z["du"], np.array([1.0 / W, 0, 0], F)) and np.array_equal(z["dv"], np.array([0, 1.0 / H, 0], F))
    assert np.array_equal(z["dn"], np.array([0, 0, 1.0 / D], F))
    y = camera.slab_plane((W, H, D), axis="y", index=k)
    assert y["image_size"] == (W, D)
    assert np.array_equal(y["origin"], np.array([0.5 / W, (k + 0.5) / H, 0.5 / D], F))
    assert np.array_equal(y["du"], np.array([1.0 / W, 0, 0], F)) and np.array_equal(y["dv"], np.array([0, 0, 1.0 / D], F))
    assert np.array_equal(y["dn"], np.array([0, 1.0 / H, 0], F))
    x = camera.slab_plane((W, H, D), axis="x", index=k)
    assert x["image_size"] == (H, D)
    assert np.array_equal(x["origin"], np.array([(k + 0.5) / W, 0.5 / H, 0.5 / D], F))
    assert np.array_equal(x["du"], np.array([0, 1.0 / H, 0], F)) and np.array_equal(x["dv"], np.array([0, 0, 1.0 / D], F))
    assert np.array_equal(x["dn"], np.array([1.0 / W, 0, 0], F))
    # a thick preset is centred on its slice
    t = camera.slab_plane((W, H, D), axis="z", index=k, thickness_voxels=4.0, sample_voxels=0.5)
    assert t["samples"] == 9
    assert np.isclose(float(t["origin"][2]) + 4 * float(t["dn"][2]), (k + 0.5) / D, rtol=1e-6)


def test_slab_kernels_use_no_scratch(tmp_path):
    kernels = {k: v["ScratchSize"] for k, v in T.kernel_listing("slab.hip", tmp_path / "slab.s").items()}
    slab = {k: v for k, v in kernels.items() if "k_slab" in k}
    # the launcher selects: two layouts x (MAX dense, MAX skipping, MIN, MEAN)
    assert len(slab) == 8 and len(kernels) == 8, kernels
    assert all(v == 0 for v in kernels.values()), kernels

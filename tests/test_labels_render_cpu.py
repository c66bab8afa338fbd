"""Label render without a GPU: the ctypes mirror of VkvLabelRenderOptions against the C header, the two fp32 facts the definition rests on
(a table byte survives base = byte * kInv255 and the RGBA8 rounding; 255 * kInv255 == 1, so a visibility byte of 255 is never skipped), the
numpy restatement of DESIGN.md §5.21 (labels_np) with its own checks on the scene the GPU tests use, the skip walk over the visibility map
against the dense walk from numpy alone, the host palette, and the compiled kernels' listing (no scratch).

labels_np and visibility_map_np are the references tests/test_gpu_labels_render.py compares the device against."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import vkv_oracle as O
from tests import helpers as T
from tests.test_components_cpu import components_np
from tests.test_iso_cpu import _clamp01, _dot3, iso_walk_dense, power_bits
from tests.test_mip_cpu import INV255, _fma, _mat4_mul, max_map_np, max_map_skip_np, params_np, rays_np, sample_linear_np
from vkvolume_amd import abi, labels as LB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPE, SEED, ISO = (37, 29, 23), 5, 0.5
BOX = (3, 2, 1, 30, 24, 20)
SIZE = (48, 40)
CAMERAS = [(30.0, 20.0, 150.0, 50.0), (200.0, -35.0, 120.0, 50.0)]
INSIDE_CAMERA = (60.0, 10.0, 12.0, 1.0)


def label_options(refine_steps=4, shade=1, ambient=0.1, diffuse=0.8, specular=0.3, shininess=32):
    return abi.LabelRenderOptions(refine_steps=refine_steps, shade=shade, ambient=ambient, diffuse=diffuse, specular=specular, shininess=shininess,
                                  flags=0)


@functools.lru_cache(maxsize=None)
def scene(shape=SHAPE, seed=SEED, box=None):
    """(vol [D, H, W] uint8, labels uint32 of the box's shape, K): the synthetic shells labelled at iso 0.5 under connectivity 6; computed
    once per (shape, seed, box) and shared (read-only)"""
    vol = O.synth_volume(shape, 1, seed)
    lab, _, counts = components_np(vol, ISO, 6, box=box)
    lab = np.ascontiguousarray(lab, np.uint32)
    vol.setflags(write=False)
    lab.setflags(write=False)
    return vol, lab, int(counts[0])


def tables(k):
    """the colour tables of the tests for labels 1 .. k: every label visible, the odd ones hidden, the even ones hidden, and a table that
    names only the first half of the labels"""
    every = LB.color_table(k, seed=3)
    return dict(all=every, odd_hidden=LB.color_table(k, seed=3, hidden=range(1, k + 1, 2)), even_hidden=LB.color_table(k, seed=3, hidden=range(2, k + 1, 2)),
                short=every[:k // 2].copy())


# ---- numpy restatement ------------------------------------------------------------------------------------------------------------------

def voxel_np(q, extent):
    """the voxel of a texture-space coordinate on one axis: c = fma(q, extent, -0.5), clamp((int) floor(c + 0.5), 0, extent - 1)"""
    c = _fma(q, F(extent), F(-0.5))
    with np.errstate(all="ignore"):
        v = np.floor(c + F(0.5))
    return np.clip(np.nan_to_num(v, nan=0.0).clip(-2 ** 30, 2 ** 30).astype(np.int64), 0, extent - 1)


def label_np(labels, box, shape_dhw, qx, qy, qz):
    """label(q): the label of the voxel of q, 0 where that voxel lies outside the box (x0, y0, z0, w, h, d; None: the whole volume)"""
    D, H, W = shape_dhw
    x0, y0, z0, bw, bh, bd = (0, 0, 0, W, H, D) if box is None else box
    assert labels.shape == (bd, bh, bw)
    x, y, z = voxel_np(qx, W) - x0, voxel_np(qy, H) - y0, voxel_np(qz, D) - z0
    inside = (x >= 0) & (x < bw) & (y >= 0) & (y < bh) & (z >= 0) & (z < bd)
    return np.where(inside, labels[np.clip(z, 0, bd - 1), np.clip(y, 0, bh - 1), np.clip(x, 0, bw - 1)], 0).astype(np.int64)


def color_np(colors, L):
    """the colour word of label L: 0 (not visible) for label 0 and for a label the table does not name"""
    colors = np.asarray(colors, np.uint32)
    named = (L >= 1) & (L <= colors.size)
    if colors.size == 0:
        return np.zeros(np.shape(L), np.uint32)
    return np.where(named, colors[np.clip(L - 1, 0, colors.size - 1)], np.uint32(0)).astype(np.uint32)


def visible_np(colors, L):
    return (color_np(colors, L) >> np.uint32(24)) != 0


def label_samples_np(shape_dhw, R, labels, box, colors):
    """every sample of every ray of rays_np's R, in the layout of samples_np: L (the label), v (1.0 where it is visible, else 0.0; 0 past a
    ray's n_steps) and cx, cy, cz (the samplers' voxel coordinates)"""
    D, H, W = shape_dhw
    n, e, s = R["n_steps"], R["e"], R["s"]
    m = int(n.max()) if n.size else 0
    live = np.arange(m)[None, :] < n[:, None]
    fi = np.arange(m, dtype=F)[None, :]
    with np.errstate(all="ignore"):
        pos = [np.where(live, _fma(fi, s[a][:, None], e[a][:, None]), F(0.5)) for a in range(3)]
        L = np.where(live, label_np(labels, box, shape_dhw, *pos), 0)
        cx, cy, cz = _fma(pos[0], F(W), F(-0.5)), _fma(pos[1], F(H), F(-0.5)), _fma(pos[2], F(D), F(-0.5))
    return dict(L=L, v=np.where(live & visible_np(colors, L), F(1), F(0)), cx=cx, cy=cy, cz=cz, live=live)


def visibility_map_np(labels, box, shape_dhw, colors, map_extent):
    """vkv_label_visibility_map: max_map_np of the volume-shaped indicator "this voxel lies in the box and carries a visible label" * 255"""
    D, H, W = shape_dhw
    x0, y0, z0, bw, bh, bd = (0, 0, 0, W, H, D) if box is None else box
    indicator = np.zeros((D, H, W), np.uint8)
    indicator[z0:z0 + bd, y0:y0 + bh, x0:x0 + bw] = visible_np(colors, labels.astype(np.int64)) * np.uint8(255)
    return max_map_np(indicator, map_extent)


def labels_np(p, labels, box, colors, options, vol=None, in_depth=None, S=None):
    """vkv_render_labels of DESIGN.md §5.21 for the whole image of RenderParams p and LabelRenderOptions `options` (refine_steps, shade and
    the light; its pointers are not read) over the labels of `box` and the colour table; vol: the (D, H, W) uint8 volume, needed with
    shade == 1.  Dict of (h, w)-shaped arrays label, color (h, w, 4), rgba8 (h, w, 4), depth, normal (h, w, 4), k (-1: no hit), t, n_steps,
    found, and the per-ray sample matrix S (label_samples_np)."""
    assert isinstance(options, abi.LabelRenderOptions) and options.flags == 0 and options.shade in (0, 1)
    shape_dhw = (p.volume_extent.depth, p.volume_extent.height, p.volume_extent.width)
    D, H, W = shape_dhw
    R = rays_np(p, in_depth)
    w, h = p.image_width, p.image_height
    n, e, s = R["n_steps"], R["e"], R["s"]
    N = n.size
    if S is None:
        S = label_samples_np(shape_dhw, R, labels, box, colors)
    k = iso_walk_dense(S["v"], n, F(1))
    with np.errstate(all="ignore"):
        found = k >= 0
        lo, hi = (k - 1).astype(F), k.astype(F)
        for _ in range(int(options.refine_steps)):
            mid = (lo + hi) * F(0.5)
            up = visible_np(colors, label_np(labels, box, shape_dhw, _fma(mid, s[0], e[0]), _fma(mid, s[1], e[1]), _fma(mid, s[2], e[2])))
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        t = np.where(k > 0, hi, F(0)).astype(F)
        P = [_fma(t, s[a], e[a]) for a in range(3)]
        L = np.where(found, label_np(labels, box, shape_dhw, *P), 0)
        word = color_np(colors, L)
        base = [((word >> np.uint32(8 * c)) & np.uint32(255)).astype(F) * INV255 for c in range(3)]
        cam = p.camera
        c4 = _mat4_mul(cam.camera_proj, _mat4_mul(cam.camera_view, _mat4_mul(cam.model, [P[0] - F(0.5), P[1] - F(0.5), P[2] - F(0.5), np.ones(N, F)])))
        depth = np.where(found, c4[2] / c4[3], R["no_colour_depth"]).astype(F)
        zero = np.zeros(N, F)
        nn, rgb = [zero, zero, zero], base
        if options.shade:
            # iso_np's shading: the tetrahedron gradient of the volume at p, the normal through model_inv's transpose, the headlight
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
            light = (F(options.ambient) + F(options.diffuse) * d) + F(options.specular) * power_bits(d, int(options.shininess))
            rgb = [_clamp01(base[c] * light) for c in range(3)]
    one = np.where(found, F(1), zero)
    color = np.stack([np.where(found, rgb[0], zero), np.where(found, rgb[1], zero), np.where(found, rgb[2], zero), one], -1).astype(F)
    rgba8 = np.rint(np.clip(color, 0, 1) * F(255)).astype(np.uint8)
    lit = found & bool(options.shade)
    normal = np.stack([np.where(lit, nn[0], zero), np.where(lit, nn[1], zero), np.where(lit, nn[2], zero), np.where(lit, F(1), zero)], -1).astype(F)
    return dict(label=L.astype(np.uint32).reshape(h, w), color=color.reshape(h, w, 4), rgba8=rgba8.reshape(h, w, 4), depth=depth.reshape(h, w),
                normal=normal.reshape(h, w, 4), k=k.reshape(h, w), t=t.reshape(h, w), n_steps=n.reshape(h, w), found=found.reshape(h, w), S=S, R=R)


def camera_params(shape, cam, size=SIZE, sampling_factor=1.0, block=4, map_extent=None):
    az, el, radius, clip = cam
    return params_np(shape, image_size=size, azimuth=az, elevation=el, radius=radius, sampling_factor=sampling_factor, block=block,
                     map_extent=map_extent, clip=clip)


# ---- tests ------------------------------------------------------------------------------------------------------------------------------

def test_label_render_options_mirror_matches_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkvolume_amd.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(VkvLabelRenderOptions));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(VkvLabelRenderOptions, %s));\n' % (f, f) for f, _ in abi.LabelRenderOptions._fields_) +
                   "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().split("\n") if line.strip())
    assert int(out.pop("sizeof")) == C.sizeof(abi.LabelRenderOptions)
    assert len(out) == 14
    for f, _ in abi.LabelRenderOptions._fields_:
        assert int(out[f]) == getattr(abi.LabelRenderOptions, f).offset, f
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bint\s+vkv_render_labels\s*\(", header) and re.search(r"\bint\s+vkv_label_visibility_map\s*\(", header)
    # the box is a host pointer that the structure keeps alive
    o = abi.LabelRenderOptions(box=C.pointer(abi.Box(1, 2, 3, 4, 5, 6)))
    assert (o.box.contents.x0, o.box.contents.depth) == (1, 6) and not abi.LabelRenderOptions().box


def test_every_table_byte_survives_the_float_colour():
    b = np.arange(256, dtype=F)
    base = b * INV255
    assert np.array_equal(np.rint(base * F(255)).astype(np.int64), np.arange(256))  # RGBA8 of an unshaded hit is the table's byte
    assert np.all((base >= 0) & (base <= 1))


def test_a_visible_cell_is_never_skipped_and_a_hidden_one_always():
    assert F(255) * INV255 == F(1.0)  # top < 1.0 fails for a byte of 255
    assert F(0) * INV255 < F(1.0)  # and holds for a byte of 0


def test_color_table_and_set_visible():
    t = LB.color_table(300, seed=1, hidden=(2, 300))
    assert t.dtype == np.uint32 and t.shape == (300,)
    alpha = t >> np.uint32(24)
    assert alpha[1] == 0 and alpha[299] == 0 and np.all(np.delete(alpha, [1, 299]) == 255)
    assert np.array_equal(t & np.uint32(0xffffff), LB.color_table(300, seed=1) & np.uint32(0xffffff))  # hiding keeps the colour
    assert np.array_equal(LB.color_table(300, seed=1), LB.color_table(300, seed=1)) and not np.array_equal(LB.color_table(300, seed=1), LB.color_table(300, seed=2))
    for shift in (0, 8, 16):
        assert np.all(((t >> np.uint32(shift)) & np.uint32(255)) >= 64)
    assert len(np.unique(LB.color_table(300) & np.uint32(0xffffff))) > 290
    LB.set_visible(t, [2], True)
    assert t[1] >> np.uint32(24) == 255 and t[299] >> np.uint32(24) == 0
    LB.set_visible(t, [1, 2, 3], False)
    assert np.all(t[:3] >> np.uint32(24) == 0) and np.array_equal(t[:3] & np.uint32(0xffffff), LB.color_table(300, seed=1)[:3] & np.uint32(0xffffff))
    assert LB.color_table(0).shape == (0,)
    with pytest.raises(ValueError):
        LB.set_visible(t, [0], True)
    with pytest.raises(ValueError):
        LB.set_visible(t, [301], True)


def test_the_scene_has_the_labels_the_tests_rest_on():
    assert scene()[2] == 192 and scene(box=BOX)[2] == 115
    assert scene(box=BOX)[1].shape == (20, 24, 30)


@pytest.mark.parametrize("box", [None, BOX])
def test_skip_walk_equals_dense_walk_and_the_scene_shows_many_bodies(box):
    vol, lab, k_labels = scene(box=box)
    shape_dhw = vol.shape
    tabs = tables(k_labels)
    for cam in CAMERAS:
        p = camera_params(SHAPE, cam)
        me = (p.map_extent.width, p.map_extent.height, p.map_extent.depth)
        for name in ("all", "odd_hidden"):
            colors = tabs[name]
            ref = labels_np(p, lab, box, colors, label_options(shade=0))
            S, R = ref["S"], ref["R"]
            k, n = ref["k"].reshape(-1), R["n_steps"]
            found = k >= 0
            hit_labels = ref["label"].reshape(-1)[found]
            assert np.all(visible_np(colors, hit_labels.astype(np.int64)))
            if name == "all":
                assert len(np.unique(hit_labels)) >= 20, (cam, box)
            else:
                # a pixel whose hit lies behind a sample that carries a hidden label: hiding a body shows what is behind it
                before = np.arange(S["L"].shape[1])[None, :] < k[:, None]
                behind = found & ((S["L"] != 0) & ~visible_np(colors, S["L"]) & before).any(axis=1)
                assert behind.sum() >= 10, (cam, box)
                assert np.all(hit_labels % 2 == 0)
            # the skip walk over the visibility map, from numpy alone
            vis = visibility_map_np(lab, box, shape_dhw, colors, me)
            assert set(np.unique(vis)) <= {0, 255}
            walk = max_map_skip_np(p, vol, vis, 1.0, True, R, S)
            assert np.array_equal(walk["k"], k), (cam, box, name)
            assert np.array_equal(walk["n_filt"] + walk["n_skip"], np.where(found, k + 1, n))
            assert walk["n_skip"].sum() > 0 and walk["n_probe"].sum() > 0
            # no skipped sample was visible
            assert not (walk["skipped"] & (S["v"] > 0)).any()


def test_the_inside_camera_hits_at_the_first_sample():
    vol, lab, k_labels = scene()
    p = camera_params(SHAPE, INSIDE_CAMERA)
    ref = labels_np(p, lab, None, tables(k_labels)["all"], label_options(refine_steps=4, shade=1), vol=vol)
    # the camera sits inside a body: every pixel hits within the first samples, and enough of them at the first one to cover the t = 0 path
    # (with nearest-voxel labels 744 of the 1920 pixels hit at k = 0 and the rest at k = 1 .. 6: the first samples of those rays fall
    # into voxels that carry label 0)
    assert ref["found"].all() and ref["found"].size == 1920
    first = ref["k"] == 0
    print("inside camera: k == 0 at %d pixels, largest k %d" % (first.sum(), ref["k"].max()))
    assert first.sum() >= 100 and ref["k"].max() <= 8
    assert np.all(ref["t"][first] == 0) and np.all(ref["t"][~first] > 0)
    assert np.all(ref["normal"][..., 3] == 1) and np.all(ref["rgba8"][..., 3] == 255)


def test_unshaded_rgba8_is_the_table_and_refinement_stays_between_the_samples():
    vol, lab, k_labels = scene()
    colors = tables(k_labels)["all"]
    p = camera_params(SHAPE, CAMERAS[0])
    for steps in (0, 4, 16):
        ref = labels_np(p, lab, None, colors, label_options(refine_steps=steps, shade=0))
        f = ref["found"]
        word = colors[ref["label"][f].astype(np.int64) - 1]
        for c in range(3):
            assert np.array_equal(ref["rgba8"][f][:, c], ((word >> np.uint32(8 * c)) & np.uint32(255)).astype(np.uint8))
        assert np.all(ref["rgba8"][f][:, 3] == 255) and np.all(ref["rgba8"][~f] == 0) and np.all(ref["label"][~f] == 0)
        assert np.all(ref["normal"] == 0)
        k, t = ref["k"][f], ref["t"][f]
        assert np.all(t <= k) and np.all(t >= np.maximum(k - 1, 0))
        if steps == 0:
            assert np.array_equal(t, k.astype(F))
    # a table shorter than the label count hides the labels it does not name
    short = tables(k_labels)["short"]
    ref = labels_np(p, lab, None, short, label_options(shade=0))
    assert ref["found"].any() and ref["label"][ref["found"]].max() <= short.size
    # nothing named, nothing shown
    assert not labels_np(p, lab, None, np.zeros(0, np.uint32), label_options(shade=0))["found"].any()


def test_label_kernels_use_no_scratch(tmp_path):
    kernels = {k: v["ScratchSize"] for k, v in T.kernel_listing("labels_render.hip", tmp_path / "labels_render.s").items()}
    render = {k: v for k, v in kernels.items() if "k_labels" in k}
    assert len(render) == 6, kernels
    assert any("k_label_visibility_map" in k for k in kernels), kernels
    assert all(v == 0 for v in kernels.values()), kernels

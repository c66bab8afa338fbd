"""CPU: the cell-summary entry points (vkv_cell_summary, vkv_occupancy_map_from_summary, vkv_update_transfer_function_from_summary) are
declared, exported and bound and refuse null, misaligned and out-of-range arguments before anything touches the HIP runtime; and a numpy
restatement of the summary format and the decision rule (DESIGN.md §5 "Cell summaries") against brute-force occupancy on random volumes and
arbitrary random bit tables: every cell the rule decides gets the brute-force answer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from vkvolume_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vkv_cell_summary", "vkv_occupancy_map_from_summary", "vkv_update_transfer_function_from_summary")
EMPTY, OCCUPIED, UNRESOLVED = 0, 1, 2


# ---- the numpy restatement (the GPU tests compare the device against it) ----------------------------------------------------------------

def blocks(extent_whd, map_whd):
    return tuple((e + m - 1) // m for e, m in zip(extent_whd, map_whd))


def cell_voxels(a, map_whd, block, fill):
    """(D, H, W) array -> (md, mh, mw, bz * by * bx) per-cell voxel lists, padded with `fill` past the volume"""
    (mw, mh, md), (bx, by, bz) = map_whd, block
    d, h, w = a.shape
    p = np.full((md * bz, mh * by, mw * bx), fill, dtype=np.int64)
    p[:min(d, md * bz), :min(h, mh * by), :min(w, mw * bx)] = a[:md * bz, :mh * by, :mw * bx]
    return p.reshape(md, bz, mh, by, mw, bx).transpose(0, 2, 4, 1, 3, 5).reshape(md, mh, mw, bz * by * bx)


def summary_np(vol, grad, map_whd):
    """The 16-byte summaries of every cell, in map order: (cells, 16) uint8.  grad None: every gradient byte is 255."""
    d, h, w = vol.shape
    block = blocks((w, h, d), map_whd)
    i = cell_voxels(vol.astype(np.int64), map_whd, block, -1)
    g = cell_voxels(np.full(vol.shape, 255, np.int64) if grad is None else grad.astype(np.int64), map_whd, block, -1)
    valid = i >= 0
    has = valid.any(axis=-1)
    big = 1 << 20
    i_lo = np.where(valid, i, big).min(-1)
    g_lo = np.where(valid, g, big).min(-1)
    ig = np.where(valid, i * 256 + g, -1).max(-1)
    gi = np.where(valid, g * 256 + i, -1).max(-1)
    bit = np.where(valid, np.left_shift(np.uint64(1), ((g >> 5) * 8 + (i >> 5)).clip(0, 63).astype(np.uint64)), np.uint64(0))
    mask = np.bitwise_or.reduce(bit, axis=-1)
    out = np.zeros(has.shape + (16,), np.uint8)
    fields = [i_lo, ig >> 8, g_lo, gi >> 8, ig & 255, gi & 255, np.ones_like(i_lo)]
    for k, f in enumerate(fields):
        out[..., k] = np.where(has, f, 0)
    out[..., 8:] = np.where(has[..., None], mask[..., None].view(np.uint8).reshape(has.shape + (8,)), 0)
    return out.reshape(-1, 16)


def occupancy_np(vol, grad, bits, use_gradient, map_whd):
    """Brute force, as vkv_occupancy_map: a cell is OCCUPIED (0) if some voxel's bit B(g, i) is set (g = 255 without use_gradient), else
    EMPTY (255); (md, mh, mw) uint8.  bits: (256, 256) bool, row = gradient byte."""
    d, h, w = vol.shape
    block = blocks((w, h, d), map_whd)
    gg = grad if (use_gradient and grad is not None) else np.full(vol.shape, 255, np.uint8)
    hit = bits[gg.astype(np.int64), vol.astype(np.int64)]
    occ = cell_voxels(hit.astype(np.int64), map_whd, block, 0).any(-1)
    return np.where(occ, 0, 255).astype(np.uint8)


def classify_np(summ, bits, use_gradient):
    """The decision rule on (cells, 16) summaries: EMPTY / OCCUPIED / UNRESOLVED per cell.  The rectangle tests count set bits with a 2-D prefix
    sum (an independent restatement of the device's row-range OR / AND table)."""
    s = summ.astype(np.int64)
    has = (s[:, 6] & 1) != 0
    ilo, ihi, glo, ghi, gai, iag = (s[:, k] for k in range(6))
    mask = summ[:, 8:].copy().view(np.uint64).reshape(-1)
    if not use_gradient:
        glo = ghi = gai = np.full_like(ilo, 255)
        iag = ihi
        folded = np.zeros_like(mask)
        for gb in range(8):
            folded |= (mask >> np.uint64(8 * gb)) & np.uint64(255)
        mask = folded << np.uint64(56)
    b = bits.astype(np.int64)
    point = (b[gai, ihi] | b[ghi, iag]) != 0
    pre = np.zeros((257, 257), np.int64)
    pre[1:, 1:] = b.cumsum(0).cumsum(1)
    anyset = np.zeros(len(s), bool)
    full = np.zeros(len(s), bool)
    for k in range(64):
        sel = ((mask >> np.uint64(k)) & np.uint64(1)).astype(bool) & has
        if not sel.any():
            continue
        gb, ib = k >> 3, k & 7
        r0, r1 = np.maximum(32 * gb, glo), np.minimum(32 * gb + 31, ghi)
        c0, c1 = np.maximum(32 * ib, ilo), np.minimum(32 * ib + 31, ihi)
        r0s, r1s, c0s, c1s = (np.where(sel, x, 0) for x in (r0, r1, c0, c1))
        assert (r0s <= r1s).all() and (c0s <= c1s).all()
        cnt = pre[r1s + 1, c1s + 1] - pre[r0s, c1s + 1] - pre[r1s + 1, c0s] + pre[r0s, c0s]
        area = (r1s - r0s + 1) * (c1s - c0s + 1)
        anyset |= sel & (cnt > 0)
        full |= sel & (cnt == area)
    return np.where(~has, EMPTY, np.where(point, OCCUPIED, np.where(~anyset, EMPTY, np.where(full, OCCUPIED, UNRESOLVED))))


def random_bits(rng, kind):
    """arbitrary bit tables (row = gradient byte): uniform noise of several densities, random rectangles, separable threshold products"""
    if kind == "noise":
        return rng.random((256, 256)) < rng.choice([0.001, 0.02, 0.3, 0.9, 0.999])
    if kind == "rects":
        t = np.zeros((256, 256), bool)
        for _ in range(rng.integers(1, 6)):
            g0, i0 = rng.integers(0, 256, 2)
            t[g0:g0 + rng.integers(1, 120), i0:i0 + rng.integers(1, 120)] = True
        return t
    gi, ii = rng.integers(0, 256, 2)
    return (np.arange(256)[:, None] >= gi) & (np.arange(256)[None, :] >= ii)


def bits_words(bits):
    """(256, 256) bool -> the device's 2048-word bit table: bits[g * 8 + (i >> 5)] holds bit i & 31"""
    return np.packbits(bits.reshape(256, 8, 32)[:, :, ::-1], axis=-1).reshape(256, 8, 4)[:, :, ::-1].copy().view(np.uint32).reshape(-1)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"#define\s+VKV_CELL_SUMMARY_BYTES\s+16\b", header) and abi.CELL_SUMMARY_BYTES == 16
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert name in lib.EXPORTS
        assert re.search(r"\b%s$" % name, out, flags=re.M)
    at = L.vkv_cell_summary.argtypes
    assert len(at) == 8 and at[3] is abi.Extent3D and at[4] is abi.Extent3D and at[5] is C.POINTER(abi.Box)
    at = L.vkv_occupancy_map_from_summary.argtypes
    assert len(at) == 11 and at[5] is C.POINTER(abi.TransferFunctionUniform) and at[6] is abi.Extent3D and at[8] is abi.Extent3D
    at = L.vkv_update_transfer_function_from_summary.argtypes
    assert len(at) == 16 and at[1] is C.POINTER(abi.VolumeOptions) and at[10] is C.c_int32
    assert "grown by one voxel" in header.split("int vkv_cell_summary(")[0].split("#define VKV_CELL_SUMMARY_BYTES")[1]


def test_bad_arguments_are_rejected_without_a_device():
    """a null context returns before the HIP runtime is touched; every other refusal is tested on the GPU, where it must write nothing"""
    L = lib.load()
    e, me = abi.Extent3D(8, 8, 8), abi.Extent3D(2, 2, 2)
    box = abi.Box(0, 0, 0, 1, 1, 1)
    tf = abi.TransferFunctionUniform()
    opts = abi.VolumeOptions()
    inv = abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_cell_summary(None, None, None, e, me, None, None, None) == inv
    assert L.vkv_cell_summary(None, None, None, e, me, C.byref(box), None, None) == inv
    assert L.vkv_occupancy_map_from_summary(None, None, None, None, None, C.byref(tf), e, None, me, None, None) == inv
    assert L.vkv_occupancy_map_from_summary(None, None, None, None, None, None, e, None, me, None, None) == inv
    assert L.vkv_update_transfer_function_from_summary(None, C.byref(opts), None, None, e, None, None, None, None, me, 0, None, None, None, None,
                                                       None) == inv
    assert L.vkv_update_transfer_function_from_summary(None, None, None, None, e, None, None, None, None, me, 9, None, None, None, None, None) == inv


# ---- the format and the rule ---------------------------------------------------------------------------------------------------------------

def test_summary_fields_on_a_hand_made_cell():
    vol = np.array([[[10, 200], [200, 40]]], np.uint8)  # one 2 x 2 x 1 cell
    grad = np.array([[[100, 7], [90, 250]]], np.uint8)
    s = summary_np(vol, grad, (1, 1, 1))[0]
    assert list(s[:8]) == [10, 200, 7, 250, 90, 40, 1, 0]
    mask = int(s[8:].view(np.uint64)[0])
    want = sum(1 << ((g >> 5) * 8 + (i >> 5)) for i, g in ((10, 100), (200, 7), (200, 90), (40, 250)))
    assert mask == want
    s = summary_np(vol, None, (1, 1, 1))[0]
    assert list(s[:8]) == [10, 200, 255, 255, 255, 200, 1, 0]
    # a map extent past the volume: the cells without voxels are all zero
    s = summary_np(np.ones((5, 5, 5), np.uint8), None, (4, 4, 4))
    assert s.shape == (64, 16) and (s.reshape(4, 4, 4, 16)[3] == 0).all() and (s.reshape(4, 4, 4, 16)[:2, :2, :2, 6] == 1).all()


def test_bits_words_layout():
    bits = np.zeros((256, 256), bool)
    bits[3, 37] = bits[255, 0] = True
    w = bits_words(bits)
    assert w[3 * 8 + 1] == 1 << 5 and w[255 * 8] == 1 and int(np.count_nonzero(w)) == 2


@pytest.mark.parametrize("seed", range(12))
def test_rule_resolves_only_what_brute_force_confirms(seed):
    rng = np.random.default_rng(seed)
    w, h, d = (int(x) for x in rng.integers(5, 30, 3))
    smooth = rng.random() < 0.5
    vol = rng.integers(0, 256, (d, h, w)).astype(np.uint8)
    if smooth:  # narrow per-cell ranges, as on real volumes
        vol = (np.add.outer(np.add.outer(np.arange(d) * 3, np.arange(h) * 5), np.arange(w) * 2) % 256 + rng.integers(0, 4, (d, h, w))).astype(np.uint8)
    grad = rng.integers(0, 256, (d, h, w)).astype(np.uint8) if rng.random() < 0.5 else (vol // 2 + 60).astype(np.uint8)
    b = int(rng.integers(1, 7))
    map_whd = ((w + b - 1) // b + int(rng.integers(0, 2)), (h + b - 1) // b, (d + b - 1) // b)
    map_whd = tuple(min(m, e) for m, e in zip(map_whd, (w, h, d)))
    for has_grad in (True, False):
        summ = summary_np(vol, grad if has_grad else None, map_whd)
        for kind in ("noise", "rects", "threshold", "noise", "rects"):
            bits = random_bits(rng, kind)
            for use_gradient in ((1, 0) if has_grad else (0,)):
                want = occupancy_np(vol, grad if has_grad else None, bits, use_gradient, map_whd).reshape(-1)
                got = classify_np(summ, bits, use_gradient)
                assert ((got == OCCUPIED) <= (want == 0)).all() and ((got == EMPTY) <= (want == 255)).all(), (kind, use_gradient)


def test_rule_decides_the_easy_tables_completely():
    rng = np.random.default_rng(99)
    vol = rng.integers(0, 256, (12, 13, 14)).astype(np.uint8)
    grad = rng.integers(0, 256, (12, 13, 14)).astype(np.uint8)
    summ = summary_np(vol, grad, (4, 4, 4))
    for bits, want in ((np.zeros((256, 256), bool), EMPTY), (np.ones((256, 256), bool), OCCUPIED)):
        for use_gradient in (0, 1):
            assert (classify_np(summ, bits, use_gradient) == want).all()

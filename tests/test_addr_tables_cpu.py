"""The prebuilt per-voxel-index address tables (vkvolume_amd/csrc/addr_tables.hpp, appended to the two-level tables by packed_addr_lut) hold,
word for word, what a workgroup used to derive from the two-level tables in stage_full_lut: the kernels now copy them instead.  The
formulas are re-stated here in numpy on the two-level words the builder itself wrote; the packed layout is re-stated independently for
the two-level words.  CPU only: the builder is a host-only header, compiled here with g++ into a few-line driver."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENTS = [(1024, 1024, 795), (1024, 1024, 1024), (512, 512, 512), (493, 493, 443), (33, 17, 9), (4, 4, 4)]
K_LUT_XM = 96  # raymarch_core.hpp: word offset of the x macro-brick terms


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("addr_tables") / "addr_tables_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "addr_tables_driver.cpp"), "-o", exe])
    return exe


def _tables(driver, extent):
    out = subprocess.check_output([driver] + [str(v) for v in extent], text=True).split("\n")
    lut_y, lut_z, words, full, full_words = (int(v) for v in out[0].split())
    table = np.array([int(v) for v in out[1:] if v], dtype=np.uint64)
    assert table.max() < 2 ** 32
    return lut_y, lut_z, words, full, full_words, table


def _two_level_reference(W, H, D):
    """the packed layout (vkv_device.hpp): brick = 4 padded voxels per axis, 5^3 (value, gradient) byte pairs, 256 bytes; 8x8x8 bricks per
    128 KiB macro-brick; macro-bricks x fastest"""
    mx, my = ((((W + 1) >> 2) + 1) + 7) >> 3, ((((H + 1) >> 2) + 1) + 7) >> 3
    j = np.arange(32, dtype=np.uint64)
    in_x = ((j >> 2) & 7) * 256 + (j & 3) * 2
    in_y = ((j >> 2) & 7) * 8 * 256 + (j & 3) * 5 * 2
    in_z = ((j >> 2) & 7) * 64 * 256 + (j & 3) * 25 * 2
    nm = [(e + 1) // 32 + 1 for e in (W, H, D)]
    mac_x = np.arange(nm[0], dtype=np.uint64) * (512 * 256)
    mac_y = np.arange(nm[1], dtype=np.uint64) * np.uint64(mx) * (512 * 256)
    mac_z = np.arange(nm[2], dtype=np.uint64) * np.uint64(mx * my) * (512 * 256)
    return in_x, in_y, in_z, mac_x, mac_y, mac_z


@pytest.mark.parametrize("extent", EXTENTS, ids=["%dx%dx%d" % e for e in EXTENTS])
def test_prebuilt_full_tables_equal_what_stage_full_lut_derived(driver, extent):
    W, H, D = extent
    lut_y, lut_z, words, full, full_words, g = _tables(driver, extent)
    nx, ny, nz = W + 2, H + 2, D + 2
    assert full % 4 == 0 and full >= words and full_words % 4 == 0 and 0 <= full_words - (nx + ny + nz) < 4
    assert g.size == full + full_words and lut_z % 2 == 0
    assert not g[words:full].any(), "the gap in front of the 16-byte aligned full tables is zero"

    # the two-level words against the packed layout
    in_x, in_y, in_z, mac_x, mac_y, mac_z = _two_level_reference(W, H, D)
    assert np.array_equal(g[0:32], in_x) and np.array_equal(g[32:64], in_y) and np.array_equal(g[64:96], in_z)
    assert np.array_equal(g[K_LUT_XM:K_LUT_XM + mac_x.size], mac_x) and np.array_equal(g[lut_y:lut_y + mac_y.size], mac_y)
    z64 = g[lut_z:lut_z + 2 * mac_z.size:2] | (g[lut_z + 1:lut_z + 2 * mac_z.size:2] << np.uint64(32))
    assert np.array_equal(z64, mac_z)

    # stage_full_lut's formulas on the two-level words (32-bit sums for x and y, a 64-bit sum for z, then >> 1, truncated to 32 bits)
    m32 = np.uint64(0xFFFFFFFF)
    b = np.arange(nx, dtype=np.uint64)
    want_x = ((g[b & 31] + g[K_LUT_XM + (b >> 5)]) & m32) >> 1
    b = np.arange(ny, dtype=np.uint64)
    want_y = ((g[32 + (b & 31)] + g[lut_y + (b >> 5)]) & m32) >> 1
    b = np.arange(nz, dtype=np.uint64)
    zm = (g[lut_z + 2 * (b >> 5) + 1] << np.uint64(32)) | g[lut_z + 2 * (b >> 5)]
    want_z = ((zm + g[64 + (b & 31)]) >> 1) & m32
    got = g[full:]
    assert np.array_equal(got[:nx], want_x)
    assert np.array_equal(got[nx:nx + ny], want_y)
    assert np.array_equal(got[nx + ny:nx + ny + nz], want_z)
    assert not got[nx + ny + nz:].any(), "the padded tail is zero"

    # and they address what the two-level sum addresses: twice the entry is the byte offset (every term is even, the image at most 8 GiB)
    assert np.array_equal(want_z * 2, mac_z[np.arange(nz) >> 5] + in_z[np.arange(nz) & 31])

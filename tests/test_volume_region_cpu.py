"""CPU: the region update of the volume (vkv_update_volume_region) is declared, exported and bound, abi.Box has VkvBox's layout, and a null
context is refused before anything touches the HIP runtime."""
import ctypes as C
import os
import re
import subprocess

from vkvolume_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vkv_update_volume_region"

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "vkvolume_amd.h"
int main(void)
{
	printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(VkvBox), offsetof(VkvBox, x0), offsetof(VkvBox, y0), offsetof(VkvBox, z0),
	       offsetof(VkvBox, width), offsetof(VkvBox, height), offsetof(VkvBox, depth));
	return 0;
}
"""


def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in lib.EXPORTS
    L = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\b%s$" % NAME, out, flags=re.M)
    at = getattr(L, NAME).argtypes
    assert at is not None and len(at) == 18
    assert at[2] is C.c_int32 and at[3] is C.c_int32 and at[4] is C.c_float and at[5] is C.c_float
    assert at[6] is C.POINTER(abi.Box)
    assert at[10] is abi.Extent3D and at[15] is abi.Extent3D and at[16] is C.c_int32


def test_box_layout_matches_the_header(tmp_path):
    src = tmp_path / "box_probe.c"
    src.write_text(PROBE)
    exe = tmp_path / "box_probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.Box)] + [getattr(abi.Box, f).offset for f in ("x0", "y0", "z0", "width", "height", "depth")]
    assert got == want == [24, 0, 4, 8, 12, 16, 20]
    b = abi.Box(1, 2, 3, 4, 5, 6)
    assert (b.x0, b.y0, b.z0, b.width, b.height, b.depth) == (1, 2, 3, 4, 5, 6)


def test_null_context_is_refused_without_a_device():
    L = lib.load()
    box = abi.Box(0, 0, 0, 1, 1, 1)
    tf = abi.TransferFunctionUniform()
    assert L.vkv_update_volume_region(None, None, 0, 0, 0.0, 255.0, C.byref(box), None, None, None, abi.Extent3D(4, 4, 4), None, C.byref(tf), None,
                                      None, abi.Extent3D(1, 1, 1), abi.SKIP_DISTANCE, None) == abi.VKV_E_INVALID_ARGUMENT

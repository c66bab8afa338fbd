"""The library's pure host arithmetic (vkvolume_amd/host/host_arith.cpp: start orders and the tile mix, the screen bound of the clipped box
and its tile rectangle, the tuning block's defaults, environment and range checks, the opacity table, tile rectangles, and host_arith.hpp's
iso_threshold, the inside rule of the meshes, the components and the distance transform) as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer: tests/host_arith_driver.cpp, built from the product's own plain C++ sources
with g++ - no HIP, nothing loaded into Python - and run as a child process.  The driver works its expected values out from the
definitions.  CPU only; a few seconds."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_mesh_cpu import KINV255

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vkvolume_amd", "host")
BUILD = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-O1", "-g", "-Wall"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """runs the driver, built once, with `args` and `stdin`; returns its output"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("host_arith") / "host_arith_driver")
    sources = [os.path.join(ROOT, "tests", "host_arith_driver.cpp"), os.path.join(HOST, "host_arith.cpp"), os.path.join(HOST, "load_volume.cpp")]
    subprocess.check_call(BUILD + sources + ["-o", exe])
    # the driver sets the tuning variables itself: none of the caller's may leak into its "nothing set" case
    env = {k: v for k, v in os.environ.items() if not k.startswith("VKV_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(args=(), stdin=""):
        r = subprocess.run([exe] + list(args), env=env, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-4000:]
        return r.stdout

    return run


def test_host_arithmetic_under_asan_and_ubsan(driver):
    out = driver()
    assert "host arith driver: ok" in out, out[-4000:]


def test_iso_threshold_counts_the_bytes_below_iso(driver):
    """iso_threshold(iso) = the smallest byte b with (float) b * kInv255 >= iso, 256 without one: as b * kInv255 is monotone in b, the number
    of bytes with b * kInv255 < iso in float32.  At every k / 255 and its float neighbours (where the threshold steps), below, at and above
    the ends of the range, at -0.0, and at the smallest denormal and normal (above 0 * kInv255 by the least that a float can be)."""
    F = np.float32
    at = np.arange(256, dtype=F) / F(255)
    isos = np.concatenate([np.nextafter(at, F(-np.inf)), at, np.nextafter(at, F(np.inf)),
                           np.array([-1.0, 0.0, -0.0, 1.0, np.nextafter(F(1), F(2)), 2.0], dtype=F),
                           np.array([1, 0x00800000], dtype=np.uint32).view(F)])
    assert isos.dtype == F and isos.size == 3 * 256 + 8
    bits = isos.view(np.uint32)
    assert bits[3 * 256 + 2] == 0x80000000 and isos[-2] == F(1.401298464324817e-45) and isos[-1] == np.finfo(F).tiny
    out = driver(["iso_threshold"], "".join("%08x\n" % b for b in bits)).split()
    assert out[0] == "kInv255" and int(out[1], 16) == int(np.array(KINV255, dtype=F).view(np.uint32)), out[:2]
    got = np.array([int(t) for t in out[2:]])
    values = np.arange(256, dtype=F) * F(KINV255)
    assert values.dtype == F
    want = np.array([np.count_nonzero(values < iso) for iso in isos])
    assert got.size == want.size and np.array_equal(got, want), [(float(i), g, w) for i, g, w in zip(isos, got, want) if g != w][:10]
    assert want.min() == 0 and want.max() == 256 and len(set(want.tolist())) == 257        # every threshold occurs


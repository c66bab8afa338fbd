"""The host-side decisions of the ray-march launchers as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/raymarch_policy_driver.cpp, built with g++ from the product's own plain C++ (vkvolume_amd/host/host_arith.cpp: frame_view and
feedback_step, when a registered target is measured again and when its measured start order is used; vkvolume_amd/csrc/raymarch_plan.hpp:
plan_batch, the grid, the shared kernel and the pull decision of a vkv_render_batch launch, and the fill_outside predicate) - no HIP, nothing
loaded into Python - and run as a child process.  No GPU test can see these decisions: any start order and any of the kernels renders the
same frame.  The driver writes its expected values out from the rules.  CPU only; a few seconds."""
import os
import shutil
import subprocess

import pytest

from tests.test_host_arith_cpu import BUILD, HOST, ROOT


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("raymarch_policy") / "raymarch_policy_driver")
    sources = [os.path.join(ROOT, "tests", "raymarch_policy_driver.cpp"), os.path.join(HOST, "host_arith.cpp"), os.path.join(HOST, "load_volume.cpp")]
    subprocess.check_call(BUILD + sources + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return r.returncode, r.stdout


def test_feedback_policy_and_batch_plan_under_asan_and_ubsan(driver_output):
    code, out = driver_output
    assert code == 0 and "raymarch policy driver: ok" in out, out[-4000:]

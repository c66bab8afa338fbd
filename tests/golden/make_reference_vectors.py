"""Generates tests/golden/reference_v1.npz: outputs of the REFERENCE'S OWN shader text, compiled for the CPU (oracle/_ref/libvkv_ref.so, built by
`make -C oracle ref` where a checkout of the reference is present; pinned arithmetic mode), for a handful of cases.
Unlike hotpath_v1.npz these are not self-generated: no line of oracle/vkv_oracle.c produced them.  tests/test_gpu_reference_vectors.py holds the
HIP kernels to them on the device, where neither the reference nor the library exists; tests/test_reference_text_cpu.py checks that a fresh run
still gives the committed file.

Inputs are regenerated from their seeds, not stored; the file keeps a SHA-256 of each so that a changed generator shows as such.

    python tests/golden/make_reference_vectors.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import vkv_oracle as O  # noqa: E402
from tests import helpers as T  # noqa: E402
from vkvolume_amd import abi  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_v1.npz")

SHAPE = (36, 30, 26)  # W, H, D: no multiple of the block size
SEED = 0xC0FFEE02
BLOCK = 4
IMAGE = (48, 48)
SMALL_SHAPE, SMALL_SEED, SMALL_BLOCK = (13, 7, 5), 5, 3  # extents that are no multiple of the block: a map of 5 x 3 x 2 cells
OCC_SHAPE_DHW, OCC_SEED, OCC_P = (9, 10, 13), 3, 0.01  # a sparse occupancy map of its own for the two transforms
MODES = (abi.SKIP_NONE, abi.SKIP_BLOCK, abi.SKIP_DISTANCE, abi.SKIP_ANISOTROPIC_DISTANCE)


def azimuth(mode):
    return 33.0 + 40.0 * mode  # the views of tests/test_frag_literal_cpu.py


def volume():
    return O.synth_volume(SHAPE, 1, SEED)


def small_volume():
    return T.random_volume(SMALL_SHAPE, SMALL_SEED, 0.7)


def sparse_occupancy():
    rng = np.random.default_rng(OCC_SEED)
    return np.where(rng.random(OCC_SHAPE_DHW) < OCC_P, 0, 255).astype(np.uint8)


def scene_for(vol, block, on_the_fly=False):
    """the host side (transfer function uniform and texture, transforms) - not part of what the fixture pins"""
    opt = abi.VolumeOptions(use_precomputed_gradient=not on_the_fly, **T.APP_TF)
    return T.OracleScene(vol, opt, block, voxel_size=(0.0003, 0.0003, 0.0007), axis_angle=(1, 0, 0, 90))


def frame_params(scene, mode, ert, test=abi.TEST_NONE):
    view, proj = T.orbit(azimuth(mode), image_size=IMAGE)
    ro = abi.RenderOptions(skipping_type=mode, clip_distance=1.0, early_ray_termination=ert, test=test)
    return scene.params(view, proj, IMAGE, ro)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def input_hashes():
    scene = scene_for(volume(), BLOCK)
    return {"sha_volume": sha(volume()), "sha_small_volume": sha(small_volume()), "sha_sparse_occupancy": sha(sparse_occupancy()),
            "sha_tf_texture": sha(scene.tex), "sha_params_m2_e1": sha(np.frombuffer(bytes(frame_params(scene, 2, True)), np.uint8))}


def compute():
    """every array of the fixture, freshly from the reference text"""
    from oracle import vkv_ref as R
    out = {k: np.array(v) for k, v in input_hashes().items()}
    for name, vol, block in (("", volume(), BLOCK), ("small_", small_volume(), SMALL_BLOCK)):
        scene = scene_for(vol, block)
        grad = R.gradient_map(vol, scene.tf)
        out[name + "gradient"] = grad
        out[name + "occupancy_precomputed"] = R.occupancy_map(vol, grad, scene.tex, scene.tf, block)
        out[name + "occupancy_on_the_fly"] = R.occupancy_map(vol, None, scene.tex, scene.tf, block)
        out[name + "distance"] = R.distance_map(out[name + "occupancy_precomputed"])
        out[name + "distance_aniso"] = R.distance_map_anisotropic(out[name + "occupancy_precomputed"])
    occ = sparse_occupancy()
    out["sparse_distance"] = R.distance_map(occ)
    out["sparse_distance_aniso"] = R.distance_map_anisotropic(occ)
    vol = volume()
    scene = scene_for(vol, BLOCK)
    grad = out["gradient"]
    for mode in MODES:
        maps = None if mode == abi.SKIP_NONE else R.compute_distance_map(vol, grad, scene.tex, scene.tf, BLOCK, mode)
        for ert in (True, False):
            p = frame_params(scene, mode, ert)
            # the interpolant ray_entry comes from the ray generator that replaces the reference's rasteriser
            entry = scene.render(frame_params(scene, mode, ert, abi.TEST_RAY_ENTRY)).color
            r = R.frag(p, entry, vol, grad, scene.tex, maps)
            assert int(r.counts.max()) < 65536
            key = "m%d_e%d" % (mode, ert)
            out["counts_" + key], out["color_" + key], out["depth_" + key] = r.counts.astype(np.uint16), r.color, r.depth
    return out


def main():
    out = compute()
    np.savez_compressed(PATH, **out)
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()

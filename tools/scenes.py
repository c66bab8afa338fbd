"""What the tools/time_*.py scripts measure on, beside bench.build_scene's scenes: the salt-noise scene and the distance family's cases."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.benchmark_sweep import PRESETS, preset_seed  # noqa: E402
from vkvolume_amd import abi, volume as V  # noqa: E402

SALT = (4, 200, 0, 0.071)  # tools/ess_crossover.py SCATTERED[1]: shells, thickness / 256, noise word, imin

# the distance family (time_distance, time_distance_weighted, time_nearest)
TARGETS = (("inside", abi.DISTANCE_TO_INSIDE), ("outside", abi.DISTANCE_TO_OUTSIDE))
CASES = (("inside", 2), ("inside", 10), ("inside", 101), ("inside", None), ("outside", None))  # (target, limit)


def limit_name(limit):
    return "none" if limit is None else str(limit)


def scene_volume(ctx, scene):
    """(Volume, iso of the salt scene or None): "c3" is bench.py's volume, anything else the salt-noise scene (492x492x442, four thin shells
    under hash noise 0..20) with its transfer function's lower edge as the iso"""
    if scene == "c3":
        return bench.build_scene(ctx, "c3")[0], None
    preset = PRESETS[0]
    extent = preset[1]
    shells, tq, noise, imin = SALT
    s = V.Volume(ctx)
    s.options = abi.VolumeOptions(intensity_min=imin, intensity_max=preset[3], gradient_min=preset[4], gradient_max=preset[5])
    s.load_synthetic(extent, kind=1 | (shells << 8) | (tq << 16) | noise, seed=preset_seed(extent), distance_map_block_size=4)
    return s, imin

"""Host helpers of vkv_geodesic_propagate (include/vkvolume_amd.h): the scratch size and the step tables.  A step table is
seven move costs, entry m - 1 for the offsets of class m = |dx| + 2 |dy| + 4 |dz|: x, y, xy, z, xz, yz, xyz; 0 means that the class of move
does not exist.  No numpy, no device."""
import math

from . import abi, lib

NONE = abi.GEODESIC_NONE  # not reached; as a limit: unlimited
MAX_ROUNDS = abi.GEODESIC_MAX_ROUNDS
MAX_STEP = 65535  # the largest cost of a move
TILE_EDGE = 8  # a round relaxes tiles of 8 x 8 x 8 voxels: a path needs about one round per tile it crosses
CHAMFER_345 = (3, 3, 4, 3, 4, 4, 5)  # the 3-4-5 chamfer: distances in thirds of a voxel
STEPS_6 = (1, 1, 0, 1, 0, 0, 0)  # 6-connected step counts
STEPS_26 = (1, 1, 1, 1, 1, 1, 1)  # 26-connected step counts (the Chebyshev path length)


def scratch_bytes(extent, box=None):
    """vkv_geodesic_scratch_bytes: the scratch vkv_geodesic_propagate needs for `box` (None: the whole volume) of `extent`: 8 bytes per voxel
    + 32 + 8 per tile of 8 x 8 x 8 voxels; 0 for an extent or box the call rejects (a box of more than 2^32 - 1 voxels included)"""
    return lib.load().vkv_geodesic_scratch_bytes(extent, box)


def chamfer_steps(spacing=None):
    """``(steps, unit)``: a step table and the length of one cost unit.  Without ``spacing``: the 3-4-5 chamfer, ((3, 3, 4, 3, 4, 4, 5), 1 / 3)
    in voxels.  With the voxel size (sx, sy, sz): steps[m - 1] = floor(3 sqrt(the sum of s_a^2 over the axes in m) / min(s) + 1 / 2) and
    unit = min(s) / 3, so that cost * unit is a length in the caller's units; integer weights as Volume.spacing_weights() gives them serve as
    well.  Sizes that are not three finite positive numbers, and sizes that give a step above 65535, raise ValueError."""
    if spacing is None:
        return CHAMFER_345, 1.0 / 3.0
    try:
        sizes = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        sizes = ()
    if len(sizes) != 3 or not all(math.isfinite(s) and s > 0 for s in sizes):
        raise ValueError("geodesic.chamfer_steps: spacing must be three finite positive numbers")
    s_min = min(sizes)
    steps = tuple(int(math.floor(3.0 * math.sqrt(sum(sizes[a] ** 2 for a in range(3) if m >> a & 1)) / s_min + 0.5)) for m in range(1, 8))
    if max(steps) > MAX_STEP:
        raise ValueError("geodesic.chamfer_steps: spacing %r gives a step above %d" % (sizes, MAX_STEP))
    return steps, s_min / 3.0

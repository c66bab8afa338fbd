"""Cost of the 3x3x3 volume filters (vkv_filter_volume: binomial, median) on the bench's C3 volume, and what a median pass buys
empty-space skipping on a salt-noise scene.

1. C3 (1024x1024x795; bench.py's volume): both filters of the whole volume next to vkv_gradient_map of the same volume, which reads the
   same +-1 footprint.  GB/s counts the algorithmic bytes, 1 B read + 1 B written per voxel.
2. A box refilter (what keeps a filtered copy current after vkv_update_volume_region): a single voxel, 256^3 and 1024x1024x64, the box
   sizes of profiles/volume_region_times.txt, both filters.
3. Evidence only: the scattered-occupancy scene of tools/ess_crossover.py (492x492x442, four thin shells under hash noise 0..20, intensity-only
   transfer function with imin 0.071): share of occupied 4^3 map cells and the 1200x1200 frame time (early ray termination off) without
   skipping and with the Chebyshev distance map, before and after one median pass.
ms from device events (blocks of --calls calls; the kinds alternate block by block in one process, --repeats blocks each after a warm-up
call of every kind; median [min .. max]).

    python tools/time_filter.py [--calls 30] [--repeats 7] [--out profiles/filter_times.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.benchmark_sweep import PRESETS, preset_seed  # noqa: E402
from tools.measure import alternate, fmt, run, stream as st  # noqa: E402
from tools.scenes import SALT  # noqa: E402
from vkvolume_amd import abi, volume as V  # noqa: E402

KINDS = (("binomial", abi.FILTER_BINOMIAL3), ("median", abi.FILTER_MEDIAN3))


def whole_volume_and_boxes(ctx, calls, repeats, out):
    v, tf, _, _ = bench.build_scene(ctx, "c3")
    e = v.extent
    n = e.width * e.height * e.depth
    src, dst, grad = v.volume, torch.empty_like(v.volume), torch.empty_like(v.volume)
    out.append("1. c3: volume %dx%dx%d (%.3f GB read + written per pass); ms per call, GB/s of the algorithmic bytes" % (
        e.width, e.height, e.depth, 2 * n / 1e9))
    kinds = {"vkv_gradient_map": lambda: ctx.gradient_map(src.data_ptr(), grad.data_ptr(), e, tf, st())}
    for name, kind in KINDS:
        kinds["vkv_filter_volume %s" % name] = lambda kind=kind: ctx.filter_volume(src.data_ptr(), dst.data_ptr(), e, None, kind, st())
    runs = alternate(kinds, calls, repeats)
    base = statistics.median(runs["vkv_gradient_map"])
    for k in kinds:
        m = statistics.median(runs[k])
        out.append("  %-28s %s ms  %7.1f GB/s  (%5.2f x the gradient map)" % (k, fmt(runs[k]), 2 * n / 1e9 / (m * 1e-3), m / base))
    out.append("2. box refilter on the same volume: ms per call")
    boxes = (("single voxel", abi.Box(512, 512, 400, 1, 1, 1)), ("256^3", abi.Box(384, 384, 270, 256, 256, 256)),
             ("1024x1024x64", abi.Box(0, 0, 365, 1024, 1024, 64)))
    kinds = {}
    for bname, box in boxes:
        for name, kind in KINDS:
            kinds["%-12s %s" % (bname, name)] = lambda box=box, kind=kind: ctx.filter_volume(src.data_ptr(), dst.data_ptr(), e, box, kind, st())
    runs = alternate(kinds, calls, repeats)
    for k in kinds:
        out.append("  %-28s %s ms" % (k, fmt(runs[k])))
    del v, src, dst, grad
    torch.cuda.empty_cache()


def salt_scene(ctx, calls, repeats, out):
    preset = PRESETS[0]
    extent = preset[1]
    shells, tq, noise, imin = SALT
    kind = 1 | (shells << 8) | (tq << 16) | noise
    size = (1200, 1200)
    out.append("3. salt-noise scene %dx%dx%d (ess_crossover's scattered occupancy, imin %.3f), block 4, frame %dx%d, ERT off: ms per frame" % (
        *extent, imin, *size))

    def prepared(voxels=None):
        v = V.Volume(ctx)
        v.options = abi.VolumeOptions(intensity_min=imin, intensity_max=preset[3], gradient_min=preset[4], gradient_max=preset[5])
        if voxels is None:
            v.load_synthetic(extent, kind=kind, seed=preset_seed(extent), distance_map_block_size=4)
        else:
            v.load_from_array(voxels, distance_map_block_size=4)
        V.default_scene(v)
        tf = v.get_transfer_function_uniform()
        V.ComputeGradientMap(ctx).compute(v, tf)
        v.update_transfer_function_texture()
        V.ComputeDistanceMap(ctx).compute(v, tf, abi.SKIP_DISTANCE)
        torch.cuda.synchronize()
        return v, tf

    raw, _ = prepared()
    filtered, _ = prepared(raw.filter(abi.FILTER_MEDIAN3))
    rgba8 = torch.empty((size[1], size[0], 4), dtype=torch.uint8, device="cuda")
    kinds = {}
    for vname, v in (("raw", raw), ("one median pass", filtered)):
        view, proj = bench.cameras(v, size[0] / size[1])[0]
        for sname, skip in (("no skipping", abi.SKIP_NONE), ("Chebyshev", abi.SKIP_DISTANCE)):
            sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=skip, early_ray_termination=0), size)
            p = sp.make_params(view, proj)
            kinds["%-16s %-12s" % (vname, sname)] = lambda sp=sp, p=p: sp.draw(p, rgba8=rgba8)
    runs = alternate(kinds, calls, repeats)
    for vname, v in (("raw", raw), ("one median pass", filtered)):
        cells = 100.0 * float((v.distance_maps[0] == 0).float().mean().item())
        voxels = bench.occupied_voxel_percent(ctx, v, v.get_transfer_function_uniform())
        out.append("  %-16s occupied voxels %6.3f %%, occupied map cells %6.2f %%" % (vname, voxels, cells))
    for k in kinds:
        out.append("  %-30s %s ms" % (k, fmt(runs[k])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter_times.txt"))
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_filter.py --calls %d --repeats %d on one MI355X (device events; median [min .. max])" % (args.calls, args.repeats)]
        whole_volume_and_boxes(ctx, args.calls, args.repeats, lines)
        salt_scene(ctx, args.calls, args.repeats, lines)
        return lines

    run(args, plain)


if __name__ == "__main__":
    main()

"""Cost of oblique slices and thick slabs (vkv_render_slab) on the bench's C3 scene, next to the dense maximum-intensity projection of the
same image size.

C3 (1024x1024x795 at 1920x1080; bench.py's volume), one pixel per voxel, planes through the volume's centre:
  slice axial     one sample per pixel on the axial plane (normal z)
  slice oblique   one sample per pixel on the plane with normal (1, 2, 3)
  slab N <mode>   N samples per pixel, one per voxel along the oblique plane's normal: MAX dense, MAX with the max map, MIN, MEAN
each on the linear volume and on the packed image, and once, on the same frame size: vkv_render_mip dense (threshold 0.2, orbit view 0).
ms per frame from device events (blocks of --frames calls; the kinds alternate block by block in one process, --repeats blocks each after a
warm-up call of every kind; median [min .. max]), samples filtered per covered pixel and covered pixels (d_out_counts).  Every frame writes
RGBA8 only.

    python tools/time_slab.py [--samples 16,64] [--frames 10] [--repeats 5] [--out profiles/slab_times.txt]
    python tools/time_slab.py --rocprof [--out profiles/slab_rocprof.txt]   the same run (fewer blocks) under rocprofv3 --kernel-trace --stats, in
                                                                           a child process of its own, summarised per kernel
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, kernel_stats, run, stats_table  # noqa: E402
from vkvolume_amd import abi, camera, volume as V  # noqa: E402

MIP_THRESHOLD = 0.2
OBLIQUE = (1.0, 2.0, 3.0)
MODE_NAMES = {abi.SLAB_MAX: "max", abi.SLAB_MIN: "min", abi.SLAB_MEAN: "mean"}


def measure(ctx, samples, frames, repeats, out):
    v, tf, (w, h), _ = bench.build_scene(ctx, "c3")
    view, proj = bench.cameras(v, w / h)[0]
    v.build_max_map()
    torch.cuda.synchronize()
    e, me = v.extent, v.map_extent
    ext = (e.width, e.height, e.depth)
    out.append("c3: volume %dx%dx%d, frame %dx%d, max map %dx%dx%d (block 4), one pixel and one sample step per voxel" % (
        *ext, w, h, me.width, me.height, me.depth))
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, early_ray_termination=0), (w, h))
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    counts = torch.empty((h, w, 3), dtype=torch.int32, device="cuda")
    params = {}
    for packed in (False, True):
        v.use_packed = packed
        params[packed] = sp.make_params(view, proj)

    def stats(fn):
        counts.zero_()
        fn(counts)
        torch.cuda.synchronize()
        c = counts.view(-1, 3).to(torch.int64)
        covered = int(((c[:, 0] + c[:, 2]) > 0).sum())
        return float(c[:, 0].sum()) / max(1, covered), covered

    planes = [("slice axial", camera.slab_plane(ext, axis="z", index=(e.depth - 1) * 0.5, image_size=(w, h)), abi.SLAB_MAX, False),
              ("slice oblique", camera.slab_plane(ext, None, OBLIQUE, (0.0, 1.0, 0.0), (w, h)), abi.SLAB_MAX, False)]
    for n in samples:
        pl = camera.slab_plane(ext, None, OBLIQUE, (0.0, 1.0, 0.0), (w, h), thickness_voxels=float(n - 1))
        assert pl["samples"] == n
        planes += [("slab %d max dense" % n, pl, abi.SLAB_MAX, False), ("slab %d max maxmap" % n, pl, abi.SLAB_MAX, True),
                   ("slab %d min" % n, pl, abi.SLAB_MIN, False), ("slab %d mean" % n, pl, abi.SLAB_MEAN, False)]
    kinds = {}
    for packed in (False, True):
        for name, pl, mode, skip in planes:
            kinds["%-20s %-6s" % (name, "packed" if packed else "linear")] = (
                lambda c=None, pl=pl, mode=mode, skip=skip, packed=packed: sp.draw_slab(params[packed], pl, samples=pl["samples"], mode=mode, skip=skip,
                                                                                        rgba8=rgba8, counts=c))
        kinds["%-20s %-6s" % ("mip %.2f dense" % MIP_THRESHOLD, "packed" if packed else "linear")] = (
            lambda c=None, packed=packed: sp.draw_mip(params[packed], MIP_THRESHOLD, 1.0, rgba8=rgba8, counts=c, skip=False))
    runs = alternate(kinds, frames, repeats)
    mip = {k.split()[-1]: statistics.median(r) for k, r in runs.items() if k.startswith("mip")}
    for k, fn in kinds.items():
        spp, covered = stats(fn)
        out.append("  %s %s ms/frame  (%5.3f of the dense MIP's %7.4f)  %7.1f samples filtered per covered pixel (%d covered)" % (
            k, fmt(runs[k], 8), statistics.median(runs[k]) / mip[k.split()[-1]], mip[k.split()[-1]], spp, covered))
    del v
    torch.cuda.empty_cache()


def rocprof(args):
    rows = kernel_stats(__file__, ["--samples", args.samples, "--frames", "5", "--repeats", "1", "--out", os.devnull], 1100)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_slab.py --samples %s --frames 5 --repeats 1` on one MI355X, a run of its own:" % args.samples,
            "# the slab kernels (k_slab<PACKED, MODE, SKIP>: MODE 0 max, 1 min, 2 mean; SKIP = max map; each kernel serves the slice and both slab",
            "# thicknesses of its mode) and the dense MIP kernels of the same frame size, ms per dispatch"] + stats_table(rows, ("k_slab", "k_mip"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", default="16,64")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_slab.py --samples %s --frames %d --repeats %d on one MI355X (device events; median [min .. max])"
                 % (args.samples, args.frames, args.repeats)]
        measure(ctx, [int(t) for t in args.samples.split(",")], args.frames, args.repeats, lines)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="slab_times.txt", rocprof_name="slab_rocprof.txt")


if __name__ == "__main__":
    main()

"""Cost of the shaded isosurface (vkv_render_isosurface) on the bench's scenes, next to the maximum-intensity projection of the same frame.

Per scene (C3: 1024x1024x795 at 1920x1080; C4: 2048^3 at 3840x2160; bench.py's volume, scale and orbit view 0) and iso value:
  iso dense    vkv_render_isosurface without a max map (every sample up to the hit filtered), 4 refinement steps
  iso maxmap   vkv_render_isosurface with the max map
and once per scene, on the same frame: vkv_render_mip dense and with the max map (threshold 0.2).  ms per frame from device events (blocks
of --frames calls; the kinds alternate block by block in one process, --repeats blocks each; median [min .. max]), samples filtered per
covered pixel and hit pixels (d_out_counts).  Every frame writes RGBA8 only.

    python tools/time_iso.py [--scenes c3,c4] [--isos 0,0.05,0.1,0.2,0.5] [--frames 10] [--repeats 5] [--out profiles/iso_times.txt]
    python tools/time_iso.py --rocprof [--out profiles/iso_rocprof.txt]   the same run (fewer blocks) under rocprofv3 --kernel-trace --stats, in a
                                                                         child process of its own, summarised per kernel
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, fmt, kernel_stats, run, stats_table  # noqa: E402
from vkvolume_amd import abi, volume as V  # noqa: E402

MIP_THRESHOLD = 0.2


def measure(ctx, name, isos, frames, repeats, out):
    v, tf, (w, h), _ = bench.build_scene(ctx, name)
    view, proj = bench.cameras(v, w / h)[0]
    v.build_max_map()
    torch.cuda.synchronize()
    me = v.map_extent
    out.append("%s: volume %dx%dx%d, frame %dx%d, max map %dx%dx%d (block 4)" % (
        name, v.extent.width, v.extent.height, v.extent.depth, w, h, me.width, me.height, me.depth))
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, early_ray_termination=0), (w, h))
    p = sp.make_params(view, proj)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    counts = torch.empty((h, w, 3), dtype=torch.int32, device="cuda")

    def stats(fn):
        counts.zero_()
        rgba8.zero_()
        fn(counts)
        torch.cuda.synchronize()
        c = counts.view(-1, 3).to(torch.int64)
        covered = int(((c[:, 0] + c[:, 2]) > 0).sum())
        hits = int((rgba8.view(-1, 4)[:, 3] == 255).sum())
        return float(c[:, 0].sum()) / max(1, covered), covered, hits

    kinds = {}
    for iso in isos:
        for skip in (False, True):
            kinds["iso %.2f %-6s" % (iso, "maxmap" if skip else "dense")] = (
                lambda c=None, iso=iso, skip=skip: sp.draw_iso(p, iso, rgba8=rgba8, counts=c, skip=skip))
    for skip in (False, True):
        kinds["mip %.2f %-6s" % (MIP_THRESHOLD, "maxmap" if skip else "dense")] = (
            lambda c=None, skip=skip: sp.draw_mip(p, MIP_THRESHOLD, 1.0, rgba8=rgba8, counts=c, skip=skip))
    runs = alternate(kinds, frames, repeats)
    for k, fn in kinds.items():
        spp, covered, hits = stats(fn)
        out.append("  %-18s %s ms/frame   %8.1f samples filtered per covered pixel (%d covered, %d hit)" % (k, fmt(runs[k], 8), spp, covered, hits))
    del v
    torch.cuda.empty_cache()


def rocprof(args):
    rows = kernel_stats(__file__, ["--scenes", args.scenes, "--isos", args.isos, "--frames", "5", "--repeats", "1", "--out", os.devnull], 1200)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_iso.py --scenes %s --isos %s --frames 5 --repeats 1` on one MI355X, a run of"
            % (args.scenes, args.isos),
            "# its own: the isosurface kernels (k_iso<PACKED, SKIP>: SKIP = max map) and the MIP kernels of the same frames, ms per dispatch"
            ] + stats_table(rows, ("k_iso", "k_mip"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="c3,c4")
    ap.add_argument("--isos", default="0,0.05,0.1,0.2,0.5")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_iso.py --scenes %s --isos %s --frames %d --repeats %d on one MI355X (device events; median [min .. max])"
                 % (args.scenes, args.isos, args.frames, args.repeats)]
        for name in args.scenes.split(","):
            measure(ctx, name, [float(t) for t in args.isos.split(",")], args.frames, args.repeats, lines)
            print("\n".join(lines), flush=True)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="iso_times.txt", rocprof_name="iso_rocprof.txt")


if __name__ == "__main__":
    main()

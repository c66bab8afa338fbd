"""Cost of the maximum-intensity projection (vkv_render_mip, vkv_max_map) on the bench's scenes.

Per scene (C3: 1024x1024x795 at 1920x1080; C4: 2048^3 at 3840x2160; bench.py's volume, scale and orbit view 0) and threshold:
  dense      vkv_render_mip without a max map (every sample filtered)
  maxmap     vkv_render_mip with the max map
  render     vkv_render with VKV_SKIP_NONE and early ray termination off, same frame (the integrator's dense march, for comparison)
in ms per frame from device events (blocks of --frames calls; the three kinds alternate block by block in one process, --repeats blocks each;
median [min .. max]), samples filtered per covered pixel (d_out_counts: a pixel is covered when its ray has samples) and, once per scene, the
whole-volume vkv_max_map.  Every frame writes RGBA8 only.

    python tools/time_mip.py [--scenes c3,c4] [--thresholds 0,0.2,0.5] [--frames 10] [--repeats 5] [--out profiles/mip_times.txt]
    python tools/time_mip.py --rocprof [--out profiles/mip_rocprof.txt]   the same run (fewer blocks) under rocprofv3 --kernel-trace --stats, in a
                                                                         child process of its own, summarised per kernel
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tools.measure import alternate, blocks_ms, fmt, kernel_stats, run, stats_table, stream as st  # noqa: E402
from vkvolume_amd import abi, volume as V  # noqa: E402


def measure(ctx, name, thresholds, frames, repeats, out):
    v, tf, (w, h), _ = bench.build_scene(ctx, name)
    view, proj = bench.cameras(v, w / h)[0]
    mm = blocks_ms(lambda: v.build_max_map(), 1, 3, repeats)
    me = v.map_extent
    out.append("%s: volume %dx%dx%d, frame %dx%d, max map %dx%dx%d (block 4)  vkv_max_map %s ms" % (
        name, v.extent.width, v.extent.height, v.extent.depth, w, h, me.width, me.height, me.depth, fmt(mm, 8)))
    mip = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=abi.SKIP_NONE, early_ray_termination=0), (w, h))
    p = mip.make_params(view, proj)
    rgba8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    counts = torch.empty((h, w, 3), dtype=torch.int32, device="cuda")
    rp = abi.RenderParams.from_buffer_copy(p)
    rp.d_out_rgba8, rp.d_out_color, rp.d_out_counts, rp.d_out_depth = rgba8.data_ptr(), None, None, None

    def render():
        ctx.render(rp, st())

    def samples(kind, thr):
        counts.zero_()
        if kind == "render":
            rc = abi.RenderParams.from_buffer_copy(rp)
            rc.d_out_counts = counts.data_ptr()
            ctx.render(rc, st())
        else:
            mip.draw_mip(abi.RenderParams.from_buffer_copy(p), thr, 1.0, rgba8=rgba8, counts=counts, skip=kind == "maxmap")
        torch.cuda.synchronize()
        c = counts.view(-1, 3).to(torch.int64)
        covered = int(((c[:, 0] + c[:, 2]) > 0).sum())
        return float(c[:, 0].sum()) / max(1, covered), covered

    render()
    for thr in thresholds:
        kinds = {"dense": lambda: mip.draw_mip(p, thr, 1.0, rgba8=rgba8, skip=False),
                 "maxmap": lambda: mip.draw_mip(p, thr, 1.0, rgba8=rgba8, skip=True), "render": render}
        runs = alternate(kinds, frames, repeats)
        for k in kinds:
            spp, covered = samples(k, thr)
            label = "render SKIP_NONE ERT off" if k == "render" else "mip %-6s" % k
            out.append("  threshold %.2f  %-24s %s ms/frame   %8.1f samples filtered per covered pixel (%d covered)" % (
                thr, label, fmt(runs[k], 8), spp, covered))
    del v
    torch.cuda.empty_cache()


def rocprof(args):
    rows = kernel_stats(__file__, ["--scenes", args.scenes, "--thresholds", args.thresholds, "--frames", "5", "--repeats", "1", "--out", os.devnull], 1200)
    return ["# rocprofv3 --kernel-trace --stats of `tools/time_mip.py --scenes %s --thresholds %s --frames 5 --repeats 1` on one MI355X, a run of"
            % (args.scenes, args.thresholds),
            "# its own: the MIP kernels (k_mip<PACKED, SKIP>: SKIP = max map), the max map and the integrator's kernels, ms per dispatch"
            ] + stats_table(rows, ("k_mip", "k_max_map", "k_raymarch"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="c3,c4")
    ap.add_argument("--thresholds", default="0,0.2,0.5")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def plain(ctx):
        lines = ["# tools/time_mip.py --scenes %s --thresholds %s --frames %d --repeats %d on one MI355X (device events; median [min .. max])"
                 % (args.scenes, args.thresholds, args.frames, args.repeats)]
        for name in args.scenes.split(","):
            measure(ctx, name, [float(t) for t in args.thresholds.split(",")], args.frames, args.repeats, lines)
            print("\n".join(lines), flush=True)
        return lines

    run(args, plain, lambda: rocprof(args), times_name="mip_times.txt", rocprof_name="mip_rocprof.txt")


if __name__ == "__main__":
    main()

"""Cost of the joint (gradient byte, intensity byte) histogram (vkv_volume_histogram) and of the count read off it (vkv_histogram_occupied_count).

Scenes of the C3 extent (1024 x 1024 x 795), each with its gradient map: bench.py's C3 shells, a constant volume (every voxel in one bin) and
uniform noise in volume and gradient (all 65536 bins in use).  Per scene: whole-volume SET next to vkv_occupied_voxel_count of the same volume
(the yardstick: it reads the same two bytes per voxel), with algorithmic GB/s (2 B/voxel) and the share of 8 TB/s; SUBTRACT + ADD of the
34^3 and 258^3 boxes a 32^3 / 256^3 region update grows; the histogram count; and a counted slider move both ways: vkv_update_transfer_function
with d_occupied_count against the same update without it followed by the histogram count.  Times are HIP events around --reps calls after
--warmup calls, median of --repeats blocks.

    python tools/time_histogram.py [--scenes shells,constant,noise] [--warmup 3] [--reps 20] [--repeats 5] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.measure import blocks_ms, ptr as p, run, spread, stream  # noqa: E402
from vkvolume_amd import abi, lib  # noqa: E402


def measure(ctx, a):
    def timed(fn):
        return spread(blocks_ms(fn, a.warmup, a.reps, a.repeats))

    v, tf, _, _ = bench.build_scene(ctx, "c3")
    st = stream()
    shells = v.volume.clone()
    n_vox = v.volume.numel()
    hist = torch.zeros(abi.HISTOGRAM_BINS, dtype=torch.int64, device="cuda")
    count = torch.zeros(2, dtype=torch.int64, device="cuda")
    lines = ["# ms on one MI355X, C3 extent 1024x1024x795 with its gradient map, app TF (tools/time_histogram.py: HIP events, median [min .. max]",
             "# of %d blocks of %d calls after %d warm-up calls); GB/s = 2 B/voxel / time, share of 8 TB/s" % (a.repeats, a.reps, a.warmup),
             "# " + lib.load().vkv_version().decode()]
    print("\n".join(lines), flush=True)

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    fmt = "%-9s %-44s %8.4f  [%8.4f .. %8.4f]"
    for scene in a.scenes.split(","):
        if scene == "shells":
            v.volume.copy_(shells)
        elif scene == "constant":
            v.volume.fill_(77)
        elif scene == "noise":
            v.volume.random_(0, 256)
        else:
            raise SystemExit("unknown scene %s" % scene)
        ctx.gradient_map(p(v.volume), p(v.gradient), v.extent, tf, st)
        if scene == "noise":  # the gradient of noise is far from uniform: fill it with noise too, so that every bin is hit
            v.gradient.random_(0, 256)
        t_hist = timed(lambda: ctx.volume_histogram(p(v.volume), p(v.gradient), v.extent, None, abi.HISTOGRAM_SET, p(hist), st))
        t_cnt = timed(lambda: ctx.occupied_voxel_count(p(v.volume), p(v.gradient), tf, v.extent, p(count[0:1]), st))
        used = int((hist != 0).sum().item())
        for label, t in (("histogram SET, whole volume", t_hist), ("vkv_occupied_voxel_count (yardstick)", t_cnt)):
            gbs = 2.0 * n_vox / (t[0] * 1e-3) / 1e9
            emit((fmt + "  %7.0f GB/s  %5.1f %%") % ((scene, label) + t + (gbs, 100.0 * gbs / 8000.0)))
        emit("%-9s %-44s %8.3f x   (%d bins in use)" % (scene, "histogram / count", t_hist[0] / t_cnt[0], used))
        w, h, d = v.extent.as_tuple()
        for n in (34, 258):
            b = abi.Box(w // 2 - n // 2, h // 2 - n // 2, d // 2 - n // 2, n, n, n)

            def sub_add():
                ctx.volume_histogram(p(v.volume), p(v.gradient), v.extent, b, abi.HISTOGRAM_SUBTRACT, p(hist), st)
                ctx.volume_histogram(p(v.volume), p(v.gradient), v.extent, b, abi.HISTOGRAM_ADD, p(hist), st)

            emit(fmt % ((scene, "SUBTRACT + ADD of a %d^3 box" % n) + timed(sub_add)))
        ctx.volume_histogram(p(v.volume), p(v.gradient), v.extent, None, abi.HISTOGRAM_SET, p(hist), st)
        emit(fmt % ((scene, "vkv_histogram_occupied_count") +
                    timed(lambda: ctx.histogram_occupied_count(p(hist), tf, p(count[1:2]), st))))
        torch.cuda.synchronize()
        assert count[0].item() == count[1].item(), "counts differ: %s" % count.tolist()
        if scene == "shells":  # a counted slider move, both ways (Chebyshev map)
            maps = [p(m) for m in (v.distance_maps[:1] if v.distance_maps else [])]
            if not maps:
                v.set_number_of_distance_maps(1)
                maps = [p(v.distance_maps[0])]
            opt = v.options

            def move(d_count):
                ctx.update_transfer_function(opt, p(v.volume), p(v.gradient), v.extent, p(v.transfer_function), p(v.transfer_function_bits), maps,
                                             p(v.distance_map_swap), v.map_extent, abi.SKIP_DISTANCE, d_count, st)

            emit(fmt % ((scene, "slider move, uncounted") + timed(lambda: move(None))))
            emit(fmt % ((scene, "slider move, counted by the volume pass") + timed(lambda: move(p(count[0:1])))))

            def move_hist():
                move(None)
                ctx.histogram_occupied_count(p(hist), tf, p(count[1:2]), st)

            emit(fmt % ((scene, "slider move, counted from the histogram") + timed(move_hist)))
    v.volume.copy_(shells)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--scenes", default="shells,constant,noise")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a, lambda ctx: measure(ctx, a), echo=False)  # the lines are printed as they are measured


if __name__ == "__main__":
    main()

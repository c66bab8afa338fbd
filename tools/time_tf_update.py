"""Cost of one transfer-function slider move (VolumeRender::update_transfer_function, src/volume_render.cpp:392-445, + one frame).

Three variants per scene, each timed as ms per move (update + one 1920x1080 / 3840x2160 frame) and as ms per update alone:
  host    Volume.update_transfer_function_texture (CPU loop over 65536 texels, pageable 256 KiB copy, stream wait, tables) +
          ComputeDistanceMap.compute (bit table from the texture, occupancy, transform) - the blocking path;
  device  Volume.update_transfer_function: one enqueue, no host loop, no upload, no wait;
  graph   the device update (+ the frame) captured once into a hipGraph and replayed (the options of the capture).
Every move shifts intensity_min by a small step (the graph replays one setting).  A block of --moves moves is timed by the wall clock
between two device synchronisations; --repeats blocks per variant give the median and the spread.  Scenes: C3 (1024x1024x795, Chebyshev
and anisotropic, block 4) and C4 (2048^3 anisotropic; skipped when the device has no room for it).

    python tools/time_tf_update.py [--scenes c3_cheb,c3_aniso,c4_aniso] [--paths host,device,graph] [--moves 20] [--repeats 5] [--out FILE]

Under `rocprofv3 --kernel-trace --stats` with --paths device, every update is one k_tf_build dispatch: the sum of the update's kernel times
per k_tf_build dispatch is what the wall-clock "update alone" column is set against.
"""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.measure import run, wall_ms  # noqa: E402
from vkvolume_amd import abi, camera, lib, volume as V  # noqa: E402

# name: (extent, seed, voxel size, axis-angle, frame, skipping type) - the C3 / C4 scenes of bench.py
SCENES = {
    "c3_cheb": ((1024, 1024, 795), 0xC0FFEE03, (0.0003, 0.0003, 0.0007), (1.0, 0.0, 0.0, 90.0), (1920, 1080), abi.SKIP_DISTANCE),
    "c3_aniso": ((1024, 1024, 795), 0xC0FFEE03, (0.0003, 0.0003, 0.0007), (1.0, 0.0, 0.0, 90.0), (1920, 1080), abi.SKIP_ANISOTROPIC_DISTANCE),
    "c4_aniso": ((2048, 2048, 2048), 0xC0FFEE04, (1.0, 1.0, 1.0), (1.0, 0.0, 0.0, 0.0), (3840, 2160), abi.SKIP_ANISOTROPIC_DISTANCE),
}
STEP = 0.002


def build(ctx, name):
    extent, seed, voxel, axis_angle, frame, skip = SCENES[name]
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(intensity_min=0.1, intensity_max=1.0, gradient_min=0.0, gradient_max=0.2)
    v.load_synthetic(extent, kind=1, seed=seed, distance_map_block_size=4)
    V.default_scene(v, voxel, axis_angle)
    V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
    v.update_transfer_function(skip)
    m = (v.node_transform.astype(np.float64).T @ v.image_transform.astype(np.float64).T)[:3, :3]
    radius = 1.5 * 0.5 * math.sqrt(sum(float(np.linalg.norm(m[:, i])) ** 2 for i in range(3)))
    view, proj = camera.orbit_camera(30.0, 20.0, radius), camera.perspective_vulkan(60.0, frame[0] / frame[1], 0.1, 1000.0)
    sp = V.VolumeRenderSubpass(ctx, v, abi.RenderOptions(skipping_type=skip, clip_distance=1.0), frame)
    params = sp.make_params(view, proj)
    rgba8 = torch.empty((frame[1], frame[0], 4), dtype=torch.uint8, device="cuda")
    params.d_out_rgba8 = rgba8.data_ptr()
    ctx.prepare_render([params], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return v, sp, params, rgba8, skip


def measure(ctx, name, moves, repeats, warmup, paths):
    v, sp, params, rgba8, skip = build(ctx, name)
    cdm = V.ComputeDistanceMap(ctx)
    base = v.options.intensity_min

    def host(k, frame):
        v.options.intensity_min = base + STEP * (k % 8)
        v.update_transfer_function_texture()
        cdm.compute(v, v.get_transfer_function_uniform(), skip)
        if frame:
            sp.draw(params, rgba8=rgba8)

    def device(k, frame):
        v.options.intensity_min = base + STEP * (k % 8)
        v.update_transfer_function(skip)
        if frame:
            sp.draw(params, rgba8=rgba8)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        device(0, True)  # the capture stream's scratch block
    torch.cuda.synchronize()
    graphs = {}
    for frame in (True, False):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            device(0, frame)
        graphs[frame] = g
    torch.cuda.synchronize()

    def graph(k, frame):
        graphs[frame].replay()

    rows = []
    for label, fn in (("host", host), ("device", device), ("graph", graph)):
        if label not in paths:
            continue
        res = {}
        for frame in (True, False):
            def block(n):  # moves 0 .. n-1: every block starts from the same setting
                for k in range(n):
                    fn(k, frame)

            wall_ms(lambda: block(warmup), 1, 1)
            res[frame] = [t / moves for t in wall_ms(lambda: block(moves), 1, repeats)]
        rows.append((label, res))
    del graphs
    ctx.release_stream(s.cuda_stream)
    del v, sp
    torch.cuda.empty_cache()
    return rows


def fmt(runs):
    return "%8.3f  [%7.3f .. %7.3f]" % (statistics.median(runs), min(runs), max(runs))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="c3_cheb,c3_aniso,c4_aniso")
    ap.add_argument("--paths", default="host,device,graph")
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def plain(ctx):
        lines = ["# ms per slider move: median [min .. max] of %d blocks of %d moves (wall clock, device synchronised around each block)" % (a.repeats, a.moves),
                 "# %s, %s" % (torch.cuda.get_device_name(0), lib.load().vkv_version().decode()),
                 "%-9s %-7s %-30s %-30s" % ("scene", "path", "update + frame (ms)", "update alone (ms)")]
        for name in a.scenes.split(","):
            try:
                rows = measure(ctx, name, a.moves, a.repeats, a.warmup, a.paths.split(","))
            except torch.cuda.OutOfMemoryError as e:
                lines.append("%-9s skipped: %s" % (name, str(e).splitlines()[0]))
                torch.cuda.empty_cache()
                continue
            for label, res in rows:
                lines.append("%-9s %-7s %-30s %-30s" % (name, label, fmt(res[True]), fmt(res[False])))
            print("\n".join(lines[-len(rows):]), flush=True)
        return lines

    run(a, plain)
    print()  # the report has always ended on an empty line


if __name__ == "__main__":
    main()

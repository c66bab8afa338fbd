"""Cost of a region update of the volume (vkv_update_volume_region) against the full rebuild it replaces, on the C3 scene.

For boxes of 1^3, 32^3, 128^3 and 256^3 voxels (centred), a 1024 x 1024 x 64 z-slab and the whole volume, and for the Chebyshev and the
anisotropic map: ms per region update (uint8 source already on the device: convert + scatter, gradient of the grown box, the bricks and
occupancy cells it reaches, map reset and the whole-map transform) and ms per full chain on the same stream (vkv_gradient_map +
vkv_pack_volume + vkv_compute_distance_map of the whole volume; no upload).  Times are HIP events around --reps calls after --warmup calls,
median of --repeats blocks.  The source holds the box's current voxels, so the scene stays the same from call to call.

    python tools/time_volume_region.py [--maps cheb,aniso] [--warmup 3] [--reps 20] [--repeats 5] [--out FILE]

Under `rocprofv3 --kernel-trace --stats` every region update starts with one k_convert_box dispatch.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.measure import blocks_ms, ptr as p, run, spread, stream  # noqa: E402
from vkvolume_amd import abi, lib, volume as V  # noqa: E402

MAPS = {"cheb": abi.SKIP_DISTANCE, "aniso": abi.SKIP_ANISOTROPIC_DISTANCE}


def boxes(ext):
    w, h, d = ext.as_tuple()
    out = []
    for n in (1, 32, 128, 256):
        out.append(("%d^3" % n, abi.Box(w // 2 - n // 2, h // 2 - n // 2, d // 2 - n // 2, n, n, n)))
    out.append(("%dx%dx64 slab" % (w, h), abi.Box(0, 0, d // 2 - 32, w, h, 64)))
    out.append(("whole volume", abi.Box(0, 0, 0, w, h, d)))
    return out


def measure(ctx, a):
    def timed(fn):
        return spread(blocks_ms(fn, a.warmup, a.reps, a.repeats))

    v, tf, _, _ = bench.build_scene(ctx, "c3")
    st = stream()
    lines = ["# ms per region update of the C3 volume (1024x1024x795, block 4, gradient precomputed, packed image, app TF) on one MI355X",
             "# (tools/time_volume_region.py: HIP events, median [min .. max] of %d blocks of %d calls after %d warm-up calls)" % (a.repeats, a.reps, a.warmup),
             "# region = vkv_update_volume_region with a uint8 source on the device; chain = vkv_gradient_map + vkv_pack_volume +",
             "# vkv_compute_distance_map of the whole volume on the same stream (no upload in either)",
             "# " + lib.load().vkv_version().decode(),
             "%-6s %-22s %-36s %-36s" % ("maps", "box", "region update (ms)", "full chain (ms)")]
    print("\n".join(lines), flush=True)
    for name in a.maps.split(","):
        skip = MAPS[name]
        V.ComputeDistanceMap(ctx).compute(v, tf, skip)
        n = 8 if skip == abi.SKIP_ANISOTROPIC_DISTANCE else 1
        maps = [p(m) for m in v.distance_maps[:n]]

        def chain():
            ctx.gradient_map(p(v.volume), p(v.gradient), v.extent, tf, st)
            ctx.pack_volume(p(v.volume), p(v.gradient), v.extent, p(v.packed), st)
            ctx.compute_distance_map(p(v.volume), p(v.gradient), p(v.transfer_function), tf, v.extent, maps, p(v.distance_map_swap), v.map_extent, skip, st)

        t_chain = timed(chain)
        for label, b in boxes(v.extent):
            src = v.volume[b.z0:b.z0 + b.depth, b.y0:b.y0 + b.height, b.x0:b.x0 + b.width].contiguous()

            def region():
                ctx.update_volume_region(p(src), 0, False, 0.0, 255.0, b, p(v.volume), p(v.gradient), p(v.packed), v.extent, p(v.transfer_function), tf,
                                         maps, p(v.distance_map_swap), v.map_extent, skip, st)

            t = timed(region)
            line = "%-6s %-22s %8.3f  [%8.3f .. %8.3f]      %8.3f  [%8.3f .. %8.3f]" % ((name, label) + t + t_chain)
            lines.append(line)
            print(line, flush=True)
            del src
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--maps", default="cheb,aniso")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a, lambda ctx: measure(ctx, a), echo=False)  # the lines are printed as they are measured


if __name__ == "__main__":
    main()

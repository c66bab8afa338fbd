"""Cost of the cell summaries and of a slider move decided from them (vkv_cell_summary, vkv_occupancy_map_from_summary,
vkv_update_transfer_function_from_summary) against the voxel path (vkv_occupancy_map, vkv_update_transfer_function).

Per scene and block size: the whole-volume summary build (ms); then for each intensity_min of the sweep (the other options are the
application's: intensity_max 1, gradient 0 .. 0.2):
  occ      the occupancy step alone: vkv_occupancy_map (bit table from the texture, fill, k_occupancy_map_waves) against
           vkv_occupancy_map_from_summary (bit table, range table, classification + the unresolved cells' voxels);
  update   the whole update alone (texture + tables, occupancy, transform of the scene's skipping type): vkv_update_transfer_function against
           vkv_update_transfer_function_from_summary;
  share    the unresolved cells' share of the map.
Times are medians [min .. max] of --repeats blocks of --moves calls (wall clock between device synchronisations, per call).  Scenes: the C3
(1024x1024x795, Chebyshev and anisotropic) and C4 (2048^3 anisotropic) scenes of tools/time_tf_update.py.

    python tools/time_cell_summary.py [--scenes c3_cheb,c3_aniso,c4_aniso] [--blocks 2,4,6] [--imins 0.05,0.1,0.2,0.3,0.5] [--moves 10]
                                      [--repeats 3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.measure import fmt as fmt_ms, run, stream as st, wall_ms  # noqa: E402
from vkvolume_amd import abi, lib, volume as V  # noqa: E402

SCENES = {
    "c3_cheb": ((1024, 1024, 795), 0xC0FFEE03, abi.SKIP_DISTANCE),
    "c3_aniso": ((1024, 1024, 795), 0xC0FFEE03, abi.SKIP_ANISOTROPIC_DISTANCE),
    "c4_aniso": ((2048, 2048, 2048), 0xC0FFEE04, abi.SKIP_ANISOTROPIC_DISTANCE),
}


def fmt(runs):
    return fmt_ms(runs, 7, 3)


def measure(ctx, name, block, imins, moves, repeats):
    extent, seed, skip = SCENES[name]
    v = V.Volume(ctx)
    v.options = abi.VolumeOptions(intensity_min=0.1, intensity_max=1.0, gradient_min=0.0, gradient_max=0.2)
    v.load_synthetic(extent, kind=1, seed=seed, distance_map_block_size=block)
    V.ComputeGradientMap(ctx).compute(v, v.get_transfer_function_uniform())
    v.update_transfer_function(skip)
    v.build_cell_summary()
    build = wall_ms(lambda: v.build_cell_summary(), max(1, moves // 2), repeats, warmup=1)
    me = v.map_extent
    n_cells = me.width * me.height * me.depth
    occ = torch.empty(n_cells, dtype=torch.uint8, device="cuda")
    unres = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = ["%-9s block %d  map %dx%dx%d  summary build %s ms" % (name, block, me.width, me.height, me.depth, fmt(build))]
    for imin in imins:
        v.options.intensity_min = imin
        v.update_transfer_function(skip)  # the texture of this setting
        tf = v.get_transfer_function_uniform()

        def occ_voxels():
            ctx.occupancy_map(v.volume.data_ptr(), v.gradient.data_ptr(), v.transfer_function.data_ptr(), tf, v.extent, occ.data_ptr(), me, st())

        def occ_summary():
            ctx.occupancy_map_from_summary(v.cell_summary.data_ptr(), v.volume.data_ptr(), v.gradient.data_ptr(), v.transfer_function.data_ptr(), tf,
                                           v.extent, occ.data_ptr(), me, unres.data_ptr(), st())

        t_ov, t_os = wall_ms(occ_voxels, moves, repeats, warmup=2), wall_ms(occ_summary, moves, repeats, warmup=2)
        torch.cuda.synchronize()
        share = int(unres.item()) / n_cells
        t_uv = wall_ms(lambda: v.update_transfer_function(skip), moves, repeats, warmup=2)
        t_us = wall_ms(lambda: v.update_transfer_function_from_summary(skip), moves, repeats, warmup=2)
        rows.append("    imin %.2f  occ voxels %s  summary %s (x%.2f)  update voxels %s  summary %s  unresolved %.4f%%" % (
            imin, fmt(t_ov), fmt(t_os), statistics.median(t_os) / statistics.median(t_ov), fmt(t_uv), fmt(t_us), 100.0 * share))
        print(rows[-1], flush=True)
    del v, occ
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="c3_cheb,c3_aniso,c4_aniso")
    ap.add_argument("--blocks", default="2,4,6")
    ap.add_argument("--imins", default="0.05,0.1,0.2,0.3,0.5")
    ap.add_argument("--moves", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def plain(ctx):
        lines = ["# ms per call: median [min .. max] of %d blocks of %d calls (wall clock, device synchronised around each block)" % (a.repeats, a.moves),
                 "# %s, %s" % (torch.cuda.get_device_name(0), lib.load().vkv_version().decode())]
        imins = [float(x) for x in a.imins.split(",")]
        for name in a.scenes.split(","):
            for block in (int(b) for b in a.blocks.split(",")):
                try:
                    lines += measure(ctx, name, block, imins, a.moves, a.repeats)
                except torch.cuda.OutOfMemoryError as e:
                    lines.append("%-9s block %d skipped: %s" % (name, block, str(e).splitlines()[0]))
                    torch.cuda.empty_cache()
                print(lines[-1], flush=True)
        return lines

    run(a, plain)
    print()  # the report has always ended on an empty line


if __name__ == "__main__":
    main()

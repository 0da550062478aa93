"""The treetops of a height raster as a GeoPackage point layer (treedetection_amd.treetops.treetops_file; the seeds of the reference's
supplementary/pretraining_generate_voronoi.py, found in one GPU launch).

    python tools/treetops.py <height.tif> <out.gpkg> [--sigma 0.5] [--window 7] [--min-height 3.0] [--device 0 | --host] [--device-decode]

The raster is smoothed with a Gaussian of ``--sigma`` pixels; a pixel is a treetop when its smoothed height exceeds ``--min-height``
and is the maximum of the ``--window`` x ``--window`` pixels around it. One point per treetop at the pixel's centre, with the columns
Height (smoothed), Row, Col and Crown (0)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    from treedetection_amd.treetops import treetops_file

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("height")
    ap.add_argument("out")
    ap.add_argument("--sigma", type=float, default=0.5)
    ap.add_argument("--window", type=int, default=7)
    ap.add_argument("--min-height", type=float, default=3.0)
    ap.add_argument("--device", type=int, default=0, help="GPU index (default 0)")
    ap.add_argument("--host", action="store_true", help="the host function instead of the GPU (same results)")
    ap.add_argument("--device-decode", action="store_true", help="decode the raster on the GPU where its layout allows")
    args = ap.parse_args(argv)
    n = treetops_file(args.height, args.out, args.sigma, args.window, args.min_height, None if args.host else args.device, args.device_decode)
    print(f"{n} treetop(s) written to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

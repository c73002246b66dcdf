#!/usr/bin/env python3
"""COLMAP dense folder (images/ + sparse/) -> the MVSNet-style folder tools/mpmvs_main.py reads: cams/%08d_cam.txt,
pair.txt and images/%08d.*, the outputs of the reference's colmap2mvsnet_acm.py (same flags).  The model is read in C++
and the view selection runs on the GPU (mp-mvs_amd/colmap.py; contract in DESIGN.md section 11).

  python tools/colmap2mvs.py --dense_folder <colmap dense folder> --save_folder <out> [--max_d 192] [--interval_scale 1]
                             [--model_ext .bin|.txt] [--num_view 20] [--device 0] [--overwrite]
                             [--undistort [--blank_pixels 0] [--min_scale 0.2] [--max_scale 2.0]]

--undistort takes a plain sparse model with distorted cameras (SIMPLE_RADIAL, OPENCV, the fisheye models ...): the images are
resampled on the GPU to the pinhole cameras COLMAP's image_undistorter would choose and written as .pgm / .ppm, and cams/
holds those cameras.  Without it the input is expected to be COLMAP's undistorted dense folder.

Differences from the reference: it refuses to replace non-empty <save_folder>/images or /cams unless --overwrite is
given (the reference deletes them); .jpeg / .JPG images are copied byte for byte like .jpg (the reference re-encodes
them), other formats are written losslessly as .pgm / .ppm; --model_ext defaults to .bin when cameras.bin exists."""
import argparse
import importlib
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description="COLMAP sparse model -> cams/, pair.txt, images/")
    ap.add_argument("--dense_folder", required=True)
    ap.add_argument("--save_folder", required=True)
    ap.add_argument("--max_d", type=int, default=192)
    ap.add_argument("--interval_scale", type=float, default=1)
    ap.add_argument("--theta0", type=float, default=5, help="accepted and ignored, as in the reference")
    ap.add_argument("--sigma1", type=float, default=1, help="accepted and ignored, as in the reference")
    ap.add_argument("--sigma2", type=float, default=10, help="accepted and ignored, as in the reference")
    ap.add_argument("--model_ext", choices=[".txt", ".bin"], default=None, help="default: .bin if sparse/cameras.bin exists, else .txt")
    ap.add_argument("--num_view", type=int, default=20, help="views listed per image (at most N - 1)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--overwrite", action="store_true", help="replace existing save_folder/images and /cams")
    ap.add_argument("--undistort", action="store_true", help="undistort the images of distorted cameras on the GPU (no image_undistorter run needed)")
    ap.add_argument("--blank_pixels", type=float, default=0.0, help="with --undistort: 0 = no blank pixel in the output ... 1 = every source pixel kept")
    ap.add_argument("--min_scale", type=float, default=0.2, help="with --undistort: lower limit of the change of image size")
    ap.add_argument("--max_scale", type=float, default=2.0, help="with --undistort: upper limit of the change of image size")
    a = ap.parse_args()
    colmap = importlib.import_module("mp-mvs_amd.colmap")
    t0 = time.perf_counter()
    try:
        times = colmap.convert(a.dense_folder, a.save_folder, max_d=a.max_d, interval_scale=a.interval_scale, model_ext=a.model_ext,
                               num_view=a.num_view, device=a.device, overwrite=a.overwrite, undistort=a.undistort, blank_pixels=a.blank_pixels,
                               min_scale=a.min_scale, max_scale=a.max_scale)
    except (FileExistsError, ValueError) as e:
        print(f"colmap2mvs: {e}", file=sys.stderr)
        return 2
    print(" ".join(f"{k} {v:.3f} s" for k, v in times.items()) + f"; total {time.perf_counter() - t0:.3f} s -> {os.path.abspath(a.save_folder)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Writes tests/golden/treetops/*.npz: small NaN-free rasters of tests/treetop_cases.py with what scipy gives for them —
``gaussian_filter(raster, sigma)`` (float32 in and out) and ``argwhere((s == maximum_filter(s, size=window)) & (s > floor))`` —
so that the comparison with scipy also runs where scipy is not installed. Recorded with scipy 1.15.3:
    python tests/golden/make_treetops_golden.py
"""
import os
import sys

import numpy as np
import scipy
import scipy.ndimage as nd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import treetop_cases as tc  # noqa: E402

PICK = [((1, 1), 0.5, 7, False), ((1, 9), 1.0, 3, False), ((3, 2), 2.0, 7, False), ((2, 7), 0.5, 15, True), ((17, 5), 2.0, 3, True),
        ((5, 300), 0.5, 7, False), ((64, 64), 1.0, 7, True), ((65, 129), 0.5, 7, True), ((70, 131), 2.0, 15, False), ((70, 131), 0.5, 7, True)]

if __name__ == "__main__":
    os.makedirs(tc.GOLDEN, exist_ok=True)
    for i, (shape, sigma, k, plateaus) in enumerate(PICK):
        a = tc.canopy(shape, 9000 + i, plateaus)
        s = nd.gaussian_filter(a, sigma=sigma)
        assert s.dtype == np.float32
        tops = np.argwhere((s == nd.maximum_filter(s, size=k)) & (s > np.float32(tc.FLOOR)))
        name = f"{shape[0]}x{shape[1]}_s{sigma}_k{k}_{'plateau' if plateaus else 'random'}.npz"
        np.savez_compressed(os.path.join(tc.GOLDEN, name), raster=a, sigma=np.float64(sigma), window=np.int64(k), floor=np.float64(tc.FLOOR),
                            smoothed=s, tops=tops.astype(np.int64), scipy_version=np.array(scipy.__version__))
        print(name, len(tops), "treetops")

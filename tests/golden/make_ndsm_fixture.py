"""Generates tests/golden/ndsm_324125317.npz from the one raster the reference ships (data/nDSM/324125317.tif):

    python tests/golden/make_ndsm_fixture.py <path to 324125317.tif>

The raster is 4 MB of float32, too large to keep here. The fixture keeps what the reader parses byte for byte: the file's
first PIXEL_OFFSET bytes (TIFF header, IFD, tag values, the strip table GDAL wrote), and, of the pixel data, every 5th row
and column in centimetres (uint16 [200, 200]). tests/test_host_api.py rebuilds a file of the original length from the two:
the header verbatim, then the grid repeated 5 x 5 as float32 metres, so the verbatim strip offsets and byte counts still
describe it. Range and mean stay those of the survey (0 .. 50.89 m, mean 5.73 m).
"""
import os
import sys

import numpy as np

PIXEL_OFFSET = 3542        # the strips follow the header and IFD, contiguous and in row order
SIDE, STEP = 1000, 5


def main(path):
    raw = open(path, "rb").read()
    assert len(raw) == PIXEL_OFFSET + SIDE * SIDE * 4
    a = np.frombuffer(raw[PIXEL_OFFSET:], "<f4").reshape(SIDE, SIDE)
    cm = np.round(a[::STEP, ::STEP].astype(np.float64) * 100).astype(np.uint16)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ndsm_324125317.npz")
    np.savez_compressed(out, header=np.frombuffer(raw[:PIXEL_OFFSET], np.uint8), cm=cm, step=np.int32(STEP))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

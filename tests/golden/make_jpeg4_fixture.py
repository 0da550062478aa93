"""Writes tests/golden/jpeg4/*.jpg + *.raw: four-component JPEG streams from Pillow's CMYK encoder (1x1 sampling, an Adobe segment of
transform 0) and the bytes they store as Pillow's libjpeg decodes them (raw mode CMYK, [h][w][4]) — the input of the stand-alone
sanitizer program treedetection_amd/csrc/checks/jpeg4_check.cpp (`make -C treedetection_amd/csrc jpeg4-check`), which has no encoder
and no libjpeg of its own. tests/test_jpeg4_decode.py checks the committed files against Pillow again.
python tests/golden/make_jpeg4_fixture.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from test_jpeg4_decode import encode, image, pillow      # noqa: E402

CASES = {"noise_40x56_q90_r3": (40, 56, "noise", dict(quality=90, restart_marker_blocks=3)),
         "smooth_13x17_q30_opt": (13, 17, "smooth", dict(quality=30, optimize=True)),
         "smooth_64x48_q100": (64, 48, "smooth", dict(quality=100))}

if __name__ == "__main__":
    os.makedirs(os.path.join(HERE, "jpeg4"), exist_ok=True)
    for name, (h, w, kind, kw) in CASES.items():
        stream = encode(image(h, w, kind, seed=7), **kw)
        with open(os.path.join(HERE, "jpeg4", name + ".jpg"), "wb") as f:
            f.write(stream)
        with open(os.path.join(HERE, "jpeg4", name + ".raw"), "wb") as f:
            f.write(pillow(stream)[1].tobytes())
        print(name, len(stream), "bytes")

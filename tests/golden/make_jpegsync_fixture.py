"""Writes tests/golden/jpegsync/*.jpg: grey and three-component JPEG streams from Pillow's encoder, the input (with the four-component
streams of tests/golden/jpeg4) of the stand-alone sanitizer program treedetection_amd/csrc/checks/jpegsync_check.cpp
(`make -C treedetection_amd/csrc jpegsync-check`), which has no encoder of its own: it compares the many-lane decoder
(td_jpeg_decode_sync) with the sequential one (td_jpeg_decode), which tests/test_jpeg_decode.py pins against Pillow.
tests/test_jpeg_sync.py checks the committed files against Pillow again.
python tests/golden/make_jpegsync_fixture.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from test_jpeg_sync import encode, image      # noqa: E402

# name: (rows, cols, content, sampling, encoder options) — six blocks per MCU on noise (slow to synchronise), smooth content (fast),
# quality 100 (FF 00 pairs everywhere), restart intervals + optimised tables (many short segments), 4:2:2, grey
CASES = {"noise_96x128_420_q90": (96, 128, "noise", "420", dict(quality=90)),
         "smooth_120x160_444_q50": (120, 160, "smooth", "444", dict(quality=50)),
         "noise_40x56_444_q100": (40, 56, "noise", "444", dict(quality=100)),
         "smooth_71x133_422_q90_r5_opt": (71, 133, "smooth", "422", dict(quality=90, restart_marker_blocks=5, optimize=True)),
         "noise_64x64_grey_q75": (64, 64, "noise", "L", dict(quality=75))}

if __name__ == "__main__":
    os.makedirs(os.path.join(HERE, "jpegsync"), exist_ok=True)
    for name, (h, w, kind, mode, kw) in CASES.items():
        stream = encode(image(h, w, kind, seed=7), mode, **kw)
        with open(os.path.join(HERE, "jpegsync", name + ".jpg"), "wb") as f:
            f.write(stream)
        print(name, len(stream), "bytes")

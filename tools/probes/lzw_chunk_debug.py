"""Debug: decode single LZW streams on the GPU (chunk path) and report the first differing byte against the host decoder."""
import sys, os
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from treedetection_amd import _lib
from treedetection_amd.device_decode import LZW, alloc_block_buffers, launch_block_decoder
from treedetection_amd.synth import make_tile
lib = _lib.load()
rng = np.random.default_rng(0)
rgb, _ = make_tile(3, 700)
cases = {"tile": np.ascontiguousarray(rgb[:128, :128]).tobytes(), "noise": rng.integers(0, 256, 30000, dtype=np.uint8).tobytes(),
         "ramp": bytes(range(256)) * 100, "few": rng.integers(0, 3, 40000, dtype=np.uint8).tobytes(), "lit300": rng.integers(0, 256, 300, dtype=np.uint8).tobytes(),
         "lit1000": rng.integers(0, 256, 1000, dtype=np.uint8).tobytes(), "pairs": (bytes([1, 2, 3, 4, 5, 6, 7, 8]) * 40)}
for name, raw in cases.items():
    src = np.frombuffer(raw, np.uint8); enc = np.empty(len(raw) * 2 + 64, np.uint8)
    n = lib.td_tiff_lzw_encode(src.ctypes.data, src.size, enc.ctypes.data, enc.size)
    comp = torch.from_numpy(np.concatenate([enc[:n], np.zeros(16, np.uint8)])).cuda()
    meta = torch.tensor([[0], [n]], dtype=torch.int64, device="cuda")
    cap = len(raw) + 64
    for one in ("1", "0"):
        os.environ["TD_LZW_ONE_BY_ONE"] = one
        bufs = alloc_block_buffers(LZW, 1, cap, "cuda")
        out, dec, st = bufs.blocks.zero_(), bufs.decoded.zero_(), bufs.status.fill_(-1)
        launch_block_decoder(LZW, comp, meta, bufs, _lib.stream_ptr())
        torch.cuda.synchronize()
        got = out[0, :len(raw)].cpu().numpy()
        d = np.nonzero(got != src)[0]
        print(name, "one_by_one" if one == "1" else "chunks", "status", st[:1].tolist(), "decoded", int(dec[0]) & 0xffffffff, "of", len(raw), "first diffs", d[:6].tolist(),
              "got", got[d[:6]].tolist() if len(d) else "", "want", src[d[:6]].tolist() if len(d) else "")

"""The steps of the device raster path, each once: where the blocks' byte ranges lie in the staging buffer, the file read into it, the
buffers a block codec needs, the decoder launch by compression, the layout launch by sample size and planar flag, and the ``check``
every device path hands back. ``GeoTiff.decode_to_device`` / ``upload_to_device`` (geotiff.py) compose them in the order the stream
sees them; tools/raster_decode_bench.py times the launches through the same calls, so it measures what the product runs."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np

from . import _lib

LZW, DEFLATE, ZSTD = 5, (8, 32946), 50000                      # TIFF Compression values of the block codecs


def stage_offsets(offs, ranges):
    """The ranges [(lo, hi), ...] of the file (``GeoTiff.device_block_plan``) lie one behind the other in the staging buffer (one range,
    unless planes were left out) → (rel: every block's offset in that buffer, starts: where each range begins there, + the end, span:
    the bytes in all)."""
    r_lo = np.array([r[0] for r in ranges], dtype=np.int64)
    starts = np.cumsum([0] + [hi - lo for lo, hi in ranges])
    which = np.searchsorted(r_lo, offs, side="right") - 1
    return offs - r_lo[which] + starts[:-1][which], starts, int(starts[-1])


def read_ranges(path, parts, buf, pool, what):
    """Reads ``parts`` [(position in ``buf``, bytes, position in the file), ...] of ``path`` into the uint8 array ``buf``, on ``pool``
    when there is more than one. A generator: each part is handed back once it (and the parts before it) is in the buffer, so the
    caller can copy on while the rest is read; nothing is read unless it is iterated. ``what`` names the data in the error."""
    fd = os.open(path, os.O_RDONLY)
    view = memoryview(buf)

    def one(pr):
        got = 0
        while got < pr[1]:
            n = os.preadv(fd, [view[pr[0] + got:pr[0] + pr[1]]], pr[2] + got)
            if n <= 0:
                raise ValueError(f"{path}: file ends inside its {what}")
            got += n
        return pr
    try:
        yield from (pool.map(one, parts) if pool is not None and len(parts) > 1 else map(one, parts))
    finally:
        os.close(fd)


def alloc_block_buffers(compression, nb, block_cap, dev):
    """What the block decoders write: ``blocks`` [nb, block_cap] bytes, ``decoded`` (bytes per block; LZW: + the slow codes in the high
    half), ``status`` ([nb] + the scratch of the wide-table pass), DEFLATE ``ends`` (where each trailer begins), ZSTD ``lits`` (the
    literal buffers of the resident decoder waves); None where the codec has no use for one."""
    import torch
    bufs = SimpleNamespace(blocks=torch.empty((nb, block_cap), dtype=torch.uint8, device=dev), decoded=torch.empty((nb,), dtype=torch.int64, device=dev),
                           status=torch.empty((2 * nb + 1,), dtype=torch.int32, device=dev), ends=None, lits=None)
    if compression in DEFLATE:
        bufs.ends = torch.empty((nb,), dtype=torch.int64, device=dev)
    if compression == ZSTD:
        bufs.lits = torch.empty((max(int(_lib.load().td_tiff_zstd_scratch_bytes(nb)), 1),), dtype=torch.uint8, device=dev)
    return bufs


def launch_block_decoder(compression, comp, meta, bufs, stream_ptr, verified=True):
    """One wave per block: ``comp`` (the staged bytes, 16 spare ones behind them) and ``meta`` ([2, nb] int64: offsets in it, sizes) →
    ``bufs``. DEFLATE also checks every block's Adler-32 trailer, in a launch of its own, unless ``verified=False``."""
    lib = _lib.load()
    nb, block_cap = bufs.blocks.shape
    head = (comp.data_ptr(), meta[0].data_ptr(), meta[1].data_ptr(), nb, bufs.blocks.data_ptr(), block_cap, bufs.decoded.data_ptr(), bufs.status.data_ptr())
    if compression == LZW:
        name, tail = "td_tiff_lzw_decode_dev", ()
    elif compression == ZSTD:
        name, tail = "td_tiff_zstd_decode_dev", (bufs.lits.data_ptr(), bufs.lits.numel())
    elif verified:
        name, tail = "td_tiff_inflate_verified_dev", (bufs.ends.data_ptr(),)
    else:
        name, tail = "td_tiff_inflate_dev", ()
    _lib.check(getattr(lib, name)(*head, *tail, stream_ptr), name)


def launch_layout(blocks, block_cap, bw, bh, nx, ny, count, predictor, image, width, height, stream_ptr, plane_mask=None):
    """The decoded blocks → ``image`` [height, width, count] (uint8 / uint16 / float32 by its element size), the predictor undone;
    ``plane_mask``: the blocks are the selected planes of a band-separate file, one sample per pixel, interleaved here."""
    name = "td_tiff_" + ("blocks" if plane_mask is None else "planes") + "_to_image" + {1: "", 2: "_u16", 4: "_f32"}[image.element_size()] + "_dev"
    mask = () if plane_mask is None else (plane_mask,)
    _lib.check(getattr(_lib.load(), name)(blocks.data_ptr(), block_cap, bw, bh, nx, ny, count, *mask, predictor, image.data_ptr(), width, height,
                                          stream_ptr), name)


def finish(image, k0, k1, copies, keep, verdict, compressed_bytes, **attrs):
    """The end of every device path, on the current stream: the ``done`` event, the device tensors ``copies`` on their way to pinned
    memory, a blocking event behind them → ``check``. ``check()`` waits, sets ``kernel_ms`` (``k0`` to ``k1``, where given), lets go of
    ``keep`` (what the kernels read), calls ``verdict(check, host arrays...)``, which raises ValueError for a bad block and may set
    attributes, and returns ``image``. ``check`` carries ``.event`` (done), ``.compressed_bytes`` and ``attrs`` from the start."""
    import torch
    done = torch.cuda.Event(blocking=not copies)
    done.record()
    hosts = [torch.empty(src.shape, dtype=src.dtype, pin_memory=True) for src in copies]
    for host, src in zip(hosts, copies):
        host.copy_(src, non_blocking=True)
    copied = done
    if copies:
        copied = torch.cuda.Event(blocking=True)
        copied.record()

    def check():
        copied.synchronize()
        if k0 is not None:
            check.kernel_ms = k0.elapsed_time(k1)
        keep.clear()
        if verdict is not None:
            verdict(check, *(h.numpy() for h in hosts))
        return image
    check.event = done
    check.compressed_bytes = compressed_bytes
    for name, value in attrs.items():
        setattr(check, name, value)
    return check

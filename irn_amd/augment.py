"""Host side of irn_amd/csrc/augment.hip: the training steps' input batches built on the GPU (resize, normalise, mirror,
crop; the IR label map alongside), and the descriptor and tap tables the two kernels take.  `irn_amd.ops` re-exports the
functions.  Host or GPU images in, GPU tensors out; no CPU fallback."""
import collections
import ctypes as C

import numpy as np
import torch

from ._host import cached
from ._lib import _stream, check, lib
from .msf import _lut, _plan

AUGMENT_DESC_WORDS = 16               # IRN_AUGMENT_DESC_WORDS
AUGMENT_LABEL_DESC_WORDS = 12         # IRN_AUGMENT_LABEL_DESC_WORDS
AugmentTables = collections.namedtuple("AugmentTables", "meta src_offsets pixels_bytes scratch_bytes")
LabelTables = collections.namedtuple("LabelTables", "meta src_offsets labels_bytes")
_NEAREST = {}             # (in_size, out_size) -> nearest_plan of that pair
_AUG_STAGED = {}          # device -> event behind the last upload out of the page-locked staging buffers


def nearest_plan(in_size, out_size):
    """Host-only: the source index Pillow's NEAREST reads for every cell of one axis resized in_size -> out_size, int32
    [out_size] (read-only, kept per size pair like `_plan`).  Pillow walks the axis in doubles: it starts at
    0.5 * in / out, adds in / out once per output cell and truncates each position — the running sum, not the textbook
    floor((x + 0.5) * in / out), which rounds differently in about one size pair out of five."""
    key = (int(in_size), int(out_size))
    tab = _NEAREST.get(key)
    if tab is None:
        if key[0] < 1 or key[1] < 1:
            raise ValueError("nearest_plan: sizes must be >= 1 (got %d -> %d)" % key)
        a = key[0] / key[1]
        steps = np.full(key[1], a, np.float64)
        steps[0] = 0.5 * a
        tab = np.cumsum(steps).astype(np.int64).astype(np.int32)           # (sequential double additions, as Pillow's loop)
        tab.setflags(write=False)
        if len(_NEAREST) >= 8192:
            _NEAREST.clear()
        _NEAREST[key] = tab
    return tab


def _draws(who, i, size, draw, crop):
    """Image i's `size` = (h, w) and draws (hs, ws, flip, box) as ints, the box checked against the resized image and the
    crop: -> (h, w, hs, ws, flip, c_top, c_left, i_top, i_left, rows, cols)."""
    (h, w), (hs, ws, flip, box) = size, draw
    h, w, hs, ws = int(h), int(w), int(hs), int(ws)
    c_top, c_left, i_top, i_left, rows, cols = (int(v) for v in box)
    if (min(h, w, hs, ws, rows, cols) < 1 or min(c_top, c_left, i_top, i_left) < 0 or i_top + rows > hs or i_left + cols > ws
            or c_top + rows > crop or c_left + cols > crop):
        raise ValueError("%s: image %d: box %s does not fit a %dx%d image in a %d^2 crop" % (who, i, tuple(box), hs, ws, crop))
    return h, w, hs, ws, flip, c_top, c_left, i_top, i_left, rows, cols


def _columns(ws, flip, i_left, cols):
    """The resized image's column behind every column of the box: i_left + j, or ws - 1 - (i_left + j) when mirrored."""
    xs = np.arange(i_left, i_left + cols)
    return ws - 1 - xs if flip else xs


def _meta(desc, tabs):
    return np.concatenate([desc.reshape(-1)] + tabs).astype(np.int32, copy=False) if len(desc) else np.zeros(0, np.int32)


def augment_tables(sizes, params, crop):
    """Host-only: the descriptors and tap tables `irn_augment_batch` takes (include/irn_hip.h), for images of `sizes[i]` =
    (h, w) and the draws `params[i]` = (hs, ws, flip, box): the image resized to hs x ws (`rescale_size`), mirrored when
    `flip`, then `box` = (c_top, c_left, i_top, i_left, rows, cols) of `imutils._crop_box` applied to that.  The X table of
    an image holds, for column j of its box, the full-axis plan row of resized column i_left + j (ws - 1 - (i_left + j) when
    mirrored); the Y table the rows i_top .. i_top + rows - 1 with `lo` counted from r0, the first source row any of them
    reads.  -> AugmentTables(meta int32 [words], byte offset of every image in the packed pixel buffer, its size, the
    scratch size)."""
    n = len(sizes)
    crop = int(crop)
    desc = np.zeros((n, AUGMENT_DESC_WORDS), np.int32)
    tabs, src_offsets = [], []
    word, src, mid = n * AUGMENT_DESC_WORDS, 0, 0
    for i, (size, draw) in enumerate(zip(sizes, params)):
        h, w, hs, ws, flip, c_top, c_left, i_top, i_left, rows, cols = _draws("augment_tables", i, size, draw, crop)
        xlo, xcnt, xk = _plan(w, ws)
        ylo, ycnt, yk = _plan(h, hs)
        xs = _columns(ws, flip, i_left, cols)
        ys = np.arange(i_top, i_top + rows)
        r0 = int(ylo[ys].min())
        r1 = int((ylo[ys] + ycnt[ys]).max())
        xt = np.concatenate([xlo[xs], xcnt[xs], xk[xs].reshape(-1)])
        yt = np.concatenate([ylo[ys] - r0, ycnt[ys], yk[ys].reshape(-1)])
        desc[i, :14] = (h, w, c_top, c_left, rows, cols, r0, r1 - r0, xk.shape[1], yk.shape[1], src, mid, word, word + xt.size)
        tabs += [xt, yt]
        src_offsets.append(src)
        word += xt.size + yt.size
        src += h * w * 3
        mid += (r1 - r0) * cols * 3
    if max(src, mid, word) >= 2 ** 31:
        raise ValueError("augment_tables: the batch's pixels, intermediates or tables exceed 2^31 - 1")
    return AugmentTables(_meta(desc, tabs), src_offsets, src, mid)


def augment_label_tables(sizes, params, crop, reduce):
    """Host-only: the descriptors and index tables `irn_augment_label_batch` takes (include/irn_hip.h), for label maps of
    `sizes[i]` = (h, w) and the draws `params[i]` = (hs, ws, flip, box) as `augment_tables` takes them: the row table of an
    image holds `nearest_plan(h, hs)` for the rows i_top .. i_top + rows - 1 of its box, the column table
    `nearest_plan(w, ws)` for the columns i_left + j (ws - 1 - (i_left + j) when mirrored).  -> LabelTables(meta int32
    [words], byte offset of every map in the packed label buffer, its size)."""
    n = len(sizes)
    crop, reduce = int(crop), int(reduce)
    if reduce < 1 or crop % reduce:
        raise ValueError("augment_label_tables: reduce %d does not divide the crop %d" % (reduce, crop))
    desc = np.zeros((n, AUGMENT_LABEL_DESC_WORDS), np.int32)
    tabs, src_offsets = [], []
    word, src = n * AUGMENT_LABEL_DESC_WORDS, 0
    for i, (size, draw) in enumerate(zip(sizes, params)):
        h, w, hs, ws, flip, c_top, c_left, i_top, i_left, rows, cols = _draws("augment_label_tables", i, size, draw, crop)
        rt = nearest_plan(h, hs)[i_top:i_top + rows]
        ct = nearest_plan(w, ws)[_columns(ws, flip, i_left, cols)]
        desc[i, :9] = (h, w, c_top, c_left, rows, cols, src, word, word + rows)
        tabs += [rt, ct]
        src_offsets.append(src)
        word += rows + cols
        src += h * w
    if max(src, word) >= 2 ** 31:
        raise ValueError("augment_label_tables: the batch's labels or tables exceed 2^31 - 1")
    return LabelTables(_meta(desc, tabs), src_offsets, src)


def _augment_device(images, device):
    if device is None:
        on_dev = [im.device for im in images if im.is_cuda]
        device = on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _need_images(who, images):
    for im in images:
        if not (isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3):
            raise ValueError("%s: uint8 [H,W,3] images expected" % who)


def _out_tensor(who, name, out, shape, dtype, dev):
    """`out`, checked to be a contiguous tensor of that shape, dtype and device; a new one when it is None."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if not (isinstance(out, torch.Tensor) and out.dtype == dtype and out.device == dev and out.is_contiguous()
            and tuple(out.shape) == tuple(shape)):
        raise ValueError("%s: %s must be a contiguous %s [%s] tensor on %s"
                         % (who, name, {torch.float32: "fp32", torch.uint8: "uint8"}[dtype], ",".join("%d" % s for s in shape), dev))
    return out


def _augment(images, labels, params, crop, reduce, mean, std, dev, out, out_label):
    """The body of `augment_batch` (labels None) and `augment_pair_batch`: the label maps ride behind the pixels in the
    same page-locked staging buffer and the same upload, their tables behind the image tables in the same meta buffer."""
    n = len(images)
    t = augment_tables([im.shape[:2] for im in images], params, crop)
    words = int(t.meta.size)
    lt = augment_label_tables([lb.shape for lb in labels], params, crop, reduce) if labels is not None else None
    lwords = int(lt.meta.size) if lt else 0
    lbytes = lt.labels_bytes if lt else 0
    if t.pixels_bytes + lbytes >= 2 ** 31:
        raise ValueError("augment: the batch's packed pixels and label maps exceed 2^31 - 1 bytes")
    sources = list(zip(images, t.src_offsets))
    if lt:
        sources += [(lb, t.pixels_bytes + off) for lb, off in zip(labels, lt.src_offsets)]
    with torch.cuda.device(dev):
        lut = _lut(mean, std, dev)
        pixels = torch.empty(t.pixels_bytes + lbytes, dtype=torch.uint8, device=dev)
        scratch = torch.empty(max(t.scratch_bytes, 1), dtype=torch.uint8, device=dev)
        meta_dev = torch.empty(words + lwords, dtype=torch.int32, device=dev)
        staged = _AUG_STAGED.get(str(dev))
        if staged is not None:
            staged.synchronize()                     # the staging buffers are free again once the last call's copies have run
        meta_host = cached("aug_meta", "pinned", words + lwords, torch.int32)
        meta_host[:words].copy_(torch.from_numpy(t.meta))
        if lt:
            meta_host[words:words + lwords].copy_(torch.from_numpy(lt.meta))
        if all(not src.is_cuda for src, _ in sources):
            stage = cached("aug_pixels", "pinned", pixels.numel(), torch.uint8)
            for src, off in sources:
                stage[off:off + src.numel()].copy_(src.reshape(-1))
            pixels.copy_(stage[:pixels.numel()], non_blocking=True)
        else:
            for src, off in sources:
                pixels[off:off + src.numel()].copy_(src.reshape(-1), non_blocking=True)
        meta_p = C.cast(meta_host.data_ptr(), C.POINTER(C.c_int32))
        check(lib.irn_augment_batch(n, crop, meta_p, words, pixels.data_ptr(), t.pixels_bytes, lut.data_ptr(), out.data_ptr(),
                                    out.numel(), scratch.data_ptr(), scratch.numel(), meta_dev.data_ptr(), words, _stream()))
        if lt:
            lmeta_p = C.cast(meta_host.data_ptr() + 4 * words, C.POINTER(C.c_int32))
            check(lib.irn_augment_label_batch(n, crop, reduce, lmeta_p, lwords, pixels.data_ptr() + t.pixels_bytes, lbytes,
                                              out_label.data_ptr(), out_label.numel(), meta_dev.data_ptr() + 4 * words, lwords,
                                              _stream()))
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        _AUG_STAGED[str(dev)] = done


def augment_batch(images, params, crop, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None, out=None):
    """The CAM training step's input batch on the GPU (irn_augment_batch): `images` is a list of uint8 [H,W,3] tensors (on the
    host or the device, ragged), `params[i]` = (hs, ws, flip, box) the draws of image i as `augment_tables` takes them ->
    GPU fp32 [B,3,crop,crop], bit-identical to resize (PIL bicubic) -> TorchvisionNormalize -> fliplr -> box into zeros -> CHW
    per image.  Two launches per batch; host images are packed into one page-locked buffer that is reused across calls and
    cross in one non-blocking copy, the descriptors and tables in a second one.  `out`: a contiguous fp32 [B,3,crop,crop]
    GPU tensor to write into (every cell is written)."""
    n = len(images)
    _need_images("augment_batch", images)
    dev = _augment_device(images, device)
    crop = int(crop)
    out = _out_tensor("augment_batch", "out", out, (n, 3, crop, crop), torch.float32, dev)
    if n:
        _augment(images, None, params, crop, 1, mean, std, dev, out, None)
    return out


def augment_pair_batch(images, labels, params, crop, reduce=4, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), device=None,
                       out=None, out_label=None):
    """The IRNet training step's (image, label) batch on the GPU: `images` as `augment_batch` takes them, `labels[i]` the uint8
    [H,W] IR label map of image i (same size), `params[i]` = (hs, ws, flip, box) the one set of draws both halves share ->
    (GPU fp32 [B,3,crop,crop], GPU uint8 [B,crop/reduce,crop/reduce]).  The image half is `augment_batch`; the label half
    (irn_augment_label_batch, one more launch) is bit-identical to Pillow NEAREST resize to hs x ws -> fliplr -> box into a
    container of 255 -> pil_rescale(label, 1 / reduce, 0) (voc12/dataloader.py:251-267 with reduce 4; reduce 1 is the whole
    cropped label).  Host pixels and labels cross in ONE upload out of the page-locked staging buffer.  `out` / `out_label`:
    contiguous GPU tensors of those shapes to write into (every cell is written)."""
    n = len(images)
    crop, reduce = int(crop), int(reduce)
    if reduce < 1 or crop % reduce:
        raise ValueError("augment_pair_batch: reduce %d does not divide the crop %d" % (reduce, crop))
    if len(labels) != n or len(params) != n:
        raise ValueError("augment_pair_batch: %d images, %d labels, %d draws" % (n, len(labels), len(params)))
    _need_images("augment_pair_batch", images)
    for im, lb in zip(images, labels):
        if not (isinstance(lb, torch.Tensor) and lb.dtype == torch.uint8 and lb.dim() == 2):
            raise ValueError("augment_pair_batch: uint8 [H,W] label maps expected")
        if tuple(lb.shape) != tuple(im.shape[:2]):
            raise ValueError("augment_pair_batch: a %dx%d label map for a %dx%d image" % (tuple(lb.shape) + tuple(im.shape[:2])))
    dev = _augment_device(images, device)
    grid = crop // reduce
    out = _out_tensor("augment_pair_batch", "out", out, (n, 3, crop, crop), torch.float32, dev)
    out_label = _out_tensor("augment_pair_batch", "out_label", out_label, (n, grid, grid), torch.uint8, dev)
    if n:
        _augment(images, labels, params, crop, reduce, mean, std, dev, out, out_label)
    return out, out_label

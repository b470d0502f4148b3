"""Host side of irn_amd/csrc/cocomask.hip: COCO mask encoding (step/make_cocoann.py) over include/irn_hip.h's
irn_mask_rle_count / _emit and irn_mask_polygon_edges / _count / _emit.  The run lengths come from the GPU; pycocotools'
string form of them (rleToString / rleFrString) is a few thousand counts per image and is made on the host, vectorised
over the counts of a mask.  The polygons (the mask's boundary along pixel edges) are traced on the GPU; `polygon_fill` is
their inverse on the host.  `irn_amd.ops` re-exports the functions."""
import numpy as np
import torch

from ._host import cached, read_back
from ._lib import _need_cuda, _stream, check, lib


def mask_rle(masks):
    """pycocotools' rleEncode + rleArea + rleToBbox for masks bool / uint8 [N,H,W] on the GPU (nonzero = in the mask).

    Returns numpy arrays on the host: counts uint32 [total] (the run lengths of every mask in column-major pixel order,
    mask i at counts[offsets[i]:offsets[i+1]], in page-locked memory of their own), offsets int64 [N+1], area int64 [N]
    and bbox int32 [N,4] = [x0, y0, width, height].  Two synchronisations: one for the run counts (with area and bbox in
    the same transfer), one for the packed counts."""
    _need_cuda(masks, "masks")
    if not (masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool)):
        raise ValueError("mask_rle: masks must be a bool / uint8 [N,H,W] tensor, got %s %s" % (masks.dtype, tuple(masks.shape)))
    dev = masks.device
    m = (masks.view(torch.uint8) if masks.dtype == torch.bool else masks).contiguous()
    n, h, w = (int(v) for v in m.shape)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros((0, 4), np.int32)
    nbytes = lib.irn_mask_rle_scratch_bytes(n, h, w)
    if nbytes == 0:
        check(1)
    scratch = cached("rle_scratch", dev, nbytes, torch.uint8)
    # one device block for everything the first transfer brings back: area int64 [n] | bbox int32 [n][4] | n_runs int32 [n]
    head = cached("rle_head", dev, 28 * n + 8 * (n + 2), torch.uint8)
    host = cached("rle_head", "pinned", 28 * n + 8 * (n + 2), torch.uint8)
    p_area = head.data_ptr()
    p_bbox, p_runs, p_off = p_area + 8 * n, p_area + 24 * n, p_area + 28 * n + (-28 * n) % 8
    with torch.cuda.device(dev):
        check(lib.irn_mask_rle_count(m.data_ptr(), n, h, w, p_runs, p_area, p_bbox, scratch.data_ptr(), _stream()))
        read_back(head[:28 * n], host, side=False).synchronize()              # host round trip 1
        raw = host[:28 * n].numpy()
        area, bbox = raw[:8 * n].view(np.int64).copy(), raw[8 * n:24 * n].view(np.int32).reshape(n, 4).copy()
        offsets = np.zeros(n + 1, np.int64)
        np.cumsum(raw[24 * n:28 * n].view(np.int32), out=offsets[1:])
        total = int(offsets[n])
        o = p_off - p_area
        host[o:o + 8 * (n + 1)].view(torch.int64).copy_(torch.from_numpy(offsets))
        head[o:o + 8 * (n + 1)].copy_(host[o:o + 8 * (n + 1)], non_blocking=True)
        counts_dev = cached("rle_counts", dev, 4 * total, torch.uint8)
        check(lib.irn_mask_rle_emit(m.data_ptr(), n, h, w, p_off, counts_dev.data_ptr(), scratch.data_ptr(), _stream()))
        # page-locked memory of the call's own: the counts are handed out as a view of it (torch's caching host allocator
        # takes it back when the last view is dropped)
        out = torch.empty(4 * total, dtype=torch.uint8, pin_memory=True)
        read_back(counts_dev[:4 * total], out, side=False).synchronize()      # host round trip 2
    return out.numpy().view(np.uint32), offsets, area, bbox


def rle_to_string(counts):
    """pycocotools' rleToString: the run lengths of one mask as COCO's compressed ASCII string (characters '0'..'o').
    Count i is stored as counts[i] - counts[i-2] for i > 2, in 5-bit groups, least significant first, bit 5 = more follow."""
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    x = c.copy()
    x[3:] -= c[1:-2]
    groups = 7                                             # |x| < 2^32: 33 bits with the sign, 7 groups of 5
    shifted = x[:, None] >> (5 * np.arange(groups + 1, dtype=np.int64))[None, :]       # arithmetic shift
    chunk = shifted[:, :groups] & 31
    rest = shifted[:, 1:]
    more = np.where(chunk & 16, rest != -1, rest != 0)
    emitted = np.ones_like(more)
    emitted[:, 1:] = np.logical_and.accumulate(more[:, :-1], axis=1)
    chars = (chunk | (more.astype(np.int64) << 5)) + 48
    return chars[emitted].astype(np.uint8).tobytes().decode("ascii")


def rle_from_string(s):
    """pycocotools' rleFrString: COCO's compressed string (str or bytes) back to the run lengths, uint32."""
    b = np.frombuffer(s.encode("ascii") if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64) - 48
    if b.size == 0:
        return np.zeros(0, np.uint32)
    if ((b < 0) | (b > 63)).any() or b[-1] & 32:
        raise ValueError("rle_from_string: not a COCO run-length string")
    last = (b & 32) == 0                                   # the last group of every count
    start = np.flatnonzero(np.concatenate([[True], last[:-1]]))
    k = np.arange(b.size) - np.repeat(start, np.diff(np.append(start, b.size)))       # group number within its count
    x = np.add.reduceat((b & 31) << (5 * k), start)
    ends = np.flatnonzero(last)
    neg = (b[ends] & 16) != 0
    x[neg] |= np.int64(-1) << (5 * (k[ends][neg] + 1))    # sign extension
    x[2::2] = np.cumsum(x[2::2])                           # counts[i] = x[i] + counts[i-2] for i > 2
    x[1::2] = np.cumsum(x[1::2])
    if (x < 0).any() or (x > 0xffffffff).any():
        raise ValueError("rle_from_string: a run length outside 0..2^32-1")
    return x.astype(np.uint32)


def rle_decode(counts, h, w):
    """The mask of pycocotools' rleDecode: bool [h,w] from the run lengths of its column-major pixel order."""
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    if (c < 0).any() or int(c.sum()) != h * w:
        raise ValueError("rle_decode: the counts sum to %d, the mask has %d pixels" % (int(c.sum()), h * w))
    bits = np.repeat(np.arange(c.size) & 1, c).astype(bool)
    return np.ascontiguousarray(bits.reshape(w, h).T)


def mask_polygons(masks):
    """The boundary of masks bool / uint8 [N,H,W] on the GPU (nonzero = in the mask) along pixel edges, as closed integer
    loops (include/irn_hip.h "COCO mask polygons"): vertex (x, y) is the top-left corner of pixel (x, y), the mask lies on
    the right of every edge, and where two mask pixels touch only diagonally the loops keep them apart (4-connectivity).

    Returns numpy arrays on the host: xy int32 [V,2], the corners of every outer loop (no vertex repeated at the end, each
    loop from its smallest vertex in (y, x) order, leaving it in +x); loop_offsets int64 [L+1] (loop k is
    xy[loop_offsets[k]:loop_offsets[k+1]]); mask_loops int64 [N+1] (mask i owns loops mask_loops[i]:mask_loops[i+1], in the
    (y, x) order of their start vertices); holes int64 [N], the hole loops of every mask: counted, not emitted, since COCO
    readers take the union of a segmentation's polygons.  Three synchronisations: the edge counts, the loop and corner
    counts, the corners."""
    _need_cuda(masks, "masks")
    if not (masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool)):
        raise ValueError("mask_polygons: masks must be a bool / uint8 [N,H,W] tensor, got %s %s" % (masks.dtype, tuple(masks.shape)))
    dev = masks.device
    m = (masks.view(torch.uint8) if masks.dtype == torch.bool else masks).contiguous()
    n, h, w = (int(v) for v in m.shape)
    empty = (np.zeros((0, 2), np.int32), np.zeros(1, np.int64), np.zeros(n + 1, np.int64), np.zeros(n, np.int64))
    if n == 0:
        return empty
    nbytes = lib.irn_mask_polygon_scratch_bytes(n, h, w)
    if nbytes == 0:
        check(1)
    scratch = cached("poly_scratch", dev, nbytes, torch.uint8)
    # one device block for both small transfers: edge_offsets int32 [n+1] | n_loops | n_holes | n_vertices int32 [n] each
    head = cached("poly_head", dev, 4 * n + 1, torch.int32)
    host = cached("poly_head", "pinned", 4 * n + 1, torch.int32)
    p_off = head.data_ptr()
    p_loops, p_holes, p_verts = (p_off + 4 * (n + 1) + 4 * n * k for k in range(3))
    with torch.cuda.device(dev):
        check(lib.irn_mask_polygon_edges(m.data_ptr(), n, h, w, p_off, scratch.data_ptr(), _stream()))
        read_back(head[:n + 1], host, side=False).synchronize()                # host round trip 1
        edge_offsets = host[:n + 1].numpy().astype(np.int64)
        n_edges, longest = int(edge_offsets[n]), int(np.diff(edge_offsets).max())
        if n_edges == 0:
            return empty
        trace = cached("poly_trace", dev, lib.irn_mask_polygon_trace_scratch_bytes(n_edges), torch.uint8)
        check(lib.irn_mask_polygon_count(m.data_ptr(), n, h, w, p_off, n_edges, longest, p_loops, p_holes, p_verts,
                                         scratch.data_ptr(), trace.data_ptr(), _stream()))
        read_back(head[n + 1:4 * n + 1], host, side=False).synchronize()       # host round trip 2
        counts = host[:3 * n].numpy().astype(np.int64).reshape(3, n)
        mask_loops = np.zeros(n + 1, np.int64)
        np.cumsum(counts[0], out=mask_loops[1:])
        holes = counts[1].copy()
        n_loops, n_verts = int(mask_loops[n]), int(counts[2].sum())
        out_dev = cached("poly_out", dev, n_loops + 2 * n_verts, torch.int32)
        check(lib.irn_mask_polygon_emit(n_edges, out_dev.data_ptr(), n_loops, out_dev.data_ptr() + 4 * n_loops, n_verts,
                                        trace.data_ptr(), _stream()))
        out = torch.empty(n_loops + 2 * n_verts, dtype=torch.int32, pin_memory=True)   # the call's own, as in mask_rle
        read_back(out_dev[:n_loops + 2 * n_verts], out, side=False).synchronize()      # host round trip 3
    raw = out.numpy()
    loop_offsets = np.zeros(n_loops + 1, np.int64)
    np.cumsum(raw[:n_loops], out=loop_offsets[1:])
    return raw[n_loops:].reshape(n_verts, 2), loop_offsets, mask_loops, holes


def polygon_fill(xy, loop_offsets, h, w):
    """The inverse of `mask_polygons` for one mask: bool [h,w], the union of the loops' fills.  Pixel (x, y) is inside a
    loop iff an odd number of the loop's vertical edges at columns <= x span row y (its centre is sampled).  The union of a
    mask's outer loops is the mask with its holes filled."""
    xy = np.asarray(xy).astype(np.int64).reshape(-1, 2)
    off = np.asarray(loop_offsets).astype(np.int64).reshape(-1)
    if off.size < 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(xy):
        raise ValueError("polygon_fill: loop_offsets do not partition the %d vertices" % len(xy))
    if len(xy) and (xy.min() < 0 or xy[:, 0].max() > w or xy[:, 1].max() > h):
        raise ValueError("polygon_fill: a vertex outside the %dx%d (height x width) image" % (h, w))
    out = np.zeros((h, w), bool)
    for a, b in zip(off[:-1], off[1:]):
        if b - a < 3:
            continue
        x, y = xy[a:b, 0], xy[a:b, 1]
        x0, y0 = int(x.min()), int(y.min())
        nx, ny = np.roll(x, -1), np.roll(y, -1)
        ver = (x == nx) & (y != ny)                        # a vertical edge toggles, at its column, the rows it spans
        rows, cols = int(y.max()) - y0, int(x.max()) - x0
        ends = np.zeros((rows + 1, cols + 1), np.int64)
        np.add.at(ends, (y[ver] - y0, x[ver] - x0), 1)
        np.add.at(ends, (ny[ver] - y0, x[ver] - x0), 1)
        toggles = np.cumsum(ends, axis=0) & 1              # parity along y: the rows between an edge's two ends
        inside = (np.cumsum(toggles, axis=1) & 1).astype(bool)
        out[y0:y0 + rows, x0:x0 + cols] |= inside[:rows, :cols]
    return out

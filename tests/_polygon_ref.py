"""Plain-loop restatement of the polygon definition of include/irn_hip.h "COCO mask polygons" (irn_amd.ops.mask_polygons):
the boundary of a binary mask along pixel edges as closed integer loops.  Test infrastructure; nothing here is shared with
irn_amd/cocomask.py or the kernels.

Vertex (x, y) is the top-left corner of pixel (x, y).  Every side of a mask pixel whose neighbour across it is not in the
mask is a directed unit edge with the mask on its right: top +x, right +y, bottom -x, left -y.  At an edge's head vertex the
successor is the right turn if that edge exists, else straight on, else the left turn.  The cycles of the successor map are
the loops; the shoelace sum is positive for an outer loop and negative for a hole.  A loop is its corners, from the tail of
its lowest-numbered edge, +x edges numbered y*w + x before all others."""
import numpy as np

DIRS = ((1, 0), (0, 1), (-1, 0), (0, -1))                  # +x, +y, -x, -y: a right turn is the next one (y points down)


def _set(mask, x, y):
    h, w = mask.shape
    return 0 <= x < w and 0 <= y < h and bool(mask[y, x])


def edge_set(mask):
    """{(tail x, tail y, direction)} of a [h,w] mask (nonzero = set)."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    edges = set()
    for y in range(h):
        for x in range(w):
            if not mask[y, x]:
                continue
            if not _set(mask, x, y - 1):
                edges.add((x, y, 0))                       # top side, +x
            if not _set(mask, x + 1, y):
                edges.add((x + 1, y, 1))                   # right side, +y
            if not _set(mask, x, y + 1):
                edges.add((x + 1, y + 1, 2))               # bottom side, -x
            if not _set(mask, x - 1, y):
                edges.add((x, y + 1, 3))                   # left side, -y
    return edges


def successor(edge, edges):
    x, y, d = edge
    hx, hy = x + DIRS[d][0], y + DIRS[d][1]
    for nd in ((d + 1) % 4, d, (d + 3) % 4):               # right, straight, left
        if (hx, hy, nd) in edges:
            return (hx, hy, nd)
    raise AssertionError("edge %r has no successor" % (edge,))


def _number(edge, w):
    x, y, d = edge
    return (0, y * w + x) if d == 0 else (1, d, y, x)


def all_loops(mask):
    """Every loop of the mask, holes included: [(corners [(x, y), ...], doubled signed area, unit edges)] in the order of
    their lowest-numbered edges, each from the tail of that edge."""
    mask = np.asarray(mask) != 0
    w = mask.shape[1]
    edges = edge_set(mask)
    seen, loops = set(), []
    for first in sorted(edges, key=lambda e: _number(e, w)):
        if first in seen:
            continue
        assert first[2] == 0                               # every loop has a +x edge, and they are numbered first
        walk, e = [], first
        while e not in seen:                               # the successor map is a permutation: the walk returns to `first`
            seen.add(e)
            walk.append(e)
            e = successor(e, edges)
        assert e == first
        area2 = 0
        for x, y, d in walk:
            x1, y1 = x + DIRS[d][0], y + DIRS[d][1]
            area2 += x * y1 - x1 * y
        corners = [(x, y) for i, (x, y, d) in enumerate(walk) if walk[i - 1][2] != d]
        loops.append((corners, area2, len(walk)))
    return loops


def outer_loops(mask):
    return [corners for corners, area2, _ in all_loops(mask) if area2 > 0]


def mask_polygons(masks):
    """What irn_amd.ops.mask_polygons returns, from the restatement: (xy, loop_offsets, mask_loops, holes)."""
    masks = np.asarray(masks)
    xy, sizes, per_mask, holes = [], [], [], []
    for m in masks:
        loops = all_loops(m)
        outer = [c for c, a, _ in loops if a > 0]
        per_mask.append(len(outer))
        holes.append(sum(1 for _, a, _ in loops if a < 0))
        for c in outer:
            sizes.append(len(c))
            xy += c
    loop_offsets = np.zeros(len(sizes) + 1, np.int64)
    loop_offsets[1:] = np.cumsum(sizes) if sizes else []
    mask_loops = np.zeros(len(masks) + 1, np.int64)
    mask_loops[1:] = np.cumsum(per_mask) if per_mask else []
    return (np.asarray(xy, np.int32).reshape(-1, 2), loop_offsets, mask_loops, np.asarray(holes, np.int64).reshape(len(masks)))


def loop_fill(corners, h, w):
    """Pixel-centre fill of one loop, pixel by pixel: (x, y) is inside iff an odd number of the loop's vertical edges at
    columns <= x span row y."""
    out = np.zeros((h, w), bool)
    n = len(corners)
    vertical = []
    for i in range(n):
        (x0, y0), (x1, y1) = corners[i], corners[(i + 1) % n]
        if x0 == x1 and y0 != y1:
            vertical.append((x0, min(y0, y1), max(y0, y1)))
    for y in range(h):
        for x in range(w):
            out[y, x] = sum(1 for c, ya, yb in vertical if c <= x and ya <= y < yb) % 2 == 1
    return out


def _flood(mask, seeds, neighbours):
    h, w = mask.shape
    seen = np.zeros((h, w), bool)
    stack = [s for s in seeds if mask[s[1], s[0]]]
    for x, y in stack:
        seen[y, x] = True
    while stack:
        x, y = stack.pop()
        for dx, dy in neighbours:
            u, v = x + dx, y + dy
            if 0 <= u < w and 0 <= v < h and mask[v, u] and not seen[v, u]:
                seen[v, u] = True
                stack.append((u, v))
    return seen


N4 = ((1, 0), (0, 1), (-1, 0), (0, -1))
N8 = N4 + ((1, 1), (1, -1), (-1, 1), (-1, -1))


def _regions(mask, neighbours):
    mask = np.asarray(mask) != 0
    left, regions = mask.copy(), []
    for y, x in zip(*np.nonzero(mask)):
        if left[y, x]:
            r = _flood(left, [(int(x), int(y))], neighbours)
            regions.append(r)
            left &= ~r
    return regions


def components4(mask):
    """The number of 4-connected components of the mask."""
    return len(_regions(mask, N4))


def enclosed_background(mask):
    """The 8-connected background regions that do not reach the border: (their number, their union)."""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    bg = ~mask
    border = [(x, y) for x in range(w) for y in (0, h - 1)] + [(x, y) for y in range(h) for x in (0, w - 1)]
    inner = bg & ~_flood(bg, border, N8)
    return len(_regions(inner, N8)), inner


def fill_holes(mask):
    """The mask with its holes filled."""
    return (np.asarray(mask) != 0) | enclosed_background(mask)[1]


# hand cases shared by the CPU and the GPU tests
def hand_cases():
    ring = np.ones((3, 3), bool)
    ring[1, 1] = False
    pinch = np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0]], bool)
    u = np.array([[1, 0, 0, 1], [1, 0, 0, 1], [1, 1, 1, 1]], bool)
    plus = np.zeros((5, 5), bool)
    plus[2, :] = plus[:, 2] = True
    stairs = np.tril(np.ones((6, 6), bool))
    nested = np.ones((7, 7), bool)
    nested[1:6, 1:6] = False
    nested[3, 3] = True                                    # a component inside the ring's hole
    nested2 = np.zeros((9, 11), bool)
    nested2[1:8, 1:10] = True
    nested2[2:7, 2:9] = False
    nested2[3:6, 4:7] = True
    nested2[4, 5] = False                                  # ... with a hole of its own
    return {"one_set": np.ones((1, 1), bool), "one_clear": np.zeros((1, 1), bool),
            "diagonal": np.eye(2, dtype=bool), "anti_diagonal": np.eye(2, dtype=bool)[::-1].copy(),
            "ring": ring, "pinch": pinch, "u": u, "plus": plus, "stairs": stairs, "nested": nested, "nested2": nested2,
            "row_runs": np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1]], bool), "column_runs": np.array([[1, 0, 1, 1, 0, 1]], bool).T.copy()}


def serpentine(h, w):
    """One 4-connected snake: every other row full, joined alternately at the right and the left end."""
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m

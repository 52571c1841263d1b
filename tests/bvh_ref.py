"""The device tree builders (raytracing-potato_amd/csrc/rp_bvh_gpu.hip), written out from their definitions in numpy and
plain Python f64: the reference tests/test_gpu_bvh_ref.py compares the device's trees with, bit for bit.

Everything in those kernels is exact to restate: f64 adds, multiplies, min/max and one division (built without
contraction), ties broken by position, a stable radix sort.  One function per stage, each in the kernel's operation
order:

    scene_boxes     hittable_box, the centroids' bounds and the Morton scale     (rp_bvh.cpp prim_input, build_gpu)
    lbvh_keys       morton_kernel: 10-bit cells, key = code << 32 | index
    ploc_keys       morton63_kernel: 21-bit cells, sorted stably with the index as the value
    radix_tree      the binary radix tree over the sorted unique keys, as its recursive definition (NOT Karras' search:
                    karras_tree below is that, kept apart, and tests/test_bvh_ref.py holds the two equal)
    ploc_merges     ploc_nn_kernel / ploc_flags_kernel / ploc_apply_kernel's merges, round by round
    ploc_sah        ploc_apply_kernel's leaf decision and cost, bottom-up
    collapse        collapse_kernel: the opening rule, the slot order, the leaf entries, the primitive order
    dfs_number      dfs_relayout: the root at 0, families consecutive and padded to `align`
    encode          the records: Node4 (f32_rd / f32_ru) or Node4Q (qframe, q_down, q_up restated)

Rules holds the eight deliberate mistakes of the sensitivity test (all off by default): what a subtly wrong builder
would do.  NaN geometry is out of scope: numpy's minimum/maximum do not state fmin/fmax on NaN.
"""
from __future__ import annotations

import bisect
import math
from dataclasses import dataclass

import numpy as np

from rtpotato import _ffi as F

BIN_LEAF = 0x80000000
ENTRY_LEAF = 0x80000000
ENTRY_EMPTY = 0xFFFFFFFF
LEAF_SHIFT = 28
LEAF_FIRST_MASK = (1 << LEAF_SHIFT) - 1
PLOC_R = 3
PLOC_B = 256
DEF_MAX_LEAF = 4
DEF_COST_TRAVERSE = 0.7
INF = math.inf


@dataclass(frozen=True)
class Rules:
    """The builders' rules; every default is the device's.  Each other value is one deliberate mistake."""
    radius: int = PLOC_R          # mistake: 2
    seam: int = 0                 # mistake: 256 -- no neighbour across a multiple of 256 positions (a lost LDS halo)
    tie_larger: bool = False      # mistake: equal distances take the larger j
    sah_leaf: bool = True         # mistake: False -- a leaf whenever size <= max_leaf
    open_first: bool = False      # mistake: the collapse opens the first openable child, not the largest
    ploc_bits: int = 21           # mistake: 20 bits per axis
    swap_xz: bool = False         # mistake: Morton x and z swapped
    pad_families: bool = True     # mistake: False -- families not padded under dfs_line


DEVICE = Rules()
MISTAKES = {
    "radius_2": Rules(radius=2),
    "seam_256": Rules(seam=PLOC_B),
    "tie_larger_j": Rules(tie_larger=True),
    "no_sah_leaf": Rules(sah_leaf=False),
    "open_first": Rules(open_first=True),
    "ploc_20_bits": Rules(ploc_bits=20),
    "swap_xz": Rules(swap_xz=True),
    "unpadded_families": Rules(pad_families=False),
}


# ---------------------------------------------------------------------------------------------------------------
# input

@dataclass
class Boxes:
    lo: np.ndarray     # (n, 3) f64
    hi: np.ndarray
    cmin: np.ndarray   # (3,) bounds of the centroids
    scale: np.ndarray  # (3,) ext > 0 ? 1024 / ext : 0


def scene_boxes(scene) -> Boxes:
    """hittable_box per hittable (sphere c -+ r; triangle min/max of its three vertices), the centroids 0.5 (lo + hi),
    their bounds and the Morton scale."""
    root = scene.root
    n = len(root)
    lo, hi = np.empty((n, 3)), np.empty((n, 3))
    sph = root["kind"] == F.RP_HITTABLE_SPHERE
    lo[sph] = root["center"][sph] - root["radius"][sph, None]
    hi[sph] = root["center"][sph] + root["radius"][sph, None]
    for mi, mesh in enumerate(scene.scene_data.mesh_table):
        rows = np.nonzero(~sph & (root["mesh"] == mi))[0]
        if not len(rows):
            continue
        t = root["triangle"][rows].astype(np.int64)
        a, b, c = (mesh.positions[mesh.indices[t + k]] for k in range(3))
        lo[rows] = np.minimum(np.minimum(a, b), c)
        hi[rows] = np.maximum(np.maximum(a, b), c)
    cen = 0.5 * (lo + hi)
    cmin, cmax = cen.min(axis=0), cen.max(axis=0)
    ext = cmax - cmin
    scale = np.where(ext > 0.0, 1024.0 / np.where(ext > 0.0, ext, 1.0), 0.0)
    return Boxes(lo, hi, cmin, scale)


def _spread3(v: int, bits: int) -> int:
    """bit b of v -> bit 3 b (expand_bits10 / expand_bits21, by their meaning)"""
    out = 0
    for b in range(bits):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def _morton(bx: Boxes, mul: float, top: float, bits: int, rules: Rules) -> list:
    cen = 0.5 * (bx.lo + bx.hi)
    q = (cen - bx.cmin) * bx.scale
    if mul != 1.0:
        q = q * mul
    q = np.where(q >= 0.0, np.where(q > top, top, q), 0.0).astype(np.int64)  # clamped, then truncated
    shift = (0, 1, 2) if rules.swap_xz else (2, 1, 0)
    return [sum(_spread3(int(q[i, k]), bits) << shift[k] for k in range(3)) for i in range(len(q))]


def lbvh_keys(bx: Boxes, rules: Rules = DEVICE):
    """-> (sorted keys, order): key = code << 32 | index over 10-bit cells; the keys are unique, order[k] = the
    primitive at sorted position k."""
    keys = sorted((c << 32) | i for i, c in enumerate(_morton(bx, 1.0, 1023.0, 10, rules)))
    return keys, [k & 0xFFFFFFFF for k in keys]


def ploc_keys(bx: Boxes, rules: Rules = DEVICE):
    """-> (codes, order): 63-bit codes ((c - cmin) * scale) * 2048 clamped to [0, 2097151], sorted stably with the
    primitive index as the value."""
    bits = rules.ploc_bits
    codes = _morton(bx, float(1 << (bits - 10)), float((1 << bits) - 1), bits, rules)
    order = sorted(range(len(codes)), key=lambda i: codes[i])  # Python's sort is stable
    return codes, order


# ---------------------------------------------------------------------------------------------------------------
# binary trees

def area(lo, hi) -> float:
    """2 (dx dy + dy dz + dz dx); 0 if an extent is negative or NaN"""
    dx, dy, dz = hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]
    if not (dx >= 0) or not (dy >= 0) or not (dz >= 0):
        return 0.0
    return 2.0 * (dx * dy + dy * dz + dz * dx)


class BinTree:
    """A binary tree over n primitives.  A child reference is BIN_LEAF | x (one primitive: x is a sorted position in
    the LBVH, a primitive in PLOC) or an inner node's id.  What collapse_kernel asks of its Src."""

    def __init__(self, kind, n, leaf_lo, leaf_hi, leaf_src):
        self.kind, self.n = kind, n
        self.leaf_lo, self.leaf_hi = leaf_lo, leaf_hi  # by x
        self.leaf_src = leaf_src                       # by x: the primitive (source hittable)
        self.left, self.right, self.size, self.leaf = [], [], [], []
        self.lo, self.hi = [], []                      # inner nodes' boxes (tuples)
        self.first = []                                # LBVH: first sorted position of the node's range
        self.root = 0

    def add(self, left, right, first=0):
        i = len(self.left)
        self.left.append(left)
        self.right.append(right)
        self.first.append(first)
        self.size.append(self.count(left) + self.count(right))
        (al, ah), (bl, bh) = self.box(left), self.box(right)
        self.lo.append(tuple(min(x, y) for x, y in zip(al, bl)))  # exact unions
        self.hi.append(tuple(max(x, y) for x, y in zip(ah, bh)))
        self.leaf.append(False)
        return i

    def count(self, c):
        return 1 if c & BIN_LEAF else self.size[c]

    def is_leaf(self, c):
        return bool(c & BIN_LEAF) or self.leaf[c]

    def box(self, c):
        if c & BIN_LEAF:
            x = c & ~BIN_LEAF
            return tuple(self.leaf_lo[x].tolist()), tuple(self.leaf_hi[x].tolist())
        return self.lo[c], self.hi[c]

    def prims_below(self, c):
        """the primitives of c's subtree, left first (place_leaf's order; the LBVH's sorted order)"""
        out, stk = [], [c]
        while stk:
            x = stk.pop()
            if x & BIN_LEAF:
                out.append(self.leaf_src[x & ~BIN_LEAF])
            else:
                stk.append(self.right[x])
                stk.append(self.left[x])
        return out


def radix_ranges(keys):
    """The binary radix tree over sorted unique keys, by definition: the range [lo, hi] (more than one key) splits at
    the highest bit in which its keys differ, after the last key whose bit is 0.  -> {(lo, hi): split}."""
    out = {}
    stk = [(0, len(keys) - 1)]
    while stk:
        lo, hi = stk.pop()
        if lo == hi:
            continue
        b = (keys[lo] ^ keys[hi]).bit_length() - 1       # sorted: the range's highest differing bit
        g = bisect.bisect_left(keys, (keys[hi] >> b) << b, lo, hi + 1) - 1  # the last key with bit b clear
        out[(lo, hi)] = g
        stk.append((lo, g))
        stk.append((g + 1, hi))
    return out


def karras_tree(keys):
    """Karras 2012, Fig. 4, as radix_tree_kernel runs it: inner node i of n - 1 finds its direction, its range by a
    doubling then a binary search on the common-prefix length, and its split.  -> {(lo, hi): split}."""
    n = len(keys)

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - (keys[i] ^ keys[j]).bit_length()

    out = {}
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        ln, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (ln + t) * d) > dmin:
                ln += t
            t //= 2
        j = i + ln * d
        dnode = delta(i, j)
        s, div = 0, 2
        while True:
            t = (ln + div - 1) // div
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
            div *= 2
        g = i + s * d + (-1 if d < 0 else 0)
        out[(min(i, j), max(i, j))] = g
    return out


def radix_tree(bx: Boxes, max_leaf: int, rules: Rules = DEVICE) -> BinTree:
    """The LBVH's binary tree: the radix tree of the sorted keys, exact unions for boxes, a subtree of <= max_leaf
    primitives a leaf (RadixSrc::is_leaf)."""
    keys, order = lbvh_keys(bx, rules)
    n = len(keys)
    bt = BinTree("lbvh", n, bx.lo[order], bx.hi[order], order)
    ranges = radix_ranges(keys)

    def ref(lo, hi):
        return BIN_LEAF | lo if lo == hi else build(lo, hi)

    def build(lo, hi):  # children first, so a node's boxes exist when it is added; the root is added last
        g = ranges[(lo, hi)]
        return bt.add(ref(lo, g), ref(g + 1, hi), first=lo)

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    bt.root = build(0, n - 1)
    bt.leaf = [s <= max_leaf for s in bt.size]
    return bt


def _areas(lo, hi):
    d = hi - lo
    ok = (d[:, 0] >= 0) & (d[:, 1] >= 0) & (d[:, 2] >= 0)
    return np.where(ok, 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]), 0.0)


def ploc_nearest(lo, hi, rules: Rules = DEVICE):
    """ploc_nn_kernel: per cluster the position j != i within `radius` of least area(union), scanned in increasing j
    with a strict <; the first candidate if none is finite."""
    m = len(lo)
    i = np.arange(m)
    best = np.full(m, INF)
    bj = np.full(m, -1)
    for off in [o for o in range(-rules.radius, rules.radius + 1) if o]:
        j = i + off
        valid = (j >= 0) & (j < m)
        if rules.seam:
            valid &= (j // rules.seam) == (i // rules.seam)
        jc = np.clip(j, 0, m - 1)
        d = _areas(np.minimum(lo, lo[jc]), np.maximum(hi, hi[jc]))
        d = np.where(np.isnan(d), INF, d)
        take = valid & (((d <= best) if rules.tie_larger else (d < best)) | (bj < 0))
        best = np.where(take, d, best)
        bj = np.where(take, j, bj)
    return bj


def ploc_merges(bx: Boxes, rules: Rules = DEVICE) -> BinTree:
    """PLOC's rounds over the Morton order: mutual nearest neighbours merge at the lower position, the array is
    compacted with its order kept, node ids are node_base + the merge's rank in the round.  n - 1 nodes, the root last.
    The leaf decisions are ploc_sah's: they do not feed back into the merges."""
    _, order = ploc_keys(bx, rules)
    n = len(order)
    bt = BinTree("ploc", n, bx.lo, bx.hi, list(range(n)))
    ref = [BIN_LEAF | p for p in order]
    lo, hi = bx.lo[order].copy(), bx.hi[order].copy()
    while len(ref) > 1:
        m = len(ref)
        nn = ploc_nearest(lo, hi, rules)
        i = np.arange(m)
        mutual = (nn >= 0) & (nn < m) & (nn[np.clip(nn, 0, m - 1)] == i)
        keep = ~mutual | (i < nn)
        merge = mutual & (i < nn)
        assert merge.any(), "no progress"
        ref2, lo2, hi2 = [], [], []
        for p in np.nonzero(keep)[0]:  # increasing position: merge ranks and kept positions are the prefix sums
            if merge[p]:
                node = bt.add(ref[p], ref[nn[p]])
                ref2.append(node)
                lo2.append(bt.lo[node])
                hi2.append(bt.hi[node])
            else:
                ref2.append(ref[p])
                lo2.append(tuple(lo[p].tolist()))
                hi2.append(tuple(hi[p].tolist()))
        ref, lo, hi = ref2, np.array(lo2).reshape(-1, 3), np.array(hi2).reshape(-1, 3)
    assert len(bt.left) == n - 1
    bt.root = n - 2
    return bt


def ploc_sah(bt: BinTree, max_leaf: int, cost_traverse: float, rules: Rules = DEVICE):
    """ploc_apply_kernel's SAH decision per merge, bottom-up (children have smaller ids): sets bt.leaf.
    split = cost_traverse + (area(u) > 0 ? (area(a) cost(a) + area(b) cost(b)) / area(u) : 0.5 (cost(a) + cost(b)));
    leaf = size <= max_leaf and size <= split; the node's cost is its size as a leaf, else split.  -> the costs."""
    cost = []

    def ccost(c):
        return 1.0 if c & BIN_LEAF else cost[c]

    for k in range(len(bt.left)):
        a, b = bt.left[k], bt.right[k]
        au = area(bt.lo[k], bt.hi[k])
        split = cost_traverse + ((area(*bt.box(a)) * ccost(a) + area(*bt.box(b)) * ccost(b)) / au if au > 0.0
                                 else 0.5 * (ccost(a) + ccost(b)))
        sz = bt.size[k]
        leaf = sz <= max_leaf and (float(sz) <= split or not rules.sah_leaf)
        bt.leaf[k] = leaf
        cost.append(float(sz) if leaf else split)
    return cost


# ---------------------------------------------------------------------------------------------------------------
# the wide collapse

class WNode:
    __slots__ = ("slots", "depth", "id", "fam", "below")

    def __init__(self, depth):
        self.slots = []  # (kind, count, first, child, lo, hi): kind "leaf" or "inner"
        self.depth = depth
        self.id = self.fam = self.below = 0

    def inner(self):
        return [s[3] for s in self.slots if s[0] == "inner"]


@dataclass
class Wide:
    root: WNode
    nodes: list      # every wide node, the root first
    perm: list       # the primitive (source hittable) at every leaf-order position
    n_leaves: int
    max_depth: int


def collapse(bt: BinTree, rules: Rules = DEVICE) -> Wide:
    """collapse_kernel: the wide root takes the binary root's two children; a node opens its inner (non-leaf) child of
    largest area -- the first of equals -- until it has four: the left grandchild takes the opened slot, the right one
    the next free slot.  A leaf child's entry is its count and first leaf-order position: its sorted range (LBVH), or
    the running offset of the depth-first walk in slot order (PLOC, which lays perm out as it goes)."""
    nodes, perm = [], [None] * bt.n
    n_leaves = 0
    todo = [(bt.root, 0, WNode(0))]
    root = todo[0][2]
    while todo:
        binid, poff, w = todo.pop()
        nodes.append(w)
        kids = [bt.left[binid], bt.right[binid]]
        while len(kids) < 4:
            best, best_area = -1, -1.0
            for k, c in enumerate(kids):
                if bt.is_leaf(c):
                    continue
                a = area(*bt.box(c))
                if a > best_area:
                    best_area, best = a, k
                if rules.open_first:
                    break
            if best < 0:
                break
            o = kids[best]
            kids[best] = bt.left[o]
            kids.append(bt.right[o])
        off = poff
        for c in kids:
            cnt = bt.count(c)
            lo, hi = bt.box(c)
            if bt.is_leaf(c):
                n_leaves += 1
                below = bt.prims_below(c)
                if bt.kind == "lbvh":
                    first = (c & ~BIN_LEAF) if c & BIN_LEAF else bt.first[c]
                else:
                    first = off
                perm[first:first + cnt] = below
                w.slots.append(("leaf", cnt, first, None, lo, hi))
            else:
                ch = WNode(w.depth + 1)
                w.slots.append(("inner", cnt, 0, ch, lo, hi))
                todo.append((c, off, ch))
            off += cnt
    assert None not in perm
    return Wide(root, nodes, perm, n_leaves, max(w.depth for w in nodes))


def dfs_number(wide: Wide, align: int = 1, rules: Rules = DEVICE) -> int:
    """dfs_relayout: the root is node 0 (padded to `align`), then its family; a node's inner children are one
    consecutive family padded to `align`, and each child's subtree -- its family first -- follows in child order.
    Sets every node's id.  -> the number of records, pads included."""
    if not rules.pad_families:
        align = 1

    def pad(m):
        return (m + align - 1) // align * align

    for w in sorted(wide.nodes, key=lambda w: -w.depth):  # bottom-up
        kids = w.inner()
        w.below = sum(c.below for c in kids) + pad(len(kids))
    wide.root.id, wide.root.fam = 0, align
    for w in sorted(wide.nodes, key=lambda w: w.depth):   # top-down
        kids = w.inner()
        slot, nxt = w.fam, w.fam + pad(len(kids))
        for c in kids:
            c.id = slot
            slot += 1
            c.fam = nxt
            nxt += c.below
    return align + wide.root.below


# ---------------------------------------------------------------------------------------------------------------
# the records (rp_layout.h)

def f32_rd(x: float) -> np.float32:
    f = np.float32(x)
    return np.nextafter(f, np.float32(-INF)) if float(f) > x else f


def f32_ru(x: float) -> np.float32:
    f = np.float32(x)
    return np.nextafter(f, np.float32(INF)) if float(f) < x else f


def plane_q(o, s, q: int) -> float:
    return float(o) + float(q) * float(s)  # exact in f64 (rp_layout.h)


def qframe(lo: float, hi: float):
    """rp_layout.h qframe, restated: -> (o, s) as float32"""
    o0 = f32_rd(lo)
    need = max((hi - lo) * (1.0 + 2.0 ** -7), hi - float(o0)) / 255.0 * (1.0 + 2.0 ** -40)
    need = max(max(need, abs(float(o0)) * 2.0 ** -28), 2.0 ** -60)
    s = f32_ru(need)
    _, e = math.frexp(float(s))
    if abs(lo) < math.ldexp(1.0, e + 15):
        g = math.ldexp(1.0, e - 9)
        o = np.float32(math.floor(lo / g) * g)
    else:
        o = o0
    while plane_q(o, s, 255) < hi:
        s = np.nextafter(s, np.float32(INF))
    return o, s


def q_down(x: float, o, s) -> int:
    f = math.floor((x - float(o)) / float(s))
    q = 0 if f <= 0.0 else (255 if f >= 255.0 else int(f))
    while q > 0 and plane_q(o, s, q) > x:
        q -= 1
    while q < 255 and plane_q(o, s, q + 1) <= x:
        q += 1
    return q


def q_up(x: float, o, s) -> int:
    c = math.ceil((x - float(o)) / float(s))
    q = 0 if c <= 0.0 else (255 if c >= 255.0 else int(c))
    while q < 255 and plane_q(o, s, q) < x:
        q += 1
    while q > 0 and plane_q(o, s, q - 1) >= x:
        q -= 1
    return q


def node_frame(w: WNode):
    """The frame of a quantized node: qframe per axis of the union of its children's boxes (0, 0 for an axis that is
    not finite or empty)."""
    o, s = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for a in range(3):
        lo = min(sl[4][a] for sl in w.slots)
        hi = max(sl[5][a] for sl in w.slots)
        ok = math.isfinite(lo) and math.isfinite(hi) and lo <= hi
        o[a], s[a] = qframe(lo, hi) if ok else qframe(0.0, 0.0)
    return o, s


def entry(slot) -> int:
    kind, cnt, first, child = slot[:4]
    return (ENTRY_LEAF | ((cnt - 1) << LEAF_SHIFT) | first) if kind == "leaf" else child.id


def encode(wide: Wide, total: int, node_format: int) -> np.ndarray:
    """The node records at their ids: child boxes f32 rounded outward (Node4; empty slots +inf / -inf) or quantized in
    the node's frame (Node4Q; empty slots lo 255, hi 0); entries ENTRY_LEAF | (count - 1) << 28 | first, a child's id,
    or ENTRY_EMPTY.  Records no node owns (dfs_line's pads) stay zero."""
    out = np.zeros(total, dtype=F.node_dtype(node_format))
    names = (("lo_x", "hi_x"), ("lo_y", "hi_y"), ("lo_z", "hi_z"))
    for w in wide.nodes:
        r = out[w.id]
        q8 = node_format == F.RP_NODES_Q8
        if q8:
            r["o"], r["s"] = node_frame(w)
        for k in range(4):
            if k >= len(w.slots):
                r["child"][k] = ENTRY_EMPTY
                for a in range(3):
                    r[names[a][0]][k] = 255 if q8 else INF
                    r[names[a][1]][k] = 0 if q8 else -INF
                continue
            sl = w.slots[k]
            r["child"][k] = entry(sl)
            for a in range(3):
                if q8:
                    r[names[a][0]][k] = q_down(sl[4][a], r["o"][a], r["s"][a])
                    r[names[a][1]][k] = q_up(sl[5][a], r["o"][a], r["s"][a])
                else:
                    r[names[a][0]][k] = f32_rd(sl[4][a])
                    r[names[a][1]][k] = f32_ru(sl[5][a])
    return out


# ---------------------------------------------------------------------------------------------------------------
# a whole build

@dataclass
class RefTree:
    nodes: np.ndarray  # records by node id (the root is 0)
    perm: list         # PrimRef.src in leaf order
    n_nodes: int
    n_leaves: int
    max_depth: int
    wide: Wide
    binary: BinTree


def finish(bt: BinTree, node_format: int, align: int = 1, rules: Rules = DEVICE) -> RefTree:
    wide = collapse(bt, rules)
    total = dfs_number(wide, align if bt.kind == "ploc" else 1, rules)
    return RefTree(encode(wide, total, node_format), wide.perm, total, wide.n_leaves, wide.max_depth, wide, bt)


def build(scene_or_boxes, builder: str, node_format: int = F.RP_NODES_F32, max_leaf: int = DEF_MAX_LEAF,
          cost_traverse: float = DEF_COST_TRAVERSE, dfs_line: bool = False, rules: Rules = DEVICE,
          merges: BinTree | None = None) -> RefTree:
    """The tree the device builder `builder` ("gpu": the LBVH, "ploc") makes.  `merges`: ploc_merges' tree of this input
    and these rules, reused between options (the leaf decisions do not feed back into the merges)."""
    bx = scene_or_boxes if isinstance(scene_or_boxes, Boxes) else scene_boxes(scene_or_boxes)
    if builder == "gpu":
        return finish(radix_tree(bx, max_leaf, rules), node_format, 1, rules)
    bt = merges if merges is not None else ploc_merges(bx, rules)
    ploc_sah(bt, max_leaf, cost_traverse, rules)
    align = 2 if dfs_line and node_format == F.RP_NODES_Q8 else 1
    return finish(bt, node_format, align, rules)


# ---------------------------------------------------------------------------------------------------------------
# what a tree must be, whoever built it

def check_valid(nodes: np.ndarray, root: int, perm, bx: Boxes, node_format: int):
    """Walks a 4-wide tree's records from the root: every primitive in exactly one leaf, every stored child box contains
    the exact boxes of the primitives below it, no record visited twice.  -> (inner nodes, leaves, max depth)."""
    names = (("lo_x", "hi_x"), ("lo_y", "hi_y"), ("lo_z", "hi_z"))
    seen_nodes, used = set(), np.zeros(len(perm), dtype=np.int64)
    stats = [0, 0, 0]

    def walk(i, depth):
        assert i not in seen_nodes and 0 <= i < len(nodes), i
        seen_nodes.add(i)
        stats[0] += 1
        stats[2] = max(stats[2], depth)
        r = nodes[i]
        lo_all, hi_all = np.full(3, INF), np.full(3, -INF)
        for k in range(4):
            c = int(r["child"][k])
            if c == ENTRY_EMPTY:
                continue
            if c & ENTRY_LEAF:
                cnt, first = ((c >> LEAF_SHIFT) & 7) + 1, c & LEAF_FIRST_MASK
                stats[1] += 1
                used[first:first + cnt] += 1
                src = np.asarray(perm[first:first + cnt])
                lo, hi = bx.lo[src].min(axis=0), bx.hi[src].max(axis=0)
            else:
                lo, hi = walk(c, depth + 1)
            for a in range(3):
                if node_format == F.RP_NODES_Q8:
                    slo = plane_q(r["o"][a], r["s"][a], int(r[names[a][0]][k]))
                    shi = plane_q(r["o"][a], r["s"][a], int(r[names[a][1]][k]))
                else:
                    slo, shi = float(r[names[a][0]][k]), float(r[names[a][1]][k])
                assert slo <= lo[a] and shi >= hi[a], (i, k, a, slo, lo[a], shi, hi[a])
            lo_all, hi_all = np.minimum(lo_all, lo), np.maximum(hi_all, hi)
        return lo_all, hi_all

    walk(root, 0)
    assert (used == 1).all(), np.nonzero(used != 1)[0][:8]
    assert sorted(perm) == list(range(len(perm)))
    return tuple(stats)

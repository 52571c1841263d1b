"""The device tree builders' trees (rp_bvh_gpu.hip: LBVH and PLOC, the wide collapse, the depth-first relayout), read
back with rp_scene_tree and held equal to tests/bvh_ref.py, the builders written out from their definitions, on the
inputs of tests/bvh_scenes.py.  Every comparison is exact: the kernels' arithmetic is f64 adds, multiplies, min/max and
one division without contraction, ties break by position and the radix sort is stable, so there is no tolerance.

options.self_check and the hit tests (test_gpu_bvh_small.py, test_intersect_rays) cannot see a tree's shape: a valid
tree of poor quality passes both.  tests/test_bvh_ref.py shows that each of eight plausible builder mistakes changes
the reference's tree on these inputs, so it would fail a case here.
"""
import numpy as np
import pytest

import bvh_ref as R
import bvh_scenes as S
from rtpotato import _ffi as F

pytestmark = pytest.mark.gpu

FORMATS = {"f32": F.RP_NODES_F32, "q8": F.RP_NODES_Q8}
COSTS = [0.0, 0.25, 4.0]  # cost_traverse: 0 = the default (0.7)
AXES = (("lo_x", "hi_x"), ("lo_y", "hi_y"), ("lo_z", "hi_z"))
CASES = [(name, b, f, m) for name in S.INPUTS for b in ("gpu", "ploc") for f in FORMATS for m in (1, 4, 8)]


def _entries_equal(dev, w, what):
    """One record against the reference's node: per slot empty, leaf (count and first index) or inner, and the child
    box bits; for a quantized node the frame bits.  -> the device ids of the inner children, in slot order."""
    want = [R.entry(s) if s[0] == "leaf" else None for s in w.slots] + [R.ENTRY_EMPTY] * (4 - len(w.slots))
    kids = []
    for k in range(4):
        c = int(dev["child"][k])
        if want[k] is None:
            assert not (c & R.ENTRY_LEAF), (what, k, hex(c))
            kids.append(c)
        else:
            assert c == want[k], (what, k, hex(c), hex(want[k]))
    return kids


def _walk_equal(nodes, ref, fmt):
    """The LBVH's node ids come from atomics, so its records are compared by a walk from the root in child slot order.
    -> [(device id, reference node)]"""
    pairs, seen = [], set()
    todo = [(0, ref.wide.root)]
    while todo:
        i, w = todo.pop()
        assert i not in seen and i < len(nodes), i
        seen.add(i)
        pairs.append((i, w))
        want = ref.nodes[w.id]
        for f in ([a for ax in AXES for a in ax] + (["o", "s"] if fmt == F.RP_NODES_Q8 else ["pad"])):
            assert nodes[i][f].tobytes() == want[f].tobytes(), (i, f, nodes[i][f], want[f])
        kids = _entries_equal(nodes[i], w, i)
        todo += list(zip(kids, w.inner()))
    assert len(seen) == len(nodes)  # every record belongs to the tree
    return pairs


def _frames_hold_the_definition(nodes, pairs):
    """On the frame the device stored: plane(q) = o + q s is exact in f64, the lo byte is the largest q whose plane is
    <= the child's exact lo, the hi byte the smallest q whose plane is >= its hi; an empty slot is lo 255, hi 0."""
    q = np.arange(256, dtype=np.float64)
    for i, w in pairs:
        r = nodes[i]
        for a in range(3):
            planes = np.float64(r["o"][a]) + q * np.float64(r["s"][a])
            for k in range(4):
                lo_b, hi_b = int(r[AXES[a][0]][k]), int(r[AXES[a][1]][k])
                if k >= len(w.slots):
                    assert (lo_b, hi_b) == (255, 0)
                    continue
                lo, hi = w.slots[k][4][a], w.slots[k][5][a]
                assert planes[0] <= lo and planes[255] >= hi, (i, a, k)
                assert lo_b == np.nonzero(planes <= lo)[0].max(), (i, a, k, lo_b)
                assert hi_b == np.nonzero(planes >= hi)[0].min(), (i, a, k, hi_b)


def _families_on_lines(nodes):
    """dfs_line: every family starts at a multiple of 2 and is consecutive; the records no entry references (the root
    apart) are pads, all zero, and no zero record is referenced."""
    raw = nodes.view(np.uint8).reshape(len(nodes), -1)
    referenced = {0}
    for i in range(len(nodes)):
        if not raw[i].any():
            continue
        kids = [int(c) for c in nodes[i]["child"] if not (int(c) & R.ENTRY_LEAF)]
        if kids:
            assert kids[0] % 2 == 0 and kids == list(range(kids[0], kids[0] + len(kids))), (i, kids)
        referenced.update(kids)
    for i in range(len(nodes)):
        assert raw[i].any() == (i in referenced), i
    return len(nodes) - len(referenced)


def _prims_follow(tree, scene, perm):
    """PrimRef.src in leaf order is the reference's, and the primitive records moved with it."""
    src = tree["prim_refs"]["src"]
    assert src.tolist() == list(perm)
    root = scene.root[src]
    tri = root["kind"] == F.RP_HITTABLE_TRIANGLE
    assert np.array_equal(tree["prims"]["kind"] == 1, tri)
    mesh = scene.scene_data.mesh_table[0]
    first = mesh.positions[mesh.indices[root["triangle"][tri]]]
    assert np.array_equal(tree["prims"]["g"][tri, 0:3], first)
    assert np.array_equal(tree["prims"]["g"][~tri, 0:3], root["center"][~tri])


@pytest.mark.parametrize("name,builder,fmt,max_leaf", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_tree_is_the_reference(gpu, name, builder, fmt, max_leaf):
    """Counts, primitive order and every node record.  PLOC: byte for byte at the same index (its depth-first relayout
    makes the ids reproducible), over cost_traverse in {default, 0.25, 4} and, for quantized nodes, node_layout auto and
    dfs_line.  LBVH: its node ids come from atomics and are not reproducible, so the records are compared by a walk
    from the root in child slot order (which is also why test_ploc_build_is_deterministic covers PLOC only)."""
    scene = S.scene(name)
    nf = FORMATS[fmt]
    n = len(scene.root)
    costs = COSTS if builder == "ploc" else [0.0]
    layouts = ["auto", "dfs_line"] if (builder, fmt) == ("ploc", "q8") else ["auto"]
    for ct in costs:
        for layout in layouts:
            what = (name, builder, fmt, max_leaf, ct, layout)
            ref = S.reference(name, builder, nf, max_leaf, ct or R.DEF_COST_TRAVERSE, layout == "dfs_line")
            opts = {"builder": builder, "node_format": fmt, "max_leaf": max_leaf, "cost_traverse": ct,
                    "node_layout": layout, "self_check": 1}
            with gpu.DeviceScene(scene, options=opts) as ds:
                info, tree = ds.info(), ds.tree()
            assert (tree["node_format"], tree["root"]) == (nf, 0), what
            got = (info["nodes"], info["leaves"], info["max_depth"], info["prims"])
            assert got == (ref.n_nodes, ref.n_leaves, ref.max_depth, n), (what, got)
            _prims_follow(tree, scene, ref.perm)
            nodes = tree["nodes"]
            if builder == "ploc":
                same = nodes.view(np.uint8).reshape(len(nodes), -1) == ref.nodes.view(np.uint8).reshape(len(nodes), -1)
                bad = np.nonzero(~same.all(axis=1))[0]
                assert not len(bad), (what, bad[:4], nodes[bad[:1]], ref.nodes[bad[:1]])
                pairs = [(w.id, w) for w in ref.wide.nodes]
                if layout == "dfs_line":
                    assert _families_on_lines(nodes) == ref.n_nodes - len(ref.wide.nodes), what
            else:
                pairs = _walk_equal(nodes, ref, nf)
            if nf == F.RP_NODES_Q8:
                _frames_hold_the_definition(nodes, pairs)


def _walk_w8(nodes, root, n):
    """Node8Q: the inner child at slot s is record (inner & W8_INDEX) + popcount(imask below s), imask = inner >> 24;
    the primitives of slot s's leaf are the set bits of pmask[s], counted from `prim`.  -> uses per primitive"""
    used, seen, todo = np.zeros(n, dtype=np.int64), set(), [root]
    while todo:
        i = todo.pop()
        assert i not in seen and i < len(nodes)
        seen.add(i)
        r = nodes[i]
        imask, base = int(r["inner"]) >> 24, int(r["inner"]) & 0x00FFFFFF
        for s in range(8):
            if imask >> s & 1:
                todo.append(base + bin(imask & ((1 << s) - 1)).count("1"))
            for b in range(32):
                if int(r["pmask"][s]) >> b & 1:
                    used[int(r["prim"]) + b] += 1
    return used, len(seen)


@pytest.mark.parametrize("fmt", ["f32", "q8", "w8"])
def test_host_trees_read_back(gpu, fmt):
    """The host builder's trees go out through the same call: every primitive in exactly one leaf of the walk from the
    root, the byte counts consistent with info()."""
    scene = S.scene("uniform_259")
    n = len(scene.root)
    with gpu.DeviceScene(scene, options={"builder": "host", "node_format": fmt, "always_max": 0}) as ds:
        info, tree = ds.info(), ds.tree()
    nodes = tree["nodes"]
    assert tree["node_format"] == {"f32": F.RP_NODES_F32, "q8": F.RP_NODES_Q8, "w8": F.RP_NODES_W8}[fmt]
    assert len(nodes) == info["nodes"] and len(tree["prims"]) == len(tree["prim_refs"]) == info["prims"] == n
    assert nodes.dtype.itemsize == (64 if fmt == "q8" else 128)
    assert nodes.nbytes + tree["prims"].nbytes + tree["prim_refs"].nbytes <= info["device_bytes"]
    assert sorted(tree["prim_refs"]["src"].tolist()) == list(range(n))
    if fmt == "w8":
        used, reached = _walk_w8(nodes, tree["root"], n)
        assert reached <= len(nodes)
    else:
        bx = R.scene_boxes(scene)
        inner, leaves, depth = R.check_valid(nodes, tree["root"], tree["prim_refs"]["src"].tolist(), bx, tree["node_format"])
        assert inner <= info["nodes"] and depth <= info["max_depth"] and leaves <= n, (inner, leaves, depth, info)
        used = np.ones(n, dtype=np.int64)  # check_valid holds every position to one leaf
    assert (used == 1).all()


def test_tree_read_back_refuses_small_buffers(gpu):
    """rp_scene_tree: NULL buffers query the format and the root; a buffer smaller than its records is RP_EINVAL with the
    bytes needed in the message, and nothing is written to any buffer; a NULL scene is RP_EINVAL."""
    import ctypes
    L = F.rp()
    scene = S.scene("uniform_33")
    with gpu.DeviceScene(scene, options={"builder": "ploc", "node_format": "q8"}) as ds:
        info, tree = ds.info(), ds.tree()
        fmt, root = ctypes.c_uint32(99), ctypes.c_uint32(99)
        assert L.rp_scene_tree(ds.handle, None, 0, None, 0, None, 0, ctypes.byref(fmt), ctypes.byref(root)) == F.RP_OK
        assert (fmt.value, root.value) == (F.RP_NODES_Q8, 0)
        need = [64 * info["nodes"], 80 * info["prims"], 16 * info["prims"]]
        assert need == [tree["nodes"].nbytes, tree["prims"].nbytes, tree["prim_refs"].nbytes]
        for short in range(3):
            bufs = [np.full(b, 0xA5, dtype=np.uint8) for b in need]
            sizes = list(need)
            sizes[short] -= 1
            rc = L.rp_scene_tree(ds.handle, bufs[0].ctypes.data, sizes[0], bufs[1].ctypes.data, sizes[1],
                                 bufs[2].ctypes.data, sizes[2], None, None)
            assert rc == F.RP_EINVAL
            assert str(need[short]) in L.rp_last_error().decode()
            assert all((b == 0xA5).all() for b in bufs)
        # one buffer alone, exactly its size
        refs = np.zeros(info["prims"], dtype=F.prim_ref_dtype())
        assert L.rp_scene_tree(ds.handle, None, 0, None, 0, refs.ctypes.data, refs.nbytes, None, None) == F.RP_OK
        assert np.array_equal(refs, tree["prim_refs"])
    assert L.rp_scene_tree(None, None, 0, None, 0, None, 0, None, None) == F.RP_EINVAL

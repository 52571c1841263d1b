"""The refit on the CPU: the host model (rph_refit_records, rph_refit_plan, rph_bvh_refit_check: the loops over
rp_refit.h that the device kernels compile too) against tests/refit_ref.py, the refit written out in numpy, bit for bit;
a refit with unchanged geometry gives back every byte of the builders' trees; the refit host tree passes the builder's
own check(); the plan; the bound; the refusals.  No tolerance anywhere: the arithmetic is f64 min, max and subtraction
and the rounding of tests/bvh_ref.py.
"""
import ctypes
import functools

import numpy as np
import pytest

import bvh_ref as R
import bvh_scenes as S
import refit_ref as RR
from rtpotato import _ffi as F
from rtpotato import render, scenes

FORMATS = {"f32": F.RP_NODES_F32, "q8": F.RP_NODES_Q8}
INPUTS = ["uniform_2", "uniform_5", "uniform_257", "mixed", "clustered", "duplicates", "planar"]
CASES = [(n, b, f, m, False) for n in INPUTS for b in ("gpu", "ploc") for f in FORMATS for m in (1, 4, 8)] + \
        [(n, "ploc", "q8", 4, True) for n in INPUTS]
IDS = ["-".join(map(str, c[:4])) + ("-dfs_line" if c[4] else "") for c in CASES]
BOUND = 2.0 ** 20


def _tree(name, builder, fmt, max_leaf, dfs_line):
    ref = S.reference(name, builder, FORMATS[fmt], max_leaf, R.DEF_COST_TRAVERSE, dfs_line)
    return RR.tree_of(S.scene(name), ref, FORMATS[fmt])


def _copy(tree, tn):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tree.items()}, tn.copy()


def _same(a, b, what):
    for k in ("nodes", "prims", "prim_refs"):
        assert a[0][k].tobytes() == b[0][k].tobytes(), (what, k)
    assert a[1].tobytes() == b[1].tobytes(), (what, "tri_normals")


@functools.lru_cache(maxsize=None)
def _deformed(name):
    return RR.deform(RR.geometry(S.scene(name)))


def _host(tree, tn, g, bound=BOUND, **kw):
    return render.refit_records_host(tree, g.get("positions"), g.get("normals"), g.get("spheres"), bound, tri_normals=tn, **kw)


@pytest.mark.parametrize("name,builder,fmt,max_leaf,dfs_line", CASES, ids=IDS)
def test_host_model_is_the_reference(name, builder, fmt, max_leaf, dfs_line):
    """Identity: the reference builders' tree refit to its own geometry keeps every byte (nodes, pads, prims, refs,
    normals).  Deformed: the host model and the numpy refit write the same bytes and the same status."""
    before = _tree(name, builder, fmt, max_leaf, dfs_line)
    g0 = RR.geometry(S.scene(name))
    same = _copy(*before)
    assert _host(*same, g0) == 0
    _same(same, before, "identity")
    g1 = _deformed(name)
    host, ref = _copy(*before), _copy(*before)
    st_host = _host(*host, g1)
    st_ref = RR.refit(ref[0], ref[1], g1["positions"], g1["normals"], g1["spheres"], BOUND)
    assert st_host == st_ref == 0
    _same(host, ref, "deformed")
    assert host[0]["nodes"].tobytes() != before[0]["nodes"].tobytes() or name == "uniform_2"
    assert host[0]["prims"].tobytes() != before[0]["prims"].tobytes()
    assert np.array_equal(host[0]["nodes"]["child"], before[0]["nodes"]["child"])  # the entries are never written


def test_normals_alone_move_no_box():
    before = _tree("mixed", "ploc", "q8", 4, False)
    g1 = _deformed("mixed")
    host, ref = _copy(*before), _copy(*before)
    assert _host(*host, {"normals": g1["normals"]}) == 0
    assert RR.refit(ref[0], ref[1], normals=g1["normals"]) == 0
    _same(host, ref, "normals")
    for k in ("nodes", "prims", "prim_refs"):
        assert host[0][k].tobytes() == before[0][k].tobytes()
    assert host[1].tobytes() != before[1].tobytes()


def _with(scene, g):
    return render.with_geometry(scene, g["positions"], g["normals"], g["spheres"])


def _refit_check(before, after, fmt, always_max=-1, always_minor=1):
    d0, d1 = before.desc(), after.desc()
    hashes, st = np.zeros(2, dtype=np.uint64), ctypes.c_uint32(7)
    F.check_host(F.host().rph_bvh_refit_check(d0.ptr(), d1.ptr(), FORMATS[fmt], always_max, always_minor,
                                              hashes.ctypes.data, ctypes.byref(st)))
    return int(hashes[0]), int(hashes[1]), st.value


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", INPUTS + ["uniform_1031"])
def test_host_builder_tree_identity(name, fmt):
    """The host SAH builder's tree, always-tested tail and all, refit to its own description: the same records."""
    sc = S.scene(name)
    for always_max, minor in ((-1, 1), (0, 0)):
        h0, h1, st = _refit_check(sc, sc, fmt, always_max, minor)
        assert h0 == h1 and st == 0, (name, fmt, always_max)


@functools.lru_cache(maxsize=None)
def _catalogue(name):
    return scenes.CATALOGUE[name]() if name in scenes.CATALOGUE else S.scene(name)


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("name", ["mixed", "uniform_1031", "three_balls", "bunny_lambert"])
def test_refit_host_tree_passes_the_builders_check(name, fmt):
    """The deformed scene's refit tree under rpb::check against the after-geometry: every child box contains its
    subtree's exact boxes, every frame lies inside the bound, every primitive is referenced once."""
    sc = _catalogue(name)
    after = _with(sc, RR.deform(RR.geometry(sc)))
    h0, h1, st = _refit_check(sc, after, fmt)
    assert h0 != h1 and st == 0


def test_refit_check_refuses_another_topology():
    a, b = S.scene("uniform_5"), S.scene("uniform_33")
    with pytest.raises(F.RPError):
        _refit_check(a, b, "f32")


# ---------------------------------------------------------------------------------------------------------------
# the plan

def _host_plan(tree):
    n = len(tree["nodes"])
    levels, order, nl = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), ctypes.c_uint32()
    F.check_host(F.host().rph_refit_plan(tree["node_format"], tree["nodes"].ctypes.data, n, tree["root"],
                                         levels.ctypes.data, order.ctypes.data, ctypes.byref(nl)))
    return levels, order, nl.value


@pytest.mark.parametrize("name,builder,fmt,max_leaf,dfs_line",
                         [("uniform_257", "gpu", "f32", 1, False), ("clustered", "ploc", "q8", 4, True),
                          ("mixed", "ploc", "f32", 8, False), ("uniform_2", "ploc", "q8", 4, True)])
def test_plan(name, builder, fmt, max_leaf, dfs_line):
    tree, _ = _tree(name, builder, fmt, max_leaf, dfs_line)
    levels, order, n_levels = _host_plan(tree)
    want_levels, want_order, want_n = RR.plan(tree["nodes"], 0)
    assert np.array_equal(levels, want_levels) and n_levels == want_n
    reached = order[order != RR.NOT_REACHED].tolist()
    assert reached == want_order and order[len(reached):].tolist() == [RR.NOT_REACHED] * (len(order) - len(reached))
    ref = S.reference(name, builder, FORMATS[fmt], max_leaf, R.DEF_COST_TRAVERSE, dfs_line)
    assert sorted(reached) == sorted(w.id for w in ref.wide.nodes)  # every node of the tree once, no pad
    raw = tree["nodes"].view(np.uint8).reshape(len(tree["nodes"]), -1)
    pads = [i for i in range(len(raw)) if not raw[i].any()]
    assert all(levels[i] == RR.NOT_REACHED for i in pads) and (not dfs_line or name == "uniform_2" or pads)
    for i in reached:  # above all of its inner children
        for c in tree["nodes"][i]["child"]:
            if int(c) != R.ENTRY_EMPTY and not int(c) & R.ENTRY_LEAF:
                assert levels[i] > levels[int(c)]
    assert sorted(levels[reached].tolist()) == levels[reached].tolist()  # sorted by level ...
    for lv in range(n_levels):
        run = [i for i in reached if levels[i] == lv]
        assert run == sorted(run) and run  # ... then by index, no level empty
    if name == "uniform_2":
        assert n_levels == 1 and reached == [0]


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_all_primitives_always_tested(fmt):
    """A root with four empty slots over three spheres outside the tree: the refit rewrites the spheres, and the node
    -- (+inf, -inf) slots, or the frame of an empty union at 0 -- refits to itself."""
    nf = FORMATS[fmt]
    nodes = np.zeros(1, dtype=F.node_dtype(nf))
    nodes["child"] = R.ENTRY_EMPTY
    RR.node_words(nf, nodes[0], [None] * 4)
    prims = np.zeros(3, dtype=F.prim_dtype())
    refs = np.zeros(3, dtype=F.prim_ref_dtype())
    refs["src"] = [2, 0, 1]
    sph = np.array([[0.0, 0.0, 0.0, 1.0], [3.0, 0.0, 0.0, 0.5], [0.0, 4.0, 0.0, 0.25]])
    prims["g"][:, 0:4] = sph[refs["src"]]
    tree = {"node_format": nf, "root": 0, "nodes": nodes.copy(), "prims": prims.copy(), "prim_refs": refs}
    assert render.refit_records_host(tree, spheres=sph, bound=BOUND) == 0
    assert tree["nodes"].tobytes() == nodes.tobytes() and tree["prims"].tobytes() == prims.tobytes()
    assert render.refit_records_host(tree, spheres=sph * 2.0, bound=BOUND) == 0
    assert tree["nodes"].tobytes() == nodes.tobytes()
    assert np.array_equal(tree["prims"]["g"][:, 0:4], 2.0 * sph[refs["src"]])  # by rank among the spheres, through src


# ---------------------------------------------------------------------------------------------------------------
# the bound, NaN

@pytest.mark.parametrize("fmt", list(FORMATS))
def test_bound_and_nan(fmt):
    before = _tree("uniform_33", "ploc", fmt, 1, False)
    g = RR.geometry(S.scene("uniform_33"))
    # one vertex at 2 B: the status bit and nothing else -- the records are still the definition's
    far = {k: v.copy() for k, v in g.items()}
    far["positions"][7, 1] = 2.0 * BOUND
    host, ref = _copy(*before), _copy(*before)
    assert _host(*host, far) == RR.OUT_OF_BOUND == F.RP_REFIT_OUT_OF_BOUND
    assert RR.refit(ref[0], ref[1], far["positions"], far["normals"], far["spheres"], BOUND) == RR.OUT_OF_BOUND
    _same(host, ref, "far")
    at = {k: v.copy() for k, v in g.items()}
    at["positions"][7, 1] = BOUND  # at the bound is inside it
    assert _host(*_copy(*before), at) == 0
    # infinities and NaN report nothing.  A NaN vertex is ignored beside the triangle's other two (fmin, fmax); a
    # triangle of three NaN vertices has a NaN box: NaN words in a Node4 slot, the whole frame (0, 255) in a Node4Q's
    nan = {k: v.copy() for k, v in g.items()}
    tri_a, tri_b = 3, 11
    nan["positions"][3 * tri_a] = np.nan
    nan["positions"][3 * tri_b:3 * tri_b + 3] = np.nan
    host, ref = _copy(*before), _copy(*before)
    assert _host(*host, nan) == 0
    assert RR.refit(ref[0], ref[1], nan["positions"], nan["normals"], nan["spheres"], BOUND) == 0
    _same(host, ref, "nan")
    nodes, src = host[0]["nodes"], host[0]["prim_refs"]["src"]
    found = 0
    for r in nodes:
        for c in range(4):
            e = int(r["child"][c])
            if e == R.ENTRY_EMPTY or not e & R.ENTRY_LEAF:
                continue
            assert (e >> R.LEAF_SHIFT) & 7 == 0  # max_leaf 1
            t = int(src[e & R.LEAF_FIRST_MASK])
            words = [r[f][c] for ax in RR.AXES for f in ax]
            if t == tri_b:
                found += 1
                assert (words == [0, 255] * 3) if fmt == "q8" else np.isnan(words).all()
            elif t == tri_a:
                found += 1
                lo, hi = np.fmin(*g["positions"][3 * t + 1:3 * t + 3]), np.fmax(*g["positions"][3 * t + 1:3 * t + 3])
                if fmt == "f32":
                    assert words == [x for a in range(3) for x in (R.f32_rd(lo[a]), R.f32_ru(hi[a]))]
                else:
                    assert words == [x for a in range(3) for x in (R.q_down(lo[a], r["o"][a], r["s"][a]),
                                                                   R.q_up(hi[a], r["o"][a], r["s"][a]))]
    assert found == 2
    inf = {k: v.copy() for k, v in g.items()}
    inf["positions"][5, 0] = np.inf
    assert _host(*_copy(*before), inf) == 0


# ---------------------------------------------------------------------------------------------------------------
# refusals, bindings

def test_refusals():
    before = _tree("mixed", "ploc", "f32", 4, False)
    g = RR.geometry(S.scene("mixed"))
    nv, ns = len(g["positions"]), len(g["spheres"])

    def refused(what, **kw):
        t = _copy(*before)
        with pytest.raises(F.RPError) as e:
            what(t, **kw)
        assert e.value.code == F.RP_EINVAL
        _same(t, before, "a refused call writes nothing")

    refused(lambda t: _host(*t, {}))                                           # all inputs NULL
    refused(lambda t: _host(*t, {"positions": g["positions"]}))                # geometry named in part: spheres missing
    refused(lambda t: _host(*t, {"spheres": g["spheres"]}))                    # ... positions missing
    refused(lambda t: _host(*t, g, n_vertices=nv - 1))                         # fewer vertices than the triangles name
    refused(lambda t: _host(*t, g, n_spheres=ns - 1))                          # not the scene's sphere count
    refused(lambda t: _host(*t, g, n_spheres=ns + 1))
    refused(lambda t: _host(*t, g, bound=float("inf")))
    refused(lambda t: _host(*t, g, bound=-1.0))
    refused(lambda t: _host({**t[0], "node_format": F.RP_NODES_W8}, t[1], g))  # an 8-wide tree is rebuilt, not refit
    refused(lambda t: _host({**t[0], "root": len(t[0]["nodes"])}, t[1], g))    # records that are no tree
    t = _copy(*before)
    rc = F.host().rph_refit_records(t[0]["node_format"], t[0]["nodes"].ctypes.data, len(t[0]["nodes"]), 0,
                                    t[0]["prims"].ctypes.data, t[0]["prim_refs"].ctypes.data, t[1].ctypes.data,
                                    len(t[0]["prims"]), g["positions"].ctypes.data, None, g["spheres"].ctypes.data, nv, ns,
                                    BOUND, None)                               # NULL status
    assert rc == F.RP_EINVAL and b"status" in F.host().rph_last_error()
    _same(t, before, "NULL status")
    h = ctypes.c_void_p(1)
    assert F.rp().rp_refit_create(None, 0.0, ctypes.byref(h)) == F.RP_EINVAL and not h.value  # a NULL scene
    assert F.rp().rp_scene_refit_device(None, None, None, None, None, None) == F.RP_EINVAL
    F.rp().rp_refit_destroy(None)


def test_bindings():
    for s in ("rp_refit_create", "rp_refit_destroy", "rp_refit_info", "rp_scene_refit_device", "rp_scene_refit"):
        assert s in F.RP_SYMBOLS and hasattr(F.rp(), s)
    for s in ("rph_refit_records", "rph_refit_plan", "rph_bvh_refit_check"):
        assert s in F.HOST_SYMBOLS and hasattr(F.host(), s)
    assert F.tri_normals_dtype().itemsize == 72 and F.RP_REFIT_OUT_OF_BOUND == 1
    assert hasattr(render.DeviceScene, "refit_handle") and hasattr(render.DeviceScene, "geometry")
    assert all(hasattr(render.Refit, m) for m in ("update", "update_device", "info", "close", "__enter__"))
    g = render.scene_geometry(S.scene("mixed"))
    want = RR.geometry(S.scene("mixed"))
    assert all(np.array_equal(g[k], want[k]) for k in want)

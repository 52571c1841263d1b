"""tests/bvh_ref.py, the written-out reference of the device tree builders, checked on the CPU: it makes valid trees on
every input of tests/bvh_scenes.py, its recursive radix tree is Karras' construction, the inputs exercise what they
are aimed at, and each of eight deliberate mistakes changes the tree on at least one of them -- so
tests/test_gpu_bvh_ref.py, which holds the device's trees equal to this reference on the same inputs, would fail if
the device made one of them."""
import numpy as np
import pytest

import bvh_ref as R
import bvh_scenes as S
from rtpotato import _ffi as F

F32, Q8 = F.RP_NODES_F32, F.RP_NODES_Q8
CT = R.DEF_COST_TRAVERSE


@pytest.mark.parametrize("builder", ["gpu", "ploc"])
@pytest.mark.parametrize("name", list(S.INPUTS))
def test_reference_is_a_valid_tree(name, builder):
    """Every primitive in exactly one leaf, every stored box (f32, or quantized in its frame) contains its subtree, the
    counts are the walk's; a PLOC build makes n - 1 binary nodes, every leaf holds at most max_leaf primitives."""
    bx = S.boxes(name)
    n = len(bx.lo)
    for fmt, max_leaf, line in [(F32, 1, False), (F32, 4, False), (F32, 8, False), (Q8, 4, False), (Q8, 4, True)]:
        ref = S.reference(name, builder, fmt, max_leaf, CT, line)
        inner, leaves, depth = R.check_valid(ref.nodes, 0, ref.perm, bx, fmt)
        assert (leaves, depth) == (ref.n_leaves, ref.max_depth)
        assert inner == len(ref.wide.nodes) <= ref.n_nodes == len(ref.nodes)
        assert -(-n // max_leaf) <= leaves <= n
        if builder == "ploc":
            assert len(ref.binary.left) == n - 1 and ref.binary.root == n - 2
        if not (line and builder == "ploc"):
            assert inner == ref.n_nodes
        for w in ref.wide.nodes:
            assert 2 <= len(w.slots) <= 4 and all(1 <= s[1] <= max_leaf for s in w.slots if s[0] == "leaf")


@pytest.mark.parametrize("name", ["clustered", "duplicates", "uniform_259", "planar", "mixed"])
def test_recursive_radix_tree_is_karras(name):
    """The radix tree over unique keys is unique: the plain recursive definition (what the reference builds from) and
    Karras' per-node search (what radix_tree_kernel runs, restated apart) give the same ranges and splits."""
    keys, _ = R.lbvh_keys(S.boxes(name))
    assert len(set(keys)) == len(keys) and keys == sorted(keys)
    assert R.radix_ranges(keys) == R.karras_tree(keys)


def test_clustered_input_shares_one_cell():
    keys, order = R.lbvh_keys(S.boxes("clustered"))
    codes = np.array([k >> 32 for k in keys])
    vals, counts = np.unique(codes, return_counts=True)
    assert counts.max() >= 300  # the cluster: one 30-bit cell, ordered by index alone
    run = [o for k, o in zip(keys, order) if k >> 32 == vals[counts.argmax()]]
    assert run == sorted(run)
    ref = S.reference("clustered", "gpu", F32, 1, CT)
    assert ref.max_depth >= 8  # deep chains


def test_planar_input_fires_the_sah_leaf_rule():
    """At least a quarter of the binary merges on the planar grid are SAH leaves (the two triangles of a quad share a
    box), and its zero-extent axis has scale 0."""
    bx = S.boxes("planar")
    assert bx.scale[1] == 0.0 and bx.scale[0] > 0.0 and bx.scale[2] > 0.0
    bt = R.ploc_merges(bx)
    R.ploc_sah(bt, R.DEF_MAX_LEAF, CT)
    assert 4 * sum(bt.leaf) >= len(bt.leaf), (sum(bt.leaf), len(bt.leaf))
    assert not all(bt.leaf[k] for k in range(len(bt.leaf)) if bt.size[k] <= R.DEF_MAX_LEAF)  # and it also refuses


def test_seam_inputs_put_a_mutual_pair_across_position_256():
    for n in S.SEAM:
        bx = S.boxes(f"seam_{n}")
        _, order = R.ploc_keys(bx)
        assert order == list(range(n))
        nn = R.ploc_nearest(bx.lo, bx.hi)
        assert nn[255] == 256 and nn[256] == 255


def test_q_bytes_are_the_definition():
    """q_down is the largest q whose plane is <= x, q_up the smallest whose plane is >= x, on the frames of a
    reference tree far from the origin."""
    ref = S.reference("mixed", "ploc", Q8, 4, CT)
    for w in ref.wide.nodes:
        o, s = R.node_frame(w)
        for sl in w.slots:
            for a in range(3):
                lo, hi = sl[4][a], sl[5][a]
                planes = np.array([R.plane_q(o[a], s[a], q) for q in range(256)])
                assert R.q_down(lo, o[a], s[a]) == np.nonzero(planes <= lo)[0].max()
                assert R.q_up(hi, o[a], s[a]) == np.nonzero(planes >= hi)[0].min()


# The options at which each mistake is looked for: PLOC's own rules on a PLOC build, the shared ones on both builders.
def _signature(name, builder, fmt, line, rules):
    ref = S.reference(name, builder, fmt, R.DEF_MAX_LEAF, CT, line, rules)
    return ref.nodes.tobytes(), tuple(ref.perm)


SENSITIVITY = {  # mistake -> (builder, format, dfs_line) it is looked for with
    "radius_2": ("ploc", F32, False), "seam_256": ("ploc", F32, False), "tie_larger_j": ("ploc", F32, False),
    "no_sah_leaf": ("ploc", F32, False), "open_first": ("ploc", F32, False), "ploc_20_bits": ("ploc", F32, False),
    "swap_xz": ("gpu", F32, False), "unpadded_families": ("ploc", Q8, True),
}
# One input per mistake that must catch it (profiles/r21/MANIFEST.md has the whole table): the named GPU case
# test_tree_is_the_reference[<input>-<builder>-...] fails if the device makes the mistake.
WITNESS = {
    "radius_2": "uniform_259", "seam_256": "seam_257", "tie_larger_j": "duplicates", "no_sah_leaf": "planar",
    "open_first": "uniform_33", "ploc_20_bits": "clustered", "swap_xz": "uniform_33", "unpadded_families": "uniform_33",
}


def catches(mistake):
    builder, fmt, line = SENSITIVITY[mistake]
    return [name for name in S.INPUTS
            if _signature(name, builder, fmt, line, R.MISTAKES[mistake]) != _signature(name, builder, fmt, line, None)]


@pytest.mark.parametrize("mistake", list(R.MISTAKES))
def test_aimed_inputs_see_the_mistakes(mistake):
    """Each deliberate mistake, applied to the reference, changes the final tree (node records or primitive order) on at
    least one input of the GPU test, its named witness among them."""
    caught = catches(mistake)
    print(mistake, "->", ", ".join(caught))
    assert WITNESS[mistake] in caught, (mistake, caught)


def test_lost_seam_neighbours_need_the_aimed_layout():
    """A search that loses neighbours across position 256 builds the same tree on uniform boxes at n = 257 and 259 --
    which is why the seam inputs exist -- and another one on every seam input."""
    caught = catches("seam_256")
    assert all(f"seam_{n}" in caught for n in S.SEAM), caught
    print("seam_256 on uniform_257 / uniform_259:", "uniform_257" in caught, "uniform_259" in caught)

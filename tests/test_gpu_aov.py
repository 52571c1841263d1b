"""GPU: the first-hit feature pass (rp_render_aov / rp_render_aov_device_ws: normal, albedo, depth, foreground)
against the oracle-built references of tests/aov_ref.py, against the render's own camera rays, across shards, with
nullable outputs, asynchronously, and on a deep tree.  32 x 32 tiles: 48 rows give an edge tile."""
from dataclasses import replace

import numpy as np
import pytest

import aov_ref
from parity import TOL_EXACT, assert_parity, compare, shard_mask

pytestmark = pytest.mark.gpu


def _assert_aov_parity(out, ref):
    """Normal and albedo at the project's parity bar (L-inf < 1e-3, >= 99.9 % of pixels within 1e-12), fg exact."""
    for name in ("normal", "albedo"):
        if out.get(name) is not None and name in ref:
            c = compare(out[name], ref[name])
            print(name, c)
            assert_parity(c)
    assert np.array_equal(out["fg"], ref["fg"])


@pytest.mark.parametrize("name,options", [("variants", None), ("variants_sky", None), ("earth", None),
                                          ("three_balls", None), ("bunny_full", None),
                                          ("bunny_full", {"node_format": "q8"}), ("bunny_full", {"node_format": "w8"})])
def test_parity_with_oracle(gpu, name, options):
    """4 spp, every texture kind behind AlbedoMap (Noise, DebugUVs, Missing, Checker, Image over sphere uv, Solid), a
    lens (three_balls), List and Bvh roots, the three node formats."""
    r = aov_ref.refs(name, 4)
    with gpu.DeviceScene(r["scene"], options=options) as ds:
        out = ds.render_aov(r["params"])
    _assert_aov_parity(out, r)
    st = out["stats"]
    n = r["params"].width * r["params"].height
    assert (st["rays"], st["samples"], st["pixels"]) == (4 * n, 4 * n, n)


@pytest.mark.parametrize("name,spp", [(n, 1) for n in aov_ref.PINHOLE] + [("bunny_full", 4)])
def test_depth(gpu, name, spp):
    """hit.t against the oracle's closest-hit query on the rebuilt camera rays: the same pixels hit, and
    |d - ref| / max(1, ref) <= 1e-12 (rp_intersect's t is bit-equal to the oracle's; a one-ulp change of a direction
    component moves t by at most 1.3e-13 relative)."""
    r = aov_ref.refs(name, spp)
    with gpu.DeviceScene(r["scene"]) as ds:
        out = ds.render_aov(r["params"], normal=False, albedo=False)
    assert np.array_equal(out["fg"], r["depth_fg"])
    assert np.array_equal(out["depth"] > 0, r["depth"] > 0)
    err = np.abs(out["depth"] - r["depth"]) / np.maximum(1.0, r["depth"])
    print(name, spp, "max relative depth error", float(err.max()), "hit pixels", int((r["depth"] > 0).sum()))
    assert err.max() <= TOL_EXACT


@pytest.mark.parametrize("name", ["bunny_full", "three_balls"])
def test_same_rays_as_the_render(gpu, name):
    """Beside a beauty frame at samples_per_stream = 1 the buffers describe the very same camera rays: the render of
    the DebugNormals-substituted scene is the normal buffer of the original scene (three_balls samples its lens)."""
    sc, p = aov_ref.scene_params(name, 4)
    with gpu.DeviceScene(aov_ref.normals_scene(sc)) as ds:
        rgb, fg, _ = ds.render(replace(p, samples_per_stream=1), foreground=True)
    with gpu.DeviceScene(sc) as ds:
        out = ds.render_aov(p, albedo=False, depth=False)
    err = np.abs(out["normal"] - rgb).max()
    print(name, "max |normal - render|", float(err))
    assert err <= TOL_EXACT
    assert np.array_equal(out["fg"], fg)


def test_shards(gpu):
    """num_shards = 3 on the 64 x 48 frame (4 tiles: shards of 2, 1 and 1): every interleaved shard is the whole
    frame's pixels bit for bit; a balanced shard is refused on a workspace without a plan and, after the beauty render
    of that frame on the workspace, holds that render's tiles."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import unpack_shard
    from rtpotato.scene import shard_slot_count, shard_slot_pixels
    sc, p = aov_ref.scene_params("variants", 4)
    with gpu.DeviceScene(sc) as ds:
        whole = ds.render_aov(p)
        sizes = []
        for s in range(3):
            q = replace(p, shard=s, num_shards=3)
            part = ds.render_aov(q)
            m = shard_mask(q)
            sizes.append(shard_slot_count(q) // (32 * 32))
            assert part["stats"]["pixels"] == int(m.sum())
            for k in ("normal", "albedo", "depth", "fg"):
                assert np.array_equal(part[k][m], whole[k][m]), (s, k)
                assert not part[k][~m].any(), (s, k)  # only the shard's pixels are written
        assert sizes == [2, 1, 1]
        q = replace(p, shard=1, num_shards=3, shard_map=F.RP_SHARD_BALANCED)
        n = shard_slot_count(q)
        ws = ds.workspace()
        nrm = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        dep = torch.zeros(n, dtype=torch.float64, device="cuda")
        with pytest.raises(F.RPError) as e:
            ds.render_aov_device(q, normal=nrm, depth=dep, workspace=ws)
        assert e.value.code == F.RP_EINVAL
        rgb = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.render_device(q, rgb, ctr, workspace=ws)
        ds.render_aov_device(q, normal=nrm, depth=dep, workspace=ws)
        torch.cuda.synchronize()
        tmap = ds.tile_map(q, ws)
        idx = shard_slot_pixels(q, tmap)
        m = np.zeros(p.width * p.height, dtype=bool)
        m[idx[idx >= 0]] = True
        m = m.reshape(p.height, p.width)
        assert np.array_equal(unpack_shard(q, nrm.cpu().numpy(), 3, tile_map=tmap)[m], whole["normal"][m])
        assert np.array_equal(unpack_shard(q, dep.cpu().numpy(), 1, tile_map=tmap)[m][:, 0], whole["depth"][m])


def test_nullable_outputs_and_counters(gpu):
    import torch
    from rtpotato import _ffi as F
    from rtpotato.scene import shard_slot_count
    sc, p = aov_ref.scene_params("bunny_full", 3)
    with gpu.DeviceScene(sc) as ds:
        full = ds.render_aov(p)
        only = ds.render_aov(p, normal=False, albedo=False, foreground=False)
        assert only["normal"] is None and only["albedo"] is None and only["fg"] is None
        assert np.array_equal(only["depth"], full["depth"])
        alb = ds.render_aov(p, normal=False, depth=False, foreground=False)
        assert np.array_equal(alb["albedo"], full["albedo"])
        with pytest.raises(F.RPError) as e:
            ds.render_aov(p, normal=False, albedo=False, depth=False, foreground=False)
        assert e.value.code == F.RP_EINVAL
        q = replace(p, shard=1, num_shards=4)
        px = int(shard_mask(q).sum())
        n = shard_slot_count(q)
        fg = torch.zeros(n, dtype=torch.float32, device="cuda")
        ctr = torch.full((F.RP_COUNTERS_LEN,), 77, dtype=torch.int64, device="cuda")  # zeroed by the call
        ds.render_aov_device(q, fg=fg, counters=ctr)
        torch.cuda.synchronize()
        assert ctr.tolist() == [3 * px, 3 * px, px, 0]
        with pytest.raises(F.RPError) as e:
            ds.render_aov_device(q, counters=ctr)
        assert e.value.code == F.RP_EINVAL


def test_asynchronous_call(gpu):
    """render_aov_device on a non-default torch stream into torch tensors: the synchronous frames after unpacking,
    and the same bytes when called again into the same buffers."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.render import unpack_shard
    from rtpotato.scene import shard_slot_count
    sc, p = aov_ref.scene_params("variants_sky", 4)
    n = shard_slot_count(p)
    with gpu.DeviceScene(sc) as ds:
        ref = ds.render_aov(p)
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            nrm = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
            alb = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
            dep = torch.zeros(n, dtype=torch.float64, device="cuda")
            fg = torch.zeros(n, dtype=torch.float32, device="cuda")
            ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
            ds.render_aov_device(p, nrm, alb, dep, fg, ctr, stream=st)
            first = [t.clone() for t in (nrm, alb, dep, fg, ctr)]
            ds.render_aov_device(p, nrm, alb, dep, fg, ctr, stream=st)
        st.synchronize()
        for a, b in zip(first, (nrm, alb, dep, fg, ctr)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert np.array_equal(unpack_shard(p, nrm.cpu().numpy(), 3), ref["normal"])
        assert np.array_equal(unpack_shard(p, alb.cpu().numpy(), 3), ref["albedo"])
        assert np.array_equal(unpack_shard(p, dep.cpu().numpy(), 1)[..., 0], ref["depth"])
        assert np.array_equal(unpack_shard(p, fg.cpu().numpy().astype(np.float64), 1)[..., 0], ref["fg"])
        assert ctr.tolist() == [4 * p.width * p.height] * 2 + [p.width * p.height, 0]


_deep = {}


def _deep_tree():
    """random_mesh(200_000) at 48 x 32, 2 spp (the setup of test_stack_overflow_is_reported) and its normal reference."""
    if not _deep:
        from rtpotato import scenes
        from rtpotato.scene import RenderParams
        sc = scenes.configure(scenes.random_mesh(200_000), 48, 32)
        p = RenderParams(48, 32, 2, 8, aov_ref.SEED, 32, 32)
        normal, fg = aov_ref.normal_ref(sc, p)
        _deep.update(scene=sc, params=p, normal=normal, fg=fg)
    return _deep


@pytest.mark.parametrize("options", [{"builder": "gpu"}, {"builder": "ploc", "node_format": "q8"}])
def test_deep_tree(gpu, options):
    r = _deep_tree()
    with gpu.DeviceScene(r["scene"], options=options) as ds:
        out = ds.render_aov(r["params"], albedo=False)
    _assert_aov_parity(out, {"normal": r["normal"], "fg": r["fg"]})


def test_stack_overflow_is_reported(gpu):
    """debug_stack_depth = 8 on a tree that needs far more: the device call leaves RP_STATUS_STACK_OVERFLOW in the
    counters, rp_render_aov returns RP_EINTERNAL (entries are dropped, never written past the stack)."""
    import torch
    from rtpotato import _ffi as F
    from rtpotato.scene import shard_slot_count
    r = _deep_tree()
    p = r["params"]
    with gpu.DeviceScene(r["scene"], options={"debug_stack_depth": 8}) as ds:
        dep = torch.zeros(shard_slot_count(p), dtype=torch.float64, device="cuda")
        ctr = torch.zeros(F.RP_COUNTERS_LEN, dtype=torch.int64, device="cuda")
        ds.render_aov_device(p, depth=dep, counters=ctr)
        torch.cuda.synchronize()
        assert int(ctr[3]) & F.RP_STATUS_STACK_OVERFLOW
        with pytest.raises(F.RPError) as e:
            ds.render_aov(p)
        assert e.value.code == F.RP_EINTERNAL and "overflow" in str(e.value)

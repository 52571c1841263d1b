"""Brute-force closest hits (test infrastructure): every ray against every root hittable with numpy, in the
reference's exact f64 expression order (hittable.rs:39-101, as tests/golden/make_golden.py PyScene.hit restates it),
vectorised over rays x primitives.  No tree and no boxes, so it is the yardstick for what a traversal may never
cull.  Exact-t ties between two hittables are flagged: which of them a tree returns is free."""
import numpy as np

SMOL = 1e-7


class Brute:
    def __init__(self, scene):
        root = scene.root
        sd = scene.scene_data
        self.tri_id = np.nonzero(root["kind"] == 1)[0]
        self.sph_id = np.nonzero(root["kind"] == 0)[0]
        tri = root[self.tri_id]
        if len(tri):
            assert len(sd.mesh_table) == 1
            m = sd.mesh_table[0]
            self.mesh = m
            idx = m.indices.reshape(-1)
            t0 = tri["triangle"].astype(np.int64)
            self.ia, self.ib, self.ic = idx[t0], idx[t0 + 1], idx[t0 + 2]
            self.A, B, C = m.positions[self.ia], m.positions[self.ib], m.positions[self.ic]
            self.ba, self.ca = self.A - B, self.A - C
        self.sph = [(np.array(h["center"], dtype=np.float64), float(h["radius"]), int(h["material"]))
                    for h in root[self.sph_id]]

    def closest(self, rays, chunk=256):
        """rays (n, 8) {o, d, t_min, t_max} -> dict of t (inf = miss), id (root index, -1), u, v (triangles), tie."""
        n = len(rays)
        out = {"t": np.full(n, np.inf), "id": np.full(n, -1, dtype=np.int64), "u": np.zeros(n), "v": np.zeros(n),
               "tie": np.zeros(n, dtype=bool)}
        for s in range(0, n, chunk):
            r = rays[s:s + chunk]
            o, d, tmin, tmax = r[:, 0:3], r[:, 3:6], r[:, 6:7], r[:, 7:8]
            T, ids, U, V = [], [], [], []
            if len(self.tri_id):
                ba, ca = self.ba[None], self.ca[None]
                pa = self.A[None] - o[:, None, :]
                dx, dy, dz = d[:, 0:1], d[:, 1:2], d[:, 2:3]
                det = (ba[..., 0] * ca[..., 1] * dz + ba[..., 1] * ca[..., 2] * dx + ba[..., 2] * ca[..., 0] * dy
                       - ba[..., 0] * ca[..., 2] * dy - ba[..., 1] * ca[..., 0] * dz - ba[..., 2] * ca[..., 1] * dx)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    inv = 1.0 / det
                    t = (pa[..., 0] * (ba[..., 1] * ca[..., 2] - ba[..., 2] * ca[..., 1])
                         + pa[..., 1] * (ba[..., 2] * ca[..., 0] - ba[..., 0] * ca[..., 2])
                         + pa[..., 2] * (ba[..., 0] * ca[..., 1] - ba[..., 1] * ca[..., 0])) * inv
                    u = (pa[..., 0] * (ca[..., 1] * dz - ca[..., 2] * dy)
                         + pa[..., 1] * (ca[..., 2] * dx - ca[..., 0] * dz)
                         + pa[..., 2] * (ca[..., 0] * dy - ca[..., 1] * dx)) * inv
                    v = (pa[..., 0] * (ba[..., 2] * dy - ba[..., 1] * dz)
                         + pa[..., 1] * (ba[..., 0] * dz - ba[..., 2] * dx)
                         + pa[..., 2] * (ba[..., 1] * dx - ba[..., 0] * dy)) * inv
                    w = 1.0 - u - v
                    ok = (~(np.abs(det) < SMOL) & ~(t < tmin) & ~(t > tmax) & ~(u < 0.0) & ~(v < 0.0) & ~(w < 0.0)
                          & ~np.isnan(t))
                T.append(np.where(ok, t, np.inf))
                U.append(u)
                V.append(v)
                ids.append(self.tri_id)
            for k, (c, rad, _) in enumerate(self.sph):
                tc = o - c[None]
                a = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                hb = (d[:, 0] * tc[:, 0] + d[:, 1] * tc[:, 1]) + d[:, 2] * tc[:, 2]
                cq = ((tc[:, 0] * tc[:, 0] + tc[:, 1] * tc[:, 1]) + tc[:, 2] * tc[:, 2]) - rad * rad
                delta = hb * hb - a * cq
                with np.errstate(invalid="ignore", divide="ignore"):
                    sq = np.sqrt(np.where(delta > 0.0, delta, 0.0))
                    t1, t2 = (-hb - sq) / a, (-hb + sq) / a
                lo, hi = tmin[:, 0], tmax[:, 0]
                in1 = ~(t1 < lo) & ~(t1 > hi)
                in2 = ~(t2 < lo) & ~(t2 > hi)
                ts = np.where(delta > 0.0, np.where(in1, t1, np.where(in2, t2, np.inf)), np.inf)
                T.append(ts[:, None])
                U.append(np.zeros((len(r), 1)))
                V.append(np.zeros((len(r), 1)))
                ids.append(self.sph_id[k:k + 1])
            if not T:
                continue
            T, U, V, ids = np.concatenate(T, axis=1), np.concatenate(U, axis=1), np.concatenate(V, axis=1), np.concatenate(ids)
            j = np.argmin(T, axis=1)
            rows = np.arange(len(r))
            best = T[rows, j]
            hit = np.isfinite(best)
            out["t"][s:s + chunk] = best
            out["id"][s:s + chunk] = np.where(hit, ids[j], -1)
            out["u"][s:s + chunk] = np.where(hit, U[rows, j], 0.0)
            out["v"][s:s + chunk] = np.where(hit, V[rows, j], 0.0)
            out["tie"][s:s + chunk] = hit & ((T == best[:, None]).sum(axis=1) > 1)
        return out

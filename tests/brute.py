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
            # per triangle: its mesh, and the corners' positions, normals and uvs out of that mesh's own arrays
            self.tri_mesh = tri["mesh"].astype(np.int64)
            t0 = tri["triangle"].astype(np.int64)
            n = len(tri)
            corner = np.zeros((3, n), dtype=np.int64)
            pos, self.nrm, self.uv = np.zeros((3, n, 3)), np.zeros((3, n, 3)), np.zeros((3, n, 2))
            self.tri_mat = np.zeros(n, dtype=np.uint32)
            for mi, m in enumerate(sd.mesh_table):
                of = self.tri_mesh == mi
                idx = m.indices.reshape(-1)
                for c in range(3):
                    corner[c, of] = idx[t0[of] + c]
                    pos[c, of], self.nrm[c, of], self.uv[c, of] = (m.positions[corner[c, of]], m.normals[corner[c, of]],
                                                                   m.uvs[corner[c, of]])
                self.tri_mat[of] = m.material
            self.ia, self.ib, self.ic = corner  # vertex indices within each triangle's own mesh
            if len(sd.mesh_table) == 1:
                self.mesh = sd.mesh_table[0]
            self.A, B, C = pos
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

    def records(self, rays, ref):
        """The reference's Hit records of closest()'s result `ref`: (rec (n, 9) {t, position, normal, uv}, material
        (n,) u32 -- 0xFFFFFFFF on a miss --, is_tri (n,) bool), recomputed from (hittable, t, u, v) in the reference's
        expression order (hittable.rs:54-62, 95-107), every triangle out of its own mesh."""
        n = len(rays)
        o, d, t = rays[:, 0:3], rays[:, 3:6], ref["t"]
        hit = ref["id"] >= 0
        rec = np.zeros((n, 9))
        rec[:, 0] = np.where(hit, t, np.inf)
        mats = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
        with np.errstate(invalid="ignore", over="ignore"):
            p = o + t[:, None] * d
        is_tri = hit & np.isin(ref["id"], self.tri_id)
        if is_tri.any():
            k = np.searchsorted(self.tri_id, np.where(is_tri, ref["id"], self.tri_id[0]))
            u, v = ref["u"][:, None], ref["v"][:, None]
            w = 1.0 - u - v
            nt = (w * self.nrm[0][k] + u * self.nrm[1][k]) + v * self.nrm[2][k]
            uvt = (w * self.uv[0][k] + u * self.uv[1][k]) + v * self.uv[2][k]
            rec[is_tri, 1:4], rec[is_tri, 4:7], rec[is_tri, 7:9] = p[is_tri], nt[is_tri], uvt[is_tri]
            mats[is_tri] = self.tri_mat[k][is_tri]
        for q, (c, rad, mat) in enumerate(self.sph):
            s = hit & (ref["id"] == self.sph_id[q])
            pc = p[s] - c[None]
            ns = pc / np.sqrt((pc[:, 0] * pc[:, 0] + pc[:, 1] * pc[:, 1]) + pc[:, 2] * pc[:, 2])[:, None]
            rec[s, 1:4], rec[s, 4:7] = p[s], ns
            rec[s, 7] = 0.5 - np.arctan2(ns[:, 2], ns[:, 0]) / (2.0 * np.pi)
            rec[s, 8] = np.arcsin(ns[:, 1]) / np.pi + 0.5
            mats[s] = mat
        return rec, mats, is_tri

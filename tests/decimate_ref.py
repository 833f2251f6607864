"""A numpy restatement of the mesh decimation contract (include/nerfhip.h) for tests/test_decimate_host.py and
tests/test_gpu_decimate.py, with the welded cube fixture and two mesh measures.  Steps 1-4, 6 and 7 are restated in the contract's
own arithmetic (fp32 quantisation with numpy float32 operations, fp64 sums in ascending index: np.add.at and np.bincount accumulate
in index order); step 5 is restated with np.linalg.solve.  Nothing here imports the package."""
import functools

import numpy as np

COUNTS = ("clusters", "bad", "collapsed", "duplicate", "unreferenced")


def decimate(vertices, triangles, colors=None, cell=1.0, placement="mean", origin=None, eps=1e-3):
    """-> dict: vertices (V', 3) float32, triangles (T', 3) int32, colors (V', 3) uint8 or None, cluster_of (V,) int32, counts
    (dict of COUNTS), and for the tests: exact (V', 3) float64, the positions before the one rounding; box (V', 2, 3) float64, the
    cells' [blo, bhi]; clamped, the number of clusters (referenced or not) the quadric placement had to clamp."""
    v, t = np.asarray(vertices, np.float32), np.asarray(triangles, np.int32)
    V, T = len(v), len(t)
    cell = np.float32(cell)
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError("cell must be > 0 and finite")
    if colors is not None and np.shape(colors) != (V, 3):
        raise ValueError("colours must be (V, 3)")
    out = {"vertices": np.zeros((0, 3), np.float32), "triangles": np.zeros((0, 3), np.int32),
           "colors": None if colors is None else np.zeros((0, 3), np.uint8), "cluster_of": np.full(V, -1, np.int32),
           "counts": dict.fromkeys(COUNTS, 0), "exact": np.zeros((0, 3)), "box": np.zeros((0, 2, 3)), "clamped": 0}
    if V == 0 or T == 0:
        return out
    finite = np.isfinite(v).all(1)
    if not finite.any():
        out["counts"]["bad"] = T
        return out
    ids = np.flatnonzero(finite)
    v_lo = v[ids].min(0)
    lo = v_lo if origin is None else np.asarray(origin, np.float32)
    if (v_lo < lo).any():
        raise ValueError("a vertex lies below the origin")
    with np.errstate(all="ignore"):
        q = np.floor((v[ids] - lo) / cell)                       # float32 throughout
    if not np.isfinite(q).all():
        raise ValueError("cell too small for this mesh")
    R = [int(x) + 1 for x in q.max(0)]
    if R[0] * R[1] * R[2] >= 1 << 31:
        raise ValueError("cell too small for this mesh")
    qi = q.astype(np.int64)
    c = (qi[:, 0] * R[1] + qi[:, 1]) * R[2] + qi[:, 2]
    cells, inv = np.unique(c, return_inverse=True)               # the non-empty cells in ascending c
    inv = inv.reshape(-1)
    C = len(cells)
    cluster_of = np.full(V, -1, np.int64)
    cluster_of[ids] = inv
    # 4: the mean, members in ascending vertex number
    n = np.bincount(inv, minlength=C)
    s = np.zeros((C, 3))
    np.add.at(s, inv, v[ids].astype(np.float64))
    m = s / n[:, None]
    col = None
    if colors is not None:
        cs = np.zeros((C, 3), np.int64)
        np.add.at(cs, inv, np.asarray(colors, np.uint8)[ids].astype(np.int64))
        col = ((2 * cs + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    # 1: good triangles
    inside = ((t >= 0) & (t < V)).all(1)
    good = inside.copy()
    good[inside] = (cluster_of[t[inside]] >= 0).all(1)
    gt = np.flatnonzero(good)
    qc = np.stack([cells // (R[1] * R[2]), (cells // R[2]) % R[1], cells % R[2]], 1)
    blo = lo.astype(np.float64) + qc * np.float64(cell)
    bhi = blo + np.float64(cell)
    clamped = 0
    if placement == "quadric":
        p = v[t[gt]].astype(np.float64)
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        A, b = np.zeros((C, 3, 3)), np.zeros((C, 3))
        for k in range(3):
            cl = cluster_of[t[gt, k]]
            d = -np.einsum("ij,ij->i", nrm, p[:, 0] - m[cl])
            np.add.at(A, cl, nrm[:, :, None] * nrm[:, None, :])
            np.add.at(b, cl, d[:, None] * nrm)
        trace = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
        ok = np.isfinite(trace) & (trace > 0)
        x = np.zeros((C, 3))
        if ok.any():
            x[ok] = np.linalg.solve(A[ok] + (eps * trace[ok])[:, None, None] * np.eye(3), -b[ok][:, :, None])[:, :, 0]
        x[~np.isfinite(x).all(1)] = 0.0
        y = m + x
        clamped = int(((y < blo) | (y > bhi)).any(1).sum())
        exact = np.clip(y, blo, bhi)
    elif placement == "mean":
        exact = m
    else:
        raise ValueError("placement must be 'mean' or 'quadric'")
    # 6: remap, collapsed, duplicates
    r = cluster_of[t[gt]]
    collapsed = (r[:, 0] == r[:, 1]) | (r[:, 1] == r[:, 2]) | (r[:, 0] == r[:, 2])
    rc = r[~collapsed]
    rot = rc[np.arange(len(rc))[:, None], (rc.argmin(1)[:, None] + np.arange(3)) % 3]
    first = np.sort(np.unique(rot, axis=0, return_index=True)[1]) if len(rc) else np.zeros(0, np.int64)    # the lowest input index of each
    tri = rc[first]
    # 7: unreferenced clusters
    used = np.unique(tri)
    vnew = np.full(C, -1, np.int64)
    vnew[used] = np.arange(len(used))
    out.update(vertices=exact[used].astype(np.float32), triangles=vnew[tri].astype(np.int32).reshape(-1, 3),
               colors=None if col is None else col[used],
               cluster_of=np.where(cluster_of >= 0, vnew[np.maximum(cluster_of, 0)], -1).astype(np.int32),
               counts=dict(zip(COUNTS, (C, T - len(gt), int(collapsed.sum()), len(rc) - len(first), C - len(used)))),
               exact=exact[used], box=np.stack([blo[used], bhi[used]], 1), clamped=clamped)
    return out


@functools.lru_cache(maxsize=None)
def cube(n):
    """(vertices float32, triangles int32): the surface of [-1, 1]^3 with n x n quads per face, welded, outward winding"""
    index, verts, tris = {}, [], []

    def vid(ijk):
        if ijk not in index:
            index[ijk] = len(verts)
            verts.append([-1.0 + 2.0 * x / n for x in ijk])
        return index[ijk]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3                           # e_b x e_c = e_a
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        ijk = [0, 0, 0]
                        ijk[a], ijk[b], ijk[c] = side, i + di, j + dj
                        return vid(tuple(ijk))
                    quad = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]
                    if side == 0:
                        quad.reverse()
                    tris += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.array(verts, np.float64).astype(np.float32), np.array(tris, np.int32)


def signed_volume(vertices, triangles):
    p = np.asarray(vertices, np.float64)[np.asarray(triangles)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def open_edges(triangles):
    """edges not shared by exactly two triangles"""
    t = np.asarray(triangles).reshape(-1, 3)
    if not len(t):
        return 0
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
    return int((np.unique(e, axis=0, return_counts=True)[1] != 2).sum())


# ---------------------------------------------------------------------------------------------------------------------- the cases
CELLS = (0.5, 0.25, 0.05)
PLACEMENTS = ("mean", "quadric")


def fixtures():
    """{name: (vertices, triangles)}: every mesh of mesh_ref.meshes() and the cubes"""
    import mesh_ref
    out = dict(mesh_ref.meshes())
    out["cube10"], out["cube12"] = cube(10), cube(12)
    return out


def colors_for(vertices):
    """seeded random uint8 colours, one per vertex"""
    return np.random.default_rng(77 + len(vertices)).integers(0, 256, (len(vertices), 3), dtype=np.uint8)


def cases():
    """[(name, cell, placement, origin, with colours)]: every fixture at CELLS with both placements and seeded colours, then the
    cases that take a path of their own — no colours, an origin, a cell larger than the mesh, the cell that puts the cube's +1
    faces on a cell boundary, the cell of the placement comparison"""
    out = [(name, cell, placement, None, True) for name in sorted(fixtures()) for cell in CELLS for placement in PLACEMENTS]
    for placement in PLACEMENTS:
        out += [("soup257", 0.25, placement, None, False), ("ico2", 0.25, placement, (-1.5, -1.25, -2.0), True),
                ("ico2", 10.0, placement, None, True), ("cube12", 0.4, placement, None, True), ("cube10", 0.37, placement, None, False)]
    return out


_REFERENCE = {}


def reference(case):
    """decimate() of a case, computed once and left unchanged"""
    if case not in _REFERENCE:
        name, cell, placement, origin, with_colors = case
        v, t = fixtures()[name]
        _REFERENCE[case] = decimate(v, t, colors_for(v) if with_colors else None, cell, placement, origin)
    return _REFERENCE[case]


def big_soup(T=100000):
    """a seeded soup of T small triangles (3 T vertices) in [-1, 1]^3, edges up to 0.04 per axis: at cell 0.02 it leaves more
    than 65,536 clusters"""
    rng = np.random.default_rng(4242)
    c = rng.uniform(-1, 1, (T, 1, 3))
    v = (c + rng.uniform(-0.02, 0.02, (T, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * T, dtype=np.int32).reshape(T, 3)

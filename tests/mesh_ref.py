"""Fixtures and numpy references of the mesh ray caster (csrc/mesh_core.h) for tests/test_meshcast_host.py and
tests/test_gpu_meshcast.py: the meshes and ray sets, the hierarchy's format restated in numpy, a float64 brute-force caster
(Moller-Trumbore, two-sided) with the rule that says which rays it cannot judge, and float64 restatements of shade and compose.
Nothing here imports the package."""
import functools

import numpy as np

CAMERA = (0.37, -0.21, 4.0)          # off-axis on purpose: an on-axis camera puts 2 % of the rays exactly on icosphere edges
SOUP_SIZES = (1, 4, 5, 32, 33, 257, 1000)


# ------------------------------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def icosphere(level):
    """(vertices (V, 3) float32 on the unit sphere, triangles (T, 3) int32, outward winding): 20 * 4^level triangles."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v, np.float64).astype(np.float32), np.array(f, np.int32)


def icosphere_edges(level):
    """(E, 2) vertex pairs"""
    _, t = icosphere(level)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    return np.unique(np.sort(e, 1), axis=0)


@functools.lru_cache(maxsize=None)
def soup(T):
    """T seeded triangles of their own three vertices, centres in [-1, 1]^3, edges up to 0.6 long per axis"""
    rng = np.random.default_rng(1000 + T)
    c = rng.uniform(-1, 1, (T, 1, 3))
    v = (c + rng.uniform(-0.3, 0.3, (T, 3, 3))).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * T, dtype=np.int32).reshape(T, 3)


@functools.lru_cache(maxsize=None)
def plate():
    """an axis-aligned 4 x 4 quad grid over [-1, 1]^2 in the plane z = 0.5: every box has zero thickness"""
    g = np.linspace(-1, 1, 5)
    v = np.array([(x, y, 0.5) for y in g for x in g], np.float32)
    t = []
    for j in range(4):
        for i in range(4):
            a = 5 * j + i
            t += [(a, a + 1, a + 6), (a, a + 6, a + 5)]
    return v, np.array(t, np.int32)


@functools.lru_cache(maxsize=None)
def identical(T=37):
    """T copies of one triangle: all keys equal but for the index"""
    v = np.array([(-0.9, -0.7, 0.1), (1.1, -0.6, -0.2), (0.2, 1.0, 0.3)], np.float32)
    return v, np.tile(np.array([[0, 1, 2]], np.int32), (T, 1))


@functools.lru_cache(maxsize=None)
def flawed():
    """the level-2 icosphere with degenerate triangles (a repeated vertex), out-of-range indices and a NaN vertex: returns
    (vertices, triangles, bad (T,) bool)"""
    v, t = icosphere(2)
    v, t = v.copy(), t.copy()
    t[3, 1] = t[3, 0]                       # degenerate, but good
    t[100] = (7, 7, 7)
    t[17, 2] = len(v)                       # one past the end
    t[200, 0] = -1
    t[201, 1] = np.iinfo(np.int32).max
    v[40, 1] = np.nan
    v[41, 0] = np.inf
    bad = bad_triangles(v, t)
    assert bad[[17, 200, 201]].all() and not bad[[3, 100]].any() and bad.sum() > 8
    return v, t, bad


def bad_triangles(v, t):
    inside = ((t >= 0) & (t < len(v))).all(1)
    ok = inside.copy()
    ok[inside] = np.isfinite(v[t[inside]]).all((1, 2))
    return ~ok


def meshes():
    """{name: (vertices, triangles)} of every CPU fixture"""
    out = {"ico%d" % k: icosphere(k) for k in range(4)}
    out.update({"soup%d" % T: soup(T) for T in SOUP_SIZES})
    out["plate"] = plate()
    out["identical"] = identical()
    out["flawed"] = flawed()[:2]
    return out


# -------------------------------------------------------------------------------------------------------------------------- rays
def _rows(o, d, near, far):
    o, d = np.broadcast_arrays(np.asarray(o, np.float32), np.asarray(d, np.float32))
    r = np.zeros((len(o), 8), np.float32)
    r[:, :3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, near, far
    return r


def pinhole(near=0.0, far=100.0, wh=32, focal=40.0):
    """a wh x wh image from CAMERA looking down -z; directions of length > 1 (not normalised)"""
    j, i = np.meshgrid(np.arange(wh), np.arange(wh), indexing="ij")
    d = np.stack([(i - wh / 2 + 0.5) / focal, -(j - wh / 2 + 0.5) / focal, -np.ones_like(i, float)], -1).reshape(-1, 3)
    return _rows(np.array(CAMERA)[None], d, near, far)


def axis_rays(on_grid):
    """axis-parallel rays along each axis in both senses, the two other components zeros of both signs; the origins on the
    lattice of quarters (on_grid: through vertices and edges of the plate and of soup boxes) or off it"""
    rows = []
    s = np.arange(-1.25, 1.3, 0.25) if on_grid else 0.137 + 0.23 * np.arange(-5, 5)
    a, b = [x.ravel() for x in np.meshgrid(s, s if on_grid else s + 0.0371)]     # off the grid: off the plate's diagonals too
    k = 0
    for ax in range(3):
        for sense in (1.0, -1.0):
            o = np.zeros((len(a), 3))
            o[:, ax] = -3.0 * sense
            o[:, (ax + 1) % 3], o[:, (ax + 2) % 3] = a, b
            d = np.zeros((len(a), 3), np.float32)
            d[:, ax] = sense * (0.5 + ax)
            d[:, (ax + 1) % 3] = np.where((np.arange(len(a)) + k) & 1, 0.0, -0.0)
            d[:, (ax + 2) % 3] = np.where((np.arange(len(a)) + k) & 2, 0.0, -0.0)
            rows.append(_rows(o, d, 0.0, 50.0))
            k += 1
    return np.concatenate(rows)


def inplane_rays():
    """rays lying in the plate's plane z = 0.5, and others grazing it"""
    y = np.linspace(-1.2, 1.2, 25)
    o = np.stack([np.full_like(y, -2.0), y, np.full_like(y, 0.5)], 1)
    flat = _rows(o, np.array([[1.0, 0.125, 0.0]]), 0.0, 10.0)
    flat2 = _rows(o[:, [1, 0, 2]], np.array([[-0.0, 1.0, -0.0]]), 0.0, 10.0)
    graze = _rows(o, np.array([[1.0, 0.125, 2.0 ** -20]]), 0.0, 10.0)
    return np.concatenate([flat, flat2, graze])


def inside_rays(n=400):
    """rays from points near the centre in seeded directions of every length from 1e-3 to 1e3"""
    rng = np.random.default_rng(5)
    d = rng.normal(size=(n, 3))
    d *= (10.0 ** rng.uniform(-3, 3, (n, 1))) / np.linalg.norm(d, axis=1, keepdims=True)
    return _rows(rng.uniform(-0.05, 0.05, (n, 3)), d, 0.0, 1e6)


def nonfinite_rays():
    r = pinhole()[:40].copy()
    for k in range(8):
        r[k, k] = np.nan
        r[8 + k, k] = np.inf
        r[16 + k, k] = -np.inf
    r[24, 3:6] = 0.0
    r[25, 3:6] = -0.0
    r[26, 3:6] = (0.0, -0.0, 0.0)
    return r


def ray_sets():
    """{name: rays (n, 8)}.  `window_near` and `window_far` cut off the unit sphere's first hit (t about 3) and keep or lose the
    second (t about 5); the sets after `window_far` go through edges and vertices, or hit nothing, on purpose: they are compared
    between casters, not judged by the float64 reference."""
    return {"pinhole": pinhole(), "axis": axis_rays(False), "inside": inside_rays(), "window_near": pinhole(near=3.9),
            "window_far": pinhole(far=3.6), "grid": axis_rays(True), "inplane": inplane_rays(), "nonfinite": nonfinite_rays()}


JUDGED = ("pinhole", "axis", "inside", "window_near", "window_far")


def watertight_rays(level=2):
    """from the centre of the icosphere at every vertex and every edge midpoint, directions rounded to fp32: 162 + 480 = 642"""
    v, _ = icosphere(level)
    e = icosphere_edges(level)
    v64 = v.astype(np.float64)
    d = np.concatenate([v64, 0.5 * (v64[e[:, 0]] + v64[e[:, 1]])])
    return _rows(np.zeros((1, 3)), d.astype(np.float32), 0.0, 10.0)


# ----------------------------------------------------------------------------------------------------- the format, in numpy
def levels(T):
    out, off, n = [], 0, (T + 3) // 4
    while n:
        out.append((off, n))
        off += n
        n = (n + 7) // 8 if n > 1 else 0
    return out


def _spread10(q):
    q = q.astype(np.uint64)
    out = np.zeros_like(q)
    for b in range(10):
        out |= ((q >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def build(v, t):
    """(order (T,) int32, boxes (n_nodes, 6) float32, n_bad) by the rules of include/nerfhip.h, in numpy's float32"""
    v, t = np.asarray(v, np.float32), np.asarray(t, np.int32)
    T = len(t)
    bad = bad_triangles(v, t)
    p = np.zeros((T, 3, 3), np.float32)
    p[~bad] = v[t[~bad]]
    morton = np.full(T, 1 << 30, np.uint64)
    if (~bad).any():
        lo, hi = p[~bad].min((0, 1)), p[~bad].max((0, 1))
        with np.errstate(all="ignore"):
            c = ((p[:, 0] + p[:, 1]) + p[:, 2]) / np.float32(3)
            ext = hi - lo
            x = np.where(ext > 0, ((c - lo) / ext) * np.float32(1024), np.float32(0)).astype(np.float32)
        q = np.where(x >= 1023, 1023, np.where(x > 0, np.floor(x), 0)).astype(np.uint64)
        m = (_spread10(q[:, 0]) << np.uint64(2)) | (_spread10(q[:, 1]) << np.uint64(1)) | _spread10(q[:, 2])
        morton[~bad] = m[~bad]
    keys = (morton << np.uint64(32)) | np.arange(T, dtype=np.uint64)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    lv = levels(T)
    n_nodes = lv[-1][0] + lv[-1][1] if lv else 0
    boxes = np.zeros((n_nodes, 6), np.float32)
    boxes[:, :3], boxes[:, 3:] = np.inf, -np.inf
    for j in range(lv[0][1] if lv else 0):
        ids = [i for i in order[4 * j:4 * j + 4] if not bad[i]]
        if ids:
            boxes[j, :3], boxes[j, 3:] = p[ids].min((0, 1)), p[ids].max((0, 1))
    for (off, n), (coff, cn) in zip(lv[1:], lv[:-1]):
        for i in range(n):
            ch = boxes[coff + 8 * i:coff + min(8 * i + 8, cn)]
            boxes[off + i, :3], boxes[off + i, 3:] = ch[:, :3].min(0), ch[:, 3:].max(0)
    return order, boxes, int(bad.sum())


# ------------------------------------------------------------------------------------------------- the float64 caster
def cast64(v, t, rays, chunk=256):
    """Brute force in float64 (Moller-Trumbore, two-sided, bad triangles left out): dict of tri (n,) (-1: miss), t, b1, b2 and
    `unsure` (n,) bool — the rays this reference cannot judge: some triangle whose plane the ray meets in front of it, within
    [near, far], has a barycentric within 1e-4 of 0 while the other two are above -1e-4 (the ray passes an edge or a vertex), or
    the two nearest hits are within 1e-5 relative of each other.  Rays with a non-finite column or a zero direction miss."""
    v64 = np.asarray(v, np.float64)
    t = np.asarray(t)
    good = ~bad_triangles(np.asarray(v, np.float32), t)
    ids = np.flatnonzero(good)
    p = v64[t[ids]]                                             # (G, 3, 3)
    rays = np.asarray(rays, np.float64)
    n = len(rays)
    out = {"tri": np.full(n, -1, np.int64), "t": np.zeros(n), "b1": np.zeros(n), "b2": np.zeros(n), "unsure": np.zeros(n, bool)}
    valid = np.isfinite(rays).all(1) & (rays[:, 3:6] != 0).any(1)
    if not len(ids):
        return out
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    for s in range(0, n, chunk):
        r = rays[s:s + chunk]
        o, d, near, far = r[:, None, :3], r[:, None, 3:6], r[:, None, 6], r[:, None, 7]
        with np.errstate(all="ignore"):
            pv = np.cross(d, e2[None])
            det = (e1[None] * pv).sum(-1)
            tv = o - p[None, :, 0]
            u = (tv * pv).sum(-1) / det
            qv = np.cross(tv, e1[None])
            w = (d * qv).sum(-1) / det
            tt = (e2[None] * qv).sum(-1) / det
            b0 = 1.0 - u - w
            lo = np.minimum(np.minimum(u, w), b0)
            front = np.isfinite(tt) & (det != 0) & (tt >= near) & (tt <= far) & valid[s:s + chunk, None]
            hit = front & (lo >= 0)
            edge = front & (lo > -1e-4) & (lo < 1e-4)
        th = np.where(hit, tt, np.inf)
        k = th.argmin(1)
        rows = np.arange(len(r))
        any_hit = hit[rows, k]
        out["tri"][s:s + chunk] = np.where(any_hit, ids[k], -1)
        for name, arr in (("t", tt), ("b1", u), ("b2", w)):
            out[name][s:s + chunk] = np.where(any_hit, arr[rows, k], 0.0)
        unsure = edge.any(1)
        if th.shape[1] > 1:
            two = np.partition(th, 1, axis=1)[:, :2]
            with np.errstate(all="ignore"):
                unsure |= np.isfinite(two[:, 1]) & (two[:, 1] - two[:, 0] <= 1e-5 * np.abs(two[:, 1]))
        out["unsure"][s:s + chunk] = unsure
    return out


# ------------------------------------------------------------------------------------------- shade and compose, in float64
def shade64(rays, tri, b1, b2, v, t, colors, ambient, background):
    rays, v64 = np.asarray(rays, np.float64), np.asarray(v, np.float64)
    n = len(rays)
    rgb = np.full((n, 3), float(background))
    hit = np.flatnonzero(np.asarray(tri) >= 0)
    ids = np.asarray(t)[np.asarray(tri)[hit]]
    p = v64[ids]
    nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    d = rays[hit, 3:6]
    with np.errstate(all="ignore"):
        cosine = np.abs((nrm * d).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d, axis=1))
    cosine = np.where(np.isfinite(cosine), np.minimum(cosine, 1.0), 0.0)
    c = np.ones((len(hit), 3, 3)) if colors is None else np.asarray(colors, np.float64)[ids] / 255.0
    w1, w2 = np.asarray(b1, np.float64)[hit], np.asarray(b2, np.float64)[hit]
    w = np.stack([1.0 - w1 - w2, w1, w2], 1)
    rgb[hit] = (w[:, :, None] * c).sum(1) * (ambient + (1.0 - ambient) * cosine)[:, None]
    return rgb


def compose64(mode, rgb_n, depth_n, opacity_n, tri, t, rgb_m, tau, background):
    """(rgb, depth, opacity, mask) of include/nerfhip.h's mixed_compose; the comparisons on the fp32 inputs as given"""
    rgb_n32, depth32, op32, t32 = (np.asarray(x, np.float32) for x in (rgb_n, depth_n, opacity_n, t))
    rgb_n, depth_n, opacity_n, t, rgb_m = (np.asarray(x, np.float64) for x in (rgb_n, depth_n, opacity_n, t, rgb_m))
    hit = np.asarray(tri) >= 0
    if mode == "ztest":
        with np.errstate(all="ignore"):
            s = np.where(op32 >= np.float32(tau), (depth32 / op32).astype(np.float32), np.float32(np.inf))
        mesh = hit & (t32 < s)
        return (np.where(mesh[:, None], rgb_m, rgb_n), np.where(mesh, t, depth_n), np.where(mesh, 1.0, opacity_n), mesh.astype(np.uint8))
    rest = 1.0 - opacity_n
    rgb = rgb_n + rest[:, None] * np.where(hit[:, None], rgb_m, float(background))
    return rgb, np.where(hit, depth_n + rest * t, depth_n), np.where(hit, 1.0, opacity_n), hit.astype(np.uint8)

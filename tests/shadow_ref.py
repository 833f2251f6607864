"""Numpy restatements of the shadow units (csrc/shadow_core.h) for tests/test_shadow_host.py and
tests/test_gpu_shadow.py.  Every function takes `dt`: np.float32 restates the routines operation for operation (numpy's float32
arithmetic rounds every operation separately, and its division and square root are IEEE, so the result is the routine's in every
bit); np.float64 is the same formulas on the same fp32 inputs in double, the reference of the deviation caps.  The integer sample
sequence is exact in both.  Nothing here imports the package."""
import numpy as np

# the constants of csrc/shadow_core.h
A1, A2 = 3242174889, 2447445414          # round(2^32 / g), round(2^32 / g^2), g the plastic number (g^3 = g + 1)
HALF, SALT = 0x80000000, 0x9E3779B9
MASK = np.uint64(0xFFFFFFFF)
assert (A1, A2) == (round(2 ** 32 / 1.32471795724474602596), round(2 ** 32 / 1.32471795724474602596 ** 2))


def hash32(x):
    x = np.asarray(x, np.uint64) & MASK
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & MASK
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & MASK
    x ^= x >> np.uint64(16)
    return x


def sample_words(n, K, rotate):
    """(x, y) (n, K) uint64 below 2^32: the sequence's words of sample k of pixel i"""
    k = np.arange(K, dtype=np.uint64)
    x = np.broadcast_to((np.uint64(HALF) + k * np.uint64(A1)) & MASK, (n, K)).copy()
    y = np.broadcast_to((np.uint64(HALF) + k * np.uint64(A2)) & MASK, (n, K)).copy()
    if rotate:
        h = hash32(np.arange(n, dtype=np.uint64))
        x = (x + h[:, None]) & MASK
        y = (y + hash32(h ^ np.uint64(SALT))[:, None]) & MASK
    return x, y


def offsets(n, K, rotate, dt=np.float32):
    """(u, v) (n, K) in [-1, 1): (word >> 8) 2^-23 - 1, exact in fp32"""
    x, y = sample_words(n, K, rotate)
    return tuple((w >> np.uint64(8)).astype(dt) * dt(2.0 ** -23) - dt(1) for w in (x, y))


def _normalise(v):
    """(v / |v| where |v| is finite and > 0 — v elsewhere —, |v|, ok)"""
    with np.errstate(all="ignore"):
        length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        ok = (length > 0) & np.isfinite(length)
        out = np.where(ok[..., None], v / length[..., None], v)
    return out, length, ok


def _pixels(rays, s, kind, light, reach, dt):
    """(p, c, dist, valid) of every pixel"""
    rays32, s32 = np.asarray(rays, np.float32), np.asarray(s, np.float32)
    r, sd = rays32.astype(dt), s32.astype(dt)
    n = len(r)
    L = np.asarray(light, np.float32).astype(dt)
    valid = np.isfinite(rays32).all(1) & np.isfinite(s32) & (s32 > 0)
    with np.errstate(all="ignore"):
        p = r[:, :3] + sd[:, None] * r[:, 3:6]
    valid &= np.isfinite(p).all(1)
    if kind == "directional":
        c = np.broadcast_to(_normalise(L[None])[0], (n, 3)).copy()
        dist = np.full(n, dt(np.float32(reach)))
    else:
        with np.errstate(all="ignore"):
            c, dist, ok = _normalise(L[None] - p)
        valid &= ok
    return p, c, dist, valid, L


def shadow_rays(rays, s, kind, light, bias, reach, K=1, radius=0.0, rotate=True, tri=None, vertices=None, triangles=None, dt=np.float32):
    """(rows (n K, 8), cosine (n,), unsure (n,) bool): nerfhip_shadow_rays.  `unsure` marks the pixels whose frame hangs on a
    comparison that double and single precision may decide differently (the two smallest |c| within 1e-5 and not equal): the
    float64 reference does not judge them."""
    n = len(rays)
    radius = dt(np.float32(radius))
    p, c, dist, valid, L = _pixels(rays, s, kind, light, reach, dt)
    rows = np.zeros((n, K, 8), dt)
    unsure = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        if radius == 0:
            d = np.broadcast_to(c[:, None], (n, K, 3))
            far = np.broadcast_to(dist[:, None], (n, K))
            ok = np.broadcast_to(valid[:, None], (n, K))
        else:
            a = np.abs(c)
            axis = np.where(a[:, 0] <= a[:, 1], np.where(a[:, 0] <= a[:, 2], 0, 2), np.where(a[:, 1] <= a[:, 2], 1, 2))
            two = np.sort(a, 1)
            gap = two[:, 1] - two[:, 0]                      # an exact tie is decided alike: equal inputs, equal operations
            unsure = valid & (gap > 0) & (gap < 1e-5)
            zero = np.zeros(n, dt)
            e1 = np.stack([np.where(axis == 0, zero, np.where(axis == 1, -c[:, 2], c[:, 1])),
                           np.where(axis == 0, c[:, 2], np.where(axis == 1, zero, -c[:, 0])),
                           np.where(axis == 0, -c[:, 1], np.where(axis == 1, c[:, 0], zero))], 1)
            e1 = _normalise(e1)[0]
            e2 = np.stack([c[:, 1] * e1[:, 2] - c[:, 2] * e1[:, 1], c[:, 2] * e1[:, 0] - c[:, 0] * e1[:, 2],
                           c[:, 0] * e1[:, 1] - c[:, 1] * e1[:, 0]], 1)
            u, v = offsets(n, K, rotate, dt)
            su, sv = radius * u, radius * v
            w = su[:, :, None] * e1[:, None] + sv[:, :, None] * e2[:, None]
            d = (L[None, None] + w) - p[:, None] if kind == "point" else c[:, None] + w
            d, length, ok = _normalise(d)
            ok = ok & valid[:, None]
            far = length if kind == "point" else np.full((n, K), dt(np.float32(reach)))
        rows[..., :3] = np.broadcast_to(p[:, None], (n, K, 3))
        rows[..., 3:6] = d
        rows[..., 6] = dt(np.float32(bias))
        rows[..., 7] = far
        rows[~ok] = 0
    cosine = np.ones(n, dt)
    if tri is not None:
        cosine = _cosine(np.asarray(rays, np.float32).astype(dt), c, valid, np.asarray(tri), vertices, triangles, dt)
    return rows.reshape(n * K, 8), cosine, unsure


def _cosine(r, c, valid, tri, vertices, triangles, dt):
    v, t = np.asarray(vertices, np.float32).astype(dt), np.asarray(triangles)
    n = len(r)
    out = np.zeros(n, dt)
    out[tri < 0] = 1
    idx = np.flatnonzero((tri >= 0) & (tri < len(t)) & valid)
    ids = t[tri[idx]].astype(np.int64)
    inside = ((ids >= 0) & (ids < len(v))).all(1)
    idx, ids = idx[inside], ids[inside]
    with np.errstate(all="ignore"):
        p = v[ids]                                          # (m, 3, 3)
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        nrm = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                        e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        d, cc = r[idx, 3:6], c[idx]
        nn = (nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2]
        nd = (nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1]) + nrm[:, 2] * d[:, 2]
        nl = (nrm[:, 0] * cc[:, 0] + nrm[:, 1] * cc[:, 1]) + nrm[:, 2] * cc[:, 2]
        length = np.sqrt(nn)
        ok = (length > 0) & np.isfinite(length) & np.isfinite(nd) & np.isfinite(nl)
        nl = np.where(nd > 0, -nl, nl)
        cosine = nl / length
        cosine = np.where(cosine > 0, np.where(cosine > 1, dt(1), cosine), dt(0))
    out[idx] = np.where(ok, cosine, dt(0))
    return out


def light_compose(rgb, mask, cosine, hit, trans, ambient, strength, dt=np.float32):
    """(rgb_out (n, 3), V (n,)): nerfhip_light_compose, the sum in k order"""
    rgb, cosine = np.asarray(rgb, np.float32).astype(dt), np.asarray(cosine, np.float32).astype(dt)
    n = len(rgb)
    K = len(hit) // n if n else 1
    mesh = np.asarray(mask).astype(bool)
    open_ = np.where(np.asarray(hit).reshape(n, K) != 0, dt(0), dt(1))
    term = open_ if trans is None else np.where(mesh[:, None], open_ * np.asarray(trans, np.float32).astype(dt).reshape(n, K), open_)
    total = np.zeros(n, dt)
    for k in range(K):
        total = total + term[:, k]
    V = total / dt(K)
    ambient, strength = dt(np.float32(ambient)), dt(np.float32(strength))
    factor = np.where(mesh, ambient + ((dt(1) - ambient) * cosine) * V, dt(1) - strength * (dt(1) - V))
    return rgb * factor[:, None], V


# ---- the analytic shadow: the level-3 icosphere at (0, 0, 2) over the plane z = 0 --------------------------------------------------
SPHERE_CENTRE = (0.0, 0.0, 2.0)
BAND = (0.99, 1.001)          # the icosphere's inscribed radius is 0.9955, its largest vertex norm 1 + 4e-8: between them, no verdict


def sphere_scene(icosphere3):
    """(vertices, triangles) of the sphere plus a two-triangle ground over [-9, 9]^2; the ground's triangles are the last two"""
    v, t = icosphere3
    v = (v.astype(np.float64) + np.array(SPHERE_CENTRE)).astype(np.float32)
    g = np.array([(-9, -9, 0), (9, -9, 0), (9, 9, 0), (-9, 9, 0)], np.float32)
    return np.concatenate([v, g]), np.concatenate([t, np.array([[0, 1, 2], [0, 2, 3]], np.int32) + len(v)]).astype(np.int32)


def down_rays(wh=48):
    """wh x wh parallel rows pointing down -z from z = 5 at the cell centres of x in (-5, 3), y in (-3, 3)"""
    x = -5.0 + 8.0 * (np.arange(wh) + 0.5) / wh
    y = -3.0 + 6.0 * (np.arange(wh) + 0.5) / wh
    xx, yy = np.meshgrid(x, y)
    r = np.zeros((wh * wh, 8), np.float32)
    r[:, 0], r[:, 1], r[:, 2] = xx.ravel(), yy.ravel(), 5.0
    r[:, 5], r[:, 7] = -1.0, 100.0
    return r


def distance_to_light_path(p, kind, light):
    """(distance from the sphere's centre to the shadow ray of each point p (m, 3) — the half-line along a directional light, the
    segment to a point light —, |p - centre|), in float64"""
    p = np.asarray(p, np.float64)
    c = np.array(SPHERE_CENTRE)
    L = np.asarray(light, np.float64)
    if kind == "directional":
        d = np.broadcast_to(L / np.linalg.norm(L), p.shape)
        tmax = np.full(len(p), np.inf)
    else:
        d = L[None] - p
        tmax = np.linalg.norm(d, axis=1)
        d = d / tmax[:, None]
    tc = np.clip(((c[None] - p) * d).sum(1), 0.0, tmax)
    return np.linalg.norm(p + tc[:, None] * d - c[None], axis=1), np.linalg.norm(p - c[None], axis=1)

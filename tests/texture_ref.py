"""Numpy restatement of the per-triangle texture atlas (include/nerfhip.h, csrc/texture_core.h) for
tests/test_texture_host.py and tests/test_gpu_texture.py: the layout, the sample points, the lookup in float64, a GL-convention
bilinear sampler, and the colour field of the resolution claim.  Nothing here imports the package."""
import numpy as np

KIND_ZERO, KIND_EVEN, KIND_ODD, KIND_DIAGONAL = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------------------ layout
def n_tex(R):
    return (R + 2) * (R + 3) // 2


def sample_number(R, i, j):
    return j * (R + 2) - j * (j - 1) // 2 + i


def lattice(R):
    """(n_tex, 2) int: (i, j) of every sample, in the order of its number"""
    ij = np.array([(i, j) for j in range(R + 2) for i in range(R + 2 - j)], np.int64)
    assert len(ij) == n_tex(R) and np.array_equal(sample_number(R, ij[:, 0], ij[:, 1]), np.arange(n_tex(R)))
    return ij


def height(T, R, Wa):
    B = R + 3
    nb = Wa // B
    return B * -(-((T + 1) // 2) // nb)


def texels(T, R, Wa):
    """(T, n_tex, 2) int: texel (x, y) of every sample"""
    B, nb = R + 3, Wa // (R + 3)
    ij = lattice(R)
    t = np.arange(T, dtype=np.int64)
    k, odd = t >> 1, (t & 1).astype(bool)
    origin = np.stack([(k % nb) * B, (k // nb) * B], 1)
    local = np.where(odd[:, None, None], B - 1 - ij[None], ij[None])
    return origin[:, None, :] + local


def classify(T, R, Wa):
    """(kind (Ha, Wa), q (Ha, Wa)): what every texel of the atlas is — KIND_EVEN / KIND_ODD: the sample q of an even / odd triangle;
    KIND_DIAGONAL: nobody's, filled with the even triangle's sample q; KIND_ZERO: q = -1.  Written texel by texel from the stated
    rules, on purpose not from `texels`."""
    B, nb, Ha = R + 3, Wa // (R + 3), height(T, R, Wa)
    kind, q = np.zeros((Ha, Wa), np.int64), np.full((Ha, Wa), -1, np.int64)
    for y in range(Ha):
        for x in range(Wa):
            bx, by = x // B, y // B
            if bx >= nb:
                continue
            lx, ly, t = x % B, y % B, 2 * (by * nb + bx)
            if t >= T:
                continue
            if lx + ly <= R + 1:
                kind[y, x], q[y, x] = KIND_EVEN, t * n_tex(R) + sample_number(R, lx, ly)
            elif lx + ly == R + 2:
                i, j = (lx - 1, ly) if lx >= 1 else (0, ly - 1)
                kind[y, x], q[y, x] = KIND_DIAGONAL, t * n_tex(R) + sample_number(R, i, j)
            elif t + 1 < T:
                kind[y, x], q[y, x] = KIND_ODD, (t + 1) * n_tex(R) + sample_number(R, B - 1 - lx, B - 1 - ly)
    return kind, q


def atlas_from(colors, T, R, Wa):
    """the atlas (Ha, Wa, 3) uint8 of colours (K, 3), by `classify`"""
    _, q = classify(T, R, Wa)
    out = np.zeros(q.shape + (3,), np.uint8)
    out[q >= 0] = np.asarray(colors, np.uint8)[q[q >= 0]]
    return out


def uv(T, R, Wa):
    """(T, 3, 2) float32: texel centres of the corners (0, 0), (R, 0), (0, R), in pixels"""
    tx = texels(T, R, Wa)
    ids = [sample_number(R, 0, 0), sample_number(R, R, 0), sample_number(R, 0, R)]
    return (tx[:, ids, :] + 0.5).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ points
def bad_triangles(v, t):
    inside = ((t >= 0) & (t < len(v))).all(1)
    ok = inside.copy()
    ok[inside] = np.isfinite(v[t[inside]]).all((1, 2))
    return ~ok


def points32(v, t, R):
    """(points (K, 3) float32 by the stated fp32 operations, normals (K, 3) float64, bad (T,) bool)"""
    v, t = np.asarray(v, np.float32), np.asarray(t, np.int32)
    T, bad = len(t), bad_triangles(np.asarray(v, np.float32), np.asarray(t))
    p = np.zeros((T, 3, 3), np.float32)
    p[~bad] = v[t[~bad]]
    ij = lattice(R)
    f = np.float32
    b1, b2 = (ij[:, 0].astype(f) / f(R))[None, :, None], (ij[:, 1].astype(f) / f(R))[None, :, None]
    e1, e2 = (p[:, 1] - p[:, 0])[:, None, :], (p[:, 2] - p[:, 0])[:, None, :]
    pts = ((p[:, 0][:, None, :] + b1 * e1).astype(f) + (b2 * e2).astype(f)).astype(f)
    pts[bad] = 0
    with np.errstate(all="ignore"):
        n = np.cross(e1[:, 0].astype(np.float64), e2[:, 0].astype(np.float64))
        ln = np.sqrt((n * n).sum(1))
        unit = ~bad & np.isfinite(ln) & (ln > 0)
        nrm = np.where(unit[:, None], n / np.where(unit, ln, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
    return pts.reshape(-1, 3), np.repeat(nrm, n_tex(R), 0), bad


# ------------------------------------------------------------------------------------------------------------------------ lookup
def _fetch(atlas, R, Wa, tri, i, j):
    B, nb = R + 3, Wa // (R + 3)
    k, odd = tri >> 1, (tri & 1).astype(bool)
    x = (k % nb) * B + np.where(odd, B - 1 - i, i)
    y = (k // nb) * B + np.where(odd, B - 1 - j, j)
    # every read inside the triangle's own block
    assert ((x >= (k % nb) * B) & (x < (k % nb + 1) * B) & (y >= (k // nb) * B) & (y < (k // nb + 1) * B)).all()
    return atlas[y, x].astype(np.float64) / 255.0


def lookup64(rays, tri, b1, b2, v, t, atlas, R, filter, ambient, background):
    """rgb (n, 3) float64 of include/nerfhip.h's mesh_shade_tex: arithmetic in float64 on the fp32 inputs; what is a decision — the
    background rules, the clamp, the cell (i, j) and the nearest texel — is taken in float32 as stated."""
    rays, v64, t = np.asarray(rays, np.float64), np.asarray(v, np.float64), np.asarray(t)
    tri, f = np.asarray(tri, np.int64), np.float32
    n, T, V, Wa = len(rays), len(t), len(v), atlas.shape[1]
    rgb = np.full((n, 3), float(background))
    ok = (tri >= 0) & (tri < T)
    ok[ok] = ((t[tri[ok]] >= 0) & (t[tri[ok]] < V)).all(1)
    hit = np.flatnonzero(ok)
    if not len(hit):
        return rgb
    ids = t[tri[hit]]
    p = v64[ids]
    with np.errstate(all="ignore"):
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        d = rays[hit, 3:6]
        cosine = np.abs((nrm * d).sum(1)) / (np.linalg.norm(nrm, axis=1) * np.linalg.norm(d, axis=1))
        cosine = np.where(np.isfinite(cosine), np.minimum(cosine, 1.0), 0.0)
        fx32 = (np.asarray(b1, f)[hit] * f(R)).astype(f)
        fy32 = (np.asarray(b2, f)[hit] * f(R)).astype(f)
    fx32 = np.where(fx32 > 0, np.minimum(fx32, f(R)), f(0)).astype(f)              # a NaN gives 0
    fy32 = np.where(fy32 > 0, np.minimum(fy32, f(R)), f(0)).astype(f)
    shade = (ambient + (1.0 - ambient) * cosine)[:, None]
    if filter == "nearest":
        i, j = (fx32 + f(0.5)).astype(np.int64), (fy32 + f(0.5)).astype(np.int64)
        rgb[hit] = _fetch(atlas, R, Wa, tri[hit], i, j) * shade
        return rgb
    i, j = np.minimum(fx32.astype(np.int64), R), np.minimum(fy32.astype(np.int64), R)
    fu, fv = (fx32.astype(np.float64) - i)[:, None], (fy32.astype(np.float64) - j)[:, None]
    c = [[_fetch(atlas, R, Wa, tri[hit], i + di, j + dj) for di in (0, 1)] for dj in (0, 1)]
    rgb[hit] = ((1 - fu) * (1 - fv) * c[0][0] + fu * (1 - fv) * c[0][1] + (1 - fu) * fv * c[1][0] + fu * fv * c[1][1]) * shade
    return rgb


def gl_sample(atlas, px):
    """A standard bilinear sampler (GL convention: texel (x, y) has its centre at ((x + 0.5) / W, (y + 0.5) / H), edges clamp):
    px (n, 2) float64 pixel coordinates from the top left -> (n, 3) float64 in [0, 1]"""
    H, W = atlas.shape[:2]
    a = atlas.astype(np.float64) / 255.0
    s = np.asarray(px, np.float64) - 0.5
    x0, y0 = np.floor(s[:, 0]).astype(np.int64), np.floor(s[:, 1]).astype(np.int64)
    fu, fv = (s[:, 0] - x0)[:, None], (s[:, 1] - y0)[:, None]
    cx = lambda x: np.clip(x, 0, W - 1)
    cy = lambda y: np.clip(y, 0, H - 1)
    return ((1 - fu) * (1 - fv) * a[cy(y0), cx(x0)] + fu * (1 - fv) * a[cy(y0), cx(x0 + 1)] + (1 - fu) * fv * a[cy(y0 + 1), cx(x0)]
            + fu * fv * a[cy(y0 + 1), cx(x0 + 1)])


def interpolate_uv(corner_uv, tri, b1, b2):
    """(n, 2) float64: the corners' uv (T, 3, 2) blended with the hit's barycentrics"""
    c = np.asarray(corner_uv, np.float64)[tri]
    w1, w2 = np.asarray(b1, np.float64)[:, None], np.asarray(b2, np.float64)[:, None]
    return (1.0 - w1 - w2) * c[:, 0] + w1 * c[:, 1] + w2 * c[:, 2]


# ------------------------------------------------------------------------------------------------------- the resolution claim
def field(p):
    """the colour field 0.5 + 0.5 sin(12 p + (0, 1, 2)) in float64, (n, 3) -> (n, 3)"""
    return 0.5 + 0.5 * np.sin(12.0 * np.asarray(p, np.float64) + np.array([0.0, 1.0, 2.0]))


def to_bytes(c):
    """rounded to nearest"""
    return np.clip(np.floor(np.asarray(c, np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)


def hit_points(v, t, tri, b1, b2):
    p = np.asarray(v, np.float64)[np.asarray(t)[tri]]
    w1, w2 = np.asarray(b1, np.float64)[:, None], np.asarray(b2, np.float64)[:, None]
    return (1.0 - w1 - w2) * p[:, 0] + w1 * p[:, 1] + w2 * p[:, 2]


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 10.0 * np.log10(1.0 / mse)

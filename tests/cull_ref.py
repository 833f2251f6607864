"""fp64 numpy oracle and fixtures for the occupancy grid and the ray cull (csrc/occupancy.hip, occupancy_core.h).

The ray oracle is deliberately not a DDA: it slab-intersects EVERY occupied cell box against every ray in float64, so it shares
nothing with the kernel's traversal.  It evaluates the boxes twice, inflated and shrunk by

    eps = 2^-18 * S,   S = the largest coordinate magnitude among the ranges, o and o + far * d   (per ray)

which is 64 fp32 ulps of the largest coordinate involved: the fp32 expressions (p - o) / d and o + t * d carry about four
roundings of relative size 2^-24 at that magnitude (the plane lo + i h, the difference, the quotient, the product-sum), so 64
ulps is a 16x margin.  It is derived, not tuned.  A ray that pierces a shrunk box inside [near, far] MUST be a hit; one that
pierces no inflated box must be a miss; in between either verdict is right.
"""
import itertools

import numpy as np

EPS_REL = 2.0 ** -18


# ---------------------------------------------------------------------------------------------- cell rule, dilation, bit layout
def cells_from_sigma(sigma, threshold):
    """(N, N, N) [iy, ix, iz] -> (M, M, M) bool: a cell is occupied iff one of its 8 corners is > threshold or NaN."""
    s = np.asarray(sigma, np.float32)
    above = ~(s <= np.float32(threshold))                 # True for NaN
    M = s.shape[0] - 1
    occ = np.zeros((M, M, M), bool)
    for a, b, c in itertools.product((0, 1), repeat=3):
        occ |= above[a:a + M, b:b + M, c:c + M]
    return occ


def dilate(occ, r):
    """Chebyshev dilation by r cells, clipped at the boundary: separable, one OR of shifted copies per axis."""
    out = np.asarray(occ, bool).copy()
    M = out.shape[0]
    r = min(int(r), M)
    for axis in range(3):
        src = out.copy()
        for k in range(1, r + 1):
            if k >= M:
                break
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, M - k), slice(k, M)
            out[tuple(lo)] |= src[tuple(hi)]
            out[tuple(hi)] |= src[tuple(lo)]
    return out


def dilate_brute(occ, r):
    """The definition itself: a cell is set iff an occupied cell lies within Chebyshev distance r of it."""
    occ = np.asarray(occ, bool)
    M = occ.shape[0]
    pts = np.argwhere(occ).astype(np.int32)
    out = np.zeros(occ.shape, bool)
    if not len(pts):
        return out
    cells = np.stack(np.meshgrid(*[np.arange(M, dtype=np.int32)] * 3, indexing="ij"), -1).reshape(-1, 3)
    flat = out.reshape(-1)
    for k in range(0, len(pts), 256):
        dist = np.abs(cells[:, None, :] - pts[None, k:k + 256, :]).max(-1)
        flat |= (dist <= r).any(1)
    return out


def pack_bits(occ):
    """(M, M, M) bool [iy, ix, iz] -> int32 words: cell c = (iy M + ix) M + iz is bit c & 31 of word c >> 5."""
    flat = np.asarray(occ, bool).reshape(-1)
    n_words = (flat.size + 31) // 32
    padded = np.zeros(n_words * 32, np.uint8)
    padded[:flat.size] = flat
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def unpack_bits(words, M):
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
    return bits[:M ** 3].astype(bool).reshape(M, M, M)


def sigma_fixture(N, seed=0):
    """A sparse small-integer lattice with one NaN, and the threshold 1.0 that sits exactly on a lattice value (so `>` and `>=`
    differ): (sigma (N, N, N) float32, threshold)."""
    rng = np.random.default_rng(1000 + 17 * N + seed)
    s = np.zeros((N, N, N), np.float32)
    mask = rng.random((N, N, N)) < (0.02 if N > 8 else 0.08)
    s[mask] = rng.integers(1, 4, size=int(mask.sum())).astype(np.float32)
    if N == 2:
        s[...] = 0
        s[1, 0, 1] = 1.0                                   # the only non-zero value equals the threshold: an empty grid
    else:
        c = N // 2
        s[c - 1:c + 2, 0:3, N - 3:N] = 0
        s[c, 1, N - 2] = 1.0                               # an isolated value equal to the threshold: its cells stay empty
        s[0:3, N - 3:N, c - 1:c + 2] = 0
        s[1, N - 2, c] = np.nan                            # an isolated NaN corner: its 8 cells are occupied
    return s, 1.0


# --------------------------------------------------------------------------------------------------------------------- grids
class Grid:
    def __init__(self, name, occ, ranges):
        self.name = name
        self.occ = np.asarray(occ, bool)                   # [iy, ix, iz]
        self.M = self.occ.shape[0]
        self.ranges = tuple((float(np.float32(lo)), float(np.float32(hi))) for lo, hi in ranges)   # x, y, z; fp32-exact
        self.words = pack_bits(self.occ)

    def boxes(self):
        """(K, 3) lower and upper corners in (x, y, z) of the occupied cells, float64: cell i spans [lo + i h, lo + (i + 1) h]."""
        idx = np.argwhere(self.occ)                        # columns iy, ix, iz
        ijk = idx[:, [1, 0, 2]].astype(np.float64)         # -> ix, iy, iz = x, y, z
        lo = np.array([r[0] for r in self.ranges])
        hi = np.array([r[1] for r in self.ranges])
        h = (hi - lo) / self.M
        return lo + ijk * h, lo + (ijk + 1) * h


def _contents(M):
    c = (np.arange(M) + 0.5) / M
    y, x, z = np.meshgrid(c, c, c, indexing="ij")
    sphere = (x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2 <= 0.3 ** 2
    blobs = ((x - 0.2) ** 2 + (y - 0.25) ** 2 + (z - 0.2) ** 2 <= 0.15 ** 2) | \
            ((x - 0.8) ** 2 + (y - 0.75) ** 2 + (z - 0.8) ** 2 <= 0.15 ** 2)
    corner = np.zeros((M, M, M), bool)
    corner[M - 1, 0, M - 1] = True
    return {"sphere": sphere, "blobs": blobs, "corner": corner, "ones": np.ones((M, M, M), bool), "zeros": np.zeros((M, M, M), bool)}


CUBE = ((-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0))
UNEQUAL = ((-0.5, 2.5), (1.0, 1.75), (-3.0, -1.0))


def grids():
    """M = 1; 5 (125 bits: a ragged last word); 9 with unequal axis ranges; 33 (rows straddle words) x sphere, two separated
    blobs, one corner cell, all ones, all zeros."""
    out = []
    for M, ranges in ((1, CUBE), (5, CUBE), (9, UNEQUAL), (33, CUBE)):
        for name, occ in _contents(M).items():
            if M == 1 and name in ("blobs", "corner"):     # one cell: `corner` is `ones`, `blobs` (centre in neither) is `zeros`
                continue
            out.append(Grid("M%d-%s" % (M, name), occ, ranges))
    return out


# ---------------------------------------------------------------------------------------------------------------------- rays
def generic_rays(grid, seed, n_each=40):
    """A few hundred rays: origins outside, inside, inside an occupied cell and behind the box; unit and non-unit d of every
    sign combination; near / far that keep, cut short on either side, or miss the box's interval.  (n, 8) float32."""
    rng = np.random.default_rng(seed)
    lo = np.array([r[0] for r in grid.ranges])
    hi = np.array([r[1] for r in grid.ranges])
    ctr, ext = (lo + hi) / 2, (hi - lo)
    diag = float(np.linalg.norm(ext))
    rows = []

    def aim(o, spread):
        target = ctr + (rng.random(3) - 0.5) * ext * spread
        d = target - o
        return d / np.linalg.norm(d)

    def interval(o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (lo - o) / d, (hi - o) / d
        return float(np.max(np.minimum(ta, tb))), float(np.min(np.maximum(ta, tb)))

    blo, bhi = grid.boxes()
    for kind in ("outside", "inside", "in_cell", "behind"):
        for k in range(n_each * (3 if kind == "outside" else 1)):
            if kind == "outside":
                v = rng.normal(size=3)
                o = ctr + v / np.linalg.norm(v) * diag * rng.uniform(0.8, 2.5)
                d = aim(o, 1.3)
            elif kind == "inside":
                o = lo + rng.random(3) * ext
                v = rng.normal(size=3)
                d = v / np.linalg.norm(v)
            elif kind == "in_cell":
                if len(blo):
                    j = rng.integers(len(blo))
                    o = blo[j] + rng.uniform(0.1, 0.9, 3) * (bhi[j] - blo[j])
                else:
                    o = lo + rng.random(3) * ext
                v = rng.normal(size=3)
                d = v / np.linalg.norm(v)
            else:
                v = rng.normal(size=3)
                o = ctr + v / np.linalg.norm(v) * diag * rng.uniform(0.8, 2.0)
                d = -aim(o, 1.0)                           # the box lies behind the origin
            if k % 2:
                d = d * rng.choice([0.05, 0.37, 3.0, 11.0])  # non-unit, as NDC rays are
            a, b = interval(o, d)
            a, b = (a, b) if a < b else (0.0, diag / np.linalg.norm(d))
            mode = k % 6
            if kind == "behind" and mode < 4:              # the whole box at negative parameters, [near, far] in front
                near, far = 0.0, rng.uniform(0.5, 3.0) * diag / np.linalg.norm(d)
            elif mode in (0, 1):
                near, far = max(0.0, a - 0.3 * (b - a)), b + 0.3 * (b - a)
            elif mode == 2:
                near, far = a + rng.uniform(0.2, 0.6) * (b - a), b + 0.2 * (b - a)         # the front is cut short
            elif mode == 3:
                near, far = min(a, 0.0), a + rng.uniform(0.3, 0.8) * (b - a)              # the back is cut short
            elif mode == 4:
                near, far = a + 0.3 * (b - a), a + 0.7 * (b - a)                           # both
            else:
                near, far = (b + 0.1 * (b - a), b + 0.5 * (b - a)) if k % 4 else (a - 0.5 * (b - a) - 1.0, a - 0.1 * (b - a) - 0.5)
            rows.append(np.concatenate([o, d, [near, far]]))
    return np.asarray(rows, np.float64).astype(np.float32)


def bulk_rays(grid, n, seed):
    """n rays from origins around the box aimed at points in and around it, with near / far around the box's interval: over
    a third of them cross a sphere grid.  (n, 8) float32."""
    rng = np.random.default_rng(seed)
    lo = np.array([r[0] for r in grid.ranges])
    hi = np.array([r[1] for r in grid.ranges])
    ctr, ext = (lo + hi) / 2, (hi - lo)
    diag = float(np.linalg.norm(ext))
    v = rng.normal(size=(n, 3))
    o = ctr + v / np.linalg.norm(v, axis=1, keepdims=True) * diag * rng.uniform(0.3, 2.0, (n, 1))
    d = ctr + (rng.random((n, 3)) - 0.5) * ext * 0.8 - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.choice([1.0, 1.0, 0.25, 7.0], (n, 1))
    near = rng.uniform(0.0, 0.3, n) * diag / np.linalg.norm(d, axis=1)
    far = near + rng.uniform(0.2, 2.5, n) * diag / np.linalg.norm(d, axis=1)
    return np.concatenate([o, d, near[:, None], far[:, None]], 1).astype(np.float32)


def degenerate_rays(grid):
    """Axis-parallel rays with +-0 components, a ray lying in a cell-face plane, a ray through a cell corner, near == far, and
    NaN / inf in every column.  (n, 8) float32 and the mask of the rows that hold a non-finite value."""
    lo = np.array([r[0] for r in grid.ranges], np.float64)
    hi = np.array([r[1] for r in grid.ranges], np.float64)
    h = (hi - lo) / grid.M
    ctr = (lo + hi) / 2
    far = float(4 * np.linalg.norm(hi - lo))
    rows = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                d = np.array([zero, zero, zero])
                d[axis] = sign
                for off in (0.25, 0.5, 0.0, 1.0, -0.3, 1.3):        # inside, on the lower / upper face, outside
                    o = lo + off * (hi - lo)
                    o[axis] = ctr[axis] - sign * 1.5 * (hi[axis] - lo[axis])
                    rows.append(np.concatenate([o, d, [0.0, far]]))
                # in a cell-face plane: the other two coordinates sit exactly on planes of the grid
                o = lo + h * (grid.M // 2)
                o[axis] = ctr[axis] - sign * 1.5 * (hi[axis] - lo[axis])
                rows.append(np.concatenate([o, d, [0.0, far]]))
    for s in itertools.product((1.0, -1.0), repeat=3):               # through a cell corner (the grid's centre-most plane crossing)
        corner = lo + h * ((grid.M + 1) // 2)
        d = np.array(s) * (hi - lo)
        rows.append(np.concatenate([corner - 1.5 * d, d / np.linalg.norm(d), [0.0, far]]))
        rows.append(np.concatenate([corner - 1.5 * d, d, [0.0, 3.0]]))
    for t in (0.0, 1.0, far / 4):                                    # near == far
        rows.append(np.concatenate([ctr - np.array([1.0, 0.3, 0.2]) * (hi - lo), np.array([1.0, 0.3, 0.2]) * (hi - lo), [t, t]]))
    rows.append(np.concatenate([ctr, [0.0, 0.0, 0.0], [0.0, 1.0]]))   # no direction at all
    rows.append(np.concatenate([ctr, [-0.0, 0.0, -0.0], [0.0, 1.0]]))
    n_finite = len(rows)
    base = np.concatenate([ctr - np.array([1.5, 0.2, 0.1]) * (hi - lo), np.array([1.0, 0.13, 0.07]), [0.0, far]])
    for col in range(8):
        for bad in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[col] = bad
            rows.append(r)
    rays = np.asarray(rows, np.float64).astype(np.float32)
    nonfinite = np.zeros(len(rows), bool)
    nonfinite[n_finite:] = True
    return rays, nonfinite


# -------------------------------------------------------------------------------------------------------------------- oracle
def oracle(grid, rays, chunk=2048):
    """Per ray (float64): hit_must, hit_may, and the entry / exit bounds T0 / T1 from the inflated and from the shrunk boxes
    (inf / -inf where no box of that set is pierced).  Rays must be finite."""
    r = np.asarray(rays, np.float32).astype(np.float64)
    o, d, near, far = r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7]
    S = np.max(np.abs(np.array(grid.ranges)))
    S = np.maximum(S, np.maximum(np.abs(o).max(1), np.abs(o + far[:, None] * d).max(1)))
    eps = EPS_REL * S                                      # (n,)
    blo, bhi = grid.boxes()
    n = r.shape[0]
    res = {"hit_must": np.zeros(n, bool), "hit_may": np.zeros(n, bool), "eps": eps,
           "T0_inflated": np.full(n, np.inf), "T1_inflated": np.full(n, -np.inf),
           "T0_shrunk": np.full(n, np.inf), "T1_shrunk": np.full(n, -np.inf)}
    for k in range(0, len(blo), chunk):
        lo_k, hi_k = blo[k:k + chunk], bhi[k:k + chunk]
        for name, sign, strict in (("inflated", 1.0, False), ("shrunk", -1.0, True)):
            en, ex, ok = _slab_margin(o, d, near, far, lo_k, hi_k, sign * eps, strict)
            res["T0_" + name] = np.minimum(res["T0_" + name], np.where(ok, en, np.inf).min(1))
            res["T1_" + name] = np.maximum(res["T1_" + name], np.where(ok, ex, -np.inf).max(1))
            res["hit_may" if name == "inflated" else "hit_must"] |= ok.any(1)
    return res


def _slab_margin(o, d, near, far, blo, bhi, margin, strict):
    """rays (n,) x boxes (K,), every box grown by margin[i] (negative: shrunk) for ray i: entry / exit with near / far folded in,
    and whether the box is pierced inside [near, far]."""
    n, K = o.shape[0], blo.shape[0]
    en = np.full((n, K), -np.inf)
    ex = np.full((n, K), np.inf)
    ok = np.ones((n, K), bool)
    m = margin[:, None]
    for a in range(3):
        oa, da = o[:, a:a + 1], d[:, a:a + 1]
        la, ha = blo[None, :, a] - m, bhi[None, :, a] + m
        ok &= la < ha if strict else la <= ha              # a cell thinner than 2 eps has no shrunk box
        zero = (da == 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (la - oa) / da
            tb = (ha - oa) / da
        inside = ((oa > la) & (oa < ha)) if strict else ((oa >= la) & (oa <= ha))
        ok &= np.where(zero, inside, True)
        en = np.where(zero, en, np.maximum(en, np.minimum(ta, tb)))
        ex = np.where(zero, ex, np.minimum(ex, np.maximum(ta, tb)))
    en = np.maximum(en, near[:, None])
    ex = np.minimum(ex, far[:, None])
    ok &= (en < ex) if strict else (en <= ex)
    return en, ex, ok


def ulp32(t):
    """The spacing of float32 at |t| (float64 array)."""
    return np.spacing(np.abs(np.asarray(t, np.float64)).astype(np.float32)).astype(np.float64)

"""The baked-volume march restated in numpy float64 with no skipping, the brick layout and the cell-brick
bitfield written from their words (loops over points and bricks, nothing shared with nerf_pl_amd.baked), and the fixtures of
tests/test_baked_host.py and tests/test_gpu_baked.py: lattices, volumes and rays, all seeded."""
import numpy as np

SEED = 1906


# ---- layouts from their words -------------------------------------------------------------------------------------------------
def point_offset(N, iy, ix, iz):
    """Byte offset of lattice point (iy, ix, iz) in the bricked volume."""
    NB = -(-N // 8)
    brick = ((iy >> 3) * NB + (ix >> 3)) * NB + (iz >> 3)
    local = ((iy & 7) * 8 + (ix & 7)) * 8 + (iz & 7)
    return brick * 2048 + local * 4


def bricks_from_dense(rgba):
    N = rgba.shape[0]
    NB = -(-N // 8)
    out = np.zeros(NB ** 3 * 2048, np.uint8)
    for iy in range(N):
        for ix in range(N):
            for iz in range(N):
                off = point_offset(N, iy, ix, iz)
                out[off:off + 4] = rgba[iy, ix, iz]
    return out


def brick_bits(rgba):
    N = rgba.shape[0]
    MB = -(-(N - 1) // 8)
    words = np.zeros(-(-MB ** 3 // 32), np.uint32)
    for by in range(MB):
        for bx in range(MB):
            for bz in range(MB):
                occupied = False
                for iy in range(8 * by, min(8 * by + 8, N - 1) + 1):
                    for ix in range(8 * bx, min(8 * bx + 8, N - 1) + 1):
                        for iz in range(8 * bz, min(8 * bz + 8, N - 1) + 1):
                            occupied = occupied or rgba[iy, ix, iz, 3] > 0
                if occupied:
                    c = (by * MB + bx) * MB + bz
                    words[c >> 5] |= np.uint32(1 << (c & 31))
    return words.view(np.int32)


# ---- the march in float64 -----------------------------------------------------------------------------------------------------
def render(rays, rgba, ranges, cell, step, t_stop=0.0, white_back=False):
    """-> dict(rgb (n,3), depth (n,), opacity (n,), K (n,) segments per ray): the semantics of include/nerfhip.h, every segment
    sampled.  rays, ranges, cell, step and t_stop are read as the float32 values the C entry point receives; everything after that
    is float64."""
    rays = np.asarray(rays, np.float32).astype(np.float64)
    cell, step, t_stop = float(np.float32(cell)), float(np.float32(step)), float(np.float32(t_stop))
    n = rays.shape[0]
    N = rgba.shape[0]
    vol = rgba.astype(np.float64)
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    lo = np.array([r[0] for r in ranges], np.float32).astype(np.float64)
    hi = np.array([r[1] for r in ranges], np.float32).astype(np.float64)
    bg = 1.0 if white_back else 0.0
    with np.errstate(all="ignore"):
        dn = np.sqrt((d * d).sum(1))
        live = np.isfinite(rays).all(1) & (dn > 0)
        t_in, t_out = near.copy(), far.copy()
        for a in range(3):
            zero = d[:, a] == 0
            live &= ~(zero & ((o[:, a] < lo[a]) | (o[:, a] > hi[a])))
            ta, tb = (lo[a] - o[:, a]) / d[:, a], (hi[a] - o[:, a]) / d[:, a]
            t_in = np.where(zero, t_in, np.maximum(t_in, np.minimum(ta, tb)))
            t_out = np.where(zero, t_out, np.minimum(t_out, np.maximum(ta, tb)))
        live &= t_in < t_out
        dt = step * cell / dn
        K = np.where(live, np.ceil((t_out - t_in) / dt), 0).astype(np.int64)
    rgb = np.zeros((n, 3))
    depth = np.zeros(n)
    opacity = np.zeros(n)
    T = np.ones(n)
    going = live.copy()
    scale = (N - 1) / (hi - lo)
    for k in range(int(K.max()) if n else 0):
        m = np.flatnonzero(going & (k < K))
        if m.size == 0:
            break
        ta = t_in[m] + k * dt[m]
        tb = np.minimum(ta + dt[m], t_out[m])
        delta = np.maximum(tb - ta, 0.0)
        tm = ta + delta / 2
        g = (o[m] + tm[:, None] * d[m] - lo) * scale
        c = np.clip(np.floor(g), 0, N - 2)
        f = np.clip(g - c, 0.0, 1.0)
        c = c.astype(np.int64)
        sa = np.zeros(m.size)
        sc = np.zeros((m.size, 3))
        for q in range(8):
            qy, qx, qz = q >> 2, (q >> 1) & 1, q & 1
            p = vol[c[:, 1] + qy, c[:, 0] + qx, c[:, 2] + qz] / 255.0
            w = (f[:, 1] if qy else 1 - f[:, 1]) * (f[:, 0] if qx else 1 - f[:, 0]) * (f[:, 2] if qz else 1 - f[:, 2])
            sa += w * p[:, 3]
            sc += (w * p[:, 3])[:, None] * p[:, :3]
        has = sa > 0
        colour = np.where(has[:, None], sc / np.where(has, sa, 1.0)[:, None], 0.0)
        a = np.minimum(sa, 1.0)
        e = delta * dn[m] / cell
        with np.errstate(all="ignore"):
            alpha = np.where(has & (e > 0), 1.0 - np.exp2(e * np.log2(1.0 - a)), 0.0)
        w = T[m] * alpha
        rgb[m] += w[:, None] * colour
        depth[m] += w * tm
        opacity[m] += w
        T[m] *= 1.0 - alpha
        going[m[T[m] < t_stop]] = False
    rgb = np.where(live[:, None], rgb + (1.0 - opacity)[:, None] * bg, bg)
    return {"rgb": rgb, "depth": depth, "opacity": opacity, "K": K, "live": live}


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
RANGES = ((-1.0, 1.5), (-0.75, 1.0), (0.25, 2.5))          # unequal on purpose
LATTICES = (2, 9, 17, 33)                                  # one cell; one cell brick; two bricks; four + a padded point brick
STEPS = (1.0, 0.5, 1.0 / 16, 8.0)
VOLUMES = ("zero", "uniform", "voxel", "shell", "random")


def cell_of(N, ranges=RANGES):
    """export_vol's default cell, as the float32 the C entry point receives"""
    return float(np.float32((ranges[0][1] - ranges[0][0]) / N))


def volume(kind, N):
    rng = np.random.default_rng(SEED + 7 * N + VOLUMES.index(kind))
    v = np.zeros((N, N, N, 4), np.uint8)
    if kind == "uniform":
        v[...] = (200, 90, 30, 140)
    elif kind == "voxel":
        v[N // 2, min(N - 1, N // 2 + 1), max(0, N // 2 - 1)] = (10, 250, 120, 230)
    elif kind == "shell":
        ax = np.linspace(-1.0, 1.0, N)
        r = np.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
        on = np.abs(r - 0.6) < max(1.2 / N, 0.08)
        v[on] = (60, 130, 220, 190)
        v[..., 0][on] = (255 * (0.5 + 0.5 * np.broadcast_to(ax[:, None, None], r.shape)[on])).astype(np.uint8)
    elif kind == "random":
        v[...] = rng.integers(0, 256, size=v.shape, dtype=np.uint8)
        low = rng.random((N, N, N)) < 0.5
        v[..., 3][low] = rng.integers(1, 12, size=int(low.sum()), dtype=np.uint8)
        v[rng.random((N, N, N)) < 0.6] = 0
    return v


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def rays(N, n_main=600, ranges=RANGES):
    """About 1,000 float32 ray rows for the box `ranges`: aimed into the box from radius 4 with |d| in [0.5, 2], rays that miss,
    origins inside the box, axis-parallel rays with zero components of both signs, near / far that cut inside the box, and as the
    last two rows one NaN row and one zero-direction row."""
    rng = np.random.default_rng(SEED + N)
    lo = np.array([r[0] for r in ranges])
    hi = np.array([r[1] for r in ranges])
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    rows = []
    # aimed into the box from radius 4
    o = mid + 4.0 * _unit(rng, n_main)
    target = mid + half * rng.uniform(-0.95, 0.95, size=(n_main, 3))
    d = target - o
    d *= (rng.uniform(0.5, 2.0, size=(n_main, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    rows.append(np.concatenate([o, d, np.zeros((n_main, 1)), np.full((n_main, 1), 20.0)], 1))
    # misses: aimed away from the box
    m = 60
    o = mid + 4.0 * _unit(rng, m)
    d = (o - mid) * rng.uniform(0.2, 0.6, size=(m, 1))
    rows.append(np.concatenate([o, d, np.zeros((m, 1)), np.full((m, 1), 20.0)], 1))
    # origins inside the box
    m = 120
    o = mid + half * rng.uniform(-0.9, 0.9, size=(m, 3))
    d = _unit(rng, m) * rng.uniform(0.5, 2.0, size=(m, 1))
    rows.append(np.concatenate([o, d, np.zeros((m, 1)), np.full((m, 1), 20.0)], 1))
    # axis-parallel, zeros of both signs, through the box and beside it
    for axis in range(3):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                m = 6
                o = mid + half * rng.uniform(-0.9, 0.9, size=(m, 3))
                o[m - 1, (axis + 1) % 3] = hi[(axis + 1) % 3] + 0.5                  # one beside the box: its zero slab misses
                o[:, axis] = mid[axis] - sign * 4.0
                d = np.full((m, 3), zero)
                d[:, axis] = sign * rng.uniform(0.5, 2.0, size=m)
                rows.append(np.concatenate([o, d, np.zeros((m, 1)), np.full((m, 1), 20.0)], 1))
    # near / far cutting inside the box
    m = 120
    o = mid + 4.0 * _unit(rng, m)
    target = mid + half * rng.uniform(-0.5, 0.5, size=(m, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t_mid = np.linalg.norm(target - o, axis=1)
    near = t_mid - rng.uniform(0.0, 0.6, size=m)
    far = t_mid + rng.uniform(0.01, 0.6, size=m)
    rows.append(np.concatenate([o, d, near[:, None], far[:, None]], 1))
    out = np.concatenate(rows, 0).astype(np.float32)
    bad = np.zeros((2, 8), np.float32)
    bad[0] = out[0]
    bad[0, 4] = np.nan
    bad[1] = out[1]
    bad[1, 3:6] = 0.0
    return np.concatenate([out, bad], 0)


def chord_length(rays, ranges=RANGES):
    """The parameter length of (the ray's chord through the box) ∩ [near, far], in float64; 0 for a miss."""
    r = np.asarray(rays, np.float32).astype(np.float64)
    o, d = r[:, 0:3], r[:, 3:6]
    t0, t1 = r[:, 6].copy(), r[:, 7].copy()
    ok = np.isfinite(r).all(1) & ((d * d).sum(1) > 0)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo, hi = (float(np.float32(v)) for v in ranges[a])            # as the C entry point receives them
            zero = d[:, a] == 0
            ok &= ~(zero & ((o[:, a] < lo) | (o[:, a] > hi)))
            ta, tb = (lo - o[:, a]) / d[:, a], (hi - o[:, a]) / d[:, a]
            t0 = np.where(zero, t0, np.maximum(t0, np.minimum(ta, tb)))
            t1 = np.where(zero, t1, np.minimum(t1, np.maximum(ta, tb)))
    return np.where(ok & (t0 < t1), t1 - t0, 0.0)

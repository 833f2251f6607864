"""GPU: mesh extraction (nerf_pl_amd.mesh) — marching cubes, largest-cluster cleanup, vertex normals, colour fusion and the
end-to-end extract_color_mesh, against geometric invariants and numpy restatements of the reference's loop."""
import numpy as np
import pytest
import torch

from tests.helpers import O, build_models

pytestmark = pytest.mark.gpu

# Bourke's corner numbering (x, y, z) = (a0, a1, a2)
CORNERS = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)])


@pytest.fixture(scope="module")
def dev():
    from nerf_pl_amd import build
    build.build(verbose=False)
    return torch.device("cuda:0")


def _mc(vol, iso, dev):
    from nerf_pl_amd import mesh
    v, t = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(dev), iso)
    torch.cuda.synchronize()
    assert v.dtype == torch.float64 and t.dtype == torch.int32
    return v.cpu().numpy(), t.cpu().numpy()


def _np_vertices(f, iso):
    """the documented vertex list: (owning point in C order, axis), a + t with t = (iso - fa) / (fb - fa) in fp64"""
    f = f.astype(np.float32)
    below = f.astype(np.float64) < iso
    n = f.shape
    rows = []
    for k in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[k], hi[k] = slice(0, n[k] - 1), slice(1, n[k])
        cr = np.zeros(n, bool)
        cr[tuple(lo)] = below[tuple(lo)] != below[tuple(hi)]
        idx = np.argwhere(cr)
        nb = idx.copy()
        nb[:, k] += 1
        fa = f[tuple(idx.T)].astype(np.float64)
        fb = f[tuple(nb.T)].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(fa == fb, 0.5, (iso - fa) / (fb - fa))
        p = idx.astype(np.float64)
        p[:, k] = p[:, k] + t
        lin = np.ravel_multi_index(tuple(idx.T), n) * 3 + k
        rows.append((lin, p))
    lin = np.concatenate([r[0] for r in rows])
    p = np.concatenate([r[1] for r in rows])
    return p[np.argsort(lin, kind="stable")]


def _directed_edges(t):
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def _closed_manifold(t):
    e = _directed_edges(t).astype(np.int64)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    rev = e[:, 1] * (1 << 32) + e[:, 0]
    if len(np.unique(key)) != len(key):
        return False, 0                      # a directed edge used twice: not oriented / not 2-manifold
    return bool(np.isin(rev, key).all()), len(key) // 2


def _signed_volume(v, t):
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def _edge_of(q):
    """(lower lattice point, axis) of a vertex on a lattice edge"""
    lo = np.floor(q)
    k = int(np.argmax(q - lo))
    return lo.astype(int), k


# ---- 1. the 256 single-cell cases -----------------------------------------------------------------------------------------------
def test_all_256_single_cell_cases(dev):
    for c in range(256):
        f = np.ones((2, 2, 2), np.float32)
        for i, p in enumerate(CORNERS):
            if (c >> i) & 1:
                f[tuple(p)] = 0.0
        v, t = _mc(f, 0.5, dev)
        below = f < 0.5
        crossed = []
        for p in np.argwhere(np.ones((2, 2, 2))):
            for k in range(3):
                if p[k] == 0:
                    q = p.copy()
                    q[k] = 1
                    if below[tuple(p)] != below[tuple(q)]:
                        crossed.append((tuple(p), k))
        assert len(v) == len(crossed), c
        assert sorted((tuple(lo), k) for lo, k in map(_edge_of, v)) == sorted(crossed), c
        assert np.allclose(v - np.floor(v), np.where(v - np.floor(v) > 0, 0.5, 0)), c   # midpoints
        if len(crossed) == 0:
            assert len(t) == 0, c
            continue
        assert set(t.ravel().tolist()) == set(range(len(v))), c                          # exactly the crossed edges
        e = [tuple(x) for x in _directed_edges(t)]
        assert len(set(e)) == len(e), c
        for a, b in e:
            if (b, a) in set(e):
                continue
            pa, pb = v[a], v[b]                                                          # boundary segment: on one cube face
            assert any(pa[k] == pb[k] and pa[k] in (0.0, 1.0) for k in range(3)), (c, a, b)
        for tri in t:                                                                    # winding: normal towards the below side
            p = v[tri]
            n = np.cross(p[1] - p[0], p[2] - p[0])
            s = 0.0
            for q in p:
                lo, k = _edge_of(q)
                hi = lo.copy()
                hi[k] += 1
                lo_below = below[tuple(lo)]
                s += np.dot(n, (lo - hi) if lo_below else (hi - lo))
            assert s > 0, (c, tri)


# ---- 2. sphere and torus -------------------------------------------------------------------------------------------------------
def _lattice(n):
    g = [np.arange(k, dtype=np.float64) for k in n]
    return np.meshgrid(*g, indexing="ij")


def _ambiguous_faces(f, iso):
    b = f.astype(np.float64) < iso
    amb = 0
    for k in range(3):
        i, j = [a for a in range(3) if a != k]
        s = [slice(None)] * 3
        def sh(di, dj):
            sl = list(s)
            sl[i] = slice(di, b.shape[i] - 1 + di)
            sl[j] = slice(dj, b.shape[j] - 1 + dj)
            return b[tuple(sl)]
        c00, c10, c01, c11 = sh(0, 0), sh(1, 0), sh(0, 1), sh(1, 1)
        amb += int(((c00 == c11) & (c10 == c01) & (c00 != c10)).sum())
    return amb


def _fields():
    N = 64
    a0, a1, a2 = _lattice((N, N, N))
    c = (N - 1) / 2.0 + 0.17
    r = np.sqrt((a0 - c) ** 2 + (a1 - c) ** 2 + (a2 - c - 0.1) ** 2)
    R, rr = 18.0, 7.3
    q = np.sqrt((np.sqrt((a0 - c) ** 2 + (a1 - c) ** 2) - R) ** 2 + (a2 - c) ** 2)
    # sigma-like fields: high inside, so the documented winding gives a positive signed volume
    return [("sphere", (25.0 - r).astype(np.float32), 2, 4.0 / 3.0 * np.pi * 25.0 ** 3),
            ("torus", (rr - q).astype(np.float32), 0, 2 * np.pi ** 2 * R * rr ** 2)]


@pytest.mark.parametrize("case", [0, 1], ids=["sphere", "torus"])
def test_sphere_torus(dev, case):
    name, f, chi, vol = _fields()[case]
    iso = 0.0
    assert _ambiguous_faces(f, iso) == 0, name
    v, t = _mc(f, iso, dev)
    want = _np_vertices(f, iso)
    assert len(v) == len(want)                                         # = the numpy count of sign-changing edges
    assert np.array_equal(v, want)
    for q in v[:: max(1, len(v) // 500)]:                               # every vertex on a crossed edge, interpolating to iso
        lo, k = _edge_of(q)
        hi = lo.copy()
        hi[k] += 1
        fa, fb = float(f[tuple(lo)]), float(f[tuple(hi)])
        assert (fa < iso) != (fb < iso)
        val = fa + (q[k] - lo[k]) * (fb - fa)
        assert abs(val - iso) <= 1e-6 * max(1.0, abs(fa), abs(fb))
    ok, n_edges = _closed_manifold(t)
    assert ok, name
    assert len(v) - n_edges + len(t) == chi
    sv = _signed_volume(v, t)
    assert sv > 0                                                       # documented winding: normals towards the lower values
    assert abs(sv - vol) <= 0.01 * vol, (sv, vol)
    v2, t2 = _mc(f, iso, dev)
    assert v.tobytes() == v2.tobytes() and t.tobytes() == t2.tobytes()


# ---- 3. non-cubic volumes: axis order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_non_cubic_plane(dev, axis):
    n = (17, 33, 9)
    a = _lattice(n)
    iso = [7.3, 20.6, 4.45][axis]
    f = a[axis].astype(np.float32)
    v, t = _mc(f, iso, dev)
    others = [n[k] for k in range(3) if k != axis]
    assert len(v) == others[0] * others[1]
    assert np.allclose(v[:, axis], iso, atol=1e-12, rtol=0)
    for k in range(3):
        if k != axis:
            assert np.array_equal(v[:, k], np.round(v[:, k])) and v[:, k].max() == n[k] - 1
    assert len(t) == 2 * (others[0] - 1) * (others[1] - 1)
    assert np.array_equal(v, _np_vertices(f, iso))


# ---- 4. cleanup ----------------------------------------------------------------------------------------------------------------
def _sdf_sphere(n, c, r):
    a0, a1, a2 = _lattice(n)
    return np.sqrt((a0 - c[0]) ** 2 + (a1 - c[1]) ** 2 + (a2 - c[2]) ** 2) - r


def _cleanup(v, t, dev):
    from nerf_pl_amd import mesh
    vv, tt = mesh.keep_largest_cluster(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev))
    return vv.cpu().numpy(), tt.cpu().numpy()


def test_keep_largest_cluster(dev):
    n = (48, 40, 44)
    spheres = [((12.3, 20.1, 21.7), 5.2), ((33.6, 19.4, 22.2), 9.1), ((24.2, 30.5, 8.3), 3.4)]
    f = np.minimum.reduce([_sdf_sphere(n, c, r) for c, r in spheres]).astype(np.float32)
    v, t = _mc(-f, 0.0, dev)
    assert len(t) > 0
    vv, tt = _cleanup(v, t, dev)
    alone_v, alone_t = _mc(-_sdf_sphere(n, *spheres[1]).astype(np.float32), 0.0, dev)
    assert np.array_equal(vv, alone_v) and np.array_equal(tt, alone_t)
    # a two-way tie: the same sphere twice (integer offset): the cluster holding the lower first triangle (lower a0) stays
    g = [((12.4, 20.2, 21.7), 6.3), ((32.4, 20.2, 21.7), 6.3)]
    f2 = np.minimum.reduce([_sdf_sphere(n, c, r) for c, r in g]).astype(np.float32)
    v2, t2 = _mc(-f2, 0.0, dev)
    vv2, tt2 = _cleanup(v2, t2, dev)
    first_v, first_t = _mc(-_sdf_sphere(n, *g[0]).astype(np.float32), 0.0, dev)
    assert len(tt2) * 2 == len(t2)
    assert np.array_equal(vv2, first_v) and np.array_equal(tt2, first_t)


def test_keep_largest_cluster_shared_vertex_only(dev):
    """two triangles sharing a vertex are separate clusters; a shared edge joins them"""
    v = np.arange(21, dtype=np.float32).reshape(7, 3)
    t = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [3, 5, 4]], np.int32)
    vv, tt = _cleanup(v, t, dev)
    # triangles 1 and 3 share edge (3, 4), 2 and 3 share edge (4, 5); triangle 0 shares vertex 2 only
    assert np.array_equal(vv, v[2:]) and np.array_equal(tt, [[0, 1, 2], [2, 3, 4], [1, 3, 2]])


# ---- 5. vertex normals ---------------------------------------------------------------------------------------------------------
def test_vertex_normals_match_open3d_rule(dev):
    from nerf_pl_amd import mesh
    f = _fields()[0][1]
    v, t = _mc(f, 0.0, dev)
    vw = (v / 64.0 * 2 - 1).astype(np.float32)
    vw = np.concatenate([vw, np.zeros((1, 3), np.float32)])            # one unreferenced vertex: zero sum -> (0, 0, 1)
    got = mesh.vertex_normals(torch.from_numpy(vw).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
    vd = vw.astype(np.float64)
    fn = np.cross(vd[t[:, 1]] - vd[t[:, 0]], vd[t[:, 2]] - vd[t[:, 0]])
    acc = np.zeros_like(vd)
    for j in range(3):
        np.add.at(acc, t[:, j], fn)
    nrm = np.linalg.norm(acc, axis=1, keepdims=True)
    want = np.where(nrm > 0, acc / np.where(nrm > 0, nrm, 1), [0.0, 0.0, 1.0])
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-6
    assert np.array_equal(got[-1], [0.0, 0.0, 1.0])


# ---- 6. colour fusion ----------------------------------------------------------------------------------------------------------
def _look_at(pos):
    pos = np.asarray(pos, np.float64)
    back = pos / np.linalg.norm(pos)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    return np.stack([right, up, back, pos], 1).astype(np.float32)       # (3, 4) camera-to-world, camera looks along -back


def _scene():
    W, H, focal, near = 64, 48, 55.0, 1.0
    poses = np.stack([_look_at(p) for p in ([2.6, 0.9, 0.7], [-1.1, 2.4, -0.6], [0.4, -2.2, 1.6])])
    # smooth images (<= ~20 levels per pixel): cv2's 1/32-pixel positions then move a sample by well under one level
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    images = np.stack([np.stack([127.5 + 100 * np.sin(x / (5.0 + i + c) + c) * np.cos(y / (7.0 + c) - i) for c in range(3)], -1)
                       for i in range(3)]).round().astype(np.uint8)
    return W, H, focal, near, poses, images


def _sphere_world_vertices(dev, N=24, radius=10.0):
    a = _sdf_sphere((N, N, N), ((N - 1) / 2 + 0.13, (N - 1) / 2 - 0.21, (N - 1) / 2 + 0.05), radius)
    v, t = _mc(-a.astype(np.float32), 0.0, dev)
    return (v / (N - 1) * 1.6 - 0.8).astype(np.float32), t


def _restated_colors(verts, poses, images, focal, near, params, occ, N_samples, white_back):
    """extract_color_mesh.py:211-279 in numpy (float bilinear instead of cv2's fixed point) + the oracle's render_rays"""
    Vn = len(verts)
    H, W = images.shape[1:3]
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]).astype(np.float32)
    homo = np.concatenate([verts, np.ones((Vn, 1))], 1)
    s_w, s_c = np.zeros((Vn, 1)), np.zeros((Vn, 3))
    opac = []
    for idx in range(len(poses)):
        c2w = np.concatenate([poses[idx], np.array([0, 0, 0, 1]).reshape(1, 4)], 0)
        w2c = np.linalg.inv(c2w)[:3]
        cam = w2c @ homo.T
        cam[1:] *= -1
        img = (K @ cam).T
        depth = img[:, -1:] + 1e-5
        uv = (img[:, :2] / depth).astype(np.float32)
        uv[:, 0] = np.clip(uv[:, 0], 0, W - 1)
        uv[:, 1] = np.clip(uv[:, 1], 0, H - 1)
        x0 = np.floor(uv[:, 0]).astype(int)
        y0 = np.floor(uv[:, 1]).astype(int)
        fx = (uv[:, 0] - x0)[:, None].astype(np.float64)
        fy = (uv[:, 1] - y0)[:, None].astype(np.float64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        im = images[idx].astype(np.float64)
        col = (im[y0, x0] * (1 - fx) * (1 - fy) + im[y0, x1] * fx * (1 - fy) + im[y1, x0] * (1 - fx) * fy + im[y1, x1] * fx * fy)
        col = np.round(col)
        rays_o = torch.FloatTensor(poses[idx][:, -1]).expand(Vn, 3)
        rays_d = torch.FloatTensor(verts) - rays_o
        rays_d = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
        nr = near * torch.ones_like(rays_o[:, :1])
        fr = torch.FloatTensor(depth) * torch.ones_like(rays_o[:, :1])
        rays = torch.cat([rays_o, rays_d, nr, fr], 1)
        op = O.render_rays([params], rays, N_samples, False, 0, 0, 0, white_back, True)["opacity_coarse"].numpy()[:, None]
        op = np.nan_to_num(op, 1)
        opac.append(op[:, 0])
        w = np.ones_like(s_w) * 0.1 / depth
        w += op < occ
        s_c += col * w
        s_w += w
    return (s_c / s_w).astype(np.uint8), np.stack(opac, 1)


def _to_dev_models(params, dev, dtype="fp32"):
    models, emb = build_models(params, dev, dtype)
    for m in models:
        m.eval()
    return models, emb


def test_fuse_vertex_colors(dev):
    from nerf_pl_amd import mesh
    W, H, focal, near, poses, images = _scene()
    verts, tris = _sphere_world_vertices(dev)
    assert 1000 <= len(verts) <= 4000
    p = O.make_params(5, 8.0, -0.19)        # density bias at the field's median over the vertices: both weights occur
    (fine,), emb = _to_dev_models([p], dev)
    occ, S = 0.2, 64
    got = mesh.fuse_vertex_colors(verts, poses, torch.from_numpy(images).to(dev), focal, near, fine, emb, occ_threshold=occ,
                                  N_samples=S, white_back=False).cpu().numpy()
    want, opac = _restated_colors(verts, poses, images, focal, near, p, occ, S, False)
    knife = (np.abs(opac - occ) <= 1e-4).any(1)
    assert knife.sum() <= 0.01 * len(verts), knife.sum()
    assert (opac < occ).any() and (opac >= occ).any()              # both weights occur
    diff = np.abs(got.astype(int) - want.astype(int))[~knife]
    assert diff.max() <= 1, (diff.max(), (diff > 1).sum())


def test_fuse_vertex_colors_vertex_normal_mode(dev):
    from nerf_pl_amd import mesh
    verts, tris = _sphere_world_vertices(dev)
    pc, pf = O.make_params(4, 8.0, 0.3), O.make_params(5, 8.0, 0.3)
    (coarse, fine), emb = _to_dev_models([pc, pf], dev)
    near, far, near_t, S, N_i = 0.5, 2.5, 1.0, 32, 32
    got = mesh.fuse_vertex_colors(verts, None, None, 50.0, near, fine, emb, N_samples=S, use_vertex_normal=True, triangles=tris,
                                  far=far, near_t=near_t, nerf_coarse=coarse, N_importance=N_i).cpu().numpy()
    vd = verts.astype(np.float64)
    fn = np.cross(vd[tris[:, 1]] - vd[tris[:, 0]], vd[tris[:, 2]] - vd[tris[:, 0]])
    acc = np.zeros_like(vd)
    for j in range(3):
        np.add.at(acc, tris[:, j], fn)
    nrm = np.linalg.norm(acc, axis=1, keepdims=True)
    normals = np.where(nrm > 0, acc / np.where(nrm > 0, nrm, 1), [0.0, 0.0, 1.0])
    rays_d = torch.FloatTensor(normals)
    nr = near * torch.ones_like(rays_d[:, :1])
    fr = far * torch.ones_like(rays_d[:, :1])
    rays_o = torch.FloatTensor(verts) - rays_d * nr * near_t
    rgb = O.render_rays([pc, pf], torch.cat([rays_o, rays_d, nr, fr], 1), S, False, 0, 0, N_i, False, True)["rgb_fine"]
    want = (rgb.numpy() * 255.0).astype(np.uint8)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_extract_color_mesh_end_to_end(dev, dtype, tmp_path):
    from nerf_pl_amd import mesh
    from nerf_pl_amd.grid import sigma_grid
    W, H, focal, near, poses, images = _scene()
    (fine,), emb = _to_dev_models([O.make_params(5, 8.0, -0.19)], dev, dtype)
    N, rng_ = 48, ((-1.2, 1.2), (-1.0, 1.0), (-1.1, 1.3))
    sig = sigma_grid(fine, N, *rng_)
    thr = float(torch.quantile(sig.flatten()[:: 7].float(), 0.75))
    assert thr > 0
    imgs = torch.from_numpy(images).to(dev)
    v, t, c = mesh.extract_color_mesh(fine, emb, N, *rng_, thr, poses=poses, images=imgs, focal=focal, near=near, N_samples=32)
    assert len(t) > 0 and v.dtype == np.float32 and t.dtype == np.int32 and c.dtype == np.uint8
    # the composition of the tested stages
    vi, ti = mesh.marching_cubes(sig, thr)
    ref = (vi.cpu().numpy() / N).astype(np.float32)                    # extract_color_mesh.py:148-153
    (xmin, xmax), (ymin, ymax), (zmin, zmax) = rng_
    x_ = (ymax - ymin) * ref[:, 1] + ymin
    y_ = (xmax - xmin) * ref[:, 0] + xmin
    ref[:, 0], ref[:, 1] = x_, y_
    ref[:, 2] = (zmax - zmin) * ref[:, 2] + zmin
    assert np.array_equal(mesh.world_coords(vi, N, *rng_), ref)
    vw, tw = mesh.keep_largest_cluster(torch.from_numpy(ref).to(dev), ti)
    cw = mesh.fuse_vertex_colors(vw, poses, imgs, focal, near, fine, emb, N_samples=32)
    assert np.array_equal(v, vw.cpu().numpy()) and np.array_equal(t, tw.cpu().numpy()) and np.array_equal(c, cw.cpu().numpy())
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, v, t, c)
    v2, t2, c2 = mesh.read_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(t2, t) and np.array_equal(c2, c)


def _np_largest_cluster(v, t):
    """open3d's rule restated: edge-sharing triangle clusters (union-find), most triangles wins, ties to the lowest triangle"""
    T = len(t)
    parent = np.arange(T)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    e = np.sort(_directed_edges(t).astype(np.int64), 1)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    tri = np.tile(np.arange(T), 3)
    order = np.argsort(key, kind="stable")
    ks, ts = key[order], tri[order]
    for i in np.nonzero(ks[1:] == ks[:-1])[0]:
        a, b = find(ts[i]), find(ts[i + 1])
        if a != b:
            parent[max(a, b)] = min(a, b)
    lab = np.array([find(x) for x in range(T)])
    cnt = np.bincount(lab, minlength=T)
    best = int(np.argmax(cnt))                         # first maximum = the lowest root among ties
    keep = lab == best
    used = np.zeros(len(v), bool)
    used[t[keep].ravel()] = True
    new = np.cumsum(used) - 1
    return v[used], new[t[keep]].astype(np.int32)


@pytest.mark.parametrize("seed", [0, 1])
def test_keep_largest_cluster_many_clusters(dev, seed):
    """a noise field with hundreds of clusters against the numpy restatement; the device result is the same on every run"""
    g = np.random.default_rng(seed)
    f = g.standard_normal((40, 36, 44)).astype(np.float32)
    for ax in range(3):                                   # smooth a little: blobs of a few cells
        f = (f + np.roll(f, 1, ax) + np.roll(f, -1, ax)) / 3
    v, t = _mc(f, 0.35, dev)
    assert len(t) > 10000
    want_v, want_t = _np_largest_cluster(v, t)
    for _ in range(3):
        vv, tt = _cleanup(v, t, dev)
        assert np.array_equal(vv, want_v) and np.array_equal(tt, want_t)

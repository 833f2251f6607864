"""GPU: the mesh decimation kernels (csrc/decimate.hip) against their host twins, bit for bit, on every case of
tests/decimate_ref.py and on one soup large enough to cross every multi-block scan; the public layer (decimate, MeshBVH.decimated,
extract_color_mesh's decimate_cell)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_ref as D  # noqa: E402
import mesh_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from nerf_pl_amd import build
    build.build(verbose=False)
    return torch.device("cuda")


def on_device(dev, v, t, c):
    return (torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), None if c is None else torch.from_numpy(c).to(dev))


def same_bytes(got, want, what):
    """(vertices', triangles', colors', cluster_of, counts) of the device against the host twin's"""
    assert got[4] == want[4], (what, got[4], want[4])
    for name, a, b in zip(("vertices", "triangles", "colors", "cluster_of"), got[:4], want[:4]):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            a = a.cpu().numpy()
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, name)


@pytest.mark.parametrize("name", sorted(D.fixtures()))
def test_device_equals_host_twin(dev, name):
    from nerf_pl_amd import ops
    v, t = D.fixtures()[name]
    for case in D.cases():
        if case[0] != name:
            continue
        _, cell, placement, origin, with_colors = case
        c = D.colors_for(v) if with_colors else None
        want = ops.mesh_decimate_host(v, t, c, cell, placement, origin)
        got = ops.mesh_decimate(*on_device(dev, v, t, c), cell, placement, origin)
        same_bytes(got, want, case)


def test_two_runs_give_identical_bytes_and_empty_inputs(dev):
    from nerf_pl_amd import ops
    v, t = R.soup(1000)
    args = on_device(dev, v, t, D.colors_for(v))
    for placement in D.PLACEMENTS:
        a, b = (ops.mesh_decimate(*args, 0.25, placement) for _ in range(2))
        assert a[4] == b[4] and all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a[:4], b[:4]))
    for vv, tt in ((v[:0], t[:0]), (v, t[:0]), (v[:0], t), (np.full_like(v, np.nan), t)):
        same_bytes(ops.mesh_decimate(*on_device(dev, vv, tt, None), 0.25, "quadric"), ops.mesh_decimate_host(vv, tt, None, 0.25, "quadric"),
                   (vv.shape, tt.shape))


@pytest.mark.parametrize("placement", D.PLACEMENTS)
def test_large_soup_crosses_every_scan(dev, placement):
    """100,000 triangles of their own 300,000 vertices: more than 2^18 items and more than 1,024 blocks of 256, so the block totals
    take more than one pass of the single-workgroup scan; the cell leaves more than 65,536 clusters (more than 256 blocks of them)"""
    from nerf_pl_amd import ops
    v, t = D.big_soup()
    t = t.copy()
    t[::997, 1] = -1                                                   # some bad triangles, spread over the blocks
    c = D.colors_for(v)
    want = ops.mesh_decimate_host(v, t, c, 0.02, placement)
    assert len(v) > 1 << 18 and len(v) > 1024 * 256 and want[4]["clusters"] > 65536 and want[4]["bad"] > 0
    assert want[4]["collapsed"] > 0 and want[4]["unreferenced"] > 0 and len(want[1]) > 1024 * 16
    same_bytes(ops.mesh_decimate(*on_device(dev, v, t, c), 0.02, placement), want, placement)


def test_public_layer_and_refusals(dev):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.decimate import decimate
    v, t = R.icosphere(2)
    c = D.colors_for(v)
    want = ops.mesh_decimate_host(v, t, c, 0.25, "quadric")
    out_v, out_t, out_c, info = decimate(v, t, c, cell=0.25, placement="quadric", return_info=True)           # numpy in, device out
    assert out_v.is_cuda and out_t.is_cuda and out_c.is_cuda
    counts = {k: info[k] for k in D.COUNTS}
    same_bytes((out_v, out_t, out_c, info["cluster_of"], counts), want, "numpy in")
    assert len(decimate(*on_device(dev, v, t, None), cell=0.25)) == 3
    with pytest.raises(NerfHipError):
        decimate(torch.from_numpy(v), torch.from_numpy(t), cell=0.25)
    with pytest.raises(NerfHipError):
        decimate(torch.from_numpy(v).to(dev), torch.from_numpy(t), cell=0.25)
    with pytest.raises(NerfHipError):
        ops.mesh_decimate(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(c), 0.25)
    for bad_cell in (0.0, -1.0, float("nan"), 1e-4):
        with pytest.raises(ValueError):
            decimate(v, t, cell=bad_cell)
    with pytest.raises(ValueError):
        decimate(v, t, cell=0.25, origin=(0.0, 0.0, 0.0))


def test_meshbvh_decimated_casts_like_the_original(dev):
    """ico3 at cell 0.25, mean placement: a sphere of radius ~0.99 against one of radius 1.  The hit masks of the 1,024 pinhole rays
    agree on 99.22 % of the rays with the mean placement and on 99.80 % with the quadric one (1,280 -> 474 triangles; measured on an
    MI355X; the bound is 90 %)."""
    from nerf_pl_amd.meshcast import MeshBVH, MeshRenderer
    v, t = R.icosphere(3)
    rays = torch.from_numpy(R.pinhole()).to(dev)
    bvh = MeshBVH(v, t, D.colors_for(v))
    full = MeshRenderer(bvh, white_back=True)(rays)["opacity_fine"] > 0
    for placement in D.PLACEMENTS:
        small = bvh.decimated(0.25, placement)
        assert small.n_bad == 0 and 0 < small.triangles.shape[0] < len(t) and small.colors.shape == small.vertices.shape
        out = MeshRenderer(small, white_back=True)(rays)
        assert out["rgb_fine"].shape == (1024, 3) and bool(torch.isfinite(out["rgb_fine"]).all())
        share = float(((out["opacity_fine"] > 0) == full).float().mean())
        print("ico3 at 0.25, %s: %d -> %d triangles, hit masks agree on %.2f %% of the rays" % (placement, len(t), small.triangles.shape[0],
                                                                                              100 * share))
        assert share >= 0.90, (placement, share)


def _look_at(pos):
    pos = np.asarray(pos, np.float64)
    back = pos / np.linalg.norm(pos)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(back, right), back, pos], 1).astype(np.float32)


def _scene():
    """the three views of tests/test_gpu_mesh.py's smallest scene"""
    W, H, focal, near = 64, 48, 55.0, 1.0
    poses = np.stack([_look_at(p) for p in ([2.6, 0.9, 0.7], [-1.1, 2.4, -0.6], [0.4, -2.2, 1.6])])
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    images = np.stack([np.stack([127.5 + 100 * np.sin(x / (5.0 + i + c) + c) * np.cos(y / (7.0 + c) - i) for c in range(3)], -1)
                       for i in range(3)]).round().astype(np.uint8)
    return W, H, focal, near, poses, images


def test_extract_color_mesh_hook(dev):
    """decimate_cell=None is the mesh of the stages as they are; a cell of two voxels gives fewer vertices, with their colours"""
    from nerf_pl_amd import mesh
    from nerf_pl_amd.grid import sigma_grid
    from tests.helpers import O, build_models
    W, H, focal, near, poses, images = _scene()
    (fine,), emb = build_models([O.make_params(5, 8.0, -0.19)], dev, "fp32")
    fine.eval()
    N, rng_ = 48, ((-1.2, 1.2), (-1.0, 1.0), (-1.1, 1.3))
    sig = sigma_grid(fine, N, *rng_)
    thr = float(torch.quantile(sig.flatten()[:: 7].float(), 0.75))
    imgs = torch.from_numpy(images).to(dev)
    kw = dict(poses=poses, images=imgs, focal=focal, near=near, N_samples=32)
    v, t, c = mesh.extract_color_mesh(fine, emb, N, *rng_, thr, decimate_cell=None, **kw)
    vi, ti = mesh.marching_cubes(sig, thr)
    vw, tw = mesh.keep_largest_cluster(torch.from_numpy(mesh.world_coords(vi, N, *rng_)).to(dev), ti)
    cw = mesh.fuse_vertex_colors(vw, poses, imgs, focal, near, fine, emb, N_samples=32)
    assert v.tobytes() == vw.cpu().numpy().tobytes() and t.tobytes() == tw.cpu().numpy().tobytes() and c.tobytes() == cw.cpu().numpy().tobytes()
    v2, t2, c2 = mesh.extract_color_mesh(fine, emb, N, *rng_, thr, decimate_cell=0.1, decimate_placement="quadric", **kw)
    assert 0 < len(v2) < len(v) and 0 < len(t2) < len(t) and c2.shape == v2.shape and c2.dtype == np.uint8
    assert v2.dtype == np.float32 and t2.dtype == np.int32 and t2.min() == 0 and t2.max() == len(v2) - 1
    dv, dt, _ = mesh_decimate_of(vw, tw)
    assert v2.tobytes() == dv.cpu().numpy().tobytes() and t2.tobytes() == dt.cpu().numpy().tobytes()


def mesh_decimate_of(vw, tw):
    from nerf_pl_amd.decimate import decimate
    return decimate(vw, tw, None, cell=0.1, placement="quadric")

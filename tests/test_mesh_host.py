"""CPU: the mesh module's PLY writer, its argument checks (made on the host, before any launch) and its C ABI exports."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ply_by_hand(v, t, c=None):
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(v)
    if c is not None:
        head += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(t)
    out = head.encode()
    for i, p in enumerate(v):
        out += struct.pack("<fff", *p)
        if c is not None:
            out += struct.pack("<BBB", *c[i])
    for tri in t:
        out += struct.pack("<Biii", 3, *tri)
    return out


@pytest.mark.parametrize("with_colors", [False, True])
def test_write_ply_bytes(tmp_path, with_colors):
    from nerf_pl_amd import mesh
    rng = np.random.default_rng(0)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    t = rng.integers(0, 7, (5, 3)).astype(np.int32)
    c = rng.integers(0, 256, (7, 3)).astype(np.uint8) if with_colors else None
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, v, t, c)
    assert open(path, "rb").read() == _ply_by_hand(v, t, c)
    v2, t2, c2 = mesh.read_ply(path)
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    assert (c2 is None) if c is None else np.array_equal(c2, c)


def test_write_ply_empty(tmp_path):
    from nerf_pl_amd import mesh
    path = str(tmp_path / "e.ply")
    mesh.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert open(path, "rb").read() == _ply_by_hand([], [])


def test_world_coords_reference_and_exact():
    from nerf_pl_amd import mesh
    v = np.array([[0.0, 0.0, 0.0], [47.0, 0.5, 12.25], [3.5, 47.0, 20.0]])
    N, xr, yr, zr = 48, (-1.0, 1.5), (-0.5, 0.75), (-1.2, 1.2)
    ref = (v / N).astype(np.float32)                        # extract_color_mesh.py:148-153
    x_ = (yr[1] - yr[0]) * ref[:, 1] + yr[0]
    y_ = (xr[1] - xr[0]) * ref[:, 0] + xr[0]
    ref[:, 0], ref[:, 1] = x_, y_
    ref[:, 2] = (zr[1] - zr[0]) * ref[:, 2] + zr[0]
    got = mesh.world_coords(v, N, xr, yr, zr)
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    ex = mesh.world_coords(v, N, xr, yr, zr, coords="exact")
    assert np.allclose(ex[1], [xr[0] + 0.5 * 2.5 / 47, yr[1], zr[0] + 12.25 * 2.4 / 47], atol=1e-6)
    with pytest.raises(ValueError):
        mesh.world_coords(v, N, xr, yr, zr, coords="nope")


@pytest.mark.parametrize("bad", ["cpu", "float64", "int32", "rank2", "rank4", "dim1"])
def test_marching_cubes_refuses_before_launch(bad):
    from nerf_pl_amd import mesh
    from nerf_pl_amd._lib import NerfHipError
    vol = {"cpu": torch.zeros(4, 4, 4), "float64": torch.zeros(4, 4, 4, dtype=torch.float64),
           "int32": torch.zeros(4, 4, 4, dtype=torch.int32), "rank2": torch.zeros(4, 4), "rank4": torch.zeros(2, 2, 2, 2),
           "dim1": torch.zeros(4, 1, 4)}[bad]
    with pytest.raises(NerfHipError):
        mesh.marching_cubes(vol, 0.5)


def test_mesh_wrappers_refuse_cpu_tensors():
    from nerf_pl_amd import mesh, ops
    from nerf_pl_amd._lib import NerfHipError
    v = torch.zeros(3, 3)
    t = torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(NerfHipError):
        mesh.keep_largest_cluster(v, t)
    with pytest.raises(NerfHipError):
        mesh.vertex_normals(v, t)
    with pytest.raises(NerfHipError):
        ops.color_finish(torch.zeros(3, 4, dtype=torch.float64))
    with pytest.raises(NerfHipError):
        ops.rgb_to_u8(torch.zeros(3, 3))


def test_fresh_build_exports_mesh_symbols():
    r = subprocess.run([sys.executable, "-m", "nerf_pl_amd.build"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from nerf_pl_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (nerfhip_[a-z0-9_]+)", out))
    want = {"nerfhip_marching_cubes_workspace_bytes", "nerfhip_marching_cubes_count", "nerfhip_marching_cubes_emit",
            "nerfhip_mesh_edge_keys", "nerfhip_mesh_cluster_workspace_bytes", "nerfhip_mesh_largest_cluster",
            "nerfhip_mesh_cluster_compact", "nerfhip_mesh_vertex_normals", "nerfhip_mesh_normal_rays", "nerfhip_mesh_view_rays",
            "nerfhip_mesh_color_accumulate", "nerfhip_mesh_color_finish", "nerfhip_mesh_rgb_to_u8"}
    assert want <= exported, sorted(want - exported)
    assert want <= set(_lib.SIGNATURES)
    lib = _lib.load()
    # workspace queries are pure host arithmetic: 0 for shapes the kernels do not take
    assert lib.nerfhip_marching_cubes_workspace_bytes(256, 256, 256) > 256 ** 3 * 6
    assert lib.nerfhip_marching_cubes_workspace_bytes(1, 4, 4) == 0
    assert lib.nerfhip_marching_cubes_workspace_bytes(2048, 2048, 2048) == 0
    assert lib.nerfhip_mesh_cluster_workspace_bytes(10, 0) == 0 and lib.nerfhip_mesh_cluster_workspace_bytes(10, 4) > 0

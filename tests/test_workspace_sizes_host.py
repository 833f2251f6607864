"""CPU: the workspace sizes of the mesh and volume calls are pinned.  csrc/mesh.hip and csrc/volume.hip state each layout once
(the size query carves it from a null base, block_scan.h), so a changed layout shows here before a caller's buffer is too small.
The literals were printed by the library before the queries were rewritten that way: every array rounded up to 256 bytes."""
import pytest

from nerf_pl_amd import _lib

# the smallest grid (8 points), 285 points (2 blocks of 256), 266,240 points (1040 blocks: two passes of the 1024-wide scan)
MARCHING_CUBES = {(2, 2, 2): 1792, (3, 5, 19): 3328, (64, 64, 65): 1623040}
# (V, T): one vertex and triangle; 2 and 5 blocks; 1025 and 2049 blocks
CLUSTER = {(1, 1): 3072, (257, 1025): 17664, (262145, 524289): 8166400}
# one point; 2 blocks; 1025 blocks
VOLUME = {1: 768, 257: 768, 262145: 13056}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_marching_cubes_workspace_bytes(lib):
    for dims, want in MARCHING_CUBES.items():
        assert lib.nerfhip_marching_cubes_workspace_bytes(*dims) == want, dims


def test_mesh_cluster_workspace_bytes(lib):
    for (V, T), want in CLUSTER.items():
        assert lib.nerfhip_mesh_cluster_workspace_bytes(V, T) == want, (V, T)


def test_vol_workspace_bytes(lib):
    for n, want in VOLUME.items():
        assert lib.nerfhip_vol_workspace_bytes(n) == want, n

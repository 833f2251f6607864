"""The Unity volume file (.vol) of a trained NeRF: the reference's extract_mesh.ipynb, cell "Generate .vol file for volume
rendering in Unity" (README_Unity.md), without the 2.1 GB host copy of the N^3 x 4 network output.

    rgbsigma_grid (full network on the lattice, fused MLP kernel) -> vol_records (csrc/volume.hip) -> write_vol

The file is a headerless sequence of little-endian uint32 pairs (i, R<<24 | G<<16 | B<<8 | A), one per lattice point whose
alpha a = 1 - exp(-cell * max(sigma, 0)) is positive, in increasing i.  i = iy N^2 + ix N + iz is the point's position in
`np.meshgrid(x, y, z)` ('xy' order), the order of grid.sigma_grid; R, G, B = trunc(rgb * 255) and A = trunc(a * 255) in float32;
cell = (xmax - xmin) / N.  The notebook insists on N = 512 because the Unity loader does; this module takes any N^3 < 2^32.

`export_vol` never holds the whole lattice: per chunk of points it runs the network and appends the chunk's kept records to one
output buffer through a device-resident cursor, which the host reads once at the end.

    python -m nerf_pl_amd.volume --ckpt_path ckpts/exp/epoch=05.ckpt --scene_name lego --N 512 \\
        --x_range -1.2 1.2 --y_range -1.2 1.2 --z_range -1.2 1.2
"""
import numpy as np
import torch

from . import _lib, ops
from ._lib import NerfHipError, check, device_guard, ptr, stream_ptr

__all__ = ["rgbsigma_grid", "vol_records", "export_vol", "write_vol", "read_vol", "load_ckpt"]

_MAX_POINTS = 1 << 32


def _check_lattice(N):
    N = int(N)
    if N < 1:
        raise ValueError("N must be >= 1, got %d" % N)
    if N ** 3 >= _MAX_POINTS:
        raise ValueError("N^3 must be < 2^32 (the file's point index is a uint32): N = %d has %d points" % (N, N ** 3))
    return N


def _model_device(model):
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise NerfHipError("nerf_pl_amd runs on MI355X only: the model is on %s (no CPU fallback)" % dev)
    return dev


def _axes(N, x_range, y_range, z_range, dev):
    # np.linspace in float64, then the float32 cast of torch.FloatTensor(...): extract_mesh.ipynb, as grid.sigma_grid
    return [torch.from_numpy(np.linspace(lo, hi, N).astype(np.float32)).to(dev) for lo, hi in (x_range, y_range, z_range)]


def _forward_points(model, N, axes, p0, p1, embeddings):
    """rgb-sigma (p1 - p0, 4) of the lattice points p0 .. p1-1 with a zero view direction."""
    xs, ys, zs = axes
    idx = torch.arange(p0, p1, device=xs.device)
    iz, row = idx % N, idx // N
    ix, iy = row % N, row // N
    n = p1 - p0
    if model.is_default_arch():
        # every point is a one-sample ray o = point, d = 0, z = 0: the fused kernel forms o + 0 * 0 = o exactly and embeds d = 0
        rays = torch.zeros(n, 8, device=xs.device, dtype=torch.float32)
        rays[:, 0], rays[:, 1], rays[:, 2] = xs[ix], ys[iy], zs[iz]
        z = torch.zeros(n, 1, device=xs.device, dtype=torch.float32)
        return ops.mlp_fwd_rays(rays, z, model.packed_weights(), False, model.mlp_dtype).view(n, 4)
    pts = torch.stack([xs[ix], ys[iy], zs[iz]], -1)
    x = torch.cat([embeddings[0](pts), embeddings[1](torch.zeros_like(pts))], 1)
    return model(x).view(n, 4)


def _check_embeddings(model, embeddings):
    if not model.is_default_arch() and (embeddings is None or len(embeddings) != 2):
        raise ValueError("a non-default NeRF needs its two Embeddings (embeddings=[embedding_xyz, embedding_dir])")


@torch.no_grad()
def rgbsigma_grid(model, N, x_range, y_range, z_range, points_per_launch=1 << 22, embeddings=None):
    """The notebook's `rgbsigma`: (N^3, 4) float32 on the device, full NeRF.forward on [Embedding_xyz(point), Embedding_dir(0)]
    for the points of np.meshgrid(x, y, z), row i = iy N^2 + ix N + iz.  The default architecture runs through the fused MLP
    kernel; any other shape layer by layer and needs `embeddings=[embedding_xyz, embedding_dir]`."""
    N = _check_lattice(N)
    dev = _model_device(model)
    _check_embeddings(model, embeddings)
    axes = _axes(N, x_range, y_range, z_range, dev)
    step = max(1, int(points_per_launch))
    out = torch.empty(N ** 3, 4, device=dev, dtype=torch.float32)
    for p0 in range(0, N ** 3, step):
        p1 = min(N ** 3, p0 + step)
        out[p0:p1] = _forward_points(model, N, axes, p0, p1, embeddings)
    return out


def _neg_cell(cell):
    return float(np.float32(-float(cell)))            # the quotient in float64, rounded once: what numpy's float32 * scalar does


def _pack(lib, rgbsigma, first_index, neg_cell, ws, records, cursor):
    check(lib.nerfhip_vol_pack(ptr(rgbsigma), rgbsigma.shape[0], int(first_index), neg_cell, ptr(ws), ptr(records), records.shape[0],
                               ptr(cursor), stream_ptr()), "nerfhip_vol_pack")


def _workspace(lib, n, dev):
    return torch.empty(lib.nerfhip_vol_workspace_bytes(n), device=dev, dtype=torch.uint8)


def _finish(records, cursor):
    K = int(cursor.item())                              # the one host read
    if K > records.shape[0]:
        raise NerfHipError("vol pack: %d records for a buffer of %d" % (K, records.shape[0]))
    return records if K == records.shape[0] else records[:K].clone()


@device_guard
def vol_records(rgbsigma, cell, first_index=0):
    """The file's records of `rgbsigma` (n, 4) float32 (a device tensor: the points first_index .. first_index+n-1 of the
    lattice), cell = (xmax - xmin) / N: a device (K, 2) int32 tensor whose bytes are the file
    (`.cpu().numpy().view(np.uint32)` is [[i, R<<24 | G<<16 | B<<8 | A], ...])."""
    if not torch.is_tensor(rgbsigma) or not rgbsigma.is_cuda:
        raise NerfHipError("nerf_pl_amd runs on MI355X only: vol_records needs a device tensor (no CPU fallback)")
    if rgbsigma.dtype != torch.float32 or rgbsigma.dim() != 2 or rgbsigma.shape[1] != 4:
        raise NerfHipError("vol_records: expected (n, 4) float32, got %s %s" % (tuple(rgbsigma.shape), rgbsigma.dtype))
    rgbsigma = rgbsigma.contiguous()
    n, first_index = rgbsigma.shape[0], int(first_index)
    if first_index < 0 or first_index + n > _MAX_POINTS:
        raise ValueError("vol_records: points %d .. %d do not fit the file's uint32 index" % (first_index, first_index + n - 1))
    dev = rgbsigma.device
    records = torch.empty(n, 2, device=dev, dtype=torch.int32)
    cursor = torch.zeros(1, device=dev, dtype=torch.int64)
    if n:
        lib = _lib.load()
        _pack(lib, rgbsigma, first_index, _neg_cell(cell), _workspace(lib, n, dev), records, cursor)
    return _finish(records, cursor)


@torch.no_grad()
def export_vol(model, N, x_range, y_range, z_range, path=None, cell=None, points_per_launch=1 << 22, embeddings=None):
    """The whole notebook cell: the records (K, 2) int32 on the device of `model` on the N^3 lattice, written to `path` when given.
    `cell` defaults to (x_range[1] - x_range[0]) / N as in the notebook (which wants the three ranges equally long).  The output
    buffer is sized for every point kept (8 N^3 bytes); the (N^3, 4) grid never exists; the result does not depend on
    `points_per_launch`."""
    N = _check_lattice(N)
    dev = _model_device(model)
    _check_embeddings(model, embeddings)
    with torch.cuda.device(dev):
        lib = _lib.load()
        axes = _axes(N, x_range, y_range, z_range, dev)
        neg_cell = _neg_cell((x_range[1] - x_range[0]) / N if cell is None else cell)
        total = N ** 3
        step = max(1, min(int(points_per_launch), total))
        records = torch.empty(total, 2, device=dev, dtype=torch.int32)
        cursor = torch.zeros(1, device=dev, dtype=torch.int64)
        ws = _workspace(lib, step, dev)
        for p0 in range(0, total, step):
            p1 = min(total, p0 + step)
            _pack(lib, _forward_points(model, N, axes, p0, p1, embeddings), p0, neg_cell, ws, records, cursor)
        records = _finish(records, cursor)
    if path is not None:
        write_vol(path, records)
    return records


def write_vol(path, records):
    """Write (K, 2) records (a tensor or array of int32 / uint32) as the .vol file; returns the number of bytes."""
    a = records.cpu().numpy() if torch.is_tensor(records) else np.asarray(records)
    if a.dtype.itemsize != 4 or a.dtype.kind not in "iu" or a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("write_vol: expected (K, 2) int32 / uint32 records, got %s %s" % (a.shape, a.dtype))
    data = np.ascontiguousarray(a).view(np.uint32).astype("<u4", copy=False).tobytes()
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


def read_vol(path_or_bytes, N):
    """The Texture3D the Unity loader builds from a .vol file: a dense (N, N, N, 4) uint8 RGBA array indexed [iy, ix, iz], zeros
    where the file has no record.  ValueError for a length that is not a multiple of 8, an index >= N^3, or indices that are
    not strictly increasing."""
    N = _check_lattice(N)
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as f:
            data = f.read()
    if len(data) % 8:
        raise ValueError("read_vol: %d bytes is not a whole number of 8-byte records" % len(data))
    rec = np.frombuffer(data, dtype="<u4").reshape(-1, 2)
    idx = rec[:, 0].astype(np.int64)
    if idx.size and int(idx.max()) >= N ** 3:
        raise ValueError("read_vol: index %d outside the %d^3 lattice" % (int(idx.max()), N))
    if idx.size > 1 and not bool((np.diff(idx) > 0).all()):
        raise ValueError("read_vol: indices are not strictly increasing")
    dense = np.zeros((N ** 3, 4), dtype=np.uint8)
    s = rec[:, 1]
    dense[idx] = np.stack([s >> 24, (s >> 16) & 255, (s >> 8) & 255, s & 255], -1).astype(np.uint8)
    return dense.reshape(N, N, N, 4)


def load_ckpt(model, ckpt_path, model_name="model"):
    """The reference's utils.load_ckpt: copy the entries `<model_name>.<key>` of a checkpoint (a pytorch-lightning one keeps
    them under 'state_dict') into `model`."""
    ckpt = torch.load(ckpt_path, map_location="cpu")
    ckpt = ckpt.get("state_dict", ckpt)
    state = model.state_dict()
    state.update({k[len(model_name) + 1:]: v for k, v in ckpt.items() if k.startswith(model_name)})
    model.load_state_dict(state)
    return model


def main(argv=None):
    import argparse
    from .models import NeRF
    ap = argparse.ArgumentParser(description="Write <scene_name>.vol (Unity volume rendering) from a trained NeRF")
    ap.add_argument("--ckpt_path", required=True)
    ap.add_argument("--scene_name", required=True)
    ap.add_argument("--N", type=int, default=512, help="lattice size (the Unity loader wants 512)")
    for ax in "xyz":
        ap.add_argument("--%s_range" % ax, nargs=2, type=float, default=[-1.2, 1.2])
    a = ap.parse_args(argv)
    model = NeRF()
    load_ckpt(model, a.ckpt_path, model_name="nerf_fine")
    model.cuda().eval()
    path = a.scene_name + ".vol"
    rec = export_vol(model, a.N, tuple(a.x_range), tuple(a.y_range), tuple(a.z_range), path=path)
    print("%s: %d records of %d lattice points" % (path, rec.shape[0], a.N ** 3))


if __name__ == "__main__":
    main()

"""`datasets/llff.py` of the reference (LLFFDataset, :159-318, and its pose helpers, :12-156) with every per-pixel operation on
the device.

The host reads each image file, parses its markers and Huffman-decodes the scan (imageio_min.jpeg_parse,
ops.jpeg_entropy_decode: C++, no GPU); the coefficient blocks go to HBM and the inverse DCT, chroma upsampling, colour
conversion, Pillow's Lanczos resize and ToTensor run as HIP kernels (csrc/jpeg.hip, csrc/image.hip) whose bytes and floats
equal what the reference's PIL + torchvision pipeline produces.  With jpeg_entropy="gpu" the scans are uploaded as the files' bytes and
Huffman-decoded on the device as well (ops.jpeg_entropy_decode_batch, csrc/jpeg_entropy.hip), to the same coefficients.  A file with the PNG signature in `images/` takes the PNG path
of the Blender loader.  The COLMAP pose handling stays on the host in float64 numpy, as in the reference.  Attribute names and
semantics are the reference's; tensors live on the device."""
import glob
import os

import numpy as np
import torch

from .. import ops, rays
from .._lib import NerfHipError
from ..imageio_min import jpeg_parse, png_idat, png_inflate

_STAGING_BYTES = 256 << 20   # RGBX bytes decoded per batch: 5 images of 4032 x 3024 (48.8 MB each, 2.2 x that with the planes
                             # and coefficients beside it), any number of small ones up to _BATCH_MAX
_BATCH_MAX = 64


def normalize(v):
    """v / |v| (llff.py:12-14)"""
    return v / np.linalg.norm(v)


def _frame(z, up, origin):
    """(3, 4) pose [x y z origin] looking along `z` (need not be unit) with `up` roughly upwards: x = up x z, y = z x x"""
    z = normalize(z)
    x = normalize(np.cross(up, z))
    return np.stack([x, np.cross(z, x), z, origin], 1)


def average_poses(poses):
    """(N, 3, 4) -> (3, 4): the mean camera centre, the normalised mean z axis, and x, y completed from the mean y axis
    (llff.py:17-53)"""
    return _frame(poses[..., 2].mean(0), poses[..., 1].mean(0), poses[..., 3].mean(0))


def center_poses(poses):
    """(N, 3, 4) -> (the poses expressed in the average pose's frame (N, 3, 4), the inverse of the homogeneous average pose
    (4, 4)) (llff.py:56-80)"""
    avg = np.eye(4)
    avg[:3] = average_poses(poses)
    homo = np.tile(np.eye(4), (len(poses), 1, 1))
    homo[:, :3] = poses
    inv = np.linalg.inv(avg)
    return (inv @ homo)[:, :3], inv


def create_spiral_poses(radii, focus_depth, n_poses=120):
    """Two turns of a spiral of per-axis `radii` around the origin, every pose looking at the point `focus_depth` in front
    (llff.py:83-115) -> (n_poses, 3, 4)"""
    out = []
    for t in np.linspace(0, 4 * np.pi, n_poses + 1)[:-1]:
        center = np.array([np.cos(t), -np.sin(t), -np.sin(0.5 * t)]) * radii
        out.append(_frame(center - np.array([0, 0, -focus_depth]), np.array([0, 1, 0]), center))
    return np.stack(out, 0)


def create_spheric_poses(radius, n_poses=120):
    """A circle around the z axis at height and distance set by `radius`, looking 36 degrees down (llff.py:118-156)
    -> (n_poses, 3, 4)"""
    phi = -np.pi / 5
    shift = np.array([[1, 0, 0, 0], [0, 1, 0, -0.9 * radius], [0, 0, 1, radius], [0, 0, 0, 1]])
    tilt = np.array([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]])
    swap = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    out = []
    for th in np.linspace(0, 2 * np.pi, n_poses + 1)[:-1]:
        turn = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]])
        out.append((swap @ (turn @ tilt @ shift))[:3])
    return np.stack(out, 0)


class LLFFDataset(torch.utils.data.Dataset):
    def __init__(self, root_dir, split='train', img_wh=(504, 378), spheric_poses=False, val_num=1, device=None, jpeg_entropy="host",
                 png_inflate="host"):
        """spheric_poses: the images were taken facing inwards around an object (default: forward-facing, NDC rays)
        val_num: number of val images (the same image, once per GPU)
        jpeg_entropy: "host" Huffman-decodes every JPEG scan on the CPU (ops.jpeg_entropy_decode) and uploads the coefficients;
        "gpu" uploads the scans' bytes and decodes each batch on the device (ops.jpeg_entropy_decode_batch).  Same colours.
        png_inflate: "host" inflates every PNG file with zlib on the CPU and uploads the scanlines; "gpu" uploads the files' IDAT
        bytes and inflates each batch on the device (ops.inflate_batch).  Same colours."""
        if jpeg_entropy not in ("host", "gpu"):
            raise ValueError('jpeg_entropy must be "host" or "gpu", got %r' % (jpeg_entropy,))
        if png_inflate not in ("host", "gpu"):
            raise ValueError('png_inflate must be "host" or "gpu", got %r' % (png_inflate,))
        self.jpeg_entropy = jpeg_entropy
        self.png_inflate = png_inflate
        self.root_dir = root_dir
        self.split = split
        self.img_wh = img_wh
        self.spheric_poses = spheric_poses
        self.val_num = max(1, val_num)
        if device is None:
            if not torch.cuda.is_available():
                raise NerfHipError("LLFFDataset decodes and resizes on an MI355X: no GPU is visible (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NerfHipError("nerf_pl_amd runs on MI355X only: got device %s (no CPU fallback)" % self.device)
        self._all_rays = None
        self.read_meta()
        self.white_back = False

    def read_meta(self):
        poses_bounds = np.load(os.path.join(self.root_dir, 'poses_bounds.npy'))            # (N_images, 17)
        self.image_paths = sorted(glob.glob(os.path.join(self.root_dir, 'images/*')))
        if self.split in ['train', 'val']:
            assert len(poses_bounds) == len(self.image_paths), \
                'Mismatch between number of images and number of poses! Please rerun COLMAP!'

        poses = poses_bounds[:, :15].reshape(-1, 3, 5)                                     # (N_images, 3, 5)
        self.bounds = poses_bounds[:, -2:].copy()                                          # (N_images, 2)

        # the files' intrinsics (the same for every image), the focal length rescaled to the training resolution
        H, W, self.focal = poses[0, :, -1]
        w, h = self.img_wh
        assert H * w == W * h, 'You must set @img_wh to have the same aspect ratio as (%s, %s) !' % (W, H)
        self.focal *= w / W

        # COLMAP's rotation columns are "down right back"; the renderer wants "right up back".  Then centre on the average pose
        poses = np.concatenate([poses[..., 1:2], -poses[..., :1], poses[..., 2:4]], -1)    # (N_images, 3, 4)
        self.poses, self.pose_avg = center_poses(poses)
        self._val_idx = int(np.argmin(np.linalg.norm(self.poses[..., 3], axis=1)))         # the pose nearest the centre

        # rescale the scene so that the nearest depth lies at 1 / 0.75
        scale_factor = self.bounds.min() * 0.75
        self.bounds /= scale_factor
        self.poses[..., 3] /= scale_factor

        # ray directions for all pixels, same for all images (same H, W, focal)
        self.directions = rays.get_ray_directions(h, w, self.focal, device=self.device)    # (h, w, 3)

        if self.split == 'train':      # colours of every image but the val one; all_rays is formed on first access
            self._train_ids = [i for i in range(len(self.image_paths)) if i != self._val_idx]
            paths = [self.image_paths[i] for i in self._train_ids]
            self.all_rgbs = torch.empty(len(paths) * h * w, 3, device=self.device, dtype=torch.float32)
            self._load(paths, out=self.all_rgbs)
        elif self.split == 'val':
            print('val image is', self.image_paths[self._val_idx])
            self.c2w_val = self.poses[self._val_idx]
            self.image_path_val = self.image_paths[self._val_idx]
        else:                          # a rendering path
            if self.split.endswith('train'):
                self.poses_test = self.poses
            elif not self.spheric_poses:
                radii = np.percentile(np.abs(self.poses[..., 3]), 90, axis=0)
                self.poses_test = create_spiral_poses(radii, 3.5)      # focus depth as hard-coded by the reference
            else:
                self.poses_test = create_spheric_poses(1.1 * self.bounds.min())

    # ---- image files -> colours --------------------------------------------------------------------------------------------
    def _read(self, path):
        """One file -> ('png', (W, H, ch), stream) or ('jpeg', (W, H, n_comp, hs, vs), (coefficient blocks — or, with
        jpeg_entropy="gpu", the parsed file —, quantisation tables)), by the file's signature."""
        with open(path, "rb") as f:
            data = f.read()
        if data[:8] == b"\x89PNG\r\n\x1a\n":
            W, H, ch, raw = png_idat(data) if self.png_inflate == "gpu" else png_inflate(data)
            if ch not in (3, 4):
                raise ValueError("%s: a %d-channel PNG; RGB or RGBA expected" % (path, ch))
            if self.png_inflate == "gpu":    # the IDAT data stays as the file's bytes: _decode inflates the batch on the device
                return 'png', (W, H, ch), (path, raw)
            return 'png', (W, H, ch), np.frombuffer(raw, dtype=np.uint8)
        if data[:2] != b"\xff\xd8":
            raise ValueError("%s: neither a JPEG nor a PNG file" % path)
        try:
            parsed = jpeg_parse(data)
        except ValueError as e:
            raise ValueError(str(e).replace("JPEG data", path, 1)) from None
        parsed["name"] = path
        comps = parsed["components"]
        quant = np.stack([parsed["quant"][c[3]] for c in comps]).astype(np.int16)
        shape = (parsed["width"], parsed["height"], len(comps), comps[0][1], comps[0][2])
        if self.jpeg_entropy == "gpu":       # the scan stays as the file's bytes: _decode decodes the batch on the device
            return 'jpeg', shape, (parsed, quant)
        return 'jpeg', shape, (ops.jpeg_entropy_decode(parsed), quant)

    def _decode(self, kind, shape, items):
        """Files of one kind and shape -> (n, H, W, 4) uint8 on the device, alpha 255."""
        if kind == 'png':
            W, H, ch = shape
            if self.png_inflate == "gpu":
                streams = ops.inflate_batch([it[1] for it in items], H * (1 + W * ch), self.device, names=[it[0] for it in items])
            else:
                streams = torch.from_numpy(np.stack(items)).to(self.device)
            px = ops.decode_png_batch(streams, H, W, ch)
            rgbx = torch.full((len(items), H, W, 4), 255, device=self.device, dtype=torch.uint8)
            rgbx[..., :3] = px[..., :3]                  # convert('RGB') drops the alpha channel
            return rgbx
        W, H, n_comp, hs, vs = shape
        if self.jpeg_entropy == "gpu":
            coefs = ops.jpeg_entropy_decode_batch([it[0] for it in items], self.device)
        else:
            coefs = [torch.from_numpy(np.stack([it[0][c].reshape(-1, 64) for it in items])).to(self.device) for c in range(n_comp)]
        quant = torch.from_numpy(np.stack([it[1] for it in items])).to(self.device)
        return ops.decode_jpeg_batch(coefs, quant, H, W, hs, vs)

    def _load(self, paths, out=None):
        """Files -> rgb (len(paths) * h * w, 3) float32 on the device: decode, Image.resize(img_wh, LANCZOS), ToTensor.  Runs of
        consecutive files of one kind and shape are decoded together, in batches that bound the staging."""
        w, h = self.img_wh
        if out is None:
            out = torch.empty(len(paths) * h * w, 3, device=self.device, dtype=torch.float32)
        done, pending, key = 0, [], None

        def flush():
            nonlocal done, pending
            if pending:
                rgbx = self._decode(key[0], key[1], pending)
                rgbx = ops.resize_rgba_lanczos(rgbx, w, h)
                # alpha is 255 everywhere: the blend onto white is c / 255 * 1 + 0, which is ToTensor
                ops.rgba_to_rgb_white(rgbx, out=out[done * h * w:(done + len(pending)) * h * w])
                done += len(pending)
                pending = []

        for p in paths:
            kind, shape, item = self._read(p)
            W, H = shape[:2]
            assert H * w == W * h, '%s has different aspect ratio than img_wh, please check your data!' % p
            limit = max(1, min(_BATCH_MAX, _STAGING_BYTES // (4 * W * H)))
            if key != (kind, shape) or len(pending) >= limit:
                flush()
                key = (kind, shape)
            pending.append(item)
        flush()
        return out

    # ---- rays --------------------------------------------------------------------------------------------------------------
    def _ray_settings(self):
        """(near, far, use_ndc): forward-facing scenes use NDC rays with the near plane at 1 (llff.py:236-245)"""
        if not self.spheric_poses:
            return 0.0, 1.0, True
        near = self.bounds.min()
        return float(near), float(min(8 * near, self.bounds.max())), False

    def _gen_rays(self, c2w):
        w, h = self.img_wh
        near, far, ndc = self._ray_settings()
        return rays.gen_rays(c2w, h, w, self.focal, near, far, use_ndc=ndc, ndc_near_plane=1.0)

    def _pose_tensor(self):
        return torch.from_numpy(self.poses[self._train_ids].astype(np.float32)).to(self.device)

    @property
    def all_rays(self):
        """(n_images * h * w, 8) = [o d near far] of every training pixel, formed on first access (RayStore never needs it)."""
        if self.split != 'train':
            raise AttributeError("all_rays exists for the train split only")
        if self._all_rays is None:
            self._all_rays = self._gen_rays(self._pose_tensor())
        return self._all_rays

    def ray_store(self):
        """The device-resident training set over this split's poses and colours (batches drawn and their rays made on the GPU)."""
        if self.split != 'train':
            raise ValueError("ray_store() is for the train split")
        w, h = self.img_wh
        near, far, ndc = self._ray_settings()
        return rays.RayStore(self._pose_tensor(), self.all_rgbs, h, w, self.focal, near, far, use_ndc=ndc, ndc_near_plane=1.0)

    def __len__(self):
        if self.split == 'train':
            return len(self.all_rays)
        if self.split == 'val':
            return self.val_num
        return len(self.poses_test)

    def __getitem__(self, idx):
        if self.split == 'train':   # use data in the buffers
            return {'rays': self.all_rays[idx], 'rgbs': self.all_rgbs[idx]}
        c2w = torch.FloatTensor(self.c2w_val if self.split == 'val' else self.poses_test[idx]).to(self.device)
        sample = {'rays': self._gen_rays(c2w), 'c2w': c2w}
        if self.split == 'val':
            sample['rgbs'] = self._load([self.image_path_val])
        return sample

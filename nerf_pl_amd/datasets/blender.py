"""`datasets/blender.py` of the reference (BlenderDataset, :11-109) with every per-pixel operation on the device.

The host reads each PNG and inflates it (zlib); the filtered scanlines go to HBM and the PNG reconstruction, Pillow's Lanczos
resize, ToTensor and the blend onto white run as HIP kernels (csrc/image.hip) whose bytes and floats equal what the reference's
PIL + torchvision pipeline produces.  With png_inflate="gpu" the files' IDAT data goes up as it stands and each batch is inflated
on the device as well (ops.inflate_batch, csrc/inflate.hip), to the same scanlines.  Attribute names and semantics are the reference's; tensors live on the device."""
import json
import os

import numpy as np
import torch

from .. import ops, rays
from .._lib import NerfHipError
from ..imageio_min import png_idat, png_inflate

_BATCH = 16            # images decoded per launch: bounds the uint8 staging (16 x 800 x 800 x 4 = 41 MB, three such buffers)


class BlenderDataset(torch.utils.data.Dataset):
    def __init__(self, root_dir, split='train', img_wh=(800, 800), device=None, png_inflate="host"):
        """png_inflate: "host" inflates every file with zlib on the CPU and uploads the scanlines; "gpu" uploads the files' IDAT
        bytes and inflates each batch on the device (ops.inflate_batch).  Same colours."""
        if png_inflate not in ("host", "gpu"):
            raise ValueError('png_inflate must be "host" or "gpu", got %r' % (png_inflate,))
        self.png_inflate = png_inflate
        self.root_dir = root_dir
        self.split = split
        assert img_wh[0] == img_wh[1], 'image width must equal image height!'
        self.img_wh = img_wh
        if device is None:
            if not torch.cuda.is_available():
                raise NerfHipError("BlenderDataset decodes and resizes on an MI355X: no GPU is visible (no CPU fallback)")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NerfHipError("nerf_pl_amd runs on MI355X only: got device %s (no CPU fallback)" % self.device)
        self._all_rays = None
        self.read_meta()
        self.white_back = True

    def read_meta(self):
        with open(os.path.join(self.root_dir, "transforms_%s.json" % self.split), 'r') as f:
            self.meta = json.load(f)

        w, h = self.img_wh
        self.focal = 0.5 * 800 / np.tan(0.5 * self.meta['camera_angle_x'])   # original focal length when W=800
        self.focal *= self.img_wh[0] / 800                                     # modify focal length to match size self.img_wh

        # bounds, common for all scenes
        self.near = 2.0
        self.far = 6.0
        self.bounds = np.array([self.near, self.far])

        # ray directions for all pixels, same for all images (same H, W, focal)
        self.directions = rays.get_ray_directions(h, w, self.focal, device=self.device)   # (h, w, 3)

        if self.split == 'train':   # buffers of all poses and rgb data; all_rays is formed on first access
            self.image_paths = [self._path(frame) for frame in self.meta['frames']]
            self.poses = [np.array(frame['transform_matrix'])[:3, :4] for frame in self.meta['frames']]
            n = len(self.image_paths)
            self.all_rgbs = torch.empty(n * h * w, 3, device=self.device, dtype=torch.float32)
            for i in range(0, n, _BATCH):
                self._load(self.image_paths[i:i + _BATCH], out=self.all_rgbs[i * h * w:(i + _BATCH) * h * w])

    def _path(self, frame):
        return os.path.join(self.root_dir, "%s.png" % frame['file_path'])

    def _load(self, paths, out=None):
        """Files -> (rgb (len(paths) * h * w, 3) float32, valid_mask (len(paths) * h * w,) bool) on the device."""
        w, h = self.img_wh
        size, rows = None, []
        gpu = self.png_inflate == "gpu"
        for p in paths:
            W, H, ch, raw = png_idat(p) if gpu else png_inflate(p)
            if ch != 4:
                raise ValueError("%s: %d channels; Blender scenes are RGBA (the reference's view(4, -1) needs it too)" % (p, ch))
            if size is None:
                size = (W, H)
            elif size != (W, H):
                raise ValueError("%s is %d x %d, the files before it %d x %d" % (p, W, H, size[0], size[1]))
            rows.append(raw if gpu else np.frombuffer(raw, dtype=np.uint8))
        W, H = size
        if gpu:
            streams = ops.inflate_batch(rows, H * (1 + W * 4), self.device, names=list(paths))
        else:
            streams = torch.from_numpy(np.stack(rows)).to(self.device)
        rgba = ops.decode_png_batch(streams, H, W, 4)
        rgba = ops.resize_rgba_lanczos(rgba, w, h)
        return ops.rgba_to_rgb_white(rgba, out=out)

    def _pose_tensor(self):
        return torch.from_numpy(np.stack(self.poses).astype(np.float32)).to(self.device)

    @property
    def all_rays(self):
        """(n_images * h * w, 8) = [o d near far] of every training pixel, formed on first access (RayStore never needs it)."""
        if self.split != 'train':
            raise AttributeError("all_rays exists for the train split only")
        if self._all_rays is None:
            w, h = self.img_wh
            self._all_rays = rays.gen_rays(self._pose_tensor(), h, w, self.focal, self.near, self.far)
        return self._all_rays

    def ray_store(self):
        """The device-resident training set over this split's poses and colours (batches drawn and their rays made on the GPU)."""
        if self.split != 'train':
            raise ValueError("ray_store() is for the train split")
        w, h = self.img_wh
        return rays.RayStore(self._pose_tensor(), self.all_rgbs, h, w, self.focal, self.near, self.far)

    def __len__(self):
        if self.split == 'train':
            return len(self.all_rays)
        if self.split == 'val':
            return 8   # only validate 8 images (to support <=8 gpus)
        return len(self.meta['frames'])

    def __getitem__(self, idx):
        if self.split == 'train':   # use data in the buffers
            return {'rays': self.all_rays[idx], 'rgbs': self.all_rgbs[idx]}
        # create data for each image separately
        frame = self.meta['frames'][idx]
        w, h = self.img_wh
        c2w = torch.FloatTensor(frame['transform_matrix'])[:3, :4].to(self.device)
        img, valid_mask = self._load([self._path(frame)])
        return {'rays': rays.gen_rays(c2w, h, w, self.focal, self.near, self.far),   # (H*W, 8)
                'rgbs': img,
                'c2w': c2w,
                'valid_mask': valid_mask}

"""Whole-image inference: the reference's `eval.py:batched_inference` (eval.py:58-86) and an
MI355X-specific variant that replays the fixed-shape 32768-ray chunk as one hipGraph and shards the
ray list across ranks (BASELINE.json configs[4]).

`batched_inference` keeps the reference's signature and behaviour (chunk forced to 32768 rays,
perturb=0, noise_std=0, test_time=True => sigma-only coarse pass, keys opacity_coarse / rgb_fine /
depth_fine / opacity_fine concatenated over chunks).
"""
from collections import defaultdict

import torch

from . import ops
from .models.rendering import _fusable, render_rays

EVAL_CHUNK = 1024 * 32          # eval.py:65 hard-codes this, ignoring --chunk


@torch.no_grad()
def batched_inference(models, embeddings, rays, N_samples, N_importance, use_disp, chunk, white_back):
    """Do batched inference on rays using chunk (eval.py:58-86; `white_back` is the argument the
    reference declares but then shadows with the global `dataset.white_back`, eval.py:78)."""
    B = rays.shape[0]
    chunk = EVAL_CHUNK
    results = defaultdict(list)
    for i in range(0, B, chunk):
        rendered_ray_chunks = render_rays(models, embeddings, rays[i:i + chunk], N_samples, use_disp, 0, 0,
                                          N_importance, chunk, white_back, test_time=True)
        for k, v in rendered_ray_chunks.items():
            results[k] += [v]
    for k, v in results.items():
        results[k] = torch.cat(v, 0)
    return results


def _render_test_time(models, rays, N_samples, N_importance, use_disp, white_back):
    """The test_time launch sequence of render_rays without the (unused, noise_std=0) RNG draws:
    sample_coarse_z -> mlp(coarse, sigma only) -> composite -> fine_z -> mlp(fine) -> composite.
    Allocation-free apart from torch.empty outputs => capturable.
    Where the single-launch kernel takes the shape (nerfhip_render_test_fwd: sigma-only coarse sub-passes, round 6) the whole
    sequence is that ONE launch — the same bits (tests/test_gpu_render_fused.py)."""
    from .models import rendering as R
    dtype = models[0].mlp_dtype
    if (R.FUSE_TEST_TIME and N_importance > 0 and models[1].mlp_dtype == dtype
            and ops.render_supported(rays.shape[0], N_samples, N_importance, dtype)):
        o = ops.render_fwd(rays, N_samples, N_importance, models[0].packed_weights(), models[1].packed_weights(), dtype, use_disp, 0.0, None,
                           None, None, 0.0, white_back, None, want_coarse=False, test_time=True)
        return {k: o[k] for k in ("opacity_coarse", "rgb_fine", "depth_fine", "opacity_fine")}
    z = ops.sample_coarse_z(rays, N_samples, use_disp, 0.0, None)
    sig = ops.mlp_fwd_rays(rays, z, models[0].packed_weights(), True, models[0].mlp_dtype)
    w, opac_c = ops.composite(sig, z, rays, None, 0.0, white_back)
    out = {"opacity_coarse": opac_c}
    if N_importance > 0:
        zf = ops.fine_z(z, w, N_importance, u=None)
        raw = ops.mlp_fwd_rays(rays, zf, models[1].packed_weights(), False, models[1].mlp_dtype)
        _, opac_f, rgb_f, depth_f = ops.composite(raw, zf, rays, None, 0.0, white_back)
        out.update(rgb_fine=rgb_f, depth_fine=depth_f, opacity_fine=opac_f)
    return out


class GraphRenderer:
    """hipGraph-captured inference of one fixed-shape ray chunk (default 32768 rays).

    The six launches of a test-time `render_rays` are captured once on static buffers
    (`torch.cuda.CUDAGraph` == hipGraph on ROCm; libnerfhip launches on torch's current stream, which
    is the capturing stream, allocates nothing and never synchronises) and replayed per chunk; a
    ragged tail chunk is padded with copies of its last ray and the outputs sliced.  Weights are
    re-packed (outside the graph, into the same packed buffers the graph reads) when they change."""

    def __init__(self, models, embeddings, N_samples=64, N_importance=128, use_disp=False, white_back=True,
                 chunk=EVAL_CHUNK, device=None):
        if not _fusable(models, embeddings):
            raise NotImplementedError("GraphRenderer needs the reference's default NeRF/Embedding configuration")
        self.models = list(models)
        self.cfg = (int(N_samples), int(N_importance), bool(use_disp), bool(white_back))
        self.chunk = int(chunk)
        dev = device or next(models[0].parameters()).device
        self.rays = torch.zeros(self.chunk, 8, device=dev, dtype=torch.float32)
        self.rays[:, 5] = 1.0
        self.rays[:, 6] = 2.0
        self.rays[:, 7] = 6.0
        self.graph = None
        self.out = None
        self._capture()

    def _pack(self):
        for m in self.models:
            m.packed_weights()          # repack into the same device buffers the captured graph reads

    def _capture(self):
        with torch.cuda.device(self.rays.device):       # streams and the graph belong to the GPU that owns the buffers
            self._capture_on_device()

    def _capture_on_device(self):
        self._pack()
        S, N, disp, wb = self.cfg
        side = torch.cuda.Stream(device=self.rays.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):           # warm-up outside capture (module load, allocator pools)
                _render_test_time(self.models, self.rays, S, N, disp, wb)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # (thread_local: an RCCL watchdog thread polling events elsewhere in the process must not abort the capture)
        with torch.no_grad(), torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.out = _render_test_time(self.models, self.rays, S, N, disp, wb)

    @torch.no_grad()
    def render_chunk(self, rays):
        n = rays.shape[0]
        if n > self.chunk:
            raise ValueError("chunk larger than the captured shape")
        with torch.cuda.device(self.rays.device):
            self._pack()
            self.rays[:n].copy_(rays)
            if n < self.chunk:
                self.rays[n:].copy_(rays[n - 1:n].expand(self.chunk - n, 8))
            self.graph.replay()
            return {k: v[:n].clone() for k, v in self.out.items()}

    @torch.no_grad()
    def render_to_host(self, rays, keys=("rgb_fine", "depth_fine")):
        """Whole ray list -> PINNED host tensors, with the device-to-host copy of every finished chunk overlapped with
        the replay of the next one (eval.py:123-131 does `.cpu()` on the whole image after the last chunk).

        Compute stream: replay chunk i, then copy its outputs into slice i of a device-side image buffer (the graph's
        static outputs are overwritten by the next replay; the slice is not) and record an event.  Copy stream: wait for
        that event, DMA the slice into the pinned buffer.  Only the last chunk's copy is exposed."""
        with torch.cuda.device(self.rays.device):       # current stream / copy stream of the GPU that owns the buffers
            return self._render_to_host(rays, keys)

    def _render_to_host(self, rays, keys):
        n = rays.shape[0]
        dev = self.rays.device
        cur = torch.cuda.current_stream(dev)
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        img = {k: torch.empty((n,) + tuple(self.out[k].shape[1:]), device=dev, dtype=torch.float32) for k in keys}
        host = {k: torch.empty(v.shape, dtype=torch.float32, pin_memory=True) for k, v in img.items()}
        self._pack()
        for i in range(0, n, self.chunk):
            m = min(self.chunk, n - i)
            self.rays[:m].copy_(rays[i:i + m])
            if m < self.chunk:
                self.rays[m:].copy_(rays[i + m - 1:i + m].expand(self.chunk - m, 8))
            self.graph.replay()
            for k in keys:
                img[k][i:i + m].copy_(self.out[k][:m])
            done = torch.cuda.Event()
            done.record(cur)
            self._copy_stream.wait_event(done)
            with torch.cuda.stream(self._copy_stream):
                for k in keys:
                    host[k][i:i + m].copy_(img[k][i:i + m], non_blocking=True)
        cur.wait_stream(self._copy_stream)
        self._copy_stream.synchronize()
        return host

    @torch.no_grad()
    def __call__(self, rays):
        """Same result dict as batched_inference for a whole ray list."""
        results = defaultdict(list)
        for i in range(0, rays.shape[0], self.chunk):
            for k, v in self.render_chunk(rays[i:i + self.chunk]).items():
                results[k] += [v]
        return {k: (torch.cat(v, 0) if len(v) > 1 else v[0]) for k, v in results.items()}


def save_image_outputs(results, h, w, dir_name, index, save_depth=False, depth_format="pfm"):
    """The per-image tail of the reference's eval loop (eval.py:123-141): `results` holds host (or device) tensors
    rgb_fine (h*w, 3) and depth_fine (h*w,); writes `{index:03d}.png` and, when asked, `depth_{index:03d}.pfm` or the raw
    float32 bytes.  Returns the uint8 image (the reference collects them for the gif, eval.py:140,149)."""
    import os

    import numpy as np

    from .imageio_min import depth_bytes, save_pfm, write_png
    img_pred = results["rgb_fine"].reshape(h, w, 3).cpu().numpy()
    if save_depth:
        depth_pred = np.nan_to_num(results["depth_fine"].reshape(h, w).cpu().numpy())
        if depth_format == "pfm":
            save_pfm(os.path.join(dir_name, "depth_%03d.pfm" % index), depth_pred)
        else:
            with open(os.path.join(dir_name, "depth_%03d" % index), "wb") as f:
                f.write(depth_bytes(depth_pred))
    img_pred_ = (img_pred * 255).astype(np.uint8)
    write_png(os.path.join(dir_name, "%03d.png" % index), img_pred_)
    return img_pred_


def image_to_u8(rgb):
    """trunc(float32(rgb * 255)) as uint8 on the device — eval.py:136 `(img_pred * 255).astype(np.uint8)` before the copy to
    the host instead of after it: 3 bytes per pixel cross the bus instead of 12 (`nerfhip_mesh_rgb_to_u8`)."""
    return ops.rgb_to_u8(rgb)


@torch.no_grad()
def evaluate(dataset, renderer, dir_name=None, save_depth=False, depth_format="pfm", window_size=3, gif_path=None, fps=30,
             png_encoder="host"):
    """The loop of the reference's eval.py (eval.py:112-149) with its tail on the GPU.

    dataset: `len`, `img_wh` = (w, h), items with 'rays' (h*w, 8) and optionally 'rgbs' (h*w, 3).  renderer: rays on the GPU ->
    a dict with 'rgb_fine' (h*w, 3) and 'depth_fine' (h*w,) (a `GraphRenderer`, or a closure over `batched_inference`).
    Per image: render; PSNR and SSIM against the ground truth on the device; uint8 on the device; copy the bytes to the host;
    with `dir_name`, write `{i:03d}.png` and (save_depth) `depth_{i:03d}.pfm` / `depth_{i:03d}` as `save_image_outputs` does.
    The metric scalars stay on the device and are read once, after the last image.
    With `gif_path`, the uint8 frames also stay on the device, `imageio_min.GIF_BATCH` (8) at a time: a full batch is quantised
    and LZW-coded there (`imageio_min.GifWriter`) and its data appended on the host, and the file is written after the loop as
    `imageio.mimsave(gif_path, imgs, fps=fps)` of eval.py:145 is.  A batch holds per frame 3 bytes per pixel of frames, 1 of
    indices, about 1.5 of worst-case data and 38.5 KB per 3838 pixels of strip workspace — about 10 MB at 800 x 800, 81 MB per
    batch.  With `gif_path=None` nothing of this runs: the returned dict and the files written are what they were.
    `png_encoder`: "host" (the default) writes `{i:03d}.png` with `imageio_min.write_png` (filter 0, zlib on the host); "gpu"
    encodes the uint8 image where it already is (`imageio_min.write_png_device`, DESIGN.md §15: adaptive filters, strip
    deflate and Adler-32 on the device) under the same name — the same pixels in a different, smaller file.  Anything else is
    a ValueError.

    Returns {'psnr': [...], 'ssim': [...], 'mean_psnr', 'mean_ssim', 'images': [(h, w, 3) uint8 arrays]} (the lists are empty
    and the means None for a dataset without ground truth)."""
    import os

    import numpy as np

    from . import metrics
    from .imageio_min import GIF_BATCH, GifWriter, depth_bytes, save_pfm, write_png, write_png_device
    if png_encoder not in ("host", "gpu"):
        raise ValueError("png_encoder must be 'host' or 'gpu', got %r" % (png_encoder,))
    w, h = dataset.img_wh
    if dir_name is not None:
        os.makedirs(dir_name, exist_ok=True)
    images, psnrs, ssims = [], [], []
    gif, pending = (GifWriter(fps), []) if gif_path is not None else (None, None)
    for i in range(len(dataset)):
        sample = dataset[i]
        rays = sample["rays"]
        dev = rays.device if rays.is_cuda else torch.device("cuda", torch.cuda.current_device())
        results = renderer(rays.to(dev))
        rgb = results["rgb_fine"].reshape(h * w, 3)
        if "rgbs" in sample:
            gt = sample["rgbs"].to(dev).reshape(h * w, 3)
            psnrs.append(metrics.psnr(gt, rgb))                      # eval.py:143's argument order
            ssims.append(metrics.ssim_hw3(rgb, gt, h, w, window_size=window_size))
        img_dev = image_to_u8(rgb).reshape(h, w, 3)
        img = img_dev.cpu().numpy()
        images.append(img)
        if gif is not None:
            pending.append(img_dev)
            if len(pending) == GIF_BATCH:
                gif.append(torch.stack(pending))
                pending = []
        if dir_name is None:
            continue
        if save_depth:
            depth = np.nan_to_num(results["depth_fine"].reshape(h, w).cpu().numpy())
            if depth_format == "pfm":
                save_pfm(os.path.join(dir_name, "depth_%03d.pfm" % i), depth)
            else:
                with open(os.path.join(dir_name, "depth_%03d" % i), "wb") as f:
                    f.write(depth_bytes(depth))
        if png_encoder == "gpu":
            write_png_device([os.path.join(dir_name, "%03d.png" % i)], img_dev.unsqueeze(0))
        else:
            write_png(os.path.join(dir_name, "%03d.png" % i), img)
    if gif is not None and images:
        if pending:
            gif.append(torch.stack(pending))
        with open(gif_path, "wb") as f:
            f.write(gif.getvalue())
    out = {"psnr": [], "ssim": [], "mean_psnr": None, "mean_ssim": None, "images": images}
    if psnrs:
        both = torch.stack([torch.stack(psnrs), torch.stack(ssims)]).cpu().numpy()       # the one read of the metric scalars
        out["psnr"], out["ssim"] = both[0].tolist(), both[1].tolist()
        out["mean_psnr"], out["mean_ssim"] = float(np.mean(out["psnr"])), float(np.mean(out["ssim"]))
    return out

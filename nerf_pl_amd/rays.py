"""`datasets/ray_utils.py` of the reference on the device, plus a device-resident ray/pixel store.

`get_ray_directions`, `get_rays`, `get_ndc_rays` keep the reference signatures (ray_utils.py:5-94) and run as single HIP
launches; `RayStore` replaces the reference's CPU-side "precompute every ray of the dataset" pattern (blender.py:42-69,81-84):
it keeps only the camera poses and the pixel colours in HBM and regenerates each batch's rays from 8-byte pixel ids
(`nerfhip_gen_rays`), so a training batch never crosses PCIe.  Two ways to pick a batch's pixels: `RayStore.sample` draws them
with torch.randint — independently, WITH replacement, which is not what the reference's DataLoader does — and `EpochSampler`
(`RayStore.epoch_sampler`) is that DataLoader (train.py:89-94, shuffle=True): every ray once per epoch in a shuffled order."""
import ctypes

import torch

from . import _lib
from ._lib import check, device_guard, ptr, require_gpu, stream_ptr
from .models.nerf import pack_ticket


def get_ray_directions(H, W, focal, device="cuda"):
    """(H, W, 3) camera-space ray directions.  Reference: datasets/ray_utils.py:5-24."""
    dirs = torch.empty(H, W, 3, device=device, dtype=torch.float32)
    with torch.cuda.device(dirs.device):
        require_gpu(dirs)
        check(_lib.load().nerfhip_ray_directions(ptr(dirs), int(H), int(W), float(focal), stream_ptr()), "nerfhip_ray_directions")
    return dirs


@device_guard
def get_rays(directions, c2w):
    """rays_o, rays_d (H*W, 3) in world coordinates.  Reference: datasets/ray_utils.py:27-52."""
    require_gpu(directions)
    directions = directions.contiguous()
    c2w = c2w.to(directions.device, torch.float32).contiguous()
    if c2w.shape != (3, 4):
        raise ValueError("c2w must be (3, 4)")
    n = directions.numel() // 3
    rays_o = torch.empty(n, 3, device=directions.device, dtype=torch.float32)
    rays_d = torch.empty(n, 3, device=directions.device, dtype=torch.float32)
    check(_lib.load().nerfhip_get_rays(ptr(directions), ptr(c2w), ptr(rays_o), ptr(rays_d), n, stream_ptr()), "nerfhip_get_rays")
    return rays_o, rays_d


@device_guard
def get_ndc_rays(H, W, focal, near, rays_o, rays_d):
    """World rays -> NDC rays.  Reference: datasets/ray_utils.py:55-94."""
    require_gpu(rays_o, rays_d)
    rays_o, rays_d = rays_o.contiguous(), rays_d.contiguous()
    n = rays_o.numel() // 3
    out_o, out_d = torch.empty_like(rays_o), torch.empty_like(rays_d)
    check(_lib.load().nerfhip_ndc_rays(int(H), int(W), float(focal), float(near), ptr(rays_o), ptr(rays_d), ptr(out_o), ptr(out_d),
                                       n, stream_ptr()), "nerfhip_ndc_rays")
    return out_o, out_d


@device_guard
def gen_rays(c2w, H, W, focal, near, far, pixel_ids=None, first_pixel=0, n=None, use_ndc=False, ndc_near_plane=1.0):
    """rays (n, 8) = [o d near far] for global pixel ids (image*H*W + row*W + col) under poses c2w (n_images, 3, 4)."""
    require_gpu(c2w)
    c2w = c2w.contiguous()
    if c2w.dim() == 2:
        c2w = c2w[None]
    if pixel_ids is not None:
        if pixel_ids.dtype != torch.int64 or not pixel_ids.is_cuda:
            raise ValueError("pixel_ids must be an int64 device tensor")
        pixel_ids = pixel_ids.contiguous()
        n = pixel_ids.numel()
    elif n is None:
        n = c2w.shape[0] * H * W - first_pixel
    rays = torch.empty(n, 8, device=c2w.device, dtype=torch.float32)
    check(_lib.load().nerfhip_gen_rays(ptr(c2w), ptr(pixel_ids), int(first_pixel), int(n), int(H), int(W), float(focal),
                                       float(near), float(far), int(bool(use_ndc)), float(ndc_near_plane), ptr(rays), stream_ptr()),
          "nerfhip_gen_rays")
    return rays


class RayStore:
    """Device-resident training set: poses (n_img,3,4) + pixel colours (n_img*H*W, 3) in HBM; batches are drawn and
    their rays generated on the GPU.  `sample(B)` returns the reference's batch dict {'rays': (B,8), 'rgbs': (B,3)}
    (blender.py:81-84); `image_rays(i)` the (H*W, 8) rays of one image (validation / eval)."""

    def __init__(self, poses, rgbs, H, W, focal, near, far, use_ndc=False, ndc_near_plane=1.0):
        if not poses.is_cuda:
            require_gpu(poses)                          # raises: no CPU fallback
        with torch.cuda.device(poses.device):
            require_gpu(poses, rgbs)
        self.poses = poses.contiguous()
        self.rgbs = rgbs.reshape(-1, 3).contiguous()
        self.H, self.W, self.focal, self.near, self.far = int(H), int(W), float(focal), float(near), float(far)
        self.use_ndc, self.ndc_near_plane = bool(use_ndc), float(ndc_near_plane)
        self.n_pixels = self.poses.shape[0] * self.H * self.W
        if self.rgbs.shape[0] != self.n_pixels:
            raise ValueError("rgbs must hold n_images*H*W pixels")

    def __len__(self):
        return self.n_pixels

    def sample(self, batch_size, generator=None, step_draws=None, return_ids=False, pack_models=None):
        """One training batch in ONE launch (nerfhip_torch_draws with a ray batch): the pixel ids torch.randint(0, n_pixels,
        (batch_size,)) would draw from `generator` (default: the device's default generator, advanced identically), their rays
        and their colours.
        step_draws = (N_samples, N_importance, perturb, noise_std): the same launch also makes the draws the training step's
        render_rays will need (draws.step_specs: the reference's rand / randn calls, in its order, right after the batch's
        randint on the generator's stream) and returns them under batch['draws'] for NeRFSystem.training_step.
        pack_models = (models, mlp_dtype): the launch also packs the weight images the step's MLP kernels stream
        (nerfhip_train_prologue); batch['packed'] then names the models, and the fused training node skips its own pack launch
        while the weights are still the ones packed here."""
        from . import draws as D
        dev = self.poses.device
        B = int(batch_size)
        rays = torch.empty(B, 8, device=dev, dtype=torch.float32)
        rgbs = torch.empty(B, 3, device=dev, dtype=torch.float32)
        rb = _lib.RayBatch()
        rb.c2w, rb.rgbs_all, rb.rays, rb.rgbs = self.poses.data_ptr(), self.rgbs.data_ptr(), rays.data_ptr(), rgbs.data_ptr()
        rb.H, rb.W, rb.focal, rb.near, rb.far = self.H, self.W, self.focal, self.near, self.far
        rb.use_ndc, rb.ndc_near_plane = int(self.use_ndc), self.ndc_near_plane
        specs, keys = [("randint", (B,), self.n_pixels, bool(return_ids))], []
        if step_draws is not None:
            S, N, perturb, noise_std = step_draws
            keys, more = D.step_specs(B, int(S), int(N), float(perturb), float(noise_std))
            specs += more
        outs = D.draws(specs, dev, generator, batch=rb, pack=pack_models)
        batch = {"rays": rays, "rgbs": rgbs}
        if pack_models is not None:
            batch["packed"] = pack_ticket(*pack_models)
        if return_ids:
            batch["ids"] = outs[0]
        if step_draws is not None:
            batch["draws"] = {k: t for k, t in zip(keys, outs[1:]) if t is not None}
        return batch

    def image_rays(self, i):
        hw = self.H * self.W
        return gen_rays(self.poses, self.H, self.W, self.focal, self.near, self.far, first_pixel=i * hw, n=hw,
                        use_ndc=self.use_ndc, ndc_near_plane=self.ndc_near_plane)

    def epoch_sampler(self, batch_size, seed=None, rank=0, world=1, last="partial"):
        """The reference's DataLoader(shuffle=True) over this store: see EpochSampler."""
        return EpochSampler(self, batch_size, seed=seed, rank=rank, world=world, last=last)


def _epoch_plan(n, batch_size, world, last):
    """(positions of one rank per epoch, batches per epoch, rows of the last batch) — host arithmetic only."""
    n, B, world = int(n), int(batch_size), int(world)
    if n < 1 or B < 1 or world < 1:
        raise ValueError("epoch sampling needs n >= 1, batch_size >= 1, world >= 1")
    if last not in ("partial", "drop"):
        raise ValueError("last must be 'partial' (the DataLoader's drop_last=False) or 'drop'")
    share = (n + world - 1) // world
    if last == "drop":
        if B > share:
            raise ValueError("last='drop' with batch_size %d above the rank's %d rays leaves no batch" % (B, share))
        return share, share // B, B
    steps = (share + B - 1) // B
    return share, steps, share - (steps - 1) * B


class EpochSampler:
    """Epoch sampling as the reference's `DataLoader(train_dataset, shuffle=True, batch_size=B)` does it (train.py:89-94): every
    ray of the store once per epoch in a fresh shuffled order, the last batch partial (`last="partial"`) or skipped (`"drop"`:
    a tail of fewer than B rays, a different one every epoch).  With `world` > 1 the ranks split an epoch as torch's
    DistributedSampler does: rank r serves ceil(n / world) positions, r, r + world, ... wrapping past n.

    The shuffle is a keyed permutation evaluated per ray (csrc/epoch_core.h) from (seed, epoch): no index tensor, no host work per
    step, and no draw from any torch generator — the step's Philox stream keeps only the render draws, as in the reference, whose
    RandomSampler shuffles with a private CPU generator.  `seed=None` takes torch.initial_seed() (a read).  One launch
    (nerfhip_epoch_batch) makes a batch; epoch and cursor live in device memory (`state`) and the launch advances them, so a
    captured `sample` walks through the epochs on replay.

    Host mirror: `epoch`, `cursor`, `steps_per_epoch`, `epoch_done` (true after the call that served an epoch's last batch) are
    counted on the host — one per eager `sample()`, one per `replayed()` for a captured one — and never read the device."""

    def __init__(self, store, batch_size, seed=None, rank=0, world=1, last="partial"):
        self.store = store
        self.batch_size, self.rank, self.world, self.last = int(batch_size), int(rank), int(world), last
        if not 0 <= self.rank < self.world:
            raise ValueError("rank must lie in [0, world)")
        self.n_rank, self.steps_per_epoch, self.tail_rows = _epoch_plan(store.n_pixels, batch_size, world, last)
        self.seed = (int(torch.initial_seed()) if seed is None else int(seed)) & ((1 << 64) - 1)
        self.epoch, self.cursor, self.epoch_done = 0, 0, False
        self.state = None              # device {seed, epoch, cursor, arrival ticket}: made at the first launch
        self._uploaded = False

    def __len__(self):
        return self.steps_per_epoch

    # ---- host mirror ----
    def _advance(self, times=1):
        for _ in range(int(times)):
            self.cursor += 1
            self.epoch_done = self.cursor >= self.steps_per_epoch
            if self.epoch_done:
                self.cursor = 0
                self.epoch += 1

    def replayed(self, times=1):
        """Tell the mirror that a captured `sample()` launch was replayed `times` times (GraphedTrainStep calls this itself)."""
        self._advance(times)

    def source(self, step_draws=None, pack_models=None):
        """`sample` with its arguments bound, as a `batch_source` for GraphedTrainStep (which tells it of every replay)."""
        def next_batch():
            return self.sample(step_draws=step_draws, pack_models=pack_models)
        next_batch.replayed = self.replayed
        return next_batch

    def rows(self, cursor=None):
        """Rows of batch `cursor` (default: the next one)."""
        c = self.cursor if cursor is None else int(cursor)
        return self.tail_rows if c == self.steps_per_epoch - 1 else self.batch_size

    def state_dict(self):
        return {"seed": self.seed, "epoch": self.epoch, "cursor": self.cursor, "rank": self.rank, "world": self.world,
                "batch_size": self.batch_size, "last": self.last}

    def load_state_dict(self, sd):
        """Continue inside the epoch the saved run was in.  The layout (rank, world, batch_size, last) must be the saved one: a
        cursor means nothing under another."""
        for k in ("rank", "world", "batch_size", "last"):
            if sd[k] != getattr(self, k):
                raise ValueError("EpochSampler.load_state_dict: saved %s=%r, this sampler has %r" % (k, sd[k], getattr(self, k)))
        if not 0 <= int(sd["cursor"]) < self.steps_per_epoch or int(sd["epoch"]) < 0:
            raise ValueError("EpochSampler.load_state_dict: cursor / epoch out of range")
        self.seed, self.epoch, self.cursor = int(sd["seed"]) & ((1 << 64) - 1), int(sd["epoch"]), int(sd["cursor"])
        self.epoch_done = False
        self._uploaded = False

    def _upload(self):
        dev = self.store.poses.device
        if torch.cuda.is_current_stream_capturing():
            raise _lib.NerfHipError("EpochSampler: the device state must be loaded before a capture starts — call sample() or "
                                    "prepare() once outside it")
        if self.state is None:
            self.state = torch.zeros(4, device=dev, dtype=torch.int64)
        wrap = lambda v: v - (1 << 64) if v >= (1 << 63) else v          # uint64 bit patterns in an int64 tensor
        self.state.copy_(torch.tensor([wrap(self.seed), wrap(self.epoch), self.cursor, 0], dtype=torch.int64))
        self._uploaded = True

    def prepare(self):
        """Load the device state from the mirror if it is not there yet (not during a capture).  sample() does it itself."""
        if not self._uploaded:
            self._upload()
        return self

    def sample(self, step_draws=None, pack_models=None, return_ids=False):
        """The next batch of the epoch in ONE launch: the batch dict of RayStore.sample ({'rays', 'rgbs'}, 'ids' on request).  The
        epoch's last batch has `rows()` < batch_size rows under last="partial".
        step_draws / pack_models as in RayStore.sample, made by one more launch (draws.draws on the step's specs without the
        leading randint): batch['draws'] and batch['packed'] are what NeRFSystem.training_step consumes."""
        st = self.store
        dev = st.poses.device
        B = self.batch_size
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and self.last == "partial" and self.n_rank % B != 0:
            raise _lib.NerfHipError("EpochSampler: a captured graph has one batch shape, but last='partial' ends every epoch with a "
                                    "batch of %d rows instead of %d; use last='drop' or a batch size dividing %d"
                                    % (self.tail_rows, B, self.n_rank))
        with torch.cuda.device(dev):
            self.prepare()
            rows = B if capturing else self.rows()
            rays = torch.empty(B, 8, device=dev, dtype=torch.float32)
            rgbs = torch.empty(B, 3, device=dev, dtype=torch.float32)
            ids = torch.empty(B, device=dev, dtype=torch.int64) if return_ids else None
            rb = _lib.RayBatch()
            rb.c2w, rb.rgbs_all, rb.rays, rb.rgbs = st.poses.data_ptr(), st.rgbs.data_ptr(), rays.data_ptr(), rgbs.data_ptr()
            rb.H, rb.W, rb.focal, rb.near, rb.far = st.H, st.W, st.focal, st.near, st.far
            rb.use_ndc, rb.ndc_near_plane = int(st.use_ndc), st.ndc_near_plane
            check(_lib.load().nerfhip_epoch_batch(ctypes.addressof(rb), st.n_pixels, B, self.rank, self.world,
                                                  int(self.last == "drop"), ptr(self.state), ptr(ids), stream_ptr()),
                  "nerfhip_epoch_batch")
        if not capturing:                  # a captured launch runs when it is replayed: replayed() counts those
            self._advance()
        batch = {"rays": rays[:rows], "rgbs": rgbs[:rows]}
        if return_ids:
            batch["ids"] = ids[:rows]
        if step_draws is not None:
            from . import draws as D
            S, N, perturb, noise_std = step_draws
            keys, specs = D.step_specs(rows, int(S), int(N), float(perturb), float(noise_std))
            outs = D.draws(specs, dev, None, batch=None, pack=pack_models)
            batch["draws"] = {k: t for k, t in zip(keys, outs) if t is not None}
        elif pack_models is not None:
            from . import ops
            ops.pack_models_train(*pack_models)
        if pack_models is not None:
            batch["packed"] = pack_ticket(*pack_models)
        return batch

"""GPU: nerfhip_ssim, nerfhip_depth_colormap, image_to_u8, evaluate and NeRFSystem.validation_panel.

SSIM gate (per pixel): with d_ref = max |fp32 restatement - fp64 restatement| on the same input (tests/image_metrics_ref.py,
computed here on the CPU), the kernel's map lies within 2 * d_ref + 1e-6 of the fp64 map (the factor 2: the summation order
differs); the mean within 2 * mean |fp32 map - fp64 map| + 2^-22 of the fp64 mean.  Each case prints the distances it measured.

Measured on an MI355X (the table is in DESIGN.md section 12): the kernel's map is 2.9e-8 ... 2.5e-6 from the fp64 map over every
case; on the flat and near-white images 3.3e-7 ... 7.0e-7 where d_ref is 2.3e-4 ... 1.57e-3 (ratio 0.0003 ... 0.002: the centred
second moments do not cancel), on random images 0.07 ... 0.23 of d_ref, on images of 1 to 9 pixels 0.33 ... 1.89 of d_ref
(d_ref 7.6e-8 ... 5.9e-7 there, so the 1e-6 of the gate carries them).  The ratios are recorded, not asserted."""
import os

import numpy as np
import pytest
import torch

from tests import image_metrics_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1, 1), (1, 2, 5), (1, 3, 3), (2, 17, 67), (1, 64, 200)]          # (B, H, W); C = 3
KINDS = ("random", "noisy_copy", "flat", "near_white")
_CASES = {}


def _images(kind, B, H, W):
    g = torch.Generator().manual_seed(1000 * H + W)
    shape = (B, 3, H, W)
    if kind == "random":
        return torch.rand(shape, generator=g), torch.rand(shape, generator=g)
    if kind == "noisy_copy":
        gt = torch.rand(shape, generator=g)
        return (gt + 0.02 * torch.randn(shape, generator=g)).clamp(0, 1), gt
    if kind == "flat":
        return 0.7 + 1e-3 * torch.randn(shape, generator=g), 0.7 + 1e-3 * torch.randn(shape, generator=g)
    return 0.999 + 1e-3 * torch.rand(shape, generator=g), 0.999 + 1e-3 * torch.rand(shape, generator=g)


def _case(kind, size, ws):
    """inputs and both restatements of one case, computed once and shared (never modified)"""
    key = (kind, size, ws)
    if key not in _CASES:
        a, b = _images(kind, *size)
        m64 = R.ssim_map(a, b, ws, torch.float64)
        m32 = R.ssim_map(a, b, ws, torch.float32).double()
        _CASES[key] = (a, b, m64, m32)
    return _CASES[key]


def _run(dev, a, b, ws, interleaved):
    """-> (map as (B,C,H,W) on the host, mean as a python float of the fp32 scalar)"""
    from nerf_pl_amd import ops
    B, C, H, W = a.shape
    if interleaved:
        x, y = a.permute(0, 2, 3, 1).contiguous().to(dev), b.permute(0, 2, 3, 1).contiguous().to(dev)
        m, mean = ops.ssim(x, y, B, C, H, W, ws, ops.IMAGE_INTERLEAVED, want_map=True, want_mean=True)
        return m.cpu().permute(0, 3, 1, 2).contiguous(), mean.cpu()
    m, mean = ops.ssim(a.to(dev), b.to(dev), B, C, H, W, ws, ops.IMAGE_PLANAR, want_map=True, want_mean=True)
    return m.cpu(), mean.cpu()


@pytest.mark.parametrize("ws", [3, 11])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_ssim_matches_float64_restatement(dev, size, ws):
    failures = []
    for kind in KINDS:
        a, b, m64, m32 = _case(kind, size, ws)
        d_ref = float((m32 - m64).abs().max())
        mean_ref = float((m32 - m64).abs().mean())
        planar = None
        for interleaved in (False, True):
            m, mean = _run(dev, a, b, ws, interleaved)
            assert m.shape == m64.shape and m.dtype == torch.float32 and bool(torch.isfinite(m).all())
            if planar is None:
                planar = (m, mean)
            else:       # the interleaved layout gives the planar layout's bits
                assert torch.equal(m, planar[0]) and torch.equal(mean, planar[1])
            d = float((m.double() - m64).abs().max())
            d_mean = abs(float(mean) - float(m64.mean()))
            d_map_mean = abs(float(m.double().mean()) - float(mean))
            print("ssim %-10s %dx%dx%d ws=%-2d %s: map %.3e (d_ref %.3e, ratio %.3f)  mean %.3e (ref %.3e)  mean-vs-map %.1e"
                  % (kind, size[0], size[1], size[2], ws, "hwc" if interleaved else "chw", d, d_ref, d / d_ref if d_ref else 0.0,
                     d_mean, mean_ref, d_map_mean))
            if not d <= 2 * d_ref + 1e-6:
                failures.append(("map", kind, interleaved, d, d_ref))
            if not d_mean <= 2 * mean_ref + 2.0 ** -22:
                failures.append(("mean", kind, interleaved, d_mean, mean_ref))
            if not d_map_mean <= 1e-6:
                failures.append(("mean-vs-map", kind, interleaved, d_map_mean))
    assert not failures, failures


@pytest.mark.parametrize("ws", [3, 11])
def test_ssim_identical_images_give_exactly_one(dev, ws):
    from nerf_pl_amd import metrics
    for size in SIZES:
        for kind in ("random", "near_white"):
            a = _case(kind, size, ws)[0].to(dev)
            m = metrics.ssim(a, a.clone(), reduction='none', window_size=ws)
            assert m.shape == a.shape and bool((m == 1.0).all()), (size, kind)
            assert float(metrics.ssim(a, a.clone(), window_size=ws)) == 1.0, (size, kind)


def test_ssim_is_deterministic_and_layouts_agree_through_the_python_surface(dev):
    from nerf_pl_amd import metrics
    a, b = (t.to(dev) for t in _case("noisy_copy", (2, 17, 67), 11)[:2])
    first = (metrics.ssim(a, b, window_size=11), metrics.ssim(a, b, reduction='none', window_size=11))
    for _ in range(2):
        assert torch.equal(metrics.ssim(a, b, window_size=11), first[0])
        assert torch.equal(metrics.ssim(a, b, reduction='none', window_size=11), first[1])
    assert first[0].shape == () and first[0].device == a.device
    # the renderer's (H*W, 3) layout, one image: the planar bits
    a1, b1 = a[:1], b[:1]
    hw3 = lambda t: t[0].permute(1, 2, 0).reshape(17 * 67, 3).contiguous()      # noqa: E731
    for ws in (3, 11):
        m = metrics.ssim_hw3(hw3(a1), hw3(b1), 17, 67, reduction='none', window_size=ws)
        assert m.shape == (17, 67, 3)
        assert torch.equal(m.permute(2, 0, 1), metrics.ssim(a1, b1, reduction='none', window_size=ws)[0])
        assert torch.equal(metrics.ssim_hw3(hw3(a1), hw3(b1), 17, 67, window_size=ws), metrics.ssim(a1, b1, window_size=ws))
    assert float(metrics.ssim(a1, b1)) == float(metrics.ssim(a1, b1, window_size=3))          # the reference's default window


def test_ssim_refuses_bad_arguments(dev):
    from nerf_pl_amd import metrics
    from nerf_pl_amd._lib import NerfHipError
    a = torch.rand(1, 3, 8, 8, device=dev)
    for ws in (2, 4, 13, 1):
        with pytest.raises(NerfHipError):
            metrics.ssim(a, a, window_size=ws)
    with pytest.raises(ValueError):
        metrics.ssim(a, a[:, :, :4])
    with pytest.raises(ValueError):
        metrics.ssim(a, a, reduction='sum')
    empty = torch.rand(0, 3, 8, 8, device=dev)
    assert metrics.ssim(empty, empty, reduction='none').shape == (0, 3, 8, 8)


def test_ssim_captures_in_a_graph(dev):
    from nerf_pl_amd import ops
    a, b = (t.to(dev) for t in _case("noisy_copy", (1, 64, 200), 11)[:2])
    B, C, H, W = a.shape
    want_map, want_mean = ops.ssim(a, b, B, C, H, W, 11, want_map=True, want_mean=True)
    sa, sb = torch.zeros_like(a), torch.zeros_like(b)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.ssim(sa, sb, B, C, H, W, 11, want_map=True, want_mean=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got_map, got_mean = ops.ssim(sa, sb, B, C, H, W, 11, want_map=True, want_mean=True)
    sa.copy_(a)
    sb.copy_(b)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got_map, want_map) and torch.equal(got_mean, want_mean)


# ----------------------------------------------------------------------------------------------------------------- depth
def _depth_inputs(shape, seed):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    base = (rng.standard_normal(n) * 3.0).astype(np.float32)            # negatives included
    out = {"plain": base.copy(), "constant": np.full(n, 2.5, np.float32)}
    for name, specials in (("nan_posinf", (np.nan, np.inf)), ("neginf", (-np.inf,)), ("all", (np.nan, np.inf, -np.inf))):
        x = base.copy()
        for k, s in enumerate(specials):
            x[(k * 7 + 1) % n::11] = s
        out[name] = x
    return {k: v.reshape(shape) for k, v in out.items()}


@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 64), (1, 65), (1, 1025), (100, 37)], ids=lambda s: "%dx%d" % s)
def test_depth_colormap_matches_numpy(dev, shape):
    from nerf_pl_amd import ops, visualization
    from nerf_pl_amd.imageio_min import jet_table
    jet = jet_table()
    rand_table = np.random.default_rng(5).integers(0, 256, (256, 3)).astype(np.uint8)
    for name, x in _depth_inputs(shape, shape[0] * 4099 + shape[1]).items():
        d = torch.from_numpy(x).to(dev)
        idx = R.depth_index(x)
        if name == "constant":
            assert not idx.any()
        # the indices, byte for byte (cmap=None: the index on all three channels)
        grey_f, grey_b = ops.depth_colormap(d, visualization._table("index", dev), want_float=True, want_bytes=True)
        assert grey_b.shape == shape + (3,) and grey_b.dtype == torch.uint8
        assert np.array_equal(grey_b.cpu().numpy(), np.repeat(idx[..., None], 3, -1)), name
        assert np.array_equal(visualization.visualize_depth(d, cmap=None).cpu().numpy(), grey_f.cpu().numpy())
        # the colours: the table lookup exactly, the float image byte / 255 exactly; the caller's table is honoured
        for table in (jet, rand_table):
            want_f, want_b = R.depth_colors(x, table)
            got = visualization.visualize_depth(d, cmap=torch.from_numpy(table).to(dev))
            assert got.shape == (3,) + shape and got.dtype == torch.float32 and got.device == d.device
            assert np.array_equal(got.cpu().numpy(), want_f), name
            f, b = ops.depth_colormap(d, torch.from_numpy(table).to(dev), want_float=False, want_bytes=True)
            assert f is None and np.array_equal(b.cpu().numpy(), want_b), name
        assert np.array_equal(visualization.visualize_depth(d).cpu().numpy(), R.depth_colors(x, jet)[0]), name     # cmap=2
        assert np.array_equal(visualization.visualize_depth(d, cmap=2).cpu().numpy(), R.depth_colors(x, jet)[0]), name


def test_depth_channel_order_is_the_references(dev):
    """The reference hands cv2's BGR image to PIL as RGB: channel 0 is the map's blue.  The nearest depth (index 0) is JET's
    dark blue, the farthest (index 255) its dark red."""
    from nerf_pl_amd import visualization
    d = torch.linspace(2.0, 6.0, 256, device=dev).reshape(1, 256)
    img = visualization.visualize_depth(d)
    near, far = img[:, 0, 0].cpu().tolist(), img[:, 0, 255].cpu().tolist()
    assert near[0] == np.float32(131) / np.float32(255) and near[1] == 0.0 and near[2] == 0.0
    assert far[0] == 0.0 and far[1] == 0.0 and far[2] == np.float32(128) / np.float32(255)
    with pytest.raises(ValueError):
        visualization.visualize_depth(d, cmap=4)
    with pytest.raises(ValueError):
        visualization.visualize_depth(d.reshape(-1))


def test_image_to_u8_is_numpy_truncation(dev):
    from nerf_pl_amd import inference
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    x = np.concatenate([k, np.nextafter(k, np.float32(-1)).clip(0, 1), np.nextafter(k, np.float32(2)).clip(0, 1),
                        np.random.default_rng(0).random(4096, dtype=np.float32), np.float32([0.0, 1.0])]).astype(np.float32)
    x = x[: (x.size // 3) * 3].reshape(-1, 3)
    got = inference.image_to_u8(torch.from_numpy(x).to(dev))
    assert got.dtype == torch.uint8 and got.shape == x.shape
    assert np.array_equal(got.cpu().numpy(), (x * 255).astype(np.uint8))


# -------------------------------------------------------------------------------------------------------------- evaluate
class _Scene:
    """4 images of 16 x 12 pixels: seeded rays and (with_rgbs) seeded ground truth"""
    img_wh = (16, 12)
    white_back = True

    def __init__(self, with_rgbs=True):
        from oracle import nerf_oracle as O
        g = torch.Generator().manual_seed(7)
        self.items = []
        for i in range(4):
            item = {"rays": O.make_rays(20 + i, 16 * 12, "blender")}
            if with_rgbs:
                item["rgbs"] = torch.rand(16 * 12, 3, generator=g)
            self.items.append(item)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


@pytest.fixture(scope="module")
def untrained(dev):
    from nerf_pl_amd.models import Embedding, NeRF
    torch.manual_seed(0)
    models = [NeRF().to(dev), NeRF().to(dev)]
    return models, [Embedding(3, 10), Embedding(3, 4)]


def test_evaluate_is_the_eval_loop(dev, untrained, tmp_path):
    from nerf_pl_amd import inference, metrics
    models, embeddings = untrained
    renders = []

    def renderer(rays):
        out = inference.batched_inference(models, embeddings, rays, 16, 16, False, 1024, True)
        renders.append({k: v.clone() for k, v in out.items()})
        return out
    scene = _Scene()
    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    res = inference.evaluate(scene, renderer, dir_name=a_dir, save_depth=True, window_size=3)
    assert len(renders) == 4 and len(res["images"]) == 4
    os.makedirs(b_dir)
    for i, r in enumerate(renders):
        img = inference.save_image_outputs(r, 12, 16, b_dir, i, save_depth=True)
        assert res["images"][i].dtype == np.uint8 and np.array_equal(res["images"][i], img)
        for name in ("%03d.png" % i, "depth_%03d.pfm" % i):
            assert open(os.path.join(a_dir, name), "rb").read() == open(os.path.join(b_dir, name), "rb").read(), name
        gt = scene[i]["rgbs"].to(dev)
        assert res["psnr"][i] == float(metrics.psnr(gt, r["rgb_fine"]))
        assert res["ssim"][i] == float(metrics.ssim_hw3(r["rgb_fine"], gt, 12, 16))
        planar = lambda t: t.reshape(12, 16, 3).permute(2, 0, 1)[None].contiguous()      # noqa: E731
        assert res["ssim"][i] == float(metrics.ssim(planar(r["rgb_fine"]), planar(gt)))
    assert res["mean_psnr"] == float(np.mean(res["psnr"])) and res["mean_ssim"] == float(np.mean(res["ssim"]))
    assert sorted(os.listdir(a_dir)) == sorted(os.listdir(b_dir))
    # the 'bytes' depth format, no directory, a dataset without ground truth
    c_dir = str(tmp_path / "c")
    inference.evaluate(scene, renderer, dir_name=c_dir, save_depth=True, depth_format="bytes")
    assert open(os.path.join(c_dir, "depth_000"), "rb").read() == \
        np.nan_to_num(renders[0]["depth_fine"].cpu().numpy()).astype(np.float32).tobytes()
    bare = inference.evaluate(_Scene(with_rgbs=False), renderer)
    assert bare["psnr"] == [] and bare["ssim"] == [] and bare["mean_psnr"] is None and len(bare["images"]) == 4
    assert np.array_equal(bare["images"][0], res["images"][0])


def test_validation_panel_and_step(dev):
    from types import SimpleNamespace
    from nerf_pl_amd.system import NeRFSystem
    from nerf_pl_amd.visualization import visualize_depth
    H, W = 12, 16
    hp = SimpleNamespace(N_importance=16, N_samples=16, use_disp=False, perturb=0.0, noise_std=0.0, chunk=1024, img_wh=(W, H),
                         white_back=True)
    torch.manual_seed(1)
    system = NeRFSystem(hp).to(dev)
    scene = _Scene()
    batch = {"rays": scene[0]["rays"][None].to(dev), "rgbs": scene[0]["rgbs"][None].to(dev)}
    with torch.no_grad():
        results = system(batch["rays"][0])
        panel = system.validation_panel(results, batch["rgbs"][0], H, W)
        assert panel.shape == (3, 3, H, W) and panel.device == batch["rays"].device and panel.dtype == torch.float32
        assert torch.equal(panel[0], batch["rgbs"][0].view(H, W, 3).permute(2, 0, 1))
        assert torch.equal(panel[1], results["rgb_fine"].view(H, W, 3).permute(2, 0, 1))
        assert torch.equal(panel[2], visualize_depth(results["depth_fine"].view(H, W)))
        # validation_step: the same dict with or without a logger; the panel goes to the logger for the first batch only
        plain = system.validation_step(batch, 0)
        logged = []
        system.logger = SimpleNamespace(experiment=SimpleNamespace(add_images=lambda tag, img, step: logged.append((tag, img, step))))
        with_logger = system.validation_step(batch, 0)
        system.validation_step(batch, 1)
    assert len(logged) == 1 and logged[0][0] == 'val/GT_pred_depth' and torch.equal(logged[0][1], panel)
    assert sorted(plain) == sorted(with_logger) == ['val_loss', 'val_psnr']
    assert torch.equal(plain['val_psnr'], with_logger['val_psnr']) and torch.equal(plain['val_loss'], with_logger['val_loss'])

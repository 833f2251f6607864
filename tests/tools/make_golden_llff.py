"""Mint tests/golden/jpeg_mini/, jpeg_mini_expected.npz, llff_mini/, llff_mini_png/ and llff_mini_expected.npz (CPU, needs PIL
built against libjpeg-turbo and the reference tree, see oracle/ref_shim.py; no GPU, no torchvision, no kornia).

    python tests/tools/make_golden_llff.py

jpeg_mini: small JPEG files written by PIL that together cover what the decoder takes — 4:4:4, 4:2:2 and 4:2:0, sizes that are
no multiple of the MCU, single-MCU images, chroma planes of at most 2 samples (plain replication instead of the triangle
filter) and of exactly 3, optimised Huffman tables, restart markers, qualities 30 / 90 / 100, a greyscale file — plus one
progressive file that exists to be refused.  The tool asserts from the written bytes that each property is really there.
jpeg_mini_expected.npz holds PIL's `Image.open(p).convert('RGB')` of every decodable file.

llff_mini: an LLFF-style scene of five 64 x 48 JPEGs and a poses_bounds.npy (off-centre, tilted poses; distinct distances from
the centre); llff_mini_png: the same scene with the second image stored as an RGBA PNG.  llff_mini_expected.npz holds what the
reference's own LLFFDataset (datasets/llff.py, run here on the CPU with stand-ins for torchvision's ToTensor and kornia's
create_meshgrid, as oracle/ref_shim.py does for the rays) makes of them, forward-facing ("fwd") and spheric_poses=True ("sph"),
at img_wh (64, 48), (32, 24) and (80, 60):
    poses, pose_avg, bounds, val_idx           the centred, rescaled poses (float64) and the val image's index
    <mode>_focal_<w>                           focal length at width w
    <mode>_poses_test, <mode>_poses_test_train the rendering paths of the `test` and `test_train` splits
    rgbs_<w>, png_rgbs_<w>                     (4 h w, 3) uint8: all_rgbs * 255 of the train split (both modes agree)
    val_rgbs_<w>                               (h w, 3) uint8: the val item's colours * 255
    <mode>_rays_<w>, <mode>_val_rays_<w>       float32 rays of the train split / the val item: every ray at w = 32, every
                                               RAY_STRIDE-th at 64 and 80 (the committed file stays under the size limit)
    <mode>_test_rays_32                        the `test` split's item 3 at w = 32
Everything is seeded and the archives carry fixed timestamps, so a second run gives the same bytes."""
import importlib
import io
import os
import shutil
import sys
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_blender import write_npz  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
JPEGS = os.path.join(GOLDEN, "jpeg_mini")
SCENE = os.path.join(GOLDEN, "llff_mini")
SCENE_PNG = os.path.join(GOLDEN, "llff_mini_png")
SIZES = ((64, 48), (32, 24), (80, 60))
PNG_INDEX = 1                           # the image llff_mini_png stores as a PNG (a training image, not the val one)
RAY_STRIDE = 7                          # coprime with every width, so the kept rays visit every column

# name: (W, H, mode, save options, expected luma sampling)
CASES = (
    ("q90_444_61x45", 61, 45, "RGB", dict(quality=90, subsampling=0), (1, 1)),
    ("q90_422_61x45", 61, 45, "RGB", dict(quality=90, subsampling=1), (2, 1)),
    ("q90_420_61x45", 61, 45, "RGB", dict(quality=90, subsampling=2), (2, 2)),
    ("q75_420_61x45_optimized", 61, 45, "RGB", dict(quality=75, subsampling=2, optimize=True), (2, 2)),
    ("q85_420_61x45_restart3", 61, 45, "RGB", dict(quality=85, subsampling=2, restart_marker_blocks=3), (2, 2)),
    ("q30_420_64x48", 64, 48, "RGB", dict(quality=30, subsampling=2), (2, 2)),
    ("q50_420_64x48_restart1", 64, 48, "RGB", dict(quality=50, subsampling=2, restart_marker_blocks=1), (2, 2)),   # RST7 -> RST0
    ("q30_422_40x24_restart3", 40, 24, "RGB", dict(quality=30, subsampling=1, restart_marker_blocks=3), (2, 1)),
    ("q100_444_17x9", 17, 9, "RGB", dict(quality=100, subsampling=0), (1, 1)),
    ("q100_420_17x9", 17, 9, "RGB", dict(quality=100, subsampling=2), (2, 2)),
    ("q90_420_8x8", 8, 8, "RGB", dict(quality=90, subsampling=2), (2, 2)),
    ("q90_420_3x5", 3, 5, "RGB", dict(quality=90, subsampling=2), (2, 2)),           # chroma 2 wide: replicated
    ("q90_422_4x7", 4, 7, "RGB", dict(quality=90, subsampling=1), (2, 1)),           # chroma 2 wide: replicated
    ("q90_420_6x6", 6, 6, "RGB", dict(quality=90, subsampling=2), (2, 2)),           # chroma 3 wide: the narrowest filtered
    ("q90_422_5x4", 5, 4, "RGB", dict(quality=90, subsampling=1), (2, 1)),
    ("q90_grey_37x29", 37, 29, "L", dict(quality=90), (1, 1)),
    ("q90_420_32x32_progressive", 32, 32, "RGB", dict(quality=90, subsampling=2, progressive=True), (2, 2)),
)


def make_image(W, H, seed):
    """Smooth ramps, a saturated flat band, noisy patches: smooth areas exercise the DC path and the filters' rounding, noise the
    long Huffman codes and the range limit."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.zeros((H, W, 3), np.int64)
    img[..., 0] = (x * 255) // max(W - 1, 1)
    img[..., 1] = (y * 255) // max(H - 1, 1)
    img[..., 2] = ((x + y) * 5 + (x * y) // 3 + 40 * seed) % 256
    img[H // 3:H // 3 + max(H // 6, 1), :, :] = (255, 0, 255 if seed % 2 else 0)
    img[: max(H // 4, 1), W // 2:] = rng.integers(0, 256, (max(H // 4, 1), W - W // 2, 3))
    img[H - max(H // 5, 1):, : max(W // 3, 1)] = rng.integers(0, 2, (max(H // 5, 1), max(W // 3, 1), 1)) * 255
    return img.astype(np.uint8)


def markers(data):
    """[(marker, payload offset)] of a JPEG file's segments up to the scan, then the RSTm / EOI markers inside and behind it"""
    out, pos = [], 2
    while True:
        assert data[pos] == 0xff
        m = data[pos + 1]
        out.append((m, pos + 4))
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xda:
            break
    while pos + 1 < len(data):
        if data[pos] == 0xff and data[pos + 1] not in (0x00, 0xff):
            out.append((data[pos + 1], pos + 2))
            pos += 2
        else:
            pos += 1
    return out


def mint_jpegs():
    from nerf_pl_amd.imageio_min import jpeg_parse
    if os.path.isdir(JPEGS):
        shutil.rmtree(JPEGS)
    os.makedirs(JPEGS)
    arrays, names, seen = {}, [], {"sampling": set(), "rst": 0, "optimized": 0, "progressive": 0, "grey": 0}
    for k, (name, W, H, mode, opts, sampling) in enumerate(CASES):
        img = make_image(W, H, k)
        pil = Image.fromarray(img, "RGB")
        if mode == "L":
            pil = pil.convert("L")
        path = os.path.join(JPEGS, name + ".jpg")
        pil.save(path, "JPEG", **opts)
        data = open(path, "rb").read()
        ms = markers(data)
        kinds = [m for m, _ in ms]
        sof = [m for m in kinds if 0xc0 <= m <= 0xcf and m not in (0xc4, 0xc8, 0xcc)]
        n_rst = sum(1 for m in kinds if 0xd0 <= m <= 0xd7)
        at = dict(ms)[sof[0]]
        ncomp = data[at + 5]
        assert ncomp == (1 if mode == "L" else 3)
        got = (data[at + 7] >> 4, data[at + 7] & 15)
        assert got == sampling or mode == "L", (name, got)
        if mode != "L":
            assert (data[at + 10], data[at + 13]) == (0x11, 0x11), name
        if opts.get("progressive"):
            assert sof == [0xc2], name
            seen["progressive"] += 1
        else:
            assert sof == [0xc0], name
            mx, my = -(-W // (8 * sampling[0])), -(-H // (8 * sampling[1]))
            if "restart_marker_blocks" in opts:
                assert n_rst == -(-mx * my // opts["restart_marker_blocks"]) - 1 and n_rst >= 2, (name, n_rst)
                seen["rst"] += n_rst
            else:
                assert n_rst == 0, name
            parsed = jpeg_parse(path)
            assert (parsed["width"], parsed["height"]) == (W, H)
            n_symbols = sum(len(s) for _, s in parsed["huffman"].values())
            if opts.get("optimize"):
                assert n_symbols < 2 * (12 + 162), name       # not the standard tables
                seen["optimized"] += 1
            with Image.open(path) as im:
                assert im.mode == mode
                arrays["rgb_%d" % k] = np.asarray(im.convert("RGB")).copy()
            seen["sampling"].add(sampling if mode != "L" else "grey")
            seen["grey"] += mode == "L"
        names.append(name)
    assert seen["sampling"] == {(1, 1), (2, 1), (2, 2), "grey"} and seen["rst"] and seen["optimized"] and seen["progressive"] == 1
    arrays["names"] = np.array(names)
    write_npz(os.path.join(GOLDEN, "jpeg_mini_expected.npz"), arrays)
    return seen


# ---- the LLFF scene ---------------------------------------------------------------------------------------------------------
def poses_bounds():
    """(5, 17) float64 as LLFF's imgs2poses.py writes it: per image a (3, 5) block [down right back position | H W focal] and the
    near / far depth bounds"""
    rows = []
    for k in range(5):
        center = np.array([0.6 + 0.45 * k - 0.07 * k * k, -0.3 + 0.21 * k, 0.25 - 0.13 * k + 0.05 * k * k])
        back = np.array([0.12 * (k - 2) + 0.05, 0.31 - 0.06 * k, 1.0])        # tilted: not along any axis
        back /= np.linalg.norm(back)
        right = np.cross([0.1, 1.0, 0.05 * k], back)
        right /= np.linalg.norm(right)
        up = np.cross(back, right)
        block = np.stack([-up, right, back, center, [48.0, 64.0, 57.5]], 1)    # (3, 5)
        rows.append(np.concatenate([block.reshape(-1), [2.4 + 0.35 * k, 11.0 + 4.5 * ((3 * k) % 5)]]))
    return np.stack(rows)


def reference_llff():
    """The reference's datasets/llff.py, unmodified, imported under a private package name with stand-ins for its two missing
    imports."""
    from oracle import ref_shim
    ref_shim.load_reference_ray_utils()                  # installs the kornia.create_meshgrid stand-in
    if "torchvision" not in sys.modules:
        tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")

        class ToTensor:
            def __call__(self, pic):                     # uint8 HWC -> float CHW / 255
                return torch.from_numpy(np.asarray(pic).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

        tr.ToTensor = ToTensor
        tv.transforms = tr
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tr
    pkg = types.ModuleType("_ref_datasets")
    pkg.__path__ = [os.path.join(ref_shim.REFERENCE_ROOT, "datasets")]
    sys.modules["_ref_datasets"] = pkg
    return importlib.import_module("_ref_datasets.llff")


def to_u8(rgbs):
    a = rgbs.numpy().astype(np.float64) * 255
    u = np.rint(a).astype(np.uint8)
    assert np.array_equal(torch.from_numpy(u).to(torch.float32).div(255).numpy(), rgbs.numpy())      # exact bytes / 255
    return u


def mint_scene():
    for d in (SCENE, SCENE_PNG):
        if os.path.isdir(d):
            shutil.rmtree(d)
        os.makedirs(os.path.join(d, "images"))
    pb = poses_bounds()
    for k in range(5):
        img = make_image(64, 48, 50 + k)
        opts = dict(quality=(92, 80, 95, 88, 70)[k], subsampling=(2, 2, 0, 1, 2)[k])
        Image.fromarray(img, "RGB").save(os.path.join(SCENE, "images", "image%03d.jpg" % k), "JPEG", **opts)
        if k == PNG_INDEX:                               # an RGBA PNG, its alpha ignored by convert('RGB')
            rgba = np.dstack([img, make_image(64, 48, 60)[..., 2]])
            Image.fromarray(rgba, "RGBA").save(os.path.join(SCENE_PNG, "images", "image%03d.png" % k))
        else:
            shutil.copyfile(os.path.join(SCENE, "images", "image%03d.jpg" % k), os.path.join(SCENE_PNG, "images", "image%03d.jpg" % k))
    for d in (SCENE, SCENE_PNG):
        with open(os.path.join(d, "poses_bounds.npy"), "wb") as f:
            np.lib.format.write_array(f, pb, allow_pickle=False)
    ref = reference_llff()
    arrays = {}
    for spheric, mode in ((False, "fwd"), (True, "sph")):
        for (w, h) in SIZES:
            keep = slice(None) if w == 32 else slice(None, None, RAY_STRIDE)
            tr = ref.LLFFDataset(SCENE, "train", (w, h), spheric_poses=spheric)
            va = ref.LLFFDataset(SCENE, "val", (w, h), spheric_poses=spheric)
            val_idx = [os.path.basename(p) for p in tr.image_paths].index(os.path.basename(va.image_path_val))
            if "poses" not in arrays:
                arrays.update(poses=tr.poses, pose_avg=tr.pose_avg, bounds=tr.bounds, val_idx=np.array(val_idx))
                dist = np.linalg.norm(tr.poses[..., 3], axis=1)
                assert np.min(np.diff(np.sort(dist))) > 1e-2, "distances from the centre must be distinct"
                assert 0 < val_idx < 4, "the val image should sit inside the list, so that the exclusion is observable"
                assert val_idx != PNG_INDEX
            assert np.array_equal(arrays["poses"], tr.poses) and arrays["val_idx"] == val_idx
            assert np.array_equal(va.c2w_val, tr.poses[val_idx])
            arrays["%s_focal_%d" % (mode, w)] = np.array(tr.focal)
            rgbs = to_u8(tr.all_rgbs)
            assert np.array_equal(arrays.setdefault("rgbs_%d" % w, rgbs), rgbs)
            arrays["%s_rays_%d" % (mode, w)] = tr.all_rays.numpy()[keep]
            item = va[0]
            assert sorted(item) == ["c2w", "rays", "rgbs"] and len(va) == 1
            arrays["%s_val_rays_%d" % (mode, w)] = item["rays"].numpy()[keep]
            vr = to_u8(item["rgbs"])
            assert np.array_equal(arrays.setdefault("val_rgbs_%d" % w, vr), vr)
            if not spheric:
                arrays["png_rgbs_%d" % w] = to_u8(ref.LLFFDataset(SCENE_PNG, "train", (w, h)).all_rgbs)
        te = ref.LLFFDataset(SCENE, "test", (32, 24), spheric_poses=spheric)
        arrays["%s_poses_test" % mode] = te.poses_test
        arrays["%s_test_rays_32" % mode] = te[3]["rays"].numpy()
        assert len(te) == 120
        arrays["%s_poses_test_train" % mode] = ref.LLFFDataset(SCENE, "test_train", (32, 24), spheric_poses=spheric).poses_test
    assert not np.array_equal(arrays["png_rgbs_64"], arrays["rgbs_64"])          # the PNG holds the unquantised image
    write_npz(os.path.join(GOLDEN, "llff_mini_expected.npz"), arrays)


def main():
    seen = mint_jpegs()
    mint_scene()
    total = 0
    for d in (JPEGS, SCENE, SCENE_PNG):
        for dp, _, fs in os.walk(d):
            total += sum(os.path.getsize(os.path.join(dp, f)) for f in fs)
    sizes = {f: os.path.getsize(os.path.join(GOLDEN, f)) for f in ("jpeg_mini_expected.npz", "llff_mini_expected.npz")}
    print("jpeg_mini: %d files, %d restart markers, samplings %s" % (len(CASES), seen["rst"], sorted(map(str, seen["sampling"]))))
    print("fixtures: %d bytes of images and poses; archives %s" % (total, sizes))
    assert max(sizes.values()) < (1 << 20)


if __name__ == "__main__":
    main()

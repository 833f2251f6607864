"""Mint tests/golden/blender_mini/ and tests/golden/blender_mini_expected.npz (CPU, needs PIL; no GPU, no torchvision).

    python tests/tools/make_golden_blender.py

A five-image Blender-style scene (transforms_{train,val,test}.json with 3 / 1 / 1 frames, 48 x 48 RGBA PNGs written by PIL with
its default adaptive scanline filtering) and what PIL makes of the files: the decoded pixels and `Image.resize(LANCZOS)` at 48
(same size), 20, 31 and 80.  The GPU tests compare the HIP decode and resize with these bytes; the float targets are derived in
the tests from the stored bytes.  Everything is seeded and the archive is written with fixed timestamps, so a second run gives
the same bytes.

Fixture contents (blender_mini_expected.npz):
    names                      the five file stems, "<split>/r_<i>"
    rgba_<k>                   (48, 48, 4) uint8: PIL's decode of names[k]
    resized<s>_<k>             (s, s, 4) uint8: PIL's resize of names[k] to s x s, s in SIZES
    poses_<split>              (n, 3, 4) float64: the frames' transform_matrix[:3, :4]
"""
import io
import json
import math
import os
import sys
import zipfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENE = os.path.join(GOLDEN, "blender_mini")
S = 48
SIZES = (48, 20, 31, 80)
SPLITS = (("train", 3), ("val", 1), ("test", 1))
CAMERA_ANGLE_X = 0.6911112070083618


def make_image(k):
    """Smooth ramps, noisy patches, and alpha 0 / 255 / in between; the mix differs per image so that PIL's filter choice does."""
    rng = np.random.default_rng(100 + k)
    y, x = np.mgrid[0:S, 0:S]
    img = np.zeros((S, S, 4), np.int64)
    img[..., 0] = (x * 5 + k * 17) % 256                         # horizontal ramp
    img[..., 1] = (y * 5 + k * 29) % 256                         # vertical ramp
    img[..., 2] = ((x + y) * 3 + (x * y) // 7) % 256             # smooth in both directions
    alpha = np.clip(255 - 12 * np.abs(np.hypot(x - 24, y - 24 + 3 * k) - 14), 0, 255).astype(np.int64)   # ring: 255 -> 0
    alpha[:6] = 0
    alpha[-6:] = 255
    img[..., 3] = alpha
    # noisy patches (colour and alpha), flat bands, a band that repeats the row above
    img[8:20, 26:44, :3] = rng.integers(0, 256, (12, 18, 3))
    img[30:40, 4:16] = rng.integers(0, 256, (10, 12, 4))
    img[20 + k:24 + k, :, :3] = (40 * k + 10, 200 - 30 * k, 90)
    if k % 2:
        img[12:30, :, :] = rng.integers(0, 256, (18, S, 4))      # rows of pure noise
        img[26:30] = img[25:26]                                  # ... and exact copies of the row above
    else:
        img[40] = rng.integers(0, 256, (S, 4))                   # a noisy row, then rows that are the mean of left and up
        img[41:46, 0] = rng.integers(0, 256, (5, 4))
        for yy in range(41, 46):
            for xx in range(1, S):
                img[yy, xx] = (img[yy, xx - 1] + img[yy - 1, xx]) >> 1
    return img.astype(np.uint8)


def pose(k):
    """camera on a sphere of radius 4 looking at the origin (Blender convention: -z forward, y up)"""
    th, ph = 0.9 * k + 0.3, 0.5 + 0.15 * k
    c = 4.0 * np.array([math.cos(th) * math.cos(ph), math.sin(th) * math.cos(ph), math.sin(ph)])
    z = c / np.linalg.norm(c)
    xa = np.cross([0.0, 0.0, 1.0], z)
    xa /= np.linalg.norm(xa)
    ya = np.cross(z, xa)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = xa, ya, z, c
    return m


def premul_roundtrip(a):
    """RGBA -> RGBa -> RGBA as Pillow converts (nerf_pl_amd/csrc/image.hip restates the same integer arithmetic)"""
    a = a.astype(np.int64)
    al = a[..., 3:4]
    t = a[..., :3] * al + 128
    c = ((t >> 8) + t) >> 8
    back = np.minimum(255, (255 * c) // np.where(al == 0, 1, al))
    return np.where((al == 0) | (al == 255), c, back)


def write_npz(path, arrays):
    """np.savez_compressed with fixed timestamps (numpy stamps each member with the current time)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    from nerf_pl_amd.imageio_min import png_inflate
    arrays, names, filters_seen, k = {}, [], set(), 0
    observable = 0
    for split, n in SPLITS:
        os.makedirs(os.path.join(SCENE, split), exist_ok=True)
        frames = []
        for i in range(n):
            stem = "%s/r_%d" % (split, i)
            path = os.path.join(SCENE, stem + ".png")
            img = make_image(k)
            # PIL's encoder tries the Average filter only under `optimize`: the last training image is saved that way, so that the
            # scene holds every filter type; the other files take PIL's defaults
            Image.fromarray(img, "RGBA").save(path, optimize=(stem == "train/r_2"))
            with Image.open(path) as im:
                assert im.mode == "RGBA" and im.size == (S, S)
                arrays["rgba_%d" % k] = np.asarray(im).copy()
                assert np.array_equal(arrays["rgba_%d" % k], img)
                for s in SIZES:
                    arrays["resized%d_%d" % (s, k)] = np.asarray(im.resize((s, s), Image.LANCZOS)).copy()
            assert np.array_equal(arrays["resized%d_%d" % (S, k)], img)          # same size: PIL copies
            w, h, ch, raw = png_inflate(path)
            assert (w, h, ch) == (S, S, 4)
            filters_seen |= set(np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)[:, 0].tolist())
            partial = (img[..., 3] > 0) & (img[..., 3] < 255)
            observable += int((premul_roundtrip(img)[partial] != img[..., :3][partial]).any(-1).sum())
            m = pose(k)
            frames.append({"file_path": "./" + stem, "rotation": 0.012566370614359171, "transform_matrix": m.tolist()})
            names.append(stem)
            k += 1
        with open(os.path.join(SCENE, "transforms_%s.json" % split), "w") as f:
            json.dump({"camera_angle_x": CAMERA_ANGLE_X, "frames": frames}, f, indent=1)
        arrays["poses_" + split] = np.stack([np.array(fr["transform_matrix"])[:3, :4] for fr in frames])
    assert filters_seen == {0, 1, 2, 3, 4}, "PIL chose only the filter types %s: add an image that makes the others" % sorted(filters_seen)
    assert observable > 0, "no partial-alpha pixel changes under premultiply -> un-premultiply: the same-size bypass is unobservable"
    arrays["names"] = np.array(names)
    write_npz(os.path.join(GOLDEN, "blender_mini_expected.npz"), arrays)
    total = os.path.getsize(os.path.join(GOLDEN, "blender_mini_expected.npz"))
    for dp, _, fs in os.walk(SCENE):
        total += sum(os.path.getsize(os.path.join(dp, f)) for f in fs)
    print("filter types in the files: %s; partial-alpha pixels a premultiply round trip would change: %d" % (sorted(filters_seen), observable))
    print("fixtures: %d bytes in all" % total)


if __name__ == "__main__":
    main()

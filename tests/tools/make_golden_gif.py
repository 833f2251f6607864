"""Writes tests/golden/gif_mini/ (needs Pillow, no GPU):

    pillow_*.gif            small GIFs written BY PILLOW: fixtures for the two decoders (tests/gif_ref.py, imageio_min.read_gif)
    pillow_expected.npz     per file the (F, H, W, 3) pixels Pillow decodes from it
    frames.npz              the fixture frames of the quality gate (more than 256 occupied bins each) and `movie` (3, 64, 200, 3)
    pillow_record.json      per fixture frame the PSNR of Pillow's quantize(256, method=0, dither=NONE) against the original;
                            the size of Pillow's own save_all GIF of `movie`, and Pillow's version

    python tests/tools/make_golden_gif.py
"""
import io
import json
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gif_ref  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "golden", "gif_mini")


def pillow_pixels(data):
    im = Image.open(io.BytesIO(data))
    frames = []
    for k in range(im.n_frames):
        im.seek(k)
        frames.append(np.asarray(im.convert("RGB")).copy())
    return np.stack(frames)


def p_image(rgb):
    return Image.fromarray(rgb).quantize(256, method=0, dither=Image.Dither.NONE)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.RandomState(7)
    expected = {}

    def keep(name, data):
        px = pillow_pixels(data)
        dec = gif_ref.decode_gif(data)       # the fixtures hold whole, opaque frames only: the decoders composite nothing
        assert len(dec["frames"]) == len(px)
        for fr, want in zip(dec["frames"], px):
            assert (fr["left"], fr["top"]) == (0, 0) and fr["transparent"] is None and fr["indices"].shape == want.shape[:2], name
            assert np.array_equal(fr["palette"][fr["indices"]], want), name
        with open(os.path.join(OUT, name + ".gif"), "wb") as f:
            f.write(data)
        expected[name] = px

    # one frame, 16 colours (5-bit codes), a global table
    small = rng.randint(0, 16, (9, 13)).astype(np.uint8)
    im = Image.fromarray(small, "P")
    im.putpalette(rng.randint(0, 256, 48).astype(np.uint8).tobytes())
    buf = io.BytesIO()
    im.save(buf, "GIF", interlace=False)
    keep("pillow_one_16", buf.getvalue())
    # incompressible 256-colour data over several 255-byte sub-blocks, the code width climbing to 12 bits and the table
    # filling up
    noise = rng.randint(0, 256, (72, 80)).astype(np.uint8)
    im = Image.fromarray(noise, "P")
    im.putpalette(rng.permutation(256).astype(np.uint8).repeat(3).tobytes())
    buf = io.BytesIO()
    im.save(buf, "GIF", interlace=False)
    assert len(buf.getvalue()) > 4 * 255
    keep("pillow_noise_subblocks", buf.getvalue())
    # three frames that differ in every pixel, each with its own palette
    base = gif_ref.render_like(24, 40, seed=5)
    frames = [p_image(base), p_image(base ^ 0x80), p_image(base[::-1, ::-1] ^ 0x40)]
    buf = io.BytesIO()
    frames[0].save(buf, "GIF", save_all=True, append_images=frames[1:], duration=[30, 70, 110], loop=0, optimize=False, interlace=False)
    keep("pillow_three_local", buf.getvalue())
    np.savez_compressed(os.path.join(OUT, "pillow_expected.npz"), **expected)

    # the quality-gate frames and Pillow's figures for them
    movie = np.stack([gif_ref.render_like(64, 200, seed=s) for s in range(3)])
    gate = {"render_64x200": movie[0], "render_96x96": gif_ref.render_like(96, 96, seed=11),
            "noise_67x117": rng.randint(0, 256, (67, 117, 3)).astype(np.uint8),
            "bins257_20x20": gif_ref.bins_frame(257, 20, 20, seed=3),
            "gradient_48x64": np.stack(list(np.meshgrid(np.arange(64) * 4, np.arange(48) * 5, indexing="xy"))
                                       + [np.add.outer(np.arange(48), np.arange(64)) * 2], axis=-1).astype(np.uint8)}
    record = {"pillow": PIL.__version__, "psnr": {}, "occupied_bins": {}}
    for name, fr in gate.items():
        q = np.asarray(p_image(fr).convert("RGB"))
        record["psnr"][name] = gif_ref.psnr_u8(q, fr)
        record["occupied_bins"][name] = int(np.count_nonzero(gif_ref.histogram(fr)))
        assert record["occupied_bins"][name] > 256
    pf = [p_image(f) for f in movie]
    buf = io.BytesIO()
    pf[0].save(buf, "GIF", save_all=True, append_images=pf[1:], duration=30, loop=0)
    record["movie_gif_bytes"] = len(buf.getvalue())
    np.savez_compressed(os.path.join(OUT, "frames.npz"), movie=movie, **gate)
    with open(os.path.join(OUT, "pillow_record.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(record, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()

"""CPU: the GIF pipeline's numpy restatement (tests/gif_ref.py) writes valid files of acceptable quality, and both decoders
(gif_ref.decode_gif, imageio_min.read_gif) read what Pillow writes.  Fixtures: tests/golden/gif_mini (tests/tools/make_golden_gif.py).

Measured on the fixture frames, restatement minus Pillow's quantize(256, method=0, dither=NONE), dB (gate: >= -1.5):
    bins257_20x20 +13.14, gradient_48x64 +0.88, noise_67x117 +3.93, render_64x200 +0.97, render_96x96 +0.26
File of the three 64 x 200 `movie` frames: 15017 bytes against Pillow's own save_all file of 14248 (recorded, not asserted)."""
import io
import json
import os

import numpy as np
import pytest

import gif_ref
from nerf_pl_amd import imageio_min
from nerf_pl_amd import ops  # noqa: F401  (without the feature this module cannot import: ops.GIF_STRIP below)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gif_mini")
PILLOW_FILES = ("pillow_one_16", "pillow_noise_subblocks", "pillow_three_local")
assert ops.GIF_STRIP == gif_ref.STRIP


@pytest.fixture(scope="module")
def frames():
    return dict(np.load(os.path.join(GOLD, "frames.npz")))


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLD, "pillow_record.json")) as f:
        return json.load(f)


def _cases(frames):
    rng = np.random.RandomState(0)
    out = {k: v[None] for k, v in frames.items() if k != "movie"}
    out["movie"] = frames["movie"]
    out["one_pixel"] = np.array([[[[9, 200, 30]]]], np.uint8)
    out["flat"] = np.full((2, 70, 60, 3), 77, np.uint8)
    out["strip_edges"] = rng.randint(0, 256, (2, 1, 2 * gif_ref.STRIP + 1, 3)).astype(np.uint8) >> 6 << 6
    out["bins256"] = gif_ref.bins_frame(256, 20, 20, seed=2)[None]
    return out


@pytest.mark.parametrize("name", PILLOW_FILES)
def test_both_decoders_reproduce_pillows_pixels(name):
    with open(os.path.join(GOLD, name + ".gif"), "rb") as f:
        data = f.read()
    want = np.load(os.path.join(GOLD, "pillow_expected.npz"))[name]
    ref = gif_ref.decode_gif(data)
    ours = imageio_min.read_gif(data)
    assert len(ref["frames"]) == len(ours["indices"]) == len(want)
    assert (ref["width"], ref["height"]) == (ours["width"], ours["height"]) == want.shape[2:0:-1]
    for k, px in enumerate(want):
        fr = ref["frames"][k]
        assert np.array_equal(fr["palette"][fr["indices"]], px)
        assert np.array_equal(ours["palettes"][k][ours["indices"][k]], px)
        assert ours["delays"][k] == fr["delay"] and ours["offsets"][k] == (fr["left"], fr["top"]) == (0, 0)
    assert ours["loop"] == ref["loop"]
    if name == "pillow_three_local":
        assert ours["delays"] == [3, 7, 11] and ours["loop"] == 0
    if name == "pillow_noise_subblocks":
        assert len(data) > 4 * 255


def test_restatement_files_decode_to_palette_of_indices(frames):
    for name, movie in _cases(frames).items():
        for K in (gif_ref.STRIP, 100):
            data = gif_ref.gif_bytes(movie, fps=30, K=K)
            quant = [gif_ref.quantize(f) for f in movie]
            for dec in (gif_ref.decode_gif(data), None):
                if dec is None:
                    o = imageio_min.read_gif(data)
                    got = list(zip(o["indices"], o["palettes"], o["delays"]))
                    loop, size = o["loop"], (o["width"], o["height"])
                else:
                    got = [(f["indices"], f["palette"], f["delay"]) for f in dec["frames"]]
                    loop, size = dec["loop"], (dec["width"], dec["height"])
                assert len(got) == len(movie) and loop == 0 and size == movie.shape[2:0:-1], name
                for (idx, pal, delay), (want_idx, want_pal, _), f in zip(got, quant, movie):
                    assert delay == 3
                    assert np.array_equal(idx.ravel(), want_idx) and np.array_equal(pal, want_pal), name
                    assert np.array_equal(pal[idx], want_pal[want_idx].reshape(f.shape)), name


def test_pillow_decodes_the_restatement_files(frames):
    Image = pytest.importorskip("PIL.Image")
    for name, movie in _cases(frames).items():
        for fps, delay in ((30, 30), (12.5, 80)):
            data = gif_ref.gif_bytes(movie, fps=fps)
            im = Image.open(io.BytesIO(data))
            assert im.n_frames == len(movie) and im.size == movie.shape[2:0:-1] and im.info.get("loop") == 0, name
            for k, f in enumerate(movie):
                im.seek(k)
                idx, pal, _ = gif_ref.quantize(f)
                assert im.info["duration"] == delay
                assert np.array_equal(np.asarray(im.convert("RGB")), pal[idx].reshape(f.shape)), (name, k)


def test_strip_length_bound():
    """K = 3838 is the longest strip whose decoder never assigns code 4095: all-distinct pairs make every pixel an emission."""
    assert 257 + gif_ref.STRIP == 4095
    seq = []                                        # a de Bruijn sequence over pairs of bytes: no pair repeats
    for i in range(256):
        seq.append(i)
        for j in range(i + 1, 256):
            seq += [i, j]
    idx = np.array(seq[:gif_ref.STRIP], np.uint8)
    codes, widths = gif_ref.lzw_codes(idx)
    assert len(codes) == gif_ref.STRIP + 2 and widths.max() == 12 and widths[-1] == 12
    with pytest.raises(AssertionError):
        gif_ref.lzw_codes(idx, K=gif_ref.STRIP + 1)
    assert len(gif_ref.lzw(np.random.RandomState(0).randint(0, 256, 3 * gif_ref.STRIP))) <= gif_ref.data_stride(3, gif_ref.STRIP)


def test_quantiser_structure(frames):
    for name, movie in _cases(frames).items():
        for f in movie:
            hist = gif_ref.histogram(f)
            boxes = gif_ref.median_cut(hist)
            assert 1 <= len(boxes) <= 256
            cover = np.zeros((32, 32, 32), np.int32)
            for lo, hi, n in boxes:
                sub = hist[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
                assert n == sub.sum() > 0
                for ax in range(3):               # shrunk: both end slabs hold pixels
                    assert np.take(sub, 0, axis=ax).sum() > 0 and np.take(sub, -1, axis=ax).sum() > 0
                cover[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] += 1
            assert cover.max() == 1 and np.all(cover[hist > 0] == 1), name
            occupied = int(np.count_nonzero(hist))
            idx, pal, nbox = gif_ref.quantize(f)
            assert nbox == len(boxes) == min(256, occupied) or occupied > 256
            if occupied <= 256:                   # one bin per entry: the entry is the bin's mean colour
                assert all(lo == hi for lo, hi, _ in boxes)
                err = np.abs(pal[idx].astype(np.int32) - f.reshape(-1, 3))
                assert err.max() <= 7, name


def test_quality_gate_against_pillows_median_cut(frames, record):
    diffs = {}
    for name, want in sorted(record["psnr"].items()):
        f = frames[name]
        assert np.count_nonzero(gif_ref.histogram(f)) == record["occupied_bins"][name] > 256
        idx, pal, _ = gif_ref.quantize(f)
        diffs[name] = gif_ref.psnr_u8(pal[idx].reshape(f.shape), f) - want
        print("%-16s restatement - Pillow = %+.2f dB" % (name, diffs[name]))
    size = len(gif_ref.gif_bytes(frames["movie"]))
    print("movie: %d bytes, Pillow's save_all %d" % (size, record["movie_gif_bytes"]))
    for name, d in diffs.items():
        assert d >= -1.5, (name, d)


def test_container_pieces_match():
    assert imageio_min._gif_header(800, 600) == gif_ref.header(800, 600)
    for fps in (30, 12.5, 1, 100):
        assert imageio_min._gif_frame_header(800, 600, fps) == gif_ref.frame_header(800, 600, fps)
    with pytest.raises(ValueError):
        imageio_min.GifWriter(fps=0)
    with pytest.raises(ValueError):
        imageio_min.GifWriter().getvalue()

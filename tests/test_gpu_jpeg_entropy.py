"""GPU: the device entropy decoder (csrc/jpeg_entropy.hip, ops.jpeg_entropy_decode_batch) against the sequential host decoder
(ops.jpeg_entropy_decode), coefficient for coefficient, and LLFFDataset(jpeg_entropy="gpu") against the default dataset, bit for
bit.  All comparisons are exact (integers, or floats formed from equal bytes): nothing is left out."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
JPEGS = os.path.join(GOLDEN, "jpeg_mini")
SCENE = os.path.join(GOLDEN, "llff_mini")
SCENE_PNG = os.path.join(GOLDEN, "llff_mini_png")
SIZES = ((64, 48), (32, 24), (80, 60))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def _parse(name):
    from nerf_pl_amd.imageio_min import jpeg_parse
    p = jpeg_parse(os.path.join(JPEGS, name + ".jpg"))
    p["name"] = name + ".jpg"
    return p


@pytest.fixture(scope="module")
def fixtures():
    """{name: (parsed, the sequential decoder's coefficients)}, computed once"""
    from nerf_pl_amd import ops
    names = [f[:-4] for f in sorted(os.listdir(JPEGS)) if f.endswith(".jpg") and "progressive" not in f]
    out = {}
    for n in names:
        p = _parse(n)
        out[n] = (p, ops.jpeg_entropy_decode(p))
    assert len(out) >= 12
    return out


@pytest.fixture(scope="module")
def synthetic(fixtures):
    import jpeg_synth
    standard = fixtures["q90_420_61x45"][0]["huffman"]
    return jpeg_synth.edge_cases(standard), jpeg_synth.damaged_cases(standard)


def _same(got, want, i=0):
    return len(got) == len(want) and all(g.dtype == torch.int16 and g.is_cuda and np.array_equal(g[i].cpu().numpy(), w)
                                         for g, w in zip(got, want))


@pytest.mark.parametrize("bits", (32, 1024))
def test_every_fixture_alone_equals_the_host_decoder(dev, fixtures, bits):
    from nerf_pl_amd import ops
    for name, (parsed, want) in fixtures.items():
        got = ops.jpeg_entropy_decode_batch([parsed], dev, bits)
        assert [tuple(g.shape) for g in got] == [(1,) + w.shape for w in want], name
        assert _same(got, want), (name, bits)


def test_the_smallest_input_with_rounds_between_workgroups(dev, fixtures):
    """q90_444_61x45 at 32 bits: 3 workgroups of 256 subsequences, records corrected across their boundaries"""
    from nerf_pl_amd import _lib, ops
    parsed, want = fixtures["q90_444_61x45"]
    assert _lib.load().nerfhip_jpeg_entropy_workgroups(len(parsed["scan"]), 1, 32) == 3
    got, rounds = ops.jpeg_entropy_decode_batch([parsed], dev, 32, return_rounds=True)
    assert rounds >= 2 and _same(got, want)           # at least one round that changed a record and the one that confirms


def test_batches_give_each_image_as_it_comes_out_alone(dev, fixtures):
    """files of one size and sampling that differ in Huffman tables, quantisation tables and restart intervals; through
    decode_jpeg_batch the bytes are PIL's"""
    from nerf_pl_amd import ops
    z = np.load(os.path.join(GOLDEN, "jpeg_mini_expected.npz"))
    names = list(z["names"])
    for group in (["q90_420_61x45", "q75_420_61x45_optimized", "q85_420_61x45_restart3"], ["q30_420_64x48", "q50_420_64x48_restart1"]):
        for bits in (32, 1024):
            got = ops.jpeg_entropy_decode_batch([fixtures[n][0] for n in group], dev, bits)
            for i, n in enumerate(group):
                assert _same(got, fixtures[n][1], i), (n, bits)
        parsed = fixtures[group[0]][0]
        comps = parsed["components"]
        quant = torch.from_numpy(np.stack([np.stack([fixtures[n][0]["quant"][c[3]] for c in comps]).astype(np.int16) for n in group])).to(dev)
        rgbx = ops.decode_jpeg_batch(got, quant, parsed["height"], parsed["width"], comps[0][1], comps[0][2]).cpu().numpy()
        for i, n in enumerate(group):
            assert np.array_equal(rgbx[i, ..., :3], z["rgb_%d" % names.index(n)]), n


@pytest.mark.parametrize("bits", (32, 256, 4096))
def test_synthetic_edge_streams_give_their_coefficients_back(dev, synthetic, bits):
    from nerf_pl_amd import ops
    for name, parsed, coef in synthetic[0]:
        assert _same(ops.jpeg_entropy_decode_batch([parsed], dev, bits), [c for c in coef]), (name, bits)


def test_damaged_files_are_named_and_spare_the_batch(dev, synthetic):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    edge, damaged = synthetic
    bad = {n: p for n, p in damaged}
    for name in ("truncated_half", "invalid_code", "wrong_restart_number", "missing_restart", "no_prefix_code", "missing_table"):
        for bits in (32, 1024):
            with pytest.raises(NerfHipError, match=name + ".*damaged"):
                ops.jpeg_entropy_decode_batch([bad[name]], dev, bits)
    # a batch of three: the damaged one in the middle is named, the other two decode (their coefficients are read from the
    # tensors the failed call filled: status is per image)
    dense = [c for c in edge if c[0] == "dense"][0]
    cut = dict(dense[1], name="cut_in_the_middle", scan=dense[1]["scan"][:len(dense[1]["scan"]) // 2])
    with pytest.raises(NerfHipError, match="cut_in_the_middle") as e:
        ops.jpeg_entropy_decode_batch([dense[1], cut, dense[1]], dev, 32)
    assert "dense" not in str(e.value)
    import nerf_pl_amd.ops as ops_module
    seen = {}
    original = ops_module._jpeg_status_error

    def keep(what, parsed_list, status):
        seen["status"] = list(status)
    ops_module._jpeg_status_error = keep
    try:
        got = ops.jpeg_entropy_decode_batch([dense[1], cut, dense[1]], dev, 32)
    finally:
        ops_module._jpeg_status_error = original
    assert seen["status"] == [0, -4, 0]
    assert _same(got, dense[2], 0) and _same(got, dense[2], 2)


def test_refusals(dev, synthetic):
    from nerf_pl_amd import ops
    from nerf_pl_amd._lib import NerfHipError
    cases = {n: p for n, p, _ in synthetic[0]}
    with pytest.raises(NerfHipError, match="no CPU fallback"):
        ops.jpeg_entropy_decode_batch([cases["dense"]], "cpu")
    with pytest.raises(NerfHipError, match="k63_no_eob.*restart5"):
        ops.jpeg_entropy_decode_batch([cases["k63_no_eob"], cases["restart5"]], dev)
    with pytest.raises(NerfHipError, match="subseq_bits"):
        ops.jpeg_entropy_decode_batch([cases["dense"]], dev, 48)


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_llff_dataset_with_the_device_entropy_stage_equals_the_default(dev, w, h):
    from nerf_pl_amd.datasets import LLFFDataset
    host = LLFFDataset(SCENE, "train", (w, h), device=dev)
    gpu = LLFFDataset(SCENE, "train", (w, h), device=dev, jpeg_entropy="gpu")
    assert host.jpeg_entropy == "host" and gpu.jpeg_entropy == "gpu"
    assert gpu.all_rgbs.shape == (4 * h * w, 3) and torch.equal(gpu.all_rgbs, host.all_rgbs)
    a = LLFFDataset(SCENE, "val", (w, h), device=dev)[0]["rgbs"]
    b = LLFFDataset(SCENE, "val", (w, h), device=dev, jpeg_entropy="gpu")[0]["rgbs"]
    assert b.shape == (h * w, 3) and torch.equal(a, b)
    host = LLFFDataset(SCENE_PNG, "train", (w, h), device=dev)
    gpu = LLFFDataset(SCENE_PNG, "train", (w, h), device=dev, jpeg_entropy="gpu")
    assert sum(p.endswith(".png") for p in gpu.image_paths) == 1 and torch.equal(gpu.all_rgbs, host.all_rgbs)


def test_llff_dataset_refuses_an_unknown_entropy_stage(dev):
    from nerf_pl_amd.datasets import LLFFDataset
    with pytest.raises(ValueError, match="jpeg_entropy"):
        LLFFDataset(SCENE, "train", (32, 24), device=dev, jpeg_entropy="fpga")

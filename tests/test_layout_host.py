"""CPU: the index maps of nerf_pl_amd/csrc/mlp_layout.h — which input column of which weight matrix a B-operand slot multiplies,
where a ReLU gate bit lives, how the packed weight stream is laid out (bias block, the two looped layer triples), which saved
sections a weight-gradient job reads — checked on the host by a small g++ program (tests/host/layout_check.cpp).  The pack
kernels and the MLP kernels share these constexpr functions, so what holds here holds on the device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_maps_are_consistent(tmp_path):
    exe = str(tmp_path / "layout_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "nerf_pl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "layout_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "layout ok" in r.stdout, r.stdout + r.stderr


def test_dw_plan_header_is_plain_host_code(tmp_path):
    """nerf_pl_amd/csrc/mlp_dw_plan.h (the weight-gradient launch's split plan) compiles and links with g++ alone — csrc/ is the only
    include path, no HIP header on it — and plans the benchmark step (fine 1024 x 192 + coarse 1024 x 64 points) as the library does
    (tests/test_dw_plan.py): 256 workgroups with e4m3 storage, 256 in bf16, 512 in fp32."""
    exe = str(tmp_path / "dw_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "nerf_pl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "dw_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["256", "256", "512"], r.stdout + r.stderr


def test_ahead_of_step_weight_images_are_trusted_only_under_a_live_announcing_optimizer():
    """the announcer's mark used to be a flag FlatAdam set and nobody cleared.  It is a weak reference to the optimizer now
    (a model later stepped by something else is not vouched for by a dead FlatAdam), and load_state_dict — the reference's load_ckpt,
    utils/__init__.py:55-76 — bumps the weights' serial like an announced update."""
    import gc

    from nerf_pl_amd.models import NeRF

    class Opt:                      # stands in for optim.FlatAdam (which needs a GPU): what matters is the weak reference
        pass
    m = NeRF()
    assert not m.announced()
    opt = Opt()
    m.announced_by(opt)
    assert m.announced()
    del opt
    gc.collect()
    assert not m.announced()
    before = m.weights_serial()
    m.load_state_dict(NeRF().state_dict())
    assert m.weights_serial() == before + 1


def _check_flat_layout(ops, gw, gb, flat):
    """12 weight views of PARAM_SHAPES, then 12 bias views, back to back in `flat` (FLAT_GRAD_FLOATS = 595,844 floats)"""
    assert ops.FLAT_GRAD_FLOATS == 595844 == flat.numel() and len(gw) == len(gb) == 12
    assert [tuple(g.shape) for g in gw] == ops.PARAM_SHAPES and [tuple(g.shape) for g in gb] == [(s[0],) for s in ops.PARAM_SHAPES]
    off = flat.storage_offset()
    for g in gw + gb:
        assert g.is_contiguous() and g.storage_offset() == off and g.data_ptr() == flat.data_ptr() + 4 * (off - flat.storage_offset())
        off += g.numel()
    assert off - flat.storage_offset() == ops.FLAT_GRAD_FLOATS


def test_flat_grad_views_layout():
    """The gradient layout optim.FlatAdam and parallel.GradSync mirror, from the one function that builds it (ops.mlp_bwd and
    ops.mlp_bwd_multi both take their views from it)."""
    import torch

    from nerf_pl_amd import ops
    gw, gb, flat = ops.flat_grad_views(7, "cpu")
    _check_flat_layout(ops, gw, gb, flat)
    gw, gb, flat = ops.flat_grad_views(0, "cpu")              # an empty batch launches nothing: explicit zeros
    _check_flat_layout(ops, gw, gb, flat)
    assert not flat.any()
    # as a slice of a larger buffer (mlp_bwd_multi): views of that slice, zeroed in place for an empty batch only
    joint = torch.ones(2 * ops.FLAT_GRAD_FLOATS)
    gw, gb, flat = ops.flat_grad_views(0, "cpu", out=joint[ops.FLAT_GRAD_FLOATS:])
    _check_flat_layout(ops, gw, gb, flat)
    assert flat.storage_offset() == ops.FLAT_GRAD_FLOATS and not flat.any() and joint[:ops.FLAT_GRAD_FLOATS].all()
    gw, gb, flat = ops.flat_grad_views(3, "cpu", out=joint[:ops.FLAT_GRAD_FLOATS])
    assert flat.all() and gw[0].data_ptr() == joint.data_ptr()


def test_render_argument_rules_reject_before_any_pointer_is_taken():
    """ops._render_args (the argument structure of the single-launch kernels) applies the shared rules for perturb_rand, the noise
    draws and u on the host: a draw tensor of the wrong size is a ValueError, not an out-of-bounds device read.  Host logic only,
    so CPU tensors do here; the same rejections through every operator: tests/test_gpu_render_fused.py."""
    import pytest
    import torch

    from nerf_pl_amd import ops
    B, S, N = 4, 8, 4
    rays, pk = torch.zeros(B, 8), torch.zeros(16, dtype=torch.uint8)

    def args(perturb=0.0, perturb_rand=None, noise_c=None, noise_f=None, noise_std=0.0, u=None, n=N):
        return ops._render_args(rays, S, n, pk, pk, False, perturb, perturb_rand, noise_c, noise_f, noise_std, True, u, 1e-5, True)
    ok = dict(perturb=1.0, perturb_rand=torch.zeros(B, S), noise_c=torch.zeros(B, S), noise_f=torch.zeros(B, S + N), noise_std=1.0,
              u=torch.zeros(B, N))
    a, bufs, keep = args(**ok)
    assert a.u_stride == N and a.u == ok["u"].data_ptr() and a.perturb_rand == ok["perturb_rand"].data_ptr()
    assert a.noise_coarse == ok["noise_c"].data_ptr() and a.noise_fine == ok["noise_f"].data_ptr()
    a, _, _ = args(**dict(ok, u=torch.zeros(N)))
    assert a.u_stride == 0
    a, _, _ = args(**dict(ok, noise_std=0.0, perturb=0.0))     # noise_std == 0: no noise; perturb == 0: no jitter, whatever was drawn
    assert a.noise_coarse is None and a.noise_fine is None and a.perturb_rand is None
    a, _, _ = args(**dict(ok, n=0))                            # no fine pass: u and noise_fine are not read
    assert a.u is None and a.u_stride == 0 and a.noise_fine is None
    bad = [dict(perturb_rand=None), dict(perturb_rand=torch.zeros(B, S - 1)), dict(perturb_rand=torch.zeros(B, S, dtype=torch.float64)),
           dict(noise_c=None), dict(noise_f=None), dict(noise_c=torch.zeros(B, S + 1)), dict(noise_f=torch.zeros(B, S)),
           dict(u=torch.zeros(B, N + 1)), dict(u=torch.zeros(N + 1)), dict(u=torch.zeros(B * N)), dict(u=torch.zeros(1, N)),
           dict(u=torch.zeros(B, N, dtype=torch.float64))]
    for change in bad:
        with pytest.raises(ValueError):
            args(**dict(ok, **change))

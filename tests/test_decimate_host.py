"""CPU: the host twins of the mesh decimation (nerfhip_mesh_decimate_*_host through ops.mesh_decimate_host; csrc/decimate_core.h,
DESIGN.md §22) against the numpy restatement of the contract in tests/decimate_ref.py, on every mesh of mesh_ref.meshes() and on
the welded cubes, at cells 0.5, 0.25 and 0.05, with both placements.

Bit equality for cluster_of, triangles, counts, colours and the mean placement's vertices.  The quadric placement's vertices within
2^-23 max(|a|, |b|) + 1e-9 cell per coordinate: the systems have condition <= (1 + eps) / eps ~ 10^3 and at most a few hundred
fp64 terms, so the cofactor solve and np.linalg.solve are both within about 10^-11 cell of the exact solution, and what is left is
the one fp32 rounding.  Measured over the cases here: the largest difference is 9.6e-9 of that bound (flawed at 0.25; every other
case agrees to the last bit)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_ref as D  # noqa: E402
import mesh_ref as R  # noqa: E402

E_BADARG, E_ALIGN = -1, -3


@pytest.fixture(scope="module")
def lib():
    from nerf_pl_amd import build
    build.build(verbose=False)
    from nerf_pl_amd import _lib
    return _lib.load()


_TWIN = {}


def twin(case):
    """(vertices', triangles', colors', cluster_of, counts) of the host twin, computed once"""
    from nerf_pl_amd import ops
    if case not in _TWIN:
        name, cell, placement, origin, with_colors = case
        v, t = D.fixtures()[name]
        _TWIN[case] = ops.mesh_decimate_host(v, t, D.colors_for(v) if with_colors else None, cell, placement, origin)
    return _TWIN[case]


def case_id(case):
    return "%s-%g-%s%s%s" % (case[0], case[1], case[2], "-origin" if case[3] else "", "" if case[4] else "-nocolor")


def check_against(got, ref, cell, placement, what):
    """the comparison of the docstring; returns the largest quadric difference in units of the bound"""
    out_v, out_t, out_c, cluster_of, counts = got
    assert counts == ref["counts"], (what, counts, ref["counts"])
    assert out_t.dtype == np.int32 and cluster_of.dtype == np.int32 and out_v.dtype == np.float32
    assert np.array_equal(cluster_of, ref["cluster_of"]), what
    assert out_t.shape == ref["triangles"].shape and np.array_equal(out_t, ref["triangles"]), what
    assert (out_c is None) == (ref["colors"] is None), what
    if out_c is not None:
        assert out_c.dtype == np.uint8 and np.array_equal(out_c, ref["colors"]), what
    assert out_v.shape == ref["vertices"].shape, what
    if placement == "mean":
        assert np.array_equal(out_v.view(np.uint32), ref["vertices"].view(np.uint32)), what
        return 0.0
    a, b = out_v.astype(np.float64), ref["vertices"].astype(np.float64)
    bound = 2.0 ** -23 * np.maximum(np.abs(a), np.abs(b)) + 1e-9 * cell
    worst = float((np.abs(a - b) / bound).max()) if a.size else 0.0
    print("%s: quadric difference %.3g of the bound" % (what, worst))
    assert worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("case", D.cases(), ids=case_id)
def test_twin_equals_the_restatement(case):
    check_against(twin(case), D.reference(case), case[1], case[2], case_id(case))


@pytest.mark.parametrize("case", D.cases(), ids=case_id)
def test_invariants_of_the_output(case):
    name, cell, placement, origin, _ = case
    v, t = D.fixtures()[name]
    out_v, out_t, out_c, cluster_of, counts = twin(case)
    n_v, n_t = len(out_v), len(out_t)
    assert ((out_t >= 0) & (out_t < n_v)).all()                                                   # every index in range
    assert not ((out_t[:, 0] == out_t[:, 1]) | (out_t[:, 1] == out_t[:, 2]) | (out_t[:, 0] == out_t[:, 2])).any()
    rot = out_t[np.arange(n_t)[:, None], (out_t.argmin(1)[:, None] + np.arange(3)) % 3] if n_t else out_t
    assert len(np.unique(rot, axis=0)) == n_t                                                     # no duplicate
    assert np.array_equal(np.unique(out_t), np.arange(n_v))                                       # every vertex referenced
    assert out_c is None or out_c.shape == (n_v, 3)
    assert counts["clusters"] - counts["unreferenced"] == n_v
    # cluster_of is consistent with the triangles: the survivors, in order, are the good, uncollapsed, first-of-their-kind inputs
    assert cluster_of.shape == (len(v),) and cluster_of.min(initial=0) >= -1 and cluster_of.max(initial=-1) < n_v
    bad = R.bad_triangles(v, t)
    assert counts["bad"] == bad.sum()
    assert len(t) == n_t + counts["bad"] + counts["collapsed"] + counts["duplicate"]
    mapped = cluster_of[np.where(bad[:, None], 0, t)][~bad]
    mapped = mapped[(mapped >= 0).all(1) & (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 0] != mapped[:, 2])]
    turned = mapped[np.arange(len(mapped))[:, None], (mapped.argmin(1)[:, None] + np.arange(3)) % 3] if len(mapped) else mapped
    first = np.sort(np.unique(turned, axis=0, return_index=True)[1]) if len(mapped) else []
    assert np.array_equal(mapped[first].reshape(-1, 3), out_t)
    # a vertex moves by at most a cell
    inside = cluster_of >= 0
    finite = np.isfinite(v).all(1)
    assert not inside[~finite].any()
    if inside.any():
        ulp = np.spacing(np.float32(np.abs(v[finite]).max()))
        moved = np.abs(v[inside].astype(np.float64) - out_v[cluster_of[inside]].astype(np.float64))
        assert (moved <= np.float32(cell) + 4.0 * ulp).all(), moved.max()
    # the positions lie in their cells: [blo, bhi] before the rounding, which is monotonic
    if placement == "quadric":
        box = D.reference(case)["box"]
        assert (out_v >= box[:, 0].astype(np.float32)).all() and (out_v <= box[:, 1].astype(np.float32)).all()


def test_every_path_is_exercised():
    """the figures of the restatement alone say that the fixtures reach every path; the twin's equal them (test above)"""
    ref = {case_id(c): D.reference(c) for c in D.cases()}
    assert ref["identical-0.5-mean"]["counts"]["duplicate"] == 36
    c = ref["soup1000-0.5-mean"]["counts"]
    assert c["collapsed"] > 0 and c["duplicate"] > 0 and c["unreferenced"] > 0
    assert ref["flawed-0.5-quadric"]["counts"]["bad"] == R.flawed()[2].sum() > 0
    assert ref["cube12-0.4-quadric"]["clamped"] > 0 and ref["cube12-0.4-mean"]["clamped"] == 0
    nothing = ref["ico2-10-quadric"]
    assert nothing["counts"]["clusters"] == 1 and len(nothing["vertices"]) == 0 and len(nothing["triangles"]) == 0
    for case in D.cases():
        if case[0] == "ico2" and case[1] == 10.0:
            out_v, out_t, out_c, cluster_of, counts = twin(case)
            assert out_v.shape == (0, 3) and out_t.shape == (0, 3) and out_c.shape == (0, 3) and (cluster_of == -1).all()
            assert counts == {"clusters": 1, "bad": 0, "collapsed": len(R.icosphere(2)[1]), "duplicate": 0, "unreferenced": 1}


@pytest.mark.parametrize("placement", D.PLACEMENTS)
def test_ico0_is_returned_unchanged(placement):
    """12 vertices further apart than any cell here: every vertex is its own cluster (a mean of one, a quadric whose planes all pass
    through it), so the mesh comes back with its vertices renumbered in cell order and nothing else changed"""
    v, t = R.icosphere(0)
    for cell in D.CELLS:
        out_v, out_t, _, cluster_of, counts = twin(("ico0", cell, placement, None, True))
        assert counts == {"clusters": 12, "bad": 0, "collapsed": 0, "duplicate": 0, "unreferenced": 0}
        assert sorted(cluster_of.tolist()) == list(range(12))
        assert np.array_equal(out_v[cluster_of].view(np.uint32), v.view(np.uint32))
        assert np.array_equal(out_t, cluster_of[t])


def measures(vertices, triangles):
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    far = np.linalg.norm(vertices.astype(np.float64)[None] - corners[:, None], axis=2).min(1).max()
    return D.signed_volume(vertices, triangles), float(far), D.open_edges(triangles)


def test_the_placements_differ_as_claimed():
    """cube(10) at cell 0.37: both outputs are closed; the quadric placement keeps the volume (measured 7.9989 of 8) and the 8
    corners (0.00089 away at most), the mean shrinks the cube (7.6583) and rounds the corners off (0.148).  The thresholds hold for
    the restatement alone, and then for the twin."""
    for name, cell in (("ico%d" % k, c) for k in range(4) for c in (0.5, 0.25)):
        for placement in D.PLACEMENTS:
            assert D.open_edges(D.reference((name, cell, placement, None, True))["triangles"]) == 0, (name, cell, placement)
    for source in ("restatement", "twin"):
        got = {}
        for placement in D.PLACEMENTS:
            case = ("cube10", 0.37, placement, None, False)
            v, t = (D.reference(case)["vertices"], D.reference(case)["triangles"]) if source == "restatement" else twin(case)[:2]
            got[placement] = measures(v, t)
            print(source, placement, "volume %.4f  corner distance %.3g  open edges %d" % got[placement])
        assert got["quadric"][2] == 0 and got["mean"][2] == 0
        assert abs(got["quadric"][0] - 8.0) <= 0.008 and got["quadric"][1] <= 0.005
        assert got["mean"][0] < 7.8 and got["mean"][1] >= 0.1


def test_two_runs_give_identical_bytes_and_empty_inputs():
    from nerf_pl_amd import ops
    v, t = R.soup(257)
    col = D.colors_for(v)
    for placement in D.PLACEMENTS:
        a, b = (ops.mesh_decimate_host(v, t, col, 0.25, placement) for _ in range(2))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
    zero = dict.fromkeys(D.COUNTS, 0)
    for vv, tt in ((v[:0], t[:0]), (v, t[:0]), (v[:0], t)):
        out_v, out_t, out_c, cluster_of, counts = ops.mesh_decimate_host(vv, tt, col[:len(vv)], 0.25)
        ref = D.decimate(vv, tt, col[:len(vv)], 0.25)
        assert out_v.shape == (0, 3) and out_t.shape == (0, 3) and out_c.shape == (0, 3) and counts == zero == ref["counts"]
        assert np.array_equal(cluster_of, ref["cluster_of"]) and (cluster_of == -1).all() and len(cluster_of) == len(vv)
    # no finite vertex: every triangle is bad
    nan = np.full_like(v, np.nan)
    out = ops.mesh_decimate_host(nan, t, None, 0.25, "quadric")
    assert out[0].shape == (0, 3) and out[2] is None and out[4] == dict(zero, bad=len(t)) == D.decimate(nan, t, None, 0.25)["counts"]


def test_argument_refusals():
    from nerf_pl_amd import ops
    v, t = R.icosphere(2)
    for cell in (0.0, -0.5, float("nan"), float("inf"), 1e-60):
        with pytest.raises(ValueError):
            ops.mesh_decimate_host(v, t, None, cell)
        with pytest.raises(ValueError):
            D.decimate(v, t, None, cell)
    for fn in (ops.mesh_decimate_host, D.decimate):
        with pytest.raises(ValueError, match="cell too small"):
            fn(v, t, None, 1e-4)                                      # 20,000^3 cells
        with pytest.raises(ValueError, match="origin"):
            fn(v, t, None, 0.25, "mean", (-2.0, 0.5, -2.0))           # above the vertices with y < 0.5
        with pytest.raises(ValueError):
            fn(v, t, np.zeros((len(v) - 1, 3), np.uint8), 0.25)
        with pytest.raises(ValueError):
            fn(v, t, None, 0.25, "median")
    with pytest.raises(ValueError):
        ops.mesh_decimate_host(v, t, np.zeros((len(v), 4), np.uint8), 0.25)
    with pytest.raises(ValueError):
        ops.mesh_decimate_host(v, t, None, 0.25, "quadric", None, 0.0)
    fn = ops.mesh_decimate_host
    assert fn(v, t, None, 0.25, "mean", (-1.0, -1.0, -1.0))[4] == fn(v, t, None, 0.25, "mean", v.min(0))[4]     # on the minimum: allowed


def test_python_layer_refuses_cpu_tensors():
    import torch
    from nerf_pl_amd._lib import NerfHipError
    from nerf_pl_amd.decimate import decimate
    from nerf_pl_amd import ops
    v, t = R.icosphere(1)
    with pytest.raises(NerfHipError):
        decimate(torch.from_numpy(v), torch.from_numpy(t), cell=0.5)
    with pytest.raises(NerfHipError):
        ops.mesh_decimate(torch.from_numpy(v), torch.from_numpy(t), None, 0.5)
    with pytest.raises(ValueError):
        decimate(torch.from_numpy(v), torch.from_numpy(t))


def test_entry_points_validate_arguments_without_a_gpu(lib):
    """BADARG / ALIGN come back before anything is launched or dereferenced: the pointers below are never read"""
    import ctypes
    null, fake, odd, big = None, 0x10000, 0x10004, (1 << 28) + 1
    lo, res = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_int32 * 3)(4, 4, 4)
    huge = (ctypes.c_int32 * 3)(2048, 1024, 1024)
    assert lib.nerfhip_mesh_decimate_bounds(fake, big, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_bounds(null, 3, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_bounds(fake, 3, null, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_bounds_host(fake, -1, fake) == E_BADARG
    assert lib.nerfhip_mesh_decimate_keys(fake, 3, lo, 0.0, res, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_keys(fake, 3, lo, float("nan"), res, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_keys(fake, 3, lo, 0.5, huge, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_keys(fake, 3, lo, 0.5, res, null, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_keys(fake, 3, lo, 0.5, res, odd, null) == E_ALIGN
    assert lib.nerfhip_mesh_decimate_keys_host(fake, 0, lo, 0.5, res, null) == 0
    assert lib.nerfhip_mesh_decimate_clusters(null, 3, fake, fake, fake, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_clusters(odd, 3, fake, fake, fake, fake, fake, null) == E_ALIGN
    assert lib.nerfhip_mesh_decimate_entries(null, 3, 3, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_entries(fake, big, 3, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_entries_host(fake, 0, 3, fake, null) == 0
    place = (fake, 3, null, fake, 3, fake, fake, 2, fake, lo, 0.5, res)
    assert lib.nerfhip_mesh_decimate_place(*place, 1e-3, 2, fake, fake, null, null) == E_BADARG            # unknown placement
    assert lib.nerfhip_mesh_decimate_place(*place, 0.0, 1, fake, fake, null, null) == E_BADARG             # eps
    assert lib.nerfhip_mesh_decimate_place(*place, 1e-3, 1, fake, fake, fake, null) == E_BADARG            # colours out, none in
    assert lib.nerfhip_mesh_decimate_place(fake, 3, null, fake, 3, fake, fake, 4, fake, lo, 0.5, res, 1e-3, 0, fake, fake, null,
                                           null) == E_BADARG                                             # C > V
    assert lib.nerfhip_mesh_decimate_place(fake, 3, null, fake, 3, fake, fake, 2, null, lo, 0.5, res, 1e-3, 1, fake, fake, null,
                                           null) == E_BADARG                                             # quadric without entries
    assert lib.nerfhip_mesh_decimate_tri_keys(fake, 3, 3, fake, null, fake, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_tri_keys(fake, 3, 3, fake, fake, odd, fake, null) == E_ALIGN
    assert lib.nerfhip_mesh_decimate_duplicates(fake, null, 3, fake, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_duplicates_host(null, null, 0, null) == 0
    assert lib.nerfhip_mesh_decimate_mark(fake, 3, 3, fake, fake, 4, fake, fake, fake, fake, fake, fake, null) == E_BADARG     # C > V
    assert lib.nerfhip_mesh_decimate_mark(fake, 3, 3, fake, fake, 2, fake, fake, fake, fake, fake, null, null) == E_BADARG
    assert lib.nerfhip_mesh_decimate_compact(fake, 3, 3, fake, fake, 2, fake, fake, fake, fake, fake, fake, fake, fake, null, fake,
                                             null) == E_BADARG                                           # colours in, none out
    assert lib.nerfhip_mesh_decimate_compact(fake, 3, 3, fake, fake, 2, fake, fake, fake, fake, null, fake, fake, null, null, fake,
                                             null) == E_BADARG                                           # no output triangles

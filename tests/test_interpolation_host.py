"""Host side of the interpolation onto box and latitude-longitude grids
(climatemachine.jl_amd/mesh/interpolation.py): unwarp and Newton inverse, coverage of the output
grid by the element point lists, the reference's four Float64 accuracy rows
(test/Numerics/Mesh/interpolation.jl:428-444) through the NumPy restatement of its kernels,
exactness in the polynomial space, and the descriptor's layout.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

from cmdg_loader import cm

import interpolation_cases as IC
import interpolation_restatement as R

M = cm.mesh
I = cm.mesh.interpolation
EPS = float(np.finfo(np.float64).eps)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def sphere(N, rank=0, size=1):
    return IC.sphere_case(N, rank, size)


@functools.lru_cache(maxsize=None)
def brick(N, rank=0, size=1):
    return IC.brick_case(N, rank, size)


def linear_index(it):
    n1, n2, _ = it.dims
    return (it.i1.astype(np.int64) - 1) + n1 * ((it.i2.astype(np.int64) - 1) + n2 * (it.i3.astype(np.int64) - 1))


# ---- unwarp -----------------------------------------------------------------------------
def test_unwarp_inverts_the_warp_on_all_six_faces():
    R0 = IC.PLANET_RADIUS
    t = np.linspace(-1.0, 1.0, 13)            # includes the edges and corners of every face
    u, w = (g.reshape(-1) for g in np.meshgrid(t, t, indexing="ij"))
    one = np.ones_like(u)
    for sgn in (-1.0, 1.0):
        for abc in ((sgn * one, u, w), (u, sgn * one, w), (u, w, sgn * one)):
            a, b, c = (R0 * x for x in abc)
            x = M.equiangular_cubed_sphere_warp(a, b, c)
            back = M.equiangular_cubed_sphere_unwarp(*x)
            # on an edge or a corner the point belongs to two or three faces, and warp and unwarp
            # may each take another of them: the cube point is the same
            for got, want in zip(back, (a, b, c)):
                err = np.max(np.abs(got - want))
                assert err <= 2 * EPS * R0, err          # toler1 of the constructor


@pytest.mark.parametrize("N", [5, (5, 6)])
def test_newton_inverse_meets_its_tolerance(N):
    grid, it = sphere(N)
    xi = np.stack([it.xi1, it.xi2, it.xi3], axis=1)
    r = I.trilinear_map(xi, grid.topology.elemtocoord[it.element]) - it.x_unwarped
    assert np.sqrt((r * r).sum(axis=1)).max() <= it.nr_toler
    assert it.nr_toler == 10 * EPS * it.rad_grd[0]
    assert np.abs(xi).max() <= 1 + 1e-10


# ---- coverage ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [sphere, brick])
def test_one_rank_claims_every_point_exactly_once(case):
    grid, it = case(5)
    assert it.Npl == it.Np == int(np.prod(it.dims))
    assert it.offset[0] == 0 and (np.diff(it.offset) >= 0).all() and it.offset[-1] == it.Npl
    assert len(it.offset) == grid.nreal + 1
    assert np.array_equal(np.sort(linear_index(it)), np.arange(it.Np))
    assert it.i1.dtype == it.i2.dtype == it.i3.dtype == np.int32
    d = I.dimensions(it)
    assert [len(v[0]) for v in d.values()] == list(it.dims)
    assert list(d) == (["long", "lat", "level"] if it.is_sphere else ["x", "y", "z"])


def test_three_sphere_ranks_partition_the_grid():
    its = [sphere(5, r, 3)[1] for r in range(3)]
    lin = np.concatenate([linear_index(it) for it in its])
    assert np.array_equal(np.sort(lin), np.arange(its[0].Np))     # disjoint and complete
    for it in its:
        assert (np.diff(it.offset) >= 0).all() and it.offset[-1] == it.Npl


def test_three_brick_ranks_cover_the_grid_and_share_only_boundaries():
    pairs = [brick(5, r, 3) for r in range(3)]
    count = np.zeros(pairs[0][1].Np, dtype=np.int64)
    for _, it in pairs:
        lin = linear_index(it)
        assert len(np.unique(lin)) == len(lin)
        count[lin] += 1
        assert (np.diff(it.offset) >= 0).all() and it.offset[-1] == it.Npl
    assert count.min() >= 1
    for _, it in pairs:                                           # claimed twice => on an element boundary
        twice = count[linear_index(it)] > 1
        onb = ((np.abs(np.abs(it.xi1) - 1) < 1e-12) | (np.abs(np.abs(it.xi2) - 1) < 1e-12)
               | (np.abs(np.abs(it.xi3) - 1) < 1e-12))
        assert onb[twice].all()


# ---- the reference's accuracy rows ------------------------------------------------------
@pytest.mark.parametrize("N", [5, (5, 6)])
def test_reference_accuracy_row_brick(N):
    """interpolation.jl:432 and :435: L-inf error below 1e-9."""
    grid, it = brick(N)
    nstate = 6
    Q = IC.reference_state(grid, IC.BRICK_MAX, nstate)
    v = R.interpolate_local(it, Q)
    fiv = np.full((nstate,) + it.dims[::-1], np.nan)
    R.accumulate_interpolated_data([it], [v], fiv)
    err = np.abs(fiv - IC.brick_expected(it, nstate)).max()
    print("brick N = %s: L-inf error %.3e" % (N, err))
    assert err < IC.BRICK_TOL


@pytest.mark.parametrize("N", [5, (5, 6)])
def test_reference_accuracy_row_sphere(N):
    """interpolation.jl:441 and :444 with the projection of columns 2-4 and the expected values of
    :389-405: L-inf error below 2e-7."""
    grid, it = sphere(N)
    nstate = 5
    Q = IC.reference_state(grid, (IC.PLANET_RADIUS,) * 3, nstate)
    v = R.interpolate_local(it, Q)
    R.project_cubed_sphere(it, v, (2, 3, 4))
    fiv = np.full((nstate,) + it.dims[::-1], np.nan)
    R.accumulate_interpolated_data([it], [v], fiv)
    err = np.abs(fiv - IC.sphere_expected(it, nstate)).max()
    print("sphere N = %s: L-inf error %.3e" % (N, err))
    assert err < IC.SPHERE_TOL


# ---- exactness in the polynomial space --------------------------------------------------
@pytest.mark.parametrize("N", [(3, 3, 3), (4, 4, 2), (5, 5, 6)])
def test_polynomials_of_the_grid_degree_are_reproduced(N):
    rng = [np.linspace(-1.0, 1.0, 3), np.linspace(-1.0, 1.0, 4), np.linspace(-1.0, 1.0, 3)]
    topl = M.StackedBrickTopology(rng, periodicity=(False,) * 3)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    xg = [np.linspace(-1.0, 1.0, n) for n in (23, 17, 29)]
    it = I.InterpolationBrick(grid, np.array([[-1.0] * 3, [1.0] * 3]), *xg)
    gen = np.random.default_rng(7)
    cf = [gen.standard_normal(n + 1) for n in N]
    f = lambda x, y, z: (np.polynomial.polynomial.polyval(x, cf[0]) * np.polynomial.polynomial.polyval(y, cf[1])
                         * np.polynomial.polynomial.polyval(z, cf[2]))
    x1, x2, x3 = IC.node_coordinates(grid)
    Q = f(x1, x2, x3)[:, None, :]
    v = R.interpolate_local(it, np.ascontiguousarray(Q))
    want = f(xg[0][it.i1 - 1], xg[1][it.i2 - 1], xg[2][it.i3 - 1])
    assert np.abs(v[0] - want).max() <= 1e-12 * np.abs(Q).max()


def test_points_on_nodes_pick_the_nodal_value():
    N = 4
    rng = [np.linspace(0.0, 2.0, 3)] * 3
    topl = M.StackedBrickTopology(rng, periodicity=(False,) * 3)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    # the output axes are the LGL nodes of the first element along each axis
    xg = [0.5 * (grid.xi[d] + 1.0) for d in range(3)]
    it = I.InterpolationBrick(grid, np.array([[0.0] * 3, [2.0] * 3]), *xg)
    flg, fac = R.flags_and_factors(it)
    assert (flg > 0).all() and (fac == 1.0).all()
    Q = IC.random_state(grid, 2, seed=3)
    v = R.interpolate_local(it, Q)
    node = (flg[0] - 1) + (N + 1) * ((flg[1] - 1) + (N + 1) * (flg[2] - 1))
    el = np.repeat(np.arange(it.Nel), np.diff(it.offset))
    assert np.array_equal(v, Q[el, :, node].T)                    # exactly: no arithmetic on them


# ---- ABI --------------------------------------------------------------------------------
def test_interp_desc_struct_matches_header_field_order():
    txt = open(os.path.join(ROOT, "include", "cmdg.h")).read()
    body = txt[txt.index("typedef struct cmdg_interp_desc {"):txt.index("} cmdg_interp_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct cmdg_interp_desc {", "")
    fields = []
    for stmt in body.split(";"):
        stmt = " ".join(stmt.split())
        if stmt:
            for nm in re.sub(r"^(const\s+)?\w+\s+", "", stmt).split(","):
                fields.append(re.sub(r"\[.*\]", "", nm).replace("*", "").strip())
    assert fields == [f[0] for f in I.CmdgInterpDesc._fields_], fields


def test_interp_symbols_are_bound():
    L = cm._lib.lib()
    for name in ("create", "destroy", "apply", "project", "scatter"):
        assert hasattr(L, "cmdg_interp_" + name)

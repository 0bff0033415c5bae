"""NTracers on the host: counts, layout, descriptor, the cross-law harness and the plug-in source.
No device needed (``cmdg_physics_counts`` is host-only; the harness check runs on the oracle)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from helpers import cm
import tracers_crosslaw as TC

A = cm.atmos


def _counts(ip):
    L = cm._lib.lib()
    out = (C.c_int32 * 6)()
    ipa = (C.c_int32 * 16)(*[int(v) for v in ip])
    cm._lib.check(L.cmdg_physics_counts(A.DryAtmosModel.physics_id, C.cast(ipa, C.c_void_p), C.cast(out, C.c_void_p)))
    return tuple(out)


def _formula(orient, ref, hyp, smag, nt):
    return (5 + nt, 3 + 4 * orient + 7 * ref + smag + hyp + 2 + nt, 4 + smag + 4 * hyp + nt,
            9 + smag + 3 * nt, 4 * hyp, 12 * hyp)


# the Python model's counts before tracers existed (atmos.py, self.ns = 5 ...), written out
def _before(orient, ref, hyp, smag):
    naux = 3 + (4 if orient else 0) + (7 if ref else 0) + (1 if smag else 0) + (1 if hyp else 0) + 2
    return (5, naux, 4 + (1 if smag else 0) + (4 if hyp else 0), 9 + (1 if smag else 0),
            4 if hyp else 0, 12 if hyp else 0)


@pytest.mark.parametrize("nt", [0, 1, 2, 4])
def test_counts_of_the_device_functor_and_the_host_model(nt):
    ps = A.PlanetParameters()
    for orient, ref, hyp, smag in itertools.product((0, 1), repeat=4):
        ip = np.zeros(16, dtype=np.int32)
        ip[0], ip[1], ip[4], ip[14] = 2 * orient, ref, hyp, smag
        ip[15] = 3 | (nt << 8)                      # bits 0 and 1 belong to others
        got = _counts(ip)
        assert got == _formula(orient, ref, hyp, smag, nt), (orient, ref, hyp, smag, nt)
        if nt == 0:
            assert got == _before(orient, ref, hyp, smag)
        # the host model, where it can be built (its constructor refuses the other combinations)
        if (smag and (hyp or not orient)) or (ref and not orient) or (hyp and not orient):
            continue
        law = A.DryAtmosModel(None, orientation=A.ORIENT_SPHERICAL if orient else A.ORIENT_NONE,
                              ref_state=A.DecayingTemperatureProfile(ps) if ref else None,
                              hyperdiffusion_timescale=3600.0 if hyp else None,
                              smagorinsky=0.21 if smag else None,
                              tracers=A.NTracers(np.arange(1.0, nt + 1)) if nt else None)
        assert (law.ns, law.naux, law.ngrad, law.ngradflux, law.ngradlap, law.nhyper) == got
        assert law.off_tracers == law.off_moist + 2 == law.naux - nt
        assert _counts(law.descriptor()[0]) == got


def test_layout_names_aux_columns_and_descriptor():
    delta = (0.5, 3.0, 7.0)
    law = TC.box_model(delta=delta)
    assert law.ntracers == 3 and law.ns == 8
    assert law.state_names() == ["ρ", "ρu[1]", "ρu[2]", "ρu[3]", "energy.ρe", "tracers.ρχ[1]",
                                 "tracers.ρχ[2]", "tracers.ρχ[3]"]
    grid = TC.periodic_brick(Ne=1, N=2)
    aux = law.init_state_auxiliary(grid)
    free = TC.box_model()
    aux0 = free.init_state_auxiliary(grid)
    assert aux.shape[1] == aux0.shape[1] + 3
    assert np.array_equal(aux[:, :aux0.shape[1]], aux0)          # nothing moved
    for k, d in enumerate(delta):
        assert np.all(aux[:, law.off_moist + 2 + k, :] == d)
    Q = law.init_state_prognostic(grid, aux, 0.0)
    assert Q.shape[1] == 8 and np.all(Q[:, 5:] > 0)
    ip, dp = law.descriptor()
    ip0, dp0 = free.descriptor()
    assert (int(ip[15]) >> 8) & 0xff == 3 and int(ip[15]) & 0xff == int(ip0[15])
    assert np.array_equal(ip[:15], ip0[:15])
    assert tuple(dp[16:19]) == delta and np.array_equal(dp[:16], dp0[:16]) and not dp[19:].any()
    # tracers=None is the model of before: the same descriptor, byte for byte
    ps = A.PlanetParameters()
    kw = dict(orientation=A.ORIENT_FLAT, ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0), viscosity=TC.NU,
              sources=A.SRC_GRAVITY, boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT), param_set=ps)
    a, b = A.DryAtmosModel(None, **kw).descriptor(), A.DryAtmosModel(None, tracers=None, **kw).descriptor()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert not a[1][14:].any() and (int(a[0][15]) >> 8) == 0


def test_init_state_must_return_the_tracers_and_too_many_are_refused():
    law = TC.box_model(delta=(1.0,))
    law.init_state = lambda law_, aux, coord, t: (1.0 + 0 * coord[0], [0 * coord[0]] * 3, 1.0 + 0 * coord[0])
    grid = TC.periodic_brick(Ne=1, N=2)
    with pytest.raises(ValueError, match="tracer"):
        law.init_state_prognostic(grid, law.init_state_auxiliary(grid), 0.0)
    with pytest.raises(ValueError, match="tracers"):
        A.NTracers(np.ones(9))
    lin = A.AtmosAcousticGravityLinearModel(law)          # carries no tracers, on the wider auxiliary array
    assert (lin.ns, lin.naux) == (5, law.naux) and lin.state_names() == law.state_names()[:5]
    with pytest.raises(ValueError, match="tracer"):
        A.AtmosAcousticLinearModel(TC.plain_model((1.0,)))
    with pytest.raises(ValueError, match="tracer"):
        cm.moist.MoistAtmosModel(None, None, tracers=A.NTracers((1.0,)))
    with pytest.raises(ValueError, match="tracer"):
        A.DryAtmosModel(None, orientation=A.ORIENT_NONE, sources=A.SRC_MMS, tracers=(1.0,))


def test_held_suarez_dummy_tracers():
    """heldsuarez.jl:99-100 (rho chi[k] = k) and :184-186 (delta_chi[k] = k), k counted from one."""
    tr = A.HeldSuarezSetup.tracers(3)
    assert tr.delta_chi == (1.0, 2.0, 3.0) and A.HeldSuarezSetup.tracers(0) is None
    ps = A.PlanetParameters()
    law = A.DryAtmosModel(A.HeldSuarezSetup(ps), orientation=A.ORIENT_SPHERICAL,
                          ref_state=A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3),
                          hyperdiffusion_timescale=8 * 3600.0, param_set=ps, tracers=tr,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT))
    grid = TC.sphere(2, 1, N=2)
    Q, aux = TC.initial_state(law, grid)
    for k in range(3):
        assert np.all(Q[:, 5 + k, :] == k + 1) and np.all(aux[:, law.off_tracers + k, :] == k + 1)


def test_crosslaw_harness_reproduces_the_oracle_mass_tendency():
    """The harness judged before it judges device code, reference side only: fed rho in place of
    rho chi, without diffusion and under the central first-order flux, it must give the oracle dry
    law's own mass tendency, -div(rho u)."""
    from oracle import oracle as O
    O.build()

    def make_dg(law, grid, d, dd, nf):
        return O.OracleDGModel(law, grid, nf_first=nf, direction=d, diffusion_direction=dd)

    grid = TC.periodic_brick()
    free = TC.plain_model()
    Q, _ = TC.initial_state(free, grid)
    T = np.zeros_like(Q)
    make_dg(free, grid, 0, 0, 1)(T, Q.copy(), 0.0, 1.0, 0.0)
    u = [Q[:, 1 + d, :] / Q[:, 0, :] for d in range(3)]
    got = TC.advdiff_tendency(make_dg, grid, Q[:, 0, :], u=u, nf=1)
    err = TC.scaled_linf(got, T[:grid.nreal, 0, :])
    print("harness vs oracle mass tendency: %.3e (max |T| %.3e)" % (err, np.abs(T[:, 0]).max()))
    assert np.abs(T[:, 0]).max() > 1e-3
    assert err <= 1e-12


def test_plugin_source_names_the_tracer_count():
    src = cm.plugins.build_dry_atmos(orient=True, ref_state=True, hyperdiffusion=True, N=4, ntracers=3,
                                     source_only=True)
    assert "DryAtmos<true, true, true, false, false, 3>" in src
    assert "((d->iparam[15] >> 8) & 0xff) != 3" in src
    src0 = cm.plugins.build_dry_atmos(orient=True, ref_state=True, hyperdiffusion=True, smagorinsky=False,
                                      source_only=True)
    assert "DryAtmos<true, true, true, false>" in src0          # the tracer-free functor, as before
    assert "((d->iparam[15] >> 8) & 0xff) != 0" in src0         # ... which no longer takes a tracer descriptor
    with pytest.raises(ValueError, match="tracers"):
        cm.plugins.build_dry_atmos(ntracers=9, source_only=True)

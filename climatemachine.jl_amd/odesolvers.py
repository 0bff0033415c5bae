"""Host-side mirrors of the reference's ODE solvers: tableaus and work arrays here, every stage
loop inside libcmdg.

Explicit low-storage 2N: ``LowStorageRungeKutta2N`` / ``dostep!`` / ``update!``
``src/Numerics/ODESolvers/LowStorageRungeKuttaMethod.jl:26-62,102-158``;
``LSRK54CarpenterKennedy`` ``:293-327`` (rational coefficients converted to Float64),
``LSRK144NiegemannDiehlBusch`` ``:349-410``;
``solve!`` / ``general_dostep!`` ``ODESolvers.jl:49-158``;
``StrongStabilityPreservingRungeKutta`` and its four tableaus
``StrongStabilityPreservingRungeKuttaMethod.jl:27-285`` (``cmdg_ssprk_step``);
``LowStorageRungeKutta3N`` ``LowStorageRungeKutta3NMethod.jl`` (``cmdg_ls3n_step``);
``AdditiveRungeKutta``, LowStorageVariant, ``AdditiveRungeKuttaMethod.jl`` (``cmdg_ark_step``,
``cmdg_ark_step_gmres``);
``MRIGARKExplicit`` / ``MRIGARKDecoupledImplicit`` ``MultirateInfinitesimalGARK*.jl``
(``cmdg_mrigark_step``, ``cmdg_mrigark_step_gmres``).

The 2N stage loop is ``cmdg_lsrk_run``: five fused RHS+update passes per step, enqueued without
host synchronisation.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from . import _lib
from .systemsolvers import ColumnLU, GeneralizedMinimalResidual, GmresSolver, ManyColumnLU

__all__ = ["LSRK54CarpenterKennedy", "LSRK144NiegemannDiehlBusch", "solve",
           "LowStorageRungeKutta2N", "LSRK144_COEFFICIENTS", "StrongStabilityPreservingRungeKutta",
           "SSPRK22Heuns", "SSPRK22Ralstons", "SSPRK33ShuOsher", "SSPRK34SpiteriRuuth",
           "SSPRK_COEFFICIENTS", "LowStorageRungeKutta3N", "LS3NRK44Classic", "LS3NRK33Heuns",
           "LS3N_COEFFICIENTS", "AdditiveRungeKutta", "ARK2GiraldoKellyConstantinescu",
           "ark2gkc_tableau", "LinearBackwardEulerSolver", "ManyColumnLU", "GeneralizedMinimalResidual",
           "MRIGARKExplicit",
           "MRIGARKDecoupledImplicit", "MRIGARKERK33aSandu", "MRIGARKERK45aSandu",
           "MRIGARKIRK21aSandu", "MRIGARKESDIRK23LSA", "MRIGARKESDIRK24LSA", "MRIGARKESDIRK34aSandu",
           "MRIGARKESDIRK46aSandu", "MRIGARK_TABLEAUS", "mrigark_explicit_coefficients",
           "mrigark_implicit_coefficients"]


def _f(num, den):
    return float(Fraction(num, den))


def _advance(solver, nsteps, dt):
    # updatetime!: t += dt once per step (the running sum, not t0 + n * dt)
    for _ in range(int(nsteps)):
        solver.t += dt
    solver.steps += int(nsteps)


def _tableau(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _run(solver, nsteps, dt, call, handle=None):
    """``nsteps`` library calls ``call(t, dt)``, each from the running sum of the time (as
    cmdg_lsrk_run's steps start); a failure raises with the message of ``handle`` (``solver.dg``'s
    by default)."""
    solver.dg._torch_ready()
    for _ in range(int(nsteps)):
        _lib.check(call(float(solver.t), float(dt)), handle or solver.dg.handle)
        _advance(solver, 1, dt)


class LowStorageRungeKutta2N:
    def __init__(self, dg, RKA, RKB, RKC, Q, dt=0.0, t0=0.0):
        self.dg = dg
        self.RKA, self.RKB, self.RKC = tuple(RKA), tuple(RKB), tuple(RKC)
        self.dt, self.t = dt, t0
        self.steps = 0
        self.dQ = dg.create_state(Q.shape[1])          # zero initialised (:52-53)

    def dostep(self, Q, nsteps=1, dt=None):
        """``nsteps`` steps of size ``dt`` from ``self.t``; the solver's time and step count
        advance as ``general_dostep!`` / ``updatetime!`` do (ODESolvers.jl:56-73, 96-98)."""
        dt = self.dt if dt is None else dt
        self.dg.lsrk_run(Q, self.dQ, self.t, dt, nsteps, self.RKA, self.RKB, self.RKC)
        _advance(self, nsteps, dt)


def LSRK54CarpenterKennedy(dg, Q, dt=0.0, t0=0.0):
    RKA = (0.0, _f(-567301805773, 1357537059087), _f(-2404267990393, 2016746695238),
           _f(-3550918686646, 2091501179385), _f(-1275806237668, 842570457699))
    RKB = (_f(1432997174477, 9575080441755), _f(5161836677717, 13612068292357),
           _f(1720146321549, 2090206949498), _f(3134564353537, 4481467310338),
           _f(2277821191437, 14882151754819))
    RKC = (0.0, _f(1432997174477, 9575080441755), _f(2526269341429, 6820363962896),
           _f(2006345519317, 3224310063776), _f(2802321613138, 2924317926251))
    return LowStorageRungeKutta2N(dg, RKA, RKB, RKC, Q, dt=dt, t0=t0)


# the published 14-stage, 4th-order coefficients (Niegemann, Diehl & Busch 2012), as tabulated
# in LowStorageRungeKuttaMethod.jl:358-407
LSRK144_COEFFICIENTS = (
    (0.0, -0.7188012108672410, -0.7785331173421570, -0.0053282796654044, -0.8552979934029281,
     -3.9564138245774565, -1.5780575380587385, -2.0837094552574054, -0.7483334182761610,
     -0.7032861106563359, 0.0013917096117681, -0.0932075369637460, -0.9514200470875948,
     -7.1151571693922548),
    (0.0367762454319673, 0.3136296607553959, 0.1531848691869027, 0.0030097086818182,
     0.3326293790646110, 0.2440251405350864, 0.3718879239592277, 0.6204126221582444,
     0.1524043173028741, 0.0760894927419266, 0.0077604214040978, 0.0024647284755382,
     0.0780348340049386, 5.5059777270269628),
    (0.0, 0.0367762454319673, 0.1249685262725025, 0.2446177702277698, 0.2476149531070420,
     0.2969311120382472, 0.3978149645802642, 0.5270854589440328, 0.6981269994175695,
     0.8190890835352128, 0.8527059887098624, 0.8604711817462826, 0.8627060376969976,
     0.8734213127600976),
)


def LSRK144NiegemannDiehlBusch(dg, Q, dt=0.0, t0=0.0):
    RKA, RKB, RKC = LSRK144_COEFFICIENTS
    return LowStorageRungeKutta2N(dg, RKA, RKB, RKC, Q, dt=dt, t0=t0)


# (RKA rows, RKB, RKC) of StrongStabilityPreservingRungeKuttaMethod.jl:203-285: Heun, Ralston,
# Shu & Osher (1988) three-stage third-order, Spiteri & Ruuth (2002) four-stage third-order
SSPRK_COEFFICIENTS = {
    "SSPRK22Heuns": (((1.0, 0.0), (1 / 2, 1 / 2)), (1.0, 1 / 2), (0.0, 1.0)),
    "SSPRK22Ralstons": (((1.0, 0.0), (5 / 8, 3 / 8)), (_f(2, 3), 3 / 4), (0.0, _f(2, 3))),
    "SSPRK33ShuOsher": (((1.0, 0.0), (3 / 4, 1 / 4), (_f(1, 3), _f(2, 3))),
                        (1.0, 1 / 4, _f(2, 3)), (0.0, 1.0, 1 / 2)),
    "SSPRK34SpiteriRuuth": (((1.0, 0.0), (0.0, 1.0), (_f(2, 3), _f(1, 3)), (0.0, 1.0)),
                            (1 / 2, 1 / 2, _f(1, 6), 1 / 2), (0.0, 1 / 2, 1.0, 1 / 2)),
}


class StrongStabilityPreservingRungeKutta:
    """``StrongStabilityPreservingRungeKutta(f, RKA, RKB, RKC, Q; dt, t0)``
    (StrongStabilityPreservingRungeKuttaMethod.jl:27-75); the stage loop is ``cmdg_ssprk_step``."""

    def __init__(self, dg, RKA, RKB, RKC, Q, dt=0.0, t0=0.0):
        self.dg, self.dt, self.t, self.steps = dg, dt, t0, 0
        self.RKA, self.RKB, self.RKC = _tableau(RKA), _tableau(RKB), _tableau(RKC)
        self.Rstage = dg.create_state(Q.shape[1])
        self.Qstage = dg.create_state(Q.shape[1])

    def dostep(self, Q, nsteps=1, dt=None):
        _run(self, nsteps, self.dt if dt is None else dt, lambda t, dt: self.dg.L.cmdg_ssprk_step(
            self.dg.handle, Q.data_ptr(), self.Rstage.data_ptr(), self.Qstage.data_ptr(), t, dt,
            len(self.RKB), _ptr(self.RKA), _ptr(self.RKB), _ptr(self.RKC)))


def _ssp(name):
    def make(dg, Q, dt=0.0, t0=0.0):
        return StrongStabilityPreservingRungeKutta(dg, *SSPRK_COEFFICIENTS[name], Q, dt=dt, t0=t0)
    make.__name__ = name
    return make


SSPRK22Heuns, SSPRK22Ralstons = _ssp("SSPRK22Heuns"), _ssp("SSPRK22Ralstons")
SSPRK33ShuOsher, SSPRK34SpiteriRuuth = _ssp("SSPRK33ShuOsher"), _ssp("SSPRK34SpiteriRuuth")


# (RKA, RKB, RKC) of LowStorageRungeKutta3NMethod.jl:228-345: the classic fourth-order scheme and
# Heun's third-order scheme in Fyfe's 3N storage form
LS3N_COEFFICIENTS = {
    "LS3NRK44Classic": (((0.0, 0.0), (0.0, 1.0), (-1 / 2, 0.0), (2.0, -6.0)),
                        ((1 / 2, 0.0), (1 / 2, -1 / 2), (1.0, 0.0), (_f(1, 6), _f(1, 6))),
                        (0.0, 1 / 2, 1 / 2, 1.0)),
    "LS3NRK33Heuns": (((0.0, 0.0), (0.0, 1.0), (-1.0, _f(1, 3))),
                      ((_f(1, 3), 0.0), (_f(2, 3), -_f(1, 3)), (3 / 4, 1 / 4)),
                      (0.0, _f(1, 3), _f(2, 3))),
}


class LowStorageRungeKutta3N:
    """``LowStorageRungeKutta3N(f, RKA, RKB, RKC, RKW, Q; dt, t0)``
    (LowStorageRungeKutta3NMethod.jl:60-120); the stage loop is ``cmdg_ls3n_step``."""

    def __init__(self, dg, RKA, RKB, RKC, Q, dt=0.0, t0=0.0):
        self.dg, self.dt, self.t, self.steps = dg, dt, t0, 0
        self.RKA, self.RKB, self.RKC = _tableau(RKA), _tableau(RKB), _tableau(RKC)
        self.dQ = dg.create_state(Q.shape[1])
        self.dR = dg.create_state(Q.shape[1])

    def dostep(self, Q, nsteps=1, dt=None):
        _run(self, nsteps, self.dt if dt is None else dt, lambda t, dt: self.dg.L.cmdg_ls3n_step(
            self.dg.handle, Q.data_ptr(), self.dQ.data_ptr(), self.dR.data_ptr(), t, dt,
            len(self.RKC), _ptr(self.RKA), _ptr(self.RKB), _ptr(self.RKC)))


def _ls3n(name):
    def make(dg, Q, dt=0.0, t0=0.0):
        return LowStorageRungeKutta3N(dg, *LS3N_COEFFICIENTS[name], Q, dt=dt, t0=t0)
    make.__name__ = name
    return make


LS3NRK44Classic, LS3NRK33Heuns = _ls3n("LS3NRK44Classic"), _ls3n("LS3NRK33Heuns")


# -- IMEX: additive Runge-Kutta, LowStorageVariant (AdditiveRungeKuttaMethod.jl) ----------------

class LinearBackwardEulerSolver:
    """``LinearBackwardEulerSolver(solver; isadjustable = true)`` (BackwardEulerSolvers.jl:108-190):
    solves ``Q = Qhat + alpha L(Q)`` with ``ManyColumnLU()``, a direct column solver refactored
    whenever alpha changes (vertical linear models on stacked grids), or with
    ``GeneralizedMinimalResidual(...)`` (a linear model of any direction on any grid, one rank).
    With ``isadjustable = False`` the solver keeps the alpha it was first set up
    for: a solve or ``updatedt`` that needs another alpha is refused (the reference's
    ``@assert lin.isadjustable``).  ``preconditioner_update_freq > 0`` (ColumnwiseLUPreconditioner)
    is not implemented."""

    def __init__(self, solver, isadjustable=True, preconditioner_update_freq=-1):
        if not isinstance(solver, (ManyColumnLU, GeneralizedMinimalResidual)):
            raise TypeError("LinearBackwardEulerSolver: ManyColumnLU() and GeneralizedMinimalResidual() "
                            "are implemented")
        if preconditioner_update_freq > 0:
            raise ValueError("LinearBackwardEulerSolver: preconditioner_update_freq > 0 "
                             "(ColumnwiseLUPreconditioner) is not implemented")
        self.solver, self.isadjustable = solver, bool(isadjustable)

    def setup(self, linear_dg, alpha):
        """``setup_backward_Euler_solver``: the device solver for ``linear_dg`` and ``alpha``."""
        if isinstance(self.solver, GeneralizedMinimalResidual):
            return GmresSolver(linear_dg, alpha, self.solver)
        return ColumnLU(linear_dg, alpha)


def _refuse_alpha(lu, alpha):
    raise ValueError("LinearBackwardEulerSolver(isadjustable = false) was factored for alpha = %r; "
                     "alpha = %r would need a refactorisation" % (lu.alpha, alpha))


def ark2gkc_tableau(paperversion=False):
    """``(RKA_explicit, RKA_implicit, RKB, RKC)`` of ``ARK2GiraldoKellyConstantinescu``
    (AdditiveRungeKuttaMethod.jl:839-895), the same Float64 expressions; B and C are shared by
    the explicit and implicit tables."""
    s2 = math.sqrt(2)
    a32 = (3 + 2 * s2) / 6 if paperversion else float(Fraction(1, 2))
    RKA_explicit = ((0.0, 0.0, 0.0), (2 - s2, 0.0, 0.0), (1 - a32, a32, 0.0))
    RKA_implicit = ((0.0, 0.0, 0.0), (1 - 1 / s2, 1 - 1 / s2, 0.0),
                    (1 / (2 * s2), 1 / (2 * s2), 1 - 1 / s2))
    RKB = (1 / (2 * s2), 1 / (2 * s2), 1 - 1 / s2)
    RKC = (0.0, 2 - s2, 1.0)
    return RKA_explicit, RKA_implicit, RKB, RKC


class AdditiveRungeKutta:
    """``AdditiveRungeKutta(F, L, backward_euler_solver, RKA_explicit, RKA_implicit, RKB, RKC,
    split_explicit_implicit, LowStorageVariant(), Q; dt, t0)`` (AdditiveRungeKuttaMethod.jl:95-200)
    with ``LinearBackwardEulerSolver(ManyColumnLU())`` or ``LinearBackwardEulerSolver(
    GeneralizedMinimalResidual(...))``.  ``dg`` is the full model (every direction), ``linear_dg``
    the linear model on the same auxiliary state: vertical on a stacked grid for the column solver,
    of any direction on any grid for GMRES.  One step is one ``cmdg_ark_step`` /
    ``cmdg_ark_step_gmres``; the solver is built once for ``dt a_ii`` and refactored when ``dt``
    changes (``updatedt``).  With GMRES ``solve_info`` holds the ``GmresInfo`` of the last step's
    solves; a solve that stops unconverged at its iteration limit warns once."""

    def __init__(self, dg, linear_dg, backward_euler_solver, RKA_explicit, RKA_implicit, RKB, RKC,
                 Q, dt=None, t0=0.0, split_explicit_implicit=False):
        assert dt is not None
        if not isinstance(backward_euler_solver, LinearBackwardEulerSolver):
            raise TypeError("AdditiveRungeKutta: a LinearBackwardEulerSolver(ManyColumnLU() or "
                            "GeneralizedMinimalResidual()) is needed")
        A_e, A_i = _tableau(RKA_explicit), _tableau(RKA_implicit)
        ns = A_e.shape[0]
        diag = [A_i[i, i] for i in range(ns)]
        # LowStorageVariant preconditions (:157-168): diagonal (0, c, ..., c)
        if diag[0] != 0 or len(set(diag[1:])) != 1 or diag[1] == 0:
            raise ValueError("LowStorageVariant needs an implicit diagonal (0, c, ..., c)")
        self.dg, self.linear_dg = dg, linear_dg
        self.RKA_explicit, self.RKA_implicit = A_e, A_i
        self.RKB, self.RKC = _tableau(RKB), _tableau(RKC)
        self.split_explicit_implicit = bool(split_explicit_implicit)
        self.dt, self.t, self.steps = float(dt), t0, 0
        self.work = [dg.create_state(Q.shape[1]) for _ in range(2 * ns + 1)]
        nsl = linear_dg.balance_law.ns
        if nsl < Q.shape[1]:
            # a linear model without the full model's trailing tracers: four work states of its own
            # shape (the leading columns of a stage and of its tendency, Qhat and Qtt of the solve).
            # (Any other mismatch is the library's to refuse.)
            if not isinstance(backward_euler_solver.solver, ManyColumnLU):
                raise ValueError("AdditiveRungeKutta: the full model has %d states, the linear model %d; served are "
                                 "equal counts, and with ManyColumnLU a linear model that ends before the full "
                                 "model's tracers (GMRES pairs with differing counts are not)" % (Q.shape[1], nsl))
            self.work += [linear_dg.create_state() for _ in range(4)]
        self._ptrs = (C.c_void_p * len(self.work))(*[w.data_ptr() for w in self.work])
        self.isadjustable = backward_euler_solver.isadjustable
        self._diag = diag[1]
        self.lu = backward_euler_solver.setup(linear_dg, self.dt * diag[1])
        self._gmres = isinstance(self.lu, GmresSolver)
        self.solve_info = []

    def updatedt(self, dt):
        """``updatedt!``: the next stage refactors the column matrices for ``dt a_ii`` (refused
        when the solver is not adjustable and ``dt a_ii`` changes)."""
        if not self.isadjustable and float(dt) * self._diag != self.lu.alpha:
            _refuse_alpha(self.lu, float(dt) * self._diag)
        self.dt = float(dt)

    def dostep(self, Q, nsteps=1, dt=None):
        dt = self.dt if dt is None else dt
        if not self.isadjustable and dt * self._diag != self.lu.alpha:
            _refuse_alpha(self.lu, dt * self._diag)
        step = self.dg.L.cmdg_ark_step_gmres if self._gmres else self.dg.L.cmdg_ark_step
        _run(self, nsteps, dt, lambda t, dt: step(
            self.dg.handle, self.lu.handle, Q.data_ptr(), C.cast(self._ptrs, C.c_void_p), t, dt,
            len(self.RKB), _ptr(self.RKA_explicit), _ptr(self.RKA_implicit), _ptr(self.RKB),
            _ptr(self.RKC), int(self.split_explicit_implicit)), self.linear_dg.handle)
        if self._gmres:
            self.lu.alpha = dt * self._diag
            self.solve_info = self.lu.step_info()

    def close(self):
        self.lu.close()


def ARK2GiraldoKellyConstantinescu(dg, linear_dg, backward_euler_solver, Q, dt=None, t0=0.0,
                                   split_explicit_implicit=False, paperversion=False):
    """``ARK2GiraldoKellyConstantinescu(F, L, backward_euler_solver, Q; dt, t0,
    split_explicit_implicit, variant = LowStorageVariant(), paperversion)``
    (AdditiveRungeKuttaMethod.jl:839-895)."""
    A_e, A_i, B, Cc = ark2gkc_tableau(paperversion)
    return AdditiveRungeKutta(dg, linear_dg, backward_euler_solver, A_e, A_i, B, Cc, Q, dt=dt,
                              t0=t0, split_explicit_implicit=split_explicit_implicit)


# -- multirate infinitesimal GARK (Sandu 2019) ----------------------------------------------------
# MultirateInfinitesimalGARKExplicit.jl and MultirateInfinitesimalGARKDecoupledImplicit.jl.  The
# rational tables are exact (Fraction) until the reference converts them to Float64; the tables
# the reference builds in Float64 arithmetic are built here in the same operation order.

def _rt(rows):
    """Rows of ``"num/den"`` strings (``"0"`` for zero) as Fractions."""
    return [[Fraction(x) for x in r.split()] for r in rows]


def _isapprox(a, b, rtol=math.sqrt(2.0 ** -52), atol=0.0):
    """Julia's ``isapprox`` (default rtol sqrt(eps)), on scalars or on arrays through the norm."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = float(np.linalg.norm((a - b).ravel()))
    return d <= max(atol, rtol * max(float(np.linalg.norm(a.ravel())), float(np.linalg.norm(b.ravel()))))


def _erk33a(delta=Fraction(-1, 2)):
    d = delta
    G0 = [[Fraction(1, 3), Fraction(0), Fraction(0)],
          [(-6 * d - 7) / 12, (6 * d + 11) / 12, Fraction(0)],
          [Fraction(0), (6 * d - 5) / 12, (3 - 2 * d) / 4]]
    G1 = [[Fraction(0)] * 3,
          [(2 * d + 1) / 2, -(2 * d + 1) / 2, Fraction(0)],
          [Fraction(1, 2), -(2 * d + 1) / 2, d]]
    return (G0, G1), ([Fraction(1, 12), Fraction(-1, 3), Fraction(7, 12)], [Fraction(0)] * 3)


def _erk45a():
    G0 = _rt(["1/5 0 0 0 0", "-53/16 281/80 0 0 0",
              "-36562993/71394880 34903117/17848720 -88770499/71394880 0 0",
              "-7631593/71394880 -166232021/35697440 6068517/1519040 8644289/8924360 0",
              "277061/303808 -209323/1139280 -1360217/1139280 -148789/56964 147889/45120"])
    G1 = _rt(["0 0 0 0 0", "503/80 -503/80 0 0 0",
              "-1365537/35697440 4963773/7139488 -1465833/2231090 0 0",
              "66974357/35697440 21445367/7139488 -3 -8388609/4462180 0",
              "-18227/7520 2 1 5 -41933/7520"])
    g0 = _rt(["-1482837/759520 175781/71205 -790577/1139280 -6379/56964 47/96"])[0]
    g1 = _rt(["6213/1880 -6213/1880 0 0 0"])[0]
    return (G0, G1), (g0, g1)


def _irk21a():
    return (_rt(["1 0", "-1/2 1/2"]),), (_rt(["-1/2 1/2"])[0],)


def _esdirk_lambda():
    """``λ`` of ESDIRK34a / ESDIRK46a, with the reference's check of its cubic."""
    mu = math.atan(1 / (2 * math.sqrt(2.0))) / 3            # acot(2 sqrt(2)) / 3
    lam = 1 - math.cos(mu) / math.sqrt(2.0) + math.sqrt(1.5) * math.sin(mu)
    assert _isapprox(-1 + 9 * lam - 18 * (lam * lam) + 6 * (lam * lam * lam), 0, atol=2 * 2.0 ** -52)
    return lam


def _esdirk34a():
    lam = _esdirk_lambda()
    l2 = lam * lam
    G0 = [[float(Fraction(1, 3)), 0.0, 0.0, 0.0],
          [-lam, lam, 0.0, 0.0],
          [(3 - 10 * lam) / (24 * lam - 6), (5 - 18 * lam) / (6 - 24 * lam), 0.0, 0.0],
          [(-24 * l2 + 6 * lam + 1) / (6 - 24 * lam), (-48 * l2 + 12 * lam + 1) / (24 * lam - 6), lam, 0.0],
          [(3 - 16 * lam) / (12 - 48 * lam), (48 * l2 - 21 * lam + 2) / (12 * lam - 3), (3 - 16 * lam) / 4, 0.0],
          [-lam, 0.0, 0.0, lam]]
    return (G0,), ([0.0] * 4,)


def _esdirk46a():
    _esdirk_lambda()
    G0 = _rt(["1/5 0 0 0 0 0", "-1/4 1/4 0 0 0 0",
              "1771023115159/1929363690800 -1385150376999/1929363690800 0 0 0 0",
              "914009/345800 -1000459/345800 1/4 0 0 0",
              "18386293581909/36657910125200 5506531089/80566835440 -178423463189/482340922700 0 0 0",
              "36036097/8299200 4621/118560 -38434367/8299200 1/4 0 0",
              "-247809665162987/146631640500800 10604946373579/14663164050080 "
              "10838126175385/5865265620032 -24966656214317/36657910125200 0 0",
              "38519701/11618880 10517363/9682400 -23284701/19364800 -10018609/2904720 1/4 0",
              "-52907807977903/33838070884800 74846944529257/73315820250400 "
              "365022522318171/146631640500800 -20513210406809/109973730375600 "
              "-2918009798/1870301537 0",
              "19/100 -73/300 127/300 127/300 -313/300 1/4"])
    G1 = _rt(["0 0 0 0 0 0", "0 0 0 0 0 0",
              "-1674554930619/964681845400 1674554930619/964681845400 0 0 0 0",
              "-1007739/172900 1007739/172900 0 0 0 0",
              "-8450070574289/18328955062600 -39429409169/40283417720 173621393067/120585230675 0 0 0",
              "-122894383/16598400 14501/237120 121879313/16598400 0 0 0",
              "32410002731287/15434909526400 -46499276605921/29326328100160 "
              "-34914135774643/11730531240064 45128506783177/18328955062600 0 0",
              "-128357303/23237760 -35433927/19364800 71038479/38729600 8015933/1452360 0 0",
              "136721604296777/67676141769600 -349632444539303/146631640500800 "
              "-1292744859249609/293263281001600 8356250416309/54986865187800 "
              "17282943803/3740603074 0",
              "3/25 -29/300 71/300 71/300 -149/300 0"])
    g0 = _rt(["-1/4 5595/8804 -2445/8804 -4225/8804 2205/4402 -567/4402"])[0]
    return (G0, G1), (g0, [Fraction(0)] * 6)


def _esdirk23lsa(delta=0):
    rt2 = math.sqrt(2.0)
    d = delta
    G0 = [[2 - rt2, 0.0, 0.0],
          [(1 - rt2) / rt2, (rt2 - 1) / rt2, 0.0],
          [float(d), rt2 - 1 - d, 0.0],
          [(3 - (2 * rt2) * (1 + d)) / (2 * rt2), (d * (2 * rt2) - 1) / (2 * rt2), (rt2 - 1) / rt2]]
    dc = [sum(r) for r in G0]
    assert _isapprox(G0[0][0], dc[0]) and _isapprox(G0[2][0] + G0[2][1], dc[2])
    assert _isapprox(G0[1][0] + G0[1][1], 0, atol=2.0 ** -52)
    assert _isapprox(G0[3][0] + G0[3][1] + G0[3][2], 0, atol=2.0 ** -52)
    assert _isapprox(G0[0][0] + G0[1][0], 1 - 1 / rt2) and _isapprox(G0[1][1], 1 - 1 / rt2)
    assert _isapprox(G0[0][0] + G0[1][0] + G0[2][0] + G0[3][0], 1 / (2 * rt2))
    assert _isapprox(G0[1][1] + G0[2][1] + G0[3][1], 1 / (2 * rt2))
    assert _isapprox(G0[3][2], 1 - 1 / rt2)
    return (G0,), ([0.0] * 3,)


def esdirk24lsa_base(gamma=0.2, c3=None, a32=0.2, alpha=-0.1, beta1=None, beta2=None):
    """The L-stable, stiffly accurate ESDIRK behind ``MRIGARKESDIRK24LSA`` and its GARK table:
    ``(A, Δc, Γ0)``, with the reference's checks."""
    g = gamma
    c3 = (2 * g + 1) / 2 if c3 is None else c3
    beta1 = c3 / 10 if beta1 is None else beta1
    beta2 = c3 / 10 if beta2 is None else beta2
    # L-stability (Kennedy and Carpenter 2016, Table 5) and increasing stage times
    if not (0.1804253064293985641345831 <= g < 0.5):
        raise ValueError("MRIGARKESDIRK24LSA: gamma must lie in [0.18042530642939856, 1/2)")
    if not (2 * g < c3 < 1):
        raise ValueError("MRIGARKESDIRK24LSA: 2 gamma < c3 < 1 is needed")
    b3 = (2 * ((1 - g) * (1 - g)) - 1) / 4 / a32
    b2 = (1 - 2 * g - 2 * b3 * c3) / (4 * g)
    A = [[0.0, 0.0, 0.0, 0.0], [g, g, 0.0, 0.0], [c3 - a32 - g, a32, g, 0.0],
         [1 - b2 - b3 - g, b2, b3, g]]
    c = [sum(r) for r in A]
    b = A[-1]
    assert _isapprox(sum(b), 1)
    assert _isapprox(2 * sum(float(np.dot(np.asarray(A).T[i], b)) for i in range(4)), 1)
    dc = [c[1], 0.0, c[2] - c[1], 0.0, c[3] - c[2], 0.0]
    G = [[0.0] * 4 for _ in range(6)]
    G[0][0] = dc[0]
    G[1][0] = A[1][0] - G[0][0]
    G[1][1] = A[1][1]
    G[2][0] = alpha
    G[2][1] = dc[2] - G[2][0]
    G[3][0] = A[2][0] - G[0][0] - G[1][0] - G[2][0]
    G[3][1] = A[2][1] - G[0][1] - G[1][1] - G[2][1]
    G[3][2] = A[2][2]
    G[4][0] = beta1
    G[4][1] = beta2
    G[4][2] = dc[4] - G[4][0] - G[4][1]
    for j in range(3):
        G[5][j] = A[3][j] - G[0][j] - G[1][j] - G[2][j] - G[3][j] - G[4][j]
    G[5][3] = A[3][3]
    acc = np.cumsum(np.asarray(G), axis=0)
    assert _isapprox(A, np.vstack([np.zeros((1, 4)), acc[1::2]]))
    assert _isapprox(dc, [sum(r) for r in G])
    return A, dc, G


def _esdirk24lsa(**kw):
    _, _, G0 = esdirk24lsa_base(**kw)
    return (G0,), ([0.0] * 4,)


# name -> (kind, raw table builder): the Γ and γ̂ as the reference passes them to the solver
MRIGARK_TABLEAUS = {
    "MRIGARKERK33aSandu": ("explicit", _erk33a),
    "MRIGARKERK45aSandu": ("explicit", _erk45a),
    "MRIGARKIRK21aSandu": ("implicit", _irk21a),
    "MRIGARKESDIRK23LSA": ("implicit", _esdirk23lsa),
    "MRIGARKESDIRK24LSA": ("implicit", _esdirk24lsa),
    "MRIGARKESDIRK34aSandu": ("implicit", _esdirk34a),
    "MRIGARKESDIRK46aSandu": ("implicit", _esdirk46a),
}


def _rowsum(row):
    s = 0
    for x in row:
        s = s + x
    return s


def mrigark_explicit_coefficients(Gs, ghats):
    """``MRIGARKExplicit``'s constructor: ``Δc = rowsum(Γ_0)``, ``Γ_k ./ Δc`` and ``γ̂_k / Δc[end]``
    (exact when the tables are rational), then Float64.  Returns ``(Γs, γ̂s, Δc)`` as numpy
    arrays."""
    dc = [_rowsum(r) for r in Gs[0]]
    G = np.array([[[float(x / dc[i]) for x in row] for i, row in enumerate(Gk)] for Gk in Gs])
    gh = np.array([[float(x / dc[-1]) for x in g] for g in ghats])
    return G, gh, np.array([float(x) for x in dc])


def mrigark_implicit_coefficients(Gs, ghats):
    """``MRIGARKDecoupledImplicit``'s constructor: ``Δc = rowsum(Γ_0)`` (exact when rational), the
    even rows' sums 0 to ``2 eps``, the odd rows' kept; ``Γ_k`` and ``γ̂_k`` as given, in Float64.
    Returns ``(Γs, γ̂s, Δc)`` as numpy arrays."""
    dc = [float(_rowsum(r)) for r in Gs[0]]
    if not all(abs(x) <= 2 * 2.0 ** -52 for x in dc[1::2]):
        raise ValueError("MRIGARKDecoupledImplicit: the implicit rows of Gamma_0 must sum to 0")
    dc = dc[0:len(dc) - 1:2]
    ns = len(dc)
    if not (ns == len(Gs[0][0]) - 1 and ns == len(Gs[0]) // 2):
        raise ValueError("MRIGARKDecoupledImplicit: Gamma must be (2 nstages, nstages + 1)")
    G = np.array([[[float(x) for x in row] for row in Gk] for Gk in Gs])
    gh = np.array([[float(x) for x in g] for g in ghats])
    return G, gh, np.array(dc)


def _operator(op):
    """(handle, subtracted handle or None, the DGModel that owns the device) of a solver operator:
    a DGModel or a ``dgmodel.RemainderDGModel``."""
    from .dgmodel import RemainderDGModel
    if isinstance(op, RemainderDGModel):
        return op.dg.handle, op.lin.handle, op.dg
    return op.handle, None, op


def _fast_solver(fastsolver, who):
    if isinstance(fastsolver, (MRIGARKExplicit, MRIGARKDecoupledImplicit)):
        raise TypeError("%s: nested (three-rate) MRI is not supported" % who)
    if not isinstance(fastsolver, LowStorageRungeKutta2N):
        raise TypeError("%s: the fast solver must be a LowStorageRungeKutta2N (LSRK54CarpenterKennedy "
                        "or LSRK144NiegemannDiehlBusch), not %s" % (who, type(fastsolver).__name__))
    if len(fastsolver.RKA) > 14:
        raise ValueError("%s: fast 2N tableaus of at most 14 stages are supported" % who)
    return fastsolver


class _MRIGARK:
    """What the two MRI-GARK kinds share: the descriptor of ``cmdg_mrigark_step`` and ``dostep``."""

    KIND = None

    def _setup(self, slow_rhs, fastsolver, G, gh, dc, Q, dt, t0, lu=None, adjustable=True):
        self.slow_rhs, self.fastsolver = slow_rhs, fastsolver
        self.Gammas, self.gammahats, self.dc = G, gh, dc
        self.dt, self.t, self.steps = float(dt), float(t0), 0
        self._slow = _operator(slow_rhs)
        self._fast = _operator(fastsolver.dg)
        self.dg = self._slow[2]
        ns = len(dc)
        self.Rstages = [self.dg.create_state(Q.shape[1]) for _ in range(ns)]
        self.Qhat = self.dg.create_state(Q.shape[1]) if self.KIND == 1 else None
        ptrs = [r.data_ptr() for r in self.Rstages] + [fastsolver.dQ.data_ptr(),
                                                        self.Qhat.data_ptr() if self.Qhat is not None else 0]
        self._work = (C.c_void_p * len(ptrs))(*ptrs)
        self._G, self._dc = _tableau(G), _tableau(dc)
        self._fa, self._fb, self._fc = (_tableau(x) for x in (fastsolver.RKA, fastsolver.RKB, fastsolver.RKC))
        d = _lib.CmdgMrigarkDesc()
        d.kind, d.nstages, d.ngamma = self.KIND, ns, self._G.shape[0]
        d.gamma, d.dc = self._G.ctypes.data, self._dc.ctypes.data
        d.fast_nstages = len(self._fa)
        d.fast_rka, d.fast_rkb, d.fast_rkc = self._fa.ctypes.data, self._fb.ctypes.data, self._fc.ctypes.data
        d.lu_adjustable = int(adjustable)
        self._desc = d
        self.lu = lu

    def updatedt(self, dt):
        self.dt = float(dt)

    def dostep(self, Q, nsteps=1, dt=None):
        self._desc.fast_dt = float(self.fastsolver.dt)
        lu = self.lu.handle if self.lu is not None else None
        gmres = isinstance(self.lu, GmresSolver)
        entry = self.dg.L.cmdg_mrigark_step_gmres if gmres else self.dg.L.cmdg_mrigark_step

        def step(t, dt):
            rc = entry(
                self._slow[0], self._slow[1], self._fast[0], self._fast[1], lu, C.byref(self._desc),
                Q.data_ptr(), C.cast(self._work, C.c_void_p), t, dt)
            if rc == 0:
                # the fast solver's clock ends at the last stage's end (updatetime! in solve!)
                for c in self.dc:
                    t += c * dt
                self.fastsolver.t = t
            return rc
        _run(self, nsteps, self.dt if dt is None else dt, step)
        if gmres:
            self.lu.alpha = (self.dt if dt is None else dt) * self.Gammas[0][2 * len(self.dc) - 1][len(self.dc)]
            self.solve_info = self.lu.step_info()

    def close(self):
        if self.lu is not None:
            self.lu.close()


class MRIGARKExplicit(_MRIGARK):
    """``MRIGARKExplicit(slowrhs!, fastsolver, Γs, γ̂s, Q, dt, t0)``
    (MultirateInfinitesimalGARKExplicit.jl:100-160): ``slow_rhs`` is a DGModel or a
    ``remainder_DGModel``, ``fastsolver`` an LSRK 2N solver whose operator is either as well.  One
    step is one ``cmdg_mrigark_step``.  ``γ̂s`` (the embedded scheme) is carried, not used."""

    KIND = 0

    def __init__(self, slow_rhs, fastsolver, Gammas, gammahats, Q, dt, t0=0.0):
        _fast_solver(fastsolver, "MRIGARKExplicit")
        G, gh, dc = mrigark_explicit_coefficients(Gammas, gammahats)
        self._setup(slow_rhs, fastsolver, G, gh, dc, Q, dt, t0)


class MRIGARKDecoupledImplicit(_MRIGARK):
    """``MRIGARKDecoupledImplicit(slowrhs!, backward_euler_solver, fastsolver, Γs, γ̂s, Q, dt, t0)``
    (MultirateInfinitesimalGARKDecoupledImplicit.jl:60-200): the slow operator is the linear
    model itself (not a remainder), solved by ``LinearBackwardEulerSolver(ManyColumnLU())``
    (vertical, stacked grid; factored for ``dt Γ_0[2, 2]``) or by
    ``LinearBackwardEulerSolver(GeneralizedMinimalResidual(...))`` (any direction, any grid;
    ``solve_info`` then holds the ``GmresInfo`` of the last step's solves).  ``updatedt`` with
    another alpha is refused when the solver is not adjustable."""

    KIND = 1

    def __init__(self, slow_rhs, backward_euler_solver, fastsolver, Gammas, gammahats, Q, dt, t0=0.0):
        from .dgmodel import RemainderDGModel
        _fast_solver(fastsolver, "MRIGARKDecoupledImplicit")
        if not isinstance(backward_euler_solver, LinearBackwardEulerSolver):
            raise TypeError("MRIGARKDecoupledImplicit: a LinearBackwardEulerSolver(ManyColumnLU() or "
                            "GeneralizedMinimalResidual()) is needed")
        if isinstance(slow_rhs, RemainderDGModel):
            raise TypeError("MRIGARKDecoupledImplicit: the implicit slow operator must be the vertical "
                            "linear model itself, not a remainder")
        G, gh, dc = mrigark_implicit_coefficients(Gammas, gammahats)
        self.isadjustable = backward_euler_solver.isadjustable
        lu = backward_euler_solver.setup(slow_rhs, float(dt) * G[0][1][1])
        self.solve_info = []
        self._setup(slow_rhs, fastsolver, G, gh, dc, Q, dt, t0, lu=lu, adjustable=self.isadjustable)

    def updatedt(self, dt):
        """``updatedt!``: ``@assert Δt_is_adjustable``; the next stage refactors for ``dt Γ_0[2, 2]``."""
        alpha = float(dt) * self.Gammas[0][1][1]
        if not self.isadjustable and alpha != self.lu.alpha:
            _refuse_alpha(self.lu, alpha)
        self.dt = float(dt)

    def dostep(self, Q, nsteps=1, dt=None):
        d = self.dt if dt is None else dt
        if not self.isadjustable:
            for s in range(len(self.dc)):
                alpha = d * self.Gammas[0][2 * s + 1][s + 1]
                if alpha != self.lu.alpha:
                    _refuse_alpha(self.lu, alpha)
        super().dostep(Q, nsteps, dt)


def _mri_explicit_factory(name):
    def make(slow_rhs, fastsolver, Q, dt=None, t0=0.0, **kw):
        assert dt is not None
        Gs, ghs = MRIGARK_TABLEAUS[name][1](**kw)
        return MRIGARKExplicit(slow_rhs, fastsolver, Gs, ghs, Q, dt, t0)
    make.__name__ = name
    return make


def _mri_implicit_factory(name):
    def make(slow_rhs, backward_euler_solver, fastsolver, Q, dt=None, t0=0.0, **kw):
        assert dt is not None
        Gs, ghs = MRIGARK_TABLEAUS[name][1](**kw)
        return MRIGARKDecoupledImplicit(slow_rhs, backward_euler_solver, fastsolver, Gs, ghs, Q, dt, t0)
    make.__name__ = name
    return make


# MRIGARKERK33aSandu(slow, fast, Q; dt, t0, delta = -1/2) and the others, as the reference names them
MRIGARKERK33aSandu = _mri_explicit_factory("MRIGARKERK33aSandu")
MRIGARKERK45aSandu = _mri_explicit_factory("MRIGARKERK45aSandu")
MRIGARKIRK21aSandu = _mri_implicit_factory("MRIGARKIRK21aSandu")
MRIGARKESDIRK23LSA = _mri_implicit_factory("MRIGARKESDIRK23LSA")
MRIGARKESDIRK24LSA = _mri_implicit_factory("MRIGARKESDIRK24LSA")
MRIGARKESDIRK34aSandu = _mri_implicit_factory("MRIGARKESDIRK34aSandu")
MRIGARKESDIRK46aSandu = _mri_implicit_factory("MRIGARKESDIRK46aSandu")

def solve(Q, solver, timeend=None, numberofsteps=0, adjustfinalstep=True, callbacks=()):
    """``solve!(Q, solver; timeend, adjustfinalstep, numberofsteps, callbacks)``: steps are issued
    one library call each, the last (shortened) step like ``general_dostep!`` does.
    ``callbacks``: ``(every_n_steps, callback)`` pairs, as ``EveryXSimulationSteps`` wraps them
    (GenericCallbacks.jl:205-229): ``callback.init(solver, Q, t)`` (if it has one) before the
    first step, then ``callback(solver, Q, t)`` after every ``every_n_steps``-th step; a return
    value > 0 stops the run (ODESolvers.jl:126-150)."""
    assert timeend is not None or numberofsteps > 0
    dt = solver.dt
    assert dt > 0
    cbs = [[int(n), cb, 0] for n, cb in callbacks]
    for c in cbs:
        if hasattr(c[1], "init"):
            c[1].init(solver, Q, solver.t)
    step = 0
    while (timeend is None or solver.t < timeend):
        if timeend is not None and adjustfinalstep and solver.t + dt > timeend:
            solver.dostep(Q, 1, dt=timeend - solver.t)
            solver.t = timeend
        else:
            solver.dostep(Q, 1)
        step += 1
        stop = False
        if cbs:
            # a callback reads or writes Q: the step (enqueued without a host wait) finishes first
            solver.dg.synchronize()
        for c in cbs:
            c[2] += 1
            if c[2] >= c[0]:
                c[2] = 0
                val = c[1](solver, Q, solver.t)
                stop = stop or (val is not None and val > 0)
        if stop or step == numberofsteps:
            break
    solver.dg.synchronize()
    return solver.t

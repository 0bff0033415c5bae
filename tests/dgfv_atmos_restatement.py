"""A NumPy restatement of the DGFVModel operator for the dry AtmosModel (test infrastructure).

Written from the reference: the law hooks of ``src/Atmos/Model/prog_prim_conversion.jl:67-78,
114-131, 187-202`` (DryModel), ``HBFVReconstruction`` of ``src/Atmos/Model/reconstructions.jl:15-73``,
the sources ``Gravity`` / ``Coriolis`` of ``tendencies_momentum.jl``, the default ``AtmosBC``
(``Impenetrable(FreeSlip)``, ``Insulating``; ``bc_momentum.jl:25-52``), ``fvm_balance!`` with
``fvm_balance_init!`` (``DGFVModel_kernels.jl:1079-1149``, ``ref_state.jl:265-285``) and
``vert_fvm_auxiliary_field_gradient!`` (``DGFVModel_kernels.jl:946-1063``), under the serial walk of
``vert_fvm_interface_tendency!`` (:47-739).  The walk's launch order, stencil widths and the
inner reconstructions are those of ``tests/dgfv_restatement.py``; the law's numerical fluxes are
those of ``tests/atmos_nf_restatement.py``; the horizontal DG terms are the oracle's kernels at
``Nq_v = 1``.  Nothing here comes from the product's kernels or from its host module.

Scope: ``ConstantDynamicViscosity(0)`` as in every use the reference makes of a DGFVModel on an
atmosphere -- the second-order fluxes then multiply the gradient-flux state by zero, and the
vertical gradient kernel's output is not formed here.
"""
import numpy as np

import atmos_nf_restatement as NF
import dgfv_restatement as R
from oracle import oracle as O

EVERY, HORIZONTAL, VERTICAL = R.EVERY, R.HORIZONTAL, R.VERTICAL
_JcV = 15
_xi3 = (2, 5, 8)              # xi3x1, xi3x2, xi3x3 of vgeo
RHO, P = 0, 4                 # primitives rho, u (3), p


# ---- the law hooks ---------------------------------------------------------------------------
class DryLaw:
    """Constants and switches of the model, and the pointwise functions the two kernels call."""

    def __init__(self, law, nf_first):
        ps = law.ps
        self.R_d, self.cv_d, self.cp_d, self.T_0 = float(ps.R_d), float(ps.cv_d), float(ps.cp_d), float(ps.T_0)
        self.grav, self.Omega = float(ps.grav), float(ps.Omega)
        self.sw = NF.Switches.of(law)
        self.orient = law.orientation != 0
        self.off_phi, self.off_ref = law.off_phi, law.off_ref
        self.subtract = bool(law.subtract_off) and law.ref_state is not None
        self.sources = int(law.sources)
        self.bcs = tuple(law.boundary_conditions)
        self.nf = nf_first
        assert law.viscosity == 0.0 and law.tau_hyper is None and law.C_smag is None

    def phi(self, aux):
        return aux[:, self.off_phi, :] if self.orient else 0.0

    def prognostic_to_primitive(self, Q, aux):
        rho = Q[:, 0, :]
        u = Q[:, 1:4, :] / rho[:, None, :]
        e_int = Q[:, 4, :] / rho - (u * u).sum(axis=1) / 2 - self.phi(aux)
        T = self.T_0 + e_int / self.cv_d
        prim = np.empty_like(Q)
        prim[:, 0, :], prim[:, 1:4, :], prim[:, 4, :] = rho, u, rho * self.R_d * T
        return prim

    def primitive_to_prognostic(self, prim, aux):
        rho, u, p = prim[:, 0, :], prim[:, 1:4, :], prim[:, 4, :]
        T = p / (rho * self.R_d)
        e_tot = self.cv_d * (T - self.T_0) + (u * u).sum(axis=1) / 2 + self.phi(aux)
        Q = np.empty_like(prim)
        Q[:, 0, :], Q[:, 1:4, :], Q[:, 4, :] = rho, rho[:, None, :] * u, rho * e_tot
        return Q

    def face_auxiliary_state(self, aux, dz):
        out = aux.copy()
        if self.orient:
            out[:, self.off_phi, :] = aux[:, self.off_phi, :] + self.grav * dz / 2
        return out

    def source(self, Q, aux):
        S = np.zeros_like(Q)
        if self.orient and self.sources & 1:                      # Gravity
            r = Q[:, 0, :] - (aux[:, self.off_ref, :] if self.subtract else 0.0)
            S[:, 1:4, :] -= r[:, None, :] * aux[:, self.off_phi + 1:self.off_phi + 4, :]
        if self.sources & 2:                                      # Coriolis: -2 Omega x rho u
            S[:, 1, :] += 2 * self.Omega * Q[:, 2, :]
            S[:, 2, :] -= 2 * self.Omega * Q[:, 1, :]
        assert not self.sources & ~3
        return S

    # (n, Q, aux) arrive as (nh, 3 | 5 | naux, Np); the flux restatement wants (k, columns)
    @staticmethod
    def _flat(a):
        return np.moveaxis(a, 1, 2).reshape(-1, a.shape[1])

    def numerical_flux(self, n, QM, auxM, QP, auxP):
        nn, qm, am, qp, ap = (self._flat(a) for a in (n, QM, auxM, QP, auxP))
        if self.nf >= NF.ROE:
            F, _ = NF.numerical_flux(self.nf, self.sw, nn, qm, am, qp, ap)
        else:
            FM, FP = NF.physical_normal_flux(self.sw, nn, qm, am), NF.physical_normal_flux(self.sw, nn, qp, ap)
            F = (FM + FP) / 2
            if self.nf == 0:                                      # Rusanov: |u . n| + c of either side
                lam = np.maximum(self._wavespeed(nn, qm, am), self._wavespeed(nn, qp, ap))
                F = F + lam[:, None] * (qm - qp) / 2
        return np.moveaxis(F.reshape(QM.shape[0], QM.shape[2], 5), 2, 1)

    def _wavespeed(self, n, Q, aux):
        u = Q[:, 1:4] / Q[:, :1]
        phi = aux[:, self.off_phi] if self.orient else 0.0
        T = self.T_0 + (Q[:, 4] / Q[:, 0] - (u * u).sum(axis=1) / 2 - phi) / self.cv_d
        return np.abs((u * n).sum(axis=1)) + np.sqrt(self.cp_d / self.cv_d * self.R_d * T)

    def boundary_flux(self, tag, n, QM, auxM):
        """numerical_boundary_flux_first_order! against the wall's ghost: the mirrored momentum."""
        assert all(self.bcs[int(b) - 1] == 1 for b in np.unique(tag))
        QP = QM.copy()
        dn = (QM[:, 1:4, :] * n).sum(axis=1)
        QP[:, 1:4, :] = QM[:, 1:4, :] - 2 * dn[:, None, :] * n
        return self.numerical_flux(n, QM, auxM, QP, auxM)


# ---- HBFVReconstruction around a Recon of dgfv_restatement -----------------------------------------
class HBRecon:
    def __init__(self, inner, grav):
        self.inner, self.grav = inner, float(grav)
        self.linear, self.width, self.limiter = inner.linear, inner.width, inner.limiter

    def __call__(self, states, weights):
        """``states``: 2 w + 1 primitive arrays (nh, 5, Np); ``weights``: as many (nh, 1, Np)."""
        D = len(states)
        W = (D - 1) // 2
        cells = [s.copy() for s in states]
        half = [cells[i][:, RHO, :] * self.grav * weights[i][:, 0, :] / 2 for i in range(D)]
        p_ref = states[W][:, P, :].copy()
        cells[W][:, P, :] -= p_ref
        lo, hi = p_ref.copy(), p_ref.copy()
        for i in range(1, W + 1):
            lo = lo + (half[W - i + 1] + half[W - i])
            cells[W - i][:, P, :] -= lo
            hi = hi - (half[W + i - 1] + half[W + i])
            cells[W + i][:, P, :] -= hi
        bot, top = self.inner(cells, weights)
        bot[:, P, :] += p_ref + half[W]
        top[:, P, :] += p_ref - half[W]
        return bot, top


# ---- one-time host set-up of a finite-volume vertical ------------------------------------------------
def _stacked(grid, a):
    nv = int(grid.topology.stacksize)
    return a.reshape((a.shape[0] // nv, nv) + a.shape[1:])


def fv_field_gradient(grid, a):
    """vert_fvm_auxiliary_field_gradient! of a nodal field (nelem, Np): (nelem, 3, Np)."""
    nv, periodic = int(grid.topology.stacksize), bool(grid.topology.periodicstack)
    out = np.zeros((a.shape[0], 3, a.shape[1]))
    s, h = _stacked(grid, a), _stacked(grid, grid.vgeo[:, _JcV, :])
    g = np.zeros_like(s)
    for k in range(nv):
        dn, up = (k - 1) % nv, (k + 1) % nv
        a_dn, a_up, h_dn, h_up = s[:, dn], s[:, up], h[:, dn], h[:, up]
        if not periodic and k == 0:
            a_dn, h_dn = 2 * s[:, k] - a_up, h_up
        if not periodic and k == nv - 1:
            a_up, h_up = 2 * s[:, k] - a_dn, h_dn
        g[:, k] = (a_up - a_dn) / (h_up + 2 * h[:, k] + h_dn)
    g = g.reshape(a.shape)
    for d in range(3):
        out[:, d, :] = grid.vgeo[:, _xi3[d], :] * grid.vgeo[:, _JcV, :] * g
    return out


def fvm_balance(grid, rho, p, R_d, grav):
    """kernel_fvm_balance! with fvm_balance_init!, one walk up every stack; returns (rho, p)."""
    nv = int(grid.topology.stacksize)
    rho, p = _stacked(grid, rho.copy()), _stacked(grid, p.copy())
    dz = 2 * _stacked(grid, grid.vgeo[:, _JcV, :])
    for k in range(1, nv):
        Tv_below = p[:, k - 1] / (R_d * rho[:, k - 1])
        Tv = p[:, k] / (R_d * rho[:, k])
        rho[:, k] = rho[:, k - 1] * (R_d * Tv_below - grav * dz[:, k - 1] / 2) / (R_d * Tv + grav * dz[:, k] / 2)
        p[:, k] = R_d * rho[:, k] * Tv
    shape = (rho.shape[0] * nv,) + rho.shape[2:]
    return rho.reshape(shape), p.reshape(shape)


# ---- the operator ----------------------------------------------------------------------------------
class DGFVAtmosRestatement(R.DGFVRestatement):
    """``DGFVModel(atmos, grid, recon, nf_first, central, central; direction)`` on the host; ``recon``
    a ``dgfv_restatement.Recon`` or an ``HBRecon`` around one."""

    def __init__(self, law, grid, recon, nf_first=0, direction=EVERY, exchange=None):
        assert grid.N[2] == 0 and law.ns == 5
        self.law, self.grid, self.recon, self.direction = law, grid, recon, direction
        self.dg = O.OracleDGModel(law, grid, nf_first=nf_first, direction=direction, exchange=exchange)
        self.state_auxiliary = self.dg.state_auxiliary
        self.nv = int(grid.topology.stacksize)
        self.periodic = bool(grid.topology.periodicstack)
        self.L = DryLaw(law, nf_first)
        self.exchange = self.dg.exchange
        self.numpy_faces = False

    def fv_gradients(self, Q, t, elems, increment):
        return                                              # (zero viscosity: see the module text)

    def fv_tendency(self, tendency, Q, t, alpha, beta, elems, increment, add_source):
        if len(elems) == 0:
            return
        g, nv, L = self.grid, self.nv, self.L
        idx = self._stacks(Q, elems)
        aux = self.state_auxiliary
        q = lambda k: Q[idx[:, k]]
        ax = lambda k: aux[idx[:, k]]
        w = lambda k: 2 * g.vgeo[idx[:, k], _JcV, :][:, None, :]
        prim = [L.prognostic_to_primitive(q(k), ax(k)) for k in range(nv)]

        def faces(k):
            """Prognostic face states and face auxiliary states (bottom, top) of cell k."""
            hw = self._half_width(k + 1)
            rng = [(k + j) % nv for j in range(-hw, hw + 1)]
            bot, top = self.recon([prim[j] for j in rng], [w(j) for j in rng])
            a_bot = L.face_auxiliary_state(ax(k), -w(k)[:, 0, :])
            a_top = L.face_auxiliary_state(ax(k), w(k)[:, 0, :])
            return (L.primitive_to_prognostic(bot, a_bot), a_bot), (L.primitive_to_prognostic(top, a_top), a_top)

        def sgeo(f, k):
            s = g.sgeo[idx[:, k], f, :g.Np, :]
            n = np.stack([s[..., 0], s[..., 1], s[..., 2]], axis=1)
            return n, s[..., 3][:, None, :], s[..., 4][:, None, :]

        def write(k, lt):
            T = tendency[idx[:, k]]
            if increment:
                tendency[idx[:, k]] = T + lt
            else:
                tendency[idx[:, k]] = (lt + beta * T) if beta != 0 else lt

        source = lambda k: L.source(q(k), ax(k)) if add_source else 0.0
        if self.periodic:
            eV = nv - 1
            (_, _), prev_top = faces(eV)
            local = -0.0 * q(eV)
            vMI2 = sgeo(5, eV)[2]
            start = 0
        else:
            eV = 0
            (Qb, ab), prev_top = faces(eV)
            n, sM, vMI2 = sgeo(4, eV)
            flux = L.boundary_flux(g.elemtobndy[idx[:, eV], 4], n, Qb, ab)
            local = -alpha * sM * vMI2 * flux
            start = 1
        for up in range(start, nv):
            dn = (up - 1) % nv
            vMI1 = vMI2
            n, sM, _ = sgeo(4, up)
            vMI2 = sgeo(5, up)[2]
            (Qb, ab), (Qt, at) = faces(up)
            flux = L.numerical_flux(n, Qb, ab, prev_top[0], prev_top[1])
            local = local + source(dn)
            local = local + alpha * sM * vMI1 * flux
            write(dn, local)
            local = -alpha * sM * vMI2 * flux
            if up == nv - 1:
                local = local + source(up)
                if self.periodic:
                    tendency[idx[:, up]] = tendency[idx[:, up]] + local
                else:
                    n, sM, _ = sgeo(5, up)
                    flux = L.boundary_flux(g.elemtobndy[idx[:, up], 5], n, Qt, at)
                    local = local - alpha * sM * vMI2 * flux
                    write(up, local)
            prev_top = (Qt, at)

"""A NumPy restatement of the DGFVModel operator for the single-equation AdvectionDiffusion law:
the two vertical finite-volume kernels (``vert_fvm_interface_tendency!`` and
``vert_fvm_interface_gradients!``, src/Numerics/DGMethods/DGFVModel_kernels.jl:47-739, :741-944)
in the reference's serial order -- one walk up each stack, vectorised over the stacks and the
horizontal nodes only -- and the launch order of ``(dgfvm::DGFVModel)(tendency, Q, _, t, alpha,
beta)`` (DGFVModel.jl:85-320, SpaceDiscretization.jl:502-1368).  The horizontal DG terms are the
oracle's kernels, called with the horizontal direction at ``Nq_v = 1``.  Nothing here comes from
the product's kernels.  Shared by tests/test_dgfv_host.py and tests/test_gpu_dgfv.py."""
import ctypes as C

import numpy as np

from oracle import oracle as O

EVERY, HORIZONTAL, VERTICAL = 0, 1, 2
_n1, _n2, _n3, _sM, _vMI = range(5)
_M, _JcV = 9, 15


# ---- FVReconstructions.jl -------------------------------------------------------------------
def van_leer(d_top, d_bot):
    same = d_top * d_bot > 0
    den = np.where(same, d_top + d_bot, 1.0)
    return np.where(same, 2 * d_top * d_bot / den, 0.0)


def no_limiter(d_top, d_bot):
    return (d_top + d_bot) / 2


class Recon:
    """``FVConstant()`` (``linear = False``) or ``FVLinear{width}(limiter)``."""

    def __init__(self, linear, width=None, limiter=van_leer):
        self.linear = bool(linear)
        self.width = (1 if width is None else width) if linear else 0
        self.limiter = limiter

    def __call__(self, states, weights):
        """``states``, ``weights``: lists of 2 w + 1 arrays; returns (bot, top)."""
        D = len(states)
        if not self.linear or D == 1:
            assert D == 1
            return states[0].copy(), states[0].copy()
        if D > 3:                                   # FVReconstructions.jl:134-143
            W = (D - 1) // 2
            states, weights = states[W - 1:W + 2], weights[W - 1:W + 2]
        wi_top = 1 / (weights[2] + weights[1])
        wi_bot = 1 / (weights[1] + weights[0])
        d_top = wi_top * (states[2] - states[1])
        d_bot = wi_bot * (states[1] - states[0])
        d = self.limiter(d_top, d_bot)
        return states[1] - d * weights[1], states[1] + d * weights[1]


# ---- the single-equation AdvectionDiffusion law (advection_diffusion_model.jl) -----------------
class _Law:
    def __init__(self, law, nf_first):
        self.law, self.nf = law, nf_first
        self.adv, self.diff = law.advection, law.diffusion
        self.ou, self.od = law.off_u, law.off_D
        ip, _ = law.descriptor()
        self.flux_bc = bool(ip[4])
        self.bc = [int(v) for v in ip[7:14]]
        self.p = law.problem

    def rho_exact(self, aux, t):
        return self.p.initial_condition([aux[:, 0], aux[:, 1], aux[:, 2]], t)

    def grad_exact(self, aux, t):
        p = self.p                                   # Pseudo1D inhomogeneous_data!(Val(1))
        xn = p.n[0] * aux[:, 0] + p.n[1] * aux[:, 1] + p.n[2] * aux[:, 2]
        a = xn - p.mu - p.alpha * t
        g = (2 * a / (4 * p.beta * (p.delta + t)) * np.exp(-(a * a) / (4 * p.beta * (p.delta + t)))
             / np.sqrt(1 + t / p.delta))
        return [-(p.n[i] * g) for i in range(3)]

    def flux1(self, Q, aux):
        if not self.adv:
            return [np.zeros_like(Q)] * 3
        return [aux[:, self.ou + d] * Q for d in range(3)]

    def wavespeed(self, n, aux):
        if not self.adv:
            return 0.0 * n[0]
        return np.abs(n[0] * aux[:, self.ou] + n[1] * aux[:, self.ou + 1] + n[2] * aux[:, self.ou + 2])

    def nf_first_order(self, n, QM, auxM, QP, auxP):
        """numerical_flux_first_order! (NumericalFluxes.jl:223-285 Rusanov, :300-340 central)."""
        FM, FP = self.flux1(QM, auxM), self.flux1(QP, auxP)
        flux = (FM[0] + FP[0]) * (n[0] / 2) + (FM[1] + FP[1]) * (n[1] / 2) + (FM[2] + FP[2]) * (n[2] / 2)
        if self.nf == 0:
            mw = np.maximum(self.wavespeed(n, auxM), self.wavespeed(n, auxP))
            flux = flux + (mw * (QM - QP)) / 2
        return flux

    def boundary_state(self, tag, QM, auxM, t):
        """boundary_state! for the first-order and the gradient numerical fluxes (:402-428)."""
        QP = QM.copy()
        for b in np.unique(tag):
            m = tag == b
            bc = self.bc[b - 1]
            if bc & 1:
                QP[m] = self.rho_exact(auxM, t)[m]
            elif bc & (2 | 32):
                QP[m] = QM[m]
            elif bc & 16:
                QP[m] = 0.0
        return QP

    def flux2(self, gf):
        if not self.diff:
            return [0.0 * gf[:, 0]] * 3 if gf.shape[1] else [0.0] * 3
        return [-gf[:, d] for d in range(3)]

    def matvecD(self, aux, g):
        D = aux[:, self.od:self.od + 9]
        return [D[:, i] * g[0] + D[:, i + 3] * g[1] + D[:, i + 6] * g[2] for i in range(3)]

    def boundary_flux2(self, tag, n, gfM, auxM, t):
        """normal_boundary_flux_second_order! (NumericalFluxes.jl:872-967, law methods :430-567)."""
        if not self.diff:
            return 0.0 * n[0]
        out = 0.0 * n[0]
        for b in np.unique(tag):
            m = tag == b
            bc = self.bc[b - 1]
            if self.flux_bc:
                if bc & (1 | 16):
                    F = [-gfM[:, d] for d in range(3)]
                elif bc & 2:
                    g = self.grad_exact(auxM, t)
                    D = auxM[:, self.od:self.od + 9]
                    F = [-D[:, i] * g[0] + -D[:, i + 3] * g[1] + -D[:, i + 6] * g[2] for i in range(3)]
                else:
                    F = [0.0 * n[0]] * 3
            else:
                if bc & (1 | 16):
                    gfP = [gfM[:, d] for d in range(3)]
                elif bc & 2:
                    gfP = self.matvecD(auxM, self.grad_exact(auxM, t))
                elif bc & 32:
                    z = 0.0 * n[0]
                    gfP = self.matvecD(auxM, [z, z, z])
                else:
                    gfP = [gfM[:, d] for d in range(3)]
                F = [-gfP[d] for d in range(3)]
            val = F[0] * n[0] + F[1] * n[1] + F[2] * n[2]
            out = np.where(m, val, out)
        return out


class DGFVRestatement:
    """``DGFVModel(law, grid, recon, nf_first, central, central; direction)`` on the host."""

    def __init__(self, law, grid, recon, nf_first=0, direction=EVERY, exchange=None):
        assert grid.N[2] == 0 and law.ns == 1
        self.law, self.grid, self.recon, self.direction = law, grid, recon, direction
        self.dg = O.OracleDGModel(law, grid, nf_first=nf_first, direction=direction, exchange=exchange)
        self.state_auxiliary = self.dg.state_auxiliary
        self.nv = int(grid.topology.stacksize)
        self.periodic = bool(grid.topology.periodicstack)
        self.L = _Law(law, nf_first)
        self.exchange = self.dg.exchange
        # boundary data of a problem the oracle's C law does not carry (fvm_advection.jl's sine wave):
        # the horizontal interface kernel is then restated here as well
        self.numpy_faces = getattr(law.problem, "problem_id", 0) == 8

    @property
    def state_gradient_flux(self):
        return self.dg.state_gradient_flux

    # -- helpers: views of the real elements as (stacks, levels, columns, nodes) -----------------
    def _stacks(self, A, elems):
        """Rows of ``A`` for the stacks that ``elems`` (1-based, whole stacks) lists."""
        nv = self.nv
        bottoms = np.asarray(elems[::nv], dtype=np.int64) - 1
        idx = bottoms[:, None] + np.arange(nv)[None, :]
        return idx

    def _half_width(self, eV):
        """Half-width of the stencil of cell eV (1-based), :475-516 and :304-311."""
        W, n = self.recon.width, self.nv
        if self.periodic or W == 0:
            return W
        if eV == 1:
            return 0
        if W < eV < n - W + 1:
            return W
        if eV <= W:
            return eV - 1
        return n - eV

    # -- dgsem_interface_tendency! with HorizontalDirection (DGModel_kernels.jl:588-901) -----------
    def horizontal_interface_tendency(self, tendency, Q, t, alpha, elems):
        """Faces 1-4 in order, every face node of the listed elements; single rank, no second-order
        terms (the advection-only law of fvm_advection.jl)."""
        g, L = self.grid, self.L
        assert not L.diff and g.nelem == g.nreal
        e = np.asarray(elems, dtype=np.int64) - 1
        if len(e) == 0:
            return
        Np, nfp = g.Np, g.Nfp[0]
        aux = self.state_auxiliary
        Qf = Q[:, 0, :].reshape(-1)
        auxn = np.moveaxis(aux, 1, 2).reshape(-1, aux.shape[1])      # (nelem * Np, naux)
        for f in range(4):
            idM = g.vmapM[e, f, :nfp] - 1
            tag = np.broadcast_to(g.elemtobndy[e, f][:, None], idM.shape)
            idP = np.where(tag != 0, idM, g.vmapP[e, f, :nfp] - 1)
            s = g.sgeo[e, f, :nfp, :]
            n, sM, vMI = [s[..., _n1], s[..., _n2], s[..., _n3]], s[..., _sM], s[..., _vMI]
            QM, QP = Qf[idM], Qf[idP]
            aM, aP = _Cols(np.moveaxis(auxn[idM], 2, 1)), _Cols(np.moveaxis(auxn[idP], 2, 1))
            if (tag != 0).any():
                QP = np.where(tag != 0, L.boundary_state(np.where(tag == 0, 1, tag), QM, aM, t), QP)
            flux = L.nf_first_order(n, QM, aM, QP, aP)
            T = tendency[:, 0, :].reshape(-1)
            T[idM] = T[idM] - alpha * vMI * sM * flux
            tendency[:, 0, :] = T.reshape(tendency.shape[0], Np)

    # -- vert_fvm_interface_tendency! -----------------------------------------------------------
    def fv_tendency(self, tendency, Q, t, alpha, beta, elems, increment, add_source):
        if len(elems) == 0:
            return
        g, nv, L = self.grid, self.nv, self.L
        idx = self._stacks(Q, elems)                       # (nh, nv) element ids
        aux, gf = self.state_auxiliary, self.dg.state_gradient_flux
        q = lambda k: Q[idx[:, k], 0, :]
        ax = lambda k: np.moveaxis(aux[idx[:, k]], 1, 0)   # (naux, nh, Np) -> index [:, c] below
        axc = lambda k: _Cols(aux[idx[:, k]])
        gfc = lambda k: _Cols(gf[idx[:, k]]) if gf.shape[1] else _Cols(np.zeros((idx.shape[0], 0, g.Np)))
        w = lambda k: 2 * g.vgeo[idx[:, k], _JcV, :]
        mod = lambda k: k % nv

        def recon(k):                                      # cell k, 0-based
            hw = self._half_width(k + 1)
            rng = [mod(k + j) for j in range(-hw, hw + 1)]
            return self.recon([q(j) for j in rng], [w(j) for j in rng])

        def sgeo(f, k):
            s = g.sgeo[idx[:, k], f, :g.Np, :]
            return [s[..., _n1], s[..., _n2], s[..., _n3]], s[..., _sM], s[..., _vMI]

        def tag(f, k):
            return np.broadcast_to(g.elemtobndy[idx[:, k], f][:, None], (idx.shape[0], g.Np))

        def write(k, lt):
            T = tendency[idx[:, k], 0, :]
            if increment:
                tendency[idx[:, k], 0, :] = T + lt
            else:
                tendency[idx[:, k], 0, :] = (lt + beta * T) if beta != 0 else lt

        # no source term in this law (source! is empty): add_source changes nothing
        if self.periodic:
            eV = nv - 1
            bot, top = recon(eV)
            local = -0.0 * bot
            vMI2 = sgeo(5, eV)[2]
            face_top_prev, aux_prev = top, axc(eV)
            start = 0
        else:
            eV = 0
            bot, top = recon(eV)
            n, sM, vMI2 = sgeo(4, eV)
            a0 = axc(eV)
            QP = L.boundary_state(tag(4, eV), bot, a0, t)
            flux = L.nf_first_order(n, bot, a0, QP, a0)
            flux = flux + L.boundary_flux2(tag(4, eV), n, gfc(eV), a0, t)
            local = -alpha * sM * vMI2 * flux
            face_top_prev, aux_prev = top, a0
            start = 1
        for up in range(start, nv):
            dn = mod(up - 1)
            vMI1 = vMI2
            n, sM, _ = sgeo(4, up)
            vMI2 = sgeo(5, up)[2]
            bot, top = recon(up)
            aU, aD = axc(up), aux_prev
            flux = L.nf_first_order(n, bot, aU, face_top_prev, aD)
            if L.diff:
                FM, FP = L.flux2(gfc(up)), L.flux2(gfc(dn))
                flux = flux + ((FM[0] + FP[0]) * (n[0] / 2) + (FM[1] + FP[1]) * (n[1] / 2)
                               + (FM[2] + FP[2]) * (n[2] / 2))
            local = local + alpha * sM * vMI1 * flux
            write(dn, local)
            local = -alpha * sM * vMI2 * flux
            if up == nv - 1:
                if self.periodic:
                    tendency[idx[:, up], 0, :] = tendency[idx[:, up], 0, :] + local
                else:
                    n, sM, _ = sgeo(5, up)
                    QP = L.boundary_state(tag(5, up), top, aU, t)
                    flux = L.nf_first_order(n, top, aU, QP, aU)
                    flux = flux + L.boundary_flux2(tag(5, up), n, gfc(up), aU, t)
                    local = local - alpha * sM * vMI2 * flux
                    write(up, local)
            face_top_prev, aux_prev = top, aU

    # -- vert_fvm_interface_gradients! ----------------------------------------------------------
    def fv_gradients(self, Q, t, elems, increment):
        if len(elems) == 0 or not self.L.diff:
            return
        g, nv, L = self.grid, self.nv, self.L
        aux, gf = self.state_auxiliary, self.dg.state_gradient_flux
        e = np.asarray(elems, dtype=np.int64) - 1
        eV = e % nv
        dn = np.where(eV > 0, e - 1, e + nv - 1 if self.periodic else e)
        up = np.where(eV < nv - 1, e + 1, e - nv + 1 if self.periodic else e)
        bc_dn = np.where((eV == 0) & (not self.periodic), g.elemtobndy[e, 4], 0)
        bc_up = np.where((eV == nv - 1) & (not self.periodic), g.elemtobndy[e, 5], 0)
        els = (dn, e, up)
        M = [g.vgeo[x, _M, :] for x in els]
        G = [Q[x, 0, :] for x in els]
        vMI = g.sgeo[e, 4, :g.Np, _vMI]
        nG = [-0.0 * G[1] for _ in range(3)]
        ac = _Cols(aux[e])
        for f, bc in ((0, bc_dn), (1, bc_up)):
            s = g.sgeo[e, 4 + f, :g.Np, :]
            n, sM = [s[..., _n1], s[..., _n2], s[..., _n3]], s[..., _sM]
            Gs = (M[f] * G[f + 1] + M[f + 1] * G[f]) / (M[f] + M[f + 1])
            tagf = np.broadcast_to(bc[:, None], G[1].shape)
            if (bc != 0).any():
                safe = np.where(tagf == 0, 1, tagf)
                GP = L.boundary_state(safe, G[1], ac, t)
            for i in range(3):
                interior = vMI * sM * n[i] * Gs
                if (bc != 0).any():
                    bnd = vMI * sM * (n[i] * GP)
                    nG[i] = nG[i] + np.where(tagf == 0, interior, bnd)
                else:
                    nG[i] = nG[i] + interior
        sig = L.matvecD(ac, nG)
        for d in range(3):
            gf[e, d, :] = gf[e, d, :] + sig[d] if increment else sig[d]

    # -- (dgfvm::DGFVModel)(tendency, Q, _, t, alpha, beta) --------------------------------------
    def __call__(self, tendency, Q, t, alpha=1.0, beta=0.0):
        dg, ph, ex, d = self.dg, self.dg.ph, self.exchange, self.direction
        og = dg.og
        communicate = not (self.grid.topology.isstacked and d == VERTICAL)
        every, horz, vert = d == EVERY, d in (EVERY, HORIZONTAL), d in (EVERY, VERTICAL)
        p = O._p
        a = (ph.c, C.byref(og.c))
        dg.update_auxiliary_state(Q, t, "real")
        tok_Q = tok_gf = None
        if communicate:
            tok_Q = ex.begin(Q, ph.ns)

        def interface_gradients(surface):
            el = og.interior if surface == "interior" else og.exterior
            if horz:
                dg.L.orc_interface_gradients(*a, HORIZONTAL, p(Q), p(dg.state_gradient_flux),
                                             p(dg.Qhypervisc_grad), p(dg.state_auxiliary), C.c_double(t),
                                             p(el), C.c_int64(len(el)))
            if vert:
                self.fv_gradients(Q, t, el, every)

        def interface_tendency(surface):
            el = og.interior if surface == "interior" else og.exterior
            if horz and self.numpy_faces:
                self.horizontal_interface_tendency(tendency, Q, t, alpha, el)
            elif horz:
                dg.L.orc_interface_tendency(*a, HORIZONTAL, p(tendency), p(Q), p(dg.state_gradient_flux),
                                            p(dg.Qhypervisc_grad), p(dg.state_auxiliary), C.c_double(t),
                                            p(el), C.c_int64(len(el)), C.c_double(alpha))
            if vert:
                self.fv_tendency(tendency, Q, t, alpha, beta, el, every, d == VERTICAL)

        if ph.ngf > 0:
            if horz:        # launch_volume_gradients!: the horizontal kernel only (:555)
                dg.L.orc_volume_gradients(*a, HORIZONTAL, p(Q), p(dg.state_gradient_flux),
                                          p(dg.Qhypervisc_grad), p(dg.state_auxiliary), C.c_double(t), 0)
            interface_gradients("interior")
            if communicate:
                ex.end(Q, ph.ns, tok_Q)
                dg.update_auxiliary_state(Q, t, "ghost")
            interface_gradients("exterior")
            if communicate:
                tok_gf = ex.begin(dg.state_gradient_flux, ph.ngf)
        if horz:            # launch_volume_tendency!: horizontal, sources added (:1152-1155)
            dg.L.orc_volume_tendency(*a, d, HORIZONTAL, p(tendency), p(Q), p(dg.state_gradient_flux),
                                     p(dg.Qhypervisc_grad), p(dg.state_auxiliary), C.c_double(t),
                                     C.c_double(alpha), C.c_double(beta), 1)
        interface_tendency("interior")
        if communicate:
            if ph.ngf > 0:
                ex.end(dg.state_gradient_flux, ph.ngf, tok_gf)
            else:
                ex.end(Q, ph.ns, tok_Q)
                dg.update_auxiliary_state(Q, t, "ghost")
        interface_tendency("exterior")


class _Cols:
    """``a[:, c]`` of an (n, ncol, Np) array."""

    def __init__(self, a):
        self.a = a
        self.shape = a.shape

    def __getitem__(self, key):
        rows, c = key
        return self.a[:, c, :]


def lsrk54_steps(dg, Q, dt, nsteps, t0=0.0):
    """``solve!`` with LSRK54CarpenterKennedy: ``nsteps`` steps of size ``dt``."""
    dQ = np.zeros_like(Q)
    t = t0
    for _ in range(nsteps):
        O.lsrk54_step(dg, Q, dQ, t, dt)
        t += dt
    return t

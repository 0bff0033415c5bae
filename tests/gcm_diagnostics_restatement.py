"""NumPy restatement of the reference's ``AtmosGCMDefault`` diagnostics group
(``src/Diagnostics/atmos_gcm_default.jl`` with ``vort`` and ``vort2``, ``diagnostic_fields.jl``,
``vorticity_balancelaw.jl``, ``thermo.jl:33-49``), operation for operation:

* ``vector_gradients_kernel!`` (:129-298): the quotients ``ρu / ρ``, every reference-space derivative
  as the sum, left to right in ascending node index, of the rounded products ``D[i, r] u[r]`` (the
  first product is the initial value), the metric combination left to right; ``vorticity_kernel!``
  (:382-396): the three differences;
* ``compute_thermo!`` of a dry model;
* the ``VorticityModel`` operator as ``DGModel`` evaluates it with central fluxes and ``beta = 0``:
  the weak-form volume term plus the face term ``vMI sM (F⁻ + F⁺)ᵀ n / 2``, boundary faces with plus
  = minus (``boundary_state!`` of ``nothing``);
* the composition of ``atmos_gcm_default_collect`` on top of tests/interpolation_restatement.py.

Arrays are ``(nelem, nvar, Np)``; ``Np`` runs with ``i`` fastest.  No device."""
from collections import OrderedDict

import numpy as np

import interpolation_restatement as IR
from cmdg_loader import cm

GR = cm.mesh.grids
NAMES = ["u", "v", "w", "rho", "temp", "pres", "thd", "et", "ei", "ht", "hi", "vort", "vort2"]
VGRAD = ["∂₁u₁", "∂₂u₁", "∂₃u₁", "∂₁u₂", "∂₂u₂", "∂₃u₂", "∂₁u₃", "∂₂u₃", "∂₃u₃"]
XI = ((GR._xi1x1, GR._xi1x2, GR._xi1x3), (GR._xi2x1, GR._xi2x2, GR._xi2x3), (GR._xi3x1, GR._xi3x2, GR._xi3x3))


def _nq(grid):
    return tuple(int(n) + 1 for n in grid.N)


def velocity(Q):
    """``u = ρu ./ ρ`` (atmos_gcm_default.jl:343-344; the kernel forms the same quotients): (n, 3, Np)."""
    return Q[:, 1:4] / Q[:, 0:1]


def _line_sum(D, u, axis):
    """``sum_r D[i, r] u[.., r, ..]`` along ``axis`` of ``u``, left to right over rounded products; the
    result's index ``i`` takes the place of ``r``."""
    u = np.moveaxis(u, axis, -1)                       # (..., r)
    acc = u[..., None, 0] * D[:, 0]                    # (..., i)
    for r in range(1, D.shape[1]):
        acc = acc + u[..., None, r] * D[:, r]
    return np.moveaxis(acc, -1, axis)


def vector_gradients(grid, Q):
    """``VectorGradients(dg, Q)``: ``(nreal, 9, Np)``, columns ``VGRAD``."""
    nr = grid.nreal
    q1, q2, q3 = _nq(grid)
    u = velocity(Q[:nr]).reshape(nr, 3, q3, q2, q1)
    vg = grid.vgeo[:nr]
    g = [_line_sum(np.asarray(grid.D[0]), u, 4).reshape(nr, 3, -1),
         _line_sum(np.asarray(grid.D[1]), u, 3).reshape(nr, 3, -1),
         _line_sum(np.asarray(grid.D[2]), u, 2).reshape(nr, 3, -1)]
    out = np.zeros((nr, 9, grid.Np))
    for c in range(3):
        for m in range(3):
            out[:, 3 * c + m] = g[0][:, c] * vg[:, XI[0][m]] + g[1][:, c] * vg[:, XI[1][m]] + g[2][:, c] * vg[:, XI[2][m]]
    return out


def vorticity(vgrad):
    """``Vorticity(dg, vgrad)``: ``(nreal, 3, Np)``."""
    return np.stack([vgrad[:, 7] - vgrad[:, 5], vgrad[:, 2] - vgrad[:, 6], vgrad[:, 3] - vgrad[:, 1]], axis=1)


def thermo(law, Q, aux):
    """``compute_thermo!`` of a ``DryModel`` (thermo.jl:33-44): temp, pres, θ_dry, e_int, h_tot, h_int."""
    ps = law.ps
    rho = Q[:, 0]
    rhoinv = 1 / rho
    e_tot = Q[:, 4] / rho
    rhoe_kin = rhoinv * (Q[:, 1] * Q[:, 1] + Q[:, 2] * Q[:, 2] + Q[:, 3] * Q[:, 3]) / 2
    rhoe_pot = rho * (aux[:, law.off_phi] if law.orientation != cm.atmos.ORIENT_NONE else -0.0)
    e_int = rhoinv * (Q[:, 4] - rhoe_kin - rhoe_pot)
    T = ps.T_0 + e_int / ps.cv_d
    p = ps.R_d * rho * T
    thd = T / (p / ps.MSLP) ** (ps.R_d / ps.cp_d)
    RT = ps.R_d * T
    return np.stack([T, p, thd, e_int, e_tot + RT, e_int + RT], axis=1)


def nodal(law, grid, Q, aux):
    """The packed nodal array ``G (nreal, 14, Np)``: ρ, ρu, ρv, ρw, ρe | thermo | Ω."""
    nr = grid.nreal
    return np.concatenate([Q[:nr, :5], thermo(law, Q[:nr], aux[:nr]), vorticity(vector_gradients(grid, Q))], axis=1)


def _face_sizes(grid):
    q1, q2, q3 = _nq(grid)
    return [q2 * q3, q2 * q3, q1 * q3, q1 * q3, q1 * q2, q1 * q2]


def vorticity_model_tendency(grid, u):
    """``vort_state.dg(dQ, state, nothing, 0)``: ``(nreal, 3, Np)`` from ``u (nelem, 3, Np)`` (ghost
    elements exchanged).  ``flux.Ω_bl`` is the matrix of vorticity_balancelaw.jl:76-80, row = direction."""
    nr, Np = grid.nreal, grid.Np
    q1, q2, q3 = _nq(grid)
    vg = grid.vgeo

    def flux(u1, u2, u3):
        z = np.zeros_like(u1)
        # F[d][c]
        return [[z, u3, -u2], [-u3, z, u1], [u2, -u1, z]]

    F = flux(u[:nr, 0], u[:nr, 1], u[:nr, 2])
    M, MI = vg[:nr, GR._M], vg[:nr, GR._MI]
    out = np.zeros((nr, 3, Np))
    D = [np.asarray(d) for d in grid.D]
    for c in range(3):
        acc = np.zeros((nr, q3, q2, q1))
        for a in range(3):
            Fa = M * (vg[:nr, XI[a][0]] * F[0][c] + vg[:nr, XI[a][1]] * F[1][c] + vg[:nr, XI[a][2]] * F[2][c])
            Fa = Fa.reshape(nr, q3, q2, q1)
            # sum_n D[n, i] Fa[n]: the transpose of the derivative along direction a
            acc = acc + np.moveaxis(np.tensordot(Fa, D[a], axes=([3 - a], [0])), -1, 3 - a)
        out[:, c] = MI * acc.reshape(nr, Np)
    uf = u.reshape(-1, 3, Np).transpose(0, 2, 1).reshape(-1, 3)            # (global node, 3)
    flat = out.transpose(0, 2, 1).reshape(-1, 3)                           # view: (node of real elems, 3)
    flat = np.ascontiguousarray(flat)
    for f, nfp in enumerate(_face_sizes(grid)):
        idM = grid.vmapM[:nr, f, :nfp] - 1
        idP = grid.vmapP[:nr, f, :nfp] - 1
        bnd = (grid.elemtobndy[:nr, f] != 0)[:, None]
        idP = np.where(bnd, idM, idP)
        sg = grid.sgeo[:nr, f, :nfp]
        n = [sg[..., GR._n1], sg[..., GR._n2], sg[..., GR._n3]]
        w = sg[..., GR._vMI] * sg[..., GR._sM]
        FM = flux(*(uf[idM, c] for c in range(3)))
        FP = flux(*(uf[idP, c] for c in range(3)))
        for c in range(3):
            fn = (n[0] * (FM[0][c] + FP[0][c]) + n[1] * (FM[1][c] + FP[1][c]) + n[2] * (FM[2][c] + FP[2][c])) / 2
            np.subtract.at(flat[:, c], idM.ravel(), (w * fn).ravel())
    return flat.reshape(nr, Np, 3).transpose(0, 2, 1).copy()


def collect(law, grid, intrp, Q, aux, u_all=None):
    """``atmos_gcm_default_collect`` on one rank: the 13 variables as ``(nlevel, nlat, nlong)`` arrays.
    ``u_all``: the velocity with exchanged ghosts (default: of ``Q`` itself, one rank)."""
    if u_all is None:
        u_all = velocity(Q)
    istate = IR.interpolate_local(intrp, Q[:grid.nreal, :5])
    ithermo = IR.interpolate_local(intrp, thermo(law, Q[:grid.nreal], aux[:grid.nreal]))
    idyn = IR.interpolate_local(intrp, vorticity(vector_gradients(grid, Q)))
    idyn_bl = IR.interpolate_local(intrp, vorticity_model_tendency(grid, u_all))
    IR.project_cubed_sphere(intrp, istate, (2, 3, 4))
    IR.project_cubed_sphere(intrp, idyn, (1, 2, 3))
    IR.project_cubed_sphere(intrp, idyn_bl, (1, 2, 3))
    return finish(intrp, istate, ithermo, idyn, idyn_bl)


def finish(intrp, istate, ithermo, idyn, idyn_bl):
    """``atmos_gcm_default_simple_3d_vars!`` (:150-165) at every interpolated point and the scatter."""
    rho = istate[0]
    v = np.stack([istate[1] / rho, istate[2] / rho, istate[3] / rho, rho, ithermo[0], ithermo[1], ithermo[2],
                  istate[4] / rho, ithermo[3], ithermo[4], ithermo[5], idyn[2], idyn_bl[2]])
    fiv = np.full((len(NAMES),) + tuple(intrp.dims[::-1]), np.nan)
    IR.accumulate_interpolated_data([intrp], [v], fiv)
    return OrderedDict((n, fiv[i]) for i, n in enumerate(NAMES))

"""A NumPy restatement of the IMEX chain of the reference's entropy-stable baroclinic wave
(test/Numerics/ESDGMethods/DryAtmos/baroclinic_wave.jl):

* ``LinearLaw``: ``DryAtmosAcousticGravityLinearModel`` of test/Numerics/ESDGMethods/DryAtmos/linear.jl
  (``total_energy = false``), term by term;
* ``DGRestatement``: a plain DG tendency of an inviscid law in the reference's order -- the
  horizontal ``volume_tendency!`` then the vertical one (DGModel_kernels.jl:64-309, :312-548, launched
  as SpaceDiscretization.jl:1090-1203 says: sources in the vertical launch unless the model is
  horizontal), then ``dgsem_interface_tendency!`` over faces 1..4 and 5..6 (:588-901) with the Rusanov
  or the central first-order flux (NumericalFluxes.jl:223-340) and ``boundary_state!`` on tagged faces;
* ``ColumnSolver``: ``I - alpha L`` of a vertical operator assembled column by column by probing the
  restated operator with unit vectors, factored without pivoting and solved per column (what
  ``ManyColumnLU`` does on a band, here dense);
* ``ark_step``: ``dostep!`` of ``AdditiveRungeKutta`` with the ``LowStorageVariant``
  (AdditiveRungeKuttaMethod.jl:415-523, ``stage_update!`` :565-605, ``solution_update!`` :670-690).

Vectorised over elements and nodes only; every array takes the ``dtype`` given, so the same code
runs in ``np.longdouble``.  Nothing here comes from the product's kernels.  The full operator of a
step is ``esdg_restatement.ESDGRestatement``.  Shared by tests/test_esdg_linear_host.py and
tests/test_gpu_esdg_imex.py."""
import math

import numpy as np

EVERY, HORIZONTAL, VERTICAL = 0, 1, 2
RUSANOV, CENTRAL = 0, 1
_M, _MI = 9, 10
_n1, _n2, _n3, _sM, _vMI = range(5)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


class LinearLaw:
    """The pointwise functions of ``DryAtmosAcousticGravityLinearModel``; states and auxiliary states
    are lists of arrays (auxiliary: Phi, grad Phi[3], ref.T, ref.p, ref.rho, ref.rho e)."""

    def __init__(self, cp_d, cv_d, dtype=np.float64):
        self.dt = dtype
        self.g = dtype(cp_d) / dtype(cv_d)

    def linearized_pressure(self, rho, rhoe, Phi):       # linear.jl:16-24
        return (self.g - 1) * rhoe

    def soundspeed(self, rho, p):                         # DryAtmos.jl:277-280
        return np.sqrt(self.g * p / rho)

    def flux_first_order(self, q, aux):                   # :133-149; F[d][s]
        negzero = -0.0 * q[0]
        pL = self.linearized_pressure(q[0], q[4], aux[0])
        h = (aux[7] + aux[5]) / aux[6]
        F = []
        for d in range(3):
            F.append([q[1 + d]] + [negzero + pL if c == d else negzero for c in range(3)] + [h * q[1 + d]])
        return F

    def source(self, q, aux, direction):                  # :150-167
        S = [-0.0 * q[0] for _ in range(5)]
        if direction in (VERTICAL, EVERY):
            for d in range(3):
                S[1 + d] = S[1 + d] - q[0] * aux[1 + d]
            S[4] = S[4] - (q[1] * aux[1] + q[2] * aux[2] + q[3] * aux[3])
        return S

    def wavespeed(self, n, q, aux):                       # :85-95
        return self.soundspeed(aux[6], aux[5])

    def boundary_state(self, n, qM):                      # DryAtmos.jl:79-94, through linear.jl:98-105
        dn = 2 * _dot(qM[1:4], n)
        return [qM[0]] + [qM[1 + d] - dn * n[d] for d in range(3)] + [qM[4]]


class DGRestatement:
    """``DGModel(law, grid, nf; direction, state_auxiliary)`` on the host, one rank, for an inviscid law
    with the pointwise interface of ``LinearLaw``."""

    def __init__(self, law, grid, state_auxiliary, direction=VERTICAL, nf=RUSANOV, dtype=np.float64):
        self.law, self.grid, self.direction, self.nf, self.dtype = law, grid, direction, nf, dtype
        self.state_auxiliary = np.asarray(state_auxiliary).astype(dtype)
        self.vgeo = grid.vgeo.astype(dtype)
        self.sgeo = grid.sgeo.astype(dtype)
        self.D = [np.asarray(D).astype(dtype) for D in grid.D]
        self.ns = 5

    def _fields(self, Q, shape):
        nr = self.grid.nreal
        q = [Q[:nr, s, :].reshape(shape) for s in range(self.ns)]
        aux = [self.state_auxiliary[:nr, c, :].reshape(shape) for c in range(self.state_auxiliary.shape[1])]
        return q, aux

    def _metric_flux(self, F, xi, shape):
        """``M (xi_x1 F1 + xi_x2 F2 + xi_x3 F3)`` of every state."""
        nr = self.grid.nreal
        M = self.vgeo[:nr, _M, :].reshape(shape)
        G = [self.vgeo[:nr, xi + 3 * c, :].reshape(shape) for c in range(3)]
        return [M * (G[0] * F[0][s] + G[1] * F[1][s] + G[2] * F[2][s]) for s in range(self.ns)]

    def _store(self, tendency, lt, alpha, beta):
        nr, dt = self.grid.nreal, self.dtype
        for s in range(self.ns):
            T = dt(alpha) * lt[s].reshape(nr, -1)
            if beta != 0:
                T = T + dt(beta) * tendency[:nr, s, :]
            tendency[:nr, s, :] = T

    def volume_horizontal(self, tendency, Q, alpha, beta, add_source):
        g, dt = self.grid, self.dtype
        Nq = g.Nq[0]
        shape = (g.nreal, g.Nq[2], Nq, Nq)            # (element, k, j, i)
        q, aux = self._fields(Q, shape)
        F = self.law.flux_first_order(q, aux)
        sf1, sf2 = self._metric_flux(F, 0, shape), self._metric_flux(F, 1, shape)
        MI = self.vgeo[:g.nreal, _MI, :].reshape(shape)
        lt = [np.zeros(shape, dtype=dt) for _ in range(self.ns)]
        if add_source:
            S = self.law.source(q, aux, self.direction)
            lt = [lt[s] + S[s] for s in range(self.ns)]
        D = self.D[0]
        for s in range(self.ns):
            for n in range(Nq):
                lt[s] = lt[s] + MI * D[n, :].reshape(1, 1, 1, Nq) * sf1[s][:, :, :, n:n + 1]
                lt[s] = lt[s] + MI * D[n, :].reshape(1, 1, Nq, 1) * sf2[s][:, :, n:n + 1, :]
        self._store(tendency, lt, alpha, beta)

    def volume_vertical(self, tendency, Q, alpha, beta, add_source):
        g, dt = self.grid, self.dtype
        Nq, Nqv = g.Nq[0], g.Nq[2]
        shape = (g.nreal, Nqv, Nq, Nq)
        q, aux = self._fields(Q, shape)
        F = self.law.flux_first_order(q, aux)
        Fv = self._metric_flux(F, 2, shape)
        MI = self.vgeo[:g.nreal, _MI, :].reshape(shape)
        S = self.law.source(q, aux, self.direction) if add_source else None
        D = self.D[2]
        lt = [np.zeros(shape, dtype=dt) for _ in range(self.ns)]
        for k in range(Nqv):
            for s in range(self.ns):
                # local_tendency[n, s] += MI[n] D[k, n] Fv[k] for every n, then the source of level k
                lt[s] = lt[s] + MI * D[k, :].reshape(1, Nqv, 1, 1) * Fv[s][:, k:k + 1, :, :]
                if add_source:
                    lt[s][:, k] = lt[s][:, k] + S[s][:, k]
        self._store(tendency, lt, alpha, beta)

    def numerical_flux(self, n, qM, auxM, qP, auxP):
        L = self.law
        FM, FP = L.flux_first_order(qM, auxM), L.flux_first_order(qP, auxP)
        flux = [(FM[0][s] + FP[0][s]) * (n[0] / 2) + (FM[1][s] + FP[1][s]) * (n[1] / 2)
                + (FM[2][s] + FP[2][s]) * (n[2] / 2) for s in range(self.ns)]
        if self.nf == CENTRAL:
            return flux
        mw = np.maximum(L.wavespeed(n, qM, auxM), L.wavespeed(n, qP, auxP))
        return [flux[s] + mw * (qM[s] - qP[s]) / 2 for s in range(self.ns)]

    def interface_tendency(self, tendency, Q, alpha, faces):
        g, dt = self.grid, self.dtype
        e = np.arange(g.nreal)
        Np = g.Np
        A = self.state_auxiliary
        for f in faces:
            nfp = g.Nfp[0] if f < 4 else g.Nq[0] * g.Nq[1]
            idM = g.vmapM[e, f, :nfp] - 1
            tag = np.broadcast_to(g.elemtobndy[e, f][:, None], idM.shape)
            idP = np.where(tag != 0, idM, g.vmapP[e, f, :nfp] - 1)
            s_ = self.sgeo[e, f, :nfp, :]
            n, sM, vMI = [s_[..., _n1], s_[..., _n2], s_[..., _n3]], s_[..., _sM], s_[..., _vMI]
            eM, nM, eP, nP = idM // Np, idM % Np, idP // Np, idP % Np
            qM = [Q[eM, s, nM] for s in range(self.ns)]
            qP = [Q[eP, s, nP] for s in range(self.ns)]
            auxM = [A[eM, c, nM] for c in range(A.shape[1])]
            auxP = [A[eP, c, nP] for c in range(A.shape[1])]       # (a tagged face: the minus side's copy)
            if (tag != 0).any():
                wall = self.law.boundary_state(n, qM)
                qP = [np.where(tag != 0, wall[s], qP[s]) for s in range(self.ns)]
            flux = self.numerical_flux(n, qM, auxM, qP, auxP)
            for s in range(self.ns):
                tendency[eM, s, nM] = tendency[eM, s, nM] - dt(alpha) * vMI * sM * flux[s]

    def __call__(self, tendency, Q, t=0.0, alpha=1.0, beta=0.0):
        d = self.direction
        if d in (EVERY, HORIZONTAL):
            self.volume_horizontal(tendency, Q, alpha, beta, d == HORIZONTAL)
        if d in (EVERY, VERTICAL):
            self.volume_vertical(tendency, Q, alpha, 1.0 if d == EVERY else beta, True)
        if d in (EVERY, HORIZONTAL):
            self.interface_tendency(tendency, Q, alpha, (0, 1, 2, 3))
        if d in (EVERY, VERTICAL):
            self.interface_tendency(tendency, Q, alpha, (4, 5))


# ---- the column solve -------------------------------------------------------------------------
def column_shape(grid, nvert, ns=5):
    return (grid.nreal // nvert, nvert, ns, grid.Nq[2], grid.Nq[0] * grid.Nq[1])


def to_columns(Q, grid, nvert):
    """``(nelem, ns, Np)`` -> ``(ncol, n)``, unknowns ordered ``s + ns k + ns Nq_v v``."""
    nh, nv, ns, nqv, nqh2 = column_shape(grid, nvert, Q.shape[1])
    V = Q[:grid.nreal].reshape(nh, nv, ns, nqv, nqh2)
    return np.ascontiguousarray(V.transpose(0, 4, 1, 3, 2)).reshape(nh * nqh2, nv * nqv * ns)


def from_columns(X, Q, grid, nvert):
    nh, nv, ns, nqv, nqh2 = column_shape(grid, nvert, Q.shape[1])
    V = X.reshape(nh, nqh2, nv, nqv, ns).transpose(0, 2, 4, 3, 1)
    Q[:grid.nreal] = V.reshape(grid.nreal, ns, grid.Np)


class ColumnSolver:
    """``LinearBackwardEulerSolver(ManyColumnLU())`` over a restated vertical operator ``lin``: the
    matrix of ``Q -> Q - alpha L(Q)`` of every column, one unit vector per probe
    (``EulerOperator``, BackwardEulerSolvers.jl:21-40), eliminated without pivoting."""

    def __init__(self, lin, nvert, alpha):
        self.lin, self.grid, self.nvert = lin, lin.grid, int(nvert)
        self.update(alpha)

    def assemble(self, alpha):
        g, dt = self.grid, self.lin.dtype
        nh, nv, ns, nqv, nqh2 = column_shape(g, self.nvert)
        n = nv * nqv * ns
        A = np.zeros((nh * nqh2, n, n), dtype=dt)
        Q = np.zeros((g.nelem, ns, g.Np), dtype=dt)
        dQ = np.zeros_like(Q)
        for v in range(nv):
            for k in range(nqv):
                for s in range(ns):
                    Q[:] = 0
                    Q[:g.nreal].reshape(nh, nv, ns, nqv, nqh2)[:, v, s, k, :] = 1
                    dQ[:] = 0
                    self.lin(dQ, Q, float("nan"), 1.0, 0.0)
                    A[:, :, s + ns * k + ns * nqv * v] = to_columns(Q + dt(-alpha) * dQ, g, self.nvert)
        self.A, self.alpha = A, alpha
        return A

    def update(self, alpha):
        A = self.assemble(alpha).copy()
        n = A.shape[1]
        bw = 2 * self.grid.Nq[2] * 5          # an element couples to itself and its two neighbours
        for kk in range(n):                   # A = L U in place, unit diagonal in L as band_lu_kernel! has it
            hi = min(n, kk + bw)
            A[:, kk + 1:hi, kk] = A[:, kk + 1:hi, kk] / A[:, kk:kk + 1, kk]
            A[:, kk + 1:hi, kk + 1:hi] = A[:, kk + 1:hi, kk + 1:hi] - A[:, kk + 1:hi, kk:kk + 1] * A[:, kk:kk + 1, kk + 1:hi]
        self.LU, self.bw = A, bw

    def solve(self, X, B):
        """``X = (I - alpha L)^-1 B`` on the real elements."""
        A = self.LU
        n = A.shape[1]
        y = to_columns(B, self.grid, self.nvert).astype(self.lin.dtype)
        for jj in range(n):                   # L y = b, column by column (band_forward_kernel!)
            hi = min(n, jj + self.bw)
            y[:, jj + 1:hi] = y[:, jj + 1:hi] - A[:, jj + 1:hi, jj] * y[:, jj:jj + 1]
        for jj in range(n - 1, -1, -1):       # U x = y (band_back_kernel!)
            lo = max(0, jj - self.bw + 1)
            y[:, jj] = y[:, jj] / A[:, jj, jj]
            y[:, lo:jj] = y[:, lo:jj] - A[:, lo:jj, jj] * y[:, jj:jj + 1]
        from_columns(y, X, self.grid, self.nvert)
        return X


# ---- ARK2GiraldoKellyConstantinescu, LowStorageVariant --------------------------------------------
def ark2gkc_tableau(dtype=np.float64, paperversion=False):
    """AdditiveRungeKuttaMethod.jl:839-895."""
    s2 = np.sqrt(dtype(2))
    a32 = (3 + 2 * s2) / 6 if paperversion else dtype(1) / 2
    z = dtype(0)
    A_e = np.array([[z, z, z], [2 - s2, z, z], [1 - a32, a32, z]], dtype=dtype)
    A_i = np.array([[z, z, z], [1 - 1 / s2, 1 - 1 / s2, z], [1 / (2 * s2), 1 / (2 * s2), 1 - 1 / s2]], dtype=dtype)
    B = np.array([1 / (2 * s2), 1 / (2 * s2), 1 - 1 / s2], dtype=dtype)
    Cc = np.array([z, 2 - s2, dtype(1)], dtype=dtype)
    return A_e, A_i, B, Cc


def ark_step(full, lin, solver, Q, t, dt, tableau, split):
    """One step on the real elements of ``Q``.  ``full``: the explicit operator; ``lin``: the linear one
    (``None`` with ``solver = None``: L = 0, the solve is the identity); with ``split`` the explicit
    tendency is full minus linear, two evaluations, and the linear tendencies join the stage tendencies
    before the solution update."""
    A_e, A_i, B, Cc = tableau
    ns = len(B)
    nr = full.grid.nreal
    dt = Q.dtype.type(dt)
    Qs = [Q] + [np.zeros_like(Q) for _ in range(ns - 1)]
    R = [np.zeros_like(Q) for _ in range(ns)]

    def rhs(Rs, Qst, time):
        full(Rs, Qst, time, 1.0, 0.0)
        if split and lin is not None:
            lin(Rs, Qst, time, -1.0, 1.0)

    rhs(R[0], Qs[0], t + Cc[0] * dt)
    Qtt = np.zeros_like(Q)
    for i in range(1, ns):
        Qhat = Q.copy()
        Qst = np.full_like(Q[:nr], -0.0)
        for j in range(i):
            rkcoeff = A_i[i, j] / A_i[i, i] if split else (A_i[i, j] - A_e[i, j]) / A_i[i, i]
            common = rkcoeff * Qs[j][:nr]
            Qhat[:nr] += common + (dt * A_e[i, j]) * R[j][:nr]
            Qst -= common
        Qs[i][:nr] = Qst
        if solver is None:
            Qtt[:nr] = Qhat[:nr]
        else:
            alpha = dt * A_i[i, i]
            if alpha != solver.alpha:
                solver.update(alpha)
            solver.solve(Qtt, Qhat)
        Qs[i][:nr] += Qtt[:nr]
        rhs(R[i], Qs[i], t + Cc[i] * dt)
    if split and lin is not None:
        for i in range(ns):
            lin(R[i], Qs[i], t + Cc[i] * dt, 1.0, 1.0)
    for i in range(ns):
        Q[:nr] += (B[i] * dt) * R[i][:nr]
    return Q


def explicit_tableau_step(full, Q, t, dt, tableau):
    """The explicit Runge-Kutta step of the explicit tableau alone: stages ``Q + dt sum_j a_ij R_j``,
    solution ``Q + dt sum_i b_i R_i``."""
    A_e, _, B, Cc = tableau
    ns = len(B)
    nr = full.grid.nreal
    R = []
    for i in range(ns):
        Qi = Q.copy()
        for j in range(i):
            Qi[:nr] += (dt * A_e[i, j]) * R[j][:nr]
        Ri = np.zeros_like(Q)
        full(Ri, Qi, t + Cc[i] * dt, 1.0, 0.0)
        R.append(Ri)
    out = Q.copy()
    for i in range(ns):
        out[:nr] += (B[i] * dt) * R[i][:nr]
    return out


# ---- Courant numbers of the full law  DryAtmos.jl:747-793 --------------------------------------------
def min_neighbor_distance(grid, direction):
    """``kernel_min_neighbor_distance!`` (Grids.jl:1228-1333): per node, the distance to the nearest
    neighbour along the grid lines of ``direction``; ``(nreal, Nq_v, Nq, Nq)``."""
    Nq, Nqv = grid.Nq[0], grid.Nq[2]
    x = [grid.vgeo[:grid.nreal, 12 + d, :].reshape(grid.nreal, Nqv, Nq, Nq) for d in range(3)]
    md = np.full(x[0].shape, np.inf)

    def along(axis):
        nonlocal md
        n = x[0].shape[axis]
        lo = [slice(None)] * 4
        hi = [slice(None)] * 4
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        d0, d1, d2 = x[0][hi] - x[0][lo], x[1][hi] - x[1][lo], x[2][hi] - x[2][lo]
        dist = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
        md[lo] = np.minimum(md[lo], dist)
        md[hi] = np.minimum(md[hi], dist)

    if direction != VERTICAL:
        along(3)
        along(2)
    if direction != HORIZONTAL:
        along(1)
    return md


def courant(kind, grid, Q, aux, dt, direction, cp_d, cv_d, grav):
    """``advective_courant`` (``kind`` 0) / ``nondiffusive_courant`` (1) of ``DryAtmosModel``, the maximum
    over the real nodes."""
    nr = grid.nreal
    shape = (nr, grid.Nq[2], grid.Nq[0], grid.Nq[0])
    q = [Q[:nr, s, :].reshape(shape) for s in range(5)]
    k = [aux[:nr, 1 + d, :].reshape(shape) / grav for d in range(3)]
    dx = min_neighbor_distance(grid, direction)
    dotk = q[1] * k[0] + q[2] * k[1] + q[3] * k[2]
    if direction == VERTICAL:
        normu = np.abs(dotk) / q[0]
    else:
        v = [(q[1 + d] - dotk * k[d]) / q[0] if direction == HORIZONTAL else q[1 + d] / q[0] for d in range(3)]
        normu = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if kind == 0:
        return float(np.max(dt * normu / dx))
    g = cp_d / cv_d
    p = (g - 1) * (q[4] - (q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) / (2 * q[0]))
    ss = np.sqrt(g * p / q[0])
    return float(np.max(dt * (normu + ss) / dx))

"""The element filters stated a third time, next to the device kernels (csrc/filters.h) and their twin
(oracle/filter_oracle.c): from the reference's ``src/Numerics/Mesh/Filters.jl`` and
``src/Atmos/Model/filters.jl``, with none of the kernels' structure.

  * Filter matrices in mpmath at 40 digits: LGL nodes by Newton on ``(1 - x^2) P'_N``, the orthonormal
    Legendre Vandermonde matrix from ``mp.legendre``, ``W = V Sigma V^-1`` (``filter_matrix``).
  * Application in ``np.longdouble`` as ONE dense contraction per element and direction: the horizontal
    application is ``F (x) F`` on (xi1, xi2), the vertical one ``F`` on xi3.  There are no per-axis
    passes with intermediates rounded to double, and sums are numpy's, in whatever order.
    ``EveryDirection`` is the horizontal application followed by the vertical application of its
    result (``apply_async!``, Filters.jl:467-503 and :566-605): each is a whole
    ``compute_filter_argument!`` -> contraction -> ``compute_filter_result!`` on the state, so the
    vertical application of ``AtmosSpecificFilterPerturbations`` divides by the density the
    horizontal one produced because that density is simply the state it is handed.
  * The mass-preserving filter rewrites every state, filtered or not, as
    ``after + (sum(M before) - sum(M after)) / sum(M)`` per element and per application; TMAR scales
    the non-negative part of a state by ``sum(MJ q) / sum(MJ max(q, 0))``.

Every value carries a bound on what double arithmetic may do to it (running error analysis: the same
walk on absolute values).  A number is a pair ``(v, e)``: ``v`` the long double value, ``e >= 0`` with
|device - v| <= e to first order in eps.  The rules, with eps = 2^-52:
  * an NQ-term dot product adds ``NQ eps sum|F||x|`` -- one per tensor pass the device makes, so the
    horizontal application adds ``2 NQ eps (|F| (x) |F|) |x|`` and the vertical ``NQ eps |F| |x|``;
  * a sum of n terms (tree or serial) adds ``(ceil(log2 n) + 2) eps sum|terms|``;
  * every other elementary operation (+, -, *, /) adds ``eps |result|``;
  * incoming bounds go through an operation by its absolute-value image (``|F| e``, ``|b| e_a +
    |a| e_b``, ``e_a / |b| + |a / b| e_b / |b|``).
No factor is tuned.  The long double arithmetic of this file rounds too, at 2^-64 per operation: the
same rules charge it (``U = eps + eps_ld`` and ``eps_ld`` times the dense contraction's term count),
which adds less than 1 % to any bound.  Terms of order eps^2 are dropped: with eps twice the unit
roundoff the first-order form still dominates ``n u / (1 - n u)`` at every n used here.

The filter matrices an application takes are data, as the device is handed them: the tests pass the
host's double matrices (``mesh/filters.py``), which tests/test_filters_restatement_host.py pins to the
40-digit ones entry by entry.
"""
import math

import mpmath as mp
import numpy as np

DIGITS = 40
LD = np.longdouble
EPS = LD(2.0) ** -52
EPS_LD = LD(np.finfo(LD).eps)
U = EPS + EPS_LD
EVERY, HORIZONTAL, VERTICAL = 0, 1, 2
T_INDICES, T_ATMOS_PERT, T_ATMOS_SPECIFIC = 0, 1, 2
K_SPECTRAL, K_MASS_PRESERVING, K_TMAR = 0, 1, 2
M_COL = 9        # vgeo column of the mass M = w_i w_j w_k J (Grids.jl:129-146)


# ---- filter matrices, 40 digits ---------------------------------------------------------------------
def lgl_nodes(N, start):
    """The N + 1 Legendre-Gauss-Lobatto nodes: roots of ``(1 - x^2) P'_N(x) = N (P_{N-1} - x P_N)``, by
    Newton from ``start``; the derivative is ``-N (N + 1) P_N`` (Legendre's equation)."""
    assert N >= 1 and len(start) == N + 1
    with mp.workdps(DIGITS):
        xs = []
        for x0 in start:
            x = mp.mpf(float(x0))
            for _ in range(100):
                f = N * (mp.legendre(N - 1, x) - x * mp.legendre(N, x))
                dx = f / (-N * (N + 1) * mp.legendre(N, x))
                x -= dx
                if abs(dx) < mp.mpf(10) ** (-DIGITS + 3):
                    break
            else:
                raise AssertionError("Newton did not converge from %r" % (x0,))
            xs.append(x)
        for a, b in zip(xs, xs[1:]):
            assert b - a > mp.mpf(10) ** -6, "LGL nodes must be distinct and ascending"
        assert xs[0] == -1 and xs[-1] == 1
        return xs


def vandermonde(x):
    """``V[i, n] = sqrt((2n + 1) / 2) P_n(x_i)``: the Legendre polynomials orthonormal on [-1, 1]."""
    n = len(x)
    return mp.matrix([[mp.sqrt(mp.mpf(2 * k + 1) / 2) * mp.legendre(k, xi) for k in range(n)] for xi in x])


def sigma_exponential(s, alpha):
    """``exp(-alpha eta^s)`` (Filters.jl:201); ``alpha`` is the double the caller configured."""
    a = mp.mpf(float(alpha))
    return lambda eta: mp.exp(-a * eta ** s)


def sigma_boyd_vandeven(s):
    """``erfc(sqrt(s) chi a) / 2``, ``a = 2 |eta| - 1``, ``chi = sqrt(-log(1 - a^2) / a^2)``, ``chi = 1``
    at ``a = 0`` (Filters.jl:255-259); the limits at ``|a| = 1`` are erfc(-inf) / 2 = 1, erfc(inf) / 2 = 0."""
    def sigma(eta):
        a = 2 * abs(eta) - 1
        if a == -1:
            return mp.mpf(1)
        if a == 1:
            return mp.mpf(0)
        chi = mp.mpf(1) if a == 0 else mp.sqrt(-mp.log1p(-a * a) / (a * a))
        return mp.erfc(mp.sqrt(s) * chi * a) / 2
    return sigma


def sigma_cutoff(eta):
    return mp.mpf(0)


def filter_matrix(x, Nc, sigma, modified=False):
    """``spectral_filter_matrix`` / ``modified_filter_matrix`` (Filters.jl:114-159): modes ``n = Nc..N``
    are scaled by ``sigma((n - Nc) / (N - Nc))``.  Returns ``(W, B)``: ``W = V Sigma V^-1`` and the
    cancellation-free scale ``B = |V| |Sigma| |V^-1|`` of its entries.  ``Nc > N`` is the identity for
    the modified matrix; at ``Nc == N`` the argument of sigma is 0 / 0, which only the constant sigma
    of the cutoff filters gives a meaning to (``eta`` is passed as ``None``)."""
    with mp.workdps(DIGITS):
        N = len(x) - 1
        assert N >= 0 and Nc >= 0
        n1 = N + 1
        if Nc > N:
            assert modified, "spectral_filter_matrix asserts 0 <= Nc <= N"
            return mp.eye(n1), mp.eye(n1)
        V = vandermonde(x)
        Vi = V ** -1
        S = [mp.mpf(1)] * n1
        for n in range(Nc, n1):
            S[n] = sigma(mp.mpf(n - Nc) / (N - Nc) if N != Nc else None)
        W = V * mp.diag(S) * Vi
        absV = V.apply(abs)
        B = absV * mp.diag([abs(v) for v in S]) * Vi.apply(abs)
        return W, B


def to_float64(A):
    """Correctly rounded doubles of an mpmath matrix (or list)."""
    if isinstance(A, mp.matrix):
        return np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])
    return np.array([float(a) for a in A])


# ---- numbers with bounds ----------------------------------------------------------------------------
def exact(a):
    v = np.asarray(a, dtype=LD)
    return v, np.zeros_like(v)


def add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def sub(a, b):
    v = a[0] - b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def mul(a, b):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + U * np.abs(v)


def div(a, b):
    v = a[0] / b[0]
    return v, (a[1] + np.abs(v) * b[1]) / np.abs(b[0]) + U * np.abs(v)


def total(a, axis):
    """Sum of n terms along ``axis`` (kept as an axis of length 1)."""
    n = a[0].shape[axis]
    v = a[0].sum(axis=axis, keepdims=True)
    depth = math.ceil(math.log2(n)) + 2
    return v, a[1].sum(axis=axis, keepdims=True) + depth * U * np.abs(a[0]).sum(axis=axis, keepdims=True)


def contract(F, x, horizontal):
    """One application of the filter to the fields ``x`` of shape ``(..., Np)``, node ``i + NQ (j + NQ k)``:
    the dense ``F (x) F`` on (j, i) for every k, or ``F`` on k for every (j, i)."""
    F = np.asarray(F, dtype=LD)
    NQ = F.shape[0]
    v, e = x
    shp = v.shape
    v, e = v.reshape(shp[:-1] + (NQ, NQ * NQ)), e.reshape(shp[:-1] + (NQ, NQ * NQ))
    if horizontal:
        H = np.kron(F, F)                       # [(j, i), (n, m)] = F[j, n] F[i, m]
        A = np.abs(H)
        w = np.matmul(v, H.T)
        b = np.matmul(e, A.T) + (2 * NQ * EPS + NQ * NQ * EPS_LD) * np.matmul(np.abs(v), A.T)
    else:
        A = np.abs(F)
        w = np.matmul(F, v)
        b = np.matmul(A, e) + NQ * U * np.matmul(A, np.abs(v))
    return w.reshape(shp), b.reshape(shp)


# ---- targets: compute_filter_argument! / compute_filter_result! -------------------------------------
def _cols(q, idx):
    return q[0][:, idx], q[1][:, idx]


def _argument(target, q, aux):
    """The filtered fields ``(nelem, nfs, Np)`` of the state ``q``."""
    kind, idx = target.target_id, [i - 1 for i in target.indices]
    if kind == T_INDICES:                       # Filters.jl:79-88
        return _cols(q, idx)
    c_rho, c_rhoe = target.aux_offsets()
    ref_rho, ref_rhoe = exact(aux[:, c_rho]), exact(aux[:, c_rhoe])
    if kind == T_ATMOS_PERT:                    # filters.jl:11-29: the state minus the reference state
        fv, fe = q[0].copy(), q[1].copy()
        for s, ref in ((0, ref_rho), (4, ref_rhoe)):
            fv[:, s], fe[:, s] = sub((q[0][:, s], q[1][:, s]), ref)
        return fv, fe
    # filters.jl:57-80: specific quantities, the energy minus the reference's specific energy
    one = exact(np.ones_like(aux[:, 0]))
    rho_inv = div(one, (q[0][:, 0], q[1][:, 0]))
    fv, fe = mul(q, (rho_inv[0][:, None], rho_inv[1][:, None]))
    e_ref = mul(ref_rhoe, div(one, ref_rho))
    fv[:, 4], fe[:, 4] = sub((fv[:, 4], fe[:, 4]), e_ref)
    return fv, fe


def _result(target, q, f, aux):
    """The state after ``compute_filter_result!``: ``q`` is the state the application started from."""
    kind, idx = target.target_id, [i - 1 for i in target.indices]
    qv, qe = q[0].copy(), q[1].copy()
    if kind == T_INDICES:                       # Filters.jl:90-99: in order, so the last writer wins
        for s, i in enumerate(idx):
            qv[:, i], qe[:, i] = f[0][:, s], f[1][:, s]
        return qv, qe
    c_rho, c_rhoe = target.aux_offsets()
    ref_rho, ref_rhoe = exact(aux[:, c_rho]), exact(aux[:, c_rhoe])
    if kind == T_ATMOS_PERT:                    # filters.jl:30-48
        qv, qe = f[0].copy(), f[1].copy()
        for s, ref in ((0, ref_rho), (4, ref_rhoe)):
            qv[:, s], qe[:, s] = add((f[0][:, s], f[1][:, s]), ref)
        return qv, qe
    # filters.jl:82-104: back to conserved quantities with the density the application started from
    rho = (q[0][:, 0], q[1][:, 0])
    ratio = div(rho, ref_rho)
    qv, qe = mul(f, (rho[0][:, None], rho[1][:, None]))
    qv[:, 4], qe[:, 4] = add((qv[:, 4], qe[:, 4]), mul(ref_rhoe, ratio))
    return qv, qe


# ---- the three filters ------------------------------------------------------------------------------
def _apply_once(q, target, F, horizontal, aux, M):
    """One application (one launch of the reference) to the real elements; ``M`` (nelem, Np) for the
    mass-preserving filter, else None."""
    after = _result(target, q, contract(F, _argument(target, q, aux), horizontal), aux)
    if M is None:
        return after
    # Filters.jl:1040-1066: every state gets the element mean it had before the application
    Mx = exact(M[:, None, :])
    mass_before = total(mul(Mx, q), axis=2)
    mass_after = total(mul(Mx, after), axis=2)
    mass = total(Mx, axis=2)
    one = exact(np.ones_like(mass[0]))
    return add(after, mul(div(one, mass), sub(mass_before, mass_after)))


def _tmar(q, target, MJ):
    """Filters.jl:796-884, the listed states in order."""
    qv, qe = q[0].copy(), q[1].copy()
    Mx = exact(MJ)
    for i in (j - 1 for j in target.indices):
        s = (qv[:, i], qe[:, i])
        pos = s[0] >= 0
        clipped = (np.where(pos, s[0], 0), np.where(pos, s[1], 0))
        num, den = total(mul(Mx, s), axis=1), total(mul(Mx, clipped), axis=1)
        up = num[0] > 0
        safe = (np.where(up, den[0], 1), np.where(up, den[1], 0))
        r = div(num, safe)
        r = (np.where(up, r[0], 0), np.where(up, r[1], 0))
        w = mul(r, s)
        qv[:, i], qe[:, i] = np.where(pos, w[0], 0), np.where(pos, w[1], 0)
    return qv, qe


def apply(Q, target, grid, kind, matrices=None, direction=EVERY, state_auxiliary=None):
    """``Filters.apply!(Q, target, grid, filter; direction, state_auxiliary)`` on a copy of the double
    array ``Q`` (nelem, nstate, Np).  ``kind``: K_SPECTRAL / K_MASS_PRESERVING / K_TMAR; ``matrices``:
    (horizontal, vertical) filter matrices, row = output node; ``target``: an object with
    ``target_id``, ``indices`` (1-based) and ``aux_offsets()``.  Returns ``(value, bound)`` as long
    doubles; ghost elements come back as they are, with bound 0."""
    nr = grid.nreal
    q = exact(Q[:nr])
    aux = None if state_auxiliary is None else np.asarray(state_auxiliary)[:nr]
    M = np.asarray(grid.vgeo)[:nr, M_COL, :]
    if kind == K_TMAR:
        q = _tmar(q, target, M)
    else:
        Mw = M if kind == K_MASS_PRESERVING else None
        if direction in (EVERY, HORIZONTAL):
            q = _apply_once(q, target, matrices[0], True, aux, Mw)
        if direction in (EVERY, VERTICAL):
            q = _apply_once(q, target, matrices[-1], False, aux, Mw)
    value, bound = exact(Q)
    value[:nr], bound[:nr] = q
    return value, bound


def ratio(computed, value, bound):
    """Largest |computed - value| / bound over the nodes (a node whose bound is 0 must agree exactly)."""
    err = np.abs(np.asarray(computed, dtype=LD) - value)
    zero = bound == 0
    if np.any(err[zero] != 0):
        return float("inf")
    if zero.all():
        return 0.0
    return float((err[~zero] / bound[~zero]).max())

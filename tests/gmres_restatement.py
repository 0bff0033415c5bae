"""A NumPy restatement of ``GeneralizedMinimalResidual`` (generalized_minimal_residual_solver.jl:
``initialize!``, ``doiteration!``), of ``linearsolve!`` (SystemSolvers.jl:240-286) and of
``LinBESolver`` on ``EulerOperator(L, -alpha)`` (BackwardEulerSolvers.jl:21-40, 112-196), in the
operation order of the device solver (csrc/gmres.hip).  ``operator(out, q)`` writes ``A q``; the
vectors are arrays of any shape, dots and norms plain sums over ``rv`` (the real elements).  Shared
by tests/test_gmres_host.py (dense systems, the IMEX goldens on the oracle operators) and
tests/test_gpu_gmres.py."""
import math

import numpy as np


def givens(f, g):
    """``givens(f, g, i1, i2)`` of LinearAlgebra (``givensAlgorithm``) for magnitudes that need no
    rescaling: ``(c, s)``."""
    if g == 0:
        return 1.0, 0.0
    if f == 0:
        return 0.0, 1.0
    r = math.sqrt(f * f + g * g)
    c, s = f / r, g / r
    if abs(f) > abs(g) and c < 0:
        c, s = -c, -s
    return c, s


class Info:
    def __init__(self):
        self.iterations, self.converged = 0, False
        self.residual_norm = self.threshold = 0.0
        self.residuals = []          # |g0[j+1]| of every inner iteration, in order

    def margin(self):
        """The smallest relative distance of a deciding residual from the threshold: the break
        test ``residual < threshold`` is safe against rounding when this is large."""
        return min([abs(r - self.threshold) / self.threshold for r in self.residuals], default=np.inf)


class GMRES:
    def __init__(self, like, M=20, rtol=math.sqrt(2.0 ** -52), atol=2.0 ** -52, rv=slice(None)):
        self.M, self.rtol, self.atol, self.rv = int(M), float(rtol), float(atol), rv
        self.basis = [np.zeros_like(like) for _ in range(self.M + 1)]
        self.H = np.zeros((self.M + 1, self.M))
        self.g0 = np.zeros(self.M + 1)

    def dot(self, a, b):
        return float(np.dot(a[self.rv].ravel(), b[self.rv].ravel()))

    def norm(self, a):
        return math.sqrt(self.dot(a, a))

    def initialize(self, operator, Q, Qrhs):
        """-> (converged, threshold, residual_norm)"""
        rv, v = self.rv, self.basis
        operator(v[0], Q)
        v[0][rv] = Qrhs[rv] - v[0][rv]
        residual_norm = self.norm(v[0])
        threshold = self.rtol * residual_norm
        if threshold < self.atol:
            return True, threshold, residual_norm
        self.g0[:] = 0.0
        self.g0[0] = residual_norm
        v[0][rv] = v[0][rv] / residual_norm
        return False, max(threshold, self.atol), residual_norm

    def doiteration(self, operator, Q, Qrhs, threshold, jmax, info):
        """One cycle of at most ``jmax <= M`` Arnoldi steps -> (converged, j, residual_norm)."""
        rv, v, H, g0 = self.rv, self.basis, self.H, self.g0
        cs, sn = [], []
        converged, residual_norm, j = False, np.inf, 0
        for j in range(jmax):
            operator(v[j + 1], v[j])
            for i in range(j + 1):
                H[i, j] = self.dot(v[j + 1], v[i])
                v[j + 1][rv] = v[j + 1][rv] - H[i, j] * v[i][rv]
            H[j + 1, j] = self.norm(v[j + 1])
            v[j + 1][rv] = v[j + 1][rv] / H[j + 1, j]
            for k in range(j):
                a1, a2 = H[k, j], H[k + 1, j]
                H[k, j] = cs[k] * a1 + sn[k] * a2
                H[k + 1, j] = -sn[k] * a1 + cs[k] * a2
            f, g = H[j, j], H[j + 1, j]
            c, s = givens(f, g)
            cs.append(c)
            sn.append(s)
            H[j, j] = c * f + s * g
            H[j + 1, j] = -s * f + c * g
            g1, g2 = g0[j], g0[j + 1]
            g0[j] = c * g1 + s * g2
            g0[j + 1] = -s * g1 + c * g2
            residual_norm = abs(g0[j + 1])
            info.residuals.append(residual_norm)
            if residual_norm < threshold:
                converged = True
                break
        nj = j + 1
        y = g0[:nj].copy()
        for col in range(nj - 1, -1, -1):
            y[col] = y[col] / H[col, col]
            for i in range(col - 1, -1, -1):
                y[i] -= H[i, col] * y[col]
        q = Q[rv].copy()
        for i in range(nj):
            q = q + y[i] * v[i][rv]
        Q[rv] = q
        return converged, nj, residual_norm

    def linearsolve(self, operator, Q, Qrhs, max_iters=None):
        """``linearsolve!``: at most ``max_iters`` inner iterations in total (default: the length
        of ``Q``'s real part); a restart keeps the first threshold."""
        info = Info()
        if max_iters is None:
            max_iters = Q[self.rv].size
        converged, threshold, nrm = self.initialize(operator, Q, Qrhs)
        info.threshold, info.residual_norm, info.converged = threshold, nrm, converged
        if not math.isfinite(nrm):
            raise FloatingPointError("norm of residual is not finite after 0 iterations")
        if converged:
            return info
        while not converged and info.iterations < max_iters:
            converged, nj, res = self.doiteration(operator, Q, Qrhs, threshold,
                                                  min(self.M, max_iters - info.iterations), info)
            info.iterations += nj
            info.residual_norm = res
            if not math.isfinite(res):
                raise FloatingPointError("norm of residual is not finite after %d iterations"
                                         % info.iterations)
            if not converged and info.iterations < max_iters:
                if not self.initialize(operator, Q, Qrhs)[0]:
                    pass                      # (threshold < atol at a restart leaves g0 and v_0 alone)
        info.converged = converged
        return info


def euler_operator(L, alpha, t=0.0):
    """``EulerOperator(L, -alpha)``: ``out = q - alpha L(q)``, with ``L(out, q, t, a, b)`` forming
    ``out = a L(q) + b out`` (an oracle ``OracleDGModel``)."""
    def A(out, q):
        out[...] = q
        L(out, q, t, -alpha, 1.0)
    return A


class LinBESolver:
    """``LinBESolver`` around the restatement, with the interface ``oracle.ark_step`` and
    ``mrigark_restatement.implicit_step`` drive: ``alpha``, ``update(alpha)``, ``solve(X, B)`` /
    ``__call__(Q, Qhat, alpha, t)``.  ``guess_from_rhs``: the ARK stage update initialises the
    guess ``Qtt`` to ``Qhat`` (AdditiveRungeKuttaMethod.jl:603)."""

    def __init__(self, L, gmres, alpha, guess_from_rhs=True):
        self.L, self.gmres, self.alpha, self.guess_from_rhs = L, gmres, alpha, guess_from_rhs
        self.infos = []

    def update(self, alpha):
        self.alpha = alpha

    def solve(self, X, B, t=0.0):
        if self.guess_from_rhs:
            X[...] = B
        self.infos.append(self.gmres.linearsolve(euler_operator(self.L, self.alpha, t), X, B))
        return X

    def __call__(self, Q, Qhat, alpha, t):
        self.alpha = alpha
        self.infos.append(self.gmres.linearsolve(euler_operator(self.L, alpha, t), Q, Qhat))

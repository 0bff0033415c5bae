"""Finite-volume reconstructions of a ``DGFVModel``: host-side mirror of
``src/Numerics/DGMethods/FVReconstructions.jl``.

The objects describe the reconstruction to the library (``cmdg_fv_desc``); called with numpy
arrays they also evaluate it on the host, as the reference's functors do:
``recon(cell_states, cell_weights) -> (state_bot, state_top)`` with ``cell_states`` of shape
``(2 w + 1, ...)`` for any ``w <= width``.
"""
import numpy as np

__all__ = ["FVConstant", "FVLinear", "VanLeer", "NoLimiter", "width"]


class VanLeer:
    """``VanLeer`` (FVReconstructions.jl:166-175): ``2 a b / (a + b)`` where the slopes agree in
    sign, zero elsewhere."""
    limiter_id = 0

    def __call__(self, d_top, d_bot):
        d_top, d_bot = np.asarray(d_top, dtype=np.float64), np.asarray(d_bot, dtype=np.float64)
        same = d_top * d_bot > 0
        den = np.where(same, d_top + d_bot, 1.0)
        return np.where(same, 2 * d_top * d_bot / den, 0.0)


class NoLimiter:
    """``NoLimiter`` (FVReconstructions.jl:188-192): the mean of the two slopes."""
    limiter_id = 1

    def __call__(self, d_top, d_bot):
        return (np.asarray(d_top, dtype=np.float64) + np.asarray(d_bot, dtype=np.float64)) / 2


class FVConstant:
    """``FVConstant`` (FVReconstructions.jl:60-67): both face values are the cell value."""
    reconstruction_id = 0
    width = 0
    limiter = VanLeer()          # unused; keeps the descriptor complete

    def __call__(self, cell_states, cell_weights=None):
        c = np.asarray(cell_states, dtype=np.float64)
        assert c.shape[0] == 1
        return c[0].copy(), c[0].copy()


class FVLinear:
    """``FVLinear{W}(limiter)`` (FVReconstructions.jl:83-143): limited linear reconstruction from
    three cells; a wider stencil (``W`` up to 3, a debugging aid of the reference) reduces to its
    middle three cells, a single cell to ``FVConstant``."""
    reconstruction_id = 1

    def __init__(self, width=1, limiter=None):
        if not 1 <= int(width) <= 3:
            raise ValueError("FVLinear: width must be 1, 2 or 3")
        self.width = int(width)
        self.limiter = VanLeer() if limiter is None else limiter

    def __call__(self, cell_states, cell_weights):
        c = np.asarray(cell_states, dtype=np.float64)
        w = np.asarray(cell_weights, dtype=np.float64)
        D = c.shape[0]
        assert D % 2 == 1 and w.shape[0] == D
        if D == 1:
            return c[0].copy(), c[0].copy()
        if D > 3:
            W = (D - 1) // 2
            c, w = c[W - 1:W + 2], w[W - 1:W + 2]
        wi_top = 1 / (w[2] + w[1])
        wi_bot = 1 / (w[1] + w[0])
        d_top = wi_top * (c[2] - c[1])
        d_bot = wi_bot * (c[1] - c[0])
        d = self.limiter(d_top, d_bot)
        return c[1] - d * w[1], c[1] + d * w[1]


def width(recon):
    """``width(recon)``: ``2 width + 1`` cells enter a reconstruction."""
    return recon.width

"""A NumPy restatement of the interpolation kernels of the reference
(src/Numerics/Mesh/Interpolation.jl): the per-point set-up of ``flg`` and ``fac`` (:247-292,
:904-949), ``interpolate_local_kernel!`` (:449-570), ``project_cubed_sphere_kernel!``
(:1373-1414) and ``accumulate_helper_kernel!`` (:1548-1561).  Float64, in the reference's order
of operations: the unnormalised barycentric terms ``wb_i / (xi - m_i)`` are summed per
direction, a direction whose ``xi`` sits on a node within ``4 eps`` picks that node (the flag
branches), and the result is scaled by ``fac = 1 / (fac1 fac2 fac3)`` at the end.  The ``xi``,
offsets and index triples come from climatemachine.jl_amd/mesh/interpolation.py.  Shared by
tests/test_interpolation_host.py and tests/test_gpu_interpolation.py.

Layouts are this project's (reversed Julia shapes): ``Q (nelem, nstate, Np)``,
``v (nstate, Npl)``, ``fiv (nstate, n3, n2, n1)``."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
TOLER = 4 * EPS


def baryweights(r):
    """``baryweights(r)`` of Elements.jl: ``wb_i = 1 / prod_{j != i} (r_i - r_j)``."""
    r = np.asarray(r, dtype=np.float64)
    wb = np.ones(len(r))
    for i in range(len(r)):
        for j in range(len(r)):
            if j != i:
                wb[i] = wb[i] * (r[i] - r[j])
    return 1.0 / wb


def flags_and_factors(intrp):
    """``flg (3, Npl)`` (1-based node, 0 = none) and ``fac (Npl)`` as the constructors set them."""
    xis = (intrp.xi1, intrp.xi2, intrp.xi3)
    flg = np.zeros((3, intrp.Npl), dtype=np.int64)
    facs = []
    for d in range(3):
        m = intrp.m_xi[d]
        wb = baryweights(m)
        fac = np.zeros(intrp.Npl)
        for ib in range(len(m)):
            hit = np.abs(m[ib] - xis[d]) < TOLER
            flg[d, hit] = ib + 1
            with np.errstate(divide="ignore", invalid="ignore"):
                term = wb[ib] / (xis[d] - m[ib])
            fac = np.where(hit, fac, fac + term)
        fac[flg[d] != 0] = 1.0
        facs.append(fac)
    return flg, 1.0 / (facs[0] * facs[1] * facs[2])


def interpolate_local(intrp, Q):
    """``interpolate_local!``: returns ``v (nstate, Npl)``."""
    q1, q2, q3 = intrp.Nq
    nstate = Q.shape[1]
    flg, fac = flags_and_factors(intrp)
    el = np.repeat(np.arange(intrp.Nel), np.diff(intrp.offset))
    wb = [baryweights(m) for m in intrp.m_xi]
    m1, m2, m3 = intrp.m_xi
    v = np.zeros((nstate, intrp.Npl))
    step = 1 << 11          # (p, s, k, j, i) temporaries that stay in cache
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(0, intrp.Npl, step):
            sl = slice(s, min(s + step, intrp.Npl))
            sv = Q[el[sl]].reshape(-1, nstate, q3, q2, q1)           # (p, s, k, j, i)
            x1, x2, x3 = intrp.xi1[sl], intrp.xi2[sl], intrp.xi3[sl]
            f1, f2, f3 = flg[0, sl], flg[1, sl], flg[2, sl]
            # phir: sum over i in order, or the flagged node
            acc = sv[..., 0] * (wb[0][0] / (x1 - m1[0]))[:, None, None, None]
            for ii in range(1, q1):
                acc = acc + sv[..., ii] * (wb[0][ii] / (x1 - m1[ii]))[:, None, None, None]
            pick = np.take_along_axis(sv, np.maximum(f1 - 1, 0)[:, None, None, None, None], axis=4)[..., 0]
            vjk = np.where((f1 == 0)[:, None, None, None], acc, pick)     # (p, s, k, j)
            # phis
            w2 = wb[1][None, :] / (x2[:, None] - m2[None, :])              # (p, j)
            scaled = vjk * w2[:, None, None, :]
            acc = scaled[..., 0]
            for ij in range(1, q2):
                acc = acc + scaled[..., ij]
            pick = np.take_along_axis(vjk, np.maximum(f2 - 1, 0)[:, None, None, None], axis=3)[..., 0]
            vk = np.where((f2 == 0)[:, None, None], acc, pick)             # (p, s, k)
            # phit
            w3 = wb[2][None, :] / (x3[:, None] - m3[None, :])
            scaled = vk * w3[:, None, :]
            acc = scaled[..., 0]
            for ik in range(1, q3):
                acc = acc + scaled[..., ik]
            pick = np.take_along_axis(vk, np.maximum(f3 - 1, 0)[:, None, None], axis=2)[..., 0]
            out = np.where((f3 == 0)[:, None], acc, pick)                  # (p, s)
            v[:, sl] = (out * fac[sl, None]).T
    return v


def project_cubed_sphere(intrp, v, uvwi):
    """``project_cubed_sphere!`` in place on ``v (nstate, Npl)``; ``uvwi`` 1-based columns."""
    deg2rad = np.pi / 180.0
    lat = intrp.lat_grd[intrp.lati - 1] * deg2rad
    lon = intrp.long_grd[intrp.longi - 1] * deg2rad
    u, w_, z = (v[c - 1].copy() for c in uvwi)
    vrad = u * np.cos(lat) * np.cos(lon) + w_ * np.cos(lat) * np.sin(lon) + z * np.sin(lat)
    vlat = -u * np.sin(lat) * np.cos(lon) - w_ * np.sin(lat) * np.sin(lon) + z * np.cos(lat)
    vlon = -u * np.sin(lon) + w_ * np.cos(lon)
    v[uvwi[0] - 1], v[uvwi[1] - 1], v[uvwi[2] - 1] = vlon, vlat, vrad
    return v


def accumulate_interpolated_data(intrps, ivs, fiv):
    """``accumulate_helper_kernel!`` over the ranks in order: ``fiv[s, i3, i2, i1] = iv[s, p]``."""
    for intrp, iv in zip(intrps, ivs):
        fiv[:, intrp.i3 - 1, intrp.i2 - 1, intrp.i1 - 1] = iv
    return fiv

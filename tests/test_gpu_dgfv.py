"""DGFVModel on the device (cmdg_create_dgfv; csrc/fv.h k_fv_tendency / k_fv_gradients) against the
NumPy restatement of the reference's serial kernels (tests/dgfv_restatement.py)."""
import ctypes as C

import numpy as np
import pytest

from cmdg_loader import cm
import dgfv_restatement as R
from helpers import rel_linf
from test_dgfv_host import (fvm_advection_diffusion_setup, fvm_advection_setup, gold_advdiff, gold_advection,
                            gold_periodic, l2_error, RTOL)

pytestmark = pytest.mark.gpu
M = cm.mesh
BL = cm.balancelaws


def _recons(width, linear=True, nolimiter=False):
    F = cm.fvreconstructions
    if not linear or width == 0:
        return F.FVConstant(), R.Recon(False)
    lim = F.NoLimiter() if nolimiter else F.VanLeer()
    return F.FVLinear(width, lim), R.Recon(True, width, R.no_limiter if nolimiter else R.van_leer)


def _setup(N, nvert, periodic, diffusion=True):
    """2 x 2 columns with unequal cell heights, mixed boundary tags, a diagonal flow."""
    z = np.cumsum(np.concatenate([[0.0], 0.1 + 0.05 * np.arange(nvert)]))
    z = -0.25 + 0.5 * z / z[-1]
    x = np.linspace(-0.5, 0.5, 3)
    topl = M.StackedBrickTopology([x, x, z], boundary=((1, 2), (2, 1), (1, 2)),
                                  periodicity=(False, False, periodic), connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, (N, 0))
    n = np.ones(3) / np.sqrt(3)
    law = BL.AdvectionDiffusion(3, BL.Pseudo1D(n, 1.0, 1 / 100, -1 / 2, 1 / 10),
                                (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)), diffusion=diffusion)
    return law, grid


class _Gaussian2D:
    """``Pseudo1D{u, v, nu}`` of fvm_advection_diffusion_periodic.jl:30-68 in the y-invariant slice:
    the 2-D point (x, y) is (x1, x3), the velocity (u, v) is (u, 0, v), the diffusivity ``nu I`` (zero
    for the reference's first equation).  Fully periodic: the kernels need no data from it."""
    problem_id = 6           # host-only

    def __init__(self, u, v, nu):
        self.u, self.v, self.nu = u, v, nu

    def dparam(self):
        return np.zeros(32)

    def init_velocity_diffusion(self, law, aux, coord):
        aux[:, law.off_u:law.off_u + 3, :] = np.array([self.u, 0.0, self.v])[None, :, None]
        aux[:, law.off_D:law.off_D + 9, :] = (self.nu * np.eye(3)).flatten(order="F")[None, :, None]

    def initial_condition(self, coord, t):
        sig = 3 / 10
        return np.exp(-((coord[0] / sig) ** 2 + (coord[2] / sig) ** 2) / 2) / (sig * np.sqrt(2 * np.pi))


def periodic_dim2_setup(level, equation, N=4):
    """fvm_advection_diffusion_periodic.jl:112-175 (dim = 2) as a 3-D grid of one periodic element
    across y with fields constant in y, after helpers.pseudo1d_dim2_setup: the xi2 derivative and the
    y-face terms vanish to rounding, what remains is the 2-D operator, and mass-weighted norms carry
    the factor sqrt(Ly).  ``equation`` 1 advects, 2 advects and diffuses (nu = 1/100)."""
    Ne = 2 ** (level - 1) * 4
    Ly = 3.0 / Ne
    topl = M.StackedBrickTopology([np.linspace(-1.5, 1.5, Ne + 1), np.array([0.0, Ly]),
                                   np.linspace(-1.5, 1.5, Ne * N + 1)],
                                  periodicity=(True, True, True), connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, (N, 0))
    law = BL.AdvectionDiffusion(3, _Gaussian2D(1.0, 1.0, 0.0 if equation == 1 else 1 / 100), ())
    nsteps = Ne * N ** 2
    return law, grid, 3.0 / nsteps, nsteps, np.sqrt(Ly)


CASES = [  # (N_h, nvertelem, width, periodic)
    (4, 2, 1, False), (1, 2, 3, False), (4, 3, 1, False), (4, 4, 3, False), (1, 5, 2, False),
    (4, 5, 0, False), (4, 2, 1, True), (1, 3, 2, True), (4, 3, 0, True),
]


@pytest.mark.parametrize("N,nvert,width,periodic", CASES)
@pytest.mark.parametrize("direction", [0, 1, 2])
def test_one_evaluation(torch, oracle, N, nvert, width, periodic, direction):
    """(alpha, beta) in {(1,0), (1,1), (0.5,2)}: tendency and gradient flux, relative Linf <= 1e-12."""
    law, grid = _setup(N, nvert, periodic)
    recon, rrecon = _recons(width)
    dg = cm.dgmodel.DGFVModel(law, grid, recon, direction=direction)
    ref = R.DGFVRestatement(law, grid, rrecon, nf_first=0, direction=direction)
    Q = dg.init_ode_state(0.0)
    Qh = Q.cpu().numpy().copy()
    rng = np.random.default_rng(7)
    T0 = rng.standard_normal(Qh.shape)
    for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (0.5, 2.0)):
        T = torch.from_numpy(T0.copy()).to(Q.device)
        Th = T0.copy()
        dg(T, Q, 0.3, alpha, beta)
        ref(Th, Qh, 0.3, alpha, beta)
        err = rel_linf(T.cpu().numpy()[:grid.nreal], Th[:grid.nreal])
        gerr = rel_linf(dg.state_gradient_flux.cpu().numpy()[:grid.nreal], ref.state_gradient_flux[:grid.nreal])
        print("N=%d nv=%d W=%d per=%d dir=%d (%.1f, %.1f): tendency %.2e gradient flux %.2e"
              % (N, nvert, width, periodic, direction, alpha, beta, err, gerr))
        assert err <= 1e-12 and gerr <= 1e-12
    dg.close()


@pytest.mark.parametrize("diffusion,nolimiter", [(False, False), (True, True)])
def test_advection_only_and_nolimiter(torch, oracle, diffusion, nolimiter):
    law, grid = _setup(4, 4, False, diffusion=diffusion)
    recon, rrecon = _recons(1, nolimiter=nolimiter)
    dg = cm.dgmodel.DGFVModel(law, grid, recon, numerical_flux_first_order=1 if nolimiter else 0)
    ref = R.DGFVRestatement(law, grid, rrecon, nf_first=1 if nolimiter else 0)
    Q = dg.init_ode_state(0.0)
    Qh = Q.cpu().numpy().copy()
    T = torch.zeros_like(Q)
    Th = np.zeros_like(Qh)
    dg(T, Q, 0.1)
    ref(Th, Qh, 0.1)
    assert rel_linf(T.cpu().numpy(), Th) <= 1e-12
    dg.close()


WIDTH = {"FVConstant": 0, "FVLinear": 1, "FVLinear3": 3}
_FINAL = {}


def _restatement_final(key, law, grid, rrecon, dt, nsteps, direction=0):
    """Final state of the restatement's run, computed once per case."""
    if key not in _FINAL:
        ref = R.DGFVRestatement(law, grid, rrecon, nf_first=0, direction=direction)
        Qh = law.init_state_prognostic(grid, ref.state_auxiliary, 0.0)
        R.lsrk54_steps(ref, Qh, dt, nsteps)
        _FINAL[key] = Qh
    return _FINAL[key]


def _device_run(law, grid, recon, dt, nsteps, direction=0):
    dg = cm.dgmodel.DGFVModel(law, grid, recon, direction=direction)
    Q = dg.init_ode_state(0.0)
    cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=dt).dostep(Q, nsteps=nsteps)
    dg.synchronize()
    out = Q.cpu().numpy()
    aux = dg.state_auxiliary.cpu().numpy()
    dg.close()
    return out, aux


@pytest.mark.parametrize("recon_name", ["FVConstant", "FVLinear", "FVLinear3"])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_golden_level1(torch, oracle, recon_name, field):
    """fvm_advection_diffusion.jl, dim 3, level 1 (4 x 4 x 4, 256 steps): the stored error within the
    reference's rtol, and the final state against the restatement's at 1e-11."""
    law, grid, dt = fvm_advection_diffusion_setup(1, field)
    recon, rrecon = _recons(WIDTH[recon_name])
    Q, aux = _device_run(law, grid, recon, dt, 256)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, aux, 1.0))
    want = gold_advdiff(1, "FVConstant" if recon_name == "FVConstant" else "FVLinear")[field]
    Qh = _restatement_final(("advdiff", recon_name, field), law, grid, rrecon, dt, 256)
    serr = rel_linf(Q[:grid.nreal], Qh[:grid.nreal])
    print("%s field %d: %.16e (reference %.16e), state vs restatement %.2e" % (recon_name, field, err, want, serr))
    assert abs(err - want) <= RTOL * abs(want)
    assert serr <= 1e-11


@pytest.mark.parametrize("direction,field", [(1, 0), (2, 1)])
def test_golden_level1_single_direction(torch, oracle, direction, field):
    """The Horizontal- and Vertical-direction runs against fields 1 and 2 (:452-466)."""
    law, grid, dt = fvm_advection_diffusion_setup(1, field)
    recon, rrecon = _recons(1)
    Q, aux = _device_run(law, grid, recon, dt, 256, direction)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, aux, 1.0))
    want = gold_advdiff(1, "FVLinear")[field]
    Qh = _restatement_final(("advdiff-dir", direction), law, grid, rrecon, dt, 256, direction)
    print("direction %d: %.16e (reference %.16e)" % (direction, err, want))
    assert abs(err - want) <= RTOL * abs(want)
    assert rel_linf(Q[:grid.nreal], Qh[:grid.nreal]) <= 1e-11


@pytest.mark.parametrize("recon_name", ["FVConstant", "FVLinear", "FVLinear3"])
@pytest.mark.parametrize("field", [0, 1, 2])
def test_golden_level2(torch, oracle, recon_name, field):
    """Level 2 (8 x 8 x 8, 512 steps): every field and reconstruction within rtol."""
    law, grid, dt = fvm_advection_diffusion_setup(2, field)
    Q, aux = _device_run(law, grid, _recons(WIDTH[recon_name])[0], dt, 512)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, aux, 1.0))
    want = gold_advdiff(2, "FVConstant" if recon_name == "FVConstant" else "FVLinear")[field]
    print("level 2 %s field %d: %.16e (reference %.16e)" % (recon_name, field, err, want))
    assert abs(err - want) <= RTOL * abs(want)


@pytest.mark.parametrize("recon_name", ["FVConstant", "FVLinear"])
def test_golden_fvm_advection(torch, oracle, recon_name):
    """fvm_advection.jl, dim 3, level 1 (4 x 4 x 16 cells, 64 steps): the stored error within rtol and
    the final state against the restatement's at 1e-11."""
    law, grid, dt, nsteps = fvm_advection_setup(1)
    recon, rrecon = _recons(WIDTH[recon_name])
    Q, aux = _device_run(law, grid, recon, dt, nsteps)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, aux, 0.25))
    want = gold_advection(1, recon_name)
    Qh = _restatement_final(("advection", recon_name), law, grid, rrecon, dt, nsteps)
    print("fvm_advection %s: %.16e (reference %.16e)" % (recon_name, err, want))
    assert abs(err - want) <= RTOL * abs(want)
    assert rel_linf(Q, Qh) <= 1e-11


@pytest.mark.parametrize("recon_name", ["FVConstant", "FVLinear", "FVLinear3"])
@pytest.mark.parametrize("equation", [1, 2])
@pytest.mark.parametrize("level", [1, 2])
def test_golden_periodic_dim2(torch, oracle, level, equation, recon_name):
    """fvm_advection_diffusion_periodic.jl (dim 2, fully periodic, one period) through the
    y-invariant slice: both equations within rtol.  Pins the periodic stack to reference-held numbers."""
    law, grid, dt, nsteps, sq = periodic_dim2_setup(level, equation)
    Q, aux = _device_run(law, grid, _recons(WIDTH[recon_name])[0], dt, nsteps)
    err = l2_error(grid, Q, law.init_state_prognostic(grid, aux, 0.0)) / sq
    want = gold_periodic(level, "FVConstant" if recon_name == "FVConstant" else "FVLinear", equation)
    print("periodic level %d eq %d %s: %.16e (reference %.16e)" % (level, equation, recon_name, err, want))
    assert abs(err - want) <= RTOL * abs(want)


def test_two_ranks(torch, oracle):
    """Two ranks of one process through connect_local: ten steps equal the single-rank state."""
    from oracle import oracle as O
    law, grid, dt = fvm_advection_diffusion_setup(1, 2)
    one = cm.dgmodel.DGFVModel(law, grid, cm.fvreconstructions.FVLinear())
    Q1 = one.init_ode_state(0.0)
    cm.odesolvers.LSRK54CarpenterKennedy(one, Q1, dt=dt).dostep(Q1, nsteps=10)
    one.synchronize()
    parts = [fvm_advection_diffusion_setup(1, 2, rank=r, size=2) for r in range(2)]
    dgs = [cm.dgmodel.DGFVModel(p[0], p[1], cm.fvreconstructions.FVLinear()) for p in parts]
    cm.dgmodel.connect_local(dgs)
    Qs = [d.init_ode_state(0.0) for d in dgs]
    dQs = [torch.zeros_like(q) for q in Qs]
    cm.dgmodel.group_lsrk_run(dgs, Qs, dQs, 0.0, dt, 10, O.RKA, O.RKB, O.RKC)
    for d in dgs:
        d.synchronize()
    full = Q1.cpu().numpy()
    by_global = {int(gid): full[i] for i, gid in enumerate(grid.topology.globalelems[:grid.nreal])}
    for p, q in zip(parts, Qs):
        g = p[1]
        want = np.stack([by_global[int(gid)] for gid in g.topology.globalelems[:g.nreal]])
        assert rel_linf(q.cpu().numpy()[:g.nreal], want) <= 1e-12
    for d in dgs + [one]:
        d.close()


def test_periodic_conservation(torch, oracle):
    """Fully periodic: the mass-weighted sum changes by at most 10 eps |sum| over 20 steps."""
    x = np.linspace(-1.0, 1.0, 5)
    topl = M.StackedBrickTopology([x, x, np.linspace(-0.25, 0.25, 5)], periodicity=(True,) * 3, connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, (4, 0))
    law = BL.AdvectionDiffusion(3, BL.Pseudo1D(np.ones(3) / np.sqrt(3), 1.0, 1 / 100, -1 / 2, 1 / 10), ())
    dg = cm.dgmodel.DGFVModel(law, grid, cm.fvreconstructions.FVLinear())
    Q = dg.init_ode_state(0.0)
    s0 = cm.weightedsum(dg, Q)
    cm.odesolvers.LSRK54CarpenterKennedy(dg, Q, dt=1.0 / 256).dostep(Q, nsteps=20)
    dg.synchronize()
    s1 = cm.weightedsum(dg, Q)
    print("weightedsum: %.17e -> %.17e" % (s0, s1))
    assert abs(s1 - s0) <= 10 * np.finfo(float).eps * abs(s0)
    dg.close()


def test_refusals(torch):
    """Every refusal of cmdg_create_dgfv and of the calls an FV handle does not serve: status and a
    message that names the cause."""
    L = cm._lib
    law, grid = _setup(4, 3, False)
    F = cm.fvreconstructions
    INVALID, UNSUPPORTED = -1, -5
    # N[2] == 0 through the wrong constructor
    with pytest.raises(L.CmdgError, match=r"\(-1\).*N\[2\] == 0.*cmdg_create_dgfv"):
        cm.dgmodel.DGModel(law, grid)
    # a law with hyperdiffusive states
    hyp = BL.AdvectionDiffusion(3, BL.ConstantHyperDiffusion(3, 0, np.eye(3) / 100), (), advection=False,
                                diffusion=False, hyperdiffusion=True)
    with pytest.raises(L.CmdgError, match=r"\(-5\).*hyperdiffusive"):
        cm.dgmodel.DGFVModel(hyp, grid, F.FVConstant())
    # a horizontal order that is not compiled in
    with pytest.raises(L.CmdgError, match=r"\(-5\).*orders compiled in are 1 and 4"):
        cm.dgmodel.DGFVModel(law, _setup(2, 3, False)[1], F.FVConstant())

    dg = cm.dgmodel.DGFVModel(law, grid, F.FVLinear())
    lib = dg.L

    def create(desc_edit=None, **fv_edit):
        d = type(dg._desc).from_buffer_copy(dg._desc)
        fv = type(dg._fv_desc).from_buffer_copy(dg._fv_desc)
        if desc_edit:
            desc_edit(d)
        for k, v in fv_edit.items():
            setattr(fv, k, v)
        h = C.c_void_p()
        rc = lib.cmdg_create_dgfv(C.byref(d), C.byref(fv), C.byref(h))
        assert not h.value
        return rc, lib.cmdg_last_error(None).decode()

    def expect(rc_msg, status, text):
        assert rc_msg[0] == status and text in rc_msg[1], rc_msg

    def set_n2(d):
        d.N[2] = 4

    def unstack(d):
        d.stacked = 0

    expect(create(set_n2), INVALID, "N[2] must be 0")
    expect(create(unstack), INVALID, "stacked grid")
    expect(create(nvertelem=1), INVALID, "nvertelem < 2")
    expect(create(width=4), INVALID, "width outside 0..3")
    expect(create(width=-1), INVALID, "width outside 0..3")
    expect(create(width=0), INVALID, "linear reconstruction needs width >= 1")
    expect(create(reconstruction=L.FV_CONSTANT, width=1), INVALID, "constant reconstruction has width 0")
    expect(create(reconstruction=7), INVALID, "unknown reconstruction")
    expect(create(limiter=5), INVALID, "unknown slope limiter")
    expect(create(nvertelem=5), INVALID, "not multiples of nvertelem")
    # element lists that are not whole stacks, bottom element first
    lists = torch.cat([dg._interior, dg._exterior]).flip(0).contiguous()

    def reorder(d):
        d.interiorelems, d.ninterior = lists.data_ptr(), lists.numel()
        d.exteriorelems, d.nexterior = 0, 0
    torch.cuda.synchronize()
    expect(create(reorder), INVALID, "whole stacks")

    Q = dg.init_ode_state(0.0)
    out = C.c_double()
    assert lib.cmdg_courant(dg.handle, 1, Q.data_ptr(), 0.1, 0.0, 0, C.byref(out)) == UNSUPPORTED
    assert b"Courant" in lib.cmdg_last_error(dg.handle)
    assert lib.cmdg_min_node_distance(dg.handle, 2, C.byref(out)) == UNSUPPORTED
    assert b"2 JcV" in lib.cmdg_last_error(dg.handle)
    fd, fh = cm.mesh.filters.CmdgFilterDesc(), C.c_void_p()
    assert lib.cmdg_filter_create(dg.handle, C.byref(fd), C.byref(fh)) == UNSUPPORTED
    assert b"element filters" in lib.cmdg_last_error(dg.handle)
    lu = C.c_void_p()
    assert lib.cmdg_columnlu_create(dg.handle, 3, 1.0, C.byref(lu)) == UNSUPPORTED
    assert b"column LU is not available on a DGFVModel handle" in lib.cmdg_last_error(dg.handle)
    dg.close()
